"""AViT baseline on the HIP kernels  (reference models/avit.py, configs/avit.yaml: the attention baseline of the comparison table, from MPP).

Same constructor arguments, attributes, `state_dict` keys / shapes and forward contract (`b t c h w -> b min(t, 4) c h w`, whatever
`out_steps` says, avit.py:450) as the reference's models.AViT.  The model is channels-last inside, its rows ordered ((t b), h, w), the
residual stream fp32, and every arithmetic step is a C-ABI call of libtante_hip:
  field stats   tante_field_stats on the batch as it arrives: mean and unbiased std + 1e-7 over (t, h, w) per (b, c), and the normalised
                channels-last image the stem reads; tante_field_affine undoes it on the head's output, writing b t c h w
  stem          the pixel-wise SubsampledLinear (labels = range(c), scale sqrt(n_states / c)) and the 4 x 4 / 4 convolution without bias
                folded in float64 at pack time into ONE convolution c -> embed_dim / 4 with a folded bias (the embed_dim / 4-channel
                full-resolution image never exists); every stride convolution is tante_im2col + tante_gemm, every RMS norm (+ GELU) is
                tante_instnorm
  time block    tante_instnorm (instance form) -> tante_gemm -> tante_time_attention (q / k LayerNorm, the bucketed relative-position
                bias, softmax) -> tante_instnorm -> tante_gemm with gamma folded into output_head and the skip as the residual operand
  space block   tante_instnorm (rms form) -> tante_gemm -> tante_axial_attention (q / k LayerNorm, attention along W and along H, the
                average) -> tante_instnorm -> tante_gemm with gamma_att folded and the skip as residual -> fc1 + erf GELU -> fc2 (K
                chunked past 512) -> tante_instnorm with the epilogue x + gamma_mlp * norm(.) in place
  head          the two 2 x 2 / 2 transposed convolutions as scatter GEMMs (tap GEMM + tante_col2im_nhwc past 512 input channels), RMS norm
                + GELU between them, the 4 x 4 / 4 one with out_kernel[:, labels] / out_bias[labels] writing channels first.  Only the
                steps that are returned are decoded: the head is per image.
torch allocates and reshapes.

Held for the state dict and NEVER applied, as in the reference: the spatial block's `rel_pos_bias` table (F.scaled_dot_product_attention
gets no mask there, avit.py:265, 270) and every RMS norm's `bias` (avit.py:132).  `in_T` is unused, as in the reference.

In bf16 mode bf16 is the GEMM operand type only, and only of the MLP's two GEMMs (BF16_SITES): the residual stream, every norm and
statistic, q / k normalisation, logits and softmax stay fp32, and so do the stem's, the head's and the attention blocks' projections.  The
RMS norms do not subtract the mean, so their outputs carry a per-channel offset that the next norm's division by the token-plane std
amplifies; operands rounded to bf16 at those GEMMs put 1.2e-2 .. 5e-2 into the fixture-sized models' outputs (DESIGN 4.7 has the per-site
figures), the MLP's alone 4e-3 .. 8e-3.

Inference only (eval mode under no_grad).  Training, `override_block`, T > 16, token axes > 64 and a 1 x 1 token grid raise; there is no
CPU fallback."""
from __future__ import annotations

import math
from functools import partial
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from . import stages as S
from .attn_backbone import _PackCache, resolve_compute
from .model_shell import ComputeSwitch, gpu_only, inference_only, site

MAX_TOKENS = 4096   # tokens per image tante_instnorm serves
MAX_AXIS = 64       # tokens per axis tante_axial_attention serves
MAX_T = 16          # time steps tante_time_attention serves
HEAD_DIMS = (16, 32, 64)
OUT_STEPS = 4       # x[-4:]  (avit.py:450)
BF16_SITES = ("mlp",)   # the GEMM groups that take bf16 operands in bf16 mode; "stem", "attn" and "head" miss the 1e-2 bar


# ---- host side of the kernels: the predicates' mirrors, the wrappers, the folds, the bias table -----------------------------------------
def instnorm_supported_py(n_img: int, HW: int, C_: int) -> bool:
    """Python mirror of tante_instnorm_supported."""
    return 2 <= HW <= MAX_TOKENS and 1 <= C_ <= (1 << 24) and 0 <= n_img and n_img * ((C_ + 63) // 64) <= 2 ** 31 - 1


def axial_attention_supported_py(n_img: int, heads: int, H: int, W: int, hd: int) -> bool:
    """Python mirror of tante_axial_attention_supported."""
    return (1 <= H <= MAX_AXIS and 1 <= W <= MAX_AXIS and hd in HEAD_DIMS and 1 <= heads <= 65535 and 0 <= n_img
            and n_img * max(H, W) <= 2 ** 31 - 1)


def time_attention_supported_py(nseq: int, T: int, heads: int, hd: int) -> bool:
    """Python mirror of tante_time_attention_supported."""
    return 1 <= T <= MAX_T and hd in HEAD_DIMS and 1 <= heads <= 65535 and 0 <= nseq <= 2 ** 31 - 1


def field_stats_supported_py(B: int, T: int, C_: int, HW: int) -> bool:
    """Python mirror of tante_field_stats_supported."""
    return (T >= 1 and HW >= 1 and C_ >= 1 and 2 <= T * HW <= 2 ** 30 and 0 <= B and B * C_ <= 2 ** 31 - 1 and B * C_ * T * HW <= 2 ** 38)


def field_affine_supported_py(B: int, Tk: int, C_: int, HW: int) -> bool:
    """Python mirror of tante_field_affine_supported."""
    return Tk >= 1 and HW >= 1 and C_ >= 1 and 0 <= B and B * C_ <= 2 ** 31 - 1 and B * C_ * Tk * HW <= 2 ** 38 and Tk * HW <= 2 ** 38


def instnorm(x: torch.Tensor, form: int, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
             out_dtype: torch.dtype = torch.float32, act: int = L.ACT_NONE, residual: Optional[torch.Tensor] = None,
             gamma: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tante_instnorm on channels-last fp32 rows x (n_img, HW, C): form L.INSTNORM_INSTANCE / L.INSTNORM_RMS, then act, then (with
    residual and gamma) residual + gamma[c] * value; `out` may be `residual`."""
    K._dev(x, weight, bias, residual, gamma, out)
    if x.dtype != torch.float32 or x.dim() != 3:
        raise RuntimeError("the instance norms take fp32 channels-last rows (n_img, HW, C)")
    n, HW, C_ = x.shape
    lib = L.lib()
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    work, nbytes = K.workspace(lib.tante_instnorm_workspace_bytes(n, HW, C_), x.device)           # (-1: the call below refuses by name)
    L.check(lib.tante_instnorm(K._p(x), n, HW, C_, form, float(eps), K._p(weight), K._p(bias), act, K._p(residual), K._p(gamma), K._p(out),
                               K._DT[out.dtype], K._p(work), nbytes, K._stream()), "tante_instnorm")
    return out


def axial_attention(qkv: torch.Tensor, n_img: int, heads: int, H: int, W: int, qnorm: nn.LayerNorm, knorm: nn.LayerNorm) -> torch.Tensor:
    """tante_axial_attention on the rows qkv (n_img H W, 3 E) fp32, channel order (head, [q | k | v], hd) -> (n_img H W, E) fp32."""
    K._dev(qkv)
    E = qkv.shape[1] // 3
    hd = E // max(heads, 1)
    if qkv.dtype != torch.float32 or qkv.dim() != 2 or qkv.shape[0] != n_img * H * W or heads * hd * 3 != qkv.shape[1]:
        raise RuntimeError(f"axial attention takes fp32 rows (n_img H W, 3 heads hd), got {tuple(qkv.shape)} for {n_img} x {H} x {W}, {heads} heads")
    out = torch.empty(qkv.shape[0], E, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().tante_axial_attention(K._p(qkv), n_img, heads, H, W, hd, K._p(qnorm.weight.detach()), K._p(qnorm.bias.detach()),
                                          K._p(knorm.weight.detach()), K._p(knorm.bias.detach()), float(qnorm.eps), K._p(out), K._stream()),
            "tante_axial_attention")
    return out


def time_attention(qkv: torch.Tensor, nseq: int, T: int, heads: int, qnorm: nn.LayerNorm, knorm: nn.LayerNorm, bias: torch.Tensor) -> torch.Tensor:
    """tante_time_attention on the rows qkv (T nseq, 3 E) fp32 ordered (t, sequence); bias (heads, T, T) fp32 -> (T nseq, E) fp32."""
    K._dev(qkv, bias)
    E = qkv.shape[1] // 3
    hd = E // max(heads, 1)
    lib = L.lib()
    if not lib.tante_time_attention_supported(nseq, T, heads, hd):
        # the call itself refuses with the reason; made here without touching the device
        L.check(lib.tante_time_attention(None, nseq, T, heads, hd, None, None, None, None, 0.0, None, None, None), "tante_time_attention")
    if qkv.dtype != torch.float32 or qkv.dim() != 2 or qkv.shape[0] != nseq * T or heads * hd * 3 != qkv.shape[1]:
        raise RuntimeError(f"time attention takes fp32 rows (T nseq, 3 heads hd), got {tuple(qkv.shape)} for T {T}, {nseq} sequences, {heads} heads")
    if bias.dtype != torch.float32 or tuple(bias.shape) != (heads, T, T):
        raise RuntimeError(f"the time bias must be fp32 ({heads}, {T}, {T}), got {tuple(bias.shape)}")
    out = torch.empty(qkv.shape[0], E, dtype=torch.float32, device=qkv.device)
    L.check(lib.tante_time_attention(K._p(qkv), nseq, T, heads, hd, K._p(qnorm.weight.detach()), K._p(qnorm.bias.detach()),
                                         K._p(knorm.weight.detach()), K._p(knorm.bias.detach()), float(qnorm.eps), K._p(bias), K._p(out),
                                         K._stream()), "tante_time_attention")
    return out


def field_stats(x: torch.Tensor, normalise: bool = True, eps: float = 1e-7):
    """tante_field_stats on x (B, T, C, H, W) fp32 -> stats (B, C, 2) = [mean, std + eps], and the normalised channels-last images
    ((t b), H, W, C) (None without `normalise`)."""
    K._dev(x)
    if x.dtype != torch.float32 or x.dim() != 5:
        raise RuntimeError("the field statistics take an fp32 batch (B, T, C, H, W)")
    B, T, C_, H, W = x.shape
    lib = L.lib()
    stats = torch.empty(B, C_, 2, dtype=torch.float32, device=x.device)
    xn = torch.empty(T * B, H, W, C_, dtype=torch.float32, device=x.device) if normalise else None
    work, nbytes = K.workspace(lib.tante_field_stats_workspace_bytes(B, T, C_, H * W), x.device)
    L.check(lib.tante_field_stats(K._p(x), B, T, C_, H * W, float(eps), K._p(stats), K._p(xn), K._p(work), nbytes, K._stream()), "tante_field_stats")
    return stats, xn


def field_affine(y: torch.Tensor, stats: torch.Tensor, B: int) -> torch.Tensor:
    """tante_field_affine: y ((t b), C, H, W) fp32 -> (B, Tk, C, H, W) = y * std + mean."""
    K._dev(y, stats)
    n, C_, H, W = y.shape
    Tk = n // max(B, 1)
    if y.dtype != torch.float32 or Tk * B != n or tuple(stats.shape) != (B, C_, 2):
        raise RuntimeError(f"the field affine takes fp32 images ((t b), C, H, W) and stats (B, C, 2), got {tuple(y.shape)} / {tuple(stats.shape)}")
    out = torch.empty(B, Tk, C_, H, W, dtype=torch.float32, device=y.device)
    L.check(L.lib().tante_field_affine(K._p(y), K._p(stats), B, Tk, C_, H * W, K._p(out), K._stream()), "tante_field_affine")
    return out


def time_bucket_table(T: int, num_buckets: int = 32, max_distance: int = 32) -> torch.Tensor:
    """The (T, T) table of relative-position buckets the time block's bias reads, entry [q, k] for the offset k - q.  Each direction has
    num_buckets / 2 buckets (keys ahead of the query take the upper half); in a direction the distances below half of those have a bucket
    each, and the longer ones share logarithmically spaced buckets up to max_distance, the last one taking everything beyond.  This is
    what the reference's model computes (avit.py:57-108) with the values that reach it: bidirectional, and max_distance 32 -- the bucket
    routine's own default, which the module's attribute of 128 never overrides.  The logarithm is evaluated on a float32 tensor and
    truncated, as there, so a distance on a bucket edge falls where the reference's does."""
    per_side = num_buckets // 2
    exact = per_side // 2
    pos = torch.arange(T, dtype=torch.long)
    offset = pos[None, :] - pos[:, None]
    dist = offset.abs()
    steps = torch.log(dist.clamp(min=exact).to(torch.float32) / exact) / math.log(max_distance / exact) * (per_side - exact)
    shared = (exact + steps.to(torch.long)).clamp(max=per_side - 1)
    return torch.where(dist < exact, dist, shared) + per_side * (offset > 0).to(torch.long)


def time_bias_table(embedding: torch.Tensor, T: int, num_buckets: int = 32) -> torch.Tensor:
    """The additive bias of the time block, bias[head, q, k] = embedding[bucket[q, k], head] (avit.py:82-108) -> (heads, T, T) fp32 on
    the embedding's device."""
    bucket = time_bucket_table(T, num_buckets).to(embedding.device)
    return embedding.detach().float()[bucket].permute(2, 0, 1).contiguous()


def fold_layer_scale(weight: torch.Tensor, bias: torch.Tensor, gamma: Optional[torch.Tensor]):
    """gamma[:, None] * W and gamma * b of a 1 x 1 convolution (avit.py:276, 330), in float64, rounded to fp32 once."""
    w64 = weight.detach().double().reshape(weight.shape[0], -1)
    b64 = bias.detach().double()
    if gamma is not None:
        g = gamma.detach().double()
        w64, b64 = w64 * g[:, None], b64 * g
    return w64.float().contiguous(), b64.float().contiguous()


def fold_stem(bag_weight: torch.Tensor, bag_bias: torch.Tensor, conv_weight: torch.Tensor, c: int):
    """scale * F.linear(x, W[:, :c], b) followed by the 4 x 4 / 4 convolution without bias (avit.py:159-165, 179) as ONE convolution:
    weight (Cout, 4, 4, c) in the channels-last im2col column order and bias (Cout,), in float64, rounded to fp32 once."""
    scale = (bag_weight.shape[1] / c) ** 0.5
    wc = conv_weight.detach().double()                                        # (Cout, E4, 4, 4)
    wb = bag_weight.detach().double()[:, :c]                                  # (E4, c)
    w = scale * torch.einsum("oekl,ec->oklc", wc, wb)
    b = scale * torch.einsum("oekl,e->o", wc, bag_bias.detach().double())
    return w.reshape(w.shape[0], -1).float().contiguous(), b.float().contiguous()


# ---- the reference's modules -------------------------------------------------------------------------------------------------------
WHY_INFERENCE_ONLY = ("the backward of the instance norms and of the axial / time attention are kernels of their own that are not "
                      "built")


def _token_grid(Hp: int, Wp: int):
    if Hp * Wp < 2:
        raise ValueError("a 1 x 1 token grid is out of scope: the reference's InstanceNorm2d refuses one spatial element and the unbiased "
                         "std of one value is NaN")


class DropPath(nn.Module):
    """Stochastic depth: the identity in eval mode, which is the only mode here; carries its rate as timm's does."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        if self.training and self.drop_prob > 0.0:
            raise NotImplementedError("DropPath in train() is out of scope: training is out of scope")
        return x

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


class ContinuousPositionBias1D(nn.Module):
    """avit.py:21-45: a parameter holder; unreachable from AViT's constructor (bias_type stays 'rel') and never evaluated."""

    def __init__(self, n_heads):
        super().__init__()
        self.num_heads = n_heads
        self.cpb_mlp = nn.Sequential(nn.Linear(1, 512, bias=True), nn.ReLU(inplace=True), nn.Linear(512, n_heads, bias=False))

    def forward(self, h, h2, bc=0):
        raise NotImplementedError("the continuous position bias is out of scope: AViT's constructor cannot reach it")


class RelativePositionBias(nn.Module):
    """avit.py:48-111: the T5-style bucketed bias; forward tabulates it on the host with the reference's own arithmetic."""

    def __init__(self, bidirectional=True, num_buckets=32, max_distance=128, n_heads=2):
        super().__init__()
        self.bidirectional = bidirectional
        self.num_buckets = num_buckets
        self.max_distance = max_distance
        self.n_heads = n_heads
        self.relative_attention_bias = nn.Embedding(self.num_buckets, self.n_heads)
        self._cache = _PackCache()

    def table(self, T: int) -> torch.Tensor:
        """(heads, T, T) fp32, built once per (T, weights)."""
        if not self.bidirectional:
            raise NotImplementedError("bidirectional = False is out of scope: the reference's blocks build the bias with its default")
        w = self.relative_attention_bias.weight
        return self._cache.get(T, [w], lambda: time_bias_table(w, T, self.num_buckets))

    def compute_bias(self, qlen, klen, bc=0):
        if qlen != klen or bc != 0:
            raise NotImplementedError("the relative position bias is tabulated for qlen == klen and bc = 0, as AViT uses it")
        return self.table(qlen).unsqueeze(0)                                   # (1, heads, qlen, klen)

    def forward(self, qlen, klen, bc=0):
        return self.compute_bias(qlen, klen, bc)


class MLP(nn.Module):
    """fc2(gelu_erf(fc1(x)))  (avit.py:114-122): a parameter holder, evaluated by AxialAttentionBlock.run."""

    def __init__(self, hidden_dim, exp_factor=4.):
        super().__init__()
        self.fc1 = nn.Linear(hidden_dim, int(hidden_dim * exp_factor))
        self.fc2 = nn.Linear(int(hidden_dim * exp_factor), hidden_dim)
        self.act = nn.GELU()


class RMSInstanceNorm2d(nn.Module):
    """x / (std_unbiased + eps) * weight over the token plane; `bias` is held and never applied  (avit.py:125-139)."""

    def __init__(self, dim, affine=True, eps=1e-8):
        super().__init__()
        self.eps = eps
        self.affine = affine
        if affine:
            self.weight = nn.Parameter(torch.ones(dim))
            self.bias = nn.Parameter(torch.zeros(dim))

    def run(self, x: torch.Tensor, out_dtype: torch.dtype = torch.float32, act: int = L.ACT_NONE, **epilogue) -> torch.Tensor:
        """x (n_img, HW, C) fp32 channels-last."""
        return instnorm(x, L.INSTNORM_RMS, self.weight.detach() if self.affine else None, None, self.eps, out_dtype, act, **epilogue)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, C, H, W) -> (B, C, H, W).  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        B, C_, H, W = x.shape
        y = self.run(x.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(B, H * W, C_).contiguous())
        return y.view(B, H, W, C_).permute(0, 3, 1, 2).to(x.dtype)


class SubsampledLinear(nn.Module):
    """avit.py:141-168: a parameter holder; AViT folds it into the stem's first convolution (fold_stem)."""

    def __init__(self, dim_in, dim_out, subsample_in=True):
        super().__init__()
        self.subsample_in = subsample_in
        self.dim_in = dim_in
        self.dim_out = dim_out
        temp_linear = nn.Linear(dim_in, dim_out)
        self.weight = nn.Parameter(temp_linear.weight.detach().clone())
        self.bias = nn.Parameter(temp_linear.bias.detach().clone())


class hMLP_stem(nn.Module):
    """Conv 4/4 -> RMS norm -> GELU -> Conv 2/2 -> RMS norm -> GELU -> Conv 2/2 -> RMS norm  (avit.py:170-192)."""

    def __init__(self, patch_size=(16, 16), in_chans=3, embed_dim=768):
        super().__init__()
        self.patch_size = patch_size
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.in_proj = torch.nn.Sequential(
            nn.Conv2d(in_chans, embed_dim // 4, kernel_size=4, stride=4, bias=False), RMSInstanceNorm2d(embed_dim // 4, affine=True), nn.GELU(),
            nn.Conv2d(embed_dim // 4, embed_dim // 4, kernel_size=2, stride=2, bias=False), RMSInstanceNorm2d(embed_dim // 4, affine=True), nn.GELU(),
            nn.Conv2d(embed_dim // 4, embed_dim, kernel_size=2, stride=2, bias=False), RMSInstanceNorm2d(embed_dim, affine=True))
        self._cache = _PackCache()

    def _packed(self, compute: int):
        c0, c3, c6 = self.in_proj[0], self.in_proj[3], self.in_proj[6]
        return self._cache.get(compute, [c0.weight, c3.weight, c6.weight], lambda: tuple(
            S.pack_linear_chunks(S.conv_rows(c.weight), None, compute) for c in (c0, c3, c6)))

    def run(self, x: torch.Tensor, compute: int, first=None) -> torch.Tensor:
        """x (n, H, W, Cin) fp32 channels-last -> rows (n H/16 W/16, embed_dim) fp32; `first`: packed chunks that replace in_proj[0]."""
        n, H, W, cin = x.shape
        if H % 16 or W % 16:
            raise ValueError(f"H and W must be multiples of 16 (the stem is 4 x 2 x 2), got {H} x {W}")
        _token_grid(H // 16, W // 16)
        compute = site(compute, "stem", BF16_SITES)
        own = self._packed(compute)
        adt = K.act_torch_dtype(compute)
        E4 = self.embed_dim // 4
        y = S.linear_chunks(K.im2col(x, False, n, cin, H, W, 4, 4, 4, 4, 0, 0, 1, adt), own[0] if first is None else first, torch.float32)
        h, w = H // 4, W // 4
        a = self.in_proj[1].run(y.view(n, h * w, E4), adt, L.ACT_GELU_ERF)
        y = S.linear_chunks(K.im2col(a, False, n, E4, h, w, 2, 2, 2, 2, 0, 0, 1, adt), own[1], torch.float32)
        h, w = h // 2, w // 2
        a = self.in_proj[4].run(y.view(n, h * w, E4), adt, L.ACT_GELU_ERF)
        y = S.linear_chunks(K.im2col(a, False, n, E4, h, w, 2, 2, 2, 2, 0, 0, 1, adt), own[2], torch.float32)
        h, w = h // 2, w // 2
        return self.in_proj[7].run(y.view(n, h * w, self.embed_dim)).view(n * h * w, self.embed_dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, in_chans, H, W) -> (n, embed_dim, H/16, W/16).  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        n, _, H, W = x.shape
        y = self.run(x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous(), resolve_compute(None))
        return y.view(n, H // 16, W // 16, self.embed_dim).permute(0, 3, 1, 2).to(x.dtype)


class hMLP_output(nn.Module):
    """ConvT 2/2 -> RMS norm -> GELU -> ConvT 2/2 -> RMS norm -> GELU -> ConvT 4/4 with out_kernel[:, labels]  (avit.py:194-221)."""

    def __init__(self, patch_size=(16, 16), out_chans=3, embed_dim=768):
        super().__init__()
        self.patch_size = patch_size
        self.out_chans = out_chans
        self.embed_dim = embed_dim
        self.out_proj = torch.nn.Sequential(
            nn.ConvTranspose2d(embed_dim, embed_dim // 4, kernel_size=2, stride=2, bias=False), RMSInstanceNorm2d(embed_dim // 4, affine=True), nn.GELU(),
            nn.ConvTranspose2d(embed_dim // 4, embed_dim // 4, kernel_size=2, stride=2, bias=False), RMSInstanceNorm2d(embed_dim // 4, affine=True),
            nn.GELU())
        out_head = nn.ConvTranspose2d(embed_dim // 4, out_chans, kernel_size=4, stride=4)
        self.out_kernel = nn.Parameter(out_head.weight.detach().clone())
        self.out_bias = nn.Parameter(out_head.bias.detach().clone())
        self._cache = _PackCache()

    def _packed(self, compute: int, labels):
        labels = list(labels)
        d0, d3 = self.out_proj[0], self.out_proj[3]
        E4 = self.embed_dim // 4
        if E4 > S.KMAX:
            raise NotImplementedError(f"embed_dim = {self.embed_dim} is out of scope: the head's pixel-row GEMMs take embed_dim / 4 <= {S.KMAX} channels")

        def build():
            wk = self.out_kernel.detach()[:, labels].contiguous()
            bk = self.out_bias.detach()[labels].contiguous()
            return (S.pack_deconv_nhwc(d0.weight, None, 2, compute), S.pack_deconv_nhwc(d3.weight, None, 2, compute),
                    K.pack_weight(wk, bk, compute, L.W_DECONV_NCHW, N=len(labels) * 16, K=E4, P=4, C_other=len(labels)))
        return self._cache.get((compute, tuple(labels)), [d0.weight, d3.weight, self.out_kernel, self.out_bias], build)

    def run(self, rows: torch.Tensor, n: int, Hp: int, Wp: int, labels, compute: int) -> torch.Tensor:
        """rows (n Hp Wp, embed_dim) fp32 -> (n, len(labels), 16 Hp, 16 Wp) fp32 channels first."""
        compute = site(compute, "head", BF16_SITES)
        d0, d3, last = self._packed(compute, labels)
        adt = K.act_torch_dtype(compute)
        E4 = self.embed_dim // 4
        img = S.deconv_nhwc(rows, d0, None, n, Hp, Wp, 2, E4)
        a = self.out_proj[1].run(img.view(n, 4 * Hp * Wp, E4), adt, L.ACT_GELU_ERF)
        img = S.deconv_nhwc(a.view(n * 4 * Hp * Wp, E4), d3, None, n, 2 * Hp, 2 * Wp, 2, E4)
        a = self.out_proj[4].run(img.view(n, 16 * Hp * Wp, E4), adt, L.ACT_GELU_ERF)
        c = len(list(labels))
        out = torch.empty(n, c, 16 * Hp, 16 * Wp, dtype=torch.float32, device=rows.device)
        return K.deconv(a.view(n * 16 * Hp * Wp, E4), last, out, n_img=n, Hi=4 * Hp, Wi=4 * Wp, P=4, Cout=c, nchw_out=True, act=L.ACT_NONE)

    def forward(self, x: torch.Tensor, state_labels) -> torch.Tensor:
        """(n, embed_dim, H', W') -> (n, len(state_labels), 16 H', 16 W').  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        n, E, Hp, Wp = x.shape
        rows = x.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(n * Hp * Wp, E).contiguous()
        return self.run(rows, n, Hp, Wp, state_labels, resolve_compute(None)).to(x.dtype)


def _heads(hidden_dim: int, num_heads: int):
    if hidden_dim % num_heads:
        raise ValueError(f"hidden_dim {hidden_dim} is not a multiple of num_heads {num_heads}")


def _bias_module(bias_type: str, num_heads: int):
    if bias_type == "none":
        return None
    if bias_type == "continuous":
        return ContinuousPositionBias1D(n_heads=num_heads)
    return RelativePositionBias(n_heads=num_heads)


class AxialAttentionBlock(nn.Module):
    """avit.py:223-286.  `rel_pos_bias` is held and never applied: the reference's attention calls get no mask."""

    def __init__(self, hidden_dim=768, num_heads=8, drop_path=0, layer_scale_init_value=1e-6, bias_type="rel"):
        super().__init__()
        _heads(hidden_dim, num_heads)
        self.num_heads = num_heads
        self.norm1 = RMSInstanceNorm2d(hidden_dim, affine=True)
        self.norm2 = RMSInstanceNorm2d(hidden_dim, affine=True)
        self.gamma_att = nn.Parameter(layer_scale_init_value * torch.ones(hidden_dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.gamma_mlp = nn.Parameter(layer_scale_init_value * torch.ones(hidden_dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.input_head = nn.Conv2d(hidden_dim, 3 * hidden_dim, 1)
        self.output_head = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.qnorm = nn.LayerNorm(hidden_dim // num_heads)
        self.knorm = nn.LayerNorm(hidden_dim // num_heads)
        self.rel_pos_bias = _bias_module(bias_type, num_heads)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.mlp = MLP(hidden_dim)
        self.mlp_norm = RMSInstanceNorm2d(hidden_dim, affine=True)
        self._cache = _PackCache()

    def _packed(self, compute: int):
        ih, oh, f1, f2 = self.input_head, self.output_head, self.mlp.fc1, self.mlp.fc2
        params = [ih.weight, ih.bias, oh.weight, oh.bias, f1.weight, f1.bias, f2.weight, f2.bias] + ([self.gamma_att] if self.gamma_att is not None else [])

        def build():
            wo, bo = fold_layer_scale(oh.weight, oh.bias, self.gamma_att)
            ca, cm = site(compute, "attn", BF16_SITES), site(compute, "mlp", BF16_SITES)
            return (S.pack_linear_chunks(ih.weight.detach().reshape(ih.weight.shape[0], -1), ih.bias, ca),
                    S.pack_linear_chunks(wo, bo, ca), S.pack_linear_chunks(f1.weight.detach(), f1.bias, cm),
                    S.pack_linear_chunks(f2.weight.detach(), f2.bias, cm))
        return self._cache.get(compute, params, build)

    def run(self, x: torch.Tensor, n: int, Hp: int, Wp: int, compute: int) -> torch.Tensor:
        """x (n Hp Wp, C) fp32 rows, updated IN PLACE and returned."""
        _token_grid(Hp, Wp)
        M, C_ = x.shape
        adt, mdt = K.act_torch_dtype(site(compute, "attn", BF16_SITES)), K.act_torch_dtype(site(compute, "mlp", BF16_SITES))
        inp, outp, fc1, fc2 = self._packed(compute)
        x3 = x.view(n, Hp * Wp, C_)
        n1 = self.norm1.run(x3, adt)
        qkv = S.linear_chunks(n1.view(M, C_), inp)
        att = axial_attention(qkv, n, self.num_heads, Hp, Wp, self.qnorm, self.knorm)
        n2 = self.norm2.run(att.view(n, Hp * Wp, C_), adt)
        S.linear_chunks(n2.view(M, C_), outp, residual=x, out=x)               # gamma_att folded; the skip rides the residual operand
        h = S.linear_chunks(x, fc1, mdt, L.ACT_GELU_ERF)
        y = S.linear_chunks(h, fc2)
        if self.gamma_mlp is None:
            instnorm(y.view(n, Hp * Wp, C_), L.INSTNORM_RMS, self.mlp_norm.weight.detach(), None, self.mlp_norm.eps, residual=x3,
                     gamma=torch.ones(C_, dtype=torch.float32, device=x.device), out=x3)
        else:
            self.mlp_norm.run(y.view(n, Hp * Wp, C_), residual=x3, gamma=self.gamma_mlp.detach(), out=x3)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, C, H, W) -> (B, C, H, W)  (avit.py:250-286).  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        B, C_, H, W = x.shape
        rows = x.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(B * H * W, C_).contiguous()
        y = self.run(rows, B, H, W, resolve_compute(None))
        return y.view(B, H, W, C_).permute(0, 3, 1, 2).to(x.dtype)


class AttentionBlock(nn.Module):
    """avit.py:288-331: attention over the T steps of every token with the bucketed relative-position bias."""

    def __init__(self, hidden_dim=768, num_heads=8, drop_path=0, layer_scale_init_value=1e-6, bias_type="rel"):
        super().__init__()
        _heads(hidden_dim, num_heads)
        self.num_heads = num_heads
        self.norm1 = nn.InstanceNorm2d(hidden_dim, affine=True)
        self.norm2 = nn.InstanceNorm2d(hidden_dim, affine=True)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(hidden_dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.input_head = nn.Conv2d(hidden_dim, 3 * hidden_dim, 1)
        self.output_head = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.qnorm = nn.LayerNorm(hidden_dim // num_heads)
        self.knorm = nn.LayerNorm(hidden_dim // num_heads)
        self.rel_pos_bias = _bias_module(bias_type, num_heads)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self._cache = _PackCache()
        self._zero = {}

    def _packed(self, compute: int):
        ih, oh = self.input_head, self.output_head
        params = [ih.weight, ih.bias, oh.weight, oh.bias] + ([self.gamma] if self.gamma is not None else [])

        def build():
            wo, bo = fold_layer_scale(oh.weight, oh.bias, self.gamma)
            ca = site(compute, "attn", BF16_SITES)
            return (S.pack_linear_chunks(ih.weight.detach().reshape(ih.weight.shape[0], -1), ih.bias, ca), S.pack_linear_chunks(wo, bo, ca))
        return self._cache.get(compute, params, build)

    def _bias(self, T: int, device) -> torch.Tensor:
        if isinstance(self.rel_pos_bias, RelativePositionBias):
            return self.rel_pos_bias.table(T)
        if self.rel_pos_bias is not None:
            raise NotImplementedError("the continuous position bias is out of scope: AViT's constructor cannot reach it")
        key = (T, str(device))
        if key not in self._zero:
            self._zero = {key: torch.zeros(self.num_heads, T, T, dtype=torch.float32, device=device)}
        return self._zero[key]

    def run(self, x: torch.Tensor, T: int, B: int, HW: int, compute: int) -> torch.Tensor:
        """x ((t b) HW, C) fp32 rows, updated IN PLACE and returned."""
        if T > MAX_T:
            raise NotImplementedError(f"T = {T} is out of scope: tante_time_attention serves 1..{MAX_T} time steps")
        _token_grid(1, HW)
        M, C_ = x.shape
        adt = K.act_torch_dtype(site(compute, "attn", BF16_SITES))
        inp, outp = self._packed(compute)
        n1 = instnorm(x.view(T * B, HW, C_), L.INSTNORM_INSTANCE, self.norm1.weight.detach(), self.norm1.bias.detach(), self.norm1.eps, adt)
        qkv = S.linear_chunks(n1.view(M, C_), inp)
        att = time_attention(qkv, B * HW, T, self.num_heads, self.qnorm, self.knorm, self._bias(T, x.device))
        n2 = instnorm(att.view(T * B, HW, C_), L.INSTNORM_INSTANCE, self.norm2.weight.detach(), self.norm2.bias.detach(), self.norm2.eps, adt)
        return S.linear_chunks(n2.view(M, C_), outp, residual=x, out=x)        # gamma folded; the skip rides the residual operand

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(T, B, C, H, W) -> (T, B, C, H, W)  (avit.py:308-331).  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        T, B, C_, H, W = x.shape
        rows = x.detach().to(torch.float32).permute(0, 1, 3, 4, 2).reshape(T * B * H * W, C_).contiguous()
        y = self.run(rows, T, B, H * W, resolve_compute(None))
        return y.view(T, B, H, W, C_).permute(0, 1, 4, 2, 3).to(x.dtype)


class SpaceTimeBlock(nn.Module):
    """The temporal block, then the spatial block with its MLP  (avit.py:333-377)."""

    def __init__(self, hidden_dim=768, num_heads=8, drop_path=0., space_override=None, time_override=None, gradient_checkpointing=False):
        super().__init__()
        if space_override is not None or time_override is not None:
            raise NotImplementedError("space_override / time_override are out of scope: the HIP path runs the axial and the time attention block")
        self.gradient_checkpointing = gradient_checkpointing
        self.spatial = AxialAttentionBlock(hidden_dim, num_heads, drop_path=drop_path)
        self.temporal = AttentionBlock(hidden_dim, num_heads, drop_path=drop_path)

    def run(self, x: torch.Tensor, T: int, B: int, Hp: int, Wp: int, compute: int) -> torch.Tensor:
        x = self.temporal.run(x, T, B, Hp * Wp, compute)
        return self.spatial.run(x, T * B, Hp, Wp, compute)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(T, B, C, H, W) -> (T, B, C, H, W).  Inference only."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        gpu_only(x, "AViT")
        T, B, C_, H, W = x.shape
        rows = x.detach().to(torch.float32).permute(0, 1, 3, 4, 2).reshape(T * B * H * W, C_).contiguous()
        y = self.run(rows, T, B, H, W, resolve_compute(None))
        return y.view(T, B, H, W, C_).permute(0, 1, 4, 2, 3).to(x.dtype)


class AViT(ComputeSwitch, nn.Module):
    """models/avit.py:379-454 -- same constructor, attributes, parameters and forward contract."""

    def __init__(self, in_T, dset_metadata=None, out_steps: int = 4, patch_size=(16, 16), embed_dim=768, num_heads=12, processor_blocks=8,
                 override_block=None, drop_path=.2):
        super().__init__()
        if override_block is not None:
            raise NotImplementedError("override_block is out of scope: the HIP path runs the reference's default SpaceTimeBlock")
        n_states = dset_metadata.n_fields if dset_metadata else 11
        self.drop_path = drop_path
        self.dp = np.linspace(0, drop_path, processor_blocks)
        self.space_bag = SubsampledLinear(n_states, embed_dim // 4)
        self.embed = hMLP_stem(patch_size=patch_size, in_chans=embed_dim // 4, embed_dim=embed_dim)
        self.out_steps = out_steps
        inner_block = partial(SpaceTimeBlock, hidden_dim=embed_dim, num_heads=num_heads)
        self.blocks = nn.ModuleList([inner_block(drop_path=self.dp[i]) for i in range(processor_blocks)])
        self.debed = hMLP_output(patch_size=patch_size, embed_dim=embed_dim, out_chans=n_states)
        self.n_states, self.embed_dim, self.num_heads, self.patch_size = n_states, embed_dim, num_heads, patch_size
        self._cache = _PackCache()

    def _packed_stem(self, compute: int, c: int):
        sb, c0 = self.space_bag, self.embed.in_proj[0]

        def build():
            w, b = fold_stem(sb.weight, sb.bias, c0.weight, c)
            return S.pack_linear_chunks(w, b, site(compute, "stem", BF16_SITES))
        return self._cache.get((compute, c), [sb.weight, sb.bias, c0.weight], build)

    def encode(self, xn: torch.Tensor, compute: Optional[int] = None) -> torch.Tensor:
        """The stem on normalised fields xn (n, H, W, c) fp32 channels-last -> rows (n H/16 W/16, embed_dim) fp32: space_bag with
        labels range(c) and the first convolution run as one folded convolution."""
        c = xn.shape[-1]
        if c > self.n_states:
            raise ValueError(f"the input has {c} fields, the model holds {self.n_states} states")
        compute = resolve_compute(self.compute) if compute is None else compute
        return self.embed.run(xn, compute, self._packed_stem(compute, c))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, min(t, 4), c, h, w)   (avit.py:419-454)."""
        inference_only(self, "AViT", WHY_INFERENCE_ONLY)
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, C, H, W), got {tuple(x.shape)}")
        gpu_only(x, "AViT")
        b, T, c, h, w = x.shape
        if c > self.n_states:
            raise ValueError(f"the input has {c} fields, the model holds {self.n_states} states")
        if h % 16 or w % 16:
            raise ValueError(f"H and W must be multiples of 16 (the stem is 4 x 2 x 2), got {h} x {w}")
        Hp, Wp = h // 16, w // 16
        _token_grid(Hp, Wp)
        if T > MAX_T:
            raise NotImplementedError(f"T = {T} is out of scope: tante_time_attention serves 1..{MAX_T} time steps")
        compute = resolve_compute(self.compute)
        stats, xn = field_stats(x.detach().to(torch.float32).contiguous())
        rows = self.encode(xn, compute)                                         # ((t b) Hp Wp, E)
        for blk in self.blocks:
            rows = blk.run(rows, T, b, Hp, Wp, compute)
        k = min(T, OUT_STEPS)
        tail = rows[(T - k) * b * Hp * Wp:]                                      # the steps x[-4:] keeps: the head is per image
        img = self.debed.run(tail, k * b, Hp, Wp, range(c), compute)
        return field_affine(img, stats, b)
