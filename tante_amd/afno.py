"""AFNO baseline on the HIP kernels  (reference models/afno.py, configs/afno.yaml: the adaptive Fourier neural operator of FourCastNet).

Same constructor arguments, attributes, `state_dict` keys / shapes and forward contract (`b t c h w -> b 1 c h w`, so the sliding-window
rollout re-feeds it one frame per call) as the reference's models.AFNO.  Every arithmetic step is a C-ABI call of libtante_hip:
tante_im2col + chunked tante_gemm (the Conv2d patch embed, with the positional embedding riding the GEMM's residual operand),
tante_layernorm_affine (norm1), tante_afno_filter (the spectral filter, its axis swap and the first skip), tante_gemm with LayerNorm 2
folded in + erf GELU, chunked tante_gemm with the second skip as the residual, and the transposed-conv de-embedding as one scatter GEMM.
torch allocates and reshapes.

Reference quirks kept on purpose (pinned by the g18 fixtures):
  * the filter transforms over dim=(2, 1): the HALF spectrum is taken over axis 1 (H), the full transform over axis 2 (W)  (afno.py:106);
  * the inverse receives s=resolution against those reversed axes, i.e. the SWAPPED sizes -- for H != W a frequency crop / zero pad --
    and returns (b, W, H, C), which Block.forward swaps back  (afno.py:113-115, 155);
  * ComplexBlockLinear takes `bias=True` and creates no bias  (afno.py:22-44); the filter runs in fp32 also under autocast (l.105);
  * a freshly initialised filter is identically zero on unit-variance input: weights of scale 0.02 against a soft threshold of 0.01.

Inference is the default: under grad a model whose parameters require one refuses (NotImplementedError), as it always did.  Training is
opt-in through `model.set_trainable()`.  An opted-in model called under grad takes afno_train_forward: the same arithmetic as a graph
of the training nodes of tante_amd/autograd.py (Im2colFn + LinearFn for the patch embedding, LayerNormAffineFn, LinearFn, ActFn,
DeconvFn) with AfnoFilterFn for the filter, whose forward is the unchanged tante_afno_filter (bit-identical to inference) and whose
backward is tante_afno_filter_bwd (csrc/afno_filter_bwd.hip).  The input receives a gradient too, so `rollout_model` back-propagates
through its re-fed frames and `train.train_step` works with FlatAdamW as for the other trained models.  Dropout / drop-path in train()
and n_spatial_dims = 3 raise NotImplementedError with or without the opt-in; there is no CPU fallback."""
from __future__ import annotations

import contextlib
from functools import partial
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L
from . import kernels as K
from . import stages as S
from .attn_backbone import _PackCache, resolve_compute
from .dft_tables import cis, device_tables, pack_tables
from .model_shell import ComputeSwitch, Trainable, gpu_only, wants_graph

MAX_GRID = 64     # token-grid points per axis the filter kernels serve
MAX_BLOCK = 64    # channels per diagonal block


# ---- host side of tante_afno_filter: the predicate's mirror, the twiddle tables, the real-ified weights ---------------------------------
def filter_supported_py(B: int, H: int, W: int, C_: int, bs: int) -> bool:
    """Python mirror of tante_afno_filter_supported."""
    return (1 <= H <= MAX_GRID and 1 <= W <= MAX_GRID and 1 <= bs <= MAX_BLOCK and C_ >= 1 and C_ % bs == 0 and 0 <= B <= 65535)


def filter_supported(B: int, H: int, W: int, C_: int, bs: int) -> bool:
    return bool(L.lib().tante_afno_filter_supported(B, H, W, C_, bs))


def kept_modes(H: int, W: int) -> Tuple[int, int]:
    """(Lc, Kc): the entries of axis 2 / axis 1 of the spectrum that the swapped-size inverse reads."""
    return min(H, W), min(H // 2 + 1, W // 2 + 1)


def twiddle_tables(H: int, W: int) -> List[np.ndarray]:
    """The four complex128 tables of tante_afno_filter (include/tante_hip.h), unpadded: T1 (Lc, W), T2 (Kc, H), T3 (W, Kc), T4 (H, Lc)."""
    Lc, Kc = kept_modes(H, W)
    l, k, w, h = np.arange(Lc), np.arange(Kc), np.arange(W), np.arange(H)
    ck = np.where((k == 0) | ((W % 2 == 0) & (k == W // 2)), 1.0, 2.0)
    return [cis(np.outer(l, w), W, -1) / np.sqrt(W), cis(np.outer(k, h), H, -1) / np.sqrt(H),
            cis(np.outer(w, k), W, +1) * ck[None, :] / np.sqrt(W), cis(np.outer(h, l), H, +1) / np.sqrt(H)]


def pack_twiddles(H: int, W: int) -> np.ndarray:
    """-> the float32 buffer tante_afno_filter reads: per table a real then an imaginary plane, rows padded to 16, columns to 4."""
    return pack_tables(twiddle_tables(H, W))


def pack_twiddles_bwd(H: int, W: int) -> np.ndarray:
    """-> the float32 buffer of adjoint tables tante_afno_filter_bwd reads: the conjugate transposes T1^H (W, Lc), T2^H (H, Kc),
    T3^H (Kc, W), T4^H (Lc, H) of the same float64 tables, rounded once and padded like pack_twiddles."""
    return pack_tables([t.conj().T for t in twiddle_tables(H, W)])


def pack_block_weight(weight: torch.Tensor) -> torch.Tensor:
    """ComplexBlockLinear.weight (n_blocks, bs, bs, 2) -> the real-ified (n_blocks, 2 bsP, 2 bsP) fp32 matrices [[Wr, Wi], [-Wi, Wr]]
    ([Re | Im] . M = [Re Wr - Im Wi | Re Wi + Im Wr]), bsP = bs rounded up to 16, zero padded."""
    w = weight.detach().to(torch.float32)
    nb, bs = w.shape[0], w.shape[1]
    bp = (bs + 15) // 16 * 16
    m = torch.zeros(nb, 2 * bp, 2 * bp, dtype=torch.float32, device=w.device)
    wr, wi = w[..., 0], w[..., 1]
    m[:, :bs, :bs] = wr
    m[:, :bs, bp:bp + bs] = wi
    m[:, bp:bp + bs, :bs] = -wi
    m[:, bp:bp + bs, bp:bp + bs] = wr
    return m.contiguous()


def _twiddles(H: int, W: int, device) -> torch.Tensor:
    return device_tables(("afno", H, W), lambda: pack_twiddles(H, W), L.lib().tante_afno_twiddle_floats(H, W),
                         f"twiddle tables for a {H} x {W} grid", device)


def _twiddles_bwd(H: int, W: int, device) -> torch.Tensor:
    return device_tables(("afno_bwd", H, W), lambda: pack_twiddles_bwd(H, W), L.lib().tante_afno_twiddle_bwd_floats(H, W),
                         f"adjoint twiddle tables for a {H} x {W} grid", device)


def afno_filter(x: torch.Tensor, residual: Optional[torch.Tensor], w1: torch.Tensor, w2: torch.Tensor, bs: int, lam: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tante_afno_filter on x (B, H, W, C) fp32 channels-last: residual + swap_hw(filter(x)); w1 / w2 from pack_block_weight."""
    return _filter_launch(x, residual, w1, w2, bs, lam, out)[0]


def _filter_launch(x, residual, w1, w2, bs, lam, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out, the call's workspace: P (B, Lc, H, 2, C) then G (B, W, Lc, 2, C), as bytes)."""
    K._dev(x, residual, w1, w2, out)
    if x.dtype != torch.float32 or x.dim() != 4 or (residual is not None and residual.dtype != torch.float32):
        raise RuntimeError("the AFNO filter takes fp32 channels-last rows (B, H, W, C)")
    B, H, W, C_ = x.shape
    lib = L.lib()
    if not lib.tante_afno_filter_supported(B, H, W, C_, bs):
        # the call itself refuses with the reason; made here without touching the device
        L.check(lib.tante_afno_filter(None, None, B, H, W, C_, bs, None, None, None, float(lam), None, None, 0, None), "tante_afno_filter")
    if out is None:
        out = torch.empty_like(x)
    work, nbytes = K.workspace(lib.tante_afno_filter_workspace_bytes(B, H, W, C_), x.device)
    L.check(lib.tante_afno_filter(K._p(x), K._p(residual), B, H, W, C_, bs, K._p(_twiddles(H, W, x.device)), K._p(w1), K._p(w2), float(lam),
                                  K._p(out), K._p(work), nbytes, K._stream()), "tante_afno_filter")
    return out, work


# ---- training: the filter as an autograd node -------------------------------------------------------------------------------------------
_KEEP_SINK = [None]


@contextlib.contextmanager
def record_keep_masks(sink: list):
    """Inside this scope every AfnoFilterFn.backward also asks the kernel for its threshold decisions [|Yp| > lambda] and appends them to
    `sink` as a (B, Lc, Kc, 2, C) uint8 tensor, in the order the backward calls run (the reverse of the forward calls).  For tests that
    restate the decisions; outside the scope nothing is allocated."""
    prev, _KEEP_SINK[0] = _KEEP_SINK[0], sink
    try:
        yield sink
    finally:
        _KEEP_SINK[0] = prev


_BLOCK_PACKS = {}     # (data_ptr, version, shape) -> (real-ified matrices, the weight), all of weight epoch _BLOCK_PACKS_EPOCH[0]
_BLOCK_PACKS_EPOCH = [-1]


def _packed_block_weight(w: torch.Tensor) -> torch.Tensor:
    """pack_block_weight(w), shared by the BPTT calls of one step.  FlatAdamW updates the parameters through raw pointers, which moves
    neither their address nor their version: it bumps attn_backbone's weight epoch instead, and a new epoch empties this cache, as it
    invalidates every _PackCache."""
    from .attn_backbone import _WEIGHT_EPOCH
    if _BLOCK_PACKS_EPOCH[0] != _WEIGHT_EPOCH[0] or len(_BLOCK_PACKS) >= 256:
        _BLOCK_PACKS.clear()
        _BLOCK_PACKS_EPOCH[0] = _WEIGHT_EPOCH[0]
    key = (w.data_ptr(), w._version, tuple(w.shape))
    hit = _BLOCK_PACKS.get(key)
    if hit is None:
        hit = _BLOCK_PACKS[key] = (pack_block_weight(w), w)      # the weight is held so that its address stays its own
    return hit[0]


class AfnoFilterFn(Function):
    """residual + swap_hw(filter(x)) on x (B, H, W, C) fp32 with ComplexBlockLinear weights weight1 / weight2 (n_blocks, bs, bs, 2).
    Forward: the unchanged tante_afno_filter on a workspace the node owns; the P part of it (the transform along w) is what the backward
    recomputes the spectrum from, so x itself is not saved.  (The entry point takes one workspace, P then G, so the G half -- as large
    as P for a square grid -- stays allocated with it until the backward ran; a copy of P would free it at the price of a launch per
    block.)  Backward: tante_afno_filter_bwd; the weight gradients go straight into the parameters' gradient slots where those exist
    (FlatAdamW), the residual's gradient is dout itself."""

    @staticmethod
    def forward(ctx, x, residual, weight1, weight2, bs, lam):
        x = x.contiguous()
        residual = None if residual is None else residual.contiguous()
        K._dev(weight1, weight2)
        w1, w2 = _packed_block_weight(weight1), _packed_block_weight(weight2)
        out, work = _filter_launch(x, residual, w1, w2, bs, lam)
        ctx.save_for_backward(work, w1, w2)      # P is the head of the workspace
        ctx.geo = (*x.shape, int(bs), float(lam))
        ctx.has_res = residual is not None
        ctx.params = (weight1, weight2)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .autograd import grad_slots
        work, w1, w2 = ctx.saved_tensors
        B, H, W, C_, bs, lam = ctx.geo
        dout = dout.contiguous()
        dev = dout.device
        lib = L.lib()
        dx = torch.empty_like(dout)
        slots = grad_slots(ctx, ctx.params, 2)
        into = slots is not None
        dws = slots if into else [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in ctx.params]
        keep = None
        if _KEEP_SINK[0] is not None:
            Lc, Kc = kept_modes(H, W)
            keep = torch.empty(B, Lc, Kc, 2, C_, dtype=torch.uint8, device=dev)
            _KEEP_SINK[0].append(keep)
        ws, nbytes = K.workspace(lib.tante_afno_filter_bwd_workspace_bytes(B, H, W, C_, bs), dev)
        L.check(lib.tante_afno_filter_bwd(K._p(dout), K._p(work), B, H, W, C_, bs, K._p(_twiddles(H, W, dev)), K._p(_twiddles_bwd(H, W, dev)),
                                          K._p(w1), K._p(w2), lam, K._p(dx), K._p(dws[0]), K._p(dws[1]), int(into), K._p(keep), K._p(ws), nbytes,
                                          K._stream()), "tante_afno_filter_bwd")
        g1, g2 = (None, None) if into else (dws[0] if ctx.needs_input_grad[2] else None, dws[1] if ctx.needs_input_grad[3] else None)
        return dx, (dout if ctx.has_res else None), g1, g2, None, None


def _no_dropout(training: bool, *rates):
    if training and any(r > 0.0 for r in rates):
        raise NotImplementedError("drop_rate / drop_path_rate > 0 in train() is out of scope: dropout and stochastic depth are not part of "
                                  "the training path (set_trainable); call .eval(), or build the model with both rates at 0")


def block_train(blk: "Block", x: torch.Tensor, compute: int) -> torch.Tensor:
    """Block.run as a graph of training nodes: x (B, H, W, C) fp32 -> block(x)."""
    from .autograd import ActFn, LayerNormAffineFn, LinearFn
    _no_dropout(blk.training, blk.drop_path_rate, blk.mlp.drop.p)
    B, H, W, C_ = x.shape
    M = B * H * W
    adt = K.act_torch_dtype(compute)
    f, m = blk.filter, blk.mlp
    n1 = LayerNormAffineFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    x1 = AfnoFilterFn.apply(n1, x if blk.double_skip else None, f.cmlp[0].weight, f.cmlp[2].weight, f.hidden_size // f.cmlp_diagonal_blocks,
                            f.sparsity_threshold)
    skip = x1 if blk.double_skip else x
    n2 = LayerNormAffineFn.apply(x1, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
    h = ActFn.apply(LinearFn.apply(n2.view(M, C_), m.fc1.weight, m.fc1.bias, None, compute, adt), L.ACT_GELU_ERF, adt)
    return LinearFn.apply(h, m.fc2.weight, m.fc2.bias, skip.reshape(M, C_), compute, torch.float32).view(B, H, W, C_)


def afno_train_forward(model: "AFNO", x: torch.Tensor, compute: int) -> torch.Tensor:
    """AFNO.forward with an autograd graph: x (b, t, c, h, w) -> (b, 1, c, h, w) fp32.  torch only re-lays out (the channels-last copy of
    the input, parameter-sized weight views); every activation-sized operation is a HIP node."""
    from .autograd import DeconvFn, Im2colFn, LinearFn, PosRowsFn
    b, t, c, h, w = x.shape
    p, C_ = model.patch_size, model.hidden_dim
    Hp, Wp = h // p, w // p
    pe, pd = model.patch_embed, model.patch_debed
    img = x.to(torch.float32).reshape(b, t * c, h, w).permute(0, 2, 3, 1).contiguous()       # 'b t c h w -> b h w (t c)'
    cols = Im2colFn.apply(img, b, t * c, h, w, p, p, 0, K.act_torch_dtype(compute))           # columns (kh, kw, channel)
    w2d = pe.weight.permute(0, 2, 3, 1).reshape(C_, -1).contiguous()                          # the same order, a parameter-sized re-layout
    y = LinearFn.apply(cols, w2d, pe.bias, PosRowsFn.apply(model.pos_embed, b), compute, torch.float32).view(b, Hp, Wp, C_)
    for blk in model.blocks:
        y = block_train(blk, y, compute)
    out = DeconvFn.apply(y.view(b * Hp * Wp, C_), pd.weight, pd.bias, b, Hp, Wp, p, True, compute, torch.float32)
    return out.unsqueeze(1)                                                                   # 'b c h w -> b 1 c h w'


# ---- the reference's modules -------------------------------------------------------------------------------------------------------
class RealImagGELU(nn.Module):
    """gelu(Re) + i gelu(Im)  (afno.py:17-19): evaluated inside tante_afno_filter."""


class ComplexBlockLinear(nn.Module):
    """Block-diagonal complex linear layer, no bias  (afno.py:22-49): the weight of one layer of tante_afno_filter's MLP."""

    def __init__(self, hidden_dim, bias=True, cmlp_diagonal_blocks=8):
        super().__init__()
        self.scale = 0.02
        self.hidden_dim = hidden_dim
        self.cmlp_diagonal_blocks = cmlp_diagonal_blocks
        self.block_size = self.hidden_dim // self.cmlp_diagonal_blocks
        self.weight = nn.Parameter(torch.view_as_real(self.scale * torch.randn(cmlp_diagonal_blocks, self.block_size, self.block_size,
                                                                                dtype=torch.cfloat)))


class Mlp(nn.Module):
    """fc2(gelu_erf(fc1(x)))  (afno.py:52-75)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class AFNO_ND(Trainable, nn.Module):
    """The spectral filter  (afno.py:78-117)."""

    def __init__(self, hidden_size: int, resolution, cmlp_diagonal_blocks=8, sparsity_threshold=0.01):
        super().__init__()
        assert hidden_size % cmlp_diagonal_blocks == 0, \
            f"hidden_size {hidden_size} should be divisble by cmlp_diagonal_blocks {cmlp_diagonal_blocks}"
        self.resolution = resolution
        self.hidden_size = hidden_size
        self.sparsity_threshold = sparsity_threshold
        self.cmlp_diagonal_blocks = cmlp_diagonal_blocks
        self.scale = 0.02
        self.cmlp = nn.Sequential(ComplexBlockLinear(hidden_size, cmlp_diagonal_blocks=cmlp_diagonal_blocks), RealImagGELU(),
                                  ComplexBlockLinear(hidden_size, cmlp_diagonal_blocks=cmlp_diagonal_blocks))
        self._cache = _PackCache()

    def _packed(self):
        ws = [self.cmlp[0].weight, self.cmlp[2].weight]
        return self._cache.get(0, ws, lambda: tuple(pack_block_weight(w) for w in ws))

    def run(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """x (B, H, W, C) fp32 -> swap_hw(filter(x)) (+ residual): the (B, H, W, C) stream Block.forward holds after its first skip."""
        w1, w2 = self._packed()
        return afno_filter(x, residual, w1, w2, self.hidden_size // self.cmlp_diagonal_blocks, self.sparsity_threshold)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(b, H, W, C) -> (b, W, H, C), as the reference returns it (afno.py:103-117).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        if x.dim() != 4:
            raise NotImplementedError("the AFNO filter is two-dimensional here: n_spatial_dims = 3 is out of scope")
        gpu_only(x, "AFNO")
        if train:
            y = AfnoFilterFn.apply(x.to(torch.float32), None, self.cmlp[0].weight, self.cmlp[2].weight,
                                   self.hidden_size // self.cmlp_diagonal_blocks, self.sparsity_threshold)
            return y.transpose(1, 2).to(x.dtype)
        return self.run(x.detach().to(torch.float32).contiguous(), None).transpose(1, 2).to(x.dtype)


class Block(Trainable, nn.Module):
    """x = swap_hw(filter(norm1 x)) + x;  x = mlp(norm2 x) + x   (afno.py:120-166)."""

    def __init__(self, hidden_dim, resolution, mlp_ratio=4.0, drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 double_skip=True, cmlp_diagonal_blocks=8, sparsity_threshold=0.01):
        super().__init__()
        self.norm1 = norm_layer(hidden_dim)
        self.filter = AFNO_ND(hidden_dim, resolution, cmlp_diagonal_blocks, sparsity_threshold)
        self.drop_path = nn.Identity()
        self.drop_path_rate = float(drop_path)
        self.norm2 = norm_layer(hidden_dim)
        mlp_hidden_dim = int(hidden_dim * mlp_ratio)
        self.mlp = Mlp(in_features=hidden_dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.double_skip = double_skip
        self.hidden_dim = hidden_dim
        self._cache = _PackCache()

    def _packed(self, compute: int):
        n2, m = self.norm2, self.mlp
        params = [n2.weight, n2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias]
        return self._cache.get(compute, params, lambda: dict(
            fc1_ln2=K.pack_weight(m.fc1.weight, m.fc1.bias, compute, gamma=n2.weight, beta=n2.bias),
            fc2=S.pack_linear_chunks(m.fc2.weight.detach(), m.fc2.bias, compute)))

    def run(self, x: torch.Tensor, compute: int) -> torch.Tensor:
        """x (B, H, W, C) fp32 -> block(x), same shape."""
        B, H, W, C_ = x.shape
        M = B * H * W
        pk = self._packed(compute)
        n1 = K.layernorm_affine(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        if self.double_skip:
            x1 = self.filter.run(n1, x)              # the filter's store epilogue adds the first skip
            skip = x1
        else:
            x1 = self.filter.run(n1, None)
            skip = x
        h = torch.empty(M, pk["fc1_ln2"].N, dtype=K.act_torch_dtype(compute), device=x.device)
        K.linear(x1.view(M, C_), pk["fc1_ln2"], h, M=M, act=L.ACT_GELU_ERF, ln=True, ln_eps=self.norm2.eps)
        return S.linear_chunks(h, pk["fc2"], residual=skip.view(M, C_)).view(B, H, W, C_)       # the skip rides the residual operand

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        train = wants_graph(self, x, _refuse)
        if train:
            _no_dropout(self.training, self.drop_path_rate, self.mlp.drop.p)
        if x.dim() != 4:
            raise NotImplementedError("the AFNO block is two-dimensional here: n_spatial_dims = 3 is out of scope")
        gpu_only(x, "AFNO")
        if train:
            return block_train(self, x.to(torch.float32), resolve_compute(None))
        return self.run(x.detach().to(torch.float32).contiguous(), resolve_compute(None))


def _refuse(module: nn.Module):
    """AFNO's refusal of a module that has not opted in.  Unlike DPOT and UNetConvNext, which hand model_shell.inference_only to the gate,
    it refuses only under grad with a parameter that requires one -- not in train() under no_grad -- and in words of its own.  That
    difference is pinned behaviour: tests/test_afno_train_cpu.py::test_opt_in_surface and tests/test_hip_afno_train.py."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise NotImplementedError("tante_amd.AFNO is inference only unless set_trainable() was called: training is out of scope for this "
                                  "model as it stands; opt in, or call it in eval mode under torch.no_grad()")


class AFNO(Trainable, ComputeSwitch, nn.Module):
    """models/afno.py:169-278 -- same constructor, attributes, parameters and forward contract."""

    def __init__(self, in_T, dset_metadata=None, hidden_dim=256, n_blocks=12, cmlp_diagonal_blocks=8, patch_size=8, mlp_ratio=4.0,
                 drop_rate=0.0, drop_path_rate=0.0, sparsity_threshold=0.01):
        super().__init__()
        n_channel = dset_metadata.n_fields if dset_metadata else 5
        dim_in = n_channel * in_T
        dim_out = n_channel
        self.dim_in = dim_in
        self.dim_out = dim_out
        self.resolution = dset_metadata.spatial_resolution if dset_metadata else (128, 384)
        self.n_spatial_dims = dset_metadata.n_spatial_dims if dset_metadata else 2
        self.n_blocks = n_blocks
        self.cmlp_diagonal_blocks = cmlp_diagonal_blocks
        self.in_T, self.hidden_dim, self.patch_size = in_T, hidden_dim, patch_size
        self.drop_rate, self.drop_path_rate = float(drop_rate), float(drop_path_rate)
        norm_layer = partial(nn.LayerNorm, eps=1e-6)
        if self.n_spatial_dims == 3:
            raise NotImplementedError("AFNO with n_spatial_dims = 3 is out of scope: the HIP filter is two-dimensional (no dataset of the "
                                      "reference is 3-D)")
        if self.n_spatial_dims != 2 or len(self.resolution) != 2:
            raise ValueError(f"n_spatial_dims must be 2, got {self.n_spatial_dims} with resolution {tuple(self.resolution)}")
        self.patch_embed = nn.Conv2d(dim_in, hidden_dim, kernel_size=patch_size, stride=patch_size)
        self.embed_permutation = ["b h w c -> b c h w", "b c h w -> b h w c"]
        self.patch_debed = nn.ConvTranspose2d(hidden_dim, dim_out, kernel_size=patch_size, stride=patch_size)
        self.inner_size = [k // patch_size for k in self.resolution]
        self.pos_embed = nn.Parameter(0.02 * torch.randn([1] + self.inner_size + [hidden_dim]))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, n_blocks)]
        self.blocks = nn.ModuleList([Block(hidden_dim=hidden_dim, resolution=self.inner_size, mlp_ratio=mlp_ratio, drop=drop_rate,
                                           drop_path=dpr[i], norm_layer=norm_layer, cmlp_diagonal_blocks=self.cmlp_diagonal_blocks,
                                           sparsity_threshold=sparsity_threshold) for i in range(n_blocks)])
        self.apply(self._init_weights)
        self.output_length = 1
        self._cache = _PackCache()
        self._pos = _PackCache()

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            torch.nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def _packed(self, compute: int):
        pe, pd = self.patch_embed, self.patch_debed
        p = self.patch_size
        return self._cache.get(compute, [pe.weight, pe.bias, pd.weight, pd.bias], lambda: (
            S.pack_linear_chunks(pe.weight.detach().reshape(pe.weight.shape[0], -1), pe.bias, compute),
            K.pack_weight(pd.weight, pd.bias, compute, L.W_DECONV_NCHW, N=pd.weight.shape[1] * p * p, K=pd.weight.shape[0], P=p,
                          C_other=pd.weight.shape[1])))

    def forward_features(self, x: torch.Tensor, compute: int) -> torch.Tensor:
        """x (b, t c, h, w) fp32 contiguous -> tokens (b, H', W', C) fp32  (afno.py:257-268)."""
        b, cin, h, w = x.shape
        p, C_ = self.patch_size, self.hidden_dim
        Hp, Wp = h // p, w // p
        M = b * Hp * Wp
        chunks, _ = self._packed(compute)
        cols = K.im2col(x, True, b, cin, h, w, p, p, p, p, 0, 0, 0, K.act_torch_dtype(compute))
        # x + pos_embed: the embedding's rows, repeated per sample, are the residual the first K-chunk accumulates onto
        pos = self._pos.get(b, [self.pos_embed], lambda: self.pos_embed.detach().expand(b, -1, -1, -1).reshape(M, C_).contiguous())
        y = S.linear_chunks(cols, chunks, residual=pos).view(b, Hp, Wp, C_)
        for blk in self.blocks:
            y = blk.run(y, compute)
        return y

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, 1, c, h, w)   (afno.py:270-278)."""
        train = wants_graph(self, x, _refuse)
        _no_dropout(self.training, self.drop_rate, self.drop_path_rate)
        if x.dim() != 5 or x.shape[1] * x.shape[2] != self.dim_in:
            raise ValueError(f"expected (B, {self.in_T}, {self.dim_out}, H, W), got {tuple(x.shape)}")
        gpu_only(x, "AFNO")
        b, t, c, h, w = x.shape
        p = self.patch_size
        if [h // p, w // p] != list(self.inner_size) or h % p or w % p:
            raise ValueError(f"input {h} x {w} does not give the {tuple(self.inner_size)} token grid of pos_embed at patch size {p}")
        compute = resolve_compute(self.compute)
        if train:
            return afno_train_forward(self, x, compute)
        x = x.detach().to(torch.float32).contiguous().view(b, t * c, h, w)       # 'b t c h w -> b (t c) h w' (the conv's channel order)
        y = self.forward_features(x, compute)
        _, pd = self._packed(compute)
        Hp, Wp = self.inner_size
        out = torch.empty(b, self.dim_out, h, w, dtype=torch.float32, device=x.device)
        K.deconv(y.view(b * Hp * Wp, self.hidden_dim), pd, out, n_img=b, Hi=Hp, Wi=Wp, P=p, Cout=self.dim_out, nchw_out=True, act=L.ACT_NONE)
        return out.unsqueeze(1)                                                  # 'b c h w -> b 1 c h w'
