"""DPOT baseline on the HIP kernels  (reference models/dpot.py, configs/dpot.yaml: the other Fourier-mixer model of the comparison table).

Same constructor arguments, attributes, `state_dict` keys / shapes and forward contract (`b t c h w -> b out_timesteps c h w`, so the
sliding-window rollout re-feeds it `out_timesteps` frames per call) as the reference's models.DPOT.  The model is channels-last inside and
every arithmetic step is a C-ABI call of libtante_hip:
  patch embed   tante_im2col + chunked tante_gemm with the erf-GELU epilogue, then tante_gemm with the positional embedding riding its
                residual operand (dpot.py:187-191, 254, 332); the three coordinate channels of get_grid_3d are constants kept in a cached
                staging image, into which the fields are copied -- ONE strided copy per call, layout only, no arithmetic;
  time agg      one GEMM with K = T C, K-chunked per t, reading the ((b t), x, y, C) rows in place and accumulating through the
                residual operand; 'exp_mlp' folds cos(linspace(0, 1, T)[t] gamma[i]) into w[t, i, :] in float64 at pack time;
  Block         tante_groupnorm (norm1), tante_dpot_filter (the truncated-mode mixer, its inner skip, and the first skip under
                double_skip), tante_groupnorm in the activation dtype (norm2), chunked tante_gemm + erf GELU, chunked tante_gemm with
                the skip as the residual (dpot.py:158-172, the 1 x 1 convolutions run as linears);
  out_layer     the transposed conv as one scatter GEMM with GELU (embed_dim <= 512) or as a chunked tap GEMM + tante_col2im_nhwc +
                tante_act_fwd, then two pixel-row linears; the last one writes (b, (t c), h, w), which IS b t c h w.
torch allocates, reshapes and makes the one copy named above.

`cls_head` holds its parameters for the state dict and is NEVER evaluated: the reference computes cls_pred and discards it
(dpot.py:343-344).

Inference is the default: a model whose parameters require a gradient refuses under grad (and in train()), as it always did.  Training is
opt-in through `model.set_trainable()`.  An opted-in model called under grad takes dpot_train_forward: the same arithmetic as a graph of
the training nodes of tante_amd/autograd.py (Im2colFn, LinearFn with K chunks, ActFn, DeconvFn / Col2imFn, PosRowsFn), with three
nodes of this module: DpotFilterFn (forward the unchanged tante_dpot_filter, bit-identical to inference; backward tante_dpot_filter_bwd:
the forward's launches 1 .. 3 again for X and U, then the chain in reverse against the conjugate-transposed tables, the block MLP against
the conjugated transposed weights, one wave per 16 x 16 tile of a weight gradient), GroupNormFn (tante_groupnorm_bwd: statistics as the
forward computes them, slab sums, a combine in order) and TimeAggFn (per-t GEMMs; the 'exp_mlp' fold's chain rule is parameter-sized
float64 torch).  Every sum of the backward kernels has a fixed order and there are no atomics, so two runs give the same bits.  The input
receives a gradient too, so `rollout_model` back-propagates through its re-fed frames and `train.train_step` works with
`FlatAdamW(model.trained_parameters())` -- every parameter except cls_head.*, which never receives a gradient.  Under no_grad an opted-in
model takes the unchanged inference path; train() changes nothing further (DPOT has no dropout).  n_spatial_dims = 3, act other than
'gelu', mixing_type other than 'afno' and hidden_size_factor != 1 raise NotImplementedError with or without the opt-in; there is no CPU
fallback."""
from __future__ import annotations

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
from .model_shell import ComputeSwitch, Trainable, gpu_only, inference_only, wants_graph

MAX_GRID = 64       # token-grid points per axis the mixer serves
MAX_BLOCK = 512     # channels per block
MAX_TOKENS = 4096   # tokens per sample tante_groupnorm serves
GROUPS = 8          # torch.nn.GroupNorm(8, width)  (dpot.py:138, 147)


# ---- host side of tante_groupnorm / tante_dpot_filter: the predicates' mirrors, the twiddle tables -----------------------------------------
def groupnorm_supported_py(B: int, HW: int, C_: int, G: int) -> bool:
    """Python mirror of tante_groupnorm_supported."""
    return 1 <= HW <= MAX_TOKENS and G >= 1 and 1 <= C_ <= (1 << 24) and C_ % G == 0 and 0 <= B and B * G <= 2 ** 31 - 1


def filter_supported_py(B: int, H: int, W: int, C_: int, bs: int, modes: int, hidden_factor: int = 1) -> bool:
    """Python mirror of tante_dpot_filter_supported."""
    return (1 <= H <= MAX_GRID and 1 <= W <= MAX_GRID and 1 <= bs <= MAX_BLOCK and C_ >= 1 and C_ % bs == 0 and C_ // bs <= 65535
            and modes >= 1 and hidden_factor == 1 and 0 <= B <= 65535)


def kept_modes(H: int, W: int, modes: int) -> Tuple[int, int]:
    """(k1, k2): the rows / columns of the half spectrum the mixer keeps -- a `modes` past the grid clamps, as Python slicing does."""
    return min(modes, H), min(modes, W // 2 + 1)


def twiddle_tables(H: int, W: int, modes: int) -> List[np.ndarray]:
    """The four complex128 tables of tante_dpot_filter (include/tante_hip.h), unpadded: T1 (k2, W), T2 (k1, H), T3 (H, k1), T4 (W, k2)."""
    k1, k2 = kept_modes(H, W, modes)
    k, l, h, w = np.arange(k1), np.arange(k2), np.arange(H), np.arange(W)
    cl = np.where((l == 0) | ((W % 2 == 0) & (l == W // 2)), 1.0, 2.0)
    return [cis(np.outer(l, w), W, -1) / np.sqrt(W), cis(np.outer(k, h), H, -1) / np.sqrt(H),
            cis(np.outer(h, k), H, +1) / np.sqrt(H), cis(np.outer(w, l), W, +1) * cl[None, :] / np.sqrt(W)]


def pack_twiddles(H: int, W: int, modes: int) -> np.ndarray:
    """-> the float32 buffer tante_dpot_filter reads: per table a real then an imaginary plane, rows padded to 16, columns to 4."""
    return pack_tables(twiddle_tables(H, W, modes))


def _twiddles(H: int, W: int, modes: int, device) -> torch.Tensor:
    return device_tables(("dpot", H, W) + kept_modes(H, W, modes), lambda: pack_twiddles(H, W, modes),
                         L.lib().tante_dpot_twiddle_floats(H, W, modes), f"twiddle tables for a {H} x {W} grid with {modes} modes", device)


def pack_twiddles_bwd(H: int, W: int, modes: int) -> np.ndarray:
    """-> the float32 buffer of adjoint tables tante_dpot_filter_bwd reads: the conjugate transposes T1^H (W, k2), T2^H (H, k1),
    T3^H (k1, H), T4^H (k2, W) of the same float64 tables, rounded once and padded like pack_twiddles."""
    return pack_tables([t.conj().T for t in twiddle_tables(H, W, modes)])


def _twiddles_bwd(H: int, W: int, modes: int, device) -> torch.Tensor:
    return device_tables(("dpot_bwd", H, W) + kept_modes(H, W, modes), lambda: pack_twiddles_bwd(H, W, modes),
                         L.lib().tante_dpot_twiddle_bwd_floats(H, W, modes),
                         f"adjoint twiddle tables for a {H} x {W} grid with {modes} modes", device)


def groupnorm_bwd_supported_py(B: int, HW: int, C_: int, G: int) -> bool:
    """Python mirror of tante_groupnorm_bwd_supported: the forward's shapes."""
    return groupnorm_supported_py(B, HW, C_, G)


def fold_time_weight(w: torch.Tensor, gamma: Optional[torch.Tensor]) -> torch.Tensor:
    """TimeAggregator's weight (T, C, C) with 'exp_mlp's cos(linspace(0, 1, T)[t] gamma[i]) folded into row i (dpot.py:216-219), in float64,
    rounded to fp32 once.  gamma None ('mlp'): w itself."""
    w64 = w.detach().double()
    if gamma is not None:
        t = torch.linspace(0, 1, w.shape[0]).double().to(w.device)                  # the reference's fp32 linspace
        w64 = w64 * torch.cos(t[:, None] * gamma.detach().double().reshape(1, -1))[:, :, None]
    return w64.float()


def groupnorm(x: torch.Tensor, G: int, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
              out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """tante_groupnorm on channels-last fp32 rows x (B, ..., C): GroupNorm(G, C) over (all tokens x channels in group) per sample."""
    K._dev(x, gamma, beta)
    if x.dtype != torch.float32 or x.dim() < 2:
        raise RuntimeError("GroupNorm takes fp32 channels-last rows (B, ..., C)")
    B, C_ = x.shape[0], x.shape[-1]
    HW = x.numel() // max(B * C_, 1)
    lib = L.lib()
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    work, nbytes = K.workspace(lib.tante_groupnorm_workspace_bytes(B, HW, C_, G), x.device)      # (-1: the call below refuses by name)
    L.check(lib.tante_groupnorm(K._p(x), B, HW, C_, G, float(eps), K._p(gamma), K._p(beta), K._p(y), K._DT[out_dtype], K._p(work), nbytes,
                                K._stream()), "tante_groupnorm")
    return y


def dpot_filter(x: torch.Tensor, residual: Optional[torch.Tensor], w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                modes: int, out: Optional[torch.Tensor] = None, hidden_factor: int = 1) -> torch.Tensor:
    """tante_dpot_filter on x (B, H, W, C) fp32 channels-last: filter(x) (+ residual); w1 / w2 (2, nb, bs, bs), b1 / b2 (2, nb, bs) as the
    state dict holds them."""
    K._dev(x, residual, w1, b1, w2, b2, out)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("the DPOT filter takes fp32 channels-last rows (B, H, W, C)")
    B, H, W, C_ = x.shape
    bs = w1.shape[2]
    if tuple(w1.shape) != (2, C_ // max(bs, 1), bs, bs) or w2.shape != w1.shape or tuple(b1.shape) != (2, C_ // max(bs, 1), bs) or b2.shape != b1.shape:
        raise RuntimeError(f"the DPOT filter's weights {tuple(w1.shape)} / biases {tuple(b1.shape)} do not belong to {C_} channels")
    lib = L.lib()
    if not lib.tante_dpot_filter_supported(B, H, W, C_, bs, modes, hidden_factor):
        # the call itself refuses with the reason; made here without touching the device
        L.check(lib.tante_dpot_filter(None, None, B, H, W, C_, bs, modes, hidden_factor, None, None, None, None, None, None, None, 0, None),
                "tante_dpot_filter")
    if out is None:
        out = torch.empty_like(x)
    work, nbytes = K.workspace(lib.tante_dpot_filter_workspace_bytes(B, H, W, C_, bs, modes), x.device)
    L.check(lib.tante_dpot_filter(K._p(x), K._p(residual), B, H, W, C_, bs, modes, hidden_factor, K._p(_twiddles(H, W, modes, x.device)), K._p(w1),
                                  K._p(b1), K._p(w2), K._p(b2), K._p(out), K._p(work), nbytes, K._stream()), "tante_dpot_filter")
    return out


# ---- training: the mixer, GroupNorm and the time aggregation as autograd nodes ----------------------------------------------------------
def groupnorm_bwd(dy: torch.Tensor, x: torch.Tensor, G: int, gamma: Optional[torch.Tensor], eps: float, dgamma: Optional[torch.Tensor] = None,
                  dbeta: Optional[torch.Tensor] = None, accumulate: bool = False):
    """tante_groupnorm_bwd: dy (fp32 or bf16) and x (fp32), channels-last rows (B, ..., C) -> (dx fp32, dgamma, dbeta); with `accumulate`
    the two parameter gradients are added onto the given buffers.  Without gamma there is no affine and no parameter gradient."""
    K._dev(dy, x, gamma, dgamma, dbeta)
    if x.dtype != torch.float32 or x.dim() < 2 or dy.shape != x.shape or dy.dtype not in K._DT:
        raise RuntimeError("GroupNorm's backward takes fp32 channels-last rows (B, ..., C) and their gradient in fp32 or bf16")
    B, C_ = x.shape[0], x.shape[-1]
    HW = x.numel() // max(B * C_, 1)
    lib = L.lib()
    dx = torch.empty_like(x)
    if gamma is not None and dgamma is None:
        dgamma = torch.empty(C_, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C_, dtype=torch.float32, device=x.device)
        accumulate = False
    work, nbytes = K.workspace(lib.tante_groupnorm_bwd_workspace_bytes(B, HW, C_, G), x.device)  # (-1: the call below refuses by name)
    L.check(lib.tante_groupnorm_bwd(K._p(dy), K._DT[dy.dtype], K._p(x), B, HW, C_, G, float(eps), K._p(gamma), K._p(dx), K._p(dgamma), K._p(dbeta),
                                    int(accumulate), K._p(work), nbytes, K._stream()), "tante_groupnorm_bwd")
    return dx, dgamma, dbeta


def dpot_filter_bwd(dout: torch.Tensor, x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, modes: int, grads=None,
                    accumulate: bool = False):
    """tante_dpot_filter_bwd: -> (dx, dw1, db1, dw2, db2) for dout, x (B, H, W, C) fp32; `grads`: the four buffers to write (or, with
    `accumulate`, to add onto) in the state dict's layout."""
    K._dev(dout, x, w1, b1, w2)
    if x.dtype != torch.float32 or x.dim() != 4 or dout.dtype != torch.float32 or dout.shape != x.shape:
        raise RuntimeError("the DPOT filter's backward takes fp32 channels-last rows (B, H, W, C) and their gradient")
    B, H, W, C_ = x.shape
    bs = w1.shape[2]
    lib = L.lib()
    if not lib.tante_dpot_filter_supported(B, H, W, C_, bs, modes, 1):
        L.check(lib.tante_dpot_filter_bwd(None, None, B, H, W, C_, bs, modes, None, None, None, None, None, None, None, None, None, None, 0, None, 0,
                                          None), "tante_dpot_filter_bwd")
    if grads is None:
        grads = [torch.empty(t.shape, dtype=torch.float32, device=x.device) for t in (w1, b1, w2, b1)]
        accumulate = False
    dx = torch.empty_like(x)
    work, nbytes = K.workspace(lib.tante_dpot_filter_bwd_workspace_bytes(B, H, W, C_, bs, modes), x.device)
    L.check(lib.tante_dpot_filter_bwd(K._p(dout), K._p(x), B, H, W, C_, bs, modes, K._p(_twiddles(H, W, modes, x.device)),
                                      K._p(_twiddles_bwd(H, W, modes, x.device)), K._p(w1), K._p(b1), K._p(w2), K._p(dx), K._p(grads[0]),
                                      K._p(grads[1]), K._p(grads[2]), K._p(grads[3]), int(accumulate), K._p(work), nbytes, K._stream()),
            "tante_dpot_filter_bwd")
    return (dx, *grads)


class DpotFilterFn(Function):
    """filter(x) (+ residual) on x (B, H, W, C) fp32 with the state dict's w1 / w2 (2, nb, bs, bs), b1 / b2 (2, nb, bs), read where the
    parameters lie (no pack).  Forward: the unchanged tante_dpot_filter, bit-identical to inference; x is saved and the backward recomputes
    the spectrum and the pre-activation from it.  Backward: tante_dpot_filter_bwd; the weight gradients go straight into the parameters'
    gradient slots where all four exist (FlatAdamW), the residual's gradient is dout itself."""

    @staticmethod
    def forward(ctx, x, residual, w1, b1, w2, b2, modes):
        x = x.contiguous()
        residual = None if residual is None else residual.contiguous()
        out = dpot_filter(x, residual, w1.detach(), b1.detach(), w2.detach(), b2.detach(), modes)
        ctx.save_for_backward(x)
        ctx.params, ctx.modes, ctx.has_res = (w1, b1, w2, b2), int(modes), residual is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        from .autograd import grad_slots
        (x,) = ctx.saved_tensors
        w1, b1, w2, _ = ctx.params
        dout = dout.contiguous()
        slots = grad_slots(ctx, ctx.params, 2)
        res = dpot_filter_bwd(dout, x, w1.detach(), b1.detach(), w2.detach(), ctx.modes, slots, slots is not None)
        gs = [None] * 4 if slots is not None else [g if ctx.needs_input_grad[2 + i] else None for i, g in enumerate(res[1:])]
        return (res[0], dout if ctx.has_res else None, *gs, None)


class GroupNormFn(Function):
    """GroupNorm(G, C) on channels-last fp32 rows x (B, ..., C), output in out_dtype: tante_groupnorm forward, tante_groupnorm_bwd backward
    (dy in fp32 or bf16, dx fp32); the affine's gradients go into the parameters' gradient slots where both exist."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, out_dtype):
        x = x.contiguous()
        y = groupnorm(x, G, None if gamma is None else gamma.detach(), None if beta is None else beta.detach(), eps, out_dtype)
        ctx.save_for_backward(x)
        ctx.params, ctx.G, ctx.eps = (gamma, beta), int(G), float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .autograd import grad_slots
        (x,) = ctx.saved_tensors
        gamma, beta = ctx.params
        dy = dy.contiguous()
        if gamma is None:
            return groupnorm_bwd(dy, x, ctx.G, None, ctx.eps)[0], None, None, None, None, None
        slots = grad_slots(ctx, ctx.params, 1) if beta is not None else None
        if slots is not None:
            dx, _, _ = groupnorm_bwd(dy, x, ctx.G, gamma.detach(), ctx.eps, slots[0], slots[1], True)
            return dx, None, None, None, None, None
        dx, dg, db = groupnorm_bwd(dy, x, ctx.G, gamma.detach(), ctx.eps)
        return dx, (dg if ctx.needs_input_grad[1] else None), (db if beta is not None and ctx.needs_input_grad[2] else None), None, None, None


class TimeAggFn(Function):
    """TimeAggregator.run on the strided ((b t) HW, C) rows.  Forward: the module's own per-t K-chunk GEMMs on the folded fp32 weights of
    its pack cache (the values inference uses; the cache is keyed on the weight epoch and the parameters' versions, so the BPTT calls of a
    step share one fold and an optimiser step rebuilds it).  Backward: the row gradient as per-t GEMMs against the same fold, the folded
    weight's gradient through autograd.wgrad on the strided rows of every t, and -- parameter-sized, in float64 -- the chain rule of the
    'exp_mlp' fold w[t, i, :] cos(t_t gamma_i) to w and gamma."""

    @staticmethod
    def forward(ctx, rows, w, gamma, agg, B, T, HW, compute):
        rows = rows.contiguous()
        out = agg.run(rows, B, T, HW, compute)
        ctx.save_for_backward(rows)
        ctx.agg, ctx.geo, ctx.params = agg, (B, T, HW, compute), (w, gamma)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .autograd import _rm_linear, wgrad
        (rows,) = ctx.saved_tensors
        agg = ctx.agg
        B, T, HW, compute = ctx.geo
        w, gamma = ctx.params
        C_ = agg.out_channels
        dout = dout.contiguous()
        M = B * HW
        drows = dw = dgamma = None
        if ctx.needs_input_grad[0]:
            parts = [S.linear_chunks(dout, chunks) for chunks in agg._packed_bwd(compute)]        # dout wf[t]^T, (b HW, C) each
            drows = torch.stack([p.view(B, HW, C_) for p in parts], dim=1).view(B * T * HW, C_)   # layout: the rows of (b, t)
        if ctx.needs_input_grad[1] or (gamma is not None and ctx.needs_input_grad[2]):
            # dwf[t][i][j] = sum over (b, HW) of rows_t[., i] dout[., j]: the gradient of the FOLDED weight
            dwf = torch.stack([wgrad(_rm_linear(rows, HW, T * HW * C_, C_, t * HW * C_, cols=C_), _rm_linear(dout), M, C_, C_, (C_, C_), compute,
                                     device=dout.device) for t in range(T)]).double()
            if gamma is None:
                dw = dwf.float()
            else:
                tt = torch.linspace(0, 1, T).double().to(dout.device)[:, None]                    # the reference's fp32 linspace
                ang = tt * gamma.detach().double().reshape(1, -1)
                dw = (dwf * torch.cos(ang)[:, :, None]).float()
                dgamma = ((dwf * w.detach().double()).sum(dim=2) * (-torch.sin(ang) * tt)).sum(dim=0).reshape(gamma.shape).float()
        return drows, dw, dgamma, None, None, None, None, None


def _conv1x1(conv: nn.Conv2d) -> torch.Tensor:
    """The (out, in) matrix of a 1 x 1 convolution: a view of the parameter."""
    return conv.weight.view(conv.weight.shape[0], -1)


def block_train(blk: "Block", x: torch.Tensor, compute: int) -> torch.Tensor:
    """Block.run as a graph of training nodes: x (B, H, W, C) fp32 channels-last -> block(x)."""
    from .autograd import ActFn, LinearFn
    B, H, W, C_ = x.shape
    M = B * H * W
    adt = K.act_torch_dtype(compute)
    f, fc1, fc2 = blk.filter, blk.mlp[0], blk.mlp[2]
    n1 = GroupNormFn.apply(x, blk.norm1.weight, blk.norm1.bias, GROUPS, blk.norm1.eps, torch.float32)
    x1 = DpotFilterFn.apply(n1, x if blk.double_skip else None, f.w1, f.b1, f.w2, f.b2, f.modes)
    skip = x1 if blk.double_skip else x
    n2 = GroupNormFn.apply(x1, blk.norm2.weight, blk.norm2.bias, GROUPS, blk.norm2.eps, adt)
    h = ActFn.apply(LinearFn.apply(n2.view(M, C_), _conv1x1(fc1), fc1.bias, None, compute, adt), L.ACT_GELU_ERF, adt)
    return LinearFn.apply(h, _conv1x1(fc2), fc2.bias, skip.reshape(M, C_), compute, torch.float32).view(B, H, W, C_)


def patch_embed_train(pe: "PatchEmbed", img: torch.Tensor, compute: int, residual: Optional[torch.Tensor]) -> torch.Tensor:
    """PatchEmbed.run as training nodes: img (n, h, w, cin) fp32 channels-last -> rows (n H' W', out_dim) fp32 (+ residual rows)."""
    from .autograd import ActFn, Im2colFn, LinearFn
    n, h, w, cin = img.shape
    p = pe.patch_size[0]
    c0, c2 = pe.proj[0], pe.proj[2]
    adt = K.act_torch_dtype(compute)
    cols = Im2colFn.apply(img, n, cin, h, w, p, p, 0, adt)                                    # columns (kh, kw, channel)
    w0 = c0.weight.permute(0, 2, 3, 1).reshape(c0.weight.shape[0], -1).contiguous()           # the same order, a parameter-sized re-layout
    h1 = ActFn.apply(LinearFn.apply(cols, w0, c0.bias, None, compute, adt), L.ACT_GELU_ERF, adt)
    return LinearFn.apply(h1, _conv1x1(c2), c2.bias, residual, compute, torch.float32)


def dpot_train_forward(model: "DPOT", x: torch.Tensor, compute: int) -> torch.Tensor:
    """DPOT.forward with an autograd graph: x (b, t, c, h, w) -> (b, out_timesteps, c, h, w) fp32.  torch allocates, re-lays out (the
    channels-last image with the constant coordinate channels beside the fields, the stacked per-t row gradients, the output's
    channels-first view) and does parameter-sized work; every activation-sized operation is a HIP node."""
    from .autograd import ActFn, LinearFn, PosRowsFn
    b, T, c, h, w = x.shape
    p, C_ = model.patch_size, model.embed_dim
    Hp, Wp = model.latent_size
    HW = Hp * Wp
    adt = K.act_torch_dtype(compute)
    # the (b T, h, w, c + 3) image: the gradient reaches x through the concatenation (layout only; the coordinates are constants)
    grid = model.get_grid_3d(T, x.device).permute(0, 2, 3, 1)
    img = torch.cat([x.to(torch.float32).permute(0, 1, 3, 4, 2), grid[None].expand(b, -1, -1, -1, -1)], dim=4).reshape(b * T, h, w, c + 3)
    pos = PosRowsFn.apply(model.pos_embed.permute(0, 2, 3, 1), b * T)                          # channels first -> rows (x, y, C) per image
    rows = patch_embed_train(model.patch_embed, img, compute, pos)                             # ((b t) x y, C): x + pos_embed
    agg = model.time_agg_layer
    y = TimeAggFn.apply(rows, agg.w, agg.gamma if agg.type == "exp_mlp" else None, agg, b, T, HW, compute).view(b, Hp, Wp, C_)
    for blk in model.blocks:
        y = block_train(blk, y, compute)
    d, a, z = model.out_layer[0], model.out_layer[2], model.out_layer[4]
    od = model.out_layer_dim
    pre = S.deconv_nhwc_train(y.view(b * HW, C_), d.weight, d.bias, b, Hp, Wp, p, compute, adt)
    img2 = ActFn.apply(pre, L.ACT_GELU_ERF, adt)
    px = ActFn.apply(LinearFn.apply(img2.view(b * h * w, od), _conv1x1(a), a.bias, None, compute, adt), L.ACT_GELU_ERF, adt)
    if od > S.KMAX:
        raise NotImplementedError("out_layer_dim above 512 is out of scope: the last pixel-row linear writes channels first from one GEMM")
    out = LinearFn.apply(px, _conv1x1(z), z.bias, None, compute, torch.float32)               # (b h w, (t c))
    return out.view(b, h, w, model.out_timesteps, model.out_channels).permute(0, 3, 4, 1, 2)


# ---- the reference's modules -------------------------------------------------------------------------------------------------------
WHY_INFERENCE_ONLY = "the mixer's and GroupNorm's backward are kernels of their own that are not built"


def _refuse(module: nn.Module):
    inference_only(module, "DPOT", WHY_INFERENCE_ONLY)


def _gelu_only(act: str):
    if act != "gelu":
        raise NotImplementedError(f"act = {act!r} is out of scope: the HIP path evaluates the erf GELU of the reference's config (act 'gelu')")


class AFNO2D(Trainable, nn.Module):
    """The truncated-mode Fourier mixer  (dpot.py:21-102): tante_dpot_filter."""

    def __init__(self, width=32, num_blocks=8, channel_first=False, sparsity_threshold=0.01, modes=32, hard_thresholding_fraction=1,
                 hidden_size_factor=1, act="gelu"):
        super().__init__()
        assert width % num_blocks == 0, f"hidden_size {width} should be divisble by num_blocks {num_blocks}"
        _gelu_only(act)
        if hidden_size_factor != 1:
            raise NotImplementedError(f"hidden_size_factor = {hidden_size_factor} is out of scope: tante_dpot_filter serves square blocks "
                                      "(hidden_size_factor 1, the value the reference's Block passes)")
        self.hidden_size = width
        self.sparsity_threshold = sparsity_threshold
        self.num_blocks = num_blocks
        self.block_size = self.hidden_size // self.num_blocks
        self.channel_first = channel_first
        self.modes = modes
        self.hidden_size_factor = hidden_size_factor
        self.scale = 1 / (self.block_size * self.block_size * self.hidden_size_factor)
        self.act = nn.GELU()
        bs = self.block_size
        self.w1 = nn.Parameter(self.scale * torch.rand(2, num_blocks, bs, bs * hidden_size_factor))
        self.b1 = nn.Parameter(self.scale * torch.rand(2, num_blocks, bs * hidden_size_factor))
        self.w2 = nn.Parameter(self.scale * torch.rand(2, num_blocks, bs * hidden_size_factor, bs))
        self.b2 = nn.Parameter(self.scale * torch.rand(2, num_blocks, bs))

    def run(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """x (B, H, W, C) fp32 channels-last -> filter(x) (+ residual); the weights are read where the parameters lie."""
        return dpot_filter(x, residual, self.w1.detach(), self.b1.detach(), self.w2.detach(), self.b2.detach(), self.modes,
                           hidden_factor=self.hidden_size_factor)

    def forward(self, x: torch.Tensor, spatial_size=None) -> torch.Tensor:
        """(B, H, W, C), or (B, C, H, W) with channel_first, -> the same layout  (dpot.py:47-102).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        if x.dim() != 4:
            raise NotImplementedError("the DPOT mixer is two-dimensional here: n_spatial_dims = 3 is out of scope")
        gpu_only(x, "DPOT")
        if train:
            xl = x.to(torch.float32).permute(0, 2, 3, 1) if self.channel_first else x.to(torch.float32)
            y = DpotFilterFn.apply(xl, None, self.w1, self.b1, self.w2, self.b2, self.modes)
            return (y.permute(0, 3, 1, 2) if self.channel_first else y).to(x.dtype)
        xl = x.detach().to(torch.float32)
        if self.channel_first:
            xl = xl.permute(0, 2, 3, 1)
        y = self.run(xl.contiguous(), None)
        if self.channel_first:
            y = y.permute(0, 3, 1, 2)
        return y.to(x.dtype)


class Mlp(nn.Module):
    """fc2(gelu_erf(fc1(x)))  (dpot.py:105-118); no module of the reference's DPOT uses it."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act="gelu", drop=0.0):
        super().__init__()
        _gelu_only(act)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, out_features)


class Block(Trainable, nn.Module):
    """n1 = GN1(x); f = filter(n1) (+ x under double_skip); y = mlp(GN2(f)) + (f if double_skip else x)   (dpot.py:121-172)."""

    def __init__(self, mixing_type="afno", double_skip=True, width=32, n_blocks=4, mlp_ratio=1.0, channel_first=True, modes=32, drop=0.0,
                 drop_path=0.0, act="gelu", h=14, w=8):
        super().__init__()
        _gelu_only(act)
        if mixing_type != "afno":
            raise NotImplementedError(f"mixing_type = {mixing_type!r} is out of scope: the reference's Block builds a filter for 'afno' only")
        self.norm1 = torch.nn.GroupNorm(GROUPS, width)
        self.width = width
        self.modes = modes
        self.act = nn.GELU()
        self.filter = AFNO2D(width=width, num_blocks=n_blocks, sparsity_threshold=0.01, channel_first=channel_first, modes=modes,
                             hard_thresholding_fraction=1, hidden_size_factor=1, act=act)
        self.norm2 = torch.nn.GroupNorm(GROUPS, width)
        mlp_hidden_dim = int(width * mlp_ratio)
        self.mlp = nn.Sequential(nn.Conv2d(in_channels=width, out_channels=mlp_hidden_dim, kernel_size=1, stride=1), self.act,
                                 nn.Conv2d(in_channels=mlp_hidden_dim, out_channels=width, kernel_size=1, stride=1))
        self.double_skip = double_skip
        self._cache = _PackCache()

    def _packed(self, compute: int):
        fc1, fc2 = self.mlp[0], self.mlp[2]
        return self._cache.get(compute, [fc1.weight, fc1.bias, fc2.weight, fc2.bias], lambda: (
            S.pack_linear_chunks(fc1.weight.detach().reshape(fc1.weight.shape[0], -1), fc1.bias, compute),
            S.pack_linear_chunks(fc2.weight.detach().reshape(fc2.weight.shape[0], -1), fc2.bias, compute)))

    def run(self, x: torch.Tensor, compute: int) -> torch.Tensor:
        """x (B, H, W, C) fp32 channels-last -> block(x), same shape."""
        B, H, W, C_ = x.shape
        M = B * H * W
        fc1, fc2 = self._packed(compute)
        n1 = groupnorm(x, GROUPS, self.norm1.weight.detach(), self.norm1.bias.detach(), self.norm1.eps)
        if self.double_skip:
            f = self.filter.run(n1, x)               # the filter's store epilogue adds the first skip
            skip = f
        else:
            f = self.filter.run(n1, None)
            skip = x
        n2 = groupnorm(f, GROUPS, self.norm2.weight.detach(), self.norm2.bias.detach(), self.norm2.eps, K.act_torch_dtype(compute))
        h = S.linear_chunks(n2.view(M, C_), fc1, K.act_torch_dtype(compute), L.ACT_GELU_ERF)
        return S.linear_chunks(h, fc2, residual=skip.view(M, C_)).view(B, H, W, C_)      # the skip rides the residual operand

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, C, H, W) -> (B, C, H, W), as the reference's Block takes its images (GroupNorm and the 1 x 1 convs act on dim 1)."""
        train = wants_graph(self, x, _refuse)
        if x.dim() != 4:
            raise NotImplementedError("the DPOT block is two-dimensional here: n_spatial_dims = 3 is out of scope")
        if not self.filter.channel_first:
            raise NotImplementedError("Block(channel_first=False) hands its channel-first image to a channels-last filter in the reference; "
                                      "that mixes channels with rows and is not reproduced")
        gpu_only(x, "DPOT")
        if train:
            return block_train(self, x.to(torch.float32).permute(0, 2, 3, 1), resolve_compute(None)).permute(0, 3, 1, 2).to(x.dtype)
        y = self.run(x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous(), resolve_compute(None))
        return y.permute(0, 3, 1, 2).to(x.dtype)


class PatchEmbed(Trainable, nn.Module):
    """Conv(p x p / p) -> GELU -> Conv(1 x 1)  (dpot.py:175-197): tante_im2col + two GEMMs, channels-last rows out."""

    def __init__(self, img_size, patch_size=16, in_chans=3, embed_dim=768, out_dim=128, act="gelu"):
        super().__init__()
        _gelu_only(act)
        patch_size = (patch_size, patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
        self.out_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.out_dim = out_dim
        self.act = nn.GELU()
        self.proj = nn.Sequential(nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size), self.act,
                                  nn.Conv2d(embed_dim, out_dim, kernel_size=1, stride=1))
        self._cache = _PackCache()

    def _packed(self, compute: int):
        c0, c2 = self.proj[0], self.proj[2]
        return self._cache.get(compute, [c0.weight, c0.bias, c2.weight, c2.bias], lambda: (
            S.pack_linear_chunks(c0.weight.detach().reshape(c0.weight.shape[0], -1), c0.bias, compute),
            S.pack_linear_chunks(c2.weight.detach().reshape(c2.weight.shape[0], -1), c2.bias, compute)))

    def run(self, x: torch.Tensor, compute: int, residual: Optional[torch.Tensor]) -> torch.Tensor:
        """x (n, C, H, W) fp32 contiguous -> rows (n H' W', out_dim) fp32 (+ residual rows)."""
        n, cin, h, w = x.shape
        p = self.patch_size[0]
        c0, c2 = self._packed(compute)
        adt = K.act_torch_dtype(compute)
        cols = K.im2col(x, True, n, cin, h, w, p, p, p, p, 0, 0, 0, adt)
        h1 = S.linear_chunks(cols, c0, adt, L.ACT_GELU_ERF)
        return S.linear_chunks(h1, c2, residual=residual)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, C, H, W) -> (B, out_dim, H', W')  (dpot.py:193-197).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        gpu_only(x, "DPOT")
        B, C_, H, W = x.shape
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        if train:
            y = patch_embed_train(self, x.to(torch.float32).permute(0, 2, 3, 1), resolve_compute(None), None)
            return y.view(B, self.out_size[0], self.out_size[1], self.out_dim).permute(0, 3, 1, 2).to(x.dtype)
        y = self.run(x.detach().to(torch.float32).contiguous(), resolve_compute(None), None)
        return y.view(B, self.out_size[0], self.out_size[1], self.out_dim).permute(0, 3, 1, 2).to(x.dtype)


class TimeAggregator(Trainable, nn.Module):
    """out[..., j] = sum_t sum_i w[t, i, j] x[..., t, i] (cos(t gamma_i) for 'exp_mlp')  (dpot.py:200-221): one K = T C GEMM."""

    def __init__(self, n_channels, n_timesteps, out_channels, type="mlp"):
        super().__init__()
        self.n_channels = n_channels
        self.n_timesteps = n_timesteps
        self.out_channels = out_channels
        self.type = type
        if type not in ("mlp", "exp_mlp"):
            raise ValueError(f"time_agg must be 'mlp' or 'exp_mlp', got {type!r}")
        self.w = nn.Parameter(1 / (n_timesteps * out_channels ** 0.5) * torch.randn(n_timesteps, out_channels, out_channels))
        if type == "exp_mlp":
            self.gamma = nn.Parameter(2 ** torch.linspace(-10, 10, out_channels).unsqueeze(0))
        self._cache = _PackCache()

    def _packed(self, compute: int):
        gamma = self.gamma if self.type == "exp_mlp" else None
        params = [self.w] + ([gamma] if gamma is not None else [])

        def build():
            wf = fold_time_weight(self.w, gamma)                           # (T, C_in, C_out)
            return [S.pack_linear_chunks(wf[t].t().contiguous(), None, compute) for t in range(wf.shape[0])]
        return self._cache.get(compute, params, build)

    def _packed_bwd(self, compute: int):
        """Per t the K-chunks of the row gradient's GEMM dout wf[t]^T, from the same fold; an entry of the same cache, so the weight epoch
        and the parameters' versions rebuild it with the forward's."""
        gamma = self.gamma if self.type == "exp_mlp" else None
        params = [self.w] + ([gamma] if gamma is not None else [])

        def build():
            wf = fold_time_weight(self.w, gamma)                           # (T, C_in, C_out)
            return [S.pack_linear_chunks(wf[t].contiguous(), None, compute) for t in range(wf.shape[0])]
        return self._cache.get(("bwd", compute), params, build)

    def run(self, rows: torch.Tensor, B: int, T: int, HW: int, compute: int) -> torch.Tensor:
        """rows ((b t) HW, C) fp32 -> (b HW, C) fp32: the K-chunks of every t read their rows in place."""
        C_ = self.out_channels
        if T != self.n_timesteps:
            raise ValueError(f"the time aggregator holds {self.n_timesteps} steps, the input has {T}")
        out = torch.empty(B * HW, C_, dtype=torch.float32, device=rows.device)
        first = True
        for t, chunks in enumerate(self._packed(compute)):
            k0 = 0
            for pw in chunks:
                K.linear(rows, pw, out, M=B * HW, a_n0=HW, a_s1=T * HW * C_, a_s0=C_, a_off=t * HW * C_ + k0, residual=None if first else out)
                first = False
                k0 += pw.K
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, X, Y, T, C) -> (B, X, Y, C)  (dpot.py:213-221).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        gpu_only(x, "DPOT")
        B, X, Y, T, C_ = x.shape
        if train:
            rows = x.to(torch.float32).permute(0, 3, 1, 2, 4).reshape(B * T * X * Y, C_)
            y = TimeAggFn.apply(rows, self.w, self.gamma if self.type == "exp_mlp" else None, self, B, T, X * Y, resolve_compute(None))
            return y.view(B, X, Y, C_).to(x.dtype)
        rows = x.detach().to(torch.float32).permute(0, 3, 1, 2, 4).contiguous().view(B * T * X * Y, C_)
        return self.run(rows, B, T, X * Y, resolve_compute(None)).view(B, X, Y, C_).to(x.dtype)


class DPOT(Trainable, ComputeSwitch, nn.Module):
    """models/dpot.py:223-350 -- same constructor, attributes, parameters and forward contract."""

    def __init__(self, in_T: int, dset_metadata, patch_size=16, mixing_type="afno", out_timesteps=1, n_blocks=4, embed_dim=768,
                 out_layer_dim=32, depth=12, modes=32, mlp_ratio=1.0, n_cls=12, act="gelu", time_agg="exp_mlp"):
        super().__init__()
        img_size = tuple(dset_metadata.spatial_resolution)
        n_channel = dset_metadata.n_fields
        if getattr(dset_metadata, "n_spatial_dims", 2) == 3 or len(img_size) == 3:
            raise NotImplementedError("DPOT with n_spatial_dims = 3 is out of scope: the HIP mixer and the reference's model are "
                                      "two-dimensional")
        if len(img_size) != 2:
            raise ValueError(f"spatial_resolution must have two entries, got {img_size}")
        _gelu_only(act)
        if mixing_type != "afno":
            raise NotImplementedError(f"mixing_type = {mixing_type!r} is out of scope: the reference's Block builds a filter for 'afno' only")
        self.in_channels = n_channel
        self.out_channels = n_channel
        self.in_timesteps = in_T
        self.out_timesteps = out_timesteps
        self.n_blocks = n_blocks
        self.modes = modes
        self.num_features = self.embed_dim = embed_dim
        self.mlp_ratio = mlp_ratio
        self.act = nn.GELU()
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=self.in_channels + 3,
                                      embed_dim=self.out_channels * patch_size + 3, out_dim=embed_dim, act=act)
        self.latent_size = self.patch_embed.out_size
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, self.patch_embed.out_size[0], self.patch_embed.out_size[1]))
        self.time_agg = time_agg
        self.n_cls = n_cls
        h, w = img_size
        self.blocks = nn.ModuleList([Block(mixing_type=mixing_type, modes=modes, width=embed_dim, mlp_ratio=mlp_ratio, channel_first=True,
                                           n_blocks=n_blocks, double_skip=False, h=h, w=w, act=act) for _ in range(depth)])
        # held for the state dict, never evaluated: the reference computes cls_pred and discards it (dpot.py:343-344)
        self.cls_head = nn.Sequential(nn.Linear(embed_dim, embed_dim), self.act, nn.Linear(embed_dim, embed_dim), self.act,
                                      nn.Linear(embed_dim, n_cls))
        self.time_agg_layer = TimeAggregator(self.in_channels, in_T, embed_dim, time_agg)
        self.out_layer = nn.Sequential(
            nn.ConvTranspose2d(in_channels=embed_dim, out_channels=out_layer_dim, kernel_size=patch_size, stride=patch_size), self.act,
            nn.Conv2d(in_channels=out_layer_dim, out_channels=out_layer_dim, kernel_size=1, stride=1), self.act,
            nn.Conv2d(in_channels=out_layer_dim, out_channels=self.out_channels * self.out_timesteps, kernel_size=1, stride=1))
        torch.nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.mixing_type = mixing_type
        self.patch_size, self.img_size, self.out_layer_dim = patch_size, img_size, out_layer_dim
        self.output_length = out_timesteps
        self._cache = _PackCache()
        self._pos = _PackCache()
        self._stage = {}

    def trained_parameters(self):
        """Every parameter except cls_head.*: the reference computes cls_pred and discards it (dpot.py:343-344), so those weights never
        receive a gradient and torch's AdamW never touches them.  FlatAdamW decays everything it is given: pass it THIS list, not
        parameters()."""
        return [p for n, p in self.named_parameters() if not n.startswith("cls_head.")]

    def get_grid_3d(self, T: int, device) -> torch.Tensor:
        """The three coordinate channels (T, 3, h, w) fp32: linspace(0, 1, n) over x, y and t  (dpot.py:309-319)."""
        h, w = self.img_size
        gx = torch.tensor(np.linspace(0, 1, h), dtype=torch.float).view(1, h, 1).expand(T, h, w)
        gy = torch.tensor(np.linspace(0, 1, w), dtype=torch.float).view(1, 1, w).expand(T, h, w)
        gt = torch.tensor(np.linspace(0, 1, T), dtype=torch.float).view(T, 1, 1).expand(T, h, w)
        return torch.stack([gx, gy, gt], dim=1).to(device)

    def _staging(self, b: int, T: int, device) -> torch.Tensor:
        """The (b T, c + 3, h, w) image the patch embed reads: the coordinate channels are written once, the fields per call."""
        key = (b, T, str(device))
        st = self._stage.get(key)
        if st is None:
            h, w = self.img_size
            st = torch.empty(b, T, self.in_channels + 3, h, w, dtype=torch.float32, device=device)
            st[:, :, self.in_channels:] = self.get_grid_3d(T, device)
            self._stage = {key: st}
        return st

    def _packed(self, compute: int):
        d, a, z = self.out_layer[0], self.out_layer[2], self.out_layer[4]
        return self._cache.get(compute, [d.weight, d.bias, a.weight, a.bias, z.weight, z.bias], lambda: (
            S.pack_deconv_nhwc(d.weight, d.bias, self.patch_size, compute),
            S.pack_linear_chunks(a.weight.detach().reshape(a.weight.shape[0], -1), a.bias, compute),
            S.pack_linear_chunks(z.weight.detach().reshape(z.weight.shape[0], -1), z.bias, compute)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, out_timesteps, c, h, w)   (dpot.py:323-350).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        if x.dim() != 5 or x.shape[1] != self.in_timesteps or x.shape[2] != self.in_channels:
            raise ValueError(f"expected (B, {self.in_timesteps}, {self.in_channels}, H, W), got {tuple(x.shape)}")
        gpu_only(x, "DPOT")
        b, T, c, h, w = x.shape
        if (h, w) != tuple(self.img_size):
            raise ValueError(f"Input image size ({h}*{w}) doesn't match model ({self.img_size[0]}*{self.img_size[1]}).")
        compute = resolve_compute(self.compute)
        if train:
            return dpot_train_forward(self, x, compute)
        adt = K.act_torch_dtype(compute)
        p, C_ = self.patch_size, self.embed_dim
        Hp, Wp = self.latent_size
        HW = Hp * Wp
        stage = self._staging(b, T, x.device)
        stage[:, :, :c].copy_(x.detach())                                        # the one strided copy: the fields beside the cached coordinates
        pos = self._pos.get((b, T), [self.pos_embed], lambda: self.pos_embed.detach()[0].permute(1, 2, 0).reshape(1, HW, C_)
                            .expand(b * T, -1, -1).reshape(b * T * HW, C_).contiguous())
        rows = self.patch_embed.run(stage.view(b * T, c + 3, h, w), compute, pos)   # ((b t) x y, C): x + pos_embed
        y = self.time_agg_layer.run(rows, b, T, HW, compute).view(b, Hp, Wp, C_)
        for blk in self.blocks:
            y = blk.run(y, compute)
        dec, mid, last = self._packed(compute)
        od = self.out_layer_dim
        img = S.deconv_nhwc(y.view(b * HW, C_), dec, self.out_layer[0].bias.detach(), b, Hp, Wp, p, od, adt, L.ACT_GELU_ERF)
        px = S.linear_chunks(img.view(b * h * w, od), mid, adt, L.ACT_GELU_ERF)
        if len(last) != 1:
            raise NotImplementedError("out_layer_dim above 512 is out of scope: the last pixel-row linear writes channels first from one GEMM")
        nout = self.out_channels * self.out_timesteps
        out = torch.empty(b, nout, h, w, dtype=torch.float32, device=x.device)
        K.deconv(px, last[0], out, n_img=b, Hi=h, Wi=w, P=1, Cout=nout, nchw_out=True, act=L.ACT_NONE)     # (b, (t c), h, w) IS b t c h w
        return out.view(b, self.out_timesteps, self.out_channels, h, w)
