"""UNetConvNext baseline on the HIP kernels  (reference models/unet_convnext.py, configs/unet_convnext.yaml: the Well benchmark's CNN).

Same constructor arguments, attributes, module tree, `state_dict` keys / shapes and forward contract (`b t c h w -> b 1 c h w`) as the
reference's models.UNetConvNext.  The model is channels-last inside, (n, H, W, C) fp32, the residual stream fp32, and every arithmetic
step is a C-ABI call of libtante_hip:
  in_proj / out_proj  tante_conv3x3, fp32 in both modes: the batch is read as it arrives (b t c h w contiguous IS b (t c) h w) and
                      written channels-last; out_proj reads channels-last and writes b 1 c h w.  Past Cin 128 / Cout 64: tante_im2col +
                      tante_gemm.
  Block               ONE launch, tante_convnext_block: depthwise 7 x 7 + bias, LayerNorm over channels, pwconv1 + erf GELU, pwconv2,
                      layer scale, skip; out of place (the stage ping-pongs two buffers).  The norm's affine is folded into pwconv1 and
                      gamma into pwconv2 in float64 at pack time.  The kernel serves C <= 256 and is the default up to C = 32, where it
                      was measured faster; wider blocks, and every block with TANTE_CONVNEXT_FUSED = 0, take the modular route:
                      tante_dwconv_ln -> tante_gemm (GELU epilogue) -> tante_gemm (skip as the residual operand).
  Downsample          tante_l2norm_rows -> tante_im2col (2 x 2 / 2) -> tante_gemm, the norm's weight folded into the columns
  Upsample            tante_l2norm_rows -> the 2 x 2 / 2 transposed convolution as a scatter GEMM (tap GEMM + tante_col2im_nhwc past 512
                      input channels), the norm's weight folded into the rows
  skip_proj           two GEMMs that accumulate through the residual operand, W[:, :C] x then + W[:, C:] skip: the concatenated tensor
                      is never written
torch allocates and reshapes.

Restated as the reference has them: the channels_first "LayerNorm" of the resamples is F.normalize(x, p=2, dim=1, eps) * weight
(unet_convnext.py:69) and its `bias` is held for the state dict and NEVER applied; skips[0] (the full-resolution in_proj output) is
stored and never read (unet_convnext.py:274, 279: skips[-j] for j >= 1); `n_spatial_dims` comes from the metadata, not from the argument
(unet_convnext.py:219); `gradient_checkpointing` is an attribute without effect here.

In bf16 mode bf16 is the GEMM operand type of the groups in BF16_SITES; the depthwise sum, every norm, the skip and the two edge
convolutions stay fp32.

Inference is the default: a model whose parameters require a gradient refuses under grad (and in train()), as it always did.  Training is
opt-in through `model.set_trainable()` (also on Stage, Block, Upsample, Downsample and the channels-last LayerNorm; it propagates to the
children).  An opted-in model called under grad takes convnext_train_forward: the same arithmetic as a graph of the training nodes of
tante_amd/autograd.py (Im2colFn, LinearFn with K chunks, ActFn, DeconvFn / Col2imFn) with two nodes of this module: DwConvLnFn (forward
the unchanged tante_dwconv_ln, bit-identical to inference; backward tante_dwconv_ln_bwd: the forward's two tile stages again from x, the
three-term LayerNorm gradient, the flipped-tap correlation and the 49 tap sums per channel) and L2NormRowsFn (tante_l2norm_rows_bwd).
Every training block is the MODULAR composition with the norm's affine applied by the kernel; the fused one-launch block stays inference
only.  gamma and the channels-first norm's weight are folded as parameter-sized differentiable torch (float64, rounded once).  Every sum
of the backward kernels has a fixed order and there are no atomics, so two runs give the same bits.  The input receives a gradient too,
so `rollout_model` back-propagates through its re-fed frames and `train.train_step` works with `FlatAdamW(model.trained_parameters())`
-- every parameter except *.resample.block.0.bias, which never receives a gradient.  Under no_grad an opted-in model takes the unchanged
inference path; train() changes nothing further (drop_path is 0).  3-D metadata, drop_path > 0, a wrong t * c and H or W not divisible by
2 ** stages raise with or without the opt-in; there is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L
from . import kernels as K
from . import options as _O
from . import stages as S
from .attn_backbone import _PackCache, resolve_compute
from .model_shell import ComputeSwitch, Trainable, gpu_only, inference_only, site, to_nchw, to_nhwc, wants_graph

FUSED_MAX_C = 256      # channels tante_convnext_block serves
FUSED_DEFAULT_MAX_C = 32   # ... and the widest block it is the DEFAULT for: on the config's pyramid (token count x C^2 constant) the one launch
#                            is 1.4 - 2.4 x faster than the modular route at C = 15 and 30 and slower from C = 60 on, where a level has too
#                            few 128-token tiles to fill the chip (DESIGN 4.8 has the table); Block.run(fused=True) forces it at any C <= 256
DWLN_MAX_C = 1024      # channels tante_dwconv_ln serves
CONV3_MAX_CIN, CONV3_MAX_COUT = 128, 64
BF16_SITES = ("block", "resample", "skip")   # the GEMM groups that take bf16 operands in bf16 mode (DESIGN 4.8 has the per-group figures)

# True: blocks up to FUSED_DEFAULT_MAX_C channels run as one launch; False: every block runs the modular route (tante_dwconv_ln + two
# tante_gemm), the A/B and parity partner of the fused launch
FUSED = _O.register("TANTE_CONVNEXT_FUSED", True, __name__, "FUSED")


# ---- host side of the kernels: the predicates' mirrors, the wrappers, the folds -----------------------------------------------------------
def _tiles_ok(n_img: int, H: int, W: int, th: int, tw: int) -> bool:
    tiles = ((W + tw - 1) // tw) * ((H + th - 1) // th)
    return tiles <= 2 ** 31 - 1 and n_img * tiles <= 2 ** 31 - 1


def convnext_block_supported_py(n_img: int, H: int, W: int, C_: int) -> bool:
    """Python mirror of tante_convnext_block_supported."""
    return 1 <= C_ <= FUSED_MAX_C and H >= 1 and W >= 1 and n_img >= 0 and _tiles_ok(n_img, H, W, 8, 16)


def dwconv_ln_supported_py(n_img: int, H: int, W: int, C_: int) -> bool:
    """Python mirror of tante_dwconv_ln_supported."""
    return 1 <= C_ <= DWLN_MAX_C and H >= 1 and W >= 1 and n_img >= 0 and _tiles_ok(n_img, H, W, 8 if C_ <= 512 else 4, 8)


def l2norm_rows_supported_py(M: int, C_: int) -> bool:
    """Python mirror of tante_l2norm_rows_supported."""
    return 1 <= C_ <= (1 << 24) and 0 <= M and (M + 3) // 4 <= 2 ** 31 - 1


def conv3x3_supported_py(n_img: int, Cin: int, Cout: int, H: int, W: int) -> bool:
    """Python mirror of tante_conv3x3_supported."""
    return (1 <= Cin <= CONV3_MAX_CIN and 1 <= Cout <= CONV3_MAX_COUT and H >= 1 and W >= 1 and 0 <= n_img <= 65535
            and (H * W + 255) // 256 <= 2 ** 31 - 1)


def fold_block(norm_w, norm_b, w1, b1, w2, b2, gamma):
    """pwconv1(LN_affine(z)) = (W1 diag(w)) z + (W1 b_ln + b1) and gamma * pwconv2(h) = (diag(gamma) W2) h + gamma b2
    (unet_convnext.py:139-144), in float64, rounded to fp32 once -> (W1', b1', W2', b2')."""
    w1d, w2d = w1.detach().double(), w2.detach().double()
    nw, nb = norm_w.detach().double(), norm_b.detach().double()
    w1f = w1d * nw[None, :]
    b1f = w1d @ nb + b1.detach().double()
    b2f = b2.detach().double()
    if gamma is not None:
        g = gamma.detach().double()
        w2d, b2f = w2d * g[:, None], b2f * g
    return w1f.float().contiguous(), b1f.float().contiguous(), w2d.float().contiguous(), b2f.float().contiguous()


def fold_cf_norm(weight: torch.Tensor, norm_w: torch.Tensor) -> torch.Tensor:
    """conv(normalize(x) * w) = conv'(normalize(x)) with the input channel's w folded into the convolution's weight (axis 1 of a Conv2d
    weight, axis 0 of a ConvTranspose2d weight is its input channel: pass the weight with the input channel on axis 1), float64."""
    w = norm_w.detach().double().reshape(-1)
    shape = [1, -1] + [1] * (weight.dim() - 2)
    return (weight.detach().double() * w.reshape(shape)).float().contiguous()


def pack_convnext(dw_w, dw_b, w1, b1, w2, b2, C_: int, compute: int) -> torch.Tensor:
    """tante_pack_convnext: the block's stream (depthwise taps, folded biases, both matrices in fragment order)."""
    ts = [t.detach().to(torch.float32).contiguous() for t in (dw_w.reshape(C_, 49), dw_b, w1, b1, w2, b2)]
    K._dev(*ts)
    lib = L.lib()
    out, _ = K.workspace(lib.tante_convnext_stream_bytes(C_), ts[0].device)      # the stream's buffer; the entry point takes no size
    L.check(lib.tante_pack_convnext(*[K._p(t) for t in ts], C_, compute, K._p(out), K._stream()), "tante_pack_convnext")
    return out


def convnext_block(x: torch.Tensor, stream: torch.Tensor, compute: int, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tante_convnext_block on x (n, H, W, C) fp32 channels-last -> a NEW tensor (or `out`, which must not be x)."""
    K._dev(x, stream, out)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("the ConvNeXt block takes fp32 channels-last images (n, H, W, C)")
    n, H, W, C_ = x.shape
    if out is None:
        out = torch.empty_like(x)
    L.check(L.lib().tante_convnext_block(K._p(x), K._p(out), K._p(stream), n, H, W, C_, compute, float(eps), K._stream()), "tante_convnext_block")
    return out


def dwconv_ln(x: torch.Tensor, dw_w: torch.Tensor, dw_b: torch.Tensor, eps: float, ln_w: Optional[torch.Tensor] = None,
              ln_b: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """tante_dwconv_ln on x (n, H, W, C) fp32 -> rows (n H W, C) fp32 or bf16."""
    K._dev(x, dw_w, dw_b, ln_w, ln_b)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("the depthwise convolution takes fp32 channels-last images (n, H, W, C)")
    n, H, W, C_ = x.shape
    out = torch.empty(n * H * W, C_, dtype=out_dtype, device=x.device)
    L.check(L.lib().tante_dwconv_ln(K._p(x), n, H, W, C_, K._p(dw_w), K._p(dw_b), float(eps), K._p(ln_w), K._p(ln_b), K._p(out), K._DT[out_dtype],
                                    K._stream()), "tante_dwconv_ln")
    return out


def l2norm_rows(x: torch.Tensor, eps: float, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """tante_l2norm_rows on rows (M, C) fp32 -> x / max(||x||_2, eps), fp32 or bf16."""
    K._dev(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("the row norm takes fp32 rows (M, C)")
    M, C_ = x.shape
    out = torch.empty(M, C_, dtype=out_dtype, device=x.device)
    L.check(L.lib().tante_l2norm_rows(K._p(x), M, C_, float(eps), K._p(out), K._DT[out_dtype], K._stream()), "tante_l2norm_rows")
    return out


# ---- training: the two backward kernels, their autograd nodes, the graph ------------------------------------------------------------------
def dwconv_ln_bwd_supported_py(n_img: int, H: int, W: int, C_: int) -> bool:
    """Python mirror of tante_dwconv_ln_bwd_supported: the forward's shapes."""
    return dwconv_ln_supported_py(n_img, H, W, C_)


def l2norm_rows_bwd_supported_py(M: int, C_: int) -> bool:
    """Python mirror of tante_l2norm_rows_bwd_supported: the forward's shapes."""
    return l2norm_rows_supported_py(M, C_)


def dwconv_ln_bwd(dy: torch.Tensor, x: torch.Tensor, dw_w: torch.Tensor, dw_b: torch.Tensor, eps: float, ln_w: Optional[torch.Tensor] = None,
                  grads=None, accumulate: bool = False):
    """tante_dwconv_ln_bwd: dy (n H W, C) fp32 or bf16, x (n, H, W, C) fp32, dw_w (C, 49) -> (dx, d_taps (C, 49), d_dwbias, d_ln_w, d_ln_b);
    the last two None without ln_w.  `grads`: the four buffers to write (or, with `accumulate`, to add onto)."""
    K._dev(dy, x, dw_w, dw_b, ln_w)
    if x.dtype != torch.float32 or x.dim() != 4 or dy.dtype not in K._DT or dy.numel() != x.numel():
        raise RuntimeError("the depthwise convolution's backward takes fp32 channels-last images (n, H, W, C) and their rows' gradient in "
                           "fp32 or bf16")
    n, H, W, C_ = x.shape
    lib = L.lib()
    if grads is None:
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)      # noqa: E731
        grads = [new(C_, 49), new(C_), new(C_) if ln_w is not None else None, new(C_) if ln_w is not None else None]
        accumulate = False
    dx = torch.empty_like(x)
    work, nbytes = K.workspace(lib.tante_dwconv_ln_bwd_workspace_bytes(n, H, W, C_), x.device)      # (-1: the call below refuses by name)
    L.check(lib.tante_dwconv_ln_bwd(K._p(dy), K._DT[dy.dtype], K._p(x), n, H, W, C_, K._p(dw_w), K._p(dw_b), float(eps), K._p(ln_w), K._p(dx),
                                    K._p(grads[0]), K._p(grads[1]), K._p(grads[2]), K._p(grads[3]), int(accumulate), K._p(work), nbytes, K._stream()),
            "tante_dwconv_ln_bwd")
    return (dx, *grads)


def l2norm_rows_bwd(dy: torch.Tensor, x: torch.Tensor, eps: float) -> torch.Tensor:
    """tante_l2norm_rows_bwd: dy (M, C) fp32 or bf16, x (M, C) fp32 -> dx fp32."""
    K._dev(dy, x)
    if x.dtype != torch.float32 or x.dim() != 2 or dy.dtype not in K._DT or dy.shape != x.shape:
        raise RuntimeError("the row norm's backward takes fp32 rows (M, C) and their gradient in fp32 or bf16")
    dx = torch.empty_like(x)
    L.check(L.lib().tante_l2norm_rows_bwd(K._p(dy), K._DT[dy.dtype], K._p(x), x.shape[0], x.shape[1], float(eps), K._p(dx), K._stream()),
            "tante_l2norm_rows_bwd")
    return dx


class DwConvLnFn(Function):
    """LN(dwconv7x7(x) + dw_b) [* ln_w + ln_b] on x (n, H, W, C) fp32 -> rows (n H W, C) in out_dtype; dw_w is the Conv2d's (C, 1, 7, 7)
    parameter, read where it lies.  Forward: the unchanged dwconv_ln, bit-identical to it; only x is saved.  Backward:
    tante_dwconv_ln_bwd (dy fp32 or bf16, dx fp32); the parameter gradients go straight into the parameters' gradient slots where all of
    them exist (FlatAdamW)."""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, ln_w, ln_b, eps, out_dtype):
        x = x.contiguous()
        C_ = x.shape[-1]
        y = dwconv_ln(x, dw_w.detach().reshape(C_, 49), dw_b.detach(), eps, None if ln_w is None else ln_w.detach(),
                      None if ln_b is None else ln_b.detach(), out_dtype)
        ctx.save_for_backward(x)
        ctx.params, ctx.eps = (dw_w, dw_b, ln_w, ln_b), float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .autograd import grad_slots
        (x,) = ctx.saved_tensors
        dw_w, dw_b, ln_w, ln_b = ctx.params
        C_ = x.shape[-1]
        dy = dy.contiguous()
        taps, lw = dw_w.detach().reshape(C_, 49), None if ln_w is None else ln_w.detach()
        slots = grad_slots(ctx, ctx.params, 1) if (ln_w is not None and ln_b is not None) else None
        if slots is not None:
            dx = dwconv_ln_bwd(dy, x, taps, dw_b.detach(), ctx.eps, lw, [slots[0].view(C_, 49), *slots[1:]], True)[0]
            return dx, None, None, None, None, None, None
        dx, dt, db, dlw, dlb = dwconv_ln_bwd(dy, x, taps, dw_b.detach(), ctx.eps, lw)
        want = ctx.needs_input_grad
        return (dx, dt.view(dw_w.shape) if want[1] else None, db if want[2] else None, dlw if (ln_w is not None and want[3]) else None,
                dlb if (ln_b is not None and want[4]) else None, None, None)


class L2NormRowsFn(Function):
    """x / max(||x||_2, eps) on rows (M, C) fp32 -> out_dtype: tante_l2norm_rows forward (bit-identical to l2norm_rows),
    tante_l2norm_rows_bwd backward (dy fp32 or bf16, dx fp32)."""

    @staticmethod
    def forward(ctx, x, eps, out_dtype):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.eps = float(eps)
        return l2norm_rows(x, eps, out_dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return l2norm_rows_bwd(dy.contiguous(), x, ctx.eps), None, None


def _fold32(expr64: torch.Tensor) -> torch.Tensor:
    """A parameter-sized float64 expression rounded to fp32 once -- differentiable torch, so the fold's chain rule is torch's."""
    return expr64.float().contiguous()


def block_train(blk: "Block", x: torch.Tensor, compute: int) -> torch.Tensor:
    """Block.run as a graph of training nodes, the MODULAR composition at every width: DwConvLnFn (the norm's affine applied by the
    kernel, not folded, so that its backward returns d_ln_w / d_ln_b) -> LinearFn -> ActFn (erf GELU) -> LinearFn with the skip as the
    residual operand and gamma folded into pwconv2 (float64, rounded once, as fold_block computes it).  The one-launch
    tante_convnext_block stays inference only: its backward is not built."""
    from .autograd import ActFn, LinearFn
    compute = site(compute, "block", BF16_SITES)
    n, H, W, C_ = x.shape
    if not dwconv_ln_supported_py(n, H, W, C_):
        raise NotImplementedError(f"a block of {C_} channels is out of scope: tante_dwconv_ln serves 1..{DWLN_MAX_C}")
    M = n * H * W
    adt = K.act_torch_dtype(compute)
    a = DwConvLnFn.apply(x, blk.dwconv.weight, blk.dwconv.bias, blk.norm.weight, blk.norm.bias, blk.norm.eps, adt)
    h = ActFn.apply(LinearFn.apply(a, blk.pwconv1.weight, blk.pwconv1.bias, None, compute, adt), L.ACT_GELU_ERF, adt)
    w2, b2 = blk.pwconv2.weight, blk.pwconv2.bias
    if blk.gamma is not None:
        g = blk.gamma.double()
        w2, b2 = _fold32(w2.double() * g[:, None]), _fold32(b2.double() * g)
    return LinearFn.apply(h, w2, b2, x.reshape(M, C_), compute, torch.float32).view(n, H, W, C_)


def downsample_train(ds: "Downsample", x: torch.Tensor, compute: int) -> torch.Tensor:
    """Downsample.run as training nodes: L2NormRowsFn -> Im2colFn (2 x 2 / 2) -> LinearFn on the weight with the norm's weight folded in."""
    from .autograd import Im2colFn, LinearFn
    compute = site(compute, "resample", BF16_SITES)
    n, H, W, C_ = x.shape
    if H % 2 or W % 2:
        raise ValueError(f"the 2 x 2 / 2 convolution takes even H and W, got {H} x {W}")
    norm, conv = ds.block[0], ds.block[1]
    adt = K.act_torch_dtype(compute)
    rows = L2NormRowsFn.apply(x.reshape(n * H * W, C_), norm.eps, adt)
    cols = Im2colFn.apply(rows.view(n, H, W, C_), n, C_, H, W, 2, 2, 0, adt)                   # columns (kh, kw, channel)
    wf = conv.weight.double() * norm.weight.double().reshape(1, -1, 1, 1)
    w = _fold32(wf.permute(0, 2, 3, 1).reshape(conv.weight.shape[0], -1))                       # the same order
    return LinearFn.apply(cols, w, conv.bias, None, compute, torch.float32).view(n, H // 2, W // 2, -1)


def upsample_train(us: "Upsample", x: torch.Tensor, compute: int) -> torch.Tensor:
    """Upsample.run as training nodes: L2NormRowsFn -> DeconvFn, or LinearFn (tap matrix) + Col2imFn past 512 input channels, on the
    weight with the norm's weight folded into its rows."""
    compute = site(compute, "resample", BF16_SITES)
    n, H, W, C_ = x.shape
    norm, dec = us.block[0], us.block[1]
    rows = L2NormRowsFn.apply(x.reshape(n * H * W, C_), norm.eps, K.act_torch_dtype(compute))
    wf = dec.weight.double() * norm.weight.double().reshape(-1, 1, 1, 1)                        # (Cin, Cout, 2, 2), rounded once by the node
    return S.deconv_nhwc_train(rows, wf, dec.bias, n, H, W, 2, compute, torch.float32)


def stage_train(st: "Stage", x: torch.Tensor, compute: int, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stage.run as training nodes; skip_proj(cat([x, skip])) is two LinearFn calls through the residual operand: the concatenated tensor
    is never written, forward or backward."""
    from .autograd import LinearFn
    if isinstance(st.skip_proj, nn.Identity):
        if skip is not None:
            raise ValueError("this stage has no skip projection")
    else:
        if skip is None:
            raise ValueError("a stage with skip_proj takes the skip")
        if tuple(skip.shape) != tuple(x.shape):
            raise ValueError(f"the skip must have the stream's shape {tuple(x.shape)}, got {tuple(skip.shape)}")
        cs = site(compute, "skip", BF16_SITES)
        n, H, W, C_ = x.shape
        sp = st.skip_proj
        w = sp.weight.view(C_, 2 * C_)
        adt = K.act_torch_dtype(cs)
        xa, sa = x.reshape(n * H * W, C_), skip.reshape(n * H * W, C_)
        if adt != torch.float32:                                                             # the GEMM's operand type, rounded by a HIP node
            from .autograd import ActFn
            xa, sa = ActFn.apply(xa, L.ACT_NONE, adt), ActFn.apply(sa, L.ACT_NONE, adt)
        out = LinearFn.apply(xa, w[:, :C_].contiguous(), sp.bias, None, cs, torch.float32)
        x = LinearFn.apply(sa, w[:, C_:].contiguous(), None, out, cs, torch.float32).view(n, H, W, C_)
    for blk in st.blocks:
        x = block_train(blk, x, compute)
    if isinstance(st.resample, Downsample):
        x = downsample_train(st.resample, x, compute)
    elif isinstance(st.resample, Upsample):
        x = upsample_train(st.resample, x, compute)
    return x


def _conv3x3_train(x: torch.Tensor, conv: nn.Conv2d) -> torch.Tensor:
    """An edge convolution as training nodes, fp32 in both modes: x (n, H, W, Cin) channels-last -> (n, H, W, Cout): Im2colFn (3 x 3, pad 1)
    + LinearFn (K chunks past 512)."""
    from .autograd import Im2colFn, LinearFn
    n, H, W, Cin = x.shape
    cols = Im2colFn.apply(x, n, Cin, H, W, 3, 1, 1, torch.float32)                             # columns (kh, kw, channel)
    w = conv.weight.permute(0, 2, 3, 1).reshape(conv.weight.shape[0], -1).contiguous()          # the same order, parameter-sized
    return LinearFn.apply(cols, w, conv.bias, None, L.F32, torch.float32).view(n, H, W, -1)


def convnext_train_forward(model: "UNetConvNext", x: torch.Tensor, compute: int) -> torch.Tensor:
    """UNetConvNext.forward with an autograd graph: x (b, t, c, h, w) -> (b, 1, c, h, w) fp32.  torch allocates, re-lays out (the input to
    channels-last, the output back: layout only) and does parameter-sized work (the folds); every other activation-sized operation is a
    HIP node."""
    b, t, c, h, w = x.shape
    cur = _conv3x3_train(x.to(torch.float32).reshape(b, t * c, h, w).permute(0, 2, 3, 1), model.in_proj)
    skips = []
    for enc in model.encoder:
        skips.append(cur)                                                   # skips[0] is stored and never read, as in the reference
        cur = stage_train(enc, cur, compute)
    cur = stage_train(model.neck, cur, compute)
    for j, dec in enumerate(model.decoder):
        cur = stage_train(dec, cur, compute, skips[-j] if j > 0 else None)
    y = _conv3x3_train(cur, model.out_proj)
    return y.permute(0, 3, 1, 2).reshape(b, 1, model.dim_out, h, w)


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], in_nchw: bool, out_nchw: bool) -> torch.Tensor:
    """tante_conv3x3: x (n, Cin, H, W) or (n, H, W, Cin) fp32 -> (n, Cout, H, W) or (n, H, W, Cout) fp32."""
    weight = weight.detach()
    bias = None if bias is None else bias.detach()
    K._dev(x, weight, bias)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("the 3 x 3 convolution takes fp32 images of four dimensions")
    n = x.shape[0]
    Cin, H, W = (x.shape[1], x.shape[2], x.shape[3]) if in_nchw else (x.shape[3], x.shape[1], x.shape[2])
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, Cin, 3, 3):
        raise RuntimeError(f"the weight must be ({Cout}, {Cin}, 3, 3), got {tuple(weight.shape)}")
    out = torch.empty((n, Cout, H, W) if out_nchw else (n, H, W, Cout), dtype=torch.float32, device=x.device)
    L.check(L.lib().tante_conv3x3(K._p(x), n, Cin, H, W, int(in_nchw), K._p(weight), K._p(bias), Cout, K._p(out), int(out_nchw), K._stream()),
            "tante_conv3x3")
    return out


def _conv3x3_any(x: torch.Tensor, conv: nn.Conv2d, cache: _PackCache, in_nchw: bool, out_nchw: bool) -> torch.Tensor:
    """The edge convolutions: tante_conv3x3 where it serves, tante_im2col + tante_gemm (fp32) beyond."""
    n = x.shape[0]
    Cin, H, W = (x.shape[1], x.shape[2], x.shape[3]) if in_nchw else (x.shape[3], x.shape[1], x.shape[2])
    Cout = conv.weight.shape[0]
    if conv3x3_supported_py(n, Cin, Cout, H, W):
        return conv3x3(x, conv.weight, conv.bias, in_nchw, out_nchw)
    korder = 0 if in_nchw else 1
    chunks = cache.get(("im2col", korder), [conv.weight, conv.bias],
                       lambda: S.pack_linear_chunks(S.conv_weight_2d(conv.weight, korder).contiguous(), conv.bias.detach(), L.F32))
    cols = K.im2col(x, in_nchw, n, Cin, H, W, 3, 3, 1, 1, 1, 1, korder, torch.float32)
    y = S.linear_chunks(cols, chunks, torch.float32)
    return S._rows_to_nchw(y, n, H, W) if out_nchw else y.view(n, H, W, Cout)


# ---- the reference's modules -------------------------------------------------------------------------------------------------------
WHY_INFERENCE_ONLY = "the backward of the fused block is a kernel of its own that is not built"


def _refuse(module: nn.Module):
    inference_only(module, "UNetConvNext", WHY_INFERENCE_ONLY)


def _two_d(n_spatial_dims: int):
    if n_spatial_dims != 2:
        raise NotImplementedError(f"n_spatial_dims = {n_spatial_dims} is out of scope: the HIP path serves 2-D fields")


class LayerNorm(Trainable, nn.Module):
    """unet_convnext.py:39-70.  channels_last: a LayerNorm over the last axis.  channels_first: NOT a LayerNorm but
    F.normalize(x, p=2, dim=1, eps) * weight; `bias` is held and never applied.  A parameter holder: its owner folds the affine into the
    GEMM behind it; forward evaluates it alone."""

    def __init__(self, normalized_shape, n_spatial_dims, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format == "channels_last":
            padded_shape = (normalized_shape,)
        else:
            padded_shape = (normalized_shape,) + (1,) * n_spatial_dims
        self.weight = nn.Parameter(torch.ones(padded_shape))
        self.bias = nn.Parameter(torch.zeros(padded_shape))
        self.n_spatial_dims = n_spatial_dims
        self.eps = eps
        self.data_format = data_format
        if self.data_format not in ["channels_last", "channels_first"]:
            raise NotImplementedError
        self.normalized_shape = (normalized_shape,)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """channels_last (..., C) -> (..., C); channels_first is evaluated by Downsample / Upsample.  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        if self.data_format != "channels_last":
            raise NotImplementedError("the channels_first norm is evaluated by its Downsample / Upsample (tante_l2norm_rows, weight folded "
                                      "into the convolution)")
        gpu_only(x, "UNetConvNext")
        if train:
            from .autograd import LayerNormAffineFn
            return LayerNormAffineFn.apply(x.to(torch.float32), self.weight, self.bias, self.eps).to(x.dtype)
        return K.layernorm_affine(x.detach().to(torch.float32), self.weight.detach(), self.bias.detach(), self.eps).to(x.dtype)


class _Resample(Trainable, nn.Module):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, C, H, W) -> (n, C', H', W').  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        gpu_only(x, "UNetConvNext")
        if train:
            fn = downsample_train if isinstance(self, Downsample) else upsample_train
            return fn(self, x.to(torch.float32).permute(0, 2, 3, 1), resolve_compute(None)).permute(0, 3, 1, 2).to(x.dtype)
        return to_nchw(self.run(to_nhwc(x), resolve_compute(None)), x)


class Upsample(_Resample):
    """channels-first norm -> ConvTranspose2d 2 x 2 / 2  (unet_convnext.py:73-86)."""

    def __init__(self, dim_in, dim_out, n_spatial_dims=2):
        super().__init__()
        _two_d(n_spatial_dims)
        self.block = nn.Sequential(LayerNorm(dim_in, n_spatial_dims, eps=1e-6, data_format="channels_first"),
                                   nn.ConvTranspose2d(dim_in, dim_out, kernel_size=2, stride=2))
        self._cache = _PackCache()

    def _packed(self, compute: int):
        norm, dec = self.block[0], self.block[1]

        def build():
            w = fold_cf_norm(dec.weight.transpose(0, 1), norm.weight).transpose(0, 1).contiguous()      # (Cin, Cout, 2, 2)
            return S.pack_deconv_nhwc(w, dec.bias.detach(), 2, compute)
        return self._cache.get(compute, [norm.weight, dec.weight, dec.bias], build)

    def run(self, x: torch.Tensor, compute: int) -> torch.Tensor:
        """x (n, H, W, C) fp32 -> (n, 2 H, 2 W, C') fp32."""
        compute = site(compute, "resample", BF16_SITES)
        n, H, W, C_ = x.shape
        dec = self.block[1]
        cout = dec.weight.shape[1]
        pw = self._packed(compute)
        rows = l2norm_rows(x.view(n * H * W, C_), self.block[0].eps, K.act_torch_dtype(compute))
        return S.deconv_nhwc(rows, pw, dec.bias.detach(), n, H, W, 2, cout)


class Downsample(_Resample):
    """channels-first norm -> Conv2d 2 x 2 / 2  (unet_convnext.py:89-100)."""

    def __init__(self, dim_in, dim_out, n_spatial_dims=2):
        super().__init__()
        _two_d(n_spatial_dims)
        self.block = nn.Sequential(LayerNorm(dim_in, n_spatial_dims, eps=1e-6, data_format="channels_first"),
                                   nn.Conv2d(dim_in, dim_out, kernel_size=2, stride=2))
        self._cache = _PackCache()

    def _packed(self, compute: int):
        norm, conv = self.block[0], self.block[1]
        return self._cache.get(compute, [norm.weight, conv.weight, conv.bias], lambda: S.pack_linear_chunks(
            S.conv_rows(fold_cf_norm(conv.weight, norm.weight)), conv.bias.detach(), compute))

    def run(self, x: torch.Tensor, compute: int) -> torch.Tensor:
        """x (n, H, W, C) fp32 -> (n, H / 2, W / 2, C') fp32."""
        compute = site(compute, "resample", BF16_SITES)
        n, H, W, C_ = x.shape
        if H % 2 or W % 2:
            raise ValueError(f"the 2 x 2 / 2 convolution takes even H and W, got {H} x {W}")
        adt = K.act_torch_dtype(compute)
        rows = l2norm_rows(x.view(n * H * W, C_), self.block[0].eps, adt)
        cols = K.im2col(rows, False, n, C_, H, W, 2, 2, 2, 2, 0, 0, 1, adt)
        y = S.linear_chunks(cols, self._packed(compute), torch.float32)
        return y.view(n, H // 2, W // 2, -1)


class Block(Trainable, nn.Module):
    """dwconv 7 x 7 -> LayerNorm -> Linear C -> 4 C -> GELU -> Linear 4 C -> C -> gamma -> + input  (unet_convnext.py:103-148)."""

    def __init__(self, dim, n_spatial_dims, drop_path=0.0, layer_scale_init_value=1e-6):
        super().__init__()
        _two_d(n_spatial_dims)
        if drop_path > 0.0:
            raise NotImplementedError("drop_path > 0 is out of scope: the reference's UNetConvNext builds every block with 0")
        self.n_spatial_dims = n_spatial_dims
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, n_spatial_dims, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True) if layer_scale_init_value > 0 else None
        self.drop_path = nn.Identity()
        self._cache = _PackCache()

    def _params(self):
        return [self.dwconv.weight, self.dwconv.bias, self.norm.weight, self.norm.bias, self.pwconv1.weight, self.pwconv1.bias, self.pwconv2.weight,
                self.pwconv2.bias] + ([self.gamma] if self.gamma is not None else [])

    def _folded(self):
        return fold_block(self.norm.weight, self.norm.bias, self.pwconv1.weight, self.pwconv1.bias, self.pwconv2.weight, self.pwconv2.bias, self.gamma)

    def _packed_fused(self, compute: int):
        C_ = self.dwconv.weight.shape[0]
        return self._cache.get(("fused", compute), self._params(),
                               lambda: pack_convnext(self.dwconv.weight, self.dwconv.bias, *self._folded(), C_, compute))

    def _packed_modular(self, compute: int):
        C_ = self.dwconv.weight.shape[0]

        def build():
            w1, b1, w2, b2 = self._folded()
            return (self.dwconv.weight.detach().reshape(C_, 49).contiguous(), self.dwconv.bias.detach().contiguous(),
                    S.pack_linear_chunks(w1, b1, compute), S.pack_linear_chunks(w2, b2, compute))
        return self._cache.get(("modular", compute), self._params(), build)

    def run(self, x: torch.Tensor, compute: int, out: Optional[torch.Tensor] = None, fused: Optional[bool] = None) -> torch.Tensor:
        """x (n, H, W, C) fp32 -> `out` (a new tensor by default; never x)."""
        compute = site(compute, "block", BF16_SITES)
        n, H, W, C_ = x.shape
        fused = (FUSED and C_ <= FUSED_DEFAULT_MAX_C) if fused is None else fused
        if out is None:
            out = torch.empty_like(x)
        if fused and convnext_block_supported_py(n, H, W, C_):
            return convnext_block(x, self._packed_fused(compute), compute, self.norm.eps, out)
        if not dwconv_ln_supported_py(n, H, W, C_):
            raise NotImplementedError(f"a block of {C_} channels is out of scope: tante_dwconv_ln serves 1..{DWLN_MAX_C}")
        dw_w, dw_b, fc1, fc2 = self._packed_modular(compute)
        adt = K.act_torch_dtype(compute)
        a = dwconv_ln(x, dw_w, dw_b, self.norm.eps, None, None, adt)
        h = S.linear_chunks(a, fc1, adt, L.ACT_GELU_ERF)
        S.linear_chunks(h, fc2, residual=x.view(n * H * W, C_), out=out.view(n * H * W, C_))  # gamma folded; the skip rides the residual operand
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, C, H, W) -> (n, C, H, W)  (unet_convnext.py:134-148).  Under grad only after set_trainable(), and then by block_train."""
        train = wants_graph(self, x, _refuse)
        gpu_only(x, "UNetConvNext")
        if train:
            return block_train(self, x.to(torch.float32).permute(0, 2, 3, 1).contiguous(), resolve_compute(None)).permute(0, 3, 1, 2).to(x.dtype)
        return to_nchw(self.run(to_nhwc(x), resolve_compute(None)), x)


class Stage(Trainable, nn.Module):
    """skip_proj -> blocks -> resample  (unet_convnext.py:151-199)."""

    def __init__(self, dim_in, dim_out, n_spatial_dims, depth=1, drop_path=0.0, layer_scale_init_value=1e-6, mode="down", skip_project=False):
        super().__init__()
        _two_d(n_spatial_dims)
        if skip_project:
            self.skip_proj = nn.Conv2d(2 * dim_in, dim_in, 1)
        else:
            self.skip_proj = nn.Identity()
        if mode == "down":
            self.resample = Downsample(dim_in, dim_out, n_spatial_dims)
        elif mode == "up":
            self.resample = Upsample(dim_in, dim_out, n_spatial_dims)
        else:
            self.resample = nn.Identity()
        self.blocks = nn.ModuleList([Block(dim_in, n_spatial_dims, drop_path, layer_scale_init_value) for _ in range(depth)])
        self._cache = _PackCache()

    def _packed_skip(self, compute: int):
        sp = self.skip_proj
        C_ = sp.weight.shape[0]

        def build():
            w = sp.weight.detach().reshape(C_, 2 * C_)
            return (S.pack_linear_chunks(w[:, :C_].contiguous(), sp.bias.detach(), compute), S.pack_linear_chunks(w[:, C_:].contiguous(), None, compute))
        return self._cache.get(compute, [sp.weight, sp.bias], build)

    def project(self, x: torch.Tensor, skip: torch.Tensor, compute: int) -> torch.Tensor:
        """skip_proj(cat([x, skip], channels)) without the concatenation: W[:, :C] x + b, then + W[:, C:] skip through the residual operand."""
        compute = site(compute, "skip", BF16_SITES)
        n, H, W, C_ = x.shape
        if tuple(skip.shape) != tuple(x.shape):
            raise ValueError(f"the skip must have the stream's shape {tuple(x.shape)}, got {tuple(skip.shape)}")
        wx, ws = self._packed_skip(compute)
        out = S.linear_chunks(x.view(n * H * W, C_), wx)
        S.linear_chunks(skip.view(n * H * W, C_), ws, residual=out, out=out)
        return out.view(n, H, W, C_)

    def run(self, x: torch.Tensor, compute: int, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x (n, H, W, C) fp32 channels-last (and the skip of the same shape for a stage with skip_proj) -> the stage's output.  x and skip
        are left unchanged: the blocks ping-pong two buffers of the stage's own."""
        if isinstance(self.skip_proj, nn.Identity):
            if skip is not None:
                raise ValueError("this stage has no skip projection")
        else:
            if skip is None:
                raise ValueError("a stage with skip_proj takes the skip")
            x = self.project(x, skip, compute)
        bufs = [torch.empty_like(x) for _ in range(min(len(self.blocks), 2))]
        for i, blk in enumerate(self.blocks):
            x = blk.run(x, compute, bufs[i % 2])
        if not isinstance(self.resample, nn.Identity):
            x = self.resample.run(x, compute)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, C, H, W), or (n, 2 C, H, W) = cat([x, skip]) for a stage with skip_proj -> the stage's output, channels first.  Under grad only
        after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        gpu_only(x, "UNetConvNext")
        compute = resolve_compute(None)
        if train:
            xl = x.to(torch.float32).permute(0, 2, 3, 1)
            if isinstance(self.skip_proj, nn.Identity):
                return stage_train(self, xl.contiguous(), compute).permute(0, 3, 1, 2).to(x.dtype)
            C_ = self.skip_proj.weight.shape[0]
            return stage_train(self, xl[..., :C_].contiguous(), compute, xl[..., C_:].contiguous()).permute(0, 3, 1, 2).to(x.dtype)
        if isinstance(self.skip_proj, nn.Identity):
            return to_nchw(self.run(to_nhwc(x), compute), x)
        C_ = self.skip_proj.weight.shape[0]
        return to_nchw(self.run(to_nhwc(x[:, :C_]), compute, to_nhwc(x[:, C_:])), x)


class UNetConvNext(Trainable, ComputeSwitch, nn.Module):
    """models/unet_convnext.py:202-283 -- same constructor, attributes, parameters and forward contract."""

    def __init__(self, in_T, dset_metadata, stages: int = 4, blocks_per_stage: int = 1, blocks_at_neck: int = 1, n_spatial_dims: int = 2,
                 init_features: int = 32, gradient_checkpointing: bool = False):
        super().__init__()
        n_channel = dset_metadata.n_fields
        dim_in = n_channel * in_T
        dim_out = n_channel
        self.dset_metadata = dset_metadata
        n_spatial_dims = dset_metadata.n_spatial_dims                       # the argument is ignored (unet_convnext.py:219)
        _two_d(n_spatial_dims)
        self.n_spatial_dims = n_spatial_dims
        features = init_features
        self.gradient_checkpointing = gradient_checkpointing
        encoder_dims = [features * 2 ** i for i in range(stages + 1)]
        decoder_dims = [features * 2 ** i for i in range(stages, -1, -1)]
        encoder = []
        decoder = []
        self.in_proj = nn.Conv2d(dim_in, features, kernel_size=3, padding=1)
        self.out_proj = nn.Conv2d(features, dim_out, kernel_size=3, padding=1)
        for i in range(stages):
            encoder.append(Stage(encoder_dims[i], encoder_dims[i + 1], n_spatial_dims, blocks_per_stage, mode="down"))
            decoder.append(Stage(decoder_dims[i], decoder_dims[i + 1], n_spatial_dims, blocks_per_stage, mode="up", skip_project=i != 0))
        self.encoder = nn.ModuleList(encoder)
        self.neck = Stage(encoder_dims[-1], encoder_dims[-1], n_spatial_dims, blocks_at_neck, mode="neck")
        self.decoder = nn.ModuleList(decoder)
        self.dim_in, self.dim_out, self.stages = dim_in, dim_out, stages
        self._cache = _PackCache()

    def trained_parameters(self):
        """Every parameter except *.resample.block.0.bias: the channels_first norm's bias, which the reference holds and never applies
        (unet_convnext.py:69), so it never receives a gradient and torch's AdamW never touches it.  FlatAdamW decays everything it is
        given: pass it THIS list, not parameters()."""
        return [p for n, p in self.named_parameters() if not n.endswith("resample.block.0.bias")]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, 1, c, h, w)   (unet_convnext.py:269-283).  Under grad only after set_trainable()."""
        train = wants_graph(self, x, _refuse)
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, C, H, W), got {tuple(x.shape)}")
        b, t, c, h, w = x.shape
        if t * c != self.dim_in:
            raise ValueError(f"the input has t * c = {t} * {c} = {t * c} channels, in_proj takes dim_in = n_fields * in_T = {self.dim_in}")
        div = 2 ** self.stages
        if h % div or w % div:
            raise ValueError(f"H and W must be multiples of 2 ** stages = {div} (the decoder's skips would not match), got {h} x {w}")
        gpu_only(x, "UNetConvNext")
        compute = resolve_compute(self.compute)
        if train:
            return convnext_train_forward(self, x, compute)
        x4 = x.detach().to(torch.float32).contiguous().view(b, t * c, h, w)       # b t c h w contiguous IS b (t c) h w
        cur = _conv3x3_any(x4, self.in_proj, self._cache, True, False)
        skips = []
        for enc in self.encoder:
            skips.append(cur)                                                   # skips[0] is stored and never read, as in the reference
            cur = enc.run(cur, compute)
        cur = self.neck.run(cur, compute)
        for j, dec in enumerate(self.decoder):
            cur = dec.run(cur, compute, skips[-j] if j > 0 else None)
        y = _conv3x3_any(cur, self.out_proj, self._cache, False, True)
        return y.view(b, 1, self.dim_out, h, w)
