"""AttentionUNet baseline on the HIP kernels  (reference models/unet_att.py, configs/unet_att.yaml).

Same constructor arguments, attributes, module tree, `state_dict` keys / shapes (the BatchNorm buffers included) and forward contract
(`b t c h w -> b out_T c h w`) as the reference's models.AttentionUNet.  The model is channels-last inside, (n, H, W, C) fp32, and every
arithmetic step is a C-ABI call of libtante_hip:
  Conv2d 3 x 3 -> BatchNorm2d -> ReLU   ONE launch, tante_conv3x3_mfma: an implicit GEMM on the matrix pipe.  The eval-mode norm and the
                      conv bias are folded in float64 at pack time (scale into the weights, shift into the epilogue).  Its staging loop
                      takes the source form, so three tensors of the model are never written: MaxPool2d(2, 2) in front of Conv2..5
                      (pooled), nn.Upsample(2) in front of Up5..2 (upsampled) and torch.cat((s, d)) in front of UpConv5..2 (two sources).
  AttentionBlock      ONE launch, tante_attn_gate: both 1 x 1 convolutions as one product over [g | x], ReLU, the dot product with
                      w_psi, the sigmoid and x * psi; the three norms folded.
  self.Conv           tante_gemm on the channels-last rows; the output channel index is read as (c t) (unet_att.py:173).
With TANTE_UNETATT_MFMA = 0 every 3 x 3 convolution runs tante_im2col + tante_gemm instead, and the pool, the upsample, the
concatenation and the gate are separate torch / tante_gemm steps: the parity and A/B partner of the two kernels.
torch allocates and reshapes.

In bf16 mode bf16 is the operand type of the groups in BF16_SITES; accumulation, the epilogues and the activations between the
launches stay fp32.

Inference only (eval mode under no_grad: the norms use their running statistics).  Training, 3-D fields, a wrong t * c and H or W not
divisible by 2 ** (depth - 1) raise (the reference fails there too, at the gate's add); there is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from . import options as _O
from . import stages as S
from .attn_backbone import _PackCache, resolve_compute
from .model_shell import ComputeSwitch, gpu_only, inference_only, site, to_nchw, to_nhwc

CONV_MAX_CIN, CONV_MAX_COUT = 2048, 1024     # channels tante_conv3x3_mfma serves
GATE_MAX_K, GATE_MAX_N = 1024, 256           # gate plus skip channels, coefficients tante_attn_gate serves
PLAIN, POOLED, UPSAMPLED = 0, 1, 2           # the source forms of tante_conv3x3_mfma
BF16_SITES = ("conv", "gate", "head")        # the groups that take bf16 operands in bf16 mode (DESIGN 4.9 has the per-group figures)

# True: the 3 x 3 convolutions and the gates run as tante_conv3x3_mfma / tante_attn_gate; False: tante_im2col + tante_gemm and separate
# pool / upsample / cat / gate steps, the A/B and parity partner
MFMA = _O.register("TANTE_UNETATT_MFMA", True, __name__, "MFMA")


# ---- host side of the kernels: the predicates' mirrors, the folds, the wrappers -----------------------------------------------------------
def conv3x3_mfma_supported_py(n_img: int, Ca: int, Cb: int, Cout: int, H: int, W: int, form: int) -> bool:
    """Python mirror of tante_conv3x3_mfma_supported."""
    if form not in (PLAIN, POOLED, UPSAMPLED) or Ca < 1 or Cb < 0 or Ca + Cb > CONV_MAX_CIN or (Cb > 0 and form != PLAIN):
        return False
    if not (1 <= Cout <= CONV_MAX_COUT) or H < 1 or W < 1 or (form == UPSAMPLED and (H % 2 or W % 2)) or n_img < 0:
        return False
    tiles = ((W + 15) // 16) * ((H + 1) // 2)
    return tiles <= 2 ** 31 - 1 and n_img * tiles <= 2 ** 31 - 1


def attn_gate_supported_py(M: int, Cg: int, Cx: int, N: int) -> bool:
    """Python mirror of tante_attn_gate_supported: any gate and skip widths with Cg + Cx <= 1024 and up to 256 coefficients (the
    reference's gates are Cg = Cx = C, N = C / 2 for C = 64 .. 512)."""
    return Cg >= 1 and Cx >= 1 and Cg + Cx <= GATE_MAX_K and 1 <= N <= GATE_MAX_N and 0 <= M and (M + 15) // 16 <= 2 ** 31 - 1


def bn_scale_shift(bn: nn.BatchNorm2d, conv_bias: Optional[torch.Tensor]):
    """Eval-mode BatchNorm behind a convolution, float64: scale = weight / sqrt(running_var + eps),
    shift = bias + (conv bias - running_mean) * scale."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    cb = 0.0 if conv_bias is None else conv_bias.detach().double()
    return s, bn.bias.detach().double() + (cb - bn.running_mean.detach().double()) * s


def fold_conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """bn(conv(x)) = conv'(x) + shift with the scale folded into the weight, in float64, rounded to fp32 once -> (W', shift)."""
    s, shift = bn_scale_shift(bn, conv.bias)
    w = conv.weight.detach().double() * s.reshape(-1, 1, 1, 1)
    return w.float().contiguous(), shift.float().contiguous()


def fold_gate(gate: "AttentionBlock"):
    """The three norms of an AttentionBlock folded in float64 -> (W (N, Cg + Cx) = [W_gate' | W_x'], b = b_gate' + b_x', w_psi (N), b_psi)."""
    wg, bg = fold_conv_bn(gate.W_gate[0], gate.W_gate[1])
    wx, bx = fold_conv_bn(gate.W_x[0], gate.W_x[1])
    wp, bp = fold_conv_bn(gate.psi[0], gate.psi[1])
    N = wg.shape[0]
    w = torch.cat([wg.reshape(N, -1), wx.reshape(N, -1)], dim=1).contiguous()
    return w, (bg.double() + bx.double()).float().contiguous(), wp.reshape(N).contiguous(), float(bp.reshape(()))


def pack_conv3x3(w: torch.Tensor, compute: int) -> torch.Tensor:
    """tante_pack_conv3x3: (Cout, Cin, 3, 3) fp32 (scale folded) -> the fragment order of `compute`, padded channels zero."""
    w = w.detach().to(torch.float32).contiguous()
    K._dev(w)
    Cout, Cin = w.shape[0], w.shape[1]
    if tuple(w.shape) != (Cout, Cin, 3, 3):
        raise RuntimeError(f"the weight must be (Cout, Cin, 3, 3), got {tuple(w.shape)}")
    lib = L.lib()
    nbytes = int(lib.tante_conv3x3_pack_bytes(Cin, Cout, compute))
    if nbytes < 0:
        raise NotImplementedError(f"a 3 x 3 convolution {Cin} -> {Cout} is out of scope: tante_conv3x3_mfma serves Cin <= {CONV_MAX_CIN}, Cout <= {CONV_MAX_COUT}")
    out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    L.check(lib.tante_pack_conv3x3(K._p(w), Cin, Cout, compute, K._p(out), K._stream()), "tante_pack_conv3x3")
    return out


def conv3x3_mfma(a: torch.Tensor, packed: torch.Tensor, shift: Optional[torch.Tensor], Cout: int, compute: int, relu: bool = True, form: int = PLAIN,
                 b: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """tante_conv3x3_mfma on a (n, Hs, Ws, Ca) [and b (n, Hs, Ws, Cb)] fp32 channels-last -> (n, H, W, Cout) fp32 or bf16."""
    K._dev(a, b, packed, shift)
    for t in (a, b):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 4):
            raise RuntimeError("the 3 x 3 convolution takes fp32 channels-last images (n, H, W, C)")
    n, Hs, Ws, Ca = a.shape
    Cb = 0 if b is None else b.shape[3]
    if b is not None and tuple(b.shape[:3]) != (n, Hs, Ws):
        raise RuntimeError(f"the second source must be {(n, Hs, Ws)} pixels, got {tuple(b.shape[:3])}")
    H, W = (Hs // 2, Ws // 2) if form == POOLED else (2 * Hs, 2 * Ws) if form == UPSAMPLED else (Hs, Ws)
    out = torch.empty(n, H, W, Cout, dtype=out_dtype, device=a.device)
    L.check(L.lib().tante_conv3x3_mfma(K._p(a), Ca, K._p(b), Cb, n, H, W, form, Hs, Ws, K._p(packed), K._p(shift), Cout,
                                       L.ACT_RELU if relu else L.ACT_NONE, compute, K._p(out), K._DT[out_dtype], K._stream()), "tante_conv3x3_mfma")
    return out


def pack_attn_gate(w: torch.Tensor, bias: torch.Tensor, wpsi: torch.Tensor, bpsi: float, Cg: int, Cx: int, compute: int) -> torch.Tensor:
    """tante_pack_attn_gate: the folded gate -> one stream."""
    ts = [t.detach().to(torch.float32).contiguous() for t in (w, bias, wpsi)]
    K._dev(*ts)
    N = ts[0].shape[0]
    lib = L.lib()
    nbytes = int(lib.tante_attn_gate_stream_bytes(Cg, Cx, N, compute))
    if nbytes < 0:
        raise NotImplementedError(f"a gate of {Cg} + {Cx} channels and {N} coefficients is out of scope: tante_attn_gate serves Cg + Cx <= {GATE_MAX_K}, "
                                  f"N <= {GATE_MAX_N}")
    out = torch.empty(nbytes, dtype=torch.uint8, device=ts[0].device)
    L.check(lib.tante_pack_attn_gate(*[K._p(t) for t in ts], float(bpsi), Cg, Cx, N, compute, K._p(out), K._stream()), "tante_pack_attn_gate")
    return out


def attn_gate(g: torch.Tensor, x: torch.Tensor, stream: torch.Tensor, N: int, compute: int) -> torch.Tensor:
    """tante_attn_gate on rows g (M, Cg), x (M, Cx) fp32 -> x * psi, (M, Cx) fp32."""
    K._dev(g, x, stream)
    if g.dtype != torch.float32 or x.dtype != torch.float32 or g.dim() != 2 or x.dim() != 2 or g.shape[0] != x.shape[0]:
        raise RuntimeError("the attention gate takes fp32 rows g (M, Cg) and x (M, Cx)")
    out = torch.empty_like(x)
    L.check(L.lib().tante_attn_gate(K._p(g), K._p(x), x.shape[0], g.shape[1], x.shape[1], N, K._p(stream), compute, K._p(out), K._stream()), "tante_attn_gate")
    return out


# ---- the reference's modules -------------------------------------------------------------------------------------------------------
WHY_INFERENCE_ONLY = "batch statistics and the backward of the convolution are kernels of their own that are not built"


def _source(a: torch.Tensor, form: int, b: Optional[torch.Tensor]) -> torch.Tensor:
    """The modular route's input of a convolution, written out: the pooled, the upsampled or the concatenated tensor."""
    if form == POOLED:
        n, Hs, Ws, C_ = a.shape
        H, W = Hs // 2, Ws // 2
        return a[:, :2 * H, :2 * W].reshape(n, H, 2, W, 2, C_).amax(dim=(2, 4))
    if form == UPSAMPLED:
        return a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return a if b is None else torch.cat((a, b), dim=3)


def _conv_bn_act(a: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, cache: _PackCache, slot: str, compute: int, form: int = PLAIN,
                 b: Optional[torch.Tensor] = None, mfma: Optional[bool] = None) -> torch.Tensor:
    """relu(bn(conv3x3(source))) on channels-last fp32 images -> (n, H, W, Cout) fp32."""
    compute = site(compute, "conv", BF16_SITES)
    mfma = MFMA if mfma is None else mfma
    params = [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    Cout = conv.weight.shape[0]
    n, Hs, Ws, Ca = a.shape
    Cb = 0 if b is None else b.shape[3]
    if mfma:
        H, W = (Hs // 2, Ws // 2) if form == POOLED else (2 * Hs, 2 * Ws) if form == UPSAMPLED else (Hs, Ws)
        if not conv3x3_mfma_supported_py(n, Ca, Cb, Cout, H, W, form):
            raise NotImplementedError(f"a 3 x 3 convolution {Ca} + {Cb} -> {Cout} on {H} x {W} (form {form}) is out of scope of tante_conv3x3_mfma")

        def build():
            w, shift = fold_conv_bn(conv, bn)
            return pack_conv3x3(w, compute), shift
        packed, shift = cache.get((slot, "mfma", compute), params, build)
        return conv3x3_mfma(a, packed, shift, Cout, compute, True, form, b)

    def build():
        w, shift = fold_conv_bn(conv, bn)
        return S.pack_linear_chunks(S.conv_rows(w), shift, compute)
    chunks = cache.get((slot, "im2col", compute), params, build)
    src = _source(a, form, b).contiguous()
    n, H, W, Cin = src.shape
    adt = K.act_torch_dtype(compute)
    cols = K.im2col(src, False, n, Cin, H, W, 3, 3, 1, 1, 1, 1, 1, adt)
    return S.linear_chunks(cols, chunks, torch.float32, L.ACT_RELU).view(n, H, W, Cout)


class ConvBlock(nn.Module):
    """(Conv2d 3 x 3 -> BatchNorm2d -> ReLU) twice  (unet_att.py:6-21)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True)
        )
        self._cache = _PackCache()

    def run(self, a: torch.Tensor, compute: int, form: int = PLAIN, b: Optional[torch.Tensor] = None, mfma: Optional[bool] = None) -> torch.Tensor:
        """a (n, Hs, Ws, Ca) [and b (n, Hs, Ws, Cb)] fp32 channels-last, read in `form` -> (n, H, W, Cout) fp32."""
        y = _conv_bn_act(a, self.conv[0], self.conv[1], self._cache, "c0", compute, form, b, mfma)
        return _conv_bn_act(y, self.conv[3], self.conv[4], self._cache, "c1", compute, PLAIN, None, mfma)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, Cin, H, W) -> (n, Cout, H, W).  Inference only."""
        inference_only(self, "AttentionUNet", WHY_INFERENCE_ONLY)
        gpu_only(x, "AttentionUNet")
        return to_nchw(self.run(to_nhwc(x), resolve_compute(None)), x)


class UpConv(nn.Module):
    """Upsample(2, nearest) -> Conv2d 3 x 3 -> BatchNorm2d -> ReLU  (unet_att.py:24-38)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.up = nn.Sequential(
            nn.Upsample(scale_factor=2),
            nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True)
        )
        self._cache = _PackCache()

    def run(self, x: torch.Tensor, compute: int, mfma: Optional[bool] = None) -> torch.Tensor:
        """x (n, H, W, C) fp32 channels-last -> (n, 2 H, 2 W, Cout) fp32; the upsampled tensor is never written on the MFMA route."""
        return _conv_bn_act(x, self.up[1], self.up[2], self._cache, "up", compute, UPSAMPLED, None, mfma)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(n, Cin, H, W) -> (n, Cout, 2 H, 2 W).  Inference only."""
        inference_only(self, "AttentionUNet", WHY_INFERENCE_ONLY)
        gpu_only(x, "AttentionUNet")
        return to_nchw(self.run(to_nhwc(x), resolve_compute(None)), x)


class AttentionBlock(nn.Module):
    """psi = sigmoid(BN(conv1x1(relu(BN(conv1x1(gate)) + BN(conv1x1(skip)))))); out = skip * psi  (unet_att.py:41-76)."""

    def __init__(self, F_g, F_l, n_coefficients):
        super().__init__()
        self.W_gate = nn.Sequential(
            nn.Conv2d(F_g, n_coefficients, kernel_size=1, stride=1, padding=0, bias=True),
            nn.BatchNorm2d(n_coefficients)
        )
        self.W_x = nn.Sequential(
            nn.Conv2d(F_l, n_coefficients, kernel_size=1, stride=1, padding=0, bias=True),
            nn.BatchNorm2d(n_coefficients)
        )
        self.psi = nn.Sequential(
            nn.Conv2d(n_coefficients, 1, kernel_size=1, stride=1, padding=0, bias=True),
            nn.BatchNorm2d(1),
            nn.Sigmoid()
        )
        self.relu = nn.ReLU(inplace=True)
        self._cache = _PackCache()

    def _params(self):
        out = []
        for seq in (self.W_gate, self.W_x, self.psi):
            conv, bn = seq[0], seq[1]
            out += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return out

    def run(self, gate: torch.Tensor, skip: torch.Tensor, compute: int, mfma: Optional[bool] = None) -> torch.Tensor:
        """gate (n, H, W, Cg), skip (n, H, W, Cx) fp32 channels-last -> skip * psi, (n, H, W, Cx) fp32."""
        compute = site(compute, "gate", BF16_SITES)
        mfma = MFMA if mfma is None else mfma
        if tuple(gate.shape[:3]) != tuple(skip.shape[:3]):
            raise ValueError(f"the gate and the skip must cover the same pixels, got {tuple(gate.shape)} and {tuple(skip.shape)}")
        n, H, W, Cx = skip.shape
        Cg = gate.shape[3]
        N = self.W_gate[0].weight.shape[0]
        M = n * H * W
        g2, x2 = gate.reshape(M, Cg), skip.reshape(M, Cx)
        if mfma:
            if not attn_gate_supported_py(M, Cg, Cx, N):
                raise NotImplementedError(f"a gate of {Cg} + {Cx} channels and {N} coefficients is out of scope of tante_attn_gate")

            def build():
                w, b, wp, bp = fold_gate(self)
                return pack_attn_gate(w, b, wp, bp, Cg, Cx, compute)
            return attn_gate(g2, x2, self._cache.get(("mfma", compute), self._params(), build), N, compute).view(n, H, W, Cx)

        def build():
            w, b, wp, bp = fold_gate(self)
            return (S.pack_linear_chunks(w[:, :Cg].contiguous(), b, compute), S.pack_linear_chunks(w[:, Cg:].contiguous(), None, compute), wp, bp)
        wg, wx, wp, bp = self._cache.get(("modular", compute), self._params(), build)
        adt = K.act_torch_dtype(compute)
        h = S.linear_chunks(g2.to(adt), wg)
        S.linear_chunks(x2.to(adt), wx, residual=h, out=h)
        psi = torch.sigmoid(torch.relu(h) @ wp + bp)
        return (x2 * psi[:, None]).view(n, H, W, Cx)

    def forward(self, gate: torch.Tensor, skip_connection: torch.Tensor) -> torch.Tensor:
        """(n, F_g, H, W), (n, F_l, H, W) -> (n, F_l, H, W)  (unet_att.py:70-76).  Inference only."""
        inference_only(self, "AttentionUNet", WHY_INFERENCE_ONLY)
        gpu_only(gate, "AttentionUNet")
        gpu_only(skip_connection, "AttentionUNet")
        return to_nchw(self.run(to_nhwc(gate), to_nhwc(skip_connection), resolve_compute(None)), skip_connection)


class AttentionUNet(ComputeSwitch, nn.Module):
    """models/unet_att.py:79-175 -- same constructor, attributes, parameters, buffers and forward contract."""

    def __init__(self, in_T, dset_metadata=None, depth=4, out_T=4):
        super().__init__()
        if dset_metadata is not None and getattr(dset_metadata, "n_spatial_dims", 2) != 2:
            raise NotImplementedError(f"n_spatial_dims = {dset_metadata.n_spatial_dims} is out of scope: the HIP path serves 2-D fields")
        if not 2 <= depth <= 5:
            raise ValueError(f"depth must be 2..5 (Conv1 and Conv2 always exist, Conv5 is the deepest), got {depth}")
        n_channel = dset_metadata.n_fields if dset_metadata else 5
        dim_in = n_channel * in_T
        dim_out = n_channel * out_T
        self.out_T = out_T
        self.depth = depth
        self.MaxPool = nn.MaxPool2d(kernel_size=2, stride=2)

        self.Conv1 = ConvBlock(dim_in, 64)
        self.Conv2 = ConvBlock(64, 128)
        if depth >= 3:
            self.Conv3 = ConvBlock(128, 256)
        if depth >= 4:
            self.Conv4 = ConvBlock(256, 512)
        if depth >= 5:
            self.Conv5 = ConvBlock(512, 1024)

        if depth >= 5:
            self.Up5 = UpConv(1024, 512)
            self.Att5 = AttentionBlock(F_g=512, F_l=512, n_coefficients=256)
            self.UpConv5 = ConvBlock(1024, 512)

        if depth >= 4:
            self.Up4 = UpConv(512, 256)
            self.Att4 = AttentionBlock(F_g=256, F_l=256, n_coefficients=128)
            self.UpConv4 = ConvBlock(512, 256)

        if depth >= 3:
            self.Up3 = UpConv(256, 128)
            self.Att3 = AttentionBlock(F_g=128, F_l=128, n_coefficients=64)
            self.UpConv3 = ConvBlock(256, 128)

        self.Up2 = UpConv(128, 64)
        self.Att2 = AttentionBlock(F_g=64, F_l=64, n_coefficients=32)
        self.UpConv2 = ConvBlock(128, 64)

        self.Conv = nn.Conv2d(64, dim_out, kernel_size=1, stride=1, padding=0)

        self.dim_in, self.dim_out = dim_in, dim_out
        self._cache = _PackCache()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, out_T, c, h, w)   (unet_att.py:126-175)."""
        inference_only(self, "AttentionUNet", WHY_INFERENCE_ONLY)
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, C, H, W), got {tuple(x.shape)}: 3-D fields are out of scope")
        b, t, c, h, w = x.shape
        if t * c != self.dim_in:
            raise ValueError(f"the input has t * c = {t} * {c} = {t * c} channels, Conv1 takes dim_in = n_fields * in_T = {self.dim_in}")
        div = 2 ** (self.depth - 1)
        if h % div or w % div:
            raise ValueError(f"H and W must be multiples of 2 ** (depth - 1) = {div} (the gates' skips would not match), got {h} x {w}")
        gpu_only(x, "AttentionUNet")
        compute = resolve_compute(self.compute)
        cur = x.detach().to(torch.float32).reshape(b, t * c, h, w).permute(0, 2, 3, 1).contiguous()       # b (t c) h w, channels last
        enc = [self.Conv1.run(cur, compute)]
        for i in range(2, self.depth + 1):
            enc.append(getattr(self, f"Conv{i}").run(enc[-1], compute, POOLED))          # MaxPool2d read by the staging loop
        d = enc[-1]                                                                         # the d4 / d3 / d2 fall-through of unet_att.py:152-166
        for i in range(self.depth, 1, -1):
            d = getattr(self, f"Up{i}").run(d, compute)                                    # Upsample read by the staging loop
            s = getattr(self, f"Att{i}").run(d, enc[i - 2], compute)
            d = getattr(self, f"UpConv{i}").run(s, compute, PLAIN, d)                      # cat((s, d)) read by the staging loop
        hc = site(compute, "head", BF16_SITES)
        pw = self._cache.get(("head", hc), [self.Conv.weight, self.Conv.bias], lambda: S.pack_linear_chunks(
            self.Conv.weight.detach().reshape(self.dim_out, 64).contiguous(), self.Conv.bias.detach(), hc))
        rows = d.view(b * h * w, 64)
        y = S.linear_chunks(rows if hc == L.F32 else rows.to(torch.bfloat16), pw)
        return y.view(b, h, w, self.dim_out // self.out_T, self.out_T).permute(0, 4, 3, 1, 2).contiguous()     # the channel index is (c t)
