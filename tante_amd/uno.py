"""UNO baseline on the HIP kernels  (reference models/uno.py, configs/uno.yaml).

Same constructor arguments, module tree (`fc`, `fc0`, `L0` .. `L6`, `fc1`, `fc2`; each `L*` an OperatorBlock_2D holding `conv`, a
SpectralConv2d_Uno with complex64 `weights1` / `weights2`, and `w`, a pointwise_op_2D with `conv`), `state_dict` keys / shapes and
forward contract (`b t c h w -> b 1 c h w`, the channel index read as (t c)) as the reference's models.UNO.  Every arithmetic step is a
C-ABI call of libtante_hip:
  fc, fc0, fc1, fc2     tante_gemm on the channels-last pixel rows, the GELU in its epilogue; fc2 reads [fc1 | fc] as two K-chunks through
                        the residual operand, so that concatenation is never written.
  L0 .. L6              tante_uno_block on channels-first planes: the truncated transforms, the resize tables of the pointwise path and
                        the 1 x 1 as MFMA products against host-built tables, the mode mix as a stream over weights1 / weights2 read in
                        place, sum + bias + GELU in the last store.  Input and output take an image stride, so L1 and L0 write straight
                        into the channel slice that L5 and L6 read, L4 / L5 / L6 write the slice in front of it, and fc0's output sits
                        behind L6's: the three concatenations of the blocks and the one with fc0 cost nothing.
torch allocates, makes the strided copies between rows and planes (the zero padding among them) and casts.

The tables (tante_hip.h has their layout) are built in float64 and rounded once, per (sizes, modes), and cached: the DFT twiddles in
closed form with the angle's integer part reduced exactly, the resize matrices A by resizing an identity on the CPU in float64
(F.interpolate is linear and separable: resize(X) = A_h X A_w^T).

In bf16 mode the four per-pixel linears take bf16 operands; the transforms, the mode mix and the 1 x 1 stay fp32.

Inference only.  Training, 3-D fields, Normalize=True, a pointwise_op_2D outside its block and sizes outside what tante_uno_block serves
raise NotImplementedError by name; a padded size whose blocks cannot hold their hard-coded modes raises ValueError where the reference
raises its shape error; there is no CPU fallback."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from . import stages as S
from .attn_backbone import _PackCache, resolve_compute
from .model_shell import ComputeSwitch, gpu_only, inference_only

MAX_DIM, MAX_CH, MAX_PLANES = 512, 512, 65535      # what tante_uno_block serves
_TABLES = {}
_RESIZE = {}
_GRIDS = {}


# ---- host side of the kernel: the tables ---------------------------------------------------------------------------------------------------
def resize_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """A (n_out, n_in) float64 with F.interpolate(x, bicubic, align_corners=True, antialias=True) along one axis = A x: an identity
    resized on the CPU, once per size pair."""
    key = (n_in, n_out)
    if key not in _RESIZE:
        eye = torch.eye(n_in, dtype=torch.float64).reshape(1, 1, n_in, n_in)
        out = torch.nn.functional.interpolate(eye, size=(n_in, n_out), mode="bicubic", align_corners=True, antialias=True)
        _RESIZE[key] = out.reshape(n_in, n_out).t().contiguous()
    return _RESIZE[key]


def _angles(freq: torch.Tensor, n: int) -> torch.Tensor:
    """2 pi freq[a] x / n for x < n, the product reduced modulo n in integers first -> (len(freq), n) float64."""
    prod = (freq.reshape(-1, 1).to(torch.int64) * torch.arange(n, dtype=torch.int64).reshape(1, -1)) % n
    return prod.double() * (2.0 * math.pi / n)


def band_rows(n: int, m1: int) -> torch.Tensor:
    """The rows [:m1] and [-m1:] of an n-row spectrum."""
    return torch.cat([torch.arange(m1), torch.arange(n - m1, n)])


def live_rows(Ho: int, m1: int) -> torch.Tensor:
    """0 for a top-band row of out_ft that the bottom band, written second, overwrites."""
    kout = band_rows(Ho, m1)
    live = torch.ones(2 * m1, dtype=torch.float64)
    live[:m1][kout[:m1] >= Ho - m1] = 0.0
    return live


def c2r_weights(Wo: int, m2: int) -> torch.Tensor:
    c = torch.full((m2,), 2.0, dtype=torch.float64)
    c[0] = 1.0
    if Wo % 2 == 0 and m2 > Wo // 2:
        c[Wo // 2] = 1.0
    return c


def table_layout(Hi: int, Wi: int, Ho: int, Wo: int, m1: int, m2: int, pointwise: bool):
    """tante_uno_table_layout -> ([(offset, rows, cols)] * 5, total floats, the 1 x 1 runs on the output grid)."""
    buf = (ctypes.c_int64 * 16)()
    L.check(L.lib().tante_uno_table_layout(Hi, Wi, Ho, Wo, m1, m2, int(pointwise), ctypes.cast(buf, ctypes.c_void_p)), "tante_uno_table_layout")
    total = int(L.lib().tante_uno_table_floats(Hi, Wi, Ho, Wo, m1, m2, int(pointwise)))
    return [(int(buf[3 * t]), int(buf[3 * t + 1]), int(buf[3 * t + 2])) for t in range(5)], total, bool(buf[15])


def block_tables(Hi: int, Wi: int, Ho: int, Wo: int, m1: int, m2: int, pointwise: bool) -> torch.Tensor:
    """The five tables of tante_uno_block, float64 rounded to fp32 once, one flat CPU tensor."""
    layout, total, down = table_layout(Hi, Wi, Ho, Wo, m1, m2, pointwise)
    J = 2 * m1
    l = torch.arange(m2)
    aw = _angles(l, Wi)
    t1 = torch.stack([torch.cos(aw), -torch.sin(aw)], dim=1).reshape(2 * m2, Wi) / (Hi * Wi)
    if pointwise and down:
        t1 = torch.cat([t1, resize_matrix(Wi, Wo)], dim=0)
    ah = _angles(band_rows(Hi, m1), Hi)
    t2 = torch.cat([torch.cat([torch.cos(ah), torch.sin(ah)], dim=1), torch.cat([-torch.sin(ah), torch.cos(ah)], dim=1)], dim=0)
    t3 = resize_matrix(Hi, Ho) if pointwise else torch.zeros(0, 0, dtype=torch.float64)
    bh = _angles(band_rows(Ho, m1), Ho).t() * 1.0                      # (Ho, J)
    live = live_rows(Ho, m1).reshape(1, J)
    ch, sh = torch.cos(bh) * live, torch.sin(bh) * live
    t4 = torch.cat([torch.cat([ch, -sh], dim=1), torch.cat([sh, ch], dim=1)], dim=0)
    bw = _angles(l, Wo).t()                                             # (Wo, m2)
    c = c2r_weights(Wo, m2).reshape(1, m2)
    t5 = torch.cat([c * torch.cos(bw), -c * torch.sin(bw)], dim=1)      # sin(0) = sin(pi x) = 0 exactly: the angle is reduced in integers
    if Wo % 2 == 0 and m2 > Wo // 2:
        t5[:, m2 + Wo // 2] = 0.0                                       # sin(pi x) in floating point is not 0; the c2r transform drops it
    if pointwise and not down:
        t5 = torch.cat([t5, resize_matrix(Wi, Wo)], dim=1)
    flat = torch.zeros(total, dtype=torch.float64)
    for (off, rows, cols), t in zip(layout, (t1, t2, t3, t4, t5)):
        if tuple(t.shape) != (rows, cols) and rows * cols:
            raise RuntimeError(f"table of {tuple(t.shape)} where the library lays out {(rows, cols)}")
        flat[off:off + rows * cols] = t.reshape(-1)
    return flat.float()


def _tables_on(device, *key) -> torch.Tensor:
    k = (str(device),) + key
    if k not in _TABLES:
        _TABLES[k] = block_tables(*key).to(device)
    return _TABLES[k]


def get_grid(h: int, w: int) -> torch.Tensor:
    """uno.py:271-280 as (h, w, 4) float64: sin x, sin y, cos x, cos y of linspace(0, 2 pi, size)."""
    gx = torch.linspace(0, 2 * math.pi, h, dtype=torch.float64).reshape(h, 1).expand(h, w)
    gy = torch.linspace(0, 2 * math.pi, w, dtype=torch.float64).reshape(1, w).expand(h, w)
    return torch.stack([torch.sin(gx), torch.sin(gy), torch.cos(gx), torch.cos(gy)], dim=-1)


def _grid_on(device, h: int, w: int, dtype: torch.dtype) -> torch.Tensor:
    k = (str(device), h, w, dtype)
    if k not in _GRIDS:
        _GRIDS[k] = get_grid(h, w).float().to(device=device, dtype=dtype)
    return _GRIDS[k]


def modes_fit(Hi: int, Wi: int, Ho: int, Wo: int, m1: int, m2: int) -> bool:
    """Whether the reference's slices x_ft[:, :, :m1, :m2] and out_ft[:, :, -m1:, :m2] have the weights' shape."""
    return m1 <= Hi and m1 <= Ho and m2 <= Wi // 2 + 1 and m2 <= Wo // 2 + 1


def uno_block_supported_py(B: int, Ci: int, Co: int, Hi: int, Wi: int, Ho: int, Wo: int, m1: int, m2: int, x_stride: int, out_stride: int) -> bool:
    """Python mirror of tante_uno_block_supported."""
    if not (1 <= Ci <= MAX_CH and 1 <= Co <= MAX_CH) or not all(1 <= d <= MAX_DIM for d in (Hi, Wi, Ho, Wo)):
        return False
    if m1 < 1 or m2 < 1 or not modes_fit(Hi, Wi, Ho, Wo, m1, m2):
        return False
    return 0 <= B and B * max(Ci, Co) <= MAX_PLANES and x_stride >= Ci * Hi * Wi and out_stride >= Co * Ho * Wo


def _planes(t: torch.Tensor, what: str):
    """(image stride, shape) of a channels-first fp32 tensor that may be a channel slice of a wider buffer."""
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{what} must be fp32 (n, C, H, W)")
    n, C, H, W = t.shape
    gpu_only(t, "UNO")
    if any(size > 1 and stride != want for size, stride, want in ((W, t.stride(3), 1), (H, t.stride(2), W), (C, t.stride(1), H * W))):
        raise RuntimeError(f"{what} must have dense channel planes (a channel slice of a channels-first buffer at most)")
    return (t.stride(0) if n > 1 else max(t.stride(0), C * H * W)), (n, C, H, W)


def uno_block(x: torch.Tensor, out: torch.Tensor, m1: int, m2: int, w1: torch.Tensor, w2: torch.Tensor, pw_w: Optional[torch.Tensor],
              pw_b: Optional[torch.Tensor], gelu: bool, name: str = "OperatorBlock_2D") -> torch.Tensor:
    """tante_uno_block: x (n, Ci, Hi, Wi) -> out (n, Co, Ho, Wo), both fp32 channels-first, either a channel slice of a wider buffer."""
    xs, (n, Ci, Hi, Wi) = _planes(x, "the input")
    os_, (no, Co, Ho, Wo) = _planes(out, "the output")
    if no != n:
        raise RuntimeError(f"{n} input and {no} output images")
    if tuple(w1.shape) != (Ci, Co, m1, m2) or tuple(w2.shape) != (Ci, Co, m1, m2) or w1.dtype != torch.complex64 or w2.dtype != torch.complex64:
        raise RuntimeError(f"weights1 / weights2 must be complex64 {(Ci, Co, m1, m2)}")
    if not modes_fit(Hi, Wi, Ho, Wo, m1, m2):
        raise ValueError(f"{name}: a {Hi} x {Wi} -> {Ho} x {Wo} block cannot hold its {m1} x {m2} modes (the reference fails at the band's shape)")
    if not uno_block_supported_py(n, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, xs, os_):
        raise NotImplementedError(f"{name}: {n} images, {Ci} -> {Co} channels, {Hi} x {Wi} -> {Ho} x {Wo} is out of scope: tante_uno_block serves "
                                  f"up to {MAX_CH} channels, {MAX_DIM} x {MAX_DIM} planes and {MAX_PLANES} (image, channel) planes per call")
    pw = pw_w is not None
    r1, r2 = torch.view_as_real(w1.detach()), torch.view_as_real(w2.detach())
    K._dev(r1, r2, pw_w, pw_b)
    lib = L.lib()
    tables = _tables_on(x.device, Hi, Wi, Ho, Wo, m1, m2, pw)
    work, nbytes = K.workspace(lib.tante_uno_block_workspace_bytes(n, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, int(pw)), x.device)
    L.check(lib.tante_uno_block(x.data_ptr(), xs, n, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, K._p(tables), K._p(r1), K._p(r2), K._p(pw_w), K._p(pw_b),
                                L.ACT_GELU_ERF if gelu else L.ACT_NONE, out.data_ptr(), os_, K._p(work), nbytes, K._stream()), "tante_uno_block")
    return out


# ---- the reference's modules ---------------------------------------------------------------------------------------------------------------
WHY_INFERENCE_ONLY = "the backward of the transforms and of the mode mix are kernels of their own that are not built"


def _fp32_planes(x: torch.Tensor) -> torch.Tensor:
    gpu_only(x, "UNO")
    if x.dim() != 4:
        raise ValueError(f"expected (n, C, H, W), got {tuple(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


class SpectralConv2d_Uno(nn.Module):
    """uno.py:58-138: the truncated, resampling Fourier layer."""

    def __init__(self, in_codim, out_codim, dim1, dim2, modes1=None, modes2=None):
        super().__init__()
        in_codim, out_codim = int(in_codim), int(out_codim)
        self.in_channels, self.out_channels = in_codim, out_codim
        self.dim1, self.dim2 = dim1, dim2
        if modes1 is not None:
            self.modes1, self.modes2 = modes1, modes2
        else:
            self.modes1, self.modes2 = dim1 // 2 - 1, dim2 // 2
        self.scale = (1 / (2 * in_codim)) ** (1.0 / 2.0)
        self.weights1 = nn.Parameter(self.scale * torch.randn(in_codim, out_codim, self.modes1, self.modes2, dtype=torch.cfloat))
        self.weights2 = nn.Parameter(self.scale * torch.randn(in_codim, out_codim, self.modes1, self.modes2, dtype=torch.cfloat))

    def forward(self, x: torch.Tensor, dim1=None, dim2=None) -> torch.Tensor:
        """(n, Ci, Hi, Wi) -> (n, Co, dim1, dim2).  Inference only."""
        inference_only(self, "UNO", WHY_INFERENCE_ONLY)
        if dim1 is not None:
            self.dim1, self.dim2 = dim1, dim2
        xp = _fp32_planes(x)
        out = torch.empty(xp.shape[0], self.out_channels, int(self.dim1), int(self.dim2), dtype=torch.float32, device=xp.device)
        return uno_block(xp, out, self.modes1, self.modes2, self.weights1, self.weights2, None, None, False, "SpectralConv2d_Uno").to(x.dtype)


class pointwise_op_2D(nn.Module):
    """uno.py:140-173: the 1 x 1 convolution and the antialiased bicubic resize.  It runs inside tante_uno_block only."""

    def __init__(self, in_codim, out_codim, dim1, dim2):
        super().__init__()
        self.conv = nn.Conv2d(int(in_codim), int(out_codim), 1)
        self.dim1, self.dim2 = int(dim1), int(dim2)

    def forward(self, x, dim1=None, dim2=None):
        raise NotImplementedError("pointwise_op_2D alone is out of scope: its 1 x 1 and its resize are launches of tante_uno_block; call the "
                                  "OperatorBlock_2D that owns it")


class OperatorBlock_2D(nn.Module):
    """uno.py:18-56: gelu(SpectralConv2d_Uno(x) + pointwise_op_2D(x))."""

    def __init__(self, in_codim, out_codim, dim1, dim2, modes1, modes2, Normalize=False, Non_Lin=True):
        super().__init__()
        if Normalize:
            raise NotImplementedError("OperatorBlock_2D(Normalize=True) is out of scope: InstanceNorm2d behind the block is not built (UNO's "
                                      "constructor never asks for it)")
        self.conv = SpectralConv2d_Uno(in_codim, out_codim, dim1, dim2, modes1, modes2)
        self.w = pointwise_op_2D(in_codim, out_codim, dim1, dim2)
        self.normalize = Normalize
        self.non_lin = Non_Lin

    def run(self, x: torch.Tensor, out: torch.Tensor, name: str = "OperatorBlock_2D") -> torch.Tensor:
        """x (n, Ci, Hi, Wi) -> out (n, Co, Ho, Wo), fp32 channels-first, either one a channel slice of a wider buffer."""
        c = self.w.conv
        return uno_block(x, out, self.conv.modes1, self.conv.modes2, self.conv.weights1, self.conv.weights2,
                         c.weight.detach().reshape(c.out_channels, c.in_channels), c.bias.detach(), bool(self.non_lin), name)

    def forward(self, x: torch.Tensor, dim1=None, dim2=None) -> torch.Tensor:
        """(n, Ci, Hi, Wi) -> (n, Co, dim1, dim2).  Inference only."""
        inference_only(self, "UNO", WHY_INFERENCE_ONLY)
        if dim1 is None:
            dim1, dim2 = self.conv.dim1, self.conv.dim2
        self.conv.dim1, self.conv.dim2 = dim1, dim2
        xp = _fp32_planes(x)
        out = torch.empty(xp.shape[0], self.conv.out_channels, int(dim1), int(dim2), dtype=torch.float32, device=xp.device)
        return self.run(xp, out).to(x.dtype)


BLOCK_MODES = ((32, 33), (8, 9), (4, 5), (4, 5), (4, 5), (8, 9), (32, 32))     # uno.py:197-221, hard-coded
BLOCK_DIVS = (4, 16, 32, 32, 16, 4, 1)                                         # uno.py:243-253: the output grid is D // div per axis


def block_sizes(D1: int, D2: int):
    """[(Hi, Wi, Ho, Wo)] of L0 .. L6 on a padded D1 x D2 grid; ValueError names the first block that cannot hold its modes."""
    out, hi, wi = [], D1, D2
    for i, (div, (m1, m2)) in enumerate(zip(BLOCK_DIVS, BLOCK_MODES)):
        ho, wo = D1 // div, D2 // div
        if not modes_fit(hi, wi, ho, wo, m1, m2):
            raise ValueError(f"L{i}: a padded {D1} x {D2} grid gives it {hi} x {wi} -> {ho} x {wo}, which cannot hold its {m1} x {m2} modes "
                             f"(the reference needs H >= 128 and W >= 256 after padding)")
        out.append((hi, wi, ho, wo))
        hi, wi = ho, wo
    return out


class UNO(ComputeSwitch, nn.Module):
    """models/uno.py:175-280 -- same constructor, attributes, parameters and forward contract."""

    def __init__(self, in_T, dset_metadata=None, width=32, pad=0, factor=1):
        super().__init__()
        if dset_metadata is not None and getattr(dset_metadata, "n_spatial_dims", 2) != 2:
            raise NotImplementedError(f"n_spatial_dims = {dset_metadata.n_spatial_dims} is out of scope: the HIP path serves 2-D fields")
        n_channel = dset_metadata.n_fields if dset_metadata else 4
        dim_in = n_channel * in_T
        dim_out = n_channel
        self.in_width = dim_in
        self.width = width
        self.factor = factor
        self.padding = pad
        self.fc = nn.Linear(self.in_width + 4, 16)
        self.fc0 = nn.Linear(16, self.width)
        f = factor
        self.L0 = OperatorBlock_2D(self.width, 2 * f * self.width, 64, 64, 32, 33)
        self.L1 = OperatorBlock_2D(2 * f * self.width, 4 * f * self.width, 16, 16, 8, 9)
        self.L2 = OperatorBlock_2D(4 * f * self.width, 8 * f * self.width, 8, 8, 4, 5)
        self.L3 = OperatorBlock_2D(8 * f * self.width, 8 * f * self.width, 8, 8, 4, 5)
        self.L4 = OperatorBlock_2D(8 * f * self.width, 4 * f * self.width, 16, 16, 4, 5)
        self.L5 = OperatorBlock_2D(8 * f * self.width, 2 * f * self.width, 64, 64, 8, 9)
        self.L6 = OperatorBlock_2D(4 * f * self.width, self.width, 256, 256, 32, 32)
        self.fc1 = nn.Linear(2 * self.width, 3 * self.width)
        self.fc2 = nn.Linear(3 * self.width + 16, dim_out)
        self.dim_out = dim_out
        self._cache = _PackCache()

    def _linears(self, compute: int):
        ps = [p for m in (self.fc, self.fc0, self.fc1, self.fc2) for p in (m.weight, m.bias)]
        k1 = 3 * self.width

        def build():
            w2 = self.fc2.weight.detach()
            return (S.pack_linear_chunks(self.fc.weight.detach(), self.fc.bias.detach(), compute),
                    S.pack_linear_chunks(self.fc0.weight.detach(), self.fc0.bias.detach(), compute),
                    S.pack_linear_chunks(self.fc1.weight.detach(), self.fc1.bias.detach(), compute),
                    S.pack_linear_chunks(w2[:, :k1].contiguous(), self.fc2.bias.detach(), compute),
                    S.pack_linear_chunks(w2[:, k1:].contiguous(), None, compute))
        return self._cache.get(("linears", compute), ps, build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, t, c, h, w) -> (b, 1, c, h, w)   (uno.py:227-269)."""
        inference_only(self, "UNO", WHY_INFERENCE_ONLY)
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, C, H, W), got {tuple(x.shape)}: 3-D fields are out of scope")
        b, t, c, h, w = x.shape
        tc = t * c
        if tc != self.in_width:
            raise ValueError(f"the input has t * c = {t} * {c} = {tc} channels, fc takes n_fields * in_T = {self.in_width} (+ 4 grid channels)")
        p, wd, fw = self.padding, self.width, self.factor * self.width
        D1, D2 = h + 2 * p, w + 2 * p
        sizes = block_sizes(D1, D2)
        if D1 > MAX_DIM or D2 > MAX_DIM or 8 * fw > MAX_CH or b * 8 * fw > MAX_PLANES:
            raise NotImplementedError(f"tante_amd.UNO: {b} images of {D1} x {D2} (padded) at {8 * fw} channels are out of scope: tante_uno_block serves "
                                      f"up to {MAX_DIM} x {MAX_DIM} planes, {MAX_CH} channels and {MAX_PLANES} (image, channel) planes per call")
        gpu_only(x, "UNO")
        compute = resolve_compute(self.compute)
        adt = K.act_torch_dtype(compute)
        fc, fc0, fc1, fc2a, fc2b = self._linears(compute)
        dev = x.device
        M = b * h * w
        rows = torch.empty(b, h, w, tc + 4, dtype=adt, device=dev)                     # [x as (t c) | grid]: two strided copies, no cat
        rows[..., :tc].unflatten(-1, (t, c)).copy_(x.detach().permute(0, 3, 4, 1, 2))
        rows[..., tc:].copy_(_grid_on(dev, h, w, adt))
        x_fc = S.linear_chunks(rows.view(M, tc + 4), fc, adt, L.ACT_GELU_ERF)          # (M, 16)
        x_fc0 = S.linear_chunks(x_fc, fc0, torch.float32, L.ACT_GELU_ERF)              # (M, width)
        new = torch.zeros if p else torch.empty
        c6 = new(b, 2 * wd, D1, D2, dtype=torch.float32, device=dev)                   # [L6 | fc0, zero padded]
        c6[:, wd:, p:p + h, p:p + w].copy_(x_fc0.view(b, h, w, wd).permute(0, 3, 1, 2))
        b5 = torch.empty(b, 4 * fw, sizes[0][2], sizes[0][3], dtype=torch.float32, device=dev)      # [L5 | L0]
        a4 = torch.empty(b, 8 * fw, sizes[1][2], sizes[1][3], dtype=torch.float32, device=dev)      # [L4 | L1]
        c2 = torch.empty(b, 8 * fw, sizes[2][2], sizes[2][3], dtype=torch.float32, device=dev)
        c3 = torch.empty(b, 8 * fw, sizes[3][2], sizes[3][3], dtype=torch.float32, device=dev)
        self.L0.run(c6[:, wd:], b5[:, 2 * fw:], "L0")
        self.L1.run(b5[:, 2 * fw:], a4[:, 4 * fw:], "L1")
        self.L2.run(a4[:, 4 * fw:], c2, "L2")
        self.L3.run(c2, c3, "L3")
        self.L4.run(c3, a4[:, :4 * fw], "L4")
        self.L5.run(a4, b5[:, :2 * fw], "L5")
        self.L6.run(b5, c6[:, :wd], "L6")
        r6 = torch.empty(b, h, w, 2 * wd, dtype=adt, device=dev)
        r6.copy_(c6[:, :, p:p + h, p:p + w].permute(0, 2, 3, 1))                       # the crop, to rows
        x_fc1 = S.linear_chunks(r6.view(M, 2 * wd), fc1, adt, L.ACT_GELU_ERF)          # (M, 3 width)
        y = S.linear_chunks(x_fc1, fc2a)
        S.linear_chunks(x_fc, fc2b, residual=y, out=y)                                 # [fc1 | fc] as two K-chunks
        return y.view(b, h, w, self.dim_out).permute(0, 3, 1, 2).unsqueeze(1).contiguous().to(x.dtype if x.dtype.is_floating_point else torch.float32)
