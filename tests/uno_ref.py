"""Float64 restatement of the reference's models/uno.py from the mathematics, on state dicts -- channels first, as the reference's blocks.

The reference cannot itself run in float64 (SpectralConv2d_Uno hard-codes a cfloat out_ft), so this restatement is the float64 truth; the
fixtures tests/golden/g23_uno_* pin it to the reference's own fp32 outputs (err32 <= 5e-6, the reference's fp32 rounding), and the GPU
suite compares the kernels with it.

The spectral convolution has two forms: `spectral_table`, the explicit sums over the kept modes only (the form the kernels implement:
truncated DFT tables, the band rows kin / kout, `live` for a top-band row the bottom band overwrites, the c2r weights c), and
`spectral_fft`, the reference's own steps on torch.fft in complex128.  The table form is the one the restatement uses; the CPU suite holds
the other to it.

`rule_state_dict` / `rule_input`: the whole-model fixtures store neither weights nor inputs (a width-4 model is 1.6 M spectral
parameters); both come from a rule that the generator and the tests apply identically: integer arithmetic only up to a 24-bit uniform
value, which is exact in fp32.  `scales`: one power of two per block on weights1 / weights2 (exact in fp32), which the generator chooses
so that the spectral path carries weight beside the pointwise one (at the default initialisation it is 0.1 .. 0.015 of it)."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

_M32 = 0xFFFFFFFF
BLOCK_MODES = ((32, 33), (8, 9), (4, 5), (4, 5), (4, 5), (8, 9), (32, 32))
BLOCK_DIVS = (4, 16, 32, 32, 16, 4, 1)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------
def rule_uniform(key: str, n: int) -> np.ndarray:
    """n values in [-0.5, 0.5), multiples of 2^-24, from a 32-bit hash of (crc32(key), element index): integer arithmetic only."""
    h0 = (zlib.crc32(key.encode()) * 0x9E3779B1 + 0x61C88647) & _M32
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x85EBCA6B) + np.uint64(h0)) & np.uint64(_M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(_M32)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(_M32)
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(8)).astype(np.float64) / float(1 << 24) - 0.5


def rule_entry(key: str, shape, scale: float = 1.0) -> torch.Tensor:
    """One entry of the state dict.  weights1 / weights2 (Ci, Co, m1, m2) complex64: (u + i u') sqrt(6 / Ci), the reference's standard
    deviation, times `scale`; real weights u * 2 sqrt(3 / fan_in); biases 0.2 u."""
    shape = tuple(int(s) for s in shape)
    leaf = key.split(".")[-1]
    n = int(np.prod(shape)) if shape else 1
    if leaf in ("weights1", "weights2"):
        a = math.sqrt(6.0 / shape[0])
        re = torch.from_numpy((rule_uniform(key + ".re", n) * a).astype(np.float32).reshape(shape))
        im = torch.from_numpy((rule_uniform(key + ".im", n) * a).astype(np.float32).reshape(shape))
        return torch.complex(re, im) * float(scale)
    u = rule_uniform(key, n)
    if leaf == "weight":
        v = u * (2.0 * math.sqrt(3.0 / int(np.prod(shape[1:]))))
    elif leaf == "bias":
        v = 0.2 * u
    else:
        raise KeyError(key)
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def rule_state_dict(keys, shapes, scales=None):
    """scales: None, or the seven per-block factors of L0 .. L6's weights1 / weights2 (powers of two)."""
    out = {}
    for k, s in zip(keys, shapes):
        sc = 1.0
        if scales is not None and k.split(".")[-1] in ("weights1", "weights2"):
            sc = float(scales[int(k.split(".")[0][1:])])
        out[k] = rule_entry(k, s, sc)
    return out


def rule_input(name: str, shape) -> torch.Tensor:
    """A model fixture's input (b, t, c, h, w) fp32: 2 u + 0.25."""
    shape = tuple(int(s) for s in shape)
    return torch.from_numpy((2.0 * rule_uniform("x." + name, int(np.prod(shape))) + 0.25).astype(np.float32).reshape(shape))


# ---- the mathematics -------------------------------------------------------------------------------------------------------------------------
def _phase(freq, n, sign):
    """e^{sign 2 pi i freq[a] x / n} -> (len(freq), n) complex128, the product reduced modulo n in integers."""
    prod = (torch.as_tensor(freq, dtype=torch.int64).reshape(-1, 1) * torch.arange(n, dtype=torch.int64).reshape(1, -1)) % n
    ang = prod.double() * (2.0 * math.pi / n)
    return torch.complex(torch.cos(ang), sign * torch.sin(ang))


def band_rows(n, m1):
    return list(range(m1)) + list(range(n - m1, n))


def spectral_table(x, w1, w2, Ho, Wo):
    """SpectralConv2d_Uno.forward as sums over the kept modes: x (B, Ci, Hi, Wi) float64, w1 / w2 (Ci, Co, m1, m2) complex ->
    (B, Co, Ho, Wo) float64."""
    B, Ci, Hi, Wi = x.shape
    m1, m2 = w1.shape[2], w1.shape[3]
    if m1 > Hi or m1 > Ho or m2 > Wi // 2 + 1 or m2 > Wo // 2 + 1:
        raise ValueError(f"a {Hi} x {Wi} -> {Ho} x {Wo} layer cannot hold {m1} x {m2} modes")
    xc = x.to(torch.complex128)
    P = torch.einsum("bihw,lw->bihl", xc, _phase(range(m2), Wi, -1.0))
    X = torch.einsum("jh,bihl->bijl", _phase(band_rows(Hi, m1), Hi, -1.0), P) / (Hi * Wi)
    Wt = torch.cat([w1, w2], dim=2).to(torch.complex128)
    kout = band_rows(Ho, m1)
    live = torch.tensor([0.0 if (j < m1 and kout[j] >= Ho - m1) else 1.0 for j in range(2 * m1)], dtype=torch.float64)
    Y = torch.einsum("bijl,iojl->bojl", X, Wt) * live.reshape(1, 1, -1, 1)
    Z = torch.einsum("jy,bojl->boyl", _phase(kout, Ho, 1.0), Y)
    c = torch.full((m2,), 2.0, dtype=torch.float64)
    c[0] = 1.0
    if Wo % 2 == 0 and m2 > Wo // 2:
        c[Wo // 2] = 1.0
    return torch.einsum("lx,boyl->boyx", _phase(range(m2), Wo, 1.0) * c.reshape(-1, 1), Z).real


def spectral_fft(x, w1, w2, Ho, Wo):
    """The reference's own steps (uno.py:112-138) in complex128."""
    B = x.shape[0]
    m1, m2 = w1.shape[2], w1.shape[3]
    w1, w2 = w1.to(torch.complex128), w2.to(torch.complex128)
    x_ft = torch.fft.rfft2(x.double(), norm="forward")
    out_ft = torch.zeros(B, w1.shape[1], Ho, Wo // 2 + 1, dtype=torch.complex128)
    out_ft[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, :m1, :m2], w1)
    out_ft[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, -m1:, :m2], w2)
    return torch.fft.irfft2(out_ft, s=(Ho, Wo), norm="forward")


def pointwise(x, weight, bias, Ho, Wo):
    """pointwise_op_2D.forward (uno.py:154-173) in float64."""
    y = F.conv2d(x.double(), weight.double().reshape(weight.shape[0], -1, 1, 1), bias.double())
    return F.interpolate(y, size=(Ho, Wo), mode="bicubic", align_corners=True, antialias=True)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(x, sd, p, Ho, Wo, parts=None, spectral=spectral_table, no_spectral=False):
    """OperatorBlock_2D.forward at prefix p ("L0." or ""); parts: a list that receives (spectral, pointwise)."""
    s = spectral(x.double(), sd[p + "conv.weights1"], sd[p + "conv.weights2"], Ho, Wo)
    if no_spectral:
        s = torch.zeros_like(s)
    w = pointwise(x, sd[p + "w.conv.weight"], sd[p + "w.conv.bias"], Ho, Wo)
    if parts is not None:
        parts.append((s, w))
    return gelu(s + w)


def get_grid(h, w):
    gx = torch.linspace(0, 2 * math.pi, h, dtype=torch.float64).reshape(h, 1).expand(h, w)
    gy = torch.linspace(0, 2 * math.pi, w, dtype=torch.float64).reshape(1, w).expand(h, w)
    return torch.stack([torch.sin(gx), torch.sin(gy), torch.cos(gx), torch.cos(gy)], dim=-1)


def linear(x, sd, p, r16=False):
    w, b = sd[p + "weight"].double(), sd[p + "bias"].double()
    if r16:
        x, w = x.float().to(torch.bfloat16).double(), w.float().to(torch.bfloat16).double()
    return x @ w.T + b


def model(x, sd, pad=0, parts=None, spectral=spectral_table, zero_block=None):
    """UNO.forward (uno.py:227-269): x (b, t, c, h, w) -> (b, 1, c, h, w) float64.  zero_block: the block whose spectral path is removed."""
    b, t, c, h, w = x.shape
    rows = torch.cat([x.double().permute(0, 3, 4, 1, 2).reshape(b, h, w, t * c), get_grid(h, w).expand(b, h, w, 4)], dim=-1)
    x_fc = gelu(linear(rows, sd, "fc."))
    x_fc0 = gelu(linear(x_fc, sd, "fc0.")).permute(0, 3, 1, 2)
    x_fc0 = F.pad(x_fc0, [pad, pad, pad, pad])
    D1, D2 = x_fc0.shape[-2], x_fc0.shape[-1]

    def run(i, v):
        return block(v, sd, f"L{i}.", D1 // BLOCK_DIVS[i], D2 // BLOCK_DIVS[i], parts, spectral, zero_block == i)
    c0 = run(0, x_fc0)
    c1 = run(1, c0)
    c2 = run(2, c1)
    c3 = run(3, c2)
    c4 = torch.cat([run(4, c3), c1], dim=1)
    c5 = torch.cat([run(5, c4), c0], dim=1)
    c6 = torch.cat([run(6, c5), x_fc0], dim=1)
    if pad:
        c6 = c6[..., pad:-pad, pad:-pad]
    x_fc1 = gelu(linear(c6.permute(0, 2, 3, 1), sd, "fc1."))
    out = linear(torch.cat([x_fc1, x_fc], dim=3), sd, "fc2.")
    return out.permute(0, 3, 1, 2).unsqueeze(1)


def rms(t):
    return float(torch.sqrt((t.double() ** 2).mean()))


def err(y, ref):
    """max(rel L2, max / 2), the project's parity figure."""
    y, ref = y.double(), ref.double()
    return max(float((y - ref).norm() / ref.norm()), float((y - ref).abs().max() / ref.abs().max()) / 2)
