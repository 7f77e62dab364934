"""Float64 restatement of the AFNO filter, block, model and re-fed rollout with the soft threshold's decisions given from outside, for the
gradient tests of the trainable AFNO (tests/test_afno_train_cpu.py, tests/test_hip_afno_train.py).  Built from tests/afno_ref.py's
pieces (dft_matrix, block_linear, gelu, layer_norm), statement for statement as afno_ref.spectrum / afno_filter / block / model compute,
with one change: the threshold is  Y = (Yp - lam sign(Yp)) keep  for a constant mask `keep`, so autograd yields dYp = dY keep.  With
keep = |Yp| > lam this is afno_ref's own arithmetic, forward and backward.

Why the decisions are restated: the gradient of the soft threshold jumps at +-lam, and among 10^4 - 10^5 pre-threshold values of size
0.04 the closest lies 1e-8 - 3e-7 from +-lam, below what fp32 resolves.  A kernel that evaluates Yp in fp32 decides a few of those the
other way, correctly for its own forward.  So inside the narrow band  S = {| |Yp| - lam | < BAND}  the reference takes the kernel's
decision, outside it its own, and the tests assert that the two agree everywhere outside the band and that the band is small."""
import math

import torch

import afno_ref as R

DT, CDT = R.DT, R.CDT
BAND = 1e-5          # absolute distance from the threshold, on values of size 0.04
BAND_SHARE = 5e-3    # at most this share of the thresholded values may lie inside the band


def kept_modes(H: int, W: int):
    """(Lc, Kc): the entries of axis 2 / axis 1 of the spectrum that the swapped-size inverse reads."""
    return min(H, W), min(H // 2 + 1, W // 2 + 1)


def pre_threshold(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """-> Yp (b, H//2+1, W, C) complex128: afno_ref.spectrum up to the soft threshold."""
    b, H, W, C = x.shape
    X = torch.einsum("lw,bhwc->bhlc", R.dft_matrix(W, -1), x.to(CDT))
    X = torch.einsum("kh,bhlc->bklc", R.dft_matrix(H, -1)[: H // 2 + 1], X)
    U = R.block_linear(X, w1)
    V = torch.complex(R.gelu(U.real), R.gelu(U.imag))
    return R.block_linear(V, w2)


def keep64(Yp: torch.Tensor, lam: float):
    """The float64 decisions (real part, imaginary part), bool, Yp's shape."""
    return Yp.real.abs() > lam, Yp.imag.abs() > lam


def band(Yp: torch.Tensor, lam: float):
    return (Yp.real.abs() - lam).abs() < BAND, (Yp.imag.abs() - lam).abs() < BAND


def restrict(t: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """(b, H//2+1, W, C) -> the part the inverse reads, (b, Kc, Lc, C)."""
    Lc, Kc = kept_modes(H, W)
    return t[:, :Kc, :Lc]


def band_share(Yp: torch.Tensor, lam: float, H: int, W: int) -> float:
    """Share of the thresholded values the inverse reads (real and imaginary parts counted separately) that lie inside the band."""
    sr, si = band(Yp, lam)
    sr, si = restrict(sr, H, W), restrict(si, H, W)
    return float((sr.sum() + si.sum()).item()) / (2 * sr.numel())


def kernel_masks(keep: torch.Tensor):
    """The kernel's record (B, Lc, Kc, 2, C) uint8 -> (real, imaginary) bool masks (B, Kc, Lc, C)."""
    k = keep.cpu().bool().permute(0, 2, 1, 3, 4)
    return k[:, :, :, 0], k[:, :, :, 1]


class Restated:
    """mask_fn of the functions below: call i takes the kernel's i-th record inside the band and float64's decision outside, and keeps
    what the tests assert: `outside_mismatch` (decisions that differ outside the band; must be 0) and `shares` (band share per call)."""

    def __init__(self, records, lam: float):
        self.records, self.lam, self.i = list(records), lam, 0
        self.outside_mismatch, self.shares, self.flipped = 0, [], 0

    def __call__(self, Yp: torch.Tensor, H: int, W: int):
        kr, ki = keep64(Yp, self.lam)
        sr, si = band(Yp, self.lam)
        gr, gi = kernel_masks(self.records[self.i])
        self.i += 1
        out = []
        for k64, s, g in ((kr, sr, gr), (ki, si, gi)):
            k64r, sr_ = restrict(k64, H, W), restrict(s, H, W)
            assert g.shape == k64r.shape, (g.shape, k64r.shape)
            self.outside_mismatch += int(((g != k64r) & ~sr_).sum())
            self.flipped += int(((g != k64r) & sr_).sum())
            m = k64.clone()
            restrict(m, H, W)[...] = torch.where(sr_, g, k64r)
            out.append(m)
        self.shares.append(band_share(Yp, self.lam, H, W))
        return out[0], out[1]


def afno_filter(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, lam: float, mask_fn=None) -> torch.Tensor:
    """x (b, H, W, C) -> (b, W, H, C) float64: afno_ref.afno_filter with the threshold's decisions from mask_fn(Yp.detach(), H, W) ->
    (keep_re, keep_im) of Yp's shape (default: float64's own)."""
    x = x.to(DT)
    b, H, W, C = x.shape
    Yp = pre_threshold(x, w1, w2)
    kr, ki = (mask_fn or (lambda y, h, w: keep64(y, lam)))(Yp.detach(), H, W)
    Y = torch.complex((Yp.real - lam * torch.sign(Yp.real).detach()) * kr.to(DT), (Yp.imag - lam * torch.sign(Yp.imag).detach()) * ki.to(DT))
    # from here on: afno_ref.afno_filter, statement for statement
    Lc = min(W, H)
    Ypad = torch.zeros(b, H // 2 + 1, H, C, dtype=CDT)
    Ypad[:, :, :Lc] = Y[:, :, :Lc]
    Z = torch.einsum("nl,bklc->bknc", R.dft_matrix(H, +1), Ypad)
    Kn = W // 2 + 1
    Kc = min(H // 2 + 1, Kn)
    Zp = torch.zeros(b, Kn, H, C, dtype=CDT)
    Zp[:, :Kc] = Z[:, :Kc]
    k = torch.arange(Kn, dtype=DT)
    n = torch.arange(W, dtype=DT)
    ang = 2.0 * math.pi * torch.outer(n, k) / W
    once = (k == 0) | ((W % 2 == 0) & (k == W // 2))
    ck = torch.where(once, torch.ones_like(k), 2.0 * torch.ones_like(k))
    Zre = Zp.real
    Zim = torch.where(once[None, :, None, None], torch.zeros_like(Zp.imag), Zp.imag)
    cosm, sinm = torch.cos(ang) * ck / math.sqrt(W), torch.sin(ang) * ck / math.sqrt(W)
    return torch.einsum("nk,bkhc->bnhc", cosm, Zre) - torch.einsum("nk,bkhc->bnhc", sinm, Zim)


def block(x: torch.Tensor, sd: dict, pre: str, lam: float, mask_fn=None, eps: float = 1e-6) -> torch.Tensor:
    """afno_ref.block on tensors that may require grad (sd's entries are float64 leaves)."""
    n1 = R.layer_norm(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    f = afno_filter(n1, sd[pre + "filter.cmlp.0.weight"], sd[pre + "filter.cmlp.2.weight"], lam, mask_fn)
    x = f.transpose(1, 2) + x
    n2 = R.layer_norm(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    h = R.gelu(n2 @ sd[pre + "mlp.fc1.weight"].T + sd[pre + "mlp.fc1.bias"])
    return h @ sd[pre + "mlp.fc2.weight"].T + sd[pre + "mlp.fc2.bias"] + x


def model(x: torch.Tensor, sd: dict, patch: int, lam: float = 0.01, mask_fn=None) -> torch.Tensor:
    """afno_ref.model with the masks of every block call from mask_fn, in call order."""
    b, t, c, h, w = x.shape
    p = patch
    Hp, Wp = h // p, w // p
    we = sd["patch_embed.weight"]
    C = we.shape[0]
    pt = x.reshape(b, t * c, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).reshape(b, Hp, Wp, t * c * p * p)
    y = pt @ we.reshape(C, -1).T + sd["patch_embed.bias"] + sd["pos_embed"]
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        y = block(y, sd, f"blocks.{i}.", lam, mask_fn)
        i += 1
    wd = sd["patch_debed.weight"]
    o = torch.einsum("bhwk,kcij->bchiwj", y, wd).reshape(b, wd.shape[1], h, w) + sd["patch_debed.bias"][None, :, None, None]
    return o.unsqueeze(1)


def rollout(x: torch.Tensor, sd: dict, patch: int, n_steps: int, lam: float = 0.01, mask_fn=None) -> torch.Tensor:
    moving, out = x, []
    for _ in range(n_steps):
        y = model(moving, sd, patch, lam, mask_fn)
        out.append(y)
        moving = torch.cat([moving[:, 1:], y], dim=1)
    return torch.cat(out, dim=1)


def leaves(sd: dict) -> dict:
    """A state dict as float64 leaves that require grad."""
    return {k: v.detach().to(DT).clone().requires_grad_(True) for k, v in sd.items()}


# ---- the cases of the filter tests: (B, H, W, C, bs), seeds and weight scale as tests/test_hip_afno.py draws them ------------------------
FILTER_CASES = [(2, 7, 9, 40, 8), (1, 12, 5, 48, 24), (1, 5, 12, 48, 24), (1, 64, 33, 48, 24), (1, 33, 64, 128, 64), (3, 1, 1, 16, 16),
                (1, 5, 12, 80, 16), (1, 12, 5, 80, 16)]


def filter_case(B, H, W, C, bs):
    """-> x, residual, w1, w2, dout (fp32, CPU) of one filter case."""
    gen = torch.Generator().manual_seed(H * 100 + W)
    s = 0.04 * (32.0 / bs) ** 0.5 * (3.0 if H * W == 1 else 1.0)
    w1, w2 = s * torch.randn(C // bs, bs, bs, 2, generator=gen), s * torch.randn(C // bs, bs, bs, 2, generator=gen)
    x = torch.randn(B, H, W, C, generator=gen)
    res = torch.randn(B, H, W, C, generator=gen)
    dout = torch.randn(B, H, W, C, generator=gen)
    return x, res, w1, w2, dout


MODEL_KW = dict(in_T=2, hidden_dim=32, n_blocks=2, cmlp_diagonal_blocks=2, patch_size=4)
MODEL_RES, MODEL_FIELDS, MODEL_B = (16, 24), 2, 2


def model_case():
    """-> (a fresh tante_amd.AFNO on the CPU with the scaled filter weights loaded, its state dict, x (B, in_T, fields, 16, 24))."""
    import tante_amd
    with torch.random.fork_rng():      # the constructor draws from the global generators: leave them as the other tests find them
        torch.manual_seed(1807)
        m = tante_amd.AFNO(dset_metadata=tante_amd.TanteMetadata(n_fields=MODEL_FIELDS, spatial_resolution=MODEL_RES), **MODEL_KW)
    sd = scale_filter_weights({k: v.detach().clone() for k, v in m.state_dict().items()}, MODEL_KW["hidden_dim"] // MODEL_KW["cmlp_diagonal_blocks"])
    m.load_state_dict(sd, strict=True)
    x = torch.randn(MODEL_B, MODEL_KW["in_T"], MODEL_FIELDS, *MODEL_RES, generator=torch.Generator().manual_seed(1808))
    return m, sd, x


class Shares:
    """mask_fn that keeps float64's own decisions and notes, per block call, the band share and the share of zeroed values."""

    def __init__(self, lam: float = 0.01):
        self.lam, self.band, self.zeroed = lam, [], []

    def __call__(self, Yp, H, W):
        kr, ki = keep64(Yp, self.lam)
        self.band.append(band_share(Yp, self.lam, H, W))
        self.zeroed.append(1.0 - float((kr.sum() + ki.sum()).item()) / (2 * kr.numel()))
        return kr, ki


def scale_filter_weights(sd: dict, bs: int) -> dict:
    """A fresh AFNO's filter is identically zero (weights of 0.02 against lam = 0.01): redraw them at the tests' scale 0.04 sqrt(32 / bs)."""
    gen = torch.Generator().manual_seed(4242)
    out = dict(sd)
    for k in sorted(sd):
        if ".cmlp." in k:
            out[k] = 0.04 * (32.0 / bs) ** 0.5 * torch.randn(sd[k].shape, generator=gen)
    return out
