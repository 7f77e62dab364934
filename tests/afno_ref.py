"""Float64 restatement of the AFNO filter, block and model with explicit DFT matrices (no torch.fft), written from the mathematics of
the reference's models/afno.py -- the counterpart of tests/gemm_forms_ref.py.  The g18 fixtures tie it to the reference
(tests/test_afno_cpu.py); the GPU tests use it where no fixture exists (odd shapes, the re-fed rollout).

The filter on x (b, H, W, C), as torch.fft.rfftn / irfftn evaluate `dim=(2, 1)` with `s=(H, W)`:
  forward   full DFT over axis 2 (W points), then the half spectrum k = 0..H//2 of the DFT over axis 1 (H points), both 1/sqrt(n);
  MLP       per channel block: U = X W1, V = gelu(Re U) + i gelu(Im U), Y = V W2, soft threshold on Re and Im separately;
  inverse   axis 2 is resized from W to H entries (crop or zero pad) and gets an H-point inverse DFT; axis 1 is resized from H//2+1 to
            W//2+1 entries and gets a W-point complex-to-real inverse: entry 0 (and entry W/2 for even W) counts once and only with
            its real part, every other entry twice (the Hermitian half that is not stored).
The result is (b, W, H, C); the block swaps the two axes back before its first skip."""
import math

import torch

DT = torch.float64
CDT = torch.complex128


def dft_matrix(n: int, sign: int) -> torch.Tensor:
    """F[j, k] = exp(sign 2 pi i j k / n) / sqrt(n)."""
    j = torch.arange(n, dtype=DT)
    ang = 2.0 * math.pi * torch.outer(j, j) / n
    return torch.complex(torch.cos(ang), sign * torch.sin(ang)) / math.sqrt(n)


def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def softshrink(x: torch.Tensor, lam: float) -> torch.Tensor:
    return torch.where(x > lam, x - lam, torch.where(x < -lam, x + lam, torch.zeros_like(x)))


def block_linear(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """x (..., C) complex, weight (n_blocks, bs, bs, 2): "...bi,bio->...bo" per channel block."""
    nb, bs = weight.shape[0], weight.shape[1]
    w = torch.complex(weight[..., 0].to(DT), weight[..., 1].to(DT))
    y = torch.einsum("...bi,bio->...bo", x.reshape(*x.shape[:-1], nb, bs), w)
    return y.reshape(*x.shape)


def spectrum(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, lam: float) -> torch.Tensor:
    """-> the thresholded half spectrum (b, H//2+1, W, C), complex."""
    b, H, W, C = x.shape
    X = torch.einsum("lw,bhwc->bhlc", dft_matrix(W, -1), x.to(CDT))
    X = torch.einsum("kh,bhlc->bklc", dft_matrix(H, -1)[: H // 2 + 1], X)
    U = block_linear(X, w1)
    V = torch.complex(gelu(U.real), gelu(U.imag))
    Y = block_linear(V, w2)
    return torch.complex(softshrink(Y.real, lam), softshrink(Y.imag, lam))


def zeroed_share(x, w1, w2, lam) -> float:
    Y = spectrum(x.to(DT), w1, w2, lam)
    return float(((Y.real == 0).sum() + (Y.imag == 0).sum()).item() / (2 * Y.numel()))


def afno_filter(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, lam: float) -> torch.Tensor:
    """x (b, H, W, C) -> (b, W, H, C) float64: AFNO_ND.forward."""
    x = x.to(DT)
    b, H, W, C = x.shape
    Y = spectrum(x, w1, w2, lam)
    # axis 2: W entries -> H entries, H-point inverse
    Lc = min(W, H)
    Yp = torch.zeros(b, H // 2 + 1, H, C, dtype=CDT)
    Yp[:, :, :Lc] = Y[:, :, :Lc]
    Z = torch.einsum("nl,bklc->bknc", dft_matrix(H, +1), Yp)
    # axis 1: H//2+1 entries -> W//2+1 entries, W-point complex-to-real inverse
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
    Zim = torch.where(once[None, :, None, None], torch.zeros_like(Zp.imag), Zp.imag)      # a real signal's DC / Nyquist bins are real
    cosm, sinm = torch.cos(ang) * ck / math.sqrt(W), torch.sin(ang) * ck / math.sqrt(W)
    return torch.einsum("nk,bkhc->bnhc", cosm, Zre) - torch.einsum("nk,bkhc->bnhc", sinm, Zim)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.to(DT) + b.to(DT)


def block(x: torch.Tensor, sd: dict, pre: str, lam: float, eps: float = 1e-6) -> torch.Tensor:
    """x (b, H, W, C) -> Block.forward with double_skip."""
    n1 = layer_norm(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    f = afno_filter(n1, sd[pre + "filter.cmlp.0.weight"], sd[pre + "filter.cmlp.2.weight"], lam)
    x = f.transpose(1, 2) + x
    n2 = layer_norm(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    h = gelu(n2 @ sd[pre + "mlp.fc1.weight"].to(DT).T + sd[pre + "mlp.fc1.bias"].to(DT))
    return h @ sd[pre + "mlp.fc2.weight"].to(DT).T + sd[pre + "mlp.fc2.bias"].to(DT) + x


def model(x: torch.Tensor, sd: dict, patch: int, lam: float = 0.01) -> torch.Tensor:
    """x (b, t, c, h, w) -> (b, 1, c, h, w) float64: AFNO.forward in eval mode."""
    x = x.to(DT)
    b, t, c, h, w = x.shape
    p = patch
    Hp, Wp = h // p, w // p
    we = sd["patch_embed.weight"].to(DT)                                   # (C, t c, p, p)
    C = we.shape[0]
    pt = x.reshape(b, t * c, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).reshape(b, Hp, Wp, t * c * p * p)
    y = pt @ we.reshape(C, -1).T + sd["patch_embed.bias"].to(DT) + sd["pos_embed"].to(DT)
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        y = block(y, sd, f"blocks.{i}.", lam)
        i += 1
    wd = sd["patch_debed.weight"].to(DT)                                   # (C, c_out, p, p)
    o = torch.einsum("bhwk,kcij->bchiwj", y, wd).reshape(b, wd.shape[1], h, w) + sd["patch_debed.bias"].to(DT)[None, :, None, None]
    return o.unsqueeze(1)


def rollout(x: torch.Tensor, sd: dict, patch: int, n_steps: int, lam: float = 0.01) -> torch.Tensor:
    """The sliding-window re-feed of rollout_model: x (b, t, c, h, w) -> (b, n_steps, c, h, w)."""
    moving, out = x.to(DT), []
    for _ in range(n_steps):
        y = model(moving, sd, patch, lam)
        out.append(y)
        moving = torch.cat([moving[:, 1:], y], dim=1)
    return torch.cat(out, dim=1)
