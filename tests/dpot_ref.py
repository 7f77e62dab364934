"""Float64 restatement of DPOT's mixer, GroupNorm, block, model and re-fed rollout with explicit DFT matrices (no torch.fft), written
from the mathematics of the reference's models/dpot.py -- the counterpart of tests/afno_ref.py.  The g19 fixtures tie it to the reference
(tests/test_dpot_cpu.py); the GPU tests use it where no fixture exists (large blocks, odd shapes, the re-fed rollout).

The mixer on x (b, H, W, C) with k1 = min(modes, H), k2 = min(modes, W//2 + 1):
  forward   X[k, l] = sum_h sum_w e^{-2 pi i (k h / H + l w / W)} x[h, w] / sqrt(H W) for k < k1, l < k2 only (axis 1 keeps its first k1
            non-negative frequencies; the negative ones are dropped);
  MLP       per channel block: U = X W1 + b1, V = gelu(Re U) + i gelu(Im U), Y = V W2 + b2, all complex; w[0] / b[0] real, w[1] / b[1]
            imaginary parts; every spectrum entry outside the kept corner is zero, not the bias;
  inverse   axis 1 an H-point complex inverse over the k1 kept rows; axis 2 a W-point complex-to-real inverse over the k2 kept columns:
            column 0 (and column W/2 for even W) counts once and with its real part only, every other column twice; both 1/sqrt(n);
  out       = inverse + x (the filter's own input)."""
import math

import numpy as np
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


def kept(H: int, W: int, modes: int):
    return min(modes, H), min(modes, W // 2 + 1)


def block_linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """x (..., C) complex, w (2, nb, bs, bs), b (2, nb, bs): "...bi,bio->...bo" per channel block, plus the complex bias."""
    nb, bs = w.shape[1], w.shape[2]
    wc = torch.complex(w[0].to(DT), w[1].to(DT))
    bc = torch.complex(b[0].to(DT), b[1].to(DT))
    y = torch.einsum("...bi,bio->...bo", x.reshape(*x.shape[:-1], nb, bs), wc) + bc
    return y.reshape(*x.shape)


def c2r_matrices(W: int, k2: int):
    """(cos, sin) (W, k2): the complex-to-real inverse over the first k2 columns, and the mask of the columns that count once."""
    l = torch.arange(k2, dtype=DT)
    n = torch.arange(W, dtype=DT)
    ang = 2.0 * math.pi * torch.outer(n, l) / W
    once = (l == 0) | ((W % 2 == 0) & (l == W // 2))
    cl = torch.where(once, torch.ones_like(l), 2.0 * torch.ones_like(l))
    return torch.cos(ang) * cl / math.sqrt(W), torch.sin(ang) * cl / math.sqrt(W), once


def filter_contribution(x, w1, b1, w2, b2, modes: int) -> torch.Tensor:
    """irfft2(MLP(rfft2(x)[:k1, :k2])): what the filter ADDS to its input, float64."""
    x = x.to(DT)
    b, H, W, C = x.shape
    k1, k2 = kept(H, W, modes)
    X = torch.einsum("lw,bhwc->bhlc", dft_matrix(W, -1)[:k2], x.to(CDT))
    X = torch.einsum("kh,bhlc->bklc", dft_matrix(H, -1)[:k1], X)
    U = block_linear(X, w1, b1)
    V = torch.complex(gelu(U.real), gelu(U.imag))
    Y = block_linear(V, w2, b2)
    Z = torch.einsum("hk,bklc->bhlc", dft_matrix(H, +1)[:, :k1], Y)
    cosm, sinm, once = c2r_matrices(W, k2)
    Zim = torch.where(once[None, None, :, None], torch.zeros_like(Z.imag), Z.imag)
    return torch.einsum("wl,bhlc->bhwc", cosm, Z.real) - torch.einsum("wl,bhlc->bhwc", sinm, Zim)


def dpot_filter(x, w1, b1, w2, b2, modes: int) -> torch.Tensor:
    """x (b, H, W, C) -> (b, H, W, C) float64: AFNO2D.forward, channels last."""
    return filter_contribution(x, w1, b1, w2, b2, modes) + x.to(DT)


def contribution_ratio(x, w1, b1, w2, b2, modes: int) -> float:
    """rms(filter(x) - x) / rms(x)."""
    d = filter_contribution(x, w1, b1, w2, b2, modes)
    return float(torch.sqrt((d ** 2).mean()) / torch.sqrt((x.to(DT) ** 2).mean()))


def group_norm(x: torch.Tensor, w, b, G: int, eps: float = 1e-5) -> torch.Tensor:
    """x (B, ..., C) channels last: statistics per (sample, group) over all tokens and the group's channels, biased variance."""
    x = x.to(DT)
    B, C = x.shape[0], x.shape[-1]
    g = x.reshape(B, -1, G, C // G)
    mu = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((g - mu) / torch.sqrt(var + eps)).reshape(x.shape)
    if w is not None:
        y = y * w.to(DT)
    if b is not None:
        y = y + b.to(DT)
    return y


def block(x: torch.Tensor, sd: dict, pre: str, modes: int, double_skip: bool, G: int = 8) -> torch.Tensor:
    """x (b, H, W, C) -> Block.forward, channels last (the 1 x 1 convolutions are linears)."""
    x = x.to(DT)
    n1 = group_norm(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], G)
    f = dpot_filter(n1, sd[pre + "filter.w1"], sd[pre + "filter.b1"], sd[pre + "filter.w2"], sd[pre + "filter.b2"], modes)
    if double_skip:
        f = f + x
        res = f
    else:
        res = x
    n2 = group_norm(f, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], G)
    wa, wb = sd[pre + "mlp.0.weight"].to(DT), sd[pre + "mlp.2.weight"].to(DT)
    h = gelu(n2 @ wa.reshape(wa.shape[0], -1).T + sd[pre + "mlp.0.bias"].to(DT))
    return h @ wb.reshape(wb.shape[0], -1).T + sd[pre + "mlp.2.bias"].to(DT) + res


def time_weight(sd: dict, T: int, time_agg: str) -> torch.Tensor:
    """(T, C, C) float64: w, with cos(t gamma_i) folded into row i for 'exp_mlp'."""
    w = sd["time_agg_layer.w"].to(DT)
    if time_agg == "exp_mlp":
        t = torch.linspace(0, 1, T).to(DT)                                   # the reference builds it in fp32
        w = w * torch.cos(t[:, None] * sd["time_agg_layer.gamma"].to(DT))[:, :, None]
    return w


def model(x: torch.Tensor, sd: dict, patch: int, modes: int, time_agg: str, out_timesteps: int) -> torch.Tensor:
    """x (b, t, c, h, w) -> (b, out_timesteps, c, h, w) float64: DPOT.forward."""
    x = x.to(DT)
    b, T, c, h, w = x.shape
    p = patch
    Hp, Wp = h // p, w // p
    gx = torch.tensor(np.linspace(0, 1, h), dtype=torch.float).to(DT)          # np.linspace -> torch.float, as get_grid_3d stores it
    gy = torch.tensor(np.linspace(0, 1, w), dtype=torch.float).to(DT)
    gt = torch.tensor(np.linspace(0, 1, T), dtype=torch.float).to(DT)
    grid = torch.stack([gx[None, :, None].expand(T, h, w), gy[None, None, :].expand(T, h, w), gt[:, None, None].expand(T, h, w)], dim=1)
    img = torch.cat([x, grid[None].expand(b, -1, -1, -1, -1)], dim=2).reshape(b * T, c + 3, h, w)
    we = sd["patch_embed.proj.0.weight"].to(DT)                              # (E1, c + 3, p, p)
    pt = img.reshape(b * T, c + 3, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).reshape(b * T, Hp, Wp, -1)
    y = gelu(pt @ we.reshape(we.shape[0], -1).T + sd["patch_embed.proj.0.bias"].to(DT))
    w2 = sd["patch_embed.proj.2.weight"].to(DT)
    y = y @ w2.reshape(w2.shape[0], -1).T + sd["patch_embed.proj.2.bias"].to(DT) + sd["pos_embed"].to(DT)[0].permute(1, 2, 0)
    y = y.reshape(b, T, Hp, Wp, -1)
    y = torch.einsum("tij,btxyi->bxyj", time_weight(sd, T, time_agg), y)
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        y = block(y, sd, f"blocks.{i}.", modes, False)
        i += 1
    wd = sd["out_layer.0.weight"].to(DT)                                     # (E, od, p, p)
    o = torch.einsum("bhwk,kcij->bhiwjc", y, wd).reshape(b, h, w, wd.shape[1]) + sd["out_layer.0.bias"].to(DT)
    wa, wb = sd["out_layer.2.weight"].to(DT), sd["out_layer.4.weight"].to(DT)
    o = gelu(gelu(o) @ wa.reshape(wa.shape[0], -1).T + sd["out_layer.2.bias"].to(DT))
    o = o @ wb.reshape(wb.shape[0], -1).T + sd["out_layer.4.bias"].to(DT)    # (b, h, w, (t c))
    return o.reshape(b, h, w, out_timesteps, c).permute(0, 3, 4, 1, 2)


def rollout(x: torch.Tensor, sd: dict, patch: int, modes: int, time_agg: str, out_timesteps: int, n_steps: int) -> torch.Tensor:
    """The sliding-window re-feed of rollout_model: x (b, t, c, h, w) -> (b, n_steps, c, h, w)."""
    moving, out, produced = x.to(DT), [], 0
    while produced < n_steps:
        y = model(moving, sd, patch, modes, time_agg, out_timesteps)
        out.append(y)
        produced += y.shape[1]
        moving = torch.cat([moving[:, y.shape[1]:], y], dim=1)
    return torch.cat(out, dim=1)[:, :n_steps]
