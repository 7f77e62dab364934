"""Float64 restatement of the reference's models/unet_convnext.py from the mathematics, on state dicts -- channels-last throughout.  The
CPU suite pins it to the reference's fixtures (tests/golden/g21_convnext_*) at <= 1e-10; the GPU suite then uses it where no fixture
reaches.

`bf16_sites`: the GEMM groups ("block", "resample", "skip") whose operands -- the activation rows AND the weight as the kernels hold it,
folds included -- are rounded to bf16 before an exact product: the exact-bf16 evaluation that decides which groups ship in bf16 mode."""
import math

import torch
import torch.nn.functional as F


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def r16(t):
    """Round to bf16 once, keep float64."""
    return t.float().to(torch.bfloat16).double()


def dwconv7(x, w, b):
    """x (n, H, W, C), w (C, 1, 7, 7), b (C): depthwise cross-correlation, zero padding 3."""
    n, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    y = torch.zeros_like(x)
    wd = w.double()
    for dy in range(7):
        for dx in range(7):
            y = y + xp[:, dy:dy + H, dx:dx + W, :] * wd[:, 0, dy, dx]
    return y + b.double()


def normalise(x, eps=1e-6):
    """(x - mean) / sqrt(biased var + eps) over the last axis, no affine."""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / (var + eps).sqrt()


def l2_normalise(x, eps=1e-6):
    """x / max(||x||_2 over the last axis, eps): the channels_first "LayerNorm" without its weight."""
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def conv3x3(x, w, b):
    """x (n, H, W, Cin), w (Cout, Cin, 3, 3), b (Cout): zero padding 1."""
    n, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = 0
    wd = w.double()
    for dy in range(3):
        for dx in range(3):
            y = y + torch.einsum("nhwc,oc->nhwo", xp[:, dy:dy + H, dx:dx + W, :], wd[:, :, dy, dx])
    return y + b.double()


def block(x, sd, p="", bf16_sites=()):
    """x (n, H, W, C) -> x + gamma * pwconv2(gelu(pwconv1(LN(dwconv(x)))))."""
    g = sd.get(p + "gamma")
    z = normalise(dwconv7(x, sd[p + "dwconv.weight"], sd[p + "dwconv.bias"]))
    nw, nb = sd[p + "norm.weight"].double(), sd[p + "norm.bias"].double()
    w1, b1 = sd[p + "pwconv1.weight"].double(), sd[p + "pwconv1.bias"].double()
    w2, b2 = sd[p + "pwconv2.weight"].double(), sd[p + "pwconv2.bias"].double()
    if "block" in bf16_sites:                       # as the kernels hold them: affine folded into W1, gamma into W2, each rounded once
        w1f, b1f = (w1 * nw[None, :]).float().double(), (w1 @ nb + b1).float().double()
        w2f, b2f = (w2, b2) if g is None else (w2 * g.double()[:, None], b2 * g.double())
        w2f, b2f = w2f.float().double(), b2f.float().double()
        h = gelu(r16(z) @ r16(w1f).T + b1f)
        return x + (r16(h) @ r16(w2f).T + b2f)
    h = gelu((z * nw + nb) @ w1.T + b1)
    y = h @ w2.T + b2
    if g is not None:
        y = y * g.double()
    return x + y


def downsample(x, sd, p="", bf16_sites=()):
    """x (n, H, W, C): l2-normalise * weight (bias never applied) -> Conv2d 2 x 2 / 2."""
    n, H, W, C = x.shape
    nw = sd[p + "block.0.weight"].double().reshape(-1)
    w, b = sd[p + "block.1.weight"].double(), sd[p + "block.1.bias"].double()
    z = l2_normalise(x)
    if "resample" in bf16_sites:
        z, w = r16(z), r16((w * nw[None, :, None, None]).float())
    else:
        z = z * nw
    return torch.einsum("nhkwlc,ockl->nhwo", z.reshape(n, H // 2, 2, W // 2, 2, C), w) + b


def upsample(x, sd, p="", bf16_sites=()):
    """x (n, H, W, C): l2-normalise * weight (bias never applied) -> ConvTranspose2d 2 x 2 / 2."""
    n, H, W, C = x.shape
    nw = sd[p + "block.0.weight"].double().reshape(-1)
    w, b = sd[p + "block.1.weight"].double(), sd[p + "block.1.bias"].double()
    z = l2_normalise(x)
    if "resample" in bf16_sites:
        z, w = r16(z), r16((w * nw[:, None, None, None]).float())
    else:
        z = z * nw
    return torch.einsum("nhwc,cokl->nhkwlo", z, w).reshape(n, 2 * H, 2 * W, w.shape[1]) + b


def stage(x, sd, p, depth, mode, skip=None, bf16_sites=()):
    if skip is not None:
        w, b = sd[p + "skip_proj.weight"].double().reshape(x.shape[-1], -1), sd[p + "skip_proj.bias"].double()
        C = x.shape[-1]
        if "skip" in bf16_sites:
            x = r16(x) @ r16(w[:, :C]).T + r16(skip) @ r16(w[:, C:]).T + b
        else:
            x = torch.cat([x, skip], dim=-1) @ w.T + b
    for i in range(depth):
        x = block(x, sd, f"{p}blocks.{i}.", bf16_sites)
    if mode == "down":
        x = downsample(x, sd, p + "resample.", bf16_sites)
    elif mode == "up":
        x = upsample(x, sd, p + "resample.", bf16_sites)
    return x


def depth_of(sd, p):
    d = 0
    while f"{p}blocks.{d}.dwconv.weight" in sd:
        d += 1
    return d


def model(x, sd, bf16_sites=()):
    """x (b, t, c, h, w) -> (b, 1, c, h, w), float64."""
    b, t, c, h, w = x.shape
    cur = conv3x3(x.double().reshape(b, t * c, h, w).permute(0, 2, 3, 1), sd["in_proj.weight"], sd["in_proj.bias"])
    n_stages = 0
    while f"encoder.{n_stages}.resample.block.1.weight" in sd:
        n_stages += 1
    skips = []
    for i in range(n_stages):
        skips.append(cur)
        cur = stage(cur, sd, f"encoder.{i}.", depth_of(sd, f"encoder.{i}."), "down", None, bf16_sites)
    cur = stage(cur, sd, "neck.", depth_of(sd, "neck."), "neck", None, bf16_sites)
    for j in range(n_stages):
        cur = stage(cur, sd, f"decoder.{j}.", depth_of(sd, f"decoder.{j}."), "up", skips[-j] if j > 0 else None, bf16_sites)
    y = conv3x3(cur, sd["out_proj.weight"], sd["out_proj.bias"])
    return y.permute(0, 3, 1, 2).unsqueeze(1)
