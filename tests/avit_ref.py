"""Float64 restatement of the reference's models/avit.py from the mathematics, on state dicts -- channels-last throughout.  The CPU suite
pins it to the reference's fixtures (tests/golden/g20_avit_*) at <= 1e-6; the GPU suite then uses it where no fixture reaches."""
import math

import torch

OUT_STEPS = 4


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def rms_norm(x, w, eps=1e-8):
    """x (n, H, W, C): x / (unbiased std over the token plane + eps) * w; the mean is not subtracted from x."""
    n = x.shape[1] * x.shape[2]
    mean = x.mean(dim=(1, 2), keepdim=True)
    std = (((x - mean) ** 2).sum(dim=(1, 2), keepdim=True) / (n - 1)).sqrt()
    return x / (std + eps) * w.double()


def inst_norm(x, w, b, eps=1e-5):
    """x (n, H, W, C): (x - mean) / sqrt(biased var + eps) * w + b over the token plane."""
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    y = (x - mean) / (var + eps).sqrt()
    if w is not None:
        y = y * w.double() + b.double()
    return y


def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / (var + eps).sqrt() * w.double() + b.double()


def conv(x, w):
    """x (n, H, W, Cin), w (Cout, Cin, k, k): kernel = stride = k, no bias."""
    n, H, W, C = x.shape
    k = w.shape[-1]
    return torch.einsum("nhkwlc,ockl->nhwo", x.reshape(n, H // k, k, W // k, k, C), w.double())


def deconv(x, w, b=None):
    """x (n, H, W, Cin), w (Cin, Cout, k, k): transposed convolution with kernel = stride = k."""
    n, H, W, _ = x.shape
    k = w.shape[-1]
    y = torch.einsum("nhwc,cokl->nhkwlo", x, w.double()).reshape(n, H * k, W * k, w.shape[1])
    return y if b is None else y + b.double()


def attention(q, k, v, bias=None):
    """softmax(q k^T / sqrt(hd) + bias) v over (..., L, hd)."""
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if bias is not None:
        s = s + bias
    return torch.softmax(s, dim=-1) @ v


def bucket(rel, num_buckets=32, max_distance=32):
    """The T5 bucket of rel = key - query, bidirectional (the static method's defaults: max_distance 32).  |rel| < 16 only: there the
    log branch never sits on an integer, so its float32 evaluation in the reference and this float64 one truncate alike."""
    assert abs(rel) < 16
    nb = num_buckets // 2
    n = -rel
    ret = nb if n < 0 else 0
    n = abs(n)
    max_exact = nb // 2
    if n < max_exact:
        return ret + n
    return ret + min(max_exact + int(math.log(n / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)), nb - 1)


def bias_table(emb, T):
    """emb (32, heads) -> (heads, T, T) float64: bias[h, q, k] = emb[bucket(k - q), h]."""
    idx = torch.tensor([[bucket(k - q) for k in range(T)] for q in range(T)])
    return emb.double()[idx].permute(2, 0, 1)


def _lin(x, sd, p):
    w = sd[p + ".weight"].double()
    return x @ w.reshape(w.shape[0], -1).T + sd[p + ".bias"].double()


def _qkv(x, sd, p, heads):
    """-> q, k, v (..., heads, hd) from the channel order (head, [q | k | v], hd), q and k normalised."""
    y = _lin(x, sd, p + "input_head")
    hd = x.shape[-1] // heads
    y = y.reshape(*y.shape[:-1], heads, 3, hd)
    q = layer_norm(y[..., 0, :], sd[p + "qnorm.weight"], sd[p + "qnorm.bias"])
    k = layer_norm(y[..., 1, :], sd[p + "knorm.weight"], sd[p + "knorm.bias"])
    return q, k, y[..., 2, :]


def spatial_block(x, sd, p, heads):
    """x (n, H, W, C) -> AxialAttentionBlock.forward."""
    n, H, W, C = x.shape
    x = x.double()
    q, k, v = _qkv(rms_norm(x, sd[p + "norm1.weight"]), sd, p, heads)          # (n, H, W, heads, hd)
    xx = attention(*(t.permute(0, 1, 3, 2, 4) for t in (q, k, v))).permute(0, 1, 3, 2, 4)      # along W per (n, H, head)
    xy = attention(*(t.permute(0, 2, 3, 1, 4) for t in (q, k, v))).permute(0, 3, 1, 2, 4)      # along H per (n, W, head)
    a = ((xx + xy) / 2).reshape(n, H, W, C)
    a = _lin(rms_norm(a, sd[p + "norm2.weight"]), sd, p + "output_head")
    x = x + sd[p + "gamma_att"].double() * a
    m = _lin(gelu(_lin(x, sd, p + "mlp.fc1")), sd, p + "mlp.fc2")
    return x + sd[p + "gamma_mlp"].double() * rms_norm(m, sd[p + "mlp_norm.weight"])


def temporal_block(x, sd, p, heads):
    """x (T, B, H, W, C) -> AttentionBlock.forward."""
    T, B, H, W, C = x.shape
    x = x.double()
    h = inst_norm(x.reshape(T * B, H, W, C), sd[p + "norm1.weight"], sd[p + "norm1.bias"]).reshape(T, B, H, W, C)
    q, k, v = _qkv(h, sd, p, heads)                                            # (T, B, H, W, heads, hd)
    bias = bias_table(sd[p + "rel_pos_bias.relative_attention_bias.weight"], T)
    a = attention(*(t.permute(1, 2, 3, 4, 0, 5) for t in (q, k, v)), bias=bias).permute(4, 0, 1, 2, 3, 5).reshape(T * B, H, W, C)
    a = _lin(inst_norm(a, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), sd, p + "output_head").reshape(T, B, H, W, C)
    return x + sd[p + "gamma"].double() * a


def stem(xn, sd, p_bag="space_bag.", p="embed.in_proj."):
    """xn (n, H, W, c) normalised fields -> (n, H/16, W/16, E): the subsampled linear, then conv / rms norm / GELU three times."""
    c = xn.shape[-1]
    wb = sd[p_bag + "weight"].double()
    z = math.sqrt(wb.shape[1] / c) * (xn.double() @ wb[:, :c].T + sd[p_bag + "bias"].double())
    z = gelu(rms_norm(conv(z, sd[p + "0.weight"]), sd[p + "1.weight"]))
    z = gelu(rms_norm(conv(z, sd[p + "3.weight"]), sd[p + "4.weight"]))
    return rms_norm(conv(z, sd[p + "6.weight"]), sd[p + "7.weight"])


def head(z, sd, labels, p="debed."):
    """z (n, H', W', E) -> (n, 16 H', 16 W', len(labels))."""
    labels = list(labels)
    z = gelu(rms_norm(deconv(z.double(), sd[p + "out_proj.0.weight"]), sd[p + "out_proj.1.weight"]))
    z = gelu(rms_norm(deconv(z, sd[p + "out_proj.3.weight"]), sd[p + "out_proj.4.weight"]))
    return deconv(z, sd[p + "out_kernel"][:, labels], sd[p + "out_bias"][labels])


def model(x, sd, heads, depth):
    """x (b, t, c, h, w) -> AViT.forward: (b, min(t, 4), c, h, w) float64."""
    b, T, c, h, w = x.shape
    x = x.double()
    n = T * h * w
    mean = x.mean(dim=(1, 3, 4), keepdim=True)
    std = (((x - mean) ** 2).sum(dim=(1, 3, 4), keepdim=True) / (n - 1)).sqrt() + 1e-7
    xn = ((x - mean) / std).permute(1, 0, 3, 4, 2)                             # (t, b, h, w, c)
    z = stem(xn.reshape(T * b, h, w, c), sd)
    Hp, Wp, E = z.shape[1:]
    z = z.reshape(T, b, Hp, Wp, E)
    for i in range(depth):
        z = temporal_block(z, sd, f"blocks.{i}.temporal.", heads)
        z = spatial_block(z.reshape(T * b, Hp, Wp, E), sd, f"blocks.{i}.spatial.", heads).reshape(T, b, Hp, Wp, E)
    y = head(z.reshape(T * b, Hp, Wp, E), sd, range(c)).reshape(T, b, h, w, c).permute(1, 0, 4, 2, 3)     # (b, t, c, h, w)
    return (y * std + mean)[:, -OUT_STEPS:]


def rollout(x, sd, heads, depth, n_steps):
    """The sliding-window rollout re-fed on the CPU: every call returns min(T, 4) frames, which replace the oldest ones."""
    frames, win = [], x.double()
    while sum(f.shape[1] for f in frames) < n_steps:
        y = model(win, sd, heads, depth)
        frames.append(y)
        win = torch.cat([win, y], dim=1)[:, -x.shape[1]:]
    return torch.cat(frames, dim=1)[:, :n_steps]
