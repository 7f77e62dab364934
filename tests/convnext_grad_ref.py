"""Cases and float64 helpers of the UNetConvNext training tests (tests/test_convnext_train_cpu.py, tests/test_hip_convnext_train.py).

The reference of every gradient is float64 autograd through tests/convnext_ref.py.  Beside it stands a float64 RESTATEMENT of the two
backward kernels as they decompose the work -- LayerNorm's three-term formula on the recomputed pre-norm sums, the flipped-tap
correlation for dx, the tap gradient as a correlation of du with the padded input; the two branches of the row norm -- which the CPU
tests hold to that autograd within 1e-10, so that a kernel that misses the bar on the GPU can be told from a decomposition that is wrong."""
import types

import torch
import torch.nn.functional as F

import convnext_ref as R

DT = torch.float64
EPS = 1e-6
IN_OFFSET = 30.0

# (n, C, H, W): all window, mostly padding; the fixture shape; an exact tile; one channel past a 32-channel chunk; ragged tiles both ways;
# the tile form's boundary; the limit; 578 tiles of 8 x 8 against the cap of 512 walking workgroups (launches A and B: the first 66 walk
# two tiles, and cross from image 0 into image 1; 16 channels, because a LayerNorm over a handful of channels meets tokens whose variance is
# near eps and is no test of a sum's order); 18 tiles against launch B's cap of 512 / 32 chunks = 16 walkers at 1024 channels
WALK_CAP = 512
DWLN_CASES = [(2, 15, 2, 3), (2, 15, 5, 7), (1, 16, 8, 8), (2, 33, 9, 9), (2, 30, 19, 37), (1, 512, 4, 4), (1, 1024, 3, 5), (2, 16, 136, 136),
              (1, 1024, 24, 48)]
L2_CASES = [1, 15, 240]
_CACHE = {}


def leaves(ts):
    return [None if t is None else t.detach().to(DT).clone().requires_grad_(True) for t in ts]


def dwln_case(n, C, H, W, offset=0.0):
    """-> x (n, H, W, C), w (C, 1, 7, 7), b, ln_w, ln_b, dy (n H W, C): seeded per shape; with an offset the window's weights sum to about
    one, as tests/test_hip_convnext.dwln_case has them, so that the offset reaches the norm."""
    gen = torch.Generator().manual_seed(n * 1009 + C * 7 + H * 5 + W + (1 if offset else 0))
    x = offset + torch.randn(n, H, W, C, generator=gen)
    w, b = 0.2 * torch.randn(C, 1, 7, 7, generator=gen), 0.3 * torch.randn(C, generator=gen)
    if offset:
        w = 0.01 * w + 1.0 / 49.0
    gw, gb = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    return x, w, b, gw, gb, torch.randn(n * H * W, C, generator=gen)


def dwln_forward(x, w, b, gw, gb):
    y = R.normalise(R.dwconv7(x, w, b), EPS)
    return y if gw is None else y * gw + gb


def dwln_autograd(x, w, b, gw, gb, dy):
    """float64 autograd of LN(dwconv7(x) + b) [* gw + gb]: (y, dx, d_taps (C, 1, 7, 7), d_dwbias, d_ln_w, d_ln_b); the last two None
    without the affine.  Computed once per (case, affine, dy) by `dwln_want`."""
    lv = leaves([x, w, b, gw, gb])
    y = dwln_forward(*lv)
    g = torch.autograd.grad(y, [t for t in lv if t is not None], dy.to(DT).reshape(y.shape))
    return (y.detach(), g[0], g[1], g[2], g[3] if gw is not None else None, g[4] if gw is not None else None)


def dwln_want(case, affine, bf16_dy, offset=0.0):
    """The case with its float64 reference, shared among the tests: the reference gradient is taken of the dy as rounded."""
    key = (case, affine, bf16_dy, offset)
    if key not in _CACHE:
        x, w, b, gw, gb, dy = dwln_case(*case, offset=offset)
        if bf16_dy:
            dy = dy.to(torch.bfloat16)
        if not affine:
            gw = gb = None
        _CACHE[key] = ((x, w, b, gw, gb, dy), dwln_autograd(x, w, b, gw, gb, dy.float()))
    return _CACHE[key]


def dwln_backward_restated(x, w, b, gw, dy):
    """The backward as tante_dwconv_ln_bwd decomposes it, float64: -> (dx, d_taps (C, 49), d_dwbias, d_ln_w, d_ln_b)."""
    x, dy = x.to(DT), dy.to(DT).reshape(x.shape)
    n, H, W, C = x.shape
    u = R.dwconv7(x, w, b)                                                      # launch A: recomputed
    mean = u.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((u - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    xh = (u - mean) * rstd
    g = dy if gw is None else dy * gw.to(DT)
    du = rstd * (g - g.mean(dim=-1, keepdim=True) - xh * (g * xh).mean(dim=-1, keepdim=True))
    d_ln_w, d_ln_b, d_dwb = (dy * xh).sum(dim=(0, 1, 2)), dy.sum(dim=(0, 1, 2)), du.sum(dim=(0, 1, 2))
    wd = w.to(DT).reshape(C, 7, 7)                                              # launch B
    dup, xp = F.pad(du, (0, 0, 3, 3, 3, 3)), F.pad(x, (0, 0, 3, 3, 3, 3))
    dx = torch.zeros_like(x)
    d_taps = torch.zeros(C, 49, dtype=DT)
    for a in range(7):
        for c in range(7):
            # dx[p] += w[a, c] du[p - (a - 3, c - 3)]: the taps flipped
            dx = dx + dup[:, 6 - a:6 - a + H, 6 - c:6 - c + W, :] * wd[:, a, c]
            d_taps[:, a * 7 + c] = (du * xp[:, a:a + H, c:c + W, :]).sum(dim=(0, 1, 2))
    return dx, d_taps, d_dwb, d_ln_w, d_ln_b


def l2_case(C, M=37):
    """Rows with a zero row (2) and a row below eps (4) when there are enough of them."""
    gen = torch.Generator().manual_seed(C + 11)
    x = torch.randn(M, C, generator=gen)
    x[2] = 0.0
    x[4] = 1e-8 * x[4]
    return x, torch.randn(M, C, generator=gen)


def l2_autograd(x, dy):
    (lx,) = leaves([x])
    y = R.l2_normalise(lx, EPS)
    return y.detach(), torch.autograd.grad(y, lx, dy.to(DT))[0]


def l2_backward_restated(x, dy, eps=EPS):
    x, dy = x.to(DT), dy.to(DT)
    r = x.norm(dim=-1, keepdim=True)
    y = x / r.clamp_min(1e-300)
    return torch.where(r > eps, (dy - y * (y * dy).sum(dim=-1, keepdim=True)) / r.clamp_min(1e-300), dy / eps)


# ---- modules and models -----------------------------------------------------------------------------------------------------------------
def block_fixture(name):
    """A g21 block fixture: -> (state dict, x (n, C, H, W) as the module takes it, dout of seed 31 in the same layout)."""
    from test_convnext_cpu import keyed_golden
    g, sd, _ = keyed_golden(name)
    x = g["x"].float()
    return sd, x, torch.randn(x.shape, generator=torch.Generator().manual_seed(31))


def block_ratio(sd, x, dout):
    """|dx - dout| / |dout| of the float64 restatement: the share of the input gradient that is not the skip's."""
    (lx,) = leaves([x])
    y = R.block(lx.permute(0, 2, 3, 1), sd).permute(0, 3, 1, 2)
    dx = torch.autograd.grad(y, lx, dout.to(DT))[0]
    return float((dx - dout.to(DT)).norm() / dout.to(DT).norm())


def sd_leaves(sd):
    return {k: (v.detach().to(DT).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}


def untrained(name):
    return name.endswith("resample.block.0.bias")


def trained_names(m):
    return [k for k, _ in m.named_parameters() if not untrained(k)]


def fixture_model(name):
    """A g21 model fixture as a tante_amd.UNetConvNext on the CPU: -> (model, state dict, input)."""
    import tante_amd
    from test_convnext_cpu import keyed_golden, model_kwargs
    g, sd, _ = keyed_golden(name)
    m = tante_amd.UNetConvNext(**model_kwargs(name)).eval()
    m.load_state_dict(sd, strict=True)
    return m, {k: v.clone() for k, v in m.state_dict().items()}, g["x"].float()


def default_model():
    """The default constructor on 16 x 16: 512 channels at the neck (tante_dwconv_ln's tile boundary), K chunks past 512, the chunked
    deconv branch; gamma near 0.5 and perturbed norms, as test_hip_convnext.seeded_model has them."""
    import tante_amd
    torch.manual_seed(11)
    m = tante_amd.UNetConvNext(4, types.SimpleNamespace(n_fields=3, n_spatial_dims=2)).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            leaf = k.split(".")[-1]
            if leaf == "gamma":
                p.copy_(0.5 * (1.0 + 0.1 * torch.randn_like(p)))
            elif ".norm." in k or ".block.0." in k:
                p.add_(0.1 * torch.randn_like(p))
    return m, {k: v.clone() for k, v in m.state_dict().items()}, torch.randn(1, 4, 3, 16, 16)


def rollout(x, sd, n_steps):
    """The float64 re-fed restatement: x (b, t, c, h, w) -> (b, n_steps, c, h, w); every call's frame replaces the oldest input frame."""
    cur, outs = x.to(DT), []
    for _ in range(n_steps):
        y = R.model(cur, sd)
        outs.append(y)
        cur = torch.cat([cur[:, 1:], y], dim=1)
    return torch.cat(outs, dim=1)
