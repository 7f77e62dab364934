"""Cases and float64 helpers of the DPOT training tests (tests/test_dpot_train_cpu.py, tests/test_hip_dpot_train.py).

The reference of every gradient is float64 autograd through tests/dpot_ref.py.  Beside it stands a float64 RESTATEMENT of the backward as
the kernels decompose it -- the adjoint (conjugate-transposed) tables of tante_amd.dpot.twiddle_tables, complex-conjugate products for the
block MLP and its weight gradients, GroupNorm's three-term formula, the chain rule of the 'exp_mlp' fold -- which the CPU tests hold to
that autograd within 1e-10, so that a kernel that misses the bar on the GPU can be told from a decomposition that is wrong."""
import math

import numpy as np
import torch

import dpot_ref as R

DT, CDT = R.DT, R.CDT

# (B, H, W, C, nb, modes): bs 6 padded to 16 on an odd W with fewer than 64 channels; a partial second channel chunk; modes past the grid
# with H > W; 216 rows (a second row group) with bs 96 in one block; exactly 192 rows with bs 36 padded to 48; a one-point grid; the
# shipped block size 384 on the shipped grid
FILTER_CASES = [(2, 7, 9, 48, 8, 3), (1, 5, 12, 80, 5, 4), (1, 12, 5, 80, 5, 20), (2, 12, 16, 96, 1, 12), (2, 16, 10, 72, 2, 16),
                (3, 1, 1, 16, 1, 5), (1, 8, 8, 768, 2, 16)]
GN_CASES = [(2, 1, 64), (2, 35, 48), (2, 64, 1536), (1, 4096, 64)]       # the forward test's shapes
GROUPS = 8


def filter_case(B, H, W, C, nb, modes):
    """-> x, residual, (w1, b1, w2, b2), dout: the random_filter recipe of tests/test_hip_dpot.py, then the residual and the gradient."""
    from test_hip_dpot import random_filter
    x, args = random_filter(B, H, W, C, nb, modes)
    gen = torch.Generator().manual_seed(77 + H * 100 + W)
    return x, torch.randn(x.shape, generator=gen), args[:4], torch.randn(x.shape, generator=gen)


def leaves(ts):
    return [t.detach().to(DT).clone().requires_grad_(True) for t in ts]


def filter_autograd(x, ws, dout, modes):
    """float64 autograd of dpot_ref.filter_contribution: (contribution, d contribution / dx, dw1, db1, dw2, db2)."""
    lv = leaves([x, *ws])
    y = R.filter_contribution(*lv, modes)
    return (y.detach(), *torch.autograd.grad(y, lv, dout.to(DT)))


def dgelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _blocks(w):
    return torch.complex(w[0].to(DT), w[1].to(DT))


def filter_backward_restated(x, ws, dout, modes, tables=None):
    """The backward as tante_dpot_filter_bwd decomposes it, float64: -> (d contribution / dx, dw1, db1, dw2, db2).  `tables`: the four
    complex forward tables (default tante_amd.dpot.twiddle_tables); the adjoints are their conjugate transposes."""
    from tante_amd import dpot as D
    w1, b1, w2, b2 = ws
    B, H, W, C = x.shape
    nb, bs = w1.shape[1], w1.shape[2]
    T = [torch.from_numpy(np.asarray(t)).to(CDT) for t in (tables if tables is not None else D.twiddle_tables(H, W, modes))]
    A = [t.conj().T for t in T]
    W1, W2 = _blocks(w1), _blocks(w2)
    # launches 1 .. 3 again
    P = torch.einsum("lw,bhwc->bhlc", T[0], x.to(CDT))
    X = torch.einsum("kh,bhlc->bklc", T[1], P).reshape(B, -1, P.shape[2], nb, bs)
    U = torch.einsum("bklgi,gio->bklgo", X, W1) + _blocks(b1)
    V = torch.complex(R.gelu(U.real), R.gelu(U.imag))
    # the chain in reverse
    dZ = torch.einsum("lw,bhwc->bhlc", A[3], dout.to(CDT))
    dY = torch.einsum("kh,bhlc->bklc", A[2], dZ).reshape(X.shape)
    dV = torch.einsum("bklgo,gio->bklgi", dY, W2.conj())
    dU = torch.complex(dV.real * dgelu(U.real), dV.imag * dgelu(U.imag))
    dX = torch.einsum("bklgo,gio->bklgi", dU, W1.conj())
    dP = torch.einsum("hk,bklc->bhlc", A[1], dX.reshape(B, -1, P.shape[2], C))
    dx = torch.einsum("wl,bhlc->bhwc", A[0], dP).real
    dW2 = torch.einsum("bklgi,bklgo->gio", V.conj(), dY)
    dW1 = torch.einsum("bklgi,bklgo->gio", X.conj(), dU)
    db2, db1 = dY.sum(dim=(0, 1, 2)), dU.sum(dim=(0, 1, 2))
    ri = lambda z: torch.stack([z.real, z.imag])
    return dx, ri(dW1), ri(db1), ri(dW2), ri(db2)


def gn_case(B, HW, C, offset, affine=True):
    gen = torch.Generator().manual_seed(B * 7 + HW * 3 + C + 1)
    x = offset + torch.randn(B, HW, C, generator=gen)
    w = 1 + 0.3 * torch.randn(C, generator=gen) if affine else None
    b = 0.3 * torch.randn(C, generator=gen) if affine else None
    return x, w, b, torch.randn(B, HW, C, generator=gen)


def gn_autograd(x, w, b, dy, G=GROUPS, eps=1e-5):
    """float64 autograd of dpot_ref.group_norm: (y, dx, dgamma, dbeta) (the last two None without affine)."""
    lv = leaves([x] + ([w, b] if w is not None else []))
    y = R.group_norm(lv[0], lv[1] if w is not None else None, lv[2] if w is not None else None, G, eps)
    g = torch.autograd.grad(y, lv, dy.to(DT))
    return (y.detach(), g[0], g[1] if w is not None else None, g[2] if w is not None else None)


def gn_backward_restated(x, w, dy, G=GROUPS, eps=1e-5):
    """dx = rstd (g dy - mean(g dy) - xh mean(g dy xh)) per (sample, group); dgamma = sum dy xh, dbeta = sum dy: float64."""
    x, dy = x.to(DT), dy.to(DT)
    B, C = x.shape[0], x.shape[-1]
    g4 = lambda t: t.reshape(B, -1, G, C // G)
    xg = g4(x)
    mu = xg.mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(((xg - mu) ** 2).mean(dim=(1, 3), keepdim=True) + eps)
    xh = (xg - mu) * rstd
    d = g4(dy * w.to(DT)) if w is not None else g4(dy)
    dx = rstd * (d - d.mean(dim=(1, 3), keepdim=True) - xh * (d * xh).mean(dim=(1, 3), keepdim=True))
    flat = (g4(dy) * xh).reshape(-1, C), dy.reshape(-1, C)
    return dx.reshape(x.shape), flat[0].sum(dim=0), flat[1].sum(dim=0)


def fold_backward_restated(dwf, w, gamma):
    """The chain rule of wf[t, i, :] = w[t, i, :] cos(t_t gamma_i) as TimeAggFn.backward states it: -> (dw, dgamma)."""
    T = w.shape[0]
    tt = torch.linspace(0, 1, T).to(DT)[:, None]
    ang = tt * gamma.to(DT).reshape(1, -1)
    dwf = dwf.to(DT)
    return dwf * torch.cos(ang)[:, :, None], ((dwf * w.to(DT)).sum(dim=2) * (-torch.sin(ang) * tt)).sum(dim=0).reshape(gamma.shape)


# ---- models -----------------------------------------------------------------------------------------------------------------------------
WIDE_KW = dict(in_T=2, patch_size=16, n_blocks=2, embed_dim=576, out_layer_dim=8, depth=1, modes=2, mlp_ratio=1.0, n_cls=2, time_agg="exp_mlp")


def fixture_model(name):
    """A g19 model fixture as a tante_amd.DPOT on the CPU: -> (model, state dict, input, the fixture's config)."""
    import tante_amd
    from test_dpot_cpu import MODELS, keyed_golden, model_kwargs
    g, sd, _ = keyed_golden(name)
    m = tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=MODELS[name]["res"]), **model_kwargs(name))
    m.load_state_dict(sd, strict=True)
    return m, {k: v.clone() for k, v in m.state_dict().items()}, g["x"], MODELS[name]


def wide_model():
    """The wide model of test_hip_dpot.test_wide_model_against_the_restatement: embed 576 (K chunks past 512, the chunked tap-GEMM deconv, a
    mixer block of 288), 'exp_mlp'."""
    import tante_amd
    torch.manual_seed(1911)
    m = tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(32, 32)), **WIDE_KW)
    with torch.no_grad():
        f = m.blocks[0].filter
        for w in (f.w1, f.w2):
            w.copy_(torch.randn_like(w) / f.block_size ** 0.5)
        for b in (f.b1, f.b2):
            b.copy_(0.3 * torch.randn_like(b))
        for k, p in m.named_parameters():
            if "norm" in k or k == "pos_embed":
                p.add_(0.2 * torch.randn_like(p))
    cfg = dict(res=(32, 32), patch=16, modes=2, time_agg="exp_mlp", out_timesteps=1)
    return m, {k: v.clone() for k, v in m.state_dict().items()}, torch.randn(2, 2, 2, 32, 32), cfg


def sd_leaves(sd):
    return {k: (v.detach().to(DT).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}


def trained_names(m):
    return [k for k, _ in m.named_parameters() if not k.startswith("cls_head.")]
