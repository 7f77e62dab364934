"""GPU parity of the CViT and spectral-path TRAINING operators, each alone, against float64 autograd.

Until now these kernels ran only inside whole-model gradient tests at toy sizes (head dim <= 12, <= 384 queries, one 32 x 32 spectral
image) under a 4e-2 bf16 bar.  Here every operator is called through its autograd.Function, the way cvit.py / spectral.py / fno.py call
it, at the shapes where its tiles and branches change:

* CrossAttentionFn        -- xattn_bwd_dq / xattn_bwd_dkv (z-slices of XB_QC = 512 queries summed with atomics, 256-key workgroups),
                             the MFMA forward up to Lk = 512 and the VALU forward above; packed self-attention and separate q / (k | v).
* LayerNormAffineFn       -- ln_affine_bwd_kernel's columns lane + 64 kq (C <= 1024) and its per-32-row gamma / beta atomics.
* GridEmbedFn             -- grid_embed_kernel / grid_embed_bwd_kernel: the ordered compaction lists (CAP 1024 / 256) and their flushes,
                             latent dims in four lane groups.
* FourierEmbedFn          -- cos / sin at the default kernel initialisation and the kernel's gradient.
* SpectralLayerFn         -- both forwards (truncated DFT, hipFFT) and tante_spectral_layer_bwd: the half-spectrum weights D_j at the
                             Nyquist column and for odd W, overlapping bands (the bottom one wins), clipped modes, the >64 KB LDS image.
* CropResizeFn, Im2colFn, Col2imFn -- resize_bwd_kernel (crop, both output layouts, non-integer scales) and col2im_nhwc_sized.

Each case compares the forward output and EVERY input / parameter gradient of a random linear functional sum(out * G) with
torch.autograd on the plain operation in float64 (bf16 cases: the same bf16-rounded inputs and G).  The references below are written
from the maths and pinned to the CPU oracles (which tests/golden pins to the reference model) by
tests/test_host_cpu.py::test_train_op_references_match_the_oracles.

Bars (from the precision, per tensor; vectors such as biases, gamma, beta and dgrid are held to their own bar):
* a fp32 result: relative L2 <= 2e-5 and max-norm (max |err| / max |ref|) <= 1e-4; a gradient summed over more than 4096 terms
  <= 1e-4 / 5e-4 (fp32 accumulation error grows with the term count).
* a bf16 result: relative L2 <= 5e-3, about 4x the RMS bf16 rounding of the result (2^-9 / sqrt(3)); max-norm <= 1.6e-2, 8x the
  largest rounding of one element (2^-9 of max |ref|).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, max_rel, record_parity

pytestmark = pytest.mark.gpu

F32_REL, F32_MAX = 2e-5, 1e-4
F32_SUM_REL, F32_SUM_MAX = 1e-4, 5e-4       # gradients summed over more than SUM_TERMS terms
SUM_TERMS = 4096
BF16_REL, BF16_MAX = 5e-3, 1.6e-2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bars(t: torch.Tensor, terms: int = 1):
    """(relative L2, max-norm) bar of a result by the dtype it is delivered in and the number of terms summed into one element."""
    if t.dtype == torch.bfloat16:
        return BF16_REL, BF16_MAX
    return (F32_SUM_REL, F32_SUM_MAX) if terms > SUM_TERMS else (F32_REL, F32_MAX)


FLOOR = 1e-2


def close(got, ref, what, terms=1, bar=None, floor=None):
    """got (kernel) vs ref (float64 reference): relative L2 and max-norm, recorded in parity_report.json with the bar.
    floor: the magnitudes of the terms summed into each element without their signs (float64, ref's shape), for a result that may cancel
    to (almost) nothing: the error is then measured against max(|ref|, FLOOR |floor|), i.e. a result that is exactly or nearly zero is
    held to the bar times a hundredth of its terms' size (a few fp32 roundings of them), not to an unreachable fraction of itself."""
    rb, mb = bar if bar is not None else bars(got, terms)
    mode = "bf16" if got.dtype == torch.bfloat16 else "fp32"
    got, ref = got.detach(), ref.detach()
    if got.is_complex():
        got, ref = torch.view_as_real(got), torch.view_as_real(ref)
    got, ref = got.to(torch.float64).cpu(), ref.to(torch.float64).cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    r, m = rel_err(got, ref), max_rel(got, ref)
    if floor is not None:
        floor = floor.detach().to(torch.float64).cpu()
        err = got - ref
        r = float(err.norm() / max(float(ref.norm()), FLOOR * float(floor.norm()), 1e-30))
        m = float(err.abs().max() / max(float(ref.abs().max()), FLOOR * float(floor.abs().max()), 1e-30))
    record_parity(r, m, rb, mode, what)
    assert r <= rb and m <= mb, f"{what}: rel {r:.3e} (bar {rb:.1e}), max {m:.3e} (bar {mb:.1e})"


def zero_close(got, natural, what, bar):
    """A result that is exactly zero in exact arithmetic (e.g. dq, dk with one key): its size relative to `natural`, the magnitude one
    of its terms has without the cancellation."""
    m = float(got.detach().abs().max()) / natural
    record_parity(m, m, bar, "bf16" if got.dtype == torch.bfloat16 else "fp32", what + " (exact zero)")
    assert m <= bar, f"{what}: |got| / natural scale = {m:.3e} (bar {bar:.1e})"


def randn(shape, gen, dtype=torch.float32, scale=1.0, shift=0.0):
    """CPU-seeded normal values rounded to `dtype` (the kernel input), so the float64 reference sees the same numbers."""
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale + shift).to(dtype)


def rounded_like(shape, gen, dtype):
    """The cotangent G of the functional sum(out * G): rounded to the dtype autograd hands the backward (that of `out`)."""
    return randn(shape, gen, dtype)


# ---- float64 references (plain torch, from the maths; pinned by test_host_cpu.py) ------------------------------------------------------
def ref_attention(q, k, v):
    """softmax(q k^T / sqrt(D)) v over (..., L, D)."""
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    return torch.softmax(s, dim=-1) @ v


def ref_layer_norm(x, gamma, beta, eps):
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def ref_grid_embed(coords, grid, latents, eps):
    """cvit.py:434-438: w = exp(-eps |x - g|^2) normalised over the grid WITHOUT a max shift (underflow as in the reference)."""
    d2 = ((coords[:, None, :] - grid[None, :, :]) ** 2).sum(dim=2)
    e = torch.exp(-eps * d2)
    return (e / e.sum(dim=1, keepdim=True)) @ latents


def ref_fourier_embed(coords, kernel):
    dp = coords @ kernel
    return torch.cat([torch.cos(dp), torch.sin(dp)], dim=-1)


def ref_spectral_layer(x, w_re, w_im, w0, b0, modes1, modes2):
    """SpectralLayer.forward (enc_dec_fno.py:213-222): rfft2 (ortho) -> one complex weight for the top band [:m1] and the bottom band
    [H - m1:], the bottom written second so it wins where they overlap (l.203-210) -> irfft2 (ortho), plus the 1x1 conv.  The weight
    may hold more modes than are used (only its first m1 x m2 are)."""
    n, Cin, H, W = x.shape
    wt = torch.complex(w_re, w_im)
    Cout = wt.shape[1]
    xf = torch.fft.rfft2(x, norm="ortho")
    Wf = xf.shape[-1]
    m1, m2 = min(modes1, H), min(modes2, Wf)
    ww = wt[:, :, :m1, :m2]
    yf = torch.zeros(n, Cout, H, Wf, dtype=xf.dtype)
    yf[:, :, :m1, :m2] = torch.einsum("bcij,coij->boij", xf[:, :, :m1, :m2], ww)
    yf[:, :, H - m1:, :m2] = torch.einsum("bcij,coij->boij", xf[:, :, H - m1:, :m2], ww)
    return torch.fft.irfft2(yf, s=(H, W), norm="ortho") + F.conv2d(x, w0, b0)


def ref_crop_resize(full, crop, Hi, Wi, Ho, Wo, nchw_out):
    """Bilinear resize (align_corners=False, F.interpolate) of the (Hi, Wi) window at `crop` of a channels-last image."""
    win = full[:, crop[0]:crop[0] + Hi, crop[1]:crop[1] + Wi, :].permute(0, 3, 1, 2)
    y = F.interpolate(win, size=(Ho, Wo), mode="bilinear", align_corners=False)
    return y if nchw_out else y.permute(0, 2, 3, 1)


def ref_im2col(x, P, stride, pad):
    """Channels-last (n, H, W, C) -> patch matrix (n Ho Wo, P P C), columns (kh, kw, c), zero padding."""
    n, H, W, C = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), P, padding=pad, stride=stride)          # (n, C P P, L), rows (c, kh, kw)
    L = u.shape[-1]
    return u.view(n, C, P, P, L).permute(0, 4, 2, 3, 1).reshape(n * L, P * P * C)


def ref_col2im(cols, bias, n, Hi, Wi, P, stride, pad, Cout):
    """Tap matrix (n Hi Wi, P P Cout), columns (kh, kw, co) -> channels-last (n, Hf, Wf, Cout) of the summed taps + bias (F.fold)."""
    Hf, Wf = (Hi - 1) * stride - 2 * pad + P, (Wi - 1) * stride - 2 * pad + P
    t = cols.view(n, Hi * Wi, P, P, Cout).permute(0, 4, 2, 3, 1).reshape(n, Cout * P * P, Hi * Wi)
    y = F.fold(t, (Hf, Wf), P, padding=pad, stride=stride)
    if bias is not None:
        y = y + bias[None, :, None, None]
    return y.permute(0, 2, 3, 1)


def _f64(t, dev=None):
    return t.detach().to(dev if dev is not None else t.device, torch.float64).requires_grad_()


# ---- cross-attention -----------------------------------------------------------------------------------------------------------------
LQS = [1, 255, 257, 511, 513, 1100]      # one / two query workgroups of 256; one / two / three z-slices of XB_QC = 512
LKS = [1, 63, 65, 257, 512, 513]         # key chunks of 64; a second 256-key workgroup; 512 = the MFMA forward's limit, 513 -> VALU
DS = [4, 8, 12, 16, 32, 64]
# every head dim meets every query and every key count once (a Latin square instead of the 216-case product)
XATTN_CASES = [(D, LQS[i], LKS[(i + j) % len(LKS)]) for j, D in enumerate(DS) for i in range(len(LQS))]


def _xattn(dev, dtype, nb, nh, D, Lq, Lk, packed, seed):
    from tante_amd.autograd import CrossAttentionFn
    C = nh * D
    g = torch.Generator().manual_seed(seed)
    if packed:                          # self-attention: the (M, 3C) projection is both buffers (cvit.py:_self_block_train)
        assert Lq == Lk
        qb = randn((nb * Lq, 3 * C), g, dtype)
        kvb, offs = qb, (0, C, 2 * C)
    else:                               # cross-attention: q (M, C) and (k | v) (M', 2C), ldkv = 2C (cvit.py:_cross_block_train)
        qb, kvb = randn((nb * Lq, C), g, dtype), randn((nb * Lk, 2 * C), g, dtype)
        offs = (0, 0, C)
    G = rounded_like((nb * Lq, C), g, dtype)
    qd = qb.to(dev).requires_grad_()
    kvd = qd if packed else kvb.to(dev).requires_grad_()
    o = CrossAttentionFn.apply(qd, kvd, *offs, nb, nh, D, Lq, Lk)
    o.backward(G.to(dev))
    torch.cuda.synchronize()

    q64 = _f64(qb, dev)
    kv64 = q64 if packed else _f64(kvb, dev)

    def heads(t, off, L):
        return t[:, off:off + C].reshape(nb, L, nh, D).transpose(1, 2)
    o64 = ref_attention(heads(q64, offs[0], Lq), heads(kv64, offs[1], Lk), heads(kv64, offs[2], Lk)).transpose(1, 2).reshape(nb * Lq, C)
    o64.backward(G.to(dev, torch.float64))
    tag = f"xattn {dtype} nb{nb} nh{nh} D{D} Lq{Lq} Lk{Lk}{' packed' if packed else ''}"
    close(o, o64, tag + " out")
    parts = [("dq", qd.grad, q64.grad, offs[0], Lk), ("dk", kvd.grad, kv64.grad, offs[1], Lq), ("dv", kvd.grad, kv64.grad, offs[2], Lq)]
    for name, gg, gr, off, terms in parts:
        got, ref = gg[:, off:off + C], gr[:, off:off + C]
        if Lk == 1 and name in ("dq", "dk"):
            # one key: p = 1, dp = delta, so dq = dk = 0 exactly; the kernel's are rounding residue of dp - delta (size |dO| |v| |q| / sqrt(D))
            natural = float(G.abs().max()) * float(kvb.abs().max()) * float(qb.abs().max()) * math.sqrt(D)
            zero_close(got, natural, f"{tag} {name}", bars(got)[0])
        else:
            close(got, ref, f"{tag} {name}", terms=terms)
    return o


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,Lq,Lk", XATTN_CASES)
def test_cross_attention_against_float64(dev, dtype, D, Lq, Lk):
    _xattn(dev, dtype, 2, 2, D, Lq, Lk, False, seed=1000 * D + Lq + 7 * Lk)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,L", [(8, 63), (16, 257), (64, 128), (64, 513)])
def test_cross_attention_packed_self_attention_against_float64(dev, dtype, D, L):
    _xattn(dev, dtype, 2, 3, D, L, L, True, seed=77 * D + L)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cross_attention_cfg4_decoder_shape(dev, dtype):
    """configs/cvit_rb.yaml: 512 x 128 query points, dec_num_heads 8 x 64, batch 1; the decoder's keys are the encoder's tokens,
    (512 / 16) x (128 / 16) = 256 patches x 1 time latent.  128 z-slices of 512 queries are summed into dk / dv."""
    _xattn(dev, dtype, 1, 8, 64, 512 * 128, 256, False, seed=4)


# ---- LayerNorm with affine -----------------------------------------------------------------------------------------------------------
LN_CS = [1, 24, 63, 64, 65, 512, 1000, 1024]
LN_MS = [1, 127, 128, 129, 65539]


def _ln(dev, M, C, seed, shift=0.0, bar=None):
    from tante_amd.autograd import LayerNormAffineFn
    g = torch.Generator().manual_seed(seed)
    x = randn((M, C), g, shift=shift)
    gamma, beta = randn((C,), g, scale=0.5, shift=1.0), randn((C,), g, scale=0.5)
    G = rounded_like((M, C), g, torch.float32)
    eps = 1e-5
    xd, gd, bd = x.to(dev).requires_grad_(), gamma.to(dev).requires_grad_(), beta.to(dev).requires_grad_()
    y = LayerNormAffineFn.apply(xd, gd, bd, eps)
    y.backward(G.to(dev))
    x64, g64, b64 = _f64(x, dev), _f64(gamma, dev), _f64(beta, dev)
    y64 = ref_layer_norm(x64, g64, b64, eps)
    y64.backward(G.to(dev, torch.float64))
    tag = f"ln_affine M{M} C{C}" + (f" mean {shift:g}" if shift else "")
    close(y, y64, tag + " y", bar=bar)
    with torch.no_grad():      # dx = rstd (dy gamma - mean(dy gamma) - x_hat mean(dy gamma x_hat)): exactly 0 for C = 1
        rstd = (x64.var(dim=-1, unbiased=False, keepdim=True) + eps).rsqrt()
        dx_terms = rstd * (G.to(dev, torch.float64) * g64).abs()
    close(xd.grad, x64.grad, tag + " dx", terms=C, bar=bar, floor=dx_terms)
    close(gd.grad, g64.grad, tag + " dgamma", terms=M, bar=bar)
    close(bd.grad, b64.grad, tag + " dbeta", terms=M, bar=bar)


@pytest.mark.parametrize("M", LN_MS)
@pytest.mark.parametrize("C", LN_CS)
def test_layernorm_affine_against_float64(dev, M, C):
    """x and dy are fp32 in every call cvit.py makes (the LayerNorm-affine inputs are fp32 residual streams, and autograd hands the
    backward the output's dtype)."""
    _ln(dev, M, C, seed=M * 1031 + C)


@pytest.mark.parametrize("C", [64, 512, 1024])
def test_layernorm_affine_large_mean(dev, C):
    # 1000 + randn: the row mean is 1000x the spread, so the fp32 sum of the row alone carries ~1000 * 2^-24 * sqrt(log2 C) ~ 3e-5 of
    # error relative to the centred values (the inputs themselves are exact in both).  The bar is that conditioning, at the model-level
    # fp32 bar (2e-4): what this case guards is the variance, which a one-pass E[x^2] - E[x]^2 would lose completely (~1e-1).
    _ln(dev, 4099, C, seed=C, shift=1000.0, bar=(2e-4, 2e-4))


def test_layernorm_affine_rejects_c_over_1024(dev):
    from tante_amd.autograd import LayerNormAffineFn
    x = torch.randn(8, 1025, device=dev, requires_grad=True)
    gamma, beta = torch.ones(1025, device=dev, requires_grad=True), torch.zeros(1025, device=dev, requires_grad=True)
    y = LayerNormAffineFn.apply(x, gamma, beta, 1e-5)
    with pytest.raises(RuntimeError, match="1024"):
        y.backward(torch.ones_like(y))
    assert x.grad is None and gamma.grad is None


# ---- grid embedding ------------------------------------------------------------------------------------------------------------------
def _grid_points(kind, G, gen):
    if kind == "lattice":                    # the CViT grid: 128 x 128 nodes on [0, 1]^2
        n = int(round(math.sqrt(G)))
        assert n * n == G
        xs, ys = torch.meshgrid(torch.linspace(0, 1, n), torch.linspace(0, 1, n), indexing="ij")
        return torch.stack([xs.flatten(), ys.flatten()], -1)
    return torch.rand((G, 2), generator=gen)


def _queries(kind, grid, N, gen):
    if kind == "random":
        return torch.rand((N, 2), generator=gen)
    idx = torch.randint(0, grid.shape[0], (N,), generator=gen)
    if kind == "on_nodes":                   # exactly on grid nodes: the node's own term has x - g = 0
        return grid[idx].clone()
    return grid[idx] + 0.004 * torch.randn((N, 2), generator=gen)      # "near": eps 1e5 keeps exp(-eps d^2) > 0 for the nearest node


GRID_CASES = [  # eps, G, grid, N, queries, LD
    (40.0, 16384, "lattice", 4097, "random", 512),     # every weight survives: the forward's 1024-list and the backward's 256-list flush
    (1e5, 16384, "lattice", 4097, "random", 512),      # cfg4 (eps 1e5 on 128 x 128): ~50 survivors per query
    (1e5, 16384, "lattice", 300, "on_nodes", 1024),
    (200.0, 16384, "lattice", 1, "random", 1024),
    (200.0, 257, "random", 300, "random", 257),
    (40.0, 257, "random", 4097, "on_nodes", 1024),
    (1e5, 257, "random", 4097, "near", 24),
    (40.0, 30, "random", 1, "random", 24),
    (1e5, 30, "random", 300, "near", 1024),
    (200.0, 30, "random", 4097, "on_nodes", 257),
]


@pytest.mark.parametrize("eps,G,gkind,N,qkind,LD", GRID_CASES)
def test_grid_embed_against_float64(dev, eps, G, gkind, N, qkind, LD):
    from tante_amd.autograd import GridEmbedFn
    gen = torch.Generator().manual_seed(G + N + LD)
    grid = _grid_points(gkind, G, gen)
    coords = _queries(qkind, grid, N, gen)
    latents = randn((G, LD), gen)
    Gc = rounded_like((N, LD), gen, torch.float32)
    gd, ld = grid.to(dev).requires_grad_(), latents.to(dev).requires_grad_()
    out = GridEmbedFn.apply(coords.to(dev), gd, ld, eps)
    out.backward(Gc.to(dev))
    g64, l64 = _f64(grid, dev), _f64(latents, dev)
    o64 = ref_grid_embed(coords.to(dev, torch.float64), g64, l64, eps)
    o64.backward(Gc.to(dev, torch.float64))
    tag = f"grid_embed eps{eps:g} G{G} {gkind} N{N} {qkind} LD{LD}"
    close(out, o64, tag + " out", terms=G)
    close(ld.grad, l64.grad, tag + " dlatents", terms=N)
    with torch.no_grad():
        # dgrid[g] = 2 eps sum_n w_ng (dout_n . (latents_g - out_n)) (x_n - g): with one surviving weight per query (eps 1e5 on a sparse
        # grid) out_n = latents_g and the exact dgrid is ~0, so it is measured against the size of its unsigned terms
        c64 = coords.to(dev, torch.float64)
        e = torch.exp(-eps * ((c64[:, None, :] - g64[None]) ** 2).sum(-1))
        w = e / e.sum(1, keepdim=True)
        Ga = Gc.to(dev, torch.float64).abs()
        amp = Ga @ l64.abs().t() + (Ga * o64.abs()).sum(1, keepdim=True)               # (N, G): |dout_n| . (|lat_g| + |out_n|)
        dgrid_terms = torch.stack([2 * eps * ((w * amp) * (c64[:, None, k] - g64[None, :, k]).abs()).sum(0) for k in range(2)], -1)
    close(gd.grad, g64.grad, tag + " dgrid", terms=N * LD, floor=dgrid_terms)


def test_grid_embed_rejects_ld_over_1024(dev):
    from tante_amd.autograd import GridEmbedFn
    grid = torch.rand(30, 2, device=dev, requires_grad=True)
    lat = torch.randn(30, 1025, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="1024"):
        GridEmbedFn.apply(torch.rand(8, 2, device=dev), grid, lat, 40.0)


# ---- Fourier embedding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 512 * 128])
def test_fourier_embed_against_float64(dev, N):
    """The default initialisation (FourierEmbs: randn(2, E/2) * 2 pi, E = dec_emb_dim 512) on [0, 1]^2 queries; N = 65 536 is the cfg4
    grid (the kernel gradient then sums 65 536 terms)."""
    from tante_amd.autograd import FourierEmbedFn
    gen = torch.Generator().manual_seed(N)
    kernel = randn((2, 256), gen, scale=2 * math.pi)
    if N == 512 * 128:
        xs, ys = torch.meshgrid(torch.linspace(0, 1, 512), torch.linspace(0, 1, 128), indexing="ij")
        coords = torch.stack([xs.flatten(), ys.flatten()], -1)
    else:
        coords = torch.rand((N, 2), generator=gen)
    Gc = rounded_like((N, 512), gen, torch.float32)
    kd = kernel.to(dev).requires_grad_()
    out = FourierEmbedFn.apply(coords.to(dev), kd)
    out.backward(Gc.to(dev))
    k64 = _f64(kernel, dev)
    o64 = ref_fourier_embed(coords.to(dev, torch.float64), k64)
    o64.backward(Gc.to(dev, torch.float64))
    close(out, o64, f"fourier N{N} out")
    close(kd.grad, k64.grad, f"fourier N{N} dkernel", terms=N)


# ---- spectral layer ------------------------------------------------------------------------------------------------------------------
SPEC_CASES = [  # n, Cin, Cout, H, W, modes1, modes2, wm1, wm2
    (2, 3, 5, 16, 16, 4, 9, 4, 9),          # W even, modes2 = W/2 + 1: the Nyquist column (D_j = 1) is kept
    (2, 4, 3, 15, 17, 5, 12, 5, 12),        # H and W odd (no Nyquist column); modes2 > W/2 + 1 -> clipped to 9, the weight holds 12
    (1, 3, 2, 12, 20, 8, 6, 8, 6),          # 2 m1 > H: the bands overlap, the bottom one wins
    (2, 2, 3, 9, 10, 12, 6, 12, 6),         # modes1 > H -> m1 = H: the bands coincide; wm1 = 12 > m1; Nyquist kept (W = 10)
    (3, 5, 4, 13, 14, 7, 8, 9, 10),         # H odd, W even, overlap, Nyquist, a weight with more modes than both used (9 x 10)
    (2, 3, 5, 32, 64, 8, 16, 8, 16),        # the truncated-DFT forward's shape class
    (1, 128, 128, 32, 32, 4, 4, 4, 4),      # 1x1 conv LDS image (128 * 64 + 128 * 128) * 4 = 96 KB > 64 KB
    (2, 8, 32, 512, 512, 20, 20, 20, 20),   # cfg5's largest: enc_spectral_1 of tante_fno.yaml (8 fields -> 256 / 8, modes 20 x 20)
]


def _set_dft(on: int):
    import tante_amd
    tante_amd.set_option("TANTE_SPECTRAL_DFT", int(on))


@pytest.mark.parametrize("n,Cin,Cout,H,W,m1,m2,wm1,wm2", SPEC_CASES)
def test_spectral_layer_against_float64(dev, n, Cin, Cout, H, W, m1, m2, wm1, wm2):
    from tante_amd import _lib
    from tante_amd.autograd import SpectralLayerFn
    gen = torch.Generator().manual_seed(H * W + Cin)
    x = randn((n, Cin, H, W), gen)
    s = 1.0 / math.sqrt(Cin * Cout)
    w_re, w_im = randn((Cin, Cout, wm1, wm2), gen, scale=s), randn((Cin, Cout, wm1, wm2), gen, scale=s)
    w0, b0 = randn((Cout, Cin, 1, 1), gen, scale=1.0 / math.sqrt(Cin)), randn((Cout,), gen, scale=0.1)
    Gc = rounded_like((n, Cout, H, W), gen, torch.float32)
    # reference on the CPU (pocketfft), independent of the device's FFT library
    x64, re64, im64, w064, b064 = (_f64(t, torch.device("cpu")) for t in (x, w_re, w_im, w0, b0))
    y64 = ref_spectral_layer(x64, re64, im64, w064, b064, m1, m2)
    y64.backward(Gc.double())
    tag = f"spectral n{n} {Cin}->{Cout} {H}x{W} modes {m1}x{m2} w {wm1}x{wm2}"
    HW = n * H * W
    old = _lib.get_option("TANTE_SPECTRAL_DFT", 1)
    try:
        for dft in (1, 0):       # truncated DFT where the shape has it (default), hipFFT (non-Hermitian column 0 into the C2R)
            _set_dft(dft)
            xd = x.to(dev).requires_grad_()
            wd = torch.complex(w_re, w_im).to(dev).requires_grad_()
            w0d, b0d = w0.to(dev).requires_grad_(), b0.to(dev).requires_grad_()
            y = SpectralLayerFn.apply(xd, wd, w0d, b0d, m1, m2)
            y.backward(Gc.to(dev))
            t = f"{tag} dft{dft}"
            close(y, y64, t + " y")
            close(xd.grad, x64.grad, t + " dx")
            close(wd.grad, torch.complex(re64.grad, im64.grad), t + " dW")
            close(w0d.grad, w064.grad, t + " dw0", terms=HW)
            close(b0d.grad, b064.grad, t + " db0", terms=HW)
    finally:
        _set_dft(old)


def test_spectral_layer_rejects_1x1_weight_over_lds(dev):
    """(200 * 64 + 200 * 200) * 4 = 211 KB of LDS > 160 KB: an error, not numbers."""
    from tante_amd.autograd import SpectralLayerFn
    x = torch.randn(1, 200, 16, 16, device=dev, requires_grad=True)
    w = torch.randn(200, 200, 4, 4, dtype=torch.complex64, device=dev, requires_grad=True)
    w0 = torch.randn(200, 200, 1, 1, device=dev, requires_grad=True)
    b0 = torch.zeros(200, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="LDS"):
        y = SpectralLayerFn.apply(x, w, w0, b0, 4, 4)
        y.backward(torch.ones_like(y))


# ---- bilinear resize (+ crop), im2col, col2im -----------------------------------------------------------------------------------------
RESIZE_CASES = [  # n, C, (Hf, Wf), crop, (Hi, Wi), (Ho, Wo), nchw_out, full dtype, out dtype
    (2, 5, (13, 11), (1, 2), (10, 7), (23, 16), True, torch.float32, torch.float32),        # upscale x2.3: the tiled channels-first kernel
    (2, 5, (13, 11), (1, 2), (10, 7), (23, 16), False, torch.float32, torch.float32),       # same, channels-last out
    (2, 6, (37, 41), (2, 3), (33, 35), (14, 20), True, torch.float32, torch.float32),       # downscale by 2.36 / 1.75
    (1, 6, (37, 41), (0, 5), (33, 35), (14, 20), False, torch.bfloat16, torch.bfloat16),    # downscale, bf16 in / out (bf16 dout)
    (2, 3, (20, 30), (3, 1), (9, 25), (21, 12), False, torch.bfloat16, torch.float32),      # up in H, down in W
    (2, 3, (20, 30), (3, 1), (9, 25), (21, 12), True, torch.float32, torch.bfloat16),
    (2, 32, (66, 66), (1, 1), (64, 64), (66, 66), True, torch.bfloat16, torch.bfloat16),    # a padded decoder's last stage (16-byte bf16 tiles)
]


@pytest.mark.parametrize("n,C,HWf,crop,HWi,HWo,nchw_out,fdt,odt", RESIZE_CASES)
def test_crop_resize_against_float64(dev, n, C, HWf, crop, HWi, HWo, nchw_out, fdt, odt):
    from tante_amd.autograd import CropResizeFn
    gen = torch.Generator().manual_seed(C * 100 + HWo[0])
    full = randn((n, *HWf, C), gen, fdt)
    oshape = (n, C, *HWo) if nchw_out else (n, *HWo, C)
    Gc = rounded_like(oshape, gen, odt)
    fd = full.to(dev).requires_grad_()
    out = CropResizeFn.apply(fd, n, C, *HWi, crop, *HWo, nchw_out, odt)
    out.backward(Gc.to(dev))
    f64 = _f64(full, dev)
    o64 = ref_crop_resize(f64, crop, *HWi, *HWo, nchw_out)
    o64.backward(Gc.to(dev, torch.float64))
    tag = f"resize {HWi}->{HWo} crop{crop} {'nchw' if nchw_out else 'nhwc'} {fdt}->{odt}"
    close(out, o64, tag + " out")
    close(fd.grad, f64.grad, tag + " dfull")


IM2COL_CASES = [  # n, C, H, W, P, stride, pad, x dtype, cols dtype
    (2, 3, 16, 16, 4, 2, 1, torch.float32, torch.float32),     # stride < P, pad
    (2, 5, 16, 12, 4, 4, 0, torch.float32, torch.float32),     # stride = P
    (1, 4, 13, 11, 4, 3, 1, torch.float32, torch.bfloat16),    # P divides neither size; stride < P
    (2, 8, 10, 14, 3, 3, 1, torch.float32, torch.bfloat16),    # stride = P, pad, P odd
    (2, 6, 9, 9, 2, 1, 0, torch.bfloat16, torch.bfloat16),
]


@pytest.mark.parametrize("n,C,H,W,P,stride,pad,xdt,cdt", IM2COL_CASES)
def test_im2col_against_float64(dev, n, C, H, W, P, stride, pad, xdt, cdt):
    from tante_amd.autograd import Im2colFn
    gen = torch.Generator().manual_seed(H * W + P)
    x = randn((n, H, W, C), gen, xdt)
    Ho, Wo = (H + 2 * pad - P) // stride + 1, (W + 2 * pad - P) // stride + 1
    Gc = rounded_like((n * Ho * Wo, P * P * C), gen, cdt)
    xd = x.to(dev).requires_grad_()
    cols = Im2colFn.apply(xd, n, C, H, W, P, stride, pad, cdt)
    cols.backward(Gc.to(dev))
    x64 = _f64(x, dev)
    c64 = ref_im2col(x64, P, stride, pad)
    c64.backward(Gc.to(dev, torch.float64))
    tag = f"im2col {H}x{W} P{P} s{stride} p{pad} {xdt}->{cdt}"
    close(cols, c64, tag + " cols")
    close(xd.grad, x64.grad, tag + " dx")


COL2IM_CASES = [  # n, Hi, Wi, P, stride, pad, Cout, cols dtype, out dtype, bias
    (2, 6, 5, 4, 2, 1, 3, torch.float32, torch.float32, True),      # overlapping taps (stride < P), pad
    (2, 4, 7, 4, 4, 0, 5, torch.float32, torch.float32, True),      # stride = P
    (2, 5, 6, 4, 3, 1, 4, torch.bfloat16, torch.bfloat16, True),    # out 14 x 17: P divides neither
    (1, 5, 6, 3, 2, 1, 4, torch.bfloat16, torch.float32, False),    # P odd, no bias
    (1, 64, 64, 4, 2, 1, 32, torch.bfloat16, torch.bfloat16, True), # an overlapping decoder stage: 128 x 128 x 32 (db sums 16 384 rows)
]


@pytest.mark.parametrize("n,Hi,Wi,P,stride,pad,Cout,cdt,odt,has_bias", COL2IM_CASES)
def test_col2im_against_float64(dev, n, Hi, Wi, P, stride, pad, Cout, cdt, odt, has_bias):
    from tante_amd.autograd import Col2imFn
    gen = torch.Generator().manual_seed(Hi * Wi + P + Cout)
    cols = randn((n * Hi * Wi, P * P * Cout), gen, cdt)
    bias = randn((Cout,), gen) if has_bias else None
    Hf, Wf = (Hi - 1) * stride - 2 * pad + P, (Wi - 1) * stride - 2 * pad + P
    Gc = rounded_like((n, Hf, Wf, Cout), gen, odt)
    cd = cols.to(dev).requires_grad_()
    bd = bias.to(dev).requires_grad_() if has_bias else None
    out = Col2imFn.apply(cd, bd, n, Hi, Wi, P, stride, pad, Cout, odt)
    out.backward(Gc.to(dev))
    c64 = _f64(cols, dev)
    b64 = _f64(bias, dev) if has_bias else None
    o64 = ref_col2im(c64, b64, n, Hi, Wi, P, stride, pad, Cout)
    o64.backward(Gc.to(dev, torch.float64))
    tag = f"col2im {Hi}x{Wi} P{P} s{stride} p{pad} C{Cout} {cdt}->{odt}"
    close(out, o64, tag + " out", terms=P * P)
    close(cd.grad, c64.grad, tag + " dcols")
    if has_bias:
        close(bd.grad, b64.grad, tag + " dbias", terms=n * Hf * Wf)
