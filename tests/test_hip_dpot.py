"""GPU: the DPOT baseline -- tante_groupnorm alone against float64, tante_dpot_filter alone against the reference's fixtures and the
float64 restatement (relative to the filter's CONTRIBUTION y - x: added to a unit-scale stream a 10 % filter error would shrink), the
block, the whole model and a re-fed rollout against the reference / its restatement, and the out-of-scope cases."""
import contextlib

import pytest
import torch

import dpot_ref as R
from conftest import load_golden, max_rel, record_parity, rel_err
from test_dpot_cpu import BLOCKS, FILTER_CF, FILTERS, MIN_RATIO, MODELS, filter_args, keyed_golden, model_kwargs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}
GN_OFFSET = 30.0      # x = 30 + randn: torch's own fp32 group_norm stays under half the fp32 bar here (asserted below), a one-pass variance does not


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(a, b, mode, note="", bar=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    bar = TOL[mode] if bar is None else bar
    r, m = rel_err(a, b), max_rel(a, b)
    print(f"{note} [{mode}]: rel {r:.3e} max {m:.3e} (bar {bar:.1e})")
    record_parity(r, m, bar, mode, note)
    assert r < bar and m < 2 * bar, f"{note}: rel={r:.3e} max={m:.3e} (bar {bar:.1e})"
    return r


def mode_scope(mode):
    return torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else contextlib.nullcontext()


# ---- GroupNorm alone -----------------------------------------------------------------------------------------------------------------
def gn_case(B, HW, C, offset):
    gen = torch.Generator().manual_seed(B * 7 + HW * 3 + C)
    x = offset + torch.randn(B, HW, C, generator=gen)
    w, b = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    return x, w, b, R.group_norm(x, w, b, 8)


@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("B,HW,C", [(2, 1, 64), (2, 35, 48), (2, 64, 1536), (1, 4096, 64)])
def test_groupnorm_against_float64(dev, B, HW, C, out):
    """One token; C/G = 6 (no multiple of 4) on an odd token count; the shipped width in several slabs; the token limit."""
    import tante_amd.dpot as D
    x, w, b, want = gn_case(B, HW, C, 0.0)
    y = D.groupnorm(x.to(dev), 8, w.to(dev), b.to(dev), 1e-5, torch.bfloat16 if out == "bf16" else torch.float32)
    assert y.dtype == (torch.bfloat16 if out == "bf16" else torch.float32) and y.shape == x.shape
    close(y, want, out, f"groupnorm ({B}, {HW}, {C}) -> {out}")
    y0 = D.groupnorm(x.to(dev), 8, None, None, 1e-5)
    close(y0, R.group_norm(x, None, None, 8), "fp32", f"groupnorm ({B}, {HW}, {C}) without affine")


@pytest.mark.parametrize("B,HW,C", [(2, 64, 1536), (1, 4096, 64)])
def test_groupnorm_on_an_offset_input(dev, B, HW, C):
    """x = 30 + randn: E[x^2] - mean^2 in fp32 loses 900 / 1 of its digits (errors of 1e-4) where mean-then-centred keeps them."""
    import tante_amd.dpot as D
    x, w, b, want = gn_case(B, HW, C, GN_OFFSET)
    own = torch.nn.functional.group_norm(x.permute(0, 2, 1), 8, w, b, 1e-5).permute(0, 2, 1)      # torch's fp32 kernel, on the CPU
    assert rel_err(own, want) < 0.5 * TOL["fp32"] and max_rel(own, want) < TOL["fp32"], (rel_err(own, want), max_rel(own, want))
    close(D.groupnorm(x.to(dev), 8, w.to(dev), b.to(dev), 1e-5), want, "fp32", f"groupnorm ({B}, {HW}, {C}) at offset {GN_OFFSET}")
    close(D.groupnorm(x.to(dev), 8, w.to(dev), b.to(dev), 1e-5, torch.bfloat16), want, "bf16", f"groupnorm ({B}, {HW}, {C}) at offset {GN_OFFSET} -> bf16")


# ---- the mixer alone -------------------------------------------------------------------------------------------------------------------
def filter_module(g, dev, channel_first=False):
    import tante_amd.dpot as D
    C = g["x"].shape[1] if channel_first else g["x"].shape[-1]
    f = D.AFNO2D(width=C, num_blocks=g["w1"].shape[1], channel_first=channel_first, modes=int(g["modes"]))
    f.load_state_dict({k: g[k] for k in ("w1", "b1", "w2", "b2")}, strict=True)
    return f.to(dev).eval()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", FILTERS + [FILTER_CF])
def test_filter_alone_against_the_reference(dev, name, mode):
    """AFNO2D.forward under the fp32 bar in BOTH compute modes (fp32 MFMA either way), relative to the contribution y - x."""
    g = load_golden(name)
    f = filter_module(g, dev, name == FILTER_CF)
    with torch.no_grad(), mode_scope(mode):
        y = f(g["x"].to(dev))
    assert y.dtype == torch.float32
    close(y.cpu().double() - g["x"].double(), g["y"].double() - g["x"].double(), "fp32", f"{name} contribution, {mode} scope")
    close(y, g["y"], "fp32", f"{name} output, {mode} scope")


def random_filter(B, H, W, C, nb, modes):
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + nb)
    bs = C // nb
    w1, w2 = torch.randn(2, nb, bs, bs, generator=gen) / bs ** 0.5, torch.randn(2, nb, bs, bs, generator=gen) / bs ** 0.5
    b1, b2 = 0.3 * torch.randn(2, nb, bs, generator=gen), 0.3 * torch.randn(2, nb, bs, generator=gen)
    return torch.randn(B, H, W, C, generator=gen), (w1, b1, w2, b2, modes)


@pytest.mark.parametrize("B,H,W,C,nb,modes", [(1, 8, 8, 768, 2, 16), (1, 64, 33, 48, 2, 20), (1, 33, 64, 128, 2, 64), (3, 1, 1, 16, 1, 5),
                                               (2, 7, 9, 40, 5, 2), (1, 5, 12, 80, 5, 4), (1, 12, 5, 80, 5, 4)])
def test_filter_shapes_without_a_fixture(dev, B, H, W, C, nb, modes):
    """The shipped block size of 384; the 64-point limit on either axis with odd partners and modes past / at the grid; a one-point grid;
    five blocks of 8 on odd axes: against the float64 restatement, relative to the contribution."""
    import tante_amd.dpot as D
    x, args = random_filter(B, H, W, C, nb, modes)
    assert R.contribution_ratio(x, *args) >= MIN_RATIO
    want = R.filter_contribution(x, *args)
    y = D.dpot_filter(x.to(dev), None, *(t.to(dev) for t in args[:4]), modes)
    close(y.cpu().double() - x.double(), want, "fp32", f"filter {H}x{W} C {C} blocks {nb} modes {modes} B {B} vs float64 restatement")


@pytest.mark.parametrize("name", ["g19_dpot_filter_8x12_m16", "g19_dpot_filter_5x7_m4"])
def test_filter_with_residual(dev, name):
    """The store epilogue's second skip (double_skip): out = filter(x) + residual is ONE more fp32 add of the finished value, so it equals
    the no-residual result plus the residual bit for bit -- with a separate output and in place on the residual stream."""
    import tante_amd.dpot as D
    g = load_golden(name)
    x = g["x"].to(dev)
    w = [t.to(dev) for t in filter_args(g)[:4]]
    modes = int(g["modes"])
    y0 = D.dpot_filter(x, None, *w, modes)
    close(y0.cpu().double() - g["x"].double(), g["y"].double() - g["x"].double(), "fp32", f"{name} kernel, no residual")
    res = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    y1 = D.dpot_filter(x, res, *w, modes)
    assert torch.equal(y1, y0 + res)
    stream = res.clone()
    D.dpot_filter(x, stream, *w, modes, out=stream)
    assert torch.equal(stream, y1)
    with pytest.raises(RuntimeError, match="out may alias residual, not x"):
        D.dpot_filter(x, None, *w, modes, out=x)


# ---- block, model, rollout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_against_the_reference(dev, name, mode):
    import tante_amd.dpot as D
    g, sd, _ = keyed_golden(name)
    blk = D.Block(width=64, n_blocks=2, mlp_ratio=2.0, channel_first=True, modes=int(g["modes"]), double_skip=BLOCKS[name])
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval()
    with torch.no_grad(), mode_scope(mode):
        y = blk(g["x"].to(dev))
    close(y, g["y"], mode, f"{name} block")


def build(name, dev, mode):
    import tante_amd
    g, sd, _ = keyed_golden(name)
    m = tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=MODELS[name]["res"]), **model_kwargs(name))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval().set_compute(mode), g, sd


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_against_the_reference(dev, name, mode):
    m, g, _ = build(name, dev, mode)
    with torch.no_grad():
        y = m(g["x"].to(dev))
    assert tuple(y.shape) == tuple(g["y"].shape)
    close(y, g["y"], mode, f"{name} model")
    if mode == "bf16":          # autocast resolves to the same mode as set_compute
        m.set_compute(None)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            assert torch.equal(m(g["x"].to(dev)), y)


def test_wide_model_against_the_restatement(dev):
    """Widths past one GEMM's K of 512 -- patch-embed K of 1280, a time aggregation and a block MLP over 576 channels, the transposed conv as
    a chunked tap GEMM + gather -- and a mixer block of 288, against the float64 restatement."""
    import tante_amd
    torch.manual_seed(1911)
    m = tante_amd.DPOT(in_T=2, dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(32, 32)), patch_size=16, n_blocks=2,
                       embed_dim=576, out_layer_dim=8, depth=1, modes=2, mlp_ratio=1.0, n_cls=2, time_agg="exp_mlp")
    with torch.no_grad():
        f = m.blocks[0].filter
        for w in (f.w1, f.w2):
            w.copy_(torch.randn_like(w) / f.block_size ** 0.5)
        for b in (f.b1, f.b2):
            b.copy_(0.3 * torch.randn_like(b))
        for k, p in m.named_parameters():
            if "norm" in k or k == "pos_embed":
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(2, 2, 2, 32, 32)
    want = R.model(x, sd, 16, 2, "exp_mlp", 1)
    m = m.to(dev).eval()
    with torch.no_grad():
        close(m(x.to(dev)), want, "fp32", "wide model (embed 576)")
        close(m.set_compute("bf16")(x.to(dev)), want, "bf16", "wide model (embed 576)")


def test_rollout_against_the_refed_restatement(dev):
    """rollout_model re-feeds out_timesteps = 2 frames per call: 3 steps (two calls, the last frame dropped) against the float64
    restatement re-fed on the CPU."""
    import tante_amd
    name = "g19_dpot_model_16x16_p2"
    m, g, sd = build(name, dev, "fp32")
    c = MODELS[name]
    x = g["x"]
    batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous().to(dev), "output": torch.zeros(2, 3, 16, 16, 2, device=dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16)))
    with torch.no_grad():
        y, y_ref = tante_amd.rollout_model(m, batch, fmt, 3)
    assert tuple(y.shape) == (2, 3, 16, 16, 2) and tuple(y_ref.shape) == (2, 3, 16, 16, 2)
    want = R.rollout(x, sd, c["patch"], c["modes"], c["time_agg"], c["out_timesteps"], 3).permute(0, 1, 3, 4, 2)
    for t in range(3):
        close(y[:, t], want[:, t], "fp32", f"rollout step {t + 1}")


def test_out_of_scope_cases_raise(dev):
    import tante_amd
    import tante_amd.dpot as D
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16))
    kw = dict(in_T=2, patch_size=4, n_blocks=2, embed_dim=32, depth=1, modes=4)
    x = torch.randn(1, 2, 2, 16, 16, device=dev)
    m = tante_amd.DPOT(dset_metadata=md, **kw).to(dev)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.train()(x)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.eval()(x)                                  # grad enabled with trainable parameters
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training is out of scope"):
        m.train()(x)
    with torch.no_grad():
        assert tuple(m.eval()(x).shape) == (1, 1, 2, 16, 16)
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16, 16), n_spatial_dims=3), **kw)
    with pytest.raises(NotImplementedError, match="act = 'silu'"):
        tante_amd.DPOT(dset_metadata=md, act="silu", **kw)
    with pytest.raises(NotImplementedError, match="mixing_type"):
        tante_amd.DPOT(dset_metadata=md, mixing_type="attn", **kw)
    with pytest.raises(NotImplementedError, match="hidden_size_factor = 2"):
        D.AFNO2D(width=32, num_blocks=2, hidden_size_factor=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            m.eval()(x.cpu())
    # shapes past the kernels' limits fail with the library's message, not silently
    f = D.AFNO2D(width=64, num_blocks=2, modes=4).to(dev).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="tante_dpot_filter: token grid outside 1..64"):
        f(torch.randn(1, 65, 8, 64, device=dev))
    with pytest.raises(RuntimeError, match="tante_groupnorm: tokens per sample outside 1..4096"):
        D.groupnorm(torch.randn(1, 4097, 16, device=dev), 8, None, None, 1e-5)
    with pytest.raises(RuntimeError, match="tante_groupnorm: channels are not a whole number of groups"):
        D.groupnorm(torch.randn(1, 4, 20, device=dev), 8, None, None, 1e-5)
    long = tante_amd.DPOT(in_T=1, dset_metadata=tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(130, 8)), patch_size=2, n_blocks=2,
                          embed_dim=32, depth=1, modes=4).to(dev).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="token grid outside 1..64"):
        long(torch.randn(1, 1, 1, 130, 8, device=dev))
