"""GPU: the UNetConvNext baseline -- tante_convnext_block on both routes, tante_dwconv_ln, tante_l2norm_rows and tante_conv3x3 alone against
float64, the resamples, the skip stage and the whole models against the reference's fixtures, a model at the config's widths and the
default constructor's widths against the float64 restatement, and the out-of-scope cases."""
import contextlib
import types

import pytest
import torch

import convnext_ref as R
from conftest import max_rel, record_parity, rel_err
from test_convnext_cpu import BLOCKS, MODELS, keyed_golden, model_kwargs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}
IN_OFFSET = 30.0      # x = 30 + randn: torch's own fp32 LayerNorm stays under half the fp32 bar here (asserted below), a one-pass variance does not


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


def compute_of(mode):
    from tante_amd import _lib as L
    return L.BF16 if mode == "bf16" else L.F32


# ---- one block, both routes ---------------------------------------------------------------------------------------------------------------
# (C, H, W): all window and mostly padding; the fixture; an exact granule; several ragged tiles in both directions; the fixture; the
# config's neck; the limit
BLOCK_CASES = [(15, 2, 3), (15, 5, 7), (16, 8, 8), (30, 19, 37), (32, 9, 20), (240, 16, 16), (256, 7, 33)]
FIXTURE_OF = {(15, 5, 7): "g21_convnext_block_c15_5x7", (32, 9, 20): "g21_convnext_block_c32_9x20"}
_BLK = {}


def block_case(C, H, W):
    """-> (module on the CPU, x (2, H, W, C) channels-last, float64 result), computed once per shape; the fixtures' shapes are the fixtures."""
    key = (C, H, W)
    if key not in _BLK:
        import tante_amd.convnext as CN
        blk = CN.Block(C, 2).eval()
        if key in FIXTURE_OF:
            g, sd, _ = keyed_golden(FIXTURE_OF[key])
            blk.load_state_dict(sd, strict=True)
            x = g["x"].permute(0, 2, 3, 1).contiguous()
            want = g["y64"].permute(0, 2, 3, 1)
        else:
            gen = torch.Generator().manual_seed(C * 131 + H * 17 + W)
            with torch.no_grad():
                for p in blk.norm.parameters():
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
                blk.gamma.copy_(0.5 * (1.0 + 0.1 * torch.randn(C, generator=gen)))
            x = 0.4 * torch.randn(2, H, W, C, generator=gen)
            want = R.block(x.double(), {k: v.detach() for k, v in blk.state_dict().items()})
        _BLK[key] = (blk, x, want)
    return _BLK[key]


def run_block(dev, C, H, W, mode, fused, batch=None):
    blk, x, _ = block_case(C, H, W)
    blk = blk.to(dev)
    xd = (x if batch is None else x[batch:batch + 1]).contiguous().to(dev)
    with torch.no_grad():
        y = blk.run(xd, compute_of(mode), fused=fused)
    assert torch.equal(xd.cpu(), x if batch is None else x[batch:batch + 1]), "the block changed its input"
    return y


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["fused", "modular"])
@pytest.mark.parametrize("C,H,W", BLOCK_CASES)
def test_block_against_float64(dev, C, H, W, route, mode):
    _, _, want = block_case(C, H, W)
    y = run_block(dev, C, H, W, mode, route == "fused")
    close(y, want, mode, f"convnext block {route} C {C} {H} x {W}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("C,H,W", [(15, 2, 3), (240, 16, 16)])
def test_block_at_batch_one(dev, C, H, W, mode):
    _, _, want = block_case(C, H, W)
    close(run_block(dev, C, H, W, mode, True, batch=1), want[1:2], mode, f"convnext block fused C {C} {H} x {W} batch 1")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("C,H,W", BLOCK_CASES)
def test_fused_and_modular_agree(dev, C, H, W, mode):
    close(run_block(dev, C, H, W, mode, True), run_block(dev, C, H, W, mode, False), mode, f"convnext block fused vs modular C {C} {H} x {W}")


@pytest.mark.parametrize("C,H,W", BLOCK_CASES)
def test_fused_block_is_bit_identical_per_image_and_per_run(dev, C, H, W):
    """No atomics, and a token's arithmetic does not depend on its tile or its image: image i of the batch equals the image run alone."""
    y = run_block(dev, C, H, W, "fp32", True)
    assert torch.equal(y, run_block(dev, C, H, W, "fp32", True))
    for i in range(2):
        assert torch.equal(y[i:i + 1], run_block(dev, C, H, W, "fp32", True, batch=i)), i


def test_fused_block_refuses_257_channels_and_aliasing(dev):
    from tante_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 4, 4, 257, device=dev)
    y = torch.empty_like(x)
    st = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert L.tante_convnext_block(x.data_ptr(), y.data_ptr(), st.data_ptr(), 1, 4, 4, 257, 0, 1e-6, None) == -2
    assert b"tante_convnext_block: channels outside 1..256" in L.tante_last_error()
    assert L.tante_convnext_block(x.data_ptr(), x.data_ptr(), st.data_ptr(), 1, 4, 4, 16, 0, 1e-6, None) == -1
    assert b"must not alias" in L.tante_last_error()


# ---- tante_dwconv_ln alone ----------------------------------------------------------------------------------------------------------------
def dwln_case(C, H, W, offset=0.0, n=2):
    gen = torch.Generator().manual_seed(C * 7 + H * 5 + W)
    x = offset + torch.randn(n, H, W, C, generator=gen)
    w, b = 0.2 * torch.randn(C, 1, 7, 7, generator=gen), 0.3 * torch.randn(C, generator=gen)
    if offset:
        w = 0.01 * w + 1.0 / 49.0   # the window's weights sum to about one: the offset reaches the norm, a token's channels spread by ~0.5 around 30
    gw, gb = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    z = R.dwconv7(x.double(), w, b)
    return x, w, b, gw, gb, z


@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("C,H,W", [(15, 5, 7), (48, 9, 20), (512, 4, 4), (1024, 3, 5)])
def test_dwconv_ln_against_float64(dev, C, H, W, affine, out):
    import tante_amd.convnext as CN
    x, w, b, gw, gb, z = dwln_case(C, H, W)
    want = R.normalise(z)
    if affine:
        want = want * gw.double() + gb.double()
    y = CN.dwconv_ln(x.to(dev), w.reshape(C, 49).contiguous().to(dev), b.to(dev), 1e-6, gw.to(dev) if affine else None, gb.to(dev) if affine else None,
                     torch.bfloat16 if out == "bf16" else torch.float32)
    assert y.dtype == (torch.bfloat16 if out == "bf16" else torch.float32)
    close(y.view(2, H, W, C), want, out, f"dwconv_ln C {C} {H} x {W} affine {affine} -> {out}")


def test_dwconv_ln_on_an_offset_input(dev):
    """x = 30 + randn: E[z^2] - mean^2 in fp32 loses its digits where mean-then-centred keeps them."""
    import tante_amd.convnext as CN
    C, H, W = 48, 9, 20
    x, w, b, gw, gb, z = dwln_case(C, H, W, IN_OFFSET)
    want = R.normalise(z) * gw.double() + gb.double()
    own = torch.nn.functional.layer_norm(z.float(), (C,), gw, gb, 1e-6)                              # torch's own fp32 kernel, on the CPU
    assert rel_err(own, want) < 0.5 * TOL["fp32"] and max_rel(own, want) < TOL["fp32"], (rel_err(own, want), max_rel(own, want))
    y = CN.dwconv_ln(x.to(dev), w.reshape(C, 49).contiguous().to(dev), b.to(dev), 1e-6, gw.to(dev), gb.to(dev))
    close(y.view(2, H, W, C), want, "fp32", f"dwconv_ln C {C} {H} x {W} at offset {IN_OFFSET}")


# ---- tante_l2norm_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 15, 240])
def test_l2norm_rows_against_float64(dev, C, out):
    import tante_amd.convnext as CN
    x = torch.randn(37, C, generator=torch.Generator().manual_seed(C))
    y = CN.l2norm_rows(x.to(dev), 1e-6, torch.bfloat16 if out == "bf16" else torch.float32)
    close(y, R.l2_normalise(x.double()), out, f"l2norm rows C {C} -> {out}")


def test_l2norm_rows_of_zeros_and_below_eps(dev):
    """max(||x||, eps): a row of zeros gives zeros (not NaN), a row with a norm below eps is divided by eps."""
    import tante_amd.convnext as CN
    x = torch.randn(6, 15, generator=torch.Generator().manual_seed(3))
    x[2] = 0.0
    x[4] = 1e-8 * x[4]
    y = CN.l2norm_rows(x.to(dev), 1e-6).cpu()
    assert torch.isfinite(y).all() and torch.equal(y[2], torch.zeros(15))
    assert float(x[4].double().norm()) < 1e-6
    close(y[4], x[4].double() / 1e-6, "fp32", "l2norm row below eps")
    close(y, R.l2_normalise(x.double()), "fp32", "l2norm rows with a zero row")


# ---- tante_conv3x3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["in", "out"])
@pytest.mark.parametrize("H,W", [(2, 3), (5, 7), (17, 33)])
@pytest.mark.parametrize("Cin,Cout", [(12, 15), (15, 3), (44, 15)])
def test_conv3x3_against_float64(dev, Cin, Cout, H, W, form):
    """form 'in': channels first in, channels last out (in_proj); 'out': channels last in, channels first out (out_proj)."""
    import tante_amd.convnext as CN
    gen = torch.Generator().manual_seed(Cin * 31 + Cout * 7 + H + W)
    x = torch.randn(2, H, W, Cin, generator=gen)
    w, b = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3.0 * Cin ** 0.5), torch.randn(Cout, generator=gen)
    want = R.conv3x3(x.double(), w, b)
    if form == "in":
        y = CN.conv3x3(x.permute(0, 3, 1, 2).contiguous().to(dev), w.to(dev), b.to(dev), True, False)
    else:
        y = CN.conv3x3(x.to(dev), w.to(dev), b.to(dev), False, True).permute(0, 2, 3, 1)
    close(y, want, "fp32", f"conv3x3 {form} {Cin} -> {Cout} {H} x {W}")


# ---- fixtures and models ----------------------------------------------------------------------------------------------------------------
def fixture_module(name, make):
    g, sd, _ = keyed_golden(name)
    m = make().eval()
    m.load_state_dict(sd, strict=True)
    return g, m


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_resamples_and_skip_stage_against_the_fixtures(dev, mode):
    import tante_amd.convnext as CN
    for name, make in (("g21_convnext_down_c15", lambda: CN.Downsample(15, 30, 2)), ("g21_convnext_up_c30", lambda: CN.Upsample(30, 15, 2)),
                       ("g21_convnext_stage_skip_c30", lambda: CN.Stage(30, 15, 2, depth=1, mode="up", skip_project=True))):
        g, m = fixture_module(name, make)
        with torch.no_grad(), mode_scope(mode):
            y = m.to(dev)(g["x"].to(dev))
        close(y, g["y64"], mode, name)


def built_model(name, dev):
    import tante_amd
    g, sd, _ = keyed_golden(name)
    m = tante_amd.UNetConvNext(**model_kwargs(name)).eval()
    m.load_state_dict(sd, strict=True)
    return g, m.to(dev)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_against_the_fixture(dev, name, mode):
    g, m = built_model(name, dev)
    with torch.no_grad():
        y = m.set_compute(mode)(g["x"].to(dev))
    assert y.shape == g["y64"].shape
    close(y, g["y64"], mode, name)


def seeded_model(dev, seed, n_fields, **kw):
    import tante_amd
    torch.manual_seed(seed)
    m = tante_amd.UNetConvNext(4, types.SimpleNamespace(n_fields=n_fields, n_spatial_dims=2), **kw).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            leaf = k.split(".")[-1]
            if leaf == "gamma":
                p.copy_(0.5 * (1.0 + 0.1 * torch.randn_like(p)))
            elif ".norm." in k or ".block.0." in k:
                p.add_(0.1 * torch.randn_like(p))
    return m


@pytest.mark.parametrize("kw,res", [(dict(init_features=15, stages=4, blocks_per_stage=1), (32, 48)), (dict(), (16, 16))],
                         ids=["config-widths-15-to-240", "default-widths-32-to-512"])
def test_seeded_model_against_the_restatement(dev, kw, res):
    """The config's widths (every fused width, neck 2 x 3) and the default constructor's (C = 512 at the neck: the modular route)."""
    m = seeded_model(dev, 11, 3, **kw)
    x = torch.randn(1, 4, 3, *res)
    want = R.model(x, {k: v.detach() for k, v in m.state_dict().items()})
    m = m.to(dev)
    for mode in ("fp32", "bf16"):
        with torch.no_grad():
            y = m.set_compute(mode)(x.to(dev))
        close(y, want, mode, f"convnext model {kw or 'default'} {res[0]} x {res[1]}")


def test_channels_first_norm_bias_is_never_applied(dev):
    name = "g21_convnext_model_f15_s2_20x28"
    g, m = built_model(name, dev)
    with torch.no_grad():
        y = m(g["x"].to(dev))
        n = 0
        for k, p in m.named_parameters():
            if k.endswith("resample.block.0.bias"):
                p.add_(1.0 + torch.randn_like(p))
                n += 1
        assert n == 4
        assert torch.equal(y, m(g["x"].to(dev)))


def test_out_of_scope_calls_raise(dev):
    name = "g21_convnext_model_f15_s2_20x28"
    g, m = built_model(name, dev)
    x = g["x"].to(dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="t \\* c"):
            m(x[:, :3])
        with pytest.raises(ValueError, match="multiples of 2 \\*\\* stages"):
            m(x[..., :18, :])
        with pytest.raises(RuntimeError, match="GPU only"):
            m(g["x"])
        m.train()
        with pytest.raises(NotImplementedError, match="inference only"):
            m(x)
        m.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)
