"""GPU: the AttentionUNet baseline -- tante_conv3x3_mfma alone against float64 (plain, pooled, upsampled and two-source forms, every tile
form, bit equality per image), tante_attn_gate alone, the components and the whole models against the reference's fixtures in both
compute modes on both routes, and depth 4 against the float64 restatement."""
import contextlib
import types

import pytest
import torch

import unet_att_ref as R
from conftest import max_rel, record_parity, rel_err
from test_unet_att_cpu import MODELS, keyed_golden, model_kwargs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(a, b, mode, note=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    bar = TOL[mode]
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


@contextlib.contextmanager
def option(name, value, restore):
    import tante_amd
    tante_amd.set_option(name, value)
    try:
        yield
    finally:
        tante_amd.set_option(name, restore)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- tante_conv3x3_mfma alone ---------------------------------------------------------------------------------------------------------
# (Cin, Cout, H, W): an image that is all padding; ragged in both directions below one tile; an exact tile row count with W past one tile
# (the component fixture's shape); ragged tiles in both directions, several tiles; Cin and Cout off every granule (16, 32, 64); the longest K
PLAIN_CASES = [(7, 24, 1, 1), (12, 64, 2, 3), (64, 64, 9, 20), (44, 64, 19, 37), (130, 72, 8, 16), (1024, 512, 2, 3)]
_CONV = {}


def conv_case(key, Cin, Cout, Hs, Ws, n=2):
    """-> (x (n, Hs, Ws, Cin) with a different offset per image, w, scale, shift), made once per key.  The offsets (3, -2, 1) make a halo
    that is wrongly zeroed, wrongly read or taken from the neighbouring image show."""
    if key not in _CONV:
        gen = torch.Generator().manual_seed(Cin * 131 + Cout * 17 + Hs * 5 + Ws)
        x = torch.randn(n, Hs, Ws, Cin, generator=gen) + torch.tensor([3.0, -2.0, 1.0])[:n].reshape(n, 1, 1, 1)
        w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3.0 * Cin ** 0.5)
        scale, shift = 1 + 0.3 * torch.rand(Cout, generator=gen), 0.3 * torch.randn(Cout, generator=gen)
        _CONV[key] = (x, w, scale, shift)
    return _CONV[key]


def conv_want(key, src, w, scale, shift):
    """The float64 result before the activation, computed once per key."""
    k = ("want",) + tuple(key)
    if k not in _CONV:
        _CONV[k] = R.conv3x3(src.double(), w) * scale.double() + shift.double()
    return _CONV[k]


def run_conv(dev, a, w, scale, shift, mode, relu=True, form=0, b=None, out="fp32"):
    import tante_amd.unet_att as UA
    wf = (w.double() * scale.double().reshape(-1, 1, 1, 1)).float()
    packed = UA.pack_conv3x3(wf.to(dev), compute_of(mode))
    y = UA.conv3x3_mfma(a.contiguous().to(dev), packed, shift.to(dev), w.shape[0], compute_of(mode), relu, form, None if b is None else b.contiguous().to(dev),
                        torch.bfloat16 if out == "bf16" else torch.float32)
    assert y.dtype == (torch.bfloat16 if out == "bf16" else torch.float32)
    return y


@pytest.mark.parametrize("mode,out", [("fp32", "fp32"), ("bf16", "fp32"), ("fp32", "bf16"), ("bf16", "bf16")])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("Cin,Cout,H,W", PLAIN_CASES)
def test_conv3x3_mfma_plain_against_float64(dev, Cin, Cout, H, W, relu, mode, out):
    key = ("plain", Cin, Cout, H, W)
    x, w, scale, shift = conv_case(key, Cin, Cout, H, W)
    want = conv_want(key, x, w, scale, shift)
    want = torch.relu(want) if relu else want
    y = run_conv(dev, x, w, scale, shift, mode, relu, 0, None, out)
    close(y, want, "bf16" if "bf16" in (mode, out) else "fp32", f"conv3x3_mfma {Cin} -> {Cout} {H} x {W} relu {relu} rows {out}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("form_id", [1, 2, 3])
@pytest.mark.parametrize("Cin,Cout,H,W", [(12, 64, 2, 3), (44, 64, 19, 37), (130, 72, 8, 16)])
def test_conv3x3_mfma_every_tile_form_gives_the_same_bits(dev, Cin, Cout, H, W, form_id, mode):
    """The tile form (8 x 16 x 64, 4 x 16 x 32, 2 x 16 x 32) changes who computes a pixel, not its sum."""
    key = ("plain", Cin, Cout, H, W)
    x, w, scale, shift = conv_case(key, Cin, Cout, H, W)
    auto = run_conv(dev, x, w, scale, shift, mode)
    with option("TANTE_CONV3_FORM", form_id, 0):
        forced = run_conv(dev, x, w, scale, shift, mode)
    assert torch.equal(auto, forced)
    close(forced, torch.relu(conv_want(key, x, w, scale, shift)), mode, f"conv3x3_mfma tile form {form_id} {Cin} -> {Cout} {H} x {W}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Cin,Cout,Hs,Ws", [(24, 40, 18, 40), (7, 24, 5, 7)])
def test_conv3x3_mfma_pooled_source(dev, Cin, Cout, Hs, Ws, mode):
    """MaxPool2d(2, 2) read by the staging loop; 5 x 7 -> 2 x 3 drops the odd row and column (floor)."""
    key = ("pooled", Cin, Cout, Hs, Ws)
    x, w, scale, shift = conv_case(key, Cin, Cout, Hs, Ws)
    src = R.maxpool2(x.double())
    assert tuple(src.shape[1:3]) == (Hs // 2, Ws // 2)
    assert torch.equal(src.float(), torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    y = run_conv(dev, x, w, scale, shift, mode, True, 1)
    close(y, torch.relu(conv_want(key, src, w, scale, shift)), mode, f"conv3x3_mfma pooled {Cin} -> {Cout} from {Hs} x {Ws}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_conv3x3_mfma_upsampled_source(dev, mode):
    """nn.Upsample(scale_factor=2) (nearest) read by the staging loop."""
    key = ("up", 24, 12, 3, 5)
    x, w, scale, shift = conv_case(key, 24, 12, 3, 5)
    src = R.upsample2(x.double())
    assert torch.equal(src.float(), torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=2).permute(0, 2, 3, 1))
    y = run_conv(dev, x, w, scale, shift, mode, True, 2)
    close(y, torch.relu(conv_want(key, src, w, scale, shift)), mode, "conv3x3_mfma upsampled 24 -> 12 from 3 x 5")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Ca,Cb", [(24, 24), (40, 7)])
def test_conv3x3_mfma_two_sources(dev, Ca, Cb, mode):
    """torch.cat((a, b), dim=1) read by the staging loop: channels [0, Ca) from a, [Ca, Ca + Cb) from b."""
    key = ("cat", Ca, Cb)
    x, w, scale, shift = conv_case(key, Ca + Cb, 32, 9, 20)
    y = run_conv(dev, x[..., :Ca], w, scale, shift, mode, True, 0, x[..., Ca:])
    close(y, torch.relu(conv_want(key, x, w, scale, shift)), mode, f"conv3x3_mfma two sources {Ca} + {Cb} -> 32 9 x 20")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("form,Cin,Cout,Hs,Ws", [(0, 44, 64, 19, 37), (1, 24, 40, 18, 40), (2, 24, 12, 3, 5), (0, 130, 72, 8, 16)])
def test_conv3x3_mfma_is_bit_identical_per_image(dev, form, Cin, Cout, Hs, Ws, mode):
    """No atomics, and a pixel's arithmetic does not depend on its tile or its image: image 1 of a batch of 3 equals the image alone."""
    key = ("bits", form, Cin, Cout, Hs, Ws)
    x, w, scale, shift = conv_case(key, Cin, Cout, Hs, Ws, n=3)
    y3 = run_conv(dev, x, w, scale, shift, mode, True, form)
    assert torch.equal(y3, run_conv(dev, x, w, scale, shift, mode, True, form))
    y1 = run_conv(dev, x[1:2], w, scale, shift, mode, True, form)
    assert torch.equal(y3[1:2], y1)
    assert not torch.equal(y3[0:1], y1)


def test_conv3x3_mfma_refuses_aliasing_and_unfitting_sources(dev):
    from tante_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 4, 4, 8, device=dev)
    pk = torch.zeros(9 * 64 * 16, dtype=torch.uint8, device=dev)
    assert L.tante_conv3x3_mfma(x.data_ptr(), 8, None, 0, 1, 4, 4, 0, 4, 4, pk.data_ptr(), None, 8, 0, 0, x.data_ptr(), 0, None) == -1
    assert b"must not alias" in L.tante_last_error()
    y = torch.empty_like(x)
    assert L.tante_conv3x3_mfma(x.data_ptr(), 8, None, 0, 1, 4, 4, 1, 4, 4, pk.data_ptr(), None, 8, 0, 0, y.data_ptr(), 0, None) == -2
    assert b"does not give 4 x 4 in form 1" in L.tante_last_error()
    assert L.tante_conv3x3_mfma(x.data_ptr(), 4, None, 4, 1, 4, 4, 0, 4, 4, pk.data_ptr(), None, 8, 0, 0, y.data_ptr(), 0, None) == -1
    assert b"null argument" in L.tante_last_error()


# ---- tante_attn_gate alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(6, 10), (1, 1)])
@pytest.mark.parametrize("C", [64, 512])
def test_attn_gate_against_float64(dev, C, H, W, mode):
    import tante_amd.unet_att as UA
    gate = UA.AttentionBlock(C, C, C // 2).eval()
    keys = list(gate.state_dict().keys())
    sd = R.rule_state_dict(keys, [tuple(v.shape) for v in gate.state_dict().values()])
    gate.load_state_dict(sd, strict=True)
    gen = torch.Generator().manual_seed(C + H)
    g, x = torch.randn(2, H, W, C, generator=gen), 0.3 + torch.randn(2, H, W, C, generator=gen)
    want = R.attention_block(g.double(), x.double(), sd)
    psi = R.gate_psi(g.double(), x.double(), sd)
    assert H * W == 1 or float(psi.std()) > 0.05
    with torch.no_grad():
        y = gate.to(dev).run(g.to(dev), x.to(dev), compute_of(mode), mfma=True)
        y0 = gate.run(g.to(dev), x.to(dev), compute_of(mode), mfma=False)
    close(y, want, mode, f"attn_gate C {C} {H} x {W}")
    close(y0, want, mode, f"attn_gate modular C {C} {H} x {W}")


# ---- components and models against the fixtures ------------------------------------------------------------------------------------------
def component(name):
    import tante_amd.unet_att as UA
    make = {"g22_unetatt_convblock_7_24_5x7": lambda: UA.ConvBlock(7, 24), "g22_unetatt_convblock_40_16_9x20": lambda: UA.ConvBlock(40, 16),
            "g22_unetatt_upconv_24_12_3x5": lambda: UA.UpConv(24, 12), "g22_unetatt_gate_24_12_6x10": lambda: UA.AttentionBlock(24, 24, 12)}[name]
    g, sd, _, _ = keyed_golden(name)
    m = make().eval()
    m.load_state_dict(sd, strict=True)
    return g, m


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("route", [1, 0], ids=["mfma", "im2col"])
@pytest.mark.parametrize("name", ["g22_unetatt_convblock_7_24_5x7", "g22_unetatt_convblock_40_16_9x20", "g22_unetatt_upconv_24_12_3x5",
                                  "g22_unetatt_gate_24_12_6x10"])
def test_component_against_the_fixture(dev, name, route, mode):
    g, m = component(name)
    m = m.to(dev)
    with torch.no_grad(), mode_scope(mode), option("TANTE_UNETATT_MFMA", route, 1):
        y = m(g["x"].to(dev), g["x2"].to(dev)) if "gate" in name else m(g["x"].to(dev))
    close(y, g["y64"], mode, f"{name} route {route}")


_MODELS = {}


def built_model(name, dev):
    if name not in _MODELS:
        import tante_amd
        g, sd, _, _ = keyed_golden(name)
        m = tante_amd.AttentionUNet(**model_kwargs(name)).eval()
        m.load_state_dict(sd, strict=True)
        _MODELS[name] = (g, m.to(dev))
    return _MODELS[name]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("route", [1, 0], ids=["mfma", "im2col"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_against_the_fixture(dev, name, route, mode):
    g, m = built_model(name, dev)
    with torch.no_grad(), option("TANTE_UNETATT_MFMA", route, 1):
        y = m.set_compute(mode)(g["x"].to(dev))
    assert y.shape == g["y64"].shape and y.dtype == torch.float32
    close(y, g["y64"], mode, f"{name} route {route}")


def test_model_takes_bf16_from_autocast(dev):
    name = "g22_unetatt_model_d2_f3_12x20"
    g, m = built_model(name, dev)
    m.set_compute(None)
    with torch.no_grad():
        y32 = m(g["x"].to(dev))
        with mode_scope("bf16"):
            y16 = m(g["x"].to(dev))
        assert torch.equal(y32, m.set_compute("fp32")(g["x"].to(dev))) and torch.equal(y16, m.set_compute("bf16")(g["x"].to(dev)))
    m.set_compute(None)
    assert not torch.equal(y32, y16)
    close(y16, g["y64"], "bf16", f"{name} under autocast")


def test_depth_four_against_the_restatement(dev):
    """Depth 4 has no fixture: the d4 = e4 fall-through of unet_att.py:152-154, rule weights, 8 x 16 (neck 1 x 2), default out_T 4."""
    import tante_amd
    m = tante_amd.AttentionUNet(4, types.SimpleNamespace(n_fields=2, n_spatial_dims=2), depth=4).eval()
    own = m.state_dict()
    sd = R.rule_state_dict(list(own.keys()), [tuple(v.shape) for v in own.values()])
    m.load_state_dict(sd, strict=True)
    x = torch.randn(2, 4, 2, 8, 16, generator=torch.Generator().manual_seed(44)) + 0.2
    want = R.model(x, sd)
    assert tuple(want.shape) == (2, 4, 2, 8, 16)
    m = m.to(dev)
    for mode in ("fp32", "bf16"):
        with torch.no_grad():
            y = m.set_compute(mode)(x.to(dev))
        close(y, want, mode, "attention unet depth 4 8 x 16")


def test_out_of_scope_calls_raise(dev):
    g, m = built_model("g22_unetatt_model_d2_f3_12x20", dev)
    x = g["x"].to(dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="t \\* c"):
            m(x[:, :3])
        with pytest.raises(ValueError, match="multiples of 2 \\*\\* \\(depth - 1\\)"):
            m(x[..., :11, :])
        with pytest.raises(RuntimeError, match="GPU only"):
            m(g["x"])
        m.train()
        with pytest.raises(NotImplementedError, match="inference only"):
            m(x)
        m.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)
