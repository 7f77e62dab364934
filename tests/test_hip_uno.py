"""GPU: tante_uno_block and tante_amd.UNO against the float64 restatement (tests/uno_ref.py) -- the fixtures in both compute modes, a
block sweep beyond them, bit-for-bit determinism over batch position and channel slices, the refusals, and autocast."""
import contextlib

import pytest
import torch

import uno_ref as R
from conftest import max_rel, record_parity, rel_err
from test_uno_cpu import BLOCKS, MIN_SHARE, MODELS, SPECS, keyed_golden, model_kwargs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}
# the block sweep: (Ci, Co, Hi, Wi, Ho, Wo, m1, m2) -- channels 1, 5, 38, 76, 304; no Wi or Wo a multiple of 16; m2 = Wi / 2 + 1 in every
# case; shrinking and growing grids (both launch orders); the fourth case has more than one 64-row and 64-column group in its products and
# bands that overlap wholly (2 m1 = 8 rows on Ho = 4)
SWEEP = [(1, 5, 9, 10, 5, 12, 2, 6), (5, 38, 20, 10, 7, 10, 3, 6), (38, 76, 12, 22, 24, 36, 5, 12), (76, 304, 70, 10, 4, 10, 4, 6),
         (304, 1, 6, 14, 11, 20, 3, 8)]
_REF = {}


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


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(SPECS))
def test_spectral_convolution_matches_the_restatement(dev, name, mode):
    """The error is relative to the spectral path's own output: nothing else is in it."""
    from tante_amd import uno as U
    g, sd, _, _ = keyed_golden(name)
    Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = SPECS[name]
    mod = U.SpectralConv2d_Uno(Ci, Co, Ho, Wo, m1, m2).eval()
    mod.load_state_dict(sd, strict=True)
    mod.to(dev)
    with torch.no_grad(), mode_scope(mode):
        y = mod(g["x"].to(dev))
        y2 = mod(g["x"].to(dev), Ho, Wo)
    assert tuple(y.shape) == (2, Co, Ho, Wo) and torch.equal(y, y2)
    close(y, g["y64"], mode, name)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_matches_the_restatement(dev, name, mode):
    """Both paths carry weight in the fixture (path_share >= 0.2 each), so the error relative to the output bounds each path's own."""
    from tante_amd import uno as U
    g, sd, _, _ = keyed_golden(name)
    Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = BLOCKS[name]
    assert float(g["path_share"].min()) >= MIN_SHARE
    mod = U.OperatorBlock_2D(Ci, Co, Ho, Wo, m1, m2).eval()
    mod.load_state_dict(sd, strict=True)
    mod.to(dev)
    with torch.no_grad(), mode_scope(mode):
        y = mod(g["x"].to(dev))
    close(y, g["y64"], mode, name)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_model_matches_the_restatement(dev, name, mode):
    import tante_amd
    g, sd, _, _ = keyed_golden(name)
    m = tante_amd.UNO(**model_kwargs(name)).eval()
    m.load_state_dict(sd, strict=True)
    m.to(dev).set_compute(mode)
    with torch.no_grad():
        y = m(g["x"].to(dev))
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g["y64"].shape)
    close(y, g["y64"], mode, name)


def sweep_case(case):
    """-> (x, state dict, float64 truth) of a sweep case, computed once; the spectral weights are scaled so that both paths carry weight."""
    if case not in _REF:
        Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = case
        gen = torch.Generator().manual_seed(sum(case))
        x = torch.randn(3, Ci, Hi, Wi, generator=gen) + 0.3
        w = [torch.complex(torch.randn(Ci, Co, m1, m2, generator=gen), torch.randn(Ci, Co, m1, m2, generator=gen)) for _ in range(2)]
        sd = {"conv.weights1": w[0], "conv.weights2": w[1], "w.conv.weight": torch.randn(Co, Ci, 1, 1, generator=gen) / Ci ** 0.5,
              "w.conv.bias": 0.2 * torch.randn(Co, generator=gen)}
        parts = []
        R.block(x, sd, "", Ho, Wo, parts)
        scale = R.rms(parts[0][1]) / R.rms(parts[0][0])
        sd["conv.weights1"], sd["conv.weights2"] = w[0] * scale, w[1] * scale
        parts = []
        y = R.block(x, sd, "", Ho, Wo, parts)
        s, p = parts[0]
        assert min(R.rms(s), R.rms(p)) / R.rms(s + p) >= MIN_SHARE
        _REF[case] = (x, sd, y)
    return _REF[case]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "x".join(str(v) for v in c))
def test_block_sweep_matches_the_restatement(dev, case):
    from tante_amd import uno as U
    Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = case
    assert m2 == Wi // 2 + 1 and Wi % 16 and Wo % 16
    x, sd, want = sweep_case(case)
    mod = U.OperatorBlock_2D(Ci, Co, Ho, Wo, m1, m2).eval()
    mod.load_state_dict(sd, strict=True)
    mod.to(dev)
    with torch.no_grad():
        y = mod(x.to(dev))
    close(y, want, "fp32", "sweep " + "x".join(str(v) for v in case))


def det_block(dev, name="g23_uno_block_6_7_20x24_9x11_m3x4"):
    from tante_amd import uno as U
    g, sd, _, _ = keyed_golden(name)
    Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = BLOCKS[name]
    mod = U.OperatorBlock_2D(Ci, Co, Ho, Wo, m1, m2).eval()
    mod.load_state_dict(sd, strict=True)
    return mod.to(dev), g["x"].to(dev), (Ci, Co, Hi, Wi, Ho, Wo)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_an_image_gives_the_same_bits_at_every_batch_position(dev, name):
    """Alone, and at positions 1 and 9 of a batch of 10: two passes of 8 of the mode mix."""
    mod, x, (Ci, Co, Hi, Wi, Ho, Wo) = det_block(dev, name)
    gen = torch.Generator().manual_seed(5)
    batch = torch.randn(10, Ci, Hi, Wi, generator=gen).to(dev)
    batch[1], batch[9] = x[0], x[0]
    with torch.no_grad():
        alone = mod(x[:1])
        many = mod(batch)
    assert torch.equal(many[1], alone[0]) and torch.equal(many[9], alone[0])
    assert not torch.equal(many[0], alone[0])


@pytest.mark.parametrize("name", list(BLOCKS))
def test_channel_slices_give_the_same_bits_as_dense_tensors(dev, name):
    """Written into, and read from, a channel slice of a wider channels-first buffer; the rest of the buffer is untouched."""
    mod, x, (Ci, Co, Hi, Wi, Ho, Wo) = det_block(dev, name)
    with torch.no_grad():
        dense = mod(x)
        wide = torch.full((2, Co + 5, Ho, Wo), 7.5, device=dev)
        mod.run(x, wide[:, 3:3 + Co])
        assert torch.equal(wide[:, 3:3 + Co], dense)
        assert bool((wide[:, :3] == 7.5).all()) and bool((wide[:, 3 + Co:] == 7.5).all())
        src = torch.full((2, Ci + 4, Hi, Wi), float("nan"), device=dev)
        src[:, 2:2 + Ci] = x
        out = torch.empty_like(dense)
        mod.run(src[:, 2:2 + Ci], out)
        assert torch.equal(out, dense)


def test_refusals_return_minus_two_and_touch_nothing(dev):
    """Every refusal of the header: _supported answers 0 for the ones it can see (sizes, modes, strides), the entry point returns -2 for all
    of them, alignment and overlap included, and the output keeps its sentinel."""
    from tante_amd import _lib
    from tante_amd import uno as U
    L = _lib.lib()
    B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = 2, 4, 4, 8, 8, 8, 8, 2, 3
    x = torch.randn(B, Ci, Hi, Wi, device=dev)
    big = torch.full((4096,), 3.25, device=dev)
    w = torch.view_as_real(torch.complex(torch.randn(Ci, Co, 8, 5), torch.randn(Ci, Co, 8, 5))).contiguous().to(dev)
    tables = U.block_tables(Hi, Wi, Ho, Wo, m1, m2, False).to(dev)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(B=B, Ci=Ci, Co=Co, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, m1=m1, m2=m2, xs=Ci * Hi * Wi, os_=Co * Ho * Wo, x=x.data_ptr(), out=big.data_ptr(),
                 w1=w.data_ptr())
        a.update(kw)
        sup = int(L.tante_uno_block_supported(a["B"], a["Ci"], a["Co"], a["Hi"], a["Wi"], a["Ho"], a["Wo"], a["m1"], a["m2"], a["xs"], a["os_"]))
        rc = int(L.tante_uno_block(a["x"], a["xs"], a["B"], a["Ci"], a["Co"], a["Hi"], a["Wi"], a["Ho"], a["Wo"], a["m1"], a["m2"], tables.data_ptr(),
                                   a["w1"], w.data_ptr(), None, None, 0, a["out"], a["os_"], work.data_ptr(), work.numel(), stream))
        torch.cuda.synchronize()
        return sup, rc
    assert call() == (1, 0) and not bool((big[:B * Co * Ho * Wo] == 3.25).any())                  # the same call, accepted, writes
    big.fill_(3.25)
    for kw in (dict(m2=6), dict(m2=5, Wo=6), dict(m1=9, Ho=16), dict(m1=5, Ho=4), dict(Hi=513), dict(Wo=0), dict(Ci=513), dict(B=20000), dict(xs=255),
               dict(os_=255), dict(m1=0)):
        assert call(**kw) == (0, -2), kw
    for kw in (dict(x=x.data_ptr() + 2), dict(out=big.data_ptr() + 2), dict(w1=w.data_ptr() + 4)):                  # alignment
        assert call(**kw) == (1, -2), kw
    xb = big[:B * Ci * Hi * Wi]
    for kw in (dict(x=xb.data_ptr()), dict(x=xb.data_ptr(), out=big.data_ptr() + 4 * 100)):                         # the output overlaps the input
        assert call(**kw) == (1, -2), kw
        assert b"overlaps the input" in L.tante_last_error()
    assert bool((big == 3.25).all())
    with pytest.raises(ValueError, match="cannot hold its 2 x 6 modes"):
        U.uno_block(x, torch.empty(B, Co, Ho, Wo, device=dev), 2, 6, torch.zeros(Ci, Co, 2, 6, dtype=torch.complex64, device=dev),
                    torch.zeros(Ci, Co, 2, 6, dtype=torch.complex64, device=dev), None, None, False)


def test_model_takes_bf16_from_autocast(dev):
    import tante_amd
    name = "g23_uno_model_w4_f1_128x256"
    g, sd, _, _ = keyed_golden(name)
    m = tante_amd.UNO(**model_kwargs(name)).eval()
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    x = g["x"].to(dev)
    with torch.no_grad():
        y32 = m(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ya = m(x)
        yb = m.set_compute("bf16")(x)
        m.set_compute(None)
    assert torch.equal(ya, yb) and not torch.equal(ya, y32)
    assert 1e-5 < rel_err(ya, y32) < 1e-2
