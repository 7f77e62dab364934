"""The column-block schedule of the whole-tile H + W propagator (axis_hw_exact_kernel, TANTE_AXIS_BLOCKS) against the one-block schedule
it replaces (TANTE_AXIS_BLOCKS=0): same arithmetic in the same order, so the planes must agree bit for bit; and against the fp64 torch
expression of the two propagators with the inputs and the bf16 bar of test_hip_parity.py::test_axis_hw_fused.

Planes: the smallest at which the block logic can go wrong.  BT = 3 planes (odd) everywhere.  With BT = 3 the launcher picks 16-channel
tiles and 8 waves; the `ct32` cases force the 32-channel, 16-wave form that the rollout runs (TANTE_AXIS_CT=32).
  (16, 16) C 32       one MFMA tile per axis: one DMA instruction per row, the schedule falls back to one block
  (32, 32) C 32, 64   the rollout's tile at 2 / 4 channel tiles (6 / 12 workgroups: gridDim % 8 != 0)
  (32, 32) C 128      24 workgroups: gridDim % 8 == 0, the XCD-major remap
  (16, 32), (32, 16)  non-square, both ways round (the second has one DMA instruction per row: one block)
  (64, 32) C 16       the largest MTH that fits 160 KiB (no room for the raw weights beside it: one block)

The FiLM-on-load form (axis_hw_film) is compared here with its own one-block schedule only; its float64 check -- B != T, a window inside
a wider cache, a FiLM table per slot, s_emb per token -- is tests/test_hip_axis_nodes.py::test_film_on_load_against_float64.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BT = 3
TOL_BF16 = 1e-2          # test_hip_parity.TOL["bf16"]: rel < TOL, max < 2 TOL
CASES = [(16, 16, 32, 0), (32, 32, 32, 0), (32, 32, 64, 0), (32, 32, 128, 0), (16, 32, 32, 0), (32, 16, 32, 0), (64, 32, 16, 0),
         (32, 32, 64, 32), (16, 32, 32, 32)]
IDS = [f"{h}x{w}-C{c}" + ("-ct32" if ct else "") for h, w, c, ct in CASES]
KEYS = ("p.0.weight", "p.0.bias", "p.2.weight", "p.2.bias")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(nH, nW, C):
    """test_axis_hw_fused's inputs: same generator seed, same draws in the same order."""
    g = torch.Generator().manual_seed(nH * 100 + nW)
    x = torch.randn(BT, nH, nW, C, generator=g)

    def mk(n):
        return {"p.0.weight": torch.randn(n, n, generator=g) / math.sqrt(n), "p.0.bias": 0.3 * torch.randn(n, generator=g),
                "p.2.weight": torch.randn(n, n, generator=g) / math.sqrt(n), "p.2.bias": 0.3 * torch.randn(n, generator=g)}
    return x, mk(nH), mk(nW)


class _Options:
    """Set library options for the block; put back what was there."""

    def __init__(self, **kw):
        self.kw = kw

    UNSET = {"TANTE_AXIS_BLOCKS": -1, "TANTE_AXIS_CT": 0, "TANTE_AXIS_GENERIC": 0}       # the values that mean "the launcher's own choice"

    def __enter__(self):
        from tante_amd import _lib as L
        self.old = {k: L.get_option(k, self.UNSET[k]) for k in self.kw}
        for k, v in self.kw.items():
            L.set_option(k, v)

    def __exit__(self, *a):
        from tante_amd import _lib as L
        for k, v in self.old.items():
            L.set_option(k, v)


def _run(variant, dev, nH, nW, C, x, wh, ww, blocks, ct):
    from tante_amd import kernels as K, _lib as L
    vp, hp = [wh[k].to(dev) for k in KEYS], [ww[k].to(dev) for k in KEYS]
    opts = {"TANTE_AXIS_CT": ct}
    if blocks is not None:
        opts["TANTE_AXIS_BLOCKS"] = blocks
    with _Options(**opts):
        if variant == "axis_hw":
            out = K.axis_hw(x.to(dev), BT, nH, nW, C, vp, hp, L.BF16)
        elif variant == "axis_hw_oop":
            xin = x.to(dev)
            out = K.axis_hw_oop(xin, torch.full_like(xin, float("nan")), BT, nH, nW, C, vp, hp, L.BF16)
            assert torch.equal(xin.cpu(), x), "the out-of-place form must leave its input alone"
        else:       # axis_hw_film: T = 3 slots of one batch entry, every slot with a FiLM table of its own
            g = torch.Generator().manual_seed(7)
            T = BT
            fa, fb = 1 + 0.5 * torch.randn(T, C, generator=g), torch.randn(T, C, generator=g)
            se = torch.randn(nH * nW, C, generator=g)
            src = x.reshape(T, 1, nH * nW, C).contiguous()
            out = torch.full((BT, nH, nW, C), float("nan"), device=dev)
            K.axis_hw_film(out, src.to(dev), nH * nW * C, nH * nW * C, (fa.to(dev), fb.to(dev), se.to(dev), T, nH * nW), BT, nH, nW, C,
                           vp, hp, L.BF16)
        torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("variant", ["axis_hw", "axis_hw_oop", "axis_hw_film"])
@pytest.mark.parametrize("nH,nW,C,ct", CASES, ids=IDS)
def test_blocks_bit_identical(dev, variant, nH, nW, C, ct):
    from tante_amd import kernels as K, _lib as L
    if not K.axis_hw_supported(nH, nW, C, L.BF16):
        pytest.skip("the plane does not fit the LDS")
    x, wh, ww = _inputs(nH, nW, C)
    one = _run(variant, dev, nH, nW, C, x, wh, ww, 0, ct)
    blk = _run(variant, dev, nH, nW, C, x, wh, ww, None, ct)
    assert torch.isfinite(one).all()
    assert torch.equal(one, blk)
    if variant == "axis_hw_film":          # a wrong slot t shows: the slots' planes differ by their FiLM tables alone
        assert not torch.equal(one[0], one[1]) and not torch.equal(one[1], one[2])


@pytest.mark.parametrize("nH,nW,C,ct", CASES, ids=IDS)
def test_blocks_against_fp64(dev, nH, nW, C, ct):
    """x + W2 gelu(W1 x + b1) + b2 along h, then along w, in float64; the bar of test_axis_hw_fused for bf16 compute."""
    from tante_amd import kernels as K, _lib as L
    if not K.axis_hw_supported(nH, nW, C, L.BF16):
        pytest.skip("the plane does not fit the LDS")
    x, wh, ww = _inputs(nH, nW, C)

    def prop(p, v, dim):      # the axis MLP on dimension `dim` of v
        v = v.movedim(dim, -1)
        h = torch.nn.functional.gelu(v @ p["p.0.weight"].double().t() + p["p.0.bias"].double())
        return (h @ p["p.2.weight"].double().t() + p["p.2.bias"].double()).movedim(-1, dim)
    ref = x.double()
    ref = ref + prop(wh, ref, 1)
    ref = ref + prop(ww, ref, 2)
    out = _run("axis_hw", dev, nH, nW, C, x, wh, ww, None, ct).double()
    rel = float((out - ref).norm() / ref.norm())
    mx = float((out - ref).abs().max() / ref.abs().max())
    print(f"{nH}x{nW} C={C} ct={ct}: rel {rel:.3e} max {mx:.3e}")
    assert rel < TOL_BF16 and mx < 2 * TOL_BF16, f"rel={rel:.3e} max={mx:.3e}"
