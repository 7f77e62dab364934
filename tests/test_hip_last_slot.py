"""GPU tests: the last Taylor order's backbone finishes only the rows of time slot T - 1 (TANTE_LAST_SLOT).

* tante_block_fused_last -- the T letter (L = 4) writing only the rows at slot 3 of its sequences, with and without the temporal
  propagator: those rows equal the full launch's bit for bit, every other row is left byte for byte as it was.
* the H and W letters on the slot-(T - 1) sub-grid (kernels.block_fused_subgrid): the slot-(T - 1) rows equal the full launch's, the
  other slots are untouched.
* TANTE rollouts with the option off and on: cfg2-shaped (order 3, THW-THW-THW) at B = 2 and 8, every call's enc_next included, cfg3
  (order 1, THWTHWTHW), and the captured-graph rollout -- all bit-identical; and the launches the last order takes.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _block(dev, seed):
    import tante_amd
    torch.manual_seed(seed)
    blk = tante_amd.TransformerBlock(256, 8, 1.0, 0.0).to(dev).eval()
    with torch.no_grad():      # LayerNorm affines away from (1, 0), so that the folded weights are exercised
        for ln in (blk.ln1, blk.ln2):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.uniform_(-0.2, 0.2)
    return blk


def _slots(x, B, T, HW):
    return x.view(B, T, HW, -1)


@pytest.mark.parametrize("tprop", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (3, 32, 32), (8, 32, 32), (1, 3, 5)])
def test_last_slot_t_letter_kernel(dev, tprop, B, H, W):
    """B = 1 / 3 / 8 at 32 x 32: the half-size and the full-size geometry; 3 x 5 planes: 15 sequences, the last workgroup partial."""
    from tante_amd import kernels as K, _lib as L
    T, HW = 4, H * W
    blk = _block(dev, 7 + B)
    assert blk.fused_inference(T, L.BF16) and K.block_fused_last_supported(256, 8, 256, T)
    x = torch.randn(B * T * HW, 256, device=dev) * 1.5 + 0.3
    tp = (torch.randn(40, device=dev) * 0.5).contiguous() if tprop else None
    seq = K.make_seq("T", B, T, H, W)
    xf, xl = x.clone(), x.clone()
    with torch.no_grad():
        blk.forward_tokens(xf, seq, True, L.BF16, tp)
        blk.forward_last_slot(xl, seq, True, tp)
    torch.cuda.synchronize()
    sf, sl, s0 = _slots(xf, B, T, HW), _slots(xl, B, T, HW), _slots(x, B, T, HW)
    assert not torch.equal(sf[:, T - 1], s0[:, T - 1])
    assert torch.equal(sl[:, T - 1], sf[:, T - 1])
    assert torch.equal(sl[:, :T - 1], s0[:, :T - 1])


@pytest.mark.parametrize("letter", ["H", "W"])
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (3, 32, 32), (8, 32, 32), (2, 6, 10)])
def test_subgrid_h_w_letters(dev, letter, B, H, W):
    from tante_amd import kernels as K, _lib as L
    T, HW = 4, H * W
    blk = _block(dev, 11 + B)
    sub = K.last_slot_seq(letter, B, T, H, W)
    assert blk.fused_inference(sub.L, L.BF16)
    x = torch.randn(B * T * HW, 256, device=dev) - 0.2
    xf, xs = x.clone(), x.clone()
    with torch.no_grad():
        blk.forward_tokens(xf, K.make_seq(letter, B, T, H, W), False, L.BF16)
        blk.forward_subgrid(xs, (T - 1) * HW, sub, False)
    torch.cuda.synchronize()
    sf, ss, s0 = _slots(xf, B, T, HW), _slots(xs, B, T, HW), _slots(x, B, T, HW)
    assert not torch.equal(sf[:, T - 1], s0[:, T - 1])
    assert torch.equal(ss[:, T - 1], sf[:, T - 1])
    assert torch.equal(ss[:, :T - 1], s0[:, :T - 1])


def _model(dev, cfg_name, n_fields=None, res=None):
    import tante_amd
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", cfg_name))
    wl = cfg["workload"]
    md = tante_amd.TanteMetadata(n_fields=n_fields or wl["n_fields"], spatial_resolution=tuple(res or wl["spatial_resolution"]))
    torch.manual_seed(cfg.get("seed", 211))
    m = tante_amd.build_model(cfg, md).to(dev).eval().set_compute("bf16")
    return m, md, wl


def _batch(dev, md, B, T_in, n_steps, seed):
    g = torch.Generator().manual_seed(seed)
    res, D = tuple(md.spatial_resolution), md.n_fields
    return {"input": torch.randn(B, T_in, *res, D, generator=g).to(dev), "output": torch.randn(B, n_steps, *res, D, generator=g).to(dev)}


def _rollout_with(model, batch, fmt, n, on, record=None):
    import tante_amd
    tante_amd.set_option("TANTE_LAST_SLOT", int(on))
    try:
        with torch.inference_mode():
            y, yr = tante_amd.rollout_model(model, batch, fmt, n)
        torch.cuda.synchronize()
        return y.clone(), yr.clone()
    finally:
        tante_amd.set_option("TANTE_LAST_SLOT", 1)


@pytest.mark.parametrize("B", [2, 8])
def test_cfg2_rollout_bit_identical(dev, monkeypatch, B):
    """cfg2's model (256 x 256 x 11, order 3, THW-THW-THW), 8-step rollout: y_pred and every call's re-encoded frame (enc_next) equal
    the full path's bit for bit."""
    import tante_amd
    from tante_amd import tante as TT
    m, md, wl = _model(dev, "tante_am.yaml")
    batch = _batch(dev, md, B, wl["n_steps_input"], 8, 100 + B)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    seen = []
    orig = TT.TANTE.forward

    def fwd(self, *a, **kw):
        r = orig(self, *a, **kw)
        if kw.get("enc_next") is not None:
            seen.append(kw["enc_next"].clone())
        return r
    monkeypatch.setattr(TT.TANTE, "forward", fwd)
    y0, r0 = _rollout_with(m, batch, fmt, 8, False)
    e0, seen[:] = list(seen), []
    y1, r1 = _rollout_with(m, batch, fmt, 8, True)
    e1 = list(seen)
    assert torch.isfinite(y0).all()
    assert torch.equal(y1, y0) and torch.equal(r1, r0)
    assert len(e0) == len(e1) > 0
    for a, b in zip(e0, e1):
        assert torch.equal(a, b)


def test_cfg3_rollout_bit_identical(dev):
    import tante_amd
    m, md, wl = _model(dev, "tante_trl.yaml")
    batch = _batch(dev, md, 2, wl["n_steps_input"], 8, 303)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    y0, _ = _rollout_with(m, batch, fmt, 8, False)
    y1, _ = _rollout_with(m, batch, fmt, 8, True)
    assert torch.isfinite(y0).all()
    assert torch.equal(y1, y0)


def test_graphed_rollout_equals_eager(dev):
    import tante_amd
    m, md, wl = _model(dev, "tante_am.yaml")
    batch = _batch(dev, md, 2, wl["n_steps_input"], 8, 404)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    assert tante_amd.get_option("TANTE_LAST_SLOT")
    ye, _ = _rollout_with(m, batch, fmt, 8, True)
    roll = tante_amd.GraphedRollout(m, batch, fmt, 8)
    yg, _ = roll(batch)
    torch.cuda.synchronize()
    assert torch.equal(yg, ye)


def test_last_order_launches(dev, monkeypatch):
    """One cfg2 call: orders 1 and 2 run their 6 blocks as full launches, the last order 1 last-slot T launch and 2 sub-grid launches;
    with the option off, 9 full launches."""
    import tante_amd
    from tante_amd import kernels as K
    m, md, wl = _model(dev, "tante_am.yaml", res=(64, 64))
    x = torch.randn(2, wl["n_steps_input"], md.n_fields, 64, 64, device=dev)
    counts = {}
    for name in ("block_fused", "block_fused_last", "block_fused_subgrid"):
        orig = getattr(K, name)

        def wrap(*a, _o=orig, _n=name, **kw):
            counts[_n] = counts.get(_n, 0) + 1
            return _o(*a, **kw)
        monkeypatch.setattr(K, name, wrap)
    res = {}
    for on in (1, 0):
        tante_amd.set_option("TANTE_LAST_SLOT", on)
        try:
            counts.clear()
            with torch.inference_mode():
                res[on] = m(x)
            torch.cuda.synchronize()
            got = dict(counts)
        finally:
            tante_amd.set_option("TANTE_LAST_SLOT", 1)
        want = {"block_fused": 6, "block_fused_last": 1, "block_fused_subgrid": 2} if on else {"block_fused": 9}
        assert got == want, (on, got)
    assert torch.equal(res[1], res[0])
