"""CPU: the host side of the trainable AFNO -- the adjoint twiddle tables, the new entry points and their refusals, the opt-in surface,
and the float64 gradient restatement (tests/afno_grad_ref.py) against afno_ref's own autograd, with the band-share cap of every GPU
case of tests/test_hip_afno_train.py checked here without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import afno_grad_ref as G
import afno_ref as R
from conftest import ROOT

ENTRIES = ("tante_afno_twiddle_bwd_floats", "tante_afno_filter_bwd_workspace_bytes", "tante_afno_filter_bwd")
GRIDS = [(7, 9), (12, 5), (5, 12), (64, 33), (33, 64), (1, 1), (64, 64), (4, 6)]


@pytest.fixture(scope="module")
def lib():
    from tante_amd import _lib
    from tante_amd.build import build
    build()
    return _lib.lib()


@pytest.mark.parametrize("H,W", GRIDS)
def test_adjoint_tables_are_the_conjugate_transposes(lib, H, W):
    """pack_twiddles_bwd: per table the conjugate transpose of the float64 table, rounded once, zero padded to 16 x 4 fragments, in the
    forward's order; as many floats as the library counts."""
    import tante_amd.afno as A
    buf = A.pack_twiddles_bwd(H, W)
    assert buf.dtype == np.float32 and buf.size == int(lib.tante_afno_twiddle_bwd_floats(H, W))
    Lc, Kc = A.kept_modes(H, W)
    tabs = A.twiddle_tables(H, W)
    assert [t.shape for t in tabs] == [(Lc, W), (Kc, H), (W, Kc), (H, Lc)]
    off = 0
    for t in tabs:
        a = np.conj(t).T                                   # float64
        Mp, Kp = -(-a.shape[0] // 16) * 16, -(-a.shape[1] // 4) * 4
        planes = buf[off:off + 2 * Mp * Kp].reshape(2, Mp, Kp)
        off += 2 * Mp * Kp
        want = np.zeros((2, Mp, Kp))
        want[0, :a.shape[0], :a.shape[1]], want[1, :a.shape[0], :a.shape[1]] = a.real, a.imag
        assert np.array_equal(planes, want.astype(np.float32))
    assert off == buf.size
    assert A.pack_twiddles(H, W).size == int(lib.tante_afno_twiddle_floats(H, W))      # the forward's tables did not move


def test_entry_points_are_declared_bound_and_exported(lib):
    from tante_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 14 and lib.tante_abi_version() == 14
    # the forward's entries and its workspace formula are what they were
    assert len(_lib.SIGNATURES["tante_afno_filter"][0]) == 15 and len(_lib.SIGNATURES["tante_afno_filter_workspace_bytes"][0]) == 4
    assert lib.tante_afno_filter_workspace_bytes(2, 7, 9, 40) == 4 * 2 * 2 * 7 * (7 + 9) * 40


def test_refusals_without_a_launch(lib):
    """Null pointers throughout: an unsupported shape is refused with -2 and the forward's reason, a supported one with -1."""
    def call(B, H, W, C, bs):
        return lib.tante_afno_filter_bwd(None, None, B, H, W, C, bs, None, None, None, None, 0.01, None, None, None, 0, None, None, 0, None)
    for shape, why in (((1, 65, 8, 64, 32), "token grid outside 1..64"), ((1, 8, 65, 64, 32), "token grid outside 1..64"),
                       ((1, 8, 8, 130, 65), "channel block size outside 1..64"), ((1, 8, 8, 40, 16), "not a whole number of blocks"),
                       ((65536, 8, 8, 64, 32), "more than 65535 samples")):
        assert call(*shape) == -2, shape
        msg = lib.tante_last_error().decode()
        assert msg.startswith("tante_afno_filter_bwd: ") and why in msg, msg
    assert call(1, 8, 8, 64, 32) == -1 and "null argument" in lib.tante_last_error().decode()
    assert lib.tante_afno_twiddle_bwd_floats(65, 8) == -1 and lib.tante_afno_twiddle_bwd_floats(8, 0) == -1
    assert lib.tante_afno_filter_bwd_workspace_bytes(1, 65, 8, 64, 32) == -1
    assert lib.tante_afno_filter_bwd_workspace_bytes(1, 8, 8, 40, 16) == -1
    # dG (B, W, Lc, 2, C) + dP (B, Lc, H, 2, C) + two sets of (B Lc) partials of (C / bs, bs, bs, 2) floats
    assert lib.tante_afno_filter_bwd_workspace_bytes(2, 7, 9, 40, 8) == 4 * (2 * 2 * 7 * (7 + 9) * 40 + 2 * (2 * 7) * 5 * 8 * 8 * 2)


def test_opt_in_surface():
    """set_trainable returns self, reaches every Block and AFNO_ND, is neither a constructor argument nor in the state_dict; without it the
    pinned refusal stands, with it the call gets as far as the device check; dropout in train() refuses either way."""
    import inspect
    import tante_amd
    import tante_amd.afno as A
    m, _, x = G.model_case()
    keys = set(m.state_dict())
    assert "trainable" not in inspect.signature(tante_amd.AFNO.__init__).parameters
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m(x)
    assert m.set_trainable() is m and set(m.state_dict()) == keys
    assert all(b._trainable and b.filter._trainable for b in m.blocks)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    assert m.set_trainable(False) is m and not any(b._trainable or b.filter._trainable for b in m.blocks)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m(x)
    blk = m.blocks[0]
    assert blk.set_trainable() is blk and blk.filter._trainable and blk.filter.set_trainable(False) is blk.filter
    d = tante_amd.AFNO(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 24)), drop_rate=0.1, **G.MODEL_KW).set_trainable()
    with pytest.raises(NotImplementedError, match="drop_rate / drop_path_rate"):
        d.train()(x)
    with pytest.raises(NotImplementedError, match="drop_rate / drop_path_rate"):
        d.blocks[0].train()(torch.randn(1, 4, 6, 32))
    assert callable(A.afno_train_forward) and callable(A.record_keep_masks) and hasattr(A.AfnoFilterFn, "apply")
    sink = []
    with A.record_keep_masks(sink) as s:
        assert s is sink and A._KEEP_SINK[0] is sink
    assert A._KEEP_SINK[0] is None and sink == []


@pytest.mark.parametrize("B,H,W,C,bs", G.FILTER_CASES)
def test_restatement_with_float64_masks_is_afno_ref(B, H, W, C, bs):
    """With keep = |Yp| > lam the restatement is afno_ref.afno_filter: the same output and the same autograd gradients, bit for bit.  And
    this case's band share is under the cap, its zeroed share inside 0.1 .. 0.9 (grids of more than one point)."""
    x, _, w1, w2, dout = G.filter_case(B, H, W, C, bs)
    g = dout.transpose(1, 2).to(G.DT)
    grads = []
    for fn in (lambda a, b, c: R.afno_filter(a, b, c, 0.01), lambda a, b, c: G.afno_filter(a, b, c, 0.01)):
        leaves = [t.detach().to(G.DT).clone().requires_grad_(True) for t in (x, w1, w2)]
        y = fn(*leaves)
        grads.append((y.detach(), *torch.autograd.grad(y, leaves, g)))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert float(grads[0][1].abs().max()) > 0 and float(grads[0][2].abs().max()) > 0 and float(grads[0][3].abs().max()) > 0
    Yp = G.pre_threshold(x.to(G.DT), w1, w2)
    share = G.band_share(Yp, 0.01, H, W)
    print(f"band share {share:.3e} (cap {G.BAND_SHARE:.1e})")
    assert share <= G.BAND_SHARE
    if H * W > 1:
        assert 0.1 <= R.zeroed_share(x, w1, w2, 0.01) <= 0.9
    else:
        assert share == 0.0


def test_band_share_of_the_model_and_rollout_cases():
    """The model of the GPU tests, one call and the 2-step re-fed rollout: every block call's band share under the cap and its zeroed
    share inside 0.1 .. 0.9; with float64's own masks the restated model is afno_ref.model."""
    _, sd, x = G.model_case()
    sh = G.Shares()
    sd64 = {k: v.to(G.DT) for k, v in sd.items()}
    y = G.model(x.to(G.DT), sd64, G.MODEL_KW["patch_size"], 0.01, sh)
    assert torch.equal(y, R.model(x, sd, G.MODEL_KW["patch_size"]))
    G.rollout(x.to(G.DT), sd64, G.MODEL_KW["patch_size"], 2, 0.01, sh)
    assert len(sh.band) == 2 + 4
    print("band shares", sh.band, "zeroed shares", sh.zeroed)
    assert max(sh.band) <= G.BAND_SHARE
    assert all(0.1 <= z <= 0.9 for z in sh.zeroed)
