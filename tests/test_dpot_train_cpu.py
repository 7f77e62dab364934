"""CPU: the host side of the trainable DPOT -- the adjoint twiddle tables, the new entry points, their predicates and refusals, the opt-in
surface, and the float64 restatement of the backward decomposition (tests/dpot_grad_ref.py) against float64 autograd of tests/dpot_ref.py
for the filter, GroupNorm and the 'exp_mlp' fold; and that every filter case of the GPU tests has a contribution gradient worth comparing."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dpot_grad_ref as G
import dpot_ref as R
from conftest import ROOT
from test_dpot_cpu import MIN_RATIO, MODELS

ENTRIES = ("tante_groupnorm_bwd_supported", "tante_groupnorm_bwd_workspace_bytes", "tante_groupnorm_bwd", "tante_dpot_twiddle_bwd_floats",
           "tante_dpot_filter_bwd_workspace_bytes", "tante_dpot_filter_bwd")
GRIDS = [(7, 9, 3), (5, 12, 4), (12, 5, 20), (12, 16, 12), (16, 10, 16), (1, 1, 5), (8, 8, 16), (64, 33, 20), (33, 64, 64)]
RTOL = 1e-10


@pytest.fixture(scope="module")
def lib():
    from tante_amd import _lib
    from tante_amd.build import build
    build()
    return _lib.lib()


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("H,W,modes", GRIDS)
def test_adjoint_tables_are_the_conjugate_transposes(lib, H, W, modes):
    """pack_twiddles_bwd: per table the conjugate transpose of the float64 table, rounded once, zero padded to 16 x 4 fragments, in the
    forward's order; as many floats as the library counts.  The forward's tables did not move."""
    import tante_amd.dpot as D
    buf = D.pack_twiddles_bwd(H, W, modes)
    assert buf.dtype == np.float32 and buf.size == int(lib.tante_dpot_twiddle_bwd_floats(H, W, modes))
    k1, k2 = D.kept_modes(H, W, modes)
    tabs = D.twiddle_tables(H, W, modes)
    assert [t.shape for t in tabs] == [(k2, W), (k1, H), (H, k1), (W, k2)]
    off = 0
    for t in tabs:
        a = np.conj(t).T
        Mp, Kp = -(-a.shape[0] // 16) * 16, -(-a.shape[1] // 4) * 4
        planes = buf[off:off + 2 * Mp * Kp].reshape(2, Mp, Kp)
        off += 2 * Mp * Kp
        want = np.zeros((2, Mp, Kp))
        want[0, :a.shape[0], :a.shape[1]], want[1, :a.shape[0], :a.shape[1]] = a.real, a.imag
        assert np.array_equal(planes, want.astype(np.float32))
    assert off == buf.size
    fwd = sum(2 * (-(-t.shape[0] // 16) * 16) * (-(-t.shape[1] // 4) * 4) for t in tabs)
    assert D.pack_twiddles(H, W, modes).size == int(lib.tante_dpot_twiddle_floats(H, W, modes)) == fwd


def test_entry_points_are_declared_bound_and_exported(lib):
    from tante_amd import _lib
    from tante_amd.build import SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_lib.SIGNATURES)
    assert "dpot_mixer_bwd.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "tante_amd", "csrc", "dpot_mixer.hip.h"))
    assert _lib.ABI_VERSION == 14 and lib.tante_abi_version() == 14
    assert len(_lib.SIGNATURES["tante_dpot_filter"][0]) == 18 and len(_lib.SIGNATURES["tante_groupnorm"][0]) == 13
    assert len(_lib.SIGNATURES["tante_dpot_filter_bwd"][0]) == 22 and len(_lib.SIGNATURES["tante_groupnorm_bwd"][0]) == 16


def test_predicates_agree_with_their_python_mirrors(lib):
    import tante_amd.dpot as D
    for B, HW, C, G_ in [(2, 35, 48, 8), (1, 4096, 64, 8), (1, 4097, 64, 8), (1, 0, 64, 8), (1, 4, 20, 8), (0, 4, 16, 8), (-1, 4, 16, 8),
                         (1, 4, 16, 0), (2 ** 28, 4, 16, 8), (1, 4, (1 << 24) + 8, 8)]:
        assert bool(lib.tante_groupnorm_bwd_supported(B, HW, C, G_)) == D.groupnorm_bwd_supported_py(B, HW, C, G_) \
            == bool(lib.tante_groupnorm_supported(B, HW, C, G_)), (B, HW, C, G_)
        assert (lib.tante_groupnorm_bwd_workspace_bytes(B, HW, C, G_) >= 0) == D.groupnorm_bwd_supported_py(B, HW, C, G_)
    for B, H, W, C, bs, modes in [(2, 7, 9, 48, 6, 3), (1, 65, 8, 64, 32, 4), (1, 8, 65, 64, 32, 4), (1, 8, 8, 1026, 513, 4), (1, 8, 8, 40, 16, 4),
                                  (1, 8, 8, 64, 32, 0), (65536, 8, 8, 64, 32, 4), (0, 8, 8, 64, 32, 4)]:
        ok = D.filter_supported_py(B, H, W, C, bs, modes)
        assert (lib.tante_dpot_filter_bwd_workspace_bytes(B, H, W, C, bs, modes) >= 0) == ok, (B, H, W, C, bs, modes)
    # statistics + group sums per (b, g, slab), then the per-channel partials per (b, slab): (2, 35, 48, 8) is one slab
    assert lib.tante_groupnorm_bwd_workspace_bytes(2, 35, 48, 8) == 4 * (2 * 2 * 2 * 8 + 2 * 2 * 48)
    # P (B, k2, H, 2, C) rounded to 4 floats, then X, U, dY, dU (nb, B k1 k2, 2, bsP)
    assert lib.tante_dpot_filter_bwd_workspace_bytes(2, 7, 9, 48, 6, 3) == 4 * (2 * 2 * 3 * 7 * 48 + 4 * 8 * (2 * 3 * 3) * 2 * 16)
    assert lib.tante_dpot_filter_workspace_bytes(2, 7, 9, 48, 6, 3) == 4 * (2 * 2 * 3 * 7 * 48 + 2 * 8 * (2 * 3 * 3) * 2 * 16)


def test_every_refusal_has_its_code_and_message(lib):
    """Null pointers throughout: an unsupported shape is refused with -2 and the forward's reason, a supported one with -1; nothing launches."""
    def filt(B, H, W, C, bs, modes):
        return lib.tante_dpot_filter_bwd(None, None, B, H, W, C, bs, modes, None, None, None, None, None, None, None, None, None, None, 0, None, 0, None)
    for shape, why in (((1, 65, 8, 64, 32, 4), "token grid outside 1..64"), ((1, 8, 65, 64, 32, 4), "token grid outside 1..64"),
                       ((1, 8, 8, 1026, 513, 4), "channel block size outside 1..512"), ((1, 8, 8, 40, 16, 4), "not a whole number of blocks"),
                       ((1, 8, 8, 64, 32, 0), "modes must be at least 1"), ((65536, 8, 8, 64, 32, 4), "more than 65535 samples")):
        assert filt(*shape) == -2, shape
        msg = lib.tante_last_error().decode()
        assert msg.startswith("tante_dpot_filter_bwd: ") and why in msg, msg
    assert filt(1, 8, 8, 64, 32, 4) == -1 and "null argument" in lib.tante_last_error().decode()
    assert lib.tante_dpot_twiddle_bwd_floats(65, 8, 4) == -1 and lib.tante_dpot_twiddle_bwd_floats(8, 8, 0) == -1

    def gn(B, HW, C, G_, dt=0):
        return lib.tante_groupnorm_bwd(None, dt, None, B, HW, C, G_, 1e-5, None, None, None, None, 0, None, 0, None)
    for shape, why in (((1, 4097, 16, 8), "tokens per sample outside 1..4096"), ((1, 4, 20, 8), "channels are not a whole number of groups"),
                       ((1, 4, (1 << 24) + 8, 8), "more than 2^24 channels"), ((2 ** 28, 4, 16, 8), "more than 2^31 - 1 (sample, group) pairs")):
        assert gn(*shape) == -2, shape
        msg = lib.tante_last_error().decode()
        assert msg.startswith("tante_groupnorm_bwd: ") and why in msg, msg
    from tante_amd import _lib
    assert gn(1, 4, 16, 8, 99) == -1 and "dy must be fp32 or bf16" in lib.tante_last_error().decode()
    assert gn(1, 4, 16, 8, _lib.F32) == -1 and "null argument" in lib.tante_last_error().decode()


@pytest.mark.parametrize("B,H,W,C,nb,modes", G.FILTER_CASES)
def test_restated_filter_backward_is_float64_autograd(B, H, W, C, nb, modes):
    """Adjoint tables, conjugate products, gelu' on the two parts: equal to autograd of dpot_ref.filter_contribution within 1e-10; and the
    contribution's input gradient is at least MIN_RATIO of dout, so the GPU comparison of dx - dout is not one of rounding noise."""
    x, _, ws, dout = G.filter_case(B, H, W, C, nb, modes)
    assert R.contribution_ratio(x, *ws, modes) >= MIN_RATIO
    want = G.filter_autograd(x, ws, dout, modes)[1:]
    got = G.filter_backward_restated(x, ws, dout, modes)
    for name, a, b in zip(("dx", "dw1", "db1", "dw2", "db2"), got, want):
        assert a.shape == b.shape and rel(a, b) < RTOL, (name, rel(a, b))
    ratio = float(want[0].norm() / dout.to(G.DT).norm())
    print(f"|dx - dout| / |dout| = {ratio:.3f}")
    assert ratio >= MIN_RATIO


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("B,HW,C", [(2, 1, 64), (2, 35, 48), (2, 64, 256)])
def test_restated_groupnorm_backward_is_float64_autograd(B, HW, C, affine):
    x, w, b, dy = G.gn_case(B, HW, C, 0.0, affine)
    _, dx, dg, db = G.gn_autograd(x, w, b, dy)
    rx, rg, rb = G.gn_backward_restated(x, w, dy)
    assert rel(rx, dx) < RTOL
    if affine:
        assert rel(rg, dg) < RTOL and rel(rb, db) < RTOL


def test_restated_fold_chain_rule_is_float64_autograd():
    """wf = w cos(t gamma) with gamma = 2^linspace(-10, 10): dw and dgamma of a random d wf, up to gamma = 2^10."""
    T, C = 3, 16
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(T, C, C, generator=gen)
    gamma = (2 ** torch.linspace(-10, 10, C)).unsqueeze(0)
    dwf = torch.randn(T, C, C, generator=gen)
    lw, lg = G.leaves([w, gamma])
    wf = R.time_weight({"time_agg_layer.w": lw, "time_agg_layer.gamma": lg}, T, "exp_mlp")
    want = torch.autograd.grad(wf, [lw, lg], dwf.to(G.DT))
    got = G.fold_backward_restated(dwf, w, gamma)
    assert float(gamma.max()) == 1024.0
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel(a, b) < RTOL


def test_opt_in_surface():
    """set_trainable returns self and reaches every child, is neither a constructor argument nor in the state_dict; without it the pinned
    refusal stands word for word, with it the call gets as far as the device check; trained_parameters omits exactly cls_head.*."""
    import tante_amd
    import tante_amd.dpot as D
    name = sorted(MODELS)[0]
    m, _, x, _ = G.fixture_model(name)
    keys = set(m.state_dict())
    text = ("tante_amd.DPOT is inference only: training is out of scope (the mixer's and GroupNorm's backward are kernels of their own that "
            "are not built); call .eval() under torch.no_grad()")
    for cls in (D.DPOT, D.Block, D.AFNO2D, D.PatchEmbed, D.TimeAggregator):
        assert "trainable" not in inspect.signature(cls.__init__).parameters and callable(cls.set_trainable)
    with pytest.raises(NotImplementedError) as e:
        m.eval()(x)
    assert str(e.value) == text
    with torch.no_grad(), pytest.raises(NotImplementedError) as e:
        m.train()(x)
    assert str(e.value) == text
    children = [m.patch_embed, m.time_agg_layer, *m.blocks, *(b.filter for b in m.blocks)]
    assert m.set_trainable() is m and set(m.state_dict()) == keys and all(c._trainable for c in children)
    for mod in (m.eval(), m.train()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(x)
    assert m.set_trainable(False) is m and not any(c._trainable for c in children)
    with pytest.raises(NotImplementedError) as e:
        m.eval()(x)
    assert str(e.value) == text
    blk = m.blocks[0]
    assert blk.set_trainable() is blk and blk.filter._trainable and blk.filter.set_trainable(False) is blk.filter
    named = dict(m.named_parameters())
    trained = {id(p) for p in m.trained_parameters()}
    assert {k for k, p in named.items() if id(p) not in trained} == {k for k in named if k.startswith("cls_head.")}
    assert len(trained) == len(named) - 6
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16))
    with pytest.raises(NotImplementedError, match="hidden_size_factor = 2"):
        D.AFNO2D(width=32, num_blocks=2, hidden_size_factor=2)
    with pytest.raises(NotImplementedError, match="mixing_type"):
        tante_amd.DPOT(in_T=2, dset_metadata=md, mixing_type="attn")
    assert callable(D.dpot_train_forward) and callable(D.block_train)
    assert all(hasattr(f, "apply") for f in (D.DpotFilterFn, D.GroupNormFn, D.TimeAggFn))
