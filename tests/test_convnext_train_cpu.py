"""CPU: the host side of the trainable UNetConvNext -- the new entry points, their predicates and refusals, the opt-in surface, the float64
restatement of the two backward kernels (tests/convnext_grad_ref.py) against float64 autograd of tests/convnext_ref.py, and that every block
case of the GPU tests has an input gradient beyond the skip's worth comparing."""
import inspect
import os
import re

import pytest
import torch

import convnext_grad_ref as G
from conftest import ROOT
from test_convnext_cpu import BLOCKS, MIN_RATIO, MODELS

ENTRIES = ("tante_dwconv_ln_bwd_supported", "tante_dwconv_ln_bwd_workspace_bytes", "tante_dwconv_ln_bwd", "tante_l2norm_rows_bwd_supported",
           "tante_l2norm_rows_bwd")
RTOL = 1e-10
# the restatement's |dx - dout| / |dout| in float64 with the output gradient convnext_grad_ref.block_fixture draws (fp32 randn of seed 31
# in the fixture's (n, C, H, W) layout); another draw of the same seed moves them in the second digit, never below MIN_RATIO
RATIOS = {"g21_convnext_block_c15_5x7": 0.227, "g21_convnext_block_c32_9x20": 0.246}


@pytest.fixture(scope="module")
def lib():
    from tante_amd import _lib
    from tante_amd.build import build
    build()
    return _lib.lib()


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_entry_points_are_declared_bound_and_exported(lib):
    from tante_amd import _lib
    from tante_amd.build import HEADERS, SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert declared == set(_lib.SIGNATURES)
    stages = os.path.join(ROOT, "tante_amd", "csrc", "convnext_stages.hip.h")
    assert "convnext_bwd.hip" in SOURCES and os.path.exists(stages) and stages in HEADERS
    for src in ("convnext.hip", "convnext_bwd.hip"):         # both sides run the one copy of the two stages
        text = open(os.path.join(ROOT, "tante_amd", "csrc", src)).read()
        assert '#include "convnext_stages.hip.h"' in text and "void dw_stage(" not in text and "void ln_stage(" not in text
    assert _lib.ABI_VERSION == 14 and lib.tante_abi_version() == 14
    assert len(_lib.SIGNATURES["tante_dwconv_ln"][0]) == 13 and len(_lib.SIGNATURES["tante_l2norm_rows"][0]) == 7
    assert len(_lib.SIGNATURES["tante_dwconv_ln_bwd"][0]) == 20 and len(_lib.SIGNATURES["tante_l2norm_rows_bwd"][0]) == 8


def test_predicates_agree_with_their_python_mirrors(lib):
    import tante_amd.convnext as CN
    n_yes = 0
    for n in (-1, 0, 1, 4, 2 ** 31 - 1, 2 ** 31):
        for H, W in ((0, 4), (1, 1), (2, 3), (19, 37), (256, 256), (4, 0), (65536, 65536)):
            for C in (0, 1, 15, 33, 512, 513, 1024, 1025):
                ok = CN.dwconv_ln_bwd_supported_py(n, H, W, C)
                assert bool(lib.tante_dwconv_ln_bwd_supported(n, H, W, C)) == ok == bool(lib.tante_dwconv_ln_supported(n, H, W, C)), (n, H, W, C)
                if n * H * W * C < 2 ** 40:
                    assert (lib.tante_dwconv_ln_bwd_workspace_bytes(n, H, W, C) >= 0) == ok, (n, H, W, C)
                n_yes += ok
    for M in (-1, 0, 1, 37, 2 ** 33 - 4, 2 ** 33 - 3):
        for C in (0, 1, 15, 240, 1 << 24, (1 << 24) + 1):
            ok = CN.l2norm_rows_bwd_supported_py(M, C)
            assert bool(lib.tante_l2norm_rows_bwd_supported(M, C)) == ok == bool(lib.tante_l2norm_rows_supported(M, C)), (M, C)
            n_yes += ok
    assert n_yes > 50
    # du (n, H, W, C), then one row (3, C) per workgroup of launch A and one row (C, 49) per walker of launch B
    assert lib.tante_dwconv_ln_bwd_workspace_bytes(2, 5, 7, 15) == 4 * (1052 + 2 * 3 * 15 + 2 * 15 * 49)
    # ... both bounded by the cap: 2 * 17 * 17 = 578 tiles -> 512 rows; 18 tiles of launch B at 32 chunks -> 512 / 32 = 16 walkers
    assert lib.tante_dwconv_ln_bwd_workspace_bytes(2, 136, 136, 16) == 4 * (2 * 136 * 136 * 16 + G.WALK_CAP * 3 * 16 + G.WALK_CAP * 16 * 49)
    assert lib.tante_dwconv_ln_bwd_workspace_bytes(1, 24, 48, 1024) == 4 * (24 * 48 * 1024 + 6 * 6 * 3 * 1024 + (G.WALK_CAP // 32) * 1024 * 49)
    assert (2, 16, 136, 136) in G.DWLN_CASES and (1, 1024, 24, 48) in G.DWLN_CASES


def test_every_refusal_has_its_code_and_message(lib):
    """Null pointers throughout: an unsupported shape is refused with -2 and the forward's reason, a supported one with -1; nothing launches."""
    from tante_amd import _lib

    def dl(n, H, W, C, dt=0):
        return lib.tante_dwconv_ln_bwd(None, dt, None, n, H, W, C, None, None, 1e-6, None, None, None, None, None, None, 0, None, 0, None)
    for shape, why in (((2, 4, 4, 1025), "channels outside 1..1024"), ((2, 4, 4, 0), "channels outside 1..1024"), ((2, 0, 4, 16), "an empty image"),
                       ((-1, 4, 4, 16), "a negative image count"), ((2 ** 31, 4, 4, 16), "more than 2^31 - 1 tiles per call")):
        assert dl(*shape) == -2, shape
        msg = lib.tante_last_error().decode()
        assert msg.startswith("tante_dwconv_ln_bwd: ") and why in msg, msg
    assert dl(2, 4, 4, 16, 99) == -1 and "dy must be fp32 or bf16" in lib.tante_last_error().decode()
    assert dl(2, 4, 4, 16, _lib.F32) == -1 and "null argument" in lib.tante_last_error().decode()
    assert lib.tante_dwconv_ln_bwd_workspace_bytes(2, 4, 4, 1025) == -1

    def l2(M, C, dt=0):
        return lib.tante_l2norm_rows_bwd(None, dt, None, M, C, 1e-6, None, None)
    for shape, why in (((4, 0), "channels outside 1..2^24"), ((4, (1 << 24) + 1), "channels outside 1..2^24"), ((-1, 8), "rows outside 0..2^33 - 4")):
        assert l2(*shape) == -2, shape
        msg = lib.tante_last_error().decode()
        assert msg.startswith("tante_l2norm_rows_bwd: ") and why in msg, msg
    assert l2(4, 8, 99) == -1 and "dy must be fp32 or bf16" in lib.tante_last_error().decode()
    assert l2(4, 8, _lib.BF16) == -1 and "null argument" in lib.tante_last_error().decode()


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("case", [c for c in G.DWLN_CASES if c[0] * c[1] * c[2] * c[3] <= 50000])
def test_restated_dwconv_ln_backward_is_float64_autograd(case, affine):
    """The three-term LN gradient on the recomputed sums, the flipped-tap correlation and the tap gradient: equal to autograd of
    convnext_ref within 1e-10 on every node case small enough for a CPU test."""
    (x, w, b, gw, gb, dy), want = G.dwln_want(case, affine, False)
    got = G.dwln_backward_restated(x, w, b, gw, dy)
    assert rel(got[0], want[1]) < RTOL and rel(got[1], want[2].reshape(-1, 49)) < RTOL and rel(got[2], want[3]) < RTOL
    if affine:
        assert rel(got[3], want[4]) < RTOL and rel(got[4], want[5]) < RTOL


def test_restated_dwconv_ln_backward_on_the_offset_input():
    C = 48
    (x, w, b, gw, gb, dy), want = G.dwln_want((2, C, 9, 20), True, False, G.IN_OFFSET)
    assert abs(float(w.sum(dim=(1, 2, 3)).mean()) - 1.0) < 0.05
    got = G.dwln_backward_restated(x, w, b, gw, dy)
    for a, c in zip(got, (want[1], want[2].reshape(-1, 49), want[3], want[4], want[5])):
        assert rel(a, c) < 1e-8                        # (conditioning: the offset's 30 against a spread of 0.5)


@pytest.mark.parametrize("C", G.L2_CASES)
def test_restated_l2norm_backward_is_float64_autograd(C):
    """Both branches: (dy - y (y . dy)) / r above eps, dy / eps at and below it -- the zero row and the row below eps included."""
    x, dy = G.l2_case(C)
    assert float(x[2].norm()) == 0.0 and 0.0 < float(x[4].double().norm()) < G.EPS
    _, want = G.l2_autograd(x, dy)
    got = G.l2_backward_restated(x, dy)
    assert rel(got, want) < RTOL
    assert torch.equal(got[2], dy[2].double() / G.EPS) and torch.equal(want[4], dy[4].double() / G.EPS)


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_cases_have_a_gradient_beyond_the_skip(name):
    """A default block adds 1e-6 of its input: dx - dout would be rounding noise.  The g21 fixtures' gamma is near 0.5."""
    sd, x, dout = G.block_fixture(name)
    ratio = G.block_ratio(sd, x, dout)
    print(f"{name}: |dx - dout| / |dout| = {ratio:.3f}")
    assert ratio >= MIN_RATIO and abs(ratio - RATIOS[name]) < 2e-3


def test_opt_in_surface():
    """set_trainable returns self and reaches every child, is neither a constructor argument nor in the state_dict; without it the pinned
    refusal stands word for word, with it the call gets as far as the device check; trained_parameters omits exactly the channels-first
    norms' biases, 2 * stages of them."""
    import tante_amd.convnext as CN
    name = sorted(MODELS)[0]
    m, _, x = G.fixture_model(name)
    keys = set(m.state_dict())
    text = ("tante_amd.UNetConvNext is inference only: training is out of scope (the backward of the fused block is a kernel of its own that "
            "is not built); call .eval() under torch.no_grad()")
    classes = (CN.UNetConvNext, CN.Stage, CN.Block, CN.Upsample, CN.Downsample, CN.LayerNorm)
    for cls in classes:
        assert "trainable" not in inspect.signature(cls.__init__).parameters and callable(cls.set_trainable)
    with pytest.raises(NotImplementedError) as e:
        m.eval()(x)
    assert str(e.value) == text
    with torch.no_grad(), pytest.raises(NotImplementedError) as e:
        m.train()(x)
    assert str(e.value) == text
    children = [c for c in m.modules() if isinstance(c, classes)]
    assert len(children) > 20 and not any(c._trainable for c in children)
    assert m.set_trainable() is m and set(m.state_dict()) == keys and all(c._trainable for c in children)
    for mod in (m.eval(), m.train()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(x)
    assert m.set_trainable(False) is m and not any(c._trainable for c in children)
    with pytest.raises(NotImplementedError) as e:
        m.eval()(x)
    assert str(e.value) == text
    st = m.encoder[0]
    assert st.set_trainable() is st and st.blocks[0]._trainable and st.blocks[0].norm._trainable and st.resample.block[0]._trainable
    assert not m._trainable and not m.neck._trainable
    assert st.blocks[0].set_trainable(False) is st.blocks[0] and not st.blocks[0].norm._trainable and st.resample._trainable
    for mname in MODELS:
        mm = G.fixture_model(mname)[0]
        named = dict(mm.named_parameters())
        trained = {id(p) for p in mm.trained_parameters()}
        left = {k for k, p in named.items() if id(p) not in trained}
        assert left == {k for k in named if k.endswith("resample.block.0.bias")} and len(left) == 2 * MODELS[mname]["stages"]
        assert [k for k in named if id(named[k]) in trained] == G.trained_names(mm)
    assert callable(CN.convnext_train_forward) and callable(CN.block_train) and callable(CN.stage_train)
    assert all(hasattr(f, "apply") for f in (CN.DwConvLnFn, CN.L2NormRowsFn))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_float64_autograd_leaves_exactly_the_channels_first_biases_unused(name):
    m, sd, x = G.fixture_model(name)
    sd64 = G.sd_leaves(sd)
    import convnext_ref as R
    y = R.model(x, sd64)
    keys = [k for k, v in sd64.items() if v.is_floating_point()]
    grads = torch.autograd.grad(y.sum(), [sd64[k] for k in keys], allow_unused=True)
    assert {k for k, g in zip(keys, grads) if g is None} == {k for k in keys if G.untrained(k)}
