"""CPU: the UNO baseline's fixtures, its float64 restatement in both forms, the rules, the host tables, the mirror's layout, the entry
points, the predicates and the refusals.  Nothing here touches a GPU."""
import ctypes
import math
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import uno_ref as R
from conftest import load_golden_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ERR32, MIN_SHARE, MIN_REACH = 5e-6, 0.2, 0.05
# (Ci, Co, Hi, Wi, Ho, Wo, m1, m2)
SPECS = {"g23_uno_spec_3_5_12x10_6x8_m2x3": (3, 5, 12, 10, 6, 8, 2, 3), "g23_uno_spec_3_5_12x10_6x8_m3x5": (3, 5, 12, 10, 6, 8, 3, 5),
         "g23_uno_spec_4_2_6x8_13x21_m3x5": (4, 2, 6, 8, 13, 21, 3, 5), "g23_uno_spec_2_3_16x16_6x16_m4x5": (2, 3, 16, 16, 6, 16, 4, 5),
         "g23_uno_spec_3_3_8x8_8x8_m4x5": (3, 3, 8, 8, 8, 8, 4, 5)}
BLOCKS = {"g23_uno_block_6_7_20x24_9x11_m3x4": (6, 7, 20, 24, 9, 11, 3, 4), "g23_uno_block_5_3_7x10_18x23_m3x5": (5, 3, 7, 10, 18, 23, 3, 5)}
MODELS = {"g23_uno_model_w4_f1_128x256": dict(width=4, factor=1, pad=0, n_fields=1, res=(128, 256), B=2),
          "g23_uno_model_w4_f2_p4_120x248": dict(width=4, factor=2, pad=4, n_fields=2, res=(120, 248), B=1),
          "g23_uno_model_w4_f1_136x264": dict(width=4, factor=1, pad=0, n_fields=2, res=(136, 264), B=1),
          "g23_uno_model_w6_f1_256x256": dict(width=6, factor=1, pad=0, n_fields=1, res=(256, 256), B=1)}
ENTRY_POINTS = ["tante_uno_block_supported", "tante_uno_table_floats", "tante_uno_table_layout", "tante_uno_block_workspace_bytes", "tante_uno_block",
                "tante_uno_mode_mix_supported", "tante_uno_mode_mix"]
_CACHE = {}


def keyed_golden(name):
    """-> (tensors, state dict, key list, shape list) of a fixture; a model fixture's state dict and input come from the rules."""
    if name not in _CACHE:
        raw = load_golden_raw(name)
        g = {k: torch.from_numpy(v) for k, v in raw.items() if k not in ("keys", "shapes")}
        keys = [str(k) for k in raw["keys"]]
        shapes = [tuple(int(s) for s in str(t).split(",")) if str(t) else () for t in raw["shapes"]]
        sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
        if not sd:
            sd = R.rule_state_dict(keys, shapes, g["scales"].tolist())
            g["x"] = R.rule_input(name, g["x_shape"].tolist())
        _CACHE[name] = (g, sd, keys, shapes)
    return _CACHE[name]


def model_kwargs(name):
    c = MODELS[name]
    return dict(in_T=2, dset_metadata=types.SimpleNamespace(n_fields=c["n_fields"], n_spatial_dims=2), width=c["width"], pad=c["pad"], factor=c["factor"])


def restated(name, spectral=R.spectral_table):
    g, sd, _, _ = keyed_golden(name)
    if name in SPECS:
        Ho, Wo = SPECS[name][4:6]
        return spectral(g["x"].double(), sd["weights1"], sd["weights2"], Ho, Wo)
    if name in BLOCKS:
        Ho, Wo = BLOCKS[name][4:6]
        return R.block(g["x"], sd, "", Ho, Wo, spectral=spectral)
    return R.model(g["x"], sd, MODELS[name]["pad"], spectral=spectral)


@pytest.mark.parametrize("name", list(SPECS) + list(BLOCKS))
def test_restatement_reproduces_the_component_fixtures(name):
    """The restatement run here equals the stored float64 truth, and the reference's stored fp32 output is within half the 1e-6 of it
    that the models get."""
    g = keyed_golden(name)[0]
    y = restated(name)
    assert y.dtype == torch.float64 and y.shape == g["y64"].shape
    assert R.err(y, g["y64"]) <= 1e-12
    e = R.err(g["y32"], y)
    assert e <= 0.5e-6 and abs(e - float(g["err32"])) <= 1e-9, (e, float(g["err32"]))
    assert tuple(g["dims"].tolist()) == (SPECS.get(name) or BLOCKS[name])[4:]


@pytest.mark.parametrize("name", list(MODELS))
def test_restatement_reproduces_the_model_fixtures(name):
    g, sd, keys, _ = keyed_golden(name)
    c = MODELS[name]
    assert (int(g["width"]), int(g["factor"]), int(g["pad"]), int(g["n_fields"]), int(g["in_T"])) == (c["width"], c["factor"], c["pad"], c["n_fields"], 2)
    assert tuple(g["x_shape"].tolist()) == (c["B"], 2, c["n_fields"], *c["res"]) and tuple(g["y64"].shape) == (c["B"], 1, c["n_fields"], *c["res"])
    y = restated(name)
    assert R.err(y, g["y64"]) <= 1e-12
    assert 0 < float(g["err32"]) <= 1e-6, float(g["err32"])                   # the reference's fp32 output against this truth


@pytest.mark.parametrize("name", list(SPECS) + list(BLOCKS) + ["g23_uno_model_w4_f1_136x264", "g23_uno_model_w4_f2_p4_120x248"])
def test_both_forms_of_the_restatement_agree(name):
    """The sums over the kept modes against the reference's own steps on torch.fft in complex128: odd grids, overlapping bands (16 -> 6
    rows, and L0 of 136 x 264), a populated Nyquist column."""
    a, b = restated(name, R.spectral_table), restated(name, R.spectral_fft)
    assert R.err(a, b) <= 1e-12, R.err(a, b)


def test_fixtures_hold_their_conditions():
    for name in list(SPECS) + list(BLOCKS) + list(MODELS):
        g = keyed_golden(name)[0]
        assert 0 < float(g["err32"]) <= MAX_ERR32, (name, float(g["err32"]))
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1000 * 1000
    for name in list(BLOCKS) + list(MODELS):
        g = keyed_golden(name)[0]
        assert float(g["path_share"].min()) >= MIN_SHARE, (name, g["path_share"])
        assert all(math.log2(s) == round(math.log2(s)) for s in g["scales"].tolist())          # powers of two: exact in fp32
    for name in MODELS:
        g = keyed_golden(name)[0]
        assert g["block_reach"].numel() == 7 and float(g["block_reach"].min()) >= MIN_REACH, (name, g["block_reach"])
        assert tuple(g["path_share"].shape) == (7, 2)
    # the stored figures are what they say: one block fixture and the smallest model
    name = "g23_uno_block_6_7_20x24_9x11_m3x4"
    g, sd, _, _ = keyed_golden(name)
    parts = []
    R.block(g["x"], sd, "", 9, 11, parts)
    s, w = parts[0]
    assert abs(R.rms(s) / R.rms(s + w) - float(g["path_share"][0, 0])) < 1e-9 and abs(R.rms(w) / R.rms(s + w) - float(g["path_share"][0, 1])) < 1e-9
    name = "g23_uno_model_w4_f1_128x256"
    g, sd, _, _ = keyed_golden(name)
    parts = []
    R.model(g["x"], sd, 0, parts)
    for i, (s, w) in enumerate(parts):
        assert abs(R.rms(s) / R.rms(s + w) - float(g["path_share"][i, 0])) < 1e-8, i
    y1 = R.model(g["x"], sd, 0, zero_block=2)
    assert abs(R.rms(g["y64"] - y1) / R.rms(g["y64"]) - float(g["block_reach"][2])) < 1e-8


def test_rules_are_exact_and_deterministic():
    u = R.rule_uniform("L0.conv.weights1.re", 4096)
    assert u.min() >= -0.5 and u.max() < 0.5 and abs(u.mean()) < 0.03 and 0.27 < u.std() < 0.31
    assert (u.astype("float32").astype("float64") == u).all()
    assert (R.rule_uniform("L0.conv.weights1.re", 16) == u[:16]).all() and (R.rule_uniform("L0.conv.weights1.im", 16) != u[:16]).any()
    w = R.rule_entry("L1.conv.weights2", (8, 16, 8, 9))
    assert w.dtype == torch.complex64 and float(w.real.abs().max()) <= 0.5 * math.sqrt(6 / 8) + 1e-7 and float(w.imag.std()) > 0.2
    assert torch.equal(R.rule_entry("L1.conv.weights2", (8, 16, 8, 9), 4.0), w * 4.0)
    sd = R.rule_state_dict(["L3.conv.weights1", "fc.weight", "fc.bias"], [(2, 2, 4, 5), (16, 6), (16,)], [1, 1, 1, 8.0, 1, 1, 1])
    assert torch.equal(sd["L3.conv.weights1"], R.rule_entry("L3.conv.weights1", (2, 2, 4, 5)) * 8.0)
    assert sd["fc.weight"].dtype == torch.float32 and float(sd["fc.weight"].abs().max()) <= math.sqrt(3 / 6) + 1e-7 and float(sd["fc.bias"].abs().max()) <= 0.1
    x = R.rule_input("a", (1, 2, 1, 4, 4))
    assert x.dtype == torch.float32 and torch.equal(x, R.rule_input("a", (1, 2, 1, 4, 4))) and not torch.equal(x, R.rule_input("b", (1, 2, 1, 4, 4)))


@pytest.mark.parametrize("n_in,n_out", [(256, 64), (64, 16), (8, 8), (16, 64), (10, 23), (24, 11), (7, 18), (2, 5), (33, 8)])
def test_resize_tables_equal_interpolate_in_float64(n_in, n_out):
    """resize(X) = A_h X A_w^T with A from tante_amd.uno.resize_matrix, against F.interpolate in float64, down- and up-scaling; the
    identity when the sizes agree; rows sum to 1 (the bias passes through)."""
    from tante_amd import uno as U
    A = U.resize_matrix(n_in, n_out)
    assert A.dtype == torch.float64 and tuple(A.shape) == (n_out, n_in)
    assert float((A.sum(dim=1) - 1).abs().max()) <= 1e-12
    if n_in == n_out:
        assert float((A - torch.eye(n_in, dtype=torch.float64)).abs().max()) <= 1e-12
    gen = torch.Generator().manual_seed(n_in * 1000 + n_out)
    other_in, other_out = (n_in // 2 + 3, n_out // 2 + 2)
    x = torch.randn(2, 3, other_in, n_in, generator=gen, dtype=torch.float64)
    want = F.interpolate(x, size=(other_out, n_out), mode="bicubic", align_corners=True, antialias=True)
    got = torch.einsum("yh,bchw,xw->bcyx", U.resize_matrix(other_in, other_out), x, A)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def table_block(x, sd, Ho, Wo, m1, m2, pointwise):
    """The seven launches of tante_uno_block replayed in float64 on the HOST tables (fp32 values), with the library's own layout."""
    from tante_amd import uno as U
    B, Ci, Hi, Wi = x.shape
    layout, total, down = U.table_layout(Hi, Wi, Ho, Wo, m1, m2, pointwise)
    flat = U.block_tables(Hi, Wi, Ho, Wo, m1, m2, pointwise)
    assert flat.dtype == torch.float32 and flat.numel() == total
    T = [flat[o:o + r * c].reshape(r, c).double() for o, r, c in layout]
    J = 2 * m1
    x = x.double()
    P1 = torch.einsum("mw,bihw->bimh", T[0], x)                                         # (B, Ci, M1, Hi)
    rows = P1[:, :, :2 * m2].reshape(B, Ci, m2, 2 * Hi)                                 # row l = [Pr | Pi]
    X = torch.einsum("mk,bilk->biml", T[1], rows)                                       # (B, Ci, 2J, m2)
    Wt = torch.cat([sd["conv.weights1"], sd["conv.weights2"]], dim=2).to(torch.complex128)
    Y = torch.einsum("bijl,iojl->bojl", torch.complex(X[:, :, :J], X[:, :, J:]), Wt)
    Yk = torch.cat([Y.real, Y.imag], dim=2)                                             # (B, Co, 2J, m2)
    Z = torch.einsum("mk,bokl->boml", T[3], Yk)                                         # (B, Co, 2Ho, m2)
    zrow = torch.cat([Z[:, :, :Ho], Z[:, :, Ho:]], dim=3)                               # (B, Co, Ho, 2 m2)
    add = 0
    if pointwise:
        w, b = sd["w.conv.weight"].double().reshape(-1, Ci), sd["w.conv.bias"].double()
        if down:
            S = torch.einsum("yh,bixh->biyx", T[2], P1[:, :, 2 * m2:])
            add = torch.einsum("oi,biyx->boyx", w, S) + b.reshape(1, -1, 1, 1)
        else:
            V = torch.einsum("oi,bihw->bohw", w, x)
            zrow = torch.cat([zrow, torch.einsum("yh,bohw->boyw", T[2], V)], dim=3)
            add = b.reshape(1, -1, 1, 1)
    out = torch.einsum("xk,boyk->boyx", T[4], zrow) + add
    return R.gelu(out) if pointwise else out


@pytest.mark.parametrize("name", list(SPECS) + list(BLOCKS))
def test_host_tables_reproduce_the_fixtures(name):
    """The tables the kernels read (float64, rounded to fp32 once), multiplied out on the host: within fp32 table rounding of the truth."""
    g, sd, _, _ = keyed_golden(name)
    Ci, Co, Hi, Wi, Ho, Wo, m1, m2 = SPECS.get(name) or BLOCKS[name]
    if name in SPECS:
        sd = {"conv.weights1": sd["weights1"], "conv.weights2": sd["weights2"]}
    y = table_block(g["x"], sd, Ho, Wo, m1, m2, name in BLOCKS)
    assert R.err(y, g["y64"]) <= 5e-7, R.err(y, g["y64"])


def test_state_dict_matches_the_reference_layout():
    import tante_amd
    from tante_amd import uno as U
    for name in MODELS:
        g, sd, keys, shapes = keyed_golden(name)
        m = tante_amd.UNO(**model_kwargs(name))
        own = m.state_dict()
        assert list(own.keys()) == keys and len(keys) == 36
        for k, s in zip(keys, shapes):
            assert tuple(own[k].shape) == s, k
        assert own["L0.conv.weights1"].dtype == torch.complex64 and own["L6.w.conv.weight"].dim() == 4
        m.load_state_dict(sd, strict=True)
    for name, make in (("g23_uno_spec_4_2_6x8_13x21_m3x5", lambda: U.SpectralConv2d_Uno(4, 2, 13, 21, 3, 5)),
                       ("g23_uno_block_6_7_20x24_9x11_m3x4", lambda: U.OperatorBlock_2D(6, 7, 9, 11, 3, 4))):
        _, sd, keys, shapes = keyed_golden(name)
        mod = make()
        assert list(mod.state_dict().keys()) == keys and [tuple(v.shape) for v in mod.state_dict().values()] == shapes
        mod.load_state_dict(sd, strict=True)


def test_constructor_mirrors_the_reference():
    import tante_amd
    from tante_amd import uno as U
    m = tante_amd.UNO(4)                                                      # no metadata: 4 fields, width 32
    assert (m.in_width, m.width, m.padding, m.dim_out) == (16, 32, 0, 4)
    assert tuple(m.fc.weight.shape) == (16, 20) and tuple(m.fc0.weight.shape) == (32, 16)
    assert tuple(m.fc1.weight.shape) == (96, 64) and tuple(m.fc2.weight.shape) == (4, 112)
    want = [(32, 64, 32, 33), (64, 128, 8, 9), (128, 256, 4, 5), (256, 256, 4, 5), (256, 128, 4, 5), (256, 64, 8, 9), (128, 32, 32, 32)]
    for i, s in enumerate(want):
        blk = getattr(m, f"L{i}")
        assert isinstance(blk, U.OperatorBlock_2D) and isinstance(blk.conv, U.SpectralConv2d_Uno) and isinstance(blk.w, U.pointwise_op_2D)
        assert tuple(blk.conv.weights1.shape) == s == tuple(blk.conv.weights2.shape) and (blk.conv.modes1, blk.conv.modes2) == U.BLOCK_MODES[i]
        assert tuple(blk.w.conv.weight.shape) == (s[1], s[0], 1, 1) and blk.non_lin and not blk.normalize
    md = types.SimpleNamespace(n_fields=11, n_spatial_dims=2)
    m2 = tante_amd.UNO(4, md, width=30, pad=3, factor=2)
    assert (m2.in_width, m2.padding) == (44, 3) and tuple(m2.L3.conv.weights1.shape) == (480, 480, 4, 5) and tuple(m2.fc2.weight.shape) == (11, 106)
    assert m.set_compute("bf16") is m and m.compute == "bf16"
    with pytest.raises(ValueError):
        m.set_compute("fp8")
    s = U.SpectralConv2d_Uno(3, 4, 10, 12)
    assert (s.modes1, s.modes2) == (4, 6) and abs(s.scale - (1 / 6) ** 0.5) < 1e-12


def test_config_aliases_build_the_reference_model_block():
    import tante_amd
    from tante_amd import config
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "uno_am.yaml"))
    ref = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_att_am.yaml"))
    assert cfg["model"] == {"_target_": "models.UNO", "in_T": 4, "width": 38, "pad": 0, "factor": 1}
    assert cfg["workload"] == ref["workload"] and cfg["workload"]["spatial_resolution"] == [256, 256]
    md = types.SimpleNamespace(n_fields=cfg["workload"]["n_fields"], n_spatial_dims=2)
    for target in ("models.UNO", "models.uno.UNO"):
        assert config._TARGET_ALIASES[target] == "tante_amd.uno.UNO"
        m = tante_amd.build_model(dict(cfg, model=dict(cfg["model"], _target_=target)), md)
        assert isinstance(m, tante_amd.UNO) and (m.in_width, m.width, m.padding, m.dim_out) == (44, 38, 0, 11)
        n_spec = sum(p.numel() for k, p in m.state_dict().items() if "weights" in k)
        assert 8 * n_spec == 242_499_584                                  # the 242 MB complex fp32 weight stream of the config


def test_block_sizes_and_the_sizes_the_reference_refuses():
    from tante_amd import uno as U
    assert U.block_sizes(256, 256) == [(256, 256, 64, 64), (64, 64, 16, 16), (16, 16, 8, 8), (8, 8, 8, 8), (8, 8, 16, 16), (16, 16, 64, 64), (64, 64, 256, 256)]
    assert U.block_sizes(136, 264)[0] == (136, 264, 34, 66) and U.block_sizes(136, 264)[2] == (8, 16, 4, 8)
    U.block_sizes(128, 256), U.block_sizes(128, 512)
    for D1, D2 in ((64, 256), (96, 256), (128, 128), (127, 256), (128, 255)):
        with pytest.raises(ValueError, match="L0: .*cannot hold its 32 x 33 modes"):
            U.block_sizes(D1, D2)
    for H in range(120, 140):                                             # exactly H >= 128 and W >= 256
        for W in range(250, 262):
            try:
                U.block_sizes(H, W)
                ok = True
            except ValueError:
                ok = False
            assert ok == (H >= 128 and W >= 256), (H, W)
    assert U.live_rows(34, 32).tolist() == [1.0] * 2 + [0.0] * 30 + [1.0] * 32 and U.live_rows(32, 32)[:32].sum() == 0 and U.live_rows(64, 32).sum() == 64
    m = U.UNO(2, types.SimpleNamespace(n_fields=1, n_spatial_dims=2), width=4, pad=4).eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="L0"):
            m(torch.zeros(1, 2, 1, 119, 248))                              # 127 x 256 after padding
        with pytest.raises(RuntimeError, match="GPU only"):
            m(torch.zeros(1, 2, 1, 120, 248))


def test_out_of_scope_calls_raise_by_name():
    import tante_amd
    from tante_amd import uno as U
    md = types.SimpleNamespace(n_fields=1, n_spatial_dims=2)
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.UNO(4, types.SimpleNamespace(n_fields=3, n_spatial_dims=3))
    with pytest.raises(NotImplementedError, match="Normalize=True"):
        U.OperatorBlock_2D(4, 4, 8, 8, 2, 2, Normalize=True)
    m = tante_amd.UNO(2, md, width=4)
    x = torch.zeros(1, 2, 1, 128, 256)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)                                                                      # train mode
    m.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)                                                                      # grad enabled on parameters that require grad
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x)
        with pytest.raises(ValueError, match="t \\* c"):
            m(torch.zeros(1, 3, 1, 128, 256))
        with pytest.raises(ValueError, match="3-D fields are out of scope"):
            m(torch.zeros(1, 2, 1, 8, 128, 256))
        with pytest.raises(NotImplementedError, match="tante_amd.UNO: .*out of scope"):
            m(torch.zeros(1, 2, 1, 128, 640))                                     # a plane past 512
        wide = tante_amd.UNO(2, md, width=40, factor=2)
        with pytest.raises(NotImplementedError, match="640 channels are out of scope"):
            wide.eval()(x)
        with pytest.raises(NotImplementedError, match="pointwise_op_2D alone"):
            m.L0.w(torch.zeros(1, 4, 8, 8))
        with pytest.raises(RuntimeError, match="GPU only"):
            m.L3(torch.zeros(1, 32, 8, 8))
        with pytest.raises(RuntimeError, match="GPU only"):
            m.L3.conv(torch.zeros(1, 32, 8, 8))


def test_entry_points_are_declared_bound_and_exported():
    import tante_amd
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "uno_ops.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert int(L.tante_abi_version()) == _lib.ABI_VERSION == 14
    assert "UNO" in tante_amd.__all__ and tante_amd.UNO is tante_amd.uno.UNO


def test_supported_predicate_agrees_with_its_python_mirror():
    from tante_amd import _lib
    from tante_amd import uno as U
    L = _lib.lib()
    n_yes = 0
    for B in (-1, 0, 2, 127, 128, 65536):
        for Ci, Co in ((0, 4), (4, 0), (1, 1), (38, 76), (512, 512), (513, 4), (4, 513)):
            for Hi, Wi, Ho, Wo in ((0, 8, 8, 8), (8, 8, 8, 0), (8, 8, 8, 8), (12, 10, 6, 8), (6, 8, 13, 21), (512, 512, 128, 128), (513, 8, 8, 8), (8, 8, 8, 513)):
                for m1, m2 in ((0, 1), (1, 0), (1, 1), (3, 5), (6, 5), (7, 5), (4, 6), (32, 33)):
                    for slack in (-1, 0, 5):
                        xs, os_ = Ci * Hi * Wi + slack, Co * Ho * Wo + (0 if slack < 0 else slack)
                        got = bool(L.tante_uno_block_supported(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, xs, os_))
                        assert got == U.uno_block_supported_py(B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, xs, os_), (B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, xs, os_)
                        n_yes += got
    assert n_yes > 100
    assert bool(L.tante_uno_block_supported(2, 4, 4, 8, 8, 8, 8, 2, 5, 256, 255)) is False          # the output stride alone
    assert int(L.tante_uno_table_floats(8, 8, 8, 8, 4, 6, 1)) == -1 and int(L.tante_uno_block_workspace_bytes(2, 4, 4, 8, 8, 8, 8, 9, 5, 1)) == -1
    lay, total, down = U.table_layout(12, 10, 6, 8, 3, 5, True)
    assert down and [(r, c) for _, r, c in lay] == [(10 + 8, 10), (12, 24), (6, 12), (12, 12), (8, 10)] and total >= sum(r * c for _, r, c in lay)
    lay, total, down = U.table_layout(6, 8, 13, 21, 3, 5, True)
    assert not down and [(r, c) for _, r, c in lay] == [(10, 8), (12, 12), (13, 6), (26, 12), (21, 18)]
    lay, _, _ = U.table_layout(6, 8, 13, 21, 3, 5, False)
    assert [(r, c) for _, r, c in lay] == [(10, 8), (12, 12), (0, 0), (26, 12), (21, 10)]
    assert all(o % 4 == 0 for o, _, _ in lay)
    assert bool(L.tante_uno_mode_mix_supported(4, 38, 76, 32, 33)) and not bool(L.tante_uno_mode_mix_supported(4, 513, 76, 32, 33))


def test_every_refusal_has_its_code_and_message():
    """Host-only argument checks: the refusal names its entry and its reason and launches nothing (every pointer is NULL or a host
    address that is never dereferenced)."""
    from tante_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    at = ctypes.addressof(buf)

    def err():
        return L.tante_last_error()

    def block(B=2, Ci=4, Co=4, Hi=8, Wi=8, Ho=8, Wo=8, m1=2, m2=3, xs=None, os_=None, x=None, out=None, w1=None, w2=None, tables=None, act=0):
        xs = Ci * Hi * Wi if xs is None else xs
        os_ = Co * Ho * Wo if os_ is None else os_
        return L.tante_uno_block(x, xs, B, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, tables, w1, w2, None, None, act, out, os_, None, 0, None)
    assert block(Ci=513) == -2 and b"tante_uno_block: channels outside 1..512" in err()
    assert block(Hi=513) == -2 and b"input grid outside 1..512" in err()
    assert block(Wo=0) == -2 and b"output grid outside 1..512" in err()
    assert block(m1=0) == -2 and b"modes must be at least 1" in err()
    assert block(m1=9, Ho=16) == -2 and b"modes1 exceeds the input rows" in err()
    assert block(m1=5, Ho=4) == -2 and b"modes1 exceeds the output rows" in err()
    assert block(m2=6) == -2 and b"modes2 exceeds the input's half spectrum" in err()
    assert block(m2=5, Wo=6) == -2 and b"modes2 exceeds the output's half spectrum" in err()
    assert block(B=16384, Ci=4, Co=4) == -2 and b"more than 65535" in err()
    assert block(xs=255) == -2 and b"the input image stride is shorter than an image" in err()
    assert block(os_=255) == -2 and b"the output image stride is shorter than an image" in err()
    assert block(act=3) == -1 and b"the activation must be none or the erf GELU" in err()
    assert block() == -1 and b"tante_uno_block: null argument" in err()
    assert block(x=at + 2, out=at + 8192, w1=at, w2=at, tables=at) == -2 and b"4-byte and the spectral weights 8-byte aligned" in err()
    assert block(x=at, out=at + 8192, w1=at + 4, w2=at, tables=at) == -2 and b"8-byte aligned" in err()
    assert block(x=at, out=at + 512, w1=at, w2=at, tables=at) == -2 and b"the output overlaps the input" in err()       # inside the 2 x 1024-byte input
    assert block(x=at, out=at, w1=at, w2=at, tables=at) == -2 and b"the output overlaps the input" in err()
    assert block(x=at, out=at + 4096, w1=at, w2=at, tables=at) == -1 and b"workspace of 0 bytes" in err()                # every check passed
    assert L.tante_uno_mode_mix(None, None, None, None, 2, 513, 4, 2, 3, None) == -2 and b"tante_uno_mode_mix: channels outside 1..512" in err()
    assert L.tante_uno_mode_mix(None, None, None, None, 2, 4, 4, 2, 300, None) == -2 and b"modes outside" in err()
    assert L.tante_uno_mode_mix(None, None, None, None, 2, 4, 4, 2, 3, None) == -1 and b"tante_uno_mode_mix: null argument" in err()
    assert L.tante_uno_mode_mix(at, at + 4, at, at + 1024, 2, 4, 4, 2, 3, None) == -2 and b"8-byte aligned" in err()
    assert L.tante_uno_mode_mix(at, at, at, at, 2, 4, 4, 2, 3, None) == -2 and b"Y may not alias X" in err()
    assert L.tante_uno_table_layout(8, 8, 8, 8, 2, 6, 1, None) == -2 and b"tante_uno_table_layout: modes2 exceeds" in err()
    assert L.tante_uno_table_layout(8, 8, 8, 8, 2, 3, 1, None) == -1 and b"tante_uno_table_layout: null argument" in err()
