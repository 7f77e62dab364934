"""CPU: the AttentionUNet baseline's fixtures, its float64 restatement, the weight rule, the host mirror's layout, the BatchNorm folds, the
entry points, the predicates, the refusals and the bf16-site pin.  Nothing here touches a GPU."""
import os
import re
import types

import pytest
import torch

import unet_att_ref as R
from conftest import load_golden_raw, max_rel, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ERR32, MIN_GATE_RATIO, MIN_PSI_STD = 5e-6, 0.2, 0.05
COMPONENTS = ["g22_unetatt_convblock_7_24_5x7", "g22_unetatt_convblock_40_16_9x20", "g22_unetatt_upconv_24_12_3x5", "g22_unetatt_gate_24_12_6x10"]
MODELS = {"g22_unetatt_model_d2_f3_12x20": dict(depth=2, n_fields=3, out_T=1, res=(12, 20), keys=72, gates=1),
          "g22_unetatt_model_d3_f2_16x24": dict(depth=3, n_fields=2, out_T=4, res=(16, 24), keys=128, gates=2),
          "g22_unetatt_model_d5_f3_16x32": dict(depth=5, n_fields=3, out_T=1, res=(16, 32), keys=240, gates=4)}
ENTRY_POINTS = ["tante_conv3x3_mfma_supported", "tante_conv3x3_pack_bytes", "tante_pack_conv3x3", "tante_conv3x3_mfma", "tante_attn_gate_supported",
                "tante_attn_gate_stream_bytes", "tante_pack_attn_gate", "tante_attn_gate"]
# the exact-bf16 evaluation of the restatement (operands of the named groups rounded to bf16, products exact) on the three model
# fixtures, rel L2 against float64: every group, and all of them together, is under the 1e-2 bar, so all three ship
BF16_FIGURES = {"g22_unetatt_model_d2_f3_12x20": {("conv",): 4.87e-3, ("gate",): 5.91e-4, ("head",): 1.92e-3, ("conv", "gate", "head"): 5.07e-3},
                "g22_unetatt_model_d3_f2_16x24": {("conv",): 6.63e-3, ("gate",): 1.23e-3, ("head",): 1.75e-3, ("conv", "gate", "head"): 6.92e-3},
                "g22_unetatt_model_d5_f3_16x32": {("conv",): 8.25e-3, ("gate",): 3.81e-3, ("head",): 2.52e-3, ("conv", "gate", "head"): 8.41e-3}}
_CACHE = {}


def keyed_golden(name):
    """-> (tensors, state dict, key list, shape list) of a fixture; a model fixture's state dict comes from the weight rule."""
    if name not in _CACHE:
        raw = load_golden_raw(name)
        g = {k: torch.from_numpy(v) for k, v in raw.items() if k not in ("keys", "shapes")}
        keys = [str(k) for k in raw["keys"]]
        shapes = [tuple(int(s) for s in str(t).split(",")) if str(t) else () for t in raw["shapes"]]
        sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")} or R.rule_state_dict(keys, shapes)
        _CACHE[name] = (g, sd, keys, shapes)
    return _CACHE[name]


def model_kwargs(name):
    c = MODELS[name]
    return dict(in_T=4, dset_metadata=types.SimpleNamespace(n_fields=c["n_fields"], n_spatial_dims=2), depth=c["depth"], out_T=c["out_T"])


def pinned(y, g):
    """The restatement against the reference's float64 result; the stored fp32 `y` is that result rounded once."""
    assert y.dtype == torch.float64 and y.shape == g["y64"].shape
    assert rel_err(y, g["y64"]) <= 1e-10 and max_rel(y, g["y64"]) <= 2e-10, (rel_err(y, g["y64"]), max_rel(y, g["y64"]))
    assert torch.equal(g["y"], g["y64"].float())


def nhwc(t):
    return t.double().permute(0, 2, 3, 1)


def component_result(name):
    """The restatement of a component fixture, channels first."""
    g, sd, _, _ = keyed_golden(name)
    if "convblock" in name:
        y = R.conv_block(nhwc(g["x"]), sd)
    elif "upconv" in name:
        y = R.up_conv(nhwc(g["x"]), sd)
    else:
        y = R.attention_block(nhwc(g["x"]), nhwc(g["x2"]), sd)
    return y.permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", COMPONENTS)
def test_restatement_reproduces_the_reference_components(name):
    pinned(component_result(name), keyed_golden(name)[0])


@pytest.mark.parametrize("name", list(MODELS))
def test_restatement_reproduces_the_reference_model(name):
    g, sd, _, _ = keyed_golden(name)
    c = MODELS[name]
    assert (int(g["depth"]), int(g["n_fields"]), int(g["in_T"]), int(g["out_T"])) == (c["depth"], c["n_fields"], 4, c["out_T"])
    assert tuple(g["x"].shape) == (2, 4, c["n_fields"], *c["res"]) and tuple(g["y64"].shape) == (2, c["out_T"], c["n_fields"], *c["res"])
    pinned(R.model(g["x"], sd), g)


def test_fixtures_hold_their_conditions():
    """err32: the reference's own fp32 within half the fp32 bar of its float64; gate_ratio: the gates matter; psi_std: no gate is a
    constant; every norm is off its defaults; every file is under the size limit.  The stored figures are what they say."""
    for name in COMPONENTS + list(MODELS):
        g, sd, _, _ = keyed_golden(name)
        assert 0 < float(g["err32"]) <= MAX_ERR32, (name, float(g["err32"]))
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1000 * 1000
        n_norms = 0
        for k, v in sd.items():
            leaf = k.split(".")[-1]
            if leaf == "running_mean":
                p = k[:-len("running_mean")]
                n_norms += 1
                if v.numel() > 1:
                    for other, default in (("running_mean", 0.0), ("running_var", 1.0), ("weight", 1.0), ("bias", 0.0)):
                        assert float((sd[p + other] - default).abs().max()) > 0.02, (name, p + other)
        assert n_norms >= 1
    for name in ["g22_unetatt_gate_24_12_6x10"] + list(MODELS):
        g, sd, _, _ = keyed_golden(name)
        assert float(g["gate_ratio"]) >= MIN_GATE_RATIO, (name, float(g["gate_ratio"]))
        assert float(g["psi_std"].min()) >= MIN_PSI_STD, (name, g["psi_std"])
    g, sd, _, _ = keyed_golden("g22_unetatt_gate_24_12_6x10")
    psi = R.gate_psi(nhwc(g["x"]), nhwc(g["x2"]), sd)
    assert abs(float(psi.std()) - float(g["psi_std"][0])) < 1e-9
    y, y1 = g["y64"], g["x2"].double()
    assert abs(float(((y - y1) ** 2).mean().sqrt() / (y ** 2).mean().sqrt()) - float(g["gate_ratio"])) < 1e-9
    for name in MODELS:
        g, sd, _, _ = keyed_golden(name)
        psis = []
        y1 = R.model(g["x"], sd, gates_open=True)
        y = g["y64"]
        R.model(g["x"], sd, psis=psis)
        assert abs(float(((y - y1) ** 2).mean().sqrt() / (y ** 2).mean().sqrt()) - float(g["gate_ratio"])) < 1e-8
        assert len(psis) == MODELS[name]["gates"] == g["psi_std"].numel()
        for p, want in zip(psis, g["psi_std"]):
            assert abs(float(p.std()) - float(want)) < 1e-8


def test_weight_rule_is_exact_and_deterministic():
    u = R.rule_uniform("Conv1.conv.0.weight", 4096)
    assert u.min() >= -0.5 and u.max() < 0.5 and abs(u.mean()) < 0.03 and 0.27 < u.std() < 0.31
    assert ((u + 0.5) * (1 << 24) == ((u + 0.5) * (1 << 24)).round()).all()                 # 24 bits: exact in fp32
    assert (u.astype("float32").astype("float64") == u).all()
    assert (R.rule_uniform("Conv1.conv.0.weight", 16) == u[:16]).all() and (R.rule_uniform("Conv1.conv.0.bias", 16) != u[:16]).any()
    w = R.rule_entry("Conv2.conv.0.weight", (128, 64, 3, 3))
    assert w.dtype == torch.float32 and float(w.abs().max()) <= (6.0 / 576) ** 0.5 + 1e-7
    assert R.rule_entry("Conv2.conv.1.num_batches_tracked", ()).dtype == torch.int64
    assert 0.75 <= float(R.rule_entry("a.running_var", (64,)).min()) and float(R.rule_entry("a.running_var", (64,)).max()) < 1.25
    assert float(R.rule_entry("a.weight", (64,)).min()) >= 0.8 and float(R.rule_entry("a.bias", (64,)).abs().max()) <= 0.1


@pytest.mark.parametrize("name", list(MODELS))
def test_state_dict_matches_the_reference_layout(name):
    import tante_amd
    g, sd, keys, shapes = keyed_golden(name)
    m = tante_amd.AttentionUNet(**model_kwargs(name))
    own = m.state_dict()
    assert list(own.keys()) == keys and len(keys) == MODELS[name]["keys"]
    for k, s in zip(keys, shapes):
        assert tuple(own[k].shape) == s, k
    assert sum(k.endswith("running_mean") for k in keys) == sum(k.endswith("num_batches_tracked") for k in keys) > 0
    m.load_state_dict(sd, strict=True)


def test_component_fixtures_load_strictly():
    import tante_amd.unet_att as UA
    for name, make in (("g22_unetatt_convblock_7_24_5x7", lambda: UA.ConvBlock(7, 24)), ("g22_unetatt_convblock_40_16_9x20", lambda: UA.ConvBlock(40, 16)),
                       ("g22_unetatt_upconv_24_12_3x5", lambda: UA.UpConv(24, 12)), ("g22_unetatt_gate_24_12_6x10", lambda: UA.AttentionBlock(24, 24, 12))):
        _, sd, keys, shapes = keyed_golden(name)
        m = make()
        own = m.state_dict()
        assert list(own.keys()) == keys and [tuple(v.shape) for v in own.values()] == shapes
        m.load_state_dict(sd, strict=True)


def test_constructor_mirrors_the_reference():
    import tante_amd
    import tante_amd.unet_att as UA
    m = tante_amd.AttentionUNet(4)                                   # no metadata: 5 fields, depth 4, out_T 4
    assert (m.depth, m.out_T, m.dim_in, m.dim_out) == (4, 4, 20, 20) and len(m.state_dict()) == 184
    assert isinstance(m.MaxPool, torch.nn.MaxPool2d) and m.MaxPool.kernel_size == 2 and m.MaxPool.stride == 2
    assert not hasattr(m, "Conv5") and not hasattr(m, "Up5") and hasattr(m, "Conv4") and hasattr(m, "Up4")
    assert tuple(m.Conv1.conv[0].weight.shape) == (64, 20, 3, 3) and tuple(m.Conv4.conv[3].weight.shape) == (512, 512, 3, 3)
    assert tuple(m.UpConv4.conv[0].weight.shape) == (256, 512, 3, 3) and tuple(m.Up4.up[1].weight.shape) == (256, 512, 3, 3)
    assert isinstance(m.Up2.up[0], torch.nn.Upsample) and m.Up2.up[0].scale_factor == 2 and m.Up2.up[0].mode == "nearest"
    assert isinstance(m.Att4, UA.AttentionBlock) and tuple(m.Att4.W_gate[0].weight.shape) == (128, 256, 1, 1)
    assert tuple(m.Att2.psi[0].weight.shape) == (1, 32, 1, 1) and isinstance(m.Att2.psi[2], torch.nn.Sigmoid) and m.Att2.psi[1].eps == 1e-5
    assert tuple(m.Conv.weight.shape) == (20, 64, 1, 1)
    md = types.SimpleNamespace(n_fields=11, n_spatial_dims=2)
    m5 = tante_amd.AttentionUNet(4, md, depth=5, out_T=1)
    assert (m5.dim_in, m5.dim_out) == (44, 11) and tuple(m5.Conv5.conv[0].weight.shape) == (1024, 512, 3, 3)
    assert tuple(m5.UpConv5.conv[0].weight.shape) == (512, 1024, 3, 3) and tuple(m5.Att5.W_x[0].weight.shape) == (256, 512, 1, 1)
    m2 = tante_amd.AttentionUNet(4, md, depth=2)
    assert not hasattr(m2, "Conv3") and not hasattr(m2, "Up3") and len(m2.state_dict()) == 72
    assert m.set_compute("bf16") is m and m.compute == "bf16"
    with pytest.raises(ValueError):
        m.set_compute("fp8")
    with pytest.raises(ValueError, match="depth"):
        tante_amd.AttentionUNet(4, md, depth=6)


def test_config_aliases_build_the_reference_model_block():
    import tante_amd
    from tante_amd import config
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_att_am.yaml"))
    ref = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_convnext_am.yaml"))
    assert cfg["model"] == {"_target_": "models.AttentionUNet", "in_T": 4, "depth": 5, "out_T": 1}
    assert cfg["workload"] == ref["workload"] and cfg["workload"]["spatial_resolution"] == [256, 256]
    md = types.SimpleNamespace(n_fields=cfg["workload"]["n_fields"], n_spatial_dims=2)
    for target in ("models.AttentionUNet", "models.unet_att.AttentionUNet"):
        assert config._TARGET_ALIASES[target] == "tante_amd.unet_att.AttentionUNet"
        m = tante_amd.build_model(dict(cfg, model=dict(cfg["model"], _target_=target)), md)
        assert isinstance(m, tante_amd.AttentionUNet) and (m.dim_in, m.dim_out, m.depth, m.out_T) == (44, 11, 5, 1)
        assert len(m.state_dict()) == 240


def test_batchnorm_folds_equal_the_direct_evaluation():
    import tante_amd.unet_att as UA
    F = torch.nn.functional
    gen = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    conv, bn = torch.nn.Conv2d(5, 6, 3, padding=1), torch.nn.BatchNorm2d(6)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * rn(6)), bn.bias.copy_(0.3 * rn(6)), bn.running_mean.copy_(0.3 * rn(6)), bn.running_var.copy_(1 + 0.4 * torch.rand(6, generator=gen))
    x = rn(2, 5, 4, 7).double()
    z = F.conv2d(x, conv.weight.detach().double(), conv.bias.detach().double(), padding=1)
    want = F.batch_norm(z, bn.running_mean.double(), bn.running_var.double(), bn.weight.detach().double(), bn.bias.detach().double(), False, 0.0, bn.eps)
    w, shift = UA.fold_conv_bn(conv, bn)
    assert w.dtype == shift.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (6, 5, 3, 3)
    assert rel_err(F.conv2d(x, w.double(), None, padding=1) + shift.double().reshape(1, -1, 1, 1), want) < 2e-7
    s, sh = UA.bn_scale_shift(bn, None)
    assert rel_err(z * s.reshape(1, -1, 1, 1) + sh.reshape(1, -1, 1, 1), F.batch_norm(
        z, bn.running_mean.double(), bn.running_var.double(), bn.weight.detach().double(), bn.bias.detach().double(), False, 0.0, bn.eps)) < 1e-14
    g, sd, _, _ = keyed_golden("g22_unetatt_gate_24_12_6x10")
    gate = UA.AttentionBlock(24, 24, 12).eval()
    gate.load_state_dict(sd, strict=True)
    wf, bf, wp, bp = UA.fold_gate(gate)
    assert tuple(wf.shape) == (12, 48) and tuple(bf.shape) == (12,) and tuple(wp.shape) == (12,) and isinstance(bp, float)
    rows = torch.cat([nhwc(g["x"]), nhwc(g["x2"])], dim=-1)
    psi = torch.sigmoid(torch.relu(rows @ wf.double().T + bf.double()) @ wp.double() + bp)
    assert rel_err(nhwc(g["x2"]) * psi[..., None], nhwc(g["y64"])) < 2e-7


def test_entry_points_are_declared_bound_and_exported():
    import tante_amd
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "unet_att.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert int(L.tante_abi_version()) == _lib.ABI_VERSION == 14
    assert "AttentionUNet" in tante_amd.__all__ and tante_amd.AttentionUNet is tante_amd.unet_att.AttentionUNet
    assert "TANTE_UNETATT_MFMA" in tante_amd.options.host_options() and tante_amd.get_option("TANTE_UNETATT_MFMA") is True
    assert "TANTE_CONV3_FORM" in _lib.LIB_OPTIONS
    tante_amd.set_option("TANTE_UNETATT_MFMA", 0)
    try:
        assert tante_amd.unet_att.MFMA is False
    finally:
        tante_amd.set_option("TANTE_UNETATT_MFMA", 1)


def test_supported_predicates_agree_with_their_python_mirrors():
    from tante_amd import _lib
    from tante_amd import unet_att as UA
    L = _lib.lib()
    n_yes = 0
    for n in (-1, 0, 2, 2 ** 31 - 1, 2 ** 31):
        for H, W in ((0, 4), (1, 1), (2, 3), (19, 37), (256, 256), (4, 0), (65536, 65536)):
            for Ca, Cb in ((0, 0), (1, 0), (44, 0), (24, 24), (40, 7), (1024, 1024), (2048, 0), (2048, 1), (7, -1)):
                for Cout in (0, 1, 24, 1024, 1025):
                    for form in (-1, 0, 1, 2, 3):
                        got = bool(L.tante_conv3x3_mfma_supported(n, Ca, Cb, Cout, H, W, form))
                        assert got == UA.conv3x3_mfma_supported_py(n, Ca, Cb, Cout, H, W, form), (n, Ca, Cb, Cout, H, W, form)
                        n_yes += got
    for M in (-1, 0, 1, 120, 2 ** 35 - 16, 2 ** 35 - 15):
        for Cg, Cx in ((0, 4), (4, 0), (1, 1), (24, 24), (64, 64), (512, 512), (512, 513), (1000, 24)):
            for N in (0, 1, 12, 32, 256, 257):
                got = bool(L.tante_attn_gate_supported(M, Cg, Cx, N))
                assert got == UA.attn_gate_supported_py(M, Cg, Cx, N), (M, Cg, Cx, N)
                n_yes += got
    assert n_yes > 200
    for Cin, Cout, compute, ok in ((1, 1, 0, True), (2048, 1024, 1, True), (2049, 8, 0, False), (8, 1025, 0, False), (0, 8, 0, False), (8, 8, 2, False)):
        assert (int(L.tante_conv3x3_pack_bytes(Cin, Cout, compute)) > 0) == ok
    assert int(L.tante_conv3x3_pack_bytes(7, 24, 0)) == 2 * 1 * 9 * 64 * 16 and int(L.tante_conv3x3_pack_bytes(130, 72, 1)) == 5 * 5 * 9 * 64 * 16
    assert int(L.tante_attn_gate_stream_bytes(64, 64, 32, 0)) == 4 * (2 * 32 + 4) + 2 * 8 * 64 * 16
    assert int(L.tante_attn_gate_stream_bytes(512, 513, 32, 0)) == -1 and int(L.tante_attn_gate_stream_bytes(64, 64, 32, 5)) == -1


def test_every_refusal_has_its_code_and_message():
    """Host-only argument checks: the refusal names its entry and its reason and launches nothing."""
    from tante_amd import _lib
    L = _lib.lib()

    def err():
        return L.tante_last_error()

    def conv(Ca=8, Cb=0, n=2, H=4, W=4, form=0, Hs=4, Ws=4, Cout=8, act=0, compute=0, ydt=0):
        return L.tante_conv3x3_mfma(None, Ca, None, Cb, n, H, W, form, Hs, Ws, None, None, Cout, act, compute, None, ydt, None)
    assert conv(Ca=2049) == -2 and b"tante_conv3x3_mfma: input channels outside 1..2048" in err()
    assert conv(Ca=2000, Cb=49) == -2 and b"input channels outside 1..2048" in err()
    assert conv(Cout=1025) == -2 and b"tante_conv3x3_mfma: output channels outside 1..1024" in err()
    assert conv(H=0, Hs=0) == -2 and b"tante_conv3x3_mfma: an empty image" in err()
    assert conv(form=3) == -2 and b"an unknown source form" in err()
    assert conv(Cb=8, form=1, Hs=8, Ws=8) == -2 and b"a second source with a pooled or upsampled form" in err()
    assert conv(form=2, H=3, W=4, Hs=1, Ws=2) == -2 and b"an upsampled image of odd height or width" in err()
    assert conv(form=1, Hs=4, Ws=4) == -2 and b"does not give 4 x 4 in form 1" in err()
    assert conv(form=2, Hs=4, Ws=4) == -2 and b"does not give 4 x 4 in form 2" in err()
    assert conv(compute=2) == -1 and b"compute must be fp32 or bf16" in err()
    assert conv(ydt=3) == -1 and b"output dtype must be fp32 or bf16" in err()
    assert conv(act=1) == -1 and b"the activation must be none or ReLU" in err()
    assert conv() == -1 and b"tante_conv3x3_mfma: null argument" in err()
    assert conv(form=1, Hs=9, Ws=8) == -1 and conv(form=2, Hs=2, Ws=2) == -1        # a fitting source reaches the null check
    assert L.tante_pack_conv3x3(None, 2049, 8, 0, None, None) == -2 and b"tante_pack_conv3x3: input channels outside 1..2048" in err()
    assert L.tante_pack_conv3x3(None, 8, 0, 0, None, None) == -2 and b"tante_pack_conv3x3: output channels outside 1..1024" in err()
    assert L.tante_pack_conv3x3(None, 8, 8, 7, None, None) == -1 and b"compute must be fp32 or bf16" in err()
    assert L.tante_pack_conv3x3(None, 8, 8, 0, None, None) == -1 and b"tante_pack_conv3x3: null argument" in err()
    assert L.tante_attn_gate(None, None, 8, 512, 513, 32, None, 0, None, None) == -2 and b"tante_attn_gate: channels outside 1..1024" in err()
    assert L.tante_attn_gate(None, None, 8, 64, 64, 257, None, 0, None, None) == -2 and b"tante_attn_gate: coefficients outside 1..256" in err()
    assert L.tante_attn_gate(None, None, 8, 64, 64, 32, None, 2, None, None) == -1 and b"compute must be fp32 or bf16" in err()
    assert L.tante_attn_gate(None, None, 8, 64, 64, 32, None, 0, None, None) == -1 and b"tante_attn_gate: null argument" in err()
    assert L.tante_pack_attn_gate(None, None, None, 0.0, 0, 64, 32, 0, None, None) == -2 and b"tante_pack_attn_gate: channels outside 1..1024" in err()
    assert L.tante_pack_attn_gate(None, None, None, 0.0, 64, 64, 0, 0, None, None) == -2 and b"tante_pack_attn_gate: coefficients outside 1..256" in err()
    assert L.tante_pack_attn_gate(None, None, None, 0.0, 64, 64, 32, 0, None, None) == -1 and b"tante_pack_attn_gate: null argument" in err()


def test_out_of_scope_calls_raise():
    import tante_amd
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.AttentionUNet(4, types.SimpleNamespace(n_fields=3, n_spatial_dims=3))
    m = tante_amd.AttentionUNet(4, types.SimpleNamespace(n_fields=2, n_spatial_dims=2), depth=3)
    x = torch.zeros(1, 4, 2, 8, 8)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)                                                                      # train mode
    m.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)                                                                      # grad enabled on parameters that require grad
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x)
        with pytest.raises(ValueError, match="t \\* c"):
            m(torch.zeros(1, 3, 2, 8, 8))
        with pytest.raises(ValueError, match="multiples of 2 \\*\\* \\(depth - 1\\)"):
            m(torch.zeros(1, 4, 2, 8, 10))
        with pytest.raises(ValueError, match="3-D fields are out of scope"):
            m(torch.zeros(1, 4, 2, 8, 8, 8))                                      # b t c d h w
        with pytest.raises(ValueError, match="expected \\(B, T, C, H, W\\)"):
            m(torch.zeros(1, 8, 8, 8))
        with pytest.raises(RuntimeError, match="GPU only"):
            m.Conv1(torch.zeros(1, 8, 4, 4))
        with pytest.raises(RuntimeError, match="GPU only"):
            m.Att2(torch.zeros(1, 64, 4, 4), torch.zeros(1, 64, 4, 4))


@pytest.mark.parametrize("name", list(MODELS))
def test_shipped_bf16_sites_meet_the_bar_in_exact_bf16_arithmetic(name):
    """The shipped tuple, and each of its groups alone, evaluated with exactly-rounded bf16 operands: the figures DESIGN 4.9 quotes."""
    import tante_amd.unet_att as UA
    assert UA.BF16_SITES == ("conv", "gate", "head")
    g, sd, _, _ = keyed_golden(name)
    for sites, figure in BF16_FIGURES[name].items():
        assert set(sites) <= set(UA.BF16_SITES)
        y = R.model(g["x"], sd, bf16_sites=sites)
        r, m = rel_err(y, g["y64"]), max_rel(y, g["y64"])
        assert r < 1e-2 and m < 2e-2, (sites, r, m)
        assert abs(r - figure) <= 0.03 * figure, (sites, r, figure)
