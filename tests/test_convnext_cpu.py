"""CPU: the UNetConvNext baseline's fixtures, its float64 restatement, the host mirror's layout, the folds, the entry points, the
predicates, the refusals and the bf16-site pin.  Nothing here touches a GPU."""
import os
import re
import types

import pytest
import torch

import convnext_ref as R
from conftest import load_golden_raw, max_rel, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_RATIO, MAX_ERR32 = 0.2, 5e-6
BLOCKS = {"g21_convnext_block_c15_5x7": (15, 5, 7), "g21_convnext_block_c32_9x20": (32, 9, 20)}
MODELS = {"g21_convnext_model_f15_s2_20x28": dict(init_features=15, stages=2, blocks_per_stage=2, blocks_at_neck=1, n_fields=3, res=(20, 28), keys=103),
          "g21_convnext_model_f8_s3_16x24": dict(init_features=8, stages=3, blocks_per_stage=1, blocks_at_neck=2, n_fields=2, res=(16, 24), keys=104)}
ENTRY_POINTS = ["tante_convnext_block_supported", "tante_convnext_stream_bytes", "tante_pack_convnext", "tante_convnext_block",
                "tante_dwconv_ln_supported", "tante_dwconv_ln", "tante_l2norm_rows_supported", "tante_l2norm_rows", "tante_conv3x3_supported",
                "tante_conv3x3"]
# the exact-bf16 evaluation of the restatement (operands of the named groups rounded to bf16, products exact) on the two model fixtures,
# rel L2 against float64: every group, and all of them together, is under the 1e-2 bar, so all three ship
BF16_FIGURES = {"g21_convnext_model_f15_s2_20x28": {("block",): 8.6e-4, ("resample",): 8.2e-4, ("skip",): 3.5e-4, ("block", "resample", "skip"): 1.23e-3},
                "g21_convnext_model_f8_s3_16x24": {("block",): 2.53e-3, ("resample",): 2.91e-3, ("skip",): 2.02e-3, ("block", "resample", "skip"): 4.71e-3}}


def keyed_golden(name):
    """-> (tensors, state dict, key list) of a fixture (its key list is a string array)."""
    raw = load_golden_raw(name)
    g = {k: torch.from_numpy(v) for k, v in raw.items() if k != "keys"}
    return g, {k[2:]: v for k, v in g.items() if k.startswith("w.")}, [str(k) for k in raw["keys"]]


def model_kwargs(name):
    c = MODELS[name]
    return dict(in_T=4, dset_metadata=types.SimpleNamespace(n_fields=c["n_fields"], n_spatial_dims=2), stages=c["stages"],
                blocks_per_stage=c["blocks_per_stage"], blocks_at_neck=c["blocks_at_neck"], init_features=c["init_features"])


def pinned(y, g):
    """The restatement against the reference's float64 result; the stored fp32 `y` is that result rounded once."""
    assert y.dtype == torch.float64 and y.shape == g["y64"].shape
    assert rel_err(y, g["y64"]) <= 1e-10 and max_rel(y, g["y64"]) <= 2e-10, (rel_err(y, g["y64"]), max_rel(y, g["y64"]))
    assert torch.equal(g["y"], g["y64"].float())


def nhwc(t):
    return t.double().permute(0, 2, 3, 1)


def test_restatement_reproduces_the_reference_blocks_and_stages():
    for name in BLOCKS:
        g, sd, _ = keyed_golden(name)
        pinned(R.block(nhwc(g["x"]), sd).permute(0, 3, 1, 2), g)
    g, sd, _ = keyed_golden("g21_convnext_down_c15")
    pinned(R.downsample(nhwc(g["x"]), sd).permute(0, 3, 1, 2), g)
    g, sd, _ = keyed_golden("g21_convnext_up_c30")
    pinned(R.upsample(nhwc(g["x"]), sd).permute(0, 3, 1, 2), g)
    g, sd, _ = keyed_golden("g21_convnext_stage_skip_c30")
    x = nhwc(g["x"])
    pinned(R.stage(x[..., :30], sd, "", 1, "up", x[..., 30:]).permute(0, 3, 1, 2), g)


@pytest.mark.parametrize("name", list(MODELS))
def test_restatement_reproduces_the_reference_model(name):
    g, sd, _ = keyed_golden(name)
    c = MODELS[name]
    assert (int(g["init_features"]), int(g["stages"]), int(g["blocks_per_stage"]), int(g["blocks_at_neck"]), int(g["n_fields"]), int(g["in_T"])) == \
        (c["init_features"], c["stages"], c["blocks_per_stage"], c["blocks_at_neck"], c["n_fields"], 4)
    assert tuple(g["x"].shape) == (2, 4, c["n_fields"], *c["res"])
    pinned(R.model(g["x"], sd), g)


def test_fixtures_hold_their_conditions():
    """(a) the blocks contribute >= 0.2 (a default-initialised block adds 1e-6 of its input); (b) the reference's own fp32 is within half
    the fp32 bar of its float64; every file is under the size limit."""
    for name in list(BLOCKS) + list(MODELS):
        g, sd, _ = keyed_golden(name)
        assert float(g["ratio"]) >= MIN_RATIO, (name, float(g["ratio"]))
        assert all(float((v - 0.5).abs().max()) < 0.3 for k, v in sd.items() if k.split(".")[-1] == "gamma")
    for name in list(BLOCKS) + list(MODELS) + ["g21_convnext_down_c15", "g21_convnext_up_c30", "g21_convnext_stage_skip_c30"]:
        g, _, _ = keyed_golden(name)
        assert 0 < float(g["err32"]) <= MAX_ERR32, (name, float(g["err32"]))
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1000 * 1000
    for name in BLOCKS:                                             # the stored ratio is what it says
        g, _, _ = keyed_golden(name)
        got = float(((g["y64"] - g["x"].double()) ** 2).mean().sqrt() / (g["x"].double() ** 2).mean().sqrt())
        assert abs(got - float(g["ratio"])) < 1e-9
    for name in MODELS:                                             # and so is the models': the restatement with every gamma zeroed
        g, sd, _ = keyed_golden(name)
        sd0 = {k: (torch.zeros_like(v) if k.split(".")[-1] == "gamma" else v) for k, v in sd.items()}
        y, y0 = g["y64"], R.model(g["x"], sd0)
        got = float(((y - y0) ** 2).mean().sqrt() / (y ** 2).mean().sqrt())
        assert abs(got - float(g["ratio"])) < 1e-8, (got, float(g["ratio"]))


@pytest.mark.parametrize("name", list(MODELS))
def test_state_dict_matches_the_reference_layout(name):
    import tante_amd
    g, sd, keys = keyed_golden(name)
    m = tante_amd.UNetConvNext(**model_kwargs(name))
    own = m.state_dict()
    assert list(own.keys()) == keys and len(keys) == MODELS[name]["keys"]
    for k in keys:
        assert tuple(own[k].shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd, strict=True)
    assert not any(isinstance(mod, torch.nn.Dropout) or type(mod).__name__ == "DropPath" for mod in m.modules())


def test_module_fixtures_load_strictly():
    import tante_amd.convnext as CN
    for name, make in (("g21_convnext_block_c15_5x7", lambda: CN.Block(15, 2)), ("g21_convnext_down_c15", lambda: CN.Downsample(15, 30, 2)),
                       ("g21_convnext_up_c30", lambda: CN.Upsample(30, 15, 2)),
                       ("g21_convnext_stage_skip_c30", lambda: CN.Stage(30, 15, 2, depth=1, mode="up", skip_project=True))):
        _, sd, keys = keyed_golden(name)
        m = make()
        assert list(m.state_dict().keys()) == keys
        m.load_state_dict(sd, strict=True)


def test_constructor_mirrors_the_reference():
    import tante_amd
    import tante_amd.convnext as CN
    md = types.SimpleNamespace(n_fields=3, n_spatial_dims=2)
    assert len(tante_amd.UNetConvNext(4, md, stages=2, blocks_per_stage=2, blocks_at_neck=1, init_features=15).state_dict()) == 103
    assert len(tante_amd.UNetConvNext(4, md, stages=4, blocks_per_stage=1, blocks_at_neck=1, init_features=15).state_dict()) == 123
    m = tante_amd.UNetConvNext(4, md, n_spatial_dims=3, gradient_checkpointing=True)          # the argument is ignored: the metadata decides
    assert m.n_spatial_dims == 2 and m.gradient_checkpointing is True and m.dset_metadata is md
    assert (m.in_proj.in_channels, m.in_proj.out_channels, m.out_proj.in_channels, m.out_proj.out_channels) == (12, 32, 32, 3)
    assert len(m.encoder) == len(m.decoder) == 4 and len(m.neck.blocks) == 1 and m.neck.blocks[0].dwconv.weight.shape[0] == 512
    assert isinstance(m.neck.resample, torch.nn.Identity) and isinstance(m.neck.skip_proj, torch.nn.Identity)
    assert isinstance(m.decoder[0].skip_proj, torch.nn.Identity) and isinstance(m.decoder[1].skip_proj, torch.nn.Conv2d)
    assert tuple(m.decoder[1].skip_proj.weight.shape) == (256, 512, 1, 1)
    assert isinstance(m.encoder[0].resample, CN.Downsample) and isinstance(m.decoder[0].resample, CN.Upsample)
    cf = m.encoder[0].resample.block[0]
    assert cf.data_format == "channels_first" and tuple(cf.weight.shape) == tuple(cf.bias.shape) == (32, 1, 1) and cf.eps == 1e-6
    blk = m.encoder[0].blocks[0]
    assert blk.norm.data_format == "channels_last" and blk.norm.eps == 1e-6 and isinstance(blk.act, torch.nn.GELU) and blk.act.approximate == "none"
    assert isinstance(blk.drop_path, torch.nn.Identity) and float(blk.gamma[0]) == pytest.approx(1e-6)
    assert tuple(blk.dwconv.weight.shape) == (32, 1, 7, 7) and blk.dwconv.padding == (3, 3) and blk.dwconv.groups == 32
    nog = CN.Block(8, 2, layer_scale_init_value=0.0)
    assert nog.gamma is None and "gamma" not in nog.state_dict()
    with pytest.raises(NotImplementedError):
        CN.LayerNorm(4, 2, data_format="channels_middle")
    assert m.set_compute("bf16") is m and m.compute == "bf16"
    with pytest.raises(ValueError):
        m.set_compute("fp8")


def test_config_aliases_build_the_reference_model_block():
    import tante_amd
    from tante_amd import config
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_convnext_am.yaml"))
    ref = tante_amd.load_config(os.path.join(ROOT, "configs", "avit_am.yaml"))
    assert cfg["model"] == {"_target_": "models.UNetConvNext", "in_T": 4, "blocks_per_stage": 4, "init_features": 15}
    assert cfg["workload"] == dict(ref["workload"], batch_size=4) and cfg["workload"]["spatial_resolution"] == [256, 256]
    md = types.SimpleNamespace(n_fields=cfg["workload"]["n_fields"], n_spatial_dims=2)
    for target in ("models.UNetConvNext", "models.unet_convnext.UNetConvNext"):
        assert config._TARGET_ALIASES[target] == "tante_amd.convnext.UNetConvNext"
        m = tante_amd.build_model(dict(cfg, model=dict(cfg["model"], _target_=target)), md)
        assert isinstance(m, tante_amd.UNetConvNext) and m.dim_in == 44
        widths = [st.blocks[0].dwconv.weight.shape[0] for st in m.encoder] + [m.neck.blocks[0].dwconv.weight.shape[0]]
        assert widths == [15, 30, 60, 120, 240] and sum(len(st.blocks) for st in list(m.encoder) + [m.neck] + list(m.decoder)) == 33


def test_weight_folds_equal_the_direct_evaluation():
    import tante_amd.convnext as CN
    gen = torch.Generator().manual_seed(5)
    C = 12
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    nw, nb, w1, b1, w2, b2, gamma = 1 + 0.3 * rn(C), 0.3 * rn(C), rn(4 * C, C), rn(4 * C), rn(C, 4 * C), rn(C), rn(C)
    z = rn(7, C).double()
    for g_ in (gamma, None):
        w1f, b1f, w2f, b2f = CN.fold_block(nw, nb, w1, b1, w2, b2, g_)
        assert w1f.dtype == torch.float32 and w1f.is_contiguous() and w2f.is_contiguous()
        h = (z * nw.double() + nb.double()) @ w1.double().T + b1.double()
        assert rel_err(z @ w1f.double().T + b1f.double(), h) < 2e-7
        y = R.gelu(h) @ w2.double().T + b2.double()
        y = y if g_ is None else y * g_.double()
        assert rel_err(R.gelu(h) @ w2f.double().T + b2f.double(), y) < 2e-7
    cw, dw_, cn = rn(9, C, 2, 2), rn(C, 9, 2, 2), 1 + 0.3 * rn(C, 1, 1)
    x = rn(2, C, 4, 6).double()
    xn = x * cn.double()
    want = torch.nn.functional.conv2d(xn, cw.double(), stride=2)
    assert rel_err(torch.nn.functional.conv2d(x, CN.fold_cf_norm(cw, cn).double(), stride=2), want) < 2e-7
    want = torch.nn.functional.conv_transpose2d(xn, dw_.double(), stride=2)
    folded = CN.fold_cf_norm(dw_.transpose(0, 1), cn).transpose(0, 1)
    assert rel_err(torch.nn.functional.conv_transpose2d(x, folded.double(), stride=2), want) < 2e-7


def test_entry_points_are_declared_bound_and_exported():
    import tante_amd
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "convnext.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert int(L.tante_abi_version()) == _lib.ABI_VERSION == 14
    assert "UNetConvNext" in tante_amd.__all__ and tante_amd.UNetConvNext is tante_amd.convnext.UNetConvNext
    assert "TANTE_CONVNEXT_FUSED" in tante_amd.options.host_options() and tante_amd.get_option("TANTE_CONVNEXT_FUSED") is True
    tante_amd.set_option("TANTE_CONVNEXT_FUSED", 0)
    try:
        assert tante_amd.convnext.FUSED is False
    finally:
        tante_amd.set_option("TANTE_CONVNEXT_FUSED", 1)


def test_supported_predicates_agree_with_their_python_mirrors():
    from tante_amd import _lib
    from tante_amd import convnext as CN
    L = _lib.lib()
    n_yes = 0
    for n in (-1, 0, 1, 4, 2 ** 31 - 1, 2 ** 31):
        for H, W in ((0, 4), (1, 1), (2, 3), (19, 37), (256, 256), (4, 0), (65536, 65536)):
            for C in (0, 1, 15, 16, 240, 256, 257, 512, 513, 1024, 1025):
                got = bool(L.tante_convnext_block_supported(n, H, W, C))
                assert got == CN.convnext_block_supported_py(n, H, W, C), (n, H, W, C)
                n_yes += got
                got = bool(L.tante_dwconv_ln_supported(n, H, W, C))
                assert got == CN.dwconv_ln_supported_py(n, H, W, C), (n, H, W, C)
                n_yes += got
                assert (int(L.tante_convnext_stream_bytes(C)) > 0) == (1 <= C <= 256)
    for M in (-1, 0, 1, 37, 2 ** 33 - 4, 2 ** 33 - 3):
        for C in (0, 1, 15, 240, 1 << 24, (1 << 24) + 1):
            got = bool(L.tante_l2norm_rows_supported(M, C))
            assert got == CN.l2norm_rows_supported_py(M, C), (M, C)
            n_yes += got
    for n in (-1, 0, 2, 65535, 65536):
        for Cin in (0, 1, 44, 128, 129):
            for Cout in (0, 1, 15, 64, 65):
                for H, W in ((0, 3), (2, 3), (256, 256)):
                    got = bool(L.tante_conv3x3_supported(n, Cin, Cout, H, W))
                    assert got == CN.conv3x3_supported_py(n, Cin, Cout, H, W), (n, Cin, Cout, H, W)
                    n_yes += got
    assert n_yes > 100


def test_every_refusal_has_its_code_and_message():
    """Host-only argument checks: the refusal names its entry and its reason and launches nothing."""
    from tante_amd import _lib
    L = _lib.lib()

    def err():
        return L.tante_last_error()
    assert L.tante_convnext_block(None, None, None, 2, 4, 4, 257, 0, 1e-6, None) == -2
    assert b"tante_convnext_block: channels outside 1..256" in err()
    assert L.tante_convnext_block(None, None, None, 2, 0, 4, 16, 0, 1e-6, None) == -2
    assert b"tante_convnext_block: an empty image" in err()
    assert L.tante_convnext_block(None, None, None, 2, 4, 4, 16, 2, 1e-6, None) == -1
    assert b"compute must be fp32 or bf16" in err()
    assert L.tante_convnext_block(None, None, None, 2, 4, 4, 16, 0, 1e-6, None) == -1
    assert b"null argument" in err()
    assert L.tante_pack_convnext(None, None, None, None, None, None, 257, 0, None, None) == -2
    assert b"tante_pack_convnext: channels outside 1..256" in err()
    assert L.tante_pack_convnext(None, None, None, None, None, None, 16, 0, None, None) == -1
    assert int(L.tante_convnext_stream_bytes(257)) == -1 and int(L.tante_convnext_stream_bytes(0)) == -1
    assert L.tante_dwconv_ln(None, 2, 4, 4, 1025, None, None, 1e-6, None, None, None, 0, None) == -2
    assert b"tante_dwconv_ln: channels outside 1..1024" in err()
    assert L.tante_dwconv_ln(None, 2, 4, 4, 16, None, None, 1e-6, None, None, None, 3, None) == -1
    assert b"output dtype must be fp32 or bf16" in err()
    assert L.tante_l2norm_rows(None, 4, 0, 1e-6, None, 0, None) == -2
    assert b"tante_l2norm_rows: channels outside 1..2^24" in err()
    assert L.tante_l2norm_rows(None, 4, 8, 1e-6, None, 0, None) == -1
    assert L.tante_conv3x3(None, 2, 129, 4, 4, 1, None, None, 15, None, 0, None) == -2
    assert b"tante_conv3x3: input channels outside 1..128" in err()
    assert L.tante_conv3x3(None, 2, 12, 4, 4, 1, None, None, 65, None, 0, None) == -2
    assert b"tante_conv3x3: output channels outside 1..64" in err()
    assert L.tante_conv3x3(None, 2, 12, 4, 4, 1, None, None, 15, None, 0, None) == -1


def test_out_of_scope_calls_raise():
    import tante_amd
    import tante_amd.convnext as CN
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.UNetConvNext(4, types.SimpleNamespace(n_fields=3, n_spatial_dims=3))
    with pytest.raises(NotImplementedError, match="drop_path"):
        CN.Block(8, 2, drop_path=0.1)
    m = tante_amd.UNetConvNext(4, types.SimpleNamespace(n_fields=2, n_spatial_dims=2), stages=2, init_features=8)
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
        with pytest.raises(ValueError, match="multiples of 2 \\*\\* stages"):
            m(torch.zeros(1, 4, 2, 8, 10))
        with pytest.raises(ValueError, match="expected \\(B, T, C, H, W\\)"):
            m(torch.zeros(1, 8, 8, 8))
        with pytest.raises(NotImplementedError, match="channels_first"):
            m.encoder[0].resample.block[0](x)


@pytest.mark.parametrize("name", list(MODELS))
def test_shipped_bf16_sites_meet_the_bar_in_exact_bf16_arithmetic(name):
    """The shipped tuple, and each of its groups alone, evaluated with exactly-rounded bf16 operands: the figures DESIGN 4.8 quotes."""
    import tante_amd.convnext as CN
    assert CN.BF16_SITES == ("block", "resample", "skip")
    g, sd, _ = keyed_golden(name)
    for sites, figure in BF16_FIGURES[name].items():
        assert set(sites) <= set(CN.BF16_SITES)
        y = R.model(g["x"], sd, bf16_sites=sites)
        r, m = rel_err(y, g["y64"]), max_rel(y, g["y64"])
        assert r < 1e-2 and m < 2e-2, (sites, r, m)
        assert abs(r - figure) <= 0.03 * figure, (sites, r, figure)
    assert rel_err(R.model(g["x"], sd, bf16_sites=()), g["y64"]) <= 1e-10
