"""CPU: the AViT baseline's host side -- the float64 restatement (tests/avit_ref.py) pinned to the reference's fixtures, the fixtures' own
conditions, the Python mirrors of the library's predicates, the weight folds, the relative-position bias table, the state-dict layout, the
config aliases, and that the source is built and its entry points are declared, bound and resolve at ABI 14."""
import os
import re
import types

import numpy as np
import pytest
import torch

import avit_ref as R
from conftest import load_golden_raw, max_rel, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_RATIO, MAX_ERR32 = 0.2, 5e-6
SPATIAL = "g20_avit_spatial_5x7"
TEMPORAL = {"g20_avit_temporal_T4": 4, "g20_avit_temporal_T6": 6}
MODELS = {"g20_avit_model_32x48_T4": dict(embed_dim=48, heads=3, depth=2, n_states=3, c=3, res=(32, 48), T=4),
          "g20_avit_model_64x64_T6": dict(embed_dim=64, heads=1, depth=1, n_states=3, c=2, res=(64, 64), T=6)}
ENTRY_POINTS = ["tante_instnorm_supported", "tante_instnorm_workspace_bytes", "tante_instnorm", "tante_axial_attention_supported",
                "tante_axial_attention", "tante_time_attention_supported", "tante_time_attention", "tante_field_stats_supported",
                "tante_field_stats_workspace_bytes", "tante_field_stats", "tante_field_affine_supported", "tante_field_affine"]


def keyed_golden(name):
    """-> (tensors, state dict, key list) of a fixture (its key list is a string array)."""
    raw = load_golden_raw(name)
    g = {k: torch.from_numpy(v) for k, v in raw.items() if k != "keys"}
    return g, {k[2:]: v for k, v in g.items() if k.startswith("w.")}, [str(k) for k in raw["keys"]]


def model_kwargs(name):
    c = MODELS[name]
    return dict(in_T=4, dset_metadata=types.SimpleNamespace(n_fields=c["n_states"]), out_steps=1, embed_dim=c["embed_dim"], num_heads=c["heads"],
                processor_blocks=c["depth"])


def pinned(y, want):
    assert y.shape == want.shape
    assert rel_err(y, want) <= 1e-6 and max_rel(y, want) <= 2e-6, (rel_err(y, want), max_rel(y, want))


def test_restatement_reproduces_the_reference_blocks():
    g, sd, _ = keyed_golden(SPATIAL)
    pinned(R.spatial_block(g["x"].permute(0, 2, 3, 1), sd, "", int(g["heads"])).permute(0, 3, 1, 2), g["y"])
    for name, T in TEMPORAL.items():
        g, sd, _ = keyed_golden(name)
        assert g["x"].shape[0] == T
        pinned(R.temporal_block(g["x"].permute(0, 1, 3, 4, 2), sd, "", int(g["heads"])).permute(0, 1, 4, 2, 3), g["y"])


def test_restatement_reproduces_the_reference_stem_and_head():
    g, sd, _ = keyed_golden("g20_avit_stem")
    pinned(R.stem(g["x"].permute(0, 2, 3, 1), sd).permute(0, 3, 1, 2), g["y"])
    g, sd, _ = keyed_golden("g20_avit_head")
    pinned(R.head(g["x"].permute(0, 2, 3, 1), sd, range(int(g["n_labels"]))).permute(0, 3, 1, 2), g["y"])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_restatement_reproduces_the_reference_model(name):
    g, sd, _ = keyed_golden(name)
    c = MODELS[name]
    assert (int(g["embed_dim"]), int(g["heads"]), int(g["depth"]), int(g["n_states"])) == (c["embed_dim"], c["heads"], c["depth"], c["n_states"])
    assert tuple(g["x"].shape) == (2, c["T"], c["c"], *c["res"]) and tuple(g["y"].shape) == (2, min(c["T"], 4), c["c"], *c["res"])
    pinned(R.model(g["x"], sd, c["heads"], c["depth"]), g["y"])


def test_fixtures_hold_their_conditions():
    """(a) the blocks contribute >= 0.2 (a default-initialised block adds 2e-6 of its input); (b) the reference's own fp32 is within half
    the fp32 bar of its float64."""
    for name in [SPATIAL] + list(TEMPORAL) + list(MODELS):
        raw = load_golden_raw(name)
        assert float(raw["ratio"]) >= MIN_RATIO, (name, float(raw["ratio"]))
    for name in [SPATIAL, "g20_avit_stem", "g20_avit_head"] + list(TEMPORAL) + list(MODELS):
        assert float(load_golden_raw(name)["err32"]) <= MAX_ERR32, name
    g, sd, _ = keyed_golden(SPATIAL)
    y = R.spatial_block(g["x"].permute(0, 2, 3, 1), sd, "", 3).permute(0, 3, 1, 2)
    ratio = float((y - g["x"]).pow(2).mean().sqrt() / g["x"].double().pow(2).mean().sqrt())
    assert abs(ratio - float(g["ratio"])) < 1e-4


@pytest.mark.parametrize("T", [1, 2, 4, 6, 16])
def test_bias_table_restates_the_reference_buckets(T):
    """The host's bucket and bias tables (float32 torch logarithm, max_distance 32) against the pure-Python buckets of the restatement."""
    from tante_amd import avit as A
    emb = torch.randn(32, 5, generator=torch.Generator().manual_seed(T))
    got = A.time_bias_table(emb, T)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, T, T)
    assert torch.equal(got.double(), R.bias_table(emb, T))
    b = A.time_bucket_table(T)
    assert b.dtype == torch.long and b.tolist() == [[R.bucket(k - q) for k in range(T)] for q in range(T)]
    if T == 16:     # the log branch is reached, and max_distance 128 (the module's attribute, which compute_bias never passes) would differ
        assert int(b[0, 15]) == 16 + 11 and int(b[15, 0]) == 11
        assert not torch.equal(b, A.time_bucket_table(T, max_distance=128))
    m = A.RelativePositionBias(n_heads=5)
    with torch.no_grad():
        m.relative_attention_bias.weight.copy_(emb)
    assert torch.equal(m(T, T)[0], got) and m.max_distance == 128


def test_weight_folds_equal_the_direct_evaluation():
    from tante_amd import avit as A
    gen = torch.Generator().manual_seed(7)
    w, b, gamma = torch.randn(24, 24, 1, 1, generator=gen), torch.randn(24, generator=gen), torch.randn(24, generator=gen)
    x = torch.randn(10, 24, generator=gen, dtype=torch.float64)
    wf, bf = A.fold_layer_scale(w, b, gamma)
    want = gamma.double() * (x @ w.double().reshape(24, 24).T + b.double())
    assert rel_err(x @ wf.double().T + bf.double(), want) < 1e-7
    wf0, bf0 = A.fold_layer_scale(w, b, None)
    assert torch.equal(wf0, w.reshape(24, 24)) and torch.equal(bf0, b)
    # the stem: scale * linear over 3 of 5 states, then the 4 x 4 / 4 convolution, against one folded convolution on im2col columns
    bag_w, bag_b, conv_w = torch.randn(12, 5, generator=gen), torch.randn(12, generator=gen), torch.randn(12, 12, 4, 4, generator=gen)
    xn = torch.randn(2, 8, 12, 3, generator=gen, dtype=torch.float64)
    z = (5 / 3) ** 0.5 * (xn @ bag_w.double()[:, :3].T + bag_b.double())
    want = R.conv(z, conv_w)
    wf, bf = A.fold_stem(bag_w, bag_b, conv_w, 3)
    assert tuple(wf.shape) == (12, 48) and tuple(bf.shape) == (12,)
    cols = xn.reshape(2, 2, 4, 3, 4, 3).permute(0, 1, 3, 2, 4, 5).reshape(2, 2, 3, 48)          # (kh, kw, c) columns
    assert rel_err(cols @ wf.double().T + bf.double(), want) < 1e-6


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_matches_the_reference_layout(name):
    import tante_amd
    g, sd, keys = keyed_golden(name)
    m = tante_amd.AViT(**model_kwargs(name))
    mine = m.state_dict()
    assert list(mine) == keys
    if MODELS[name]["depth"] == 2:
        assert len(keys) == 89
    for k in keys:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd, strict=True)


def test_constructor_mirrors_the_reference():
    import tante_amd
    from tante_amd import avit as A
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=3), out_steps=1, embed_dim=48, num_heads=3, processor_blocks=3, drop_path=0.2)
    assert np.allclose(m.dp, np.linspace(0, 0.2, 3)) and m.out_steps == 1 and m.drop_path == 0.2 and tuple(m.patch_size) == (16, 16)
    assert isinstance(m.blocks[0].spatial.drop_path, torch.nn.Identity) and isinstance(m.blocks[2].temporal.drop_path, A.DropPath)
    assert m.blocks[2].spatial.drop_path.drop_prob == pytest.approx(0.2)
    assert isinstance(m.blocks[0].spatial.rel_pos_bias, A.RelativePositionBias)              # held, never applied
    assert tuple(m.space_bag.weight.shape) == (12, 3) and tuple(m.debed.out_kernel.shape) == (12, 3, 4, 4)
    assert tuple(m.embed.in_proj[0].weight.shape) == (12, 12, 4, 4)                           # 4 . 2 . 2 whatever patch_size says
    assert tante_amd.AViT(4).space_bag.dim_in == 11 and tante_amd.AViT(4, processor_blocks=1).embed.embed_dim == 768
    for cls in ("ContinuousPositionBias1D", "RelativePositionBias", "MLP", "RMSInstanceNorm2d", "SubsampledLinear", "hMLP_stem", "hMLP_output",
                "AxialAttentionBlock", "AttentionBlock", "SpaceTimeBlock", "DropPath", "AViT"):
        assert issubclass(getattr(A, cls), torch.nn.Module)
    import sys
    assert "timm" not in sys.modules


def test_config_aliases_build_the_reference_model_block():
    import tante_amd
    from tante_amd import config
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "avit_am.yaml"))
    assert cfg["model"] == {"_target_": "models.AViT", "in_T": 4, "out_steps": 1, "patch_size": [16, 16], "processor_blocks": 12,
                            "embed_dim": 384, "num_heads": 6}
    assert config._TARGET_ALIASES["models.avit.AViT"] == config._TARGET_ALIASES["models.AViT"] == "tante_amd.avit.AViT"
    wl = cfg["workload"]
    m = tante_amd.build_model(cfg, tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"])))
    assert isinstance(m, tante_amd.AViT) and len(m.blocks) == 12 and m.blocks[0].spatial.num_heads == 6 and m.space_bag.dim_in == 11
    assert len(m.state_dict()) == 19 + 12 * 35
    cfg["model"]["_target_"] = "models.avit.AViT"
    assert isinstance(tante_amd.build_model(cfg, tante_amd.TanteMetadata(n_fields=11, spatial_resolution=(256, 256)), processor_blocks=1), tante_amd.AViT)


def test_out_of_scope_constructions_and_modes_say_so():
    import tante_amd
    from tante_amd import avit as A
    with pytest.raises(NotImplementedError, match="override_block"):
        tante_amd.AViT(4, override_block=A.SpaceTimeBlock)
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=2), embed_dim=32, num_heads=2, processor_blocks=1)
    x = torch.randn(1, 2, 2, 16, 32)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.train()(x)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.eval()(x)                                  # grad enabled with trainable parameters
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(x)
    with pytest.raises(ValueError, match="compute must be"):
        m.set_compute("fp16")


def test_entry_points_are_declared_bound_and_exported():
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "avit_ops.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert int(L.tante_abi_version()) == _lib.ABI_VERSION == 14
    assert (_lib.INSTNORM_INSTANCE, _lib.INSTNORM_RMS) == (0, 1)


def test_supported_predicates_agree_with_their_python_mirrors():
    from tante_amd import _lib
    from tante_amd import avit as A
    L = _lib.lib()
    n_yes = 0
    for n in (-1, 0, 1, 16, 2 ** 31 - 1, 2 ** 31):
        for HW in (0, 1, 2, 35, 4096, 4097):
            for C in (0, 1, 48, 64, 65, 384, (1 << 24) + 1):
                got = bool(L.tante_instnorm_supported(n, HW, C))
                assert got == A.instnorm_supported_py(n, HW, C), (n, HW, C)
                n_yes += got
                assert (int(L.tante_instnorm_workspace_bytes(n, HW, C)) >= 0) == got
    for n in (-1, 0, 2, 2 ** 31 // 64 + 1):
        for heads in (0, 1, 6, 65536):
            for H, W in ((0, 4), (1, 5), (16, 16), (64, 64), (65, 3), (3, 65)):
                for hd in (8, 16, 32, 48, 64, 128):
                    got = bool(L.tante_axial_attention_supported(n, heads, H, W, hd))
                    assert got == A.axial_attention_supported_py(n, heads, H, W, hd), (n, heads, H, W, hd)
                    n_yes += got
    for nseq in (-1, 0, 13, 2 ** 31 - 1, 2 ** 31):
        for T in (0, 1, 4, 16, 17):
            for heads in (0, 3, 65536):
                for hd in (16, 24, 64):
                    got = bool(L.tante_time_attention_supported(nseq, T, heads, hd))
                    assert got == A.time_attention_supported_py(nseq, T, heads, hd), (nseq, T, heads, hd)
                    n_yes += got
    for B in (-1, 0, 4, 2 ** 31):
        for T in (0, 1, 4):
            for C in (0, 1, 11):
                for HW in (0, 1, 2, 65536, 2 ** 30, 2 ** 30 + 1):
                    got = bool(L.tante_field_stats_supported(B, T, C, HW))
                    assert got == A.field_stats_supported_py(B, T, C, HW), (B, T, C, HW)
                    n_yes += got
                    assert (int(L.tante_field_stats_workspace_bytes(B, T, C, HW)) >= 0) == got
                    got = bool(L.tante_field_affine_supported(B, T, C, HW))
                    assert got == A.field_affine_supported_py(B, T, C, HW), (B, T, C, HW)
                    n_yes += got
    assert L.tante_field_affine_supported(1, 1, 1, 1) == 1 and A.field_affine_supported_py(1, 1, 1, 1)      # one pixel de-normalises; it has no std
    assert not L.tante_field_affine_supported(4, 2 ** 31 - 1, 11, 2 ** 30) and not A.field_affine_supported_py(4, 2 ** 31 - 1, 11, 2 ** 30)
    assert n_yes > 100


def test_every_refusal_has_its_code_and_message():
    """Host-only argument checks: the refusal names its entry and its reason and launches nothing."""
    from tante_amd import _lib
    L = _lib.lib()

    def err():
        return L.tante_last_error()
    assert L.tante_instnorm(None, 1, 1, 8, 1, 1e-8, None, None, 0, None, None, None, 0, None, 0, None) == -2
    assert b"tante_instnorm: tokens per image outside 2..4096" in err()
    assert L.tante_instnorm(None, 1, 4097, 8, 0, 1e-5, None, None, 0, None, None, None, 0, None, 0, None) == -2
    assert L.tante_instnorm(None, 1, 4, 8, 2, 1e-5, None, None, 0, None, None, None, 0, None, 0, None) == -1
    assert b"form must be instance (0) or rms (1)" in err()
    assert L.tante_instnorm(None, 1, 4, 8, 0, 1e-5, None, None, 0, None, None, None, 0, None, 0, None) == -1
    assert b"null argument" in err()
    assert L.tante_axial_attention(None, 1, 2, 65, 4, 16, None, None, None, None, 1e-5, None, None) == -2
    assert b"tante_axial_attention: token axes outside 1..64" in err()
    assert L.tante_axial_attention(None, 1, 2, 4, 4, 48, None, None, None, None, 1e-5, None, None) == -2
    assert b"head dim not one of 16, 32, 64" in err()
    assert L.tante_time_attention(None, 8, 17, 2, 16, None, None, None, None, 1e-5, None, None, None) == -2
    assert b"tante_time_attention: time steps outside 1..16" in err()
    assert L.tante_time_attention(None, 8, 4, 2, 20, None, None, None, None, 1e-5, None, None, None) == -2
    assert b"head dim not one of 16, 32, 64" in err()
    assert L.tante_field_stats(None, 1, 1, 1, 1, 1e-7, None, None, None, 0, None) == -2
    assert b"tante_field_stats: fewer than two values per (sample, field)" in err()
    assert L.tante_field_affine(None, None, 1, 0, 1, 4, None, None) == -2
    assert b"tante_field_affine: an empty axis" in err()
    assert L.tante_field_affine(None, None, 2 ** 31, 1, 1, 4, None, None) == -2
    assert b"tante_field_affine: more than 2^31 - 1 (sample, field) pairs per call" in err()
    m = __import__("tante_amd").avit.RelativePositionBias(bidirectional=False)
    with pytest.raises(NotImplementedError, match="bidirectional = False"):
        m(4, 4)
