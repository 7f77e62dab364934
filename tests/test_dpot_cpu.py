"""CPU: the DPOT baseline's host side -- the float64 restatement against the reference's fixtures, the twiddle pack and the folded
time-aggregation weight against float64, the module surface, the config aliases and the C-ABI surface (host-only calls: there is no GPU
here)."""
import os
import re

import numpy as np
import pytest
import torch

import dpot_ref as R
from conftest import ROOT, load_golden, load_golden_raw, max_rel, rel_err

FILTERS = ["g19_dpot_filter_8x8_m3", "g19_dpot_filter_8x12_m16", "g19_dpot_filter_5x7_m4", "g19_dpot_filter_6x9_m2", "g19_dpot_filter_4x4_m1"]
FILTER_CF = "g19_dpot_filter_cf_6x8_m3"
# (H, W, C, nb, modes, B) as the issue lists them
FILTER_SHAPES = {"g19_dpot_filter_8x8_m3": (8, 8, 64, 2, 3, 2), "g19_dpot_filter_8x12_m16": (8, 12, 64, 2, 16, 2),
                 "g19_dpot_filter_5x7_m4": (5, 7, 48, 4, 4, 2), "g19_dpot_filter_6x9_m2": (6, 9, 40, 2, 2, 1),
                 "g19_dpot_filter_4x4_m1": (4, 4, 64, 2, 1, 1)}
BLOCKS = {"g19_dpot_block_ds0": False, "g19_dpot_block_ds1": True}
MODELS = {"g19_dpot_model_32x48_p4": dict(res=(32, 48), patch=4, modes=3, time_agg="exp_mlp", out_timesteps=1),
          "g19_dpot_model_16x16_p2": dict(res=(16, 16), patch=2, modes=16, time_agg="mlp", out_timesteps=2)}
ENTRY_POINTS = ("tante_groupnorm_supported", "tante_groupnorm_workspace_bytes", "tante_groupnorm", "tante_dpot_filter_supported",
                "tante_dpot_twiddle_floats", "tante_dpot_filter_workspace_bytes", "tante_dpot_filter")
MIN_RATIO = 0.2


def keyed_golden(name):
    """-> (tensors, state dict, key list) of a block / model fixture (its key list is a string array, which load_golden cannot take)."""
    raw = load_golden_raw(name)
    g = {k: torch.from_numpy(v) for k, v in raw.items() if k != "keys"}
    return g, {k[2:]: v for k, v in g.items() if k.startswith("w.")}, [str(k) for k in raw["keys"]]


def model_kwargs(name):
    c = MODELS[name]
    return dict(in_T=3, patch_size=c["patch"], out_timesteps=c["out_timesteps"], n_blocks=2, embed_dim=64, out_layer_dim=16, depth=2,
                modes=c["modes"], mlp_ratio=2.0, n_cls=4, time_agg=c["time_agg"])


def filter_args(g):
    return g["w1"], g["b1"], g["w2"], g["b2"], int(g["modes"])


@pytest.mark.parametrize("name", FILTERS + [FILTER_CF])
def test_restatement_reproduces_the_reference_filter(name):
    """The float64 DFT-matrix restatement against the reference's fp32 output, relative to the filter's CONTRIBUTION y - x: <= 1e-6 (the
    reference's own rounding is 1.6e-7 .. 4.4e-7)."""
    g = load_golden(name)
    x, want = g["x"], g["y"]
    if name == FILTER_CF:
        x, want = x.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)
    else:
        H, W, C, nb, modes, B = FILTER_SHAPES[name]
        assert tuple(x.shape) == (B, H, W, C) and tuple(g["w1"].shape) == (2, nb, C // nb, C // nb) and int(g["modes"]) == modes
    d = R.filter_contribution(x, *filter_args(g))
    dw = want.double() - x.double()
    assert rel_err(d, dw) <= 1e-6 and max_rel(d, dw) <= 1e-6, (rel_err(d, dw), max_rel(d, dw))
    y = R.dpot_filter(x, *filter_args(g))
    assert rel_err(y, want) <= 1e-6 and max_rel(y, want) <= 1e-6


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_restatement_reproduces_the_reference_block(name):
    g, sd, _ = keyed_golden(name)
    assert bool(g["double_skip"]) == BLOCKS[name]
    y = R.block(g["x"].permute(0, 2, 3, 1), sd, "", int(g["modes"]), BLOCKS[name]).permute(0, 3, 1, 2)
    assert y.shape == g["y"].shape
    assert rel_err(y, g["y"]) <= 1e-6 and max_rel(y, g["y"]) <= 2e-6, (rel_err(y, g["y"]), max_rel(y, g["y"]))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_restatement_reproduces_the_reference_model(name):
    g, sd, _ = keyed_golden(name)
    c = MODELS[name]
    assert (int(g["patch"]), int(g["modes"]), int(g["out_timesteps"]), bool(g["exp_mlp"])) == \
        (c["patch"], c["modes"], c["out_timesteps"], c["time_agg"] == "exp_mlp")
    y = R.model(g["x"], sd, c["patch"], c["modes"], c["time_agg"], c["out_timesteps"])
    assert y.shape == g["y"].shape
    assert rel_err(y, g["y"]) <= 1e-6 and max_rel(y, g["y"]) <= 2e-6, (rel_err(y, g["y"]), max_rel(y, g["y"]))


def test_fixture_filters_contribute():
    """A default-init mixer adds 3e-4 of its input: the fixtures hold rescaled weights, and every filter in them must add >= 0.2."""
    for name in FILTERS + [FILTER_CF]:
        g = load_golden(name)
        x = g["x"].permute(0, 2, 3, 1) if name == FILTER_CF else g["x"]
        assert float(g["ratio"]) >= MIN_RATIO, (name, float(g["ratio"]))
        assert abs(R.contribution_ratio(x, *filter_args(g)) - float(g["ratio"])) < 1e-4
    for name in list(BLOCKS) + list(MODELS):
        assert all(float(r) >= MIN_RATIO for r in np.atleast_1d(load_golden_raw(name)["ratio"])), name
    # and the parameters a default init leaves at 0 / 1 are off them
    _, sd, _ = keyed_golden("g19_dpot_model_32x48_p4")
    assert float(sd["pos_embed"].abs().max()) > 0.1 and float((sd["blocks.0.norm1.weight"] - 1).abs().max()) > 0.01
    assert float(sd["blocks.1.norm2.bias"].abs().max()) > 0.01 and float(sd["out_layer.4.bias"].abs().max()) > 0.01
    g0 = 2 ** torch.linspace(-10, 10, 64)
    assert float((sd["time_agg_layer.gamma"][0] / g0 - 1).abs().max()) > 0.01


@pytest.mark.parametrize("H,W,modes", [(8, 8, 3), (8, 12, 16), (5, 7, 4), (6, 9, 2), (4, 4, 1), (64, 33, 20), (33, 64, 64), (1, 1, 5), (8, 8, 16)])
def test_twiddle_tables_equal_the_restatement_matrices(H, W, modes):
    from tante_amd import dpot as D
    k1, k2 = D.kept_modes(H, W, modes)
    assert (k1, k2) == R.kept(H, W, modes) == (min(modes, H), min(modes, W // 2 + 1))
    cosm, sinm, _ = R.c2r_matrices(W, k2)
    want = [R.dft_matrix(W, -1)[:k2], R.dft_matrix(H, -1)[:k1], R.dft_matrix(H, +1)[:, :k1], torch.complex(cosm, sinm)]
    got = D.twiddle_tables(H, W, modes)
    for t, w in zip(got, want):
        assert t.shape == tuple(w.shape)
        assert np.abs(t - w.numpy()).max() < 1e-14
    # the columns that count once are exactly real, so their imaginary input drops out inside the kernel
    l = np.arange(k2)
    once = (l == 0) | ((W % 2 == 0) & (l == W // 2))
    assert not got[3].imag[:, once].any()
    # the packed buffer: per table a real then an imaginary plane, rows padded to 16 and columns to 4 with zeros, float32
    buf = D.pack_twiddles(H, W, modes)
    assert buf.dtype == np.float32
    off = 0
    for t in got:
        Mp, Kp = -(-t.shape[0] // 16) * 16, -(-t.shape[1] // 4) * 4
        for part in (t.real, t.imag):
            plane = buf[off: off + Mp * Kp].reshape(Mp, Kp)
            assert np.array_equal(plane[:t.shape[0], :t.shape[1]], part.astype(np.float32))
            assert not plane[t.shape[0]:].any() and not plane[:, t.shape[1]:].any()
            off += Mp * Kp
    assert off == buf.size
    from tante_amd import _lib
    assert int(_lib.lib().tante_dpot_twiddle_floats(H, W, modes)) == buf.size


@pytest.mark.parametrize("name", FILTERS)
def test_the_six_launch_decomposition_from_the_packed_buffers_reproduces_the_fixture(name):
    """What tante_dpot_filter evaluates -- T1 along w, T2 along h, the four-product complex MLP on the state dict's own weights, T3 along k,
    Re(T4 along l), each table read back from the PACKED host buffer -- in float64: ties the pack layout and the kept-corner bookkeeping to
    the reference."""
    from tante_amd import dpot as D
    g = load_golden(name)
    x, modes = g["x"].double(), int(g["modes"])
    B, H, W, C = x.shape
    nb, bs = g["w1"].shape[1], g["w1"].shape[2]
    k1, k2 = D.kept_modes(H, W, modes)
    buf, T, off = D.pack_twiddles(H, W, modes).astype(np.float64), [], 0
    for M, K in [(k2, W), (k1, H), (H, k1), (W, k2)]:
        Mp, Kp = -(-M // 16) * 16, -(-K // 4) * 4
        re, im = buf[off: off + Mp * Kp].reshape(Mp, Kp), buf[off + Mp * Kp: off + 2 * Mp * Kp].reshape(Mp, Kp)
        T.append(torch.from_numpy(re[:M, :K] + 1j * im[:M, :K]))
        off += 2 * Mp * Kp
    P = torch.einsum("lw,bhwc->blhc", T[0], x.to(torch.complex128))
    X = torch.einsum("kh,blhc->bklc", T[1], P).reshape(B, k1, k2, nb, bs)
    w1, b1, w2, b2 = (t.double() for t in (g["w1"], g["b1"], g["w2"], g["b2"]))

    def layer(re, im, w, b):
        return (torch.einsum("...gi,gio->...go", re, w[0]) - torch.einsum("...gi,gio->...go", im, w[1]) + b[0],
                torch.einsum("...gi,gio->...go", im, w[0]) + torch.einsum("...gi,gio->...go", re, w[1]) + b[1])
    ur, ui = layer(X.real, X.imag, w1, b1)
    yr, yi = layer(R.gelu(ur), R.gelu(ui), w2, b2)
    Y = torch.complex(yr, yi).reshape(B, k1, k2, C)
    Z = torch.einsum("hk,bklc->bhlc", T[2], Y)
    out = torch.einsum("wl,bhlc->bhwc", T[3], Z).real
    want = g["y"].double() - x
    assert rel_err(out, want) <= 1e-6 and max_rel(out, want) <= 1e-6, (rel_err(out, want), max_rel(out, want))


@pytest.mark.parametrize("T,C", [(3, 64), (4, 40), (1, 16)])
def test_folded_time_weight_equals_the_direct_einsum(T, C):
    """'exp_mlp': einsum('tij,...ti->...j', w, x * cos(t gamma)) == einsum with cos folded into w's rows, in float64; 'mlp' folds nothing."""
    from tante_amd import dpot as D
    gen = torch.Generator().manual_seed(T * 100 + C)
    w = torch.randn(T, C, C, generator=gen) / (T * C ** 0.5)
    gamma = (2 ** torch.linspace(-10, 10, C) * (1 + 0.1 * torch.randn(C, generator=gen))).unsqueeze(0)
    x = torch.randn(2, 3, 5, T, C, generator=gen, dtype=torch.float64)
    t = torch.linspace(0, 1, T).unsqueeze(-1)
    t_embed = torch.cos(t.double() @ gamma.double())
    want = torch.einsum("tij,...ti->...j", w.double(), x * t_embed)
    wf = D.fold_time_weight(w, gamma)
    assert wf.dtype == torch.float32 and tuple(wf.shape) == (T, C, C)
    got = torch.einsum("tij,...ti->...j", wf.double(), x)
    # the only difference is the fp32 rounding of the folded weight
    assert rel_err(got, want) < 2e-7, rel_err(got, want)
    assert torch.equal(D.fold_time_weight(w, None), w)
    assert torch.equal(R.time_weight({"time_agg_layer.w": w, "time_agg_layer.gamma": gamma}, T, "exp_mlp").float(), wf)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_matches_the_reference_layout(name):
    import tante_amd
    g, sd, keys = keyed_golden(name)
    res = MODELS[name]["res"]
    m = tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=res), **model_kwargs(name))
    mine = m.state_dict()
    assert list(mine) == keys
    for k in keys:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    p = MODELS[name]["patch"]
    assert tuple(mine["blocks.0.filter.w1"].shape) == (2, 2, 32, 32) and tuple(mine["blocks.1.filter.b2"].shape) == (2, 2, 32)
    assert tuple(mine["pos_embed"].shape) == (1, 64, res[0] // p, res[1] // p)
    assert tuple(mine["patch_embed.proj.0.weight"].shape) == (2 * p + 3, 5, p, p)
    assert ("time_agg_layer.gamma" in mine) == (MODELS[name]["time_agg"] == "exp_mlp")
    assert m.blocks[0].norm1.num_groups == 8 and m.blocks[0].norm2.eps == 1e-5 and m.blocks[0].double_skip is False
    assert (m.in_channels, m.out_channels, m.in_timesteps, m.out_timesteps, m.output_length, tuple(m.latent_size)) == \
        (2, 2, 3, MODELS[name]["out_timesteps"], MODELS[name]["out_timesteps"], (res[0] // p, res[1] // p))
    m.load_state_dict(sd, strict=True)
    for bname in BLOCKS:
        gb, sdb, kb = keyed_golden(bname)
        from tante_amd import dpot as D
        blk = D.Block(width=64, n_blocks=2, mlp_ratio=2.0, channel_first=True, modes=int(gb["modes"]), double_skip=BLOCKS[bname])
        assert list(blk.state_dict()) == kb
        blk.load_state_dict(sdb, strict=True)


def test_config_aliases_build_the_reference_model_block():
    import tante_amd
    from tante_amd import config
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "dpot_am.yaml"))
    assert cfg["model"] == {"_target_": "models.DPOT", "in_T": 4, "out_timesteps": 1, "depth": 24, "embed_dim": 1536, "mlp_ratio": 4.0,
                            "out_layer_dim": 8, "patch_size": 32, "mixing_type": "afno", "modes": 16, "n_cls": 16, "act": "gelu",
                            "time_agg": "exp_mlp"}
    assert config._TARGET_ALIASES["models.dpot.DPOT"] == config._TARGET_ALIASES["models.DPOT"] == "tante_amd.dpot.DPOT"
    wl = cfg["workload"]
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    small = dict(cfg, model=dict(cfg["model"], depth=1, embed_dim=64, _target_="models.dpot.DPOT"))
    m = tante_amd.build_model(small, md)
    assert isinstance(m, tante_amd.DPOT) and type(m).__module__ == "tante_amd.dpot"
    assert len(m.blocks) == 1 and tuple(m.latent_size) == (8, 8) and m.n_blocks == 4 and tuple(m.blocks[0].filter.w1.shape) == (2, 4, 16, 16)
    assert tuple(m.patch_embed.proj[0].weight.shape) == (11 * 32 + 3, 14, 32, 32) and tuple(m.cls_head[4].weight.shape) == (16, 64)
    with torch.device("meta"):       # the shipped geometry, without its half a billion parameters
        big = tante_amd.build_model(cfg, md)
    assert len(big.blocks) == 24 and tuple(big.blocks[0].filter.w1.shape) == (2, 4, 384, 384) and big.blocks[0].mlp[0].out_channels == 6144


def test_out_of_scope_constructions_say_so():
    import tante_amd
    from tante_amd import dpot as D
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(16, 16))
    kw = dict(in_T=2, dset_metadata=md, patch_size=4, n_blocks=2, embed_dim=32, depth=1, modes=4)
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.DPOT(**dict(kw, dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16, 16), n_spatial_dims=3)))
    with pytest.raises(NotImplementedError, match="act = 'relu'"):
        tante_amd.DPOT(**kw, act="relu")
    with pytest.raises(NotImplementedError, match="mixing_type = 'attn'"):
        tante_amd.DPOT(**kw, mixing_type="attn")
    with pytest.raises(NotImplementedError, match="act = 'tanh'"):
        D.Block(width=32, n_blocks=2, act="tanh")
    with pytest.raises(NotImplementedError, match="mixing_type"):
        D.Block(width=32, n_blocks=2, mixing_type="fno")
    with pytest.raises(NotImplementedError, match="hidden_size_factor = 2"):
        D.AFNO2D(width=32, num_blocks=2, hidden_size_factor=2)
    with pytest.raises(ValueError, match="compute"):
        tante_amd.DPOT(**kw).set_compute("fp16")
    with pytest.raises(ValueError, match="time_agg"):
        tante_amd.DPOT(**kw, time_agg="sum")
    m = tante_amd.DPOT(**kw).eval()
    assert "NEVER evaluated" in D.__doc__ and "cls_head" in D.__doc__
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(1, 2, 1, 16, 16))


def test_entry_points_are_declared_bound_and_exported():
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "dpot_mixer.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert declared == set(_lib.SIGNATURES)
    assert L.tante_abi_version() == _lib.ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "tante_hip.h")).read()
    assert "dpot.py:47-102" in hdr and "dpot.py:138, 147" in hdr


def test_supported_predicates_agree_with_their_python_mirrors():
    from tante_amd import _lib
    from tante_amd import dpot as D
    L = _lib.lib()
    n_yes = 0
    for B in (0, 1, 4, 65535, 65536):
        for H in (0, 1, 5, 64, 65):
            for W in (1, 12, 64, 65):
                for C, bs in ((64, 32), (1536, 384), (1024, 512), (1026, 513), (40, 20), (48, 32), (32, 0), (0, 8), (7, 7)):
                    for modes, hf in ((1, 1), (16, 1), (100, 1), (0, 1), (4, 2)):
                        got = bool(L.tante_dpot_filter_supported(B, H, W, C, bs, modes, hf))
                        assert got == D.filter_supported_py(B, H, W, C, bs, modes, hf), (B, H, W, C, bs, modes, hf)
                        n_yes += got
    assert n_yes > 200
    n_yes = 0
    for B in (0, 1, 3, 2 ** 28, 2 ** 40):
        for HW in (0, 1, 35, 4096, 4097):
            for C, G in ((64, 8), (48, 8), (1536, 8), (7, 7), (7, 1), (20, 8), (0, 8), (8, 0), (2 ** 24 + 8, 8)):
                got = bool(L.tante_groupnorm_supported(B, HW, C, G))
                assert got == D.groupnorm_supported_py(B, HW, C, G), (B, HW, C, G)
                n_yes += got
    assert n_yes > 40
    assert L.tante_dpot_filter_supported(1, 8, 8, 1536, 384, 16, 1) == 1 and L.tante_groupnorm_supported(1, 64, 1536, 8) == 1


def test_every_refusal_has_its_code_and_message():
    """Host-only argument checks: the refusal names its entry and its reason and launches nothing."""
    from tante_amd import _lib
    L = _lib.lib()

    def filt(B=1, H=8, W=8, C=64, bs=32, modes=4, hf=1):
        return L.tante_dpot_filter(None, None, B, H, W, C, bs, modes, hf, None, None, None, None, None, None, None, 0, None)
    for kw, why in ((dict(H=65), b"token grid outside 1..64"), (dict(W=0), b"token grid outside 1..64"), (dict(C=1026, bs=513), b"block size outside 1..512"),
                    (dict(C=48), b"whole number of blocks"), (dict(modes=0), b"modes must be at least 1"), (dict(hf=2), b"hidden_size_factor other than 1"),
                    (dict(B=65536), b"more than 65535 samples")):
        assert filt(**kw) == -2, kw
        err = L.tante_last_error()
        assert err.startswith(b"tante_dpot_filter:") and why in err, (kw, err)
    assert filt() == -1 and b"tante_dpot_filter: null" in L.tante_last_error()
    assert L.tante_dpot_twiddle_floats(65, 8, 4) == -1 and L.tante_dpot_twiddle_floats(8, 8, 0) == -1
    assert L.tante_dpot_filter_workspace_bytes(1, 65, 8, 64, 32, 4) == -1
    # P / Z (B, k2, H, 2, C) + two (nb, B k1 k2, 2, bsP) block buffers, floats
    assert L.tante_dpot_filter_workspace_bytes(2, 8, 12, 40, 20, 3) == 4 * (2 * 2 * 3 * 8 * 40 + 2 * (2 * (2 * 3 * 3) * 2 * 32))

    def gn(B=1, HW=16, C=64, G=8, dt=0):
        return L.tante_groupnorm(None, B, HW, C, G, 1e-5, None, None, None, dt, None, 0, None)
    for kw, why in ((dict(HW=4097), b"tokens per sample outside 1..4096"), (dict(HW=0), b"tokens per sample outside 1..4096"),
                    (dict(C=20), b"whole number of groups"), (dict(G=0), b"whole number of groups"), (dict(B=2 ** 40), b"(sample, group) pairs")):
        assert gn(**kw) == -2, kw
        err = L.tante_last_error()
        assert err.startswith(b"tante_groupnorm:") and why in err, (kw, err)
    assert gn(dt=2) == -1 and b"tante_groupnorm: output dtype" in L.tante_last_error()
    assert gn() == -1 and b"tante_groupnorm: null" in L.tante_last_error()
    assert L.tante_groupnorm_workspace_bytes(1, 4097, 64, 8) == -1
    assert L.tante_groupnorm_workspace_bytes(2, 64, 1536, 8) == 4 * 2 * 2 * 8 * 3      # 64 rows in slabs of 22: 3 per (sample, group)
