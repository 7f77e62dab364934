"""CPU: the AFNO baseline's host side -- the float64 restatement against the reference's fixtures, the twiddle / weight packs against the
restatement, the module surface, the config alias and the C-ABI surface (host-only calls: there is no GPU here)."""
import os
import re

import numpy as np
import pytest
import torch

import afno_ref as R
from conftest import ROOT, load_golden, load_golden_raw, max_rel, rel_err

FILTERS = ["g18_afno_filter_8x8", "g18_afno_filter_24x8", "g18_afno_filter_4x16", "g18_afno_filter_5x12", "g18_afno_filter_16x16_c256"]
MODELS = {"g18_afno_model_32x32_p4": ((32, 32), 4), "g18_afno_model_16x48_p2": ((16, 48), 2)}
ENTRY_POINTS = ("tante_afno_filter_supported", "tante_afno_twiddle_floats", "tante_afno_filter_workspace_bytes", "tante_afno_filter")


def model_golden(name):
    """-> (tensors, state dict, key list) of a whole-model fixture (its key list is a string array, which load_golden cannot take)."""
    raw = load_golden_raw(name)
    g = {k: torch.from_numpy(v) for k, v in raw.items() if k != "keys"}
    return g, {k[2:]: v for k, v in g.items() if k.startswith("w.")}, [str(k) for k in raw["keys"]]


@pytest.mark.parametrize("name", FILTERS)
def test_restatement_reproduces_the_reference_filter(name):
    """The float64 DFT-matrix restatement against the reference's fp32 output: <= 1e-6 relative (the reference's own rounding is 2.5e-7)."""
    g = load_golden(name)
    y = R.afno_filter(g["x"], g["w1"], g["w2"], float(g["lam"]))
    assert y.shape == g["y"].shape
    assert rel_err(y, g["y"]) <= 1e-6 and max_rel(y, g["y"]) <= 1e-6, (rel_err(y, g["y"]), max_rel(y, g["y"]))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_restatement_reproduces_the_reference_model(name):
    g, sd, _ = model_golden(name)
    y = R.model(g["x"], sd, MODELS[name][1])
    assert y.shape == g["y"].shape
    assert rel_err(y, g["y"]) <= 1e-6 and max_rel(y, g["y"]) <= 2e-6, (rel_err(y, g["y"]), max_rel(y, g["y"]))


@pytest.mark.parametrize("name", FILTERS)
def test_fixture_filters_are_neither_dead_nor_transparent(name):
    """A default-init filter is identically zero: the fixtures hold scaled weights, and the thresholded share must say so."""
    g = load_golden(name)
    share = float(g["zeroed_share"])
    assert 0.2 <= share <= 0.8, share
    assert abs(R.zeroed_share(g["x"], g["w1"], g["w2"], float(g["lam"])) - share) < 1e-3
    assert float(g["y"].abs().max()) > 1e-2
    for gm in MODELS:
        assert all(0.2 <= float(s) <= 0.8 for s in load_golden_raw(gm)["zeroed_share"])


@pytest.mark.parametrize("H,W", [(8, 8), (24, 8), (4, 16), (5, 12), (7, 9), (64, 33), (1, 1), (32, 32)])
def test_twiddle_tables_equal_the_restatement_matrices(H, W):
    from tante_amd import afno as A
    Lc, Kc = A.kept_modes(H, W)
    assert (Lc, Kc) == (min(H, W), min(H // 2 + 1, W // 2 + 1))
    k = torch.arange(Kc)
    ck = torch.where((k == 0) | ((W % 2 == 0) & (k == W // 2)), 1.0, 2.0).to(torch.float64)
    want = [R.dft_matrix(W, -1)[:Lc], R.dft_matrix(H, -1)[:Kc], R.dft_matrix(W, +1)[:, :Kc] * ck[None, :], R.dft_matrix(H, +1)[:, :Lc]]
    got = A.twiddle_tables(H, W)
    for t, w in zip(got, want):
        assert t.shape == tuple(w.shape)
        assert np.abs(t - w.numpy()).max() < 1e-14
    # the packed buffer: per table a real then an imaginary plane, rows padded to 16 and columns to 4 with zeros, float32
    buf = A.pack_twiddles(H, W)
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
    assert int(_lib.lib().tante_afno_twiddle_floats(H, W)) == buf.size


@pytest.mark.parametrize("bs", [32, 8, 20, 64])
def test_realified_weight_equals_the_complex_block_product(bs):
    from tante_amd import afno as A
    gen = torch.Generator().manual_seed(bs)
    w = torch.randn(3, bs, bs, 2, generator=gen)
    x = torch.complex(torch.randn(5, 3 * bs, generator=gen, dtype=torch.float64), torch.randn(5, 3 * bs, generator=gen, dtype=torch.float64))
    want = R.block_linear(x, w).reshape(5, 3, bs)
    m = A.pack_block_weight(w).double()
    bp = -(-bs // 16) * 16
    assert tuple(m.shape) == (3, 2 * bp, 2 * bp)
    ri = torch.zeros(5, 3, 2 * bp, dtype=torch.float64)
    ri[..., :bs], ri[..., bp:bp + bs] = x.real.reshape(5, 3, bs), x.imag.reshape(5, 3, bs)
    y = torch.einsum("ngi,gio->ngo", ri, m)
    assert (y[..., :bs] - want.real).abs().max() < 1e-12 and (y[..., bp:bp + bs] - want.imag).abs().max() < 1e-12
    assert not y[..., bs:bp].any() and not y[..., bp + bs:].any()


@pytest.mark.parametrize("name", FILTERS)
def test_the_three_launch_decomposition_from_the_packed_buffers_reproduces_the_fixture(name):
    """What tante_afno_filter evaluates -- T1 along w, T2 along h, the real-ified MLP, T3 along k, Re(T4 along l), each read back from the
    PACKED host buffers -- in float64: ties the pack layout and the kept-mode bookkeeping (crop / pad, swapped sizes) to the reference."""
    from tante_amd import afno as A
    g = load_golden(name)
    x, lam = g["x"].double(), float(g["lam"])
    B, H, W, C = x.shape
    bs = g["w1"].shape[1]
    Lc, Kc = A.kept_modes(H, W)
    buf, T, off = A.pack_twiddles(H, W).astype(np.float64), [], 0
    for M, K in [(Lc, W), (Kc, H), (W, Kc), (H, Lc)]:
        Mp, Kp = -(-M // 16) * 16, -(-K // 4) * 4
        re, im = buf[off: off + Mp * Kp].reshape(Mp, Kp), buf[off + Mp * Kp: off + 2 * Mp * Kp].reshape(Mp, Kp)
        T.append(torch.from_numpy(re[:M, :K] + 1j * im[:M, :K]))
        off += 2 * Mp * Kp
    P = torch.einsum("lw,bhwc->blhc", T[0], x.to(torch.complex128))
    X = torch.einsum("kh,blhc->blkc", T[1], P).reshape(B, Lc, Kc, C // bs, bs)
    bp = -(-bs // 16) * 16
    ri = torch.zeros(B, Lc, Kc, C // bs, 2 * bp, dtype=torch.float64)
    ri[..., :bs], ri[..., bp:bp + bs] = X.real, X.imag
    U = R.gelu(torch.einsum("...gi,gio->...go", ri, A.pack_block_weight(g["w1"]).double()))
    Y = R.softshrink(torch.einsum("...gi,gio->...go", U, A.pack_block_weight(g["w2"]).double()), lam)
    Yc = torch.complex(Y[..., :bs], Y[..., bp:bp + bs]).reshape(B, Lc, Kc, C)
    out = torch.einsum("hl,bwlc->bhwc", T[3], torch.einsum("wk,blkc->bwlc", T[2], Yc)).real        # (B, H, W, C): already swapped back
    want = g["y"].transpose(1, 2)
    assert rel_err(out, want) <= 1e-6 and max_rel(out, want) <= 1e-6, (rel_err(out, want), max_rel(out, want))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_matches_the_reference_layout(name):
    import tante_amd
    g, sd, keys = model_golden(name)
    res, patch = MODELS[name]
    m = tante_amd.AFNO(in_T=3, dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=res), hidden_dim=64, n_blocks=2,
                       cmlp_diagonal_blocks=2, patch_size=patch)
    mine = m.state_dict()
    assert list(mine) == keys
    for k in keys:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    assert tuple(mine["blocks.0.filter.cmlp.0.weight"].shape) == (2, 32, 32, 2)
    assert tuple(mine["pos_embed"].shape) == (1, res[0] // patch, res[1] // patch, 64)
    assert m.blocks[0].norm1.eps == 1e-6 and m.blocks[1].norm2.eps == 1e-6
    assert (m.dim_in, m.dim_out, m.n_blocks, m.cmlp_diagonal_blocks, list(m.inner_size)) == (6, 2, 2, 2, [res[0] // patch, res[1] // patch])
    m.load_state_dict(sd, strict=True)
    # default init: zero biases, unit LayerNorm, truncated-normal fc weights of scale 0.02
    fresh = tante_amd.AFNO(in_T=3, dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=res), hidden_dim=64, n_blocks=1,
                           cmlp_diagonal_blocks=2, patch_size=patch)
    b0 = fresh.blocks[0]
    assert not b0.mlp.fc1.bias.any() and not b0.mlp.fc2.bias.any() and bool((b0.norm1.weight == 1).all()) and not b0.norm2.bias.any()
    # (the median, not the standard deviation: trunc_normal_ with its default bounds of +-2 lets the rare uniform draw at the very end
    # of its range through as a weight of +-2, the reference's initialiser included, and one such weight moves the standard deviation)
    assert 0.012 < float(b0.mlp.fc1.weight.detach().abs().median()) < 0.015        # 0.6745 sigma, sigma = 0.02


def test_config_alias_builds_the_reference_model_block():
    import tante_amd
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "afno_am.yaml"))
    assert cfg["model"] == {"_target_": "models.AFNO", "in_T": 4, "hidden_dim": 256, "n_blocks": 8}
    wl = cfg["workload"]
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md)
    assert isinstance(m, tante_amd.AFNO) and type(m).__module__ == "tante_amd.afno"
    assert len(m.blocks) == 8 and m.hidden_dim == 256 and list(m.inner_size) == [32, 32] and m.dim_in == 44
    assert tuple(m.blocks[0].filter.cmlp[0].weight.shape) == (8, 32, 32, 2)
    from tante_amd import config
    assert config._TARGET_ALIASES["models.afno.AFNO"] == config._TARGET_ALIASES["models.AFNO"] == "tante_amd.afno.AFNO"


def test_out_of_scope_constructions_say_so():
    import tante_amd
    md3 = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16, 16), n_spatial_dims=3)
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.AFNO(in_T=2, dset_metadata=md3, hidden_dim=32, n_blocks=1, patch_size=4)
    with pytest.raises(ValueError, match="compute"):
        tante_amd.AFNO(in_T=2, dset_metadata=tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(16, 16)), hidden_dim=32, n_blocks=1,
                       patch_size=4).set_compute("fp16")


def test_entry_points_are_declared_bound_and_exported():
    from tante_amd import _lib
    from tante_amd.build import SOURCES, build
    build()
    L = _lib.lib()
    assert "afno_filter.hip" in SOURCES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert declared == set(_lib.SIGNATURES)
    assert L.tante_abi_version() == _lib.ABI_VERSION == 14


def test_supported_predicate_agrees_with_its_python_mirror():
    from tante_amd import _lib
    from tante_amd import afno as A
    L = _lib.lib()
    n_yes = 0
    for B in (0, 1, 4, 65535, 65536):
        for H in (0, 1, 5, 32, 64, 65):
            for W in (1, 12, 64, 65, 128):
                for C, bs in ((64, 32), (256, 32), (64, 64), (128, 128), (40, 8), (48, 32), (32, 0), (0, 8)):
                    got = bool(L.tante_afno_filter_supported(B, H, W, C, bs))
                    assert got == A.filter_supported_py(B, H, W, C, bs), (B, H, W, C, bs)
                    n_yes += got
    assert n_yes > 50
    assert L.tante_afno_filter_supported(1, 32, 32, 256, 32) == 1 and L.tante_afno_filter_supported(1, 65, 32, 256, 32) == 0
    # host-only argument checks: the refusal names its reason and launches nothing
    assert L.tante_afno_filter(None, None, 1, 65, 32, 256, 32, None, None, None, 0.01, None, None, 0, None) == -2
    assert b"token grid" in L.tante_last_error()
    assert L.tante_afno_filter(None, None, 1, 32, 32, 48, 32, None, None, None, 0.01, None, None, 0, None) == -2
    assert b"whole number of blocks" in L.tante_last_error()
    assert L.tante_afno_filter(None, None, 1, 32, 32, 64, 32, None, None, None, 0.01, None, None, 0, None) == -1
    assert b"null" in L.tante_last_error()
    assert L.tante_afno_twiddle_floats(65, 8) == -1
    # P (B, Lc, H, 2, C) + G (B, W, Lc, 2, C) floats
    assert L.tante_afno_filter_workspace_bytes(2, 24, 8, 64) == 4 * 2 * 2 * 8 * (24 + 8) * 64
