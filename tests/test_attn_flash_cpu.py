"""CPU: the flash attention entry points on the C ABI and the routing predicate of tante_amd/attn_flash.py."""
import os
import re

import pytest

from conftest import ROOT

ENTRIES = ("tante_attention_flash_stats_floats", "tante_attention_flash_supported", "tante_attention_flash", "tante_attention_flash_bwd")


def test_flash_entry_points_are_declared_bound_and_exported():
    from tante_amd import _lib
    from tante_amd.build import build
    build()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert declared == set(_lib.SIGNATURES)
    assert "attn_flash.hip" in __import__("tante_amd.build", fromlist=["SOURCES"]).SOURCES


def test_abi_version_is_14():
    from tante_amd import _lib
    assert _lib.ABI_VERSION == 14
    assert _lib.lib().tante_abi_version() == 14


def test_supported_mirror_matches_the_library():
    """Host-only calls: tante_attention_flash_supported launches nothing."""
    from tante_amd import _lib, attn_flash as FA
    L = _lib.lib()
    for dtype in (_lib.F32, _lib.BF16, 2):
        for C_, nh in ((256, 8), (160, 5), (48, 4), (64, 4), (512, 8), (64, 0), (100, 3)):
            for Lq in (0, 1, 129, 4096):
                assert bool(L.tante_attention_flash_supported(dtype, C_, nh, Lq)) == FA.supported(dtype, C_, nh, Lq), (dtype, C_, nh, Lq)
    s = _lib.Seq()
    s.nseq, s.L, s.n_s0, s.S1, s.S0, s.n_l0, s.P1, s.P0 = 3, 320, 1, 320, 0, 320, 0, 1
    import ctypes
    assert L.tante_attention_flash_stats_floats(8, ctypes.byref(s)) == 3 * 8 * 320 * 2


@pytest.mark.parametrize("opt", [0, 1])
def test_routing_table(opt):
    """Which kernel takes which (L, p, dense, supported) call: the routing table of DESIGN.md 4.4.  Option 0 routes only what the
    older kernels refuse; option 1 adds the supported calls that work without it."""
    from tante_amd import attn_flash as FA
    for ok in (True, False):
        flash_if_opt = bool(opt and ok)
        # forward
        for Lq in (1, 64, 128, 200, 256):
            assert FA.forward_route(Lq, 0.1, ok, opt) == FA.FWD_DROPOUT
            assert FA.forward_route(Lq, 0.0, ok, opt) == FA.FWD_PLAIN
        for Lq in (257, 320, 1024, 4096):
            assert FA.forward_route(Lq, 0.1, ok, opt) == FA.FWD_FLASH                 # refused before: flash whatever the shape
            assert FA.forward_route(Lq, 0.0, ok, opt) == (FA.FWD_FLASH if flash_if_opt else FA.FWD_PLAIN)
        # backward
        for Lq in (1, 64, 128):
            for p in (0.0, 0.1):
                for dense in (True, False):
                    assert FA.backward_route(Lq, p, dense, ok, opt) == FA.BWD_MFMA
        for Lq in (129, 200, 256, 257, 1024, 4096):
            for dense in (True, False):
                assert FA.backward_route(Lq, 0.1, dense, ok, opt) == FA.BWD_FLASH       # refused before
            assert FA.backward_route(Lq, 0.0, False, ok, opt) == FA.BWD_FLASH           # refused before (strided)
            assert FA.backward_route(Lq, 0.0, True, ok, opt) == (FA.BWD_FLASH if flash_if_opt else FA.BWD_MASKED)


def test_option_is_registered_and_off_by_default():
    import tante_amd
    from tante_amd import attn_flash as FA, kernels as K, options as O
    assert "TANTE_ATTN_FLASH" in O.host_options()
    assert tante_amd.get_option("TANTE_ATTN_FLASH") == 0 or os.environ.get("TANTE_ATTN_FLASH")
    tante_amd.set_option("TANTE_ATTN_FLASH", 1)
    try:
        assert FA.ATTN_FLASH == 1
    finally:
        tante_amd.set_option("TANTE_ATTN_FLASH", 0)
    assert FA.ATTN_FLASH == 0
    assert FA.seq_is_dense(K.dense_seq(4, 300)) and FA.seq_is_dense(K.make_seq("L", 2, 4, 16, 16)) and FA.seq_is_dense(K.make_seq("A", 2, 4, 8, 8))
    assert not FA.seq_is_dense(K.make_seq("X", 2, 4, 8, 64)) and not FA.seq_is_dense(K.make_seq("Y", 2, 4, 64, 8))
