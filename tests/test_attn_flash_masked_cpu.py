"""CPU: the masked flash attention entry points on the C ABI and the masked routing predicate of tante_amd/attn_flash.py."""
import os
import re

import pytest

from conftest import ROOT

ENTRIES = ("tante_attention_flash_masked", "tante_attention_flash_masked_bwd")


def test_masked_flash_entry_points_are_declared_bound_and_exported():
    from tante_amd import _lib
    from tante_amd.build import build
    build()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tante_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tante_[a-z_0-9]+)\s*\(", txt))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert declared == set(_lib.SIGNATURES)
    # the arguments of the unmasked pair with (Bp, L) for the descriptor, plus (attn_mask, mask_bstride, key_padding_mask)
    for name in ENTRIES:
        plain, _ = _lib.SIGNATURES[name.replace("_masked", "")]
        masked, res = _lib.SIGNATURES[name]
        assert len(masked) == len(plain) + 4 and res is _lib.SIGNATURES[name.replace("_masked", "")][1], name
    # additions only: the number the suite pins did not move
    assert _lib.ABI_VERSION == 14 and L.tante_abi_version() == 14


def test_masked_entry_points_refuse_bad_arguments_without_a_launch():
    """Host-side checks only (every call returns before a launch): shapes, the mask stride, the head dim by flash_refusal's message."""
    from tante_amd import _lib
    L = _lib.lib()
    fwd, bwd = L.tante_attention_flash_masked, L.tante_attention_flash_masked_bwd
    assert fwd(None, None, None, _lib.F32, 64, 2, 2, 200, 0, None, 0, None, 0.0, 0, None) == -1                 # null qkv / o
    assert fwd(16, 16, None, _lib.F32, 64, 2, 0, 200, 0, None, 0, None, 0.0, 0, None) == -1                     # Bp = 0
    assert fwd(16, 16, None, _lib.F32, 64, 2, 2, 200, 0, 16, 7, None, 0.0, 0, None) == -1                       # stride neither 0 nor L L
    assert fwd(16, 16, None, _lib.F32, 64, 2, 2, 200, 0, 8, 0, None, 0.0, 0, None) == -1                        # attn_mask alignment
    assert fwd(16, 16, None, _lib.F32, 48, 4, 2, 200, 0, 16, 0, None, 0.0, 0, None) == -2                       # head dim 12
    assert "tante_attention_flash_masked: head dim unsupported (supported: 32)" in L.tante_last_error().decode()
    assert fwd(16, 16, None, _lib.F32, 64, 2, 2, 200, 0, 16, 0, None, 1.0, 0, None) == -1                       # p = 1
    assert bwd(16, 16, 16, None, 16, _lib.F32, 64, 2, 2, 200, 0, 16, 0, None, 0.0, 0, None) == -1               # the backward needs stats
    assert bwd(16, 16, 16, 16, 16, 2, 64, 2, 2, 200, 0, 16, 0, None, 0.0, 0, None) == -2                        # dtype


@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("ok", [True, False])
def test_masked_route(opt, ok):
    """p > 0: only the flash kernels have masks with dropout, whatever the shape; p = 0: the flash kernels only under the option, for a
    supported shape past 128 tokens; everything else keeps tante_attention_masked(_bwd)."""
    from tante_amd import attn_flash as FA
    for Lq in (1, 128, 129, 320, 4096):
        assert FA.masked_route(Lq, 0.1, ok, opt) == FA.MASKED_FLASH
        want = FA.MASKED_FLASH if (opt and ok and Lq > 128) else FA.MASKED_LANES
        assert FA.masked_route(Lq, 0.0, ok, opt) == want, (Lq, ok, opt)
    assert FA.masked_route(320, 0.0, True) == FA.MASKED_LANES      # the option's default is off
    assert FA.ATTN_FLASH == 0


def test_unmasked_routes_are_what_they_were():
    """forward_route and backward_route keep their signatures and their tables (restated here in full, not read from the code)."""
    import inspect
    from tante_amd import attn_flash as FA
    assert list(inspect.signature(FA.forward_route).parameters) == ["Lq", "p", "ok", "flash_opt"]
    assert list(inspect.signature(FA.backward_route).parameters) == ["Lq", "p", "dense", "ok", "flash_opt"]
    for opt in (0, 1):
        for ok in (True, False):
            for Lq in (1, 128, 129, 256, 257, 320, 4096):
                assert FA.forward_route(Lq, 0.1, ok, opt) == ("flash" if Lq > 256 else "attention_dropout")
                assert FA.forward_route(Lq, 0.0, ok, opt) == ("flash" if (opt and ok and Lq > 256) else "attention")
                for dense in (True, False):
                    for p in (0.0, 0.1):
                        if Lq <= 128:
                            want = "attention_bwd"
                        elif p > 0 or not dense:
                            want = "flash_bwd"
                        else:
                            want = "flash_bwd" if (opt and ok) else "attention_masked_bwd"
                        assert FA.backward_route(Lq, p, dense, ok, opt) == want, (Lq, p, dense, ok, opt)


def test_masked_operator_is_public_and_the_train_guard_stands():
    """MaskedFlashAttentionFn is exported next to MaskedAttentionFn; block_train still refuses masks with dropout in train() mode (the
    operator exists, the guard is lifted separately: DESIGN.md section 7)."""
    import inspect
    from tante_amd import autograd as A, train_forward as TF
    assert list(inspect.signature(A.MaskedFlashAttentionFn.forward).parameters)[1:] == [
        "qkv", "Cc", "n_head", "Bp", "Lq", "causal", "attn_mask", "key_padding_mask", "p", "seed"]
    assert "NotImplementedError" in inspect.getsource(TF.block_train)
