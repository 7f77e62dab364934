"""The route table of tante_cross_attention (host code, no GPU): which kernel a (dtype, head dim, key count) takes.

0 = the exact lane-per-query VALU kernel, 1 = matrix pipe with K and V resident in LDS (K + V of the keys rounded up to 128 fit 128 KiB:
512 keys at D = 64, 1024 at D = 32), 2 = matrix pipe with K and V streamed through the LDS ring.  The launcher decides by this same
function (csrc/operators.hip), and kernels.cross_attention_route is its Python mirror.
"""
import pytest
import torch

from tante_amd import _lib as L, kernels as K

NAMES = {0: "valu", 1: "resident", 2: "stream"}
TORCH = {L.BF16: torch.bfloat16, L.F32: torch.float32}
TABLE = [((L.BF16, 64, 1), 1), ((L.BF16, 64, 512), 1), ((L.BF16, 64, 513), 2), ((L.BF16, 32, 1024), 1), ((L.BF16, 32, 1025), 2),
         ((L.F32, 64, 100), 0), ((L.BF16, 16, 100), 0)]


def route(dtype, D, Lk):
    return L.lib().tante_cross_attention_route(dtype, D, Lk)


class option:
    """Set a library option for a block and restore what it was."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = L.get_option(self.name, 0)
        L.set_option(self.name, self.value)

    def __exit__(self, *exc):
        L.set_option(self.name, self.old)


@pytest.mark.parametrize("call,want", TABLE)
def test_default_route(call, want):
    assert route(*call) == want


def test_python_mirror_returns_the_matching_strings():
    for (dtype, D, Lk), want in TABLE:
        assert K.cross_attention_route(TORCH[dtype], D, Lk) == NAMES[want]


def test_valu_option_forces_route_0_everywhere():
    with option("TANTE_XATTN_VALU", 1):
        for call, _ in TABLE:
            assert route(*call) == 0
            assert K.cross_attention_route(TORCH[call[0]], *call[1:]) == "valu"
    assert route(L.BF16, 64, 100) == 1


def test_stream_option_forces_route_2_where_the_matrix_pipe_applies():
    with option("TANTE_XATTN_STREAM", 1):
        assert route(L.BF16, 64, 100) == 2
        assert route(L.BF16, 32, 100) == 2
        assert route(L.F32, 64, 100) == 0
        assert route(L.BF16, 16, 100) == 0
        assert K.cross_attention_route(torch.bfloat16, 64, 100) == "stream"
        with option("TANTE_XATTN_VALU", 1):      # the VALU switch wins over the stream switch
            assert route(L.BF16, 64, 100) == 0
    assert route(L.BF16, 64, 100) == 1 and route(L.BF16, 32, 100) == 1


def test_the_new_entry_did_not_bump_the_abi():
    assert L.lib().tante_abi_version() == 14 == L.ABI_VERSION
    assert "TANTE_XATTN_STREAM" in L.LIB_OPTIONS
