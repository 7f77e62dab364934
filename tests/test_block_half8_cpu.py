"""No GPU: the rule of the 8-wave half-size launcher (tante_fs_half8_launch, block_sliced.hip) restated in tests/block_half8_ref.py, held
against the source text and against the restated 4-wave dispatch: it serves exactly the plain launches that reach the 4-wave 2-tile
instances, with their geometry, and nothing else; the option is forwarded and documented; the cases of the GPU test are what they say."""
import os
import re

import pytest

import block_forms_ref as R
import block_half8_ref as H
from conftest import ROOT

CSRC = os.path.join(ROOT, "tante_amd", "csrc")
FS_SRC = open(os.path.join(CSRC, "block_sliced.hip")).read()
TS_SRC = open(os.path.join(CSRC, "block_fused.hip")).read()


def _launcher_text():
    i, j = FS_SRC.index("int tante_fs_half8_launch("), FS_SRC.index("int tante_fs_launch(")
    assert i < j, "the launcher is defined above tante_fs_launch"
    return FS_SRC[i:j]


def test_launcher_text_is_the_restated_rule():
    t = _launcher_text()
    assert not re.findall(r"case \d{3}:", t)
    for text in ("if (sq.nseq >= (1 << 23)) return -2;",
                 "if (sq.nseq < 1 || L < 1 || 32 % L != 0 || (L == 32 && causal) || fs_waves(L) != 4) return 0;",
                 'if (!tante_opt("TANTE_FS_HALF", 1) || !tante_opt("TANTE_FS_HALF8", 1)) return 0;',
                 "auto nwg_at = [&](int ntt) { return ((long)sq.nseq + 16 * ntt / L - 1) / (16 * ntt / L); };",
                 "auto rounds = [&](int ntt) { return ((nwg_at(ntt) + 511) / 512) * ntt; };",
                 "const int ntt_full = (L != 32 && rounds(3) < rounds(4)) ? 3 : 4;", "if (nwg_at(ntt_full) * 4 > 512) return 0;",
                 "A.spw = 32 / L;", "A.skew = 0;", "A.tprop = nullptr;", "A.out = nullptr;", "const int nwg = (int)nwg_at(2);",
                 "if (L == 32) fs_launch_half8<2>(A, nwg, s);", "else fs_launch_half8<1>(A, nwg, s);"):
        assert text in t, text
    # the one instantiation family behind it: 2 tiles, 8 waves, inference, pair-chained statistics; 512 threads
    assert FS_SRC.count("block_fs_kernel<TPS, 2, 8, false, 1, false, false, true>") == 2
    assert "dim3(nwg), dim3(512), LDS, s, A);" in FS_SRC
    assert "constexpr int LDS = 2 * 16 * 2 * FS_ROW + 16 * 2 * 8 * 8 + FS_BIAS_FLOATS * 4 + 4 * 2 * 64 * 8;" in FS_SRC
    assert 'static_assert(!PAIR || (NW == 8 && NTT == 2 && G == 1 && !TRAIN && !TPROP && !LASTQ)' in FS_SRC


def test_only_the_plain_entry_asks_the_launcher():
    assert TS_SRC.count("tante_fs_half8_launch(") == 1
    i = TS_SRC.index('extern "C" int tante_block_fused(float* x')
    body = TS_SRC[i:TS_SRC.index('extern "C" int tante_block_fused_train(')]
    a, b = body.index("tante_fs_half8_launch("), body.index("tante_fs_launch(")
    assert a < b
    assert "if (half8 < 0 || (half8 == 0 && tante_fs_launch(x, st + block_ts_stream_bytes(C, hidden), *seq, causal, eps, s) != 0))" in body
    assert body.index("if (use_fs(C, n_head, hidden, seq->L, causal)) {") < a


def test_option_is_forwarded_and_documented():
    lib_py = open(os.path.join(ROOT, "tante_amd", "_lib.py")).read()
    m = re.search(r"LIB_OPTIONS = \((.*?)\)\n", lib_py, re.S)
    assert '"TANTE_FS_HALF8"' in m.group(1)
    assert '"TANTE_FS_HALF8"' in open(os.path.join(ROOT, "include", "tante_hip.h")).read()
    assert FS_SRC.count('tante_opt("TANTE_FS_HALF8", 1)') == 1
    assert H.OPTION_DEFAULTS["TANTE_FS_HALF8"] == 1 and "TANTE_FS_HALF8" not in R.OPTION_DEFAULTS


NSEQS = sorted(set(list(range(1, 40)) + [n + d for n in (64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288)
                                         for d in (-1, 0, 1)]))
OPTS = [{}, {"TANTE_FS_HALF": 0}, {"TANTE_FS_WAVES": 8}, {"TANTE_FS_HALF8": 0}, {"TANTE_FS_GROUPS": 2}, {"TANTE_FS_SKEW": 3}]


@pytest.mark.parametrize("opts", OPTS, ids=[str(sorted(o.items())) for o in OPTS])
def test_rule_is_the_half_size_launches_of_the_4_wave_dispatch(opts):
    """Covered <=> TANTE_FS_HALF8 on and the restated tante_fs_launch reaches a 4-wave 2-tile instance; same sequences per workgroup and
    workgroup count, at most one workgroup per CU, no entry skew."""
    base = {k: v for k, v in opts.items() if k in R.OPTION_DEFAULTS}
    covered = 0
    for L in range(1, 129):
        for causal in (False, True):
            for nseq in NSEQS:
                r = R.fs_route(L, nseq, causal, options=base)
                got = H.half8_rule(L, nseq, causal, opts)
                want = r.name in H.HALF4_ROUTES and H._opt(opts, "TANTE_FS_HALF8") != 0
                assert (got is not None) == want, (L, nseq, causal, opts, r, got)
                if got is not None:
                    covered += 1
                    assert got == (int(r.name[6]), r.spw, r.nwg) and r.nwg <= R.CUS and r.skew == 0 and got[1] * L == 32
    assert (covered > 0) == (opts in ({}, {"TANTE_FS_GROUPS": 2}, {"TANTE_FS_SKEW": 3}))


def test_rule_at_its_thresholds():
    f = H.half8_rule
    assert f(32, 256, False) == (2, 1, 256) and f(32, 257, False) is None and f(32, 5, True) is None
    assert f(16, 384, False) == (1, 2, 192) and f(16, 385, False) is None
    assert f(4, 1536, True) == (1, 8, 192) and f(4, 1537, True) is None
    assert f(1, 3, False) == (1, 32, 1) and f(3, 8, False) is None and f(64, 2, False) is None
    with pytest.raises(R.Refused):
        f(4, 1 << 23, False)
    # the launches the issue names: cfg2 (H = W = 32) at B = 8 on the slot-(T - 1) sub-grid, and every H / W launch at B = 1 and B = 2
    assert f(32, 8 * 32, False) == (2, 1, 256) and f(32, 1 * 4 * 32, False) == (2, 1, 128) and f(32, 2 * 4 * 32, False) == (2, 1, 256)
    assert f(32, 8 * 4 * 32, False) is None


def test_cases_of_the_gpu_test():
    ids = [c.id for c in H.COVERED + H.NOT_COVERED]
    assert len(set(ids)) == len(ids)
    for c in H.COVERED:
        assert R.route(c, {}) == c.route and c.route in H.HALF4_ROUTES and H.half8_rule(c.L, c.nseq, c.causal) is not None, c.id
        assert not c.tprop and not c.last
    for c in H.NOT_COVERED:
        assert R.route(c, {}) == c.route and c.route not in H.HALF4_ROUTES and H.half8_rule(c.L, c.nseq, c.causal) is None, c.id
    shapes = {(c.L, c.nseq, c.causal) for c in H.COVERED if c.layout is None}
    assert {(32, 1, False), (32, 5, False), (16, 3, False), (1, 3, False)} <= shapes
    assert {(L, n, k) for L in (8, 4) for n in (5, 9) for k in (False, True)} <= shapes
    sub = {c.id: c for c in H.COVERED + H.NOT_COVERED if c.layout is not None}
    assert all(c.row0 > 0 for c in sub.values())
    assert (sub["half8-subH-2x4x32x3"].L, sub["half8-subH-2x4x32x3"].nseq) == (32, 6) and sub["half8-subW-2x4x32x3"].L == 3
    assert (sub["half8-subW-2x4x3x32"].L, sub["half8-subW-2x4x3x32"].nseq) == (32, 6)
