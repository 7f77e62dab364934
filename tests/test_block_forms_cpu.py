"""No GPU: what tests/test_hip_block_forms.py relies on is itself held here.  The float64 reference of tests/block_forms_ref.py against
oracle.tante_oracle (a contiguous block; every axis letter through attn_backbone's regrouping; the temporal propagator; the last-slot
sub-grid); the restated launch dispatch against the text of block_sliced.hip and block_fused.hip; the case list against the launch
switches (every template instance reached by the case that names it); the exact-bf16 evaluation's distance to float64 (at most half of
every bar on every case, and the per-token bar is the rule applied to that figure); and the bars against wrong results of the kinds a block
kernel can produce.

Why a per-token bar.  PLANTED below lists, for each fault planted into the exact-bf16 result of a case, whether the whole-tensor bars
test_fused_block holds (relative L2 1e-2 on y and 2e-2 on y - x; scale-relative max 2e-2 on y) would have passed it.  On the 24 592-token
launch the relative L2 bar on y passes every fault that is confined to one token or one sequence, and a dropped head or a last key left
out of one sequence's softmax pass all three; the per-token bar rejects every one of them on every case -- but for BELOW_FORMAT."""
import os
import re

import pytest
import torch

import block_forms_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "tante_amd", "csrc")
FS_SRC = open(os.path.join(CSRC, "block_sliced.hip")).read()
TS_SRC = open(os.path.join(CSRC, "block_fused.hip")).read()

FAULT_CASES = ("412-L4x37c", "412-L4x37c-tprop", "412-L4x37c-last", "412-L4x37c-tprop-last", "404-L5x13c", "422-L32x5", "Y-2x4x5x3",
               "ts16-C64h64-L4x33c", "ts32-C128h256-L32x5c", "414-L16x1537")
# fault -> (relative L2 1e-2 on y passes it, relative L2 2e-2 on y - x passes it, scale-relative max 2e-2 on y passes it) on the
# 24 592-token launch BIG; measured by test_planted_faults, which asserts this table.
BIG = "414-L16x1537"
PLANTED = {
    "drop_last_key": (True, True, True),
    "drop_head": (True, True, True),
    "row_from_next_seq": (True, False, False),
    "last_seq_unwritten": (True, False, False),
    "ln_c_minus_1": (True, True, True),
}
# A fault no bf16 bar can see.  LayerNorm statistics over C - 1 of C channels move a token's rstd by about 1 / (2 C): planted into the
# exact-bf16 result it leaves the worst token at 4.4e-3 (C = 256), 4.0e-3 (C = 128) and 1.1e-2 (C = 64) -- at or below what the format
# itself costs (EXACT_BF16_WORST_TOKEN = 5.5e-3, twice that at C = 64) and below any bar the exact-bf16 evaluation passes with the
# factor of two the rule asks for.  It stays in the list so that the figures are on record; it is asserted to be BELOW the bar.
BELOW_FORMAT = ("ln_c_minus_1",)


@pytest.fixture(scope="module")
def evaluated():
    """Per shape: inputs, float64 reference, exact-bf16 evaluation (computed once; `last` cases share their shape's inputs)."""
    out = {}
    for c in R.BLOCK_CASES:
        key = (c.shape_id, c.last)
        if key not in out:
            inp = R.make_inputs(c)
            out[key] = (inp, R.launch_ref(c, inp), R.launch_ref(c, inp, exact_bf16=True))
    return out


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,hidden,L,nseq,causal", [(64, 64, 4, 5, True), (64, 128, 32, 3, False), (256, 256, 12, 3, False),
                                                    (256, 256, 1, 7, True), (128, 128, 50, 2, True)])
def test_block_ref_is_the_oracles_transformer_block(C, hidden, L, nseq, causal):
    from oracle import tante_oracle as O
    w = {k: v.double() for k, v in R.block_weights(C, hidden, 11).items()}
    x = torch.randn(nseq, L, C, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.3
    ref = O.transformer_block(w, x, C // 32, causal)
    assert float((R.block_ref(w, x, causal) - ref).abs().max()) < 1e-10


@pytest.mark.parametrize("grid", [R.GRID_A, R.GRID_B, R.GRID_TS])
@pytest.mark.parametrize("letter", ["T", "H", "W", "L", "Y", "X", "A"])
def test_letters_are_attn_backbones_regrouping(letter, grid):
    """One block of oracle.attn_backbone (propagator weights zero, so only the block acts) against block_ref on the rows seq_tokens gives."""
    from oracle import tante_oracle as O
    B, T, H, W = grid
    C = 64
    bw = R.block_weights(C, C, 3)
    w = {f"blocks.0.{k}": v.double() for k, v in bw.items() if k != "tprop"}
    for p, n in (("vertical_propagator", H), ("horizontal_propagator", W), ("temporal_propagator", T)):
        w.update({f"{p}.0.weight": torch.zeros(n, n, dtype=torch.float64), f"{p}.0.bias": torch.zeros(n, dtype=torch.float64),
                  f"{p}.2.weight": torch.zeros(n, n, dtype=torch.float64), f"{p}.2.bias": torch.zeros(n, dtype=torch.float64)})
    x = torch.randn(B, T, H, W, C, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    ref = O.attn_backbone(w, x, letter, C // 32).reshape(-1, C)
    tok = R.seq_tokens(R.make_seq(letter, *grid))
    assert sorted(tok.reshape(-1).tolist()) == list(range(B * T * H * W))
    out = x.reshape(-1, C).clone()
    out[tok.reshape(-1)] = R.block_ref(bw, x.reshape(-1, C)[tok], letter == "T").reshape(-1, C)
    assert float((out - ref).abs().max()) < 1e-10


def test_tprop_ref_is_the_oracles_temporal_propagator():
    from oracle import tante_oracle as O
    B, T, H, W, C = 2, 4, 5, 3, 64
    bw = R.block_weights(C, C, 9)
    w1, b1, w2, b2 = R.tprop_parts(bw)
    w = {f"blocks.0.{k}": v.double() for k, v in bw.items() if k != "tprop"}
    for p, n in (("vertical_propagator", H), ("horizontal_propagator", W)):
        w.update({f"{p}.0.weight": torch.zeros(n, n, dtype=torch.float64), f"{p}.0.bias": torch.zeros(n, dtype=torch.float64),
                  f"{p}.2.weight": torch.zeros(n, n, dtype=torch.float64), f"{p}.2.bias": torch.zeros(n, dtype=torch.float64)})
    w.update({"temporal_propagator.0.weight": w1.double(), "temporal_propagator.0.bias": b1.double(),
              "temporal_propagator.2.weight": w2.double(), "temporal_propagator.2.bias": b2.double()})
    x = torch.randn(B, T, H, W, C, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    ref = O.attn_backbone(w, x, "T", C // 32).reshape(-1, C)
    tok = R.seq_tokens(R.make_seq("T", B, T, H, W))
    out = x.reshape(-1, C).clone()
    out[tok.reshape(-1)] = R.block_ref(bw, R.tprop_ref(x.reshape(-1, C)[tok], (w1, b1, w2, b2)), True).reshape(-1, C)
    assert float((out - ref).abs().max()) < 1e-10


@pytest.mark.parametrize("grid", [R.GRID_A, R.GRID_B])
@pytest.mark.parametrize("letter", ["H", "W", "L"])
def test_sub_grid_is_the_letters_sequences_of_the_last_slot(letter, grid):
    """last_slot_seq from row (T - 1) H W addresses exactly the sequences of make_seq that lie in slot T - 1, token by token."""
    B, T, H, W = grid
    full = R.seq_tokens(R.make_seq(letter, *grid))
    sub = R.seq_tokens(R.last_slot_seq(letter, *grid), (T - 1) * H * W)
    in_last = ((full // (H * W)) % T == T - 1).all(dim=1)
    assert {tuple(r) for r in full[in_last].tolist()} == {tuple(r) for r in sub.tolist()}


# ---- the dispatch against the sources ---------------------------------------------------------------------------------------------------
def _fs_launch_text():
    i = FS_SRC.index("int tante_fs_launch(")
    return FS_SRC[i:]


def test_fs_dispatch_constants_are_where_the_restatement_says():
    t = _fs_launch_text()
    assert {int(k) for k in re.findall(r"case (\d{3}):", t)} == set(R.FS_KEYS) and len(re.findall(r"case (\d{3}):", t)) == len(R.FS_KEYS)
    for text in ("if (sq.nseq >= (1 << 23)) return -2;", "if (tprop && (tr || sq.L != 4)) return -5;", "if (lastq && (tr || sq.L != 4)) return -5;",
                 "nw = (tr || tprop || lastq) ? 4 : fs_waves(L);", "if (16 % L == 0) tps = 1;",
                 "else if (!causal && (L == 32 || L == 48 || L == 64)) tps = L / 16;",
                 "const int full = nw == 8 ? 8 : 4, tq = nw == 8 ? 6 : 3;", "const long resident = 256L * (8 / nw);",
                 "const int spw = 16 * ntt / L;", "return ((nwg + resident - 1) / resident) * ntt;", "if (tps == 3) ntt = tq;",
                 "else if (tps >= 1 && (16 * tq) % L == 0 && (16 * tq) / L >= 1 && (tps == 1 || tq % tps == 0) && rounds(tq) < rounds(full)) ntt = tq;",
                 'if (!tr && nw == 4 && (tps == 1 || tps == 2) && 32 % L == 0 && tante_opt("TANTE_FS_HALF", 1)) {',
                 "if (((long)sq.nseq + spw_full - 1) / spw_full * 4 <= resident) ntt = 2;", "if (lastq && ntt == tq) ntt = full;",
                 "A.spw = tps ? 16 * ntt / L : (16 * full) / L;",
                 'A.skew = (!tr && nw == 4 && nwg > 256 && nwg <= 512) ? tante_opt("TANTE_FS_SKEW", 0) : 0;',
                 "if (ntt == 2) fs_launch_last<2>(A, nwg, s);", "else fs_launch_last<4>(A, nwg, s);", "const int key = nw * 100 + tps * 10 + ntt;",
                 "if (A.tprop) fs_launch_tt<1, 2, 4, false, 1, true>(A, nwg, s);"):
        assert text in t, text
    assert R.CUS == 256 and R.TILE == 16 and R.SKEW_WINDOW == (257, 512) and R.FS_MAX_NSEQ == 1 << 23
    for text in ('const int force8 = tante_opt("TANTE_FS_WAVES", 0) == 8;', "return (force8 || L > 64) ? 8 : 4;",
                 "return C == FS_C && n_head == 8 && hidden == FS_C && L >= 1 && L <= 128;",
                 'const int groups = tante_opt("TANTE_FS_GROUPS", 0);', "if (groups == 2) return fs_launch_tt<TPS, NTT, NW, false, 2>(A, nwg, s);",
                 "if (A.tprop) return fs_launch_tt<TPS, NTT, NW, false, 1, true>(A, nwg, s);",
                 "if (A.tprop) fs_launch_tt<1, NTT, 4, false, 1, true, true>(A, nwg, s);", "else fs_launch_tt<1, NTT, 4, false, 1, false, true>(A, nwg, s);"):
        assert text in FS_SRC, text
    # the keys that go through fs_launch_t at 4 waves are the ones that have a paired and (TPS 1) a propagator instance
    via_t = {int(k) for k, nw in re.findall(r"case (\d{3}): fs_launch_t<\d, \d, (\d)>", t) if nw == "4"}
    assert via_t == {413, 414, 424, 433, 444, 404}
    assert {r for r in R.ALL_FS_ROUTES if r.endswith(",G2>")} == {f"fs<TPS{k // 10 % 10},NTT{k % 10},NW4,G2>" for k in via_t}
    assert {r for r in R.ALL_FS_ROUTES if r.endswith(",TPROP>")} == {f"fs<TPS1,NTT{k % 10},NW4,TPROP>" for k in via_t | {412} if k // 10 % 10 == 1}
    assert len(R.ALL_FS_ROUTES) == 15 + 3 + 4 + 6


def test_ts_dispatch_constants_are_where_the_restatement_says():
    for text in ("const int per_wg = sq.L == 32 ? 4 : 8 * (16 / sq.L);  // sequences per workgroup", 'const int which = tante_opt("TANTE_BLOCK_KERNEL", 0);',
                 "if (which != 32 && (sq.L == 32 || 16 % sq.L == 0)) return launch_block16<CB, HB>(x, stream, sq, causal, eps, s);",
                 "const int spw = 32 / sq.L;", "const int waves = (sq.nseq + spw - 1) / spw;", "dim3((waves + 3) / 4), dim3(256)",
                 "dim3((sq.nseq + per_wg - 1) / per_wg), dim3(512)", "if (C != 64 && C != 128 && C != 256) return 0;",
                 "if (hidden != C && hidden != 2 * C) return 0;", "if (hidden > 256 && C == 256) return 0;", "if (L <= 0 || L > 32 || 32 % L) return 0;",
                 "if (!tante_fs_supported(C, n_head, hidden, L, causal)) return false;", "return which == 0 || !block_ts_supported(C, n_head, hidden, L);",
                 "const int key = (C / 32) * 100 + hidden / 32;"):
        assert text in TS_SRC, text
    inst = {(int(a), int(b)) for a, b in re.findall(r"case \d{3}: launch_block<(\d), (\d)>", TS_SRC)}
    assert inst == set(R.TS_INSTANCES)
    assert {int(k) for k in re.findall(r"case (\d{3}): launch_block<", TS_SRC)} == {cb * 100 + hb for cb, hb in R.TS_INSTANCES}
    assert TS_SRC.count('tante_opt("TANTE_BLOCK_KERNEL"') == 2      # launch_block and use_fs: both read "no choice" as 0
    # tprop / last under a forced round-1 kernel are refused: both entries ask use_fs
    assert "|| !use_fs(C, n_head, hidden, seq->L, causal))" in TS_SRC and "L == 4 && use_fs(C, n_head, hidden, L, 0);" in TS_SRC


def test_rule_at_its_thresholds():
    """The shapes of the case table are the smallest the rule allows: one sequence fewer takes another instance."""
    f = lambda *a, **k: R.fs_route(*a, **k).name      # noqa: E731
    assert f(16, 384, False) == "fs<TPS1,NTT2,NW4>" and f(16, 385, False) == "fs<TPS1,NTT3,NW4>"
    assert f(16, 1536, False) == "fs<TPS1,NTT3,NW4>" and f(16, 1537, False) == "fs<TPS1,NTT4,NW4>" and f(16, 2048, False) == "fs<TPS1,NTT4,NW4>"
    assert f(4, 6144, True) == "fs<TPS1,NTT3,NW4>" and f(4, 6145, True) == "fs<TPS1,NTT4,NW4>"      # test_fused_block's (4, 6144): 413
    assert f(32, 256, False) == "fs<TPS2,NTT2,NW4>" and f(32, 257, False) == "fs<TPS2,NTT4,NW4>"
    assert f(4, 1536, True, last=True) == "fs<TPS1,NTT2,NW4,LASTQ>" and f(4, 1537, True, last=True) == "fs<TPS1,NTT4,NW4,LASTQ>"
    w8 = {"TANTE_FS_WAVES": 8}
    assert f(16, 1536, False, options=w8) == "fs<TPS1,NTT6,NW8>" and f(16, 1537, False, options=w8) == "fs<TPS1,NTT8,NW8>"
    assert f(32, 768, False, options=w8) == "fs<TPS2,NTT6,NW8>" and f(32, 769, False, options=w8) == "fs<TPS2,NTT8,NW8>"
    r = R.fs_route(16, 1537, False, options={"TANTE_FS_SKEW": 3})
    assert (r.nwg, r.spw, r.skew) == (385, 4, 3) and R.fs_route(16, 385, False, options={"TANTE_FS_SKEW": 3}).skew == 0
    assert R.fs_route(5, 13, True).spw == 12 and R.fs_route(5, 13, True).nwg == 2
    assert not R.fs_supported(256, 8, 256, 129) and R.fs_supported(256, 8, 256, 128)
    with pytest.raises(R.Refused):
        R.fs_route(4, 1 << 23, False)
    with pytest.raises(R.Refused):
        R.fs_route(8, 4, True, tprop=True)
    assert not R.use_fs(256, 8, 256, 4, {"TANTE_BLOCK_KERNEL": 16}) and R.use_fs(256, 8, 256, 5, {"TANTE_BLOCK_KERNEL": 16})
    assert not R.ts_supported(256, 8, 512, 4) and not R.fs_supported(256, 8, 512, 4)


def test_every_case_reaches_the_route_it_names_and_all_routes_are_reached():
    reached = set()
    for c in R.BLOCK_CASES:
        got = R.route(c, c.opts)
        assert got == c.route, (c.id, got, c.route)
        reached.add(got)
        assert set(c.opts) <= set(R.OPTION_DEFAULTS)
    every = R.ALL_FS_ROUTES | R.ALL_TS_ROUTES
    assert set(R.UNREACHABLE_ROUTES) <= every
    assert reached == every - set(R.UNREACHABLE_ROUTES), sorted(every ^ reached)
    # what the issue's notes ask of the table beyond the routes
    ids = set(R.CASE_BY_ID)
    assert {"414-L16x1537", "414-L16x1537-skew3"} <= ids and R.fs_route(16, R.BIG16, False, options={"TANTE_FS_SKEW": 3}).skew == 3
    for c in R.BLOCK_CASES:
        if c.route.endswith(",G2>"):
            assert R.fs_route(c.L, c.nseq, c.causal, options=c.opts).nwg % 2 == 1, c.id      # the last workgroup's second group is empty
    ts = [c for c in R.TS_CASES]
    for C, hidden in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256)):
        for k in (16, 32):
            mine = [c for c in ts if (c.C, c.hidden) == (C, hidden) and c.opts["TANTE_BLOCK_KERNEL"] == k]
            assert {c.L for c in mine} >= {1, 4, 32} and {c.causal for c in mine} == {False, True}
            assert {c.nseq for c in mine if c.L == 4} == {33, 1}
        if C < 256:
            assert any(c.opts["TANTE_BLOCK_KERNEL"] == 0 for c in ts if (c.C, c.hidden) == (C, hidden))
    assert {c.L for c in ts} == {1, 2, 4, 8, 16, 32}
    lay = {c.layout[0] for c in R.LAYOUT_CASES if c.C == 256}
    assert lay >= {"T", "H", "W", "L", "Y", "X", "sub"}


# ---- the exact-bf16 evaluation and the per-token bar -------------------------------------------------------------------------------------
def test_exact_bf16_headroom_and_bar_rule(evaluated):
    worst, worst_id = 0.0, None
    for c in R.BLOCK_CASES:
        inp, ref, bf = evaluated[c.shape_id, c.last]
        wr = R.written_rows(c, inp)
        rel, mx, dl = R.errors(bf, ref, inp.buf, wr)
        tok = R.worst_token(bf, ref, inp.buf, wr)
        assert rel <= R.BAR_L2 / 2 and mx <= R.BAR_MAX / 2 and dl <= R.BAR_DELTA / 2 and tok <= R.BAR_TOKEN / 2, (c.id, rel, mx, dl, tok)
        if tok > worst:
            worst, worst_id = tok, c.id
    print(f"exact bf16 vs float64, worst token over {len(R.BLOCK_CASES)} cases: {worst:.4e} ({worst_id})")
    assert worst <= R.EXACT_BF16_WORST_TOKEN < 1.05 * worst, (worst, worst_id)
    assert R.bar_token_rule(worst) == pytest.approx(R.BAR_TOKEN) and R.BAR_TOKEN <= 2e-2
    assert R.bar_token_rule(4.7e-3) == pytest.approx(1e-2) and R.bar_token_rule(5.01e-3) == pytest.approx(2e-2)


# ---- planted faults ----------------------------------------------------------------------------------------------------------------------
def test_planted_faults(evaluated):
    """Every fault, planted into the exact-bf16 result of every FAULT_CASES entry that can have it, breaks the per-token bar (but the one
    of BELOW_FORMAT, whose size is the format's own); which of them the whole-tensor bars pass on the largest launch is PLANTED."""
    measured, seen = {}, set()
    for cid in FAULT_CASES:
        c = R.CASE_BY_ID[cid]
        inp, ref, _ = evaluated[c.shape_id, c.last]
        wr = R.written_rows(c, inp)
        for kind in R.FAULTS:
            bug = R.fault_for(c, kind)
            if bug is None:
                continue
            seen.add(kind)
            got = R.launch_ref(c, inp, exact_bf16=True, bug=bug)
            rel, mx, dl = R.errors(got, ref, inp.buf, wr)
            tok = R.worst_token(got, ref, inp.buf, wr)
            passes = (rel < R.BAR_L2, dl < R.BAR_DELTA, mx < R.BAR_MAX)
            print(f"{cid} {kind}: rel {rel:.2e} delta {dl:.2e} max {mx:.2e} worst token {tok:.2e} -> whole-tensor bars pass {passes}")
            if kind in BELOW_FORMAT:
                assert tok < R.BAR_TOKEN and all(passes), (cid, kind, tok)
            else:
                assert tok > R.BAR_TOKEN, (cid, kind, tok)
            if cid == BIG:
                measured[kind] = passes
    assert seen == set(R.FAULTS)
    assert measured == PLANTED, measured
    assert all(PLANTED[k][0] for k in R.SINGLE_TOKEN_FAULTS)      # the reason the per-token bar exists: one wrong token in 24 592 passes
    assert all(PLANTED["drop_head"])                               # ... and a dropped head passes every whole-tensor bar


def test_token_errors_leave_no_row_out():
    """A written row with NaN, a changed row outside the addressed ones and a changed slot-0 row of a `last` launch each give inf."""
    c = R.CASE_BY_ID["412-L4x37c-last"]
    inp = R.make_inputs(c)
    ref = R.launch_ref(c, inp)
    wr = R.written_rows(c, inp)
    assert int(wr.sum()) == c.nseq and R.worst_token(ref, ref, inp.buf, wr) == 0.0
    for row in (int(inp.tok[3, 3]), inp.buf.shape[0] - 1, int(inp.tok[5, 0])):
        got = ref.clone()
        got[row, 7] = float("nan") if row == int(inp.tok[3, 3]) else 1.0
        assert R.worst_token(got, ref, inp.buf, wr) == float("inf")
