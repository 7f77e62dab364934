"""Every launch form of the inference block kernels, alone, against float64 and per token: tante_block_fused, tante_block_fused_tprop and
tante_block_fused_last (csrc/block_sliced.hip: the feature-sliced kernel; csrc/block_fused.hip: the two round-1 kernels).

The cases, their float64 reference on the flat buffer, the exact-bf16 evaluation and the restated dispatch live in tests/block_forms_ref.py;
tests/test_block_forms_cpu.py pins them to the oracle, to the text of the two sources and to planted faults without a GPU.  Here every
case packs its weights with kernels.pack_block, sets its library options (TANTE_BLOCK_KERNEL, TANTE_FS_WAVES / _HALF / _GROUPS / _SKEW;
the earlier values come back in a `finally`), asserts the restated route from the option values the library reports, and calls
kernels.block_fused / block_fused_last / block_fused_subgrid on a buffer that is longer than the addressed rows and NaN there.

The buffer contract (the kernels work in place, so this is the whole memory-safety contract): every row the launch does not write --
before row0, between the addressed rows, the slack behind them, slots 0 .. L - 2 of a `last` launch -- holds the bits it held; written
rows hold no NaN.  Bars against float64: the project's whole-tensor bars (relative L2 1e-2 and scale-relative max 2e-2 on y, relative
L2 2e-2 on y - x) and BAR_TOKEN on EVERY written token's own contribution y - x.  The distance to the exact-bf16 evaluation is recorded
without a bar.  Bit equalities (torch.equal) the sources claim: a sequence's rows do not depend on the launch geometry (sequences of a
413 / 414 / 424 launch run alone), TANTE_FS_GROUPS 2 = 1, TANTE_FS_SKEW 3 = 0, TANTE_FS_HALF 0 = 1, the last-slot form = the slot-(L - 1) rows
of the full launch, a repeated launch.  For 8 against 4 waves, round-1 against feature-sliced and the 16 against the 32 form the sources say
"the same function": each side is held to float64 and whether they are bit-equal is recorded, not asserted.  The fused propagator against
tante_axis_mlp_c followed by tante_block_fused was claimed bit for bit by the header and is not (test_fused_propagator_against_its_own_launch).

The worst figures per route go to block_forms_parity.json beside parity_report.json (profiles/block_forms_parity.json is one such run)."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

import block_forms_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

FIGURES = {}        # route -> worst figures of this run
FAMILIES = {}       # kernel family -> worst per-token figure (kernel | exact bf16 against float64)
EQUALITIES = {}     # name -> held (asserted)
RECORDED = {}       # name -> bit-equal? (not asserted)
ROUTES_RUN = set()
CASES_RUN = set()
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    every = R.ALL_FS_ROUTES | R.ALL_TS_ROUTES
    try:
        with open(os.path.join(ROOT, "block_forms_parity.json"), "w") as f:
            json.dump({"bars": {"whole tensor rel L2 (y)": R.BAR_L2, "whole tensor max (y)": R.BAR_MAX, "whole tensor rel L2 (y - x)": R.BAR_DELTA,
                                "per token rel L2 (y - x)": R.BAR_TOKEN, "exact bf16 vs float64, worst token (CPU)": R.EXACT_BF16_WORST_TOKEN},
                       "routes": FIGURES, "families: worst token, kernel | exact bf16": FAMILIES, "bit_equalities": EQUALITIES,
                       "recorded_pairs_bit_equal": RECORDED, "routes_run": sorted(ROUTES_RUN), "routes_run_is_every_route": ROUTES_RUN == every,
                       "unreachable_routes": R.UNREACHABLE_ROUTES, "cases_run": len(CASES_RUN)}, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _ops():
    from tante_amd import kernels as K, _lib as L
    return K, L


@contextlib.contextmanager
def options(opts):
    """The library options of one launch; the earlier values come back whatever happens."""
    _, L = _ops()
    prev = {n: L.get_option(n, R.OPTION_DEFAULTS[n]) for n in opts}
    try:
        for n, v in opts.items():
            L.set_option(n, v)
            assert L.get_option(n, R.OPTION_DEFAULTS[n]) == v
        yield
    finally:
        for n, v in prev.items():
            L.set_option(n, v)


def reported_options():
    _, L = _ops()
    return {n: L.get_option(n, d) for n, d in R.OPTION_DEFAULTS.items()}


_EVAL, _PACKED, _OUT = {}, {}, {}


def evaluated(c):
    """A case's inputs, float64 reference and exact-bf16 evaluation: computed once per shape, shared, never modified."""
    key = (c.shape_id, c.last)
    if key not in _EVAL:
        inp = R.make_inputs(c)
        _EVAL[key] = (inp, R.launch_ref(c, inp), R.launch_ref(c, inp, exact_bf16=True), R.written_rows(c, inp))
    return _EVAL[key]


def packed(c, inp, dev):
    K, _ = _ops()
    key = (c.C, c.hidden, inp.wseed)
    if key not in _PACKED:
        _PACKED[key] = (K.pack_block([inp.w[k].to(dev) for k in R.PACK_ORDER], c.C, c.hidden), inp.w["tprop"].to(dev).contiguous())
    return _PACKED[key]


def lib_seq(c):
    """The TanteSeq of a case from tante_amd.kernels, checked against the restated one."""
    K, _ = _ops()
    if c.layout is None:
        s = K.dense_seq(c.nseq, c.L)
    elif c.layout[0] == "sub":
        s = K.last_slot_seq(*c.layout[1:])
    else:
        s = K.make_seq(*c.layout)
    assert tuple(getattr(s, f) for f in R.Seq._fields) == tuple(c.seq()), c.id
    return s


def launch(dev, c, inp, opts=None, pre=None):
    """One launch of a case under `opts` (default: the case's own) -> (the buffer afterwards on the CPU, the route)."""
    K, _ = _ops()
    st, tp = packed(c, inp, dev)
    x = inp.buf.to(dev).contiguous()
    assert x.data_ptr() % 16 == 0 and int(inp.tok.max()) < x.shape[0] and int(inp.tok.min()) >= 0
    seq = lib_seq(c)
    with options(c.opts if opts is None else opts):
        route = R.route(c, reported_options())
        if pre is not None:
            pre(x)
        if c.last:
            K.block_fused_last(x, st, c.C, c.C // 32, c.hidden, seq, c.causal, EPS, tp if c.tprop else None)
        elif c.row0:
            K.block_fused_subgrid(x, c.row0, st, c.C, c.C // 32, c.hidden, seq, c.causal, EPS)
        else:
            K.block_fused(x, st, c.C, c.C // 32, c.hidden, seq, c.causal, EPS, tp if c.tprop else None)
    torch.cuda.synchronize()
    return x.cpu(), route


def family(route):
    return "feature-sliced" if route.startswith("fs<") else route.split("<")[0]


def hold(c, route, got, what=None):
    """The buffer contract and the four bars of one result, every figure printed and recorded before it is asserted."""
    inp, ref, bf, wr = evaluated(c)
    what = what or f"{c.id} {route}"
    untouched = bool(R._same(got[~wr], inp.buf[~wr]).all())
    finite = bool(torch.isfinite(got[wr]).all())
    rel, mx, dl = R.errors(got, ref, inp.buf, wr)
    tok = R.worst_token(got, ref, inp.buf, wr)
    rel2, mx2, dl2 = R.errors(got, bf, inp.buf, wr)
    tok2 = R.worst_token(got, bf, inp.buf, wr)
    tokbf = R.worst_token(bf, ref, inp.buf, wr)
    print(f"{what}: vs float64 rel {rel:.3e} max {mx:.3e} y-x {dl:.3e} worst token {tok:.3e} | vs exact bf16 rel {rel2:.3e} max {mx2:.3e} "
          f"y-x {dl2:.3e} worst token {tok2:.3e} | exact bf16 vs float64 worst token {tokbf:.3e} | unwritten rows unchanged {untouched}")
    record_parity(rel, mx, R.BAR_L2, "bf16", f"{what}: whole tensor")
    record_parity(dl, mx, R.BAR_DELTA, "bf16", f"{what}: y - x")
    record_parity(tok, mx, R.BAR_TOKEN, "bf16", f"{what}: worst token of y - x")
    w = FIGURES.setdefault(route, {"vs float64": {"rel": 0.0, "max": 0.0, "y-x": 0.0, "worst token": 0.0},
                                   "vs exact bf16 (recorded)": {"rel": 0.0, "max": 0.0, "y-x": 0.0, "worst token": 0.0},
                                   "exact bf16 vs float64, worst token": 0.0, "cases": []})
    for key, vals in (("vs float64", (rel, mx, dl, tok)), ("vs exact bf16 (recorded)", (rel2, mx2, dl2, tok2))):
        for n, v in zip(("rel", "max", "y-x", "worst token"), vals):
            w[key][n] = max(w[key][n], v) if v == v else float("nan")
    w["exact bf16 vs float64, worst token"] = max(w["exact bf16 vs float64, worst token"], tokbf)
    w["cases"].append(c.id)
    fam = FAMILIES.setdefault(family(route), {"kernel": 0.0, "exact bf16": 0.0})
    fam["kernel"], fam["exact bf16"] = max(fam["kernel"], tok), max(fam["exact bf16"], tokbf)
    assert untouched, f"{what}: a row the launch does not address (or a slot a `last` launch leaves alone) changed"
    assert finite, f"{what}: NaN / inf in a written row"
    assert rel < R.BAR_L2 and mx < R.BAR_MAX and dl < R.BAR_DELTA and tok < R.BAR_TOKEN, \
        f"{what}: rel {rel:.3e} max {mx:.3e} y-x {dl:.3e} worst token {tok:.3e}"


def equal(name, a, b):
    eq = bool(torch.equal(a, b))
    EQUALITIES[name] = eq
    assert eq, f"{name}: not bit-equal (max difference {float((a.double() - b.double()).nan_to_num().abs().max()):.3e})"


def record_pair(name, a, b):
    RECORDED[name] = bool(torch.equal(a, b))
    print(f"{name}: bit-equal {RECORDED[name]}")


def run(dev, c):
    """A case's launch, held to its bars, once per session (the equality tests below read the same result)."""
    if c.id not in _OUT:
        inp = evaluated(c)[0]
        got, route = launch(dev, c, inp)
        assert route == c.route, (c.id, route, c.route)
        ROUTES_RUN.add(route)
        hold(c, route, got)
        _OUT[c.id] = got
        CASES_RUN.add(c.id)
    return _OUT[c.id]


def rows_of(c, got):
    """The written rows of a case's buffer (NaN-free, so torch.equal compares values)."""
    return got[evaluated(c)[3]]


@pytest.mark.parametrize("c", R.BLOCK_CASES, ids=[c.id for c in R.BLOCK_CASES])
def test_block_form(dev, c):
    """One case: the route it names, the buffer contract, the four bars; and the same launch once more gives the same bits."""
    got = run(dev, c)
    again, _ = launch(dev, c, evaluated(c)[0])
    equal(f"{c.id}: the same launch repeated", rows_of(c, got), rows_of(c, again))


# which options two cases of one shape may differ in and still have to give the same bits (the sources' claims)
_SAME_BITS = {"TANTE_FS_GROUPS", "TANTE_FS_SKEW", "TANTE_FS_HALF"}


def _shape_groups():
    groups = {}
    for c in R.BLOCK_CASES:
        groups.setdefault((c.shape_id, c.last), []).append(c)
    return [g for g in groups.values() if len(g) > 1]


@pytest.mark.parametrize("group", _shape_groups(), ids=[g[0].id + "+" for g in _shape_groups()])
def test_forms_of_one_shape(dev, group):
    """Cases that share a shape (inputs, weights) and differ in the launch form.  Asserted bit-equal: the paired form, the entry skew, the
    half-size rule, and TANTE_BLOCK_KERNEL 16 against no choice at C = 64 / 128 (the same kernel).  Recorded: 8 against 4 waves, the 16
    against the 32 form."""
    base = group[0]
    a = rows_of(base, run(dev, base))
    for c in group[1:]:
        b = rows_of(c, run(dev, c))
        differ = {n for n in R.OPTION_DEFAULTS if R._opt(base.opts, n) != R._opt(c.opts, n)}
        same_kernel = differ == {"TANTE_BLOCK_KERNEL"} and base.route == c.route
        name = f"{c.id} vs {base.id} ({c.route} vs {base.route})"
        if differ <= _SAME_BITS or same_kernel:
            equal(name, a, b)
        else:
            record_pair(name, a, b)


def _alone(dev, c, s):
    """Sequence s of a dense case as a launch of its own (no option set): its rows."""
    inp = evaluated(c)[0]
    one = c._replace(name=f"{c.id}-seq{s}-alone", nseq=1, options=(), route=None)
    i1 = R.Inputs()
    i1.tok = R.seq_tokens(one.seq())
    i1.buf = torch.full((c.L + R.SLACK_ROWS, c.C), float("nan"))
    i1.buf[:c.L] = inp.buf[inp.tok[s]]
    i1.w, i1.wseed = inp.w, inp.wseed
    got, route = launch(dev, one, i1)
    return got[:c.L], route


@pytest.mark.parametrize("cid,small", [("413-L16x385", "fs<TPS1,NTT2,NW4>"), ("414-L16x1537", "fs<TPS1,NTT2,NW4>"),
                                       ("424-L32x257", "fs<TPS2,NTT2,NW4>"), ("413-L4x1537c", "fs<TPS1,NTT2,NW4>")])
def test_rows_do_not_depend_on_the_geometry(dev, cid, small):
    """The first and the last sequence of a three-quarter / full-size launch, each run alone (the half-size form), equal their rows in the
    large launch: the last sequence sits in the ragged last workgroup, the first one in a full workgroup."""
    c = R.CASE_BY_ID[cid]
    inp = evaluated(c)[0]
    got = run(dev, c)
    for s in (0, c.nseq - 1):
        rows, route = _alone(dev, c, s)
        assert route == small, route
        equal(f"{cid}: sequence {s} alone ({small}) vs inside the launch ({c.route})", rows, got[inp.tok[s]])


# tests/test_hip_round2.py::test_temporal_propagator_inside_the_block_launch holds the two forms to these through a whole backbone
TPROP_PAIR_L2, TPROP_PAIR_MAX = 2e-4, 2e-3


@pytest.mark.parametrize("cid", [c.id for c in R.BLOCK_CASES if c.tprop and not c.last])
def test_fused_propagator_against_its_own_launch(dev, cid):
    """tante_block_fused_tprop against tante_axis_mlp_c (bf16 compute) along T followed by tante_block_fused.  include/tante_hip.h said
    "bit for bit"; they are not (first seen on 412-L4x37c-tprop: 2.1e-3 apart behind the block).  Both run the same k-ordered chains from the
    bias in fp32 with the same GELU polynomial -- axis_mlp_vec_kernel<4, true> as v_pk_fma_f32 (read in its ISA), the fused form as
    v_mfma_f32_4x4x1 -- so the propagated rows agree to fp32 rounding, and behind the bf16 block a last-bit difference of a row moves the
    bf16 rounding of a LayerNorm output here and there.  Held: each side to float64 (all four bars), the pair to a fiftieth of the bf16
    bars (relative L2 2e-4, scale-relative max 2e-3: the project's bars for this pair, tests/test_hip_round2.py); bit equality is recorded."""
    K, L = _ops()
    c = R.CASE_BY_ID[cid]
    inp = evaluated(c)[0]
    w1, b1, w2, b2 = [t.to(dev).contiguous() for t in R.tprop_parts(inp.w)]
    if c.layout is None:
        outer, inner = c.nseq, c.C                       # dense (nseq, 4, C)
    else:
        _, B, T, H, W = c.layout
        outer, inner = B, H * W * c.C                    # (B, 4, H W C)
    plain = c._replace(tprop=False)
    got2, route2 = launch(dev, plain, inp, pre=lambda x: K.axis_mlp(x, outer, 4, inner, w1, b1, w2, b2, L.BF16))
    assert route2 == c.route.replace(",TPROP", ""), route2
    hold(c, route2, got2, f"{cid}: tante_axis_mlp_c + tante_block_fused {route2}")
    a, b = rows_of(c, run(dev, c)).double(), rows_of(c, got2).double()
    rel, mx = float((a - b).norm() / b.norm()), float((a - b).abs().max() / b.abs().max())
    print(f"{cid}: fused propagator vs its own launch: rel {rel:.3e} max {mx:.3e}")
    record_parity(rel, mx, TPROP_PAIR_L2, "bf16", f"{cid}: fused propagator vs tante_axis_mlp_c + tante_block_fused")
    record_pair(f"{cid}: fused propagator vs tante_axis_mlp_c + tante_block_fused ({route2})", a, b)
    assert rel < TPROP_PAIR_L2 and mx < TPROP_PAIR_MAX, (rel, mx)


@pytest.mark.parametrize("cid", [c.id for c in R.BLOCK_CASES if c.last])
def test_last_slot_form_equals_the_full_launch(dev, cid):
    """tante_block_fused_last writes the slot-(L - 1) rows of the full launch, bit for bit, at both tile counts, with and without the
    propagator (that the other slots keep their bits is part of every case's buffer contract)."""
    c = R.CASE_BY_ID[cid]
    full = R.CASE_BY_ID[cid.replace("-last", "")]
    assert (full.shape_id, full.tprop, full.last) == (c.shape_id, c.tprop, False)
    inp = evaluated(c)[0]
    rows = inp.tok[:, c.L - 1]
    equal(f"{cid} ({c.route}) vs slot {c.L - 1} of {full.id} ({full.route})", run(dev, c)[rows], run(dev, full)[rows])


@pytest.mark.parametrize("cid", [c.id for c in R.TS_CASES if c.C == 256 and c.opts["TANTE_BLOCK_KERNEL"] == 16])
def test_round1_against_feature_sliced_is_recorded(dev, cid):
    """The same shape with no kernel forced (the feature-sliced kernel): held to float64 like any case; bit equality with the round-1
    kernel is recorded, not asserted ("the same function")."""
    c = R.CASE_BY_ID[cid]
    inp = evaluated(c)[0]
    fs = c._replace(options=())
    got, route = launch(dev, fs, inp)
    assert route.startswith("fs<") and route == R.route(fs, {}), route
    ROUTES_RUN.add(route)
    hold(fs, route, got, f"{cid} with no kernel forced {route}")
    record_pair(f"{cid} ({c.route}) vs the feature-sliced kernel ({route})", rows_of(c, run(dev, c)), rows_of(c, got))


def test_refusals(dev):
    """Calls the C side must turn away with a negative code and a message before anything is launched: the buffer keeps its bits.  The
    guards are read in the source first -- none of these calls is made against a library without them -- and every buffer is large enough
    for what such a launch would have touched.  -2 (unsupported shape) for the propagator / last-slot entries under a forced round-1
    kernel, L = 129 and hidden 512 at C = 256; a misaligned x is a bad ARGUMENT, -1 by the header's convention (include/tante_hip.h:
    "-1 bad argument, -2 unsupported shape")."""
    K, L = _ops()
    src = open(os.path.join(ROOT, "tante_amd", "csrc", "block_fused.hip")).read()
    for guard in ("if (seq->L != 4 || !tante_block_fused_supported(C, n_head, hidden, seq->L) || !use_fs(C, n_head, hidden, seq->L, causal))",
                  "if (!tante_block_fused_last_supported(C, n_head, hidden, seq->L))", "if (!tante_block_fused_supported(C, n_head, hidden, seq->L))",
                  'if (((uintptr_t)x % 16) || ((uintptr_t)block_stream % 16)) TANTE_FAIL(-1, "tante_block_fused: buffers must be 16-byte aligned");'):
        assert guard in src, guard
    c = R.CASE_BY_ID["412-L4x37c"]
    inp = evaluated(c)[0]
    st, tp = packed(c, inp, dev)
    x0 = torch.randn(4096, 256, generator=torch.Generator().manual_seed(1))
    x = x0.to(dev)
    lib, s = L.lib(), K._stream()

    def refused(rc, code, text):
        assert rc == code, (rc, text)
        msg = lib.tante_last_error().decode(errors="replace")
        assert text in msg, msg
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), x0), text

    q4 = K.dense_seq(37, 4)
    with options({"TANTE_BLOCK_KERNEL": 16}):
        assert not R.use_fs(256, 8, 256, 4, reported_options())
        refused(lib.tante_block_fused_tprop(x.data_ptr(), st.data_ptr(), 256, 8, 256, C.byref(q4), 1, EPS, tp.data_ptr(), s), -2,
                "tante_block_fused_tprop: the feature-sliced kernel at L = 4 only")
        refused(lib.tante_block_fused_last(x.data_ptr(), st.data_ptr(), 256, 8, 256, C.byref(q4), 1, EPS, None, s), -2,
                "tante_block_fused_last: the feature-sliced kernel at C = 256")
    q129 = K.dense_seq(2, 129)
    refused(lib.tante_block_fused(x.data_ptr(), st.data_ptr(), 256, 8, 256, C.byref(q129), 0, EPS, s), -2, "unsupported shape C=256 heads=8 hidden=256 L=129")
    refused(lib.tante_block_fused(x.data_ptr(), st.data_ptr(), 256, 8, 512, C.byref(q4), 0, EPS, s), -2, "unsupported shape C=256 heads=8 hidden=512 L=4")
    assert lib.tante_block_stream_bytes(256, 256) > 0 and not K.block_fused_supported(256, 8, 512, 4) and not K.block_fused_supported(256, 8, 256, 129)
    for entry, call in (("tante_block_fused", lambda: lib.tante_block_fused(x.data_ptr() + 4, st.data_ptr(), 256, 8, 256, C.byref(q4), 0, EPS, s)),
                        ("tante_block_fused_tprop", lambda: lib.tante_block_fused_tprop(x.data_ptr() + 4, st.data_ptr(), 256, 8, 256, C.byref(q4), 1, EPS,
                                                                                        tp.data_ptr(), s)),
                        ("tante_block_fused_last", lambda: lib.tante_block_fused_last(x.data_ptr() + 8, st.data_ptr(), 256, 8, 256, C.byref(q4), 1, EPS,
                                                                                      None, s))):
        refused(call(), -1, f"{entry}: buffers must be 16-byte aligned")
    with pytest.raises(RuntimeError, match="unsupported shape"):
        K.block_fused(x, st, 256, 8, 256, q129, False, EPS)
    assert reported_options() == R.OPTION_DEFAULTS


def test_every_template_instance_ran(dev):
    """After the cases above: the routes asserted on the way are every template instance the two launchers can select (counted from the
    launch switches by tests/test_block_forms_cpu.py), every asserted equality held, and the options are back at their defaults."""
    assert reported_options() == R.OPTION_DEFAULTS
    if CASES_RUN != {c.id for c in R.BLOCK_CASES}:
        pytest.skip("only part of this module was selected")
    every = (R.ALL_FS_ROUTES | R.ALL_TS_ROUTES) - set(R.UNREACHABLE_ROUTES)
    assert ROUTES_RUN == every, sorted(every ^ ROUTES_RUN)
    assert EQUALITIES and all(EQUALITIES.values())
    for fam, w in FAMILIES.items():
        print(f"{fam}: worst token of y - x vs float64: kernel {w['kernel']:.3e} | exact bf16 {w['exact bf16']:.3e}")
    print("recorded pairs bit-equal:", json.dumps(RECORDED, indent=1))
