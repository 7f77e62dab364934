"""The weight-gradient GEMM alone: every dispatch form of tante_amd/csrc/wgrad.hip against float64.

The cases, their float64 references and the restated dispatch (`wgrad_route`) live in tests/wgrad_forms_ref.py; tests/test_wgrad_forms_cpu.py
pins them to the text of wgrad.hip, to torch's own operators and to wrong results without a GPU.  Here every case builds its TanteRowMats by
hand (tante_amd._lib.RowMat / WgradJob) on real device pointers, asserts that those descriptors take the route its id names, sets its options
and restores them, and calls the C entry point into gradient slots with guard elements on either side (NaN-filled for accumulate = 0, a random
pre-fill for accumulate = 1).  Bars (tests/test_hip_train_ops.py): relative L2 2e-5 / max-norm 1e-4, 1e-4 / 5e-4 past 4096 summed terms --
bf16 sources hold bf16-exact values, so only the fp32 accumulation order differs from float64.  bf16 compute on fp32 sources is held to
5e-3 / 1.6e-2 against the unrounded reference and, since pack_bf16x2 (common.hip.h: a __bf16 cast) rounds to nearest even, to the fp32 bars
against the reference on bf16-rounded operands."""
import ctypes as C
import json
import os

import pytest
import torch

import wgrad_forms_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

FIGURES = {}        # group -> what was compared -> worst [relative L2, max-norm] of this run (wgrad_forms_parity.json)
EQUALITIES = {}     # pairs of forms on the same values: bit-equal or not, and their distance
GUARD, GUARD_VALUE = 8, 7.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    try:
        with open(os.path.join(ROOT, "wgrad_forms_parity.json"), "w") as f:
            json.dump({"groups": FIGURES, "same_values": EQUALITIES}, f, indent=1, sort_keys=True)
    except OSError:
        pass


_INPUTS, _RESULTS, _WS = {}, {}, {}


def inputs(c):
    """The operands and references of a case, computed once on the CPU and shared (never modified: every run uploads its own copies)."""
    if c.id not in _INPUTS:
        inp = R.make_inputs(c)
        inp.ref = R.reference(c, inp)
        inp.ref_bf = R.reference(c, inp, exact_bf16=True) if c.rounds_sources() else None
        _INPUTS[c.id] = inp
    return _INPUTS[c.id]


def workspace(dev):
    if dev not in _WS:
        _WS[dev] = torch.empty(R.BIG_WS, dtype=torch.uint8, device=dev)
    return _WS[dev]


def _rowmat(L, m, buf):
    assert buf.data_ptr() % 16 == 0
    rm = L.RowMat()
    rm.p = buf.data_ptr() + m.lead * buf.element_size()
    rm.dtype, rm.mode, rm.s1, rm.s0, rm.off, rm.es, rm.n0 = m.dtype, m.mode, m.s1, m.s0, m.off, m.es, m.n0
    rm.Hin, rm.Win, rm.Cin, rm.P = m.Hin, m.Win, m.Cin, m.P
    return rm


def run_case(c, inp, dev):
    """One call of the case's entry point.  -> per job (dW as the flat parameter, dbias or None), CPU tensors; the guards are checked here."""
    import tante_amd
    from tante_amd import _lib as L
    assert (L.F32, L.BF16, L.A_LINEAR, L.A_PATCH_NHWC, L.A_PATCH_NCHW) == (R.F32, R.BF16, R.A_LINEAR, R.A_PATCH_NHWC, R.A_PATCH_NCHW)
    assert (L.W_LINEAR, L.W_CONV_NHWC, L.W_DECONV_NHWC, L.W_DECONV_NCHW) == (R.W_LINEAR, R.W_CONV_NHWC, R.W_DECONV_NHWC, R.W_DECONV_NCHW)
    keep, mats, slots = [], [], []
    for k, jb in enumerate(c.jobs):
        arrs = []
        for side, ms in ((0, jb.U), (1, jb.V)):
            dbufs = [b.to(dev) for b in inp.bufs[k][side]]
            keep.append(dbufs)
            arrs.append((L.RowMat * jb.n_seg)(*[_rowmat(L, m, b) for m, b in zip(ms, dbufs)]))
        mats.append(arrs)
        slot = []
        for n, pre in ((jb.I * jb.J, inp.pre[k][0]), (jb.I, inp.pre[k][1])):
            t = torch.full((n + 2 * GUARD,), GUARD_VALUE)
            t[GUARD:GUARD + n] = pre if c.acc else float("nan")
            slot.append(t.to(dev))
        slots.append(slot)
    ws = workspace(dev)
    ws.fill_(255)       # NaN in every float: a partial that is read without having been written shows
    assert ws.data_ptr() % 16 == 0
    plan = c.route_for([(list(a[0]), list(a[1])) for a in mats])
    assert plan.name == c.route, (plan.name, c.route)
    wsp, wsb = (ws.data_ptr(), c.ws_bytes) if c.ws_bytes else (None, 0)
    s = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    opts = dict(R.DEFAULTS, **c.options)
    before = {k: L.get_option(k, R.DEFAULTS[k]) for k in opts}
    before = {k: v for k, v in before.items() if v != opts[k]}      # only what differs is set (the library's option table is small) and restored
    try:
        for k in before:
            tante_amd.set_option(k, opts[k])
        jb = c.jobs[0]
        dW, db = slots[0][0].data_ptr() + 4 * GUARD, (slots[0][1].data_ptr() + 4 * GUARD) if jb.bias else None
        if c.entry == "one":
            U, V = mats[0]
            if c.ws_bytes:
                rc = lib.tante_wgrad_ws(U, V, jb.R, jb.I, jb.J, dW, db, jb.layout, jb.P, jb.Co, jb.swap, c.compute, c.accumulate, wsp, wsb, s)
            else:
                rc = lib.tante_wgrad(U, V, jb.R, jb.I, jb.J, dW, db, jb.layout, jb.P, jb.Co, jb.swap, c.compute, c.accumulate, s)
        elif c.entry == "multi":
            U, V = mats[0]
            if c.ws_bytes:
                rc = lib.tante_wgrad_multi_ws(C.byref(U), C.byref(V), jb.n_seg, jb.R, jb.I, jb.J, dW, db, jb.layout, jb.P, jb.Co, jb.swap, c.compute,
                                              c.accumulate, wsp, wsb, s)
            else:
                rc = lib.tante_wgrad_multi(C.byref(U), C.byref(V), jb.n_seg, jb.R, jb.I, jb.J, dW, db, jb.layout, jb.P, jb.Co, jb.swap, c.compute,
                                           c.accumulate, s)
        else:
            jobs = (L.WgradJob * len(c.jobs))()
            for w, jb, (U, V), slot in zip(jobs, c.jobs, mats, slots):
                w.U, w.V, w.n_seg, w.R, w.I, w.J = U, V, jb.n_seg, jb.R, jb.I, jb.J
                w.dW, w.dbias = slot[0].data_ptr() + 4 * GUARD, (slot[1].data_ptr() + 4 * GUARD) if jb.bias else None
                w.layout, w.P, w.C_other, w.swap = jb.layout, jb.P, jb.Co, jb.swap
            rc = lib.tante_wgrad_jobs_ws(jobs, len(c.jobs), c.compute, wsp, wsb, s)
        L.check(rc, c.id)
        torch.cuda.synchronize()
    finally:
        for k, v in before.items():
            tante_amd.set_option(k, v)
    out = []
    for k, (jb, slot) in enumerate(zip(c.jobs, slots)):
        got = []
        for t, n, used in ((slot[0].cpu(), jb.I * jb.J, True), (slot[1].cpu(), jb.I, jb.bias)):
            assert bool((t[:GUARD] == GUARD_VALUE).all()) and bool((t[GUARD + n:] == GUARD_VALUE).all()), f"{c.id}: wrote outside the parameter"
            body = t[GUARD:GUARD + n]
            if not used:       # no dbias pointer: the slot is as it was
                assert torch.equal(body, inp.pre[k][1]) if c.acc else bool(torch.isnan(body).all()), c.id
            got.append(body if used else None)
        out.append(tuple(got))
    return out


def _worst(group, key, rel, mx):
    w = FIGURES.setdefault(group, {}).setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel), max(w[1], mx)


def hold(c, got, inp):
    """The bars of a case, per job and per tensor (the bias gradient is held to its own bar); every figure is printed and recorded."""
    bad = []
    for k, jb in enumerate(c.jobs):
        for what, g, r, rb in (("dW", got[k][0], inp.ref[k][0], inp.ref_bf and inp.ref_bf[k][0]), ("dbias", got[k][1], inp.ref[k][1], inp.ref_bf and inp.ref_bf[k][1])):
            if g is None:
                continue
            rel, mx = R.errors(g, r)
            bl2, bmx = c.bars(jb, exact=False)
            mode = "bf16-rounds" if c.rounds_sources() else ("bf16" if c.compute == R.BF16 else "fp32")
            print(f"{c.id} job {k} {what}: route {c.route}: vs float64 rel {rel:.3e} max {mx:.3e} (bar {bl2:.0e} / {bmx:.0e})")
            record_parity(rel, mx, bl2, mode, f"{c.route} {what}")
            _worst(c.group, f"{mode} vs float64, bar {bl2:.0e} / {bmx:.0e}", rel, mx)
            if not (rel < bl2 and mx < bmx):
                bad.append((k, what, rel, mx))
            if rb is not None:
                rel2, mx2 = R.errors(g, rb)
                f2, fm = c.bars(jb, exact=True)
                print(f"{c.id} job {k} {what}: vs float64 on bf16-rounded operands rel {rel2:.3e} max {mx2:.3e} (bar {f2:.0e} / {fm:.0e})")
                record_parity(rel2, mx2, f2, "bf16-exact", f"{c.route} {what}: against the reference on rounded operands")
                _worst(c.group, f"bf16-rounds vs rounded operands, bar {f2:.0e} / {fm:.0e}", rel2, mx2)
                if not (rel2 < f2 and mx2 < fm):
                    bad.append((k, what + " (rounded operands)", rel2, mx2))
    assert not bad, (c.id, bad)


def result(c, dev):
    if c.id not in _RESULTS:
        _RESULTS[c.id] = run_case(c, inputs(c), dev)
    return _RESULTS[c.id]


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_form(dev, c):
    """Groups (a) - (f) of the case list: one call each, the route asserted from the real descriptors."""
    hold(c, result(c, dev), inputs(c))


def _same_value_groups():
    groups = {}
    for c in R.CASES:
        groups.setdefault((c.vkey, c.compute, c.acc, tuple((j.R, j.I, j.J, j.n_seg) for j in c.jobs)), []).append(c)
    return [cs for cs in groups.values() if len(cs) > 1]


def code_guarantees_equality(a, b):
    """Two launches of wgrad_kernel<BF16, T, .., ..> that differ only in how the operands are staged hold the same LDS image chunk by chunk
    and run the same MFMA sequence; with at most two splits added onto zeros the atomics cannot reorder a sum (x + y = y + x)."""
    ra, rb = a.route, b.route
    return (a.entry == b.entry == "one" and ra.startswith("gen<") and rb.startswith("gen<") and ra.split(",")[:2] == rb.split(",")[:2] and
            ra.endswith("+atomic") and rb.endswith("+atomic") and a.plan.split == b.plan.split <= 2 and not a.acc)


SAME = _same_value_groups()


@pytest.mark.parametrize("cs", SAME, ids=[cs[0].id + "-and-%d" % (len(cs) - 1) for cs in SAME])
def test_two_forms_on_the_same_values(dev, cs):
    """Aligned / misaligned operands, tr / NO_TR, slab / atomic (TANTE_WGRAD_NO_SLAB), jobs / one-by-one, RG / DEEP: the same values through
    two forms.  Each is held to float64 (test_form's bars, again here), their distance stays inside the bar, and they are bit-equal where
    the code guarantees it (code_guarantees_equality) -- not after TANTE_WGRAD_NO_SLAB and the like, where atomics reorder the sums."""
    a = cs[0]
    ya = result(a, dev)
    hold(a, ya, inputs(a))
    for b in cs[1:]:
        yb = result(b, dev)
        hold(b, yb, inputs(b))
        for k, jb in enumerate(a.jobs):
            for what, u, v in (("dW", ya[k][0], yb[k][0]), ("dbias", ya[k][1], yb[k][1])):
                if u is None or v is None:
                    continue
                rel, mx = R.errors(v, u)
                eq = bool(torch.equal(u, v))
                EQUALITIES[f"{a.id} | {b.id} job {k} {what}"] = {"bit_equal": eq, "rel": rel, "max": mx}
                print(f"{a.id} | {b.id} job {k} {what}: bit-equal {eq}, distance rel {rel:.3e} max {mx:.3e}")
                bl2, bmx = a.bars(jb, exact=True)
                assert rel < 2 * bl2 and mx < 2 * bmx, (a.id, b.id, what, rel, mx)      # each within the bar of float64
                if code_guarantees_equality(a, b):
                    assert eq, (a.id, b.id, what, rel, mx)


def test_workspace_below_one_partial_returns(dev):
    """tante_wgrad_ws with a 16-byte workspace (launch_wgrad used to divide by ws_bytes / partial = 0): returns 0, takes the atomic form and
    gives the gradient; so do 1 .. 2 partials minus a byte."""
    for comp in (R.F32, R.BF16):
        for name in ("ws-below-one-partial", "ws-below-two-partials"):
            c = [x for x in R.CASES if x.group == "c" and x.name == name and x.compute == comp][0]
            assert c.route.endswith("+atomic")
            hold(c, result(c, dev), inputs(c))
