"""The half-size block launches on 8 waves (TANTE_FS_HALF8, block_sliced.hip: tante_fs_half8_launch) against the same call on the
4-wave 2-tile form (TANTE_FS_HALF8 = 0), against the full-size 4-wave form (TANTE_FS_HALF = 0) -- torch.equal, not a tolerance -- against
itself on a fresh copy of the buffer, and against float64 under the bars of tests/block_forms_ref.py.  The buffer contract is the one of
tests/test_hip_block_forms.py: the buffer is longer than the addressed rows and NaN there, unwritten rows keep their bits, written rows
hold no NaN.  Cases: tests/block_half8_ref.py (the issue's W letter on the (2, 4, 32, 3) grid is L = 3, which no tile-aligned form takes:
it is held as a shape the rule does not cover, and the W letter at L = 32 comes from the (2, 4, 3, 32) grid)."""
import contextlib

import pytest
import torch

import block_forms_ref as R
import block_half8_ref as H

pytestmark = pytest.mark.gpu
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ops():
    from tante_amd import kernels as K, _lib as L
    return K, L


@contextlib.contextmanager
def options(opts):
    """The library options of one launch; the earlier values come back whatever happens."""
    _, L = _ops()
    prev = {n: L.get_option(n, H.OPTION_DEFAULTS[n]) for n in opts}
    try:
        for n, v in opts.items():
            L.set_option(n, v)
            assert L.get_option(n, H.OPTION_DEFAULTS[n]) == v
        yield
    finally:
        for n, v in prev.items():
            L.set_option(n, v)


def reported_options():
    _, L = _ops()
    return {n: L.get_option(n, d) for n, d in H.OPTION_DEFAULTS.items()}


_EVAL, _PACKED = {}, {}


def evaluated(c):
    """A case's inputs, float64 reference and written rows: computed once, shared, never modified."""
    if c.id not in _EVAL:
        inp = R.make_inputs(c)
        _EVAL[c.id] = (inp, R.launch_ref(c, inp), R.written_rows(c, inp))
    return _EVAL[c.id]


def launch(dev, c, opts):
    """One launch of a case on a fresh copy of its buffer under `opts` -> (the buffer afterwards on the CPU, the rule's answer)."""
    K, _ = _ops()
    inp = evaluated(c)[0]
    if inp.wseed not in _PACKED:
        _PACKED[inp.wseed] = K.pack_block([inp.w[k].to(dev) for k in R.PACK_ORDER], c.C, c.hidden)
    st = _PACKED[inp.wseed]
    x = inp.buf.to(dev).contiguous()
    assert x.data_ptr() % 16 == 0 and int(inp.tok.max()) < x.shape[0] and int(inp.tok.min()) >= 0
    if c.layout is None:
        seq = K.dense_seq(c.nseq, c.L)
    else:
        assert c.layout[0] == "sub"
        seq = K.last_slot_seq(*c.layout[1:])
    assert tuple(getattr(seq, f) for f in R.Seq._fields) == tuple(c.seq()), c.id
    with options(opts):
        rep = reported_options()
        assert all(rep[n] == v for n, v in opts.items())
        rule = H.half8_rule(c.L, c.nseq, c.causal, rep)
        if c.row0:
            K.block_fused_subgrid(x, c.row0, st, c.C, c.C // 32, c.hidden, seq, c.causal, EPS)
        else:
            K.block_fused(x, st, c.C, c.C // 32, c.hidden, seq, c.causal, EPS)
    torch.cuda.synchronize()
    return x.cpu(), rule


def same_buffer(what, a, b, wr):
    """Every row of two result buffers: the written rows by torch.equal (they hold no NaN), the others bit for bit with NaN = NaN."""
    assert bool(torch.isfinite(a[wr]).all()) and bool(torch.isfinite(b[wr]).all()), f"{what}: NaN / inf in a written row"
    assert torch.equal(a[wr], b[wr]), f"{what}: not bit-equal (max difference {float((a[wr].double() - b[wr].double()).abs().max()):.3e})"
    assert bool(R._same(a[~wr], b[~wr]).all()), f"{what}: an unwritten row differs"


@pytest.mark.parametrize("c", H.COVERED, ids=[c.id for c in H.COVERED])
def test_half8_form(dev, c):
    inp, ref, wr = evaluated(c)
    got, rule = launch(dev, c, {"TANTE_FS_HALF8": 1})
    assert rule is not None and rule[2] <= 256, (c.id, rule)
    # the buffer contract and the float64 bars, every figure printed before it is asserted
    untouched = bool(R._same(got[~wr], inp.buf[~wr]).all())
    finite = bool(torch.isfinite(got[wr]).all())
    rel, mx, dl = R.errors(got, ref, inp.buf, wr)
    tok = R.worst_token(got, ref, inp.buf, wr)
    print(f"{c.id} (8 waves, {rule[2]} workgroups): vs float64 rel {rel:.3e} max {mx:.3e} y-x {dl:.3e} worst token {tok:.3e} | "
          f"unwritten rows unchanged {untouched}")
    assert untouched, f"{c.id}: a row the launch does not address changed"
    assert finite, f"{c.id}: NaN / inf in a written row"
    assert rel < R.BAR_L2 and mx < R.BAR_MAX and dl < R.BAR_DELTA and tok < R.BAR_TOKEN, (c.id, rel, mx, dl, tok)
    again, _ = launch(dev, c, {"TANTE_FS_HALF8": 1})
    same_buffer(f"{c.id}: the same launch on a fresh copy", got, again, wr)
    four, rule4 = launch(dev, c, {"TANTE_FS_HALF8": 0})
    assert rule4 is None and R.route(c, {}) in H.HALF4_ROUTES
    same_buffer(f"{c.id}: 8 waves vs the 4-wave 2-tile form (TANTE_FS_HALF8 = 0)", got, four, wr)
    full, rulef = launch(dev, c, {"TANTE_FS_HALF": 0})
    assert rulef is None and R.route(c, {"TANTE_FS_HALF": 0}) not in H.HALF4_ROUTES
    same_buffer(f"{c.id}: 8 waves vs the full-size 4-wave form (TANTE_FS_HALF = 0)", got, full, wr)
    assert reported_options() == H.OPTION_DEFAULTS


@pytest.mark.parametrize("c", H.NOT_COVERED, ids=[c.id for c in H.NOT_COVERED])
def test_shapes_outside_the_rule_take_todays_kernel(dev, c):
    """The option is on and the rule says no: the launch is tante_fs_launch's, the same bits with the option off, and within the bars."""
    inp, ref, wr = evaluated(c)
    on, rule = launch(dev, c, {"TANTE_FS_HALF8": 1})
    assert rule is None and R.route(c, {}) == c.route
    off, _ = launch(dev, c, {"TANTE_FS_HALF8": 0})
    same_buffer(f"{c.id}: TANTE_FS_HALF8 1 vs 0", on, off, wr)
    assert bool(R._same(on[~wr], inp.buf[~wr]).all())
    rel, mx, dl = R.errors(on, ref, inp.buf, wr)
    tok = R.worst_token(on, ref, inp.buf, wr)
    print(f"{c.id} ({c.route}): vs float64 rel {rel:.3e} max {mx:.3e} y-x {dl:.3e} worst token {tok:.3e}")
    assert rel < R.BAR_L2 and mx < R.BAR_MAX and dl < R.BAR_DELTA and tok < R.BAR_TOKEN, (c.id, rel, mx, dl, tok)
    assert reported_options() == H.OPTION_DEFAULTS
