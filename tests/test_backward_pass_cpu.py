"""CPU: the lifecycle of autograd.BackwardPass -- one record and one engine callback per backward pass, the three ways its flush runs,
what a dead pass leaves behind, backward_scope.  No kernel runs: the nodes are tiny Functions on CPU tensors whose backward calls into
tante_amd.autograd as the real nodes do, and the two launch functions are replaced by recorders."""
import contextlib

import pytest
import torch

from tante_amd import autograd as A

M, N, Kk = 64, 128, 128                       # a shape _tr_shape accepts: the use is recorded, not run
USE_BYTES = 2 * M * N * 2                     # the bf16 operands (dy, a) one recorded use keeps alive


class _Node(torch.autograd.Function):
    """Identity whose backward calls fn()."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _loss(*fns):
    """A graph whose backward pass calls fns in the order given."""
    y = torch.zeros(1, requires_grad=True)
    for fn in reversed(fns):
        y = _Node.apply(y, fn)
    return y.sum()


class _World:
    """Weights 0..3 as views of one flat bucket, one fold whose accumulator nothing pending writes, and the launch recorders."""

    def __init__(self, monkeypatch):
        self.bucket = torch.zeros(4 * (N * Kk + N))
        self.gW = [self.bucket[i * (N * Kk + N):][:N * Kk].view(N, Kk) for i in range(4)]
        self.gb = [self.bucket[i * (N * Kk + N) + N * Kk:][:N] for i in range(4)]
        acc = torch.zeros(N * Kk + N)
        z = lambda *s: torch.zeros(*s)
        self.the_fold = A.PendingFold(acc, acc[:N * Kk].view(N, Kk), acc[N * Kk:], z(N, Kk), z(Kk), z(Kk), z(N, Kk), z(N), z(Kk), z(Kk), N, Kk)
        self.log, self.records, self.ends, self.used = [], [], [], []
        index = {w.data_ptr(): i for i, w in enumerate(self.gW)}
        monkeypatch.setattr(A, "_launch_group", lambda grp: self.log.append(("group", [(index[e.gW.data_ptr()], len(e.uses)) for e in grp])))
        monkeypatch.setattr(A, "_launch_folds", lambda folds: self.log.append(("folds", list(folds))) if folds else None)
        real = A._end_of_pass
        monkeypatch.setattr(A, "_end_of_pass", lambda: (self.ends.append(1), real())[1])
        monkeypatch.setattr(A, "DEFER_WGRAD", True)
        monkeypatch.setattr(A, "WGRAD_JOBS", 4)

    def use(self, i):
        """What LinearFn.backward does with a deferrable shape."""
        def fn():
            dy, a = torch.zeros(M, N, dtype=torch.bfloat16), torch.zeros(M, Kk, dtype=torch.bfloat16)
            self.used.append(A._defer_wgrad(self.gW[i], self.gb[i], dy, a, M, N, Kk, A.L.BF16))
        return fn

    def fold(self):
        """What FoldFn.backward does in a pass that deferred (its own slot checks want CUDA gradient slots)."""
        p = A._pass()
        assert p is not None and p.deferred
        p.folds.append(self.the_fold)

    def frame(self):
        """What FilmPosFramesFn.backward does with a frame encoding's accumulator."""
        A._frame_accumulators()[id(self)] = torch.zeros(3)

    def note(self):
        self.records.append(A._pass())


@pytest.fixture
def w(monkeypatch):
    saved = A._PASS, A._SCOPE, dict(A._FOLD_DIRTY)
    A._PASS, A._SCOPE = None, (None, False)
    A._FOLD_DIRTY.clear()
    yield _World(monkeypatch)
    A._PASS, A._SCOPE = saved[:2]
    A._FOLD_DIRTY.clear()
    A._FOLD_DIRTY.update(saved[2])


BOTH = ("group", [(0, 1), (1, 1)])


def test_one_record_per_pass(w):
    _loss(w.note, w.use(0), w.note).backward()
    assert len(w.records) == 2 and w.records[0] is w.records[1] and isinstance(w.records[0], A.BackwardPass)
    assert w.used == [True] and w.log == [("group", [(0, 1)])]
    assert A._PASS is None
    assert A._pass() is None                                     # outside a backward pass: no record ...
    w.use(0)()
    assert w.used == [True, False] and A._PASS is None           # ... and nothing is deferred: nothing would flush it
    _loss(w.note).backward()
    assert w.records[2] is not w.records[0]                      # the next pass gets a record of its own


def test_one_callback_for_deferred_frame_and_side_stream_uses(w, monkeypatch):
    class FakeStream:
        def __init__(self):
            self.waited_for = []

        def wait_stream(self, other):
            self.waited_for.append(other)
    main, side = FakeStream(), FakeStream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: main)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(A, "SIDE_STREAM_WGRAD", True)
    monkeypatch.setattr(A, "_SIDE_STREAM", side)
    in_pass = []

    def side_use():      # what an immediate weight gradient does under TANTE_WGRAD_SIDE_STREAM
        with A._side_wgrad() as s:
            in_pass.append(s.in_pass)
    _loss(w.frame, side_use, w.use(0), w.note, w.use(1), side_use).backward()
    assert w.ends == [1]
    assert in_pass == [True, True] and side.waited_for == [main, main]
    assert main.waited_for == [side]          # joined by the callback, once, not by each use
    assert w.log == [BOTH] and w.records[0].frames == {} and A._PASS is None
    with A._side_wgrad():                     # no pass is running: the use joins at once
        pass
    assert main.waited_for == [side, side] and A._PASS is None


def test_end_of_pass_without_a_driver_launches_groups_then_folds(w):
    A.run_backward(_loss(w.use(0), w.note, w.use(1), w.fold, w.frame))
    assert w.log == [BOTH, ("folds", [w.the_fold])]
    assert w.ends == [1] and w.records[0].frames == {} and A._PASS is None


def test_end_of_pass_calls_the_driver_once_and_launches_nothing_itself(w):
    seen = []

    def driver():
        seen.append((A._PASS, A.flush_plan(w.bucket, 1)))
    A.run_backward(_loss(w.use(0), w.note, w.use(1), w.fold, w.frame), driver=driver)
    half = 2 * (N * Kk + N)
    assert seen == [(w.records[0], ([(half, 2 * half)], [[(0, half)]]))]          # the record is still there for flush_plan
    assert w.log == [] and w.records[0].frames == {} and A._PASS is None
    A.run_backward(_loss(w.use(0), w.use(1), w.fold), driver=lambda: A.flush_run(1))
    assert w.log == [BOTH, ("folds", [w.the_fold])] and A._PASS is None


def test_driver_is_not_called_in_a_pass_that_deferred_nothing(w):
    called = []
    A.run_backward(_loss(w.note, w.frame), driver=lambda: called.append(1))
    assert called == [] and w.ends == [1] and w.log == []
    assert w.records[0].frames == {} and A._PASS is None


def test_hold_keeps_the_record_for_flush_steps(w):
    with A.backward_scope(hold=True):
        _loss(w.use(0), w.note, w.use(1), w.fold, w.frame).backward()
        p = A._PASS
        assert w.log == [] and w.ends == [1]
        assert p is w.records[0] and p.ended and p.frames == {} and len(p.pending) == 2 and p.folds == [w.the_fold]
        assert list(A.flush_steps(1)) == [0]
        assert w.log == [BOTH, ("folds", [w.the_fold])] and A._PASS is None
    assert A._SCOPE == (None, False)


def test_a_dead_pass_is_dropped_not_launched(w):
    def boom():
        raise RuntimeError("injected failure inside backward")
    with pytest.raises(RuntimeError, match="injected"):
        _loss(w.use(0), w.use(1), w.fold, boom).backward()
    dead = A._PASS
    assert dead is not None and len(dead.pending) == 2 and dead.folds == [w.the_fold] and w.ends == [] and w.log == []
    _loss(w.note, w.use(2)).backward()          # the raw call, no scope and no reset
    assert w.records[0] is not dead and w.ends == [1]
    assert w.log == [("group", [(2, 1)])] and A._PASS is None


def test_backward_scope_resets_on_entry_and_on_any_exit(w):
    buf = torch.ones(4)
    A._PASS = A.BackwardPass(-1)
    with pytest.raises(KeyError):
        with A.backward_scope():
            assert A._PASS is None
            A._PASS = A.BackwardPass(-1)
            A._FOLD_DIRTY[id(buf)] = buf
            raise KeyError("the body raises")
    assert A._PASS is None and not A._FOLD_DIRTY and not bool(buf.any())


def test_nested_scope_restores_the_outer_driver(w):
    outer, inner = [], []
    with A.backward_scope(driver=lambda: outer.append(1)):
        with A.backward_scope(driver=lambda: inner.append(1)):
            _loss(w.use(0)).backward()
        assert (outer, inner) == ([], [1])
        _loss(w.use(0)).backward()
        assert (outer, inner) == ([1], [1])
    assert A._SCOPE == (None, False)
    _loss(w.use(0)).backward()
    assert (outer, inner) == ([1], [1]) and w.log == [("group", [(0, 1)])]


def test_reset_zeroes_fold_accumulators_only_after(w):
    buf = torch.ones(4)
    A._FOLD_DIRTY[id(buf)] = buf
    A.reset_backward_state()
    assert bool(buf.all()) and A._FOLD_DIRTY == {id(buf): buf}
    A.reset_backward_state(after=True)
    assert not bool(buf.any()) and not A._FOLD_DIRTY


def test_overflow_in_the_middle_of_a_pass(w, monkeypatch):
    """TANTE_WGRAD_DEFER_MAX_GB at two and a half uses' operands: the third use launches what is recorded so far."""
    monkeypatch.setattr(A, "DEFER_MAX_GB", 2.5 * USE_BYTES / 2 ** 30)
    at_overflow = []

    def look():
        p = A._pass()
        at_overflow.append((list(w.log), dict(p.pending), list(p.folds), p.bytes))
    _loss(w.use(0), w.use(1), w.fold, w.use(2), look, w.use(3)).backward()
    first = ("group", [(0, 1), (1, 1), (2, 1)])
    assert at_overflow == [([first], {}, [w.the_fold], 0)]          # the fold stays queued
    assert w.log == [first, ("group", [(3, 1)]), ("folds", [w.the_fold])]
    assert w.ends == [1] and w.used == [True] * 4 and A._PASS is None
