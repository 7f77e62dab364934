"""CPU: which kernels an inference call and a rollout take, with every kernel wrapper replaced by a recorder (the pattern of
test_adaptive_tail_cpu.py).  The launch-order tests drive the public surface only -- model(x, ...), rollout_model, set_option -- and
their literals are what the code did before the route record existed; the record tests hold tante_amd.route to the same table."""
import contextlib

import pytest
import torch

T, DT = 4, 1.0
THIRDS = [1.0, 0.5, 1.0 / 6.0]      # dt^(k+1) / (k+1)! at dt = 1


def _lib():
    from tante_amd import _lib as L
    from tante_amd.build import build
    build()
    return L.lib()


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the host code's device checks pass and every kernel wrapper below is a recorder."""

    @property
    def is_cuda(self):
        return True


def _gpu(t):
    return None if t is None else t.as_subclass(_OnGpu)


@contextlib.contextmanager
def _options(**kw):
    import tante_amd
    old = {k: tante_amd.get_option(k) for k in kw}
    for k, v in kw.items():
        tante_amd.set_option(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            tante_amd.set_option(k, int(v))


# name -> (constructor arguments over the defaults below, compute mode)
CASES = {
    "order1": (dict(), "bf16"),
    "order3": (dict(taylor_order=3, attn_axes="THW-THW-THW", res=128), "bf16"),
    "order2_c128": (dict(taylor_order=2, attn_axes="T-H", embed_dim=128), "bf16"),
    "two_frames_c128": (dict(taylor_order=2, attn_axes="T-H", embed_dim=128, output_length=2), "bf16"),
    "order1_fp32": (dict(), "fp32"),
    "order3_fp32": (dict(taylor_order=3, attn_axes="THW-THW-THW", res=128), "fp32"),
    "patch16": (dict(patch_scale=16), "bf16"),
    "order1_128": (dict(res=128), "bf16"),
}


def _model(case):
    import tante_amd
    kw, mode = CASES[case]
    kw = dict(kw)
    res = kw.pop("res", 32)
    torch.manual_seed(0)
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(res, res))
    args = dict(in_T=T, dset_metadata=md, taylor_order=1, attn_axes="THW", n_head=8, embed_dim=256, patch_scale=8, dropout=0.0)
    args.update(kw)
    return tante_amd.TANTE(**args).eval().set_compute(mode), res, md


class _Stubs:
    """Recorders for every kernel wrapper and sub-module a deg=True inference call or rollout reaches.  An entry is (name, salient
    arguments...); run() gives a call's launch order without the weight packs and the FiLM table."""

    def __init__(self, mp, B):
        from tante_amd import _lib as L, kernels as K, tante as TT
        from tante_amd.attn_backbone import Attn_Backbone
        self.log, self.B = [], B
        streams = set()       # the buffers the backbones of the running call wrote

        def kinds(rows):      # a head's rows: those token streams (read at slot T - 1 by stride) or dense copies of the slot's rows
            assert len({r.data_ptr() for r in rows}) == len(rows)
            return tuple("stream" if r.data_ptr() in streams else "copy" for r in rows)

        def encoder(self_, inp, compute, film, *a, **k):
            self.log.append(("encoder",))
            return torch.zeros(inp.shape[0] * inp.shape[1] * self_.patch_shape[0] * self_.patch_shape[1], self_.embed_dim)

        def backbone(self_, x, Bq, compute, film_src=None, x_in=None, film_frames=None, last_slot_only=False):
            self.log.append(("backbone", "oop" if x_in is not None else "cache" if film_src is not None else "in_place", bool(last_slot_only)))
            assert film_frames is None and Bq == B
            streams.add(x.data_ptr())
            return x

        def head_enc_fused(rows, a_n0, a_s1, a_s0, a_off, *a, enc_stream=None, z=None):
            assert (enc_stream is None) == (z is None) and a_s1 == T * a_n0 * a_s0 and a_off == (T - 1) * a_n0 * a_s0
            self.log.append(("head_enc_fused", kinds(rows), list(a[6]), z is not None))

        def head_fused_multi(rows, a_n0, a_s1, a_s0, a_off, *a, streams):
            self.log.append(("head_fused_multi", kinds(rows), list(a[6]), streams))

        def head_fused(x, a_n0, a_s1, a_s0, a_off, Bq, Hp, Wp, C_, D, stream, out, out_bstride, coefs, last, *a):
            self.log.append(("head_fused", kinds([x])[0], list(coefs), last is not None))

        def decoder(self_, src, n_img, compute, *a, **k):
            self.log.append(("decoder",))
            return torch.zeros(n_img, self_.chans[3], self_.H, self_.W)

        def taylor(last, off, bstride, derivs, dt, n_out, out, *a, **k):
            self.log.append(("taylor", len(derivs), n_out))

        def frames(self_, inp, compute, item_stride, z):
            self.log.append(("encode_frames", inp.shape[1]))
            return z

        def window_raw(self_, raw, compute, z, frame_out):
            self.log.append(("window_raw", z.shape[0]))
            return z

        def format_input(*a):
            self.log.append(("format_input",))
            return 0

        def rec(name, ret=None):
            def f(*a, **k):
                self.log.append((name,))
                return ret(*a, **k) if callable(ret) else ret
            return f
        mp.setattr(K, "film_table", rec("film_table", lambda t, p, C_, add: (torch.zeros(t.numel(), C_), torch.zeros(t.numel(), C_))))
        for n in ("pack_head", "pack_head_enc", "pack_weight", "pack_enc23", "pack_enc1_raw"):
            mp.setattr(K, n, rec(n, lambda *a, **k: torch.zeros(1)))
        mp.setattr(K, "_stream", lambda: None)
        mp.setattr(TT.enc_CNN, "forward_tokens", encoder)
        mp.setattr(TT.enc_CNN, "forward_frames", frames)
        mp.setattr(TT.enc_CNN, "forward_window_raw", window_raw)
        mp.setattr(TT.dec_CNN, "forward_tokens", decoder)
        mp.setattr(Attn_Backbone, "forward_tokens", backbone)
        mp.setattr(K, "head_enc_fused", head_enc_fused)
        mp.setattr(K, "head_fused_multi", head_fused_multi)
        mp.setattr(K, "head_fused", head_fused)
        mp.setattr(K, "taylor", taylor)
        mp.setattr(L.lib(), "tante_format_input", format_input)
        # the rollout's buffers come from torch.empty: the model call sees them as GPU tensors, and the call's arguments are recorded
        forward = TT.TANTE.forward

        def call(self_, inp, out_T=1, out=None, enc_cache=None, enc_next=None, **k):
            self.log.append(("call", enc_cache is not None, enc_next is not None))
            streams.clear()
            return forward(self_, _gpu(inp), out_T, out=_gpu(out), enc_cache=enc_cache, enc_next=_gpu(enc_next), **k)
        mp.setattr(TT.TANTE, "forward", call)

    def run(self, m, res):
        self.log.clear()
        with torch.no_grad():
            y = m(torch.zeros(self.B, T, 1, res, res).as_subclass(_OnGpu))
        assert y.shape == (self.B, m.output_length, 1, res, res)
        return [e for e in self.log if not e[0].startswith("pack_") and e[0] not in ("call", "film_table")]


def test_fixed_step_call_launch_order(monkeypatch):
    _lib()
    st = _Stubs(monkeypatch, 2)
    bb = lambda *flags: [("backbone", how, ls) for how, ls in flags]      # noqa: E731
    m, res, _ = _model("order1")
    st.log.clear()
    with torch.no_grad():
        m(torch.zeros(2, T, 1, res, res).as_subclass(_OnGpu))
    assert [e[0] for e in st.log] == ["call", "film_table", "encoder", "backbone", "pack_head", "head_enc_fused"]      # the tables first
    assert st.run(m, res) == [("encoder",), ("backbone", "in_place", True), ("head_enc_fused", ("stream",), [1.0], False)]
    m, res, _ = _model("order3")
    three = [("encoder",)] + bb(("in_place", False), ("oop", False), ("oop", True))
    assert st.run(m, res) == three + [("head_enc_fused", ("stream",) * 3, THIRDS, False)]
    with _options(TANTE_HEAD_ENC=0):
        assert st.run(m, res) == three + [("head_fused_multi", ("stream",) * 3, THIRDS, True)]
        with _options(TANTE_HEAD_STREAMS=0):
            assert st.run(m, res) == [("encoder",)] + bb(("in_place", False), ("in_place", False), ("in_place", True)) + [
                ("head_fused_multi", ("copy", "copy", "stream"), THIRDS, False)]
        with _options(TANTE_HEAD_MULTI=0):
            assert st.run(m, res) == [("encoder",), ("backbone", "in_place", False), ("head_fused", "stream", [1.0], True),
                                      ("backbone", "in_place", False), ("head_fused", "stream", [0.5], False),
                                      ("backbone", "in_place", False), ("head_fused", "stream", [1.0 / 6.0], False)]
    with _options(TANTE_LAST_SLOT=0):
        assert st.run(m, res) == [("encoder",)] + bb(("in_place", False), ("oop", False), ("oop", False)) + [
            ("head_enc_fused", ("stream",) * 3, THIRDS, False)]
    m, res, _ = _model("order2_c128")      # 4 x 4 planes have no out-of-place propagator: copied rows
    assert st.run(m, res) == [("encoder",)] + bb(("in_place", False), ("in_place", True)) + [
        ("head_fused_multi", ("copy", "stream"), [1.0, 0.5], False)]
    m, res, _ = _model("two_frames_c128")
    assert st.run(m, res) == [("encoder",), ("backbone", "in_place", False), ("head_fused", "stream", [1.0, 2.0], True),
                              ("backbone", "in_place", False), ("head_fused", "stream", [0.5, 2.0], False)]
    for case, n in (("order1_fp32", 1), ("order3_fp32", 3), ("patch16", 1)):
        m, res, _ = _model(case)
        assert st.run(m, res) == [("encoder",)] + [("backbone", "in_place", False), ("decoder",)] * n + [("taylor", n, 1)], case


def _rollout(st, m, res, md, n_steps=3):
    import tante_amd
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    batch = {"input": torch.randn(2, T, res, res, 1).as_subclass(_OnGpu), "output": torch.zeros(2, n_steps, res, res, 1)}
    st.log.clear()
    with torch.no_grad():
        y, y_ref = tante_amd.rollout_model(m, batch, fmt, n_steps)
    assert y.shape == (2, n_steps, res, res, 1) and y_ref.shape == y.shape
    return [e for e in st.log if not e[0].startswith("pack_") and e[0] != "film_table"]


def test_rollout_launch_order(monkeypatch):
    _lib()
    st = _Stubs(monkeypatch, 2)
    m, res, md = _model("order1_128")

    def call(enc_next, encoder=False):
        src = [("call", False, False), ("encoder",), ("backbone", "in_place", True)] if encoder else \
            [("call", True, enc_next), ("backbone", "cache", True)]
        return src + [("head_enc_fused", ("stream",), [1.0], enc_next)]
    # raw first window, every frame encoded once, the tail launch encodes the predicted frame for every call but the last
    assert _rollout(st, m, res, md) == [("window_raw", T)] + call(True) + call(True) + call(False)
    with _options(TANTE_RAW_ENCODE=0):
        assert _rollout(st, m, res, md) == [("format_input",), ("encode_frames", T)] + call(True) + call(True) + call(False)
    with _options(TANTE_NO_TAIL_ENC=1):
        assert _rollout(st, m, res, md) == [("window_raw", T)] + call(False) + [("encode_frames", 1)] + call(False) + [
            ("encode_frames", 1)] + call(False)
    with _options(TANTE_NO_ENC_CACHE=1):
        assert _rollout(st, m, res, md) == [("format_input",)] + call(False, True) * 3
    with _options(TANTE_NO_FUSED_FORMAT=1):      # the formatter's own pass, then the same loop on the copied window
        assert _rollout(st, m, res, md) == [("encode_frames", T)] + call(True) + call(True) + call(False)


# ---- the record -----------------------------------------------------------------------------------------------------------------------
# case -> (Route of model(x), public predicates: tail_fused_supported, enc_cache_supported, encoder.fuses_23, encoder.raw_window_supported,
#          blocks[0].takes_x_in)
ROUTES = {
    "order1": (("encoder", "head_enc", True, True, 0, True), (True, True, True, True, False)),
    "order3": (("encoder", "head_enc", True, True, 0, True), (True, True, True, True, True)),
    "order2_c128": (("encoder", "head_multi", False, True, 0, True), (False, False, False, False, False)),
    "two_frames_c128": (("encoder", "head_per_order", False, False, 0, True), (False, False, False, False, False)),
    "order1_fp32": (("encoder", "decoders", False, False, 0, False), (False, False, False, False, False)),
    "order3_fp32": (("encoder", "decoders", False, False, 0, False), (False, False, False, False, False)),
    "patch16": (("encoder", "decoders", False, False, 0, False), (False, False, False, False, False)),
    "order1_128": (("encoder", "head_enc", True, True, 0, True), (True, True, True, True, True)),
}


def _predicates(m):
    from tante_amd.attn_backbone import resolve_compute
    c = resolve_compute(m.compute)
    return (m.tail_fused_supported(), m.enc_cache_supported(), m.encoder.fuses_23(c), m.encoder.raw_window_supported(c),
            m.blocks[0].takes_x_in(c))


@pytest.mark.parametrize("case", sorted(CASES))
def test_public_predicates(case):
    """These answers do not depend on the route record: the same literals hold before and after it."""
    _lib()
    m, _, _ = _model(case)
    assert _predicates(m) == ROUTES[case][1]
    assert not m.adaptive_tail_route(1.5)      # deg=True


@pytest.mark.parametrize("case", sorted(CASES))
def test_route_record(case):
    from tante_amd.route import Route
    _lib()
    m, _, _ = _model(case)
    with torch.no_grad():
        assert m.route(B=2) == Route(*ROUTES[case][0])
        if ROUTES[case][1][1]:
            assert m.route(enc_cache=True, B=2) == Route(*ROUTES[case][0])._replace(source="cache_fused")
    if ROUTES[case][0][3]:      # the last-slot form is an inference form: with autograd on the whole stream is finished
        assert m.route(B=2) == Route(*ROUTES[case][0])._replace(last_slot=False)


def test_route_record_under_the_switches():
    from tante_amd.route import Route
    _lib()
    m, _, _ = _model("order3")
    with torch.no_grad():
        with _options(TANTE_HEAD_ENC=0):
            assert m.route() == Route("encoder", "head_multi", True, True, 0, True) and not m.tail_fused_supported()
            with _options(TANTE_HEAD_STREAMS=0):
                assert m.route() == Route("encoder", "head_multi", False, True, 0, True)
            with _options(TANTE_HEAD_MULTI=0):
                assert m.route() == Route("encoder", "head_per_order", False, False, 0, True)
        with _options(TANTE_LAST_SLOT=0):
            assert m.route() == Route("encoder", "head_enc", True, False, 0, True)
        m.fused_head = False
        assert m.route() == Route("encoder", "decoders", False, False, 0, False)


def test_adaptive_route_record():
    """deg=False, the model of test_adaptive_tail_cpu.py: the adaptive tail with its frame cap, and the unfused chain it replaces."""
    import tante_amd
    from tante_amd.route import Route
    _lib()
    torch.manual_seed(0)
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(32, 32))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=2, attn_axes="T-H", n_head=4, embed_dim=128, patch_scale=8, dropout=0.0,
                        deg=False).eval().set_compute("bf16")
    with torch.no_grad():
        assert m.route(6.0) == Route("encoder", "adaptive", False, False, 6, True) and m.route(1.5).n_cap == 1
        assert m.route(9.0) == Route("encoder", "unfused", False, False, 0, True)
        assert m.adaptive_tail_route(6.0) and not m.adaptive_tail_route(9.0) and not m.enc_cache_supported(6.0) and not m.enc_cache_supported()
        with _options(TANTE_ADAPTIVE_TAIL=0):
            assert m.route(6.0) == Route("encoder", "unfused", False, False, 0, True)
        for kw in (dict(enc_cache=True), dict(enc_next=True)):
            with pytest.raises(RuntimeError, match=next(iter(kw))):
                m.route(6.0, **kw)
        assert m.set_compute("fp32").route(6.0) == Route("encoder", "unfused", False, False, 0, False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_and_rollout_cannot_disagree(case):
    """Whatever the rollout plans to pass -- enc_cache, enc_next -- the call's route accepts, and what it plans not to pass under the
    default switches the route refuses: both read the same helpers."""
    from tante_amd import rollout as R
    from tante_amd.route import RolloutRoute
    _lib()
    m, res, _ = _model(case)
    raw = torch.zeros(2, T, res, res, 1)

    def accepts(**kw):
        try:
            m.route(B=2, **kw)
            return True
        except RuntimeError:
            return False
    with torch.no_grad():
        plan = R._plan(m, raw)
        cache = ROUTES[case][1][1]
        assert plan == RolloutRoute("raw" if cache else "format", cache, cache and ROUTES[case][1][0])
        assert plan.cache == accepts(enc_cache=True) and plan.tail_enc == accepts(enc_cache=plan.cache, enc_next=True)
        assert R._plan(m, None) == plan._replace(first="copy")
        for off in ("TANTE_NO_ENC_CACHE", "TANTE_NO_TAIL_ENC", "TANTE_NO_FUSED_FORMAT"):
            with _options(**{off: 1}):
                p = R._plan(m, raw)
                assert accepts(enc_cache=p.cache, enc_next=p.tail_enc)
                assert p.first == ("copy" if off == "TANTE_NO_FUSED_FORMAT" else "format" if off == "TANTE_NO_ENC_CACHE" or not cache else "raw")
        with _options(TANTE_RAW_ENCODE=0):
            assert R._plan(m, raw) == plan._replace(first="format")
