"""CPU: the host side of the adaptive-step tail (csrc/adaptive_tail.hip) -- the shape rule and its Python mirror, the frame cap, the
argument refusals of the C entries (all of them answer before any launch: there is no GPU here), and which route TANTE.forward and
rollout_adaptive take, with the kernels replaced by recorders."""
import ctypes as Ct
import itertools

import pytest
import torch


def _lib():
    from tante_amd import _lib as L
    from tante_amd.build import build
    build()
    return L.lib()


def test_supported_mirror_equals_the_library():
    from tante_amd import kernels as K
    lib = _lib()
    seen = set()
    for C_, D, HW, n_ord, n_cap in itertools.product((64, 128, 256, 512), (1, 16, 17), (16, 24, 48), (1, 4, 5), (1, 8, 9)):
        Hp, Wp = 4, HW // 4
        want = bool(lib.tante_adaptive_tail_supported(C_, D, Hp, Wp, n_ord, n_cap))
        assert K.adaptive_tail_supported_py(C_, D, Hp, Wp, n_ord, n_cap) is want, (C_, D, HW, n_ord, n_cap)
        assert K.adaptive_tail_supported(C_, D, Hp, Wp, n_ord, n_cap) is want
        seen.add(want)
        assert want == (C_ in (128, 256) and D <= 16 and HW % 16 == 0 and n_ord <= 4 and n_cap <= 8)
    assert seen == {True, False}
    for bad in ((128, 0, 4, 4, 1, 1), (128, 1, 0, 16, 1, 1), (128, 1, 4, 4, 0, 1), (128, 1, 4, 4, 1, 0)):
        assert not lib.tante_adaptive_tail_supported(*bad) and not K.adaptive_tail_supported_py(*bad)


def test_frame_cap_of_out_T():
    """n_cap = floor(out_T - 1 + ep) in the kernel's fp32 arithmetic: fl(1.999f - 1) + fl(1.001f) rounds to 2.0, so 1.999 already allows
    two frames (rollout_adaptive's own threshold for 'one frame per call whatever the sample' is out_T < 1.999)."""
    from tante_amd import kernels as K
    assert [K.adaptive_n_cap(v) for v in (1, 1.5, 1.999, 2, 8, 8.5)] == [1, 1, 2, 2, 8, 8]
    assert K.adaptive_n_cap(9) == 9 and K.adaptive_n_cap(1.99) == 1


def test_sizes():
    lib = _lib()
    for C_ in (128, 256):
        C1, C2 = C_ // 2, C_ // 4
        assert lib.tante_adaptive_rt_stream_bytes(C_) == C1 * C_ * 2 + 1024 + C2 * C1 * 2 + 1024 + 1024
    assert lib.tante_adaptive_ws_bytes(3, 8, 16, 48) == 4 * 3 * (8 * 16 * 48 // 16)
    assert lib.tante_adaptive_ws_bytes(0, 8, 16, 48) == 0
    assert lib.tante_abi_version() == 14


def _err(lib):
    return lib.tante_last_error().decode()


def test_argument_refusals_come_before_any_launch():
    """Every refusal is -1 (argument) or -2 (unsupported shape) with the entry's name in the message; a launch on this machine would
    have answered -3."""
    lib = _lib()
    host = Ct.create_string_buffer(4096)
    a = (Ct.addressof(host) + 63) // 64 * 64
    one = (Ct.c_void_p * 1)(a)
    rt = lambda **k: lib.tante_adaptive_rt(*[k.get(n, d) for n, d in (      # noqa: E731
        ("n_ord", 1), ("rows", one), ("streams", one), ("film", a), ("a_n0", 16), ("a_s1", 0), ("a_s0", 128), ("a_off", 0), ("n_img", 1), ("Hp", 4),
        ("Wp", 4), ("C", 128), ("out_T", 1.5), ("ep", 1.001), ("ws", a), ("ws_bytes", 4), ("r", a), ("R", a), ("count", a), ("fa", a), ("fs", a),
        ("stream", None))])
    assert rt(rows=None) == -1 and "tante_adaptive_rt: null pointer" in _err(lib)
    assert rt(count=None) == -1 and "tante_adaptive_rt: null pointer" in _err(lib)
    assert rt(C=64) == -2 and "tante_adaptive_rt: unsupported" in _err(lib)
    assert rt(Wp=6) == -2 and "tante_adaptive_rt: unsupported" in _err(lib)
    assert rt(n_ord=5) == -2 and "tante_adaptive_rt: unsupported" in _err(lib)
    assert rt(n_img=0) == -1 and "tante_adaptive_rt: bad shape" in _err(lib)
    assert rt(a_n0=24) == -1 and "tante_adaptive_rt: row addressing" in _err(lib)
    assert rt(a_s0=130) == -1 and "tante_adaptive_rt: row addressing" in _err(lib)
    assert rt(ws_bytes=0) == -1 and "tante_adaptive_rt: workspace" in _err(lib)
    assert rt(fa=a + 4) == -1 and "tante_adaptive_rt: alignment" in _err(lib)
    assert rt(rows=(Ct.c_void_p * 1)(a + 4)) == -1 and "tante_adaptive_rt: order 0" in _err(lib)
    hd = lambda **k: lib.tante_head_adaptive(*[k.get(n, d) for n, d in (      # noqa: E731
        ("n_ord", 1), ("rows", one), ("streams", one), ("a_n0", 16), ("a_s1", 0), ("a_s0", 128), ("a_off", 0), ("n_img", 1), ("Hp", 4), ("Wp", 4),
        ("C", 128), ("D", 1), ("fa", a), ("fs", a), ("count", a), ("rule", 0), ("coefs", a), ("n_cap", 1), ("out", a), ("out_bstride", 1024),
        ("last", a), ("last_bstride", 1024), ("stream", None))])
    assert hd(out=None) == -1 and "tante_head_adaptive: null pointer" in _err(lib)
    assert hd(count=None) == -1 and "tante_head_adaptive: null pointer" in _err(lib)
    assert hd(n_cap=9) == -2 and "tante_head_adaptive: unsupported" in _err(lib)
    assert hd(D=17) == -2 and "tante_head_adaptive: unsupported" in _err(lib)
    assert hd(C=512) == -2 and "tante_head_adaptive: unsupported" in _err(lib)
    assert hd(rule=2) == -1 and "tante_head_adaptive: bad shape" in _err(lib)
    assert hd(a_off=2) == -1 and "tante_head_adaptive: row addressing" in _err(lib)
    assert hd(out=a + 8) == -1 and "tante_head_adaptive: alignment" in _err(lib)
    assert hd(out_bstride=1022) == -1 and "tante_head_adaptive: alignment" in _err(lib)
    assert hd(streams=(Ct.c_void_p * 1)(None)) == -1 and "tante_head_adaptive: order 0" in _err(lib)
    assert lib.tante_pack_adaptive_rt(None, a, a, a, a, a, 128, a, None) == -1 and "tante_pack_adaptive_rt: null pointer" in _err(lib)
    assert lib.tante_pack_adaptive_rt(a, a, a, a, a, a, 64, a, None) == -2 and "tante_pack_adaptive_rt: unsupported" in _err(lib)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from tante_amd import kernels as K
    _lib()
    x = torch.zeros(16, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.adaptive_rt([x], 16, 0, 128, 0, 1, 4, 4, 128, [torch.zeros(8, dtype=torch.uint8)], torch.zeros(8), 1.5, 1.001)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.head_adaptive([x], 16, 0, 128, 0, 1, 4, 4, 128, 1, [torch.zeros(8, dtype=torch.uint8)], x, x, torch.zeros(1, dtype=torch.int32), False,
                        torch.zeros(8), 1, torch.zeros(1, 1, 1, 32, 32), 1024, torch.zeros(1, 1, 32, 32), 0, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.pack_adaptive_rt([torch.zeros(1)] * 6, 128)


# ---- route decisions, kernels stubbed -----------------------------------------------------------------------------------------------
class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the host code's device checks pass and every kernel wrapper below is a recorder."""

    @property
    def is_cuda(self):
        return True


def _model(C_=128, nh=4, **kw):
    import tante_amd
    torch.manual_seed(0)
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(32, 32))
    args = dict(in_T=4, dset_metadata=md, taylor_order=2, attn_axes="T-H", n_head=nh, embed_dim=C_, patch_scale=8, dropout=0.0, deg=False)
    args.update(kw)
    return tante_amd.TANTE(**args).eval().set_compute("bf16")


def test_adaptive_tail_route_predicate():
    import tante_amd
    _lib()
    m = _model()
    assert m.adaptive_tail_route(1.5) and m.adaptive_tail_route(6.0) and m.adaptive_tail_route(8.5)
    assert not m.adaptive_tail_route(9.0)                                   # n_cap = 9
    assert not _model().set_compute("fp32").adaptive_tail_route(1.5)
    assert not _model(32, 2).adaptive_tail_route(1.5)                       # a width the kernels do not serve
    assert not _model(deg=True).adaptive_tail_route(1.5)
    assert not _model(taylor_order=5, attn_axes="T-T-T-T-T").adaptive_tail_route(1.5)
    assert "TANTE_ADAPTIVE_TAIL" in tante_amd.options.host_options() and tante_amd.get_option("TANTE_ADAPTIVE_TAIL") is True
    tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 0)
    try:
        assert tante_amd.tante.ADAPTIVE_TAIL is False and not m.adaptive_tail_route(1.5)
    finally:
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
    assert not m.enc_cache_supported()          # deg=False: only for a stated out_T on the route


class _Stubs:
    """Recorders for every kernel wrapper a deg=False inference call reaches on either route."""

    def __init__(self, mp, counts):
        from tante_amd import kernels as K, tante as TT
        from tante_amd.attn_backbone import Attn_Backbone
        self.log, self.counts = [], counts
        B = len(counts)

        def rec(name, ret=None):
            def f(*a, **k):
                self.log.append((name, a, k))
                return ret(*a, **k) if callable(ret) else ret
            return f
        mp.setattr(K, "film_table", rec("film_table", lambda t, p, C_, add: (torch.zeros(t.numel(), C_), torch.zeros(t.numel(), C_))))
        mp.setattr(TT.enc_CNN, "forward_tokens", rec("encoder", lambda self_, inp, *a, **k: torch.zeros(inp.shape[0] * inp.shape[1] * 16, self_.embed_dim)))
        mp.setattr(Attn_Backbone, "forward_tokens", rec("backbone"))
        for n in ("pack_adaptive_rt", "pack_adaptive_film", "pack_head", "pack_weight"):
            mp.setattr(K, n, rec(n, lambda *a, **k: torch.zeros(1)))

        def adaptive_rt(rows, a_n0, a_s1, a_s0, a_off, n_img, Hp, Wp, C_, streams, film, out_T, ep):
            n = len(rows)
            return (torch.ones(n, n_img), torch.tensor([float(c) + 0.5 for c in counts]), torch.tensor(counts, dtype=torch.int32),
                    torch.zeros(n, n_img, C_), torch.zeros(n, n_img, C_))
        mp.setattr(K, "adaptive_rt", rec("adaptive_rt", adaptive_rt))
        mp.setattr(K, "head_adaptive", rec("head_adaptive"))
        mp.setattr(K, "linear", rec("linear"))
        mp.setattr(K, "rt_reduce", rec("rt_reduce", lambda t, Bq, Lq, out_T, ep: torch.tensor([float(c) + 0.5 for c in counts])))
        mp.setattr(K, "film_apply", rec("film_apply"))
        mp.setattr(K, "head_fused", rec("head_fused"))
        self.B = B

    def names(self):
        return [e[0] for e in self.log]


def test_forward_route_with_stubbed_kernels(monkeypatch):
    """The new route: backbones, then adaptive_rt and head_adaptive once each and nothing of the old tail; the frame count comes from the
    device counts (sample 0's, or the largest with per_sample_counts); out= is the returned storage.  Switch off: the old launches, and
    out= / enc_cache= raise as they always did."""
    import tante_amd
    _lib()
    m = _model()
    st = _Stubs(monkeypatch, [2, 3])
    x = torch.zeros(2, 4, 1, 32, 32).as_subclass(_OnGpu)
    old_tail = {"linear", "rt_reduce", "film_apply", "head_fused"}
    with torch.no_grad():
        y, rt = m(x, 6.0)
        assert y.shape == (2, 2, 1, 32, 32) and rt.shape == (2,)
        names = st.names()
        assert names.count("adaptive_rt") == 1 and names.count("head_adaptive") == 1 and names.count("backbone") == 2
        assert not old_tail & set(names) and names.index("adaptive_rt") < names.index("head_adaptive")
        assert all(names.index(n) < names.index("adaptive_rt") for n in ("backbone", "encoder"))
        head = [e for e in st.log if e[0] == "head_adaptive"][0][1]
        assert head[14] is False and head[16] == 6 and tuple(head[17].shape) == (2, 6, 1, 32, 32)      # rule 0, n_cap, the out buffer
        rows = [e for e in st.log if e[0] == "adaptive_rt"][0][1][0]
        assert len(rows) == 2 and all(tuple(r.shape) == (2 * 16, 128) for r in rows)      # 4 x 4 planes: dense copies of the last-slot rows
        st.log.clear()
        y, _ = m(x, 6.0, per_sample_counts=True)
        assert y.shape[1] == 3 and [e for e in st.log if e[0] == "head_adaptive"][0][1][14] is True
        buf = torch.zeros(2, 10, 1, 32, 32).as_subclass(_OnGpu)
        y, _ = m(x, 6.0, out=buf[:, 2:8])
        assert y.data_ptr() == buf[:, 2:].data_ptr() and y.shape[1] == 2
        with pytest.raises(ValueError, match="out must be"):
            m(x, 6.0, out=buf[:, 2:7])
        with pytest.raises(RuntimeError, match="enc_next"):
            m(x, 6.0, enc_next=torch.zeros(2, 16, 128).as_subclass(_OnGpu))
        st.log.clear()
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 0)
        try:
            y, rt = m(x, 6.0)
            names = st.names()
            assert y.shape == (2, 2, 1, 32, 32)
            assert "adaptive_rt" not in names and "head_adaptive" not in names
            assert names.count("linear") == 6 and names.count("rt_reduce") == 2 and names.count("film_apply") == 2 and names.count("head_fused") == 2
            with pytest.raises(ValueError, match="out= is only meaningful"):
                m(x, 6.0, out=buf[:, 2:8])
            with pytest.raises(RuntimeError, match="enc_cache"):
                m(x, 6.0, enc_cache=(torch.zeros(4, 2, 16, 128), 2 * 16 * 128, 16 * 128))
        finally:
            tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
        st.log.clear()
        m.set_compute("fp32")
        with pytest.raises(ValueError, match="out= is only meaningful"):
            m(x, 6.0, out=buf[:, 2:8])
        assert "adaptive_rt" not in st.names()


def test_rollout_route_with_a_stubbed_model(monkeypatch):
    """rollout_adaptive runs in place exactly when the model takes the adaptive tail, the rule is sample 0's and there is no autograd; the
    in-place loop advances by what each call returned, reads its window and writes its frames inside ONE buffer."""
    import tante_amd
    from tante_amd import rollout as R
    _lib()
    m = _model()
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(32, 32))
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    batch = {"input": torch.randn(2, 4, 32, 32, 1).as_subclass(_OnGpu), "output": torch.zeros(2, 7, 32, 32, 1)}
    calls = []
    plan = iter([3, 1, 2, 6])

    def forward(self, inp, out_T=1, out=None, enc_cache=None, per_sample_counts=False, **k):
        n = next(plan)
        calls.append((inp.data_ptr(), inp.storage_offset(), None if out is None else (out.storage_offset(), out.shape[1]), enc_cache is not None, n))
        if out is None:
            out = torch.zeros(inp.shape[0], 6, *inp.shape[2:])
        out[:] = -1.0                               # whatever the slots past the count hold is not a frame
        out[:, :n] = float(len(calls))
        return out[:, :n], torch.full((inp.shape[0],), n + 0.5)
    encoded = []
    monkeypatch.setattr(tante_amd.TANTE, "forward", forward)
    monkeypatch.setattr(tante_amd.TANTE, "enc_cache_supported", lambda self, out_T=None: out_T is not None)
    monkeypatch.setattr(tante_amd.TANTE, "encode_frames", lambda self, frames, z: encoded.append((frames.shape[1], z.shape[0])))
    with torch.no_grad():
        y, y_ref, rts = tante_amd.rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=False)
    assert y.shape == (2, 7, 32, 32, 1) and rts.shape == (8,) and y_ref.shape == (2, 7, 32, 32, 1)
    frame = 32 * 32
    # one buffer of T + n_steps + n_cap - 1 = 16 frames; pos = 0, 3, 4, 6; each call writes n_cap = 6 slots behind its window
    assert [c[1] for c in calls] == [0, 3 * frame, 4 * frame, 6 * frame] and len({c[0] - 4 * c[1] for c in calls}) == 1
    assert [c[2] for c in calls] == [(4 * frame, 6), (7 * frame, 6), (8 * frame, 6), (10 * frame, 6)]
    assert [c[4] for c in calls] == [3, 1, 2, 6] and all(c[3] for c in calls)
    assert encoded == [(4, 4), (3, 3), (1, 1), (2, 2)]      # the window once, then only what each call added: every frame encoded once
    assert y[0, :, 0, 0, 0].tolist() == [1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 4.0]      # frames past a call's count were overwritten by the next call
    # not in place: the switch off, the per-sample rule at an out_T where the samples differ, autograd
    seen = []
    monkeypatch.setattr(R, "_rollout_adaptive_in_place", lambda *a: seen.append(a) or (torch.zeros(2, 7, 1, 32, 32), torch.zeros(2)))
    with torch.no_grad():
        tante_amd.rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=False)
        tante_amd.rollout_adaptive(m, batch, fmt, 7, 1.5, per_sample=True)      # every sample one frame per call: runs as one batch
    assert len(seen) == 2
    plan = iter([6] * 64)
    tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 0)
    try:
        with torch.no_grad():
            tante_amd.rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=False)
    finally:
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
    with torch.no_grad():
        tante_amd.rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=True)
        tante_amd.rollout_adaptive(m, batch, fmt, 7, 9.0, per_sample=False)
    tante_amd.rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=False)          # autograd on
    assert len(seen) == 2
