"""The head and encoder kernels alone, against float64 and per token: tante_head_fused, tante_head_fused_multi, tante_head_fused_multi_streams
(csrc/head_fused.hip), tante_head_enc_fused (csrc/head_enc.hip), tante_enc23_fused and tante_enc23_frames (csrc/enc_fused.hip).

The cases, their float64 references, the exact-bf16 evaluation and the restated dispatch live in tests/tail_enc_ref.py;
tests/test_tail_enc_cpu.py pins them to the oracle, to the text of the three sources and to planted faults without a GPU.  Here every case
packs its weights with pack_head / pack_head_enc / pack_enc23, sets its launch form through the library option (TANTE_HEAD_WAVES,
TANTE_ENC23_SPLIT; restored in a `finally`), asserts the restated route from the option the library reports, and calls the kernel through
tante_amd.kernels on real pointers: token streams that are NaN outside the addressed rows, output buffers that are longer than what is
written and NaN there (frames past n_out inside out_bstride, the slack of `last`, the tail of z and of the frame-major cache).

Bars against float64: the project's bf16 bars over the whole tensor (relative L2 1e-2, max 2e-2) and the same 1e-2 on EVERY token's own
block against that block's reference norm (no token is left out).  The head figures are taken on the derivative part out - base, never on
out; z of head_enc is held to the float64 encoder of the frame the kernel itself wrote.  The distance to the exact-bf16 evaluation is
recorded without a bar: it is the kernel's own share of the error.  Bit equalities (torch.equal): the 4- and 8-wave forms of every head
kernel (a wave's arithmetic on its 16 tokens does not depend on the group size -- head_enc.hip included: TT = 1 in both forms, and the
reducing workgroup runs stage 3 per wave over the four taps in the fixed order 0..3), dense copies against whole streams, the head_enc
frame against the multi_streams frame (n_ord >= 2) and with against without encoding, every split of enc23, enc23_frames against
enc23_fused under identity FiLM, and a repeated head_enc launch on the same workspace (its arrival counters are back at zero).

The worst figures per kernel go to tail_enc_parity.json beside parity_report.json (profiles/tail_enc_parity.json is one such run)."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

import tail_enc_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

FIGURES = {}        # kernel -> worst figures of this run
EQUALITIES = {}     # name -> held
ROUTES_RUN = set()
CASES_RUN = set()
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    try:
        with open(os.path.join(ROOT, "tail_enc_parity.json"), "w") as f:
            json.dump({"bars": {"whole tensor rel L2": R.BAR_L2, "whole tensor max": R.BAR_MAX, "per token rel L2": R.BAR_TOKEN},
                       "kernels": FIGURES, "bit_equalities": EQUALITIES, "routes_run": sorted(ROUTES_RUN)}, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _ops():
    from tante_amd import kernels as K, _lib as L
    return K, L


@contextlib.contextmanager
def option(name, value):
    """One library option for the launches inside; the earlier value comes back whatever happens."""
    _, L = _ops()
    prev = L.get_option(name, 0)
    L.set_option(name, value)
    try:
        assert L.get_option(name, 0) == value
        yield
    finally:
        L.set_option(name, prev)


_EVAL = {}


def evaluated(c):
    """A case's inputs, float64 reference and exact-bf16 evaluation: computed once, shared, never modified."""
    if c.id not in _EVAL:
        if isinstance(c, R.Enc23Case):
            inp = R.make_enc23_inputs(c)
            e = {"inp": inp}
            for form in ("film", "frames", "rows"):
                e[form] = (R.enc23_reference(c, inp, form), R.enc23_reference(c, inp, form, exact_bf16=True))
        else:
            inp = R.make_head_inputs(c)
            e = {"inp": inp, "ref": R.head_reference(c, inp), "bf": R.head_reference(c, inp, exact_bf16=True), "base": R.head_base_blocks(c, inp)}
        _EVAL[c.id] = e
    return _EVAL[c.id]


def hold(kernel, what, got, ref, ref_bf):
    """The bars of one result, every figure printed and recorded before it is asserted."""
    rel, mx = R.errors(got, ref)
    tok = R.worst_token(got, ref)
    rel2, mx2 = R.errors(got, ref_bf)
    tok2 = R.worst_token(got, ref_bf)
    print(f"{what}: vs float64 rel {rel:.3e} max {mx:.3e} worst token {tok:.3e} | vs exact bf16 rel {rel2:.3e} max {mx2:.3e} worst token {tok2:.3e}")
    record_parity(rel, mx, R.BAR_L2, "bf16", f"{what}: whole tensor")
    record_parity(tok, mx, R.BAR_TOKEN, "bf16", f"{what}: worst token")
    w = FIGURES.setdefault(kernel, {"vs float64": {"rel": 0.0, "max": 0.0, "worst token": 0.0},
                                    "vs exact bf16 (recorded)": {"rel": 0.0, "max": 0.0, "worst token": 0.0}, "skipped tokens": 0})
    for key, vals in (("vs float64", (rel, mx, tok)), ("vs exact bf16 (recorded)", (rel2, mx2, tok2))):
        for n, v in zip(("rel", "max", "worst token"), vals):
            w[key][n] = max(w[key][n], v) if v == v else NAN
    assert rel < R.BAR_L2 and mx < R.BAR_MAX and tok < R.BAR_TOKEN, f"{what}: rel {rel:.3e} max {mx:.3e} worst token {tok:.3e}"


def equal(name, a, b):
    eq = bool(torch.equal(a, b))
    EQUALITIES[name] = eq
    assert eq, f"{name}: not bit-equal (max difference {float((a.double() - b.double()).abs().max()):.3e})"


def pack_heads(c, inp, dev):
    K, _ = _ops()
    return [K.pack_head([t.to(dev) for t in w], c.C, c.D) for w in inp.w]


def run_head(dev, c, inp, packed, variant, we_stream=None):
    """One launch of a head kernel.  variant: "one", "dense", "streams", "enc", "noenc".
    -> the derivative part out - base as token blocks (n_out, rows, D, 8, 8) in float64, the frames themselves, z or None."""
    K, _ = _ops()
    n_img, Hp, Wp = c.shape
    a, frame = inp.addr, inp.frame
    streams = [s.to(dev) for s in inp.streams]
    out = torch.full((n_img * inp.out_bstride + 64,), NAN, device=dev)
    written = torch.zeros(out.numel(), dtype=torch.bool)
    for img in range(n_img):
        written[img * inp.out_bstride: img * inp.out_bstride + c.n_out * frame] = True
    last = None
    if c.last == "null":
        filled = torch.full((out.numel(),), NAN)
        for img in range(n_img):
            filled[img * inp.out_bstride: img * inp.out_bstride + c.n_out * frame] = inp.base[img].reshape(-1)
        out.copy_(filled.to(dev))
    else:
        lb = torch.full((n_img * inp.last_bstride + 64,), NAN)
        for img in range(n_img):
            lb[img * inp.last_bstride: img * inp.last_bstride + frame] = inp.base[img, 0].reshape(-1)
        last = lb.to(dev)
    assert out.data_ptr() % 16 == 0 and all(s.data_ptr() % 16 == 0 for s in streams)
    addr = (a.a_n0, a.a_s1, a.a_s0, a.a_off, n_img, Hp, Wp, c.C, c.D)
    zbuf = None
    if variant == "one":
        K.head_fused(streams[0], *addr, packed[0], out, inp.out_bstride, [row[0] for row in c.coefs()], last, 0, inp.last_bstride)
    elif variant in ("dense", "streams"):
        rows = streams if variant == "streams" else [x.to(dev).contiguous() for x in inp.X[:-1]] + [streams[-1]]
        K.head_fused_multi(rows, *addr, packed, c.coefs()[0], out, inp.out_bstride, last, 0, inp.last_bstride, streams=variant == "streams")
    else:
        z = None
        if variant == "enc":
            zbuf = torch.full((c.rows * c.C + 512,), NAN, device=dev)
            z = zbuf[:c.rows * c.C]
        K.head_enc_fused(streams, *addr, packed, c.coefs()[0], out, inp.out_bstride, last, 0, inp.last_bstride,
                         enc_stream=we_stream if variant == "enc" else None, z=z)
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool(torch.isnan(o[~written]).all()), f"{c.id} {variant}: wrote outside its frames"
    got = torch.stack([o[img * inp.out_bstride: img * inp.out_bstride + c.n_out * frame].view(c.n_out, c.D, 8 * Hp, 8 * Wp) for img in range(n_img)])
    zc = None
    if zbuf is not None:
        zc = zbuf.cpu()
        assert bool(torch.isnan(zc[c.rows * c.C:]).all()), f"{c.id}: wrote past the end of z"
        zc = zc[:c.rows * c.C].view(c.rows, c.C)
    return got, zc


def derivative(c, e, got):
    """out - base as token blocks (n_out, rows, D, 8, 8), float64."""
    return torch.stack([R.frames_to_blocks(got[:, i].double()) for i in range(c.n_out)]) - e["base"]


def head_form(c, multi, o):
    """Inside `option("TANTE_HEAD_WAVES", o)`: the route the restated dispatch gives for what the library reports."""
    _, L = _ops()
    route = R.head_route(c.C, multi, c.rows, L.get_option("TANTE_HEAD_WAVES", 0))
    assert f"NWV{o or 8}," in route and route in c.routes(), (c.id, o, route)       # no option: the 8-wave form by the default rule
    return route


ONE_CASES = [c for c in R.HEAD_CASES if c.kind == "one"]
MULTI_CASES = [c for c in R.HEAD_CASES if c.kind == "multi"]


@pytest.mark.parametrize("c", ONE_CASES, ids=[c.id for c in ONE_CASES])
def test_head_fused(dev, c):
    """tante_head_fused under each wave form: n_out frames with distinct coefficients, `last` given or accumulation onto the pre-filled
    frames, batch strides with slack, rows addressed as the model does, padded, or in blocks of 11."""
    e = evaluated(c)
    inp = e["inp"]
    packed = pack_heads(c, inp, dev)
    outs = {}
    for o in c.options:
        with option("TANTE_HEAD_WAVES", o):
            route = head_form(c, False, o)
            got, _ = run_head(dev, c, inp, packed, "one")
        ROUTES_RUN.add(route)
        hold(f"tante_head_fused C{c.C}", f"{c.id} {route}", derivative(c, e, got), e["ref"], e["bf"])
        outs[o] = got
    if len(outs) == 2:
        equal(f"{c.id}: 4 waves vs 8 waves", outs[4], outs[8])
    CASES_RUN.add(c.id)


@pytest.mark.parametrize("c", MULTI_CASES, ids=[c.id for c in MULTI_CASES])
def test_head_fused_multi(dev, c):
    """tante_head_fused_multi (dense copies of the earlier orders' rows) and tante_head_fused_multi_streams (whole streams) under each wave
    form: distinct weights and coefficients per order; the two give the same bits, and so do the two wave forms."""
    e = evaluated(c)
    inp = e["inp"]
    packed = pack_heads(c, inp, dev)
    outs = {}
    for o in c.options:
        with option("TANTE_HEAD_WAVES", o):
            route = head_form(c, True, o)
            got_of = {variant: run_head(dev, c, inp, packed, variant)[0] for variant in ("dense", "streams")}
        for variant, got in got_of.items():
            hold(f"tante_head_fused_multi{'_streams' if variant == 'streams' else ''} C{c.C}", f"{c.id} {variant} {route}", derivative(c, e, got),
                 e["ref"], e["bf"])
            outs[o, variant] = got
        ROUTES_RUN.add(route)
        equal(f"{c.id} {route}: dense copies vs whole streams", outs[o, "dense"], outs[o, "streams"])
    equal(f"{c.id}: 4 waves vs 8 waves", outs[4, "streams"], outs[8, "streams"])
    CASES_RUN.add(c.id)


@pytest.mark.parametrize("c", R.HEAD_ENC_CASES, ids=[c.id for c in R.HEAD_ENC_CASES])
def test_head_enc_fused(dev, c):
    """tante_head_enc_fused under each wave form, with and without the encoding.  The frame's derivative part is held like the heads'; z is
    held to the float64 encoder of the frame the kernel wrote (head error does not leak into the encoder figure).  The encoding launch runs
    twice on the workspace kernels.head_enc_workspace keeps for the option in force: the same bits, and the arrival counters are zero."""
    K, L = _ops()
    e = evaluated(c)
    inp = e["inp"]
    n_img, Hp, Wp = c.shape
    packed = pack_heads(c, inp, dev)
    we_stream = K.pack_head_enc([t.to(dev) for t in inp.we], c.C, c.D)
    frames, zs = {}, {}
    for o in c.options:
        with option("TANTE_HEAD_WAVES", o):
            opt = L.get_option("TANTE_HEAD_WAVES", 0)
            gt = R.head_group_tokens(c.rows, opt)
            assert gt == 16 * o
            for variant in ("enc", "noenc"):
                route = R.head_enc_route(c.D, variant == "enc", c.rows, opt)
                assert route in c.routes() and f"NWV{o}," in route
                got, z = run_head(dev, c, inp, packed, variant, we_stream)
                ROUTES_RUN.add(route)
                hold("tante_head_enc_fused frame", f"{c.id} {route} frame", derivative(c, e, got), e["ref"], e["bf"])
                frames[o, variant] = got
                if variant == "enc":
                    fr = got[:, 0]
                    hold("tante_head_enc_fused z", f"{c.id} {route} z", z, R.encoder_rows(fr, inp.we), R.encoder_rows(fr, inp.we, exact_bf16=True))
                    zs[o] = z
                    got2, z2 = run_head(dev, c, inp, packed, variant, we_stream)
                    equal(f"{c.id} {route}: a second launch on the same workspace, frame", got, got2)
                    equal(f"{c.id} {route}: a second launch on the same workspace, z", z, z2)
                    ws = K.head_enc_workspace(c.rows, dev)
                    groups = (c.rows + gt - 1) // gt
                    assert ws.numel() == L.lib().tante_head_enc_ws_bytes(c.rows)
                    assert not bool(ws[groups * 4 * gt * 128 * 2:].any()), f"{c.id} {route}: arrival counters left non-zero"
            equal(f"{c.id} NWV{o}: frame with vs without the encoding", frames[o, "enc"], frames[o, "noenc"])
            if c.n_ord >= 2:
                ms, _ = run_head(dev, c, inp, packed, "streams")
                equal(f"{c.id} NWV{o}: frame vs tante_head_fused_multi_streams", frames[o, "enc"], ms)
    equal(f"{c.id}: 4 waves vs 8 waves, frame", frames[4, "enc"], frames[8, "enc"])
    equal(f"{c.id}: 4 waves vs 8 waves, z", zs[4], zs[8])
    CASES_RUN.add(c.id)


@pytest.mark.parametrize("c", R.ENC23_CASES, ids=[c.id for c in R.ENC23_CASES])
def test_enc23(dev, c):
    """tante_enc23_fused (FiLM tables with distinct rows per t) and tante_enc23_frames (frames = T) on the same bf16 stage-1 image, under
    every split: the same bits at every split; under identity FiLM the fused form equals the frame-major one once its rows are reordered."""
    K, L = _ops()
    e = evaluated(c)
    inp = e["inp"]
    n_img, Hp, Wp = c.shape
    HW, Cc = Hp * Wp, c.C
    h1 = inp.h1.to(dev).contiguous()
    stream = K.pack_enc23([t.to(dev) for t in inp.w], Cc)
    film = (inp.film_a.to(dev), inp.film_b.to(dev), inp.s_emb.to(dev), c.T, HW)
    ident = (torch.ones(c.T, Cc, device=dev), torch.zeros(c.T, Cc, device=dev), torch.zeros(HW, Cc, device=dev), c.T, HW)
    n = c.rows * Cc

    def run(fn):
        buf = torch.full((n + 512,), NAN, device=dev)
        fn(buf[:n].view(c.rows, Cc))
        torch.cuda.synchronize()
        o = buf.cpu()
        assert bool(torch.isnan(o[n:]).all()), f"{c.id}: wrote past the end of its rows"
        return o[:n].view(c.rows, Cc)
    outs = {}
    for o in c.options:
        with option("TANTE_ENC23_SPLIT", o):
            route = R.enc23_route(c.rows, L.get_option("TANTE_ENC23_SPLIT", 0))
            assert route == f"enc23<SPLIT{o}>" and route in c.routes()
            outs[o, "film"] = run(lambda out: K.enc23_fused(h1, n_img, Hp, Wp, Cc, stream, film, out))
            outs[o, "ident"] = run(lambda out: K.enc23_fused(h1, n_img, Hp, Wp, Cc, stream, ident, out))
            outs[o, "frames"] = run(lambda out: K.enc23_frames(h1, n_img, c.T, Hp, Wp, Cc, stream, out))
            ROUTES_RUN.add(route)
        hold("tante_enc23_fused", f"{c.id} {route} FiLM", outs[o, "film"], *e["film"])
        hold("tante_enc23_fused", f"{c.id} {route} identity FiLM", outs[o, "ident"], *e["rows"])
        hold("tante_enc23_frames", f"{c.id} {route} frame-major", outs[o, "frames"], *e["frames"])
        equal(f"{c.id} {route}: enc23_frames vs enc23_fused under identity FiLM, rows reordered",
              R.frame_major(outs[o, "ident"], n_img, c.T, HW), outs[o, "frames"])
    for o in c.options[1:]:
        for form in ("film", "frames"):
            equal(f"{c.id} {form}: split {o} vs split {c.options[0]}", outs[o, form], outs[c.options[0], form])
    CASES_RUN.add(c.id)


@pytest.mark.parametrize("name,Hp,Wp,a_n0", [("Hp*Wp=15", 5, 3, 16), ("a_n0=24", 4, 4, 24)])
def test_head_enc_c_entry_refuses_partial_tiles(dev, name, Hp, Wp, a_n0):
    """The exported C entry itself (not the Python wrapper, which has its own check) returns -2 with a message when Hp * Wp or a_n0 is no
    multiple of 16, before anything is launched: frame, z and workspace are untouched.  The guard is read in the source first -- this call
    is never made against a library without it -- and every buffer is large enough for the tiles such a launch would have touched."""
    K, L = _ops()
    src = open(os.path.join(ROOT, "tante_amd", "csrc", "head_enc.hip")).read()
    assert "if (((long)Hp * Wp) % 16 || a_n0 % 16)" in src
    Cc, D, n_img = 256, 1, 3
    gen = torch.Generator().manual_seed(5)
    rows = n_img * Hp * Wp
    x = torch.randn(8 * 64 * Cc, generator=gen).to(dev)
    frame = D * 64 * Hp * Wp
    out = torch.full((8 * n_img * frame,), NAN, device=dev)
    last = torch.randn(8 * n_img * frame, generator=gen).to(dev)
    z = torch.full((8 * 64 * Cc,), NAN, device=dev)
    hs = K.pack_head([t.to(dev) for t in R.dec_weights(Cc, D, 1)], Cc, D)
    es = K.pack_head_enc([t.to(dev) for t in R.enc_weights(Cc, D, 1)], Cc, D)
    ws = torch.zeros(max(int(L.lib().tante_head_enc_ws_bytes(rows)), 1) + (1 << 20), dtype=torch.uint8, device=dev)
    rp, sp, cf = (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(hs.data_ptr()), (C.c_float * 1)(1.0)
    rc = L.lib().tante_head_enc_fused(1, rp, sp, cf, a_n0, a_n0 * Cc, Cc, 0, n_img, Hp, Wp, Cc, D, out.data_ptr(), frame, last.data_ptr(), frame,
                                      es.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(), K._stream())
    assert rc == -2, rc
    with pytest.raises(RuntimeError, match="whole 16-token tiles expected"):
        L.check(rc, "tante_head_enc_fused")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(z).all()) and not bool(ws.any()), name
    with pytest.raises(RuntimeError, match="whole 16-token tiles per image expected"):       # the Python check stays
        K.head_enc_fused([x], a_n0, a_n0 * Cc, Cc, 0, n_img, Hp, Wp, Cc, D, [hs], [1.0], out, frame, last, 0, frame)


def test_every_template_instance_ran(dev):
    """After the cases above: the routes asserted on the way are every template instance the three launchers can select (counted from the
    launch switches by tests/test_tail_enc_cpu.py), and no token was left out of a per-token figure."""
    every = {c.id for c in R.HEAD_CASES + R.HEAD_ENC_CASES + R.ENC23_CASES}
    if CASES_RUN != every:
        pytest.skip("only part of this module was selected")
    assert ROUTES_RUN == R.ALL_HEAD_ROUTES | R.ALL_HEAD_ENC_ROUTES | R.ALL_ENC23_ROUTES, sorted(
        (R.ALL_HEAD_ROUTES | R.ALL_HEAD_ENC_ROUTES | R.ALL_ENC23_ROUTES) ^ ROUTES_RUN)
    assert all(v for v in EQUALITIES.values()) and all(f["skipped tokens"] == 0 for f in FIGURES.values())
