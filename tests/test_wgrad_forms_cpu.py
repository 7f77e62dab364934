"""No GPU: what tests/test_hip_wgrad_forms.py relies on is itself held here.  The restated dispatch of tests/wgrad_forms_ref.py against the
text of tante_amd/csrc/wgrad.hip; the case list against the dispatch (every route reached, every case at the edge it is named for); the
restated gather (rm_elem) and scatter (out_index) against torch's own unfold / conv2d / conv_transpose2d in float64; the bars against the
wrong results these kernels can produce."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import wgrad_forms_ref as R
from conftest import ROOT

SRC = open(os.path.join(ROOT, "tante_amd", "csrc", "wgrad.hip")).read()


def by_name(group, name, compute=None):
    cs = [c for c in R.CASES if c.group == group and c.name == name and compute in (None, c.compute)]
    assert cs, (group, name)
    return cs[0] if compute is not None or len(cs) == 1 else cs


@pytest.fixture(scope="module")
def evaluated():
    """Every case's operands and float64 reference, computed once."""
    out = {}
    for c in R.CASES:
        inp = R.make_inputs(c)
        out[c.id] = (inp, R.reference(c, inp))
    return out


def _body(name):
    """The text of a function of wgrad.hip, from its name to the closing brace in column 0."""
    m = re.search(r"^[^\n]*\b" + re.escape(name) + r"\([^;]*?\{\n.*?^\}", SRC, re.S | re.M)
    assert m, name
    return m.group(0)


def test_wgrad_route_matches_the_source():
    """`wgrad_route` is a restatement: its constants, thresholds and conditions are read out of wgrad.hip here, so that a changed line of
    the dispatch fails THIS test (and points at tests/wgrad_forms_ref.py) instead of leaving the case ids silently wrong."""
    consts = dict((k, int(v)) for k, v in re.findall(r"constexpr int (RC|WT|WRC|WSEG|WJOBS|WGJ_OCC) = (\d+)", SRC))
    m = re.search(r"constexpr int WT = (\d+), WRC = (\d+);", SRC)
    consts["WT"], consts["WRC"] = int(m.group(1)), int(m.group(2))
    assert consts == dict(RC=R.RC, WT=R.WT, WRC=R.WRC, WSEG=R.WSEG, WJOBS=R.WJOBS, WGJ_OCC=R.WGJ_OCC), consts
    # the default option values
    opts = dict(re.findall(r'tante_opt\("(TANTE_WGRAD_\w+)", ([^()]+?)\)', SRC))
    want = {"TANTE_WGRAD_WGS": "512", "TANTE_WGRAD_SLAB_WGS": "1536", "TANTE_WGRAD_JOBS_WGS": "256 * WGJ_OCC", "TANTE_WGRAD_NO_TR": "0",
            "TANTE_WGRAD_NO_SLAB": "0", "TANTE_WGRAD_RG": "1", "TANTE_WGRAD_DEEP": "-1", "TANTE_WGRAD_JOBS": "1", "TANTE_WGRAD_REDUCE_NY": "0"}
    got = {k: v for k, v in opts.items() if k in want}
    # TANTE_WGRAD_WGS appears twice: 512 in launch_wgrad, 0 as the fall-back of TANTE_WGRAD_TR_WGS
    assert re.search(r'tante_opt\("TANTE_WGRAD_WGS", 512\)', SRC) and re.search(r'tante_opt\("TANTE_WGRAD_WGS", 0\)\)', SRC)
    got["TANTE_WGRAD_WGS"] = "512"
    assert got == want, got
    for k, v in want.items():
        if k in R.DEFAULTS:
            assert R.DEFAULTS[k] == eval(v, {"WGJ_OCC": R.WGJ_OCC}), k
    assert R.DEFAULTS["TANTE_WGRAD_TR_WGS"] == 0
    # the 8 * RC threshold
    m = re.search(r"R >= (\d+) \* RC", SRC)
    assert m and int(m.group(1)) == R.SLAB_MIN_CHUNKS
    # every restated line is in the source, verbatim
    for line in R.SOURCE_LINES:
        assert line in SRC, f"wgrad.hip no longer holds this line; restate tests/wgrad_forms_ref.py:\n{line}"
    # no line beside the restated ones decides a staging mode or a template
    sm = _body("rm_stage_mode")
    assert re.findall(r"return (ST_\w+);", sm) == ["ST_PATCH_NHWC", "ST_PATCH_NCHW2", "ST_GENERIC", "ST_ROWMAJOR", "ST_COLMAJOR", "ST_GENERIC"]
    assert sm.count("if (") == 5
    lw = _body("launch_wgrad")
    table = re.findall(r"(?:else )?if \(mu == ST_(\w+)(?: && mv == ST_(\w+))?\) TANTE_WG\(ST_(\w+), ST_(\w+)\);", lw)
    table.append((None, None) + re.search(r"\n  else TANTE_WG\(ST_(\w+), ST_(\w+)\);", lw).groups())
    assert [(a, b or None, c, d) for a, b, c, d in table] == R.STAGE_TABLE
    assert lw.count("TANTE_WG(") == len(R.STAGE_TABLE) + 1      # + the #define
    assert len(re.findall(r"hipLaunchKernelGGL\(\(wgrad_tr_kernel<", SRC)) == 3 and SRC.count("launch_wgrad<") == 3
    assert _body("wgrad_tr_launch").count("return false;") == 4
    # the thresholds, on either side
    u, v = R.rows(R.F32, 512, 24), R.rows(R.F32, 512, 16)
    assert R.wgrad_route("one", u, v, 1, 8 * R.RC, 24, 16, R.F32, R.BIG_WS).endswith("+slab")
    assert R.wgrad_route("one", u, v, 1, 8 * R.RC - 1, 24, 16, R.F32, R.BIG_WS).endswith("+atomic")
    assert R.wgrad_route("one", u, v, 1, 8 * R.RC, 24, 16, R.F32, R.BIG_WS, {"TANTE_WGRAD_SLAB_WGS": 0}).endswith("+atomic")
    assert "T64" in R.wgrad_route("one", u, v, 1, 512, 64, 64, R.BF16, 0) and "T128" in R.wgrad_route("one", u, v, 1, 512, 65, 64, R.BF16, 0)
    assert "T128" in R.wgrad_route("one", u, v, 1, 512, 64, 65, R.BF16, 0) and "T64" in R.wgrad_route("one", u, v, 1, 512, 65, 65, R.F32, 0)
    partial = (24 * 16 + 24) * 4
    for ws, ep, split in ((2 * partial, "slab", 2), (2 * partial - 1, "atomic", 2), (1, "atomic", 2)):
        p = R.wgrad_plan("one", u, v, 1, 512, 24, 16, R.F32, ws)
        assert p.name.endswith(ep) and p.split == split, (ws, p.name, p.split)      # never 0 splits: the workspace below one partial


def test_wgrad_cases_reach_every_route():
    """The launch forms of the case list plus COVERED_ELSEWHERE are ALL_ROUTES -- no form is left out silently -- and the list holds the
    shapes the forms change at."""
    reached = set()
    for c in R.CASES:
        atoms = R.route_atoms(c.route)
        assert atoms, c.id
        reached |= atoms
    assert reached | set(R.COVERED_ELSEWHERE) == R.ALL_ROUTES, (R.ALL_ROUTES - reached, reached - R.ALL_ROUTES)
    assert not (reached & set(R.COVERED_ELSEWHERE))
    for why, where in R.COVERED_ELSEWHERE.values():
        for f, t in re.findall(r"tests/(\w+)\.py::(\w+)", where):
            assert f"def {t}(" in open(os.path.join(ROOT, "tests", f + ".py")).read(), where
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:      # the limits on the shapes
        for jb in c.jobs:
            assert jb.R <= 8192 and jb.I <= 384 and jb.J <= 384, c.id
            for m in jb.U + jb.V:
                assert m.mode == R.A_LINEAR or (m.Hin // m.P <= 16 and m.Win // m.P <= 16), c.id
    # every multi grouping and every reason for one-by-one is there
    routes = {c.route for c in R.CASES}
    assert "multi: tr<4,1>+slab x8 | tr<4,1>+atomic x1" in routes and "multi: tr<4,1>+slab x8 | tr<4,1>+slab x3" in routes
    whys = {re.match(r"one-by-one\[(.*?)\]", r).group(1) for r in routes if r.startswith("one-by-one")}
    assert whys == {"1 jobs", "5 jobs", "a job outside the shape rules", "workspace too small", "TANTE_WGRAD_JOBS=0"}, whys


def _straddles(m, R_):
    """Does a 4-row block of the stager (rows 4 q .. 4 q + 3) lie across two n0 groups?"""
    return m.s1 != 0 and any((r % m.n0) + 3 >= m.n0 for r in range(0, R_ - 3, 4))


def test_wgrad_cases_sit_on_their_edges():
    """Every case reaches the edge it is named for (read from the restated plan, not from the name)."""
    for comp in (R.F32, R.BF16):
        c6, c8 = by_name("a", "blocks-n0=6", comp), by_name("a", "blocks-n0=8", comp)
        assert "ROW,ROW" in c6.route and _straddles(c6.jobs[0].U[0], 333) and _straddles(c6.jobs[0].V[0], 333)
        assert "ROW,ROW" in c8.route and not _straddles(c8.jobs[0].U[0], 333) and c8.jobs[0].U[0].s1 != 0
        for c in (by_name("a", "col-col-T64-atomic", comp), by_name("a", "72x132-lines", comp)):
            assert "COL,COL" in c.route and c.jobs[0].R % 4 != 0 and c.jobs[0].R % c.jobs[0].U[0].n0 != 0       # ragged tail, a partial last block
        c = by_name("a", "72x132", comp)
        T = c.plan.launches[0].extra["T"]
        assert (c.jobs[0].I % T, c.jobs[0].J % T) != (0, 0) and c.plan.launches[0].extra["ti"] * c.plan.launches[0].extra["tj"] >= 2
        assert c.jobs[0].I % T and c.jobs[0].J % T
        for name in ("frames-nhwc", "frames-nchw2"):
            m = by_name("a", name, comp).jobs[0].V[0]
            assert m.s1 > m.n0 * m.Cin * m.Hin * m.Win and m.n0 == 2 and m.R // ((m.Hin // m.P) * (m.Win // m.P)) % m.n0 == 1
        for name, twin in (("v+4B", "twin-rows"), ("u+4B", "twin-rows"), ("ncols%4-J66", "twin-J68"), ("Cin%4", "twin-Cin%4"), ("Win%8", "twin-Win%8"),
                           ("P=4-nchw", "twin-P=4-nchw"), ("nhwc+4B", "twin-nhwc"), ("nchw2+4B", "twin-nchw2")):
            a, b = by_name("a", name, comp), by_name("a", twin, comp)
            assert "GEN" in a.route and "GEN" not in b.route and a.vkey == b.vkey, (a.id, b.id)
    # rows with padding carry NaN there; off != 0 occurs
    inp = R.make_inputs(by_name("a", "row-row-T64-atomic", R.F32))
    assert bool(torch.isnan(inp.bufs[0][0][0]).any()) and by_name("a", "row-row-T64-atomic", R.F32).jobs[0].U[0].off == 4
    # (b) every layout x swap x bias, both accumulate values
    b = [c for c in R.CASES if c.group == "b"]
    assert {(c.jobs[0].layout, c.jobs[0].swap, c.jobs[0].bias) for c in b} == {(l, s, bi) for l in range(4) for s in (0, 1) for bi in (True, False)}
    assert {(c.jobs[0].layout, c.accumulate) for c in b} == {(l, a) for l in range(4) for a in (0, 1)}
    # (c) the R threshold, the reduce grid's y on either side of 64 splits, the workspace limits
    for comp in (R.F32, R.BF16):
        assert [by_name("c", f"R{r}", comp).route.split("+")[1] for r in (511, 512, 513)] == ["atomic", "slab", "slab"]
        assert by_name("c", "R513", comp).plan.ranges[-1] == (512, 513)
        ys = [(by_name("c", n, comp).plan.split, by_name("c", n, comp).plan.launches[0].reduce_y) for n in ("split63", "split64", "split65-ragged")]
        assert ys == [(63, 1), (64, 16), (65, 16)], ys
        assert by_name("c", "ws-limits-split", comp).plan.split == 10 and by_name("c", "ws-two-partials", comp).plan.split == 2
        for n in ("ws-below-two-partials", "ws-below-one-partial"):
            c = by_name("c", n, comp)
            assert c.route.endswith("+atomic") and c.plan.split >= 1 and c.ws_bytes < 2 * (24 * 16 + 24) * 4
        assert by_name("c", "ws-below-one-partial", comp).ws_bytes < (24 * 16 + 24) * 4
    # (d) the ring: start-up (fewer chunks than buffers), exactly the ring, a wrap, odd and even tails of the two-register-set pipeline
    for nch in (1, 2, 3, 4, 5, 8, 9):
        for n in (f"one-split-{nch}chunks", f"one-split-{nch}chunks-ws"):
            l = by_name("d", n).plan.launches[0]
            assert l.split == 1 and l.chunks == [nch] and l.extra["ring"] == 4, n
    assert by_name("d", "one-split-5chunks").plan.launches[0].chunks[0] > 4       # "ring wraps"
    assert by_name("d", "one-split-1chunks").route == "tr<4,1>+atomic" and by_name("d", "one-split-1chunks-ws").route == "multi: tr<4,1>+slab x2"
    for nch in (1, 7, 8, 9, 17):
        l = by_name("d", f"deep-{nch}chunks").plan.launches[0]
        assert l.name == "tr<8,1>+atomic" and l.chunks == [nch] and l.extra["ring"] == 8
    assert by_name("d", "deep-ws").route == "multi: tr<8,1>+slab x2"
    assert [by_name("d", f"per-search-R{r}").plan.split for r in (384, 416, 4064)] == [3, 1, 1]
    assert by_name("d", "per-search-R4064").plan.launches[0].chunks == [127]
    for I, J in ((128, 128), (256, 128), (128, 256), (256, 384)):
        e = by_name("d", f"{I}x{J}").plan.launches[0].extra
        assert (e["ti"], e["tj"]) == (I // 128, J // 128)
    for n in ("R%32", "s0%8", "I192", "u+4B", "no-tr-128x128", "no-tr-256x384"):
        assert by_name("d", n).route.startswith("gen<bf16,T128,"), n
    for nch, chunks in ((6, 3), (16, 4), (24, 4)):
        l = by_name("d", f"rg2-{nch}chunks").plan.launches[0]
        assert l.name == "tr<4,2>+slab" and l.rg == 2 and l.chunks[0] == chunks
    assert by_name("d", "rg2-5chunks-refused").route == "multi: 2*(tr<4,1>+atomic x1)"
    assert by_name("d", "no-slab").route == "multi: tr<4,1>+atomic x2" and by_name("d", "twin-no-slab").route == "multi: tr<4,1>+slab x2"
    # (f) uneven chunk ranges, XCD rotation, one split per segment
    p = by_name("f", "4jobs").plan
    assert p.name == "jobs" and [b - a for a, b in p.launches[0].ranges] == [96, 96, 96, 128]
    assert p.launches[0].extra["total"] % 8 != 0 and p.launches[1].extra["rot"] != 0
    assert any(l.extra["total"] % 8 for l in p.launches[1:]) and len({(l.n_seg, l.split) for l in p.launches}) >= 3
    p = by_name("f", "2jobs-wgs8").plan
    assert p.name == "jobs" and all(l.split == 1 for l in p.launches)
    assert {len(c.jobs) for c in R.CASES if c.route == "jobs"} == {2, 3, 4}


def test_restated_gather_and_scatter_match_torch():
    """rm_index against unfold on the same images (both patch orders, image blocks with a gap), and out_index against float64 autograd:
    the weight gradient of F.linear, of F.conv2d(stride = P) on channels-last and channels-first patches and of F.conv_transpose2d(stride = P)
    in both output layouts is U^T V scattered by out_index, exactly as the header says."""
    gen = torch.Generator().manual_seed(5)
    n_img, Hin, Win, Cin, P = 3, 6, 8, 4, 2
    Ho, Wo = Hin // P, Win // P
    x = torch.randn(n_img, Cin, Hin, Win, generator=gen, dtype=torch.float64)
    unf = F.unfold(x, P, stride=P)                                   # (n, Cin P P, Ho Wo): rows (ci, kh, kw)
    want_nchw = unf.permute(0, 2, 1).reshape(n_img * Ho * Wo, Cin * P * P)
    want_nhwc = unf.view(n_img, Cin, P, P, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(n_img * Ho * Wo, P * P * Cin)
    m = R.patches(R.F32, False, n_img, Hin, Win, Cin, P)
    assert torch.equal(x.reshape(-1)[R.rm_index(m, m.R, m.ncols)], want_nchw)
    m = R.patches(R.F32, True, n_img, Hin, Win, Cin, P)
    xl = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(xl.reshape(-1)[R.rm_index(m, m.R, m.ncols)], want_nhwc)
    # image blocks of 2 with a gap and an offset: images 0, 1 | gap | 2
    m = R.patches(R.F32, False, n_img, Hin, Win, Cin, P, n0=2, gap=16, off=8)
    buf = torch.zeros(8 + 2 * (2 * x[0].numel() + 16), dtype=torch.float64)
    for i in range(n_img):
        o = 8 + (i // 2) * (2 * x[0].numel() + 16) + (i % 2) * x[0].numel()
        buf[o:o + x[0].numel()] = x[i].reshape(-1)
    assert torch.equal(buf[R.rm_index(m, m.R, m.ncols)], want_nchw)
    # strided rows in blocks
    m = R.rows(R.F32, 10, 5, pad=3, off=2, n0=4, gap=7)
    a = torch.arange(200, dtype=torch.float64)
    want = torch.stack([a[(r // 4) * (4 * 8 + 7) + (r % 4) * 8 + 2:][:5] for r in range(10)])
    assert torch.equal(a[R.rm_index(m, 10, 5)], want)

    def scattered(U, V, layout, Pp, Co, swap, shape):
        flat = torch.zeros(U.shape[1] * V.shape[1], dtype=torch.float64)
        flat[R.out_index(layout, U.shape[1], V.shape[1], Pp, Co, swap).reshape(-1)] = (U.t() @ V).reshape(-1)
        return flat.view(shape)
    # Linear: y = x W^T; U = dY, V = X
    X = torch.randn(11, 5, generator=gen, dtype=torch.float64)
    W = torch.randn(7, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(11, 7, generator=gen, dtype=torch.float64)
    (gW,) = torch.autograd.grad(F.linear(X, W), W, dY)
    assert torch.allclose(scattered(dY, X, R.W_LINEAR, 0, 0, 0, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(X, dY, R.W_LINEAR, 0, 0, 1, gW.shape), gW, rtol=0, atol=1e-12)
    # Conv2d(stride = P): U = dPre rows (co), V = patches of the input
    Cout = 6
    Wc = torch.randn(Cout, Cin, P, P, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, Wc, stride=P)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (gW,) = torch.autograd.grad(y, Wc, dy)
    dpre = dy.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert torch.allclose(scattered(dpre, want_nhwc, R.W_CONV_NHWC, P, Cin, 0, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(want_nhwc, dpre, R.W_CONV_NHWC, P, Cin, 1, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(dpre, want_nchw, R.W_LINEAR, 0, 0, 0, gW.shape), gW, rtol=0, atol=1e-12)      # channels-first patches: (co, (ci, kh, kw)) is the parameter
    # ConvTranspose2d(stride = P): U = X rows (pixels, ci), V = patches of the output gradient
    Wt = torch.randn(Cin, Cout, P, P, generator=gen, dtype=torch.float64, requires_grad=True)
    xs = torch.randn(n_img, Cin, Ho, Wo, generator=gen, dtype=torch.float64)
    y = F.conv_transpose2d(xs, Wt, stride=P)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (gW,) = torch.autograd.grad(y, Wt, dy)
    pix = xs.permute(0, 2, 3, 1).reshape(-1, Cin)
    m = R.patches(R.F32, False, n_img, Hin, Win, Cout, P)
    p_nchw = dy.reshape(-1)[R.rm_index(m, m.R, m.ncols)]
    m = R.patches(R.F32, True, n_img, Hin, Win, Cout, P)
    p_nhwc = dy.permute(0, 2, 3, 1).reshape(-1)[R.rm_index(m, m.R, m.ncols)]
    assert torch.allclose(scattered(pix, p_nhwc, R.W_DECONV_NHWC, P, Cout, 1, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(p_nhwc, pix, R.W_DECONV_NHWC, P, Cout, 0, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(pix, p_nchw, R.W_DECONV_NCHW, P, Cout, 1, gW.shape), gW, rtol=0, atol=1e-12)
    assert torch.allclose(scattered(p_nchw, pix, R.W_DECONV_NCHW, P, Cout, 0, gW.shape), gW, rtol=0, atol=1e-12)
    # every out_index is a bijection onto the parameter, on the shapes of the case list
    for c in R.CASES:
        for jb in c.jobs:
            idx = R.out_index(jb.layout, jb.I, jb.J, jb.P, jb.Co, jb.swap).reshape(-1)
            assert torch.equal(idx.sort().values, torch.arange(jb.I * jb.J)), c.id


def test_same_values_share_a_reference(evaluated):
    """Cases that serve the same values through two forms (one vkey, the same shape) have the same reference, bit for bit; the J = 66 case
    is the first 66 columns of its J = 68 twin."""
    groups = {}
    for c in R.CASES:
        groups.setdefault((c.vkey, c.compute, tuple((j.R, j.I, j.J, j.n_seg) for j in c.jobs)), []).append(c)
    pairs = 0
    for cs in groups.values():
        for c in cs[1:]:
            for (a, ab), (b, bb) in zip(evaluated[cs[0].id][1], evaluated[c.id][1]):
                if cs[0].acc == c.acc:
                    assert torch.equal(a, b) and (ab is None or bb is None or torch.equal(ab, bb)), (cs[0].id, c.id)
            pairs += 1
    assert pairs >= 26
    for comp in (R.F32, R.BF16):
        a, b = by_name("a", "ncols%4-J66", comp), by_name("a", "twin-J68", comp)
        assert torch.equal(evaluated[a.id][1][0][0].view(40, 66), evaluated[b.id][1][0][0].view(40, 68)[:, :66])


def test_wgrad_bars_reject_wrong_results(evaluated):
    """Rounding the fp32 sources to bf16 stays under half the bf16 bar on every case that is held to it, and each wrong result of the kinds
    these kernels can produce -- the ragged last chunk dropped, one split dropped, one segment dropped, one 32-row chunk counted twice, two
    16-column groups of a tile exchanged (a wrong swizzle), one tile transposed -- lies beyond twice the bar of EVERY case it applies to."""
    for c in R.CASES:
        if c.rounds_sources():
            inp, ref = evaluated[c.id]
            for (a, ab), (b, bb) in zip(R.reference(c, inp, exact_bf16=True), ref):
                rel, mx = R.errors(a, b)
                assert rel < 0.5 * R.BF16_BARS[0] and mx < 0.5 * R.BF16_BARS[1], (c.id, rel, mx)
    seen = {b: 0 for b in R.BUGS}
    for c in R.CASES:
        inp, ref = evaluated[c.id]
        bl2, bmx = c.bars(c.jobs[0], exact=False)
        for bug in R.BUGS:
            if not R.bug_applies(c, bug):
                continue
            wrong = R.reference(c, inp, bug=bug)[0][0]
            rel, mx = R.errors(wrong, ref[0][0])
            assert rel > 2 * bl2 and mx > 2 * bmx, (c.id, bug, rel, mx)
            seen[bug] += 1
    assert all(n >= 10 for n in seen.values()), seen
