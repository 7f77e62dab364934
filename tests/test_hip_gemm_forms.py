"""tante_gemm alone: every dispatch form of the GEMM front end (tante_amd/csrc/gemm.hip) against float64.

The cases, their float64 references, the exact-bf16 evaluation and the restated dispatch (`gemm_route`) live in tests/gemm_forms_ref.py;
tests/test_gemm_forms_cpu.py pins them to the oracle, to the text of gemm.hip and to wrong results without a GPU.  Here every case builds
a TanteGemm directly (tante_amd._lib.Gemm), asserts that the descriptor with its REAL pointers takes the route its id names, runs it into
a NaN-filled buffer that is wider and longer than what is written, and holds the result to the per-format bars (fp32 compute 2e-5 / 1e-4,
bf16 compute 1e-2 / 2e-2, relative L2 / max-norm against float64).  bf16 forms whose only roundings are the operands' (no LayerNorm, act
none / relu, fp32 output) are also held to the fp32 bar against the exact-bf16 evaluation; for the other bf16 forms that error is recorded.

Left to other files (gemm_forms_ref.COVERED_ELSEWHERE): the patch-fragment forms of the lite kernel and its training epilogues."""
import ctypes as C
import json
import os

import pytest
import torch

import gemm_forms_ref as R
from conftest import ROOT, record_parity

pytestmark = pytest.mark.gpu

FIGURES = {}        # group -> worst figures of this run (written to gemm_forms_parity.json beside conftest's parity_report.json when the module ends)
EQUALITIES = {}     # bit-equalities of groups (c) and (d): name -> held


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    try:
        with open(os.path.join(ROOT, "gemm_forms_parity.json"), "w") as f:
            json.dump({"groups": FIGURES, "bit_equalities": EQUALITIES}, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _ops():
    from tante_amd import kernels as K, _lib as L
    return K, L


_INPUTS = {}


def inputs(c):
    """The operands of a case, drawn once and shared (never modified: every run uploads its own copies)."""
    if c.id not in _INPUTS:
        inp = R.make_inputs(c)
        inp.ref = R.reference(c, inp)
        inp.ref_bf = R.reference(c, inp, exact_bf16=True) if c.mode == "bf16" else None
        _INPUTS[c.id] = inp
    return _INPUTS[c.id]


def _tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def out_size(c):
    if c.e_mode in ("lin", "film"):
        return (c.M + 1) * c.out_ld
    return c.M * c.N


def pack(c, inp, dev):
    K, L = _ops()
    lay, _, P, Co = R.w_layout(c)
    return K.pack_weight(inp.w.to(dev), inp.bias.to(dev), c.compute, lay, N=c.N, K=c.K, P=P, C_other=Co,
                         gamma=None if inp.gamma is None else inp.gamma.to(dev), beta=None if inp.beta is None else inp.beta.to(dev))


def run_case(c, inp, dev, pw=None, expect_route=True):
    """One tante_gemm call of a case.  -> (the output in its logical shape as a CPU tensor, the NaN check of everything else)."""
    K, L = _ops()
    pw = pack(c, inp, dev) if pw is None else pw
    a_dev = inp.a_buf.to(dev)
    odt = _tdt(c.out_dtype)
    n_out = out_size(c)
    o_dev = torch.full((c.out_lead + n_out + 8,), float("nan"), dtype=odt, device=dev)
    written = torch.zeros(c.out_lead + n_out + 8, dtype=torch.bool)
    if c.e_mode in ("lin", "film"):
        idx = (c.out_lead + torch.arange(c.M)[:, None] * c.out_ld + torch.arange(c.N)[None, :]).reshape(-1)
    else:
        idx = c.out_lead + torch.arange(n_out)
    written[idx] = True
    keep = []
    f = R.fields(c)
    g = L.Gemm()
    for name, _ in L.Gemm._fields_:
        if hasattr(f, name) and name not in ("a", "out", "residual", "dact"):
            setattr(g, name, getattr(f, name))
    assert a_dev.data_ptr() % 16 == 0 and o_dev.data_ptr() % 16 == 0
    g.a = a_dev.data_ptr() + c.a_lead * a_dev.element_size()
    g.out = o_dev.data_ptr() + c.out_lead * o_dev.element_size()
    g.w, g.bias = pw.w.data_ptr(), pw.bias.data_ptr()
    if c.res == "out":
        o_dev[idx.to(dev)] = inp.res.reshape(-1).to(dev).to(odt)
        assert odt == torch.float32
        g.residual = g.out
    elif c.res == "other":
        r_dev = inp.res_buf.to(dev)
        keep.append(r_dev)
        g.residual = r_dev.data_ptr() + c.res_lead * 4
    if c.film:
        tabs = [t.to(dev) for t in (inp.film_a, inp.film_b, inp.s_emb)]
        keep += tabs
        g.film_a, g.film_b, g.s_emb = (t.data_ptr() for t in tabs)
    if expect_route:
        assert R.gemm_route(g, small_m=c.small_m) == c.route, (R.gemm_route(g), c.route)
    L.check(L.lib().tante_gemm(C.byref(g), K._stream()), "tante_gemm")
    torch.cuda.synchronize()
    o = o_dev.float().cpu()
    assert bool(torch.isnan(o[~written]).all()), f"{c.id}: wrote outside its region"
    got = o[idx]
    if c.e_mode in ("lin", "film"):
        return got.view(c.M, c.N)
    return got.view(inp.ref.shape)


def _worst(group, key, rel, mx):
    w = FIGURES.setdefault(group, {}).setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel), max(w[1], mx)


def hold(c, got, inp, what=""):
    """The bars of a case; every comparison is recorded with the route."""
    rel, mx = R.errors(got, inp.ref)
    bl2, bmx = c.bars
    print(f"{c.id}{what}: vs float64 rel {rel:.3e} max {mx:.3e} (bar {bl2:.0e} / {bmx:.0e})")
    record_parity(rel, mx, bl2, c.mode, f"{c.route}{what}")
    _worst(c.group, f"{c.mode} vs float64", rel, mx)
    ok = rel < bl2 and mx < bmx
    msg = f"{c.id}{what}: rel {rel:.3e} max {mx:.3e} against float64"
    if c.mode == "bf16":
        rel2, mx2 = R.errors(got, inp.ref_bf)
        print(f"{c.id}{what}: vs exact bf16 rel {rel2:.3e} max {mx2:.3e}")
        if c.operand_rounding_only():
            f2, fm = R.BARS["fp32"]
            record_parity(rel2, mx2, f2, "bf16-exact", f"{c.route}{what}: operand rounding only, against the exact-bf16 evaluation")
            _worst(c.group, "bf16 operand-rounding forms vs exact bf16", rel2, mx2)
            ok = ok and rel2 < f2 and mx2 < fm
            msg += f"; rel {rel2:.3e} max {mx2:.3e} against exact bf16 (fp32 bar)"
        else:
            _worst(c.group, "bf16 other forms vs exact bf16 (recorded)", rel2, mx2)
    assert ok, msg


FORM_CASES = [c for c in R.CASES]


@pytest.mark.parametrize("c", FORM_CASES, ids=[c.id for c in FORM_CASES])
def test_form(dev, c):
    """Groups (a), (b), (e) - (j) of the case list: one launch each, the route asserted from the real descriptor."""
    inp = inputs(c)
    got = run_case(c, inp, dev)
    hold(c, got, inp)
    if c.rows == "const":       # a constant row normalises to zero: the output is act(folded bias), finite
        rows = torch.arange(0, c.M, 3)
        rel, mx = R.errors(got[rows], inp.ref[rows])
        assert rel < c.bars[0] and mx < c.bars[1], (rel, mx)
        assert bool((got[rows] == got[rows][0:1]).all())


def test_small_kernel_ends_at_its_row_limit(dev):
    """M = 1024 and 1025 on the same weights: the second leaves gemm_small_kernel (gemm_route says so) and agrees within the bf16 bar."""
    by = {c.name: c for c in R.CASES if c.group == "i"}
    a, b = by["M1024"], by["M1025"]
    assert a.route.startswith("small<") and b.route.startswith("kernel<bf16,CB16")
    ia = inputs(a)
    ib2 = R.make_inputs(b)
    ib2.w, ib2.bias = ia.w, ia.bias
    ib2.ref, ib2.ref_bf = R.reference(b, ib2), R.reference(b, ib2, exact_bf16=True)
    pw = pack(a, ia, dev)
    hold(a, run_case(a, ia, dev, pw), ia, " (shared weights)")
    hold(b, run_case(b, ib2, dev, pw), ib2, " (shared weights)")


# ---- (c) alignment fallbacks: the same GEMM aligned and with ONE misalignment -----------------------------------------------------
ALIGN_BASES = []
for _mode in ("bf16", "fp32"):
    for _adt in ("f32", "bf16"):
        for _act in ("none", "relu", "gelu_erf", "gelu_tanh"):
            _K = R.K_OF_CB[_mode][4]
            ALIGN_BASES.append(dict(mode=_mode, a_dtype=_adt, act=_act, M=65, N=64, K=_K, a_n0=5, a_s0=_K + 8, a_s1=5 * (_K + 8) + 16, a_off=24,
                                    res="other", out_ld=72, res_ld=80))


def same_arithmetic(mode, act, a_side):
    """Does the generic kernel evaluate this form with the arithmetic of the dedicated one?  gemm_kernel<.., AM_GEN, EP_GEN> is ONE template:
    a misaligned `a` moves the epilogue to epilogue4 / apply_act as well, exactly as a misaligned `out` does.  Products, their order, bias,
    relu and the residual add are the same code; erf-GELU in fp32 compute is gelu_erf_f on both sides; the dedicated tanh-GELU
    (x / (1 + exp(-2u))) and both bf16 GELUs (polynomial / fast forms) are not apply_act's."""
    return act in ("none", "relu") or (mode == "fp32" and act == "gelu_erf")


@pytest.mark.parametrize("base", ALIGN_BASES, ids=[f"{b['mode']}-{b['a_dtype']}rows-{b['act']}" for b in ALIGN_BASES])
def test_alignment_fallbacks(dev, base):
    """`a` 4 bytes off (2 for bf16 rows), an odd a_s0, `out` 4 bytes off, out_ld % 4 != 0, `residual` 4 bytes off: each alone moves the
    launch to kernel<.., AM_GEN, EP_GEN>.  Every run is held to the bars; it is bit-equal to the aligned run wherever the two kernels share
    their arithmetic (same_arithmetic: none, relu, fp32 erf-GELU -- for a misaligned operand on either side), and the GELU forms that differ
    between the dedicated epilogues and apply_act stay within the bars, their distance to the aligned run recorded."""
    mode, act, adt = base["mode"], base["act"], base["a_dtype"]
    c0 = R.Case("c", f"aligned-{act}-{adt}rows", **base)
    assert "AM_LIN" in c0.route and "EP_GEN" not in c0.route, c0.route
    inp = inputs(c0)
    pw = pack(c0, inp, dev)
    y0 = run_case(c0, inp, dev, pw)
    hold(c0, y0, inp)
    variants = [("a+%dB" % (2 if adt == "bf16" else 4), dict(a_lead=1)), ("a_s0-odd", dict(a_s0=base["a_s0"] + 1)),
                ("out+4B", dict(out_lead=1)), ("out_ld%4", dict(out_ld=73)), ("res+4B", dict(res_lead=1))]
    for name, kw in variants:
        c1 = R.Case("c", f"{name}-{act}-{adt}rows", **dict(base, **kw))
        c1.seed = c0.seed
        i1 = R.make_inputs(c1)
        assert torch.equal(i1.w, inp.w) and torch.equal(i1.A, inp.A) and torch.equal(i1.res, inp.res)
        i1.ref, i1.ref_bf = inp.ref, inp.ref_bf
        assert c1.route.endswith("AM_GEN,EP_GEN>"), c1.route
        y1 = run_case(c1, i1, dev, pw)
        hold(c1, y1, i1)
        equal = bool(torch.equal(y0, y1))
        dist = R.errors(y1, y0)
        key = f"{mode} compute, {adt} rows, {act}: {name}"
        EQUALITIES[key] = {"bit_equal": equal, "max_rel_to_aligned": dist[1]}
        print(f"{key}: bit-equal {equal}, distance to the aligned run rel {dist[0]:.3e} max {dist[1]:.3e}")
        if same_arithmetic(mode, act, name.startswith("a")):
            assert equal, f"{key}: not bit-equal to the aligned run (max {dist[1]:.3e})"
        else:
            assert dist[0] < c0.bars[0] and dist[1] < c0.bars[1], (key, dist)


# ---- (d) the N split --------------------------------------------------------------------------------------------------------------
SPLIT_CASES = [dict(mode="bf16", M=130, N=768, K=64, act="gelu_erf"), dict(mode="fp32", M=130, N=768, K=64, ln=True),
               dict(mode="bf16", M=65, N=100, K=64), dict(mode="fp32", M=65, N=100, K=64, act="relu"),
               dict(mode="fp32", M=256, N=1536, K=512, ln=True)]


@pytest.mark.parametrize("kw", SPLIT_CASES, ids=[f"{k['mode']}-M{k['M']}-N{k['N']}-K{k['K']}" for k in SPLIT_CASES])
def test_n_split_is_invisible(dev, kw):
    """TANTE_GEMM_WGS in {1, 8, 512, 4096}: launch_variant splits the tiles of N over 1 .. n_tiles workgroup columns; every output tile is
    one workgroup's whatever the split, so all runs are bit-equal (and each is held to the bars)."""
    import tante_amd
    c = R.Case("d", "split", **kw)
    assert c.route.startswith("kernel<")
    inp = inputs(c)
    pw = pack(c, inp, dev)
    ys = {}
    try:
        for wgs in (1, 8, 512, 4096):
            tante_amd.set_option("TANTE_GEMM_WGS", wgs)
            ys[wgs] = run_case(c, inp, dev, pw)
            hold(c, ys[wgs], inp, f" WGS={wgs}")
    finally:
        tante_amd.set_option("TANTE_GEMM_WGS", 512)
    for wgs, y in ys.items():
        eq = bool(torch.equal(y, ys[512]))
        EQUALITIES[f"{c.id}: WGS={wgs} vs 512"] = eq
        assert eq, f"{c.id}: TANTE_GEMM_WGS={wgs} differs from 512"


# ---- (k) tante_pack_weight --------------------------------------------------------------------------------------------------------
def _int_weight(shape):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) * 7 + (torch.arange(n) // 5) * 3) % 61).float().reshape(shape)       # asymmetric, exact in bf16


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("layout", ["LINEAR", "CONV_NHWC", "DECONV_NHWC", "DECONV_NCHW", "LINEAR_T", "CONV_NHWC_T", "DECONV_NHWC_T", "DECONV_NCHW_T"])
def test_pack_weight_layouts_exact(dev, mode, layout):
    """Identity-like rows against an asymmetric integer weight (exact in bf16), torch.equal: row k of the left operand is the unit vector
    e_k, so the output is the packed matrix itself and a transposed or permuted (n, k) order fails.  Each forward layout is read back through
    the form that consumes it -- CONV_NHWC through the channels-last patch gather (an image whose patches are the unit vectors), the two
    DECONV layouts through their pixel shuffles, against torch's own conv2d / conv_transpose2d on the same integers -- and the four
    data-gradient layouts through dense rows (their consumers differ from these only in forms the forward layouts already ran)."""
    import torch.nn.functional as F
    K, L = _ops()
    comp = K.COMPUTE[mode]
    Ci, Co, P = 6, 5, 2
    lay = getattr(L, "W_" + layout)
    if layout == "CONV_NHWC":              # Conv2d (Cout, Cin, P, P): k = (kh, kw, ci); 24 patches of a (1, 8, 12, 6) image = e_0 .. e_23
        w = _int_weight((Co, Ci, P, P))
        Kd, Ho, Wo = Ci * P * P, 4, 6
        img = torch.eye(Kd).view(Ho, Wo, P, P, Ci).permute(0, 2, 1, 3, 4).reshape(1, Ho * P, Wo * P, Ci).contiguous()
        want = F.conv2d(img.permute(0, 3, 1, 2).double(), w.double(), stride=P).permute(0, 2, 3, 1).reshape(Kd, Co).float()
        assert torch.equal(want, w.permute(0, 2, 3, 1).reshape(Co, Kd).t())
        pw = K.pack_weight(w.to(dev), None, comp, lay, N=Co, K=Kd, P=P, C_other=Ci)
        out = torch.full((Kd + 1, Co), float("nan"), device=dev)
        K.patch_embed(img.to(dev), pw, out, n_img=1, Hin=Ho * P, Win=Wo * P, Cin=Ci, P=P, nchw=False, act=L.ACT_NONE)
        o = out.cpu()
        assert torch.equal(o[:Kd], want) and bool(torch.isnan(o[Kd]).all())
    elif layout in ("DECONV_NHWC", "DECONV_NCHW"):     # ConvTranspose2d (Cin, Cout, P, P): pixel (hi, wi) of a (1, 2, 3) grid holds e_(3 hi + wi)
        w = _int_weight((Ci, Co, P, P))
        nchw = layout == "DECONV_NCHW"
        x = torch.eye(Ci).view(1, 2, 3, Ci)
        want = F.conv_transpose2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=P).float()      # (1, Co, 4, 6)
        if not nchw:
            want = want.permute(0, 2, 3, 1).contiguous()
        pw = K.pack_weight(w.to(dev), None, comp, lay, N=Co * P * P, K=Ci, P=P, C_other=Co)
        out = torch.full((want.numel() + 8,), float("nan"), device=dev)
        K.deconv(x.reshape(Ci, Ci).contiguous().to(dev), pw, out, n_img=1, Hi=2, Wi=3, P=P, Cout=Co, nchw_out=nchw, act=L.ACT_NONE)
        o = out.cpu()
        assert torch.equal(o[:want.numel()].view(want.shape), want) and bool(torch.isnan(o[want.numel():]).all())
    else:
        if layout == "LINEAR":
            w = _int_weight((20, 12))
            N, Kd, want, args = 20, 12, w, dict()
        elif layout == "LINEAR_T":             # source (K, N) row-major
            w = _int_weight((12, 20))
            N, Kd, want, args = 20, 12, w.t(), dict()
        elif layout == "CONV_NHWC_T":          # Conv2d (Cout, Cin, P, P): n = (kh, kw, ci), k = co
            w = _int_weight((Co, Ci, P, P))
            N, Kd, want, args = Ci * P * P, Co, w.permute(2, 3, 1, 0).reshape(-1, Co), dict(P=P, C_other=Ci)
        elif layout == "DECONV_NHWC_T":        # ConvTranspose2d (Cin, Cout, P, P): n = ci, k = (kh, kw, co)
            w = _int_weight((Ci, Co, P, P))
            N, Kd, want, args = Ci, Co * P * P, w.permute(0, 2, 3, 1).reshape(Ci, -1), dict(P=P, C_other=Co)
        else:                                  # DECONV_NCHW_T: n = ci, k = (co, kh, kw)
            w = _int_weight((Ci, Co, P, P))
            N, Kd, want, args = Ci, Co * P * P, w.reshape(Ci, -1), dict(P=P, C_other=Co)
        want = want.contiguous()
        assert want.shape == (N, Kd)
        pw = K.pack_weight(w.to(dev), None, comp, lay, N=N, K=Kd, **args)
        out = torch.full((Kd + 1, N + 3), float("nan"), device=dev)
        K.linear(torch.eye(Kd).to(dev), pw, out, M=Kd, out_ld=N + 3)
        o = out.cpu()
        assert torch.equal(o[:Kd, :N], want.t().contiguous()), layout
        assert bool(torch.isnan(o[Kd]).all()) and bool(torch.isnan(o[:, N:]).all())
    assert bool((pw.bias == 0).all()) and pw.bias.numel() == pw.geom.n_pad
    assert len(set(w.reshape(-1).tolist())) > 30


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("N,Kd", [(20, 44), (100, 256), (132, 512)])
def test_pack_weight_layernorm_fold(dev, mode, N, Kd):
    """bias_out = b + W beta to the fp32 bar (an fp32 sum over K <= 512), zero in the padded entries; the packed matrix is W gamma: read back
    through identity rows (no LayerNorm in the read-back GEMM) it is W gamma rounded to the compute format, exactly."""
    K, L = _ops()
    comp = K.COMPUTE[mode]
    gen = torch.Generator().manual_seed(N * 1000 + Kd)
    w = torch.randn(N, Kd, generator=gen) / Kd ** 0.5
    b = torch.randn(N, generator=gen)
    gamma, beta = -4.0 + 3.0 * torch.randn(Kd, generator=gen), 2.0 + 5.0 * torch.randn(Kd, generator=gen)
    pw = K.pack_weight(w.to(dev), b.to(dev), comp, gamma=gamma.to(dev), beta=beta.to(dev))
    bias = pw.bias.cpu()
    assert bias.numel() == pw.geom.n_pad and bool((bias[N:] == 0).all())
    ref = b.double() + w.double() @ beta.double()
    rel, mx = R.errors(bias[:N], ref)
    record_parity(rel, mx, R.BARS["fp32"][0], mode, f"tante_pack_weight LN fold bias N={N} K={Kd}")
    _worst("k", "folded bias vs float64", rel, mx)
    assert rel < R.BARS["fp32"][0] and mx < R.BARS["fp32"][1], (rel, mx)
    zero_b = torch.zeros_like(pw.bias)
    out = torch.full((Kd, N), float("nan"), device=dev)
    K.linear(torch.eye(Kd).to(dev), K.PackedWeight(pw.w, zero_b, N, Kd, comp, pw.geom), out, M=Kd)
    wg = w * gamma[None, :]
    if mode == "bf16":
        wg = wg.to(torch.bfloat16).float()
    assert torch.equal(out.cpu(), wg.t().contiguous())


# ---- (l) refusals -----------------------------------------------------------------------------------------------------------------
def _refusal_descs():
    img = dict(B=1, n0=1, Ttot=1, Hin=4, Win=4, Cin=4, P=2, gap=0, off=0)
    dec = dict(n_img=1, Hi=4, Wi=4, Po=2, Cout=4)
    return [
        ("K513-bf16", "register-stationary limit", dict(mode="bf16", M=17, N=64, K=64), dict(K=513)),
        ("K513-fp32", "register-stationary limit", dict(mode="fp32", M=17, N=64, K=64), dict(K=513)),
        ("Hin%P", "bad patch geometry", dict(mode="fp32", N=64, a_mode="nchw", img=img), dict(Hin=5)),
        ("K!=CinPP", "K != Cin\\*P\\*P", dict(mode="fp32", N=64, a_mode="nchw", img=img), dict(K=12)),
        ("M-images", "M is not a whole number of images", dict(mode="fp32", N=64, a_mode="nhwc", img=img), dict(M=3)),
        ("N!=CoutPP", "N != Cout\\*P\\*P", dict(mode="fp32", K=64, e_mode="dnhwc", dec=dec), dict(Cout=3)),
        ("nchw-bf16-out", "NCHW output is fp32", dict(mode="bf16", K=64, e_mode="dnchw", dec=dec, out_dtype="bf16"), dict()),
        ("a_pad", "a_pad", dict(mode="bf16", N=64, a_mode="nchw", img=dict(img, Cin=16, P=4, Hin=8, Win=8)), dict(a_pad=1)),
        ("drop_p-smallM", "dropout / activation-gradient", dict(mode="bf16", a_dtype="bf16", M=130, N=64, K=128, res="other"), dict(drop_p=0.1)),
    ]


REFUSALS = _refusal_descs()


@pytest.mark.parametrize("name,msg,kw,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_output_untouched(dev, name, msg, kw, over):
    """What tante_gemm cannot serve raises with the C side's message before any launch: the NaN pre-fill of the output is untouched."""
    K, L = _ops()
    if name == "nchw-bf16-out":
        c = R.Case("l", name, **dict(kw, out_dtype="f32"))      # the case constructor routes (and would refuse): the valid fp32 twin, dtype flipped below
        over = dict(out_dtype=L.BF16)
    else:
        c = R.Case("l", name, **kw)
    inp = R.make_inputs(c)
    pw = pack(c, inp, dev)
    a_dev = inp.a_buf.to(dev)
    o_dev = torch.full((out_size(c) + 8,), float("nan"), device=dev)
    r_dev = None if inp.res_buf is None else inp.res_buf.to(dev)
    f = R.fields(c)
    g = L.Gemm()
    for fname, _ in L.Gemm._fields_:
        if hasattr(f, fname) and fname not in ("a", "out", "residual", "dact"):
            setattr(g, fname, getattr(f, fname))
    g.a, g.out, g.w, g.bias = a_dev.data_ptr(), o_dev.data_ptr(), pw.w.data_ptr(), pw.bias.data_ptr()
    if r_dev is not None:
        g.residual = r_dev.data_ptr()
    for k, v in over.items():
        setattr(g, k, v)
    with pytest.raises(R.Refused):
        R.gemm_route(g)
    with pytest.raises(RuntimeError, match=msg):
        L.check(L.lib().tante_gemm(C.byref(g), K._stream()), "tante_gemm")
    torch.cuda.synchronize()
    assert bool(torch.isnan(o_dev).all()), name


# ---- kernels.linear: res_ld -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_linear_wrapper_residual_leading_dimension(dev, mode):
    """kernels.linear(residual=, out_ld=): in place on a stream whose rows are out_ld apart the residual rows are out_ld apart too (the
    wrapper used to pass res_ld = N: row r of the residual was then read at r * N of the padded buffer); a separate residual is dense
    unless res_ld says otherwise."""
    K, L = _ops()
    comp = K.COMPUTE[mode]
    M, N, Kd, ld = 17, 64, 64, 72
    gen = torch.Generator().manual_seed(77)
    a, w, b = torch.randn(M, Kd, generator=gen), torch.randn(N, Kd, generator=gen) / 8.0, torch.randn(N, generator=gen)
    res = torch.randn(M, N, generator=gen)
    ref = a.double() @ w.double().t() + b.double() + res.double()
    pw = K.pack_weight(w.to(dev), b.to(dev), comp)
    bl2, bmx = R.BARS[mode]

    def check(out, what):
        o = out.cpu()
        rel, mx = R.errors(o[:M, :N], ref)
        record_parity(rel, mx, bl2, mode, f"kernels.linear {what}")
        assert rel < bl2 and mx < bmx, (what, rel, mx)
        assert bool(torch.isnan(o[M]).all()) and bool(torch.isnan(o[:, N:]).all()), what
    out = torch.full((M + 1, ld), float("nan"), device=dev)
    out[:M, :N] = res.to(dev)
    K.linear(a.to(dev), pw, out, M=M, residual=out, out_ld=ld)                       # in place: res_ld defaults to out_ld
    check(out, "residual is out, out_ld = 72")
    out = torch.full((M + 1, ld), float("nan"), device=dev)
    K.linear(a.to(dev), pw, out, M=M, residual=res.to(dev), out_ld=ld)               # a dense residual: res_ld defaults to N
    check(out, "dense residual, out_ld = 72")
    rb = torch.full((M, 80), float("nan"), device=dev)
    rb[:, :N] = res.to(dev)
    out = torch.full((M + 1, ld), float("nan"), device=dev)
    K.linear(a.to(dev), pw, out, M=M, residual=rb, out_ld=ld, res_ld=80)
    check(out, "residual rows 80 apart, out_ld = 72")
