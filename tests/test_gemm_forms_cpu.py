"""No GPU: what tests/test_hip_gemm_forms.py relies on is itself held here.  The float64 references of tests/gemm_forms_ref.py against
oracle.tante_oracle; the restated dispatch (`gemm_route`) against the text of tante_amd/csrc/gemm.hip; the case list against the dispatch
(every route reached, or named with the test that covers it); the bars against wrong results of the kinds these kernels can produce."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import gemm_forms_ref as R
from conftest import ROOT

SRC = open(os.path.join(ROOT, "tante_amd", "csrc", "gemm.hip")).read()


@pytest.fixture(scope="module")
def evaluated():
    """Every case's operands and float64 reference, computed once."""
    out = {}
    for c in R.CASES:
        inp = R.make_inputs(c)
        out[c.id] = (inp, R.reference(c, inp))
    return out


def test_gemm_form_references_match_the_oracle(evaluated):
    """`reference` (written from include/tante_hip.h: gather, LayerNorm, product, activation, epilogue) agrees with the oracle's own
    operators -- layer_norm, gelu_erf / gelu_tanh, real_conv2d for both patch modes, real_transconv2d for both pixel shuffles, film() +
    s_emb with the tables of a real FiLM MLP -- to 1e-12 on every shape of the case list.  The placement of the operands in the flat
    buffers is held too: the header's addressing formulas find exactly the logical rows."""
    from oracle import tante_oracle as O
    acts = {"none": lambda x: x, "relu": torch.relu, "gelu_erf": O.gelu_erf, "gelu_tanh": O.gelu_tanh}
    gen = torch.Generator().manual_seed(3)

    # the oracle's stages pad by (P - 1) // 2 (enc_dec_cnn.py:66-81): at P <= 2 that is the descriptor's un-padded patch stage; at P = 4
    # the un-padded stage (TanteGemm.a_pad = 0, and every pixel shuffle) is torch's own operator with padding 0
    def conv(x, w, b, P):
        return O.real_conv2d(x, w, b, P, 0.0) if P <= 2 else F.conv2d(x, w, b, stride=P)

    def tconv(x, w, b, P):
        return O.real_transconv2d(x, w, b, P, 0.0) if P <= 2 else F.conv_transpose2d(x, w, b, stride=P)
    for c in R.CASES:
        inp, ref = evaluated[c.id]
        w, b = inp.w.double(), inp.bias.double()
        if c.img is not None:
            x = inp.x.double()
            y = conv(x, w, b, c.img["P"]).permute(0, 2, 3, 1).reshape(c.M, c.N)
            A = R.patch_rows(x, c.img["P"], c.a_mode == "nchw")
        else:
            A = inp.A.double()
            xin = O.layer_norm(A, inp.gamma.double(), inp.beta.double(), c.ln_eps) if c.ln else A
            if c.dec is None:
                y = O.linear(xin, w, b)
        assert torch.equal(R.gather_by_header(c, inp.a_buf), A), c.id
        if c.dec is not None:
            d = c.dec
            n_img = c.M // (d["Hi"] * d["Wi"])
            img = xin.view(n_img, d["Hi"], d["Wi"], c.K).permute(0, 3, 1, 2)
            y = acts[c.act](tconv(img, w, b, d["Po"]))
            want = y if c.e_mode == "dnchw" else y.permute(0, 2, 3, 1)
        elif c.e_mode == "film":
            B, T, HW = c.film
            fw = {f"condition_to_{n}.{i}.{p}": torch.randn(*s, generator=gen, dtype=torch.float64)
                  for n in ("scale", "shift") for i, p, s in ((0, "weight", (7, 1)), (0, "bias", (7,)), (2, "weight", (c.N, 7)), (2, "bias", (c.N,)))}
            t = torch.tensor([-2.0, -1.0, 0.5], dtype=torch.float64)[:T]
            inp2 = R.make_inputs(c)
            inp2.film_a = 1.0 + O._film_mlp(fw, "condition_to_scale", t)
            inp2.film_b = O._film_mlp(fw, "condition_to_shift", t)
            ref = R.reference(c, inp2)
            y5 = acts[c.act](y).view(B, T, 1, HW, c.N)
            want = (O.film(fw, y5, t) + inp2.s_emb.double()[None, None, None]).view(c.M, c.N)
        else:
            want = acts[c.act](y)
            if inp.res is not None:
                want = want + inp.res.double()
        rel, mx = R.errors(ref, want.reshape(ref.shape))
        assert rel < 1e-12 and mx < 1e-12, (c.id, rel, mx)


def test_gemm_route_matches_the_source():
    """`gemm_route` is a restatement: its tables and thresholds are read out of gemm.hip here, so that a new or removed line of launch_gemm's
    list, of try_small or of the lite forms, or a changed threshold, fails THIS test instead of leaving the case ids silently wrong."""
    vs = re.findall(r"return TANTE_V\((true|false), (AM_\w+), (EP_\w+)\);", SRC)
    assert [(ln == "true", am, ep) for ln, am, ep in vs] == R.KERNEL_VARIANTS
    sm = re.findall(r"TANTE_SM\((true|false), (EP_\w+)\);", SRC)
    assert [(ln == "true", ep) for ln, ep in sm] == R.SMALL_VARIANTS
    patch_ams = sorted(int(a) for a in set(re.findall(r"lite_patch<CB, (\d)>\(g", SRC)))
    assert patch_ams == [1, 2, 3, 4]
    lite = set()
    for ep, tr, am in re.findall(r"launch_lite<CB, (EP_\w+)(?:, (\d))?(?:, (\w+))?>\(g, n_tiles, s\)", SRC):
        for a in (patch_ams if am == "AM" else [int(am or 0)]):
            lite.add((ep, int(tr or 0), a))
    assert lite == set(R.LITE_PLAIN + R.LITE_DNCHW2 + R.LITE_TRAIN + R.LITE_PATCH)
    assert len(lite) == len(R.LITE_PLAIN) + len(R.LITE_DNCHW2) + len(R.LITE_TRAIN) + len(R.LITE_PATCH)
    # thresholds
    m = re.search(r'tante_opt\("TANTE_GEMM_SMALLM", (\d+)\)', SRC)
    assert m and int(m.group(1)) == R.SMALL_M_MAX
    m = re.search(r"if \(g\.M > lim \|\| g\.K != (\d+) \|\| am != AM_LIN \|\| \(flags & 3\) != 3 \|\| g\.e_mode != TANTE_E_LINEAR", SRC)
    assert m and int(m.group(1)) == R.SMALL_K
    assert "if constexpr (BF16 && CB == 16) {\n    if (try_small(" in SRC and R.pack_geom(64, R.SMALL_K, R.BF16).cb == 16
    lims = set(int(x) for x in re.findall(r"g\.M (?:<|>=) (\d+)", SRC))
    assert lims == {R.LITE_M_MIN}, lims
    m = re.search(r"if constexpr \(BF16 && CB >= (\d+) && CB <= (\d+)\) \{\n    if \(try_lite<CB>", SRC)
    assert m and (int(m.group(1)), int(m.group(2))) == (min(R.LITE_CBS), max(R.LITE_CBS))
    assert SRC.count("g.K != CB * 32") == 2 and "g.K == cb * 32" in SRC and "(cb == 8 || cb == 16)" in SRC and R.PATCH_LITE_CBS == (8, 16)
    assert "(g.K != 128 && g.K != 256 && g.K != 512)" in SRC
    assert "const int kb = (compute == TANTE_BF16) ? 32 : 16;" in SRC and "const int cb_max = (compute == TANTE_BF16) ? 16 : 32;" in SRC
    assert "return (512 / CB) < 64 ? (512 / CB) : 64;" in SRC
    assert "g.a_mode == TANTE_A_PATCH_NCHW && g.P == 2 && g.a_dtype == TANTE_F32 && g.Win % 2 == 0 && ((uintptr_t)g.a % 8) == 0" in SRC
    for mode, comp in (("bf16", R.BF16), ("fp32", R.F32)):
        for cb, K in R.K_OF_CB[mode].items():
            geo = R.pack_geom(64, K, comp)
            assert (geo.cb, geo.k_pad) == (cb, K)
        with pytest.raises(R.Refused):
            R.pack_geom(64, R.K_MAX + 1, comp)
    # the row limits, on either side
    f = R.fields(R.Case("t", "x", mode="bf16", M=R.SMALL_M_MAX, N=64, K=512))
    assert R.gemm_route(f).startswith("small<")
    f.M += 1
    assert R.gemm_route(f) == "kernel<bf16,CB16,noLN,AM_LIN,EP_LIN_NONE>"
    assert R.gemm_route(f, small_m=2048).startswith("small<")
    f = R.fields(R.Case("t", "x", mode="bf16", a_dtype="bf16", M=R.LITE_M_MIN, N=64, K=256))
    assert R.gemm_route(f) == "lite<CB8,EP_LIN_NONE,TR0,AM0>" and R.gemm_route(f, no_lite=True).startswith("kernel<bf16,CB8")
    f.M -= 1
    assert R.gemm_route(f).startswith("kernel<bf16,CB8")


def test_gemm_form_cases_reach_every_route():
    """Every line of the dispatch is reached by a case of the GPU list: every kernel template in both compute modes, `LN + none` and
    `no-LN + none` at every CB, every form of the small kernel, the plain lite forms and the four channels-first pixel-shuffle forms.  What
    is left to other files is named with the test that covers it, and is nothing else."""
    reached = {c.route for c in R.CASES}
    allr = R.all_routes()
    assert reached <= set(allr), reached - set(allr)
    for mode in ("bf16", "fp32"):
        for ln, am, ep in R.KERNEL_VARIANTS:
            t = f"{'LN' if ln else 'noLN'},{am},{ep}>"
            assert any(r.startswith(f"kernel<{mode},") and r.endswith(t) for r in reached), (mode, t)
        for cb in R.K_OF_CB[mode]:
            for t in ("LN,AM_LIN,EP_LIN_NONE", "noLN,AM_LIN,EP_LIN_NONE"):
                assert f"kernel<{mode},CB{cb},{t}>" in reached, (mode, cb, t)
    left = {}
    for r, fam in allr.items():
        if fam == "small":
            assert r in reached, r
        elif fam in ("lite", "lite-dnchw2"):
            assert any(R.route_template(r) == R.route_template(x) for x in reached), r
        elif fam != "kernel":
            left.setdefault(fam, []).append(r)
            assert r not in reached
    assert {c.route for c in R.CASES if c.route.startswith("lite<")} >= {"lite<CB4,EP_LIN_GELU_TANH,TR0,AM0>", "lite<CB8,EP_LIN_NONE,TR0,AM0>",
                                                                        "lite<CB16,EP_LIN_NONE,TR0,AM0>"}
    assert set(left) == set(R.COVERED_ELSEWHERE)
    for fam, (what, where) in R.COVERED_ELSEWHERE.items():
        for ref in re.findall(r"tests/(\w+)\.py::(\w+)", where):
            text = open(os.path.join(ROOT, "tests", ref[0] + ".py")).read()
            assert f"def {ref[1]}(" in text, ref
    # the shapes the issue sets
    ms = {c.M for c in R.CASES}
    ns = {c.N for c in R.CASES}
    assert {1, 17, 65, 130, 1024, 1025, 4096, 4097} <= ms and {1, 20, 64, 100, 132, 768, 36} <= ns
    assert {44, 100} <= {c.K for c in R.CASES}
    ids = [c.id for c in R.CASES]
    assert all(c.route in i for c, i in zip(R.CASES, ids))


def test_gemm_form_bars_reject_near_misses(evaluated):
    """On every case the exact-bf16 evaluation (both operands of every product rounded as the kernel rounds them, float64 accumulation) stays
    under half its bar: the bar leaves the kernel room for its fp32 accumulation only.  And each wrong result of the kinds these kernels can
    produce lies beyond twice the bar of at least one case that exercises it."""
    worst = {}
    for c in R.CASES:
        inp, ref = evaluated[c.id]
        rel, mx = R.errors(R.reference(c, inp, exact_bf16=True), ref)
        assert rel < 0.5 * c.bars[0] and mx < 0.5 * c.bars[1], (c.id, rel, mx)
        w = worst.setdefault((c.group, c.mode), [0.0, 0.0])
        w[0], w[1] = max(w[0], rel), max(w[1], mx)
    print({k: (f"{v[0]:.1e}", f"{v[1]:.1e}") for k, v in sorted(worst.items())})

    def beyond(c, bug, factor=2.0):
        inp, ref = evaluated[c.id]
        rel, mx = R.errors(R.reference(c, inp, bug=bug), ref)
        return rel > factor * c.bars[0] or mx > factor * c.bars[1]
    for bug, applies in R.WRONG.items():
        cases = [c for c in R.CASES if applies(c)]
        assert cases, bug
        seen = [c.id for c in cases if beyond(c, bug)]
        assert seen, bug
        for mode in ("bf16", "fp32"):      # every one of them is seen in both compute modes
            assert any(f"-{mode}-" in i for i in seen), (bug, mode)
    # what a format cannot see
    ln = [c for c in R.CASES if R.BLIND["ln_unbiased"](c)]
    assert all(beyond(c, "ln_unbiased") for c in ln if c.mode == "fp32") and any(c.K == 512 for c in ln if c.mode == "fp32")
    assert not any(beyond(c, "ln_unbiased") for c in ln if c.mode == "bf16" and c.K >= 64)
    ge = [c for c in R.CASES if R.BLIND["tanh_for_erf"](c)]
    assert any(beyond(c, "tanh_for_erf", 1.0) for c in ge if c.mode == "fp32")
    assert not any(beyond(c, "tanh_for_erf", 1.0) for c in ge if c.mode == "bf16") and any(c.mode == "bf16" for c in ge)
