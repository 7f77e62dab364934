"""GPU parity of every form of the axis propagators  y = x + W2 gelu_erf(W1 x + b1) + b2  (attn_backbone.py:111-119, 140-146), each alone,
against plain float64 torch: the kernels that open every backbone, in inference and in training.

* K.axis_hw_film          -- the H + W propagator that applies film(t) + s_emb + t_emb while it loads its planes from a frame-major cache:
                             B != T (the bt -> (b, t) split), a window inside a wider, per-plane padded cache (neither stride is the dense
                             one, the window does not start at the allocation), a FiLM table per slot, s_emb per token; every whole-tile
                             form and the generic kernel in bf16 and fp32 compute.
* K.axis_hw_train         -- the training forward: y AND the saved plane xm (after H alone) at all whole-tile pairs the launcher's switch has,
                             16-channel tiles and both wave counts of the 32-channel ones; the input bit-unchanged; y bit-equal to K.axis_hw.
* AxisMlpFn               -- the three backward routes (one fused launch: MFMA in bf16 compute for n = 16 / 32 / 48, vector fp32 for n = 4;
                             tante_axis_mlp_bwd + two tante_axis_wgrad_ws; tante_axis_mlp_bwd + the generic strided-lines wgrad), each with
                             returned gradients and with gradient slots, both forwards (tante_axis_mlp_oop, clone + in place), the host
                             option AXIS_BWD_FUSED, the slot form on the side stream, mixed slots, one weight used twice, the refusal of
                             n > 64.  Which route ran is counted
                             on the library's entries, not assumed.
* AxisHWFn                -- y, dx and all eight parameter gradients, returned and slot forms, shared weights, the C = 16 case in which the two
                             inner backward calls take different routes.
* non-contiguous inputs   -- a transposed view into both nodes: the node makes it dense once in forward and saves that copy.
* refusals                -- planes that fit no form of a kernel ((48, 48) everywhere, (64, 32) in the generic kernel): the C side answers
                             with an error return before any launch (test_planes_that_fit_no_form_are_refused).

References are written here from the maths (ref_prop, ref_hw, ref_film) and pinned to the CPU oracles by
tests/test_host_cpu.py::test_axis_node_references_match_the_oracles; test_axis_node_bars_reject_near_misses shows that the bars see the
errors these kernels are able to make and that an exact kernel with bf16 operands stays well inside them.

Bars.  fp32 results: those of test_hip_train_ops.py (2e-5 / 1e-4; sums over more than 4096 terms 1e-4 / 5e-4).  The forward of AxisMlpFn is
always fp32 (K.axis_mlp is called without a compute mode).  bf16 compute delivers fp32 tensors computed from bf16-rounded operands:
  forward (y, xm)             relative L2 < 1e-2, max-norm < 2e-2      (test_axis_hw_blocks.py / test_hip_parity.TOL["bf16"])
  dx                          relative L2 < 1e-2, max-norm < 2e-2      (test_axis_mlp_bwd_fused_against_float64; max-norm = 2 x, as above)
  parameter gradients         relative L2 < 2e-2, max-norm < 2e-2      (the same test; test_fused_axis_hw_training_forward_equals_two_axis_mlps)
"""
import functools
import math
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from test_hip_train_ops import close, randn, bars, dev  # noqa: F401  (dev: the module-scoped device fixture)
from test_hip_train_ops import F32_REL, F32_MAX
from test_hip_train_nodes import param, grad_of, exact, functional, Spy, SLOT_FILL  # noqa: F401
from test_axis_hw_blocks import _Options

pytestmark = pytest.mark.gpu

F32_BAR = (F32_REL, F32_MAX)
BF16_FWD = (1e-2, 2e-2)          # y, xm of the bf16 propagators
BF16_DX = (1e-2, 2e-2)
BF16_DP = (2e-2, 2e-2)
NAMES = ("w1", "b1", "w2", "b2")
AXIS_ENTRIES = ("tante_axis_mlp_oop", "tante_axis_mlp_c", "tante_axis_mlp_bwd_fused_ws", "tante_axis_mlp_bwd", "tante_axis_wgrad_ws",
                "tante_wgrad_ws", "tante_axis_hw_train")


# ---- float64 references (plain torch, from the maths; pinned by tests/test_host_cpu.py) ------------------------------------------------
def ref_prop(x, p, dim):
    """x + W2 gelu_erf(W1 x + b1) + b2 with the two Linear(n, n) acting along dimension `dim`; p = (w1, b1, w2, b2)."""
    w1, b1, w2, b2 = p
    v = x.movedim(dim, -1)
    h = F.gelu(v @ w1.t() + b1, approximate="none")
    return x + (h @ w2.t() + b2).movedim(-1, dim)


def ref_axis_mlp(x, p):
    """AxisMlpFn: the propagator along the middle axis of (outer, n, inner)."""
    return ref_prop(x, p, 1)


def ref_hw(x, vp, hp):
    """(BT, H, W, C): the H propagator, then the W propagator on its result -> (y, xm = the planes between the two)."""
    xm = ref_prop(x, vp, 1)
    return ref_prop(xm, hp, 2), xm


def ref_film(src, fa, fb, se):
    """tante.py:136-141 on a frame-major cache: src (T, B, HW, C), fa = 1 + scale(t) and fb = shift(t) + t_emb (T, C), se (HW, C)
    -> x (B, T, HW, C) with x[b, t, hw, c] = src[t, b, hw, c] fa[t, c] + fb[t, c] + se[hw, c]."""
    return (src * fa[:, None, None, :] + fb[:, None, None, :] + se[None, None]).transpose(0, 1)


# ---- what an exact kernel with bf16 operands would give (CPU; used by tests/test_host_cpu.py to size the inputs against the bars) ------
def bf(t):
    """The values of t rounded to bf16, in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def emul_prop(x, p, dim):
    """ref_prop in fp32 with both operands of each product rounded to bf16 (fp32 accumulation, exact GELU)."""
    w1, b1, w2, b2 = p
    v = x.movedim(dim, -1)
    h = F.gelu(bf(v) @ bf(w1).t() + b1, approximate="none")
    return x + (bf(h) @ bf(w2).t() + b2).movedim(-1, dim)


def emul_prop_bwd(x, dy, p, dim):
    """The backward of ref_prop for the cotangent dy, every product on bf16-rounded operands -> (dx, dw1, db1, dw2, db2)."""
    w1, b1, w2, _ = p
    n = x.shape[dim]
    v, g = x.movedim(dim, -1).reshape(-1, n), dy.movedim(dim, -1).reshape(-1, n)
    pre = bf(v) @ bf(w1).t() + b1
    h = F.gelu(pre, approximate="none")
    dpre = (bf(g) @ bf(w2)) * gelu_grad(pre)
    dx = g + bf(dpre) @ bf(w1)
    shape = x.movedim(dim, -1).shape
    return dx.reshape(shape).movedim(-1, dim), bf(dpre).t() @ bf(v), dpre.sum(0), bf(g).t() @ bf(h), g.sum(0)


def emul_hw(x, vp, hp):
    xm = emul_prop(x, vp, 1)
    return emul_prop(xm, hp, 2), xm


def emul_hw_bwd(x, G, vp, hp):
    """AxisHWFn's backward on bf16 operands: the W axis on the (bf16-accurate) saved plane, then the H axis on the input
    -> (dx, the eight parameter gradients in the node's order)."""
    xm = emul_prop(x, vp, 1)
    rw = emul_prop_bwd(xm, G, hp, 2)
    rh = emul_prop_bwd(x, rw[0], vp, 1)
    return rh[0], list(rh[1:]) + list(rw[1:])


# ---- seeded inputs (CPU, fp32: what the kernels read) and their float64 references, computed once and left unchanged -------------------
def mlp_params(n, gen):
    """(w1, b1, w2, b2) of one propagator: weights N(0, 1 / n), biases N(0, 0.3^2)."""
    return (randn((n, n), gen, scale=1.0 / math.sqrt(n)), randn((n,), gen, scale=0.3),
            randn((n, n), gen, scale=1.0 / math.sqrt(n)), randn((n,), gen, scale=0.3))


def f64(ts):
    return tuple(t.double() for t in ts)


FILM_BT = [(2, 3), (3, 2)]        # B != T: a transposed (b, t) order shows
FILM_PAD = 1                      # token rows of padding behind every plane of the cache: the batch stride is (HW + 1) C, not the plane size
FILM_PLANES = [(16, 16, 32, 0), (32, 32, 64, 0), (32, 32, 128, 0), (16, 64, 32, 0), (64, 32, 16, 0), (48, 48, 32, 0), (32, 32, 64, 32)]


@functools.lru_cache(maxsize=None)
def film_case(B, T, nH, nW, C):
    """The cache z (T + 1, B + 1, HW + FILM_PAD, C) whose window win = z[1:1 + T, :B, :HW] the kernel reads, the FiLM tables, s_emb, both
    propagators, and the float64 (y, xm, x after FiLM) of the window."""
    gen = torch.Generator().manual_seed(((B * 10 + T) * 100 + nH) * 100 + nW + C)
    HW = nH * nW
    z = randn((T + 1, B + 1, HW + FILM_PAD, C), gen)
    win = z[1:1 + T, :B, :HW]
    fa, fb, se = randn((T, C), gen, scale=0.5, shift=1.0), randn((T, C), gen), randn((HW, C), gen)
    vp, hp = mlp_params(nH, gen), mlp_params(nW, gen)
    x0 = ref_film(win.double(), fa.double(), fb.double(), se.double()).reshape(B * T, nH, nW, C)
    y, xm = ref_hw(x0, f64(vp), f64(hp))
    return NS(B=B, T=T, nH=nH, nW=nW, C=C, HW=HW, z=z, win=win, fa=fa, fb=fb, se=se, vp=vp, hp=hp, x0=x0, y=y, xm=xm)


TRAIN_BT = 3
def _train_fits(case):
    from tante_amd import _lib as L, kernels as K
    return K.axis_hw_train_supported(case[0], case[1], case[2], L.BF16)


TRAIN_ALL = ([(16 * h, 16 * w, 16, 0) for h in range(1, 5) for w in range(1, 5) if (h, w) not in ((3, 4), (4, 3), (4, 4))]      # the switch's 13 pairs
             + [(32, 32, 32, 32), (16, 48, 32, 32)])      # 32-channel tiles: 16 waves, 8 waves
TRAIN_CASES = [c for c in TRAIN_ALL if _train_fits(c)]
TRAIN_REFUSED = [c for c in TRAIN_ALL if not _train_fits(c)]      # (48, 48): in the switch, but the plane and its weights exceed 160 KiB of LDS


@functools.lru_cache(maxsize=None)
def hw_case(BT, nH, nW, C):
    """x (BT, nH, nW, C), both propagators, the cotangent G, and float64 y, xm, dx and the eight parameter gradients of sum(y G)."""
    gen = torch.Generator().manual_seed((BT * 100 + nH) * 100 + nW + 7 * C)
    x, G = randn((BT, nH, nW, C), gen), randn((BT, nH, nW, C), gen)
    vp, hp = mlp_params(nH, gen), mlp_params(nW, gen)
    xd = x.double().requires_grad_()
    pd = [t.double().requires_grad_() for t in vp + hp]
    y, xm = ref_hw(xd, pd[:4], pd[4:])
    grads = torch.autograd.grad((y * G.double()).sum(), [xd] + pd)
    return NS(BT=BT, nH=nH, nW=nW, C=C, x=x, G=G, vp=vp, hp=hp, y=y.detach(), xm=xm.detach(), dx=grads[0], dp=list(grads[1:]))


@functools.lru_cache(maxsize=None)
def mlp_case(outer, n, inner):
    """x (outer, n, inner), one propagator, the cotangent G, and float64 y, dx, dw1, db1, dw2, db2 of sum(y G)."""
    gen = torch.Generator().manual_seed((outer * 100 + n) * 10000 + inner)
    x, G = randn((outer, n, inner), gen), randn((outer, n, inner), gen)
    p = mlp_params(n, gen)
    xd = x.double().requires_grad_()
    pd = [t.double().requires_grad_() for t in p]
    y = ref_axis_mlp(xd, pd)
    grads = torch.autograd.grad((y * G.double()).sum(), [xd] + pd)
    return NS(outer=outer, n=n, inner=inner, x=x, G=G, p=p, y=y.detach(), dx=grads[0], dp=list(grads[1:]))


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def _mods():
    from tante_amd import _lib as L, autograd as A, kernels as K
    return L, A, K


class host_option:
    """Set a registered host option (tante_amd.options) for the block; put back what was there."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from tante_amd import options as O
        self.old = O.get_option(self.name)
        O.set_option(self.name, self.value)

    def __exit__(self, *a):
        from tante_amd import options as O
        O.set_option(self.name, self.old)


@pytest.fixture(autouse=True)
def _options_unchanged():
    """No option of the library or the package is left changed by a test."""
    if not torch.cuda.is_available():
        yield
        return
    from tante_amd import _lib as L, options as O
    lib_before = {k: L.get_option(k, d) for k, d in _Options.UNSET.items()}
    host_before = [O.get_option(k) for k in ("TANTE_AXIS_BWD_FUSED", "TANTE_WGRAD_SIDE_STREAM")]
    yield
    assert {k: L.get_option(k, d) for k, d in _Options.UNSET.items()} == lib_before
    assert [O.get_option(k) for k in ("TANTE_AXIS_BWD_FUSED", "TANTE_WGRAD_SIDE_STREAM")] == host_before


def on_dev(ts, dev):
    return [t.to(dev) for t in ts]


def refused(call, match):
    """The C side answers an unsupported shape with an error return (RuntimeError through _lib.check) before any launch."""
    with pytest.raises(RuntimeError, match=match):
        call()


# ---- A. FiLM-on-load H + W propagator ---------------------------------------------------------------------------------------------------
def _film_fits(form, plane):
    """The launcher's own shape rules (their Python mirrors: no GPU needed), so that the cases are split when the tests are collected."""
    from tante_amd import _lib as L, kernels as K
    nH, nW, C, _ = plane
    return K.axis_hw_train_supported(nH, nW, C, L.BF16) if form == "tile" else K.axis_hw_supported(nH, nW, C)


def _film_id(f, p):
    return f"{f}-{p[0]}x{p[1]}-C{p[2]}" + ("-ct32" if p[3] else "")


FILM_ALL = ([("tile", p) for p in FILM_PLANES]
            + [(f, p) for f in ("generic-bf16", "generic-fp32") for p in FILM_PLANES if p[3] == 0])      # (the generic kernel has no channel-tile option)
FILM_FORMS = [fp for fp in FILM_ALL if _film_fits(*fp)]
FILM_REFUSED = [fp for fp in FILM_ALL if not _film_fits(*fp)]      # (48, 48) in every form, (64, 32) in the generic kernel


def _film_opts(form, ct):
    return {"TANTE_AXIS_CT": ct} if form == "tile" else {"TANTE_AXIS_GENERIC": 1}


def _film_run(dev, c, compute, opts):
    """K.axis_hw_film on the window z[1:1 + T, :B, :HW] of the cache with its real strides, into a NaN-filled output."""
    L, _, K = _mods()
    z = c.z.to(dev)
    win = z[1:1 + c.T, :c.B, :c.HW]
    plane, padded = c.HW * c.C, (c.HW + FILM_PAD) * c.C
    assert (win.stride(0), win.stride(1), win.stride(2)) == ((c.B + 1) * padded, padded, c.C)
    assert win.stride(0) != c.B * plane and win.stride(1) != plane and padded % 4 == 0                        # neither stride is the dense one
    assert win.data_ptr() == z.data_ptr() + 4 * (c.B + 1) * padded                                            # ... nor the start the allocation's
    src = z[1:]       # the front end wants a dense tensor: the cache from the window's first plane on (the same address)
    assert src.data_ptr() == win.data_ptr() and src.is_contiguous() and not win.is_contiguous()
    out = torch.full((c.B * c.T, c.nH, c.nW, c.C), float("nan"), device=dev)
    with _Options(**opts):
        K.axis_hw_film(out, src, win.stride(0), win.stride(1), (c.fa.to(dev), c.fb.to(dev), c.se.to(dev), c.T, c.HW), c.B * c.T, c.nH, c.nW,
                       c.C, on_dev(c.vp, dev), on_dev(c.hp, dev), compute)
        torch.cuda.synchronize()
    assert torch.equal(z.cpu(), c.z), "the cache is read only"
    return out


@pytest.mark.parametrize("B,T", FILM_BT, ids=[f"B{b}T{t}" for b, t in FILM_BT])
@pytest.mark.parametrize("form,plane", FILM_FORMS, ids=[_film_id(f, p) for f, p in FILM_FORMS])
def test_film_on_load_against_float64(dev, form, plane, B, T):
    """x[b, t] = z[1 + t, b] fa[t] + fb[t] + se, then H, then W, in float64.  bf16 compute at the bf16 forward bar (an exact kernel with
    bf16 operands is at 2.5e-3 .. 2.8e-3 / <= 4.4e-3 on these inputs: under a third of it), the generic kernel in fp32 at the fp32 bar."""
    L, _, K = _mods()
    nH, nW, C, ct = plane
    c = film_case(B, T, nH, nW, C)
    compute = L.F32 if form == "generic-fp32" else L.BF16
    out = _film_run(dev, c, compute, _film_opts(form, ct))
    close(out, c.y, f"axis_hw_film {form} B={B} T={T} {nH}x{nW} C={C} ct={ct}", bar=F32_BAR if compute == L.F32 else BF16_FWD)


# ---- B. the training forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nH,nW,C,ct", TRAIN_CASES, ids=[f"{h}x{w}-C{c}" + ("-ct32" if ct else "") for h, w, c, ct in TRAIN_CASES])
def test_axis_hw_train_against_float64(dev, nH, nW, C, ct):
    """K.axis_hw_train: y and the saved plane xm (after H alone) against float64 at the bf16 forward bar; the input bit-unchanged; NaN
    pre-fills fully overwritten; y bit-equal to K.axis_hw's one-block schedule on a copy (the same kernel instance: xm is one more store)."""
    L, _, K = _mods()
    c = hw_case(TRAIN_BT, nH, nW, C)
    vp, hp = on_dev(c.vp, dev), on_dev(c.hp, dev)
    assert K.axis_hw_train_supported(nH, nW, C, L.BF16)
    x = c.x.to(dev)
    with _Options(TANTE_AXIS_CT=ct):
        y, xm = K.axis_hw_train(x, TRAIN_BT, nH, nW, C, vp, hp, L.BF16)
        y2, xm2 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        L.check(L.lib().tante_axis_hw_train(x.data_ptr(), y2.data_ptr(), xm2.data_ptr(), TRAIN_BT, nH, nW, C, *[t.data_ptr() for t in vp + hp],
                                            L.BF16, K._stream()), "tante_axis_hw_train")
        with _Options(TANTE_AXIS_BLOCKS=0):
            inplace = K.axis_hw(c.x.to(dev), TRAIN_BT, nH, nW, C, vp, hp, L.BF16)
        torch.cuda.synchronize()
    what = f"axis_hw_train {nH}x{nW} C={C} ct={ct}"
    exact(x.cpu(), c.x, what + ": the input")
    exact(y2, y, what + ": y into a NaN-filled buffer")
    exact(xm2, xm, what + ": xm into a NaN-filled buffer")
    exact(y, inplace, what + ": y = axis_hw (one-block schedule)")
    close(y, c.y, what + ": y", bar=BF16_FWD)
    close(xm, c.xm, what + ": xm", bar=BF16_FWD)


def test_planes_that_fit_no_form_are_refused(dev):
    """The cases of A and B whose plane fits no form of the kernel -- (48, 48): the (3, 3) entry of the launcher's switch needs 178 944
    bytes of LDS; (64, 32) in the generic kernel -- are answered by the C side with an error return before any launch: the output keeps
    its NaN pre-fill.  They are cases of this test, not skips of the parity tests."""
    L, _, K = _mods()
    assert sorted({p[:2] for _, p in FILM_REFUSED}) == [(48, 48), (64, 32)] and [c[:2] for c in TRAIN_REFUSED] == [(48, 48)]
    assert ("tile", (64, 32, 16, 0)) in FILM_FORMS and len(FILM_REFUSED) == 5
    for form, (nH, nW, C, ct) in FILM_REFUSED:
        c = film_case(2, 3, nH, nW, C)
        refused(lambda: _film_run(dev, c, L.F32 if form == "generic-fp32" else L.BF16, _film_opts(form, ct)), "tante_axis_hw")
    for nH, nW, C, ct in TRAIN_REFUSED:
        c = hw_case(TRAIN_BT, nH, nW, C)
        x = c.x.to(dev)
        y, xm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        ps = on_dev(c.vp + c.hp, dev)
        rc = L.lib().tante_axis_hw_train(x.data_ptr(), y.data_ptr(), xm.data_ptr(), TRAIN_BT, nH, nW, C, *[t.data_ptr() for t in ps], L.BF16, K._stream())
        torch.cuda.synchronize()
        assert rc == -2 and bool(torch.isnan(y).all()) and bool(torch.isnan(xm).all())
        refused(lambda: K.axis_hw_train(x, TRAIN_BT, nH, nW, C, ps[:4], ps[4:], L.BF16), "tante_axis_hw")
        exact(x.cpu(), c.x, f"axis_hw_train {nH}x{nW} C={C}: refused, the input untouched")


# ---- C. AxisMlpFn -----------------------------------------------------------------------------------------------------------------------
FUSED, AWGRAD, LINES = "fused", "axis_wgrad", "lines_wgrad"
#            outer, n, inner, compute, AXIS_BWD_FUSED, the route the node must take
MLP_CASES = [(3, 4, 1236, "fp32", True, FUSED), (3, 4, 1236, "bf16", True, FUSED),                      # vector fp32, every compute mode
             (3, 16, 448, "bf16", True, FUSED), (5, 32, 64, "bf16", True, FUSED), (6, 48, 128, "bf16", True, FUSED),      # MFMA, bf16 operands
             (3, 16, 448, "fp32", True, AWGRAD), (5, 32, 64, "fp32", True, AWGRAD), (6, 48, 128, "fp32", True, AWGRAD),
             (2, 64, 64, "fp32", True, AWGRAD), (5, 8, 160, "fp32", True, AWGRAD), (2, 3, 96, "fp32", True, AWGRAD),
             (3, 16, 96, "bf16", True, AWGRAD),                                                          # inner % 64 != 0: the fused launch refuses
             (3, 16, 448, "bf16", False, AWGRAD), (5, 32, 64, "bf16", False, AWGRAD), (6, 48, 128, "bf16", False, AWGRAD),
             (3, 4, 1236, "fp32", False, LINES), (3, 4, 1236, "bf16", False, LINES),                     # 1236 % 16 != 0
             (2, 7, 33, "fp32", True, LINES), (2, 3, 100, "fp32", True, LINES)]
MLP_IDS = [f"{o}x{n}x{i}-{m}" + ("" if fz else "-unfused") + f"-{r}" for o, n, i, m, fz, r in MLP_CASES]
ROUTE_CALLS = {FUSED: {"tante_axis_mlp_bwd_fused_ws": 1, "tante_axis_mlp_bwd": 0, "tante_axis_wgrad_ws": 0, "tante_wgrad_ws": 0},
               AWGRAD: {"tante_axis_mlp_bwd_fused_ws": 0, "tante_axis_mlp_bwd": 1, "tante_axis_wgrad_ws": 2, "tante_wgrad_ws": 0},
               LINES: {"tante_axis_mlp_bwd_fused_ws": 0, "tante_axis_mlp_bwd": 1, "tante_axis_wgrad_ws": 0, "tante_wgrad_ws": 2}}


def mlp_bars(c, mode, route):
    """(y, dx, parameter gradients): the MFMA launch alone computes on bf16 operands; everything else is fp32 arithmetic."""
    if route == FUSED and c.n != 4:
        assert mode == "bf16"
        return F32_BAR, BF16_DX, BF16_DP
    t = torch.empty(0)
    return F32_BAR, F32_BAR, bars(t, c.outer * c.inner)


def _mlp_params_on(c, dev, routes, gen):
    """The four parameters by their gradient routes -> ([tensor], [pre-fill or None])."""
    made = [param(t, dev, r, gen) for t, r in zip(c.p, routes)]
    return [m[0] for m in made], [m[1] for m in made]


def _mlp_run(dev, monkeypatch, c, mode, fused_opt, route, routes, view=False, side=False):
    """One forward + backward of AxisMlpFn alone; checks the launches and y, dx, dw1, db1, dw2, db2.  view: x arrives as a transposed
    (non-contiguous) view of a dense leaf.  side: with the host option TANTE_WGRAD_SIDE_STREAM on."""
    L, A, K = _mods()
    gen = torch.Generator().manual_seed(5)
    ps, fills = _mlp_params_on(c, dev, routes, gen)
    if view:
        leaf = c.x.transpose(1, 2).contiguous().to(dev).requires_grad_()
        x = leaf.transpose(1, 2)
        assert not x.is_contiguous() and torch.equal(x.detach().cpu(), c.x)
    else:
        leaf = x = c.x.to(dev).requires_grad_()
    spy = Spy(monkeypatch, entries=AXIS_ENTRIES)
    streams = []
    if side:      # which stream the two weight-gradient launches are issued on
        lib, counted = L.lib(), L.lib().tante_axis_wgrad_ws
        monkeypatch.setattr(lib, "tante_axis_wgrad_ws", lambda *a: (streams.append(a[-1]), counted(*a))[1])
    with host_option("TANTE_AXIS_BWD_FUSED", fused_opt), host_option("TANTE_WGRAD_SIDE_STREAM", side):
        y = A.AxisMlpFn.apply(x, *ps, c.outer, c.n, c.inner, K.COMPUTE[mode])
        oop = c.n <= 8 and c.inner % 4 == 0
        assert (spy.n["tante_axis_mlp_oop"], spy.n["tante_axis_mlp_c"]) == ((1, 0) if oop else (0, 1)), spy.n
        A.run_backward(functional(y, c.G.to(dev)))
        torch.cuda.synchronize()
    assert {k: spy.n[k] for k in ROUTE_CALLS[route]} == ROUTE_CALLS[route], (route, spy.n)
    if side:
        assert len(streams) == 2 and streams[0] == streams[1] == A._SIDE_STREAM.cuda_stream != K._stream(), streams
    what = (f"AxisMlpFn ({c.outer},{c.n},{c.inner}) {mode} {route} {'/'.join(sorted(set(routes)))}" + (" view" if view else "")
            + (" side stream" if side else ""))
    by, bx, bp = mlp_bars(c, mode, route)
    assert y.is_contiguous() and y.shape == c.x.shape
    close(y, c.y, what + ": y", bar=by)
    dx = leaf.grad.transpose(1, 2) if view else leaf.grad
    close(dx, c.dx, what + ": dx", bar=bx)
    for name, p, fill, ref in zip(NAMES, ps, fills, c.dp):
        close(grad_of(p, fill).float(), ref, what + ": d" + name, bar=bp)


@pytest.mark.parametrize("grads", ["returned", "slot"])
@pytest.mark.parametrize("outer,n,inner,mode,fused_opt,route", MLP_CASES, ids=MLP_IDS)
def test_axis_mlp_node_against_float64(dev, monkeypatch, outer, n, inner, mode, fused_opt, route, grads):
    """Every backward route of AxisMlpFn with all four gradients returned and with all four added into pre-filled slots (read back as slot
    minus pre-fill: an overwrite or a double add is far outside the bar)."""
    _mlp_run(dev, monkeypatch, mlp_case(outer, n, inner), mode, fused_opt, route, [grads] * 4)


@pytest.mark.parametrize("outer,n,inner,mode", [(3, 16, 448, "fp32"), (5, 8, 160, "fp32"), (3, 16, 96, "bf16")])
def test_axis_mlp_node_slots_on_the_side_stream(dev, monkeypatch, outer, n, inner, mode):
    """The slot form of the tante_axis_mlp_bwd + axis-wgrad route with TANTE_WGRAD_SIDE_STREAM on: the two weight-gradient launches go to
    the side stream (behind everything issued so far, with a workspace of that stream's own), the main stream re-joins when the backward
    pass ends, and the slots then hold pre-fill + gradient at the fp32 bars."""
    _mlp_run(dev, monkeypatch, mlp_case(outer, n, inner), mode, True, AWGRAD, ["slot"] * 4, side=True)


@pytest.mark.parametrize("outer,n,inner,mode,route", [(3, 16, 448, "bf16", FUSED), (3, 16, 448, "fp32", AWGRAD), (2, 7, 33, "fp32", LINES)])
def test_axis_mlp_node_mixed_slots(dev, monkeypatch, outer, n, inner, mode, route):
    """Only w1 and b2 have slots: the node returns all four gradients and autograd adds them -- onto the pre-fill for the two slots (so slot
    minus pre-fill is still the gradient, added once), into a fresh .grad for the others."""
    _mlp_run(dev, monkeypatch, mlp_case(outer, n, inner), mode, True, route, ["slot", "param", "param", "slot"])


@pytest.mark.parametrize("outer,n,inner,mode,route", [(3, 16, 448, "bf16", FUSED), (5, 8, 160, "fp32", AWGRAD), (2, 3, 100, "fp32", LINES),
                                                       (3, 4, 1236, "fp32", FUSED)])
def test_axis_mlp_node_shared_weights(dev, monkeypatch, outer, n, inner, mode, route):
    """y = f(f(x)) with ONE set of weights: the first use hands the node the Parameters (slot form: added into .grad by the kernels), the
    second a view of each (no slot: returned, and autograd adds them onto the same .grad).  The gradients are the sum of both uses."""
    L, A, K = _mods()
    c = mlp_case(outer, n, inner)
    xd = c.x.double().requires_grad_()
    pd = [t.double().requires_grad_() for t in c.p]
    ref = torch.autograd.grad((ref_axis_mlp(ref_axis_mlp(xd, pd), pd) * c.G.double()).sum(), [xd] + pd)
    ps, fills = _mlp_params_on(c, dev, ["slot"] * 4, torch.Generator().manual_seed(6))
    x = c.x.to(dev).requires_grad_()
    spy = Spy(monkeypatch, entries=AXIS_ENTRIES)
    y1 = A.AxisMlpFn.apply(x, *ps, outer, n, inner, K.COMPUTE[mode])
    y2 = A.AxisMlpFn.apply(y1, *[p.view_as(p) for p in ps], outer, n, inner, K.COMPUTE[mode])
    A.run_backward(functional(y2, c.G.to(dev)))
    torch.cuda.synchronize()
    assert {k: spy.n[k] for k in ROUTE_CALLS[route]} == {k: 2 * v for k, v in ROUTE_CALLS[route].items()}, spy.n
    _, bx, bp = mlp_bars(c, mode, route)
    what = f"AxisMlpFn twice ({outer},{n},{inner}) {mode} {route}"
    close(x.grad, ref[0], what + ": dx", bar=bx)
    for name, p, fill, r in zip(NAMES, ps, fills, ref[1:]):
        close(grad_of(p, fill).float(), r, what + ": d" + name, bar=bp)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_axis_mlp_node_refuses_long_axes_in_backward(dev, monkeypatch, mode):
    """(2, 100, 40): the forward runs (the LDS kernel) and is held to float64; the backward raises from the C side's refusal of n > 64
    before anything is launched -- no weight-gradient call follows, and the pre-filled slots stay bit-unchanged."""
    L, A, K = _mods()
    c = mlp_case(2, 100, 40)
    ps, fills = _mlp_params_on(c, dev, ["slot"] * 4, torch.Generator().manual_seed(7))
    x = c.x.to(dev).requires_grad_()
    spy = Spy(monkeypatch, entries=AXIS_ENTRIES)
    y = A.AxisMlpFn.apply(x, *ps, 2, 100, 40, K.COMPUTE[mode])
    close(y, c.y, f"AxisMlpFn (2,100,40) {mode}: y", bar=F32_BAR)
    with pytest.raises(RuntimeError, match="axis length 100 > 64"):
        A.run_backward(functional(y, c.G.to(dev)))
    torch.cuda.synchronize()
    assert spy.n["tante_axis_mlp_bwd"] == 1 and spy.n["tante_axis_mlp_bwd_fused_ws"] == spy.n["tante_axis_wgrad_ws"] == spy.n["tante_wgrad_ws"] == 0
    assert x.grad is None
    for name, p, fill in zip(NAMES, ps, fills):
        exact(p.grad.cpu(), fill, f"AxisMlpFn (2,100,40) {mode}: the slot of {name} after the refusal")


# ---- D. AxisHWFn ------------------------------------------------------------------------------------------------------------------------
HW_NODE_CASES = [(3, 16, 16, 64), (2, 32, 32, 64), (2, 16, 48, 64), (2, 48, 32, 64), (1, 64, 16, 64),
                 (3, 16, 32, 16)]       # C = 16: the W-axis backward (inner = 16) takes the three-launch route, the H-axis one stays fused
HW_NAMES = tuple("v" + k for k in NAMES) + tuple("h" + k for k in NAMES)


def hw_calls(c, fused_opt=True):
    """The backward launches AxisHWFn must make: per inner call (W axis: inner = C; H axis: inner = W C) the fused launch where it applies."""
    want = {k: 0 for k in ROUTE_CALLS[FUSED]}
    for n, inner in ((c.nW, c.C), (c.nH, c.nW * c.C)):
        route = FUSED if (fused_opt and inner % 64 == 0 and n in (16, 32, 48)) else (AWGRAD if inner % 16 == 0 else LINES)
        for k, v in ROUTE_CALLS[route].items():
            want[k] += v
    return want


def _hw_params_on(c, dev, routes, gen):
    made = [param(t, dev, r, gen) for t, r in zip(c.vp + c.hp, routes)]
    return [m[0] for m in made], [m[1] for m in made]


def _hw_run(dev, monkeypatch, c, routes, fused_opt=True, view=False):
    L, A, K = _mods()
    assert K.axis_hw_train_supported(c.nH, c.nW, c.C, L.BF16)
    ps, fills = _hw_params_on(c, dev, routes, torch.Generator().manual_seed(8))
    if view:
        leaf = c.x.transpose(1, 2).contiguous().to(dev).requires_grad_()
        x = leaf.transpose(1, 2)
        assert not x.is_contiguous() and torch.equal(x.detach().cpu(), c.x)
    else:
        leaf = x = c.x.to(dev).requires_grad_()
    spy = Spy(monkeypatch, entries=AXIS_ENTRIES)
    with host_option("TANTE_AXIS_BWD_FUSED", fused_opt):
        y = A.AxisHWFn.apply(x, *ps, c.BT, c.nH, c.nW, c.C, L.BF16)
        assert spy.n["tante_axis_hw_train"] == 1
        A.run_backward(functional(y, c.G.to(dev)))
        torch.cuda.synchronize()
    want = hw_calls(c, fused_opt)
    assert {k: spy.n[k] for k in want} == want, spy.n
    what = (f"AxisHWFn ({c.BT},{c.nH},{c.nW},{c.C}) {'/'.join(sorted(set(routes)))}" + ("" if fused_opt else " unfused") + (" view" if view else ""))
    close(y, c.y, what + ": y", bar=BF16_FWD)
    close(leaf.grad.transpose(1, 2) if view else leaf.grad, c.dx, what + ": dx", bar=BF16_DX)
    for name, p, fill, ref in zip(HW_NAMES, ps, fills, c.dp):
        close(grad_of(p, fill).float(), ref, what + ": d" + name, bar=BF16_DP)


@pytest.mark.parametrize("grads", ["returned", "slot"])
@pytest.mark.parametrize("BT,nH,nW,C", HW_NODE_CASES, ids=["x".join(map(str, s)) for s in HW_NODE_CASES])
def test_axis_hw_node_against_float64(dev, monkeypatch, BT, nH, nW, C, grads):
    """AxisHWFn alone: y, dx and the eight parameter gradients against float64 autograd at the bf16 train bars, the gradients being
    computed from a saved plane xm that is itself bf16-accurate (an exact bf16-operand evaluation stays under half of each bar:
    tests/test_host_cpu.py::test_axis_node_bars_reject_near_misses)."""
    _hw_run(dev, monkeypatch, hw_case(BT, nH, nW, C), [grads] * 8)


@pytest.mark.parametrize("BT,nH,nW,C", [(2, 32, 32, 64), (3, 16, 32, 16)], ids=["2x32x32x64", "3x16x32x16"])
def test_axis_hw_node_shared_weights(dev, monkeypatch, BT, nH, nW, C):
    """y = f(f(x)) with one set of weights: Parameters with slots for the first use, views of them (returned gradients) for the second."""
    L, A, K = _mods()
    c = hw_case(BT, nH, nW, C)
    xd = c.x.double().requires_grad_()
    pd = [t.double().requires_grad_() for t in c.vp + c.hp]
    ref = torch.autograd.grad((ref_hw(ref_hw(xd, pd[:4], pd[4:])[0], pd[:4], pd[4:])[0] * c.G.double()).sum(), [xd] + pd)
    ps, fills = _hw_params_on(c, dev, ["slot"] * 8, torch.Generator().manual_seed(9))
    x = c.x.to(dev).requires_grad_()
    spy = Spy(monkeypatch, entries=AXIS_ENTRIES)
    y1 = A.AxisHWFn.apply(x, *ps, BT, nH, nW, C, L.BF16)
    y2 = A.AxisHWFn.apply(y1, *[p.view_as(p) for p in ps], BT, nH, nW, C, L.BF16)
    A.run_backward(functional(y2, c.G.to(dev)))
    torch.cuda.synchronize()
    assert {k: spy.n[k] for k in ROUTE_CALLS[FUSED]} == {k: 2 * v for k, v in hw_calls(c).items()}, spy.n
    what = f"AxisHWFn twice ({BT},{nH},{nW},{C})"
    close(x.grad, ref[0], what + ": dx", bar=BF16_DX)
    for name, p, fill, r in zip(HW_NAMES, ps, fills, ref[1:]):
        close(grad_of(p, fill).float(), r, what + ": d" + name, bar=BF16_DP)


# ---- E. non-contiguous inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outer,n,inner,mode,route", [(3, 16, 448, "bf16", FUSED), (3, 16, 448, "fp32", AWGRAD), (3, 4, 1236, "fp32", FUSED)],
                         ids=["n16-bf16", "n16-fp32", "n4"])
def test_axis_mlp_node_takes_a_transposed_view(dev, monkeypatch, outer, n, inner, mode, route):
    """x as a .transpose view that only .contiguous() makes dense: n = 16 (clone + the in-place kernel) and n = 4 (the out-of-place
    kernel).  The node makes x dense once in forward and saves that copy: the same launches and the same bars as for a dense input.
    (Before, the clone kept the view's strides and the front end refused it: a RuntimeError ahead of any launch.)"""
    _mlp_run(dev, monkeypatch, mlp_case(outer, n, inner), mode, True, route, ["returned"] * 4, view=True)


@pytest.mark.parametrize("fused_opt", [True, False], ids=["fused", "unfused"])
def test_axis_hw_node_takes_a_transposed_view(dev, monkeypatch, fused_opt):
    """The same for AxisHWFn; with the fused backward off the saved input reaches tante_axis_mlp_bwd, which reads it as dense rows."""
    _hw_run(dev, monkeypatch, hw_case(2, 16, 48, 64), ["returned"] * 8, fused_opt=fused_opt, view=True)
