"""GPU parity of the SHARED training nodes, each alone, against float64 autograd.

LinearFn, BranchOutFn, LayerNormFn, LayerNormSkipFn, ActFn, DropoutAddFn, PatchEmbedFn and DeconvFn (tante_amd/autograd.py) are the
training path of every model here; between them they choose among about twenty kernel and launch forms by shape, dtype, pointer
alignment and host options.  Until now those choices ran only inside whole-model gradient tests at the models' shapes.  Here every node
is called through its `.apply`, the way train_forward.py / cvit.py / spectral.py / fno.py call it, at the shapes where its branches change:

* LayerNormFn / LayerNormSkipFn -- the vector kernels (C 256 / 512, 16-byte aligned) and the generic one, the four-rows-per-workgroup
                                   row guard, bf16 and fp32 cotangents, the `dskip` operand in every form the host accepts.
* ActFn                         -- the 4-wide and the scalar forms of tante_act_fwd / tante_act_bwd, saturated and near-zero arguments.
* DropoutAddFn                  -- p = 0 (CViT's head), p > 0 with the mask restated from the node's seed, both kernel forms.
* LinearFn                      -- K chunks past 512 forward, N chunks past 512 backward, deferred and immediate weight gradients,
                                   gradient slots (pre-filled .grad) and returned gradients, one weight used twice (BPTT).
* BranchOutFn                   -- fused GEMM epilogues or tante_dropout_add / tante_act_bwd, the fp32 bias sum or the bf16 tiles' one.
* PatchEmbedFn / DeconvFn       -- the dense-row (im2col) path and the gathering path, act_in, both output layouts, both colsum forms.

Each case compares the forward output and EVERY gradient the node can produce for a random linear functional sum(out * G) with
torch.autograd on the plain operation in float64.  Inputs (and, in bf16 compute, the fp32 master weights) are CPU-seeded and rounded to
what the kernel reads, so the reference sees the same numbers.  The backward runs through autograd.run_backward.  The references below
are pinned to the CPU oracles by tests/test_host_cpu.py::test_train_node_references_match_the_oracles, and
test_train_node_bars_reject_near_misses shows that the bars see the errors these kernels are able to make.

Bars: those of test_hip_train_ops.py, by the dtype a tensor is delivered in (fp32 2e-5 / 1e-4; sums over more than 4096 terms
1e-4 / 5e-4; bf16 5e-3 / 1.6e-2).  A tensor delivered in fp32 but computed from an operand that the node itself rounds to bf16 is held
to the bf16 bar; each test's docstring names those tensors.
"""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.autograd import Function

from conftest import record_parity
from test_hip_train_ops import (close, zero_close, bars, randn, dev,  # noqa: F401  (dev: the module-scoped device fixture)
                                F32_REL, F32_MAX, F32_SUM_REL, F32_SUM_MAX, SUM_TERMS, BF16_REL, BF16_MAX)

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU = 0, 1, 2, 3      # tante_amd._lib.ACT_* (checked in _lib_mods)
F32_BAR, BF16_BAR = (F32_REL, F32_MAX), (BF16_REL, BF16_MAX)
LARGE_MEAN_BAR = (2e-4, 2e-4)       # see test_layernorm_large_mean
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def bar_for(dtype, terms=1, rounded=False):
    """The bar of a tensor delivered in `dtype`, one element of which sums `terms` products; rounded: the node computed it from an
    operand it rounds to bf16 itself."""
    if dtype == torch.bfloat16 or rounded:
        return BF16_BAR
    return (F32_SUM_REL, F32_SUM_MAX) if terms > SUM_TERMS else F32_BAR


# ---- float64 references (plain torch; pinned by tests/test_host_cpu.py) ----------------------------------------------------------------
def ref_ln(x, eps):
    return F.layer_norm(x, (x.shape[-1],), None, None, eps)


def ref_linear(a, W, b=None, res=None):
    y = F.linear(a, W, b)
    return y if res is None else res + y


def ref_act(x, act):
    if act == ACT_GELU_ERF:
        return F.gelu(x, approximate="none")
    if act == ACT_GELU_TANH:
        return F.gelu(x, approximate="tanh")
    if act == ACT_RELU:
        return F.relu(x)
    return x


def ref_dropout(y, keep, p):
    """keep: the 0 / 1 mask the kernel drew, restated from the node's seed (never sampled here)."""
    return y if keep is None else keep * y / (1.0 - p)


def ref_branch_out(pre, W, b, res, act, keep=None, p=0.0):
    return res + ref_dropout(F.linear(ref_act(pre, act), W, b), keep, p)


def ref_patch_embed(x_nchw, W, b, P, act_in=ACT_NONE):
    """(n, Cin, H, W) -> (n H/P W/P, Cout) channels-last rows of the kernel = stride = P convolution of act_in(x)."""
    y = F.conv2d(ref_act(x_nchw, act_in), W, b, stride=P)
    return y.permute(0, 2, 3, 1).reshape(-1, W.shape[0])


def ref_deconv(a, W, b, n_img, Hi, Wi, P, nchw_out):
    """(n Hi Wi, Cin) pixel rows -> the kernel = stride = P transposed convolution, (n, Cout, Hi P, Wi P) or channels-last."""
    y = F.conv_transpose2d(a.view(n_img, Hi, Wi, -1).permute(0, 3, 1, 2), W, b, stride=P)
    return y if nchw_out else y.permute(0, 2, 3, 1)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def _lib_mods():
    from tante_amd import _lib as L, autograd as A, kernels as K
    assert (L.ACT_NONE, L.ACT_GELU_ERF, L.ACT_GELU_TANH, L.ACT_RELU) == (ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU)
    return L, A, K


@pytest.fixture(autouse=True)
def _clean_packs():
    yield
    if torch.cuda.is_available():
        from tante_amd import autograd as A
        A.clear_pack_cache()


def _f64(t, dev):
    return t.detach().to(dev, torch.float64).requires_grad_()


def _bf16_values(t, mode):
    """fp32 master values that the bf16 GEMM's own rounding leaves unchanged (bf16 compute only)."""
    return t.to(torch.bfloat16).float() if mode == "bf16" else t


def exact(got, ref, what):
    """Bit-for-bit equality (a gradient that is passed through, a p = 0 dropout), recorded like every other comparison."""
    same = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref)
    record_parity(0.0 if same else 1.0, 0.0 if same else 1.0, 1e-30, "bf16" if got.dtype == torch.bfloat16 else "fp32", what + " (exact)")
    assert same, f"{what}: not bit-identical"


def misaligned(t, dev):
    """The same values on the device in a view that starts one element (4 or 2 bytes) into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def leaf(t, dev, off=False):
    """-> (tensor handed to the node, the leaf that collects its gradient, a function leaf.grad -> gradient in the tensor's shape)."""
    if not off:
        d = t.to(dev).requires_grad_()
        return d, d, lambda g: g
    base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    base[1:] = t.flatten().to(dev)
    base.requires_grad_()
    v = base[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0
    return v, base, lambda g: g[1:].view(t.shape)


class _Inject(Function):
    """Identity whose backward hands `g` on as it is (dtype and strides) instead of what arrives: the gradient of a skip operand in a form
    of the caller's choosing."""

    @staticmethod
    def forward(ctx, t, g):
        ctx.g = g
        return t.view_as(t)

    @staticmethod
    def backward(ctx, _):
        return ctx.g, None


SLOT_FILL = 8.0      # the pre-fill's spread: a tenth of the largest gradients here (|dW| ~ sqrt(2 x 4096)), so that an overwritten slot is
#                      far outside every bar (test_train_node_bars_reject_near_misses), and small enough that adding onto it in fp32 costs
#                      8 x 2^-24 ~ 5e-7 against gradients of size >= 5


def param(t, dev, route, gen):
    """A weight by one of the three routes its gradient can take: 'returned' (a plain tensor), 'param' (a Parameter whose .grad is None:
    returned too) or 'slot' (a Parameter whose .grad is pre-filled with seeded non-zero values the kernels add into).
    -> (tensor, pre-fill on the CPU or None)"""
    if t is None:
        return None, None
    if route == "returned":
        return t.to(dev).requires_grad_(), None
    p = torch.nn.Parameter(t.to(dev))
    if route == "param":
        return p, None
    fill = randn(t.shape, gen, scale=SLOT_FILL)
    p.grad = fill.to(dev)
    return p, fill


def grad_of(p, fill):
    """The gradient a route delivered, in float64: .grad, minus the pre-fill of a slot (so a double add shows as 2x, an overwrite as a
    missing pre-fill)."""
    assert p.grad is not None
    g = p.grad.detach().double().cpu()
    return g if fill is None else g - fill.double()


class Spy:
    """Counts calls on entries of the loaded library and on autograd._defer_wgrad (with its answers), and keeps what a node's backward
    returned -- which branch ran, not only what it computed."""

    def __init__(self, monkeypatch, node=None, entries=()):
        L, A, _ = _lib_mods()
        self.n = {e: 0 for e in entries}
        self.deferred = []
        self.returned = []
        lib = L.lib()
        for e in entries:
            orig = getattr(lib, e)

            def wrap(*a, _o=orig, _e=e):
                self.n[_e] += 1
                return _o(*a)
            monkeypatch.setattr(lib, e, wrap)
        orig_defer = A._defer_wgrad

        def defer(*a, **k):
            r = orig_defer(*a, **k)
            self.deferred.append(bool(r))
            return r
        monkeypatch.setattr(A, "_defer_wgrad", defer)
        if node is not None:
            orig_bwd = node.backward

            def bwd(ctx, *g):
                r = orig_bwd(ctx, *g)
                self.returned.append(r)
                return r
            monkeypatch.setattr(node, "backward", staticmethod(bwd))

    def flushes(self):
        return self.n.get("tante_wgrad_multi_ws", 0) + self.n.get("tante_wgrad_jobs_ws", 0)


WGRAD_ENTRIES = ("tante_wgrad_ws", "tante_wgrad_multi_ws", "tante_wgrad_jobs_ws")


def tr_shape(M, I, J):
    return M % 32 == 0 and I % 128 == 0 and J % 128 == 0


def keep_mask(n, p, seed, dev):
    """The 0 / 1 keep mask of flat indices 0 .. n - 1 at (p, seed): tante_dropout_add on ones and zeros, the method of
    test_dropout_add_of_ones_is_the_attention_keep_mask (test_gemm_training_epilogues proves the fused epilogue draws the same elements)."""
    L, _, K = _lib_mods()
    ones, zeros, out = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
    L.check(L.lib().tante_dropout_add(ones.data_ptr(), L.F32, zeros.data_ptr(), float(p), seed, n, out.data_ptr(), K._stream()), "dropout_add")
    torch.cuda.synchronize()
    assert bool(((out == 0) | ((out - 1.0 / (1.0 - p)).abs() < 1e-6)).all())
    return (out != 0).double()


def functional(out, G):
    """sum(out * G): the gradient that reaches `out` is G bit for bit, in out's dtype."""
    return (out.float() * G.float()).sum()


# ---- LayerNormFn / LayerNormSkipFn -----------------------------------------------------------------------------------------------------
LN_CS = [8, 100, 192, 256, 512, 768]        # 256 / 512: the vector kernels; the rest (and every misaligned pointer): the generic one
LN_MS = [1, 3, 5, 4097]                     # four rows per workgroup: 1, 3, 5 and 4097 end inside one
LN_SKIPS = ["fp32", "strided", "none", "bf16"]
# every C meets every M once; the output / cotangent dtype and the form of gskip rotate with them (a Latin square, not the product)
LN_CASES = [(C, LN_MS[(i + j) % 4], ("fp32", "bf16")[(i + j) % 2]) for i, C in enumerate(LN_CS) for j in range(4)]
LNS_CASES = [(C, LN_MS[(i + j) % 4], ("bf16", "fp32")[(i + j + j // 2) % 2], LN_SKIPS[j]) for i, C in enumerate(LN_CS) for j in range(4)]


def _ln_case(dev, M, C, odt, skip=None, off=False, shift=0.0, bar=None, seed=0):
    """skip None: LayerNormFn; else LayerNormSkipFn with gskip in that form.  The cotangent has the output's dtype (autograd casts any
    other to it before the node sees it), so fp32 / bf16 outputs are the fp32 / bf16 cotangent loads of the backward kernels."""
    _, A, _ = _lib_mods()
    g = torch.Generator().manual_seed(seed + 7919 * C + M)
    x = randn((M, C), g, shift=shift)
    G = randn((M, C), g, odt)
    Gs = randn((M, C), g, torch.bfloat16 if skip == "bf16" else torch.float32) if skip not in (None, "none") else None
    eps = 1e-5
    xd, xleaf, view = leaf(x, dev, off)
    tag = f"ln{'_skip ' + skip if skip else ''} M{M} C{C} {odt}{' +4B' if off else ''}{f' mean {shift:g}' if shift else ''}"
    if skip is None:
        xh = A.LayerNormFn.apply(xd, eps, odt)
        A.run_backward(functional(xh, G.to(dev)))
        dx = view(xleaf.grad)
    else:
        xh, xs = A.LayerNormSkipFn.apply(xd, eps, odt)
        exact(xs.detach(), xd.detach(), tag + " skip operand")
        if skip in ("bf16", "none"):
            # autograd casts a gradient to its tensor's dtype (fp32 here) and materialises a missing one as zeros on the way in, so a bf16
            # gskip and an absent one (None) reach the host's branches only through the node itself: call its backward as the engine
            # does, with exactly those arguments
            dx = xh.grad_fn.apply(G.to(dev), None if Gs is None else Gs.to(dev))[0]
        else:
            loss = functional(xh, G.to(dev))
            if skip == "fp32":
                loss = loss + _Inject.apply(xs, Gs.to(dev)).sum()
            else:
                gv = Gs.t().contiguous().to(dev).t()          # (M, C) view of a (C, M) buffer: the host makes it contiguous
                assert gv.shape == (M, C) and (not gv.is_contiguous() or M == 1 or C == 1)
                loss = loss + _Inject.apply(xs, gv).sum()
            A.run_backward(loss)
            dx = view(xleaf.grad)
    x64 = _f64(x, dev)
    y64 = ref_ln(x64, eps)
    y64.backward(G.to(dev, torch.float64))
    dx64 = x64.grad if Gs is None else x64.grad + Gs.to(dev, torch.float64)
    close(xh, y64, tag + " xhat", bar=bar if bar is not None else bar_for(odt))
    close(dx, dx64, tag + " dx", bar=bar if bar is not None else bar_for(torch.float32, C))


@pytest.mark.parametrize("C,M,odt", LN_CASES)
def test_layernorm_against_float64(dev, C, M, odt):
    """xhat in the output dtype, dx in fp32 (from the same cotangent numbers the reference sees: fp32 bar)."""
    _ln_case(dev, M, C, DT[odt])


@pytest.mark.parametrize("C,M,odt,skip", LNS_CASES)
def test_layernorm_skip_against_float64(dev, C, M, odt, skip):
    """dx = LayerNorm's data gradient + gskip in one kernel; gskip fp32 contiguous, bf16, a non-contiguous view, or absent."""
    _ln_case(dev, M, C, DT[odt], skip=skip, seed=1)


@pytest.mark.parametrize("odt", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [256, 512])
def test_layernorm_misaligned_takes_the_generic_kernel(dev, C, odt):
    """x in a view that starts 4 bytes into its storage: not the 16-byte loads of the vector kernels, the same bars as the aligned run."""
    _ln_case(dev, 37, C, DT[odt], off=True, seed=2)
    _ln_case(dev, 37, C, DT[odt], skip="fp32", off=True, seed=3)


def test_layernorm_skip_without_a_branch_gradient_is_gskip(dev):
    """g is None (the normalised output took no part in the loss): the node hands gskip on, the same tensor.  Through the engine the
    unused output's gradient is materialised as zeros and the kernel adds gskip to an exact zero: the same bits."""
    _, A, _ = _lib_mods()
    g = torch.Generator().manual_seed(11)
    x, Gs = randn((5, 256), g), randn((5, 256), g)
    xd = x.to(dev).requires_grad_()
    xh, xs = A.LayerNormSkipFn.apply(xd, 1e-5, torch.bfloat16)
    gs = Gs.to(dev)
    out = xh.grad_fn.apply(None, gs)
    assert out[0] is gs and all(o is None for o in out[1:])
    A.run_backward(_Inject.apply(xs, gs).sum())
    exact(xd.grad, gs, "ln_skip g None: dx is gskip")


@pytest.mark.parametrize("C", [192, 512])
def test_layernorm_large_mean(dev, C):
    """1000 + randn, the intent of test_layernorm_affine_large_mean: the row mean is 1000x the spread, so the fp32 row sum alone carries
    ~1000 * 2^-24 * sqrt(log2 C) ~ 2e-4 of the centred values' size at worst (the inputs are exact in both).  The bar is that
    conditioning, 2e-4 / 2e-4 as there; what it guards is the variance, which a one-pass E[x^2] - E[x]^2 would lose completely (~1e-1)."""
    _ln_case(dev, 4097, C, torch.float32, shift=1000.0, bar=LARGE_MEAN_BAR, seed=4)
    _ln_case(dev, 4097, C, torch.float32, skip="fp32", shift=1000.0, bar=LARGE_MEAN_BAR, seed=5)


# ---- ActFn -----------------------------------------------------------------------------------------------------------------------------
ACT_SPECIAL = [12.0, -12.0, 30.0, -30.0, 5e-4, -5e-4, 9e-4, -1e-4]      # saturated tails (derivative 1 / 0) and |x| < 1e-3
ACT_EXPECT = [1.0, 0.0, 1.0, 0.0]


def act_inputs(n, gen, dtype):
    """n values: the special ones first, then 1.5 randn (no exact zero: ReLU's derivative there is a convention)."""
    x = torch.cat([torch.tensor(ACT_SPECIAL, dtype=torch.float64), torch.randn(n - len(ACT_SPECIAL), generator=gen, dtype=torch.float64) * 1.5])
    x = x.to(dtype)
    assert bool((x != 0).all())
    return x


@pytest.mark.parametrize("n,off", [(2048, False), (2049, False), (2051, False), (2048, True)], ids=["4k", "4k+1", "4k+3", "4k misaligned"])
@pytest.mark.parametrize("idt,odt", [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "bf16")])
@pytest.mark.parametrize("act", [ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU], ids=["erf", "tanh", "relu"])
def test_act_against_float64(dev, act, idt, odt, n, off):
    """n = 4k takes the 4-wide kernels (two workgroups of 256 lanes), 4k + 1 / 4k + 3 and a misaligned input the scalar ones.  The bulk
    (1.5 randn) and the special values (+-12, +-30, |x| < 1e-3) are compared apart, so the tails' size does not hide the bulk's error; at
    +-12 and +-30 the derivative itself must be finite and within the bar of 1 / 0."""
    _, A, _ = _lib_mods()
    g = torch.Generator().manual_seed(100 * act + n)
    x = act_inputs(n, g, DT[idt])
    G = randn((n,), g, DT[odt], shift=0.0)
    G[:8] = torch.tensor([1.0, -1.5, 2.0, 0.75, 1.0, -1.0, 1.25, -0.5], dtype=G.dtype)
    xd, xleaf, view = leaf(x, dev, off)
    y = A.ActFn.apply(xd, act, DT[odt])
    A.run_backward(functional(y, G.to(dev)))
    d = view(xleaf.grad)
    x64 = _f64(x, dev)
    y64 = ref_act(x64, act)
    y64.backward(G.to(dev, torch.float64))
    tag = f"act{act} {idt}->{odt} n{n}{' +1 elem' if off else ''}"
    ns = len(ACT_SPECIAL)
    close(y[ns:], y64[ns:], tag + " y bulk", bar=bar_for(DT[odt]))
    close(y[:ns], y64[:ns], tag + " y special", bar=bar_for(DT[odt]))
    close(d[ns:], x64.grad[ns:], tag + " d bulk", bar=bar_for(DT[idt]))
    close(d[:ns], x64.grad[:ns], tag + " d special", bar=bar_for(DT[idt]))
    deriv = (d[:4].double() / G[:4].to(dev, torch.float64)).cpu()
    assert torch.isfinite(deriv).all()
    err = float((deriv - torch.tensor(ACT_EXPECT, dtype=torch.float64)).abs().max())
    record_parity(err, err, bar_for(DT[idt])[1], idt, tag + " derivative at +-12, +-30 against 1 / 0")
    assert err <= bar_for(DT[idt])[1], (deriv, err)


# ---- DropoutAddFn ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 33), (65, 33)], ids=["n%4=0", "n%4=1"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("ydt", ["fp32", "bf16"])
def test_dropout_add_against_float64(dev, ydt, p, shape):
    """out = res + keep y / (1 - p) with the mask restated from the node's seed; dy = keep dout / (1 - p) in y's dtype; dres is dout
    itself.  p = 0 (cvit.py's x + gelu(dense(x))) keeps every element and adds exactly."""
    _, A, _ = _lib_mods()
    M, N = shape
    g = torch.Generator().manual_seed(int(p * 100) + M)
    y, res, G = randn(shape, g, DT[ydt]), randn(shape, g), randn(shape, g)
    yd, rd = y.to(dev).requires_grad_(), res.to(dev).requires_grad_()
    out = A.DropoutAddFn.apply(yd, rd, p)
    seed = out.grad_fn.seed
    A.run_backward(functional(out, G.to(dev)))
    keep = keep_mask(M * N, p, seed, dev).view(M, N)
    tag = f"dropout_add {ydt} p{p} {M}x{N}"
    if p == 0.0:
        assert bool((keep == 1).all())
        exact(out.detach(), rd.detach() + yd.detach().float(), tag + " out = res + y")
    else:
        frac = float(keep.mean())
        assert abs(frac - (1 - p)) < 6 * math.sqrt(p * (1 - p) / (M * N)), frac      # a mask, not all ones: 6 sigma of the binomial
    y64, r64 = _f64(y, dev), _f64(res, dev)
    o64 = r64 + ref_dropout(y64, keep, p)
    o64.backward(G.to(dev, torch.float64))
    close(out, o64, tag + " out", bar=F32_BAR)
    close(yd.grad, y64.grad, tag + " dy", bar=bar_for(DT[ydt]))
    exact(rd.grad, G.to(dev), tag + " dres is dout")


# ---- LinearFn --------------------------------------------------------------------------------------------------------------------------
LIN_CASES = [  # M, N, K, bias, residual, route, TANTE_WGRAD_DEFER
    (77, 20, 44, True, True, "returned", True),          # odd everywhere
    (77, 20, 44, True, True, "slot", True),
    (300, 96, 1024, True, False, "slot", True),          # two K chunks (CViT's 16 x 16 patch embed: test_linear_fn_long_contraction's shape)
    (300, 96, 1100, False, True, "returned", True),      # three K chunks, ragged last
    (300, 96, 1100, True, False, "param", True),         # ... with the bias (packed with the first chunk only)
    (257, 1100, 64, True, False, "param", True),         # three dgrad chunks over N, ragged last
    (257, 1100, 64, True, True, "slot", True),
    (4096, 256, 256, True, False, "slot", True),         # bf16: _tr_shape holds, the weight gradient is deferred
    (4096, 256, 256, True, True, "slot", False),         # ... TANTE_WGRAD_DEFER off: immediate launch
    (4064, 256, 256, True, False, "slot", True),         # M % 32 == 0 but no other convenient divisor
    (4064, 256, 256, True, False, "returned", True),
    (4097, 128, 512, False, False, "slot", True),        # no bias: dW comes back through autograd onto the pre-filled .grad
    (4097, 128, 512, True, True, "returned", True),
]


def _with_option(name, value):
    import contextlib
    from tante_amd import options

    @contextlib.contextmanager
    def cm():
        old = options.get_option(name)
        options.set_option(name, value)
        try:
            yield
        finally:
            options.set_option(name, old)
    return cm()


@pytest.mark.parametrize("M,N,Kk,has_bias,has_res,route,defer", LIN_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_linear_against_float64(dev, monkeypatch, mode, M, N, Kk, has_bias, has_res, route, defer):
    """y = a W^T + b (+ residual), a requires grad in every case.  bf16 compute: a is bf16 and W holds bf16 values, so nothing the
    forward reads is rounded; y is fp32 with a residual and bf16 without.  With an fp32 y the node rounds the incoming dy to bf16 once
    for both backward GEMMs: dW and db (delivered in fp32) are then held to the bf16 bar, da is delivered in bf16 anyway.  With a bf16
    y the cotangent is exact and dW / db meet the fp32 bar.  dres must be dy bit for bit."""
    L, A, _ = _lib_mods()
    comp, adt = (L.BF16, torch.bfloat16) if mode == "bf16" else (L.F32, torch.float32)
    g = torch.Generator().manual_seed(M + 3 * N + 5 * Kk + has_res)
    a = randn((M, Kk), g, adt)
    W = _bf16_values(randn((N, Kk), g, scale=1.0 / math.sqrt(Kk)), mode)
    b = randn((N,), g) if has_bias else None
    res = randn((M, N), g) if has_res else None
    odt = torch.float32 if has_res else adt
    G = randn((M, N), g, odt)
    ad = a.to(dev).requires_grad_()
    Wp, Wfill = param(W, dev, route, g)
    bp, bfill = param(b, dev, route, g)
    rd = res.to(dev).requires_grad_() if has_res else None
    spy = Spy(monkeypatch, A.LinearFn, WGRAD_ENTRIES)
    with _with_option("TANTE_WGRAD_DEFER", int(defer)):
        out = A.LinearFn.apply(ad, Wp, bp, rd, comp, odt)
        assert out.dtype == odt
        A.run_backward(functional(out, G.to(dev)))
    torch.cuda.synchronize()
    a64, W64 = _f64(a, dev), _f64(W, dev)
    b64 = _f64(b, dev) if has_bias else None
    r64 = _f64(res, dev) if has_res else None
    o64 = ref_linear(a64, W64, b64, r64)
    o64.backward(G.to(dev, torch.float64))
    tag = f"linear {mode} {M}x{N}x{Kk}{' bias' if has_bias else ''}{' res' if has_res else ''} {route}{'' if defer else ' no-defer'}"
    dy_rounded = mode == "bf16" and odt == torch.float32
    close(out, o64, tag + " out", bar=bar_for(odt, Kk))
    close(ad.grad, a64.grad, tag + " da", bar=bar_for(adt, N, dy_rounded))
    close(grad_of(Wp, Wfill), W64.grad, tag + " dW", bar=bar_for(torch.float32, M, dy_rounded))
    if has_bias:
        close(grad_of(bp, bfill), b64.grad, tag + " db", bar=bar_for(torch.float32, M, dy_rounded),
              floor=G.to(dev, torch.float64).abs().sum(0))
    if has_res:
        exact(rd.grad, G.to(dev), tag + " dres is dy")
    # the branch this case is here for
    in_slots = route == "slot" and has_bias
    want_defer = in_slots and defer and mode == "bf16" and tr_shape(M, N, Kk)
    ret = spy.returned[0]
    assert len(spy.returned) == 1 and ret[0] is not None
    if in_slots:
        assert ret[1] is None and ret[2] is None, "gradients that went into their slots must not be returned as well"
    else:
        assert ret[1] is not None and (ret[2] is not None) == has_bias
    if want_defer:
        assert spy.deferred == [True] and spy.n["tante_wgrad_ws"] == 0 and spy.flushes() == 1, (spy.deferred, spy.n)
    else:
        assert True not in spy.deferred and spy.n["tante_wgrad_ws"] == 1 and spy.flushes() == 0, (spy.deferred, spy.n)


def test_linear_one_weight_used_twice_sums_into_its_slot(dev, monkeypatch):
    """BPTT: the same Parameters in two LinearFn calls of one graph, deferred: ONE shared launch at the end of the pass, and the slots
    hold pre-fill + the sum of both uses (dW / db from the exact bf16 cotangents: fp32 bar over 2 x 4096 terms)."""
    L, A, _ = _lib_mods()
    M, N, Kk = 4096, 256, 256
    g = torch.Generator().manual_seed(77)
    a1, a2 = randn((M, Kk), g, torch.bfloat16), randn((M, Kk), g, torch.bfloat16)
    W = _bf16_values(randn((N, Kk), g, scale=1.0 / math.sqrt(Kk)), "bf16")
    b = randn((N,), g)
    G1, G2 = randn((M, N), g, torch.bfloat16), randn((M, N), g, torch.bfloat16)
    Wp, Wfill = param(W, dev, "slot", g)
    bp, bfill = param(b, dev, "slot", g)
    a1d, a2d = a1.to(dev).requires_grad_(), a2.to(dev).requires_grad_()
    spy = Spy(monkeypatch, A.LinearFn, WGRAD_ENTRIES)
    y1 = A.LinearFn.apply(a1d, Wp, bp, None, L.BF16, torch.bfloat16)
    y2 = A.LinearFn.apply(a2d, Wp, bp, None, L.BF16, torch.bfloat16)
    A.run_backward(functional(y1, G1.to(dev)) + functional(y2, G2.to(dev)))
    torch.cuda.synchronize()
    a164, a264, W64, b64 = (_f64(t, dev) for t in (a1, a2, W, b))
    (ref_linear(a164, W64, b64) * G1.to(dev, torch.float64)).sum().backward()
    one_use = W64.grad.clone()
    (ref_linear(a264, W64, b64) * G2.to(dev, torch.float64)).sum().backward()
    tag = "linear bptt 2 x 4096x256x256"
    close(grad_of(Wp, Wfill), W64.grad, tag + " dW", bar=bar_for(torch.float32, 2 * M))
    close(grad_of(bp, bfill), b64.grad, tag + " db", bar=bar_for(torch.float32, 2 * M))
    close(a1d.grad, a164.grad, tag + " da1", bar=BF16_BAR)
    close(a2d.grad, a264.grad, tag + " da2", bar=BF16_BAR)
    assert float((one_use - W64.grad).norm() / W64.grad.norm()) > 0.5      # (one use alone is far outside the bar)
    assert spy.deferred == [True, True] and spy.n["tante_wgrad_ws"] == 0 and spy.flushes() == 1, (spy.deferred, spy.n)
    assert all(r[1] is None and r[2] is None for r in spy.returned)


# ---- BranchOutFn -----------------------------------------------------------------------------------------------------------------------
BO_SHAPES = [
    (4096, 256, 256),      # bf16: linear_train_epilogue_ok holds forward (K = 256) and backward (N = 256)
    (4096, 256, 512),
    (4095, 256, 256),      # just outside it (M): tante_dropout_add forward, tante_act_bwd backward
    (512, 200, 192),       # outside it on K
    (300, 1100, 64),       # N > 512: chunked dgrad, finished by tante_act_bwd also with act none
    (77, 20, 44),
]
# every shape meets act x p; bias and the gradient route rotate (three of four cases with a bias, two of four into slots)
BO_CASES = [(M, N, Kk, act, p, (si + ai + pi) % 4 != 3, "slot" if (si + ai) % 2 == 0 else "returned")
            for si, (M, N, Kk) in enumerate(BO_SHAPES) for ai, act in enumerate((ACT_NONE, ACT_GELU_TANH)) for pi, p in enumerate((0.0, 0.1))]


def epilogue_ok(mode, M, N, Kk):
    return mode == "bf16" and M >= 4096 and Kk in (128, 256, 512) and N % 4 == 0


def _branch_out(dev, monkeypatch, mode, M, N, Kk, act, p, has_bias, route, fp32_sums):
    L, A, _ = _lib_mods()
    comp, adt = (L.BF16, torch.bfloat16) if mode == "bf16" else (L.F32, torch.float32)
    g = torch.Generator().manual_seed(M + 3 * N + 5 * Kk + 7 * act + int(100 * p))
    pre = randn((M, Kk), g, adt)
    W = _bf16_values(randn((N, Kk), g, scale=1.0 / math.sqrt(Kk)), mode)
    b = randn((N,), g) if has_bias else None
    res, G = randn((M, N), g), randn((M, N), g)
    pd, rd = pre.to(dev).requires_grad_(), res.to(dev).requires_grad_()
    Wp, Wfill = param(W, dev, route, g)
    bp, bfill = param(b, dev, route, g)
    spy = Spy(monkeypatch, A.BranchOutFn, WGRAD_ENTRIES + ("tante_dropout_add", "tante_act_bwd", "tante_colsum", "tante_dropout_bwd"))
    with _with_option("TANTE_TRAIN_FP32_BIAS_SUMS", int(fp32_sums)):
        out = A.BranchOutFn.apply(pd, Wp, bp, rd, act, p, comp)
        n_dropout_add = spy.n["tante_dropout_add"]
        seed = out.grad_fn.seed
        A.run_backward(functional(out, G.to(dev)))
    torch.cuda.synchronize()
    keep = keep_mask(M * N, p, seed, dev).view(M, N) if p > 0.0 else None
    p64, W64, r64 = _f64(pre, dev), _f64(W, dev), _f64(res, dev)
    b64 = _f64(b, dev) if has_bias else None
    o64 = ref_branch_out(p64, W64, b64, r64, act, keep, p)
    G64 = G.to(dev, torch.float64)
    o64.backward(G64)
    tag = (f"branch_out {mode} {M}x{N}x{Kk} act{act} p{p}{' bias' if has_bias else ''} {route}"
           f"{'' if fp32_sums else ' bf16-bias-sums'}")
    bf = mode == "bf16"
    fused_fwd = p > 0.0 and Kk <= 512 and epilogue_ok(mode, M, N, Kk)
    fused_bwd = act != ACT_NONE and N <= 512 and epilogue_ok(mode, M, Kk, N)
    bias32 = bf and fp32_sums and p == 0.0 and has_bias
    out_rounded = bf and (act != ACT_NONE or (p > 0.0 and not fused_fwd))
    close(out, o64, tag + " out", bar=bar_for(torch.float32, Kk, out_rounded))
    close(pd.grad, p64.grad, tag + " dpre", bar=bar_for(adt, N))
    close(grad_of(Wp, Wfill), W64.grad, tag + " dW", bar=bar_for(torch.float32, M, bf))
    if has_bias:
        dy_abs = (G64 if keep is None else keep * G64 / (1.0 - p)).abs().sum(0)
        close(grad_of(bp, bfill), b64.grad, tag + " db", bar=bar_for(torch.float32, M, bf and not bias32), floor=dy_abs)
    exact(rd.grad, G.to(dev), tag + " dres is dout")
    # branches
    assert n_dropout_add == (1 if p > 0.0 and not fused_fwd else 0), (n_dropout_add, fused_fwd)
    assert spy.n["tante_dropout_bwd"] == (1 if p > 0.0 else 0)
    assert spy.n["tante_act_bwd"] == (1 if (N > 512 or (act != ACT_NONE and not fused_bwd)) else 0), (spy.n, fused_bwd)
    assert spy.n["tante_colsum"] == (1 if bias32 else 0), spy.n
    in_slots = route == "slot" and has_bias
    ret = spy.returned[0]
    assert ret[0] is not None and ret[3] is not None
    if in_slots:
        assert ret[1] is None and ret[2] is None
    else:
        assert ret[1] is not None and (ret[2] is not None) == has_bias
    if in_slots and bf and tr_shape(M, N, Kk):
        assert spy.deferred == [True] and spy.n["tante_wgrad_ws"] == 0 and spy.flushes() == 1, (spy.deferred, spy.n)
    else:
        assert True not in spy.deferred and spy.n["tante_wgrad_ws"] == 1 and spy.flushes() == 0, (spy.deferred, spy.n)


@pytest.mark.parametrize("M,N,Kk,act,p,has_bias,route", BO_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_branch_out_against_float64(dev, monkeypatch, mode, M, N, Kk, act, p, has_bias, route):
    """out = res + dropout_p(act(pre) W^T + b): out, dpre, dW, db, and dres = dout bit for bit.
    fp32 compute: every tensor at the fp32 bar.  bf16 compute (pre bf16, W bf16 values, out fp32), the node's own roundings per tensor:
    * out: act(pre) is stored in bf16 (act != none), and on the unfused dropout path the product is stored in bf16 before
      tante_dropout_add reads it: bf16 bar in those cases; with act none and p = 0 or the fused epilogue nothing is rounded: fp32 bar.
    * dpre: delivered in bf16.
    * dW: from the bf16 copy of dout / (1 - p) (tante_dropout_bwd or tante_act_fwd writes it): bf16 bar.
    * db: p = 0 with TANTE_TRAIN_FP32_BIAS_SUMS: the fp32 column sum of dout, fp32 bar; otherwise summed from the bf16 copy: bf16 bar.
      A column sum cancels (autograd.py names 12 % on g15), so it is measured against max(|db|, 1e-2 sum |dy|)."""
    _branch_out(dev, monkeypatch, mode, M, N, Kk, act, p, has_bias, route, True)


@pytest.mark.parametrize("M,N,Kk,act,has_bias,route", [(M, N, Kk, act, True, route) for (M, N, Kk, act, p, hb, route) in BO_CASES if p == 0.0])
def test_branch_out_bias_from_the_bf16_tiles(dev, monkeypatch, M, N, Kk, act, has_bias, route):
    """TANTE_TRAIN_FP32_BIAS_SUMS off, bf16, p = 0: db comes from the weight-gradient kernel's staged bf16 tiles (bf16 bar, no
    tante_colsum launch); everything else as above."""
    _branch_out(dev, monkeypatch, "bf16", M, N, Kk, act, 0.0, has_bias, route, False)


# ---- PatchEmbedFn ----------------------------------------------------------------------------------------------------------------------
PE_CASES = [  # n_img, Cin, Cout, Ho, Wo, P, nchw, mode, out dtype, act_in, route
    # the generic shape (8 x 12 patches), every P in both layouts and both compute modes
    (2, 6, 10, 8, 12, 2, True, "fp32", "fp32", ACT_NONE, "returned"), (2, 6, 10, 8, 12, 2, False, "bf16", "bf16", ACT_NONE, "slot"),
    (2, 6, 10, 8, 12, 4, True, "bf16", "bf16", ACT_NONE, "slot"), (2, 6, 10, 8, 12, 4, False, "fp32", "fp32", ACT_NONE, "param"),
    (2, 6, 10, 8, 12, 8, True, "fp32", "fp32", ACT_NONE, "slot"), (2, 6, 10, 8, 12, 8, False, "bf16", "fp32", ACT_NONE, "returned"),
    (2, 6, 10, 8, 12, 2, True, "bf16", "fp32", ACT_NONE, "returned"), (2, 6, 10, 8, 12, 2, False, "fp32", "fp32", ACT_NONE, "slot"),
    (2, 6, 10, 8, 12, 4, True, "fp32", "fp32", ACT_NONE, "slot"), (2, 6, 10, 8, 12, 4, False, "bf16", "bf16", ACT_NONE, "returned"),
    (2, 6, 10, 8, 12, 8, True, "bf16", "bf16", ACT_NONE, "param"), (2, 6, 10, 8, 12, 8, False, "fp32", "fp32", ACT_NONE, "returned"),
    # channels-last bf16, M = 64, Cout = 128, Cin P P = 128: the dense im2col path; into slots -> deferred; returned -> immediate
    (2, 8, 128, 8, 4, 4, False, "bf16", "bf16", ACT_NONE, "slot"), (2, 8, 128, 8, 4, 4, False, "bf16", "fp32", ACT_NONE, "returned"),
    # one image row less: M = 56, _tr_shape fails, the gathering path
    (2, 8, 128, 7, 4, 4, False, "bf16", "bf16", ACT_NONE, "slot"),
    # act_in: the node applies GELU itself and dx is the gradient of the PRE-activation
    (2, 8, 10, 8, 12, 2, False, "fp32", "fp32", ACT_GELU_ERF, "returned"), (2, 8, 10, 8, 12, 4, False, "bf16", "bf16", ACT_GELU_ERF, "slot"),
    (2, 8, 128, 8, 4, 4, False, "bf16", "bf16", ACT_GELU_ERF, "slot"),
]


@pytest.mark.parametrize("n_img,Cin,Cout,Ho,Wo,P,nchw,mode,odt,act_in,route", PE_CASES)
def test_patch_embed_against_float64(dev, monkeypatch, n_img, Cin, Cout, Ho, Wo, P, nchw, mode, odt, act_in, route):
    """Kernel = stride = P convolution: out (rows, Cout), dx, dW, db.  bf16 compute: W holds bf16 values; a channels-last x is bf16, a
    channels-first x is the fp32 input frame holding bf16 values (its dx is fp32).  The node's roundings, per tensor:
    * an fp32 `out` makes the cotangent fp32, which both backward kernels round to bf16: dx, dW, db at the bf16 bar in that case;
    * act_in: act(pre) is stored in x's dtype, bf16: out (if fp32), dW at the bf16 bar.
    With a bf16 cotangent and no act_in nothing is rounded: dW, db and a channels-first dx meet the fp32 bar."""
    L, A, _ = _lib_mods()
    comp, adt = (L.BF16, torch.bfloat16) if mode == "bf16" else (L.F32, torch.float32)
    odt = DT[odt]
    Hin, Win, Kk = Ho * P, Wo * P, Cin * P * P
    M = n_img * Ho * Wo
    g = torch.Generator().manual_seed(Cin + 3 * Cout + 5 * P + 7 * M + nchw)
    xdt = torch.float32 if nchw else adt
    x = randn((n_img, Cin, Hin, Win) if nchw else (n_img, Hin, Win, Cin), g, adt).to(xdt)
    W = _bf16_values(randn((Cout, Cin, P, P), g, scale=1.0 / math.sqrt(Kk)), mode)
    b = randn((Cout,), g)
    G = randn((M, Cout), g, odt)
    xd = x.to(dev).requires_grad_()
    Wp, Wfill = param(W, dev, route, g)
    bp, bfill = param(b, dev, route, g)
    spy = Spy(monkeypatch, A.PatchEmbedFn, WGRAD_ENTRIES + ("tante_im2col",))
    out = A.PatchEmbedFn.apply(xd, Wp, bp, n_img, Hin, Win, Cin, P, nchw, comp, odt, act_in)
    assert out.shape == (M, Cout) and out.dtype == odt
    A.run_backward(functional(out, G.to(dev)))
    torch.cuda.synchronize()
    x64, W64, b64 = _f64(x, dev), _f64(W, dev), _f64(b, dev)
    o64 = ref_patch_embed(x64 if nchw else x64.permute(0, 3, 1, 2), W64, b64, P, act_in)
    o64.backward(G.to(dev, torch.float64))
    tag = f"patch_embed {mode} {'nchw' if nchw else 'nhwc'} n{n_img} {Cin}->{Cout} {Ho}x{Wo} P{P} out {odt} act_in{act_in} {route}"
    bf = mode == "bf16"
    g_rounded = bf and odt == torch.float32
    a_rounded = bf and act_in != ACT_NONE
    close(out, o64, tag + " out", bar=bar_for(odt, Kk, a_rounded))
    close(xd.grad, x64.grad, tag + " dx", bar=bar_for(xdt, Cout, g_rounded))
    close(grad_of(Wp, Wfill), W64.grad, tag + " dW", bar=bar_for(torch.float32, M, g_rounded or a_rounded))
    close(grad_of(bp, bfill), b64.grad, tag + " db", bar=bar_for(torch.float32, M, g_rounded), floor=G.to(dev, torch.float64).abs().sum(0))
    dense = bf and not nchw and tr_shape(M, Cout, Kk)
    assert spy.n["tante_im2col"] == (1 if dense else 0), spy.n
    ret = spy.returned[0]
    if route == "slot":
        assert ret[1] is None and ret[2] is None
    else:
        assert ret[1] is not None and ret[2] is not None
    if dense and route == "slot":
        assert spy.deferred == [True] and spy.n["tante_wgrad_ws"] == 0 and spy.flushes() == 1, (spy.deferred, spy.n)
    else:
        assert True not in spy.deferred and spy.n["tante_wgrad_ws"] == 1 and spy.flushes() == 0, (spy.deferred, spy.n)


@pytest.mark.parametrize("nchw,Cin", [(True, 8), (False, 6)])
def test_patch_embed_refuses_act_in_it_cannot_fold(dev, nchw, Cin):
    """act_in needs a contiguous channels-last input with Cin % 4 == 0: anything else is an error, not an unactivated convolution."""
    L, A, _ = _lib_mods()
    x = torch.randn((2, Cin, 8, 8) if nchw else (2, 8, 8, Cin), device=dev, requires_grad=True)
    W, b = torch.randn(10, Cin, 2, 2, device=dev, requires_grad=True), torch.zeros(10, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="act_in"):
        A.PatchEmbedFn.apply(x, W, b, 2, 8, 8, Cin, 2, nchw, L.F32, torch.float32, ACT_GELU_ERF)
    record_parity(0.0, 0.0, 1.0, "fp32", f"patch_embed act_in refused ({'nchw' if nchw else 'nhwc'}, Cin {Cin})")


# ---- DeconvFn --------------------------------------------------------------------------------------------------------------------------
DC_CASES = [  # n_img, Cin, Cout, Hi, Wi, P, nchw_out, mode, a dtype, out dtype, route
    # the generic shape, both P, both layouts, both compute modes
    (2, 10, 6, 5, 7, 2, True, "fp32", "fp32", "fp32", "returned"), (2, 10, 6, 5, 7, 2, False, "bf16", "bf16", "bf16", "slot"),
    (2, 10, 6, 5, 7, 4, True, "bf16", "bf16", "fp32", "slot"), (2, 10, 6, 5, 7, 4, False, "fp32", "fp32", "fp32", "param"),
    (2, 10, 6, 5, 7, 2, True, "bf16", "bf16", "fp32", "returned"), (2, 10, 6, 5, 7, 2, False, "fp32", "fp32", "fp32", "slot"),
    (2, 10, 6, 5, 7, 4, True, "fp32", "fp32", "fp32", "slot"), (2, 10, 6, 5, 7, 4, False, "bf16", "bf16", "bf16", "returned"),
    (2, 10, 8, 5, 7, 2, False, "bf16", "bf16", "fp32", "param"),        # channels-last with an fp32 output: an fp32 cotangent in bf16 compute
    # channels-first, inner = 80 x 64 = 5120 > 4096: two chunks of the bias column sum
    (1, 8, 4, 20, 16, 4, True, "fp32", "fp32", "fp32", "returned"),
    # bf16 channels-last, N = 32 x 4 = 128, M = 64, Cin = 128: the cols path, a in bf16 and in fp32 (rounded for the weight gradient only)
    (1, 128, 32, 8, 8, 2, False, "bf16", "bf16", "bf16", "slot"), (1, 128, 32, 8, 8, 2, False, "bf16", "fp32", "bf16", "slot"),
    (1, 128, 32, 8, 8, 2, False, "bf16", "bf16", "bf16", "returned"),
    # N = 64 x 16 = 1024 > 512: leaves the cols path; the data gradient contracts over N in chunks
    (1, 128, 64, 8, 8, 4, False, "bf16", "bf16", "bf16", "slot"), (1, 128, 64, 8, 8, 4, True, "fp32", "fp32", "fp32", "returned"),
    (1, 128, 64, 8, 8, 4, False, "fp32", "fp32", "fp32", "slot"),
]


@pytest.mark.parametrize("n_img,Cin,Cout,Hi,Wi,P,nchw_out,mode,a_dt,odt,route", DC_CASES)
def test_deconv_against_float64(dev, monkeypatch, n_img, Cin, Cout, Hi, Wi, P, nchw_out, mode, a_dt, odt, route):
    """Kernel = stride = P transposed convolution: out, da, dW, db (tante_colsum with inner = 1 channels-last, inner = H W channels-first).
    bf16 compute: W holds bf16 values.  The node's roundings, per tensor:
    * an fp32 `a` (the first stage reads the fp32 residual stream) is rounded to bf16 by the forward GEMM and, on the cols path, by the
      host for the weight gradient: out and dW at the bf16 bar; da (fp32, from exact bf16 cotangents) at the fp32 bar;
    * an fp32 output (channels-first always) makes the cotangent fp32, which both backward GEMMs round: da, dW at the bf16 bar.
    db is the column sum of the cotangent as it arrives: fp32 bar."""
    L, A, _ = _lib_mods()
    comp = L.BF16 if mode == "bf16" else L.F32
    a_dt, odt = DT[a_dt], (torch.float32 if nchw_out else DT[odt])
    M, N = n_img * Hi * Wi, Cout * P * P
    g = torch.Generator().manual_seed(Cin + 3 * Cout + 5 * P + 7 * M + nchw_out)
    a = randn((M, Cin), g, a_dt)
    W = _bf16_values(randn((Cin, Cout, P, P), g, scale=1.0 / math.sqrt(Cin)), mode)
    b = randn((Cout,), g)
    oshape = (n_img, Cout, Hi * P, Wi * P) if nchw_out else (n_img, Hi * P, Wi * P, Cout)
    G = randn(oshape, g, odt)
    ad = a.to(dev).requires_grad_()
    Wp, Wfill = param(W, dev, route, g)
    bp, bfill = param(b, dev, route, g)
    spy = Spy(monkeypatch, A.DeconvFn, WGRAD_ENTRIES + ("tante_im2col", "tante_colsum"))
    out = A.DeconvFn.apply(ad, Wp, bp, n_img, Hi, Wi, P, nchw_out, comp, odt)
    assert out.shape == oshape and out.dtype == odt
    A.run_backward(functional(out, G.to(dev)))
    torch.cuda.synchronize()
    a64, W64, b64 = _f64(a, dev), _f64(W, dev), _f64(b, dev)
    o64 = ref_deconv(a64, W64, b64, n_img, Hi, Wi, P, nchw_out)
    G64 = G.to(dev, torch.float64)
    o64.backward(G64)
    tag = f"deconv {mode} {'nchw' if nchw_out else 'nhwc'} n{n_img} {Cin}->{Cout} {Hi}x{Wi} P{P} a {a_dt} out {odt} {route}"
    bf = mode == "bf16"
    a_rounded = bf and a_dt == torch.float32
    g_rounded = bf and odt == torch.float32
    close(out, o64, tag + " out", bar=bar_for(odt, Cin, a_rounded))
    close(ad.grad, a64.grad, tag + " da", bar=bar_for(a_dt, N, g_rounded))
    close(grad_of(Wp, Wfill), W64.grad, tag + " dW", bar=bar_for(torch.float32, M, a_rounded or g_rounded))
    sum_dims = (0, 2, 3) if nchw_out else (0, 1, 2)
    close(grad_of(bp, bfill), b64.grad, tag + " db", bar=bar_for(torch.float32, M * P * P), floor=G64.abs().sum(sum_dims))
    cols = bf and not nchw_out and odt == torch.bfloat16 and N <= 512 and tr_shape(M, Cin, N)
    assert spy.n["tante_colsum"] == 1
    assert spy.n["tante_im2col"] == (1 if cols or N > 512 else 0), spy.n
    ret = spy.returned[0]
    assert (ret[1] is None) == (route == "slot") and (ret[2] is None) == (route == "slot")
    if cols and route == "slot":
        assert spy.deferred == [True] and spy.n["tante_wgrad_ws"] == 0 and spy.flushes() == 1, (spy.deferred, spy.n)
    else:
        assert True not in spy.deferred and spy.n["tante_wgrad_ws"] == 1 and spy.flushes() == 0, (spy.deferred, spy.n)


# ---- colsum: what test_colsum_dense_rows lacks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outer,Cc,off", [(777, 24, False), (301, 2056, False), (1000, 256, True)], ids=["C24", "C2056", "C256 +2B"])
def test_colsum_scalar_forms_and_accumulation(dev, outer, Cc, off):
    """bf16 rows the 16-byte kernel does not take -- C = 24 (256 % 3 != 0), C = 2056 (> 2048), a pointer that is not 16-byte aligned --
    and `into=` adding onto a non-zero vector.  The sum cancels: measured against max(|sum|, 1e-2 sum |x|)."""
    _, A, _ = _lib_mods()
    g = torch.Generator().manual_seed(outer + Cc)
    x = randn((outer, Cc), g, torch.bfloat16)
    xd = misaligned(x, dev) if off else x.to(dev)
    ref = x.double().sum(0)
    floor = x.double().abs().sum(0)
    tag = f"colsum bf16 {outer}x{Cc}{' +2B' if off else ''}"
    close(A.colsum(xd, outer, Cc, 1), ref, tag, bar=F32_BAR, floor=floor)
    fill = randn((Cc,), g, scale=3.0)
    into = fill.to(dev)
    got = A.colsum(xd, outer, Cc, 1, into=into)
    assert got is into
    close(into.double().cpu() - fill.double(), ref, tag + " into", bar=F32_BAR, floor=floor)


# ---- the end-of-pass flush: one graph, every way of running it ---------------------------------------------------------------------------
FL_N, FL_M, FL_USES, FL_FOLDED = 128, 64, 2, (1, 4)
FL_ENTRIES = WGRAD_ENTRIES + ("tante_fold_bwd_multi", "tante_fold_bwd", "tante_fold_bwd_clear")
FL_KINDS = ("W", "b", "gamma", "beta")
_FL_DATA = {}


def _flush_graph_data():
    """CPU-seeded inputs of the flush graph and its float64 gradients, computed once: six 128 x 128 linears with biases, weights 1 and 4
    behind a LayerNorm fold (We = W diag(gamma), be = b + W beta), every weight used twice on 64 rows of its own; the loss is
    sum(y * G) over the twelve uses.  layout: (weight, kind, offset, shape) of every parameter in the flat buffers."""
    if _FL_DATA:
        return _FL_DATA
    N = FL_N
    g = torch.Generator().manual_seed(2024)
    layout, off, vals = [], 0, {}
    for i in range(6):
        for kind, shape in [("W", (N, N)), ("b", (N,))] + ([("gamma", (N,)), ("beta", (N,))] if i in FL_FOLDED else []):
            layout.append((i, kind, off, shape))
            vals[(i, kind)] = {"W": lambda: randn(shape, g, scale=1.0 / math.sqrt(N)).to(torch.bfloat16).float(),
                               "gamma": lambda: randn(shape, g, scale=0.25, shift=1.0)}.get(kind, lambda: randn(shape, g))()
            off += math.prod(shape)
    a = {(i, u): randn((FL_M, N), g, torch.bfloat16) for i in range(6) for u in range(FL_USES)}
    G = {k: randn((FL_M, N), g, torch.bfloat16) for k in a}
    fill = randn((off,), g, scale=SLOT_FILL)
    p64 = {k: v.double().requires_grad_() for k, v in vals.items()}
    loss = 0.0
    for (i, u), au in a.items():
        W, b = p64[(i, "W")], p64[(i, "b")]
        if i in FL_FOLDED:
            W, b = W * p64[(i, "gamma")][None, :], b + W @ p64[(i, "beta")]
        loss = loss + (ref_linear(au.double(), W, b) * G[(i, u)].double()).sum()
    loss.backward()
    ref = torch.cat([p64[(i, kind)].grad.flatten() for i, kind, _, _ in layout])
    _FL_DATA.update(layout=layout, n=off, vals=vals, a=a, G=G, fill=fill, ref=ref)
    return _FL_DATA


def _flush_graph_run(dev, spy, driver=None):
    """One backward of the graph from the same inputs -> (the flat gradient buffer, calls per library entry).  Parameters and their
    pre-filled .grad are views of flat buffers; a folded pair is wired as train_forward._folded does.  What run_backward does, with the
    state looked at BEFORE its closing reset (which would empty the lists and zero the accumulators whatever the flush left)."""
    L, A, _ = _lib_mods()
    d = _flush_graph_data()
    flat_p, flat_g = torch.empty(d["n"], device=dev), d["fill"].to(dev)
    P = {}
    for i, kind, off, shape in d["layout"]:
        n = math.prod(shape)
        flat_p[off: off + n] = d["vals"][(i, kind)].flatten().to(dev)
        p = P[(i, kind)] = torch.nn.Parameter(flat_p[off: off + n].view(shape))
        p.grad = flat_g[off: off + n].view(shape)
    terms = []
    for i in range(6):
        W, b = P[(i, "W")], P[(i, "b")]
        if i in FL_FOLDED:
            W, b, gw, gb = A.FoldFn.apply(W, b, P[(i, "gamma")], P[(i, "beta")])
            W._tante_grad, b._tante_grad = gw, gb
        for u in range(FL_USES):
            y = A.LinearFn.apply(d["a"][(i, u)].to(dev), W, b, None, L.BF16, torch.bfloat16)
            terms.append(functional(y, d["G"][(i, u)].to(dev)))
    loss = torch.stack(terms).sum()
    before = dict(spy.n)
    with A.backward_scope(driver=driver):
        loss.backward()
        torch.cuda.synchronize()
        assert A._PASS is None and not A._FOLD_DIRTY
        for i in FL_FOLDED:
            assert not bool(P[(i, "W")]._tante_fold_acc.any()), f"fold accumulator of weight {i} not left zeroed"
    return flat_g, {e: spy.n[e] - before[e] for e in spy.n}


def _flush_kind(flat, kind):
    d = _flush_graph_data()
    return torch.cat([flat[off: off + math.prod(shape)] for _, k, off, shape in d["layout"] if k == kind])


def _flush_close(flat_g, tag):
    """pre-fill + gradient in every slot, per kind of parameter, at the fp32 bar (exact bf16 cotangents, 2 x 64 terms; the fold's outputs
    are fp32 products and 128-term sums of the accumulated gradients)."""
    d = _flush_graph_data()
    got = flat_g.detach().double().cpu() - d["fill"].double()
    for kind in FL_KINDS:
        close(_flush_kind(got, kind), _flush_kind(d["ref"], kind), f"flush graph {tag} d{kind}", bar=F32_BAR)


def test_flush_paths_agree(dev, monkeypatch):
    """The same backward run by the engine callback alone, by a scope driver that calls flush_run(1), by one that calls flush_run(2), and
    with one weight per launch.  Recording order is the reverse of the forward's: groups (5, 4, 3, 2) and (1, 0), a fold behind each.
    * callback, flush_run(1), flush_run(2): 2 shared launches; the folds as one launch, one launch, two launches; on_segment(0), (1).
      The weight and bias slots are equal bit for bit (the shared launches sum their split-R partials in a fixed order, and the fold
      kernel's dW / db have one writer per element).  dgamma / dbeta are NOT compared bit for bit: the fold kernel adds the partial
      column sums of its 128 / 16 = 8 row slabs onto the slot with atomics, in the order the workgroups happen to arrive.
    * one weight per launch: 6 launches, one fold launch.
    Every run meets the fp32 bar against float64 in every slot and leaves no recorded state and zeroed accumulators behind."""
    _, A, _ = _lib_mods()
    spy = Spy(monkeypatch, entries=FL_ENTRIES)
    g1, n1 = _flush_graph_run(dev, spy)
    g2, n2 = _flush_graph_run(dev, spy, driver=lambda: A.flush_run(1))
    segs = []
    g3, n3 = _flush_graph_run(dev, spy, driver=lambda: A.flush_run(2, on_segment=segs.append))
    with _with_option("TANTE_WGRAD_JOBS_PER_LAUNCH", 1):
        g4, n4 = _flush_graph_run(dev, spy)
    for tag, gr in (("callback", g1), ("flush_run(1)", g2), ("flush_run(2)", g3), ("one per launch", g4)):
        _flush_close(gr, tag)
    for kind in FL_KINDS:
        same = [torch.equal(_flush_kind(g1, kind), _flush_kind(o, kind)) for o in (g2, g3)]
        print(f"flush graph d{kind}: callback == flush_run(1) {same[0]}, == flush_run(2) {same[1]}")
    for kind in ("W", "b"):
        exact(_flush_kind(g2, kind), _flush_kind(g1, kind), f"flush graph d{kind}: flush_run(1) against the callback")
        exact(_flush_kind(g3, kind), _flush_kind(g1, kind), f"flush graph d{kind}: flush_run(2) against the callback")
    assert segs == [0, 1]
    for n, groups, folds in ((n1, 2, 1), (n2, 2, 1), (n3, 2, 2), (n4, 6, 1)):
        assert n["tante_wgrad_multi_ws"] + n["tante_wgrad_jobs_ws"] == groups and n["tante_fold_bwd_multi"] == folds, n
        assert n["tante_wgrad_ws"] == n["tante_fold_bwd"] == n["tante_fold_bwd_clear"] == 0, n
    assert spy.deferred == [True] * (4 * 6 * FL_USES)


def test_flush_overflow_in_the_middle_of_a_pass(dev, monkeypatch):
    """TANTE_WGRAD_DEFER_MAX_GB at two and a half uses' operands (a use records 2 x 64 x 128 bf16 values = 32 KiB): every third of the
    twelve uses runs what is recorded so far, so most weights' two uses land in different launches.  The folds still wait for the end of
    the pass and run once; the slots hold pre-fill + gradient; nothing is left behind."""
    spy = Spy(monkeypatch, entries=FL_ENTRIES)
    with _with_option("TANTE_WGRAD_DEFER_MAX_GB", 2.5 * (2 * FL_M * FL_N * 2) / 2 ** 30):
        g5, n5 = _flush_graph_run(dev, spy)
    _flush_close(g5, "overflow")
    assert n5["tante_wgrad_multi_ws"] + n5["tante_wgrad_jobs_ws"] == 4 and n5["tante_fold_bwd_multi"] == 1, n5
    assert n5["tante_wgrad_ws"] == n5["tante_fold_bwd"] == n5["tante_fold_bwd_clear"] == 0, n5
    assert spy.deferred == [True] * (6 * FL_USES)
