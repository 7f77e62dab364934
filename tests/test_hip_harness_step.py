"""GPU parity of the LAST stage of a train step, each kernel alone, against float64.

tante_amd/csrc/train.hip behind tante_amd/optim.py, tante_amd/metrics.py, MseMeanFn and RtReduceFn: the loss, its gradient, the gradient
norm, both clips and the AdamW update.  Until now these ran only behind a whole model, at bars sized for the model's gradient error, and
after ONE step from zero moments -- where Adam's update is lr * sign(g) and the clip coefficient and grad_scale cancel out of it.

* FlatAdamW            -- six steps over bare parameters whose gradient norm crosses max_norm from step to step (so the coefficient shows
                          in m / sqrt(v)), entries small enough for eps to matter, exact zeros, a complex parameter; grad_scale, the lr=
                          override, max_norm = 0 behind a stale sum of squares, bias correction at step 100001, clip_grad_value_.
* tante_sumsq          -- the 16-byte pieces, the scalar tail, a misaligned start, the grid-stride form, inf and NaN.
* tante_clip_value     -- torch.clamp_'s rule element by element (NaN stays NaN, +-inf clamps).
* tante_metric_sums    -- all five sums per (b, t, c) on both kernels and every loop form, the prediction in every layout the host accepts,
                          on fields whose frame means differ by 1e3 (a pivot from the wrong frame moves the shifted sums far outside the bar).
* tante_mse_grad, MseMeanFn, RtReduceFn, Metric.forward -- against float64 autograd / the oracle.

Every reference is float64 on the CPU, built from the fp32 numbers the kernel reads.  The AdamW reference restarts at every step from the
fp32 state read back from the GPU, so each step is its own comparison.  The references are pinned to torch.optim.AdamW + clip_grad_norm_
and to the oracle's metrics by tests/test_host_cpu.py, which also shows that six single mutations of the update land outside these bars.

Bars: fp32 results 2e-5 relative L2 / 1e-4 max-norm; sums over more than 4096 terms 1e-4 / 5e-4; variance metrics of the large-mean
fields 1e-4 max-norm (test_vrmse_of_large_mean_field's); the parameter update max |p - p_ref| / max |update_ref| <= 1e-4, whose floor is
the fp32 spacing of p over lr (6e-8 / 1e-2 = 6e-6 per rounding); tante_sumsq 1e-6 relative.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err, max_rel, record_parity
from test_hip_train_ops import (close, dev,  # noqa: F401  (dev: the module-scoped device fixture)
                                F32_REL, F32_MAX, F32_SUM_REL, F32_SUM_MAX)

pytestmark = pytest.mark.gpu

F32_BAR, SUM_BAR = (F32_REL, F32_MAX), (F32_SUM_REL, F32_SUM_MAX)
VAR_BAR = (1e-4, 1e-4)        # variance metrics on the large-mean fields (tests/test_hip_round2.py::test_vrmse_of_large_mean_field)
UPDATE_BAR = 1e-4             # max |p - p_ref| / max |update_ref|
SUMSQ_BAR = 1e-6
f64 = torch.float64


# ---- 1. AdamW with both clips: inputs, the float64 reference, the fp32 restatement of the kernel ---------------------------------------
ADAM_SIZES = [1, 3, 5, 255, 257, 4099]
ADAM_COMPLEX = (3, 5)
ADAM_HYPER = dict(lr=1e-2, weight_decay=1e-1, betas=(0.9, 0.999), eps=1e-6, max_norm=1.0)
ADAM_NORMS = [10.0, 0.1, 3.0, 0.3, 20.0, 1.0]       # above and below max_norm in turn
ADAM_CLIP_VALUE = 0.05
ADAM_LOADED_STEP = 100000
# the lr= override of case c: every value within a factor 2 of the constructor's lr -- the update bar's floor is the spacing of p over lr
ADAM_LRS = [2e-2, 5e-3, 1.5e-2, 8e-3, 1e-2, 6e-3]
ADAM_CASES = {
    "a-grad_scale1": dict(),
    "b-grad_scale0.5": dict(grad_scale=0.5),
    "c-lr_per_step": dict(lrs=ADAM_LRS),
    "d-max_norm0-stale_sumsq": dict(max_norm=0.0, stale=True),
    "e-loaded_step100000": dict(loaded=True),
    "f-clip_grad_value": dict(clip_value=ADAM_CLIP_VALUE),
}


def adam_layout():
    """(offsets, sizes in floats, bucket length) -- tante_amd.optim.flat_layout restated: complex as (re, im), every view 16-byte aligned."""
    sizes = ADAM_SIZES + [2 * ADAM_COMPLEX[0] * ADAM_COMPLEX[1]]
    offs, n = [], 0
    for sz in sizes:
        offs.append(n)
        n += (sz + 3) // 4 * 4
    return offs, sizes, n


def adam_live_mask():
    offs, sizes, n = adam_layout()
    live = torch.zeros(n, dtype=torch.bool)
    for o, sz in zip(offs, sizes):
        live[o:o + sz] = True
    return live


def _to_bucket(values):
    """Values over the parameters' elements in order -> the padded fp32 bucket (padding 0)."""
    out = torch.zeros(adam_layout()[2], dtype=torch.float32)
    out[adam_live_mask()] = values.to(torch.float32)
    return out


def adam_weights(gen):
    n = int(adam_live_mask().sum())
    return _to_bucket(torch.rand(n, generator=gen, dtype=f64) * 2.0 - 1.0)


def adam_grad(gen, norm):
    """One step's gradient bucket: normal values, every 7th entry 1e-4 times smaller (eps matters there), every 11th (offset 3) exactly 0,
    scaled to the 2-norm `norm`."""
    n = int(adam_live_mask().sum())
    g = torch.randn(n, generator=gen, dtype=f64)
    g[::7] *= 1e-4
    g[3::11] = 0.0
    return _to_bucket(g * (norm / float(g.norm())))


def adam_moments(gen):
    """Non-zero moments of a long run: m / sqrt(v) of order one."""
    n = int(adam_live_mask().sum())
    m = 1e-2 * torch.randn(n, generator=gen, dtype=f64)
    v = 1e-4 * (0.5 + torch.rand(n, generator=gen, dtype=f64))
    return _to_bucket(m), _to_bucket(v)


def ref_adamw_step(p, m, v, g, step, lr, weight_decay, betas, eps, max_norm, grad_scale=1.0, clip_value=None, f32_hyper=False):
    """float64: [clip_grad_value_] -> gradients x grad_scale -> clip_grad_norm_(max_norm) -> torch.optim.AdamW, step counted from 1.
    f32_hyper: the hyper-parameters rounded to fp32 first, as the kernel receives them.  -> (p, m, v)"""
    b1, b2 = betas
    if f32_hyper:
        lr, weight_decay, b1, b2, eps, max_norm, grad_scale = (float(np.float32(h)) for h in (lr, weight_decay, b1, b2, eps, max_norm, grad_scale))
    p, m, v, g = (t.to(f64) for t in (p, m, v, g))
    if clip_value is not None:
        g = g.clamp(-clip_value, clip_value)
    g = g * grad_scale
    if max_norm > 0:
        g = g * min(max_norm / (float(g.norm()) + 1e-6), 1.0)
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


ADAM_MUTATIONS = ("no norm clip", "grad_scale ignored", "no weight decay", "coupled weight decay", "no bias correction", "no eps")


def kernel_adamw_step32(p, m, v, g, step, lr, weight_decay, betas, eps, max_norm, grad_scale=1.0, mutation=None):
    """adamw_kernel + tante_adamw_step restated in fp32 torch: hyper-parameters cast to fp32, operations in the kernel's order, the sum of
    squares in double.  mutation: one of ADAM_MUTATIONS, the single defects the bars must see.  -> (p, m, v) in fp32"""
    assert mutation is None or mutation in ADAM_MUTATIONS
    F = np.float32
    lr, wd, b1, b2, eps, max_norm, gs = (F(h) for h in (lr, weight_decay, betas[0], betas[1], eps, max_norm, grad_scale))
    one = F(1.0)
    bc1 = one - F(np.power(b1, F(step)))
    bc2s = F(np.sqrt(one - F(np.power(b2, F(step)))))
    if mutation == "no bias correction":
        bc1, bc2s = one, one
    if mutation == "no eps":
        eps = F(0.0)
    if mutation == "grad_scale ignored":
        gs = one
    coef = gs
    if max_norm > 0 and mutation != "no norm clip":
        total = F(math.sqrt(float((g.double() ** 2).sum()))) * gs
        coef = coef * min(max_norm / (total + F(1e-6)), one)
    t = lambda s: torch.tensor(float(s), dtype=torch.float32)      # noqa: E731  (an fp32 scalar operand)
    gi = g * t(coef)
    if mutation == "coupled weight decay":
        gi = gi + t(wd) * p
    pi = p if mutation in ("no weight decay", "coupled weight decay") else p * t(one - lr * wd)
    mi = t(b1) * m + t(one - b1) * gi
    vi = t(b2) * v + t(one - b2) * gi * gi
    denom = vi.sqrt() / t(bc2s) + t(eps)
    return pi - t(lr / bc1) * (mi / denom), mi, vi


def update_ratio(p_got, p_ref, p_before):
    """max |p - p_ref| / max |update_ref|; a non-finite result counts as infinitely far."""
    p_got, p_ref, p_before = p_got.double(), p_ref.double(), p_before.double()
    if not torch.isfinite(p_got).all():
        return float("inf")
    return float((p_got - p_ref).abs().max() / (p_ref - p_before).abs().max())


def adam_case_args(case, k):
    """Keyword arguments of ref_adamw_step / kernel_adamw_step32 at step index k of a case (without step and clip_value)."""
    h = dict(ADAM_HYPER)
    if "max_norm" in case:
        h["max_norm"] = case["max_norm"]
    if "lrs" in case:
        h["lr"] = case["lrs"][k]
    h["grad_scale"] = case.get("grad_scale", 1.0)
    return h


def _bucket_params(bucket, dev):
    """Bare nn.Parameters holding the bucket's values: the real ones and the complex (3, 5) one."""
    offs, sizes, _ = adam_layout()
    ps = [torch.nn.Parameter(bucket[o:o + sz].clone().to(dev)) for o, sz in zip(offs[:-1], sizes[:-1])]
    c = torch.view_as_complex(bucket[offs[-1]:offs[-1] + sizes[-1]].clone().view(*ADAM_COMPLEX, 2))
    return ps + [torch.nn.Parameter(c.to(dev))]


def _param_views(bucket):
    """The bucket cut into the parameters' shapes (CPU), the complex one as complex."""
    offs, sizes, _ = adam_layout()
    out = [bucket[o:o + sz] for o, sz in zip(offs[:-1], sizes[:-1])]
    return out + [torch.view_as_complex(bucket[offs[-1]:offs[-1] + sizes[-1]].view(*ADAM_COMPLEX, 2))]


@pytest.mark.parametrize("name", list(ADAM_CASES))
def test_adamw_six_steps_against_float64(dev, name):
    """FlatAdamW over bare parameters, six steps; after EVERY step the parameters, exp_avg and exp_avg_sq against the float64 reference
    restarted from the fp32 state the GPU held before the step.  The exact-hyper-parameter reference must meet the bars (update 1e-4 of
    the reference's largest update; moments 2e-5 / 1e-4); the distance to the reference with fp32-rounded hyper-parameters is recorded
    beside it (the kernel forms 1 - beta2 from the rounded beta2, 1.3e-5 on exp_avg_sq)."""
    import tante_amd
    from tante_amd.attn_backbone import _WEIGHT_EPOCH
    case = ADAM_CASES[name]
    gen = torch.Generator().manual_seed(101)
    live = adam_live_mask()
    w0 = adam_weights(gen)
    params = _bucket_params(w0, dev)
    opt = tante_amd.FlatAdamW(params, **dict(ADAM_HYPER, max_norm=case.get("max_norm", ADAM_HYPER["max_norm"])))
    assert opt.numel == live.numel() and torch.equal(opt.flat_p.cpu(), w0)
    if case.get("loaded"):
        m0, v0 = adam_moments(gen)
        sd = {"param_groups": [dict(lr=ADAM_HYPER["lr"], betas=ADAM_HYPER["betas"], eps=ADAM_HYPER["eps"], weight_decay=ADAM_HYPER["weight_decay"])],
              "state": {i: {"step": torch.tensor(float(ADAM_LOADED_STEP)), "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
                        for i, (a, b) in enumerate(zip(_param_views(m0), _param_views(v0)))}}
        opt.load_state_dict(sd)
        assert opt.step_count == ADAM_LOADED_STEP and torch.equal(opt.exp_avg.cpu(), m0) and torch.equal(opt.exp_avg_sq.cpu(), v0)
    epoch0 = _WEIGHT_EPOCH[0]
    worst = 0.0
    for k, norm in enumerate(ADAM_NORMS):
        g = adam_grad(gen, norm)
        for p, gv in zip(params, _param_views(g)):
            p.grad.copy_(gv.to(dev))
        assert torch.equal(opt.flat_g.cpu(), g)
        if case.get("stale"):      # leaves this gradient's sum of squares in _sumsq; max_norm = 0 must not read it
            gn = float(opt.grad_norm())
            e = abs(gn - float(g.double().norm())) / float(g.double().norm())
            record_parity(e, e, SUMSQ_BAR, "fp32", f"adamw {name} step {k + 1}: grad_norm()")
            assert e <= SUMSQ_BAR, (k, gn)
        p0, m0, v0 = opt.flat_p.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()
        kw = adam_case_args(case, k)
        if "clip_value" in case:
            opt.clip_grad_value_(case["clip_value"])
        step_kw = {}
        if "grad_scale" in case:
            step_kw["grad_scale"] = case["grad_scale"]
        if "lrs" in case:
            step_kw["lr"] = case["lrs"][k]
        opt.step(**step_kw)
        step = opt.step_count
        assert step == k + 1 + (ADAM_LOADED_STEP if case.get("loaded") else 0)
        p1, m1, v1 = opt.flat_p.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()
        tag = f"adamw {name} step {k + 1} (norm {norm})"
        pr, mr, vr = ref_adamw_step(p0, m0, v0, g, step, clip_value=case.get("clip_value"), f32_hyper=True, **kw)
        record_parity(update_ratio(p1, pr, p0), update_ratio(p1, pr, p0), UPDATE_BAR, "fp32", tag + ": update vs the fp32-hyper-parameter reference")
        record_parity(rel_err(m1, mr), max_rel(m1, mr), F32_REL, "fp32", tag + ": exp_avg vs the fp32-hyper-parameter reference")
        record_parity(rel_err(v1, vr), max_rel(v1, vr), F32_REL, "fp32", tag + ": exp_avg_sq vs the fp32-hyper-parameter reference")
        pr, mr, vr = ref_adamw_step(p0, m0, v0, g, step, clip_value=case.get("clip_value"), **kw)
        r = update_ratio(p1, pr, p0)
        worst = max(worst, r)
        record_parity(r, r, UPDATE_BAR, "fp32", tag + ": update")
        print(f"{tag}: update ratio {r:.3e}  exp_avg {rel_err(m1, mr):.3e}  exp_avg_sq {rel_err(v1, vr):.3e}")
        assert r <= UPDATE_BAR, f"{tag}: update off by {r:.3e} of the largest update (bar {UPDATE_BAR:.1e})"
        close(m1, mr, tag + ": exp_avg", bar=F32_BAR)
        close(v1, vr, tag + ": exp_avg_sq", bar=F32_BAR)
        for p, pv in zip(params, _param_views(p1)):      # the parameters ARE the bucket
            assert torch.equal(p.detach().cpu(), pv)
    for what, t in (("flat_p", opt.flat_p), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
        assert not t.cpu()[~live].any(), f"{what}: padding touched"
    assert _WEIGHT_EPOCH[0] >= epoch0 + len(ADAM_NORMS)


def test_scheduler_drives_flat_adamw(dev):
    """LinearWarmupCosineAnnealingLR on a real FlatAdamW: the lr the NEXT step() uses follows the schedule (param_groups is rebuilt on
    every access, so writing the group's entry alone would leave the optimiser at its first lr)."""
    import tante_amd
    from tante_amd import harness as H
    p = torch.nn.Parameter(torch.zeros(8, device=dev))      # (starts at 0: the weight's fp32 spacing stays far below lr x the bar)
    opt = tante_amd.FlatAdamW([p], lr=1e-2, weight_decay=0.0, eps=1e-8, max_norm=0.0)
    sch = H.LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=6, warmup_start_lr=1e-3, eta_min=1e-3)
    want = 0.0
    for e in range(4):
        lr = tante_amd.warmup_cosine_lr(e, 1e-2, 2, 6, 1e-3, 1e-3)
        assert opt.lr == lr == sch.get_last_lr()[0] == opt.param_groups[0]["lr"], (e, opt.lr, lr)
        p.grad.fill_(1.0)      # a constant gradient: every step moves the weight by exactly lr (m / sqrt(v) = 1 after bias correction)
        opt.step()
        want -= lr
        e_ = abs(float(p[0]) - want) / lr
        record_parity(e_, e_, UPDATE_BAR, "fp32", f"scheduler epoch {e}: weight moved by the scheduled lr")
        assert e_ <= UPDATE_BAR, (e, float(p[0]), want)
        sch.step()


# ---- 2. tante_sumsq --------------------------------------------------------------------------------------------------------------------
def _sumsq(t, out):
    from tante_amd import _lib as L
    L.check(L.lib().tante_sumsq(t.data_ptr(), t.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "tante_sumsq")
    return float(out.cpu()[0])


SUMSQ_CASES = [(1, 0), (3, 0), (4, 0), (5, 0), (4099, 0), (4099, 1), (1048581, 0)]


@pytest.mark.parametrize("n,off", SUMSQ_CASES, ids=[f"n{n}" + ("-misaligned" if off else "") for n, off in SUMSQ_CASES])
def test_sumsq_against_float64(dev, n, off):
    """The library entry on n floats of magnitude 1e-18 .. 1e15: the 16-byte pieces and the scalar tail (n % 4 != 0), a start one float
    into the storage (all scalar), more than 256 x 4096 elements (the 256-workgroup cap: grid-stride trips).  1e-6 relative against the
    float64 sum (expected ~1e-7: four fp32 squares are summed in fp32 before the double accumulation); a second call returns the same
    number (the output is zeroed per call; the 256 double atomics arrive in any order, 256 x 2^-53 < 1e-12); one inf -> inf; one NaN -> NaN."""
    gen = torch.Generator().manual_seed(202 + n + off)
    v = torch.sign(torch.rand(n, generator=gen, dtype=f64) - 0.5) * 10.0 ** (torch.rand(n, generator=gen, dtype=f64) * 33.0 - 18.0)
    v = v.to(torch.float32)
    buf = torch.zeros(n + off, dtype=torch.float32, device=dev)
    t = buf[off:]
    t.copy_(v)
    assert (t.data_ptr() % 16 != 0) == bool(off)
    out = torch.full((1,), 7.0, dtype=f64, device=dev)      # (a non-zero start: the entry zeroes it)
    want = float((v.double() ** 2).sum())
    got = _sumsq(t, out)
    e = abs(got - want) / want
    record_parity(e, e, SUMSQ_BAR, "fp32", f"sumsq n={n} offset {off}")
    print(f"sumsq n={n} offset {off}: {e:.3e}")
    assert e <= SUMSQ_BAR, (got, want)
    again = _sumsq(t, out)
    assert abs(again - got) <= 1e-12 * got, (again, got)
    t[n // 2] = float("inf")
    assert _sumsq(t, out) == float("inf")
    t[n // 2] = float("nan")
    assert math.isnan(_sumsq(t, out))


# ---- 3. clip_grad_value_ ---------------------------------------------------------------------------------------------------------------
def test_clip_grad_value_elementwise(dev):
    """n = 1000 (not a multiple of 256), c = 0.5: inside +-c bitwise unchanged, outside exactly +-c, +-inf -> +-c, NaN stays NaN."""
    import tante_amd
    n, c = 1000, 0.5
    gen = torch.Generator().manual_seed(303)
    g = torch.randn(n, generator=gen)
    g[[5, 256, 999]] = float("inf")
    g[[6, 511, 998]] = float("-inf")
    g[[0, 7, 255, 997]] = float("nan")
    g[[8, 9]] = torch.tensor([c, -c])
    p = torch.nn.Parameter(torch.zeros(n, device=dev))
    opt = tante_amd.FlatAdamW([p])
    assert opt.numel == n
    p.grad.copy_(g.to(dev))
    opt.clip_grad_value_(c)
    got = opt.flat_g.cpu()
    nan = torch.isnan(g)
    inside = ~nan & (g.abs() <= c)
    assert int(inside.sum()) > 100 and int((~nan & (g.abs() > c)).sum()) > 100
    assert torch.equal(got[inside].view(torch.int32), g[inside].view(torch.int32)), "an entry inside +-c changed"
    assert torch.equal(got[~nan & (g > c)], torch.full((int((~nan & (g > c)).sum()),), c)), "an entry above c is not exactly c"
    assert torch.equal(got[~nan & (g < -c)], torch.full((int((~nan & (g < -c)).sum()),), -c)), "an entry below -c is not exactly -c"
    assert torch.isnan(got[nan]).all() and not torch.isnan(got[~nan]).any(), "NaN must stay NaN, and only NaN"
    record_parity(0.0, 0.0, 1e-30, "fp32", "clip_grad_value_ n=1000 c=0.5 (exact)")


# ---- 4. tante_metric_sums: every kernel form -------------------------------------------------------------------------------------------
MB, MT = 2, 3
# the dispatch rule of tante_metric_sums, restated (tests/test_host_cpu.py::test_metric_sums_dispatch_constants_match_the_source reads the
# same numbers out of train.hip, so a change of the rule there shows here as wrong ids)
PX_CHANNELS, PX_MIN_HW, PX_CHUNK = (1, 2, 4), 4096, 4096
GENERIC_ELEMS_PER_BLOCK = 256 * 64


def sums_form(C, HW):
    """Which kernel and loop forms tante_metric_sums(C, HW) reaches, as the test id."""
    if C in PX_CHANNELS and HW >= PX_MIN_HW:
        nch = -(-HW // PX_CHUNK)

        def trips(n):      # per thread: trips of the four-pixel loop, then of the scalar loop; the maxima over the 256 threads
            u = t = 0
            for tid in range(256):
                s, a, b = tid, 0, 0
                while s + 768 < n:
                    s, a = s + 1024, a + 1
                while s < n:
                    s, b = s + 256, b + 1
                u, t = max(u, a), max(t, b)
            return f"unroll{u}+tail{t}"
        last = HW - (nch - 1) * PX_CHUNK
        return f"px{C}-hw{HW}-{nch}chunks-" + (f"full[{trips(PX_CHUNK)}]-" if nch > 1 else "") + f"last{last}[{trips(last)}]"
    chunks = max(1, -(-HW * C // GENERIC_ELEMS_PER_BLOCK))
    chunk = -(-HW // chunks)
    nblk = -(-HW // chunk)
    return f"generic-{'fixedc' if 256 % C == 0 else 'varc'}-C{C}-hw{HW}-{nblk}chunks-last{HW - (nblk - 1) * chunk}"


# (C, spatial shape, layout of the prediction)
_M = [
    (8, (37, 29), "copy"), (16, (3000,), "slice"), (16, (3001,), "cl"), (3, (33, 20), "cf"), (7, (33, 20), "cl"), (7, (33, 20), "slice"),
    (4, (4095,), "cf"), (8, (4, 6, 5), "cf"),
    (1, (4096,), "cl"), (2, (4096,), "cf"), (4, (4096,), "slice"),
    (1, (4097,), "cf"), (2, (4097,), "slice"), (4, (4097,), "cl"),
    (1, (64, 80), "copy"), (2, (64, 80), "cl"), (4, (64, 80), "copy"),
    (1, (16, 331), "slice"), (2, (16, 331), "copy"), (4, (16, 331), "cf"),      # 4096 + 1200: one four-pixel trip, then one scalar one
    (1, (9001,), "slice"), (2, (9001,), "cl"), (4, (9001,), "cf"),
    (4, (16, 16, 17), "copy"),                                               # three spatial axes on the per-pixel kernel
]
METRIC_CASES = [pytest.param(C, sp, lay, id=f"{sums_form(C, math.prod(sp))}-{'x'.join(map(str, sp))}-{lay}") for C, sp, lay in _M]


def metric_fields(C, sp, gen):
    """(x, y) fp32 (B, T, *sp, C): unit-variance frames whose means differ by 1e3 between the (b, t) pairs and by 7e3 between channels, and
    a prediction 0.1 away."""
    mean = 1e3 * (1.0 + torch.arange(MB * MT, dtype=f64).view(MB, MT, 1)) + 7e3 * torch.arange(C, dtype=f64)
    mean = mean.view(MB, MT, *([1] * len(sp)), C)
    y = (mean + torch.randn(MB, MT, *sp, C, generator=gen, dtype=f64)).to(torch.float32)
    x = (y.double() + 0.1 * torch.randn(MB, MT, *sp, C, generator=gen, dtype=f64)).to(torch.float32)
    return x, y


def as_layout(x, layout, dev):
    """x (B, T, *sp, C) on the device, the same values in one of the prediction layouts the host accepts."""
    nsp = x.dim() - 3
    if layout == "cl":
        v = x.to(dev)
    elif layout == "cf":      # the channels-last view of a channels-first buffer
        v = x.movedim(-1, 2).contiguous().to(dev).movedim(2, -1)
        assert not v.is_contiguous() or x.shape[-1] == 1
    elif layout == "slice":   # a time slice of a longer buffer: the frame stride is not the batch stride / T
        buf = torch.full((x.shape[0], 7) + tuple(x.shape[2:]), float("nan"), device=dev)
        buf[:, 2:5] = x.to(dev)
        v = buf[:, 2:5]
        assert v.stride(0) != v.shape[1] * v.stride(1)
    elif layout == "copy":    # every other row of a taller buffer: the spatial axes do not collapse to one stride
        assert nsp >= 2
        buf = torch.full(tuple(x.shape[:2]) + (2 * x.shape[2],) + tuple(x.shape[3:]), float("nan"), device=dev)
        buf[:, :, ::2] = x.to(dev)
        v = buf[:, :, ::2]
        from tante_amd.metrics import _spatial_strides
        assert _spatial_strides(v) is None
    else:
        raise ValueError(layout)
    assert v.shape == x.shape
    return v


def ref_metric_sums(x, y):
    """float64 (B, T, C, 5): sum (x-y)^2, sum y^2, sum y, sum (y-p)^2, sum (y-p) over the spatial axes, p = y[b, t, first pixel, c]."""
    B, T, C = x.shape[0], x.shape[1], x.shape[-1]
    x, y = x.double().reshape(B, T, -1, C), y.double().reshape(B, T, -1, C)
    z = y - y[:, :, :1, :]
    return torch.stack([((x - y) ** 2).sum(2), (y * y).sum(2), y.sum(2), (z * z).sum(2), z.sum(2)], dim=-1)


def ref_metrics(x, y, eps=1e-7):
    """float64, trainer/metrics.py from the maths: every metric class over channels-last (B, T, *spatial, C); NMSE and NNMSE in both
    norm modes."""
    x, y = x.double(), y.double()
    B, C = x.shape[0], x.shape[-1]
    sp = tuple(range(2, x.dim() - 1))
    mse = ((x - y) ** 2).mean(dim=sp)
    nmse = mse / ((y * y).mean(dim=sp) + eps)
    vmse = mse / (y.var(dim=sp, unbiased=True) + eps)
    d, yy = (x - y).reshape(B, -1, C), y.reshape(B, -1, C)
    spc = sp + (x.dim() - 1,)
    return {"MSE": mse, "RMSE": mse.sqrt(), "NMSE": nmse, "NRMSE": nmse.sqrt(), "VMSE": vmse, "VRMSE": vmse.sqrt(),
            "L2RE": (d * d).sum(1).sqrt() / ((yy * yy).sum(1).sqrt() + eps),
            "NNMSE": mse.mean(-1) / ((y * y).mean(dim=spc) + eps),
            "NNMSE_std": mse.mean(-1) / (y.var(dim=spc, unbiased=True) + eps)}


VARIANCE_METRICS = ("VMSE", "VRMSE", "NNMSE_std")
NMSE_EPS = 2.5e6      # of the size of the smallest frames' mean square (1e6), so that it changes the result


@pytest.mark.parametrize("C,sp,layout", METRIC_CASES)
def test_metric_sums_every_form(dev, C, sp, layout):
    """The raw (B, T, C, 5) sums, each of the five on its own, and every metric class built on them, against float64."""
    import tante_amd
    from tante_amd import metrics as Mx
    gen = torch.Generator().manual_seed(404 + C + math.prod(sp))
    x, y = metric_fields(C, sp, gen)
    xd, yd = as_layout(x, layout, dev), y.to(dev)
    tag = f"metric_sums {sums_form(C, math.prod(sp))} {layout}"
    got, ref = Mx.metric_sums(xd, yd).cpu(), ref_metric_sums(x, y)
    for i, what in enumerate(("sum (x-y)^2", "sum y^2", "sum y", "sum (y-p)^2", "sum (y-p)")):
        close(got[..., i], ref[..., i], f"{tag}: {what}", bar=SUM_BAR)
    want = ref_metrics(x, y)
    for name in ("MSE", "RMSE", "NMSE", "NRMSE", "VMSE", "VRMSE", "L2RE", "NNMSE"):
        close(getattr(tante_amd, name).eval(xd, yd), want[name], f"{tag}: {name}", bar=VAR_BAR if name in VARIANCE_METRICS else SUM_BAR)
    close(tante_amd.NNMSE.eval(xd, yd, norm_mode="std"), want["NNMSE_std"], f"{tag}: NNMSE std", bar=VAR_BAR)
    close(tante_amd.NMSE.eval(xd, yd, eps=NMSE_EPS), ref_metrics(x, y, NMSE_EPS)["NMSE"], f"{tag}: NMSE eps={NMSE_EPS:g}", bar=SUM_BAR)


# ---- 5. loss and its gradient ----------------------------------------------------------------------------------------------------------
def ref_mse_mean(x, y):
    return ((x - y) ** 2).mean()


GRAD_CASES = [(8, (37, 29), "copy"), (3, (33, 20), "cf"), (4, (4097,), "slice"), (7, (33, 20), "cl"), (2, (9001,), "cf")]


@pytest.mark.parametrize("C,sp,layout", GRAD_CASES, ids=[f"C{C}-{'x'.join(map(str, sp))}-{lay}" for C, sp, lay in GRAD_CASES])
def test_mse_mean_grad_against_autograd(dev, C, sp, layout):
    """metrics.mse_mean_grad on strided and sliced predictions against float64 autograd of mean((x - y)^2); every element count here
    leaves a ragged last workgroup (not a multiple of 256)."""
    from tante_amd import metrics as Mx
    gen = torch.Generator().manual_seed(505 + C)
    x, y = metric_fields(C, sp, gen)
    assert x.numel() % 256 != 0
    x64 = x.double().requires_grad_()
    ref_mse_mean(x64, y.double()).backward()
    g = Mx.mse_mean_grad(as_layout(x, layout, dev), y.to(dev))
    assert g.is_contiguous() and g.shape == x.shape
    close(g, x64.grad, f"mse_mean_grad C{C} {sp} {layout}", bar=F32_BAR)


def test_mse_mean_fn_scaled_backward_into_a_strided_leaf(dev):
    """MseMeanFn on the channels-last VIEW of a channels-first leaf, then (loss * 1024).backward() -- the GradScaler case, an upstream
    gradient other than 1: the loss (a sum of 169 944 terms: the long-sum bar) and the leaf's .grad against float64."""
    from tante_amd.autograd import MseMeanFn
    gen = torch.Generator().manual_seed(606)
    x, y = metric_fields(4, (73, 97), gen)
    leaf = x.movedim(-1, 2).contiguous().to(dev).requires_grad_()      # (B, T, C, H, W)
    view = leaf.movedim(2, -1)
    assert not view.is_contiguous()
    loss = MseMeanFn.apply(view, y.to(dev))
    l64 = x.movedim(-1, 2).contiguous().double().requires_grad_()
    ref = ref_mse_mean(l64.movedim(2, -1), y.double())
    close(loss.detach().reshape(1), ref.detach().reshape(1), "MseMeanFn loss", bar=SUM_BAR)
    (loss * 1024.0).backward()
    (ref * 1024.0).backward()
    assert leaf.grad.shape == leaf.shape
    close(leaf.grad, l64.grad, "MseMeanFn x 1024: leaf gradient through the channels-last view", bar=F32_BAR)


@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (5, 130)])
def test_rt_reduce_forward_and_backward(dev, B, L):
    """rt[b] = mean_l clamp(t[b, l], 0, out_T - 1) + ep; the clamp is straight-through, so dt = drt / L on EVERY entry, clamped ones
    included.  Entries below 0, inside, and above out_T - 1."""
    from tante_amd.autograd import RtReduceFn
    out_T, ep = 4.0, 0.25
    gen = torch.Generator().manual_seed(707 + L)
    t = (1.5 + 3.0 * torch.randn(B * L, 1, generator=gen, dtype=f64)).to(torch.float32)
    t.view(-1)[0] = 5.0
    if B * L > 2:
        t.view(-1)[1], t.view(-1)[2] = -2.0, 1.0
        assert (t < 0).any() and (t > out_T - 1).any() and ((t > 0) & (t < out_T - 1)).any()
    G = torch.randn(B, generator=gen, dtype=f64).to(torch.float32)
    td = t.to(dev).requires_grad_()
    rt = RtReduceFn.apply(td, B, L, out_T, ep)
    assert rt.shape == (B,)
    close(rt, t.double().view(B, L).clamp(0.0, out_T - 1.0).mean(1) + ep, f"rt_reduce ({B}, {L}) forward", bar=F32_BAR)
    rt.backward(G.to(dev))
    want = (G.double() / L).view(B, 1).expand(B, L).reshape(B * L, 1)
    close(td.grad, want, f"rt_reduce ({B}, {L}) backward", bar=F32_BAR)


@pytest.mark.parametrize("band,rt_mean", [("below", 1.0), ("inside", 2.5), ("above", 5.0)])
def test_metric_forward_with_rt(dev, band, rt_mean):
    """Metric.forward(x, y, rt, eps, n) = MSE.mean() + the step-size band regulariser, in the three bands of eval_rt (eps = 0.5: below 1.5,
    inside, above 4), against the oracle's mse_with_rt in float64."""
    import tante_amd
    from oracle import tante_oracle as O
    gen = torch.Generator().manual_seed(808)
    x, y = metric_fields(3, (33, 20), gen)
    rt = (rt_mean + 0.1 * torch.randn(6, generator=gen)).float()
    want = O.mse_with_rt(x.double(), y.double(), rt.double(), 0.5, 2)
    assert (float(O.eval_rt(rt.double(), 0.5, 2)) > 0) == (band != "inside")
    got = tante_amd.MSE()(as_layout(x, "cf", dev), y.to(dev), rt.to(dev), 0.5, 2)
    close(got.reshape(1), torch.as_tensor(want).reshape(1), f"Metric.forward with rt {band}", bar=F32_BAR)
