"""GPU: the masked form of the flash attention kernels (csrc/attn_flash.hip under attn_mask / key_padding_mask, with dropout), its two C
entry points, MaskedFlashAttentionFn and the routes TANTE_ATTN_FLASH opens.  2 heads of dim 32 (C = 64), Bp = 2, bf16-rounded operands
for both dtypes (as tests/test_hip_attn_flash.py).  Metric everywhere: max |a - b| / max |b| per tensor."""
import math

import pytest
import torch

from conftest import max_rel, rel_err, record_parity
from test_hip_attn_flash import _keep, _lib, _qkv, _stream, _with_flash, dev      # noqa: F401  (dev: the module's GPU fixture)

pytestmark = pytest.mark.gpu

NH, C, BP = 2, 64, 2
NINF = float("-inf")
BARS = {torch.float32: (1e-5, 2e-4), torch.bfloat16: (1e-2, 1e-2)}      # (o, gradients): DESIGN.md 4.4
MODE = {torch.float32: "fp32", torch.bfloat16: "bf16"}
FORMS = ["bool", "float_per_head", "kpm", "causal_kpm", "both"]


def _masks(form, Lq, seed=0):
    """CPU, seeded -> (causal, attn_mask additive (1, L, L) | (BP NH, L, L) | None, key_padding_mask additive (BP, L) | None)."""
    g = torch.Generator().manual_seed(1000 + seed)
    eye = torch.eye(Lq, dtype=torch.bool)
    am = kp = None
    if form in ("bool", "both"):
        blocked = (torch.rand(Lq, Lq, generator=g) < 0.3) & ~eye      # ~30 % blocked, the diagonal open
        am = torch.zeros(1, Lq, Lq).masked_fill_(blocked[None], NINF)
    if form == "float_per_head":
        am = torch.rand(BP * NH, Lq, Lq, generator=g) * 4.0 - 2.0      # finite addends in [-2, 2]
        am.masked_fill_((torch.rand(BP * NH, Lq, Lq, generator=g) < 0.2) & ~eye[None], NINF)
    if form in ("kpm", "causal_kpm", "both"):
        kp = torch.zeros(BP, Lq)
        kp[1, Lq - 37:] = NINF      # the last 37 keys of sample 1 are padding
    return form == "causal_kpm", am, kp


def _additive(Lq, causal, am, kp):
    """The (BP, NH, L, L) additive mask a restatement adds to the scaled scores."""
    tot = torch.zeros(BP, NH, Lq, Lq, dtype=torch.float64)
    if causal:
        tot = tot.masked_fill(torch.ones(Lq, Lq, dtype=torch.bool).triu(1), NINF)
    if am is not None:
        tot = tot + (am.double().view(1, 1, Lq, Lq) if am.shape[0] == 1 else am.double().view(BP, NH, Lq, Lq))
    if kp is not None:
        tot = tot + kp.double()[:, None, None, :]
    return tot


def _ref64(qkv, Lq, add, keep, dO):
    """float64 softmax(q k^T / sqrt(d) + add) [* keep] v under autograd -> o (tokens, C), (dq | dk | dv) (tokens, 3 C)."""
    x = qkv.double().view(BP, Lq, 3, NH, 32).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    P = torch.softmax(x[0] @ x[1].transpose(-1, -2) / math.sqrt(32) + add, -1)
    if keep is not None:
        P = P * keep.double().view(BP, NH, Lq, Lq)
    o = (P @ x[2]).permute(0, 2, 1, 3).reshape(BP * Lq, C)
    (g,) = torch.autograd.grad(o, x, dO.double())
    return o.detach(), g.permute(1, 3, 0, 2, 4).reshape(BP * Lq, 3 * C)


def _flash(qkv, Lq, causal, am, kp, p, seed, dO, finite=True):
    """The masked flash forward and backward through attn_flash.forward / backward, with one NaN row behind each output checked."""
    L, K, FA = _lib()
    n = qkv.shape[0]
    seq = K.dense_seq(BP, Lq)
    o = torch.full((n + 1, C), float("nan"), dtype=qkv.dtype, device=qkv.device)
    g = torch.full((n + 1, 3 * C), float("nan"), dtype=qkv.dtype, device=qkv.device)
    stats = FA.new_stats(qkv, NH, seq)
    FA.forward(qkv, o, stats, C, NH, seq, causal, p, seed, am, kp)
    FA.backward(qkv, o, dO.to(qkv.dtype), stats, g, C, NH, seq, causal, p, seed, am, kp)
    assert torch.isnan(o[n].float()).all() and torch.isnan(g[n].float()).all(), "the row behind an output was written"
    if finite:
        assert torch.isfinite(o[:n].float()).all() and torch.isfinite(g[:n].float()).all()
    return o[:n].float(), g[:n].float()


def _errs(o, g, ro, rg):
    return [max_rel(o, ro)] + [max_rel(g[:, i * C:(i + 1) * C], rg[:, i * C:(i + 1) * C]) for i in range(3)]


def _hold(e, dt, what):
    for v, nm, bar in zip(e, ("o", "dq", "dk", "dv"), (BARS[dt][0],) + (BARS[dt][1],) * 3):
        record_parity(v, v, bar, MODE[dt], f"{what} {nm}")
    print(f"{what} {MODE[dt]}: o {e[0]:.2e} dq {e[1]:.2e} dk {e[2]:.2e} dv {e[3]:.2e}")
    assert e[0] <= BARS[dt][0] and max(e[1:]) <= BARS[dt][1], (what, MODE[dt], e)


# ---- 1: against float64 autograd with the materialised masks and keep-mask ------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Lq", [67, 200, 320])
def test_masked_flash_against_float64_autograd(dev, Lq, form, p):
    """o, dq, dk, dv of both dtypes against ONE float64 autograd restatement per case (masks and the restated keep-mask materialised).
    L = 200, 320: a ragged last query block, a ragged last key tile, more than one 128-query workgroup; L = 67: L % 4 != 0, the unaligned
    mask and keep-mask reads.  fp32: o 1e-5, gradients 2e-4; bf16: 1e-2 per tensor.
    Worst of the 30 cases on an MI355X: fp32 o 7.5e-7, dq 1.2e-6, dk 9.2e-7, dv 7.8e-7; bf16 o 4.3e-3, dq 5.1e-3, dk 5.2e-3, dv 4.0e-3."""
    causal, am, kp = _masks(form, Lq)
    add = _additive(Lq, causal, am, kp)
    assert bool((add > NINF).any(-1).all()), "a row with every key blocked"
    n = BP * Lq
    q32, dO = _qkv(n, Lq + 3, dev, 3 * C), _qkv(n, Lq + 4, dev, C)
    keep = _keep(BP * NH * Lq * Lq, p, 1234, dev) if p > 0 else None
    ro, rg = _ref64(q32, Lq, add.to(dev), keep, dO)
    amd, kpd = (None if t is None else t.to(dev) for t in (am, kp))
    for dt in (torch.float32, torch.bfloat16):
        o, g = _flash(q32.to(dt), Lq, causal, amd, kpd, p, 1234, dO)
        _hold(_errs(o, g, ro, rg), dt, f"masked flash vs float64 L={Lq} {form} p={p}")


# ---- 2: null masks are the unmasked kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_null_masks_equal_the_unmasked_kernels(dev, causal):
    """tante_attention_flash_masked(_bwd) with both masks NULL against tante_attention_flash(_bwd) on dense_seq(2, 320), p = 0.1, one
    seed: o, the row statistics (lse2 and delta) and dqkv bit for bit, fp32 and bf16."""
    L, K, FA = _lib()
    Lq, n = 320, BP * 320
    seq = K.dense_seq(BP, Lq)
    dO32 = _qkv(n, 12, dev, C)
    for dt in (torch.float32, torch.bfloat16):
        qkv, dO = _qkv(n, 11, dev, 3 * C).to(dt), dO32.to(dt)
        o0, g0, st0 = torch.empty(n, C, dtype=dt, device=dev), torch.empty(n, 3 * C, dtype=dt, device=dev), FA.new_stats(qkv, NH, seq)
        FA.forward(qkv, o0, st0, C, NH, seq, causal, 0.1, 77)
        FA.backward(qkv, o0, dO, st0, g0, C, NH, seq, causal, 0.1, 77)
        o1, g1, st1 = torch.zeros_like(o0), torch.zeros_like(g0), torch.zeros_like(st0)
        L.check(L.lib().tante_attention_flash_masked(qkv.data_ptr(), o1.data_ptr(), st1.data_ptr(), FA._DT[dt], C, NH, BP, Lq, int(causal), None, 0,
                                                     None, 0.1, 77, _stream()), "flash_masked")
        L.check(L.lib().tante_attention_flash_masked_bwd(qkv.data_ptr(), o1.data_ptr(), dO.data_ptr(), st1.data_ptr(), g1.data_ptr(), FA._DT[dt], C,
                                                         NH, BP, Lq, int(causal), None, 0, None, 0.1, 77, _stream()), "flash_masked_bwd")
        assert torch.equal(o0, o1) and torch.equal(st0, st1) and torch.equal(g0, g1), dt


# ---- 3: against the existing masked kernels ------------------------------------------------------------------------------------------
def _old(q32, Lq, causal, am, kp, dO):
    """tante_attention_masked and tante_attention_masked_bwd in fp32 under the same masks."""
    L, K, FA = _lib()
    n = q32.shape[0]
    o, g = torch.empty(n, C, device=q32.device), torch.empty(n, 3 * C, device=q32.device)
    K.attention_masked(q32, o, C, NH, BP, Lq, causal, am, kp)
    st = torch.empty(BP * NH * Lq * 3, device=q32.device)
    L.check(L.lib().tante_attention_masked_bwd(q32.data_ptr(), dO.data_ptr(), g.data_ptr(), L.F32, C, NH, BP, Lq, int(causal),
                                               am.data_ptr() if am is not None else None, 0 if am is None or am.shape[0] == 1 else Lq * Lq,
                                               kp.data_ptr() if kp is not None else None, st.data_ptr(), _stream()), "attention_masked_bwd")
    return o, g


@pytest.mark.parametrize("form", ["bool", "float_per_head", "both"])
def test_masked_flash_matches_the_masked_kernels(dev, form):
    """p = 0, L = 200: both dtypes against tante_attention_masked / _bwd in fp32 on the same bf16-rounded operands, at test 1's bars."""
    Lq, n = 200, BP * 200
    causal, am, kp = _masks(form, Lq, seed=3)
    am, kp = (None if t is None else t.to(dev) for t in (am, kp))
    q32, dO = _qkv(n, 21, dev, 3 * C), _qkv(n, 22, dev, C)
    ro, rg = _old(q32, Lq, causal, am, kp, dO)
    for dt in (torch.float32, torch.bfloat16):
        o, g = _flash(q32.to(dt), Lq, causal, am, kp, 0.0, 0, dO)
        _hold(_errs(o, g, ro, rg), dt, f"masked flash vs masked kernels L=200 {form}")


def test_fully_blocked_rows_follow_the_masked_kernels(dev):
    """The first 3 queries of sample 0 blocked everywhere through a per-head attn_mask (L = 200, p = 0).  tante_attention_masked's rule:
    such a row's o is NaN (torch's softmax of it), its dq is 0, and it adds nothing to dk and dv.  On those rows the flash o has the same
    NaN pattern and the flash dq equals the old kernel's; every other row of o and dq, and all of dk and dv, stay within test 1's bars."""
    Lq, n = 200, BP * 200
    g = torch.Generator().manual_seed(5)
    am = torch.zeros(BP * NH, Lq, Lq).masked_fill_((torch.rand(BP * NH, Lq, Lq, generator=g) < 0.3) & ~torch.eye(Lq, dtype=torch.bool)[None], NINF)
    am[:NH, :3, :] = NINF
    am = am.to(dev)
    q32, dO = _qkv(n, 31, dev, 3 * C), _qkv(n, 32, dev, C)
    ro, rg = _old(q32, Lq, False, am, None, dO)
    assert torch.isnan(ro[:3]).all() and torch.isfinite(ro[3:]).all() and torch.isfinite(rg).all() and not rg[:3, :C].any()
    for dt in (torch.float32, torch.bfloat16):
        o, gr = _flash(q32.to(dt), Lq, False, am, None, 0.0, 0, dO, finite=False)
        assert torch.equal(torch.isnan(o), torch.isnan(ro)), "NaN pattern of o"
        assert torch.isfinite(gr).all() and torch.equal(gr[:3, :C], rg[:3, :C]), "dq of the blocked rows"
        _hold(_errs(o[3:], gr, ro[3:], rg), dt, "masked flash vs masked kernels, 3 fully blocked rows")


# ---- 4: the block's routes under the option ------------------------------------------------------------------------------------------
class _Routes:
    """Counts what the two masked attention nodes launch in forward: MaskedFlashAttentionFn calls attn_flash.forward WITH a mask,
    MaskedAttentionFn calls kernels.attention_masked; attn_flash.backward with a mask is MaskedFlashAttentionFn's backward."""

    def __init__(self, monkeypatch):
        from tante_amd import attn_flash as FA, kernels as K
        self.flash = self.flash_bwd = self.lanes = 0
        f0, b0, m0 = FA.forward, FA.backward, K.attention_masked

        def masked(a, k, first):      # attn_mask / key_padding_mask are the two arguments from position `first`
            return any(t is not None for t in a[first:first + 2]) or k.get("attn_mask") is not None or k.get("key_padding_mask") is not None

        def fwd(*a, **k):
            self.flash += masked(a, k, 9)
            return f0(*a, **k)

        def bwd(*a, **k):
            self.flash_bwd += masked(a, k, 11)
            return b0(*a, **k)

        def lanes(*a, **k):
            self.lanes += 1
            return m0(*a, **k)
        monkeypatch.setattr(FA, "forward", fwd)
        monkeypatch.setattr(FA, "backward", bwd)
        monkeypatch.setattr(K, "attention_masked", lanes)


def _masked_block(dev, mode, train):
    import tante_amd
    torch.manual_seed(41)
    blk = tante_amd.TransformerBlock(C, NH, mlp_ratio=1.0, dropout=0.0).to(dev)
    blk.compute = mode
    return blk.train() if train else blk.eval()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_masked_block_trains_through_the_flash_option(dev, mode, monkeypatch):
    """TransformerBlock(64, 2, dropout = 0) with a boolean attn_mask over L = 200 under autograd: with TANTE_ATTN_FLASH on,
    MaskedFlashAttentionFn runs (forward and backward), with it off MaskedAttentionFn does; output, input gradient and parameter gradients
    of the two runs agree within G17's bars (fp32 1e-5 / 2e-4 max-relative; bf16 1e-2 / 4e-2 with relative L2 for gradients, vectors 1.25 x)."""
    Lq = 200
    blk = _masked_block(dev, mode, True)
    mask = _masks("bool", Lq, seed=7)[1][0] == NINF
    x = torch.randn(BP, Lq, C, generator=torch.Generator().manual_seed(42)).to(dev)
    w = torch.randn(BP, Lq, C, generator=torch.Generator().manual_seed(43)).to(dev)
    spy = _Routes(monkeypatch)

    def run():
        for q in blk.parameters():
            q.grad = None
        xx = x.clone().requires_grad_(True)
        y = blk(xx, attn_mask=mask.to(dev))
        (y.float() * w).sum().backward()
        return y.detach(), xx.grad, {k: q.grad.clone() for k, q in blk.named_parameters()}
    y0, dx0, g0 = run()
    assert (spy.lanes, spy.flash, spy.flash_bwd) == (1, 0, 0), (spy.lanes, spy.flash, spy.flash_bwd)
    y1, dx1, g1 = _with_flash(run)
    assert (spy.lanes, spy.flash, spy.flash_bwd) == (1, 1, 1), (spy.lanes, spy.flash, spy.flash_bwd)
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    gerr = max_rel if mode == "fp32" else rel_err
    ey, ex = max_rel(y1, y0), gerr(dx1, dx0)
    record_parity(ey, ey, ft, mode, "masked block, flash option vs default, y")
    record_parity(ex, ex, gt, mode, "masked block, flash option vs default, dx")
    print(f"masked block through the option {mode}: y {ey:.2e} dx {ex:.2e}")
    assert ey < ft and ex < gt, (ey, ex)
    for k in g0:
        e = gerr(g1[k], g0[k])
        record_parity(e, e, gt if (mode == "fp32" or g0[k].dim() > 1) else 1.25 * gt, mode, f"masked block, flash option vs default, {k}")
        assert e < (gt if (mode == "fp32" or g0[k].dim() > 1) else 1.25 * gt), (k, e)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_masked_block_inference_through_the_flash_option(dev, mode, monkeypatch):
    """eval(), no grad, L = 320, a boolean attn_mask and a key_padding_mask: _forward_masked takes the masked flash forward with the
    option and tante_attention_masked without it; the outputs agree within G17's forward bars."""
    Lq = 320
    blk = _masked_block(dev, mode, False)
    _, am, kp = _masks("both", Lq, seed=8)
    mask, pad = (am[0] == NINF).to(dev), (kp == NINF).to(dev)
    x = torch.randn(BP, Lq, C, generator=torch.Generator().manual_seed(44)).to(dev)
    spy = _Routes(monkeypatch)

    def run():
        with torch.no_grad():
            return blk(x, key_padding_mask=pad, attn_mask=mask)
    y0 = run()
    assert (spy.lanes, spy.flash) == (1, 0)
    y1 = _with_flash(run)
    assert (spy.lanes, spy.flash, spy.flash_bwd) == (1, 1, 0)
    e = max_rel(y1, y0)
    record_parity(e, e, 1e-5 if mode == "fp32" else 1e-2, mode, "masked block inference, flash option vs default")
    assert torch.isfinite(y1).all() and e < (1e-5 if mode == "fp32" else 1e-2), e


# ---- 5: the operator's dropout ---------------------------------------------------------------------------------------------------
def test_masked_operator_dropout_statistics(dev):
    """MaskedFlashAttentionFn, p = 0.25, L = 320, q = k = 0 (uniform probabilities) and v = 1 under a key_padding_mask: an output row is
    (1 / n_open) sum_j keep_j / (1 - p) over its n_open open keys, so its mean is 1 and its variance p / ((1 - p) n_open); rows are
    independent, so the mean over all (sample, head, query) rows has standard error sqrt(sum var) / N.  Within 4 of them of 1; one seed
    gives the same bits, another seed does not."""
    from tante_amd import autograd as A
    Lq, p = 320, 0.25
    _, _, kp = _masks("kpm", Lq)
    n_open = (kp > NINF).sum(-1)      # (BP,)
    qkv = torch.zeros(BP * Lq, 3 * C, device=dev)
    qkv[:, 2 * C:] = 1.0
    o1 = A.MaskedFlashAttentionFn.apply(qkv, C, NH, BP, Lq, False, None, kp.to(dev), p, 5)
    rows = o1.view(BP, Lq, NH, 32)
    assert torch.equal(rows, rows[..., :1].expand_as(rows)), "v = 1: every dim of a head carries the same row sum"
    per_row = rows[..., 0].double().cpu()      # (BP, L, NH)
    var = (p / (1.0 - p)) / n_open.double()      # per row of each sample
    se = math.sqrt(float((var * Lq * NH).sum())) / (BP * Lq * NH)
    mean = float(per_row.mean())
    print(f"masked operator dropout: mean {mean:.6f}, standard error {se:.2e}, |mean - 1| = {abs(mean - 1) / se:.2f} se")
    assert abs(mean - 1.0) <= 4.0 * se, (mean, se)
    assert per_row.std() > 0      # dropout did drop
    o2 = A.MaskedFlashAttentionFn.apply(qkv, C, NH, BP, Lq, False, None, kp.to(dev), p, 5)
    o3 = A.MaskedFlashAttentionFn.apply(qkv, C, NH, BP, Lq, False, None, kp.to(dev), p, 6)
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)
