"""GPU: the flash attention kernels (csrc/attn_flash.hip) and the train-path calls they open (sequences past 128 / 256 tokens with
dropout, strided sequences past 128).  Metric everywhere: max |a - b| / max |b| per tensor."""
import ctypes as Ct
import math

import pytest
import torch

from conftest import load_golden, max_rel, rel_err, split_prefix

pytestmark = pytest.mark.gpu

NH, C = 5, 160      # 5 heads of dim 32: a ragged head group for the 4-heads-per-workgroup kernels it is compared with


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from tante_amd import _lib as L, kernels as K, attn_flash as FA
    return L, K, FA


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _seq(spec):
    L, K, FA = _lib()
    if spec[0] == "dense":
        return K.dense_seq(spec[1], spec[2]), spec[1] * spec[2]
    letter, B, T, H, W = spec
    return K.make_seq(letter, B, T, H, W), B * T * H * W


def _tokens(seq, dev):
    s = torch.arange(seq.nseq, device=dev)[:, None]
    l = torch.arange(seq.L, device=dev)[None, :]
    return (s // seq.n_s0) * seq.S1 + (s % seq.n_s0) * seq.S0 + (l // seq.n_l0) * seq.P1 + (l % seq.n_l0) * seq.P0


def _keep(n, p, seed, dev):
    """The keep mask of flat indices 0 .. n - 1, times 1 / (1 - p), from tante_dropout_add(ones, zeros)."""
    L, K, FA = _lib()
    ones, zeros, out = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
    L.check(L.lib().tante_dropout_add(ones.data_ptr(), L.F32, zeros.data_ptr(), float(p), seed, n, out.data_ptr(), _stream()), "dropout_add")
    torch.cuda.synchronize()      # ones / zeros stay alive until the kernel has read them
    return out


def _ref64(qkv, seq, nh, causal, keep=None, dO=None):
    """float64 softmax(q k^T / sqrt(d)) [* keep] v per (sequence, head) on the gathered tokens -> o, (dq | dk | dv) in token order."""
    dev = qkv.device
    tok = _tokens(seq, dev)
    Cc = qkv.shape[1] // 3
    d = Cc // nh
    x = qkv.double()[tok].view(seq.nseq, seq.L, 3, nh, d).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(dO is not None)
    s = x[0] @ x[1].transpose(-1, -2) / math.sqrt(d)
    if causal:
        s = s.masked_fill(torch.ones(seq.L, seq.L, dtype=torch.bool, device=dev).triu(1), float("-inf"))
    P = torch.softmax(s, -1)
    del s
    if keep is not None:
        P = P * keep.view(seq.nseq, nh, seq.L, seq.L)
    o = (P @ x[2]).permute(0, 2, 1, 3).reshape(seq.nseq, seq.L, Cc)
    o_tok = torch.empty(qkv.shape[0], Cc, dtype=torch.float64, device=dev)
    o_tok[tok] = o.detach()
    if dO is None:
        return o_tok, None
    (g,) = torch.autograd.grad(o, x, dO.double()[tok])
    g_tok = torch.empty(qkv.shape[0], 3 * Cc, dtype=torch.float64, device=dev)
    g_tok[tok] = g.permute(1, 3, 0, 2, 4).reshape(seq.nseq, seq.L, 3 * Cc)
    return o_tok, g_tok


def _flash(qkv, seq, nh, causal, p=0.0, seed=0, dO=None):
    """-> o (with one NaN row behind it checked), dqkv or None"""
    L, K, FA = _lib()
    n, Cc = qkv.shape[0], qkv.shape[1] // 3
    o = torch.full((n + 1, Cc), float("nan"), dtype=qkv.dtype, device=qkv.device)
    stats = FA.new_stats(qkv, nh, seq) if dO is not None else None
    FA.forward(qkv, o, stats, Cc, nh, seq, causal, p, seed)
    assert torch.isnan(o[n].float()).all(), "the row behind the output was written"
    assert torch.isfinite(o[:n].float()).all()
    if dO is None:
        return o[:n], None
    dqkv = torch.full((n + 1, 3 * Cc), float("nan"), dtype=qkv.dtype, device=qkv.device)
    FA.backward(qkv, o, dO.to(qkv.dtype), stats, dqkv, Cc, nh, seq, causal, p, seed)
    assert torch.isnan(dqkv[n].float()).all() and torch.isfinite(dqkv[:n].float()).all()
    return o[:n], dqkv[:n]


def _qkv(n, seed, dev, cols=3 * C):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, cols, generator=g).to(torch.bfloat16).float().to(dev)      # bf16-rounded operands for both dtypes


FWD_SHAPES = [("L", 1, 2, 3, 43), ("L", 1, 2, 16, 20), ("L", 1, 2, 32, 32), ("A", 1, 4, 32, 32), ("X", 1, 4, 3, 40), ("X", 1, 4, 2, 64),
              ("Y", 1, 4, 40, 3), ("Y", 1, 4, 64, 2), ("T", 1, 257, 1, 3), ("T", 1, 1000, 2, 1), ("dense", 2, 257), ("dense", 2, 1000)]


# ---- A: forward against the existing fp32 kernel (bf16) and float64 (fp32) -----------------------------------------------------------
FWD_CASES = [(sp, c) for sp in FWD_SHAPES for c in (False, True) if not (sp[0] == "A" and c)]      # 'A' (4096 tokens) is pinned non-causal


@pytest.mark.parametrize("spec,causal", FWD_CASES, ids=lambda v: "-".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_flash_forward_matches_fp32_kernel_and_float64(dev, spec, causal):
    """bf16: <= 1e-2 against tante_attention in fp32 on the same bf16-rounded operands (the scheme and bar of
    test_attention_fwd_mfma_matches_fp32_kernel); fp32: <= 1e-5 against float64."""
    L, K, FA = _lib()
    seq, n = _seq(spec)
    q32 = _qkv(n, n + seq.L, dev)
    yard = torch.empty(n, C, device=dev)
    K.attention(q32, yard, C, NH, seq, causal)
    o16, _ = _flash(q32.to(torch.bfloat16), seq, NH, causal)
    e16 = max_rel(o16.float(), yard)
    o32, _ = _flash(q32, seq, NH, causal)
    ref, _ = _ref64(q32, seq, NH, causal)
    e32 = max_rel(o32, ref)
    print(f"flash fwd {spec} causal={causal}: bf16 {e16:.2e} fp32 {e32:.2e}")
    assert e16 <= 1e-2, e16
    assert e32 <= 1e-5, e32


# ---- B: the dropout mask is the existing kernels' --------------------------------------------------------------------------------
def test_dropout_add_of_ones_is_the_attention_keep_mask(dev):
    """The equivalence the float64 tests below rely on, checked where the existing kernel runs (L = 64): tante_dropout_add(ones, zeros)
    over nseq n_head L L elements is tante_attention_dropout's keep mask times 1 / (1 - p)."""
    L, K, FA = _lib()
    seq, n = _seq(("dense", 3, 64))
    q32 = _qkv(n, 7, dev)
    o = torch.empty(n, C, device=dev)
    L.check(L.lib().tante_attention_dropout(q32.data_ptr(), o.data_ptr(), L.F32, C, NH, Ct.byref(seq), 0, 0.25, 99, _stream()))
    keep = _keep(3 * NH * 64 * 64, 0.25, 99, dev)
    assert set(keep.unique().tolist()) == {0.0, float(torch.tensor(1.0 / 0.75, dtype=torch.float32))}
    ref, _ = _ref64(q32, seq, NH, False, keep)
    assert max_rel(o, ref) <= 1e-5


@pytest.mark.parametrize("Lq", [129, 200, 256])
def test_flash_forward_draws_the_existing_dropout_mask(dev, Lq):
    """p = 0.25, seed 99 against tante_attention_dropout in fp32 on the same seed; bars as the forward test."""
    L, K, FA = _lib()
    seq, n = _seq(("dense", 3, Lq))
    q32 = _qkv(n, Lq, dev)
    yard = torch.empty(n, C, device=dev)
    L.check(L.lib().tante_attention_dropout(q32.data_ptr(), yard.data_ptr(), L.F32, C, NH, Ct.byref(seq), 1, 0.25, 99, _stream()))
    e16 = max_rel(_flash(q32.to(torch.bfloat16), seq, NH, True, 0.25, 99)[0].float(), yard)
    e32 = max_rel(_flash(q32, seq, NH, True, 0.25, 99)[0], yard)
    print(f"flash fwd dropout L={Lq}: bf16 {e16:.2e} fp32 {e32:.2e}")
    assert e16 <= 1e-2 and e32 <= 1e-5, (e16, e32)


@pytest.mark.parametrize("Lq", [48, 100, 128])
def test_flash_backward_draws_the_existing_dropout_mask(dev, Lq):
    """Where tante_attention_bwd runs (L <= 128): the flash backward against it in fp32 on the same seed.  bf16 <= 1e-2, fp32 <= 2e-4 (the
    gradient bars of the float64 test below)."""
    L, K, FA = _lib()
    seq, n = _seq(("dense", 3, Lq))
    q32 = _qkv(n, Lq, dev)
    dO = _qkv(n, Lq + 1, dev, C)
    yard = torch.empty(n, 3 * C, device=dev)
    L.check(L.lib().tante_attention_bwd(q32.data_ptr(), dO.data_ptr(), yard.data_ptr(), L.F32, C, NH, Ct.byref(seq), 1, 0.25, 99, _stream()))
    for dt, bar in ((torch.bfloat16, 1e-2), (torch.float32, 2e-4)):
        _, g = _flash(q32.to(dt), seq, NH, True, 0.25, 99, dO)
        for i, nm in enumerate(("dq", "dk", "dv")):
            e = max_rel(g[:, i * C:(i + 1) * C].float(), yard[:, i * C:(i + 1) * C])
            print(f"flash bwd dropout L={Lq} {dt} {nm}: {e:.2e}")
            assert e <= bar, (dt, nm, e)


# ---- C: forward and backward against float64 autograd with the mask materialised -----------------------------------------------------
def _against_float64(dev, spec, causal, p, nh=NH):
    seq, n = _seq(spec)
    Cc = nh * 32
    q32 = _qkv(n, n + seq.L + 3, dev, 3 * Cc)
    dO = _qkv(n, n + seq.L + 4, dev, Cc)
    keep = _keep(seq.nseq * nh * seq.L * seq.L, p, 1234, dev) if p > 0 else None
    ref_o, ref_g = _ref64(q32, seq, nh, causal, keep, dO)
    del keep
    out = {}
    for dt in (torch.bfloat16, torch.float32):
        o, g = _flash(q32.to(dt), seq, nh, causal, p, 1234, dO)
        out[dt] = (o.float(), g.float())
    errs = {}
    for dt in out:
        e = [max_rel(out[dt][0], ref_o)] + [max_rel(out[dt][1][:, i * Cc:(i + 1) * Cc], ref_g[:, i * Cc:(i + 1) * Cc]) for i in range(3)]
        errs[dt] = e
        print(f"flash vs float64 {spec} causal={causal} p={p} {dt}: o {e[0]:.2e} dq {e[1]:.2e} dk {e[2]:.2e} dv {e[3]:.2e}")
    return out, errs


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("spec,causal", [(("L", 1, 2, 16, 20), False), (("L", 1, 2, 16, 20), True), (("L", 1, 2, 32, 32), False),
                                         (("L", 1, 2, 32, 32), True), (("A", 1, 4, 32, 32), False), (("X", 1, 4, 2, 64), False)],
                         ids=["L320", "L320c", "L1024", "L1024c", "A4096", "X256"])
def test_flash_against_float64_autograd(dev, spec, causal, p):
    """o and (dq, dk, dv) against float64 autograd on the bf16-rounded operands with the materialised keep mask: bf16 <= 1e-2 per tensor;
    fp32 <= 1e-5 for o and <= 2e-4 for the gradients (the G17 gradient bar)."""
    _, errs = _against_float64(dev, spec, causal, p)
    assert max(errs[torch.bfloat16]) <= 1e-2, errs[torch.bfloat16]
    assert errs[torch.float32][0] <= 1e-5 and max(errs[torch.float32][1:]) <= 2e-4, errs[torch.float32]


def test_flash_causal_4096(dev):
    """Causal attention over 4096 tokens, p = 0.1: outside the 1e-2 set on purpose (rounding P and dS to bf16 alone reaches 1.4e-2 on dk in
    a CPU emulation of the design).  Finite, the fp32 form within its bars against float64, and bf16 within 3e-2 of the fp32 form.
    Measured on an MI355X (2 heads): bf16 against the fp32 form o 3.0e-3, dq 3.9e-3, dk 2.4e-3, dv 2.9e-3; bf16 against float64 o 3.0e-3,
    dq 3.9e-3, dk 2.5e-3, dv 2.9e-3; fp32 against float64 o 2.4e-7, dq 3.7e-7, dk 2.7e-6, dv 2.6e-6."""
    out, errs = _against_float64(dev, ("A", 1, 4, 32, 32), True, 0.1, nh=2)
    assert errs[torch.float32][0] <= 1e-5 and max(errs[torch.float32][1:]) <= 2e-4, errs[torch.float32]
    Cc = 64
    a, b = out[torch.bfloat16], out[torch.float32]
    e = [max_rel(a[0], b[0])] + [max_rel(a[1][:, i * Cc:(i + 1) * Cc], b[1][:, i * Cc:(i + 1) * Cc]) for i in range(3)]
    print("flash causal 4096 bf16 vs fp32:", e)
    assert max(e) <= 3e-2, e


# ---- D: module level ---------------------------------------------------------------------------------------------------------------
def _block(dev, mode):
    import tante_amd
    torch.manual_seed(5)
    blk = tante_amd.TransformerBlock(256, 8, mlp_ratio=1.0, dropout=0.1).to(dev).train()
    blk.compute = mode
    return blk


def _run_block(blk, x, seed):
    from tante_amd import autograd as A
    torch.manual_seed(seed)
    A._SEED[0] = 0
    for q in blk.parameters():
        q.grad = None
    xx = x.clone().requires_grad_(True)
    y = blk(xx)
    (y.float() * torch.linspace(-1, 1, y.numel(), device=y.device).view_as(y)).sum().backward()
    return y.detach(), xx.grad, [q.grad.clone() for q in blk.parameters()]


class _Spy:
    """Counts the calls of attn_flash.forward / backward and keeps what they wrote (o, dqkv), so that a test can prove the flash
    kernels were reached and compare their results between runs."""

    def __init__(self, monkeypatch):
        from tante_amd import attn_flash as FA
        self.fwd, self.bwd, self.o, self.dqkv = 0, 0, [], []
        f0, b0 = FA.forward, FA.backward

        def fwd(qkv, o, *a, **k):
            self.fwd += 1
            r = f0(qkv, o, *a, **k)
            self.o.append(o.detach().clone())
            return r

        def bwd(qkv, o, do, stats, dqkv, *a, **k):
            self.bwd += 1
            r = b0(qkv, o, do, stats, dqkv, *a, **k)
            self.dqkv.append(dqkv.detach().clone())
            return r
        monkeypatch.setattr(FA, "forward", fwd)
        monkeypatch.setattr(FA, "backward", bwd)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Lq", [200, 320])
def test_block_trains_with_dropout_past_128_tokens(dev, mode, Lq, monkeypatch):
    """TransformerBlock(dropout = 0.1).train() under autograd at L = 200 (the backward used to raise: "longer than 128") and L = 320 (the
    forward used to raise: "up to 256 tokens"): runs, finite, reproducible from the seed, and the seed matters."""
    spy = _Spy(monkeypatch)
    blk = _block(dev, mode)
    x = torch.randn(2, Lq, 256, generator=torch.Generator().manual_seed(Lq)).to(dev)
    y1, dx1, g1 = _run_block(blk, x, 11)
    assert len(g1) == 12
    assert torch.isfinite(y1).all() and torch.isfinite(dx1).all() and all(torch.isfinite(g).all() for g in g1)
    y2, dx2, g2 = _run_block(blk, x, 11)
    # Bit for bit: the block's output, its input gradient, and everything the new path itself produced inside the block -- the flash
    # forward's o (the saved one at L = 320, the recomputed one at L = 200) and the attention node's dqkv -- so a mask or a sum that
    # differed between the runs anywhere on the new path fails here.
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    assert spy.fwd == 2 and spy.bwd == 2, (spy.fwd, spy.bwd)
    assert torch.equal(spy.o[0], spy.o[1]) and torch.equal(spy.dqkv[0], spy.dqkv[1])
    # The 12 parameter gradients are NOT bit-stable in this project at 640 rows, with or without the flash kernels: the weight- and
    # bias-gradient kernels split their row sums over workgroups and join them with atomic adds in arrival order (the same block with
    # dropout = 0, which launches no flash kernel, moved by up to 9.6e-6 between two runs, mlp.2.bias).  With dqkv pinned bit for bit
    # above, what remains is a re-ordered fp32 sum of identical terms; it is held to 2e-4, the project's fp32 gradient bar (a
    # re-ordered sum may move by what the sum is accurate to), not to a figure read off these kernels.
    for (k, q), a, b in zip(blk.named_parameters(), g1, g2):
        assert max_rel(a, b) <= 2e-4, (k, max_rel(a, b))
    y3, _, _ = _run_block(blk, x, 12)
    assert not torch.equal(y1, y3)
    assert not torch.equal(spy.dqkv[0], spy.dqkv[2])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_flash_backward_is_deterministic(dev, dt):
    """dq, dk, dv are fixed-order sums (no atomics): two runs give the same bits."""
    seq, n = _seq(("X", 2, 4, 3, 80))
    q = _qkv(n, 1, dev).to(dt)
    dO = _qkv(n, 2, dev, C)
    o1, g1 = _flash(q, seq, NH, True, 0.1, 5, dO)
    o2, g2 = _flash(q, seq, NH, True, 0.1, 5, dO)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    o3, _ = _flash(q, seq, NH, True, 0.1, 6)
    assert not torch.equal(o1, o3)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Lq", [200, 320])
def test_block_with_dropout_matches_float64_restatement(dev, mode, Lq, monkeypatch):
    """With next_seed pinned, the block's output and input gradient against a float64 restatement that uses the three materialised masks
    (attention: the (nseq, n_head, L, L) index; both residual dropouts: row * 256 + column).  bf16: 1e-2; fp32: 1e-5 / 2e-4, the
    project's fp32 forward / gradient bars."""
    import torch.nn.functional as F
    from tante_amd import autograd as A
    blk = _block(dev, mode)
    seeds = iter([101, 202, 303])
    monkeypatch.setattr(A, "next_seed", lambda: next(seeds))
    x = torch.randn(2, Lq, 256, generator=torch.Generator().manual_seed(Lq + 1)).to(dev)
    w = torch.randn(2, Lq, 256, generator=torch.Generator().manual_seed(Lq + 2)).to(dev)
    xx = x.clone().requires_grad_(True)
    y = blk(xx)
    (y.float() * w).sum().backward()
    n = 2 * Lq
    ka = _keep(2 * 8 * Lq * Lq, 0.1, 101, dev).view(2, 8, Lq, Lq).double()
    ko = _keep(n * 256, 0.1, 202, dev).view(2, Lq, 256).double()
    km = _keep(n * 256, 0.1, 303, dev).view(2, Lq, 256).double()
    P = {k: v.detach().double() for k, v in blk.named_parameters()}
    xr = x.double().requires_grad_(True)
    h = F.layer_norm(xr, (256,), P["ln1.weight"], P["ln1.bias"], blk.ln1.eps)
    qkv = (h @ P["attn.in_proj_weight"].t() + P["attn.in_proj_bias"]).view(2, Lq, 3, 8, 32).permute(2, 0, 3, 1, 4)
    pr = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(32), -1) * ka
    o = (pr @ qkv[2]).permute(0, 2, 1, 3).reshape(2, Lq, 256)
    x1 = xr + (o @ P["attn.out_proj.weight"].t() + P["attn.out_proj.bias"]) * ko
    h2 = F.layer_norm(x1, (256,), P["ln2.weight"], P["ln2.bias"], blk.ln2.eps)
    m = F.gelu(h2 @ P["mlp.0.weight"].t() + P["mlp.0.bias"], approximate="tanh") @ P["mlp.2.weight"].t() + P["mlp.2.bias"]
    yr = x1 + m * km
    (yr * w.double()).sum().backward()
    ey, ex = max_rel(y.detach(), yr.detach()), max_rel(xx.grad, xr.grad)
    print(f"block L={Lq} {mode}: y {ey:.2e} dx {ex:.2e}")
    if mode == "bf16":
        assert ey <= 1e-2 and ex <= 1e-2, (ey, ex)
    else:
        assert ey <= 1e-5 and ex <= 2e-4, (ey, ex)


def test_small_tante_trains_with_an_L_letter_and_dropout(dev, monkeypatch):
    """attn_axes with 'L' over a 16 x 16 patch grid (256 tokens) and dropout = 0.1: two optimiser steps run, the loss is finite and moves.
    In eval() with TANTE_ATTN_FLASH at its default 0 the rollout must give the bits it gave before the flash kernels existed.  A test cannot
    hold the older build's output, so this is checked by PROXY: the route is the only thing that could change those bits, and the rollout
    is run with both flash entries replaced by a function that raises -- it launches none of the new kernels."""
    import tante_amd
    from tante_amd import attn_flash as FA
    from tante_amd.rollout import rollout_model
    assert FA.ATTN_FLASH == 0
    torch.manual_seed(3)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(128, 128))
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    m = tante_amd.TANTE(dset_metadata=md, in_T=4, taylor_order=1, attn_axes="TL", n_head=2, embed_dim=64, patch_scale=8, dropout=0.1).to(dev)
    g = torch.Generator().manual_seed(4)
    batch = {"input": torch.randn(2, 4, 128, 128, 2, generator=g).to(dev), "output": torch.randn(2, 2, 128, 128, 2, generator=g).to(dev)}
    m.train()
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-3)
    losses = [float(tante_amd.train_step(m, opt, batch, fmt, 2)) for _ in range(2)]
    assert all(math.isfinite(v) for v in losses) and losses[0] != losses[1], losses
    m.eval()

    def boom(*a, **k):
        raise AssertionError("a flash kernel was launched on the default inference route")
    monkeypatch.setattr(FA, "forward", boom)
    monkeypatch.setattr(FA, "backward", boom)
    with torch.no_grad():
        y, _ = rollout_model(m, batch, fmt, 2)
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_backbone_letter_X_past_128_tokens_trains(dev, mode):
    """Attn_Backbone with letter 'X' at T W = 256, p = 0, under autograd (the strided backward used to raise "longer than 128"): output,
    input and parameter gradients against float64 autograd through the oracle's backbone on the same weights, at
    test_g15_channel_letter_train's bars."""
    import tante_amd
    from oracle import tante_oracle as O
    T, H, W, Cc, nh = 4, 2, 64, 64, 2
    torch.manual_seed(9)
    bb = tante_amd.Attn_Backbone((T, H, W, Cc), "X", n_head=nh, mlp_ratio=1.0, dropout=0.0).to(dev).train()
    bb.compute = mode
    x = torch.randn(2, T, H, W, Cc, generator=torch.Generator().manual_seed(10))
    w = torch.randn(2, T, H, W, Cc, generator=torch.Generator().manual_seed(11))
    xx = x.to(dev).requires_grad_(True)
    y = bb(xx)
    (y.float() * w.to(dev)).sum().backward()
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in bb.state_dict().items()}
    xr = x.double().requires_grad_(True)
    yr = O.attn_backbone(w64, xr, "X", nh)
    (yr * w.double()).sum().backward()
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    ey, ex = max_rel(y.detach().cpu(), yr.detach()), max_rel(xx.grad.cpu(), xr.grad)
    print(f"backbone X {mode}: y {ey:.2e} dx {ex:.2e}")
    assert ey < ft and ex < gt, (ey, ex)
    ours, refs = [], []
    for k, q in bb.named_parameters():
        ref = w64[k].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, k
            continue
        ours.append(q.grad.cpu().reshape(-1))
        refs.append(ref.reshape(-1))
        e = (max_rel if mode == "fp32" else rel_err)(q.grad.cpu(), ref)
        print(f"backbone X {mode} {k}: {e:.2e}")
        assert e < (gt if (mode == "fp32" or ref.dim() > 1) else 1.25 * gt), (k, e)
    e = rel_err(torch.cat(ours), torch.cat(refs))
    print(f"backbone X {mode} all parameters: {e:.2e}")
    assert e < gt, ("all parameters", e)


def test_unsupported_head_dim_is_refused_by_name(dev):
    """Head dim 12 past 256 tokens with dropout: tante_attention_flash refuses with its message (nothing is launched), and the process
    goes on computing."""
    from tante_amd import autograd as A, kernels as K
    seq = K.dense_seq(2, 300)
    qkv = torch.randn(600, 3 * 48, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"tante_attention_flash: head dim unsupported \(supported: 32\)"):
        A.AttentionFn.apply(qkv, seq, 48, 4, False, 0.1)
    assert float((torch.ones(8, device=dev) * 2).sum()) == 16.0


# ---- E: TANTE_ATTN_FLASH = 1 parity ----------------------------------------------------------------------------------------------
def _with_flash(fn):
    import tante_amd
    tante_amd.set_option("TANTE_ATTN_FLASH", 1)
    try:
        return fn()
    finally:
        tante_amd.set_option("TANTE_ATTN_FLASH", 0)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["g4_backbone_L", "g4_backbone_A"])
def test_g4_backbone_through_the_flash_option(dev, name, mode):
    """test_g4_backbone's 'L' and 'A' fixtures with the option on: the same bars as the default route (test_hip_parity.close).  These
    fixtures are 24 and 72 tokens of head dim 8, which the option does not divert: they show that it leaves such calls alone.  The calls
    it does divert are in test_backbone_inference_through_the_flash_option."""
    import tante_amd
    from test_hip_parity import close
    g = load_golden(name)
    axes = name.split("_")[-1]
    T, H, W, Cc, E, nh = (int(v) for v in g["meta"])
    bb = tante_amd.Attn_Backbone((T, H, W, Cc), axes, expanded_channel=E, n_head=nh, mlp_ratio=1.0, dropout=0.0).to(dev).eval()
    bb.load_state_dict(split_prefix(g, "w."))
    bb.compute = mode

    def run():
        with torch.no_grad():
            return bb(g["x"].to(dev))
    close(_with_flash(run), g["y"], mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_g17_C256_backward_through_the_flash_option(dev, mode):
    """G17's channel letter over 256 channels (dense, p = 0, L = 256) with the option on, at
    test_g17_channel_letter_over_256_channels_trains' bars.  The fixture's channel block has head dim 4, which the flash kernels do not
    support, so the option leaves it on tante_attention_masked_bwd: this shows the option refuses cleanly.  The dense p = 0 backward the
    option does divert is in test_dense_backward_through_the_flash_option."""
    import tante_amd
    g = load_golden("g17_backbone_grad_C256")
    T, H, W, Cc, E, nh = (int(v) for v in g["meta"])
    bb = tante_amd.Attn_Backbone((T, H, W, Cc), "C", expanded_channel=E, n_head=nh, mlp_ratio=1.0, dropout=0.0).to(dev).train()
    bb.load_state_dict(split_prefix(g, "w."))
    bb.compute = mode
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    x = g["x"].to(dev).requires_grad_(True)

    def run():
        y = bb(x)
        (y.float() * g["w"].to(dev)).sum().backward()
        return y
    y = _with_flash(run)
    assert max_rel(y.detach().float().cpu(), g["y"]) < ft
    worst = (max_rel if mode == "fp32" else rel_err)(x.grad.cpu(), g["dx"])
    assert worst < gt, ("dx", worst)
    ours, refs = [], []
    for k, q in bb.named_parameters():
        ref = g["g." + k]
        if float(ref.abs().max()) == 0.0:
            continue
        ours.append(q.grad.cpu().reshape(-1))
        refs.append(ref.reshape(-1))
        err = max_rel(q.grad.cpu(), ref) if mode == "fp32" else rel_err(q.grad.cpu(), ref)
        assert err < (gt if (mode == "fp32" or ref.dim() > 1) else 1.25 * gt), (k, err)
    assert rel_err(torch.cat(ours), torch.cat(refs)) < gt


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("axes", ["L", "A"])
def test_backbone_inference_through_the_flash_option(dev, axes, mode, monkeypatch):
    """Attn_Backbone in eval() with head dim 32 and sequences past 256 tokens ('L': 320, 'A': 640) with the option on: K.attention runs
    the flash forward (asserted by a call counter) and the output meets test_g4_backbone's bars (test_hip_parity.close) against the
    oracle's backbone in float64.  Without the option the same call does not reach it."""
    import tante_amd
    from oracle import tante_oracle as O
    from test_hip_parity import close
    T, H, W, Cc, nh = 2, 16, 20, 64, 2
    torch.manual_seed(21)
    bb = tante_amd.Attn_Backbone((T, H, W, Cc), axes, n_head=nh, mlp_ratio=1.0, dropout=0.0).to(dev).eval()
    bb.compute = mode
    x = torch.randn(2, T, H, W, Cc, generator=torch.Generator().manual_seed(22))
    ref = O.attn_backbone({k: v.detach().cpu().double() for k, v in bb.state_dict().items()}, x.double(), axes, nh)
    spy = _Spy(monkeypatch)

    def run():
        with torch.no_grad():
            return bb(x.to(dev))
    y0 = run()
    assert spy.fwd == 0
    y = _with_flash(run)
    assert spy.fwd == 1 and spy.bwd == 0, (spy.fwd, spy.bwd)
    close(y, ref.float(), mode)
    close(y0, ref.float(), mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Lq", [200, 320])
def test_dense_backward_through_the_flash_option(dev, mode, Lq, monkeypatch):
    """A TransformerBlock with head dim 32 and no dropout over dense sequences past 128 tokens, under autograd with the option on: the
    backward is the flash one instead of tante_attention_masked_bwd (asserted by a call counter; at L = 320 the forward is the flash one
    as well), and the output, the input gradient and every parameter gradient meet G17's bars (fp32 1e-5 / 2e-4 max-relative, bf16 1e-2 /
    4e-2 with relative L2 for the gradients, vectors 1.25 x) against float64 autograd."""
    import torch.nn.functional as F
    import tante_amd
    E, nh = 64, 2
    torch.manual_seed(31)
    blk = tante_amd.TransformerBlock(E, nh, mlp_ratio=1.0, dropout=0.0).to(dev).train()
    blk.compute = mode
    x = torch.randn(2, Lq, E, generator=torch.Generator().manual_seed(Lq + 5)).to(dev)
    w = torch.randn(2, Lq, E, generator=torch.Generator().manual_seed(Lq + 6)).to(dev)
    spy = _Spy(monkeypatch)
    xx = x.clone().requires_grad_(True)

    def run():
        y = blk(xx)
        (y.float() * w).sum().backward()
        return y
    y = _with_flash(run)
    # L = 200: the forward stays on tante_attention, the backward recomputes the statistics (one flash forward) and runs the flash backward;
    # L = 320: the forward is the flash one too, and the backward recomputes as well (the p = 0 forward saves no statistics)
    assert spy.bwd == 1 and spy.fwd == (1 if Lq <= 256 else 2), (spy.fwd, spy.bwd)
    P = {k: v.detach().double().requires_grad_(True) for k, v in blk.named_parameters()}
    xr = x.double().requires_grad_(True)
    h = F.layer_norm(xr, (E,), P["ln1.weight"], P["ln1.bias"], blk.ln1.eps)
    qkv = (h @ P["attn.in_proj_weight"].t() + P["attn.in_proj_bias"]).view(2, Lq, 3, nh, E // nh).permute(2, 0, 3, 1, 4)
    pr = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(E // nh), -1)
    x1 = xr + (pr @ qkv[2]).permute(0, 2, 1, 3).reshape(2, Lq, E) @ P["attn.out_proj.weight"].t() + P["attn.out_proj.bias"]
    h2 = F.layer_norm(x1, (E,), P["ln2.weight"], P["ln2.bias"], blk.ln2.eps)
    yr = x1 + F.gelu(h2 @ P["mlp.0.weight"].t() + P["mlp.0.bias"], approximate="tanh") @ P["mlp.2.weight"].t() + P["mlp.2.bias"]
    (yr * w.double()).sum().backward()
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    gerr = max_rel if mode == "fp32" else rel_err
    ey, ex = max_rel(y.detach(), yr.detach()), gerr(xx.grad, xr.grad)
    print(f"dense backward through the option L={Lq} {mode}: y {ey:.2e} dx {ex:.2e}")
    assert ey < ft and ex < gt, (ey, ex)
    for k, q in blk.named_parameters():
        e = gerr(q.grad, P[k].grad)
        print(f"dense backward through the option L={Lq} {mode} {k}: {e:.2e}")
        assert e < (gt if (mode == "fp32" or q.dim() > 1) else 1.25 * gt), (k, e)
