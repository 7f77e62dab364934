"""GPU parity, round 5.

* autograd.FilmPosFramesFn -- the frame-encoding gradient accumulators are keyed to the backward pass, not to the tensors: a loss on some
  of the rollout's calls, and a second pass over a retained graph (trainer/trainer.py:144-159's sliding window, tante.py:136-141).
* csrc/block_bwd_fs.hip -- the WHOLE backward of a TransformerBlock in one launch (attn_backbone.py:59-83 backwards) against the three
  launches it replaces, against a float64 autograd of the same block, and inside the production-shape train step (fixture g14).

Bars: fp32 compute 1e-5 / gradients 2e-4, bf16 compute 1e-2 / gradients 4e-2, relative to the reference's fp32 CPU result.
"""
import ctypes as Ct

import numpy as np
import pytest
import torch

from conftest import rel_err, max_rel, record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------
# FilmPosFramesFn: whichever windows take part in a backward pass, the frame's encoder receives their sum
# ---------------------------------------------------------------------------------------------------
def _g14_grads(dev, monkeypatch, frame_film, n_loss_calls, passes=1):
    """Gradients of the g14 model (C = 256, fp32 compute, per-operator nodes) for a loss on the first `n_loss_calls` predicted frames."""
    import tante_amd
    from tante_amd import autograd as A
    from tante_amd import train_forward as TF
    from conftest import g14_setup, G14_FIELDS, G14_RES
    monkeypatch.setattr(TF, "FRAME_FILM", frame_film)
    m, batch, _, names = g14_setup()
    m = m.to(dev).train().set_compute("fp32")
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-4)
    opt.zero_grad()
    md = tante_amd.TanteMetadata(n_fields=G14_FIELDS, spatial_resolution=G14_RES)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    b = {k: v.to(dev) for k, v in batch.items()}
    y_pred, y_ref = tante_amd.rollout_model(m, b, fmt, 4)
    loss = A.MseMeanFn.apply(y_pred[:, :n_loss_calls].contiguous(), y_ref[:, :n_loss_calls].contiguous())
    with A.backward_scope():
        for i in range(passes):
            loss.backward(retain_graph=i + 1 < passes)
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}, names


@pytest.mark.parametrize("n_loss_calls", [2, 1])
def test_frame_gradients_with_a_loss_on_some_calls_only(dev, monkeypatch, n_loss_calls):
    """The loss reads the first calls' frames only: the later calls' FilmPosFramesFn nodes never run, and the frames they share with the
    earlier windows must still hand their (partial) sums to the encoder.  Against the plain path (one stacked window per call, autograd
    sums the frame gradients): fp32, 2e-5 of each tensor's largest entry.  (Round 4's per-tensor window counters never completed here
    and the encoder silently received no gradient.)"""
    g_acc, names = _g14_grads(dev, monkeypatch, True, n_loss_calls)
    g_ref, _ = _g14_grads(dev, monkeypatch, False, n_loss_calls)
    worst = 0.0
    for k in names:
        e = max_rel(g_acc[k].cpu(), g_ref[k].cpu())
        worst = max(worst, e)
        assert e < 2e-5, (k, e)
    enc = [k for k in names if k.startswith("encoder.")]
    assert enc and all(float(g_acc[k].abs().max()) > 0.0 for k in enc), "the encoder received no gradient"
    record_parity(worst, worst, 2e-5, "fp32", f"FilmPosFramesFn: loss on {n_loss_calls} of 4 calls vs the stacked-window path")


def test_frame_gradients_second_pass_over_a_retained_graph(dev, monkeypatch):
    """backward(retain_graph=True) followed by a second backward over the same graph: the gradient slots hold exactly twice one pass's
    gradients (round 4's node cleared its records in backward and crashed on re-entry)."""
    g2, names = _g14_grads(dev, monkeypatch, True, 4, passes=2)
    g1, _ = _g14_grads(dev, monkeypatch, True, 4, passes=1)
    worst = 0.0
    for k in names:
        e = max_rel(g2[k].cpu(), 2.0 * g1[k].cpu())
        worst = max(worst, e)
        assert e < 2e-5, (k, e)
    record_parity(worst, worst, 2e-5, "fp32", "FilmPosFramesFn: two passes over a retained graph = 2 x one pass")


# ---------------------------------------------------------------------------------------------------
# tante_block_bwd_fused: the whole backward of a TransformerBlock in one launch
# ---------------------------------------------------------------------------------------------------
def _block64(x, blk, idx, causal):
    """The block in float64 on the CPU from the module's own parameters (attn_backbone.py:59-83, eval-mode arithmetic)."""
    import torch.nn.functional as F
    from test_hip_round2 import _sdpa64
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in blk.named_parameters()}
    h = F.layer_norm(x, (256,), P["ln1.weight"], P["ln1.bias"], blk.ln1.eps)
    qkv = h @ P["attn.in_proj_weight"].T + P["attn.in_proj_bias"]
    o = _sdpa64(qkv, idx, 8, causal)
    x1 = x + o @ P["attn.out_proj.weight"].T + P["attn.out_proj.bias"]
    h2 = F.layer_norm(x1, (256,), P["ln2.weight"], P["ln2.bias"], blk.ln2.eps)
    hp = h2 @ P["mlp.0.weight"].T + P["mlp.0.bias"]
    return x1 + F.gelu(hp, approximate="tanh") @ P["mlp.2.weight"].T + P["mlp.2.bias"], P


BWD_SHAPES = [("T", 1, 4, 16, 48), ("H", 1, 4, 16, 48), ("W", 1, 4, 16, 48),      # cfg3's three letters: L = 4 (causal), 16, 48
              ("T", 1, 4, 5, 7),          # 35 sequences of 4: the last workgroup (12 per workgroup) has one live sequence
              ("H", 1, 2, 8, 5),          # L = 8: 10 sequences, 6 per workgroup
              ("T", 2, 2, 4, 4),          # L = 2, causal
              ("W", 2, 1, 3, 32),         # L = 32: two tiles per sequence, 32-token workgroups
              ("W", 1, 1, 3, 64),         # L = 64: four tiles per sequence, one workgroup per CU
              ("H", 3, 1, 1, 2)]          # L = 1: attention is the identity on v


@pytest.mark.parametrize("letter,B,T,H,W", BWD_SHAPES)
def test_block_backward_in_one_launch_against_float64(dev, letter, B, T, H, W, monkeypatch):
    """One TransformerBlock (C = 256, 8 heads, train() mode, dropout 0) through the one-launch training forward and the ONE-LAUNCH
    backward (tante_block_bwd_fused: q | k | v recomputed, the attention's backward between the two token-wise halves in LDS): the
    gradient of the input and of every parameter against float64 autograd of the same block on the CPU.  Bar: bf16 gradients, 4e-2 of
    each tensor's largest entry (measured: see the parity report).  Also: the forward really stored no packed projection."""
    import tante_amd
    from tante_amd import autograd as A, train_forward as TF, kernels as Kk, _lib as L
    from test_hip_round2 import _seq_tokens
    torch.manual_seed(17)
    blk = tante_amd.TransformerBlock(256, 8, mlp_ratio=1.0, dropout=0.0).to(dev).train()
    with torch.no_grad():
        for ln in (blk.ln1, blk.ln2):
            ln.weight.add_(0.2 * torch.randn_like(ln.weight))
            ln.bias.add_(0.2 * torch.randn_like(ln.bias))
        blk.attn.in_proj_bias.add_(0.2 * torch.randn_like(blk.attn.in_proj_bias))
        blk.attn.out_proj.bias.add_(0.2 * torch.randn_like(blk.attn.out_proj.bias))
    causal = letter == "T"
    seq = Kk.make_seq(letter, B, T, H, W)
    assert Kk.block_bwd_fused_supported(256, 8, 256, seq.L, causal)
    n = B * T * H * W
    x0 = torch.randn(n, 256, generator=torch.Generator().manual_seed(n)) * 1.3 + 0.2
    w = torch.randn(n, 256, generator=torch.Generator().manual_seed(n + 1))
    opt = tante_amd.FlatAdamW(blk.parameters(), lr=1e-3)
    opt.zero_grad()
    calls = []
    real = Kk.block_bwd_fused
    monkeypatch.setattr(Kk, "block_bwd_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = x0.to(dev).requires_grad_(True)
    with TF.fold_scope():
        y = TF.block_train(blk, x, seq, causal, L.BF16)
        assert y.grad_fn.saved_tensors[3] is None, "the forward stored the packed projection although the backward recomputes it"
        A.run_backward((y * w.to(dev)).sum())
    assert calls == [1], "the one-launch backward did not run"
    x64 = x0.double().requires_grad_(True)
    y64, P = _block64(x64, blk, _seq_tokens(seq), causal)
    (y64 * w.double()).sum().backward()
    e = max_rel(y.detach().cpu(), y64.detach())
    record_parity(rel_err(y.detach().cpu(), y64.detach()), e, 1e-2, "bf16", f"block training forward vs float64, {letter} L={seq.L}")
    assert e < 1e-2, e
    e = max_rel(x.grad.cpu(), x64.grad)
    record_parity(rel_err(x.grad.cpu(), x64.grad), e, 4e-2, "bf16", f"one-launch block backward vs float64, dx, {letter} L={seq.L}")
    assert e < 4e-2 and rel_err(x.grad.cpu(), x64.grad) < 1e-2, (e, rel_err(x.grad.cpu(), x64.grad))
    for k, p in blk.named_parameters():
        a_, b_ = p.grad.detach().cpu(), P[k].grad
        if k == "attn.in_proj_bias":      # its k third is zero up to rounding (a key bias cannot change a softmax)
            a_, b_ = torch.cat([a_[:256], a_[512:]]), torch.cat([b_[:256], b_[512:]])
        if seq.L == 1 and k in ("attn.in_proj_weight", "attn.in_proj_bias"):      # L = 1: q and k gradients vanish identically; compare v
            a_, b_ = a_[-256:], b_[-256:]
        e = max_rel(a_, b_)
        record_parity(rel_err(a_, b_), e, 4e-2, "bf16", f"one-launch block backward vs float64, {k}, {letter} L={seq.L}")
        assert e < 4e-2, (k, e)


@pytest.mark.parametrize("letter,B,T,H,W", [("T", 1, 4, 16, 48), ("H", 1, 4, 16, 48), ("W", 1, 4, 16, 48), ("H", 1, 2, 8, 5), ("W", 2, 1, 3, 32)])
def test_block_backward_in_one_launch_row_operands(dev, letter, B, T, H, W):
    """tante_block_bwd_fused against the three launches it replaces (tante_block_tail_bwd, tante_attention_bwd, tante_block_head_bwd) on the
    tensors ONE training forward saved, with dropout 0.1 and the same seeds: the row operands of the fc2 / fc1 / out-proj weight gradients
    are BIT-IDENTICAL (same arithmetic, same masks); dq | dk | dv and dx differ by the q | k | v recompute (q' rounded with the softmax
    scale folded in, exp2 domain) -- bf16 bar."""
    import tante_amd
    from tante_amd import kernels as Kk, _lib as L, train_forward as TF
    torch.manual_seed(23)
    blk = tante_amd.TransformerBlock(256, 8, mlp_ratio=1.0, dropout=0.1).to(dev).train()
    causal = letter == "T"
    seq = Kk.make_seq(letter, B, T, H, W)
    n = B * T * H * W
    x = (torch.randn(n, 256, generator=torch.Generator().manual_seed(n)) * 1.3 + 0.2).to(dev)
    dout = torch.randn(n, 256, generator=torch.Generator().manual_seed(n + 2)).to(dev)
    a, m = blk.attn, blk.mlp
    with torch.no_grad(), TF.fold_scope():
        w_in, b_in = TF._folded(a.in_proj_weight, a.in_proj_bias, blk.ln1)
        w1, b1 = TF._folded(m[0].weight, m[0].bias, blk.ln2)
        w_in, b_in, w1, b1 = w_in.detach(), b_in.detach(), w1.detach(), b1.detach()
        fs = Kk.pack_block_train((w_in, b_in, a.out_proj.weight, a.out_proj.bias, w1, b1, m[2].weight, m[2].bias), 256, 256)
        bst = Kk.pack_block_tail_bwd(m[2].weight, w1, a.out_proj.weight, 256, 256)
        hst = Kk.pack_block_tail_bwd(w_in[0:256], w_in[256:512], w_in[512:768], 256, 256)
    seeds = (0x1234567890ABCDEF, 0x0FEDCBA987654321, 0x55AA55AA12345678)
    t = Kk.block_fused_train(x, fs, 256, 8, 256, seq, causal, blk.ln1.eps, 0.1, seeds, need_x1=False)
    r = Kk.block_tail_bwd(dout, t["hpre"], t["xh2"], t["st2"], bst, 256, 256, 0.1, seeds[1], seeds[2])
    dqkv = torch.empty_like(t["qkv"])
    s = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().tante_attention_bwd(t["qkv"].data_ptr(), r["do"].data_ptr(), dqkv.data_ptr(), L.BF16, 256, 8, Ct.byref(seq), int(causal), 0.1,
                                        seeds[0], s), "attention_bwd")
    dx3 = Kk.block_head_bwd(dqkv, t["xh1"], t["st1"], r["dx1"], hst, 256)
    f = Kk.block_bwd_fused(dout, t["xh1"], t["st1"], t["hpre"], t["xh2"], t["st2"], bst, fs, hst, 256, 8, 256, seq, causal, 0.1, seeds)
    for k in ("dy2", "dhpre", "dy1"):
        assert torch.equal(f[k], r[k]), k
    for i, name in enumerate(("dq", "dk", "dv")):
        a_, b_ = f["dqkv"][:, 256 * i:256 * (i + 1)].float().cpu(), dqkv[:, 256 * i:256 * (i + 1)].float().cpu()
        e = max_rel(a_, b_)
        record_parity(rel_err(a_, b_), e, 2e-2, "bf16", f"one-launch block backward vs tante_attention_bwd, {name}, {letter} L={seq.L}, p=0.1")
        assert e < 2e-2 and rel_err(a_, b_) < 1e-2, (name, e, rel_err(a_, b_))
    e = max_rel(f["dx"].cpu(), dx3.cpu())
    record_parity(rel_err(f["dx"].cpu(), dx3.cpu()), e, 2e-2, "bf16", f"one-launch block backward vs three launches, dx, {letter} L={seq.L}, p=0.1")
    assert e < 2e-2 and rel_err(f["dx"].cpu(), dx3.cpu()) < 5e-3, (e, rel_err(f["dx"].cpu(), dx3.cpu()))


# ---------------------------------------------------------------------------------------------------
# g15: training-surface cases closed in round 5, against the REFERENCE's gradients
# ---------------------------------------------------------------------------------------------------
def _names(pattern):
    import glob
    import os
    from conftest import GOLDEN
    return sorted(os.path.basename(q)[:-4] for q in glob.glob(os.path.join(GOLDEN, pattern + ".npz")))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", _names("g15_encdec_grad_*"))
def test_g15_padded_stages_train(dev, name, mode):
    """enc_CNN / dec_CNN with 'same'-padded kernel-4 stages (patch_scale 16 / 32 / 64; 32 is the constructor default,
    enc_dec_cnn.py:39-46, 66-81, 128-143) under autograd: round 4 raised NotImplementedError on the train path.  Output, input gradient
    and every parameter's gradient against the reference's backward() (fixture g15).  Bars: fp32 1e-5 / 2e-4, bf16 1e-2 / 4e-2."""
    import contextlib
    import tante_amd
    from conftest import load_golden, split_prefix
    g = load_golden(name)
    ps, _, H, W, nf, C = (int(v) for v in g["meta"])
    md = tante_amd.TanteMetadata(n_fields=nf, spatial_resolution=(H, W))
    e = tante_amd.enc_CNN(md, embed_dim=C, patch_scale=ps, overlap_ratio=0.0).to(dev).train()
    d = tante_amd.dec_CNN(md, embed_dim=C, patch_scale=ps, overlap_ratio=0.0).to(dev).train()
    e.load_state_dict(split_prefix(g, "enc."))
    d.load_state_dict(split_prefix(g, "dec."))
    amp = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if mode == "bf16" else contextlib.nullcontext
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    x = g["x"].to(dev).requires_grad_(True)
    with amp():
        z = e(x)
    (z.float() * g["wz"].to(dev)).sum().backward()
    assert max_rel(z.detach().float().cpu(), g["z"]) < ft
    worst = max_rel(x.grad.cpu(), g["dx"])
    assert worst < gt, ("dx", worst)
    for k, q in e.named_parameters():
        err = max_rel(q.grad.cpu(), g["genc." + k])
        worst = max(worst, err)
        assert err < gt, (k, err)
    record_parity(worst, worst, gt, mode, f"{name}: enc_CNN gradients (input and parameters) vs the reference")
    zz = g["zz"].to(dev).requires_grad_(True)
    with amp():
        r = d(zz)
    (r.float() * g["wr"].to(dev)).sum().backward()
    assert max_rel(r.detach().float().cpu(), g["r"]) < ft
    worst = max_rel(zz.grad.cpu(), g["dzz"])
    assert worst < gt, ("dzz", worst)
    for k, q in d.named_parameters():
        err = max_rel(q.grad.cpu(), g["gdec." + k])
        worst = max(worst, err)
        assert err < gt, (k, err)
    record_parity(worst, worst, gt, mode, f"{name}: dec_CNN gradients (input and parameters) vs the reference")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", _names("g15_backbone_grad_*"))
def test_g15_channel_letter_train(dev, name, mode):
    """Attn_Backbone with the channel-attention letter 'C' (attn_backbone.py:184-189) under autograd -- alone and inside "LTCAXY":
    round 4 raised on the train path.  Output, input gradient and every parameter's gradient against the reference's backward()."""
    import tante_amd
    from conftest import load_golden, split_prefix
    g = load_golden(name)
    axes = name.split("_")[-1]
    T, H, W, C, E, nh = (int(v) for v in g["meta"])
    bb = tante_amd.Attn_Backbone((T, H, W, C), axes, expanded_channel=E, n_head=nh, mlp_ratio=1.0, dropout=0.0).to(dev).train()
    bb.load_state_dict(split_prefix(g, "w."))
    bb.compute = mode
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    x = g["x"].to(dev).requires_grad_(True)
    y = bb(x)
    (y.float() * g["w"].to(dev)).sum().backward()
    assert max_rel(y.detach().float().cpu(), g["y"]) < ft * (3 if len(axes) > 1 else 1)
    worst = max_rel(x.grad.cpu(), g["dx"])
    assert worst < gt, ("dx", worst)
    ours, refs = [], []
    for k, q in bb.named_parameters():
        ref = g["g." + k]
        ours.append(q.grad.cpu().reshape(-1))
        refs.append(ref.reshape(-1))
        if float(ref.abs().max()) == 0.0:
            assert float(q.grad.abs().max()) == 0.0, k
            continue
        if mode == "fp32":
            err = max_rel(q.grad.cpu(), ref)
            assert err < gt, (k, err)
        else:
            # bf16: relative L2 per tensor (as test_submodules_are_differentiable_standalone).  A bias gradient is a sum over 4 608 rows; where
            # the reference's sum is a cancellation (the C block's fc2 bias: 1.55 against entries of magnitude ~2.4) the rounding noise of
            # bf16 TERMS was 12 % of the value (round 5: vectors got 3.5 x the bar).  Round 6: the closing projections of a branch sum their
            # fp32 rows (autograd.BranchOutFn, FP32_BIAS_SUMS): that vector is at 2.3e-2 now and the worst vector (LayerNorm1's bias, whose
            # gradient comes through the bf16 q | k | v gradient rows) at 4.0e-2: vectors 1.25 x the bar, matrices and the whole gradient the bar.
            err = rel_err(q.grad.cpu(), ref)
            assert err < (gt if ref.dim() > 1 else 1.25 * gt), (k, err)
        worst = max(worst, err)
    err = rel_err(torch.cat(ours), torch.cat(refs))
    assert err < gt, ("all parameters", err)
    record_parity(max(worst, err), max(worst, err), gt if mode == "fp32" else 1.25 * gt, mode,
                  f"{name}: Attn_Backbone gradients (input and parameters) vs the reference; all parameters concatenated: {err:.2e}")


def test_constructor_default_patch_scale_trains(dev):
    """TANTE's constructor default is patch_scale = 32 (tante.py:38-60: Patch_map[32] = (2, 4, 4), two 'same'-padded kernel-4 stages):
    a forward + backward through the whole model on the HIP train path against torch autograd through the CPU oracle (fp32 compute;
    output 1e-5, gradients 2e-4 of each tensor's largest entry).  Round 4 raised NotImplementedError here."""
    import tante_amd
    from oracle import tante_oracle as O
    torch.manual_seed(77)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(64, 64))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=2, attn_axes="TH-WL", n_head=4, embed_dim=64, dropout=0.0).to(dev).train().set_compute("fp32")
    assert sorted(m.encoder.P) == [2, 4, 4]
    g = torch.Generator().manual_seed(78)
    x = torch.randn(2, 4, 2, 64, 64, generator=g)
    w = torch.randn(2, 1, 2, 64, 64, generator=g)
    y = m(x.to(dev))
    (y * w.to(dev)).sum().backward()
    wo = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    cfg = O.TanteCfg(4, 2, (64, 64), taylor_order=2, attn_axes="TH-WL", n_head=4, embed_dim=64, patch_scale=32)
    yo = O.tante_forward(wo, cfg, x)
    (yo * w).sum().backward()
    e = max_rel(y.detach().cpu(), yo.detach())
    record_parity(rel_err(y.detach().cpu(), yo.detach()), e, 1e-5, "fp32", "TANTE(patch_scale=32) training forward vs oracle")
    assert e < 1e-5, e
    worst = 0.0
    for k, q in m.named_parameters():
        if wo[k].grad is None:
            continue
        err = max_rel(q.grad.cpu(), wo[k].grad)
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    record_parity(worst, worst, 2e-4, "fp32", "TANTE(patch_scale=32) parameter gradients vs oracle autograd")


def test_graphed_rollout_follows_compute_and_option_changes(dev):
    """GraphedRollout keyed its capture on the parameters only and kept replaying a stale graph after
    `model.set_compute(...)` or a `set_option` flip.  The key now carries the resolved compute mode and the options epoch."""
    import tante_amd
    torch.manual_seed(3)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(64, 64))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=1, attn_axes="THW", n_head=8, embed_dim=256, patch_scale=8, dropout=0.0).to(dev).eval()
    m.set_compute("bf16")
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    g = torch.Generator().manual_seed(4)
    batch = {"input": torch.randn(2, 4, 64, 64, 2, generator=g).to(dev), "output": torch.randn(2, 3, 64, 64, 2, generator=g).to(dev)}
    roll = tante_amd.GraphedRollout(m, batch, fmt, 3)
    y16 = roll(batch)[0].clone()
    with torch.inference_mode():
        e16 = tante_amd.rollout_model(m, batch, fmt, 3, device=dev)[0]
    assert torch.equal(y16, e16)
    k0 = roll._key
    m.set_compute("fp32")
    y32 = roll(batch)[0].clone()
    assert roll._key != k0, "no re-capture after set_compute"
    with torch.inference_mode():
        e32 = tante_amd.rollout_model(m, batch, fmt, 3, device=dev)[0]
    assert torch.equal(y32, e32) and not torch.equal(y32, y16)
    k1 = roll._key
    tante_amd.set_option("TANTE_HEAD_ENC", 1)      # any set_option bumps the options epoch
    roll(batch)
    assert roll._key != k1, "no re-capture after set_option"


def test_epoch_with_amp_equals_the_bf16_compute_mode_and_float_masks_block_under_causal(dev):
    """ADVICE round 4, harness.py: train_one_epoch(enable_amp=True) wrapped backward and the optimizer step in the autocast context (the
    reference leaves it before backward, trainer/trainer.py:183-196).  It now switches the model's compute mode for the forward only: two
    steps land exactly where two `set_compute("bf16")` steps land, and the model's own setting is restored.  And TransformerBlock.forward
    with a FLOAT attn_mask plus causal=True blocks every non-zero entry (attn_backbone.py:70-72: `attn_mask.bool() | causal_mask`)."""
    import copy
    import tante_amd
    from tante_amd import autograd as A, harness as H
    from tante_amd.train import train_step
    torch.manual_seed(5)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(64, 64))
    m1 = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=1, attn_axes="THW", n_head=8, embed_dim=256, patch_scale=8, dropout=0.0).to(dev).train()
    m2 = copy.deepcopy(m1)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    g = torch.Generator().manual_seed(9)
    batches = [{"input": torch.randn(2, 4, 64, 64, 2, generator=g), "output": torch.randn(2, 2, 64, 64, 2, generator=g)} for _ in range(2)]
    o1 = tante_amd.FlatAdamW(m1.parameters(), lr=1e-4, weight_decay=0.01, max_norm=1.0)
    o2 = tante_amd.FlatAdamW(m2.parameters(), lr=1e-4, weight_decay=0.01, max_norm=1.0)
    A._SEED[0] = 77
    l1 = H.train_one_epoch(m1, o1, batches, fmt, 2, enable_amp=True, amp_type="bfloat16")
    assert m1.compute is None
    A._SEED[0] = 77
    m2.set_compute("bf16")
    l2 = [float(train_step(m2, o2, {k: v.to(dev) for k, v in b.items()}, fmt, 2, 1)) for b in batches]
    assert abs(l1 - sum(l2) / 2) < 1e-6 * abs(l1)
    assert float((o1.flat_p - o2.flat_p).abs().max()) < 1e-7
    # float mask + causal
    torch.manual_seed(6)
    blk = tante_amd.TransformerBlock(64, 4, mlp_ratio=1.0, dropout=0.0).to(dev).eval()
    x = torch.randn(3, 8, 64, device=dev)
    fm = torch.zeros(8, 8)
    fm[5, 2] = 0.5          # a float entry that an ADDITIVE mask would merely nudge; under causal it must block (5 -> 2)
    fm[1, 0] = -3.0
    with torch.no_grad():
        y_f = blk(x, attn_mask=fm.to(dev), causal=True)
        y_b = blk(x, attn_mask=(fm != 0).to(dev), causal=True)
        y_c = blk(x, causal=True)
    assert torch.equal(y_f, y_b) and not torch.equal(y_f, y_c)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Cin,src", [(4, 32, torch.bfloat16), (4, 16, torch.float32), (2, 128, torch.float32), (2, 64, torch.bfloat16)])
def test_conv_stage_gathers_patches_inside_the_gemm(dev, P, Cin, src):
    """stages.conv_stage on a channels-first image without overlap (enc_dec_fno.py:224-273's two conv stages at cfg5): the patch gather as
    the dense GEMM's fragment load (gemm.hip patch_frag) -- bit-identical to tante_im2col + the dense GEMM it replaces, and equal to
    torch's conv2d on the bf16-rounded operands within fp32 accumulation order."""
    import tante_amd
    from tante_amd import stages as S, _lib as L
    torch.manual_seed(P * 100 + Cin)
    n, H, W, Cout = 3, 24 * P, 32 * P, 48          # 3 * 24 * 32 = 2304 patches < 4096: falls back; 6 images -> 4608 use the fused route
    pad = (P - 1) // 2                             # enc_dec_cnn.py:66-81: P = 4 reaches one pixel over the top / left edge
    conv = torch.nn.Conv2d(Cin, Cout, (P, P), stride=(P, P), padding=(pad, pad)).to(dev)
    chunks = S.pack_linear_chunks(S.conv_weight_2d(conv.weight, 0), conv.bias, L.BF16)
    for n_img in (n, 2 * n):
        x = torch.randn(n_img, Cin, H, W, device=dev).to(src).contiguous()
        outs = {}
        for on in (1, 0):
            tante_amd.set_option("TANTE_CONV_PATCH_GEMM", on)
            try:
                for act in (L.ACT_NONE, L.ACT_GELU_ERF):
                    y, ht, wt = S.conv_stage(x, True, n_img, Cin, H, W, P, 0.0, chunks, L.BF16, act, torch.float32)
                    assert (ht, wt) == (H // P, W // P)
                    outs[(on, act)] = y
            finally:
                tante_amd.set_option("TANTE_CONV_PATCH_GEMM", 1)
        for act in (L.ACT_NONE, L.ACT_GELU_ERF):
            assert torch.equal(outs[(1, act)], outs[(0, act)]), (n_img, act, (outs[(1, act)] - outs[(0, act)]).abs().max().item())
            # channels-first output (the GEMM's own epilogue on the fused route, a layout copy otherwise): the same numbers, transposed
            ycf, _, _ = S.conv_stage(x, True, n_img, Cin, H, W, P, 0.0, chunks, L.BF16, act, torch.float32, nchw_out=True)
            assert ycf.shape == (n_img, Cout, H // P, W // P)
            assert torch.equal(ycf.permute(0, 2, 3, 1).reshape(-1, Cout), outs[(1, act)]), (n_img, act)
        wq = conv.weight.detach().bfloat16().float()
        ref = torch.nn.functional.conv2d(x.bfloat16().float(), wq, conv.bias.detach(), stride=P, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
        e = rel_err(outs[(1, L.ACT_NONE)], ref)
        record_parity(e, e, 1e-5, "bf16", f"conv stage with the patch gather inside the GEMM vs conv2d on bf16-rounded operands, P={P} Cin={Cin} n={n_img}")
        assert e < 1e-5, e


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", _names("g16_encdec_grad_*"))
def test_g16_overlapping_stages_train(dev, name, mode):
    """enc_CNN / dec_CNN with OVERLAPPING stages (overlap_ratio 0.5 is their constructor default, enc_dec_cnn.py:39-46; 0.25 gives stride 3
    under kernel 4 = uneven pooling windows) under autograd: conv with stride < kernel -> adaptive average pool (AvgPoolFn, new
    tante_avgpool_nhwc_bwd) / tap GEMM -> summed taps (Col2imFn) -> bilinear resize.  Until round 5 the train path raised
    NotImplementedError.  Output, input gradient and every parameter's gradient against the reference's backward() (fixture g16)."""
    import contextlib
    import tante_amd
    from conftest import load_golden, split_prefix
    g = load_golden(name)
    ps, ov, H, W, nf, C = (int(v) for v in g["meta"])
    ov = ov / 100.0
    md = tante_amd.TanteMetadata(n_fields=nf, spatial_resolution=(H, W))
    e = tante_amd.enc_CNN(md, embed_dim=C, patch_scale=ps, overlap_ratio=ov).to(dev).train()
    d = tante_amd.dec_CNN(md, embed_dim=C, patch_scale=ps, overlap_ratio=ov).to(dev).train()
    e.load_state_dict(split_prefix(g, "enc."))
    d.load_state_dict(split_prefix(g, "dec."))
    amp = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if mode == "bf16" else contextlib.nullcontext
    ft, gt = (1e-5, 2e-4) if mode == "fp32" else (1e-2, 4e-2)
    x = g["x"].to(dev).requires_grad_(True)
    with amp():
        z = e(x)
    (z.float() * g["wz"].to(dev)).sum().backward()
    assert max_rel(z.detach().float().cpu(), g["z"]) < ft
    worst = max_rel(x.grad.cpu(), g["dx"])
    assert worst < gt, ("dx", worst)
    for k, q in e.named_parameters():
        err = max_rel(q.grad.cpu(), g["genc." + k])
        worst = max(worst, err)
        assert err < gt, (k, err)
    record_parity(worst, worst, gt, mode, f"{name}: enc_CNN gradients (input and parameters) vs the reference")
    zz = g["zz"].to(dev).requires_grad_(True)
    with amp():
        r = d(zz)
    (r.float() * g["wr"].to(dev)).sum().backward()
    assert max_rel(r.detach().float().cpu(), g["r"]) < ft
    worst = max_rel(zz.grad.cpu(), g["dzz"])
    assert worst < gt, ("dzz", worst)
    for k, q in d.named_parameters():
        err = max_rel(q.grad.cpu(), g["gdec." + k])
        worst = max(worst, err)
        assert err < gt, (k, err)
    record_parity(worst, worst, gt, mode, f"{name}: dec_CNN gradients (input and parameters) vs the reference")


@pytest.mark.gpu
def test_overlapping_model_trains(dev):
    """A whole TANTE with overlap_ratio = 0.5 (tante.py:58 passes it to both enc_CNN and dec_CNN) on the HIP train path: forward + backward
    against torch autograd through the CPU oracle, fp32 compute (output 1e-5, gradients 2e-4 of each tensor's largest entry), then one
    train_step in bf16 that must move the loss."""
    import tante_amd
    from oracle import tante_oracle as O
    torch.manual_seed(81)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(32, 64))
    kw = dict(taylor_order=2, attn_axes="TH-WL", n_head=4, embed_dim=64, patch_scale=16, overlap_ratio=0.5)
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, dropout=0.0, **kw).to(dev).train().set_compute("fp32")
    g = torch.Generator().manual_seed(82)
    x = torch.randn(2, 4, 2, 32, 64, generator=g)
    w = torch.randn(2, 1, 2, 32, 64, generator=g)
    y = m(x.to(dev))
    (y * w.to(dev)).sum().backward()
    wo = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    cfg = O.TanteCfg(4, 2, (32, 64), **kw)
    yo = O.tante_forward(wo, cfg, x)
    (yo * w).sum().backward()
    e = max_rel(y.detach().cpu(), yo.detach())
    record_parity(rel_err(y.detach().cpu(), yo.detach()), e, 1e-5, "fp32", "TANTE(overlap_ratio=0.5) training forward vs oracle")
    assert e < 1e-5, e
    worst = 0.0
    for k, q in m.named_parameters():
        if wo[k].grad is None:
            continue
        err = max_rel(q.grad.cpu(), wo[k].grad)
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    record_parity(worst, worst, 2e-4, "fp32", "TANTE(overlap_ratio=0.5) parameter gradients vs oracle autograd")
    m.set_compute("bf16")
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=0.0, max_norm=1.0)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    batch = {"input": torch.randn(2, 4, 32, 64, 2, generator=g).to(dev), "output": torch.randn(2, 2, 32, 64, 2, generator=g).to(dev)}
    l0 = float(tante_amd.train_step(m, opt, batch, fmt, 2, 1))
    for _ in range(5):
        l1 = float(tante_amd.train_step(m, opt, batch, fmt, 2, 1))
    assert l1 < l0, (l0, l1)


@pytest.mark.gpu
@pytest.mark.parametrize("src", [torch.float32, torch.bfloat16])
def test_deconv2_channels_first_in_the_register_stationary_kernel(dev, src):
    """stages.deconv_stage with kernel = stride = 2 and a channels-first fp32 output (enc_dec_fno.py:276-323's first decoder stage at cfg5:
    32768 x 256 -> 128 x 2 x 2): the register-stationary GEMM with the pixel shuffle as its epilogue (gemm.hip epilogue4_dnchw2) against
    the generic kernel it replaces (TANTE_GEMM_NO_LITE) and against torch's conv_transpose2d on bf16-rounded operands."""
    import tante_amd
    from tante_amd import stages as S, kernels as K, _lib as L
    torch.manual_seed(5)
    n, h, w, Cin, Cout = 2, 48, 64, 256, 40          # 6144 rows
    dc = torch.nn.ConvTranspose2d(Cin, Cout, (2, 2), stride=(2, 2)).to(dev)
    pw = K.pack_weight(dc.weight, dc.bias, L.BF16, L.W_DECONV_NCHW, N=Cout * 4, K=Cin, P=2, C_other=Cout)
    rows = torch.randn(n * h * w, Cin, device=dev).to(src).contiguous()
    for act in (L.ACT_NONE, L.ACT_GELU_ERF):
        y = S.deconv_stage(rows, n, h, w, 2, 0.0, pw, Cout, L.BF16, act, True, torch.float32)
        tante_amd.set_option("TANTE_GEMM_NO_LITE", 1)
        try:
            y0 = S.deconv_stage(rows, n, h, w, 2, 0.0, pw, Cout, L.BF16, act, True, torch.float32)
        finally:
            tante_amd.set_option("TANTE_GEMM_NO_LITE", 0)
        assert y.shape == (n, Cout, 2 * h, 2 * w)
        e0 = rel_err(y, y0)
        assert e0 < 1e-6, (act, e0)
        x4 = rows.float().bfloat16().float().view(n, h, w, Cin).permute(0, 3, 1, 2)
        ref = torch.nn.functional.conv_transpose2d(x4, dc.weight.detach().bfloat16().float(), dc.bias.detach(), stride=2)
        if act == L.ACT_GELU_ERF:
            ref = torch.nn.functional.gelu(ref)
        e = rel_err(y, ref)
        record_parity(e, e, 2e-5, "bf16", f"kernel-2 transposed conv, channels-first epilogue, act {act}, rows {str(src).split('.')[-1]}")
        assert e < 2e-5, (act, e)


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout", [(64, 128), (128, 64)])
def test_wide_spectral_layers_on_the_bf16_matrix_pipe(dev, Cin, Cout):
    """SpectralLayer (enc_dec_fno.py:184-222) at cfg5's two wide shapes (64 -> 128 and 128 -> 64 channels on 128 x 128, modes 10 x 10) in the
    bf16 compute mode: the inverse row transform + 1 x 1 conv with split-operand products on the bf16 matrix pipe
    (idft_rows_conv_x3w_kernel, a . b ~= a_hi b_hi + a_lo b_hi + a_hi b_lo) against the fp32-MFMA kernel it replaces there
    (TANTE_SPECTRAL_X3 = 0) and against the torch.fft restatement of the layer; 5 images, so that workgroups walk several rows."""
    import tante_amd
    from tante_amd import _lib as L
    from oracle import spectral_oracle as SO
    torch.manual_seed(Cin)
    layer = tante_amd.SpectralLayer(Cin, Cout, 10, 10).to(dev)
    x = torch.randn(5, Cin, 128, 128, device=dev)
    for act in (L.ACT_NONE, L.ACT_GELU_ERF):
        y = layer.run(x, act, L.BF16)
        tante_amd.set_option("TANTE_SPECTRAL_X3", 0)
        try:
            y0 = layer.run(x, act, L.BF16)
        finally:
            tante_amd.set_option("TANTE_SPECTRAL_X3", 1)
        e0 = max_rel(y, y0)
        assert e0 < 2e-4, (act, e0)
        sd = {k: v.detach().cpu() for k, v in layer.state_dict().items()}
        ref = SO.spectral_layer(sd, x.cpu(), 10, 10)
        if act == L.ACT_GELU_ERF:
            ref = torch.nn.functional.gelu(ref)
        e = max_rel(y.cpu(), ref)
        record_parity(rel_err(y.cpu(), ref), e, 2e-4, "bf16", f"wide spectral layer {Cin}->{Cout}, split-bf16 inverse rows, act {act}")
        assert e < 2e-4, (act, e)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol", [("fp32", 1e-5), ("bf16", 1e-2)])
def test_spectral_encoder_frame_cache_in_the_rollout(dev, mode, tol):
    """rollout._rollout_in_place with the spectral encoder: every frame encoded once and a window assembled from the cached per-frame
    encodings + tante_film_pos_fwd_frames (TANTE._enc_cache_frames; enc_dec_fno.py:224-273 is per frame, tante.py:136-141 applies FiLM(t)
    and the positional terms behind it) against the window-by-window path (TANTE_NO_ENC_CACHE = 1) -- the same function; the mode mixing's
    channel split depends on the image count, so fp32 agrees to rounding and bf16 to its own bar."""
    import tante_amd
    from tante_amd import rollout as R
    torch.manual_seed(31)
    md = tante_amd.TanteMetadata(n_fields=3, spatial_resolution=(64, 64))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=1, attn_axes="THW", n_head=8, embed_dim=256, patch_scale=8, overlap_ratio=0.0,
                        enc_dec_type="fno", modes1=8, modes2=8).to(dev).eval().set_compute(mode)
    assert m.enc_cache_supported() and m.route(enc_cache=True, B=2).source == "cache_film_pass"
    x = torch.randn(2, 4, 3, 64, 64, device=dev)
    with torch.no_grad():
        y1 = R._rollout_in_place(m, x, 5).clone()
        tante_amd.set_option("TANTE_NO_ENC_CACHE", 1)
        try:
            y0 = R._rollout_in_place(m, x, 5).clone()
        finally:
            tante_amd.set_option("TANTE_NO_ENC_CACHE", 0)
    assert y1.shape == (2, 5, 3, 64, 64) and torch.isfinite(y1).all()
    e = rel_err(y1, y0)
    record_parity(e, max_rel(y1, y0), tol, mode, "rollout with the spectral encoder's frame cache vs window-by-window encoding")
    assert e < tol, e


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,Ht,Wt", [(7, 10, 3, 4), (15, 9, 5, 3), (12, 12, 6, 6), (5, 5, 5, 5), (9, 4, 2, 1)])
def test_adaptive_average_pool_backward_against_torch(dev, H, W, Ht, Wt):
    """tante_avgpool_nhwc / tante_avgpool_nhwc_bwd (AvgPoolFn: F.adaptive_avg_pool2d behind an overlapping conv, enc_dec_cnn.py:104-110) on
    window geometries where cells overlap (H % Ht != 0), against torch's own forward and backward."""
    from tante_amd.autograd import AvgPoolFn
    torch.manual_seed(H * 100 + W)
    n, C_ = 3, 12
    x = torch.randn(n, H, W, C_, device=dev, requires_grad=True)
    y = AvgPoolFn.apply(x.reshape(n * H * W, C_), n, H, W, C_, Ht, Wt, torch.float32)
    w = torch.randn_like(y)
    (y * w).sum().backward()
    xr = x.detach().clone().requires_grad_(True)
    yr = torch.nn.functional.adaptive_avg_pool2d(xr.permute(0, 3, 1, 2), (Ht, Wt)).permute(0, 2, 3, 1).reshape(n * Ht * Wt, C_)
    (yr * w).sum().backward()
    assert rel_err(y.detach(), yr.detach()) < 1e-6
    e = rel_err(x.grad, xr.grad)
    record_parity(e, e, 1e-6, "fp32", f"adaptive average pool backward {H}x{W} -> {Ht}x{Wt}")
    assert e < 1e-6, e


@pytest.mark.gpu
def test_gemm_refuses_padding_it_cannot_serve(dev):
    """TanteGemm.a_pad is implemented by the register-stationary bf16 patch path only (P = 4, pad 1, K = 256 / 512, M >= 4096): anything else
    must fail loudly (-2), not run unpadded."""
    from tante_amd import kernels as K, stages as S, _lib as L
    conv = torch.nn.Conv2d(64, 32, (2, 2), stride=(2, 2)).to(dev)
    pw = S.pack_linear_chunks(S.conv_weight_2d(conv.weight, 0), conv.bias, L.BF16)[0]
    x = torch.randn(8, 64, 64, 64, device=dev)
    y = torch.empty(8 * 32 * 32, 32, device=dev)
    with pytest.raises(RuntimeError, match="a_pad"):
        K.patch_embed(x, pw, y, n_img=8, Hin=64, Win=64, Cin=64, P=2, nchw=True, act=L.ACT_NONE, pad=1)
    conv4 = torch.nn.Conv2d(16, 32, (4, 4), stride=(4, 4), padding=1).to(dev)
    pw4 = S.pack_linear_chunks(S.conv_weight_2d(conv4.weight, 0), conv4.bias, L.BF16)[0]
    xs = torch.randn(1, 16, 64, 64, device=dev)      # 256 patches: below the path's M >= 4096
    with pytest.raises(RuntimeError, match="a_pad"):
        K.patch_embed(xs, pw4, torch.empty(256, 32, device=dev), n_img=1, Hin=64, Win=64, Cin=16, P=4, nchw=True, act=L.ACT_NONE, pad=1)


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,H,W,m", [(8, 32, 64, 512, 20), (32, 8, 48, 256, 12), (3, 5, 32, 96, 6)])
def test_row_transform_with_split_operands(dev, Cin, Cout, H, W, m):
    """SpectralLayer (enc_dec_fno.py:184-222) in the bf16 compute mode: the forward row DFT as split-bf16 products on the bf16 matrix pipe
    (dft_rows_x3_kernel) against the fp32-MFMA kernels (TANTE_SPECTRAL_X3 = 0) and the torch.fft restatement -- 2e-4 of the largest entry
    (the bf16 mode's own bar is 1e-2); ragged row counts (n Cin H not a multiple of 32) and a width that is not a multiple of 64."""
    import tante_amd
    from tante_amd import _lib as L
    from oracle import spectral_oracle as SO
    torch.manual_seed(W + Cin)
    layer = tante_amd.SpectralLayer(Cin, Cout, m, m).to(dev)
    x = torch.randn(3, Cin, H, W, device=dev)
    y = layer.run(x, L.ACT_NONE, L.BF16)
    tante_amd.set_option("TANTE_SPECTRAL_X3", 0)
    try:
        y0 = layer.run(x, L.ACT_NONE, L.BF16)
    finally:
        tante_amd.set_option("TANTE_SPECTRAL_X3", 1)
    assert max_rel(y, y0) < 2e-4, max_rel(y, y0)
    ref = SO.spectral_layer({k: v.detach().cpu() for k, v in layer.state_dict().items()}, x.cpu(), m, m)
    e = max_rel(y.cpu(), ref)
    record_parity(rel_err(y.cpu(), ref), e, 2e-4, "bf16", f"spectral layer {Cin}->{Cout} at {H}x{W}, split-bf16 row transform")
    assert e < 2e-4, e


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_cvit_query_chunks_share_one_encoding(dev, mode):
    """Evaler.rollout_cvit (trainer/evaler.py:140-165) runs the whole model per query chunk; the encoder half (cvit.py:437-448) does not
    depend on the query points: `CViT.encode(x)` once per window + `forward(x, coords, encoded=...)` per chunk gives the same bits as
    the per-chunk full forward, and harness.rollout_cvit_eval (which now does that) the same as a loop of plain calls."""
    import tante_amd
    from tante_amd import harness as Hn
    torch.manual_seed(4)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 24))
    m = tante_amd.CViT(4, md, out_steps=2, patch_size=(1, 8, 8), grid_size=(16, 24), latent_dim=24, emb_dim=32, depth=2, num_heads=4,
                       dec_emb_dim=32, dec_num_heads=4, dec_depth=2).to(dev).eval().set_compute(mode)
    x = torch.randn(2, 4, 2, 16, 24, device=dev)
    cc, ii = Hn.generate_chunked_coords_with_indices(16, 24, 100, dev)
    with torch.no_grad():
        enc = m.encode(x)
        for c in cc:
            assert torch.equal(m(x, c, encoded=enc), m(x, c))
        with pytest.raises(ValueError):
            m(x[:1], cc[0], encoded=enc)
        fmt = tante_amd.DefaultChannelsFirstFormatter(md)
        batch = {"input": torch.randn(2, 4, 16, 24, 2), "output": torch.randn(2, 4, 16, 24, 2)}
        y, _ = Hn.rollout_cvit_eval(m, batch, fmt, n_steps=4, num_query_points=100, device=dev)
        mov = fmt.process_input(batch)[0][0].to(dev)
        outs = []
        for _ in range(2):
            f = Hn.reconstruct_full_field([m(mov, c) for c in cc], ii, 16, 24)
            outs.append(fmt.process_output(f))
            mov = torch.cat([mov[:, f.shape[1]:], f], dim=1)
        assert torch.equal(y, torch.cat(outs, dim=1)[:, :4])


@pytest.mark.gpu
def test_graphed_rollout_with_the_spectral_frame_cache(dev):
    """GraphedRollout (one captured HIP graph per rollout) over a TANTE with the spectral encoder: the frame cache's copies and the
    per-window FiLM pass are captured with the rest -- the replay gives the eager rollout's bits, twice."""
    import tante_amd
    torch.manual_seed(33)
    md = tante_amd.TanteMetadata(n_fields=3, spatial_resolution=(64, 64))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=1, attn_axes="THW", n_head=8, embed_dim=256, patch_scale=8, overlap_ratio=0.0,
                        enc_dec_type="fno", modes1=8, modes2=8).to(dev).eval().set_compute("bf16")
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    batch = {"input": torch.randn(2, 4, 64, 64, 3, device=dev), "output": torch.randn(2, 3, 64, 64, 3, device=dev)}
    with torch.no_grad():
        y0, _ = tante_amd.rollout_model(m, batch, fmt, 3)
        roll = tante_amd.GraphedRollout(m, batch, fmt, 3)
        y1 = roll(batch)[0].clone()
        y2 = roll(batch)[0].clone()
    assert torch.equal(y0, y1) and torch.equal(y1, y2)
