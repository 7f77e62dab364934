"""GPU: training the AFNO baseline behind set_trainable() -- the filter's autograd node alone, one Block, the whole model, BPTT through a
re-fed rollout and an optimiser loop, every gradient against float64 autograd of the restatement in tests/afno_grad_ref.py.

The soft threshold's gradient jumps at +-lam, and fp32 cannot resolve the pre-threshold values closest to it, so the reference takes the
kernel's recorded decisions inside the band | |Yp| - lam | < 1e-5 and float64's own outside; each comparison asserts that the kernel
agrees with float64 everywhere outside the band and that the band holds at most 0.5 % of the values (afno_grad_ref.Restated).  Errors are
relative to each gradient's own norm, under the project's fp32 bar 1e-5 with max < 2 x bar, as test_hip_afno.close applies it."""
import pytest
import torch

import afno_grad_ref as G
from test_hip_afno import close

pytestmark = pytest.mark.gpu

LAM = 0.01


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def check_masks(rs, n_calls):
    assert rs.i == n_calls == len(rs.records)
    print(f"threshold decisions: {rs.outside_mismatch} differ outside the band, {rs.flipped} inside; band shares {['%.2e' % s for s in rs.shares]}")
    assert rs.outside_mismatch == 0
    assert max(rs.shares) <= G.BAND_SHARE


@pytest.mark.parametrize("B,H,W,C,bs", G.FILTER_CASES)
def test_filter_node_alone(dev, B, H, W, C, bs):
    """AfnoFilterFn: forward bit-identical to afno.afno_filter; dx, dW1, dW2 against float64 with restated masks, dresidual = dout exactly;
    the same bits under autocast(bf16) and on a second run; accumulation into an existing gradient slot."""
    import tante_amd.afno as A
    x, res, w1, w2, dout = G.filter_case(B, H, W, C, bs)
    xd, rd = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    p1, p2 = torch.nn.Parameter(w1.to(dev)), torch.nn.Parameter(w2.to(dev))
    g = dout.to(dev)

    def run():
        y = A.AfnoFilterFn.apply(xd, rd, p1, p2, bs, LAM)
        return y, torch.autograd.grad(y, [xd, rd, p1, p2], g)

    sink = []
    with A.record_keep_masks(sink):
        y, grads = run()
    assert len(sink) == 1 and tuple(sink[0].shape) == (B, *A.kept_modes(H, W), 2, C) and sink[0].dtype == torch.uint8
    assert torch.equal(y.detach(), A.afno_filter(xd.detach(), rd.detach(), A.pack_block_weight(p1), A.pack_block_weight(p2), bs, LAM))
    assert torch.equal(grads[1], g)
    y2, grads2 = run()                                   # nothing recorded outside the scope, the same bits
    assert len(sink) == 1 and torch.equal(y2, y) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y3, grads3 = run()
    assert y3.dtype == torch.float32 and torch.equal(y3, y) and all(torch.equal(a, b) for a, b in zip(grads, grads3))
    # an existing .grad is the slot the kernel adds into
    fill = [torch.randn(p.shape, generator=torch.Generator().manual_seed(5 + i)).to(dev) for i, p in enumerate((p1, p2))]
    p1.grad, p2.grad = fill[0].clone(), fill[1].clone()
    A.AfnoFilterFn.apply(xd.detach(), rd.detach(), p1, p2, bs, LAM).backward(g)
    assert torch.equal(p1.grad, fill[0] + grads[2]) and torch.equal(p2.grad, fill[1] + grads[3])
    # float64 with the decisions restated
    rs = G.Restated(sink, LAM)
    leaves = [t.detach().to(G.DT).clone().requires_grad_(True) for t in (x, res, w1, w2)]
    want_y = G.afno_filter(leaves[0], leaves[2], leaves[3], LAM, rs).transpose(1, 2) + leaves[1]
    want = torch.autograd.grad(want_y, leaves, dout.to(G.DT))
    check_masks(rs, 1)
    note = f"filter node {H}x{W} C {C} block {bs} B {B}"
    close(y - rd.detach(), want_y.detach() - leaves[1].detach(), "fp32", f"{note}: forward")
    for name, a, b in zip(("dx", "dresidual", "dW1", "dW2"), grads, want):
        close(a, b, "fp32", f"{note}: {name}")


def on_device(dev):
    m, sd, x = G.model_case()
    return m.to(dev).eval().set_compute("fp32").set_trainable(), sd, x


def test_one_block_fp32(dev):
    """Block.forward under grad after set_trainable: output, input gradient and every parameter gradient against float64."""
    import tante_amd.afno as A
    m, sd, _ = on_device(dev)
    blk = m.blocks[1]
    gen = torch.Generator().manual_seed(31)
    x, gy = torch.randn(2, 4, 6, 32, generator=gen), torch.randn(2, 4, 6, 32, generator=gen)
    xd = x.to(dev).requires_grad_(True)
    names = [k for k, _ in blk.named_parameters()]
    sink = []
    with A.record_keep_masks(sink):
        y = blk(xd)
        grads = torch.autograd.grad(y, [xd] + [p for _, p in blk.named_parameters()], gy.to(dev))
    rs = G.Restated(sink, LAM)
    sd64 = G.leaves({k: v for k, v in sd.items() if k.startswith("blocks.1.")})
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = G.block(x64, sd64, "blocks.1.", LAM, rs)
    want = torch.autograd.grad(want_y, [x64] + [sd64["blocks.1." + k] for k in names], gy.to(G.DT))
    check_masks(rs, 1)
    close(y, want_y, "fp32", "block: forward")
    for name, a, b in zip(["dx"] + names, grads, want):
        close(a, b, "fp32", f"block: {name}")


def test_model_fp32(dev):
    """The whole model under grad: the input gradient and every parameter gradient against float64 autograd of afno_ref.model's arithmetic,
    the masks of the two block calls restated in call order."""
    import tante_amd.afno as A
    m, sd, x = on_device(dev)
    gy = torch.randn(G.MODEL_B, 1, G.MODEL_FIELDS, *G.MODEL_RES, generator=torch.Generator().manual_seed(32))
    xd = x.to(dev).requires_grad_(True)
    names = [k for k, _ in m.named_parameters()]
    with torch.no_grad():
        y_inf = m(xd.detach())
    sink = []
    with A.record_keep_masks(sink):
        y = m(xd)
        grads = torch.autograd.grad(y, [xd] + [p for _, p in m.named_parameters()], gy.to(dev))
    assert tuple(y.shape) == tuple(y_inf.shape)
    rs = G.Restated(reversed(sink), LAM)                 # recorded in backward order
    sd64 = G.leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = G.model(x64, sd64, G.MODEL_KW["patch_size"], LAM, rs)
    want = torch.autograd.grad(want_y, [x64] + [sd64[k] for k in names], gy.to(G.DT))
    check_masks(rs, 2)
    close(y_inf, want_y, "fp32", "model: inference forward")
    close(y, want_y, "fp32", "model: training forward")
    for name, a, b in zip(["dx"] + names, grads, want):
        close(a, b, "fp32", f"model: {name}")


def rollout_batch(x, dev, n_steps):
    import tante_amd
    ref = torch.randn(G.MODEL_B, n_steps, *G.MODEL_RES, G.MODEL_FIELDS, generator=torch.Generator().manual_seed(33))
    batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous().to(dev), "output": ref.to(dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(tante_amd.TanteMetadata(n_fields=G.MODEL_FIELDS, spatial_resolution=G.MODEL_RES))
    return batch, fmt, ref


def test_bptt_through_a_refed_rollout(dev):
    """rollout_model under grad, 2 re-fed steps: the parameter gradients of a weighted sum of both predicted frames against the float64
    re-fed restatement, the four block calls' masks restated in call order."""
    import tante_amd
    import tante_amd.afno as A
    m, sd, x = on_device(dev)
    batch, fmt, gy = rollout_batch(x, dev, 2)
    names = [k for k, _ in m.named_parameters()]
    sink = []
    with A.record_keep_masks(sink):
        y, _ = tante_amd.rollout_model(m, batch, fmt, 2)
        grads = torch.autograd.grad(y, [p for _, p in m.named_parameters()], gy.to(dev))
    assert tuple(y.shape) == (G.MODEL_B, 2, *G.MODEL_RES, G.MODEL_FIELDS)
    rs = G.Restated(reversed(sink), LAM)
    sd64 = G.leaves(sd)
    want_y = G.rollout(x.to(G.DT), sd64, G.MODEL_KW["patch_size"], 2, LAM, rs).permute(0, 1, 3, 4, 2)
    want = torch.autograd.grad(want_y, [sd64[k] for k in names], gy.to(G.DT))
    check_masks(rs, 4)
    close(y, want_y, "fp32", "rollout: both frames")
    for name, a, b in zip(names, grads, want):
        close(a, b, "fp32", f"rollout: {name}")


def test_train_steps_bf16(dev):
    """train_step with FlatAdamW, 20 steps on one fixed batch in bf16 compute: finite losses, the last below the first, every parameter
    (the two filter weights of each block included) moved."""
    import tante_amd
    m, _, x = on_device(dev)
    m.set_compute("bf16").train()
    batch, fmt, _ = rollout_batch(x, dev, 2)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-3)
    losses = [float(tante_amd.train_step(m, opt, batch, fmt, 2)) for _ in range(20)]
    print("losses", ["%.4f" % v for v in losses])
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert losses[-1] < losses[0]
    still = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, still
    assert sum(".cmlp." in k for k in before) == 4


def test_training_forward_follows_the_optimiser(dev):
    """FlatAdamW updates the parameters through raw pointers (neither their address nor their version moves): after its steps the node must
    run the NEW filter weights -- bit-identical to afno_filter on freshly packed ones, and different from before the steps -- and the
    opted-in forward under grad must agree with the no_grad inference forward of the same model under the fp32 bar."""
    import tante_amd
    import tante_amd.afno as A
    m, _, x = on_device(dev)
    batch, fmt, _ = rollout_batch(x, dev, 1)
    f = m.blocks[0].filter
    bs = f.hidden_size // f.cmlp_diagonal_blocks
    t = torch.randn(2, 4, 6, 32, generator=torch.Generator().manual_seed(41)).to(dev)

    def node():
        return A.AfnoFilterFn.apply(t, None, f.cmlp[0].weight, f.cmlp[2].weight, bs, LAM).detach()

    y0 = node()
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-2)
    for _ in range(2):
        tante_amd.train_step(m, opt, batch, fmt, 1)
    y1 = node()
    assert torch.equal(y1, A.afno_filter(t, None, A.pack_block_weight(f.cmlp[0].weight), A.pack_block_weight(f.cmlp[2].weight), bs, LAM))
    assert not torch.equal(y1, y0)
    xd = x.to(dev)
    y_train = m(xd)
    assert y_train.requires_grad
    with torch.no_grad():
        y_inf = m(xd)
    close(y_train, y_inf, "fp32", "after two optimiser steps: training forward vs inference forward")


def test_refusals(dev):
    """Without the opt-in the pinned refusal; with it, dropout in train() still refuses; set_trainable(False) restores the refusal."""
    import tante_amd
    m, _, x = on_device(dev)
    xd = x.to(dev)
    plain = G.model_case()[0].to(dev)
    for mod in (plain.train(), plain.eval()):
        with pytest.raises(NotImplementedError, match="training is out of scope"):
            mod(xd)
    assert m(xd).requires_grad
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.set_trainable(False)(xd)
    with torch.no_grad():
        assert not m(xd).requires_grad
    md = tante_amd.TanteMetadata(n_fields=G.MODEL_FIELDS, spatial_resolution=G.MODEL_RES)
    for kw in (dict(drop_rate=0.1), dict(drop_path_rate=0.1)):
        d = tante_amd.AFNO(dset_metadata=md, **G.MODEL_KW, **kw).to(dev).set_trainable()
        with pytest.raises(NotImplementedError, match="drop_rate / drop_path_rate"):
            d.train()(xd)
        assert tuple(d.eval()(xd).shape) == (G.MODEL_B, 1, G.MODEL_FIELDS, *G.MODEL_RES)
