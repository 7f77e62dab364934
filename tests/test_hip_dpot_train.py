"""GPU: training the DPOT baseline behind set_trainable() -- the filter's and GroupNorm's autograd nodes alone, one Block, the whole model
(the g19 fixtures' configurations and a wide one), BPTT through a re-fed rollout, an optimiser loop and the refusals; every gradient
against float64 autograd of tests/dpot_ref.py.  Errors are relative to each gradient's own norm, under the project's fp32 bar 1e-5 with
max < 2 x bar, as test_hip_dpot.close applies it; the filter's input gradient is compared without the skip's share (dx - dout), which
tests/test_dpot_train_cpu.py holds to at least MIN_RATIO of dout for every case."""
import pytest
import torch

import dpot_grad_ref as G
import dpot_ref as R
from test_dpot_cpu import BLOCKS, MODELS, keyed_golden
from test_hip_dpot import GN_OFFSET, close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- the filter node alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,nb,modes", G.FILTER_CASES)
def test_filter_node_alone(dev, B, H, W, C, nb, modes):
    """DpotFilterFn: forward bit-identical to dpot.dpot_filter; dx - dout, dw1, db1, dw2, db2 against float64, dresidual = dout exactly; the
    same bits on a second run and under autocast(bf16); accumulation into existing gradient slots."""
    import tante_amd.dpot as D
    x, res, ws, dout = G.filter_case(B, H, W, C, nb, modes)
    xd, rd = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    ps = [torch.nn.Parameter(t.to(dev)) for t in ws]
    g = dout.to(dev)

    def run():
        y = D.DpotFilterFn.apply(xd, rd, *ps, modes)
        return y, torch.autograd.grad(y, [xd, rd, *ps], g)

    y, grads = run()
    assert torch.equal(y.detach(), D.dpot_filter(xd.detach(), rd.detach(), *(p.detach() for p in ps), modes))
    assert torch.equal(grads[1], g)
    y2, grads2 = run()
    assert torch.equal(y2, y) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y3, grads3 = run()
    assert y3.dtype == torch.float32 and torch.equal(y3, y) and all(torch.equal(a, b) for a, b in zip(grads, grads3))
    # existing .grads are the slots the kernel adds into
    fill = [torch.randn(p.shape, generator=torch.Generator().manual_seed(5 + i)).to(dev) for i, p in enumerate(ps)]
    for p, f in zip(ps, fill):
        p.grad = f.clone()
    D.DpotFilterFn.apply(xd.detach(), rd.detach(), *ps, modes).backward(g)
    for p, f, gr in zip(ps, fill, grads[2:]):
        assert torch.equal(p.grad, f + gr)
    want = G.filter_autograd(x, ws, dout, modes)
    note = f"filter node {H}x{W} C {C} blocks {nb} modes {modes} B {B}"
    close(y.detach().cpu().double() - x.double() - res.double(), want[0], "fp32", f"{note}: forward contribution")
    close(grads[0].cpu().double() - dout.double(), want[1], "fp32", f"{note}: dx - dout")
    for name, a, b in zip(("dw1", "db1", "dw2", "db2"), grads[2:], want[2:]):
        close(a, b, "fp32", f"{note}: {name}")


# ---- the GroupNorm node alone ---------------------------------------------------------------------------------------------------------------
def gn_check(dev, B, HW, C, offset, dy_dtype, affine):
    import tante_amd.dpot as D
    x, w, b, dy = G.gn_case(B, HW, C, offset, affine)
    dy = dy.to(dy_dtype)
    xd = x.to(dev).requires_grad_(True)
    ps = [torch.nn.Parameter(t.to(dev)) for t in (w, b)] if affine else [None, None]
    wanted = [xd] + (ps if affine else [])

    def run():
        y = D.GroupNormFn.apply(xd, ps[0], ps[1], G.GROUPS, 1e-5, dy_dtype)
        return y, torch.autograd.grad(y, wanted, dy.to(dev))

    y, grads = run()
    assert y.dtype == dy_dtype and grads[0].dtype == torch.float32
    assert torch.equal(y.detach(), D.groupnorm(xd.detach(), G.GROUPS, *(None if p is None else p.detach() for p in ps), 1e-5, dy_dtype))
    y2, grads2 = run()
    assert torch.equal(y2, y) and all(torch.equal(a, c) for a, c in zip(grads, grads2))
    want = G.gn_autograd(x, w, b, dy.float())                 # of the gradient the node received: the bf16 one as rounded
    note = f"groupnorm node ({B}, {HW}, {C}) offset {offset} dy {str(dy_dtype)[6:]}{'' if affine else ' without affine'}"
    close(grads[0], want[1], "fp32", f"{note}: dx")
    if affine:
        close(grads[1], want[2], "fp32", f"{note}: dgamma")
        close(grads[2], want[3], "fp32", f"{note}: dbeta")
        fill = [torch.randn(C, generator=torch.Generator().manual_seed(9 + i)).to(dev) for i in range(2)]
        ps[0].grad, ps[1].grad = fill[0].clone(), fill[1].clone()
        D.GroupNormFn.apply(xd.detach(), ps[0], ps[1], G.GROUPS, 1e-5, dy_dtype).backward(dy.to(dev))
        assert torch.equal(ps[0].grad, fill[0] + grads[1]) and torch.equal(ps[1].grad, fill[1] + grads[2])


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,HW,C", G.GN_CASES)
def test_groupnorm_node_alone(dev, B, HW, C, dy_dtype, affine):
    """One token; C/G = 6 on an odd token count; the shipped width in several slabs; the token limit: forward bit-identical to
    dpot.groupnorm, dx / dgamma / dbeta against float64, the same bits on two runs, accumulation into the slots."""
    gn_check(dev, B, HW, C, 0.0, dy_dtype, affine)


def test_groupnorm_node_on_an_offset_input(dev):
    """x = 30 + randn: statistics by E[x^2] - mean^2 in fp32 would miss the bar here (see test_hip_dpot.GN_OFFSET)."""
    gn_check(dev, 2, 64, 1536, GN_OFFSET, torch.float32, True)


# ---- one block ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_one_block_fp32(dev, name):
    """Block.forward under grad after set_trainable, both double_skip values: output, input gradient and every parameter gradient."""
    import tante_amd.dpot as D
    g, sd, _ = keyed_golden(name)
    blk = D.Block(width=64, n_blocks=2, mlp_ratio=2.0, channel_first=True, modes=int(g["modes"]), double_skip=BLOCKS[name])
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).eval().set_trainable()
    x = g["x"].float()
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(31))
    xd = x.to(dev).requires_grad_(True)
    names = [k for k, _ in blk.named_parameters()]
    y = blk(xd)
    grads = torch.autograd.grad(y, [xd] + [p for _, p in blk.named_parameters()], gy.to(dev))
    sd64 = G.sd_leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = R.block(x64.permute(0, 2, 3, 1), sd64, "", int(g["modes"]), BLOCKS[name]).permute(0, 3, 1, 2)
    want = torch.autograd.grad(want_y, [x64] + [sd64[k] for k in names], gy.to(G.DT))
    close(y, want_y, "fp32", f"{name}: forward")
    for k, a, b in zip(["dx"] + names, grads, want):
        close(a, b.reshape(a.shape), "fp32", f"{name}: {k}")


def test_modules_alone_under_grad(dev):
    """AFNO2D (channels last), TimeAggregator ('exp_mlp', gamma up to 2^10) and PatchEmbed called alone after set_trainable: outputs and
    every gradient against float64."""
    import tante_amd.dpot as D
    B, H, W, C, nb, modes = G.FILTER_CASES[0]
    x, _, ws, dout = G.filter_case(B, H, W, C, nb, modes)
    f = D.AFNO2D(width=C, num_blocks=nb, modes=modes)
    f.load_state_dict(dict(zip(("w1", "b1", "w2", "b2"), ws)), strict=True)
    f = f.to(dev).set_trainable()
    xd = x.to(dev).requires_grad_(True)
    y = f(xd)
    grads = torch.autograd.grad(y, [xd, f.w1, f.b1, f.w2, f.b2], dout.to(dev))
    want = G.filter_autograd(x, ws, dout, modes)
    close(y.detach().cpu().double() - x.double(), want[0], "fp32", "AFNO2D alone: contribution")
    close(grads[0].cpu().double() - dout.double(), want[1], "fp32", "AFNO2D alone: dx - dout")
    for k, a, b in zip(("dw1", "db1", "dw2", "db2"), grads[1:], want[2:]):
        close(a, b, "fp32", f"AFNO2D alone: {k}")

    gen = torch.Generator().manual_seed(51)
    T, Ct = 3, 16
    agg = D.TimeAggregator(Ct, T, Ct, "exp_mlp")
    assert float(agg.gamma.detach().max()) == 1024.0
    sd = {"time_agg_layer." + k: v.detach().clone() for k, v in agg.state_dict().items()}
    agg = agg.to(dev).set_trainable()
    xt, gt = torch.randn(2, 4, 5, T, Ct, generator=gen), torch.randn(2, 4, 5, Ct, generator=gen)
    xd = xt.to(dev).requires_grad_(True)
    y = agg(xd)
    grads = torch.autograd.grad(y, [xd, agg.w, agg.gamma], gt.to(dev))
    sd64, x64 = G.sd_leaves(sd), xt.to(G.DT).requires_grad_(True)
    want_y = torch.einsum("tij,bxyti->bxyj", R.time_weight(sd64, T, "exp_mlp"), x64)
    want = torch.autograd.grad(want_y, [x64, sd64["time_agg_layer.w"], sd64["time_agg_layer.gamma"]], gt.to(G.DT))
    close(y, want_y, "fp32", "TimeAggregator alone: forward")
    for k, a, b in zip(("dx", "dw", "dgamma"), grads, want):
        close(a, b, "fp32", f"TimeAggregator alone: {k}")

    pe = D.PatchEmbed(img_size=(8, 12), patch_size=4, in_chans=5, embed_dim=12, out_dim=16)
    sd = {k: v.detach().clone() for k, v in pe.state_dict().items()}
    pe = pe.to(dev).set_trainable()
    xi, gi = torch.randn(2, 5, 8, 12, generator=gen), torch.randn(2, 16, 2, 3, generator=gen)
    xd = xi.to(dev).requires_grad_(True)
    names = [k for k, _ in pe.named_parameters()]
    y = pe(xd)
    grads = torch.autograd.grad(y, [xd] + [p for _, p in pe.named_parameters()], gi.to(dev))
    sd64, x64 = G.sd_leaves(sd), xi.to(G.DT).requires_grad_(True)
    pt = x64.reshape(2, 5, 2, 4, 3, 4).permute(0, 2, 4, 1, 3, 5).reshape(2, 2, 3, -1)
    h = R.gelu(pt @ sd64["proj.0.weight"].reshape(12, -1).T + sd64["proj.0.bias"])
    want_y = (h @ sd64["proj.2.weight"].reshape(16, -1).T + sd64["proj.2.bias"]).permute(0, 3, 1, 2)
    want = torch.autograd.grad(want_y, [x64] + [sd64[k] for k in names], gi.to(G.DT))
    close(y, want_y, "fp32", "PatchEmbed alone: forward")
    for k, a, b in zip(["dx"] + names, grads, want):
        close(a, b.reshape(a.shape), "fp32", f"PatchEmbed alone: {k}")


# ---- the whole model ----------------------------------------------------------------------------------------------------------------------
def model_case(name):
    return G.wide_model() if name == "wide" else G.fixture_model(name)


def on_device(name, dev, mode="fp32"):
    m, sd, x, cfg = model_case(name)
    return m.to(dev).eval().set_compute(mode).set_trainable(), sd, x, cfg


@pytest.mark.parametrize("name", sorted(MODELS) + ["wide"])
def test_model_fp32(dev, name):
    """An 'exp_mlp' fixture, an 'mlp' one with out_timesteps = 2, and the wide model (embed 576: K chunks past 512, the chunked tap-GEMM
    deconv, a mixer block of 288): the inference and the training forward, the input gradient and every trained parameter's gradient
    against float64; cls_head receives none."""
    m, sd, x, cfg = on_device(name, dev)
    names = [k for k, _ in m.named_parameters()]
    xd = x.to(dev).requires_grad_(True)
    with torch.no_grad():
        y_inf = m(xd.detach())
    y = m(xd)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(32))
    grads = torch.autograd.grad(y, [xd] + [p for _, p in m.named_parameters()], gy.to(dev), allow_unused=True)
    assert tuple(y.shape) == tuple(y_inf.shape) and not y_inf.requires_grad
    sd64 = G.sd_leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = R.model(x64, sd64, cfg["patch"], cfg["modes"], cfg["time_agg"], cfg["out_timesteps"])
    trained = G.trained_names(m)
    assert [k for k in names if k not in trained] == [k for k in names if k.startswith("cls_head.")] and len(names) - len(trained) == 6
    assert {id(p) for p in m.trained_parameters()} == {id(p) for k, p in m.named_parameters() if k in trained}
    want = dict(zip(["dx"] + trained, torch.autograd.grad(want_y, [x64] + [sd64[k] for k in trained], gy.to(G.DT))))
    close(y_inf, want_y, "fp32", f"{name} model: inference forward")
    close(y, want_y, "fp32", f"{name} model: training forward")
    for k, a in zip(["dx"] + names, grads):
        if k.startswith("cls_head."):
            assert a is None, k
        else:
            close(a, want[k].reshape(a.shape), "fp32", f"{name} model: {k}")


def rollout_batch(x, dev, n_steps, res):
    import tante_amd
    ref = torch.randn(x.shape[0], n_steps, *res, x.shape[2], generator=torch.Generator().manual_seed(33))
    batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous().to(dev), "output": ref.to(dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(tante_amd.TanteMetadata(n_fields=x.shape[2], spatial_resolution=res))
    return batch, fmt, ref


ROLL = "g19_dpot_model_16x16_p2"       # out_timesteps = 2


def test_bptt_through_a_refed_rollout(dev):
    """rollout_model under grad, 3 steps at out_timesteps = 2 (two calls, the last frame dropped): the trained parameters' gradients of a
    weighted sum of the three frames against the float64 re-fed restatement."""
    import tante_amd
    m, sd, x, cfg = on_device(ROLL, dev)
    batch, fmt, gy = rollout_batch(x, dev, 3, cfg["res"])
    trained = G.trained_names(m)
    y, _ = tante_amd.rollout_model(m, batch, fmt, 3)
    grads = torch.autograd.grad(y, m.trained_parameters(), gy.to(dev))
    assert tuple(y.shape) == (x.shape[0], 3, *cfg["res"], x.shape[2])
    sd64 = G.sd_leaves(sd)
    want_y = R.rollout(x, sd64, cfg["patch"], cfg["modes"], cfg["time_agg"], cfg["out_timesteps"], 3).permute(0, 1, 3, 4, 2)
    want = torch.autograd.grad(want_y, [sd64[k] for k in trained], gy.to(G.DT))
    close(y, want_y, "fp32", "rollout: three frames")
    for k, a, b in zip(trained, grads, want):
        close(a, b.reshape(a.shape), "fp32", f"rollout: {k}")


def test_optimiser_loop_bf16(dev):
    """20 train_steps with FlatAdamW(model.trained_parameters()) on one fixed batch in bf16 compute: finite losses, the last below the
    first, every trained parameter moved, cls_head bit-identical; afterwards, in fp32 compute, the training forward agrees with the
    inference forward and the filter node equals dpot_filter on the updated weights (FlatAdamW moves neither a parameter's address nor
    its version: no stale fold or pack)."""
    import tante_amd
    import tante_amd.dpot as D
    m, _, x, cfg = on_device(ROLL, dev, "bf16")
    m.train()
    batch, fmt, _ = rollout_batch(x, dev, 2, cfg["res"])
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    f = m.blocks[0].filter
    t = torch.randn(2, 8, 8, 64, generator=torch.Generator().manual_seed(41)).to(dev)

    def node():
        return D.DpotFilterFn.apply(t, None, f.w1, f.b1, f.w2, f.b2, f.modes).detach()

    y0 = node()
    opt = tante_amd.FlatAdamW(m.trained_parameters(), lr=1e-3)
    losses = [float(tante_amd.train_step(m, opt, batch, fmt, 2)) for _ in range(20)]
    print("losses", ["%.4f" % v for v in losses])
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert losses[-1] < losses[0]
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) == k.startswith("cls_head."), k
    y1 = node()
    assert torch.equal(y1, D.dpot_filter(t, None, f.w1.detach(), f.b1.detach(), f.w2.detach(), f.b2.detach(), f.modes)) and not torch.equal(y1, y0)
    m.set_compute("fp32")
    xd = x.to(dev)
    y_train = m(xd)
    assert y_train.requires_grad
    with torch.no_grad():
        y_inf = m(xd)
    close(y_train, y_inf, "fp32", "after 20 optimiser steps: training forward vs inference forward")


def test_refusals(dev):
    """A plain model and set_trainable(False) refuse word for word; no_grad on an opted-in model takes inference, in train() too; the
    out-of-scope constructions refuse as before."""
    import tante_amd
    import tante_amd.dpot as D
    m, _, x, _ = on_device(ROLL, dev)
    xd = x.to(dev)
    plain = G.fixture_model(ROLL)[0].to(dev)
    for mod in (plain.train(), plain.eval()):
        with pytest.raises(NotImplementedError, match="training is out of scope"):
            mod(xd)
    assert m(xd).requires_grad and m.train()(xd).requires_grad
    with torch.no_grad():
        y_inf = m(xd)
        assert not y_inf.requires_grad and torch.equal(y_inf, m.eval()(xd)) and torch.equal(y_inf, plain.eval()(xd))
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.set_trainable(False)(xd)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16))
    kw = dict(in_T=2, patch_size=4, n_blocks=2, embed_dim=32, depth=1, modes=4)
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.DPOT(dset_metadata=tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(16, 16, 16), n_spatial_dims=3), **kw)
    with pytest.raises(NotImplementedError, match="act = 'silu'"):
        tante_amd.DPOT(dset_metadata=md, act="silu", **kw)
    with pytest.raises(NotImplementedError, match="mixing_type"):
        tante_amd.DPOT(dset_metadata=md, mixing_type="attn", **kw)
    with pytest.raises(NotImplementedError, match="hidden_size_factor = 2"):
        D.AFNO2D(width=32, num_blocks=2, hidden_size_factor=2)
    f = D.AFNO2D(width=64, num_blocks=2, modes=4).to(dev).set_trainable()
    with pytest.raises(RuntimeError, match="tante_dpot_filter: token grid outside 1..64"):
        f(torch.randn(1, 65, 8, 64, device=dev))
