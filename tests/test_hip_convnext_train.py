"""GPU: training the UNetConvNext baseline behind set_trainable() -- the two new autograd nodes alone, one Block, the resamples and the skip
stage, the whole model (the g21 fixtures and the default constructor's widths), BPTT through a re-fed rollout, an optimiser loop and the
refusals; every gradient against float64 autograd of tests/convnext_ref.py.  Errors are relative to each gradient's own norm, under the
project's fp32 bar 1e-5 with max < 2 x bar, as test_hip_convnext.close applies it; a block's input gradient is compared without the
skip's share (dx - dout), which tests/test_convnext_train_cpu.py holds to at least MIN_RATIO of dout."""
import pytest
import torch

import convnext_grad_ref as G
import convnext_ref as R
from conftest import max_rel, rel_err
from test_convnext_cpu import BLOCKS, MODELS, keyed_golden
from test_hip_convnext import TOL, close

pytestmark = pytest.mark.gpu

MODULES = {"g21_convnext_down_c15": lambda CN: CN.Downsample(15, 30, 2), "g21_convnext_up_c30": lambda CN: CN.Upsample(30, 15, 2),
           "g21_convnext_stage_skip_c30": lambda CN: CN.Stage(30, 15, 2, depth=1, mode="up", skip_project=True)}
ROLL = "g21_convnext_model_f8_s3_16x24"        # the smaller model fixture


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- DwConvLnFn alone -----------------------------------------------------------------------------------------------------------------------
def dwln_run(dev, args, dy_dtype, batch=None):
    """-> (y, grads) of the node on the device; `batch`: image i alone."""
    import tante_amd.convnext as CN
    x, w, b, gw, gb, dy = args
    n, H, W, C = x.shape
    if batch is not None:
        x, dy = x[batch:batch + 1], dy.view(n, H * W, C)[batch].reshape(H * W, C)
    xd = x.contiguous().to(dev).requires_grad_(True)
    ps = [None if t is None else torch.nn.Parameter(t.to(dev)) for t in (w, b, gw, gb)]
    y = CN.DwConvLnFn.apply(xd, *ps, G.EPS, dy_dtype)
    return xd, ps, y, torch.autograd.grad(y, [xd] + [p for p in ps if p is not None], dy.contiguous().to(dev))


@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16], ids=["dy32", "dy16"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("case", G.DWLN_CASES, ids=lambda c: "n%d-C%d-%dx%d" % c)
def test_dwconv_ln_node_alone(dev, case, affine, dy_dtype):
    """Forward bit-identical to convnext.dwconv_ln; dx, d_taps, d_dwbias, d_ln_w, d_ln_b against float64 autograd of the dy as rounded; the
    same bits on a second run; accumulation into pre-filled gradient slots; image i of the batch gives the bits of the image alone.
    (2, 16, 136, 136) and (1, 1024, 24, 48) were chosen against the cap of 512 walking workgroups (512 / 32 chunks = 16 walkers at 1024
    channels): there a workgroup of launch B (and of launch A) walks two tiles."""
    import tante_amd.convnext as CN
    args, want = G.dwln_want(case, affine, dy_dtype == torch.bfloat16)
    x, w, b, gw, gb, dy = args
    n, C, H, W = case
    xd, ps, y, grads = dwln_run(dev, args, dy_dtype)
    assert y.dtype == dy_dtype and all(g.dtype == torch.float32 for g in grads)
    assert torch.equal(y.detach(), CN.dwconv_ln(xd.detach(), ps[0].detach().reshape(C, 49), ps[1].detach(), G.EPS,
                                                None if gw is None else ps[2].detach(), None if gb is None else ps[3].detach(), dy_dtype))
    _, _, y2, grads2 = dwln_run(dev, args, dy_dtype)
    assert torch.equal(y2, y) and all(torch.equal(a, c) for a, c in zip(grads, grads2))
    note = f"dwconv_ln node n {n} C {C} {H} x {W} {'affine' if affine else 'plain'} dy {str(dy_dtype)[6:]}"
    names = ["dx", "d_taps", "d_dwbias"] + (["d_ln_w", "d_ln_b"] if affine else [])
    for k, a, c in zip(names, grads, want[1:]):
        close(a, c.reshape(a.shape), "fp32", f"{note}: {k}")
    # existing .grads are the slots the kernel adds into (all four exist: with the affine)
    if affine:
        live = [p for p in ps if p is not None]
        fill = [torch.randn(p.shape, generator=torch.Generator().manual_seed(5 + i)).to(dev) for i, p in enumerate(live)]
        for p, f in zip(live, fill):
            p.grad = f.clone()
        CN.DwConvLnFn.apply(xd.detach(), *ps, G.EPS, dy_dtype).backward(dy.to(dev))
        for p, f, gr in zip(live, fill, grads[1:]):
            assert torch.equal(p.grad, f + gr)
    if n == 2:
        for i in range(2):
            assert torch.equal(grads[0][i:i + 1], dwln_run(dev, args, dy_dtype, batch=i)[3][0]), i


def test_dwconv_ln_node_refuses_1025_channels(dev):
    import tante_amd.convnext as CN
    x = torch.zeros(1, 4, 4, 1025, device=dev, requires_grad=True)
    p = [torch.zeros(1025, 1, 7, 7, device=dev), torch.zeros(1025, device=dev)]
    with pytest.raises(RuntimeError, match="tante_dwconv_ln: channels outside 1..1024"):
        CN.DwConvLnFn.apply(x, *p, None, None, G.EPS, torch.float32)
    with pytest.raises(RuntimeError, match="tante_dwconv_ln_bwd: channels outside 1..1024"):
        CN.dwconv_ln_bwd(torch.zeros(16, 1025, device=dev), x.detach(), p[0].reshape(1025, 49), p[1], G.EPS)


def test_dwconv_ln_node_on_an_offset_input(dev):
    """x = 30 + randn with window weights that sum to one: the forward sits at half the fp32 bar here, so this case has a bar of its own --
    twice the error of torch's fp32 autograd of F.layer_norm on the float64 conv sum (the reference's arithmetic; the margin of 2 allows
    for the 49-term fp32 sum that figure does not carry).  The statistics are ln_stage's, mean first and then the centred squares:
    E[u^2] - mean^2 in fp32 loses its digits at this input (test_hip_convnext.test_dwconv_ln_on_an_offset_input), and rstd enters du."""
    import torch.nn.functional as F
    case = (2, 48, 9, 20)
    args, want = G.dwln_want(case, True, False, G.IN_OFFSET)
    x, w, b, gw, gb, dy = args
    x64 = x.double().requires_grad_(True)
    z = R.dwconv7(x64, w, b)                                  # the float64 conv sum; the norm and its backward in torch's fp32
    F.layer_norm(z.float(), (48,), gw, gb, G.EPS).backward(dy.reshape(z.shape))
    own = rel_err(x64.grad, want[1])
    _, _, _, grads = dwln_run(dev, args, torch.float32)
    got = rel_err(grads[0].cpu().double(), want[1])
    print(f"offset {G.IN_OFFSET}: dx of torch's fp32 layer_norm on the float64 conv sum rel {own:.3e}; the kernel's dx rel {got:.3e} "
          f"max {max_rel(grads[0].cpu().double(), want[1]):.3e}")
    assert torch.isfinite(grads[0]).all() and own > 0
    assert got <= 2 * own, (got, own)


# ---- L2NormRowsFn alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16], ids=["dy32", "dy16"])
@pytest.mark.parametrize("C", G.L2_CASES)
def test_l2norm_node_alone(dev, C, dy_dtype):
    import tante_amd.convnext as CN
    x, dy = G.l2_case(C)
    dy = dy.to(dy_dtype)
    xd = x.to(dev).requires_grad_(True)

    def run():
        y = CN.L2NormRowsFn.apply(xd, G.EPS, dy_dtype)
        return y, torch.autograd.grad(y, xd, dy.to(dev))[0]

    y, dx = run()
    assert y.dtype == dy_dtype and dx.dtype == torch.float32 and torch.equal(y.detach(), CN.l2norm_rows(xd.detach(), G.EPS, dy_dtype))
    y2, dx2 = run()
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    _, want = G.l2_autograd(x, dy.float())
    close(dx, want, "fp32", f"l2norm node C {C} dy {str(dy_dtype)[6:]}")
    eps32 = torch.full((C,), G.EPS, dtype=torch.float32)
    for row in (2, 4):                                        # the zero row and the row below eps: dy / eps exactly
        assert torch.equal(dx[row].cpu(), dy[row].float() / eps32), row


# ---- one block ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_one_block_fp32(dev, name):
    """Block.forward under grad after set_trainable: the output, dx - dout and every parameter gradient, gamma included."""
    import tante_amd.convnext as CN
    sd, x, gy = G.block_fixture(name)
    blk = CN.Block(BLOCKS[name][0], 2).eval()
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev).set_trainable()
    xd = x.to(dev).requires_grad_(True)
    names = [k for k, _ in blk.named_parameters()]
    assert "gamma" in names
    y = blk(xd)
    grads = torch.autograd.grad(y, [xd] + [p for _, p in blk.named_parameters()], gy.to(dev))
    sd64 = G.sd_leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = R.block(x64.permute(0, 2, 3, 1), sd64).permute(0, 3, 1, 2)
    want = torch.autograd.grad(want_y, [x64] + [sd64[k] for k in names], gy.to(G.DT))
    close(y, want_y, "fp32", f"{name}: forward")
    close(grads[0].cpu().double() - gy.double(), want[0] - gy.double(), "fp32", f"{name}: dx - dout")
    for k, a, b in zip(names, grads[1:], want[1:]):
        close(a, b.reshape(a.shape), "fp32", f"{name}: {k}")


# ---- resamples and the skip stage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULES))
def test_resamples_and_skip_stage_fp32(dev, name):
    """The three g21 module fixtures called alone after set_trainable: outputs and all gradients; the channels-first bias gets None."""
    import tante_amd.convnext as CN
    g, sd, _ = keyed_golden(name)
    m = MODULES[name](CN).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).set_trainable()
    x = g["x"].float()
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(34))
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [xd] + [p for _, p in m.named_parameters()], gy.to(dev), allow_unused=True)
    sd64 = G.sd_leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    xl = x64.permute(0, 2, 3, 1)
    if name.endswith("down_c15"):
        want_y = R.downsample(xl, sd64)
    elif name.endswith("up_c30"):
        want_y = R.upsample(xl, sd64)
    else:
        want_y = R.stage(xl[..., :30], sd64, "", 1, "up", xl[..., 30:])
    want_y = want_y.permute(0, 3, 1, 2)
    used = [k for k in names if not k.endswith("block.0.bias")]
    assert len(used) == len(names) - 1
    want = dict(zip(["dx"] + used, torch.autograd.grad(want_y, [x64] + [sd64[k] for k in used], gy.to(G.DT))))
    close(y, want_y, "fp32", f"{name}: forward")
    close(y, g["y64"], "fp32", f"{name}: forward against the fixture")
    for k, a in zip(["dx"] + names, grads):
        if k.endswith("block.0.bias"):
            assert a is None, k
        else:
            close(a, want[k].reshape(a.shape), "fp32", f"{name}: {k}")


# ---- the whole model ----------------------------------------------------------------------------------------------------------------------
def on_device(name, dev, mode="fp32"):
    m, sd, x = G.default_model() if name == "default" else G.fixture_model(name)
    return m.to(dev).eval().set_compute(mode).set_trainable(), sd, x


@pytest.mark.parametrize("name", sorted(MODELS) + ["default"])
def test_model_fp32(dev, name):
    """Both model fixtures, and the default constructor on 16 x 16 (512 channels at the neck, K chunks past 512, the chunked deconv
    branch): the inference and the training forward, the input gradient and every trained parameter's gradient against float64; the
    channels-first biases receive none."""
    m, sd, x = on_device(name, dev)
    names = [k for k, _ in m.named_parameters()]
    xd = x.to(dev).requires_grad_(True)
    with torch.no_grad():
        y_inf = m(xd.detach())
    y = m(xd)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(32))
    grads = torch.autograd.grad(y, [xd] + [p for _, p in m.named_parameters()], gy.to(dev), allow_unused=True)
    assert tuple(y.shape) == tuple(y_inf.shape) and not y_inf.requires_grad and y.requires_grad
    sd64 = G.sd_leaves(sd)
    x64 = x.to(G.DT).requires_grad_(True)
    want_y = R.model(x64, sd64)
    trained = G.trained_names(m)
    assert len(names) - len(trained) == 2 * m.stages
    assert {id(p) for p in m.trained_parameters()} == {id(p) for k, p in m.named_parameters() if k in trained}
    want = dict(zip(["dx"] + trained, torch.autograd.grad(want_y, [x64] + [sd64[k] for k in trained], gy.to(G.DT))))
    close(y_inf, want_y, "fp32", f"{name} model: inference forward")
    close(y, want_y, "fp32", f"{name} model: training forward")
    for k, a in zip(["dx"] + names, grads):
        if G.untrained(k):
            assert a is None, k
        else:
            close(a, want[k].reshape(a.shape), "fp32", f"{name} model: {k}")


def rollout_batch(x, dev, n_steps):
    import tante_amd
    b, _, c, h, w = x.shape
    ref = torch.randn(b, n_steps, h, w, c, generator=torch.Generator().manual_seed(33))
    batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous().to(dev), "output": ref.to(dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(tante_amd.TanteMetadata(n_fields=c, spatial_resolution=(h, w)))
    return batch, fmt, ref


def test_bptt_through_a_refed_rollout(dev):
    """rollout_model under grad, 3 steps on the smaller model fixture: the trained parameters' gradients of a weighted sum of the three
    frames against the float64 re-fed restatement."""
    import tante_amd
    m, sd, x = on_device(ROLL, dev)
    batch, fmt, gy = rollout_batch(x, dev, 3)
    trained = G.trained_names(m)
    y, _ = tante_amd.rollout_model(m, batch, fmt, 3)
    grads = torch.autograd.grad(y, m.trained_parameters(), gy.to(dev))
    assert tuple(y.shape) == tuple(gy.shape)
    sd64 = G.sd_leaves(sd)
    want_y = G.rollout(x, sd64, 3).permute(0, 1, 3, 4, 2)
    want = torch.autograd.grad(want_y, [sd64[k] for k in trained], gy.to(G.DT))
    close(y, want_y, "fp32", "rollout: three frames")
    for k, a, b in zip(trained, grads, want):
        close(a, b.reshape(a.shape), "fp32", f"rollout: {k}")


def test_optimiser_loop_bf16(dev):
    """20 train_steps with FlatAdamW(model.trained_parameters()) on one fixed batch in bf16 compute: finite losses, the last below the
    first, every trained parameter moved, the channels-first biases bit-identical; afterwards, in fp32 compute, the training forward
    agrees with the inference forward on the updated weights (no stale pack or fold)."""
    import tante_amd
    m, _, x = on_device(ROLL, dev, "bf16")
    m.train()
    batch, fmt, _ = rollout_batch(x, dev, 2)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    with torch.no_grad():
        y_old = m.set_compute("fp32")(x.to(dev))
        m.set_compute("bf16")
    opt = tante_amd.FlatAdamW(m.trained_parameters(), lr=1e-3)
    losses = [float(tante_amd.train_step(m, opt, batch, fmt, 2)) for _ in range(20)]
    print("losses", ["%.4f" % v for v in losses])
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert losses[-1] < losses[0]
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) == G.untrained(k), k
    m.set_compute("fp32")
    xd = x.to(dev)
    y_train = m(xd)
    assert y_train.requires_grad
    with torch.no_grad():
        y_inf = m(xd)
    assert not torch.equal(y_inf, y_old)
    close(y_train, y_inf, "fp32", "after 20 optimiser steps: training forward vs inference forward")


def test_refusals(dev):
    """A plain model and set_trainable(False) refuse word for word; no_grad on an opted-in model takes inference bit for bit, in train()
    too; 3-D metadata and drop_path > 0 refuse as before."""
    import types

    import tante_amd
    import tante_amd.convnext as CN
    m, _, x = on_device(ROLL, dev)
    xd = x.to(dev)
    plain = G.fixture_model(ROLL)[0].to(dev)
    text = ("tante_amd.UNetConvNext is inference only: training is out of scope (the backward of the fused block is a kernel of its own that "
            "is not built); call .eval() under torch.no_grad()")
    for mod in (plain.train(), plain.eval()):
        with pytest.raises(NotImplementedError) as e:
            mod(xd)
        assert str(e.value) == text
    assert m(xd).requires_grad and m.train()(xd).requires_grad
    with torch.no_grad():
        y_inf = m(xd)
        assert not y_inf.requires_grad and torch.equal(y_inf, m.eval()(xd)) and torch.equal(y_inf, plain.eval()(xd))
    with pytest.raises(NotImplementedError) as e:
        m.set_trainable(False)(xd)
    assert str(e.value) == text
    with pytest.raises(NotImplementedError, match="n_spatial_dims = 3"):
        tante_amd.UNetConvNext(4, types.SimpleNamespace(n_fields=3, n_spatial_dims=3))
    with pytest.raises(NotImplementedError, match="drop_path"):
        CN.Block(8, 2, drop_path=0.1)
    m.set_trainable()
    with pytest.raises(NotImplementedError, match="channels_first"):
        m.encoder[0].resample.block[0](xd)
