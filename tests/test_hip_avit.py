"""GPU: the AViT baseline -- tante_instnorm, tante_axial_attention, tante_time_attention and the field statistics alone against float64,
the blocks, the stem, the head and the whole models against the reference's fixtures, a width-384 model and a re-fed rollout against the
float64 restatement, and the out-of-scope cases."""
import contextlib
import types

import pytest
import torch

import avit_ref as R
from conftest import max_rel, record_parity, rel_err
from test_avit_cpu import MODELS, SPATIAL, TEMPORAL, keyed_golden, model_kwargs

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}
IN_OFFSET = 30.0      # x = 30 + randn: torch's own fp32 norms stay under half the fp32 bar here (asserted below), a one-pass variance does not


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(a, b, mode, note="", bar=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    bar = TOL[mode] if bar is None else bar
    r, m = rel_err(a, b), max_rel(a, b)
    print(f"{note} [{mode}]: rel {r:.3e} max {m:.3e} (bar {bar:.1e})")
    record_parity(r, m, bar, mode, note)
    assert r < bar and m < 2 * bar, f"{note}: rel={r:.3e} max={m:.3e} (bar {bar:.1e})"
    return r


def mode_scope(mode):
    return torch.autocast("cuda", dtype=torch.bfloat16) if mode == "bf16" else contextlib.nullcontext()


# ---- the instance norms alone --------------------------------------------------------------------------------------------------------
IN_CASES = [(2, 2, 16), (2, 35, 48), (3, 256, 384), (1, 4096, 96)]
_IN = {}


def in_case(n, HW, C, offset=0.0):
    """x, weight, bias, residual, gamma and the float64 results of both forms, computed once per shape."""
    key = (n, HW, C, offset)
    if key not in _IN:
        gen = torch.Generator().manual_seed(n * 7 + HW * 3 + C)
        x = offset + torch.randn(n, HW, C, generator=gen)
        w, b = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
        res, gamma = torch.randn(n, HW, C, generator=gen), torch.randn(C, generator=gen)
        x4 = x.double().view(n, 1, HW, C)
        want = {"instance": R.inst_norm(x4, w, b).view(n, HW, C), "rms": R.rms_norm(x4, w).view(n, HW, C)}
        _IN[key] = (x, w, b, res, gamma, want)
    return _IN[key]


def run_instnorm(dev, x, w, b, form, out="fp32", res=None, gamma=None, in_place=False):
    import tante_amd.avit as A
    from tante_amd import _lib as L
    r = None if res is None else res.to(dev)
    return A.instnorm(x.to(dev), L.INSTNORM_RMS if form == "rms" else L.INSTNORM_INSTANCE, w.to(dev), b.to(dev), 1e-8 if form == "rms" else 1e-5,
                      torch.bfloat16 if out == "bf16" else torch.float32, residual=r, gamma=None if gamma is None else gamma.to(dev),
                      out=r if in_place else None)


@pytest.mark.parametrize("out", ["fp32", "bf16"])
@pytest.mark.parametrize("form", ["instance", "rms"])
@pytest.mark.parametrize("n,HW,C", IN_CASES)
def test_instnorm_against_float64(dev, n, HW, C, form, out):
    """Two tokens (the unbiased divisor is 1); an odd token count and a ragged channel strip; the shipped block shape; the token limit at
    the stem's width -- both forms, both output types, with and without the epilogue."""
    x, w, b, res, gamma, want = in_case(n, HW, C)
    y = run_instnorm(dev, x, w, b, form, out)
    assert y.dtype == (torch.bfloat16 if out == "bf16" else torch.float32) and y.shape == x.shape
    close(y, want[form], out, f"instnorm {form} ({n}, {HW}, {C}) -> {out}")
    y = run_instnorm(dev, x, w, b, form, out, res, gamma)
    close(y, res.double() + gamma.double() * want[form], out, f"instnorm {form} ({n}, {HW}, {C}) + epilogue -> {out}")


@pytest.mark.parametrize("form", ["instance", "rms"])
@pytest.mark.parametrize("n,HW,C", IN_CASES[2:])
def test_instnorm_on_an_offset_input(dev, n, HW, C, form):
    """x = 30 + randn: E[x^2] - mean^2 in fp32 loses 900 / 1 of its digits where mean-then-centred keeps them."""
    x, w, b, _, _, want = in_case(n, HW, C, IN_OFFSET)
    xi = x.permute(0, 2, 1).reshape(n, C, HW, 1)                                                   # torch's own fp32 kernels, on the CPU
    if form == "instance":
        own = torch.nn.functional.instance_norm(xi, weight=w, bias=b, eps=1e-5)
    else:
        std, _ = torch.std_mean(xi, dim=(-2, -1), keepdim=True)
        own = xi / (std + 1e-8) * w[None, :, None, None]
    own = own.reshape(n, C, HW).permute(0, 2, 1)
    assert rel_err(own, want[form]) < 0.5 * TOL["fp32"] and max_rel(own, want[form]) < TOL["fp32"], (rel_err(own, want[form]), max_rel(own, want[form]))
    close(run_instnorm(dev, x, w, b, form), want[form], "fp32", f"instnorm {form} ({n}, {HW}, {C}) at offset {IN_OFFSET}")


@pytest.mark.parametrize("n,HW,C", [(2, 2, 16), (2, 35, 48), (3, 256, 384)])
@pytest.mark.parametrize("form", ["instance", "rms"])
def test_instnorm_epilogue_in_place_equals_out_of_place(dev, form, n, HW, C):
    """One slab of two rows; two slabs with a ragged strip; eight slabs over six strips."""
    x, w, b, res, gamma, _ = in_case(n, HW, C)
    assert torch.equal(run_instnorm(dev, x, w, b, form, "fp32", res, gamma, in_place=True), run_instnorm(dev, x, w, b, form, "fp32", res, gamma))


@pytest.mark.parametrize("form", ["instance", "rms"])
def test_instnorm_without_affine(dev, form):
    """weight = bias = None: the plain normalisation (the kernel's weight of 1 and bias of 0)."""
    import tante_amd.avit as A
    from tante_amd import _lib as L
    x = in_case(2, 35, 48)[0]
    x4 = x.double().view(2, 1, 35, 48)
    want = (R.inst_norm(x4, None, None) if form == "instance" else R.rms_norm(x4, torch.ones(48))).view(2, 35, 48)
    y = A.instnorm(x.to(dev), L.INSTNORM_RMS if form == "rms" else L.INSTNORM_INSTANCE, None, None, 1e-8 if form == "rms" else 1e-5)
    close(y, want, "fp32", f"instnorm {form} without affine")


def test_instnorm_with_gelu(dev):
    """The nn.GELU() behind the stem's and the head's norms rides the same launch."""
    import tante_amd.avit as A
    from tante_amd import _lib as L
    x, w, b, _, _, want = in_case(2, 35, 48)
    y = A.instnorm(x.to(dev), L.INSTNORM_RMS, w.to(dev), None, 1e-8, act=L.ACT_GELU_ERF)
    close(y, R.gelu(want["rms"]), "fp32", "instnorm rms + GELU")


# ---- the attention kernels alone ---------------------------------------------------------------------------------------------------------
def norms(hd, gen, dev, qscale=1.0):
    qn, kn = torch.nn.LayerNorm(hd), torch.nn.LayerNorm(hd)
    with torch.no_grad():
        for m in (qn, kn):
            m.weight.copy_(1 + 0.2 * torch.randn(hd, generator=gen))
            m.bias.copy_(0.2 * torch.randn(hd, generator=gen))
        qn.weight.mul_(qscale)
        qn.bias.mul_(qscale)
    return qn, kn


def qkv_ref(y, qn, kn):
    """y (..., heads, 3, hd) float64 -> normalised q, k and v."""
    return (R.layer_norm(y[..., 0, :], qn.weight.detach(), qn.bias.detach()), R.layer_norm(y[..., 1, :], kn.weight.detach(), kn.bias.detach()),
            y[..., 2, :])


@pytest.mark.parametrize("n,heads,H,W,hd,qscale", [(2, 1, 1, 5, 16, 1.0), (2, 3, 2, 3, 16, 1.0), (1, 2, 16, 16, 64, 1.0), (1, 1, 17, 33, 32, 1.0),
                                                   (1, 1, 64, 64, 64, 1.0), (1, 2, 16, 16, 64, 8.0)])
def test_axial_attention_against_float64(dev, n, heads, H, W, hd, qscale):
    """An axis of one key; a tiny plane; the shipped plane; odd lengths past one and two 16-tiles; the limit; and the shipped plane with q
    scaled by 8, where the softmax saturates and the maximum subtraction matters."""
    import tante_amd.avit as A
    gen = torch.Generator().manual_seed(n + 3 * heads + 5 * H + 7 * W + hd)
    E = heads * hd
    qkv = torch.randn(n * H * W, 3 * E, generator=gen)
    qn, kn = norms(hd, gen, dev, qscale)
    q, k, v = qkv_ref(qkv.double().view(n, H, W, heads, 3, hd), qn, kn)
    xx = R.attention(*(t.permute(0, 1, 3, 2, 4) for t in (q, k, v))).permute(0, 1, 3, 2, 4)
    xy = R.attention(*(t.permute(0, 2, 3, 1, 4) for t in (q, k, v))).permute(0, 3, 1, 2, 4)
    want = ((xx + xy) / 2).reshape(n * H * W, E)
    got = A.axial_attention(qkv.to(dev), n, heads, H, W, qn.to(dev), kn.to(dev))
    close(got, want, "fp32", f"axial attention ({n}, {heads}, {H}, {W}, {hd}) q x {qscale}")


@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("T", [1, 2, 4, 6, 16])
def test_time_attention_against_float64(dev, T, hd):
    """37 sequences (no multiple of the wave size, nor of the sequences a workgroup stages), a random bias table."""
    import tante_amd.avit as A
    gen = torch.Generator().manual_seed(T * 10 + hd)
    heads, nseq = 3, 37
    E = heads * hd
    qkv = torch.randn(T * nseq, 3 * E, generator=gen)
    bias = torch.randn(heads, T, T, generator=gen)
    qn, kn = norms(hd, gen, dev)
    q, k, v = qkv_ref(qkv.double().view(T, nseq, heads, 3, hd), qn, kn)
    want = R.attention(*(t.permute(1, 2, 0, 3) for t in (q, k, v)), bias=bias.double()).permute(2, 0, 1, 3).reshape(T * nseq, E)
    got = A.time_attention(qkv.to(dev), nseq, T, heads, qn.to(dev), kn.to(dev), bias.to(dev))
    close(got, want, "fp32", f"time attention T {T}, hd {hd}")


def test_time_bias_reaches_the_log_buckets_on_the_device(dev):
    """T = 16 with the module's own table: positions past 8 take the log branch."""
    import tante_amd.avit as A
    torch.manual_seed(5)
    blk = A.AttentionBlock(48, 3)
    with torch.no_grad():
        blk.rel_pos_bias.relative_attention_bias.weight.normal_()
        blk.gamma.fill_(0.5)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    x = torch.randn(16, 1, 48, 2, 3)
    want = R.temporal_block(x.permute(0, 1, 3, 4, 2), sd, "", 3).permute(0, 1, 4, 2, 3)
    with torch.no_grad():
        close(blk.to(dev).eval()(x.to(dev)), want, "fp32", "temporal block T 16")


@pytest.mark.parametrize("B,T,C,H,W", [(2, 3, 2, 5, 7), (1, 4, 3, 64, 80)])
def test_field_stats_and_affine_against_float64(dev, B, T, C, H, W):
    """A tiny batch in one slab; several slabs that cross time steps.  Fields with different offsets and scales."""
    import tante_amd.avit as A
    gen = torch.Generator().manual_seed(B + T + C + H)
    x = torch.randn(B, T, C, H, W, generator=gen) * (1 + torch.rand(1, 1, C, 1, 1, generator=gen)) + 10 * torch.randn(B, 1, C, 1, 1, generator=gen)
    x64 = x.double()
    mean = x64.mean(dim=(1, 3, 4), keepdim=True)
    std = (((x64 - mean) ** 2).sum(dim=(1, 3, 4), keepdim=True) / (T * H * W - 1)).sqrt() + 1e-7
    stats, xn = A.field_stats(x.to(dev))
    close(stats[..., 0], mean.view(B, C), "fp32", "field mean")
    close(stats[..., 1], std.view(B, C), "fp32", "field std")
    close(xn, ((x64 - mean) / std).permute(1, 0, 3, 4, 2).reshape(T * B, H, W, C), "fp32", "normalised fields", bar=1e-5)
    y = torch.randn(2 * B, C, H, W, generator=gen)                                                # two returned steps, (t b) ordered
    want = y.double().view(2, B, C, H, W).permute(1, 0, 2, 3, 4) * std + mean
    close(A.field_affine(y.to(dev), stats, B), want, "fp32", "field affine")


# ---- blocks, stem, head, models, rollout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_spatial_block_against_the_reference(dev, mode):
    import tante_amd.avit as A
    g, sd, _ = keyed_golden(SPATIAL)
    blk = A.AxialAttentionBlock(48, int(g["heads"]))
    blk.load_state_dict(sd, strict=True)
    with torch.no_grad(), mode_scope(mode):
        y = blk.to(dev).eval()(g["x"].to(dev))
    close(y, g["y"], mode, "spatial block 5 x 7")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(TEMPORAL))
def test_temporal_block_against_the_reference(dev, name, mode):
    import tante_amd.avit as A
    g, sd, _ = keyed_golden(name)
    blk = A.AttentionBlock(48, int(g["heads"]))
    blk.load_state_dict(sd, strict=True)
    with torch.no_grad(), mode_scope(mode):
        y = blk.to(dev).eval()(g["x"].to(dev))
    close(y, g["y"], mode, f"{name} block")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_stem_and_head_against_the_reference(dev, mode):
    import tante_amd
    g, sd, _ = keyed_golden("g20_avit_stem")
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=int(g["n_states"])), embed_dim=48, num_heads=3, processor_blocks=1)
    m.load_state_dict(sd, strict=False)
    g2, sd2, _ = keyed_golden("g20_avit_head")
    m.load_state_dict(sd2, strict=False)
    m = m.to(dev).eval().set_compute(mode)
    n, c, H, W = g["x"].shape
    with torch.no_grad():
        rows = m.encode(g["x"].permute(0, 2, 3, 1).contiguous().to(dev))
        close(rows.view(n, H // 16, W // 16, 48).permute(0, 3, 1, 2), g["y"], mode, "stem (folded first convolution, 3 of 4 states)")
        with mode_scope(mode):
            close(m.debed(g2["x"].to(dev), range(int(g2["n_labels"]))), g2["y"], mode, "head (3 of 4 states)")


def build(name, dev, mode):
    import tante_amd
    g, sd, _ = keyed_golden(name)
    m = tante_amd.AViT(**model_kwargs(name))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval().set_compute(mode), g, sd


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_against_the_reference(dev, name, mode):
    m, g, _ = build(name, dev, mode)
    with torch.no_grad():
        y = m(g["x"].to(dev))
    assert tuple(y.shape) == tuple(g["y"].shape)
    close(y, g["y"], mode, f"{name} model")
    if mode == "bf16":          # autocast resolves to the same mode as set_compute
        m.set_compute(None)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            assert torch.equal(m(g["x"].to(dev)), y)


def rescale(m, gen):
    """The fixtures' recipe: layer scales 0.5 (1 + 0.1 randn), norms moved by 0.1 randn, the relative-bias embedding randn."""
    with torch.no_grad():
        for k, p in m.named_parameters():
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                p.copy_(0.5 * (1 + 0.1 * torch.randn(p.shape, generator=gen)))
            elif "norm" in k or ("_proj." in k and p.dim() == 1):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
            elif "relative_attention_bias" in k:
                p.copy_(torch.randn(p.shape, generator=gen))


def test_wide_model_against_the_restatement(dev):
    """Width 384, 6 heads of 64, depth 1 on 32 x 48 input, B 1, T 2: fc2's K of 1536 runs as three chunks with the accumulation through
    the residual operand; the shipped width's strips, head count and head dim."""
    import tante_amd
    gen = torch.Generator().manual_seed(2011)
    torch.manual_seed(2011)
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=2), out_steps=1, embed_dim=384, num_heads=6, processor_blocks=1)
    rescale(m, gen)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(1, 2, 2, 32, 48, generator=gen)
    want = R.model(x, sd, 6, 1)
    m = m.to(dev).eval()
    with torch.no_grad():
        close(m(x.to(dev)), want, "fp32", "wide model (embed 384)")
        close(m.set_compute("bf16")(x.to(dev)), want, "bf16", "wide model (embed 384)")


def test_default_width_model_against_the_restatement(dev):
    """The constructor's default width 768 with 12 heads of 64, depth 1, on a 2 x 3 token grid: every projection's K of 768 runs in two
    chunks and the head's first transposed convolution as a tap GEMM + gather."""
    import tante_amd
    gen = torch.Generator().manual_seed(2012)
    torch.manual_seed(2012)
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=2), processor_blocks=1)
    assert m.embed.embed_dim == 768 and m.blocks[0].spatial.num_heads == 12
    rescale(m, gen)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = torch.randn(1, 2, 2, 32, 48, generator=gen)
    want = R.model(x, sd, 12, 1)
    with torch.no_grad():
        close(m.to(dev).eval()(x.to(dev)), want, "fp32", "default-width model (embed 768)")


def test_rollout_against_the_refed_restatement(dev):
    """rollout_model at T 4 re-feeds four frames per call: 6 steps (two calls, the last two frames dropped) against the float64
    restatement re-fed on the CPU."""
    import tante_amd
    name = "g20_avit_model_32x48_T4"
    m, g, sd = build(name, dev, "fp32")
    c = MODELS[name]
    x = g["x"]
    batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous().to(dev), "output": torch.zeros(2, 6, 32, 48, 3, device=dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(tante_amd.TanteMetadata(n_fields=3, spatial_resolution=(32, 48)))
    with torch.no_grad():
        y, y_ref = tante_amd.rollout_model(m, batch, fmt, 6)
    assert tuple(y.shape) == (2, 6, 32, 48, 3) and tuple(y_ref.shape) == (2, 6, 32, 48, 3)
    want = R.rollout(x, sd, c["heads"], c["depth"], 6).permute(0, 1, 3, 4, 2)
    for t in range(6):
        close(y[:, t], want[:, t], "fp32", f"rollout step {t + 1}")


def test_out_of_scope_cases_raise(dev):
    import tante_amd
    import tante_amd.avit as A
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=2), embed_dim=32, num_heads=2, processor_blocks=1).to(dev)
    x = torch.randn(1, 2, 2, 16, 32, device=dev)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.train()(x)
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        m.eval()(x)                                  # grad enabled with trainable parameters
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training is out of scope"):
        m.train()(x)
    m.eval()
    with torch.no_grad():
        assert tuple(m(x).shape) == (1, 2, 2, 16, 32)                     # min(t, 4) steps, whatever out_steps says
        with pytest.raises(ValueError, match="multiples of 16"):
            m(torch.randn(1, 2, 2, 16, 24, device=dev))
        with pytest.raises(ValueError, match="1 x 1 token grid"):
            m(torch.randn(1, 2, 2, 16, 16, device=dev))
        with pytest.raises(NotImplementedError, match="T = 17 is out of scope"):
            m(torch.randn(1, 17, 2, 16, 32, device=dev))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x.cpu())
        # shapes past the kernels' limits fail with the library's message, not silently
        blk = A.AxialAttentionBlock(32, 2).to(dev).eval()
        with pytest.raises(RuntimeError, match="tante_axial_attention: token axes outside 1..64"):
            blk(torch.randn(1, 32, 2, 65, device=dev))
        with pytest.raises(RuntimeError, match="tante_axial_attention: head dim not one of 16, 32, 64"):
            A.AxialAttentionBlock(48, 2).to(dev).eval()(torch.randn(1, 48, 2, 3, device=dev))
        with pytest.raises(RuntimeError, match="tante_instnorm: tokens per image outside 2..4096"):
            A.instnorm(torch.randn(1, 4097, 16, device=dev), 1, None, None, 1e-8)
        with pytest.raises(RuntimeError, match="tante_time_attention: time steps outside 1..16"):
            A.time_attention(torch.randn(17 * 2, 96, device=dev), 2, 17, 2, blk.qnorm, blk.knorm, torch.zeros(2, 17, 17, device=dev))
    with pytest.raises(NotImplementedError, match="override_block"):
        tante_amd.AViT(4, override_block=A.SpaceTimeBlock)
