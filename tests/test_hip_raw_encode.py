"""GPU tests: the rollout's first window encoded straight from the channels-last batch (TANTE_RAW_ENCODE, kernels.encode_window_raw).

Every comparison is byte for byte against the launches the route replaces, on the same weights: tante_format_input of all T frames into
a full rollout buffer, then the encoder's forward_frames (what TANTE.encode_frames runs) on that buffer.  Byte for byte means torch.equal on
the BIT PATTERNS: a planted +-inf becomes +-FLT_MAX, which rounds to +-inf as a bf16 operand, so the tokens of its patch are +-inf or NaN on
both paths (gelu(-inf) = -inf * 0), and torch.equal on floats calls NaN unequal to itself.

* kernel level -- D = 11 / 4 / 3 / 16 fields at 32 x 32 and 32 x 64, NaN and +-inf planted in the corners of the images and of the field
  axis: the frame cache z and the slot-(T - 1) frame equal the reference's; every other slot of the buffer keeps its sentinel; a buffer
  with the batch stride of a longer rollout; an 8 x 640 image (three row segments, dead token rows); each case on the shipped two-launch
  form and on the one-launch form (TANTE_RAW_ENCODE_ONE_LAUNCH).
* rollout level -- cfg2's model block at 32 x 32: rollout_model with the switch on against off, eager and as a captured graph.
* routing -- 17 fields (K = 68), fp32 compute, TANTE_NO_ENC_CACHE and the training branch keep the old launches.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 123.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _encoder(dev, D, H, W):
    import tante_amd
    from tante_amd.tante import enc_CNN
    torch.manual_seed(31 + D)
    md = tante_amd.TanteMetadata(n_fields=D, spatial_resolution=(H, W))
    return enc_CNN(md, embed_dim=256, patch_scale=8, overlap_ratio=0.0).to(dev).eval()


def _raw(dev, B, T, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, T, H, W, D, generator=g)
    nan, inf = float("nan"), float("inf")
    # first / last pixel of an image, first / last field, slot T - 1 and an earlier slot
    raw[0, T - 1, 0, 0, 0] = nan
    raw[0, T - 1, H - 1, W - 1, D - 1] = inf
    raw[B - 1, T - 1, 0, 0, D - 1] = -inf
    raw[B - 1, T - 1, H - 1, W - 1, 0] = nan
    raw[0, 0, 0, 0, 0] = inf
    raw[B - 1, 0, H - 1, W - 1, D - 1] = nan
    raw[0, 1, 0, W - 1, 0] = -inf
    raw[B - 1, T - 2, H - 1, 0, D - 1] = inf
    return raw.to(dev)


class _LibOption:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from tante_amd import _lib
        self.old = _lib.get_option(self.name, 0)
        _lib.set_option(self.name, int(self.value))

    def __exit__(self, *a):
        from tante_amd import _lib
        _lib.set_option(self.name, int(self.old))


# 8 x 640, B = 1: three 256-pixel row segments (the last one 128 wide), every wave of a workgroup with a tile, two tiles for wave 0,
# three LDS-DMA passes per pixel row at D = 11; 80 tokens, so the one-launch form's workgroup has dead rows
@pytest.mark.parametrize("one_launch", [0, 1])
@pytest.mark.parametrize("B,H,W,extra", [(2, 32, 32, 1), (2, 32, 32, 8), (2, 32, 64, 1), (2, 32, 64, 8), (1, 8, 640, 1)])
@pytest.mark.parametrize("D", [11, 4, 3, 16])
def test_encode_window_raw_kernel(dev, D, B, H, W, extra, one_launch):
    """`extra`: the slots behind the window, i.e. the batch stride of a (B, T + extra, D, H, W) rollout buffer.  `one_launch`: the form
    with stage 1 inside the stage 2 + 3 kernel (TANTE_RAW_ENCODE_ONE_LAUNCH), which is built and held to the same bits, not the default."""
    from tante_amd import _lib as L, kernels as K
    T, C_ = 4, 256
    enc = _encoder(dev, D, H, W)
    assert enc.raw_window_supported(L.BF16)
    raw = _raw(dev, B, T, H, W, D, 5 * D + W + extra)
    HW = (H // 8) * (W // 8)
    # the launches the route replaces
    buf0 = torch.full((B, T + extra, D, H, W), SENTINEL, device=dev)
    z0 = torch.full((T, B, HW, C_), SENTINEL, device=dev)
    L.check(L.lib().tante_format_input(raw.data_ptr(), B * T, T, H * W, D, buf0.data_ptr(), buf0.stride(0), K._stream()), "tante_format_input")
    with torch.no_grad():
        enc.forward_frames(buf0[:, :T], L.BF16, buf0.stride(0), z0)
    # the route
    buf1 = torch.full((B, T + extra, D, H, W), SENTINEL, device=dev)
    z1 = torch.full((T, B, HW, C_), -SENTINEL, device=dev)
    with torch.no_grad(), _LibOption("TANTE_RAW_ENCODE_ONE_LAUNCH", one_launch):
        enc.forward_window_raw(raw, L.BF16, z1, buf1[:, T - 1])
    torch.cuda.synchronize()
    assert not (z0 == SENTINEL).any()
    assert torch.isfinite(z0).float().mean() > 0.5, "the planted values reach their own patches only"
    assert torch.equal(buf0[:, T - 1], torch.nan_to_num(raw[:, T - 1].permute(0, 3, 1, 2)))
    assert _same_bits(z1, z0)
    assert _same_bits(buf1[:, T - 1], buf0[:, T - 1])
    assert (buf1[:, T:] == SENTINEL).all(), "slots behind the window were written"
    assert (buf1[:, :T - 1] == SENTINEL).all(), "slots 0 .. T - 2 were written"


def test_pack_follows_the_weights(dev):
    """The stage-1 stream is rebuilt when a conv parameter changes."""
    from tante_amd import _lib as L, kernels as K
    B, T, D, H, W = 1, 2, 4, 32, 32
    enc = _encoder(dev, D, H, W)
    raw = _raw(dev, 2, 4, H, W, D, 77)[:B, :T].contiguous()
    zs = []
    for k in range(2):
        if k:
            with torch.no_grad():
                enc.enc_conv_1.conv.weight.mul_(0.5)
        buf = torch.empty(B, T, D, H, W, device=dev)
        z0, z1 = torch.empty(T, B, 16, 256, device=dev), torch.empty(T, B, 16, 256, device=dev)
        L.check(L.lib().tante_format_input(raw.data_ptr(), B * T, T, H * W, D, buf.data_ptr(), buf.stride(0), K._stream()), "tante_format_input")
        with torch.no_grad():
            enc.forward_frames(buf, L.BF16, buf.stride(0), z0)
            enc.forward_window_raw(raw, L.BF16, z1, torch.empty(B, D, H, W, device=dev))
        torch.cuda.synchronize()
        assert _same_bits(z1, z0)
        zs.append(z1)
    assert not _same_bits(zs[0], zs[1])


def _model(dev, n_fields=11, compute="bf16"):
    import tante_amd
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "tante_am.yaml"))
    md = tante_amd.TanteMetadata(n_fields=n_fields, spatial_resolution=(32, 32))
    torch.manual_seed(cfg.get("seed", 211))
    m = tante_amd.build_model(cfg, md).to(dev).eval().set_compute(compute)
    return m, md


def _batch(dev, md, B, T, n_steps, seed):
    g = torch.Generator().manual_seed(seed)
    res, D = tuple(md.spatial_resolution), md.n_fields
    x = torch.randn(B, T, *res, D, generator=g)
    x[0, T - 1, 0, 0, 0] = float("nan")                     # -> 0: the rollout stays finite
    x[B - 1, 0, res[0] - 1, res[1] - 1, D - 1] = float("nan")
    return {"input": x.to(dev), "output": torch.randn(B, n_steps, *res, D, generator=g).to(dev)}


class _Switch:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        import tante_amd
        self.old = tante_amd.get_option(self.name)
        tante_amd.set_option(self.name, int(self.value))

    def __exit__(self, *a):
        import tante_amd
        tante_amd.set_option(self.name, int(self.old))


def _count_route(monkeypatch):
    from tante_amd import kernels as K
    calls = []
    orig = K.encode_window_raw

    def wrap(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    monkeypatch.setattr(K, "encode_window_raw", wrap)
    return calls


@pytest.fixture(scope="module")
def cfg2_small(dev):
    import tante_amd
    m, md = _model(dev)
    batch = _batch(dev, md, 2, 4, 3, 909)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    with _Switch("TANTE_RAW_ENCODE", 0), torch.inference_mode():
        y, yr = tante_amd.rollout_model(m, batch, fmt, 3)
        torch.cuda.synchronize()
        ref = (y.clone(), yr.clone())
    return m, md, batch, fmt, ref


def test_rollout_on_equals_off(dev, cfg2_small, monkeypatch):
    import tante_amd
    m, md, batch, fmt, (y0, r0) = cfg2_small
    calls = _count_route(monkeypatch)
    assert tante_amd.get_option("TANTE_RAW_ENCODE")
    with torch.inference_mode():
        y1, r1 = tante_amd.rollout_model(m, batch, fmt, 3)
    torch.cuda.synchronize()
    assert len(calls) == 1, "the rollout did not take the raw-encode route"
    assert torch.isfinite(y0).all()
    assert _same_bits(y1, y0) and _same_bits(r1, r0)
    with _Switch("TANTE_RAW_ENCODE", 0), torch.inference_mode():
        tante_amd.rollout_model(m, batch, fmt, 3)
    assert len(calls) == 1, "TANTE_RAW_ENCODE=0 still took the route"


def test_graphed_rollout_on_equals_off(dev, cfg2_small):
    import tante_amd
    m, md, batch, fmt, (y0, r0) = cfg2_small
    assert tante_amd.get_option("TANTE_RAW_ENCODE")
    roll = tante_amd.GraphedRollout(m, batch, fmt, 3)
    for _ in range(2):
        yg, rg = roll(batch)
        torch.cuda.synchronize()
        assert torch.isfinite(yg).all() and _same_bits(yg, y0) and _same_bits(rg, r0)


@pytest.mark.parametrize("case", ["d17", "fp32", "no_enc_cache", "training"])
def test_other_paths_keep_their_launches(dev, monkeypatch, case):
    import tante_amd
    calls = _count_route(monkeypatch)
    m, md = _model(dev, n_fields=17 if case == "d17" else 11, compute="fp32" if case == "fp32" else "bf16")
    batch = _batch(dev, md, 1, 4, 1, 41)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    assert tante_amd.get_option("TANTE_RAW_ENCODE")
    if case == "training":
        m.train()
        y, _ = tante_amd.rollout_model(m, batch, fmt, 1)
        assert y.requires_grad
    elif case == "no_enc_cache":
        with _Switch("TANTE_NO_ENC_CACHE", 1), torch.inference_mode():
            y, _ = tante_amd.rollout_model(m, batch, fmt, 1)
    else:
        with torch.inference_mode():
            y, _ = tante_amd.rollout_model(m, batch, fmt, 1)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (1, 1, 32, 32, md.n_fields)
    assert not calls, f"{case}: took the raw-encode route"
