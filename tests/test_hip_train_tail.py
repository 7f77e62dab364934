"""GPU parity of the one-launch TRAINING TAIL (csrc/tail_chain.hip) and of the Taylor sum, each alone, against float64 autograd.

The tail is what every TANTE train step runs per rollout call at the shipped shapes (train_forward.tail_train_cfg): every order's dec_CNN
head -> Taylor sum -> re-encoding of the predicted frame by enc_CNN, one launch forward and one backward (autograd.TailFn), and the
encoder half alone on the initial window's frames (autograd.EncTailFn).  Until now it ran only inside whole-model runs, compared with the
per-operator bf16 path at 2e-2 per gradient (tests/test_hip_round6.py) or with the reference at 4e-2 (test_g14_wide_train_step), and only
the RT3 = 1 and RT3 = 3 instantiations of its kernels (RT3 = ceil(4 D / 16) row tiles at the pixel level) ever ran.  Here TailFn is driven
with a hand-built TailCfg (coefficients of similar size, so that no order hides behind a small dt^k / k!) at every RT3, padded and full
row tiles, one to 129 workgroups (the bias / pixel-weight-gradient reduce walks its rows in pairs of 64), and through each branch of its
host code: no re-encoding, a loss through y or z only, the immediate weight-gradient paths (PIXEL_WGRAD_IN_KERNEL off, DEFER_WGRAD off,
Tk % 32 != 0), gradient slots that already hold values, two nodes sharing the parameters in one backward.  One case goes through
tail_train_cfg with a real model, so the production wiring (coefficients, parameter order, streams) is what is tested.

Every case compares, against torch.autograd on the plain operation in float64 (the same bf16-rounded weights and residual rows the
kernel reads), the increment y - base (the fp32 base passes through exactly and would hide a wrong derivative), z, the encoder's share of
the frame's gradient dbase - Gy (same reason), the last time slot of every residual stream's gradient (the other slots exactly zero) and
all six gradients of every decoder and of the encoder.  The references are pinned to the CPU oracles by
tests/test_host_cpu.py::test_train_tail_references_match_the_oracles.

Bars (derivation): the kernel rounds to bf16 at known places; one rounding of a value is an error uniform in +- 2^-9 of it, RMS
U = 2^-9 / sqrt(3), and independent roundings add in quadrature.  A result reached through n roundings after the rounded inputs is held
to relative L2 <= 4 U sqrt(n) (4x the expected RMS), max-norm <= 3.2x that, neither above 1e-2 / 3.2e-2.  n is counted from the source
(see the N_* constants); a bf16 rounding of a value that only enters through a GELU derivative is counted as a full one.
"""
import math

import pytest
import torch

from conftest import rel_err, max_rel, record_parity

pytestmark = pytest.mark.gpu

U_BF16 = 2.0 ** -9 / math.sqrt(3.0)      # RMS relative error of one round-to-nearest to bf16 (8 significant bits)
CAP_REL, MAX_FACTOR = 1e-2, 3.2
F32_REL, F32_MAX = 2e-5, 1e-4            # tests/test_hip_train_ops.py's fp32 bars (the Taylor sum; sums of exact fp32 terms)

# Rounding counts, from tail_chain.hip (forward: tail_fwd_kernel; backward: tail_bwd_kernel; the wide weight gradients read the bf16
# row operands it writes):
N_INC = 4            # y - base: pre1, act1 (stage 1), pre2, act2 (stage 2); stage 3 and the Taylor sum accumulate in fp32
N_Z = N_INC + 1 + 4  # z: the decoders' four, the frame's bf16 image (L3 / f16), pre1e, act1e, pre2e, act2e; stage 3 fp32       -> cap
N_ENC_Z = 4          # EncTailFn's z from bf16-exact frames: pre1e, act1e, pre2e, act2e
N_DZ = 1             # the encoder's last bias gradient: column sums of dz16 (= bf16(Gz)) in fp32
# the encoder's backward (dbase - Gy, the encoder's gradients): dz16, dpre2e, dpre1e, and the GELU derivatives read pre2e, pre1e, whose
# values carry the frame's image, pre1e, act1e, pre2e and the decoders' four: 3 + 8 = 11                                          -> cap
N_ENC_BWD = 11
# the decoders' backward (dx, the decoders' gradients): dfr carries the encoder's share (11), then L3 = bf16(coef dfr), dpre2, dpre1
# and the GELU derivatives at pre2, pre1 (with act1 in front of pre2): 11 + 6 = 17 -> 4 U sqrt(17) = 1.9e-2, held to the 1e-2 cap.
# Measured on a clean build the closest results are these with the loss through z only (dfr is then the encoder's share alone, nothing
# exact dilutes it): up to 9.3e-3 on the decoders' last bias gradient at D = 5, twice the RMS model U sqrt(17) = 4.6e-3 -- the bias
# and weight gradients are sums over every pixel, and one rounding of dpre1e reaches the 4 D pixels of its patch with one sign, so
# those errors do not average out over the sum the way independent ones would.  With a loss through y as well, dfr = Gy (exact) + the
# encoder's share and the same results stay at or below 5.1e-3.
N_DEC_BWD = 17


def bf16_bar(n: int):
    r = min(4.0 * U_BF16 * math.sqrt(n), CAP_REL)
    return r, MAX_FACTOR * r


BAR_INC, BAR_Z, BAR_ENC_Z, BAR_DZ, BAR_ENC_BWD, BAR_DEC_BWD = (bf16_bar(n) for n in (N_INC, N_Z, N_ENC_Z, N_DZ, N_ENC_BWD, N_DEC_BWD))
COEFS = [1.0, -0.7, 1.3]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(got, ref, what, bar, mode="bf16"):
    """got (kernel) vs ref (float64 reference): relative L2 and max-norm, recorded in parity_report.json with the bar."""
    rb, mb = bar
    got, ref = got.detach().to(torch.float64).cpu(), ref.detach().to(torch.float64).cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    r, m = rel_err(got, ref), max_rel(got, ref)
    record_parity(r, m, rb, mode, what)
    assert r <= rb and m <= mb, f"{what}: rel {r:.3e} (bar {rb:.1e}), max {m:.3e} (bar {mb:.1e})"


def randn(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).to(torch.float32)


# ---- float64 references (plain torch, from the maths; pinned by test_host_cpu.py) ------------------------------------------------------
def ref_gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ref_deconv2(x, w, b):
    """ConvTranspose2d(kernel 2, stride 2) on channels-last x (n, H, W, Cin), weight (Cin, Cout, 2, 2): y[2h + kh, 2w + kw] = x[h, w] W[:, :, kh, kw]."""
    n, H, W, _ = x.shape
    return torch.einsum("nhwc,cokl->nhkwlo", x, w).reshape(n, 2 * H, 2 * W, w.shape[1]) + b


def ref_conv2(x, w, b):
    """Conv2d(kernel 2, stride 2) on channels-last x (n, H, W, Cin), weight (Cout, Cin, 2, 2)."""
    n, H, W, C = x.shape
    return torch.einsum("nhkwlc,ockl->nhwo", x.reshape(n, H // 2, 2, W // 2, 2, C), w) + b


def ref_dec(x, p):
    """dec_CNN at patch scale 8: tokens (n, Hp, Wp, 256) -> (n, D, 8 Hp, 8 Wp); p = (w1, b1, w2, b2, w3, b3); GELU(erf) after stages 1, 2."""
    for i in range(3):
        x = ref_deconv2(x, p[2 * i], p[2 * i + 1])
        if i < 2:
            x = ref_gelu(x)
    return x.permute(0, 3, 1, 2)


def ref_enc(y, p):
    """enc_CNN at patch scale 8, pre-FiLM: frames (n, D, H, W) -> (n, Hp Wp, 256)."""
    x = y.permute(0, 2, 3, 1)
    for i in range(3):
        x = ref_conv2(x, p[2 * i], p[2 * i + 1])
        if i < 2:
            x = ref_gelu(x)
    return x.reshape(x.shape[0], -1, x.shape[-1])


def ref_taylor(inp, dt, n_out, derivs):
    """tante.py:165-171: out_i = inp[:, -1] + sum_k derivs[k] (i dt)^(k + 1) / (k + 1)!, i = 1 .. n_out."""
    return torch.cat([inp[:, -1:] + sum(d * ((i * dt) ** (k + 1) / math.factorial(k + 1)) for k, d in enumerate(derivs))
                      for i in range(1, n_out + 1)], dim=1)


# ---- driving the kernels ---------------------------------------------------------------------------------------------------------
def _enc_params(enc):
    return [q for i in range(3) for q in (getattr(enc, f"enc_conv_{i + 1}").conv.weight, getattr(enc, f"enc_conv_{i + 1}").conv.bias)]


def _dec_params(dec):
    return [q for i in range(3) for q in (getattr(dec, f"dec_conv_{i + 1}").deconv.weight, getattr(dec, f"dec_conv_{i + 1}").deconv.bias)]


def _modules(dev, n_dec, D, Hp, Wp, gen):
    """enc_CNN and n_dec dec_CNN at patch scale 8 without overlap, CPU-seeded weights of unit-scale outputs (fp32: the pack rounds them),
    biases large enough to matter, zero-filled gradient slots (as FlatAdamW.zero_grad leaves them)."""
    import tante_amd
    from tante_amd.tante import enc_CNN, dec_CNN
    md = tante_amd.TanteMetadata(n_fields=D, spatial_resolution=(8 * Hp, 8 * Wp))
    enc = enc_CNN(md, embed_dim=256, patch_scale=8, overlap_ratio=0.0)
    decs = [dec_CNN(md, embed_dim=256, patch_scale=8, overlap_ratio=0.0) for _ in range(n_dec)]
    for p in _enc_params(enc) + [q for d in decs for q in _dec_params(d)]:
        if p.dim() == 1:
            p.data.copy_(randn(p.shape, gen, 0.5))
    for p in _enc_params(enc)[0::2]:          # conv weight (Cout, Cin, 2, 2): fan-in 4 Cin
        p.data.copy_(randn(p.shape, gen, 1.0 / math.sqrt(4 * p.shape[1])))
    for d in decs:
        for p in _dec_params(d)[0::2]:        # transposed-conv weight (Cin, Cout, 2, 2): each output sees Cin inputs
            p.data.copy_(randn(p.shape, gen, 1.0 / math.sqrt(p.shape[0])))
    enc, decs = enc.to(dev), [d.to(dev) for d in decs]
    for p in _enc_params(enc) + [q for d in decs for q in _dec_params(d)]:
        p.grad = torch.zeros_like(p)
    return enc, decs


def _cfg(B, T, Hp, Wp, D, coefs, enc, decs, want_z):
    from tante_amd import kernels as K
    from tante_amd.autograd import TailCfg
    ep, dps = _enc_params(enc), [_dec_params(d) for d in decs]
    return TailCfg(B, T, Hp, Wp, 256, D, list(coefs), dps, [K.pack_tail(p, D, True) for p in dps], ep, K.pack_tail(ep, D, False), want_z)


def _ref_params(params, dev):
    """float64 leaves of the values the kernel computes with: weights bf16-rounded (tc_pack), biases fp32."""
    return [(p.detach().to(torch.bfloat16) if p.dim() > 1 else p.detach()).to(dev, torch.float64).requires_grad_() for p in params]


class _Call:
    """One TailFn call's inputs (CPU-seeded) and its outputs."""

    def __init__(self, dev, cfg, gen):
        B, T, HW, D, H, W = cfg.B, cfg.T, cfg.HW, cfg.D, 8 * cfg.Hp, 8 * cfg.Wp
        self.xs = [randn((B * T * HW, 256), gen).to(dev).requires_grad_() for _ in cfg.coefs]
        self.base = randn((B, 1, D, H, W), gen).to(dev).requires_grad_()
        self.Gy, self.Gz = randn((B, 1, D, H, W), gen).to(dev), randn((B, HW, 256), gen).to(dev)

    def run(self, cfg, use_y, use_z):
        from tante_amd.autograd import TailFn
        self.y, self.z = TailFn.apply(self.base, cfg, *self.xs)
        loss = 0.0
        if use_y:
            loss = loss + (self.y * self.Gy).sum()
        if use_z and cfg.want_z:
            loss = loss + (self.z * self.Gz).sum()
        return loss

    def reference(self, cfg, dec64, enc64, use_y, use_z):
        B, T, HW = cfg.B, cfg.T, cfg.HW
        self.x64 = [x.detach().view(B, T, HW, 256)[:, -1].to(torch.bfloat16).to(torch.float64).view(B, cfg.Hp, cfg.Wp, 256).requires_grad_()
                    for x in self.xs]
        self.b64 = self.base.detach().to(torch.float64).requires_grad_()
        self.inc64 = sum(c * ref_dec(x, p) for c, x, p in zip(cfg.coefs, self.x64, dec64)).unsqueeze(1)
        y64 = self.b64 + self.inc64
        self.z64 = ref_enc(y64[:, 0], enc64)
        loss = 0.0
        if use_y:
            loss = loss + (y64 * self.Gy.double()).sum()
        if use_z and cfg.want_z:
            loss = loss + (self.z64 * self.Gz.double()).sum()
        return loss


def _slots(params):
    return [p.grad for p in params]


def _check_call(c, cfg, tag, use_y, use_z):
    B, T, HW = cfg.B, cfg.T, cfg.HW
    close(c.y.detach().double() - c.base.detach().double(), c.inc64, tag + " y - base", BAR_INC)
    if cfg.want_z:
        close(c.z, c.z64, tag + " z", BAR_Z)
    else:
        assert c.z is None
    Gy = c.Gy if use_y else torch.zeros_like(c.Gy)
    if use_z and cfg.want_z:
        close(c.base.grad.double() - Gy.double(), c.b64.grad - Gy.double(), tag + " dbase - Gy (encoder's share)", BAR_ENC_BWD)
    else:      # no gradient reaches the encoder: the frame's gradient is d_out, passed through exactly
        assert torch.equal(c.base.grad, Gy), tag + " dbase != Gy"
    for k, (x, x64) in enumerate(zip(c.xs, c.x64)):
        g = x.grad.view(B, T, HW, 256)
        assert torch.count_nonzero(g[:, :-1]) == 0, f"{tag} dx{k}: earlier time slots written"
        close(g[:, -1], x64.grad.view(B, HW, 256), f"{tag} dx{k} (last time slot)", BAR_DEC_BWD)


NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def _check_params(got, init, ref64, tag, enc):
    for i, (g, g0, r) in enumerate(zip(got, init, ref64)):
        bar = (BAR_DZ if i == 5 else BAR_ENC_BWD) if enc else BAR_DEC_BWD
        close(g - g0, r.grad, f"{tag} d{NAMES[i]}", bar)


# (orders, D, Hp, Wp, B, T): tiles = B Hp Wp / 16, one workgroup each; RT3 = ceil(4 D / 16)
TAIL_CASES = [
    (1, 1, 1, 16, 1, 1),       # one tile; 12 padded stage-3 rows; Tk = 16: the widest weight gradient runs immediately
    (3, 5, 2, 16, 3, 4),       # RT3 = 2 (never run before), padded
    (2, 8, 4, 32, 2, 2),       # RT3 = 2, full
    (3, 9, 3, 16, 1, 1),       # RT3 = 3, padded; Tk = 48: the widest weight gradient runs immediately
    (3, 12, 13, 16, 5, 4),     # RT3 = 3, full; 65 tiles: one row past the reduce's 64
    (1, 7, 43, 16, 3, 1),      # 129 tiles: past 2 x 64 rows, both halves of the reduce's paired loop and its tail
    (3, 11, 32, 32, 2, 4),     # cfg2's field count and order at 256 x 256, 128 tiles
]


def _tail(dev, orders, D, Hp, Wp, B, T, seed, *, want_z=True, use_y=True, use_z=True, prefill=False, two=False):
    gen = torch.Generator().manual_seed(seed)
    enc, decs = _modules(dev, orders, D, Hp, Wp, gen)
    cfg = _cfg(B, T, Hp, Wp, D, COEFS[:orders], enc, decs, want_z)
    ep, dps = _enc_params(enc), [_dec_params(d) for d in decs]
    allp = ep + [q for dp in dps for q in dp]
    if prefill or not (want_z and use_z):      # slots that already hold values: added into (or, for the encoder here, left alone)
        for p in allp:
            p.grad.copy_(randn(p.shape, gen, 0.1).to(dev))
    init = [p.grad.clone() for p in allp]
    calls = [_Call(dev, cfg, gen) for _ in range(2 if two else 1)]
    return cfg, enc, decs, calls, init


def _run_and_check(dev, cfg, enc, decs, calls, init, tag, use_y=True, use_z=True):
    from tante_amd.autograd import run_backward
    ep, dps = _enc_params(enc), [_dec_params(d) for d in decs]
    loss = sum(c.run(cfg, use_y, use_z) for c in calls)
    run_backward(loss)
    torch.cuda.synchronize()
    enc64, dec64 = _ref_params(ep, dev), [_ref_params(dp, dev) for dp in dps]
    sum(c.reference(cfg, dec64, enc64, use_y, use_z) for c in calls).backward()
    for i, c in enumerate(calls):
        _check_call(c, cfg, tag + (f" call{i}" if len(calls) > 1 else ""), use_y, use_z)
    n_enc = len(ep)
    if cfg.want_z and use_z:
        _check_params(_slots(ep), init[:n_enc], enc64, tag + " enc", True)
    else:
        for i, p in enumerate(ep):
            assert torch.equal(p.grad, init[i]), f"{tag}: encoder slot {NAMES[i]} changed"
    for k, (dp, d64) in enumerate(zip(dps, dec64)):
        off = n_enc + 6 * k
        _check_params(_slots(dp), init[off:off + 6], d64, f"{tag} dec{k}", False)


@pytest.mark.parametrize("orders,D,Hp,Wp,B,T", TAIL_CASES)
def test_tail_against_float64(dev, orders, D, Hp, Wp, B, T):
    cfg, enc, decs, calls, init = _tail(dev, orders, D, Hp, Wp, B, T, seed=1000 * D + Hp * Wp + orders)
    _run_and_check(dev, cfg, enc, decs, calls, init, f"tail o{orders} D{D} {Hp}x{Wp} B{B} T{T}")


BRANCH_SHAPES = [(3, 5, 2, 16, 3, 4), (2, 11, 4, 16, 2, 2)]       # RT3 = 2 padded, RT3 = 3 (Tk = 128: the deferred wide gradients)
BRANCHES = ["no_z", "y_only", "z_only", "pixel_wgrad_off", "defer_off", "prefilled", "two_nodes"]


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("shape", BRANCH_SHAPES, ids=["rt3_2", "rt3_3"])
def test_tail_branches_against_float64(dev, monkeypatch, shape, branch):
    """no_z: want_z = False (the rollout's last call) -- z is None, the encoder's slots are bit-unchanged, dbase = Gy exactly.
    y_only: z is computed but unused (d_z None) -- the encoder's slots are bit-unchanged.  z_only: d_out None.
    pixel_wgrad_off / defer_off: the immediate weight-gradient paths.  prefilled: the kernels add into what the slots hold.
    two_nodes: two calls sharing the parameters in one backward (as the rollout's calls do) -- the sum of both references."""
    from tante_amd import autograd as A
    orders, D, Hp, Wp, B, T = shape
    if branch == "pixel_wgrad_off":
        monkeypatch.setattr(A, "PIXEL_WGRAD_IN_KERNEL", False)
    if branch == "defer_off":
        monkeypatch.setattr(A, "DEFER_WGRAD", False)
    use_y, use_z = branch != "z_only", branch != "y_only"
    cfg, enc, decs, calls, init = _tail(dev, orders, D, Hp, Wp, B, T, seed=77 * D + BRANCHES.index(branch), want_z=branch != "no_z",
                                        use_y=use_y, use_z=use_z, prefill=branch == "prefilled", two=branch == "two_nodes")
    _run_and_check(dev, cfg, enc, decs, calls, init, f"tail {branch} o{orders} D{D} {Hp}x{Wp}", use_y=use_y, use_z=use_z)


def test_tail_production_wiring_cfg3(dev):
    """cfg3's tail: a real TANTE (4 fields, 128 x 384 -> 16 x 48 tokens, order 1, dt = 1, B = 2, T = 4: 96 tiles, the reduce past 64 rows)
    through train_forward.tail_train_cfg inside a fold scope -- the coefficients, parameter order and packed streams production uses --
    against the reference built from the model's own modules."""
    import tante_amd
    from tante_amd import _lib as L, train_forward as TF
    from tante_amd.autograd import run_backward
    D, B = 4, 2
    md = tante_amd.TanteMetadata(n_fields=D, spatial_resolution=(128, 384))
    torch.manual_seed(3)
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=1, attn_axes="T", n_head=8, embed_dim=256, patch_scale=8, dropout=0.0,
                        frame_interval=1.0).to(dev).train()
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    gen = torch.Generator().manual_seed(33)
    with TF.fold_scope():
        cfg = TF.tail_train_cfg(m, B, L.BF16, True)
        assert cfg is not None, "cfg3's model does not take the fused tail"
        c = _Call(dev, cfg, gen)
        loss = c.run(cfg, True, True)
    run_backward(loss)
    torch.cuda.synchronize()
    ep, dps = _enc_params(m.encoder), [_dec_params(d) for d in m.decoders]
    enc64, dec64 = _ref_params(ep, dev), [_ref_params(dp, dev) for dp in dps]
    ref_cfg = type("Cfg", (), dict(B=B, T=m.T, HW=m.H_p * m.W_p, Hp=m.H_p, Wp=m.W_p, D=D, want_z=True,
                                   coefs=[m.frame_interval ** (k + 1) / math.factorial(k + 1) for k in range(m.taylor_order)]))
    assert (ref_cfg.Hp, ref_cfg.Wp, ref_cfg.T) == (16, 48, 4) and list(cfg.coefs) == ref_cfg.coefs
    c.reference(ref_cfg, dec64, enc64, True, True).backward()
    tag = "tail cfg3 (tail_train_cfg)"
    _check_call(c, ref_cfg, tag, True, True)
    _check_params([p.grad for p in ep], [torch.zeros_like(p) for p in ep], enc64, tag + " enc", True)
    for k, (dp, d64) in enumerate(zip(dps, dec64)):
        _check_params([p.grad for p in dp], [torch.zeros_like(p) for p in dp], d64, f"{tag} dec{k}", False)


# ---- EncTailFn alone ---------------------------------------------------------------------------------------------------------------
ENC_CASES = [(1, 1, 1, 16), (4, 8, 16, 48), (6, 3, 5, 16), (12, 5, 13, 16)]      # D, n_img, Hp, Wp


@pytest.mark.parametrize("pixel", [True, False], ids=["pixel_wgrad_in_kernel", "pixel_wgrad_immediate"])
@pytest.mark.parametrize("D,n_img,Hp,Wp", ENC_CASES)
def test_enc_tail_against_float64(dev, monkeypatch, D, n_img, Hp, Wp, pixel):
    """The initial window's frames through the tail kernels' encoder half (n_ord = 0): z and the encoder's six gradients.  The frames
    are bf16-exact, so the kernel's first rounding is not part of the comparison."""
    from tante_amd import autograd as A
    monkeypatch.setattr(A, "PIXEL_WGRAD_IN_KERNEL", pixel)
    gen = torch.Generator().manual_seed(100 * D + n_img)
    enc, _ = _modules(dev, 0, D, Hp, Wp, gen)
    cfg = _cfg(n_img, 1, Hp, Wp, D, [], enc, [], True)
    ep = _enc_params(enc)
    frames = randn((n_img, D, 8 * Hp, 8 * Wp), gen).to(torch.bfloat16).to(torch.float32).to(dev)
    Gz = randn((n_img * Hp * Wp, 256), gen).to(dev)
    z = A.EncTailFn.apply(frames, cfg, *ep)
    A.run_backward((z * Gz).sum())
    torch.cuda.synchronize()
    enc64 = _ref_params(ep, dev)
    z64 = ref_enc(frames.double(), enc64).reshape(-1, 256)
    (z64 * Gz.double()).sum().backward()
    tag = f"enc_tail D{D} n{n_img} {Hp}x{Wp} {'in-kernel' if pixel else 'immediate'}"
    close(z, z64, tag + " z", BAR_ENC_Z)
    _check_params([p.grad for p in ep], [torch.zeros_like(p) for p in ep], enc64, tag, True)


# ---- a second backward over a retained graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", ["TailFn", "EncTailFn"])
def test_tail_second_backward_is_a_clear_error(dev, node):
    """Both nodes free their saved activations in their first backward: a second one must say so (and how to avoid it), not die on a
    None subscript."""
    from tante_amd import autograd as A
    gen = torch.Generator().manual_seed(9)
    enc, decs = _modules(dev, 1, 4, 1, 16, gen)
    if node == "TailFn":
        cfg = _cfg(1, 1, 1, 16, 4, [1.0], enc, decs, True)
        loss = _Call(dev, cfg, gen).run(cfg, True, True)
    else:
        cfg = _cfg(1, 1, 1, 16, 4, [], enc, [], True)
        loss = A.EncTailFn.apply(randn((1, 4, 8, 128), gen).to(dev), cfg, *_enc_params(enc)).sum()
    with A.backward_scope():
        loss.backward(retain_graph=True)
        with pytest.raises(RuntimeError, match=f"{node}: the fused training tail.*TANTE_TRAIN_FUSED_TAIL"):
            loss.backward()


# ---- TaylorFn alone (fp32) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_out,orders", [(1, 1, 1), (4, 3, 3), (2, 8, 8)])
@pytest.mark.parametrize("fshape", [(1, 2, 2), (3, 7, 20)], ids=["frame4", "frame420"])
def test_taylor_against_float64(dev, fshape, T, n_out, orders):
    """The Taylor sum of every non-fused path (fp32 compute, order > 3, more than one output frame): forward, dinp (the last frame; the
    earlier frames exactly zero) and every derivative's gradient."""
    from tante_amd.autograd import TaylorFn
    B, dt = 3, 0.37
    gen = torch.Generator().manual_seed(T * 100 + n_out * 10 + orders + fshape[-1])
    inp = randn((B, T, *fshape), gen).to(dev).requires_grad_()
    ds = [randn((B, 1, *fshape), gen).to(dev).requires_grad_() for _ in range(orders)]
    G = randn((B, n_out, *fshape), gen).to(dev)
    out = TaylorFn.apply(inp, dt, n_out, *ds)
    (out * G).sum().backward()
    i64, d64 = inp.detach().double().requires_grad_(), [d.detach().double().requires_grad_() for d in ds]
    o64 = ref_taylor(i64, dt, n_out, d64)
    (o64 * G.double()).sum().backward()
    tag = f"taylor frame{math.prod(fshape)} T{T} n_out{n_out} orders{orders}"
    close(out, o64, tag + " out", (F32_REL, F32_MAX), "fp32")
    assert torch.count_nonzero(inp.grad[:, :-1]) == 0, tag + ": earlier frames of dinp written"
    close(inp.grad[:, -1], i64.grad[:, -1], tag + " dinp", (F32_REL, F32_MAX), "fp32")
    for k, (d, r) in enumerate(zip(ds, d64)):
        close(d.grad, r.grad, f"{tag} dd{k + 1}", (F32_REL, F32_MAX), "fp32")
