"""GPU: the adaptive-step tail (csrc/adaptive_tail.hip) -- tante_adaptive_rt and tante_head_adaptive alone against float64, the
deg=False model and rollout on them against the CPU oracle, the launch accounting of a call, and the routes that must not change.

Kernel-alone bars are not derivable (bf16 intermediate rounding, another accumulation order), so each kernel test also runs the chain
the kernel replaces (K.linear x 3 + rt_reduce; film_apply + head_fused per order: the TANTE_ADAPTIVE_TAIL=0 route) on the same inputs
against the same float64 restatement and holds the new kernel to 2 x that error (the factor is for summation order only); both values go
through record_parity.  Model bars: R_t under close(.., "bf16") and the frames by their derivative part, rel_err(y - last, ref - last) <
1e-2, the bar of test_g8_rollout -- under the condition, asserted on the ORACLE's values alone, that every R_t lies at least 0.1 from an
integer (a frame-count flip would turn a rounding difference into a shape difference).  The fixtures (seed, amplitudes) were chosen by
running the oracle on the CPU; the assertion stays so that a drifting fixture fails loudly."""
import functools
import math

import pytest
import torch

from conftest import rel_err, max_rel, record_parity
from test_hip_train_nodes import Spy

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "bf16": 1e-2}
EP = 1.001
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def close(a, b, mode, note="", scale=1.0):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    r, m = rel_err(a, b), max_rel(a, b)
    print(f"[adaptive] {note}: rel={r:.3e} max={m:.3e} (tol {TOL[mode] * scale:.1e})")
    record_parity(r, m, TOL[mode] * scale, mode, note)
    assert r < TOL[mode] * scale and m < TOL[mode] * scale * 2, f"{note}: rel={r:.3e} max={m:.3e} (tol {TOL[mode] * scale:.1e})"
    return r


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


class _Switch:
    """TANTE_ADAPTIVE_TAIL set for a with-block, restored afterwards."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import tante_amd
        self.old = tante_amd.get_option("TANTE_ADAPTIVE_TAIL")
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", int(self.on))

    def __exit__(self, *a):
        import tante_amd
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", int(self.old))


# ---------------------------------------------------------------------------------------------------------------------------------
# tante_adaptive_rt alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _rt_setup(dev, C_, n_ord, B, Hp, Wp, case):
    """n_ord interprators + modifiers and the streams they read at the last slot of a (B, T = 4, HW, C) stream; the last layer is scaled so
    that the tokens spread over the clamp range ("mixed") or all land above it ("high")."""
    import tante_amd
    HW = Hp * Wp
    torch.manual_seed(7 * C_ + 13 * n_ord + HW)
    ips = [tante_amd.interprator(C_, HW) for _ in range(n_ord)]
    mods = [tante_amd.film(C_, in_dim=1) for _ in range(n_ord)]
    xs = [torch.randn(B, 4, HW, C_) for _ in range(n_ord)]
    with torch.no_grad():
        for ip, x in zip(ips, xs):
            if case == "mixed":      # the raw token scalars re-centred on the middle of [0, out_T - 1] = [0, 0.5], spread 0.35
                t = ip.interprete(x[:, -1])
                s = 0.35 / float(t.std())
                ip.interprete[4].weight.mul_(s)
                ip.interprete[4].bias.copy_((ip.interprete[4].bias - t.mean()) * s + 0.25)
            else:
                ip.interprete[4].bias.fill_(100.0)
    return ips, mods, xs


def _rt_float64(ips, xs, out_T):
    """interprator (tante.py:191-201) in float64 on the bf16-rounded operands; the two hidden activations rounded to bf16 as both
    routes store them.  -> (r (n_ord, B), per-token t list)."""
    rs, ts = [], []
    for ip, x in zip(ips, xs):
        l1, l2, l3 = ip.interprete[0], ip.interprete[2], ip.interprete[4]
        h = bf(x[:, -1])
        h = bf(torch.relu(h @ bf(l1.weight).t() + l1.bias.double()).float())
        h = bf(torch.relu(h @ bf(l2.weight).t() + l2.bias.double()).float())
        t = (h @ bf(l3.weight).t() + l3.bias.double())[..., 0]
        c = t + torch.relu(-t) - torch.relu(t - (out_T - 1))
        rs.append((c.mean(dim=1) + float(torch.tensor(EP, dtype=torch.float32))).detach())
        ts.append(t.detach())
    return torch.stack(rs), ts


@pytest.mark.parametrize("case", ["mixed", "high"])
@pytest.mark.parametrize("B,Hp,Wp", [(1, 4, 4), (3, 4, 12)])
@pytest.mark.parametrize("n_ord", [1, 3])
@pytest.mark.parametrize("C_", [128, 256])
def test_adaptive_rt_kernel(dev, C_, n_ord, B, Hp, Wp, case):
    """Every order's step-size head in one entry, rows read by stride from the last slot of a (B, 4, HW, C) stream.  (1, 4, 4): one tile
    per image, one workgroup; (3, 4, 12): three tiles per image, Hp != Wp, 144 rows = 9 tiles, so the last workgroup of 4 has dead waves.
    "mixed": tokens clamp at 0, at out_T - 1 and in between (asserted on the float64 values); "high": every token saturates and R must
    equal (out_T - 1) + ep exactly.  r against float64 at 2 x the error of the chain it replaces; R = mean_k r and count = floor(R)
    exactly; the FiLM rows against the modifier's table kernel on the same r; two runs give the same bits."""
    from tante_amd import kernels as K, _lib as L
    out_T, HW = 1.5, Hp * Wp
    ips, mods, xs = _rt_setup(dev, C_, n_ord, B, Hp, Wp, case)
    ref, ts = _rt_float64(ips, xs, out_T)
    if case == "mixed":
        t = torch.cat([v.reshape(-1) for v in ts])
        assert (t < 0).any() and (t > out_T - 1).any() and ((t > 0) & (t < out_T - 1)).any(), "the fixture must put tokens at both clamps and between them"
    else:
        assert all((v > out_T - 1).all() for v in ts)
    for m_ in ips + mods:
        m_.to(dev)
    xd = [x.to(dev) for x in xs]
    addr = (HW, 4 * HW * C_, C_, 3 * HW * C_)
    film_pack = K.pack_adaptive_film([(m_.condition_to_scale[0].weight, m_.condition_to_scale[0].bias, m_.condition_to_scale[2].weight,
                                       m_.condition_to_scale[2].bias, m_.condition_to_shift[0].weight, m_.condition_to_shift[0].bias,
                                       m_.condition_to_shift[2].weight, m_.condition_to_shift[2].bias) for m_ in mods])
    streams = [ip.packed_rt() for ip in ips]
    with torch.no_grad():
        r, R, cnt, fa, fs = K.adaptive_rt(xd, *addr, B, Hp, Wp, C_, streams, film_pack, out_T, EP)
        r2, R2, cnt2, fa2, fs2 = K.adaptive_rt(xd, *addr, B, Hp, Wp, C_, streams, film_pack, out_T, EP)
        old = torch.stack([ip.forward_tokens(x, B, out_T, L.BF16, *addr) for ip, x in zip(ips, xd)])      # K.linear x 3 + rt_reduce
        tabs = [m_.tables(r[k].contiguous()) for k, m_ in enumerate(mods)]
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(R, R2) and torch.equal(cnt, cnt2) and torch.equal(fa, fa2) and torch.equal(fs, fs2)
    rc, Rc = r.cpu(), R.cpu()
    e_new, e_old = float((rc.double() - ref).abs().max()), float((old.cpu().double() - ref).abs().max())
    # the floor under 2 x e_old: one fp32 rounding of the mean and of the sum with ep (values < 2), for the cases where the old chain
    # happens to land on the float64 value
    floor_ = 2 * 2.0 ** -23
    print(f"[adaptive] rt kernel C={C_} K={n_ord} B={B} HW={HW} {case}: new={e_new:.3e} old chain={e_old:.3e}")
    record_parity(e_new, e_new, 2 * e_old + floor_, "bf16", f"adaptive_rt alone ({case}) vs float64: max abs error of r")
    record_parity(e_old, e_old, 2 * e_old + floor_, "bf16", f"linear x 3 + rt_reduce ({case}) vs float64: max abs error of r (sets the bar)")
    assert e_new <= 2 * e_old + floor_, (e_new, e_old)
    hi_ep = torch.tensor(out_T - 1, dtype=torch.float32) + torch.tensor(EP, dtype=torch.float32)
    if case == "high":
        assert torch.equal(rc, hi_ep.expand_as(rc)) and torch.equal(Rc, hi_ep.expand_as(Rc)), (rc, Rc, hi_ep)
    assert torch.equal(Rc, rc.double().mean(dim=0).float()), "R = mean_k r, formed in double"
    assert torch.equal(cnt.cpu(), torch.floor(Rc).to(torch.int32))
    for k in range(n_ord):
        close(fa[k], tabs[k][0], "fp32", f"adaptive_rt: FiLM scale rows of order {k} vs tante_film_table")
        close(fs[k], tabs[k][1], "fp32", f"adaptive_rt: FiLM shift rows of order {k} vs tante_film_table")


# ---------------------------------------------------------------------------------------------------------------------------------
# tante_head_adaptive alone
# ---------------------------------------------------------------------------------------------------------------------------------
HB, HHp, HWp = 3, 4, 12      # 144 rows: three 64-token groups, the last with three dead waves; Hp != Wp


@functools.lru_cache(maxsize=None)
def _head_setup(C_, D, n_ord):
    import tante_amd
    torch.manual_seed(5 * C_ + 3 * D + n_ord)
    md = tante_amd.TanteMetadata(n_fields=D, spatial_resolution=(HHp * 8, HWp * 8))
    decs = [tante_amd.dec_CNN(dset_metadata=md, embed_dim=C_, patch_scale=8, overlap_ratio=0.0) for _ in range(n_ord)]
    HW = HHp * HWp
    xs = [torch.randn(HB, 4, HW, C_) for _ in range(n_ord)]
    fa = 1.0 + 0.3 * torch.randn(n_ord, HB, C_)
    fs = 0.3 * torch.randn(n_ord, HB, C_)
    last = torch.randn(HB, D, HHp * 8, HWp * 8)
    # float64 composition: FiLM rows (the fp32 product both routes form, rounded to the bf16 operand) -> three transposed-conv stages on
    # bf16-rounded weights -> derivative fields D_k (B, D, H, W)
    from oracle import tante_oracle as O
    ders = []
    for k in range(n_ord):
        d = bf(xs[k][:, -1] * fa[k][:, None, :] + fs[k][:, None, :]).view(HB, 1, HHp, HWp, C_)
        w = {n: (bf(p) if n.endswith("weight") else p.detach().double()) for n, p in decs[k].state_dict().items()}
        ders.append(O.dec_cnn(w, d, 8, 0.0)[:, 0])
    return decs, xs, fa, fs, last, ders


def _taylor_ref(last, ders, dt, n):
    out = []
    for j in range(1, n + 1):
        o = last.double()
        for k, d in enumerate(ders):
            o = o + d * ((j * dt) ** (k + 1) / math.factorial(k + 1))
        out.append(o)
    return torch.stack(out, dim=1)      # (B, n, D, H, W)


@pytest.mark.parametrize("n_cap", [1, 3, 8])
@pytest.mark.parametrize("n_ord", [1, 2, 3])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("C_", [128, 256])
def test_head_adaptive_kernel(dev, C_, D, n_ord, n_cap):
    """Every order's derivative head and every frame's Taylor sum in one launch, against a float64 composition, with hand-written
    counts: rule 0 with count = [2, 7, 1] (every image gets min(2, n_cap) frames) and rule 1 with count = [1, 3, 2] (per image).  `out`
    is a strided slice of a larger NaN-filled buffer: frames past n_b and everything outside the slice must still hold the fill.  The
    written frames, by their derivative part, at 2 x the error of film_apply + head_fused per order on the same inputs."""
    from tante_amd import kernels as K
    dt = 0.5
    decs, xs, fa, fs, last, ders = _head_setup(C_, D, n_ord)
    HW, H, W = HHp * HWp, HHp * 8, HWp * 8
    frame = D * H * W
    for d_ in decs:
        d_.to(dev)
    xd = [x.to(dev) for x in xs]
    fad, fsd, lastd = fa.to(dev).contiguous(), fs.to(dev).contiguous(), last.to(dev).contiguous()
    addr = (HW, 4 * HW * C_, C_, 3 * HW * C_)
    coefs = torch.tensor([[(j * dt) ** (k + 1) / math.factorial(k + 1) for j in range(1, 9)] for k in range(n_ord)], dtype=torch.float32, device=dev)
    heads = [d_.packed_head() for d_ in decs]
    ref = _taylor_ref(last, ders, dt, n_cap)
    base = last.double()[:, None]
    # the chain this kernel replaces, n_cap frames for every image: sets the bar
    old = torch.empty(HB, n_cap, D, H, W, device=dev)
    with torch.no_grad():
        for k in range(n_ord):
            d3 = torch.empty(HB * HW, C_, device=dev)
            K.film_apply(xd[k], 3 * HW * C_, 4 * HW * C_, d3, HB * HW, C_, HW, fad[k].contiguous(), fsd[k].contiguous())
            K.head_fused(d3, HB * HW, 0, C_, 0, HB, HHp, HWp, C_, D, heads[k], old, old.stride(0),
                         [(j * dt) ** (k + 1) / math.factorial(k + 1) for j in range(1, n_cap + 1)], lastd if k == 0 else None, 0, frame)
    oldc = old.cpu().double()
    for rule, counts in ((0, [2, 7, 1]), (1, [1, 3, 2])):
        big = torch.full((HB, n_cap + 3, D, H, W), NAN, device=dev)
        out = big[:, 1: 1 + n_cap]
        cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        with torch.no_grad():
            K.head_adaptive(xd, *addr, HB, HHp, HWp, C_, D, heads, fad, fsd, cnt, bool(rule), coefs, n_cap, out, out.stride(0), lastd, 0, frame)
        torch.cuda.synchronize()
        got = big.cpu()
        assert torch.isnan(got[:, 0]).all() and torch.isnan(got[:, 1 + n_cap:]).all(), "outside the slice"
        num_n = num_o = den = 0.0
        for b in range(HB):
            nb = min(counts[b] if rule else counts[0], n_cap)
            assert torch.isnan(got[b, 1 + nb: 1 + n_cap]).all(), f"rule {rule}: image {b} must keep the fill past frame {nb}"
            g = got[b, 1: 1 + nb].double()
            assert torch.isfinite(g).all()
            num_n += float(((g - ref[b, :nb]) ** 2).sum())
            num_o += float(((oldc[b, :nb] - ref[b, :nb]) ** 2).sum())
            den += float(((ref[b, :nb] - base[b]) ** 2).sum())
        e_new, e_old = math.sqrt(num_n / den), math.sqrt(num_o / den)
        print(f"[adaptive] head kernel C={C_} D={D} K={n_ord} n_cap={n_cap} rule {rule}: new={e_new:.3e} old chain={e_old:.3e}")
        record_parity(e_new, e_new, 2 * e_old, "bf16", f"head_adaptive alone (rule {rule}) vs float64: derivative part")
        record_parity(e_old, e_old, 2 * e_old, "bf16", f"film_apply + head_fused per order (rule {rule}) vs float64: derivative part (sets the bar)")
        assert e_new <= 2 * e_old, (rule, e_new, e_old)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model on the two kernels, against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------
RES, D_, T_ = (32, 96), 3, 4
SEED = {256: 3, 128: 33}         # chosen on the CPU oracle: every R_t of every call below lies >= 0.2 from an integer
HEADS = {256: 8, 128: 4}
AMP = (0.2, 1.0, 5.0)            # per-sample input amplitudes: the samples get different step sizes


@functools.lru_cache(maxsize=None)
def _model_cpu(C_):
    """(model on the CPU, oracle weights, oracle cfg, input (3, T, D, H, W)).  The interprators' last layer is steepened as
    test_adaptive_rollout_batched_with_per_sample_frame_counts does (weight x 60, bias + 2.2)."""
    import tante_amd
    from oracle import tante_oracle as O
    seed = SEED[C_]
    torch.manual_seed(seed)
    md = tante_amd.TanteMetadata(n_fields=D_, spatial_resolution=RES)
    m = tante_amd.TANTE(in_T=T_, dset_metadata=md, taylor_order=2, attn_axes="THW-THW", n_head=HEADS[C_], embed_dim=C_, patch_scale=8,
                        frame_interval=0.5, dropout=0.0, deg=False).eval()
    with torch.no_grad():
        for it in m.interprators:
            it.interprete[4].weight.mul_(60.0)
            it.interprete[4].bias.add_(2.2)
    w = {k: v.detach().clone() for k, v in m.state_dict().items()}
    cfg = O.TanteCfg(T_, D_, RES, taylor_order=2, frame_interval=0.5, attn_axes="THW-THW", n_head=HEADS[C_], embed_dim=C_, patch_scale=8, deg=False)
    x = torch.randn(3, T_, D_, *RES, generator=torch.Generator().manual_seed(seed + 1000)) * torch.tensor(AMP).view(3, 1, 1, 1, 1)
    return m, w, cfg, x


@functools.lru_cache(maxsize=None)
def _oracle_call(C_, out_T):
    """-> (y, R_t) of the batch of three, and the three single-sample calls."""
    from oracle import tante_oracle as O
    _, w, cfg, x = _model_cpu(C_)
    with torch.no_grad():
        full = O.tante_forward(w, cfg, x, out_T)
        single = [O.tante_forward(w, cfg, x[i:i + 1], out_T) for i in range(3)]
    return full, single


def _margin_ok(rt, what):
    """The condition of every model bar, on the oracle's values alone."""
    m = float((rt - torch.round(rt)).abs().min())
    assert m >= 0.1, f"{what}: an oracle R_t lies {m:.3f} from an integer ({rt.tolist()}): the fixture drifted"


def _deriv_err(y, ref, last):
    return rel_err(y.detach().cpu() - last, ref - last)


@pytest.mark.parametrize("out_T", [1.5, 6.0])
@pytest.mark.parametrize("C_", [256, 128])
def test_adaptive_model_against_oracle(dev, C_, out_T):
    """C = 256 / 8 heads and C = 128 / 4 heads, THW-THW, T = 4, D = 3, 32 x 96 field (Hp, Wp = 4, 12): R_t and the frames of one call
    against oracle.tante_forward -- sample 0's count for the batch, then per_sample_counts against single-sample oracle calls -- and the
    same call with TANTE_ADAPTIVE_TAIL=0: same shapes, the two routes agree within the bf16 bar."""
    m, _, _, x = _model_cpu(C_)
    (y_ref, rt_ref), single = _oracle_call(C_, out_T)
    _margin_ok(rt_ref, "batched call")
    for _, r1 in single:
        _margin_ok(r1, "single-sample call")
    if out_T == 6.0:
        assert len(set(torch.floor(rt_ref).tolist())) > 1, "the fixture must give the samples different frame counts"
    m = m.to(dev).set_compute("bf16")
    assert m.adaptive_tail_route(out_T)
    xd = x.to(dev)
    last = x[:, -1:]
    with torch.no_grad():
        y, rt = m(xd, out_T)
        yp, rtp = m(xd, out_T, per_sample_counts=True)
        with _Switch(False):
            assert not m.adaptive_tail_route(out_T)
            y0, rt0 = m(xd, out_T)
            yp0, rtp0 = m(xd, out_T, per_sample_counts=True)
    assert y.shape == y_ref.shape == y0.shape and yp.shape == yp0.shape
    close(rt, rt_ref, "bf16", f"C={C_} out_T={out_T}: R_t vs oracle")
    e = _deriv_err(y, y_ref, last)
    record_parity(e, e, 1e-2, "bf16", f"C={C_} out_T={out_T}: frames vs oracle, derivative part")
    print(f"[adaptive] model C={C_} out_T={out_T}: derivative part vs oracle {e:.3e}; switch off {_deriv_err(y0, y_ref, last):.3e}")
    assert e < 1e-2, e
    close(rtp, rt_ref, "bf16", f"C={C_} out_T={out_T}: R_t (per_sample_counts) vs oracle")
    assert yp.shape[1] == int(torch.floor(rt_ref).max())
    for i, (yi, ri) in enumerate(single):
        n = math.floor(float(ri[0]))
        assert yi.shape[1] == n
        ei = _deriv_err(yp[i:i + 1, :n], yi, last[i:i + 1])
        record_parity(ei, ei, 1e-2, "bf16", f"C={C_} out_T={out_T}: sample {i} frames (per_sample_counts) vs single-sample oracle call")
        assert ei < 1e-2, (i, ei)
    # the two routes: bf16 rounding order only
    close(rt, rt0, "bf16", f"C={C_} out_T={out_T}: R_t, adaptive tail vs switch off")
    e0 = _deriv_err(y, y0.cpu(), last)
    record_parity(e0, e0, 1e-2, "bf16", f"C={C_} out_T={out_T}: frames, adaptive tail vs switch off, derivative part")
    assert e0 < 1e-2, e0
    for i in range(3):
        n = math.floor(float(rt_ref[i]))
        assert _deriv_err(yp[i:i + 1, :n], yp0[i:i + 1, :n].cpu(), last[i:i + 1]) < 1e-2


def test_adaptive_out_view_and_enc_cache(dev):
    """out= (a slice of a larger buffer) and enc_cache= on a deg=False call: the same frames as the plain call, bit for bit where the
    encoder ran in the same launches; frames past the count keep the fill; off the route both still raise."""
    m, _, _, x = _model_cpu(256)
    m = m.to(dev).set_compute("bf16")
    from tante_amd import kernels as K
    out_T, B = 6.0, 3
    n_cap = K.adaptive_n_cap(out_T)
    assert n_cap == 6
    HW, C_ = m.H_p * m.W_p, m.C
    buf = torch.full((B, T_ + n_cap + 2, D_, *RES), NAN, device=dev)
    buf[:, :T_] = x.to(dev)
    with torch.no_grad():
        y, rt = m(x.to(dev), out_T)
        y2, rt2 = m(buf[:, :T_], out_T, out=buf[:, T_: T_ + n_cap])
        n = y.shape[1]
        assert y2.shape == y.shape and y2.data_ptr() == buf[:, T_:].data_ptr()
        assert torch.equal(y2, y) and torch.equal(rt2, rt)
        assert torch.isnan(buf[:, T_ + n:]).all(), "frames past the count are not written"
        assert m.enc_cache_supported(out_T)
        z = torch.empty(T_, B, HW, C_, device=dev)
        m.encode_frames(buf[:, :T_], z)
        y3, rt3 = m(buf[:, :T_], out_T, enc_cache=(z, B * HW * C_, HW * C_))
        close(rt3, rt, "bf16", "enc_cache: R_t vs the plain call")
        e = _deriv_err(y3, y.cpu(), x[:, -1:])
        record_parity(e, e, 1e-2, "bf16", "enc_cache: frames vs the plain call, derivative part")
        assert y3.shape == y.shape and e < 1e-2, e
        with pytest.raises(ValueError, match="out must be"):
            m(buf[:, :T_], out_T, out=buf[:, T_: T_ + n_cap - 1])
        with _Switch(False):
            with pytest.raises(ValueError, match="out= is only meaningful"):
                m(buf[:, :T_], out_T, out=buf[:, T_: T_ + n_cap])
            with pytest.raises(RuntimeError, match="enc_cache"):
                m(buf[:, :T_], out_T, enc_cache=(z, B * HW * C_, HW * C_))


# ---------------------------------------------------------------------------------------------------------------------------------
# launch accounting
# ---------------------------------------------------------------------------------------------------------------------------------
TAIL_ENTRIES = ("tante_adaptive_rt", "tante_head_adaptive", "tante_gemm", "tante_rt_reduce", "tante_film_table", "tante_film_apply",
                "tante_head_fused", "tante_taylor")


def test_adaptive_tail_launch_accounting(dev, monkeypatch):
    """One deg=False call at K = 3.  New route: tante_adaptive_rt once (two launches inside), tante_head_adaptive once, and from the
    moment the rt entry is called no GEMM (the K.linear chain), no rt_reduce, no FiLM table / pass and no per-order head launch.  Switch
    off: the old counts -- three GEMMs, one reduction, one FiLM table and one FiLM pass per order, then one head launch per order."""
    import tante_amd
    from tante_amd import _lib as L
    torch.manual_seed(5)
    md = tante_amd.TanteMetadata(n_fields=2, spatial_resolution=(32, 32))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=3, attn_axes="T-H-W", n_head=4, embed_dim=128, patch_scale=8, frame_interval=0.5,
                        dropout=0.0, deg=False).to(dev).eval().set_compute("bf16")
    x = torch.randn(2, 4, 2, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        m(x, 4.0)                               # packs and cached tables exist before the count
        with _Switch(False):
            m(x, 4.0)
    spy = Spy(monkeypatch, entries=TAIL_ENTRIES)
    lib = L.lib()
    at_rt = {}
    counted = lib.tante_adaptive_rt

    def rt_entry(*a):
        at_rt.update(spy.n)
        return counted(*a)
    monkeypatch.setattr(lib, "tante_adaptive_rt", rt_entry)
    with torch.no_grad():
        y, rt = m(x, 4.0)
    assert spy.n["tante_adaptive_rt"] == 1 and spy.n["tante_head_adaptive"] == 1
    for e in ("tante_gemm", "tante_rt_reduce", "tante_film_table", "tante_film_apply", "tante_head_fused", "tante_taylor"):
        assert spy.n[e] == at_rt[e], (e, spy.n[e], at_rt[e])
    for e in ("tante_rt_reduce", "tante_film_table", "tante_film_apply", "tante_head_fused", "tante_taylor"):
        assert spy.n[e] == 0, e
    before = dict(spy.n)
    with torch.no_grad(), _Switch(False):
        y0, rt0 = m(x, 4.0)
    d = {e: spy.n[e] - before[e] for e in TAIL_ENTRIES}
    assert d["tante_adaptive_rt"] == 0 and d["tante_head_adaptive"] == 0
    assert d["tante_rt_reduce"] == 3 and d["tante_film_table"] == 3 and d["tante_film_apply"] == 3 and d["tante_head_fused"] == 3, d
    assert d["tante_gemm"] - (at_rt["tante_gemm"]) == 9, (d, at_rt)      # the backbones' own GEMMs are the same on both routes
    assert y.shape == y0.shape


# ---------------------------------------------------------------------------------------------------------------------------------
# rollout
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_rollout(per_sample):
    from oracle import tante_oracle as O
    _, w, cfg, x = _model_cpu(256)
    xin = x.permute(0, 1, 3, 4, 2).contiguous()
    sel = xin if per_sample else xin[1:3]
    batch = {"input": sel, "output": torch.zeros(sel.shape[0], 7, *RES, D_)}
    with torch.no_grad():
        return batch, O.rollout_adaptive(w, cfg, batch, 7, 6.0, per_sample)


def _calls_of(rts, B, n_steps):
    """The per-call frame counts of a sample-0-rule rollout, from its concatenated R_t."""
    counts, produced, i = [], 0, 0
    while produced < n_steps:
        n = math.floor(float(rts[i * B]))
        counts.append(n)
        produced += n
        i += 1
    assert len(rts) == B * len(counts)
    return counts


def test_adaptive_rollout_in_place(dev):
    """rollout_adaptive(m, batch, fmt, 7, 6.0, per_sample=False) at B = 2 against oracle.rollout_adaptive: every call's R_t and frames
    (each call's derivative part, against the call's own last input frame), encode_frames on exactly T + the re-fed frames (never T per
    call), the switch-off result's shapes; then per_sample=True at B = 3 (the batched per-sample form on the new forward)."""
    import tante_amd
    m, _, _, _ = _model_cpu(256)
    m = m.to(dev).set_compute("bf16")
    md = tante_amd.TanteMetadata(n_fields=D_, spatial_resolution=RES)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    batch, (y_ref, _, rt_ref) = _oracle_rollout(False)
    _margin_ok(rt_ref, "rollout, sample-0 rule")
    counts = _calls_of(rt_ref, 2, 7)
    gb = {k: v.to(dev) for k, v in batch.items()}
    encoded = []
    orig = m.encode_frames

    def spy_encode(frames, z):
        encoded.append(frames.shape[1])
        return orig(frames, z)
    m.encode_frames = spy_encode
    try:
        with torch.no_grad():
            y, yr, rt = tante_amd.rollout_adaptive(m, gb, fmt, 7, 6.0, per_sample=False)
    finally:
        del m.encode_frames
    assert sum(encoded) == T_ + sum(counts[:-1]), (encoded, counts)
    assert encoded[0] == T_ and len(encoded) == len(counts)
    assert y.shape == y_ref.shape == (2, 7, *RES, D_) and rt.shape == rt_ref.shape
    close(rt, rt_ref, "bf16", "in-place adaptive rollout: R_t of every call vs oracle")
    yc = y.cpu()
    prev_y = torch.cat([batch["input"][:, -1:], yc], dim=1)
    prev_r = torch.cat([batch["input"][:, -1:], y_ref], dim=1)
    t0 = 0
    for c, n in enumerate(counts):
        t1 = min(t0 + n, 7)
        e = rel_err(yc[:, t0:t1] - prev_y[:, t0:t0 + 1], y_ref[:, t0:t1] - prev_r[:, t0:t0 + 1])
        record_parity(e, e, 1e-2, "bf16", f"in-place adaptive rollout: call {c} ({t1 - t0} frames), derivative part vs oracle")
        print(f"[adaptive] rollout call {c}: frames {t0}..{t1 - 1} derivative part {e:.3e}")
        assert e < 1e-2, (c, e)
        t0 = t1
    with torch.no_grad(), _Switch(False):
        y0, yr0, rt0 = tante_amd.rollout_adaptive(m, gb, fmt, 7, 6.0, per_sample=False)
    assert y0.shape == y.shape and rt0.shape == rt.shape and yr0.shape == yr.shape
    close(rt, rt0, "bf16", "in-place adaptive rollout: R_t vs switch off")
    # the batched per-sample form (rule 1) on the new forward
    batch3, (y3_ref, _, rt3_ref) = _oracle_rollout(True)
    _margin_ok(rt3_ref, "rollout, per sample")
    with torch.no_grad():
        y3, _, rt3 = tante_amd.rollout_adaptive(m, {k: v.to(dev) for k, v in batch3.items()}, fmt, 7, 6.0, per_sample=True)
    assert y3.shape == y3_ref.shape == (3, 7, *RES, D_) and rt3.shape == rt3_ref.shape
    close(rt3, rt3_ref, "bf16", "batched per-sample adaptive rollout on the new forward: R_t vs oracle, in order")
    last3 = batch3["input"][:, -1:]
    i = 0
    for b in range(3):      # R_t comes back sample by sample, call by call: each call's frames against the frame the call started from
        t0, prev = 0, last3[b:b + 1]
        prev_r = prev
        while t0 < 7:
            n = math.floor(float(rt3_ref[i]))
            t1 = min(t0 + n, 7)
            e = rel_err(y3[b:b + 1, t0:t1].cpu() - prev, y3_ref[b:b + 1, t0:t1] - prev_r)
            record_parity(e, e, 1e-2, "bf16", f"batched per-sample adaptive rollout: sample {b}, frames {t0}..{t1 - 1}, derivative part")
            assert e < 1e-2, (b, t0, e)
            prev, prev_r = y3[b:b + 1, t1 - 1:t1].cpu(), y3_ref[b:b + 1, t1 - 1:t1]
            t0, i = t1, i + 1
    assert i == len(rt3_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# routes that must not change
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fp32", "embed32", "out_T9"])
def test_unchanged_routes_are_bit_equal(dev, monkeypatch, case):
    """fp32 compute, a width the kernels do not serve, and n_cap = 9: each goes down the old route with the switch at its default (the
    adaptive entries are never called) and gives the bits it gives with the switch off."""
    import tante_amd
    torch.manual_seed(21)
    C_, nh = (32, 2) if case == "embed32" else (128, 4)
    md = tante_amd.TanteMetadata(n_fields=1, spatial_resolution=(32, 32))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=2, attn_axes="TH-TW", n_head=nh, embed_dim=C_, patch_scale=8, frame_interval=0.5,
                        dropout=0.0, deg=False).to(dev).eval().set_compute("fp32" if case == "fp32" else "bf16")
    with torch.no_grad():
        for it in m.interprators:
            it.interprete[4].weight.mul_(60.0)
            it.interprete[4].bias.add_(2.2)
    out_T = 9.0 if case == "out_T9" else 6.0
    assert tante_amd.get_option("TANTE_ADAPTIVE_TAIL") is True and not m.adaptive_tail_route(out_T)
    x = (torch.randn(3, 4, 1, 32, 32, generator=torch.Generator().manual_seed(22)) * torch.tensor([0.3, 1.0, 4.0]).view(3, 1, 1, 1, 1)).to(dev)
    spy = Spy(monkeypatch, entries=("tante_adaptive_rt", "tante_head_adaptive"))
    with torch.no_grad():
        y, rt = m(x, out_T)
        yp, rtp = m(x, out_T, per_sample_counts=True)
        with _Switch(False):
            y0, rt0 = m(x, out_T)
            yp0, rtp0 = m(x, out_T, per_sample_counts=True)
        with pytest.raises(ValueError, match="out= is only meaningful"):
            m(x, out_T, out=torch.empty(3, 1, 1, 32, 32, device=dev))
    assert spy.n["tante_adaptive_rt"] == 0 and spy.n["tante_head_adaptive"] == 0
    assert y.shape[1] >= 1 and torch.equal(y, y0) and torch.equal(rt, rt0) and torch.equal(yp, yp0) and torch.equal(rtp, rtp0)
