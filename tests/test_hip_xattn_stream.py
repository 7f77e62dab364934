"""tante_cross_attention on the matrix pipe past the resident window: head dim 32, and any number of keys (the streamed form).

bf16 with D = 32 or 64 takes xattn_mfma_kernel<D, STREAM> (csrc/operators.hip): K and V resident in LDS while they fit 128 KiB (512 keys
at D = 64, 1024 at D = 32), 128-key chunks streamed through a 64 KiB LDS ring beyond that.  Every case asserts the route it expects
(kernels.cross_attention_route) before it compares, with nb = 2 samples and nh = 2 heads unless said otherwise.

1. parity with float64 softmax attention on the same bf16-rounded inputs, under the bars of test_hip_train_ops.py (relative L2 <= 5e-3,
   max-norm <= 1.6e-2, derived there from bf16 rounding; a CPU emulation of the kernel's scheme -- fp32 scores, 128-key online softmax,
   P rounded to bf16, fp32 accumulation, bf16 output -- gives 2.2e-3 and 2.2 - 3.5e-3 at these shapes);
2. every key counted exactly once: q = 0 makes P exactly 1, one-hot values make every sum exact, so o[d] = n_d / Lk to one bf16 rounding,
   while a skipped, duplicated or unmasked padded key moves an element by ~D / Lk >= 1.5 %;
3. one dominant key in the first, a middle and the last chunk: the output row is v[j*] (rescale of the running sums, K - V pairing across
   ring stages);
4. the streamed form equals the resident one bit for bit wherever both apply (TANTE_XATTN_STREAM = 1 forces it);
5. the training forward (CrossAttentionFn) and its gradients against float64 autograd;
6. CViT in bf16 against the oracle with 1 024 keys at D = 64 and 1 536 at D = 32.
"""
import math

import pytest
import torch

from conftest import record_parity, rel_err, max_rel
from test_hip_train_ops import close, ref_attention, randn, _xattn

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NB, NH = 2, 2
ULP = 2.0 ** -8          # one bf16 ulp, relative (8 significand bits)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class option:
    """Set a library option for a block and restore what it was."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from tante_amd import _lib
        self.old = _lib.get_option(self.name, 0)
        _lib.set_option(self.name, self.value)

    def __exit__(self, *exc):
        from tante_amd import _lib
        _lib.set_option(self.name, self.old)


def route(D, Lk):
    from tante_amd import kernels as K
    return K.cross_attention_route(BF16, D, Lk)


def attend(dev, q, k, v, layout="separate"):
    """q (nb | 1, nh, Lq, D), k / v (nb, nh, Lk, D), bf16 on the CPU -> o (nb, nh, Lq, D) bf16 on the CPU through K.cross_attention.
    separate: q (M, C) and k | v (M', 2C); shared: the same with ONE set of Lq query rows for every sample; packed: q | k | v (M, 3C)."""
    from tante_amd import kernels as K
    nb, nh, Lk, D = k.shape
    Lq, C = q.shape[2], nh * D

    def rows(t):
        return t.transpose(1, 2).reshape(-1, C)
    o = torch.full((nb * Lq, C), float("nan"), dtype=BF16, device=dev)
    if layout == "packed":
        buf = torch.cat([rows(q), rows(k), rows(v)], 1).to(dev)
        K.cross_attention(buf, buf[:, C:], buf[:, 2 * C:], o, nb, nh, D, Lq, Lk, 3 * C, 3 * C, C)
    else:
        qb, kv = rows(q).to(dev), torch.cat([rows(k), rows(v)], 1).to(dev)
        assert qb.shape[0] == (Lq if layout == "shared" else nb * Lq)
        K.cross_attention(qb, kv, kv[:, C:], o, nb, nh, D, Lq, Lk, C, 2 * C, C, shared_q=layout == "shared")
    torch.cuda.synchronize()
    return o.view(nb, Lq, nh, D).transpose(1, 2).cpu()


# ---- 1. parity with float64 ------------------------------------------------------------------------------------------------------------
PARITY = [  # D, Lq, Lk, layout, route
    (64, 129, 513, "separate", "stream"), (64, 1, 640, "separate", "stream"), (64, 300, 1300, "separate", "stream"),
    (64, 100, 641, "shared", "stream"), (64, 1024, 1024, "packed", "stream"),
    (32, 5, 4, "separate", "resident"), (32, 1, 1, "separate", "resident"), (32, 300, 130, "separate", "resident"),
    (32, 129, 1024, "separate", "resident"),
    (32, 129, 1025, "separate", "stream"), (32, 300, 2100, "separate", "stream"), (32, 1536, 1536, "packed", "stream"),
]


@pytest.mark.parametrize("D,Lq,Lk,layout,want", PARITY)
def test_parity_with_float64(dev, D, Lq, Lk, layout, want):
    assert route(D, Lk) == want
    g = torch.Generator().manual_seed(1000 * D + Lq + 7 * Lk)
    q = randn((1 if layout == "shared" else NB, NH, Lq, D), g, BF16)
    k, v = randn((NB, NH, Lk, D), g, BF16), randn((NB, NH, Lk, D), g, BF16)
    o = attend(dev, q, k, v, layout)
    ref = ref_attention(q.double(), k.double(), v.double())
    close(o, ref.expand(NB, -1, -1, -1), f"xattn {want} D{D} Lq{Lq} Lk{Lk} {layout} out")


# ---- 2. every key counted exactly once ---------------------------------------------------------------------------------------------------
COUNT = ([(64, Lk, False) for Lk in (513, 639, 640, 641, 1300)] + [(32, Lk, False) for Lk in (1025, 1151, 2100)] +
         [(D, Lk, True) for D in (64, 32) for Lk in (1, 127, 129)])


@pytest.mark.parametrize("D,Lk,forced", COUNT)
def test_every_key_counted_once(dev, D, Lk, forced):
    Lq = 33
    g = torch.Generator().manual_seed(D + Lk)
    q = torch.zeros(NB, NH, Lq, D, dtype=BF16)
    k = randn((NB, NH, Lk, D), g, BF16)
    v = torch.zeros(NB, NH, Lk, D, dtype=BF16)
    j = torch.arange(Lk)
    v[:, :, j, j % D] = 1.0
    with option("TANTE_XATTN_STREAM", int(forced)):
        assert route(D, Lk) == "stream"
        o = attend(dev, q, k, v).double()
    ref = (torch.bincount(j % D, minlength=D).double() / Lk).expand_as(o)
    err = ((o - ref).abs() / ref.clamp_min(1e-300)).where(ref > 0, (o - ref).abs())      # relative; absolute where the count is 0
    worst = float(err.max())
    print(f"count D{D} Lk{Lk}{' forced' if forced else ''}: worst relative error {worst:.3e} (bar {ULP:.3e})")
    record_parity(worst, worst, ULP, "bf16", f"xattn stream D{D} Lk{Lk}: every key once")
    assert worst <= ULP, f"D{D} Lk{Lk}: an element is off by {worst:.3e} of n_d / Lk (one bf16 ulp = {ULP:.3e})"


# ---- 3. one dominant key -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Lk", [(64, 1300), (32, 2100)])
def test_one_dominant_key(dev, D, Lk):
    assert route(D, Lk) == "stream"
    Lq = 33
    g = torch.Generator().manual_seed(3 * D + Lk)
    q = torch.zeros(NB, NH, Lq, D, dtype=BF16)
    q[..., 0] = 16.0                                          # score 256 / sqrt(D) at j*, 0 elsewhere: the other keys weigh < 1e-13 each
    v = randn((NB, NH, Lk, D), g, BF16)
    for js in (0, 127, 128, Lk - 129, Lk - 1):
        k = randn((NB, NH, Lk, D), g, BF16)
        k[..., 0] = 0.0
        k[:, :, js, 0] = 16.0
        o = attend(dev, q, k, v).double()
        ref = v[:, :, js].double()[:, :, None, :].expand_as(o)
        worst = float(((o - ref).abs() / ref.abs()).max())
        print(f"dominant D{D} Lk{Lk} j*={js}: worst relative error {worst:.3e} (bar {ULP:.3e})")
        record_parity(worst, worst, ULP, "bf16", f"xattn stream D{D} Lk{Lk}: dominant key {js}")
        assert worst <= ULP, f"D{D} Lk{Lk} j* = {js}: the output row is not v[j*] ({worst:.3e} relative, one bf16 ulp = {ULP:.3e})"


# ---- 4. streamed equals resident, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [1, 300])
@pytest.mark.parametrize("D,Lk", [(64, 1), (64, 127), (64, 128), (64, 130), (64, 256), (64, 512), (32, 130), (32, 1024)])
def test_streamed_equals_resident(dev, D, Lk, Lq):
    g = torch.Generator().manual_seed(5 * D + Lk + Lq)
    q, k, v = randn((NB, NH, Lq, D), g, BF16), randn((NB, NH, Lk, D), g, BF16), randn((NB, NH, Lk, D), g, BF16)
    assert route(D, Lk) == "resident"
    resident = attend(dev, q, k, v)
    with option("TANTE_XATTN_STREAM", 1):
        assert route(D, Lk) == "stream"
        streamed = attend(dev, q, k, v)
    assert torch.isfinite(resident.float()).all()
    assert torch.equal(streamed.view(torch.int16), resident.view(torch.int16)), f"D{D} Lk{Lk} Lq{Lq}: the two forms differ"


# ---- 5. the training forward ---------------------------------------------------------------------------------------------------------------
def test_training_forward_and_gradients(dev):
    assert route(64, 1300) == "stream"
    _xattn(dev, BF16, NB, NH, 64, 257, 1300, False, seed=64 + 257 + 1300)


# ---- 6. the model --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,heads,D", [((256, 256), 2, 64), ((256, 384), 4, 32)])
def test_cvit_against_oracle(dev, res, heads, D):
    """bf16 CViT with (res / 8) tokens against oracle.cvit_forward under north_star's bf16 bar (relative < 1e-2, max < 2e-2, as
    test_hip_parity.close).  The same model under TANTE_XATTN_VALU = 1 (every attention on the exact VALU kernel, what bf16 did at
    these sizes before the streamed form) is run too and its error recorded beside it."""
    import tante_amd
    from oracle import cvit_oracle as OC
    tokens = res[0] // 8 * (res[1] // 8)
    assert route(D, tokens) == "stream"
    kw = dict(out_steps=2, patch_size=(1, 8, 8), grid_size=(16, 16), latent_dim=64, emb_dim=128, depth=1, num_heads=heads, dec_emb_dim=128,
              dec_num_heads=heads, dec_depth=1, num_mlp_layers=1, mlp_ratio=1, eps=300.0)
    torch.manual_seed(17 + D)
    m = tante_amd.CViT(2, tante_amd.TanteMetadata(n_fields=2, spatial_resolution=res), **kw).to(dev).eval().set_compute("bf16")
    g = torch.Generator().manual_seed(D)
    x = torch.randn(2, 2, 2, *res, generator=g)
    coords = torch.rand(512, 2, generator=g)
    w = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = OC.cvit_forward(w, OC.CvitCfg(2, 2, res, **kw), x, coords)
        y = m(x.to(dev), coords.to(dev)).float().cpu()
        with option("TANTE_XATTN_VALU", 1):
            assert route(D, tokens) == "valu"
            y_valu = m(x.to(dev), coords.to(dev)).float().cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    r, mx = rel_err(y, ref), max_rel(y, ref)
    rv, mv = rel_err(y_valu, ref), max_rel(y_valu, ref)
    print(f"CViT {res} D{D} {tokens} keys: matrix pipe rel {r:.3e} max {mx:.3e}; forced VALU rel {rv:.3e} max {mv:.3e} (bars 1e-2 / 2e-2)")
    record_parity(rv, mv, 1e-2, "bf16", f"CViT {res} D{D} {tokens} keys, attention forced to the VALU kernel")
    record_parity(r, mx, 1e-2, "bf16", f"CViT {res} D{D} {tokens} keys, streamed attention")
    assert r < 1e-2 and mx < 2e-2, f"rel={r:.3e} max={mx:.3e} (forced VALU: rel={rv:.3e} max={mv:.3e})"
