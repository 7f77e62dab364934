"""GPU: stages.deconv_nhwc / deconv_nhwc_train, the kernel = stride = P transposed convolution on channels-last rows, alone against float64
F.conv_transpose2d on both routes (the scatter GEMM up to 512 input channels, the K-chunked tap GEMM + tante_col2im_nhwc beyond) in fp32
and bf16: the output, and the gradients of the rows, the weight and the bias.  Cin 30 is the width of the g21 Upsample fixture (scatter),
576 the wide DPOT model's (the one width the suite runs the tap route at); n 2, a 2 x 3 grid and Cout 3 are the smallest odd, non-square
shapes.  The bars are those of test_hip_convnext.close, which the Upsample and the DPOT out_layer tests apply to the same routes."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_convnext import close, compute_of

pytestmark = pytest.mark.gpu

N, HI, WI, COUT = 2, 2, 3, 3
CASES = [(30, 2), (576, 2), (30, 4)]        # (Cin, P); P = 4 is DPOT's out_layer form, on the scatter route
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def case(cin, P):
    """-> (rows (n Hi Wi, Cin), weight (Cin, Cout, P, P), bias, dout (n, P Hi, P Wi, Cout), and in float64 the channels-last output and
    the three gradients), computed once per shape."""
    key = (cin, P)
    if key not in _REF:
        gen = torch.Generator().manual_seed(97 * cin + P)
        rows = torch.randn(N * HI * WI, cin, generator=gen)
        w = torch.randn(cin, COUT, P, P, generator=gen) / cin ** 0.5
        b = torch.randn(COUT, generator=gen)
        dout = torch.randn(N, P * HI, P * WI, COUT, generator=gen)
        r64, w64, b64 = (t.double().requires_grad_(True) for t in (rows, w, b))
        y64 = F.conv_transpose2d(r64.view(N, HI, WI, cin).permute(0, 3, 1, 2), w64, b64, stride=P).permute(0, 2, 3, 1)
        g64 = torch.autograd.grad(y64, [r64, w64, b64], dout.double())
        _REF[key] = (rows, w, b, dout, y64.detach(), g64)
    return _REF[key]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,P", CASES)
def test_deconv_nhwc_against_float64(dev, cin, P, mode):
    """The inference form as Upsample and AViT call it: rows in the activation dtype, no activation, fp32 out."""
    from tante_amd import kernels as K
    from tante_amd import stages as S
    rows, w, b, _, y64, _ = case(cin, P)
    compute = compute_of(mode)
    packed = S.pack_deconv_nhwc(w.to(dev), b.to(dev), P, compute)
    assert isinstance(packed, K.PackedWeight) == (cin <= S.KMAX)
    y = S.deconv_nhwc(rows.to(dev).to(K.act_torch_dtype(compute)), packed, b.to(dev), N, HI, WI, P, COUT)
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, P * HI, P * WI, COUT)
    close(y, y64, mode, f"deconv_nhwc Cin {cin} P {P}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_deconv_nhwc_gelu_in_the_activation_dtype(dev, mode):
    """DPOT's out_layer form: fp32 rows, P = 4, the erf GELU in the scatter GEMM's epilogue, the image in the activation dtype."""
    from tante_amd import _lib as L
    from tante_amd import kernels as K
    from tante_amd import stages as S
    cin, P = 30, 4
    rows, w, b, _, y64, _ = case(cin, P)
    compute = compute_of(mode)
    adt = K.act_torch_dtype(compute)
    y = S.deconv_nhwc(rows.to(dev), S.pack_deconv_nhwc(w.to(dev), b.to(dev), P, compute), b.to(dev), N, HI, WI, P, COUT, adt, L.ACT_GELU_ERF)
    assert y.dtype == adt
    close(y, F.gelu(y64), mode, f"deconv_nhwc + GELU Cin {cin} P {P}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,P", CASES)
def test_deconv_nhwc_train_against_float64(dev, cin, P, mode):
    """The training form, pre-activation in fp32 as upsample_train asks for it: the forward, and the gradients of the rows, the weight and
    the bias against float64 autograd."""
    from tante_amd import kernels as K
    from tante_amd import stages as S
    rows, w, b, dout, y64, g64 = case(cin, P)
    compute = compute_of(mode)
    rd = rows.to(dev).requires_grad_(True)
    wd, bd = torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(b.to(dev))
    y = S.deconv_nhwc_train(rd.to(K.act_torch_dtype(compute)), wd, bd, N, HI, WI, P, compute, torch.float32)
    grads = torch.autograd.grad(y, [rd, wd, bd], dout.to(dev))
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, P * HI, P * WI, COUT)
    close(y, y64, mode, f"deconv_nhwc_train Cin {cin} P {P}: forward")
    for name, a, want in zip(("d_rows", "d_weight", "d_bias"), grads, g64):
        assert a.dtype == torch.float32 and a.shape == want.shape
        close(a, want, mode, f"deconv_nhwc_train Cin {cin} P {P}: {name}")
