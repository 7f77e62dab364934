#!/usr/bin/env python3
"""Where bf16 operands hurt AViT: the float64 restatement (tests/avit_ref.py) with the operands of chosen GEMM groups rounded to bf16,
on the CPU, against the same restatement with none rounded.  This is the experiment behind the per-site table of DESIGN 4.7 and behind
`tante_amd.avit.BF16_SITES`; it needs no GPU and no reference checkout.

    python tools/avit_bf16_sites.py            # the width-48 depth-2 fixture, the width-384 depth-1 model, the width-64 fixture

Rounding: activations and weights of a GEMM to bf16 (round to nearest even), products and sums exact (float64) -- the matrix pipe's
arithmetic up to its fp32 accumulation.  The stem's first convolution is rounded as the unfolded pair (fields, then its own weight), which
is the folded convolution's rounding to first order.  Groups: stem0 / stem1 / stem2, the temporal and spatial input_head (qkv; `.v`: its
v rows only), both output_heads, fc1, fc2, head0 / head1 / head2."""
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avit_ref as R  # noqa: E402
from test_avit_cpu import keyed_golden  # noqa: E402

ALL = {"stem0", "stem1", "stem2", "t.qkv", "s.qkv", "t.out", "s.out", "fc1", "fc2", "head0", "head1", "head2"}
ROUNDED = set()          # the groups whose operands are rounded in the current evaluation ("t.qkv.v" / "s.qkv.v": the v rows only)
_lin, _conv, _deconv = R._lin, R.conv, R.deconv


def rb(t):
    return t.float().bfloat16().double()


def group_of(prefix):
    side = "t." if "temporal" in prefix else "s."
    for tail, name in (("input_head", side + "qkv"), ("output_head", side + "out"), ("fc1", "fc1"), ("fc2", "fc2")):
        if prefix.endswith(tail):
            return name
    raise KeyError(prefix)


def lin(x, sd, p):
    g = group_of(p)
    w = sd[p + ".weight"].double()
    w = w.reshape(w.shape[0], -1)
    if g in ROUNDED:
        return rb(x) @ rb(w).T + sd[p + ".bias"].double()
    if g + ".v" in ROUNDED:
        hd3 = 3 * sd[p.replace("input_head", "qnorm.weight")].shape[0]
        is_v = (torch.arange(w.shape[0]) % hd3) >= 2 * hd3 // 3
        return torch.where(is_v, rb(x) @ rb(w).T, x @ w.T) + sd[p + ".bias"].double()
    return _lin(x, sd, p)


def conv(x, w):
    g = "stem1" if w.shape[0] == w.shape[1] else "stem2"
    return _conv(rb(x), rb(w)) if g in ROUNDED else _conv(x, w)


def deconv(x, w, b=None):
    g = "head2" if b is not None else ("head1" if w.shape[0] == w.shape[1] else "head0")
    return _deconv(rb(x), rb(w), b) if g in ROUNDED else _deconv(x, w, b)


def stem(xn, sd, p_bag="space_bag.", p="embed.in_proj."):
    c = xn.shape[-1]
    wb = sd[p_bag + "weight"].double()
    r = rb if "stem0" in ROUNDED else (lambda t: t.double())
    z = math.sqrt(wb.shape[1] / c) * (r(xn) @ wb[:, :c].T + sd[p_bag + "bias"].double())
    z = R.gelu(R.rms_norm(_conv(z, r(sd[p + "0.weight"])), sd[p + "1.weight"]))
    z = R.gelu(R.rms_norm(conv(z, sd[p + "3.weight"]), sd[p + "4.weight"]))
    return R.rms_norm(conv(z, sd[p + "6.weight"]), sd[p + "7.weight"])


R._lin, R.conv, R.deconv, R.stem = lin, conv, deconv, stem

QKV, QKV_V, OUT, FC, STEM, HEAD = {"t.qkv", "s.qkv"}, {"t.qkv.v", "s.qkv.v"}, {"t.out", "s.out"}, {"fc1", "fc2"}, {"stem0", "stem1", "stem2"}, \
    {"head0", "head1", "head2"}
CASES = [("every GEMM", ALL), ("stem convolution 1", {"stem0"}), ("stem convolution 2", {"stem1"}), ("stem convolution 3", {"stem2"}),
         ("both input_heads", QKV), ("their v rows only", QKV_V), ("both output_heads", OUT), ("fc1 + fc2", FC), ("the head's three", HEAD),
         ("fc1 + fc2 + output_heads", FC | OUT), ("fc1 + fc2 + head", FC | HEAD), ("everything but stem and input_heads", ALL - STEM - QKV)]


def run(name, x, sd, heads, depth):
    global ROUNDED
    ROUNDED = set()
    want = R.model(x, sd, heads, depth)
    for label, groups in CASES:
        ROUNDED = set(groups)
        y = R.model(x, sd, heads, depth)
        print(f"{name}: bf16 operands at {label}: rel {float((y - want).norm() / want.norm()):.3e}", flush=True)


def wide_model():
    """The width-384, 6-head, depth-1 model of tests/test_hip_avit.py::test_wide_model_against_the_restatement."""
    import tante_amd
    gen = torch.Generator().manual_seed(2011)
    torch.manual_seed(2011)
    m = tante_amd.AViT(4, types.SimpleNamespace(n_fields=2), out_steps=1, embed_dim=384, num_heads=6, processor_blocks=1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                p.copy_(0.5 * (1 + 0.1 * torch.randn(p.shape, generator=gen)))
            elif "norm" in k or ("_proj." in k and p.dim() == 1):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
            elif "relative_attention_bias" in k:
                p.copy_(torch.randn(p.shape, generator=gen))
    return torch.randn(1, 2, 2, 32, 48, generator=gen), {k: v.clone() for k, v in m.state_dict().items()}


if __name__ == "__main__":
    torch.set_num_threads(8)
    g, sd, _ = keyed_golden("g20_avit_model_32x48_T4")
    run("width 48, hd 16, depth 2", g["x"], sd, 3, 2)
    x, sd = wide_model()
    run("width 384, hd 64, depth 1", x, sd, 6, 1)
    g, sd, _ = keyed_golden("g20_avit_model_64x64_T6")
    run("width 64, hd 64, depth 1", g["x"], sd, 1, 1)
