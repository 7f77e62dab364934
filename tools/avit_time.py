#!/usr/bin/env python3
"""Time the AViT baseline (configs/avit_am.yaml: 256 x 256 x 11 fields, in_T 4, width 384, 6 heads of 64, 12 space-time blocks, a 16 x 16
token grid) at B = 1 and B = 4, bf16, against a plain eager-torch composition of the same model from the same weights under bf16 autocast
(F.scaled_dot_product_attention, F.instance_norm, torch.std_mean, kernel = stride convolutions as reshapes + F.linear) -- there is no
earlier HIP form of this model to compare with.  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps
forwards each, synchronised on both sides.

The gate: before anything is timed the HIP bf16 output must be under the bf16 bar (1e-2) from the eager composition's FP32 evaluation
(--time-anyway: timed and marked gate_passed: false).  The autocast composition's own distance from it is recorded beside that, not as a
gate.  No ratio is promised: the file reports what was measured, with the spread.

    python tools/avit_time.py [--steps 5] [--out profiles/avit_time.json]

Writes both times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tante_amd  # noqa: E402
from afno_time import kernel_split, timed  # noqa: E402


def rms_norm(x, norm):
    """RMSInstanceNorm2d.forward on a channels-last image (n, H, W, C)."""
    std, _ = torch.std_mean(x, dim=(1, 2), keepdim=True)
    return x / (std + norm.eps) * norm.weight


def inst_norm(x, norm):
    """nn.InstanceNorm2d through torch's own kernel (which wants the channels on dim 1)."""
    return F.instance_norm(x.permute(0, 3, 1, 2), weight=norm.weight, bias=norm.bias, eps=norm.eps).permute(0, 2, 3, 1)


def conv(x, w):
    """kernel = stride convolution without bias on a channels-last image as a reshape + F.linear."""
    n, H, W, C = x.shape
    k = w.shape[-1]
    cols = x.reshape(n, H // k, k, W // k, k, C).permute(0, 1, 3, 5, 2, 4).reshape(n, H // k, W // k, C * k * k)
    return F.linear(cols, w.flatten(1))


def deconv(x, w, b=None):
    """kernel = stride transposed convolution on a channels-last image as F.linear + a pixel shuffle."""
    n, H, W, _ = x.shape
    co, k = w.shape[1], w.shape[-1]
    y = F.linear(x, w.flatten(1).t()).view(n, H, W, co, k, k).permute(0, 1, 4, 2, 5, 3).reshape(n, H * k, W * k, co)
    return y if b is None else y + b


def qkv_of(y, blk):
    he = blk.num_heads
    y = y.reshape(*y.shape[:-1], he, 3, y.shape[-1] // (3 * he))
    return blk.qnorm(y[..., 0, :]), blk.knorm(y[..., 1, :]), y[..., 2, :]


def eager_forward(m, x):
    """models.AViT.forward from the mathematics, on m's parameters, as eager torch ops, channels last."""
    b, T, c, h, w = x.shape
    x = x.permute(1, 0, 2, 3, 4)
    std, mean = torch.std_mean(x, dim=(0, -2, -1), keepdim=True)
    std = std + 1e-7
    z = ((x - mean) / std).permute(0, 1, 3, 4, 2).reshape(T * b, h, w, c)
    sb = m.space_bag
    z = (sb.dim_in / c) ** 0.5 * F.linear(z, sb.weight[:, :c], sb.bias)
    ip = m.embed.in_proj
    z = F.gelu(rms_norm(conv(z, ip[0].weight), ip[1]))
    z = F.gelu(rms_norm(conv(z, ip[3].weight), ip[4]))
    z = rms_norm(conv(z, ip[6].weight), ip[7])
    n, Hp, Wp, E = z.shape
    for blk in m.blocks:
        t, s = blk.temporal, blk.spatial
        q, k, v = qkv_of(F.linear(inst_norm(z, t.norm1), t.input_head.weight.flatten(1), t.input_head.bias).view(T, b, Hp, Wp, -1), t)
        a = F.scaled_dot_product_attention(*(u.permute(1, 2, 3, 4, 0, 5) for u in (q, k, v)), attn_mask=t.rel_pos_bias.table(T).to(q.dtype))
        a = a.permute(4, 0, 1, 2, 3, 5).reshape(n, Hp, Wp, E)
        z = z + t.gamma * F.linear(inst_norm(a, t.norm2), t.output_head.weight.flatten(1), t.output_head.bias)
        q, k, v = qkv_of(F.linear(rms_norm(z, s.norm1), s.input_head.weight.flatten(1), s.input_head.bias), s)
        xx = F.scaled_dot_product_attention(*(u.permute(0, 1, 3, 2, 4) for u in (q, k, v))).permute(0, 1, 3, 2, 4)
        xy = F.scaled_dot_product_attention(*(u.permute(0, 2, 3, 1, 4) for u in (q, k, v))).permute(0, 3, 1, 2, 4)
        a = ((xx + xy) / 2).reshape(n, Hp, Wp, E)
        z = z + s.gamma_att * F.linear(rms_norm(a, s.norm2), s.output_head.weight.flatten(1), s.output_head.bias)
        z = z + s.gamma_mlp * rms_norm(s.mlp.fc2(F.gelu(s.mlp.fc1(z))), s.mlp_norm)
    op = m.debed.out_proj
    k_ = min(T, 4)
    z = z[(T - k_) * b:]                # the head is per image: only the returned steps, as the HIP path decodes them
    z = F.gelu(rms_norm(deconv(z, op[0].weight), op[1]))
    z = F.gelu(rms_norm(deconv(z, op[3].weight), op[4]))
    y = deconv(z, m.debed.out_kernel[:, :c], m.debed.out_bias[:c]).view(k_, b, h, w, c).permute(0, 1, 4, 2, 3)
    return (y.float() * std + mean).permute(1, 0, 2, 3, 4)


def rescale(m):
    """A default-initialised block contributes 2e-6 of its input (layer scales of 1e-6): move the parameters as the fixtures do, or the
    gate would pass with every block deleted."""
    with torch.no_grad():
        for k, p in m.named_parameters():
            leaf = k.split(".")[-1]
            if leaf.startswith("gamma"):
                p.copy_(0.5 * (1 + 0.1 * torch.randn_like(p)))
            elif "norm" in k or ("_proj." in k and p.dim() == 1):
                p.add_(0.1 * torch.randn_like(p))
            elif "relative_attention_bias" in k:
                p.copy_(torch.randn_like(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avit_time.json"))
    ap.add_argument("--time-anyway", action="store_true", help="time also when the HIP bf16 output misses the gate (recorded as gate_passed: false)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "avit_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).eval().set_compute("bf16")
    rescale(m)
    result = {"workload": {"config": "configs/avit_am.yaml", "compute": "bf16", "bf16_gemm_groups": list(tante_amd.avit.BF16_SITES),
                           "resolution": wl["spatial_resolution"], "n_fields": wl["n_fields"], "parameters": sum(p.numel() for p in m.parameters())},
              "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in args.batches:
        x = torch.randn(B, cfg["model"]["in_T"], wl["n_fields"], *wl["spatial_resolution"], device=dev)

        def hip_step():
            with torch.no_grad():
                return m(x)

        def eager_step():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return eager_forward(m, x)

        with torch.no_grad():
            ref = eager_forward(m, x).double()
            m.set_compute("fp32")
            a32 = m(x).double()
            m.set_compute("bf16")
        a = hip_step().double()
        b = eager_step().double()
        torch.cuda.synchronize()
        hip32, hip16, eager16 = (float((u - ref).norm() / ref.norm()) for u in (a32, a, b))
        gate = bool(hip16 < 1e-2)
        print(f"B = {B}: against the fp32 eager composition: HIP fp32 {hip32:.3e}, HIP bf16 {hip16:.3e} (gate 1e-2: {'passed' if gate else 'MISSED'}), "
              f"eager autocast {eager16:.3e}", flush=True)
        if not gate and not args.time_anyway:
            raise SystemExit(f"B = {B}: the HIP bf16 output is {hip16:.3e} from the fp32 composition (>= 1e-2): nothing timed")
        hip = timed(hip_step, args.steps)
        eager = timed(eager_step, args.steps)
        n_hip, split_hip = kernel_split(hip_step)
        n_eager, split_eager = kernel_split(eager_step)
        spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
        result["batches"][str(B)] = {"gate_passed": gate, "hip_bf16_vs_fp32_eager_rel": hip16, "hip_fp32_vs_fp32_eager_rel": hip32,
                                     "eager_autocast_vs_fp32_eager_rel": eager16, "hip": hip, "eager_torch_autocast": eager,
                                     "eager_over_hip_median": round(eager["ms_median"] / hip["ms_median"], 3), "spread_ms": round(spread, 4),
                                     "launches_per_forward": {"hip": n_hip, "eager_torch": n_eager}, "kernels_hip": split_hip,
                                     "kernels_eager_torch": split_eager}
        print(f"B = {B}: HIP {hip['ms_median']} ms, eager torch {eager['ms_median']} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {"hip_ms": v["hip"]["ms_median"], "eager_ms": v["eager_torch_autocast"]["ms_median"]} for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
