#!/usr/bin/env python3
"""Time the AttentionUNet baseline (configs/unet_att_am.yaml: 256 x 256 x 11 fields, in_T 4, depth 5, out_T 1, widths 64 .. 1024, 22
convolutions 3 x 3 and four attention gates) at B = 1 and B = 4, bf16 and fp32, against a plain eager-torch composition of the same
model from the same weights (the modules' own nn.Conv2d / nn.BatchNorm2d / nn.Upsample layers in eval mode, F.max_pool2d, torch.cat;
under bf16 autocast for the bf16 rows).  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps
forwards each, synchronised on both sides.

The gate: before anything is timed the HIP output of either mode must be under its bar (1e-5 fp32 is held against float64 by the suite;
float64 of this model is not affordable here, so 1e-4 against the composition's own fp32 evaluation, and 1e-2 bf16) from the eager
composition's FP32 evaluation (--time-anyway: timed and marked gate_passed: false).  No ratio is promised: the file reports what was
measured, with the spread.

It also times every distinct 3 x 3 convolution of the config -- (source form, Cin, Cout, image) -- tante_conv3x3_mfma against
tante_im2col + tante_gemm (with the pool / upsample / cat written out, as that route has them), and every gate, tante_attn_gate against
its modular route, interleaved in one process (new, old, new, ... regions), in both modes, with the matrix-pipe utilisation of the new
kernel worked out from its time (2 n H W 9 Cin Cout flop against 2.5 Pflop/s bf16, 157.3 Tflop/s fp32).

    python tools/unet_att_time.py [--steps 5] [--out profiles/unet_att_time.json]

Writes the times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward)."""
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
import tante_amd.unet_att as UA  # noqa: E402
from afno_time import kernel_split, timed  # noqa: E402
from convnext_time import interleaved  # noqa: E402

PEAK = {"bf16": 2.5e15, "fp32": 157.3e12}


def eager_gate(att, g, x):
    psi = att.psi(torch.relu(att.W_gate(g) + att.W_x(x)))
    return x * psi


def eager_forward(m, x):
    """models.AttentionUNet.forward from the mathematics, on m's own torch layers, as eager torch ops, channels first."""
    b, t, c, h, w = x.shape
    enc = [m.Conv1.conv(x.reshape(b, t * c, h, w))]
    for i in range(2, m.depth + 1):
        enc.append(getattr(m, f"Conv{i}").conv(F.max_pool2d(enc[-1], 2, 2)))
    d = enc[-1]
    for i in range(m.depth, 1, -1):
        d = getattr(m, f"Up{i}").up(d)
        s = eager_gate(getattr(m, f"Att{i}"), d, enc[i - 2])
        d = getattr(m, f"UpConv{i}").conv(torch.cat((s, d), dim=1))
    out = m.Conv(d).float()
    return out.reshape(b, c_out(m), m.out_T, h, w).permute(0, 2, 1, 3, 4)


def c_out(m):
    return m.dim_out // m.out_T


def move_norms(m):
    """A default-initialised BatchNorm is the identity in eval mode: move all four of its tensors, or the gate would pass with every norm
    deleted."""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(1.0 + 0.4 * (torch.rand_like(mod.weight) - 0.5))
                mod.bias.copy_(0.2 * (torch.rand_like(mod.bias) - 0.5))
                mod.running_mean.copy_(0.2 * (torch.rand_like(mod.running_mean) - 0.5))
                mod.running_var.copy_(1.0 + 0.5 * (torch.rand_like(mod.running_var) - 0.5))


def conv_sites(m, res):
    """Every distinct 3 x 3 convolution of the model: (label, conv, bn, cache, slot, form, source pixels, Ca, Cb)."""
    seen, out = set(), []

    def add(label, conv, bn, cache, slot, form, hs, ws, Ca, Cb):
        key = (form, hs, ws, Ca, Cb, conv.weight.shape[0])
        if key not in seen:
            seen.add(key)
            out.append((label, conv, bn, cache, slot, form, hs, ws, Ca, Cb))
    for i in range(1, m.depth + 1):
        blk = getattr(m, f"Conv{i}")
        h, w = res[0] >> (i - 1), res[1] >> (i - 1)
        cin = blk.conv[0].weight.shape[1]
        if i == 1:
            add("Conv1.0", blk.conv[0], blk.conv[1], blk._cache, "c0", UA.PLAIN, h, w, cin, 0)
        else:
            add(f"Conv{i}.0 pooled", blk.conv[0], blk.conv[1], blk._cache, "c0", UA.POOLED, 2 * h, 2 * w, cin, 0)
        add(f"Conv{i}.1", blk.conv[3], blk.conv[4], blk._cache, "c1", UA.PLAIN, h, w, blk.conv[3].weight.shape[1], 0)
    for i in range(m.depth, 1, -1):
        up, blk = getattr(m, f"Up{i}"), getattr(m, f"UpConv{i}")
        h, w = res[0] >> (i - 1), res[1] >> (i - 1)
        add(f"Up{i} upsampled", up.up[1], up.up[2], up._cache, "up", UA.UPSAMPLED, h, w, up.up[1].weight.shape[1], 0)
        half = blk.conv[0].weight.shape[1] // 2
        add(f"UpConv{i}.0 two sources", blk.conv[0], blk.conv[1], blk._cache, "c0", UA.PLAIN, 2 * h, 2 * w, half, half)
        add(f"UpConv{i}.1", blk.conv[3], blk.conv[4], blk._cache, "c1", UA.PLAIN, 2 * h, 2 * w, blk.conv[3].weight.shape[1], 0)
    return out


def conv_ab(m, B, res, steps):
    from tante_amd import _lib as L
    dev = m.Conv.weight.device
    rows = []
    for label, conv, bn, cache, slot, form, hs, ws, Ca, Cb in conv_sites(m, res):
        a = torch.randn(B, hs, ws, Ca, device=dev)
        b = torch.randn(B, hs, ws, Cb, device=dev) if Cb else None
        Cout = conv.weight.shape[0]
        H, W = (hs // 2, ws // 2) if form == UA.POOLED else (2 * hs, 2 * ws) if form == UA.UPSAMPLED else (hs, ws)
        flop = 2.0 * B * H * W * 9 * (Ca + Cb) * Cout
        for mode, compute in (("bf16", L.BF16), ("fp32", L.F32)):
            with torch.no_grad():
                f = lambda: UA._conv_bn_act(a, conv, bn, cache, slot, compute, form, b, mfma=True)        # noqa: E731
                g = lambda: UA._conv_bn_act(a, conv, bn, cache, slot, compute, form, b, mfma=False)       # noqa: E731
                ya, yb = f(), g()
                agree = float((ya - yb).double().norm() / yb.double().norm())
                n = max(2, min(4 * steps, int(steps * 2e9 / flop) + 2))
                tn, to = interleaved(f, g, n, ramp_s=0.15)
            util = flop / (tn["us_median"] * 1e-6) / PEAK[mode]
            rows.append({"site": label, "form": form, "Cin": [Ca, Cb], "Cout": Cout, "image": [H, W], "batch": B, "mode": mode, "mfma": tn, "im2col_gemm": to,
                         "im2col_over_mfma_median": round(to["us_median"] / tn["us_median"], 3), "mfma_vs_im2col_rel": agree, "gflop": round(flop / 1e9, 3),
                         "mfma_utilisation": round(util, 4)})
            print(f"  {label} {Ca}+{Cb} -> {Cout} {H} x {W} B {B} {mode}: mfma {tn['us_median']} us ({100 * util:.1f} % of peak), im2col + gemm "
                  f"{to['us_median']} us", flush=True)
    return rows


def gate_ab(m, B, res, steps):
    from tante_amd import _lib as L
    dev = m.Conv.weight.device
    rows = []
    for i in range(m.depth, 1, -1):
        att = getattr(m, f"Att{i}")
        C_ = att.W_gate[0].weight.shape[1]
        h, w = res[0] >> (i - 2), res[1] >> (i - 2)
        g_, x_ = torch.randn(B, h, w, C_, device=dev), torch.randn(B, h, w, C_, device=dev)
        for mode, compute in (("bf16", L.BF16), ("fp32", L.F32)):
            with torch.no_grad():
                f = lambda: att.run(g_, x_, compute, mfma=True)        # noqa: E731
                g = lambda: att.run(g_, x_, compute, mfma=False)       # noqa: E731
                agree = float((f() - g()).double().norm() / g().double().norm())
                tn, to = interleaved(f, g, 4 * steps, ramp_s=0.15)
            rows.append({"site": f"Att{i}", "C": C_, "image": [h, w], "batch": B, "mode": mode, "one_launch": tn, "modular": to,
                         "modular_over_one_launch_median": round(to["us_median"] / tn["us_median"], 3), "one_launch_vs_modular_rel": agree})
            print(f"  Att{i} C {C_} {h} x {w} B {B} {mode}: one launch {tn['us_median']} us, modular {to['us_median']} us", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_att_time.json"))
    ap.add_argument("--time-anyway", action="store_true", help="time also when a HIP output misses its gate (recorded as gate_passed: false)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_att_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).eval()
    move_norms(m)
    result = {"workload": {"config": "configs/unet_att_am.yaml", "bf16_groups": list(UA.BF16_SITES), "resolution": wl["spatial_resolution"],
                           "n_fields": wl["n_fields"], "parameters": sum(p.numel() for p in m.parameters())},
              "device": torch.cuda.get_device_name(0), "batches": {}, "conv_mfma_vs_im2col": [], "gate_one_launch_vs_modular": []}
    gates = {"fp32": 1e-4, "bf16": 1e-2}
    for B in args.batches:
        x = torch.randn(B, cfg["model"]["in_T"], wl["n_fields"], *wl["spatial_resolution"], device=dev)
        with torch.no_grad():
            ref = eager_forward(m, x).double()
        entry = {}
        for mode in ("bf16", "fp32"):
            m.set_compute(mode)

            def hip_step():
                with torch.no_grad():
                    return m(x)

            def eager_step():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
                    return eager_forward(m, x)

            a, b = hip_step().double(), eager_step().double()
            torch.cuda.synchronize()
            hip_rel, eager_rel = (float((u - ref).norm() / ref.norm()) for u in (a, b))
            gate = bool(hip_rel < gates[mode])
            print(f"B = {B} {mode}: against the fp32 eager composition: HIP {hip_rel:.3e} (gate {gates[mode]:.0e}: {'passed' if gate else 'MISSED'}), "
                  f"eager {eager_rel:.3e}", flush=True)
            if not gate and not args.time_anyway:
                raise SystemExit(f"B = {B} {mode}: the HIP output is {hip_rel:.3e} from the fp32 composition (>= {gates[mode]:.0e}): nothing timed")
            hip = timed(hip_step, args.steps)
            eager = timed(eager_step, args.steps)
            with tante_amd_option("TANTE_UNETATT_MFMA", 0):
                old = timed(hip_step, max(1, args.steps // 2), ramp_s=0.2)
            n_hip, split_hip = kernel_split(hip_step)
            n_eager, split_eager = kernel_split(eager_step)
            spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
            entry[mode] = {"gate_passed": gate, "hip_vs_fp32_eager_rel": hip_rel, "eager_vs_fp32_eager_rel": eager_rel, "hip": hip, "eager_torch": eager,
                           "hip_im2col_route": old, "eager_over_hip_median": round(eager["ms_median"] / hip["ms_median"], 3),
                           "im2col_route_over_hip_median": round(old["ms_median"] / hip["ms_median"], 3), "spread_ms": round(spread, 4),
                           "launches_per_forward": {"hip": n_hip, "eager_torch": n_eager}, "kernels_hip": split_hip, "kernels_eager_torch": split_eager}
            print(f"B = {B} {mode}: HIP {hip['ms_median']} ms, im2col route {old['ms_median']} ms, eager torch {eager['ms_median']} ms, launches "
                  f"{n_hip} / {n_eager}", flush=True)
        m.set_compute(None)
        result["batches"][str(B)] = entry
        result["conv_mfma_vs_im2col"] += conv_ab(m, B, wl["spatial_resolution"], args.steps)
        result["gate_one_launch_vs_modular"] += gate_ab(m, B, wl["spatial_resolution"], args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {md_: {"hip_ms": v[md_]["hip"]["ms_median"], "eager_ms": v[md_]["eager_torch"]["ms_median"]} for md_ in v}
                      for k, v in result["batches"].items()}))


class tante_amd_option:
    """`with tante_amd_option(name, value)`: a host switch set for the block and put back to 1."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        tante_amd.set_option(self.name, self.value)

    def __exit__(self, *exc):
        tante_amd.set_option(self.name, 1)


if __name__ == "__main__":
    main()
