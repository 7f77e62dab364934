#!/usr/bin/env python3
"""Time the UNetConvNext baseline (configs/unet_convnext_am.yaml: 256 x 256 x 11 fields, in_T 4, widths 15 / 30 / 60 / 120 / 240, 33
ConvNeXt blocks) at B = 1 and B = 4, bf16 and fp32, against a plain eager-torch composition of the same model from the same weights
(F.conv2d, F.layer_norm, F.linear, F.normalize; under bf16 autocast for the bf16 rows) -- there is no earlier HIP form of this model to
compare with.  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps forwards each, synchronised on
both sides.

The gate: before anything is timed the HIP output of either mode must be under its bar (1e-5 fp32 -- taken against the composition in
float64 is not affordable here, so 1e-4 against the composition's own fp32 evaluation, whose distance from float64 the suite bounds --
and 1e-2 bf16) from the eager composition's FP32 evaluation (--time-anyway: timed and marked gate_passed: false).  No ratio is promised:
the file reports what was measured, with the spread.

It also times ONE block per width on the stage's own image size, fused against modular, interleaved in one process (fused, modular,
fused, ... regions), in both modes.

    python tools/convnext_time.py [--steps 5] [--out profiles/convnext_time.json]

Writes the times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tante_amd  # noqa: E402
from afno_time import kernel_split, timed  # noqa: E402


def eager_block(blk, x):
    y = blk.dwconv(x).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (y.shape[-1],), blk.norm.weight, blk.norm.bias, blk.norm.eps)
    y = blk.pwconv2(F.gelu(blk.pwconv1(y)))
    if blk.gamma is not None:
        y = blk.gamma * y
    return x + y.permute(0, 3, 1, 2)


def eager_stage(st, x):
    if not isinstance(st.skip_proj, torch.nn.Identity):
        x = st.skip_proj(x)
    for blk in st.blocks:
        x = eager_block(blk, x)
    if not isinstance(st.resample, torch.nn.Identity):
        norm, conv = st.resample.block[0], st.resample.block[1]
        x = conv(F.normalize(x, p=2, dim=1, eps=norm.eps) * norm.weight)
    return x


def eager_forward(m, x):
    """models.UNetConvNext.forward from the mathematics, on m's parameters, as eager torch ops, channels first."""
    b, t, c, h, w = x.shape
    x = m.in_proj(x.reshape(b, t * c, h, w))
    skips = []
    for enc in m.encoder:
        skips.append(x)
        x = eager_stage(enc, x)
    x = eager_stage(m.neck, x)
    for j, dec in enumerate(m.decoder):
        if j > 0:
            x = torch.cat([x, skips[-j]], dim=1)
        x = eager_stage(dec, x)
    return m.out_proj(x).float().unsqueeze(1)


def rescale(m):
    """A default-initialised block contributes 1e-6 of its input: move the parameters as the fixtures do, or the gate would pass with
    every block deleted."""
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.split(".")[-1] == "gamma":
                p.copy_(0.5 * (1 + 0.1 * torch.randn_like(p)))
            elif ".norm." in k or ".block.0." in k:
                p.add_(0.1 * torch.randn_like(p))


def interleaved(steps_a, steps_b, steps, reps=7, ramp_s=0.3):
    """Median of `reps` regions of each of two steps, the regions interleaved a, b, a, b, ..."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        steps_a()
        steps_b()
        torch.cuda.synchronize()
    out = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((steps_a, steps_b)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t) / steps)
    res = []
    for r in out:
        r.sort()
        res.append({"us_median": round(1e6 * r[len(r) // 2], 2), "us_min": round(1e6 * r[0], 2), "us_max": round(1e6 * r[-1], 2)})
    return res


def block_ab(m, B, res, steps):
    """One block per width on its stage's image, fused against modular."""
    from tante_amd import _lib as L
    rows = []
    stages = list(m.encoder) + [m.neck]
    for i, st in enumerate(stages):
        blk = st.blocks[0]
        C_ = blk.dwconv.weight.shape[0]
        x = 0.4 * torch.randn(B, res[0] >> i, res[1] >> i, C_, device=blk.dwconv.weight.device)
        out = torch.empty_like(x)
        for mode, compute in (("bf16", L.BF16), ("fp32", L.F32)):
            with torch.no_grad():
                f = lambda: blk.run(x, compute, out, fused=True)        # noqa: E731
                g = lambda: blk.run(x, compute, out, fused=False)       # noqa: E731
                a, b = f().clone(), g().clone()
                agree = float((a - b).double().norm() / b.double().norm())
                tf, tm = interleaved(f, g, steps * 4)
            rows.append({"C": C_, "image": [res[0] >> i, res[1] >> i], "batch": B, "mode": mode, "fused": tf, "modular": tm,
                         "modular_over_fused_median": round(tm["us_median"] / tf["us_median"], 3), "fused_vs_modular_rel": agree})
            print(f"  block C {C_} {res[0] >> i} x {res[1] >> i} B {B} {mode}: fused {tf['us_median']} us, modular {tm['us_median']} us", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_time.json"))
    ap.add_argument("--time-anyway", action="store_true", help="time also when a HIP output misses its gate (recorded as gate_passed: false)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_convnext_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).eval()
    rescale(m)
    result = {"workload": {"config": "configs/unet_convnext_am.yaml", "bf16_gemm_groups": list(tante_amd.convnext.BF16_SITES),
                           "resolution": wl["spatial_resolution"], "n_fields": wl["n_fields"], "parameters": sum(p.numel() for p in m.parameters())},
              "device": torch.cuda.get_device_name(0), "batches": {}, "block_fused_vs_modular": []}
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
            n_hip, split_hip = kernel_split(hip_step)
            n_eager, split_eager = kernel_split(eager_step)
            spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
            entry[mode] = {"gate_passed": gate, "hip_vs_fp32_eager_rel": hip_rel, "eager_vs_fp32_eager_rel": eager_rel, "hip": hip, "eager_torch": eager,
                           "eager_over_hip_median": round(eager["ms_median"] / hip["ms_median"], 3), "spread_ms": round(spread, 4),
                           "launches_per_forward": {"hip": n_hip, "eager_torch": n_eager}, "kernels_hip": split_hip, "kernels_eager_torch": split_eager}
            print(f"B = {B} {mode}: HIP {hip['ms_median']} ms, eager torch {eager['ms_median']} ms, launches {n_hip} / {n_eager}", flush=True)
        result["batches"][str(B)] = entry
        result["block_fused_vs_modular"] += block_ab(m, B, wl["spatial_resolution"], args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {md_: {"hip_ms": v[md_]["hip"]["ms_median"], "eager_ms": v[md_]["eager_torch"]["ms_median"]} for md_ in v}
                      for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
