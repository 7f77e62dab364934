#!/usr/bin/env python3
"""Time the UNO baseline (configs/uno_am.yaml: 256 x 256 x 11 fields, in_T 4, width 38, factor 1, seven resampling spectral operator
blocks, 242 MB of complex fp32 spectral weights) at B = 1 and B = 4, bf16 and fp32, against a plain eager-torch composition of the same
model from the same weights on the same GPU: torch.fft.rfft2 / irfft2 with a zero-filled out_ft, two einsums, the module's own nn.Conv2d,
F.interpolate(bicubic, align_corners, antialias) and torch.cat, under bf16 autocast for the bf16 rows (the transforms and the resize of
the composition take fp32 there, as autocast leaves them).  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed
regions of --steps forwards each, synchronised on both sides.

The gate: before anything is timed the HIP output of either mode must be under its bar (1e-5 fp32 is held against float64 by the suite;
float64 of this model is not affordable here, so 1e-4 against the composition's own fp32 evaluation, and 1e-2 bf16) from the eager
composition's FP32 evaluation (--time-anyway: timed and marked gate_passed: false).  The spectral weights are scaled per block as the
fixtures scale them (at the default initialisation the spectral path is a few per cent of the pointwise one and the gate would not see
it).  No ratio is promised: the file reports what was measured, with the spread.

It also times, per block, the mode-mix launch alone (tante_uno_mode_mix on a spectrum of the block's shape) and reports the bytes per
second it achieves over the weight bytes it must read.

    python tools/uno_time.py [--steps 5] [--out profiles/uno_time.json]

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
import tante_amd.uno as U  # noqa: E402
from afno_time import kernel_split, timed  # noqa: E402

SCALES = (8.0, 4.0, 2.0, 2.0, 2.0, 2.0, 2.0)      # what tests/golden/make_golden_uno.py chose for its 128 x 256 model


def eager_spectral(conv, x, Ho, Wo):
    """SpectralConv2d_Uno.forward from the mathematics, as eager torch ops."""
    m1, m2 = conv.modes1, conv.modes2
    x_ft = torch.fft.rfft2(x.float(), norm="forward")
    out_ft = torch.zeros(x.shape[0], conv.out_channels, Ho, Wo // 2 + 1, dtype=torch.cfloat, device=x.device)
    out_ft[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, :m1, :m2], conv.weights1)
    out_ft[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", x_ft[:, :, -m1:, :m2], conv.weights2)
    return torch.fft.irfft2(out_ft, s=(Ho, Wo), norm="forward")


def eager_block(blk, x, Ho, Wo):
    pw = F.interpolate(blk.w.conv(x).float(), size=(Ho, Wo), mode="bicubic", align_corners=True, antialias=True)
    return F.gelu(eager_spectral(blk.conv, x, Ho, Wo) + pw)


def eager_forward(m, x):
    """models.UNO.forward from the mathematics, on m's own parameters, as eager torch ops."""
    b, t, c, h, w = x.shape
    rows = torch.cat((x.permute(0, 3, 4, 1, 2).reshape(b, h, w, t * c), U.get_grid(h, w).float().to(x.device).expand(b, h, w, 4)), dim=-1)
    x_fc = F.gelu(m.fc(rows))
    x_fc0 = F.gelu(m.fc0(x_fc)).permute(0, 3, 1, 2)
    p = m.padding
    x_fc0 = F.pad(x_fc0, [p, p, p, p])
    D1, D2 = x_fc0.shape[-2], x_fc0.shape[-1]
    run = lambda i, v: eager_block(getattr(m, f"L{i}"), v, D1 // U.BLOCK_DIVS[i], D2 // U.BLOCK_DIVS[i])      # noqa: E731
    c0 = run(0, x_fc0)
    c1 = run(1, c0)
    c3 = run(3, run(2, c1))
    c4 = torch.cat([run(4, c3), c1], dim=1)
    c5 = torch.cat([run(5, c4), c0], dim=1)
    c6 = torch.cat([run(6, c5), x_fc0.float()], dim=1)
    if p:
        c6 = c6[..., p:-p, p:-p]
    x_fc1 = F.gelu(m.fc1(c6.permute(0, 2, 3, 1)))
    out = m.fc2(torch.cat([x_fc1, x_fc.to(x_fc1.dtype)], dim=3)).float()
    return out.permute(0, 3, 1, 2).unsqueeze(1)


def mix_rows(m, B, sizes, steps):
    """Per block: tante_uno_mode_mix alone on a spectrum of the block's shape, and its bytes per second over the weight bytes."""
    from tante_amd import _lib as L
    from tante_amd import kernels as K
    dev = m.fc.weight.device
    rows = []
    for i in range(7):
        conv = getattr(m, f"L{i}").conv
        Ci, Co, m1, m2 = conv.weights1.shape
        X = torch.randn(B, Ci, 2, 2 * m1, m2, device=dev)
        Y = torch.empty(B, Co, 2, 2 * m1, m2, device=dev)
        w1, w2 = torch.view_as_real(conv.weights1.detach()), torch.view_as_real(conv.weights2.detach())

        def step():
            L.check(L.lib().tante_uno_mode_mix(X.data_ptr(), w1.data_ptr(), w2.data_ptr(), Y.data_ptr(), B, Ci, Co, m1, m2, K._stream()), "tante_uno_mode_mix")
        t = timed(step, 20 * steps, ramp_s=0.15)
        wbytes = 2 * 8 * Ci * Co * m1 * m2
        rows.append({"block": f"L{i}", "batch": B, "Ci": Ci, "Co": Co, "modes": [m1, m2], "grid": list(sizes[i]), "weight_mbytes": round(wbytes / 1e6, 3),
                     "us_median": round(1e3 * t["ms_median"], 2), "us_min": round(1e3 * t["ms_min"], 2), "us_max": round(1e3 * t["ms_max"], 2),
                     "weight_gbytes_per_s": round(wbytes / (t["ms_median"] * 1e-3) / 1e9, 1)})
        print(f"  L{i} mode mix B {B}: {rows[-1]['weight_mbytes']} MB of weights in {rows[-1]['us_median']} us: {rows[-1]['weight_gbytes_per_s']} GB/s", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uno_time.json"))
    ap.add_argument("--time-anyway", action="store_true", help="time also when a HIP output misses its gate (recorded as gate_passed: false)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "uno_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).eval()
    with torch.no_grad():
        for i, s in enumerate(SCALES):
            getattr(m, f"L{i}").conv.weights1.mul_(s), getattr(m, f"L{i}").conv.weights2.mul_(s)
    sizes = U.block_sizes(*wl["spatial_resolution"])
    result = {"workload": {"config": "configs/uno_am.yaml", "bf16_operands": "fc, fc0, fc1, fc2", "resolution": wl["spatial_resolution"], "n_fields": wl["n_fields"],
                           "parameters": sum(p.numel() for p in m.parameters()), "spectral_weight_mbytes": round(sum(
                               8 * p.numel() for k, p in m.named_parameters() if "weights" in k) / 1e6, 1), "spectral_scales": list(SCALES)},
              "device": torch.cuda.get_device_name(0), "batches": {}, "mode_mix": []}
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
        m.set_compute(None)
        result["batches"][str(B)] = entry
        result["mode_mix"] += mix_rows(m, B, sizes, args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {md_: {"hip_ms": v[md_]["hip"]["ms_median"], "eager_ms": v[md_]["eager_torch"]["ms_median"]} for md_ in v}
                      for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
