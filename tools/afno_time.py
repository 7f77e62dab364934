#!/usr/bin/env python3
"""Time the AFNO baseline (configs/afno_am.yaml: 256 x 256 x 11 fields, in_T 4, patch 8, hidden 256, 8 blocks) at B = 1 and B = 4, bf16,
against a plain eager-torch composition of the same model from the same weights (torch.fft on the GPU) -- there is no earlier HIP form of
this model to compare with.  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps forwards each,
synchronised on both sides.  The two outputs must agree under the bf16 bar (1e-2) before anything is timed.

    python tools/afno_time.py [--steps 20] [--out profiles/afno_time.json]

Writes both times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tante_amd  # noqa: E402


def eager_forward(m, x):
    """models.AFNO.forward from the mathematics, on m's parameters, as eager torch ops (the filter in fp32, as the reference keeps it)."""
    b, t, c, h, w = x.shape
    p, C = m.patch_size, m.hidden_dim
    y = F.conv2d(x.reshape(b, t * c, h, w), m.patch_embed.weight, m.patch_embed.bias, stride=p).permute(0, 2, 3, 1) + m.pos_embed
    H, W = y.shape[1], y.shape[2]
    for blk in m.blocks:
        r = y
        f = F.layer_norm(y, (C,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps).float()
        X = torch.fft.rfftn(f, dim=(2, 1), norm="ortho")
        for i in (0, 2):
            wt = torch.view_as_complex(blk.filter.cmlp[i].weight)
            X = torch.einsum("...bi,bio->...bo", X.reshape(*X.shape[:-1], wt.shape[0], wt.shape[1]), wt).reshape(*X.shape[:-1], C)
            if i == 0:
                X = torch.complex(F.gelu(X.real), F.gelu(X.imag))
        X = torch.view_as_complex(F.softshrink(torch.view_as_real(X), lambd=blk.filter.sparsity_threshold))
        f = torch.fft.irfftn(X, s=(H, W), dim=(2, 1), norm="ortho").transpose(1, 2)
        y = f + r
        r = y
        n = F.layer_norm(y, (C,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        y = F.linear(F.gelu(F.linear(n, blk.mlp.fc1.weight, blk.mlp.fc1.bias)), blk.mlp.fc2.weight, blk.mlp.fc2.bias) + r
    o = F.conv_transpose2d(y.permute(0, 3, 1, 2), m.patch_debed.weight, m.patch_debed.bias, stride=p)
    return o.unsqueeze(1)


def timed(step, steps, reps=7, ramp_s=0.5):
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < ramp_s:
        step()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
    regions = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t) / steps)
    regions.sort()
    return {"ms_median": round(1e3 * regions[len(regions) // 2], 4), "ms_min": round(1e3 * regions[0], 4), "ms_max": round(1e3 * regions[-1], 4),
            "reps": reps, "steps_per_region": steps, "ramp_steps_untimed": n}


def kernel_split(step):
    """-> (launches per forward, [{name, calls, us}] by device time) from one profiled forward; None when the profiler is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))) for e in prof.key_averages()]
        rows = [r for r in rows if r[2] > 0.0]
        rows.sort(key=lambda r: -r[2])
        return sum(r[1] for r in rows), [{"name": r[0][:96], "calls": r[1], "us": round(r[2], 1)} for r in rows[:12]]
    except Exception as e:      # the split is a report, not a gate
        return None, f"profiler unavailable: {type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afno_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "afno_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).eval().set_compute("bf16")
    with torch.no_grad():       # a default-init filter is identically zero: scale it as the fixtures do, or its kernels would time zeros
        for k, p in m.named_parameters():
            if ".cmlp." in k:
                p.mul_(2.0)
    result = {"workload": {"config": "configs/afno_am.yaml", "compute": "bf16", "resolution": wl["spatial_resolution"], "n_fields": wl["n_fields"]},
              "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in args.batches:
        x = torch.randn(B, cfg["model"]["in_T"], wl["n_fields"], *wl["spatial_resolution"], device=dev)

        def hip_step():
            with torch.no_grad():
                return m(x)

        def eager_step():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return eager_forward(m, x)

        a, b = hip_step().double(), eager_step().double()
        rel = float((a - b).norm() / b.norm())
        if not rel < 1e-2:
            raise SystemExit(f"B = {B}: the HIP path and the eager composition disagree (rel {rel:.3e} >= 1e-2): nothing timed")
        hip, eager = timed(hip_step, args.steps), timed(eager_step, args.steps)
        n_hip, split_hip = kernel_split(hip_step)
        n_eager, split_eager = kernel_split(eager_step)
        spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
        result["batches"][str(B)] = {"agreement_rel": rel, "hip": hip, "eager_torch": eager, "speedup_median": round(eager["ms_median"] / hip["ms_median"], 3),
                                     "hip_not_slower_beyond_spread": bool(hip["ms_median"] <= eager["ms_median"] + spread),
                                     "launches_per_forward": {"hip": n_hip, "eager_torch": n_eager}, "kernels_hip": split_hip,
                                     "kernels_eager_torch": split_eager}
        print(f"B = {B}: HIP {hip['ms_median']} ms, eager torch {eager['ms_median']} ms, agreement {rel:.2e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {"hip_ms": v["hip"]["ms_median"], "eager_ms": v["eager_torch"]["ms_median"]} for k, v in result["batches"].items()}))


if __name__ == "__main__":
    main()
