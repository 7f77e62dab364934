#!/usr/bin/env python3
"""Time the AFNO baseline (configs/afno_am.yaml: 256 x 256 x 11 fields, in_T 4, patch 8, hidden 256, 8 blocks) at B = 1 and B = 4, bf16,
against a plain eager-torch composition of the same model from the same weights (torch.fft on the GPU) -- there is no earlier HIP form of
this model to compare with.  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps forwards each,
synchronised on both sides.  The two outputs must agree under the bf16 bar (1e-2) before anything is timed.

    python tools/afno_time.py [--steps 20] [--out profiles/afno_time.json]

Writes both times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward).

    python tools/afno_time.py --train [--train-rollout 1] [--out profiles/afno_train_time.json]

times one train step instead (model.set_trainable(), train_step with FlatAdamW, bf16, the config's batch of 4): the same ramp and median
of 7 regions, and the per-kernel device times of a warm step from one `rocprofv3 --kernel-trace --stats` run of a child process of its own."""
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


def train_setup(dev, rollout):
    """The config's model, opted in to training, bf16 compute, with FlatAdamW and one fixed random batch of the config's shape."""
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "afno_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    m = tante_amd.build_model(cfg, md).to(dev).train().set_compute("bf16").set_trainable()
    with torch.no_grad():       # a default-init filter is identically zero (see main)
        for k, p in m.named_parameters():
            if ".cmlp." in k:
                p.mul_(2.0)
    B, T, res, nf = wl["batch_size"], cfg["model"]["in_T"], wl["spatial_resolution"], wl["n_fields"]
    batch = {"input": torch.randn(B, T, *res, nf, device=dev), "output": torch.randn(B, rollout, *res, nf, device=dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    opt = tante_amd.FlatAdamW(m.parameters(), lr=1e-4)
    return (lambda: tante_amd.train_step(m, opt, batch, fmt, rollout)), {"config": "configs/afno_am.yaml", "compute": "bf16", "batch": B, "in_T": T,
                                                                          "resolution": res, "n_fields": nf, "n_steps_output": rollout}


WARM_STEPS, PROFILED_STEPS = 5, 5


def kernel_stats_under_rocprof(rollout):
    """Per-kernel device time of one WARM train step: `rocprofv3 --kernel-trace --stats` around a fresh child process that runs
    WARM_STEPS + PROFILED_STEPS train steps and nothing else.  The trace is cut into steps at the optimiser's kernel (the last launch of a
    step) and only the last PROFILED_STEPS of them are counted, so first-step work (weight packing, table uploads, allocator growth) is
    left out; -> ([{name, calls_per_step, us_per_step}], device us per step) or a string saying why there is none."""
    import csv
    import glob
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--train",
               "--profiled-child", "--train-rollout", str(rollout)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        except (OSError, subprocess.TimeoutExpired) as e:
            return f"rocprofv3 run failed: {type(e).__name__}: {e}"
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return f"rocprofv3 run left no kernel trace (exit {r.returncode}): {r.stderr[-300:]}"
        rows = sorted(csv.DictReader(open(files[0])), key=lambda q: int(q["Start_Timestamp"]))
    steps, cur = [], []
    for q in rows:
        cur.append((q["Kernel_Name"], int(q["End_Timestamp"]) - int(q["Start_Timestamp"])))
        if "adamw_kernel" in q["Kernel_Name"]:
            steps.append(cur)
            cur = []
    if len(steps) != WARM_STEPS + PROFILED_STEPS:
        return f"the trace holds {len(steps)} optimiser launches, {WARM_STEPS + PROFILED_STEPS} steps were run"
    agg = {}
    for st in steps[-PROFILED_STEPS:]:
        for name, ns in st:
            e = agg.setdefault(name, [0, 0])
            e[0] += 1
            e[1] += ns
    kernels = sorted(agg.items(), key=lambda kv: -kv[1][1])
    total = round(sum(v[1] for v in agg.values()) / PROFILED_STEPS / 1e3, 1)
    return [{"name": k[:110], "calls_per_step": round(v[0] / PROFILED_STEPS, 2), "us_per_step": round(v[1] / PROFILED_STEPS / 1e3, 1)}
            for k, v in kernels[:24]], total


def train_main(args):
    dev = torch.device("cuda:0")
    if args.profiled_child:
        step, _ = train_setup(dev, args.train_rollout)
        for _ in range(WARM_STEPS + PROFILED_STEPS):
            step()
        torch.cuda.synchronize()
        return
    kernels = kernel_stats_under_rocprof(args.train_rollout)      # before this process opens the GPU
    step, workload = train_setup(dev, args.train_rollout)
    losses = [float(step()) for _ in range(3)]
    if not all(v == v and abs(v) != float("inf") for v in losses):
        raise SystemExit(f"the train step's loss is not finite ({losses}): nothing timed")
    t = timed(step, args.steps)
    kernels, total = kernels if isinstance(kernels, tuple) else (kernels, None)
    result = {"workload": workload, "device": torch.cuda.get_device_name(0), "train_step": t, "first_losses": losses,
              "kernels_rocprofv3": kernels, "kernel_us_per_step_all": total,
              "note": "a first measurement of this path, not a target.  kernels_rocprofv3: the largest kernels of the last "
                      f"{PROFILED_STEPS} of {WARM_STEPS + PROFILED_STEPS} steps of a profiled child process (warm steps only); "
                      "kernel_us_per_step_all: the device time of ALL kernels of such a step, measured under the profiler, next to the "
                      "unprofiled wall-clock median in train_step"}
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "afno_train_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"train_step_ms": t["ms_median"], "kernel_us_per_step_all": total}))


DEFAULT_OUT = os.path.join(ROOT, "profiles", "afno_time.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--train", action="store_true", help="time one train step (set_trainable, FlatAdamW, bf16) -> profiles/afno_train_time.json")
    ap.add_argument("--train-rollout", type=int, default=1, help="--train: frames predicted (and back-propagated through) per step")
    ap.add_argument("--profiled-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.train:
        return train_main(args)
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
