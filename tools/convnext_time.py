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

Writes the times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward).

    python tools/convnext_time.py --train [--steps 3] [--out profiles/convnext_train_time.json]

times one TRAIN step of the same config (B = 4, bf16 compute): tante_amd.train_step on the opted-in model with
FlatAdamW(model.trained_parameters()), against the same eager composition under autograd (bf16 autocast) with clip_grad_norm_ and torch's
fused AdamW on its own copy of the weights -- the parent has no training path, so eager torch is the only yardstick, and no ratio is
promised.  It also records, on the two g21 model fixtures, every trained parameter's bf16-mode gradient error against the eager
composition in float64, beside the error of the eager composition under bf16 autocast against the same float64, and names the HIP
gradients that are more than twice as far from float64 as the eager ones."""
import argparse
import copy
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


def eager_forward(m, x, out_dtype=torch.float32):
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
    return m.out_proj(x).to(out_dtype).unsqueeze(1)


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


NEW_KERNELS = ("dlb_a_kernel", "dlb_b_kernel", "dlb_c_kernel", "l2_bwd_kernel", "dl_kernel", "l2_kernel")


def step_profile(step):
    """One profiled step: -> (launches, device us in all, the twelve heaviest kernels, the block's and the row norm's kernels by name)."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))) for e in prof.key_averages()]
    rows = sorted((r for r in rows if r[2] > 0.0), key=lambda r: -r[2])
    fmt = lambda r: {"name": r[0][:96], "calls": r[1], "us": round(r[2], 1)}      # noqa: E731
    return (sum(r[1] for r in rows), round(sum(r[2] for r in rows), 1), [fmt(r) for r in rows[:12]],
            [fmt(r) for r in rows if any(k in r[0] for k in NEW_KERNELS)])


def gradient_errors(dev):
    """The two g21 model fixtures: rel L2 error per trained parameter of the bf16-mode HIP gradient and of the eager composition's gradient
    under bf16 autocast, both against the eager composition in float64 (same weights, same output gradient)."""
    import types

    import numpy as np
    out = {}
    for name in ("g21_convnext_model_f15_s2_20x28", "g21_convnext_model_f8_s3_16x24"):
        raw = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        sd = {k[2:]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith("w.")}
        m = tante_amd.UNetConvNext(int(raw["in_T"]), types.SimpleNamespace(n_fields=int(raw["n_fields"]), n_spatial_dims=2), stages=int(raw["stages"]),
                                   blocks_per_stage=int(raw["blocks_per_stage"]), blocks_at_neck=int(raw["blocks_at_neck"]),
                                   init_features=int(raw["init_features"]))
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval().set_compute("bf16").set_trainable()
        m64 = copy.deepcopy(m).double()
        names = [k for k, _ in m.named_parameters() if not k.endswith("resample.block.0.bias")]
        x = torch.from_numpy(raw["x"]).float().to(dev)
        y64 = eager_forward(m64, x.double(), torch.float64)
        gy = torch.randn(y64.shape, generator=torch.Generator().manual_seed(32)).to(dev)
        want = torch.autograd.grad(y64, m64.trained_parameters(), gy.double())
        hip = torch.autograd.grad(m(x), m.trained_parameters(), gy)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ye = eager_forward(m, x)
        eager = torch.autograd.grad(ye, m.trained_parameters(), gy)
        rel = lambda a, b: float((a.double() - b).norm() / b.norm())      # noqa: E731
        rows = {k: {"hip": rel(a, w), "eager_autocast": rel(e, w)} for k, a, e, w in zip(names, hip, eager, want)}
        flagged = [k for k, r in rows.items() if r["hip"] > 2 * r["eager_autocast"]]
        hs, es = sorted(r["hip"] for r in rows.values()), sorted(r["eager_autocast"] for r in rows.values())
        out[name] = {"parameters": len(rows), "hip_median": hs[len(hs) // 2], "hip_max": hs[-1], "eager_median": es[len(es) // 2], "eager_max": es[-1],
                     "hip_more_than_twice_eager": flagged, "per_parameter": rows}
        print(f"{name}: bf16 gradients vs float64: HIP median {hs[len(hs) // 2]:.3e} max {hs[-1]:.3e}; eager autocast median {es[len(es) // 2]:.3e} "
              f"max {es[-1]:.3e}; HIP > 2 x eager: {flagged}", flush=True)
    return out


def train_main(args, dev):
    """The train step of configs/unet_convnext_am.yaml: HIP (train_step, FlatAdamW) against eager torch under autograd."""
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "unet_convnext_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    grad_err = gradient_errors(dev)
    m = tante_amd.build_model(cfg, md).to(dev)
    rescale(m)
    m = m.train().set_compute("bf16").set_trainable()
    me = copy.deepcopy(m)           # the eager composition trains its own copy of the weights
    B, T, res, nf = wl["batch_size"], cfg["model"]["in_T"], wl["spatial_resolution"], wl["n_fields"]
    batch = {"input": torch.randn(B, T, *res, nf, device=dev), "output": torch.randn(B, 1, *res, nf, device=dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    opt = tante_amd.FlatAdamW(m.trained_parameters(), lr=1e-5)
    eparams = me.trained_parameters()
    eopt = torch.optim.AdamW(eparams, lr=1e-5, weight_decay=1e-5, fused=True)
    x = batch["input"].permute(0, 1, 4, 2, 3).contiguous()

    def hip_step():
        return tante_amd.train_step(m, opt, batch, fmt, 1)

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = eager_forward(me, x)
        loss = F.mse_loss(y.permute(0, 1, 3, 4, 2).float(), batch["output"])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(eparams, 1.0)
        eopt.step()
        return loss.detach()

    l_hip, l_eager = float(hip_step()), float(eager_step())         # the first step of each, from the same weights
    torch.cuda.synchronize()
    print(f"first losses: HIP {l_hip:.6f}, eager torch {l_eager:.6f}", flush=True)
    if not abs(l_hip - l_eager) < 1e-2 * abs(l_eager) and not args.time_anyway:
        raise SystemExit(f"the first losses disagree ({l_hip} vs {l_eager}): nothing timed")
    hip = timed(hip_step, args.steps)
    print("HIP timed", flush=True)
    eager = timed(eager_step, args.steps)
    print("eager timed", flush=True)
    n_hip, us_hip, split_hip, new_hip = step_profile(hip_step)
    n_eager, us_eager, split_eager, _ = step_profile(eager_step)
    spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
    result = {"workload": {"config": "configs/unet_convnext_am.yaml", "compute": "bf16", "batch": B, "in_T": T, "resolution": res, "n_fields": nf,
                           "n_steps_output": 1, "parameters": sum(p.numel() for p in m.parameters()),
                           "trained_parameters": sum(p.numel() for p in m.trained_parameters())},
              "device": torch.cuda.get_device_name(0), "first_loss": {"hip": l_hip, "eager_torch": l_eager},
              "hip": hip, "eager_torch": eager, "speedup_median": round(eager["ms_median"] / hip["ms_median"], 3),
              "hip_not_slower_beyond_spread": bool(hip["ms_median"] <= eager["ms_median"] + spread),
              "launches_per_step": {"hip": n_hip, "eager_torch": n_eager}, "device_us_per_step": {"hip": us_hip, "eager_torch": us_eager},
              "kernels_hip": split_hip, "block_and_row_norm_kernels_hip": new_hip, "kernels_eager_torch": split_eager,
              "bf16_gradient_rel_errors_vs_float64": grad_err}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"hip_ms": hip["ms_median"], "eager_ms": eager["ms_median"], "launches": n_hip, "device_us": us_hip}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time the train step instead of the forward (default --out profiles/convnext_train_time.json)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    ap.add_argument("--time-anyway", action="store_true", help="time also when a HIP output misses its gate (recorded as gate_passed: false)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "convnext_train_time.json" if args.train else "convnext_time.json")
    dev = torch.device("cuda:0")
    if args.train:
        return train_main(args, dev)
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
