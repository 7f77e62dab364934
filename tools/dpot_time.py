#!/usr/bin/env python3
"""Time the DPOT baseline (configs/dpot_am.yaml: 256 x 256 x 11 fields, in_T 4, patch 32, width 1536, 24 blocks, 16 modes) at B = 1 and
B = 4, bf16, against a plain eager-torch composition of the same model from the same weights (torch.fft on the GPU, the mixer in fp32 as
the HIP path keeps it, kernel = stride convolutions as reshapes + F.linear) -- there is no earlier HIP form of this model to compare
with.  bench.py's scheme: a >= 0.5 s untimed ramp, then the MEDIAN of 7 timed regions of --steps forwards each, synchronised on both
sides.  The two outputs must agree under the bf16 bar (1e-2) before anything is timed (--time-anyway: timed and marked); each one's
distance from the same composition in fp32 is recorded beside it.

    python tools/dpot_time.py [--steps 10] [--out profiles/dpot_time.json]

Writes both times, the spread of the regions, the launches per forward and the per-kernel split (torch.profiler, one forward).

    python tools/dpot_time.py --train [--steps 5] [--out profiles/dpot_train_time.json]

times one TRAIN step of the same config (B = 4, 8 x 8 tokens, bf16 compute): tante_amd.train_step on the opted-in model with
FlatAdamW(model.trained_parameters()), against the same eager composition under autograd with clip_grad_norm_ and torch's fused AdamW on
a copy of the weights -- the same scheme, and a per-kernel split of one step in which the mixer's and GroupNorm's backward kernels are
listed by name."""
import argparse
import copy
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


def eager_filter(f, x):
    """AFNO2D.forward from the mathematics, channels last, on f's parameters, in fp32."""
    with torch.autocast("cuda", enabled=False):
        x = x.float()
        B, H, W, C = x.shape
        k1, k2 = min(f.modes, H), min(f.modes, W // 2 + 1)
        X = torch.fft.rfft2(x, dim=(1, 2), norm="ortho")[:, :k1, :k2].reshape(B, k1, k2, f.num_blocks, f.block_size)
        U = torch.einsum("...bi,bio->...bo", X, torch.complex(f.w1[0], f.w1[1])) + torch.complex(f.b1[0], f.b1[1])
        V = torch.complex(F.gelu(U.real), F.gelu(U.imag))
        Y = torch.einsum("...bi,bio->...bo", V, torch.complex(f.w2[0], f.w2[1])) + torch.complex(f.b2[0], f.b2[1])
        full = torch.zeros(B, H, W // 2 + 1, C, dtype=Y.dtype, device=x.device)
        full[:, :k1, :k2] = Y.reshape(B, k1, k2, C)
        return torch.fft.irfft2(full, s=(H, W), dim=(1, 2), norm="ortho") + x


def group_norm_last(x, norm):
    """GroupNorm on a channels-last image through torch's own kernel (which wants the channels on dim 1)."""
    return F.group_norm(x.permute(0, 3, 1, 2), norm.num_groups, norm.weight, norm.bias, norm.eps).permute(0, 2, 3, 1)


def eager_forward(m, x, grid):
    """models.DPOT.forward from the mathematics, on m's parameters, as eager torch ops; grid = m.get_grid_3d(T, device), built once.
    Channels last, and every kernel = stride convolution written as a reshape + F.linear: the GEMM library answers at once, where the
    convolution library searches and compiles kernels for every new shape at run time -- minutes that are no property of the model."""
    b, T, c, h, w = x.shape
    p, C = m.patch_size, m.embed_dim
    Hp, Wp = h // p, w // p
    img = torch.cat([x, grid[None].expand(b, -1, -1, -1, -1)], dim=2).reshape(b * T, c + 3, Hp, p, Wp, p)
    pe = m.patch_embed.proj
    y = F.gelu(F.linear(img.permute(0, 2, 4, 1, 3, 5).reshape(b * T, Hp, Wp, -1), pe[0].weight.flatten(1), pe[0].bias))
    y = F.linear(y, pe[2].weight.flatten(1), pe[2].bias) + m.pos_embed[0].permute(1, 2, 0)
    y = y.view(b, T, Hp, Wp, C)
    ta = m.time_agg_layer
    if ta.type == "exp_mlp":
        y = y * torch.cos(torch.linspace(0, 1, T, device=x.device).unsqueeze(-1) @ ta.gamma)[:, None, None, :]
    y = torch.einsum("tij,btxyi->bxyj", ta.w, y)
    for blk in m.blocks:
        r = y
        f = eager_filter(blk.filter, group_norm_last(y, blk.norm1))
        if blk.double_skip:
            f = f + r
            r = f
        n = group_norm_last(f, blk.norm2)
        y = F.linear(F.gelu(F.linear(n, blk.mlp[0].weight.flatten(1), blk.mlp[0].bias)), blk.mlp[2].weight.flatten(1), blk.mlp[2].bias) + r
    ol = m.out_layer
    od = ol[0].weight.shape[1]
    o = F.linear(y, ol[0].weight.flatten(1).t()).view(b, Hp, Wp, od, p, p).permute(0, 1, 4, 2, 5, 3).reshape(b, h, w, od) + ol[0].bias
    o = F.linear(F.gelu(F.linear(F.gelu(o), ol[2].weight.flatten(1), ol[2].bias)), ol[4].weight.flatten(1), ol[4].bias)
    return o.view(b, h, w, m.out_timesteps, m.out_channels).permute(0, 3, 4, 1, 2)


NEW_KERNELS = ("dpot_mlp_bwd_kernel", "dpot_wgrad_kernel", "gn_bwd_sums_kernel", "gn_bwd_apply_kernel", "gn_bwd_param_kernel", "DpotBwdEpilogue",
               "gn_stats_kernel", "dpot_fwd_h_kernel", "dpot_inv_h_kernel", "dft_r2c_rows_kernel", "dpot_mlp_kernel")


def step_profile(step):
    """One profiled step: -> (launches, device us in all, the twelve heaviest kernels, the mixer's / GroupNorm's kernels by name -- the
    new backward ones and the forward ones the backward runs again)."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))) for e in prof.key_averages()]
    rows = sorted((r for r in rows if r[2] > 0.0), key=lambda r: -r[2])
    fmt = lambda r: {"name": r[0][:96], "calls": r[1], "us": round(r[2], 1)}
    return (sum(r[1] for r in rows), round(sum(r[2] for r in rows), 1), [fmt(r) for r in rows[:12]],
            [fmt(r) for r in rows if any(k in r[0] for k in NEW_KERNELS)])


def train_main(args, dev):
    """The train step of configs/dpot_am.yaml: HIP (train_step, FlatAdamW) against eager torch under autograd, same scheme as main()."""
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "dpot_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    with torch.device(dev):
        m = tante_amd.build_model(cfg, md)
    m = m.to(dev).train().set_compute("bf16").set_trainable()
    with torch.no_grad():       # as in main(): a default-init mixer adds 3e-4 of its input
        for blk in m.blocks:
            f = blk.filter
            for wt in (f.w1, f.w2):
                wt.copy_(torch.randn_like(wt) / f.block_size ** 0.5)
            for bt in (f.b1, f.b2):
                bt.copy_(0.3 * torch.randn_like(bt))
    me = copy.deepcopy(m)           # the eager composition trains its own copy of the weights
    B, T, res, nf = wl["batch_size"], cfg["model"]["in_T"], wl["spatial_resolution"], wl["n_fields"]
    n_out = cfg["model"]["out_timesteps"]
    batch = {"input": torch.randn(B, T, *res, nf, device=dev), "output": torch.randn(B, n_out, *res, nf, device=dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    opt = tante_amd.FlatAdamW(m.trained_parameters(), lr=1e-5)
    eparams = me.trained_parameters()
    eopt = torch.optim.AdamW(eparams, lr=1e-5, weight_decay=1e-5, fused=True)
    x = batch["input"].permute(0, 1, 4, 2, 3).contiguous()
    grid = me.get_grid_3d(T, dev)

    def hip_step():
        return tante_amd.train_step(m, opt, batch, fmt, n_out)

    def eager_step():
        eopt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = eager_forward(me, x, grid)
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
    result = {"workload": {"config": "configs/dpot_am.yaml", "compute": "bf16", "batch": B, "in_T": T, "resolution": res, "n_fields": nf,
                           "n_steps_output": n_out, "tokens": list(m.latent_size), "parameters": sum(p.numel() for p in m.parameters()),
                           "trained_parameters": sum(p.numel() for p in m.trained_parameters())},
              "device": torch.cuda.get_device_name(0), "first_loss": {"hip": l_hip, "eager_torch": l_eager},
              "hip": hip, "eager_torch": eager, "speedup_median": round(eager["ms_median"] / hip["ms_median"], 3),
              "hip_not_slower_beyond_spread": bool(hip["ms_median"] <= eager["ms_median"] + spread),
              "launches_per_step": {"hip": n_hip, "eager_torch": n_eager}, "device_us_per_step": {"hip": us_hip, "eager_torch": us_eager},
              "kernels_hip": split_hip, "mixer_and_groupnorm_kernels_hip": new_hip, "kernels_eager_torch": split_eager}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"hip_ms": hip["ms_median"], "eager_ms": eager["ms_median"], "launches": n_hip, "device_us": us_hip}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time the train step instead of the forward (default --out profiles/dpot_train_time.json)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    ap.add_argument("--time-anyway", action="store_true", help="time also when the two outputs miss the agreement bar (recorded as agree_under_bf16_bar: false)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "dpot_train_time.json" if args.train else "dpot_time.json")
    dev = torch.device("cuda:0")
    if args.train:
        return train_main(args, dev)
    cfg = tante_amd.load_config(os.path.join(ROOT, "configs", "dpot_am.yaml"))
    wl = cfg["workload"]
    torch.manual_seed(cfg["seed"])
    md = tante_amd.TanteMetadata(n_fields=wl["n_fields"], spatial_resolution=tuple(wl["spatial_resolution"]))
    with torch.device(dev):
        m = tante_amd.build_model(cfg, md)
    m = m.to(dev).eval().set_compute("bf16")
    torch.cuda.synchronize()
    print("model built", flush=True)
    with torch.no_grad():       # a default-init mixer adds 3e-4 of its input: scale it as the fixtures do, or the agreement check would not see it
        for blk in m.blocks:
            f = blk.filter
            for wt in (f.w1, f.w2):
                wt.copy_(torch.randn_like(wt) / f.block_size ** 0.5)
            for bt in (f.b1, f.b2):
                bt.copy_(0.3 * torch.randn_like(bt))
    result = {"workload": {"config": "configs/dpot_am.yaml", "compute": "bf16", "resolution": wl["spatial_resolution"], "n_fields": wl["n_fields"],
                           "parameters": sum(p.numel() for p in m.parameters())},
              "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in args.batches:
        x = torch.randn(B, cfg["model"]["in_T"], wl["n_fields"], *wl["spatial_resolution"], device=dev)
        grid = m.get_grid_3d(x.shape[1], dev)

        def hip_step():
            with torch.no_grad():
                return m(x)

        def eager_step():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return eager_forward(m, x, grid)

        with torch.no_grad():       # the same composition in fp32: what each bf16 path is away from, beside their mutual distance
            ref = eager_forward(m, x, grid).double()
        torch.cuda.synchronize()
        print(f"B = {B}: fp32 eager forward done", flush=True)
        a = hip_step().double()
        torch.cuda.synchronize()
        print(f"B = {B}: first HIP forward done", flush=True)
        b = eager_step().double()
        torch.cuda.synchronize()
        rel, rel_hip32, rel_eager32 = (float((u - v).norm() / v.norm()) for u, v in ((a, b), (a, ref), (b, ref)))
        print(f"B = {B}: HIP bf16 vs eager bf16 {rel:.3e}; against the fp32 composition: HIP bf16 {rel_hip32:.3e}, eager bf16 {rel_eager32:.3e}", flush=True)
        if not rel < 1e-2 and not args.time_anyway:
            raise SystemExit(f"B = {B}: the HIP path and the eager composition disagree (rel {rel:.3e} >= 1e-2): nothing timed")
        hip = timed(hip_step, args.steps)
        print(f"B = {B}: HIP timed", flush=True)
        eager = timed(eager_step, args.steps)
        print(f"B = {B}: eager timed", flush=True)
        n_hip, split_hip = kernel_split(hip_step)
        n_eager, split_eager = kernel_split(eager_step)
        spread = max(hip["ms_max"] - hip["ms_min"], eager["ms_max"] - eager["ms_min"])
        result["batches"][str(B)] = {"agreement_rel": rel, "agree_under_bf16_bar": bool(rel < 1e-2), "hip_bf16_vs_fp32_rel": rel_hip32, "eager_bf16_vs_fp32_rel": rel_eager32, "hip": hip, "eager_torch": eager, "speedup_median": round(eager["ms_median"] / hip["ms_median"], 3),
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
