#!/usr/bin/env python3
"""Headline benchmark: autoregressive rollout frames/sec of TANTE on Active-Matter-shaped fields
(BASELINE.json configs[1]: configs/tante_am.yaml -- 256x256x11, order-3 Taylor, bf16).

A "step" is one full rollout of one batch: B samples x n_steps_rollout frames through the
Evaler.rollout_model loop (trainer/evaler.py:121-138) with the window already resident in HBM.
`value` = frames produced by all ranks / wall time of the K timed steps (max over ranks).
Multi-GPU: the rollout shards over batch (independent samples, no data-path collective) -> weak scaling.

Launch: `python bench.py --gpus N` with WORLD_SIZE unset spawns the N ranks ITSELF (one process per GPU, before this process makes
any GPU call) and prints rank 0's line; under torchrun (RANK / LOCAL_RANK / WORLD_SIZE set) it is one of the ranks.  It fails loudly
when --gpus disagrees with WORLD_SIZE or with the number of visible GPUs.

A plain run does only what the headline figure needs: set up, warm up, time the steps, write --dump-outputs, print the line.
With --full the same JSON line also reports (each leg still switched off by its --no-* flag):
  roofline      dominant kernel (LayerNorm-fused projection GEMM, bf16 MFMA) algorithmic FLOP/s vs the dense
                bf16 peak, timed with HIP events around each of its launches in an instrumented pass
  cpu_baseline  the CPU oracle (oracle/tante_oracle.py, kind "port") timed on this box's host cores on a bounded
                sample of the same workload (rank 0, N=1 only)
  train         the cfg3 train step (configs/tante_trl.yaml), weak and strong (cfg2 runs only)
  workloads     compact legs of cfg2 at other batches, cfg4 and cfg5 (cfg2 runs, rank 0, N=1 only)
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}      # dense MFMA peaks, MI355X_MICROARCH.md
PMC_FILE = "r06_pmc_rollout.json"                    # HBM counters of the dominant kernel (separate --pmc passes, committed)
DUMP_BYTES, DUMP_SEED = 48 << 20, 20240                # --dump-outputs: bytes of array data in all, seed of the sampled positions


def _sha16(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--config", default=os.path.join(ROOT, "configs", "tante_am.yaml"))
    p.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: workload.batch_size)")
    p.add_argument("--dtype", default=None, choices=["bf16", "fp32"])
    p.add_argument("--full", action="store_true", help="also run the legs the headline figure does not need: the roofline pass, the train-step "
                                                         "leg, the CPU baseline and the compact side workloads (off: a plain run stops after "
                                                         "the headline leg's timed steps and --dump-outputs)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-roofline", action="store_true")
    p.add_argument("--no-train", action="store_true", help="skip the train-step leg (configs/tante_trl.yaml)")
    p.add_argument("--train-steps", type=int, default=12)
    p.add_argument("--no-train-strong", action="store_true", help="skip the strong-scaling train line (global batch 64)")
    p.add_argument("--graph", action="store_true", help="replay each rollout as one captured HIP graph (small batches are launch-bound on the host)")
    p.add_argument("--no-graph", action="store_true", help="the eager loop only (default: decided in the warm-up, eager unless the captured rollout is > 2 %% faster)")
    p.add_argument("--no-workloads", action="store_true", help="skip the compact cfg2 B=1 / cfg4 / cfg5 legs (the `workloads` object)")
    p.add_argument("--reps", type=int, default=7, help="the timed region of exactly --steps steps is repeated this many times behind a >= 0.5 s "
                                                       "ramp; `value` / `ms_per_step` are the MEDIAN region (min / max / reps in config.timing)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the headline leg's last timed step returned as DIR/<name>.npy (rank 0; fp32, fp64 "
                        "stays fp64): the whole array when it fits its share of %d MiB, else a fixed seeded sample of its flattened elements "
                        "(the same positions in every run with the same arguments), so that two builds can be compared output for output"
                        % (DUMP_BYTES >> 20))
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


def dump_outputs(result, names, out_dir):
    """Write each tensor of `result` (one tensor or a tuple) as out_dir/<name>.npy.  An array larger than its share of DUMP_BYTES is
    reduced to the elements at DUMP_SEED's sorted random flat positions (a 1-D array; they depend only on the element count and the
    share).  -> {name: (shape of the full output, number of elements written)}"""
    import numpy as np
    ts = (result,) if isinstance(result, torch.Tensor) else tuple(result)
    names = list(names) if len(names) == len(ts) else [f"out{i}" for i in range(len(ts))]
    os.makedirs(out_dir, exist_ok=True)
    info = {}
    for name, t in zip(names, ts):
        t = t.detach()
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        cap = (DUMP_BYTES // len(ts)) // (8 if dt == torch.float64 else 4)
        flat = t.reshape(-1)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(flat.numel(), cap, replace=False))
            flat = flat.index_select(0, torch.from_numpy(idx).to(flat.device))
            arr = flat.to(dt).cpu().numpy()
        else:
            arr = t.to(dt).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), arr)
        info[name] = (list(t.shape), int(arr.size))
    return info


def visible_gpus():
    """Number of GPUs this process would see, WITHOUT any torch.cuda / HIP call (the parent must not initialise the GPU before it starts
    its ranks): the KFD topology (nodes with simd_count > 0), cut down by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES.  None = unknown
    (no sysfs): the pre-check is skipped then and every rank still fails loudly on its own (`LOCAL_RANK >= device_count`)."""
    import glob
    n = 0
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    for f in nodes:
        try:
            with open(f) as fh:
                props = dict(ln.split(None, 1) for ln in fh.read().splitlines() if " " in ln)
            n += int(props.get("simd_count", "0")) > 0
        except (OSError, ValueError):
            return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


def launch_ranks(args) -> int:
    """--gpus N without a launcher: start N copies of this script, one per GPU, with the torchrun environment (RANK, LOCAL_RANK,
    WORLD_SIZE, MASTER_ADDR = 127.0.0.1, a free MASTER_PORT).  Nothing here touches the GPU (the GPUs are counted from sysfs, not through
    torch.cuda), so no initialised process is ever replaced or forked.  All ranks are polled: when one exits non-zero the others are
    terminated after a short grace period (they would otherwise sit in the rendezvous or a collective until its timeout) and that exit
    code is returned; every rank's stderr is passed through with its rank as a prefix, rank 0's stdout (the one JSON line) as it is."""
    import socket
    import subprocess
    import threading
    n = args.gpus
    plumbing = os.environ.get("TANTE_ALL_ON_GPU0") == "1"
    have = visible_gpus()
    if not plumbing and have is not None and have < n:
        raise SystemExit(f"bench.py: --gpus {n} but only {have} GPU(s) are visible; refusing to run fewer ranks than asked "
                         "(TANTE_DIST_BACKEND=gloo TANTE_ALL_ON_GPU0=1 runs the N-rank code path on one GPU: plumbing, not performance)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs, pumps = [], []

    def pump(r, stream):
        for line in stream:
            sys.stderr.write(f"[rank {r}] {line}")
        stream.close()

    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                             stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        procs.append(p)
        t = threading.Thread(target=pump, args=(r, p.stderr), daemon=True)
        t.start()
        pumps.append(t)
    out_lines = []
    t0 = threading.Thread(target=lambda: out_lines.extend(procs[0].stdout.readlines()), daemon=True)
    t0.start()
    failed = None
    while any(p.poll() is None for p in procs):
        bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad:
            failed = bad
            time.sleep(5.0)                                  # grace: let the other ranks notice and report on their own
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            time.sleep(2.0)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
    t0.join(timeout=5)
    for t in pumps:
        t.join(timeout=5)
    sys.stdout.write("".join(out_lines))
    sys.stdout.flush()
    bad = failed or [(r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0]
    if bad:
        raise SystemExit(f"bench.py: ranks failed (rank, exit code): {bad}")
    return 0


def train_flops_per_sample(cfg, wl) -> float:
    """Algorithmic FLOPs of one training sample of the TANTE train step: forward per model call =
    encoder (3 strided patch convs on T frames) + per Taylor order [3 axis propagators + the order's blocks + one derivative head],
    blocks = tokens x [2 C (3C + C + 2 hidden) + 4 L C]; a train step is n_steps_output calls, backward = 2 x forward."""
    mk = cfg["model"]
    C, T, D = mk.get("embed_dim", 256), mk["in_T"], wl["n_fields"]
    H, W = wl["spatial_resolution"]
    P = {4: (1, 2, 2), 8: (2, 2, 2), 16: (2, 2, 4), 32: (2, 4, 4), 64: (4, 4, 4)}[mk.get("patch_scale", 8)]
    chans = (D, C // 4, C // 2, C)
    enc = dec = 0.0
    h, w = H, W
    for i in range(3):
        h, w = h // P[i], w // P[i]
        stage = 2.0 * h * w * chans[i + 1] * chans[i] * P[i] * P[i]
        enc += T * stage
        dec += stage
    Hp, Wp = h, w
    tokens = T * Hp * Wp
    hidden = int(C * mk.get("mlp_ratio", 1.0))
    fwd = enc
    for order_axes in mk.get("attn_axes", "THWTHWTHW").split("-"):
        fwd += tokens * C * 4.0 * (Hp + Wp + T) + dec
        for letter in order_axes:
            Lq = {"T": T, "H": Hp, "W": Wp, "L": Hp * Wp, "Y": T * Hp, "X": T * Wp, "A": tokens}[letter]
            fwd += tokens * (2.0 * C * (3 * C + C + 2 * hidden) + 4.0 * Lq * C)
    return 3.0 * fwd * wl["n_steps_output"]


def physical_cores():
    """Physical cores of the host from /proc/cpuinfo (unique (physical id, core id) pairs); None when it cannot be read."""
    try:
        seen, phys, core = set(), None, None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                phys = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                core = ln.split(":")[1].strip()
            elif not ln.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            seen.add((phys, core))
        return len(seen) or None
    except OSError:
        return None


def shader_clock_mhz(local=0):
    """The shader clock the card reports right now (the starred line of sysfs pp_dpm_sclk of the local-th amdgpu card), or None when sysfs does
    not show it to this user.  Read before and after the timed regions: two readings that differ say the regions ran in different DVFS states."""
    import glob
    try:
        cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/pp_dpm_sclk"))
        with open(cards[min(local, len(cards) - 1)]) as f:
            for ln in f:
                if "*" in ln:
                    return int(re_mhz(ln))
    except (OSError, IndexError, ValueError):
        pass
    return None


def re_mhz(ln):
    import re
    return re.search(r"(\d+)\s*[Mm][Hh]z", ln).group(1)


def timed_regions(step, steps, reps, sync, dist, dev, ramp_s=0.5):
    """`reps` timed regions of EXACTLY `steps` steps each, every one bracketed by barrier + synchronize on both sides (MAX over ranks per
    region), behind a ramp of untimed steps lasting >= ramp_s: the clock state of a 75 ms region on a freshly woken card is one DVFS
    state, and a box-to-box +- 4 % hid a round's kernel work in round 4.  -> (median seconds per region, sorted list of all regions)."""
    sync()
    t_ramp = time.perf_counter()
    n_ramp = 0
    while time.perf_counter() - t_ramp < ramp_s:
        step()
        n_ramp += 1
        if n_ramp % 4 == 0:
            torch.cuda.synchronize()
    regions = []
    for _ in range(max(1, reps)):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        regions.append(el)
    regions.sort()
    return regions[len(regions) // 2], regions, n_ramp


def cvit_cpu_leg(lg, gpu_frames_per_s):
    """cfg4's CPU baseline: the oracle (oracle/cvit_oracle.py, kind "port") on the shipped model with 1 024 and 4 096 random query points
    -- as written the full 65 536-query grid embedding needs an 8.6 GB temporary -- extrapolated linearly in the query count to the
    full grid (the encoder is the intercept, the grid embedding + decoder + head are per query)."""
    import torch
    from oracle import cvit_oracle as OC
    cfg, wl, model = lg["cfg"], lg["wl"], lg["model"]
    H, W = lg["res"]
    mk = {k: v for k, v in cfg["model"].items() if k not in ("_target_", "in_T")}
    mk["grid_size"] = tuple(mk["grid_size"])
    ocfg = OC.CvitCfg(cfg["model"]["in_T"], lg["D"], (H, W), **mk)
    w = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    # the box's 16-core share (TANTE_CPU_THREADS), the faster of the two thread counts the cfg2 leg times: all 128 physical cores
    # oversubscribe the cgroup and made this short measurement noisy enough to extrapolate a NEGATIVE time once
    affinity = len(os.sched_getaffinity(0))
    threads = max(1, min(affinity, physical_cores() or affinity, int(os.environ.get("TANTE_CPU_THREADS", "16"))))
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, lg["T_in"], lg["D"], H, W, generator=g)
    ts = {}
    n_lo, n_hi = 1024, 4096
    with torch.no_grad():
        OC.cvit_forward(w, ocfg, x, torch.rand(256, 2, generator=g))      # warm-up
        for n in (n_lo, n_hi):
            c = torch.rand(n, 2, generator=g)
            best = float("inf")
            for _ in range(2):                                             # the better of two
                t0 = time.perf_counter()
                OC.cvit_forward(w, ocfg, x, c)
                best = min(best, time.perf_counter() - t0)
            ts[n] = best
    per_q = (ts[n_hi] - ts[n_lo]) / float(n_hi - n_lo)
    if per_q <= 0.0:      # still noise-dominated: no intercept, the larger sample's time per query (an upper bound of the CPU's speed)
        per_q, base = ts[n_hi] / n_hi, 0.0
    else:
        base = max(0.0, ts[n_lo] - n_lo * per_q)
    t_full = base + per_q * H * W
    fps = lg["n_steps"] / t_full
    return {"value": round(fps, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"oracle CViT forward, B = 1, {n_lo} / {n_hi} random query points in {ts[n_lo]:.2f} / {ts[n_hi]:.2f} s (the better of two runs each), extrapolated linearly to the "
                      f"{H * W}-query grid ({t_full:.1f} s per forward: encoder intercept {base:.2f} s + {1e3 * per_q:.3f} ms per query)",
            "gpu_over_cpu": round(gpu_frames_per_s / fps, 1)}


def rollout_leg(config, batch_arg, dtype_arg, steps, warmup, dev, rank, world, dist, want_roofline, graph=False, reps=1, dump_dir=None):
    """One timed leg: `steps` rollouts (CViT: model calls) of `config` at per-GPU batch `batch_arg` (None: workload.batch_size), barrier +
    synchronize on both sides, MAX over ranks; then (rank 0) the instrumented pass for the roofline entry.  graph=True replays the whole
    rollout as ONE captured HIP graph (B = 1: the 100-odd launches of a rollout are issue-bound on the host).  dump_dir: write what the
    last timed step returned there (dump_outputs)."""
    class _A:      # the names the body below was written against
        pass
    args = _A()
    args.config, args.batch, args.dtype, args.steps, args.warmup, args.no_roofline = config, batch_arg, dtype_arg, steps, warmup, not want_roofline
    import tante_amd
    from tante_amd import kernels as K
    cfg = tante_amd.load_config(args.config)
    wl = cfg["workload"]
    tgt = cfg["model"]["_target_"]
    kind = "cvit" if tgt.endswith("CViT") else ("fno" if tgt.endswith("FNO") else ("tante_fno" if cfg["model"].get("enc_dec_type", "cnn") == "fno" else "tante"))
    B = args.batch or wl["batch_size"]
    # CViT predicts all out_steps frames in ONE model call (trainer/trainer.py:161-172, `cvit: False` full-grid mode): a step = one call
    n_steps = cfg["model"]["out_steps"] if kind == "cvit" else wl["n_steps_rollout"]
    T_in = wl["n_steps_input"]
    res = tuple(wl["spatial_resolution"])
    D = wl["n_fields"]
    dtype = args.dtype or {"bfloat16": "bf16", "float32": "fp32"}[wl.get("amp", "bfloat16")]
    md = tante_amd.TanteMetadata(n_fields=D, spatial_resolution=res)
    torch.manual_seed(cfg.get("seed", 211))
    model = tante_amd.build_model(cfg, md).to(dev).eval()
    if kind == "fno":      # models.FNO has no compute switch: the reference's AMP context selects bf16 (the spectral layers stay fp32 either way)
        import contextlib
        amp = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if dtype == "bf16" else contextlib.nullcontext
    else:
        model.set_compute(dtype)
    gen = torch.Generator().manual_seed(cfg.get("seed", 211) + rank)
    batch = {"input": torch.randn(B, T_in, *res, D, generator=gen).to(dev),          # channels-last, like the dataset
             "output": torch.randn(B, n_steps, *res, D, generator=gen).to(dev)}
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)

    x_cvit = fmt.process_input(batch)[0][0].to(dev) if kind == "cvit" else None

    def step():      # -> what a caller of the timed path receives: CViT's prediction, a rollout's (y_pred, y_ref)
        with torch.inference_mode():
            if kind == "cvit":
                return model(x_cvit)
            if kind == "fno":
                with amp():
                    return tante_amd.rollout_model(model, batch, fmt, n_steps, device=dev)
            return tante_amd.rollout_model(model, batch, fmt, n_steps, device=dev)

    # graph: False = the eager loop, True = tante_amd.GraphedRollout (one captured HIP graph per rollout), "auto" = decided in the warm-up:
    # the eager loop unless the captured rollout is clearly (> 2 %) faster -- small batches and busy hosts, where the host's ~100 launches
    # per rollout are the bottleneck, not the device
    graph_note = "off"
    eager_step = step
    graph_step = None
    if graph:
        try:
            if kind in ("tante", "tante_fno"):       # the product's own captured rollout (tante_amd.GraphedRollout)
                roll = tante_amd.GraphedRollout(model, batch, fmt, n_steps, device=dev)

                def graph_step():
                    return roll(batch)
            else:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(2):
                        eager_step()                      # packs, tables, workspaces and allocator pools exist before the capture
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                g_ = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_):
                    g_out = eager_step()

                def graph_step():
                    g_.replay()
                    return g_out
            graph_note = "on"
            step = graph_step
        except Exception as e:      # noqa: BLE001
            graph_note = f"capture failed ({type(e).__name__}: {e}): eager"
            step, graph_step = eager_step, None
    if graph == "auto" and graph_step is not None:
        def pair_ms(fn):
            fn()
            torch.cuda.synchronize(dev)
            t_ = time.perf_counter()
            fn(); fn()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t_) * 500.0
        te, tg = pair_ms(eager_step), pair_ms(graph_step)
        te = min(te, pair_ms(eager_step))      # (the first pair also pays the clock ramp: eager is timed on both sides of the captured pair)
        step = graph_step if tg < 0.98 * te else eager_step
        graph_note = f"auto: eager {te:.3f} ms, captured {tg:.3f} ms per rollout in the warm-up -> {'captured' if step is graph_step else 'eager'}"

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    last = [None]
    if dump_dir is not None:      # keep each step's result (from the warm-up on, so the allocator holds both generations before timing)
        run_step = step

        def step():
            last[0] = run_step()
    for _ in range(args.warmup):
        step()
    clk0 = shader_clock_mhz(dev.index or 0)
    elapsed, regions, n_ramp = timed_regions(step, args.steps, reps, sync, dist, dev, ramp_s=0.5 if reps > 1 else 0.0)
    clk1 = shader_clock_mhz(dev.index or 0)
    dumped = None
    if dump_dir is not None:      # the last timed step's result, read before anything else runs (graph outputs are overwritten by a replay)
        dumped = dump_outputs(last[0], ("y",) if kind == "cvit" else ("y_pred", "y_ref"), dump_dir)
        last[0] = None
    frames = B * n_steps * args.steps * world
    value = frames / elapsed
    timing = {"reps": len(regions), "statistic": "median region" if len(regions) > 1 else "single region", "ramp_steps_untimed": n_ramp,
              "ms_per_step_min": round(1e3 * regions[0] / args.steps, 4), "ms_per_step_max": round(1e3 * regions[-1] / args.steps, 4),
              "spread_pct": round(100.0 * (regions[-1] - regions[0]) / elapsed, 2), "sclk_mhz_before": clk0, "sclk_mhz_after": clk1}

    roofline = None
    if not args.no_roofline and rank == 0:
        # instrumented pass: HIP events (recorded on the launch stream) around every launch of the matrix kernels;
        # the roofline entry is the kernel with the largest total time.  FLOPs are algorithmic.
        prof = {}

        def timed(name, fn, flops_of, name_of=None):
            def wrapper(*a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*a, **kw)
                e1.record()
                prof.setdefault(name_of(*a, **kw) if name_of else name, []).append((e0, e1, flops_of(*a, **kw)))
                return r
            return wrapper

        # the T-letter launch that also carries the temporal propagator (block_fs_kernel<..., TPROP = true>: two more passes over its rows
        # on fp32 4x4x1 MFMAs, not counted in its FLOPs) is a kernel of its own in a rocprof trace: keep it apart from the plain block kernel
        def block_name(x, st, C_, nh, hidden, seq, causal, eps, tprop=None):
            return ("fused_block_kernel + temporal propagator (T letter: tprop+LN1+QKV+attention+out-proj+res, LN2+fc1+GELU+fc2+res)" if tprop is not None
                    else "fused_block_kernel (LN1+QKV+attention+out-proj+res, LN2+fc1+GELU+fc2+res)")

        def fl_block(x, st, C_, nh, hidden, seq, causal, eps, tprop=None):
            # (the temporal propagator a T-letter launch carries -- tprop, 64 flops per element on fp32 4x4x1 MFMAs -- is not counted)
            n_tok = x.numel() // C_
            attn = 2.0 * (seq.L + 1) * C_ if causal else 4.0 * seq.L * C_
            return n_tok * (2.0 * C_ * 3 * C_ + attn + 2.0 * C_ * C_ + 4.0 * C_ * hidden)

        def fl_lin(a, pw, out, **kw):
            M = kw.get("M") or (a.numel() // pw.K)
            return 2.0 * M * pw.N * pw.K
        def fl_xattn(q, k, v, o, n_batch, n_head, D_, Lq, Lk, *a, **kw):
            return 4.0 * n_batch * n_head * Lq * Lk * D_

        def by_spectral(x, w_re, *a, **kw):          # HBM-bound: algorithmic bytes = the layer's input read once + its output written once
            n_, Cin, H_, W_ = x.shape
            return 4.0 * n_ * (Cin + w_re.shape[1]) * H_ * W_
        def fl_chain(a, resid, w, bias, eps_ln2, M, out, tail=None):      # out_proj + fc1 + fc2 (+ the Mlp's dense layer + the output layer)
            return 2.0 * M * 512 * 512 * (3 if tail is None else 4) + (0.0 if tail is None else 2.0 * M * 512 * tail[6])

        def chain_name(a, resid, w, bias, eps_ln2, M, out, tail=None):
            return ("chain512_kernel<1> (CViT block tail + model tail: out-proj+res, LN2+fc1+GELU+fc2+res, norm2, dense+GELU+res, LN, output layer)" if tail is not None
                    else "chain512_kernel<0> (CViT block tail: out-proj+res, LN2+fc1+GELU+fc2+res)")
        def fl_head_enc(rows, a_n0, a_s1, a_s0, a_off, n_img, Hp, Wp, C_, D_, *a, **kw):
            tok = n_img * Hp * Wp      # per token: n_ord x [4 C (C/2) + 16 (C/2)(C/4) + 64 (C/4) D] heads, + the encoder back: 16 (4 D)(C/4) + 4 C (C/2) + 2 C C
            head = len(rows) * 2.0 * (4 * C_ * C_ // 2 + 16 * (C_ // 2) * (C_ // 4) + 64 * (C_ // 4) * D_)
            enc = 2.0 * (16 * 4 * D_ * (C_ // 4) + 4 * C_ * (C_ // 2) + 2 * C_ * C_) if kw.get("enc_stream") is not None else 0.0
            return tok * (head + enc)

        def head_enc_name(*a, **kw):
            return ("head_enc_kernel (derivative heads of every order + Taylor sum + re-encoding of the predicted frame)" if kw.get("enc_stream") is not None
                    else "head_enc_kernel (derivative heads of every order + Taylor sum)")
        saved = (K.block_fused, K.linear, K.cross_attention, K.spectral_layer)
        saved_chain = K.cvit_chain512
        saved_he = K.head_enc_fused
        K.head_enc_fused = timed("head_enc_kernel", K.head_enc_fused, fl_head_enc, head_enc_name)
        K.cvit_chain512 = timed("chain512_kernel", K.cvit_chain512, fl_chain, chain_name)
        K.block_fused = timed("fused_block_kernel", K.block_fused, fl_block, block_name)
        K.linear = timed("gemm_kernel (token-stationary projection GEMM)", K.linear, fl_lin)
        K.cross_attention = timed("xattn_mfma_kernel (cross / self attention of CViT)", K.cross_attention, fl_xattn)
        K.spectral_layer = timed("spectral_layer (truncated DFT on fp32 MFMA: row DFT, column DFT, mode mixing, inverse column DFT, inverse row DFT + 1x1 conv + act)", K.spectral_layer, by_spectral)
        try:
            eager_step()      # (a captured rollout replays without passing through the wrappers)
            torch.cuda.synchronize()
        finally:
            K.block_fused, K.linear, K.cross_attention, K.spectral_layer = saved
            K.cvit_chain512 = saved_chain
            K.head_enc_fused = saved_he
        tot = {k: (sum(e0.elapsed_time(e1) for e0, e1, _ in v), sum(f for _, _, f in v), len(v)) for k, v in prof.items()}
        name = max(tot, key=lambda k: tot[k][0])
        ms, fl, n = tot[name]
        ach = fl / (ms * 1e-3) / 1e12
        # HBM bytes per launch of that kernel from the committed PMC passes (profiles/r01_pmc_rollout.json: separate
        # `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs of this command, FETCH_SIZE doubled per the gfx950 note of
        # MI355X_MICROARCH.md); bench.py itself cannot run the profiler, so the figure is null when the file is absent.
        traffic = traffic_source = None
        try:
            with open(os.path.join(ROOT, "profiles", PMC_FILE)) as f:
                pm = json.load(f)
            if name.startswith("fused_block") and dtype == "bf16" and os.path.basename(args.config) == pm.get("config", "tante_am.yaml"):
                traffic = pm["fused_block_kernel"]["hbm_bytes_per_launch"]
                # the counters come from a separate rocprofv3 --pmc pass (tools/collect_profiles.sh), not from this run: say which
                traffic_source = {"file": "profiles/" + PMC_FILE, "kernel_source_sha16": pm.get("kernel_source_sha16"),
                                  "current_kernel_source_sha16": _sha16(os.path.join(ROOT, "tante_amd", "csrc", "block_sliced.hip"))}
                traffic_source["stale"] = traffic_source["kernel_source_sha16"] != traffic_source["current_kernel_source_sha16"]
        except (OSError, KeyError, ValueError):
            pass
        try:      # cfg5: the spectral path's HBM bytes per SpectralLayer call (its five kernels), same rules
            with open(os.path.join(ROOT, "profiles", "r06_pmc_fno.json")) as f:
                pf = json.load(f)
            if name.startswith("spectral") and os.path.basename(args.config) == pf.get("config"):
                traffic = pf["spectral_layer"]["hbm_bytes_per_call"]
                traffic_source = {"file": "profiles/r06_pmc_fno.json", "kernel_source_sha16": pf.get("kernel_source_sha16"),
                                  "current_kernel_source_sha16": _sha16(os.path.join(ROOT, "tante_amd", "csrc", "spectral_dft.hip"))}
                traffic_source["stale"] = traffic_source["kernel_source_sha16"] != traffic_source["current_kernel_source_sha16"]
        except (OSError, KeyError, ValueError):
            pass
        others = {k: {("TB/s" if k.startswith("spectral") else "TFLOP/s"): round(v[1] / (v[0] * 1e-3) / 1e12, 3), "avg_launch_us": round(1e3 * v[0] / v[2], 2),
                      "launches": v[2]} for k, v in tot.items() if k != name}
        if name.startswith("spectral"):              # cfg5: the FFT passes are HBM-bound; `achieved` in algorithmic GB/s against 8 TB/s
            roofline = {"bound": "hbm", "kernel": name, "achieved": round(ach * 1e3, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(ach * 1e3 / 8000.0, 4), "traffic": traffic, "traffic_source": traffic_source, "launches": n,
                        "avg_launch_us": round(1e3 * ms / max(1, n), 2), "others": others}
        else:
            roofline = {"bound": "mfma", "kernel": name, "achieved": round(ach, 2), "peak": PEAK_TFLOPS[dtype], "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_TFLOPS[dtype], 4), "traffic": traffic, "traffic_source": traffic_source, "launches": n,
                        "avg_launch_us": round(1e3 * ms / max(1, n), 2), "others": others}
        if kind == "cvit":
            # whole forward against the algorithmic work of SURVEY 8d: every dense contraction as written EXCEPT the grid embedding, which
            # the reference evaluates as a dense 65 536 x 16 384 x 512 product (1 104 GFLOP) and this build evaluates exactly on the ~50
            # non-zero weights per query (grid_embed_kernel) and caches for the default full-grid queries: it is NOT in the timed forward
            alg = sum(v[1] for v in tot.values())
            roofline["whole_forward"] = {"algorithmic_gflop": round(alg / 1e9, 1), "ms": round(1e3 * elapsed / args.steps, 3),
                                         "TFLOP/s": round(alg / (elapsed / args.steps) / 1e12, 2),
                                         "frac": round(alg / (elapsed / args.steps) / 1e12 / PEAK_TFLOPS[dtype], 4),
                                         "note": "FLOPs of the launches as executed: the grid embedding (input-independent) is cached outside the timed "
                                                 "forward (dense-as-written it would add 1 104 GFLOP per forward), and so is the decoder's LayerNorm1 + "
                                                 "query projection of those coordinate queries (as written: once per sample, 34 GFLOP each); both "
                                                 "are rebuilt when a weight changes"}

    return {"value": value, "elapsed": elapsed, "roofline": roofline, "model": model, "batch": batch, "cfg": cfg, "wl": wl, "kind": kind, "B": B,
            "n_steps": n_steps, "T_in": T_in, "res": res, "D": D, "dtype": dtype, "graph": graph_note, "timing": timing, "dumped": dumped}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag must agree")
    # TANTE_DIST_BACKEND=gloo TANTE_ALL_ON_GPU0=1: every rank on GPU 0, collectives through gloo -- the N-rank code path (sharding,
    # broadcast, the all-reduce beside the captured graph, MAX-reduced timing, weak / strong lines) end to end on a 1-GPU box.
    # PLUMBING, NOT PERFORMANCE: the ranks share one GPU and gloo stages through the host; the line says so.
    backend = os.environ.get("TANTE_DIST_BACKEND", "nccl")
    plumbing = os.environ.get("TANTE_ALL_ON_GPU0") == "1"
    if plumbing and backend == "nccl" and world > 1:
        raise SystemExit("bench.py: TANTE_ALL_ON_GPU0=1 needs TANTE_DIST_BACKEND=gloo (RCCL cannot put two ranks on one device)")
    if plumbing:
        local = 0
    if local >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: LOCAL_RANK {local} but only {torch.cuda.device_count()} GPU(s) are visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    leg = rollout_leg(args.config, args.batch, args.dtype, args.steps, args.warmup, dev, rank, world, dist, args.full and not args.no_roofline,
                      graph=True if args.graph else (False if (args.no_graph or world > 1) else "auto"),      # (multi-rank runs: eager unless asked)
                      reps=args.reps, dump_dir=args.dump_outputs if rank == 0 else None)
    if leg["dumped"] is not None:
        for name, (shape, n) in leg["dumped"].items():
            print(f"bench.py: {args.dump_outputs}/{name}.npy: {n} of the {shape} output's elements"
                  + ("" if n == torch.Size(shape).numel() else f" (sample seeded {DUMP_SEED})"), file=sys.stderr)
    import tante_amd
    from tante_amd import kernels as K
    value, elapsed, roofline, model, batch, cfg, wl, kind = (leg[k] for k in ("value", "elapsed", "roofline", "model", "batch", "cfg", "wl", "kind"))
    B, n_steps, T_in, res, D, dtype = (leg[k] for k in ("B", "n_steps", "T_in", "res", "D", "dtype"))
    graph_mode, timing_main = leg["graph"], leg["timing"]

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    train = None
    if args.full and not args.no_train and kind == "tante" and os.path.basename(args.config) == "tante_am.yaml":
        # second leg of the metric: train-step samples/sec on cfg3 (TRL-2D shaped fields, 4-step BPTT, MSE + clip + AdamW, one summed
        # all-reduce of the flat gradient bucket per step when N > 1), weak (8 samples per GPU) and strong (global batch 64)
        tcfg = tante_amd.load_config(os.path.join(ROOT, "configs", "tante_trl.yaml"))
        twl = tcfg["workload"]
        tmd = tante_amd.TanteMetadata(n_fields=twl["n_fields"], spatial_resolution=tuple(twl["spatial_resolution"]))
        drop = float(os.environ.get("TANTE_TRAIN_DROPOUT", tcfg["model"].get("dropout", 0.0)))
        oc = tcfg["optimizer"]
        tn = twl["n_steps_output"]
        tfmt = tante_amd.DefaultChannelsFirstFormatter(tmd)
        flops_sample = train_flops_per_sample(tcfg, twl)

        def train_leg(tB, n_timed):
            torch.manual_seed(tcfg.get("seed", 211))
            tmodel = tante_amd.build_model(tcfg, tmd, dropout=drop).to(dev).train().set_compute(dtype)
            opt = tante_amd.FlatAdamW(tmodel.parameters(), lr=oc["lr"], weight_decay=oc["weight_decay"], max_norm=1.0)
            opt.broadcast_parameters(0)                                         # every rank starts from rank 0's weights
            tgen = torch.Generator().manual_seed(1000 + rank)
            tbatch = {"input": torch.randn(tB, twl["n_steps_input"], *twl["spatial_resolution"], twl["n_fields"], generator=tgen).to(dev),
                      "output": torch.randn(tB, tn, *twl["spatial_resolution"], twl["n_fields"], generator=tgen).to(dev)}
            # zero_grad + rollout + loss + backward replayed as one HIP graph (tante_amd.GraphedTrainStep: fresh dropout masks per step
            # through a device-resident seed word; all-reduce, clip and AdamW stay ordinary launches); TANTE_TRAIN_GRAPH=0, or a capture
            # that fails, leaves the eager step
            step_fn, graph_note = (lambda: tante_amd.train_step(tmodel, opt, tbatch, tfmt, tn, world)), "off"
            graphed = None
            if os.environ.get("TANTE_TRAIN_GRAPH", "1") != "0":
                try:
                    graphed = tante_amd.GraphedTrainStep(tmodel, opt, tbatch, tfmt, tn, world, seed=tcfg.get("seed", 211) + rank)
                    step_fn, graph_note = (lambda: graphed(tbatch)), "on"
                except Exception as e:      # noqa: BLE001
                    graph_note = f"capture failed ({type(e).__name__}: {e}): eager"
            for _ in range(3 if tB <= 16 else 1):                              # warm-up (packs, allocator pools, workspace slabs)
                step_fn()
            # the same protocol as the rollout leg: median of `reps` regions of exactly n_timed steps behind a ramp
            t_reps = max(1, min(args.reps, 5)) if tB <= 16 else 1
            tel, tregions, _ = timed_regions(step_fn, n_timed, t_reps, sync, dist, dev, ramp_s=0.3 if t_reps > 1 else 0.0)
            nbytes = opt.numel * 4
            if graphed is not None:
                graphed.close()
            del graphed, step_fn, tmodel, opt, tbatch
            torch.cuda.empty_cache()
            sps = tB * world * n_timed / tel
            return {"value": round(sps, 2), "unit": "samples/s", "ms_per_step": round(1e3 * tel / n_timed, 2), "global_batch": tB * world,
                    "batch_per_gpu": tB, "steps": n_timed, "hip_graph": graph_note,
                    "timing": {"reps": len(tregions), "statistic": "median region" if len(tregions) > 1 else "single region",
                               "ms_per_step_min": round(1e3 * tregions[0] / n_timed, 3), "ms_per_step_max": round(1e3 * tregions[-1] / n_timed, 3)},
                    "roofline": {"bound": "mfma", "achieved": round(sps * flops_sample / world / 1e12, 2), "peak": PEAK_TFLOPS[dtype],
                                 "unit": "TFLOP/s per GPU", "frac": round(sps * flops_sample / world / 1e12 / PEAK_TFLOPS[dtype], 4),
                                 "algorithmic_gflop_per_sample": round(flops_sample / 1e9, 1)}}, nbytes

        weak, nbytes = train_leg(twl["batch_size"], args.train_steps)
        train = {"metric": "train-step samples/sec, TANTE on 128x384 TRL-2D (4-step BPTT, MSE, clip, AdamW)", "scaling": "weak", **weak,
                 "dropout": drop,
                 "collective": ("%s all-reduce(sum) of the flat fp32 gradient bucket, %d bytes per step in %d call(s) of %s elements, %.2f of them issued "
                                "beside compute (dist.GradAllReduce: what the end-of-pass weight-gradient flush does not write when the flush starts, "
                                "the spans of each flush segment while the next one runs, the last segment's behind it; the ranks agreed on the call "
                                "list once); 1/world folded into clip + AdamW [%s]; UNMEASURED on more than one GPU in this round"
                                % ("RCCL" if backend == "nccl" else backend, nbytes, len(tante_amd.dist.LAST_CALLS), list(tante_amd.dist.LAST_CALLS),
                                   tante_amd.dist.LAST_OVERLAPPED[0], tante_amd.dist.collective_info())) if world > 1 else None}
        if 64 % world == 0 and not args.no_train_strong:
            strong, _ = train_leg(64 // world, max(1, args.train_steps if world > 1 else 2))
            train["strong"] = {"scaling": "strong", **strong}

    cpu = None
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1 and kind not in ("cvit", "fno"):      # (cfg4: the `workloads` object's own CPU leg)
        from oracle import tante_oracle as O
        mk = cfg["model"]
        ocfg = O.TanteCfg(mk["in_T"], D, res, taylor_order=mk.get("taylor_order", 1), frame_interval=mk.get("frame_interval", 1.0),
                          attn_axes=mk.get("attn_axes", "THWTHWTHW"), n_head=mk.get("n_head", 8), mlp_ratio=mk.get("mlp_ratio", 1.0),
                          embed_dim=mk.get("embed_dim", 256), patch_scale=mk.get("patch_scale", 32),
                          **({"enc_dec_type": "fno", "modes1": mk.get("modes1", 32), "modes2": mk.get("modes2", 32)} if kind == "tante_fno" else {}))
        w = {k: (v.detach().cpu() if v.is_complex() else v.detach().float().cpu()) for k, v in model.state_dict().items()}
        # BASELINE.md's protocol: the CPU path on all physical host cores.  The GPU box reports 256 hardware threads in the affinity
        # mask while one GPU job gets a 16-core share of the host, so BOTH are timed and reported: `value` is the run at
        # min(affinity, physical cores), `share_16` the run at the 16-thread share (TANTE_CPU_THREADS changes that number).
        affinity, cap = len(os.sched_getaffinity(0)), int(os.environ.get("TANTE_CPU_THREADS", "16"))
        phys = physical_cores()
        full = max(1, min(affinity, phys or affinity))
        cpu_name = "unknown"
        try:
            cpu_name = next(ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name"))
        except (OSError, StopIteration):
            pass

        def oracle_leg(threads, Bc, nc):
            torch.set_num_threads(threads)
            cb = {"input": batch["input"][:Bc].cpu(), "output": batch["output"][:Bc, :nc].cpu()}
            # the oracle in its fused-op spelling: the form tools/cpu_reference_time.py checks against the REAL reference's time on the same
            # tensors in the build container (profiles/cpu_reference.json: the oracle takes 1.09 x the reference's time, i.e. this
            # baseline is ~9 % SLOWER than the reference would be); the written-out spelling the parity tests use runs ~2x slower
            O.set_fast(True)
            try:
                with torch.no_grad():
                    O.rollout(w, ocfg, {"input": cb["input"][:1], "output": cb["output"][:1, :1]}, 1)      # warm-up
                    t0 = time.perf_counter()
                    O.rollout(w, ocfg, cb, nc)
                    tc = time.perf_counter() - t0
            finally:
                O.set_fast(False)
            return {"value": round(Bc * nc / tc, 3), "cores": torch.get_num_threads(), "seconds": round(tc, 1),
                    "sample": f"{Bc} samples x {nc} frames of the same workload, fp32"}
        legs = {}
        share = min(affinity, cap)
        for th in sorted({full, share}, reverse=True):
            # (the affinity mask of a GPU box lists every hardware thread of the host while the job's cgroup holds a 16-core share:
            # the all-physical-cores run oversubscribes that share and is the SLOWER one there -- it gets half the frames)
            legs[th] = oracle_leg(th, B, n_steps if th == share else max(1, n_steps // 2))
        best = max(legs, key=lambda th: legs[th]["value"])
        cpu = {"value": legs[best]["value"], "unit": "frames/s", "cores": legs[best]["cores"], "cpu_model": cpu_name, "kind": "port",
               "affinity_cores": affinity, "physical_cores": phys,
               "sample": "oracle rollout (fused-op spelling; it takes 1.09 x the reference's own CPU time on the same tensors: "
                         f"profiles/cpu_reference.json), {legs[best]['sample']}, {legs[best]['seconds']} s; `value` is the FASTER of the two thread "
                         "counts timed (BASELINE.md asks for all physical cores; the box's 16-core share is the other)",
               "threads_timed": {f"{th}{' = min(affinity, physical cores)' if th == full else ' = the 16-core share (TANTE_CPU_THREADS)'}": legs[th]
                                 for th in legs},
               "gpu_over_cpu": round(value / legs[best]["value"], 1)}

    workloads = None
    if (args.full and not args.no_workloads and rank == 0 and world == 1 and kind == "tante" and os.path.basename(args.config) == "tante_am.yaml"):
        # The other BASELINE configurations, compact, in the driver's own run (round-3 verdict item 7): cfg2 at B = 1 (eager and as ONE
        # captured graph), cfg4 at B = 1 / 4 with its whole-forward fraction and a CPU leg, cfg5 with its HBM roofline.  Short legs.
        del model, batch, leg
        torch.cuda.empty_cache()
        workloads = {}

        def compact(lg, steps):
            r = lg["roofline"] or {}
            o = {"value": round(lg["value"], 1), "unit": "frames/s", "ms_per_step": round(1e3 * lg["elapsed"] / steps, 3), "batch": lg["B"]}
            if lg["graph"] != "off":
                o["hip_graph"] = lg["graph"]
            if r:
                o["roofline"] = {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us") if k in r}
                o["roofline"]["kernel"] = r["kernel"].split(" (")[0]
                if "whole_forward" in r:
                    o["whole_forward"] = {k: r["whole_forward"][k] for k in ("algorithmic_gflop", "ms", "TFLOP/s", "frac")}
            return o
        try:
            # cfg2 at two and four resident rounds of the fused block kernel (B = 8 is exactly one round of 512 workgroups): the same model,
            # the same kernels, the block kernel's own roofline entry -- the curve DESIGN 4.1 reads the "one resident round" explanation from
            for tag, bb in (("cfg2_b16", 16), ("cfg2_b32", 32)):
                lg = rollout_leg(args.config, bb, args.dtype, 6 if bb == 16 else 4, 2, dev, rank, world, dist, True, graph=False, reps=3)
                workloads[tag] = compact(lg, 6 if bb == 16 else 4)
                workloads[tag]["timing"] = lg["timing"]
                del lg
                torch.cuda.empty_cache()
            for tag, gr in (("cfg2_b1", False), ("cfg2_b1_graph", True)):
                lg = rollout_leg(args.config, 1, args.dtype, 20, 4, dev, rank, world, dist, False, graph=gr)
                workloads[tag] = compact(lg, 20)
                del lg
            for tag, cfile, bb, st in (("cfg4_b1", "cvit_rb.yaml", 1, 30), ("cfg4_b4", "cvit_rb.yaml", 4, 12), ("cfg5", "tante_fno.yaml", None, 6)):
                lg = rollout_leg(os.path.join(ROOT, "configs", cfile), bb, None, st, 3, dev, rank, world, dist, True)
                workloads[tag] = compact(lg, st)
                if tag == "cfg4_b1" and not args.no_cpu_baseline:
                    workloads[tag]["cpu_baseline"] = cvit_cpu_leg(lg, workloads[tag]["value"])
                del lg
                torch.cuda.empty_cache()
                if tag == "cfg4_b1":      # 47 launches of 10-30 us each: near the host's issue rate on a busy box; as one captured graph
                    lg = rollout_leg(os.path.join(ROOT, "configs", cfile), bb, None, st, 3, dev, rank, world, dist, False, graph=True)
                    workloads["cfg4_b1_graph"] = compact(lg, st)
                    wf = workloads["cfg4_b1"].get("whole_forward")
                    if wf:      # the same algorithmic work over the graph-replayed time (the eager leg above is host-bound at 46 launches)
                        ms_g = workloads["cfg4_b1_graph"]["ms_per_step"]
                        tf = wf["algorithmic_gflop"] / ms_g      # GFLOP / ms = TFLOP/s
                        workloads["cfg4_b1_graph"]["whole_forward"] = {"algorithmic_gflop": wf["algorithmic_gflop"], "ms": ms_g,
                                                                       "TFLOP/s": round(tf, 1), "frac": round(tf / PEAK_TFLOPS["bf16"], 4)}
                    del lg
                    torch.cuda.empty_cache()
        except Exception as e:      # noqa: BLE001 -- a side leg must never cost the headline line
            workloads["error"] = f"{type(e).__name__}: {e}"

    if rank == 0:
        title = {"tante": "rollout frames/sec (fwd), TANTE on 256x256 Active Matter" if os.path.basename(args.config).startswith("tante_am")
                 else "rollout frames/sec (fwd), TANTE (%s)" % os.path.basename(args.config),
                 "cvit": "frames/sec (fwd, full-grid queries), CViT on Rayleigh-Benard 512x128",
                 "tante_fno": "rollout frames/sec (fwd), TANTE with the spectral encoder/decoder on 512x512x8",
                 "fno": "rollout frames/sec (fwd), models.FNO (configs/fno.yaml model block) on 512x512x8"}[kind]
        out = {"metric": title, "value": round(value, 2), "unit": "frames/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic", "full": args.full,
               "config": {"workload": os.path.basename(args.config), "fields": D, "resolution": list(res), "batch_per_gpu": B,
                          "n_steps_input": T_in, "n_steps_rollout": n_steps, "taylor_order": cfg["model"].get("taylor_order", 1),
                          "attn_axes": cfg["model"].get("attn_axes"), "parallelism": f"batch-sharded x{world} (no collective)",
                          "hip_graph": graph_mode, "timing": timing_main,
                          "h2d": "excluded (the window is resident in HBM when the timed region starts); PCIe-inclusive, a host-resident window of "
                                 "%.1f MB per sample over PCIe Gen5 x16 (63 GB/s): ~%.0f frames/s" % (
                                     T_in * D * res[0] * res[1] * 4 / 1e6,
                                     B * n_steps / (1e-3 * 1e3 * elapsed / args.steps + B * T_in * D * res[0] * res[1] * 4 / 63e9))},
               "roofline": roofline, "cpu_baseline": cpu, "train": train, "workloads": workloads}
        # Scalar top-level copies of the other half of the metric and of the side workloads (round-5 verdict item 3: the driver's `parsed`
        # record keeps scalar top-level keys only; the nested objects above stay the full account).
        def _dig(o, *path):
            for k in path:
                if not isinstance(o, dict) or o.get(k) is None:
                    return None
                o = o[k]
            return o
        out["roofline_frac"] = _dig(roofline, "frac")
        out["roofline_avg_launch_us"] = _dig(roofline, "avg_launch_us")
        out["train_samples_per_s"] = _dig(train, "value")
        out["train_ms_per_step"] = _dig(train, "ms_per_step")
        out["train_roofline_frac"] = _dig(train, "roofline", "frac")
        out["train_global_batch"] = _dig(train, "global_batch")
        out["train_b64_ms_per_step"] = _dig(train, "strong", "ms_per_step")
        out["train_b64_samples_per_s"] = _dig(train, "strong", "value")
        out["cfg2_b32_roofline_frac"] = _dig(workloads, "cfg2_b32", "roofline", "frac")
        out["cfg4_b1_ms"] = _dig(workloads, "cfg4_b1_graph", "ms_per_step") or _dig(workloads, "cfg4_b1", "ms_per_step")
        out["cfg4_b1_whole_forward_frac"] = (_dig(workloads, "cfg4_b1_graph", "whole_forward", "frac")
                                             or _dig(workloads, "cfg4_b1", "whole_forward", "frac"))
        out["cfg4_b4_ms"] = _dig(workloads, "cfg4_b4", "ms_per_step")
        out["cfg5_frames_per_s"] = _dig(workloads, "cfg5", "value")
        out["cfg5_roofline_frac"] = _dig(workloads, "cfg5", "roofline", "frac")
        _t5, _a5, _us5 = _dig(workloads, "cfg5", "roofline", "traffic"), _dig(workloads, "cfg5", "roofline", "achieved"), _dig(workloads, "cfg5", "roofline", "avg_launch_us")
        out["cfg5_traffic_over_algorithmic"] = round(_t5 / (_a5 * 1e9 * _us5 * 1e-6), 3) if (_t5 and _a5 and _us5) else None
        if plumbing or (world > 1 and backend != "nccl"):
            out["plumbing"] = (f"NOT A PERFORMANCE NUMBER: {world} ranks share GPU 0 and the collectives go through '{backend}' "
                               "(TANTE_ALL_ON_GPU0 / TANTE_DIST_BACKEND); run to exercise the multi-rank code path only")
            out["config"]["parallelism"] = f"batch-sharded x{world} on ONE GPU over {backend} (plumbing run)"
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
