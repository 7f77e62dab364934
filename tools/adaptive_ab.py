"""A/B timing of the adaptive-step tail (csrc/adaptive_tail.hip): TANTE_ADAPTIVE_TAIL on against off, in one process and one build.

The model is cfg2 (configs/tante_am.yaml: 256 x 256, 11 fields, order 3, THW-THW-THW, C = 256, bf16) built with deg=False; the
interprators' last layer is steepened (weight x 60, bias + 2.2, as the adaptive tests do) so that the step sizes are not pinned to a clamp.
Timed, at B = 8 and B = 1:
  call     one model call at out_T = 1.5 (R_Trainer's; one frame) and out_T = 8 (R_Evaler's cap; the frames it returns are printed)
  rollout  rollout_adaptive(model, batch, formatter, 8, 8.0, per_sample=False): R_Evaler's loop, 8 frames
Both switch positions alternate behind a warm-up; a region is `--calls` calls between two device synchronisations on the host clock (a
call ends in a host read of the frame count on either route, so the clock sees whole calls); the figure of a side is the median of its
regions, its spread (max - min) / median.  The new route counts as not slower when its median is below the off route's median plus the
off route's own spread.  Results of the two routes are compared on the timed inputs (frame counts equal, frames within the bf16 bar).

  python tools/adaptive_ab.py [--regions 9] [--calls 100] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tante_amd      # noqa: E402


def build(dev):
    torch.manual_seed(211)
    md = tante_amd.TanteMetadata(n_fields=11, spatial_resolution=(256, 256))
    m = tante_amd.TANTE(in_T=4, dset_metadata=md, taylor_order=3, frame_interval=1.0, attn_axes="THW-THW-THW", n_head=8, mlp_ratio=1.0, dropout=0.0,
                        enc_dec_type="cnn", embed_dim=256, patch_scale=8, overlap_ratio=0.0, deg=False).to(dev).eval().set_compute("bf16")
    with torch.no_grad():
        for it in m.interprators:
            it.interprete[4].weight.mul_(60.0)
            it.interprete[4].bias.add_(2.2)
    return m, md


def regions(fn, n_regions, calls):
    out = []
    for _ in range(n_regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


def ab(fn, n_regions, calls):
    """-> {"on": us, "off": us, spreads}: regions of the two switch positions alternate."""
    t = {1: [], 0: []}
    for sw in (1, 0):
        tante_amd.set_option("TANTE_ADAPTIVE_TAIL", sw)
        for _ in range(3):
            fn()
    for _ in range(n_regions):
        for sw in (1, 0):
            tante_amd.set_option("TANTE_ADAPTIVE_TAIL", sw)
            t[sw] += regions(fn, 1, calls)
    tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
    med = {sw: statistics.median(v) for sw, v in t.items()}
    spread = {sw: (max(v) - min(v)) / med[sw] for sw, v in t.items()}
    return {"on_us": round(med[1], 1), "off_us": round(med[0], 1), "on_spread": round(spread[1], 4), "off_spread": round(spread[0], 4),
            "not_slower": bool(med[1] <= med[0] * (1.0 + spread[0])), "speedup": round(med[0] / med[1], 4)}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_ab.py times GPU calls: no GPU here (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    m, md = build(dev)
    fmt = tante_amd.DefaultChannelsFirstFormatter(md)
    res = {"model": "cfg2 shape, deg=False", "regions": a.regions, "calls_per_region": a.calls, "cases": {}}
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in (8, 1):
            x = torch.randn(B, 4, 11, 256, 256, generator=g).to(dev)
            batch = {"input": x.permute(0, 1, 3, 4, 2).contiguous(), "output": torch.zeros(B, 8, 256, 256, 11, device=dev)}
            for out_T in (1.5, 8.0):
                assert m.adaptive_tail_route(out_T)
                y1, r1 = m(x, out_T)
                tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 0)
                y0, r0 = m(x, out_T)
                tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
                assert y1.shape == y0.shape, (y1.shape, y0.shape)
                last = x[:, -1:]
                r = ab(lambda: m(x, out_T), a.regions, a.calls)
                r.update(frames=int(y1.shape[1]), R_t=[round(float(v), 3) for v in r1.tolist()], frames_rel_on_vs_off=rel(y1 - last, y0 - last),
                         R_t_rel_on_vs_off=rel(r1, r0))
                res["cases"][f"call_B{B}_outT{out_T}"] = r
                print(f"call    B={B} out_T={out_T}: {json.dumps(r)}", flush=True)
            roll = lambda: tante_amd.rollout_adaptive(m, batch, fmt, 8, 8.0, per_sample=False)      # noqa: E731
            y1, _, r1 = roll()
            tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 0)
            y0, _, r0 = roll()
            tante_amd.set_option("TANTE_ADAPTIVE_TAIL", 1)
            assert y1.shape == y0.shape and r1.shape == r0.shape
            r = ab(roll, a.regions, max(1, a.calls // 4))
            r.update(model_calls=int(r1.numel() // B), frames_rel_on_vs_off=rel(y1, y0))
            res["cases"][f"rollout8_B{B}_outT8"] = r
            print(f"rollout B={B} 8 frames out_T=8: {json.dumps(r)}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
