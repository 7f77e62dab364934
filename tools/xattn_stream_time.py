"""A/B timing of tante_cross_attention in bf16 beyond the old matrix-pipe window (head dim 64 with more than 512 keys, head dim 32):
the default route (kernels.cross_attention_route: resident or streamed MFMA kernel) against TANTE_XATTN_VALU = 1, the exact
lane-per-query kernel these shapes took before.  Also D = 32 at 1 024 keys resident against TANTE_XATTN_STREAM = 1, the evidence for
where the resident cap sits.

    python tools/xattn_stream_time.py [--rounds 5] [--out profiles]

The arms of a shape alternate inside every round (other work shares the machine); a figure is the MEDIAN over the rounds of the mean
call time in a window of >= 50 ms, by device events.  FLOP = 4 nb nh Lq Lk D (scores and P V).  Writes <out>/xattn_stream_ab.json
and .log, and compares the two arms' outputs at the timed size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tante_amd import _lib as L, kernels as K  # noqa: E402

SHAPES = [  # label, nb, nh, D, Lq, Lk, packed, note
    ("a", 1, 8, 64, 262144, 1024, False, "decoder, 512 x 512 field at patch 16"),
    ("b", 4, 8, 64, 1024, 1024, True, "encoder self-attention at the same size (packed q|k|v)"),
    ("c", 4, 8, 32, 65536, 256, False, "the default constructor (8 x 32) at 256 x 256, resident"),
    ("d", 4, 8, 32, 65536, 2048, False, "head dim 32, streamed"),
]
CAP = ("cap", 4, 8, 32, 65536, 1024, False, "head dim 32 at the resident cap: resident against forced stream")


def make(nb, nh, D, Lq, Lk, packed):
    C = nh * D
    g = torch.Generator(device="cuda").manual_seed(Lq + Lk + D)
    o = torch.empty(nb * Lq, C, dtype=torch.bfloat16, device="cuda")
    if packed:
        buf = torch.randn(nb * Lq, 3 * C, device="cuda", generator=g).to(torch.bfloat16)
        return o, lambda: K.cross_attention(buf, buf[:, C:], buf[:, 2 * C:], o, nb, nh, D, Lq, Lk, 3 * C, 3 * C, C)
    q = torch.randn(nb * Lq, C, device="cuda", generator=g).to(torch.bfloat16)
    kv = torch.randn(nb * Lk, 2 * C, device="cuda", generator=g).to(torch.bfloat16)
    return o, lambda: K.cross_attention(q, kv, kv[:, C:], o, nb, nh, D, Lq, Lk, C, 2 * C, C)


def window(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3      # us per call


def ab(shape, arms, rounds, log):
    """arms: [(name, option or None)]; the option is set to 1 for that arm's calls only."""
    label, nb, nh, D, Lq, Lk, packed, note = shape
    o, f = make(nb, nh, D, Lq, Lk, packed)
    flop = 4.0 * nb * nh * Lq * Lk * D
    res, outs = {}, {}
    for name, opt in arms:                    # warm-up, the call count of a >= 50 ms window, and the arm's output
        if opt:
            L.set_option(opt, 1)
        try:
            route = K.cross_attention_route(torch.bfloat16, D, Lk)
            f()
            torch.cuda.synchronize()
            one = window(f, 2)
            outs[name] = o.float().clone()
        finally:
            if opt:
                L.set_option(opt, 0)
        res[name] = {"route": route, "calls_per_window": max(2, int(50e3 / one) + 1), "rounds_us": []}
    for _ in range(rounds):
        for name, opt in arms:
            if opt:
                L.set_option(opt, 1)
            try:
                res[name]["rounds_us"].append(window(f, res[name]["calls_per_window"]))
            finally:
                if opt:
                    L.set_option(opt, 0)
    for name, _ in arms:
        r = res[name]
        r["median_us"] = statistics.median(r["rounds_us"])
        r["min_us"], r["max_us"] = min(r["rounds_us"]), max(r["rounds_us"])
        r["tflops"] = flop / r["median_us"] / 1e6
    (n0, _), (n1, _) = arms
    ref = outs[n1]
    diff = float((outs[n0] - ref).norm() / ref.norm())
    ratio = res[n1]["median_us"] / res[n0]["median_us"]
    log(f"({label}) nb {nb} nh {nh} D {D} Lq {Lq} Lk {Lk}{' packed' if packed else ''} -- {note}")
    for name, _ in arms:
        r = res[name]
        log(f"    {name:<14s} route {r['route']:<8s} median {r['median_us']:10.1f} us  (min {r['min_us']:.1f}, max {r['max_us']:.1f}, "
            f"{rounds} rounds x {r['calls_per_window']} calls)  {r['tflops']:7.1f} TFLOP/s")
    log(f"    {n1} / {n0} = {ratio:.2f}x; outputs differ by {diff:.2e} relative L2")
    return {"label": label, "nb": nb, "nh": nh, "D": D, "Lq": Lq, "Lk": Lk, "packed": packed, "note": note, "flop": flop, "arms": res,
            "ratio": {"of": f"{n1} / {n0}", "value": ratio}, "outputs_rel_l2": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xattn_stream_time.py needs a GPU")
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f"tante_cross_attention bf16, {torch.cuda.get_device_name(0)}; median of {a.rounds} interleaved rounds, device events")
    results = [ab(s, [("default", None), ("forced_valu", "TANTE_XATTN_VALU")], a.rounds, log) for s in SHAPES]
    results.append(ab(CAP, [("resident", None), ("forced_stream", "TANTE_XATTN_STREAM")], a.rounds, log))
    with open(os.path.join(a.out, "xattn_stream_ab.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": results}, fh, indent=1)
    with open(os.path.join(a.out, "xattn_stream_ab.log"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
