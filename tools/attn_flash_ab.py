"""A/B timing of the flash attention kernels (csrc/attn_flash.hip) against the kernels that take the same calls by default.

Six pairs; the first four at cfg2's geometry (B = 8, T = 4, 32 x 32 patches, C = 256, 8 heads of dim 32, bf16, random operands):
  fwd_L   tante_attention (attn_long_kernel)        vs tante_attention_flash       letter 'L': 32 sequences of 1024
  fwd_A   the same                                  vs the same                    letter 'A': 8 sequences of 4096
  bwd_L   tante_attention_masked_bwd (lane per row) vs tante_attention_flash_bwd   dense 'L' shape, p = 0; o and the row statistics given
  bwd_L_routed   the same old kernel                vs flash forward into scratch + flash backward: what AttentionFn.backward runs on the
                 route TANTE_ATTN_FLASH=1 enables (the p = 0 forward saved no statistics, so the backward recomputes them)
and the masked pair, on the dense 'L' shape (32 sequences of 1024) under a shared boolean (L, L) attn_mask (30 % blocked, the diagonal
open) and a (Bp, L) key_padding_mask (the last 37 keys of every odd sample), p = 0:
  fwd_L_masked   tante_attention_masked (lane per row)     vs tante_attention_flash_masked
  bwd_L_masked   tante_attention_masked_bwd (lane per row) vs tante_attention_flash_masked_bwd   o and the row statistics given
(FLOP/s of the masked pair count the full L^2 products, blocked keys included: both sides compute them.)
One process, old and new alternating behind a warm-up; every region is timed with device events and holds enough calls for >= 0.2 s;
the figure of a kernel is the median of its regions (>= 7), its spread is (max - min) / median over those regions.  The new kernel counts
as faster when the gap between the medians exceeds the larger of the two spreads.  FLOP/s = 4 L^2 d per (sequence, head) for a forward
(x 2.5 for a backward: five products against two) over the time of one call.

  python tools/attn_flash_ab.py [--regions 7] [--seconds 0.2] [--out FILE.json] [--once] [--pairs fwd_L_masked,bwd_L_masked]
--once: one call of each kernel and nothing else (the program to put behind `rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tante_amd import _lib as L, kernels as K, attn_flash as FA      # noqa: E402

NH, CH, D = 8, 256, 32


def cases(dev):
    g = torch.Generator().manual_seed(0)
    out = []
    for name, seq in (("fwd_L", K.make_seq("L", 8, 4, 32, 32)), ("fwd_A", K.make_seq("A", 8, 4, 32, 32)), ("bwd_L", K.dense_seq(32, 1024))):
        n = seq.nseq * seq.L
        qkv = torch.randn(n, 3 * CH, generator=g).to(torch.bfloat16).to(dev)
        o = torch.empty(n, CH, dtype=torch.bfloat16, device=dev)
        flops = 4.0 * seq.L * seq.L * D * seq.nseq * NH
        if name.startswith("fwd"):
            old = lambda qkv=qkv, o=o, seq=seq: K.attention(qkv, o, CH, NH, seq, False)
            new = lambda qkv=qkv, o=o, seq=seq: FA.forward(qkv, o, None, CH, NH, seq, False)
        else:
            flops *= 2.5
            do = torch.randn(n, CH, generator=g).to(torch.bfloat16).to(dev)
            dqkv = torch.empty_like(qkv)
            st_old = torch.empty(n * NH * 3, dtype=torch.float32, device=dev)
            st_new = FA.new_stats(qkv, NH, seq)
            FA.forward(qkv, o, st_new, CH, NH, seq, False)
            s = torch.cuda.current_stream().cuda_stream

            def old(qkv=qkv, do=do, dqkv=dqkv, st=st_old, seq=seq):
                L.check(L.lib().tante_attention_masked_bwd(qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), L.BF16, CH, NH, seq.nseq, seq.L, 0, None, 0,
                                                           None, st.data_ptr(), s), "masked_bwd")
            new = lambda qkv=qkv, o=o, do=do, st=st_new, dqkv=dqkv, seq=seq: FA.backward(qkv, o, do, st, dqkv, CH, NH, seq, False)
        out.append((name, seq, flops, old, new))
        if name == "bwd_L":
            o2 = torch.empty_like(o)

            def routed(qkv=qkv, o2=o2, do=do, st=st_new, dqkv=dqkv, seq=seq):
                FA.forward(qkv, o2, st, CH, NH, seq, False)
                FA.backward(qkv, o2, do, st, dqkv, CH, NH, seq, False)
            out.append(("bwd_L_routed", seq, flops, old, routed))
    # the masked pair: what MaskedAttentionFn runs by default against what MaskedFlashAttentionFn runs
    seq = K.dense_seq(32, 1024)
    n = seq.nseq * seq.L
    am = torch.zeros(1, seq.L, seq.L).masked_fill_(((torch.rand(seq.L, seq.L, generator=g) < 0.3) & ~torch.eye(seq.L, dtype=torch.bool))[None],
                                                   float("-inf")).to(dev)
    kp = torch.zeros(seq.nseq, seq.L)
    kp[1::2, seq.L - 37:] = float("-inf")
    kp = kp.to(dev)
    qkv = torch.randn(n, 3 * CH, generator=g).to(torch.bfloat16).to(dev)
    do = torch.randn(n, CH, generator=g).to(torch.bfloat16).to(dev)
    o, dqkv = torch.empty(n, CH, dtype=torch.bfloat16, device=dev), torch.empty_like(qkv)
    st_old = torch.empty(n * NH * 3, dtype=torch.float32, device=dev)
    st_new = FA.new_stats(qkv, NH, seq)
    FA.forward(qkv, o, st_new, CH, NH, seq, False, 0.0, 0, am, kp)
    s = torch.cuda.current_stream().cuda_stream
    flops = 4.0 * seq.L * seq.L * D * seq.nseq * NH

    def old_bwd():
        L.check(L.lib().tante_attention_masked_bwd(qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), L.BF16, CH, NH, seq.nseq, seq.L, 0, am.data_ptr(), 0,
                                                   kp.data_ptr(), st_old.data_ptr(), s), "masked_bwd")
    out.append(("fwd_L_masked", seq, flops, lambda: K.attention_masked(qkv, o, CH, NH, seq.nseq, seq.L, False, am, kp),
                lambda: FA.forward(qkv, o, None, CH, NH, seq, False, 0.0, 0, am, kp)))
    out.append(("bwd_L_masked", seq, flops * 2.5, old_bwd, lambda: FA.backward(qkv, o, do, st_new, dqkv, CH, NH, seq, False, 0.0, 0, am, kp)))
    return out


def region(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--pairs", default=None, help="comma-separated pair names (default: all)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, seq, flops, old, new in cases(dev):
        if a.pairs and name not in a.pairs.split(","):
            continue
        if a.once:
            old()
            new()
            torch.cuda.synchronize()
            continue
        for fn in (old, new):      # warm-up
            region(fn, 3)
        calls = {}
        for k, fn in (("old", old), ("new", new)):      # enough calls for a region of a.seconds, checked on a region of that size
            n = max(3, int(a.seconds * 1e3 / region(fn, 3)) + 1)
            while region(fn, n) * n < a.seconds * 1e3:
                n = int(n * 1.25) + 1
            calls[k] = n
        t = {"old": [], "new": []}
        for _ in range(max(7, a.regions)):
            t["old"].append(region(old, calls["old"]))
            t["new"].append(region(new, calls["new"]))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        gap = (med["old"] - med["new"]) / med["old"]
        row = {"pair": name, "nseq": seq.nseq, "L": seq.L, "old_ms": med["old"], "new_ms": med["new"], "old_spread": spread["old"],
               "new_spread": spread["new"], "speedup": med["old"] / med["new"], "gap": gap, "clears_spread": gap > max(spread.values()),
               "old_tflops": flops / med["old"] * 1e-9, "new_tflops": flops / med["new"] * 1e-9, "regions": len(t["old"]),
               "calls_per_region": calls, "old_regions_ms": t["old"], "new_regions_ms": t["new"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out and rows:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
