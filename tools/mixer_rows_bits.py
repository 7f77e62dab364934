#!/usr/bin/env python3
"""Do two builds of the library give the same bits from the AFNO filter, its backward and the DPOT mixer?  (profiles/mixer_rows_identity.md)

    TANTE_LIB=<build A> python tools/mixer_rows_bits.py dump DIR_A      # each dump in a process of its own
    python tools/mixer_rows_bits.py dump DIR_B
    python tools/mixer_rows_bits.py compare DIR_A DIR_B

dump: tante_afno_filter with and without a residual, tante_afno_filter_bwd (dx, dw1, dw2) and tante_dpot_filter with and without a residual
on seeded inputs, at the shapes of the filter tests and at the token grid and width of configs/afno_am.yaml / configs/dpot_am.yaml, one
.npy per output.  compare: the two dumps as int32 bit patterns, so that the sign of zero counts; exit status 1 if any file differs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AFNO = [(2, 7, 9, 40, 8), (1, 12, 5, 48, 24), (1, 5, 12, 48, 24), (1, 64, 33, 48, 24), (1, 33, 64, 128, 64), (3, 1, 1, 16, 16), (1, 5, 12, 80, 16),
        (1, 12, 5, 80, 16), (4, 32, 32, 256, 32)]                          # (B, H, W, C, bs); the last one is afno_am
DPOT = [(1, 8, 8, 768, 2, 16), (1, 64, 33, 48, 2, 20), (1, 33, 64, 128, 2, 64), (3, 1, 1, 16, 1, 5), (2, 7, 9, 40, 5, 2), (1, 5, 12, 80, 5, 4),
        (1, 12, 5, 80, 5, 4), (4, 8, 8, 1536, 4, 16)]                      # (B, H, W, C, blocks, modes); the last one is dpot_am


def dump(out):
    import torch
    import tante_amd.afno as A
    import tante_amd.dpot as D
    dev = torch.device("cuda:0")
    os.makedirs(out, exist_ok=True)

    def save(name, t):
        np.save(os.path.join(out, name + ".npy"), t.detach().cpu().numpy())

    for B, H, W, C, bs in AFNO:
        gen = torch.Generator().manual_seed(H * 100 + W)
        s = 0.04 * (32.0 / bs) ** 0.5 * (3.0 if H * W == 1 else 1.0)
        w1, w2 = (s * torch.randn(C // bs, bs, bs, 2, generator=gen)).to(dev), (s * torch.randn(C // bs, bs, bs, 2, generator=gen)).to(dev)
        x, res, dout = (torch.randn(B, H, W, C, generator=gen).to(dev) for _ in range(3))
        tag = f"afno_{B}_{H}x{W}_{C}_{bs}"
        for r in (None, res):
            save(f"{tag}_{'res' if r is not None else 'plain'}", A.afno_filter(x, r, A.pack_block_weight(w1), A.pack_block_weight(w2), bs, 0.01))
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, w2)]
        A.AfnoFilterFn.apply(leaves[0], res, leaves[1], leaves[2], bs, 0.01).backward(dout)
        for n, t in zip(("dx", "dw1", "dw2"), leaves):
            save(f"{tag}_{n}", t.grad)
    for B, H, W, C, nb, modes in DPOT:
        gen = torch.Generator().manual_seed(H * 1000 + W * 10 + nb)
        bs = C // nb
        w1, w2 = (torch.randn(2, nb, bs, bs, generator=gen) / bs ** 0.5).to(dev), (torch.randn(2, nb, bs, bs, generator=gen) / bs ** 0.5).to(dev)
        b1, b2 = (0.3 * torch.randn(2, nb, bs, generator=gen)).to(dev), (0.3 * torch.randn(2, nb, bs, generator=gen)).to(dev)
        x, res = torch.randn(B, H, W, C, generator=gen).to(dev), torch.randn(B, H, W, C, generator=gen).to(dev)
        for r in (None, res):
            save(f"dpot_{B}_{H}x{W}_{C}_{nb}_{modes}_{'res' if r is not None else 'plain'}", D.dpot_filter(x, r, w1, b1, w2, b2, modes))
    torch.cuda.synchronize()
    print(f"{len(os.listdir(out))} outputs in {out}")


def compare(a, b):
    names = sorted(os.listdir(a))
    bad = sorted(set(names) ^ set(os.listdir(b)))
    for n in names:
        if n in bad:
            continue
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        same = x.shape == y.shape and x.dtype == y.dtype == np.float32 and np.array_equal(x.view(np.int32), y.view(np.int32))
        finite = bool(np.isfinite(x).all()) and float(np.abs(x).max()) > 0.0
        print(f"| {n[:-4]} | {x.size} | {'equal' if same else 'DIFFERENT'} |" + ("" if finite else " not finite or all zero"))
        if not (same and finite):
            bad.append(n)
    print(f"{len(names) - len(bad)} of {len(names)} outputs bit-equal")
    sys.exit(1 if bad or not names else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
