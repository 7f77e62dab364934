"""axis_hw_exact_kernel: the column-block schedule against the one-block schedule (TANTE_AXIS_BLOCKS=0), one process, interleaved rounds:
    python tools/axis_blocks_time.py      (cfg2 plane: 32 planes x 32 x 32 tokens x 256 channels, in place and out of place)"""
import os, sys, statistics, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tante_amd
from tante_amd import _lib as L, kernels as K
dev = torch.device("cuda:0")
torch.manual_seed(0)
BT, H, W, C = 32, 32, 32, 256
x0 = torch.randn(BT, H, W, C, device=dev)
wh = [torch.randn(H, H, device=dev) / 6, torch.randn(H, device=dev) * 0.1, torch.randn(H, H, device=dev) / 6, torch.randn(H, device=dev) * 0.1]
ww = [torch.randn(W, W, device=dev) / 6, torch.randn(W, device=dev) * 0.1, torch.randn(W, W, device=dev) / 6, torch.randn(W, device=dev) * 0.1]
ts = {}
ref = None
for r in range(9):
    for blocks in (0, -1):
        L.set_option("TANTE_AXIS_BLOCKS", blocks)
        for oop in (False, True):
            x, y = x0.clone(), torch.empty_like(x0)
            run = (lambda: K.axis_hw_oop(x, y, BT, H, W, C, wh, ww, L.BF16)) if oop else (lambda: K.axis_hw(x, BT, H, W, C, wh, ww, L.BF16))
            run()
            if r == 0 and not oop:
                if ref is None:
                    ref = x.clone()
                else:
                    print("column blocks == one block:", torch.equal(x, ref))
            for _ in range(3):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                run()
            e1.record(); torch.cuda.synchronize()
            ts.setdefault((blocks, oop), []).append(e0.elapsed_time(e1) * 1e3 / 30)
L.set_option("TANTE_AXIS_BLOCKS", -1)
for (blocks, oop), v in sorted(ts.items(), reverse=True):
    print(f"{'one block    ' if blocks == 0 else 'column blocks'} {'out of place' if oop else 'in place    '}: median {statistics.median(v):.2f} us  min {min(v):.2f}  max {max(v):.2f}")
