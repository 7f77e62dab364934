#!/usr/bin/env python3
"""Generate the g21_convnext_* fixtures by running the REFERENCE's models/unet_convnext.py on the CPU (import by path, as
make_golden_avit.py does).

    TANTE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_convnext.py   # writes tests/golden/g21_convnext_*.npz

Nothing of the reference travels: the fixtures hold tensors, scalars and key lists only.  models/unet_convnext.py imports
timm.models.layers.DropPath, which is not installed: it is stubbed by an identity; einops is installed.

A default-initialised block contributes 1e-6 of its input (the layer scale starts at 1e-6), so a default fixture would pass with every
block deleted.  Every gamma is therefore set to 0.5 (1 + 0.1 randn), every norm weight and bias moves by 0.1 randn, and every fixture
asserts -- conditions, not measurements -- and stores
  (a) `ratio`   the blocks' contribution, rms(y - y_gammas_zeroed) / rms(y) for models, rms(block(x) - x) / rms(x) per block: >= 0.2
  (b) `err32`   the reference's own fp32 result against the same module in float64 (rel, max / 2): <= 5e-6, half the fp32 bar
The stored `y` is the float64 result rounded to fp32 once; `y64` is the float64 result itself, which the restatement is pinned to.

  g21_convnext_block_c15_5x7, _block_c32_9x20      Block alone, batch 2
  g21_convnext_down_c15, _up_c30                   Downsample 15 -> 30 / Upsample 30 -> 15 alone on 6 x 10, batch 2
  g21_convnext_stage_skip_c30                      a decoder Stage with skip_project (30 -> 15, one block) on 6 x 10; x is cat([x, skip])
  g21_convnext_model_f15_s2_20x28                  init_features 15, stages 2, blocks_per_stage 2, 3 fields, T 4, batch 2: neck 5 x 7
  g21_convnext_model_f8_s3_16x24                   init_features 8, stages 3, blocks_per_stage 1, blocks_at_neck 2, 2 fields: neck 2 x 3
"""
import copy
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("TANTE_REFERENCE", "")
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"reference not found at {REF!r}: set TANTE_REFERENCE to a checkout of it (the fixtures can only be generated beside one)")
    timm, tm, layers = types.ModuleType("timm"), types.ModuleType("timm.models"), types.ModuleType("timm.models.layers")

    class DropPath(torch.nn.Identity):
        def __init__(self, drop_prob=0.0, scale_by_keep=True):
            super().__init__()
    layers.DropPath = DropPath
    tm.layers = layers
    timm.models = tm
    sys.modules["timm"], sys.modules["timm.models"], sys.modules["timm.models.layers"] = timm, tm, layers
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg


_import_reference()
import models.unet_convnext as RC  # noqa: E402

torch.set_num_threads(8)
MIN_RATIO = 0.2
MAX_ERR32 = 5e-6


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1000 * 1000, name


def rescale(module):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, RC.LayerNorm):
                for p in m.parameters():
                    p.add_(0.1 * torch.randn_like(p))
        for k, p in module.named_parameters():
            if k.split(".")[-1] == "gamma":
                p.copy_(0.5 * (1.0 + 0.1 * torch.randn_like(p)))


def rms(t):
    return float(torch.sqrt((t.double() ** 2).mean()))


def both(module, run):
    """-> (float64 result, err32): run(module) in fp32 and run(module.double()) on the float64 inputs."""
    with torch.no_grad():
        y32 = run(module, torch.float32)
        y64 = run(copy.deepcopy(module).double(), torch.float64)
    rel = float((y32.double() - y64).norm() / y64.norm())
    mx = float((y32.double() - y64).abs().max() / y64.abs().max())
    err = max(rel, mx / 2)
    assert err <= MAX_ERR32, (rel, mx)
    return y64, err


def state(module):
    sd = module.state_dict()
    return dict(keys=np.array(list(sd.keys())), **{"w." + k: v for k, v in sd.items()})


def block_fixture(name, seed, C, H, W, B=2):
    torch.manual_seed(seed)
    blk = RC.Block(C, 2).eval()
    rescale(blk)
    x = 0.4 * torch.randn(B, C, H, W)          # the block's output does not scale with x (LayerNorm): at unit rms its share is 0.11
    y, err = both(blk, lambda m, dt: m(x.to(dt)))
    ratio = rms(y - x) / rms(x)
    assert ratio >= MIN_RATIO, ratio
    print(f"  {name}: contribution {ratio:.3f}, fp32 vs float64 {err:.2e}")
    save(name, x=x, y=y.float(), y64=y, ratio=np.float64(ratio), err32=np.float64(err), **state(blk))


def module_fixture(name, seed, make, cin, H=6, W=10, B=2):
    torch.manual_seed(seed)
    mod = make().eval()
    rescale(mod)
    x = torch.randn(B, cin, H, W) * (1.0 + torch.rand(1, cin, 1, 1))
    y, err = both(mod, lambda m, dt: m(x.to(dt)))
    print(f"  {name}: fp32 vs float64 {err:.2e}")
    save(name, x=x, y=y.float(), y64=y, err32=np.float64(err), **state(mod))


def model_fixture(name, seed, features, stages, bps, neck, n_fields, res, T=4, B=2):
    torch.manual_seed(seed)
    md = types.SimpleNamespace(n_fields=n_fields, n_spatial_dims=2)
    m = RC.UNetConvNext(T, md, stages=stages, blocks_per_stage=bps, blocks_at_neck=neck, init_features=features).eval()
    rescale(m)
    x = torch.randn(B, T, n_fields, *res) * (1.0 + torch.rand(1, 1, n_fields, 1, 1)) + 0.3 * torch.randn(B, 1, n_fields, 1, 1)
    y, err = both(m, lambda mod, dt: mod(x.to(dt)))
    assert tuple(y.shape) == (B, 1, n_fields, *res), y.shape
    z = copy.deepcopy(m).double()
    with torch.no_grad():
        for k, p in z.named_parameters():
            if k.split(".")[-1] == "gamma":
                p.zero_()
        y0 = z(x.double())
    ratio = rms(y - y0) / rms(y)
    assert ratio >= MIN_RATIO, ratio
    print(f"  {name}: contribution {ratio:.3f}, fp32 vs float64 {err:.2e}, {len(m.state_dict())} keys")
    save(name, x=x, y=y.float(), y64=y, init_features=np.int64(features), stages=np.int64(stages), blocks_per_stage=np.int64(bps),
         blocks_at_neck=np.int64(neck), n_fields=np.int64(n_fields), in_T=np.int64(T), ratio=np.float64(ratio), err32=np.float64(err), **state(m))


if __name__ == "__main__":
    block_fixture("g21_convnext_block_c15_5x7", 2101, 15, 5, 7)
    block_fixture("g21_convnext_block_c32_9x20", 2102, 32, 9, 20)
    module_fixture("g21_convnext_down_c15", 2103, lambda: RC.Downsample(15, 30, 2), 15)
    module_fixture("g21_convnext_up_c30", 2104, lambda: RC.Upsample(30, 15, 2), 30)
    module_fixture("g21_convnext_stage_skip_c30", 2105, lambda: RC.Stage(30, 15, 2, depth=1, mode="up", skip_project=True), 60)
    model_fixture("g21_convnext_model_f15_s2_20x28", 2106, 15, 2, 2, 1, 3, (20, 28))
    model_fixture("g21_convnext_model_f8_s3_16x24", 2107, 8, 3, 1, 2, 2, (16, 24))
