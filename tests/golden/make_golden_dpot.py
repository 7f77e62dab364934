#!/usr/bin/env python3
"""Generate the g19_dpot_* fixtures by running the REFERENCE's models/dpot.py on the CPU (import by path, as make_golden_afno.py does).

    TANTE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_dpot.py       # writes tests/golden/g19_dpot_*.npz

Nothing of the reference travels: the fixtures hold tensors, scalars and key lists only.  models/dpot.py imports
data.dataset.TanteMetadata for an annotation only: it is stubbed; einops is installed.

A freshly initialised mixer contributes 3e-4 of its input (weights scale * rand with scale = 1 / bs^2), so a default-init fixture would
pass with the mixer deleted.  Every w1 / w2 is therefore set to randn / sqrt(bs) and every b1 / b2 to 0.3 randn, the norm weights and
biases, pos_embed, the conv biases and gamma are moved off their initial values, and every fixture asserts -- a condition, not a
measurement -- that rms(filter(x) - x) / rms(x) >= 0.2 for every filter it holds, and stores the value.

  g19_dpot_filter_8x8_m3, _8x12_m16, _5x7_m4, _6x9_m2, _4x4_m1   filter alone, channels last (truncation on both axes; modes past the
                                                                  grid; odd axes with bs 12; bs 20; a single mode)
  g19_dpot_filter_cf_6x8_m3                                       filter alone, channel_first=True
  g19_dpot_block_ds0, _ds1                                        one Block, double_skip False / True
  g19_dpot_model_32x48_p4, _16x16_p2                              whole model, embed 64, depth 2, 2 blocks, in_T 3, 2 fields, batch 2
"""
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
    data, dataset = types.ModuleType("data"), types.ModuleType("data.dataset")
    dataset.TanteMetadata = type("TanteMetadata", (), {})
    data.dataset = dataset
    sys.modules["data"], sys.modules["data.dataset"] = data, dataset
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg


_import_reference()
from models.dpot import AFNO2D, DPOT, Block  # noqa: E402

torch.set_num_threads(8)
MIN_RATIO = 0.2


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1000 * 1000, name


def rescale(module):
    """Every mixer under `module`: w = randn / sqrt(bs), b = 0.3 randn; everything else that starts at 0 / 1 / a fixed table moves off it."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, AFNO2D):
                for w in (m.w1, m.w2):
                    w.copy_(torch.randn_like(w) / m.block_size ** 0.5)
                for b in (m.b1, m.b2):
                    b.copy_(0.3 * torch.randn_like(b))
        for k, p in module.named_parameters():
            if ".norm" in "." + k or k.endswith(".bias") and ".filter." not in k:
                p.add_(0.1 * torch.randn_like(p))
            elif k == "pos_embed":
                p.add_(0.2 * torch.randn_like(p))
            elif k.endswith("gamma"):
                p.mul_(1.0 + 0.1 * torch.randn_like(p))


def ratios_of(module, run):
    """rms(filter(x) - x) / rms(x) of every AFNO2D under `module` during run(), read off forward hooks."""
    got = []

    def hook(m, i, o):
        got.append(float(torch.sqrt(((o - i[0]) ** 2).mean()) / torch.sqrt((i[0] ** 2).mean())))
    hooks = [m.register_forward_hook(hook) for m in module.modules() if isinstance(m, AFNO2D)]
    with torch.no_grad():
        y = run()
    for h in hooks:
        h.remove()
    assert got and all(r >= MIN_RATIO for r in got), got
    return y, got


def filter_fixture(name, H, W, C, nb, modes, B, seed, channel_first=False):
    torch.manual_seed(seed)
    f = AFNO2D(width=C, num_blocks=nb, channel_first=channel_first, modes=modes).eval()
    rescale(f)
    x = torch.randn(B, C, H, W) if channel_first else torch.randn(B, H, W, C)
    y, r = ratios_of(f, lambda: f(x))
    assert y.shape == x.shape
    print(f"  {name}: contribution {r[0]:.3f}")
    save(name, x=x, y=y, w1=f.w1, b1=f.b1, w2=f.w2, b2=f.b2, modes=np.int64(modes), ratio=np.float64(r[0]))


def block_fixture(name, double_skip, seed, H=6, W=10, C=64, nb=2, modes=4, B=2):
    torch.manual_seed(seed)
    blk = Block(width=C, n_blocks=nb, mlp_ratio=2.0, channel_first=True, modes=modes, double_skip=double_skip).eval()
    rescale(blk)
    x = torch.randn(B, C, H, W)
    y, r = ratios_of(blk, lambda: blk(x))
    print(f"  {name}: contribution {r[0]:.3f}")
    sd = blk.state_dict()
    save(name, x=x, y=y, keys=np.array(list(sd.keys())), modes=np.int64(modes), double_skip=np.int64(double_skip), ratio=np.float64(r[0]),
         **{"w." + k: v for k, v in sd.items()})


def model_fixture(name, res, patch, modes, time_agg, out_timesteps, seed):
    torch.manual_seed(seed)
    md = types.SimpleNamespace(n_fields=2, spatial_resolution=res, n_spatial_dims=2)
    m = DPOT(in_T=3, dset_metadata=md, patch_size=patch, out_timesteps=out_timesteps, n_blocks=2, embed_dim=64, out_layer_dim=16, depth=2,
             modes=modes, mlp_ratio=2.0, n_cls=4, time_agg=time_agg).eval()
    rescale(m)
    x = torch.randn(2, 3, 2, *res)
    y, r = ratios_of(m, lambda: m(x))
    assert tuple(y.shape) == (2, out_timesteps, 2, *res), y.shape
    print(f"  {name}: contributions {['%.3f' % v for v in r]}")
    sd = m.state_dict()
    save(name, x=x, y=y, keys=np.array(list(sd.keys())), ratio=np.array(r), patch=np.int64(patch), modes=np.int64(modes),
         out_timesteps=np.int64(out_timesteps), exp_mlp=np.int64(time_agg == "exp_mlp"), **{"w." + k: v for k, v in sd.items()})


if __name__ == "__main__":
    filter_fixture("g19_dpot_filter_8x8_m3", 8, 8, 64, 2, 3, 2, 1901)
    filter_fixture("g19_dpot_filter_8x12_m16", 8, 12, 64, 2, 16, 2, 1902)
    filter_fixture("g19_dpot_filter_5x7_m4", 5, 7, 48, 4, 4, 2, 1903)
    filter_fixture("g19_dpot_filter_6x9_m2", 6, 9, 40, 2, 2, 1, 1904)
    filter_fixture("g19_dpot_filter_4x4_m1", 4, 4, 64, 2, 1, 1, 1905)
    filter_fixture("g19_dpot_filter_cf_6x8_m3", 6, 8, 32, 2, 3, 2, 1906, channel_first=True)
    block_fixture("g19_dpot_block_ds0", False, 1907)
    block_fixture("g19_dpot_block_ds1", True, 1908)
    model_fixture("g19_dpot_model_32x48_p4", (32, 48), 4, 3, "exp_mlp", 1, 1909)
    model_fixture("g19_dpot_model_16x16_p2", (16, 16), 2, 16, "mlp", 2, 1910)
