#!/usr/bin/env python3
"""Generate the g20_avit_* fixtures by running the REFERENCE's models/avit.py on the CPU (import by path, as make_golden_dpot.py does).

    TANTE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_avit.py       # writes tests/golden/g20_avit_*.npz

Nothing of the reference travels: the fixtures hold tensors, scalars and key lists only.  models/avit.py imports timm.layers.DropPath,
which is not installed: it is stubbed by an identity; einops is installed.

A default-initialised block contributes 2e-6 of its input (the layer scales start at 1e-6), so a default fixture would pass with every
block deleted.  Every gamma* is therefore set to 0.5 (1 + 0.1 randn), every norm weight and bias (q / k norms included) moves by
0.1 randn, the relative-bias embedding is set to randn, and every fixture asserts -- conditions, not measurements -- and stores
  (a) `ratio`   the blocks' contribution, rms(y - y_gammas_zeroed) / rms(y) for models, rms(block(x) - x) / rms(x) per block: >= 0.2
  (b) `err32`   the reference's own fp32 result against the same module in float64 (rel, max / 2): <= 5e-6, half the fp32 bar
The stored `y` is the float64 result rounded to fp32 once.

  g20_avit_spatial_5x7                       AxialAttentionBlock alone, width 48, 3 heads, 5 x 7 tokens, batch 2
  g20_avit_temporal_T4, _T6                  AttentionBlock alone, width 48, 3 heads, 3 x 4 tokens, batch 2
  g20_avit_stem, g20_avit_head               space_bag + embed / debed alone: width 48, 3 of 4 states, 32 x 48 pixels, 3 images
  g20_avit_model_32x48_T4                    embed 48, 3 heads (hd 16), depth 2, 3 fields, batch 2
  g20_avit_model_64x64_T6                    embed 64, 1 head (hd 64), depth 1, 2 of 3 fields, batch 2: x[-4:] cuts
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
    timm, layers = types.ModuleType("timm"), types.ModuleType("timm.layers")

    class DropPath(torch.nn.Identity):
        def __init__(self, drop_prob=0.0, scale_by_keep=True):
            super().__init__()
    layers.DropPath = DropPath
    timm.layers = layers
    sys.modules["timm"], sys.modules["timm.layers"] = timm, layers
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg


_import_reference()
import models.avit as RA  # noqa: E402

RA.device = torch.device("cpu")
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
            if isinstance(m, (RA.RMSInstanceNorm2d, torch.nn.InstanceNorm2d, torch.nn.LayerNorm)):
                for p in m.parameters():
                    p.add_(0.1 * torch.randn_like(p))
            if isinstance(m, RA.RelativePositionBias):
                m.relative_attention_bias.weight.copy_(torch.randn_like(m.relative_attention_bias.weight))
        for k, p in module.named_parameters():
            if k.split(".")[-1].startswith("gamma"):
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


def spatial_fixture(name, seed, C=48, heads=3, H=5, W=7, B=2):
    torch.manual_seed(seed)
    blk = RA.AxialAttentionBlock(C, heads).eval()
    rescale(blk)
    x = torch.randn(B, C, H, W)
    y, err = both(blk, lambda m, dt: m(x.to(dt)))
    ratio = rms(y - x) / rms(x)
    assert ratio >= MIN_RATIO, ratio
    print(f"  {name}: contribution {ratio:.3f}, fp32 vs float64 {err:.2e}")
    save(name, x=x, y=y.float(), heads=np.int64(heads), ratio=np.float64(ratio), err32=np.float64(err), **state(blk))


def temporal_fixture(name, seed, T, C=48, heads=3, H=3, W=4, B=2):
    torch.manual_seed(seed)
    blk = RA.AttentionBlock(C, heads).eval()
    rescale(blk)
    x = torch.randn(T, B, C, H, W)
    y, err = both(blk, lambda m, dt: m(x.to(dt)))
    ratio = rms(y - x) / rms(x)
    assert ratio >= MIN_RATIO, ratio
    print(f"  {name}: contribution {ratio:.3f}, fp32 vs float64 {err:.2e}")
    save(name, x=x, y=y.float(), heads=np.int64(heads), ratio=np.float64(ratio), err32=np.float64(err), **state(blk))


def stem_head_fixtures(seed, E=48, n_states=4, c=3, H=32, W=48, n=3):
    torch.manual_seed(seed)
    m = RA.AViT(4, types.SimpleNamespace(n_fields=n_states), embed_dim=E, num_heads=3, processor_blocks=1).eval()
    rescale(m)
    x = torch.randn(n, c, H, W)

    def stem(mod, dt):
        z = mod.space_bag(x.to(dt).permute(0, 2, 3, 1), range(c))
        return mod.embed(z.permute(0, 3, 1, 2))
    y, err = both(m, stem)
    print(f"  g20_avit_stem: fp32 vs float64 {err:.2e}")
    sd = {k: v for k, v in m.state_dict().items() if k.startswith(("space_bag.", "embed."))}
    save("g20_avit_stem", x=x, y=y.float(), n_states=np.int64(n_states), err32=np.float64(err), keys=np.array(list(sd)), **{"w." + k: v for k, v in sd.items()})
    z = torch.randn(n, E, H // 16, W // 16)
    y, err = both(m, lambda mod, dt: mod.debed(z.to(dt), range(c)))
    print(f"  g20_avit_head: fp32 vs float64 {err:.2e}")
    sd = {k: v for k, v in m.state_dict().items() if k.startswith("debed.")}
    save("g20_avit_head", x=z, y=y.float(), n_states=np.int64(n_states), n_labels=np.int64(c), err32=np.float64(err), keys=np.array(list(sd)),
         **{"w." + k: v for k, v in sd.items()})


def model_fixture(name, seed, E, heads, depth, n_states, c, res, T, B=2):
    torch.manual_seed(seed)
    m = RA.AViT(4, types.SimpleNamespace(n_fields=n_states), out_steps=1, embed_dim=E, num_heads=heads, processor_blocks=depth).eval()
    rescale(m)
    x = torch.randn(B, T, c, *res) * (1.0 + torch.rand(1, 1, c, 1, 1)) + 0.3 * torch.randn(B, 1, c, 1, 1)
    y, err = both(m, lambda mod, dt: mod(x.to(dt)))
    assert tuple(y.shape) == (B, min(T, 4), c, *res), y.shape
    z = copy.deepcopy(m).double()
    with torch.no_grad():
        for k, p in z.named_parameters():
            if k.split(".")[-1].startswith("gamma"):
                p.zero_()
        y0 = z(x.double())
    ratio = rms(y - y0) / rms(y)
    assert ratio >= MIN_RATIO, ratio
    print(f"  {name}: contribution {ratio:.3f}, fp32 vs float64 {err:.2e}")
    save(name, x=x, y=y.float(), embed_dim=np.int64(E), heads=np.int64(heads), depth=np.int64(depth), n_states=np.int64(n_states),
         ratio=np.float64(ratio), err32=np.float64(err), **state(m))


if __name__ == "__main__":
    spatial_fixture("g20_avit_spatial_5x7", 2001)
    temporal_fixture("g20_avit_temporal_T4", 2002, 4)
    temporal_fixture("g20_avit_temporal_T6", 2003, 6)
    stem_head_fixtures(2004)
    model_fixture("g20_avit_model_32x48_T4", 2005, 48, 3, 2, 3, 3, (32, 48), 4)
    model_fixture("g20_avit_model_64x64_T6", 2006, 64, 1, 1, 3, 2, (64, 64), 6)
