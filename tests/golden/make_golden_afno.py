#!/usr/bin/env python3
"""Generate the g18_afno_* fixtures by running the REFERENCE's models/afno.py on the CPU (import by path, as make_golden.py does).

    python tests/golden/make_golden_afno.py       # writes tests/golden/g18_afno_*.npz

Nothing of the reference travels: the fixtures hold tensors, scalars and key lists only.  `timm` is not installed and touches no
arithmetic at drop rate 0: it is stubbed with an identity DropPath and torch's own trunc_normal_.

A freshly initialised filter is identically ZERO on unit-variance input (complex weights of scale 0.02 against a soft threshold of
0.01: every real and imaginary part falls under it), so a default-init fixture would pass with the filter deleted.  Every cmlp weight
is therefore multiplied by 2 after construction, and every filter fixture asserts -- a condition, not a measurement -- that the
soft-thresholded share of its spectrum lies in [0.2, 0.8], and stores it.  LayerNorm weights / biases, pos_embed and the fc biases are
moved away from 1 / 0 so that a dropped affine, bias or positional term shows.

  g18_afno_filter_8x8, _24x8, _4x16, _5x12   filter alone, C 64 = 2 blocks of 32, batch 2 (H' > W', H' < W': crop and pad; an odd axis)
  g18_afno_filter_16x16_c256                 filter alone, C 256 = 8 blocks of 32, one sample: the shipped channel geometry
  g18_afno_model_32x32_p4, _16x48_p2         whole model, hidden 64, 2 blocks, in_T 3, 2 fields, batch 2
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("TANTE_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"reference not found at {REF}; fixtures can only be generated in the build container")

    class DropPath(torch.nn.Module):
        def __init__(self, drop_prob=0.0):
            super().__init__()

        def forward(self, x):
            return x

    for name in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["timm"].models = sys.modules["timm.models"]
    sys.modules["timm.models"].layers = sys.modules["timm.models.layers"]
    sys.modules["timm.models.layers"].DropPath = DropPath
    sys.modules["timm.models.layers"].trunc_normal_ = torch.nn.init.trunc_normal_
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg


_import_reference()
from models.afno import AFNO, AFNO_ND  # noqa: E402

torch.set_num_threads(8)
SCALE = 2.0


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1024 * 1024, name


def zeroed_share_of(filt, x):
    """Share of the real / imaginary parts the soft threshold zeroes, read off the filter's own cmlp output."""
    got = []
    h = filt.cmlp.register_forward_hook(lambda m, i, o: got.append(torch.view_as_real(o).detach()))
    with torch.no_grad():
        y = filt(x)
    h.remove()
    return y, float((got[0].abs() <= filt.sparsity_threshold).float().mean())


def filter_fixture(name, H, W, C, nblk, batch, seed):
    torch.manual_seed(seed)
    f = AFNO_ND(C, [H, W], cmlp_diagonal_blocks=nblk, sparsity_threshold=0.01).eval()
    with torch.no_grad():
        for i in (0, 2):
            f.cmlp[i].weight.mul_(SCALE)
    x = torch.randn(batch, H, W, C)
    y, share = zeroed_share_of(f, x)
    assert tuple(y.shape) == (batch, W, H, C), y.shape
    assert 0.2 <= share <= 0.8, (name, share)
    print(f"  {name}: zeroed share {share:.3f}, |y| max {float(y.abs().max()):.3f}")
    save(name, x=x, y=y, w1=f.cmlp[0].weight, w2=f.cmlp[2].weight, lam=np.float64(f.sparsity_threshold), zeroed_share=np.float64(share))


def model_fixture(name, res, patch, seed):
    torch.manual_seed(seed)
    md = types.SimpleNamespace(n_fields=2, spatial_resolution=res, n_spatial_dims=2)
    m = AFNO(in_T=3, dset_metadata=md, hidden_dim=64, n_blocks=2, cmlp_diagonal_blocks=2, patch_size=patch).eval()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".cmlp." in k:
                p.mul_(SCALE)
            elif "norm" in k or k.endswith("fc1.bias") or k.endswith("fc2.bias"):
                p.add_(0.1 * torch.randn_like(p))
            elif k == "pos_embed":
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(2, 3, 2, *res)
    shares = []
    hooks = [b.filter.cmlp.register_forward_hook(lambda mod, i, o: shares.append(float((torch.view_as_real(o).abs() <= 0.01).float().mean())))
             for b in m.blocks]
    with torch.no_grad():
        y = m(x)
    for h in hooks:
        h.remove()
    assert tuple(y.shape) == (2, 1, 2, *res)
    assert all(0.2 <= s <= 0.8 for s in shares), (name, shares)
    print(f"  {name}: zeroed shares {['%.3f' % s for s in shares]}")
    sd = m.state_dict()
    save(name, x=x, y=y, keys=np.array(list(sd.keys())), zeroed_share=np.array(shares), patch=np.int64(patch),
         **{"w." + k: v for k, v in sd.items()})


if __name__ == "__main__":
    filter_fixture("g18_afno_filter_8x8", 8, 8, 64, 2, 2, 1801)
    filter_fixture("g18_afno_filter_24x8", 24, 8, 64, 2, 2, 1802)
    filter_fixture("g18_afno_filter_4x16", 4, 16, 64, 2, 2, 1803)
    filter_fixture("g18_afno_filter_5x12", 5, 12, 64, 2, 2, 1804)
    filter_fixture("g18_afno_filter_16x16_c256", 16, 16, 256, 8, 1, 1805)
    model_fixture("g18_afno_model_32x32_p4", (32, 32), 4, 1806)
    model_fixture("g18_afno_model_16x48_p2", (16, 48), 2, 1807)
