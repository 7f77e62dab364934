#!/usr/bin/env python3
"""Generate the g23_uno_* fixtures by running the REFERENCE's models/uno.py on the CPU (import by path, as make_golden_unet_att.py does).

    TANTE_REFERENCE=<checkout of the reference> python tests/golden/make_golden_uno.py   # writes tests/golden/g23_uno_*.npz

Nothing of the reference travels: the fixtures hold tensors, scalars and key lists only.  models/uno.py imports torch, numpy and einops,
all installed, and matplotlib, which it never uses: where that is missing an empty stand-in module is registered for the import.

The reference cannot run in float64 (its out_ft is hard-coded cfloat), so the stored truth `y64` is tests/uno_ref.py's float64
restatement and the fixture pins it to the reference's own fp32 output.  Every fixture asserts -- conditions, not measurements -- and
stores
  `err32`        the reference's fp32 output against the restatement, max(rel L2, max / 2): <= 5e-6, half the fp32 bar
  `path_share`   per block, rms(spectral) / rms(sum) and rms(pointwise) / rms(sum): each >= 0.2        (blocks and models)
  `block_reach`  per block, rms(y - y_without_the_block's_spectral_path) / rms(y): >= 0.05             (models)
At the default initialisation the spectral path of L0 / L1 / L2 is 0.1 / 0.03 / 0.015 of the pointwise one, so a wrong spectral path
would pass: the fixtures scale weights1 / weights2 per block by a power of two (exact in fp32), chosen here block by block so that the two
paths have about the same rms (in the models the spectral one about twice the pointwise one), and store the `scales`.

The component fixtures store their weights and inputs.  The models cannot (a width-4 model has 1.6 M spectral parameters): their state
dict and their input come from tests/uno_ref.rule_state_dict / rule_input, which the tests apply identically; the fixture stores y64, the
key list with shapes, the constructor arguments and the scales.

  g23_uno_spec_*     SpectralConv2d_Uno alone, batch 2: (Ci, Co, Hi x Wi -> Ho x Wo, m1, m2) =
                     (3, 5, 12 x 10 -> 6 x 8, 2, 3); (3, 5, 12 x 10 -> 6 x 8, 3, 5) Nyquist column populated;
                     (4, 2, 6 x 8 -> 13 x 21, 3, 5) odd output, upsampling; (2, 3, 16 x 16 -> 6 x 16, 4, 5) bands overlap;
                     (3, 3, 8 x 8 -> 8 x 8, 4, 5) same grid, every row kept
  g23_uno_block_*    OperatorBlock_2D, batch 2: 6 -> 7 channels 20 x 24 -> 9 x 11 (down), 5 -> 3 channels 7 x 10 -> 18 x 23 (up)
  g23_uno_model_*    in_T 2: width 4 factor 1 on 128 x 256 (the smallest size the reference runs); width 4 factor 2 pad 4 on 120 x 248;
                     width 4 on 136 x 264 (floor divisions, overlapping bands in L0); width 6, one field, on 256 x 256
"""
import math
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("TANTE_REFERENCE", "")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import uno_ref as R  # noqa: E402


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit(f"reference not found at {REF!r}: set TANTE_REFERENCE to a checkout of it (the fixtures can only be generated beside one)")
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot


_import_reference()
import models.uno as RU  # noqa: E402

torch.set_num_threads(8)
MAX_ERR32, MIN_SHARE, MIN_REACH = 5e-6, 0.2, 0.05
BOOST = 2.0      # the models aim the spectral path at twice the pointwise one: at equal rms the inner blocks reach the output by 0.03 only


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1000 * 1000, name


def shapes_of(sd):
    return np.array([",".join(str(s) for s in v.shape) for v in sd.values()])


def state(module):
    sd = module.state_dict()
    return dict(keys=np.array(list(sd.keys())), shapes=shapes_of(sd), **{"w." + k: v for k, v in sd.items()})


def checked_err(y32, y64):
    e = R.err(y32, y64)
    assert 0 < e <= MAX_ERR32, e
    return e


def shares(parts):
    out = []
    for s, w in parts:
        tot = R.rms(s + w)
        out.append((R.rms(s) / tot, R.rms(w) / tot))
    return out


def spec_fixture(name, seed, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, B=2):
    torch.manual_seed(seed)
    mod = RU.SpectralConv2d_Uno(Ci, Co, Ho, Wo, m1, m2).eval()
    x = torch.randn(B, Ci, Hi, Wi) + 0.3
    with torch.no_grad():
        y32 = mod(x)
    sd = mod.state_dict()
    y64 = R.spectral_table(x.double(), sd["weights1"], sd["weights2"], Ho, Wo)
    e = checked_err(y32, y64)
    print(f"  {name}: reference fp32 vs restatement {e:.2e}")
    save(name, x=x, y64=y64, y32=y32, err32=np.float64(e), dims=np.array([Ho, Wo, m1, m2]), **state(mod))


def block_fixture(name, seed, Ci, Co, Hi, Wi, Ho, Wo, m1, m2, B=2):
    torch.manual_seed(seed)
    mod = RU.OperatorBlock_2D(Ci, Co, Ho, Wo, m1, m2).eval()
    x = torch.randn(B, Ci, Hi, Wi) + 0.3
    parts = []
    R.block(x, mod.state_dict(), "", Ho, Wo, parts)
    scale = 2.0 ** round(math.log2(R.rms(parts[0][1]) / R.rms(parts[0][0])))
    with torch.no_grad():
        mod.conv.weights1.mul_(scale), mod.conv.weights2.mul_(scale)
        y32 = mod(x)
    parts = []
    y64 = R.block(x, mod.state_dict(), "", Ho, Wo, parts)
    e = checked_err(y32, y64)
    sh = shares(parts)
    assert min(sh[0]) >= MIN_SHARE, sh
    print(f"  {name}: reference fp32 vs restatement {e:.2e}, scale {scale}, shares {sh[0][0]:.2f} / {sh[0][1]:.2f}")
    save(name, x=x, y64=y64, y32=y32, err32=np.float64(e), dims=np.array([Ho, Wo, m1, m2]), scales=np.array([scale]), path_share=np.array(sh), **state(mod))


def model_fixture(name, width, factor, pad, n_fields, res, in_T=2, B=1):
    md = types.SimpleNamespace(n_fields=n_fields, n_spatial_dims=2)
    m = RU.UNO(in_T, md, width=width, pad=pad, factor=factor).eval()
    sd0 = m.state_dict()
    keys, shapes = list(sd0.keys()), [tuple(v.shape) for v in sd0.values()]
    x = R.rule_input(name, (B, in_T, n_fields, *res))
    scales = [1.0] * 7
    for i in range(7):                       # block by block: the later blocks see the earlier ones' scaled output
        parts = []
        R.model(x, R.rule_state_dict(keys, shapes, scales), pad, parts)
        scales[i] = 2.0 ** round(math.log2(BOOST * R.rms(parts[i][1]) / R.rms(parts[i][0])))
    sd = R.rule_state_dict(keys, shapes, scales)
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y32 = m(x)
    parts = []
    y64 = R.model(x, sd, pad, parts)
    assert tuple(y64.shape) == (B, 1, n_fields, *res) == tuple(y32.shape)
    e = checked_err(y32, y64)
    sh = shares(parts)
    assert min(min(s) for s in sh) >= MIN_SHARE, sh
    reach = [R.rms(y64 - R.model(x, sd, pad, zero_block=i)) / R.rms(y64) for i in range(7)]
    assert min(reach) >= MIN_REACH, reach
    print(f"  {name}: reference fp32 vs restatement {e:.2e}, scales {scales}, shares {[f'{a:.2f}/{b:.2f}' for a, b in sh]}, "
          f"reach {[f'{r:.2f}' for r in reach]}, {len(keys)} keys, {sum(int(np.prod(s)) for s in shapes)} values")
    save(name, y64=y64, keys=np.array(keys), shapes=shapes_of(sd0), width=np.int64(width), factor=np.int64(factor), pad=np.int64(pad),
         n_fields=np.int64(n_fields), in_T=np.int64(in_T), x_shape=np.array([B, in_T, n_fields, *res]), err32=np.float64(e), scales=np.array(scales),
         path_share=np.array(sh), block_reach=np.array(reach))


if __name__ == "__main__":
    spec_fixture("g23_uno_spec_3_5_12x10_6x8_m2x3", 2301, 3, 5, 12, 10, 6, 8, 2, 3)
    spec_fixture("g23_uno_spec_3_5_12x10_6x8_m3x5", 2302, 3, 5, 12, 10, 6, 8, 3, 5)
    spec_fixture("g23_uno_spec_4_2_6x8_13x21_m3x5", 2303, 4, 2, 6, 8, 13, 21, 3, 5)
    spec_fixture("g23_uno_spec_2_3_16x16_6x16_m4x5", 2304, 2, 3, 16, 16, 6, 16, 4, 5)
    spec_fixture("g23_uno_spec_3_3_8x8_8x8_m4x5", 2305, 3, 3, 8, 8, 8, 8, 4, 5)
    block_fixture("g23_uno_block_6_7_20x24_9x11_m3x4", 2306, 6, 7, 20, 24, 9, 11, 3, 4)
    block_fixture("g23_uno_block_5_3_7x10_18x23_m3x5", 2307, 5, 3, 7, 10, 18, 23, 3, 5)
    model_fixture("g23_uno_model_w4_f1_128x256", 4, 1, 0, 1, (128, 256), B=2)
    model_fixture("g23_uno_model_w4_f2_p4_120x248", 4, 2, 4, 2, (120, 248))
    model_fixture("g23_uno_model_w4_f1_136x264", 4, 1, 0, 2, (136, 264))
    model_fixture("g23_uno_model_w6_f1_256x256", 6, 1, 0, 1, (256, 256))
