"""Host side of the packed twiddle buffers that the AFNO filter and the DPOT mixer read (csrc/dft_rows.hip.h): the float64 roots of
unity, the padded real / imaginary planes, and the once-per-shape device copy checked against the library's own float count."""
from __future__ import annotations

from typing import Callable, Sequence

import numpy as np
import torch


def cis(num: np.ndarray, n: int, sign: int) -> np.ndarray:
    """e^{sign 2 pi i num / n} in float64 with the angle reduced in integers (so the entries that are real / imaginary are exactly so)."""
    m = np.mod(num, n).astype(np.float64)
    z = np.cos(2.0 * np.pi * m / n) + sign * 1j * np.sin(2.0 * np.pi * m / n)
    z.real[np.abs(z.real) < 1e-15] = 0.0
    z.imag[np.abs(z.imag) < 1e-15] = 0.0
    return z


def pack_tables(tables: Sequence[np.ndarray]) -> np.ndarray:
    """complex128 tables -> the float32 buffer the kernels read: per table a real then an imaginary plane, rows padded to 16, columns
    to 4, rounded once."""
    planes = []
    for t in tables:
        p = np.zeros((2, -(-t.shape[0] // 16) * 16, -(-t.shape[1] // 4) * 4), dtype=np.float32)
        p[0, :t.shape[0], :t.shape[1]] = t.real
        p[1, :t.shape[0], :t.shape[1]] = t.imag
        planes.append(p.reshape(-1))
    return np.concatenate(planes)


_DEVICE_TABLES = {}     # cache_key + (device,) -> packed tables on the device: weight independent, built once per shape


def device_tables(cache_key: tuple, build: Callable[[], np.ndarray], expected_floats: int, what: str, device) -> torch.Tensor:
    """build()'s buffer on `device`, built once per cache_key; `expected_floats` is the library's count for the same shape."""
    key = cache_key + (str(device),)
    t = _DEVICE_TABLES.get(key)
    if t is None:
        host = build()
        if int(expected_floats) != host.size:
            raise RuntimeError(f"{what}: {host.size} floats packed, the library expects {int(expected_floats)}")
        t = _DEVICE_TABLES[key] = torch.from_numpy(host).to(device)
    return t
