"""numpy reference of the occupancy-grid convention, written from the convention, not from the kernels:

* a density grid of (nx, ny, nz) points over [lo, hi] (ops.grid_points: x = lo + idx * step, each operation rounded to fp32) has
  (nx-1, ny-1, nz-1) cells, cell (i, j, k) named by its lowest corner;
* a cell is occupied iff the largest of its 8 corner densities is above the threshold; a NaN corner counts as occupied;
* the result is dilated by `dilate` cells (Chebyshev max filter);
* bits in C order (k fastest), bit c & 31 of uint32 word c >> 5;
* sample x lies in cell floor((x_a - lo_a) / step_a) per axis in fp32 (IEEE division), clamped to cells_a - 1; outside
  [lo_a, lo_a + cells_a * step_a] (multiply then add, fp32) or NaN: empty.
"""
from __future__ import annotations

import numpy as np


def cell_occupancy(density, threshold: float, dilate: int) -> np.ndarray:
    d = np.asarray(density, dtype=np.float32)
    hot = ~(d <= np.float32(threshold))            # above the threshold, or NaN
    occ = np.zeros(tuple(n - 1 for n in d.shape), dtype=bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                occ |= hot[di: di + occ.shape[0], dj: dj + occ.shape[1], dk: dk + occ.shape[2]]
    if dilate > 0:
        r = int(dilate)
        pad = np.pad(occ, r, constant_values=False)
        out = np.zeros_like(occ)
        for a in range(-r, r + 1):
            for b in range(-r, r + 1):
                for c in range(-r, r + 1):
                    out |= pad[r + a: r + a + occ.shape[0], r + b: r + b + occ.shape[1], r + c: r + c + occ.shape[2]]
        occ = out
    return occ


def pack_bits(occ: np.ndarray) -> np.ndarray:
    flat = occ.reshape(-1).astype(np.uint64)
    n = flat.size
    words = np.zeros((n + 31) // 32, dtype=np.uint64)
    idx = np.arange(n)
    np.add.at(words, idx >> 5, flat << (idx & 31).astype(np.uint64))
    return words.astype(np.uint32)


def grid_step(dims, lo, hi):
    """ops.grid_step in numpy: fp32 lo and step = (hi - lo) / (n - 1)."""
    lo32 = np.asarray(np.broadcast_to(lo, 3), dtype=np.float32)
    hi32 = np.asarray(np.broadcast_to(hi, 3), dtype=np.float32)
    den = np.asarray([max(n - 1, 1) for n in dims], dtype=np.float32)
    return lo32, ((hi32 - lo32) / den).astype(np.float32)


def lookup(occ: np.ndarray, lo, step, x) -> np.ndarray:
    """(..., 3) fp32 points -> bool occupied, by the convention above."""
    x = np.asarray(x, dtype=np.float32)
    lo = np.asarray(lo, dtype=np.float32)
    step = np.asarray(step, dtype=np.float32)
    cells = np.asarray(occ.shape, dtype=np.int64)
    hi = (lo + (cells.astype(np.float32) * step).astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.all((x >= lo) & (x <= hi), axis=-1)
        q = np.floor(((x - lo).astype(np.float32) / step).astype(np.float32))
    q = np.where(np.isfinite(q), q, 0).astype(np.int64)
    c = np.minimum(np.maximum(q, 0), cells - 1)
    return inside & occ[c[..., 0], c[..., 1], c[..., 2]]


def cast(o, d, t) -> np.ndarray:
    """helper.cast_rays in fp32: o + t * d, multiply then add; o, d (n, 3), t (n, S) -> (n, S, 3)."""
    o = np.asarray(o, dtype=np.float32)[:, None, :]
    d = np.asarray(d, dtype=np.float32)[:, None, :]
    t = np.asarray(t, dtype=np.float32)[..., None]
    return (o + (t * d).astype(np.float32)).astype(np.float32)
