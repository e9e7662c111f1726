"""The yardstick of occupancy grids for scenes, composed of tests/_occ_ref.py (the lookup of section 4.9, written from
the convention) and the dense stage call: for object k's segment of the pair rows, the raw records of ``ops.scene_art_mlp_fwd`` with every
row where ``_occ_ref.lookup(grid_k, _occ_ref.cast(o', d', t))`` is false overwritten by the sentinel (0, 0, 0, -inf).  An object without a
grid keeps its dense records.  Also: fabricated segments (the stage call takes ``starts`` and the pair arrays directly, so sizes are exact)
and the grid kinds the tests rotate through.  numpy only; nothing here imports the package at module level."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _occ_ref  # noqa: E402

SENTINEL = np.array([0.0, 0.0, 0.0, -np.inf], dtype=np.float32)
KINDS = ("random", "halfspace", "full", "empty", None)


class Cells:
    """A grid on the host: ``occ`` (cx, cy, cz) bool, fp32 ``lo`` / ``step`` (3,)."""

    def __init__(self, occ, lo, step):
        self.occ = np.asarray(occ, dtype=bool)
        self.lo = np.asarray(np.broadcast_to(lo, 3), dtype=np.float32).copy()
        self.step = np.asarray(np.broadcast_to(step, 3), dtype=np.float32).copy()

    @property
    def hi(self):
        return (self.lo + (np.asarray(self.occ.shape, dtype=np.float32) * self.step).astype(np.float32)).astype(np.float32)

    def to_ops(self, device):
        """-> ops.OccupancyGrid with these bits on `device` (a torch device, "cpu" included: the argument tests)"""
        import torch
        from aon_amd import ops

        bits = torch.from_numpy(_occ_ref.pack_bits(self.occ).view(np.int32).copy()).to(device)
        return ops.OccupancyGrid(bits, self.occ.shape, self.lo, self.step, 0.0, 0)


def make_cells(kind, seed, cells=(7, 5, 6), lo=(-1.0, -0.9, -1.1), step=(0.3, 0.35, 0.37)):
    """One of KINDS -> Cells or None.  The default extent (about [-1, 1.1]^3, uneven steps) is smaller than where fabricated samples fall, so
    every kind but None also meets samples outside the grid."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    shape = tuple(cells)
    if kind == "random":
        occ = rng.random(shape) < 0.5
    elif kind == "halfspace":
        i, j, _ = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
        occ = (2 * i + j) >= shape[0]
    elif kind == "full":
        occ = np.ones(shape, dtype=bool)
    elif kind == "empty":
        occ = np.zeros(shape, dtype=bool)
    else:
        raise ValueError(kind)
    return Cells(occ, lo, step)


def enclosing(kind, seed, half=64.0, cells=(3, 2, 2)):
    """"full" / "empty" cells over [-half, half]^3: a grid every sample of a scene falls into"""
    c = make_cells(kind, seed, cells, (-half,) * 3, [2 * half / n for n in cells])
    return c


def fabricated_pairs(seed, P, S):
    """(P, 3) origins and directions, (P, 3) unit view directions and ascending (P, S) t with samples in and around [-1.6, 1.6]^3, some NaN-free
    but far outside every grid"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.5, 1.5, (P, 3)).astype(np.float32)
    d = rng.normal(size=(P, 3)).astype(np.float32)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6).astype(np.float32)
    v = d.copy()
    t = np.sort(rng.uniform(0.0, 2.5, (P, S)), axis=1).astype(np.float32)
    return o, d, v, t


def segment_mask(cells, o, d, t):
    """(rows, S) bool: the samples of a segment that are occupied; all of them for cells None"""
    if cells is None:
        return np.ones(t.shape, dtype=bool)
    return _occ_ref.lookup(cells.occ, cells.lo, cells.step, _occ_ref.cast(o, d, t))


def local_list(mask):
    """the ascending segment-local sample indices row_local * S + i of the occupied samples"""
    return np.flatnonzero(np.asarray(mask).reshape(-1)).astype(np.int32)


def yardstick(dense_raw, starts, grids, o, d, t):
    """dense_raw (P, S, 4) -> (the expected records, [occupied count per object], [mask per object])"""
    want = np.array(dense_raw, dtype=np.float32, copy=True)
    counts, masks = [], []
    for k, cells in enumerate(grids):
        seg = slice(int(starts[k]), int(starts[k + 1]))
        m = segment_mask(cells, o[seg], d[seg], t[seg])
        want[seg][~m] = SENTINEL
        counts.append(int(m.sum()))
        masks.append(m)
    return want, counts, masks
