"""Occupancy grids for scenes, what can be checked without a GPU: the fourth header include/aon_hip_scene_occ.h
against the library and the binding (the discipline tests/test_scene_cpu.py keeps for its header), every refusal of the stage call -- code,
message, rank -- on fake pointers, the workspace query, the argument rules of scene.SceneObject's grid, and the reference's own list."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _occ_ref  # noqa: E402
import _scene_occ_ref as oref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene_occ.h"

# ---- header, library, binding ----
# hand-written: p = c_void_p, i = c_int, l = c_int64
SCENE_OCC_ARGTYPES = {
    "aon_scene_occ_workspace_bytes": (C.c_int64, "l i i"),
    "aon_scene_art_mlp_fwd_occ": (C.c_int, "p p p p p p p p i i p p p l p"),
}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def scene_occ_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))


def scene_occ_stream_entry_points():
    return sorted({m.group(1) for m in re.finditer(r"\b(aon_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", _stripped(HEADER), flags=re.S)
                   if re.search(r"\bstream\b", m.group(2))})


def test_scene_occ_header_library_and_binding_agree():
    from aon_amd import _lib
    from test_abi_cpu import declared_symbols
    from test_scene_cpu import scene_declared_symbols
    from test_vanilla_ray_grads_cpu import ext_declared_symbols

    names = scene_occ_declared_symbols()
    assert names == sorted(SCENE_OCC_ARGTYPES) == _lib.scene_occ_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = SCENE_OCC_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_OCC_SIGS[n][1]) == list(fn.argtypes), n
    # none of the other three headers nor their tables know them
    others = (set(declared_symbols()) | set(ext_declared_symbols()) | set(scene_declared_symbols()) | set(_lib.exported_symbols())
              | set(_lib.extension_symbols()) | set(_lib.scene_symbols()))
    assert not set(names) & others
    assert '#include "aon_hip_scene.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5
    # the grid record the entry point reads: 56 bytes, bits first
    assert C.sizeof(_lib.OccupancyC) == 56 and [f[0] for f in _lib.OccupancyC._fields_] == ["bits", "cells", "lo", "step"]


def test_the_stream_entry_point_of_the_header_is_in_the_guard_cases():
    import test_hip_scene_occ as gpu

    names = scene_occ_stream_entry_points()
    assert names == ["aon_scene_art_mlp_fwd_occ"]
    assert set(names) <= set(gpu.GUARD_REACHES) and len(gpu.STAGE_CASES) >= 3


# ---- the refusal table ----
BASE = 0x7C000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced
INVALID, WORKSPACE = -1, -2
FORMS = ("two of the packed buffers of this call were made in different forms (aon_set_bottleneck_fold changed between the pack / prepare calls), "
         "or one of them was never packed or declared by this process (a copy: aon_declare_stream_form)")


def _fake(i):
    return BASE + 0x1000 * i


class OccEntry:
    """ORDER: the argument names in the ABI's order; base: a call that would be valid (3 objects, the middle one without rows and without a
    per-call block, the last one without a grid); rows(): (label, overrides, rank, rc, message)"""
    WHO = "aon_scene_art_mlp_fwd_occ"
    ORDER = ["packed", "smalls", "grids", "starts", "pair_o", "pair_d", "pair_v", "t_vals", "k", "s", "raw", "occupied", "ws", "ws_bytes", "stream"]
    POINTERS = ["packed", "smalls", "grids", "pair_o", "pair_d", "pair_v", "t_vals", "raw", "ws"]
    K, S, STARTS = 3, 65, (0, 5, 5, 12)

    def __init__(self):
        from aon_amd import _lib

        self._lib = _lib
        self.lib = _lib.lib
        self.keep = []
        a = {k: _fake(i + 1) for i, k in enumerate(["packed", "pair_o", "pair_d", "pair_v", "t_vals", "raw", "occupied", "ws"])}
        self.small_ptrs = [_fake(40), None, _fake(42)]
        a.update(smalls=self.smalls(self.small_ptrs), grids=self.grids([self.grid(), self.grid(), None]), starts=self.starts(self.STARTS),
                 k=self.K, s=self.S, stream=None, ws_bytes=self.lib.aon_scene_occ_workspace_bytes(self.STARTS[-1], self.K, self.S))
        assert a["ws_bytes"] > 0
        self.base = a

    # host arrays (kept alive by self.keep)
    def smalls(self, ptrs):
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self.keep.append(arr)
        return arr

    def starts(self, values):
        arr = (C.c_int64 * len(values))(*values)
        self.keep.append(arr)
        return arr

    def grid(self, bits=_fake(60), cells=(4, 5, 6), lo=(-1.0, -1.0, -1.0), step=(0.5, 0.4, 0.4)):
        st = self._lib.OccupancyC()
        st.bits = bits
        st.cells[:], st.lo[:], st.step[:] = cells, lo, step
        self.keep.append(st)
        return st

    def grids(self, structs):
        arr = (C.c_void_p * len(structs))(*[None if st is None else C.addressof(st) for st in structs])
        self.keep.append(arr)
        return arr

    def call(self, overrides):
        args = dict(self.base)
        args.update({k: v for k, v in overrides.items() if not k.startswith("_")})
        # the forms of the fake packed stream and per-call blocks, declared anew for every call
        assert self.lib.aon_declare_stream_form(C.c_void_p(self.base["packed"]), 1) == 0
        for j, p in enumerate(self.small_ptrs):
            if p is not None:
                assert self.lib.aon_declare_stream_form(C.c_void_p(p), overrides.get(f"_form_small{j}", 1)) == 0
        rc = getattr(self.lib, self.WHO)(*[args[k] for k in self.ORDER])
        return rc, self.lib.aon_last_error().decode()

    def rows(self):
        who, g = self.WHO, self.grid
        size = "bad object count / sample count (1 <= k <= 16, s >= 1)"
        asc = "starts_host must ascend from starts_host[0] = 0"
        cells = "every cell count must be in [1, 2^24]"
        step = "occupancy lo must be finite and step finite and > 0"
        r = [("k = 0", {"k": 0}, 1, INVALID, size), ("k = 17", {"k": 17}, 1, INVALID, size), ("s = 0", {"s": 0}, 1, INVALID, size),
             ("starts = NULL", {"starts": None}, 2, INVALID, asc), ("starts[0] = 1", {"starts": self.starts((1, 5, 5, 12))}, 2, INVALID, asc),
             ("starts descend", {"starts": self.starts((0, 5, 4, 12))}, 2, INVALID, asc),
             ("starts[k] = -1", {"starts": self.starts((0, 0, 0, -1))}, 2, INVALID, asc),
             ("pairs * s = 2^31", {"starts": self.starts((0, 5, 5, 2 ** 31 // 64)), "s": 64}, 3, INVALID, "more than 2^31 - 1 samples (starts_host[k] * s)")]
        r += [(k + " = NULL", {k: None}, 4, INVALID, "null pointer") for k in self.POINTERS]
        r += [("smalls[0] = NULL", {"smalls": self.smalls([None, None, _fake(42)])}, 4, INVALID, "null pointer"),
              ("smalls[2] = NULL", {"smalls": self.smalls([_fake(40), None, None])}, 4, INVALID, "null pointer")]
        r += [("grid 0: null bits", {"grids": self.grids([g(bits=None), g(), None])}, 5, INVALID, "object 0: null occupancy grid"),
              ("grid 1 (no rows): cells = 0", {"grids": self.grids([g(), g(cells=(4, 0, 6)), None])}, 5, INVALID, "object 1: " + cells),
              ("grid 2: cells = -3", {"grids": self.grids([None, None, g(cells=(-3, 5, 6))])}, 5, INVALID, "object 2: " + cells),
              ("grid 0: step = 0", {"grids": self.grids([g(step=(0.5, 0.0, 0.4)), g(), None])}, 5, INVALID, "object 0: " + step),
              ("grid 0: step < 0", {"grids": self.grids([g(step=(-0.5, 0.4, 0.4)), g(), None])}, 5, INVALID, "object 0: " + step),
              ("grid 0: step = NaN", {"grids": self.grids([g(step=(float("nan"), 0.4, 0.4)), g(), None])}, 5, INVALID, "object 0: " + step)]
        align = "raw must be 16-byte aligned and the workspace 256-byte aligned"
        r += [("misaligned raw", {"raw": self.base["raw"] + 8}, 6, INVALID, align), ("misaligned workspace", {"ws": self.base["ws"] + 128}, 6, INVALID, align)]
        rows = [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]
        rows += [("small 0 in the other form", {"_form_small0": 0}, 7, INVALID, FORMS), ("small 2 in the other form", {"_form_small2": 0}, 7, INVALID, FORMS)]
        rows += [("workspace one byte short", {"ws_bytes": self.base["ws_bytes"] - 1}, 8, WORKSPACE,
                  f"{who}: workspace smaller than aon_scene_occ_workspace_bytes()")]
        return rows


def test_every_prelaunch_refusal():
    e = OccEntry()
    rows = e.rows()
    assert len(rows) >= 28 and {r[2] for r in rows} == set(range(1, 9))
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label


def test_refusals_keep_their_rank():
    """Two faults at once: the refusal that ranks first is the one reported."""
    e = OccEntry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > 200


def test_a_segment_without_rows_needs_no_block_and_no_pairs_is_a_success():
    e = OccEntry()
    # the base call's middle object has no rows and a NULL per-call block: the call gets as far as its last refusal
    assert e.base["smalls"][1] is None
    assert e.call({"ws_bytes": e.base["ws_bytes"] - 1})[0] == WORKSPACE
    # no pairs: success before any pointer is looked at, nothing launched
    empty = {"starts": e.starts((0, 0, 0, 0))}
    assert e.call(empty)[0] == 0
    assert e.call({**empty, "raw": None, "ws": None, "packed": None, "ws_bytes": 0})[0] == 0
    assert e.call({**empty, "k": 17})[0] == INVALID


def test_workspace_query_is_monotone_and_aligned():
    from aon_amd import _lib

    q = _lib.lib.aon_scene_occ_workspace_bytes
    # lists (4 B per sample) + tile counts + tile offsets (a tile: 1,024 samples of one object) + k counters, 256-byte aligned pieces
    assert q(12, 3, 65) == 3328 + 256 + 256 + 256
    assert q(0, 1, 1) == 4 * 256
    sizes = [(p, k, s) for p in (0, 1, 15, 16, 17, 300, 4097, 70000) for k in (1, 3, 16) for s in (1, 9, 64, 65, 193)]
    for p, k, s in sizes:
        b = q(p, k, s)
        tiles = p * s // 1024 + k                       # >= sum_k ceil(P_k s / 1024) for every split of p rows over k objects
        assert b > 0 and b % 256 == 0 and b >= 4 * p * s + 8 * tiles + 8 * k, (p, k, s)
        assert q(p + 1, k, s) >= b and q(p, k, s + 1) >= b and (k == 16 or q(p, k + 1, s) >= b), (p, k, s)
    for p, k, s in ((-1, 1, 1), (5, 0, 9), (5, 17, 9), (5, 3, 0), (2 ** 31 // 64, 3, 64)):
        assert q(p, k, s) == 0, (p, k, s)
    assert q((2 ** 31 - 1) // 64, 3, 64) > 0


# ---- scene.SceneObject's grid ----
def _latents():
    return {"density": torch.zeros(1, 128), "color": torch.zeros(1, 128), "articulation": torch.zeros(1, 32)}


def _pose():
    return torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)


def test_scene_object_grid_rules():
    from aon_amd import ops, scene

    assert scene.SceneObject(_latents(), _pose(), 2.0).grid is None and scene.SceneObject(_latents(), _pose(), 2.0, None).grid is None
    with pytest.raises(TypeError, match="grid must be an ops.OccupancyGrid"):
        scene.SceneObject(_latents(), _pose(), 2.0, grid=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="grid must be an ops.OccupancyGrid"):
        scene.SceneObject(_latents(), _pose(), 2.0, grid={"bits": None})
    # [-1, 1]^3 in 4 cells of 0.5 per axis: the box of side 2 fits exactly, one of side 2.1 does not, nor does a shifted one
    inside = oref.make_cells("full", 0, (4, 4, 4), (-1.0,) * 3, (0.5,) * 3).to_ops("cpu")
    assert isinstance(inside, ops.OccupancyGrid)
    for box in (2.1, ((-0.5, -0.5, -0.5), (0.5, 1.01, 0.5)), ((-1.2, 0.0, 0.0), (0.0, 0.5, 0.5))):
        with pytest.raises(ValueError, match="does not contain the box"):
            scene.SceneObject(_latents(), _pose(), box, grid=inside)
    # a grid that contains the box but lives on the host: refused for that
    for box in (2.0, 1.0, ((-1.0, -0.5, 0.0), (0.25, 1.0, 0.5))):
        with pytest.raises(ValueError, match="must be on a cuda"):
            scene.SceneObject(_latents(), _pose(), box, grid=inside)


def test_render_scene_refuses_what_it_refused_before_with_a_grid_argument_present():
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ok = scene.SceneObject(_latents(), _pose(), 2.0)
    rays = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs")}
    with pytest.raises(RuntimeError, match="inference only: call it under torch.no_grad"):
        scene.render_scene(NeRF_AE_Art(), [ok], rays, True, want_occupied=True)
    with torch.no_grad():
        with pytest.raises(ValueError, match="randomized=True is refused"):
            scene.render_scene(NeRF_AE_Art(), [ok], rays, True, randomized=True, want_occupied=True)


# ---- the reference's own list ----
def test_one_object_list_is_the_flatnonzero_of_the_occupancy_mask():
    """K = 1: the segment-local list of the scene yardstick is np.flatnonzero of section 4.9's mask, and the yardstick overwrites exactly the
    other rows"""
    P, S = 17, 64
    o, d, v, t = oref.fabricated_pairs(3, P, S)
    for kind in ("random", "halfspace", "full", "empty"):
        cells = oref.make_cells(kind, 11)
        mask49 = _occ_ref.lookup(cells.occ, cells.lo, cells.step, _occ_ref.cast(o, d, t))
        assert np.array_equal(oref.local_list(oref.segment_mask(cells, o, d, t)), np.flatnonzero(mask49))
        dense = np.random.default_rng(5).normal(size=(P, S, 4)).astype(np.float32)
        want, counts, masks = oref.yardstick(dense, [0, P], [cells], o, d, t)
        assert counts == [int(mask49.sum())] and np.array_equal(masks[0], mask49)
        assert np.array_equal(want[mask49], dense[mask49]) and np.array_equal(want[~mask49], np.broadcast_to(oref.SENTINEL, want[~mask49].shape))
        if kind in ("random", "halfspace"):
            assert 0 < counts[0] < P * S
        if kind == "full":
            assert 0 < counts[0] < P * S          # samples outside the grid's extent are empty even when every cell is set
    # no grid: dense
    want, counts, _ = oref.yardstick(dense, [0, 5, 5, P], [None, None, None], o, d, t)
    assert np.array_equal(want, dense) and counts == [5 * S, 0, (P - 5) * S]
    # a NaN coordinate is empty
    t_nan = t.copy()
    t_nan[0, 0] = np.nan
    assert not oref.segment_mask(oref.make_cells("full", 0), o, d, t_nan)[0, 0]
