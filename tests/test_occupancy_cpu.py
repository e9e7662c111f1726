"""CPU: the occupancy-grid convention through its numpy reference on hand-computed cases, and the C ABI / Python
wrappers' argument checks, which need no GPU."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import _occ_ref as ref

AON_E_INVALID = -1


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_single_hot_corner_dilates_into_a_cube():
    d = np.zeros((9, 9, 9), np.float32)
    d[4, 4, 4] = 1.0
    for r, lo_c, hi_c in ((0, 3, 4), (1, 2, 5), (2, 1, 6)):
        occ = ref.cell_occupancy(d, 0.5, r)
        want = np.zeros((8, 8, 8), bool)
        want[lo_c: hi_c + 1, lo_c: hi_c + 1, lo_c: hi_c + 1] = True
        assert np.array_equal(occ, want), r
        assert occ.sum() == (2 + 2 * r) ** 3


def test_hot_corner_on_the_boundary_is_clamped():
    d = np.zeros((6, 7, 8), np.float32)
    d[0, 0, 7] = 3.0
    occ = ref.cell_occupancy(d, 0.5, 1)
    want = np.zeros((5, 6, 7), bool)
    want[0:2, 0:2, 5:7] = True   # cell (0, 0, 6) owns the corner; dilation by 1 stays inside the grid
    assert np.array_equal(occ, want)


def test_threshold_is_strict_and_nan_counts_as_occupied():
    d = np.zeros((3, 3, 3), np.float32)
    d[0, 0, 0] = 0.25                      # == threshold: empty
    assert not ref.cell_occupancy(d, 0.25, 0).any()
    d[2, 2, 2] = np.nan
    occ = ref.cell_occupancy(d, 0.25, 0)
    assert occ.sum() == 1 and occ[1, 1, 1]
    assert ref.cell_occupancy(d, 0.25, 1).all()


def test_sphere_field_against_brute_force():
    n, lo, hi, rad = 9, -1.0, 1.0, 0.55
    xs = [lo + i * (hi - lo) / (n - 1) for i in range(n)]
    d = np.zeros((n, n, n), np.float32)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                d[i, j, k] = 1.0 if math.sqrt(xs[i] ** 2 + xs[j] ** 2 + xs[k] ** 2) < rad else 0.0
    occ = ref.cell_occupancy(d, 0.5, 0)
    count = 0
    for i in range(n - 1):
        for j in range(n - 1):
            for k in range(n - 1):
                hot = any(d[i + a, j + b, k + c] > 0.5 for a in (0, 1) for b in (0, 1) for c in (0, 1))
                assert occ[i, j, k] == hot
                count += hot
    # 33 points lie within 0.55 of the origin (integer offsets o with |o|^2 <= 4 at spacing 0.25): the 3^3 block around it, touched by
    # 4^3 cells, and the 6 points at distance 2 on the axes, each adding the 4 cells beyond the block -> 64 + 24
    assert count == occ.sum() == 4 ** 3 + 6 * 4


def test_bit_packing_order():
    occ = np.zeros((2, 3, 7), bool)          # 42 cells, 2 words
    occ.reshape(-1)[33] = True
    occ.reshape(-1)[0] = True
    occ.reshape(-1)[31] = True
    w = ref.pack_bits(occ)
    assert w.dtype == np.uint32 and w.tolist() == [1 | (1 << 31), 2]


def test_lookup_boundaries():
    occ = np.ones((4, 4, 4), bool)
    lo, step = ref.grid_step((5, 5, 5), -1.0, 1.0)
    hi = np.float32(-1.0) + np.float32(4.0) * step[0]
    pts = np.array([[-1, -1, -1], [hi, hi, hi], [0, 0, 0], [np.nextafter(hi, np.float32(9)), 0, 0], [np.nextafter(np.float32(-1), np.float32(-9)), 0, 0],
                    [np.nan, 0, 0], [0, 5, 0], [0, 0, -5]], np.float32)
    assert ref.lookup(occ, lo, step, pts).tolist() == [True, True, True, False, False, False, False, False]
    # x == hi clamps into the last cell; which cell a point falls into
    occ = np.zeros((4, 4, 4), bool)
    occ[3, 3, 3] = True
    assert ref.lookup(occ, lo, step, np.array([[hi, hi, hi]], np.float32)).tolist() == [True]
    occ = np.zeros((4, 4, 4), bool)
    occ[2, 1, 0] = True
    assert ref.lookup(occ, lo, step, np.array([[0.0, -0.5, -1.0], [0.49, -0.01, -0.6], [-0.01, -0.5, -1.0]], np.float32)).tolist() == [True, True, False]


def test_lookup_matches_brute_force_on_random_points():
    rng = np.random.default_rng(0)
    occ = rng.random((5, 6, 7)) < 0.5
    lo, step = ref.grid_step((6, 7, 8), (-1.0, -1.5, -0.5), (1.0, 1.5, 0.5))
    x = rng.uniform(-2, 2, size=(4000, 3)).astype(np.float32)
    got = ref.lookup(occ, lo, step, x)
    for p, g in zip(x, got):
        want = True
        idx = []
        for a in range(3):
            hi_a = np.float32(lo[a] + np.float32(np.float32(occ.shape[a]) * step[a]))
            if not (lo[a] <= p[a] <= hi_a):
                want = False
                break
            idx.append(min(int(np.floor(np.float32(np.float32(p[a] - lo[a]) / step[a]))), occ.shape[a] - 1))
        if want:
            want = bool(occ[tuple(idx)])
        assert g == want


# ---------------------------------------------------------------------------------------------------------------- C ABI without a GPU
def test_symbols_exported_and_sizes():
    from aon_amd import _lib

    for name in ("aon_occupancy_bytes", "aon_occupancy_build", "aon_render_occ_workspace_bytes", "aon_render_fwd_occ", "aon_art_render_fwd_occ"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    lib = _lib.lib
    assert lib.aon_occupancy_bytes((ctypes.c_int64 * 3)(128, 128, 128)) == 256 * 1024
    assert lib.aon_occupancy_bytes((ctypes.c_int64 * 3)(3, 3, 3)) == 4
    assert lib.aon_occupancy_bytes((ctypes.c_int64 * 3)(0, 3, 3)) == AON_E_INVALID
    assert lib.aon_occupancy_bytes(None) == AON_E_INVALID
    # the workspace holds the render workspace plus 4 B per fine sample (the sample list)
    plain = lib.aon_render_workspace_bytes_ex(1000, None)
    occ = lib.aon_render_occ_workspace_bytes(1000, None)
    assert occ >= plain + 1000 * 193 * 4


def _occ_struct(bits=0x1000):
    from aon_amd import _lib

    st = _lib.OccupancyC()
    st.bits = bits
    for a in range(3):
        st.cells[a], st.lo[a], st.step[a] = 4, -1.0, 0.5
    return st


def test_build_refuses_bad_arguments():
    from aon_amd import _lib

    lib = _lib.lib
    dims = (ctypes.c_int64 * 3)(5, 5, 5)
    fake = ctypes.c_void_p(0x1000)
    assert lib.aon_occupancy_build(None, dims, 0.01, 1, fake, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, dims, 0.01, 1, None, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, None, 0.01, 1, fake, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, (ctypes.c_int64 * 3)(1, 5, 5), 0.01, 1, fake, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, dims, 0.01, 9, fake, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, dims, 0.01, -1, fake, None) == AON_E_INVALID
    assert lib.aon_occupancy_build(fake, dims, float("nan"), 1, fake, None) == AON_E_INVALID
    assert b"NaN" in lib.aon_last_error()


def _render(fn, art, occ, t_rand=None, opts=None):
    n_ptrs = 4 if art else 2
    fake = ctypes.c_void_p(0x1000)
    args = [fake] * n_ptrs + [fake, fake, fake, 8, 2.0, 6.0, 1, 2, t_rand, fake, 0] + [fake] * 6 + [fake, 1 << 30, None, opts,
                                                                                                  None if occ is None else ctypes.byref(occ), None]
    return fn(*args)


def test_render_refuses_bad_grids_and_training_options():
    from aon_amd import _lib, ops

    lib = _lib.lib
    for fn, art in ((lib.aon_render_fwd_occ, False), (lib.aon_art_render_fwd_occ, True)):
        assert _render(fn, art, None) == AON_E_INVALID
        assert b"null occupancy grid" in lib.aon_last_error()
        assert _render(fn, art, _occ_struct(bits=0)) == AON_E_INVALID
        bad = _occ_struct()
        bad.step[1] = 0.0
        assert _render(fn, art, bad) == AON_E_INVALID
        bad = _occ_struct()
        bad.cells[2] = 0
        assert _render(fn, art, bad) == AON_E_INVALID
        assert _render(fn, art, _occ_struct(), t_rand=ctypes.c_void_p(0x1000)) == AON_E_INVALID
        assert b"t_rand" in lib.aon_last_error()
        st, _ = ops.RenderOpts(noise_std=1.0).c_struct(2.0, 6.0)
        st.noise_std, st.noise_c = 1.0, 0x1000
        assert _render(fn, art, _occ_struct(), opts=ctypes.byref(st)) == AON_E_INVALID
        assert b"noise" in lib.aon_last_error()
    st, _ = ops.RenderOpts(degrees=(0, 8, 4)).c_struct(2.0, 6.0)
    assert _render(lib.aon_render_fwd_occ, False, _occ_struct(), opts=ctypes.byref(st)) == AON_E_INVALID
    assert b"degrees" in lib.aon_last_error()


def test_python_wrappers_raise_on_bad_arguments():
    from aon_amd import ops

    with pytest.raises(RuntimeError):
        ops.occupancy_grid(torch.zeros(4, 4, 4), -1.0, 1.0)          # a CPU tensor: no host fallback
    x = torch.zeros(4, 3)
    with pytest.raises(TypeError):
        ops.render_fwd_occ(None, None, x, x, x, 2.0, 6.0, True, grid="not a grid")
    with pytest.raises(TypeError):
        ops.art_render_fwd_occ(None, None, None, None, x, x, x, 2.0, 6.0, True, grid=None)
    g = ops.OccupancyGrid(torch.zeros(2, dtype=torch.int32), (4, 4, 4), (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5), 0.01, 1)
    with pytest.raises(ValueError):
        ops.render_fwd_occ(None, None, x, x, x, 2.0, 6.0, True, g, num_levels=3)


# ---------------------------------------------------------------------------------------------------------------- the workspace queries
def _workspace_table():
    """The three occupancy workspace queries over the table of tests/golden/g29_occ_workspace_bytes.json, in that file's shape."""
    from aon_amd import _lib, ops

    lib = _lib.lib
    render = {}
    for name, opts in (("default", None), ("63_64", ops.RenderOpts(num_coarse_samples=63, num_fine_samples=64))):
        st = None if opts is None else ctypes.byref(opts.c_struct(2.0, 6.0)[0])
        render[name] = [[n, int(lib.aon_render_occ_workspace_bytes(n, st)), int(lib.aon_render_stop_workspace_bytes(n, st))]
                        for n in (0, 1, 5, 16, 17, 340, 1024, 65536, 327680)]
    scene = [[pairs, k, s, int(lib.aon_scene_occ_workspace_bytes(pairs, k, s))]
             for pairs in (0, 1, 16, 17, 300, 65536) for k in (1, 3, 16) for s in (9, 64, 193)]
    return {"render": render, "scene": scene}


def test_workspace_queries_return_the_recorded_sizes():
    """aon_render_occ_workspace_bytes, aon_render_stop_workspace_bytes (rows: n_rays, occ bytes, stop bytes; default and (63, 64) sample
    counts) and aon_scene_occ_workspace_bytes (rows: pairs, k, s, bytes) against the answers recorded from the library before the three
    compactions shared one workspace layout: callers size their buffers with these, so every answer stays what it was."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g29_occ_workspace_bytes.json")) as f:
        want = json.load(f)
    assert _workspace_table() == want
