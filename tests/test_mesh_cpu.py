"""CPU: the numpy marching-cubes reference (tests/_mc_ref.py) -- its case table, watertight and consistently oriented meshes of analytic fields
with the right volume and area -- argument validation of the mesh entry points (no GPU needed), and the PLY writer's round trip."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mc_ref as R


def _field(N, f, lo=-1.0, hi=1.0):
    st = R.step_of(lo, hi, N)
    c = R.grid_coords(N, lo, st).astype(np.float64)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    return f(X, Y, Z).astype(np.float32), st


def sphere(r, c=(0.0, 0.0, 0.0)):
    return lambda X, Y, Z: r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)


def torus(R0, r):
    return lambda X, Y, Z: r - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R0) ** 2 + Z ** 2)


FIELDS = {
    "sphere": (sphere(0.7), 4 / 3 * np.pi * 0.7 ** 3, 4 * np.pi * 0.7 ** 2),
    "torus": (torus(0.55, 0.25), 2 * np.pi ** 2 * 0.55 * 0.25 ** 2, 4 * np.pi ** 2 * 0.55 * 0.25),
    "offcentre_sphere": (sphere(0.4, (0.21, -0.13, 0.3)), 4 / 3 * np.pi * 0.4 ** 3, 4 * np.pi * 0.4 ** 2),
}


def test_table_uses_exactly_the_sign_change_edges():
    assert len(R.TRI_TABLE) == 256
    assert R.table_mismatches() == []
    assert R.TRI_TABLE[0] == [] and R.TRI_TABLE[255] == []
    for case in range(256):   # a case and its complement cut the same edges
        assert R.EDGE_TABLE[case] == R.EDGE_TABLE[255 - case]


@pytest.mark.parametrize("name,N", [("sphere", 128), ("torus", 128), ("offcentre_sphere", 40), ("offcentre_sphere", 77), ("offcentre_sphere", 128)])
def test_reference_mesh_is_closed_oriented_and_accurate(name, N):
    f, vol, area = FIELDS[name]
    v, st = _field(N, f)
    assert R.ambiguous_faces(v, 0.0) == 0   # no face where the classic table may leave a hole
    verts, faces = R.marching_cubes(v, 0.0, [-1.0] * 3, [st] * 3)
    assert len(faces) > 0
    _, cnt = R.edge_use_counts(faces)
    assert (cnt == 2).all(), "every edge is shared by exactly two faces"
    assert R.directed_edges_consistent(faces)
    sv = R.signed_volume(verts, faces)
    assert sv > 0
    if N == 128:
        assert abs(sv / vol - 1) < 0.01
        assert abs(R.area(verts, faces) / area - 1) < 0.02
    # every vertex is used, and sits on its edge
    assert np.unique(faces).size == len(verts)


def test_reference_ordering_and_nan():
    v = np.full((3, 3, 3), -1.0, dtype=np.float32)
    v[1, 1, 1] = 1.0
    v[1, 1, 2] = np.nan
    verts, faces = R.marching_cubes(v, 0.0, [0.0] * 3, [1.0] * 3)
    # six edges around the centre: owned by (0,1,1) +x, (1,0,1) +y, (1,1,0) +z, then the centre's own +x, +y, +z
    assert verts.tolist()[:3] == [[0.5, 1.0, 1.0], [1.0, 0.5, 1.0], [1.0, 1.0, 0.5]]
    assert verts.tolist()[3:5] == [[1.5, 1.0, 1.0], [1.0, 1.5, 1.0]]
    assert verts.tolist()[5] == [1.0, 1.0, 1.0]   # the NaN endpoint is outside: the vertex sits on the inside endpoint
    assert len(faces) == 8 and R.signed_volume(verts, faces) > 0


def test_argument_validation_without_gpu():
    from aon_amd import _lib

    lib = _lib.lib
    d = (C.c_int64 * 3)(4, 4, 4)
    lo, st = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert lib.aon_density_grid(None, d, lo, st, 0, 64, 1, None, None) == -1
    assert b"null pointer" in lib.aon_last_error()
    assert lib.aon_density_grid(None, d, lo, st, 0, 65, 1, None, None) == -1
    assert b"g_end" in lib.aon_last_error()
    assert lib.aon_density_grid(None, d, lo, st, 0, 64, 3, None, None) == -1
    assert b"act" in lib.aon_last_error()
    assert lib.aon_density_grid(None, None, lo, st, 0, 64, 1, None, None) == -1
    assert lib.aon_density_grid(None, (C.c_int64 * 3)(4, 0, 4), lo, st, 0, 0, 1, None, None) == -1
    assert lib.aon_art_density_grid(None, None, d, lo, st, 0, 64, 2, None, None) == -1
    assert b"null pointer" in lib.aon_last_error()
    assert lib.aon_density_grid(None, d, lo, st, 5, 5, 1, None, None) == 0   # an empty slab is a no-op
    assert lib.aon_art_density_grid(None, None, d, lo, st, 7, 7, 2, None, None) == 0
    # marching cubes
    assert lib.aon_marching_cubes_workspace_bytes((C.c_int64 * 3)(1, 4, 4)) == -1
    assert b"[2, 2^24]" in lib.aon_last_error()
    ws = lib.aon_marching_cubes_workspace_bytes(d)
    assert ws >= 64 * 4
    counts = (C.c_int64 * 2)()
    assert lib.aon_marching_cubes_count(None, d, C.c_float(0.0), None, ws, counts, None) == -1
    assert b"null pointer" in lib.aon_last_error()
    assert lib.aon_marching_cubes_count(C.c_void_p(16), d, C.c_float(0.0), C.c_void_p(16), ws - 1, counts, None) == -2
    assert lib.aon_marching_cubes_count(C.c_void_p(16), d, C.c_float(0.0), C.c_void_p(24), ws, counts, None) == -1
    assert b"aligned" in lib.aon_last_error()
    assert lib.aon_marching_cubes(C.c_void_p(16), d, C.c_float(0.0), lo, st, C.c_void_p(16), ws, None, 3, None, 0, None) == -1
    assert b"null output" in lib.aon_last_error()
    assert lib.aon_marching_cubes(C.c_void_p(16), d, C.c_float(0.0), lo, st, C.c_void_p(16), ws, None, -1, None, 0, None) == -1


def test_ops_mesh_entries_reject_cpu_tensors():
    from aon_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.0, -1.0, 1.0)
    with pytest.raises(RuntimeError, match="cuda tensor"):
        ops.density_grid(torch.zeros(16), 4, -1.0, 1.0, 1)


def test_grid_points_formula():
    from aon_amd import ops

    lo32, step = ops.grid_step((5, 3, 9), (-1.0, 0.0, -0.3), (1.0, 2.0, 0.7))
    assert step.dtype == torch.float32
    assert step[0].item() == np.float32(np.float32(2.0) / np.float32(4))
    pts = ops.grid_points((5, 3, 9), (-1.0, 0.0, -0.3), (1.0, 2.0, 0.7), 10, 20, device="cpu")
    for n, g in enumerate(range(10, 20)):
        i, j, k = g // 27, (g // 9) % 3, g % 9
        for a, idx in enumerate((i, j, k)):
            want = np.float32(np.float32(lo32[a].item()) + np.float32(np.float32(idx) * np.float32(step[a].item())))
            assert pts[n, a].item() == want


@pytest.mark.parametrize("with_color", [False, True])
def test_write_ply_round_trips(tmp_path, with_color):
    from aon_amd.mesh import Mesh, read_ply, write_ply

    g = torch.Generator().manual_seed(0)
    verts = torch.randn(50, 3, generator=g)
    faces = torch.randint(0, 50, (70, 3), generator=g, dtype=torch.int64).to(torch.int32)
    colors = torch.randint(0, 256, (50, 3), generator=g).float() / 255.0 if with_color else None
    p = tmp_path / "m.ply"
    write_ply(p, Mesh(verts, faces, colors))
    head = p.read_bytes()[:200]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 50\n")
    back = read_ply(p)
    assert torch.equal(back.verts, verts)
    assert torch.equal(back.faces, faces)
    if with_color:
        assert torch.equal(back.colors, colors)
    else:
        assert back.colors is None
    # the file is exactly header + 12 (+3) bytes per vertex + 13 bytes per face
    data = p.read_bytes()
    body = len(data) - (data.index(b"end_header\n") + len(b"end_header\n"))
    assert body == 50 * (12 + (3 if with_color else 0)) + 70 * 13
