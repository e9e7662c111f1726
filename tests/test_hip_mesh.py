"""GPU: mesh extraction.  The grid kernels' density against the existing fused entries on the same points (bit equality, both stream forms),
against the fp64 oracle, the activations, slabbed calls and the per-point fallback; marching cubes against the numpy reference
(tests/_mc_ref.py) bit for bit, run-to-run identity and edge cases; extract_mesh / extract_meshes end to end."""
import types

import numpy as np
import pytest
import torch

import _mc_ref as R

pytestmark = pytest.mark.gpu

from oracle import nerf_oracle as orc  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


LO, HI = (-1.3, -1.1, -1.2), (1.2, 1.4, 1.0)


def _nerf(dev, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = NeRF(**kw).to(dev)
    if kw:
        sd = syn.make_general_nerf_state_dict(seed=3, **kw)
    else:
        sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)
    model.load_state_dict(sd)
    return model, sd


def _art(dev, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    model = NeRF_AE_Art(**kw).to(dev)
    sd = syn.make_art_state_dict(seed=0, density_scale=30.0, **kw)
    model.load_state_dict(sd)
    return model, sd


def _latents(dev, art_id=3):
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated

    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    with torch.no_grad():
        return lib({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([art_id], device=dev)}, is_test=True)


@pytest.fixture(scope="module")
def fold_state():
    from aon_amd import ops

    was = ops.bottleneck_fold()
    yield
    ops.set_bottleneck_fold(was)


# ---------------------------------------------------------------- density, bit equality with the existing entries
@pytest.mark.parametrize("dims", [(37, 41, 43), (128, 128, 128)])
@pytest.mark.parametrize("fold", [True, False])
def test_vanilla_density_bits_equal_mlp_fwd(dev, dims, fold, fold_state):
    from aon_amd import ops

    ops.set_bottleneck_fold(fold)
    model, _ = _nerf(dev)
    packed = model.fine_mlp.packed(True)
    assert ops.bottleneck_fold() == fold
    raw = ops.density_grid(packed, dims, LO, HI, ops.ACT_NONE)
    assert raw.shape == dims
    pts = ops.grid_points(dims, LO, HI, device=dev)
    n = pts.shape[0]
    ref = ops.mlp_fwd(packed, pts, torch.ones_like(pts), torch.zeros_like(pts) + torch.tensor([0.0, 0.0, 1.0], device=dev),
                      torch.zeros(n, 1, device=dev))[..., 3].reshape(-1)
    assert torch.equal(raw.reshape(-1), ref)
    relu = ops.density_grid(packed, dims, LO, HI, ops.ACT_VANILLA)
    assert torch.equal(relu, torch.relu(raw))


@pytest.mark.parametrize("dims", [(37, 41, 43), (128, 128, 128)])
def test_art_density_bits_equal_art_mlp_fwd_pos(dev, dims):
    from aon_amd import ops

    model, _ = _art(dev)
    lat = _latents(dev)
    mlp = model.fine_mlp
    packed, small = mlp.packed(True), ops.art_prepare(dict(mlp.named_parameters()), lat)
    raw = ops.density_grid(packed, dims, LO, HI, ops.ACT_NONE, small=small)
    pts = ops.grid_points(dims, LO, HI, device=dev)
    venc = ops.pos_enc(torch.zeros_like(pts[:4096]) + torch.tensor([0.0, 0.0, 1.0], device=dev), 0, 4)
    ref = torch.empty(pts.shape[0], device=dev)
    for b in range(0, pts.shape[0], 4096):   # (the view encoding is per ray: one ray per point)
        e = min(pts.shape[0], b + 4096)
        ref[b:e] = ops.art_mlp_fwd_pos(packed, small, pts[b:e, None, :].contiguous(), venc[: e - b].contiguous())[..., 3].reshape(-1)
    assert torch.equal(raw.reshape(-1), ref)
    sp = ops.density_grid(packed, dims, LO, HI, ops.ACT_ARTICULATED, small=small)
    # softplus_f32 (the compositing kernels' function) against fp64 softplus of the same fp32 argument raw - 1: 2.5e-7 relative, plus the
    # rounding of |x| * log2(e) in front of the exp2 that grows with |x| (about |x| * 2^-24 relative; x = raw - 1 reaches -30 here)
    x = (raw - 1).double()
    want = torch.nn.functional.softplus(x)
    rel = ((sp.double() - want).abs() / want).max().item()
    assert ((sp.double() - want).abs() <= want * (2.5e-7 + x.abs() * 2.0 ** -23)).all(), rel
    print(f"softplus_f32 vs fp64: max relative error {rel:.2e}, argument range [{x.min().item():.1f}, {x.max().item():.1f}]")
    # the model entry returns the same
    assert torch.equal(model.density_grid((LO, HI), dims, lat), sp)


@pytest.mark.parametrize("fold", [True, False])
def test_art_density_bits_equal_art_mlp_fwd_pos_both_forms(dev, fold, fold_state):
    """The grid kernel and art_mlp_fwd_pos run the same deformation MLP and trunk code on two chunk maps (the truncated stream; the
    literal or the folded one): on a stream of either form the raw sigma is the same bits.  693 points: 6 passes, a ragged last one."""
    from aon_amd import ops

    ops.set_bottleneck_fold(fold)
    model, _ = _art(dev)
    lat = _latents(dev)
    mlp = model.fine_mlp
    packed, small = mlp.packed(True), ops.art_prepare(dict(mlp.named_parameters()), lat)
    assert ops.bottleneck_fold() == fold
    dims = (7, 9, 11)
    raw = ops.density_grid(packed, dims, LO, HI, ops.ACT_NONE, small=small)
    pts = ops.grid_points(dims, LO, HI, device=dev)
    assert pts.shape[0] == 693
    venc = ops.pos_enc(torch.zeros_like(pts) + torch.tensor([0.0, 0.0, 1.0], device=dev), 0, 4)
    ref = ops.art_mlp_fwd_pos(packed, small, pts[:, None, :].contiguous(), venc.contiguous())[..., 3].reshape(-1)
    assert torch.equal(raw.reshape(-1), ref)


# ---------------------------------------------------------------- density against the fp64 oracle
def _sample(dims, n, seed):
    P = dims[0] * dims[1] * dims[2]
    return torch.randperm(P, generator=torch.Generator().manual_seed(seed))[:n]


def test_density_vs_oracle(dev):
    from aon_amd import ops

    dims = (64, 64, 64)
    idx = _sample(dims, 3000, 0)
    pts = ops.grid_points(dims, LO, HI, device="cpu")[idx].double()
    model, sd = _nerf(dev)
    sd64 = {k: v.double() for k, v in sd.items()}
    raw = ops.density_grid(model.fine_mlp.packed(), dims, LO, HI, ops.ACT_NONE).reshape(-1).cpu()[idx]
    _, sig = orc.nerf_mlp(sd64, "fine_mlp.", orc.pos_enc(pts[:, None, :], 0, 10), orc.pos_enc(torch.zeros_like(pts), 0, 4))
    torch.testing.assert_close(raw.double(), sig.reshape(-1), rtol=5e-5, atol=2e-3)

    amodel, asd = _art(dev)
    lat = _latents(dev)
    asd64 = {k: v.double() for k, v in asd.items()}
    lat64 = {k: v.detach().cpu().double() for k, v in lat.items()}
    small = ops.art_prepare(dict(amodel.coarse_mlp.named_parameters()), lat)
    raw = ops.density_grid(amodel.coarse_mlp.packed(), dims, LO, HI, ops.ACT_NONE, small=small).reshape(-1).cpu()[idx]
    _, sig = orc.art_mlp(asd64, "coarse_mlp.", pts[:, None, :], orc.pos_enc(torch.zeros_like(pts), 0, 4), lat64)
    torch.testing.assert_close(raw.double(), sig.reshape(-1), rtol=5e-5, atol=2e-3)


def test_art_other_degrees_vs_oracle(dev):
    from aon_amd import ops

    dims = (33, 35, 31)
    idx = _sample(dims, 2000, 1)
    pts = ops.grid_points(dims, LO, HI, device="cpu")[idx].double()
    model, sd = _art(dev, min_deg_point=1, max_deg_point=7, deg_view=2)
    lat = _latents(dev, 5)
    sd64 = {k: v.double() for k, v in sd.items()}
    lat64 = {k: v.detach().cpu().double() for k, v in lat.items()}
    sp = model.density_grid((LO, HI), dims, lat).reshape(-1).cpu()[idx]
    _, sig = orc.art_mlp(sd64, "fine_mlp.", pts[:, None, :], orc.pos_enc(torch.zeros_like(pts), 0, 2), lat64, min_deg_point=1, max_deg_point=7)
    torch.testing.assert_close(sp.double(), torch.nn.functional.softplus(sig.reshape(-1) - 1), rtol=5e-5, atol=2e-3)


def test_slabbed_calls_give_the_same_bits(dev):
    from aon_amd import ops

    dims = (37, 41, 43)
    P = 37 * 41 * 43
    model, _ = _nerf(dev)
    packed = model.fine_mlp.packed()
    whole = ops.density_grid(packed, dims, LO, HI, ops.ACT_VANILLA).reshape(-1)
    out = torch.full((P,), float("nan"), device=dev)
    cuts = [0, 1, 130, 131, 4099, 30001, 50000, P]   # ragged and unaligned slab edges
    for b, e in zip(cuts[:-1], cuts[1:]):
        ops.density_grid(packed, dims, LO, HI, ops.ACT_VANILLA, g_begin=b, g_end=e, out=out[b:e])
    assert torch.equal(out, whole)
    amodel, _ = _art(dev)
    lat = _latents(dev)
    mlp = amodel.fine_mlp
    small = mlp.prepared(lat)
    whole = ops.density_grid(mlp.packed(), dims, LO, HI, ops.ACT_ARTICULATED, small=small).reshape(-1)
    part = ops.density_grid(mlp.packed(), dims, LO, HI, ops.ACT_ARTICULATED, small=small, g_begin=777, g_end=40000)
    assert torch.equal(part, whole[777:40000])


def test_non_default_vanilla_geometry_takes_the_fallback(dev, monkeypatch):
    from aon_amd import ops

    geom = dict(min_deg_point=0, max_deg_point=6, deg_view=2)
    model, sd = _nerf(dev, **geom)
    called = []
    monkeypatch.setattr(ops.lib, "aon_density_grid", lambda *a: called.append(a) or -1)
    dims = (19, 23, 21)
    grid = model.density_grid((LO, HI), dims, "coarse", chunk=1000)   # several chunks
    assert not called, "a non-default vanilla geometry must not reach the grid kernel"
    assert grid.shape == dims
    pts = ops.grid_points(dims, LO, HI, device="cpu").double()
    sd64 = {k: v.double() for k, v in sd.items()}
    _, sig = orc.nerf_mlp(sd64, "coarse_mlp.", orc.pos_enc(pts[:, None, :], 0, 6), orc.pos_enc(torch.zeros_like(pts), 0, 2))
    torch.testing.assert_close(grid.reshape(-1).cpu().double(), torch.relu(sig.reshape(-1)), rtol=5e-5, atol=2e-3)


# ---------------------------------------------------------------- marching cubes against the numpy reference
def _mc_check(dev, v, level, lo, hi):
    from aon_amd import ops

    verts, faces = ops.marching_cubes(torch.from_numpy(v).to(dev), level, lo, hi)
    lo32, step = ops.grid_step(v.shape, lo, hi)
    rv, rf = R.marching_cubes(v, level, lo32.numpy(), step.numpy())
    assert faces.shape == rf.shape and verts.shape == rv.shape
    assert np.array_equal(faces.cpu().numpy(), rf)
    assert np.array_equal(verts.cpu().numpy().view(np.uint32), rv.view(np.uint32))   # bit equality (NaN-safe)
    return verts, faces


def _analytic(N, f):
    c = R.grid_coords(N, -1.0, R.step_of(-1.0, 1.0, N)).astype(np.float64)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    return f(X, Y, Z).astype(np.float32)


@pytest.mark.parametrize("name,N", [("sphere", 64), ("torus", 128), ("offcentre", 77)])
def test_marching_cubes_equals_reference_on_analytic_fields(dev, name, N):
    f = {"sphere": lambda X, Y, Z: 0.7 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2),
         "torus": lambda X, Y, Z: 0.25 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2),
         "offcentre": lambda X, Y, Z: 0.4 - np.sqrt((X - 0.21) ** 2 + (Y + 0.13) ** 2 + (Z - 0.3) ** 2)}[name]
    v = _analytic(N, f)
    verts, faces = _mc_check(dev, v, 0.0, -1.0, 1.0)
    _, cnt = R.edge_use_counts(faces.cpu().numpy())
    assert (cnt == 2).all() and R.signed_volume(verts.cpu().numpy(), faces.cpu().numpy()) > 0


def test_marching_cubes_random_field_all_cases_and_repeatable(dev):
    rng = np.random.default_rng(7)
    v = rng.standard_normal((45, 38, 51)).astype(np.float32)
    v[rng.random(v.shape) < 0.01] = np.nan
    ins = (v > 0.1).astype(np.int64)
    case = np.zeros((44, 37, 50), dtype=np.int64)
    for c, (di, dj, dk) in enumerate(R.CORNERS):
        case |= ins[di:di + 44, dj:dj + 37, dk:dk + 50] << c
    assert np.unique(case).size == 256   # every case of the table is exercised
    a = _mc_check(dev, v, 0.1, (-2.0, 0.5, -1.0), (3.0, 1.5, 4.0))
    from aon_amd import ops

    b = ops.marching_cubes(torch.from_numpy(v).to(dev), 0.1, (-2.0, 0.5, -1.0), (3.0, 1.5, 4.0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_marching_cubes_large_grid_equals_reference(dev):
    rng = np.random.default_rng(3)
    c = np.linspace(-1, 1, 160, dtype=np.float32)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    v = (np.sin(5 * X) * np.cos(4 * Y) + 0.8 * np.sin(3 * Z + 1) + 0.05 * rng.standard_normal(X.shape)).astype(np.float32)
    _mc_check(dev, v, 0.2, -1.0, 1.0)


def test_marching_cubes_edge_cases(dev):
    from aon_amd import ops

    out = np.full((9, 7, 8), -1.0, dtype=np.float32)   # all outside
    verts, faces = _mc_check(dev, out, 0.0, 0.0, 1.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    verts, faces = _mc_check(dev, -out, 0.0, 0.0, 1.0)   # all inside
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    for case in (1, 0x81, 0x7e, 0x3c, 0xfe):   # 2 x 2 x 2: one cell
        v = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)
        g = np.zeros((2, 2, 2), dtype=np.float32)
        for c, (di, dj, dk) in enumerate(R.CORNERS):
            g[di, dj, dk] = v[c]
        _, faces = _mc_check(dev, g, 0.0, -1.0, 1.0)
        assert faces.shape[0] == len(R.TRI_TABLE[case]) // 3
    q = np.round(np.random.default_rng(1).random((12, 13, 11)) * 4).astype(np.float32)   # level equal to grid values: value == level is outside
    _mc_check(dev, q, 2.0, -1.0, 1.0)
    from aon_amd._lib import AonError

    with pytest.raises(AonError, match="2, 2"):
        ops.marching_cubes(torch.zeros((1, 4, 4), device=dev), 0.0, 0.0, 1.0)


# ---------------------------------------------------------------- end to end
def test_extract_mesh_vanilla_and_articulated(dev, tmp_path):
    from aon_amd import ops
    from aon_amd.mesh import extract_mesh, read_ply, write_ply

    model, _ = _nerf(dev)
    bounds = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    mesh = extract_mesh(model, bounds, 48, threshold=5.0, color=True)
    grid = model.density_grid(bounds, 48)
    lo32, step = ops.grid_step(grid.shape, *bounds)
    rv, rf = R.marching_cubes(grid.cpu().numpy(), 5.0, lo32.numpy(), step.numpy())
    assert len(rf) > 0
    assert np.array_equal(mesh.faces.cpu().numpy(), rf) and np.array_equal(mesh.verts.cpu().numpy(), rv)
    assert mesh.colors.shape == mesh.verts.shape and (mesh.colors >= 0).all() and (mesh.colors <= 1).all()
    write_ply(tmp_path / "m.ply", mesh)
    assert torch.equal(read_ply(tmp_path / "m.ply").faces, mesh.faces.cpu())

    amodel, _ = _art(dev)
    lat = _latents(dev)
    agrid = amodel.density_grid(bounds, 40, lat)
    level = float(torch.quantile(agrid.reshape(-1), 0.9))   # a level the seeded field crosses
    amesh = extract_mesh(amodel, bounds, 40, threshold=level, latents=lat, color=True)
    rv, rf = R.marching_cubes(agrid.cpu().numpy(), level, lo32.numpy(), ops.grid_step(agrid.shape, *bounds)[1].numpy())
    assert len(rf) > 0
    assert np.array_equal(amesh.faces.cpu().numpy(), rf) and np.array_equal(amesh.verts.cpu().numpy(), rv)
    assert amesh.colors.shape == amesh.verts.shape


def test_extract_meshes_one_per_articulation_state(dev):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(dict(N_max_objs=2))
    lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    lit.model.to(dev)
    lit.code_library.to(dev)
    with torch.no_grad():
        lat = lit.code_library({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([4], device=dev)}, is_test=True)
        level = float(torch.quantile(lit.model.density_grid((-1.5, 1.5), 24, lat).reshape(-1), 0.9))
    meshes = lit.extract_meshes(instance_id=1, resolution=24, bounds=(-1.5, 1.5), threshold=level)
    assert len(meshes) == 19
    assert all(m.faces.shape[1] == 3 and m.verts.shape[1] == 3 for m in meshes)
    # row 4 of the table is the code the level was taken from: its mesh is that grid's
    from aon_amd import ops

    rv, rf = R.marching_cubes(lit.model.density_grid((-1.5, 1.5), 24, lat).cpu().numpy(), level, *[t.numpy() for t in ops.grid_step((24,) * 3, -1.5, 1.5)])
    assert len(rf) > 0 and np.array_equal(meshes[4].faces.cpu().numpy(), rf) and np.array_equal(meshes[4].verts.cpu().numpy(), rv)
