"""GPU: the chunk and the deferred slab of the whole-path renders are the largest that the workspace admits, found from the layout itself
(carve / defer_bytes in csrc/aon_capi_render.hip) -- so a workspace of exactly `query(k)` bytes runs chunks of k rays, one byte less runs
chunks of k - 1, and less than `query(1)` is refused.  Outputs do not depend on chunk borders: every such render must have the bits of the
render on the full workspace.  300 rays at 9 / 25 samples per ray, so that chunk borders fall inside a 128-sample pass; both networks, one
and two levels, the plain layout (reached through per-ray bounds, the route that takes `workspace_bytes` from Python), the occupancy layout
and the early-termination layout."""
import ctypes as C
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
N = 300
QUERIES = {"plain": "aon_render_workspace_bytes_ex", "occ": "aon_render_occ_workspace_bytes", "stop": "aon_render_stop_workspace_bytes"}
REFUSALS = {"plain": "render: workspace smaller than aon_render_workspace_bytes(1)",
            "occ": "render: workspace smaller than aon_render_occ_workspace_bytes(1)",
            "stop": "render: workspace smaller than aon_render_stop_workspace_bytes(1)"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from aon_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _switches_back(ops):
    yield
    ops.set_deferred_view(True)
    ops.lib.aon_test_set_deferred_slab(0)


@pytest.fixture(scope="module")
def scene(ops, dev):
    """Rays (a 15 x 20 frame: 300), per-ray near / far, a half-full grid and the packs of both networks -- made once."""
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    rays = {k: v.to(dev) for k, v in syn.make_rays(15, 20, syn.look_at_pose(4.0, 60, 20), syn.focal_from_fovy(15)).items()}
    assert rays["rays_o"].shape[0] == N
    gen = torch.Generator().manual_seed(7)
    grid = ops.occupancy_grid((torch.rand((17, 17, 17), generator=gen) > 0.45).float().to(dev), -1.0, 1.0, 0.5, 0)
    nerf = NeRF().to(dev)
    nerf.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    art = NeRF_AE_Art().to(dev)
    art.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
    codes = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    codes.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    with torch.no_grad():
        lat = {k: v.clone() for k, v in codes({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([3], device=dev)}).items()}
    return types.SimpleNamespace(
        o=rays["rays_o"], d=rays["rays_d"], v=rays["viewdirs"], grid=grid,
        near=(NEAR + 0.3 * syn.seeded_uniform(71, N)).to(dev), far=(FAR - 0.3 * syn.seeded_uniform(72, N)).to(dev),
        opts=ops.RenderOpts(num_coarse_samples=8, num_fine_samples=16),
        vanilla=(nerf.coarse_mlp.packed(fresh=True), nerf.fine_mlp.packed(fresh=True)),
        articulated=(art.coarse_mlp.packed(fresh=True), ops.clone_packed(art.coarse_mlp.prepared(lat)),
                     art.fine_mlp.packed(fresh=True), ops.clone_packed(art.fine_mlp.prepared(lat))))


def _query(ops, sc, form):
    st = sc.opts.c_struct(NEAR, FAR, None)[0]
    fn = getattr(ops.lib, QUERIES[form])
    return lambda k: int(fn(k, C.byref(st)))


def _render(ops, sc, net, form, levels, workspace_bytes=None):
    """-> every output of the call as a flat list: the levels' (rgb, acc, depth), then [occ, stop] the tallies and [stop] the stop map."""
    stem = "render_fwd" if net == "vanilla" else "art_render_fwd"
    kw = dict(num_levels=levels, opts=sc.opts, workspace_bytes=workspace_bytes)
    if form == "plain":
        outs = (getattr(ops, stem)(*getattr(sc, net), sc.o, sc.d, sc.v, sc.near, sc.far, True, **kw),)
    elif form == "occ":
        outs = getattr(ops, stem + "_occ")(*getattr(sc, net), sc.o, sc.d, sc.v, NEAR, FAR, True, sc.grid, **kw)
    else:
        outs = getattr(ops, stem + "_stop")(*getattr(sc, net), sc.o, sc.d, sc.v, NEAR, FAR, True, sc.grid, 1e-2, round_samples=5, **kw)
    torch.cuda.synchronize()
    return [t.clone() for lvl in outs[0] for t in lvl] + [t.clone() for t in outs[1:]]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: output {i} differs"


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("net", ["vanilla", "articulated"])
@pytest.mark.parametrize("form", ["plain", "occ", "stop"])
def test_workspace_of_k_rays(ops, dev, scene, form, net, levels):
    q = _query(ops, scene, form)
    want = _render(ops, scene, net, form, levels)
    assert not any(bool(torch.isnan(t).any()) for t in want if t.is_floating_point())      # (torch.equal below compares values)
    if form != "plain":      # not vacuous: the grid skips some samples of every level run, not all
        for lvl in range(levels):
            assert 0 < int(want[3 * levels][lvl]) < N * scene.opts.S(lvl)
    # 1. a workspace of exactly query(k) bytes: chunks of k rays
    for k in (1, 37, 127, 129):
        _same(_render(ops, scene, net, form, levels, q(k)), want, f"{form}, {net}, {levels} levels, query({k}) bytes")
    # 2. one byte less: still a success, in chunks of k - 1
    for k in (2, 129):
        assert q(k - 1) <= q(k) - 1
        _same(_render(ops, scene, net, form, levels, q(k) - 1), want, f"{form}, {net}, {levels} levels, query({k}) - 1 bytes")
    # 3. less than one ray's: AON_E_WORKSPACE (-2) with the form's message
    with pytest.raises(ops._lib.AonError) as err:
        _render(ops, scene, net, form, levels, q(1) - 1)
    assert "(code -2)" in str(err.value) and REFUSALS[form] in str(err.value)


def test_deferred_slab_fit(ops, dev, scene):
    """Vanilla, the deferred view branch on.  A workspace one 256-byte step short of the slab the size query counts (the hook's 128 rays)
    still holds a smaller slab; exactly the plain workspace holds none, and the single kernel runs.  Both: the single kernel's bits."""
    st = scene.opts.c_struct(NEAR, FAR, None)[0]
    lib = ops.lib
    ops.set_deferred_view(False)
    want = _render(ops, scene, "vanilla", "plain", 2)
    ops.set_deferred_view(True)
    lib.aon_test_set_deferred_slab(0)
    try:
        lib.aon_test_set_deferred_slab(128)
        plain, need = int(lib.aon_render_workspace_bytes_ex(N, C.byref(st))), int(lib.aon_render_deferred_workspace_bytes(N, C.byref(st)))
        assert need - 256 > plain
        _same(_render(ops, scene, "vanilla", "plain", 2, need - 256), want, "a slab below the hook's 128 rays")
        lib.aon_test_set_deferred_slab(0)
        _same(_render(ops, scene, "vanilla", "plain", 2, plain), want, "no room for a slab")
    finally:
        lib.aon_test_set_deferred_slab(0)
