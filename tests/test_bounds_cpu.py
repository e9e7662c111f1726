"""CPU: per-ray near / far.  The numpy restatement (tests/_bounds_ref.py) against the reference's recorded outputs
(G26, value for value with the raw form's NaN positions), the live fraction of the forward fixture, and every refusal of the new entry
points, which happen on the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import _bounds_ref as ref


@pytest.fixture(scope="module")
def g(golden):
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in golden("g26_ray_bounds").items()}


def _eq(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a, b, equal_nan=True), np.nanmax(np.abs(a - b))


@pytest.mark.parametrize("side", [2, 3])
@pytest.mark.parametrize("tag", ["lim", "none"])
def test_limits_equal_the_reference(g, side, tag):
    o, d = g[f"{tag}_rays_o"], g[f"{tag}_rays_d"]
    near, far = ref.ray_limits_box(o, d, side)
    _eq(near, g[f"{tag}_box_near_s{side}"])
    _eq(far, g[f"{tag}_box_far_s{side}"])
    near, far, live = ref.ray_limits(o, d, side)
    _eq(near, g[f"{tag}_near_s{side}"])
    _eq(far, g[f"{tag}_far_s{side}"])
    if tag == "none":
        assert side == 3 or not live.any()     # (no ray of this set is valid for the side-2 box; one hits the side-3 box)
    else:
        assert live.any() and not live.all()
        assert np.isnan(g[f"lim_box_near_s{side}"]).any() or np.isnan(g[f"lim_box_far_s{side}"]).any()   # the reference's NaN case ...
        assert np.isfinite(near).all() and np.isfinite(far).all()                                         # ... is finite after the fix-up


def test_general_box_equals_the_cube(g):
    o, d = g["lim_rays_o"], g["lim_rays_d"]
    for a, b in zip(ref.ray_limits(o, d, 3), ref.ray_limits(o, d, ([-1.5] * 3, [1.5] * 3))):
        assert np.array_equal(a, b, equal_nan=True)


def test_edge_cases_of_the_fixture(g):
    names = g["edge_names"].split(",")
    n0 = int(g["n_frame"])
    near, far, live = ref.ray_limits(g["lim_rays_o"], g["lim_rays_d"], 2)
    at = lambda name: n0 + names.index(name)   # noqa: E731
    assert (near[at("behind")], far[at("behind")], live[at("behind")]) == (0.0, 0.0, 0)      # valid to the reference, nothing to render
    assert live[at("inside")] == 1 and near[at("inside")] == 0.0                             # entry behind the origin, clamped
    assert live[at("axis_px_pos0")] == 1 and live[at("axis_px_neg0")] == 1
    assert live[at("miss_zero_comp")] == 0 and live[at("plain_miss")] == 0 and live[at("on_face_parallel_s2")] == 0
    valid = g["lim_box_far_s2"].reshape(-1) > g["lim_box_near_s2"].reshape(-1)
    assert near[at("plain_miss")] == max(g["lim_box_near_s2"].reshape(-1)[valid].min(), 0.0)  # the fallback of the ray set, clamped
    assert far[at("plain_miss")] == g["lim_box_far_s2"].reshape(-1)[valid].max()


@pytest.mark.parametrize("S", [65, 41])
def test_per_ray_t_equals_the_reference(g, S):
    import aon_amd.synthetic as syn

    pick, pos = g["smp_pick"], g["smp_pos"]
    near, far = g["lim_near_s2"].reshape(-1)[pick], g["lim_far_s2"].reshape(-1)[pick]
    t_rand = syn.seeded_uniform(int(g[f"seed_t{S}"]), len(pick), S).numpy()
    _eq(ref.sample_t(near, far, S), g[f"t_det_{S}"])
    _eq(ref.sample_t(near, far, S, t_rand=t_rand), g[f"t_rnd_{S}"])
    _eq(ref.sample_t(near[pos], far[pos], S, lindisp=True), g[f"t_lin_det_{S}"])
    _eq(ref.sample_t(near[pos], far[pos], S, lindisp=True, t_rand=t_rand[pos]), g[f"t_lin_rnd_{S}"])


def test_forward_fixture_live_fraction(g):
    near, far, live = ref.ray_limits(g["fwd_rays_o"], g["fwd_rays_d"], 2)
    _eq(near, g["fwd_near"])
    _eq(far, g["fwd_far"])
    assert np.array_equal(live, g["fwd_live"])
    assert 0.2 <= live.mean() <= 0.8
    # the reference's own fp32-fp64 distance on these rays, recorded by the generator, lies within the bars of tests/test_hip_smooth.py
    for kind, depth_bar in (("van", 1e-5), ("art", 2e-5)):
        for lvl in ("coarse", "fine"):
            assert g[f"{kind}_dist_{lvl}_rgb"] <= 2e-6 and g[f"{kind}_dist_{lvl}_acc"] <= 2e-6 and g[f"{kind}_dist_{lvl}_depth"] <= depth_bar


def test_refusals_without_gpu():
    from aon_amd import _lib

    lib = _lib.lib
    p = C.c_void_p(0x10000)          # never dereferenced: every call below is refused (or empty) before any launch
    box = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    assert lib.aon_ray_limits_box(None, None, 0, *box, None, None, None) == 0                      # empty problem
    assert lib.aon_ray_limits_box(None, None, 4, *box, None, None, None) == -1 and b"null" in lib.aon_last_error()
    assert lib.aon_ray_limits_box(p, p, -1, *box, p, p, None) == -1
    assert lib.aon_ray_limits_box(p, p, 4, None, box[1], p, p, None) == -1 and b"box" in lib.aon_last_error()
    assert lib.aon_ray_limits_box(p, p, 4, (C.c_float * 3)(float("nan"), 0, 0), box[1], p, p, None) == -1
    need = lib.aon_ray_limits_workspace_bytes(1000)
    assert 2 * 4 * 4 <= need <= 2 * 256 * 4 and lib.aon_ray_limits_workspace_bytes(307200) >= 2 * 4 * 1200
    assert lib.aon_ray_limits(p, p, 1000, *box, p, p, None, None, need, None) == -1 and b"null" in lib.aon_last_error()
    assert lib.aon_ray_limits(p, p, 1000, *box, p, p, None, p, need - 1, None) == -2               # AON_E_WORKSPACE
    assert lib.aon_ray_limits(p, p, 0, *box, p, p, None, p, need, None) == 0
    assert lib.aon_sample_along_rays_bounds(None, None, 4, 65, None, p, 0, None, p, None, None) == -1 and b"null" in lib.aon_last_error()
    assert lib.aon_sample_along_rays_bounds(None, None, 4, 1, p, p, 0, None, p, None, None) == -1 and b"bad size" in lib.aon_last_error()
    assert lib.aon_sample_along_rays_bounds(None, None, 4, 65, p, p, 0, None, p, p, None) == -1   # coords without rays
    assert lib.aon_sample_along_rays_bounds(None, None, 0, 65, p, p, 0, None, p, None, None) == 0

    full = _lib.RayBoundsC(p, p, p)
    no_near, no_far, no_live = _lib.RayBoundsC(None, p, None), _lib.RayBoundsC(p, None, None), _lib.RayBoundsC(p, p, None)
    ws = C.c_void_p(0x10000)
    tail = lambda b, t_rand=None, eps=0.0, R=16: (8, 2.0, 6.0, 1, 2, t_rand, p, 0, p, p, p, p, p, p, ws, 1 << 30, None, None, None, None,   # noqa: E731
                                                  C.c_float(eps), R, None, C.byref(b) if b is not None else None)
    for fn, packs in ((lib.aon_render_fwd_bounds, (p, p)), (lib.aon_art_render_fwd_bounds, (p, p, p, p))):
        rays = (p, p, p)
        for b in (no_near, no_far):
            assert fn(*packs, *rays, *tail(b)) == -1 and b"near_ray / far_ray" in lib.aon_last_error()
        assert fn(*packs, *rays, *tail(full, t_rand=p)) == -1 and b"ray_live" in lib.aon_last_error()       # live together with t_rand
        assert fn(*packs, *rays, *tail(full, eps=1.0)) == -1 and b"eps" in lib.aon_last_error()             # what the _stop call refuses ...
        assert fn(*packs, *rays, *tail(no_live, eps=0.5, R=0)) == -1 and b"round_samples" in lib.aon_last_error()
        assert fn(*packs, *rays, *tail(no_live, t_rand=p, eps=0.5)) == -1 and b"t_rand" in lib.aon_last_error()
        assert fn(*packs, *rays, *tail(None, t_rand=p)) == -1 and b"t_rand" in lib.aon_last_error()         # bounds == NULL: the _stop call
        assert fn(*((None,) * len(packs)), *rays, *tail(no_live)) == -1 and b"null" in lib.aon_last_error()  # ... and what render_fwd_ex refuses
    ttail = lambda b: (8, 2.0, 6.0, 1, 2, None, p, 0, p, p, p, p, p, p, ws, 1 << 40, None, None, C.byref(b))   # noqa: E731
    for fn, packs in ((lib.aon_render_fwd_train_bounds, (p, p)), (lib.aon_art_render_fwd_train_bounds, (p, p, p, p))):
        assert fn(*packs, p, p, p, *ttail(full)) == -1 and b"ray_live is inference only" in lib.aon_last_error()
        assert fn(*packs, p, p, p, *ttail(no_near)) == -1 and b"near_ray / far_ray" in lib.aon_last_error()
        assert fn(*packs, None, p, p, *ttail(no_live)) == -1 and b"null" in lib.aon_last_error()


def test_python_surface_refuses_cpu_tensors():
    import torch

    from aon_amd import ops
    from aon_amd.models.vanilla_nerf import helper

    o = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ray_limits(o, o, 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        helper.get_ray_limits_box(o, o, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        helper.sample_along_rays(o, o, 64, torch.zeros(4, 1), torch.ones(4, 1), False, False)
