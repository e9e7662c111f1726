"""GPU: per-ray near / far from a ray-box intersection.  The limits and the per-ray sampler against the reference's
recorded outputs (G26) and the numpy restatement (tests/_bounds_ref.py), bit for bit; constant tensors against the scalar calls (forward and
every gradient); the full forward against the reference within the bars of tests/test_hip_smooth.py; the whole-path call against the stage
entry points composed by hand (one chunk and several); ray_live against a yardstick with the dead rays' records overwritten; the Lit
modules at two chunk sizes; one stream-ordering probe."""
import types

import numpy as np
import pytest
import torch

import _bounds_ref as ref

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from aon_amd import ops as _ops

    was = _ops.bottleneck_fold()
    yield _ops
    _ops.set_bottleneck_fold(was)


@pytest.fixture(scope="module")
def g(golden, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in golden("g26_ray_bounds").items()}


def _nerf(dev, smooth=False, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = NeRF(**kw).to(dev)
    model.load_state_dict(syn.make_smooth_nerf_state_dict() if smooth else syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    return model


def _art(dev, smooth=False, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    model = NeRF_AE_Art(**kw).to(dev)
    model.load_state_dict(syn.make_art_state_dict(seed=5, density_scale=2.0) if smooth else syn.make_art_state_dict(seed=0, density_scale=30.0))
    return model


def _latents(dev):
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated

    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    with torch.no_grad():
        return {k: v.clone() for k, v in lib({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([3], device=dev)}).items()}


def _frame(dev, H=15, W=20):
    import aon_amd.synthetic as syn

    return {k: v.to(dev) for k, v in syn.make_rays(H, W, syn.look_at_pose(4.0, 60, 20), syn.focal_from_fovy(H)).items()}


def _same(a, b):
    for la, lb in zip(a, b):
        for x, y in zip(la, lb):
            assert torch.equal(x, y), (x - y).abs().max()


def _eq_nan(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


# ---------------------------------------------------------------- 1. the limits: the reference's bits, the numpy restatement's bits
@pytest.mark.parametrize("side", [2, 3])
@pytest.mark.parametrize("tag", ["lim", "none"])
def test_ray_limits_equal_fixture_and_reference_copy(ops, g, side, tag):
    o, d = g[f"{tag}_rays_o"], g[f"{tag}_rays_d"]
    near, far = ops.ray_limits_box(o, d, side)
    assert near.shape == far.shape == (o.shape[0], 1)
    _eq_nan(near, g[f"{tag}_box_near_s{side}"])
    _eq_nan(far, g[f"{tag}_box_far_s{side}"])
    rn, rf = ref.ray_limits_box(o.cpu().numpy(), d.cpu().numpy(), side)
    _eq_nan(near.cpu(), torch.from_numpy(rn))
    _eq_nan(far.cpu(), torch.from_numpy(rf))
    near, far, live = ops.ray_limits(o, d, side)
    _eq_nan(near, g[f"{tag}_near_s{side}"])
    _eq_nan(far, g[f"{tag}_far_s{side}"])
    rn, rf, rl = ref.ray_limits(o.cpu().numpy(), d.cpu().numpy(), side)
    _eq_nan(near.cpu(), torch.from_numpy(rn))
    _eq_nan(far.cpu(), torch.from_numpy(rf))
    assert live.dtype == torch.uint8 and torch.equal(live.cpu(), torch.from_numpy(rl))
    if tag == "lim":   # a general box, the helper's shapes, and N = 1
        from aon_amd.models.vanilla_nerf import helper

        half = side / 2
        for a, b in zip(ops.ray_limits(o, d, ([-half] * 3, [half] * 3)), (near, far, live)):
            _eq_nan(a.float(), b.float())
        hn, hf = helper.get_ray_limits(o.view(-1, 2, 3), d.view(-1, 2, 3), box_side_length=side)
        assert hn.shape == (o.shape[0] // 2, 2, 1) and torch.equal(hn.reshape(-1, 1), near) and torch.equal(hf.reshape(-1, 1), far)
        for i in (0, o.shape[0] - 6):   # a hit, and the ray behind which the box lies
            n1, f1, l1 = ops.ray_limits(o[i: i + 1], d[i: i + 1], side)
            r1 = ref.ray_limits(o[i: i + 1].cpu().numpy(), d[i: i + 1].cpu().numpy(), side)
            _eq_nan(n1.cpu(), torch.from_numpy(r1[0]))
            _eq_nan(f1.cpu(), torch.from_numpy(r1[1]))
            assert int(l1) == int(r1[2][0])


def test_ray_limits_many_blocks(ops, dev):
    """More rays than one block of partials (and no multiple of the block): the reduction over the per-block min / max."""
    import aon_amd.synthetic as syn

    r = syn.random_rays(70001, seed=3)
    o, d = r["rays_o"].to(dev), r["rays_d"].to(dev)
    o[-1], d[-1] = torch.tensor([0.0, 0.0, 9.0], device=dev), torch.tensor([0.0, 0.0, -1.0], device=dev)   # the largest far sits in the last block
    near, far, live = ops.ray_limits(o, d, 1.0)
    rn, rf, rl = ref.ray_limits(o.cpu().numpy(), d.cpu().numpy(), 1.0)
    _eq_nan(near.cpu(), torch.from_numpy(rn))
    _eq_nan(far.cpu(), torch.from_numpy(rf))
    assert torch.equal(live.cpu(), torch.from_numpy(rl)) and 0 < int(live.sum()) < live.numel()


# ---------------------------------------------------------------- 2. the per-ray sampler
@pytest.mark.parametrize("S", [65, 41])
def test_per_ray_sampler_equals_fixture(ops, g, dev, S):
    import aon_amd.synthetic as syn

    pick, pos = g["smp_pick"], g["smp_pos"]
    o, d = g["lim_rays_o"][pick], g["lim_rays_d"][pick]
    near, far = g["lim_near_s2"][pick], g["lim_far_s2"][pick]              # (N, 1)
    t_rand = syn.seeded_uniform(int(g[f"seed_t{S}"]), len(pick), S).to(dev)
    for want_coords in (False, True):                                      # the 16-byte-store kernel / the per-element kernel
        t, c = ops.sample_along_rays(o, d, S - 1, near, far, want_coords=want_coords)
        assert torch.equal(t, g[f"t_det_{S}"])
        if want_coords and S == 65:
            assert torch.equal(c[:32], g["coords_det_65"])
        t, _ = ops.sample_along_rays(o, d, S - 1, near[:, 0], far[:, 0], t_rand, want_coords=want_coords)   # (N,) as well as (N, 1)
        assert torch.equal(t, g[f"t_rnd_{S}"])
        t, _ = ops.sample_along_rays(o[pos], d[pos], S - 1, near[pos], far[pos], want_coords=want_coords, lindisp=True)
        assert torch.equal(t, g[f"t_lin_det_{S}"])
        t, _ = ops.sample_along_rays(o[pos], d[pos], S - 1, near[pos], far[pos], t_rand[pos].contiguous(), want_coords=want_coords, lindisp=True)
        assert torch.equal(t, g[f"t_lin_rnd_{S}"])
    # 37 rays x 65: n * S is no multiple of 4, a thread's four elements straddle rays
    t, _ = ops.sample_along_rays(o[:37], d[:37], S - 1, near[:37], far[:37], t_rand[:37].contiguous(), want_coords=False)
    assert torch.equal(t, g[f"t_rnd_{S}"][:37])
    want = ref.sample_t(near[:37].cpu().numpy(), far[:37].cpu().numpy(), S, t_rand=t_rand[:37].cpu().numpy())
    assert torch.equal(t.cpu(), torch.from_numpy(want))


def test_per_ray_sampler_unaligned_output(ops, g, dev):
    """A t_vals pointer that is not 16-byte aligned takes the per-element kernel through the stage entry point: the same bits."""
    import ctypes as C

    from aon_amd._lib import check, lib

    pick = g["smp_pick"][:37]
    near, far = g["lim_near_s2"][pick].reshape(-1).contiguous(), g["lim_far_s2"][pick].reshape(-1).contiguous()
    buf = torch.full((37 * 65 + 8,), -7.0, device=dev)
    out = buf[1: 1 + 37 * 65]
    assert out.data_ptr() % 16 == 4
    with torch.cuda.device(dev):
        check(lib.aon_sample_along_rays_bounds(None, None, 37, 65, C.c_void_p(near.data_ptr()), C.c_void_p(far.data_ptr()), 0, None,
                                               C.c_void_p(out.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(out.view(37, 65), g["t_det_65"][:37])
    assert buf[0] == -7.0 and bool((buf[1 + 37 * 65:] == -7.0).all())     # nothing written outside the view


# ---------------------------------------------------------------- 3. constant tensors are the scalar call: forward and every gradient
@pytest.mark.parametrize("sizes", [(64, 128), (40, 72)], ids=["65_193", "41_113"])
@pytest.mark.parametrize("net", ["vanilla", "articulated"])
def test_constant_tensors_equal_scalars(ops, dev, fold_form, net, sizes):
    import aon_amd.synthetic as syn

    n = 130
    r = syn.random_rays(n, seed=11)
    rays = {k: v.to(dev) for k, v in r.items()}
    kw = dict(num_coarse_samples=sizes[0], num_fine_samples=sizes[1])
    model = _nerf(dev, **kw) if net == "vanilla" else _art(dev, **kw)
    lat = None if net == "vanilla" else _latents(dev)
    t_rand, u = syn.seeded_uniform(31, n, sizes[0] + 1).to(dev), syn.seeded_uniform(32, n, sizes[1]).to(dev)
    target = syn.seeded_uniform(33, n, 3).to(dev)
    tn, tf = torch.full((n, 1), NEAR, device=dev), torch.full((n,), FAR, device=dev)

    def call(near, far, randomized, latents):
        extra = () if net == "vanilla" else (latents,)
        return model(rays, randomized, True, near, far, *extra, t_rand=t_rand if randomized else None, u=u if randomized else None)

    with torch.no_grad():
        _same(call(tn, tf, False, lat), call(NEAR, FAR, False, lat))
        _same(call(tn, tf, True, lat), call(NEAR, FAR, True, lat))

    def grads(near, far):
        model.zero_grad(set_to_none=True)
        latents = None if lat is None else {k: v.clone().requires_grad_(True) for k, v in lat.items()}
        out = call(near, far, True, latents)
        loss = ((out[0][0] - target) ** 2).mean() + ((out[1][0] - target) ** 2).mean()
        loss.backward()
        gs = {k: p.grad.clone() for k, p in model.named_parameters()}
        if latents is not None:
            gs.update({"lat_" + k: v.grad.clone() for k, v in latents.items()})
        return loss.detach(), gs

    l_s, g_s = grads(NEAR, FAR)
    l_t, g_t = grads(tn, tf)
    assert torch.equal(l_s, l_t) and g_s.keys() == g_t.keys() and len(g_s) >= 48
    for k in g_s:
        assert torch.equal(g_s[k], g_t[k]), k
        assert bool(torch.isfinite(g_s[k]).all())


# ---------------------------------------------------------------- 4. the full forward against the reference
@pytest.mark.parametrize("net", ["vanilla", "articulated"])
def test_forward_with_ray_limits_matches_reference(ops, dev, g, net):
    from aon_amd.models.vanilla_nerf import helper

    rays = {k: g["fwd_" + k] for k in ("rays_o", "rays_d", "viewdirs")}
    near, far = helper.get_ray_limits(rays["rays_o"], rays["rays_d"], box_side_length=2)
    assert torch.equal(near, g["fwd_near"]) and torch.equal(far, g["fwd_far"])
    with torch.no_grad():
        if net == "vanilla":
            out, kind, depth_bar = _nerf(dev, smooth=True)(rays, False, True, near, far), "van", 1e-5
        else:
            lat = {k: g["fwd_lat_" + k] for k in ("density", "color", "articulation")}
            out, kind, depth_bar = _art(dev, smooth=True)(rays, False, True, near, far, lat), "art", 2e-5
    for lvl, name in ((0, "coarse"), (1, "fine")):
        for i, (q, bar) in enumerate((("rgb", 2e-6), ("acc", 2e-6), ("depth", depth_bar))):
            err = (out[lvl][i] - g[f"{kind}_{name}_{q}"]).abs().max().item()
            print(f"{net} {name} {q}: max |hip - reference fp32| = {err:.3e} (bar {bar:.0e})")
            assert err <= bar, (name, q, err)


# ---------------------------------------------------------------- 5. render_fwd with bounds == the stage entry points composed by hand
@pytest.mark.parametrize("net", ["vanilla", "articulated"])
def test_whole_path_equals_composed_stages(ops, dev, net):
    rays = _frame(dev)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    near, far, live = ops.ray_limits(o, d, 2.0)
    if net == "vanilla":
        m = _nerf(dev)
        pc, pf = m.coarse_mlp.packed(fresh=True), m.fine_mlp.packed(fresh=True)
        mlp = lambda lvl, t: ops.mlp_fwd(pc if lvl == 0 else pf, o, d, v, t)   # noqa: E731
        whole = lambda **kw: ops.render_fwd(pc, pf, o, d, v, near, far, True, **kw)   # noqa: E731
        act = ops.ACT_VANILLA
    else:
        m, lat = _art(dev), _latents(dev)
        pc, pf = m.coarse_mlp.packed(fresh=True), m.fine_mlp.packed(fresh=True)
        sc, sf = ops.clone_packed(m.coarse_mlp.prepared(lat)), ops.clone_packed(m.fine_mlp.prepared(lat))
        mlp = lambda lvl, t: ops.art_mlp_fwd(pc if lvl == 0 else pf, sc if lvl == 0 else sf, o, d, v, t)   # noqa: E731
        whole = lambda **kw: ops.art_render_fwd(pc, sc, pf, sf, o, d, v, near, far, True, **kw)   # noqa: E731
        act = ops.ACT_ARTICULATED
    t_c, _ = ops.sample_along_rays(o, d, 64, near, far, want_coords=False)
    comp_c, acc_c, w_c, depth_c = ops.composite_raw(mlp(0, t_c), t_c, d, True, act, want_weights=True)
    t_f = ops.sample_pdf_t(t_c, w_c)
    comp_f, acc_f, _, depth_f = ops.composite_raw(mlp(1, t_f), t_f, d, True, act, want_weights=False)
    want = [(comp_c, acc_c, depth_c), (comp_f, acc_f, depth_f)]
    _same(whole(), want)
    # a workspace that holds about 128 rays: three chunks, each with its own offset into near / far
    small = int(ops.lib.aon_render_workspace_bytes(128))
    _same(whole(workspace_bytes=small), want)
    # the same with the ray mask, which takes the compaction path: one chunk against three (the mask offset by the chunk's first ray)
    masked = whole(ray_live=live)
    for a, b in zip(masked, want):
        for x, y in zip(a, b):
            assert torch.equal(x[live == 1], y[live == 1])
    _same(whole(ray_live=live, workspace_bytes=int(ops.lib.aon_render_stop_workspace_bytes(128, None))), masked)


# ---------------------------------------------------------------- 6. ray_live
def _random_grid(ops, dev, seed=7):
    gen = torch.Generator().manual_seed(seed)
    dens = (torch.rand((17, 17, 17), generator=gen) > 0.45).float().to(dev)
    return ops.occupancy_grid(dens, -1.0, 1.0, 0.5, 0)


@pytest.mark.parametrize("eps", [0.0, 1e-2])
@pytest.mark.parametrize("with_grid", [False, True], ids=["nogrid", "grid"])
def test_ray_live_against_overwritten_records(ops, dev, with_grid, eps):
    """The yardstick: the same call without ray_live gives t (through the stage sampler) and the records; the dead rays' records are
    overwritten by the sentinel before compositing, by hand from the stage entry points (as test_hip_occupancy.py); with eps > 0 the samples
    behind a ray's stop are overwritten as well.  Outputs, `occupied` and the stop map, one chunk and three."""
    import _occ_ref as occ_ref

    rays = _frame(dev)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    near, far, live = ops.ray_limits(o, d, 2.0)
    assert 0.2 <= live.float().mean().item() <= 0.8
    m = _nerf(dev)
    pc, pf = m.coarse_mlp.packed(fresh=True), m.fine_mlp.packed(fresh=True)
    grid = _random_grid(ops, dev) if with_grid else None
    dead = live == 0
    kw = dict(round_samples=16)
    outs, occupied, stop = ops.render_fwd_stop(pc, pf, o, d, v, near, far, True, grid, eps, ray_live=live, **kw)
    for lvl in outs:   # dead rays: exactly the background
        assert bool((lvl[0][dead] == 1.0).all()) and bool((lvl[1][dead] == 0.0).all()) and bool((lvl[2][dead] == 0.0).all())
    ones, occ1, _ = ops.render_fwd_stop(pc, pf, o, d, v, near, far, True, grid, eps, ray_live=torch.ones_like(live), **kw)
    plain, occ0, _ = ops.render_fwd_stop(pc, pf, o, d, v, near, far, True, grid, eps, **kw)
    _same(ones, plain)                                   # live all ones: the call without it
    assert torch.equal(occ1, occ0)

    def mask(t):
        if grid is None:
            return torch.ones_like(t, dtype=torch.bool)
        occ = grid.occupied().cpu().numpy()
        mk = occ_ref.lookup(occ, grid.lo.numpy(), grid.step.numpy(), occ_ref.cast(o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()))
        return torch.from_numpy(mk).to(dev)

    # the stop map: a live ray stops where it stops without the mask (tests/test_hip_stop.py holds that map to its reference); a dead ray
    # never stops -- its optical depth stays 0 -- so its entry is S
    plain_stop = ops.render_fwd_stop(pc, pf, o, d, v, near, far, True, grid, eps, **kw)[2]
    assert torch.equal(stop[~dead], plain_stop[~dead])
    assert bool((stop[dead, 0] == 65).all()) and bool((stop[dead, 1] == 193).all())
    if eps == 0.0:
        assert bool((stop[:, 0] == 65).all()) and bool((stop[:, 1] == 193).all())
    else:
        assert bool((stop[~dead, 1] < 193).any())        # (the case is not vacuous: rays do stop)

    # the yardstick, for every combination: the stage entry points, with the record of every sample that is in an empty cell, behind its
    # ray's stop, or on a dead ray overwritten by the sentinel before compositing
    def kept(t, level):
        idx = torch.arange(t.shape[1], device=dev)[None, :]
        return mask(t) & (idx < stop[:, level: level + 1]) & ~dead[:, None]

    sentinel = torch.tensor([0.0, 0.0, 0.0, float("-inf")], device=dev)
    t_c, _ = ops.sample_along_rays(o, d, 64, near, far, want_coords=False)
    raw = ops.mlp_fwd(pc, o, d, v, t_c)
    m0 = kept(t_c, 0)
    raw[~m0] = sentinel
    comp_c, acc_c, _, depth_c, t_f = ops.composite_pdf(raw, t_c, d, True, ops.ACT_VANILLA)
    raw_f = ops.mlp_fwd(pf, o, d, v, t_f)
    m1 = kept(t_f, 1)
    raw_f[~m1] = sentinel
    comp_f, acc_f, _, depth_f = ops.composite_raw(raw_f, t_f, d, True, ops.ACT_VANILLA, want_weights=False)
    _same(outs, [(comp_c, acc_c, depth_c), (comp_f, acc_f, depth_f)])
    assert occupied.tolist() == [int(m0.sum()), int(m1.sum())]      # the samples run: the yardstick's mask sums
    for a, b in zip(outs, plain):                        # rays are independent: a live ray's bits do not depend on the mask
        for x, y in zip(a, b):
            assert torch.equal(x[~dead], y[~dead])
    # the same call in chunks of about 128 rays (a forced small workspace): near / far / live offset by the chunk's first ray
    small = int(ops.lib.aon_render_stop_workspace_bytes(128, None))
    o3, c3, s3 = ops.render_fwd_stop(pc, pf, o, d, v, near, far, True, grid, eps, ray_live=live, workspace_bytes=small, **kw)
    _same(o3, outs)
    assert torch.equal(c3, occupied) and torch.equal(s3, stop)
    # the occupancy entry point takes the mask too
    if grid is not None and eps == 0.0:
        o2, c2 = ops.render_fwd_occ(pc, pf, o, d, v, near, far, True, grid, ray_live=live)
        _same(o2, outs)
        assert torch.equal(c2, occupied)


def test_ray_live_articulated_and_plain_entry(ops, dev):
    rays = _frame(dev)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    near, far, live = ops.ray_limits(o, d, 2.0)
    dead = live == 0
    m, lat = _art(dev), _latents(dev)
    pc, pf = m.coarse_mlp.packed(fresh=True), m.fine_mlp.packed(fresh=True)
    sc, sf = ops.clone_packed(m.coarse_mlp.prepared(lat)), ops.clone_packed(m.fine_mlp.prepared(lat))
    masked = ops.art_render_fwd(pc, sc, pf, sf, o, d, v, near, far, False, ray_live=live)
    plain = ops.art_render_fwd(pc, sc, pf, sf, o, d, v, near, far, False)
    for a, b in zip(masked, plain):
        for x, y in zip(a, b):
            assert torch.equal(x[~dead], y[~dead]) and bool((x[dead] == 0.0).all())      # black background: rgb = acc = depth = 0
    with torch.no_grad():
        _same(m(rays, False, False, near, far, lat, ray_live=live), masked)
    with pytest.raises(ValueError, match="inference only"):
        m(rays, True, False, near, far, lat, ray_live=live)


# ---------------------------------------------------------------- 7. the Lit modules
def _image_batch(dev, H=15, W=20):
    import aon_amd.synthetic as syn

    b = _frame(dev, H, W)
    b["target"] = syn.seeded_uniform(41, H * W, 3).to(dev)
    b["instance_mask"] = torch.ones(H * W, dtype=torch.bool, device=dev)
    return b


def test_lit_modules_chunk_size_does_not_change_the_picture(ops, dev):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    batch = _image_batch(dev)
    pics = []
    for chunk in (3840, 97):
        lit = LitNeRF(hparams=dict(chunk=chunk), ray_box=2.0).to(dev)
        lit.model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
        ret = lit.render_rays(dict(batch), 0)
        pics.append((ret["comp_rgb"], ret["acc"], ret["depth"], lit.render_rays_test(dict(batch), 0)["rgb"]))
    for a, b in zip(*pics):
        assert torch.equal(a, b)
    assert torch.equal(pics[0][0], pics[0][3])
    dead = ops.ray_limits(batch["rays_o"], batch["rays_d"], 2.0)[2] == 0
    assert bool(dead.any()) and bool((pics[0][0][dead] == 1.0).all()) and bool((pics[0][1][dead] == 0.0).all())
    # training_step on per-ray limits: finite loss, gradients everywhere
    lit.train()
    tb = {k: v[None] for k, v in batch.items() if k != "instance_mask"}
    loss = lit.training_step(tb, 0)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in lit.model.parameters())
    # ray_box=None keeps the scalar path (tests/test_harness.py holds its logged values)
    assert LitNeRF(hparams=dict(chunk=97)).ray_box is None


def test_lit_autodecoder_chunk_size_does_not_change_the_picture(ops, dev):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    batch = _image_batch(dev)
    batch.update(instance_id=torch.tensor([0], device=dev), articulation_id=torch.tensor([3], device=dev))
    pics = []
    for chunk in (3840, 97):
        lit = LitNeRF_AutoDecoder(hparams=dict(chunk=chunk), ray_box=(-1.0, 1.0)).to(dev)
        lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
        lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=1))
        with torch.no_grad():
            pics.append(lit.render_rays(dict(batch), lit.code_library(batch))["comp_rgb"])
    assert torch.equal(pics[0], pics[1])
    lit.train()
    tb = {k: (v if k in ("instance_id", "articulation_id") else v[None]) for k, v in batch.items() if k != "instance_mask"}
    loss = lit.training_step(tb, 0)
    loss.backward()
    assert bool(torch.isfinite(loss))


# ---------------------------------------------------------------- 8. streams
def test_bounds_render_is_ordered_on_a_side_stream(ops, dev):
    """render_fwd with bounds + ray_live on a non-default stream whose inputs are written on that stream right before the call, behind a
    long-running kernel: every launch of the call (limits, sampler, mark / scan / emit, MLP, compositing) must be on that stream."""
    rays = _frame(dev)
    m = _nerf(dev)
    pc, pf = m.coarse_mlp.packed(fresh=True), m.fine_mlp.packed(fresh=True)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    near, far, live = ops.ray_limits(o, d, 2.0)
    serial = ops.render_fwd(pc, pf, o, d, v, near, far, True, ray_live=live)
    torch.cuda.synchronize(dev)
    o2, d2, v2 = (torch.full_like(x, float("nan")) for x in (o, d, v))
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for _ in range(6):
            big = big @ big * 1e-3          # keeps the stream busy while the host races ahead
        o2.copy_(o); d2.copy_(d); v2.copy_(v)
        n2, f2, l2 = ops.ray_limits(o2, d2, 2.0)
        out = ops.render_fwd(pc, pf, o2, d2, v2, n2, f2, True, ray_live=l2)
    side.synchronize()
    assert torch.equal(l2, live) and torch.equal(n2, near)
    _same(out, serial)


# ---------------------------------------------------------------- 9. occupancy.render_image(ray_bounds=True)
def test_render_image_with_ray_bounds(ops, dev):
    import aon_amd.synthetic as syn
    from aon_amd import occupancy

    m = _nerf(dev)
    H, W = 15, 20
    c2w, focal = syn.look_at_pose(4.0, 60, 20), syn.focal_from_fovy(H)
    grid = _random_grid(ops, dev)
    whole = occupancy.render_image(m, c2w, H, W, focal, NEAR, FAR, grid, ray_bounds=True)
    parts = occupancy.render_image(m, c2w, H, W, focal, NEAR, FAR, grid, ray_bounds=True, chunk=97)   # the limits belong to the image
    for k in ("rgb", "acc", "depth"):
        assert torch.equal(whole[k], parts[k])
    assert whole["occupied"] == parts["occupied"] and 0.2 * H * W <= whole["live"] <= 0.8 * H * W
    # the grid's box is [-1, 1]^3: the same picture as the direct call with the limits of a side-2 cube
    o, v = ops.raygen(c2w, H, W, focal, device=dev)
    near, far, live = ops.ray_limits(o, v, 2.0)
    outs, occupied = ops.render_fwd_occ(m.coarse_mlp.packed(), m.fine_mlp.packed(), o, v, v, near, far, True, grid, ray_live=live)
    assert torch.equal(whole["rgb"].view(-1, 3), outs[1][0]) and whole["occupied"] == occupied.tolist()
    nogrid = occupancy.render_image(m, c2w, H, W, focal, NEAR, FAR, None, ray_bounds=True, box=2.0)
    assert nogrid["occupied"] == [int(live.sum()) * 65, int(live.sum()) * 193]
    with pytest.raises(ValueError, match="box="):
        occupancy.render_image(m, c2w, H, W, focal, NEAR, FAR, None, ray_bounds=True)
