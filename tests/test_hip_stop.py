"""GPU: early ray termination on the occupancy renders.  Off is off (the bits of the existing paths); the
terminated renders against a yardstick built from the stage entry points with the empty and the dead samples' density zeroed (the same
bits); the stop indices against the rule (tests/_stop_ref.py); the error bound; the model-level keywords; the frame quality."""
import types

import numpy as np
import pytest
import torch

import _occ_ref as occ_ref
import _stop_ref as ref

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


# The test field.  Random weights give every ray about the same optical depth, so no density scale makes a quarter of the rays stop and
# leaves a quarter running.  This one varies from ray to ray: both levels carry the SAME network (so both see the same matter), only the
# lowest position-encoding level is kept (a smooth field, as synthetic.sparsify_nerf_ cuts), and the density bias is shifted so that 60 %
# of a 21^3 grid over [-4, 4]^3 is empty (relu <= 0.01, softplus argument <= -5).  Scale and shift per eps, so that the median ray's
# optical depth sits near -ln(eps); computed beforehand with the fp64 CPU oracle (oracle/nerf_oracle.py) on 400 random rays: at every
# level and for R in {16, 48} between 36 % and 64 % of the rays stop before the last round (asserted below: at least a quarter each way).
FIELD = {False: {1e-2: (53.0, -1.2655729), 1e-4: (105.0, -2.5275760)},
         True: {1e-2: (170.0, 3.5058274), 1e-4: (230.0, 6.1516800)}}
CUT = [3 + 3 * lv + a + s for lv in range(1, 10) for a in range(3) for s in (0, 30)]


def _field_state(articulated, eps):
    import aon_amd.synthetic as syn

    ds, shift = FIELD[articulated][eps]
    sd = (syn.make_art_state_dict if articulated else syn.make_nerf_state_dict)(seed=0, density_scale=ds)
    for k in list(sd):
        if k.startswith("coarse_mlp."):
            sd[k] = sd["fine_mlp." + k[len("coarse_mlp."):]].clone()
    for p in ("coarse_mlp.", "fine_mlp."):
        sd[p + "pts_linears.0.weight"][:, CUT] = 0.0
        sd[p + "pts_linears.5.weight"][:, [256 + c for c in CUT]] = 0.0
        sd[p + "density_layer.bias"] += shift
    return sd


def _model(dev, articulated, eps=None):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    model = (NeRF_AE_Art if articulated else NeRF)().to(dev)
    if eps is None:
        model.load_state_dict((syn.make_art_state_dict if articulated else syn.make_nerf_state_dict)(seed=0, density_scale=30.0))
    else:
        model.load_state_dict(_field_state(articulated, eps))
    return model


def _latents(dev, art_id=3):
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated

    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    with torch.no_grad():
        return lib({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([art_id], device=dev)}, is_test=True)


def _rays(dev, n=700, seed=1):
    import aon_amd.synthetic as syn

    r = syn.random_rays(n, seed=seed)
    return r["rays_o"].to(dev), r["rays_d"].to(dev), r["viewdirs"].to(dev)


class Net:
    """The two packed levels of a vanilla or articulated model in the current stream form, with the stage and whole-path calls."""

    def __init__(self, ops, model, latents=None):
        self.ops, self.art = ops, latents is not None
        self.pc, self.pf = model.coarse_mlp.packed(fresh=True), model.fine_mlp.packed(fresh=True)
        if self.art:
            self.sc, self.sf = ops.clone_packed(model.coarse_mlp.prepared(latents)), ops.clone_packed(model.fine_mlp.prepared(latents))
        self.act = ops.ACT_ARTICULATED if self.art else ops.ACT_VANILLA

    def exact(self, o, d, v, num_levels=2, opts=None):
        if self.art:
            return self.ops.art_render_fwd(self.pc, self.sc, self.pf, self.sf, o, d, v, NEAR, FAR, True, num_levels, opts=opts)
        return self.ops.render_fwd(self.pc, self.pf, o, d, v, NEAR, FAR, True, num_levels, opts=opts)

    def occ(self, o, d, v, grid, num_levels=2, opts=None, workspace_bytes=None):
        if self.art:
            return self.ops.art_render_fwd_occ(self.pc, self.sc, self.pf, self.sf, o, d, v, NEAR, FAR, True, grid, num_levels, opts=opts,
                                               workspace_bytes=workspace_bytes)
        return self.ops.render_fwd_occ(self.pc, self.pf, o, d, v, NEAR, FAR, True, grid, num_levels, opts=opts, workspace_bytes=workspace_bytes)

    def stop(self, o, d, v, grid, eps, R=None, num_levels=2, opts=None, workspace_bytes=None):
        if self.art:
            return self.ops.art_render_fwd_stop(self.pc, self.sc, self.pf, self.sf, o, d, v, NEAR, FAR, True, grid, eps, R, num_levels, opts=opts,
                                                workspace_bytes=workspace_bytes)
        return self.ops.render_fwd_stop(self.pc, self.pf, o, d, v, NEAR, FAR, True, grid, eps, R, num_levels, opts=opts,
                                        workspace_bytes=workspace_bytes)

    def mlp(self, level, o, d, v, t):
        pk = self.pc if level == 0 else self.pf
        if self.art:
            return self.ops.art_mlp_fwd(pk, self.sc if level == 0 else self.sf, o, d, v, t)
        return self.ops.mlp_fwd(pk, o, d, v, t)


def _mask(grid, o, d, t):
    """numpy lookup of the section 4.9 convention on cast_rays' bits -> (n, S) bool cuda tensor; no grid: everything occupied"""
    if grid is None:
        return torch.ones(t.shape, dtype=torch.bool, device=t.device)
    occ = grid.occupied().cpu().numpy()
    m = occ_ref.lookup(occ, grid.lo.numpy(), grid.step.numpy(), occ_ref.cast(o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy()))
    return torch.from_numpy(m).to(t.device)


def _zeroed(raw, keep):
    r = raw.clone()
    r[..., 3][~keep] = float("-inf")
    return r


def _yardstick(net, o, d, v, grid, stop, nc=64, nf=128, num_levels=2):
    """Stage entry points with the sigma of the empty samples (numpy grid lookup) and of the dead ones (i >= stop[ray], the product's own
    stop map) overwritten by the sentinel: sample_along_rays (nc + 1 samples) -> mlp -> mask -> composite_pdf -> mlp on t_fine -> mask ->
    composite; one level: sample_along_rays -> mlp -> mask -> composite.
    Returns per level: the terminated tuple, the tuple with the grid mask alone on the same t values, t, the exact raw records, the grid
    mask and the count of samples that are neither empty nor dead."""
    ops = net.ops
    dev = o.device
    out = []
    t_c, _ = ops.sample_along_rays(o, d, nc, NEAR, FAR, want_coords=False)
    raw = net.mlp(0, o, d, v, t_c)
    m0 = _mask(grid, o, d, t_c)
    live0 = m0 & torch.from_numpy(ref.live_mask(stop[:, 0].cpu().numpy(), nc + 1)).to(dev)
    if num_levels == 1:
        comp_c, acc_c, _, depth_c = ops.composite_raw(_zeroed(raw, live0), t_c, d, True, net.act, want_weights=False)
        g_c, ga_c, _, gd_c = ops.composite_raw(_zeroed(raw, m0), t_c, d, True, net.act, want_weights=False)
    else:
        comp_c, acc_c, _, depth_c, t_f = ops.composite_pdf(_zeroed(raw, live0), t_c, d, True, net.act)
        g_c, ga_c, _, gd_c, _ = ops.composite_pdf(_zeroed(raw, m0), t_c, d, True, net.act)
    out.append({"got": (comp_c, acc_c, depth_c), "grid_only": (g_c, ga_c, gd_c), "t": t_c, "raw": raw, "mask": m0, "count": int(live0.sum())})
    if num_levels == 1:
        return out
    raw_f = net.mlp(1, o, d, v, t_f)
    m1 = _mask(grid, o, d, t_f)
    live1 = m1 & torch.from_numpy(ref.live_mask(stop[:, 1].cpu().numpy(), nc + 1 + nf)).to(dev)
    comp_f, acc_f, _, depth_f = ops.composite_raw(_zeroed(raw_f, live1), t_f, d, True, net.act, want_weights=False)
    g_f, ga_f, _, gd_f = ops.composite_raw(_zeroed(raw_f, m1), t_f, d, True, net.act, want_weights=False)
    out.append({"got": (comp_f, acc_f, depth_f), "grid_only": (g_f, ga_f, gd_f), "t": t_f, "raw": raw_f, "mask": m1, "count": int(live1.sum())})
    return out


def _same(a, b):
    for la, lb in zip(a, b):
        for x, y in zip(la, lb):
            assert torch.equal(x, y), (x - y).abs().max()


def _grid(ops, dev, kind):
    if kind == "none":
        return None
    if kind == "random":
        g = torch.Generator().manual_seed(7)
        return ops.occupancy_grid(torch.rand(9, 10, 11, generator=g).to(dev), -1.5, 1.5, 0.917, 0)   # about half of the cells
    dims, lo, hi = (12, 13, 14), (-1.4, -1.5, -1.3), (1.5, 1.2, 1.4)
    pts = ops.grid_points(dims, lo, hi, device=dev).view(*dims, 3)
    return ops.occupancy_grid((pts[..., 0] + 0.5 * pts[..., 1] > 0.1).float().contiguous(), lo, hi, 0.5, 0)


# ---------------------------------------------------------------- 1. off is off
@pytest.mark.parametrize("articulated", [False, True])
@pytest.mark.parametrize("fold", [True, False])
def test_eps_zero_is_bit_equal(ops, dev, articulated, fold):
    ops.set_bottleneck_fold(fold)
    net = Net(ops, _model(dev, articulated), _latents(dev) if articulated else None)
    o, d, v = _rays(dev)
    n = o.shape[0]
    full = ops.occupancy_grid(torch.ones(5, 5, 5, device=dev), -12.0, 12.0, 0.01, 0)   # encloses every sample (|x| <= 10)
    some = _grid(ops, dev, "random")
    for opts in (None, ops.RenderOpts(num_coarse_samples=40, num_fine_samples=72)):
        op = ops._opts(opts)
        S = [op.Sc, op.Sf]
        for num_levels in (1, 2):
            exact = net.exact(o, d, v, num_levels, opts)
            want, want_occ = net.occ(o, d, v, some, num_levels, opts)
            for R in (1, 32):
                got, occupied, stop = net.stop(o, d, v, some, 0.0, R, num_levels, opts)
                _same(want, got)
                assert occupied.tolist() == want_occ.tolist()
                for lvl in range(2):
                    assert stop[:, lvl].eq(S[lvl] if lvl < num_levels else 0).all()
            for grid in (full, None):
                got, occupied, stop = net.stop(o, d, v, grid, 0.0, 16, num_levels, opts)
                _same(exact, got)
                assert occupied.tolist() == [n * op.Sc, n * op.Sf if num_levels == 2 else 0]
                assert stop[:, 0].eq(op.Sc).all()
        # a workspace for 97 rays: eight chunks, the last one ragged
        small = int(ops.lib.aon_render_stop_workspace_bytes(97, ops.C.byref(op.c_struct(NEAR, FAR)[0])))
        got, occupied, stop = net.stop(o, d, v, some, 0.0, 32, 2, opts, workspace_bytes=small)
        _same(net.occ(o, d, v, some, 2, opts)[0], got)
        assert stop[:, 1].eq(op.Sf).all()


# ---------------------------------------------------------------- 2.-5. zeroing, the rule, not vacuous, the bound
# shape: rays, levels, coarse / fine sample counts (None: the default 64 / 128, levels of 65 and 193 samples).  The compaction works on tiles
# of 1,024 slots of a round and scans 2,048 tile counts a round:
#   tiles / tiles_plus1  one level of 64 samples, R = 48 (rounds of 48 and 16: the width divides neither 64 nor 1,024), 64 and 65 rays:
#                        exactly 3 tiles and exactly 1 tile, and one slot past each
#   many_tiles           11,000 rays, R = 192: the fine level's first round has ceil(11000 * 192 / 1024) = 2,063 tiles, so the scan carries a
#                        total into a second round
SHAPES = {"default": (900, 2, None), "tiles": (64, 1, (63, 64)), "tiles_plus1": (65, 1, (63, 64)), "many_tiles": (11000, 2, None)}
#             (the ids of the cases that were here before the shapes)
STOP_CASES = [pytest.param(eps, R, kind, art, "default", id=f"{eps}-{R}-{kind}-{art}") for art in (False, True) for kind in ("none", "random", "halfspace")
              for R in (500, 16, 48) for eps in (1e-2, 1e-4)]
STOP_CASES += [pytest.param(1e-2, R, kind, art, shape, id=f"0.01-{R}-{kind}-{shape}-{art}") for art in (False, True)
               for R, kind, shape in ((48, "random", "tiles"), (48, "none", "tiles"), (48, "random", "tiles_plus1"), (48, "none", "tiles_plus1"),
                                      (192, "halfspace", "many_tiles"))]


@pytest.mark.parametrize("eps,R,kind,articulated,shape", STOP_CASES)
def test_stop_equals_zeroing_and_follows_the_rule(ops, dev, articulated, kind, R, eps, shape):
    ops.set_bottleneck_fold(True)
    net = Net(ops, _model(dev, articulated, eps), _latents(dev) if articulated else None)
    n, num_levels, sizes = SHAPES[shape]
    opts = None if sizes is None else ops.RenderOpts(num_coarse_samples=sizes[0], num_fine_samples=sizes[1])
    op = ops._opts(opts)
    o, d, v = _rays(dev, n, seed=4)
    grid = _grid(ops, dev, kind)
    got, occupied, stop = net.stop(o, d, v, grid, eps, R, num_levels, opts)
    yard = _yardstick(net, o, d, v, grid, stop, op.num_coarse_samples, op.num_fine_samples, num_levels)
    # 2. the same bits as zeroing the empty and the dead samples; `occupied` counts the samples that ran
    _same([y["got"] for y in yard], got)
    assert occupied.tolist() == [y["count"] for y in yard] + [0] * (2 - num_levels)
    # determinism and chunking: the same bits, the same stops
    small = int(ops.lib.aon_render_stop_workspace_bytes(101, None if opts is None else ops.C.byref(op.c_struct(NEAR, FAR)[0])))
    again, occ2, stop2 = net.stop(o, d, v, grid, eps, R, num_levels, opts, workspace_bytes=small)
    _same(got, again)
    assert torch.equal(stop, stop2) and occ2.tolist() == occupied.tolist()

    ts = float(ref.tau_stop(eps))
    d_np = d.cpu().numpy()
    for lvl, y in enumerate(yard):
        S = y["t"].shape[1]
        st = stop[:, lvl].cpu().numpy()
        # 3. the stops are the rule's
        assert np.all((st == S) | ((st % R == 0) & (st < S) & (st > 0)))
        raw_sigma = _zeroed(y["raw"], y["mask"])[..., 3].cpu().numpy()
        t_np = y["t"].cpu().numpy()
        sig64 = ref.sigma64(raw_sigma, "softplus" if articulated else "relu", -1.0)
        t64 = t_np.astype(np.float64)
        delta64 = np.empty_like(t64)
        delta64[:, :-1] = (t64[:, 1:] - t64[:, :-1]) * np.linalg.norm(d_np.astype(np.float64), axis=1, keepdims=True)
        delta64[:, -1] = 0.0   # never part of a deciding boundary
        bt = ref.boundary_tau64(sig64, delta64, R)          # (n, B): tau at the end of every deciding round
        for k in range(bt.shape[1]):
            end = (k + 1) * R
            at = st == end
            before = st > end                                # still live after this boundary (S included)
            assert np.all(bt[at, k] >= ts * (1 - 1e-4)), (lvl, k)
            assert np.all(bt[before, k] < ts * (1 + 1e-4)), (lvl, k)
        if not articulated:   # relu: pure IEEE arithmetic on device-produced inputs -> exactly the reference's stops
            want = ref.stops(ref.relu_sigma(raw_sigma), ref.deltas(t_np, d_np), eps, R)
            assert np.array_equal(st, want), int((st != want).sum())
        # 4. not vacuous (the field was chosen for the renders without a grid)
        stopped = float((st < S).mean())
        print(f"articulated={articulated} grid={kind} R={R} eps={eps} level {lvl}: {stopped:.3f} of the rays stop, "
              f"ran {occupied[lvl].item() / (n * S):.3f} of the samples")
        if R >= S:
            assert stopped == 0.0
        elif kind == "none":
            assert stopped >= 0.25 and 1.0 - stopped >= 0.25
        # 5. the bound: the same t values with and without the dead samples' sentinels
        bound = eps + S * 1e-10 + 1e-6
        (rgb, acc, depth), (rgb0, acc0, depth0) = y["got"], y["grid_only"]
        e_rgb, e_acc, e_depth = (rgb - rgb0).abs().max().item(), (acc - acc0).abs().max().item(), (depth - depth0).abs().max().item()
        print(f"    |d rgb| {e_rgb:.3e}  |d acc| {e_acc:.3e}  |d depth| {e_depth:.3e}  (bound {bound:.3e})")
        assert e_rgb <= bound and e_acc <= bound
        assert e_depth <= FAR * bound


def test_literal_stream_form(ops, dev):
    """The round loop on the literal (unfolded) streams, both networks: the yardstick's bits."""
    ops.set_bottleneck_fold(False)
    o, d, v = _rays(dev, 500, seed=4)
    for articulated in (False, True):
        net = Net(ops, _model(dev, articulated, 1e-2), _latents(dev) if articulated else None)
        grid = _grid(ops, dev, "halfspace")
        got, occupied, stop = net.stop(o, d, v, grid, 1e-2, 16)
        yard = _yardstick(net, o, d, v, grid, stop)
        _same([y["got"] for y in yard], got)
        assert occupied.tolist() == [y["count"] for y in yard]


# ---------------------------------------------------------------- 6. model level
def test_model_forward_and_render_image(ops, dev):
    import aon_amd.synthetic as syn
    from aon_amd.occupancy import build_occupancy, render_image

    ops.set_bottleneck_fold(True)
    model = _model(dev, False, 1e-2)
    grid = build_occupancy(model, (-1.2, 1.2), 32)
    o, d, v = _rays(dev, 300)
    rays = {"rays_o": o, "rays_d": d, "viewdirs": v}
    pc, pf = model.coarse_mlp.packed(), model.fine_mlp.packed()
    with torch.no_grad():
        for g in (grid, None):
            got = model(rays, False, True, NEAR, FAR, occupancy=g, early_stop=1e-2)
            want, _, _ = ops.render_fwd_stop(pc, pf, o, d, v, NEAR, FAR, True, g, 1e-2)
            _same(want, got)
        _same(model(rays, False, True, NEAR, FAR, occupancy=grid), model(rays, False, True, NEAR, FAR, occupancy=grid, early_stop=0.0))
        with pytest.raises(ValueError):
            model(rays, True, True, NEAR, FAR, early_stop=1e-2)
    with pytest.raises(RuntimeError):
        model(rays, False, True, NEAR, FAR, early_stop=1e-2)

    art, lat = _model(dev, True, 1e-2), _latents(dev)
    agrid = build_occupancy(art, (-1.2, 1.2), 32, threshold=1.0, latents=lat)
    with torch.no_grad():
        for g in (agrid, None):
            got = art(rays, False, True, NEAR, FAR, lat, train=False, occupancy=g, early_stop=1e-2)
            want, _, _ = ops.art_render_fwd_stop(art.coarse_mlp.packed(), art.coarse_mlp.prepared(lat), art.fine_mlp.packed(),
                                                 art.fine_mlp.prepared(lat), o, d, v, NEAR, FAR, True, g, 1e-2)
            _same(want, got)
    with pytest.raises(RuntimeError):
        art(rays, False, True, NEAR, FAR, lat, early_stop=1e-2)

    H, W = 24, 32
    c2w, focal = syn.look_at_pose(), syn.focal_from_fovy(H)
    for g in (grid, None):
        img = render_image(model, c2w, H, W, focal, NEAR, FAR, g, early_stop=1e-2, round_samples=16, chunk=500)
        assert img["stop"].shape == (H, W) and img["stop"].dtype == torch.int32
        st = img["stop"]
        assert bool(((st == 193) | ((st % 16 == 0) & (st > 0) & (st < 193))).all())
        assert img["occupied"][1] <= img["samples"][1]
    assert "stop" not in render_image(model, c2w, H, W, focal, NEAR, FAR, grid)
    # an empty grid plus stop: the background, nothing evaluated, nobody stops
    empty = ops.occupancy_grid(torch.zeros(5, 5, 5, device=dev), -12.0, 12.0, 0.01, 2)
    img = render_image(model, c2w, H, W, focal, NEAR, FAR, empty, early_stop=1e-2)
    assert img["occupied"] == [0, 0] and bool((img["stop"] == 193).all())
    assert torch.equal(img["rgb"], torch.ones_like(img["rgb"])) and torch.equal(img["acc"], torch.zeros_like(img["acc"]))


# ---------------------------------------------------------------- 7. frame quality
def test_sparse_frame_quality(ops, dev):
    """The 160 x 120 sparse synthetic frame of section 4.9, both levels, the default grid, eps = 1e-3, the default round size, against the
    exact render_fwd frame.  The bits are deterministic: the bar sits 3 dB below the measured PSNR, never below the project's 40 dB floor."""
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.occupancy import build_occupancy, render_image

    ops.set_bottleneck_fold(True)
    model = NeRF().to(dev)
    model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    model = syn.sparsify_nerf_(model, 0.8, 4.0)
    grid = build_occupancy(model, (-4.0, 4.0))
    H, W = 120, 160
    c2w = syn.look_at_pose()
    focal = syn.focal_from_fovy(H)
    only = render_image(model, c2w, H, W, focal, NEAR, FAR, grid)
    both = render_image(model, c2w, H, W, focal, NEAR, FAR, grid, early_stop=1e-3)
    ro, vd = ops.raygen(c2w, H, W, focal, device=dev)
    with torch.no_grad():
        exact = model({"rays_o": ro, "rays_d": vd, "viewdirs": vd}, False, True, NEAR, FAR)

    def psnr(img):
        mse = torch.mean((img["rgb"].reshape(-1, 3) - exact[1][0]) ** 2).item()
        return float("inf") if mse == 0 else -10 * np.log10(mse)

    frac = [o / s for o, s in zip(both["occupied"], both["samples"])]
    frac0 = [o / s for o, s in zip(only["occupied"], only["samples"])]
    print(f"sparse frame: grid only ran coarse {frac0[0]:.3f} fine {frac0[1]:.3f} of the samples, PSNR {psnr(only):.2f} dB; grid + stop ran "
          f"coarse {frac[0]:.3f} fine {frac[1]:.3f}, PSNR {psnr(both):.2f} dB, {float((both['stop'] < 193).float().mean()):.3f} of the rays stop")
    assert both["occupied"][0] <= only["occupied"][0]   # the coarse t values are the same: a subset
    # measured 63.03 dB -- the grid-only frame's own figure: on this field (density scale 30) no ray reaches -ln(1e-3) before its last round,
    # so nothing stops and the bits are the grid-only frame's.  The bar: 3 dB below the measurement.
    assert psnr(both) > 60.0
