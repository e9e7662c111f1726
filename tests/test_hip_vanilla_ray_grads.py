"""Ray gradients of a frozen vanilla network (csrc/aon_ray_grad.hip, include/aon_hip_inputs.h): dL/d rays_o, rays_d,
viewdirs against the reference's autograd (G28) and the live oracle under the project's gradient yardstick (tests/_gradcheck.py: as close to
the fp64 truth as the reference's fp32 is, factor 5, floor 1e-4); the bit-equality, determinism and permutation properties of the contract;
the refusals and the memory contract of aon_render_bwd_inputs; the routing of NeRF.forward; the stream contract; LitNeRF.fit_pose."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_extents import NEAR, FAR, Case, _flat, _net, _opts, _packs, _rays, _S, _uni, run_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rays_o", "rays_d", "viewdirs")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _sizes(min_deg_point=0, max_deg_point=10, deg_view=4, **_):
    return dict(pos_size=3 + 6 * (max_deg_point - min_deg_point), view_pos_size=3 + 6 * deg_view)


def _model(dev, seed=2, density_scale=10.0, num_levels=2, sd=None, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = NeRF(num_levels=num_levels, **kw).to(dev)
    model.load_state_dict(sd if sd is not None else syn.make_nerf_state_dict(seed=seed, density_scale=density_scale, **_sizes(**kw)))
    return model.requires_grad_(False)


def _inputs(model, n, seed):
    """CPU tensors: rays, target, t_rand, u (shared by the HIP call and the oracle)."""
    import aon_amd.synthetic as syn

    rays = syn.random_rays(n, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    return rays, torch.rand(n, 3, generator=gen), torch.rand(n, model.num_coarse_samples + 1, generator=gen), torch.rand(n, model.num_fine_samples, generator=gen)


def _loss(out, target, acc_depth):
    loss = sum(torch.mean((o[0] - target) ** 2) for o in out)
    if acc_depth:
        loss = loss + sum(0.3 * torch.mean(o[1]) + 0.1 * torch.mean(o[2] ** 2) for o in out)
    return loss


def _hip_grads(model, dev, rays, target, t_rand, u, acc_depth=False, near=2.0, far=6.0, shared_dir=False, which=NAMES, randomized=True):
    """One forward + backward of the frozen model with the rays as leaves -> ({name: grad on the device}, loss)."""
    leaves = {k: rays[k].to(dev).clone().requires_grad_(k in which) for k in NAMES}
    if shared_dir:
        leaves["viewdirs"] = leaves["rays_d"]
    out = model(leaves, randomized, True, near, far, t_rand=t_rand.to(dev) if randomized else None, u=u.to(dev) if randomized else None)
    loss = _loss(out, target.to(dev), acc_depth)
    loss.backward()
    return {k: leaves[k].grad.clone() for k in NAMES if leaves[k].grad is not None}, loss.detach()


def _oracle_grads(model, rays, target, t_rand, u, dtype, acc_depth=False, near=2.0, far=6.0, randomized=True):
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    leaves = {k: rays[k].to(dtype).clone().requires_grad_(True) for k in NAMES}
    cast = lambda x: x.detach().cpu().to(dtype) if isinstance(x, torch.Tensor) else x   # noqa: E731
    out = orc.nerf_forward(sd, leaves, randomized, True, cast(near), cast(far), num_levels=model.num_levels, min_deg_point=model.min_deg_point,
                           max_deg_point=model.max_deg_point, deg_view=model.deg_view, num_coarse_samples=model.num_coarse_samples,
                           num_fine_samples=model.num_fine_samples, t_rand=t_rand.to(dtype) if randomized else None,
                           u=u.to(dtype) if randomized else None)
    loss = _loss(out, target.to(dtype), acc_depth)
    return dict(zip(NAMES, torch.autograd.grad(loss, [leaves[k] for k in NAMES])))


def _yardstick():
    import _gradcheck

    return _gradcheck


# ---------------------------------------------------------------- against the reference's autograd (G28)
def _fixture_inputs(g):
    import aon_amd.synthetic as syn

    n = int(g["n"])
    return (syn.random_rays(n, seed=int(g["seed_rays"])), syn.seeded_uniform(int(g["seed_target"]), n, 3), syn.seeded_uniform(int(g["seed_t"]), n, 65),
            syn.seeded_uniform(int(g["seed_u"]), n, 128))


@pytest.mark.parametrize("num_levels,draw", [(2, "a"), (2, "b"), (1, "a")])
def test_ray_gradients_meet_the_reference_fixture(dev, golden, fold_form, num_levels, draw):
    """G28: 48 rays, default sizes, white background, the reference's fp32 / fp64 autograd with respect to the three ray tensors.  Two levels:
    both draws under the yardstick.  One level: G28 holds two-level gradients only, so the one-level call is held to the live oracle
    (fp64 truth, its fp32 as the reference) on G28's inputs."""
    g = golden("g28_ray_grads_vanilla")
    model = _model(dev, seed=int(g["model_seed"]), density_scale=float(g["density_scale"]), num_levels=num_levels)
    rays, target, t_rand, u = _fixture_inputs(g)
    hip, loss = _hip_grads(model, dev, rays, target, t_rand, u, acc_depth=draw == "b")
    hip = {k: v.cpu() for k, v in hip.items()}
    assert set(hip) == set(NAMES) and all(torch.isfinite(v).all() and v.abs().max() > 0 for v in hip.values())
    if num_levels == 2:
        l32, l64 = float(g[f"{draw}.loss32"]), float(g[f"{draw}.loss64"])
        print(f"G28 draw {draw} {fold_form}: loss {loss.item():.9e} fixture fp64 {l64:.9e} fp32 {l32:.9e}")
        for k in NAMES:
            dist = (hip[k].double() - torch.as_tensor(g[f"{draw}.{k}|truth"]).double()).norm().item()
            print(f"  {k}: |hip - truth| {dist:.3e}, |ref32 - truth| {float(g[f'{draw}.{k}|ref32_dist']):.3e}, |truth| {float(g[f'{draw}.{k}|norm']):.3e}")
        assert abs(loss.item() - l64) <= max(5.0 * abs(l32 - l64), 2e-6 * abs(l64))
        sub = {k[2:]: v for k, v in g.items() if k.startswith(draw + ".") and "|" in k and not k.endswith("|ref32")}
        _yardstick().assert_as_close_as_fp32_fixture(hip, sub, f"vanilla ray gradients, G28 draw {draw}, {fold_form}", factor=5.0, floor=1e-4)
    else:
        truth = _oracle_grads(model, rays, target, t_rand, u, torch.float64)
        ref32 = _oracle_grads(model, rays, target, t_rand, u, torch.float32)
        _yardstick().assert_as_close_as_fp32(hip, truth, ref32, f"vanilla ray gradients, one level, {fold_form}", factor=5.0, floor=1e-4)


# ---------------------------------------------------------------- against the live oracle
# n = 3 / 37 at 65 + 193 samples (a partial block of the sample kernel; 9,546 valid samples, no multiple of 128: padding); 300 rays at
# 39 + 32 samples: rays straddle the 32-sample steps, S is no multiple of the reduce kernel's unroll; two `_deg` degree sets (min_deg != 0:
# the scale is 2^(min_deg + l)); per-ray bounds; the smooth field
CASES = {
    "n3": dict(n=3), "n37": dict(n=37), "n300_sizes": dict(n=300, kw=dict(num_coarse_samples=39, num_fine_samples=32)),
    "deg_0_6_2": dict(n=70, kw=dict(min_deg_point=0, max_deg_point=6, deg_view=2)),
    "deg_1_8_3": dict(n=70, kw=dict(min_deg_point=1, max_deg_point=8, deg_view=3)),
    "bounds": dict(n=70, bounds=True), "smooth": dict(n=37, smooth=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_ray_gradients_against_the_live_oracle(dev, case):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf import helper

    c = CASES[case]
    model = _model(dev, sd=syn.make_smooth_nerf_state_dict() if c.get("smooth") else None, **c.get("kw", {}))
    rays, target, t_rand, u = _inputs(model, c["n"], seed=80 + c["n"])
    near, far = 2.0, 6.0
    if c.get("bounds"):
        near, far = helper.get_ray_limits(rays["rays_o"].to(dev), rays["rays_d"].to(dev), 2.4)
        assert near.shape == (c["n"], 1) and (far > near).any()
    rnd = not c.get("bounds")   # (the oracle's stratified draw takes scalar near / far only: the per-ray case samples deterministically)
    hip, _ = _hip_grads(model, dev, rays, target, t_rand, u, near=near, far=far, randomized=rnd)
    hip = {k: v.cpu() for k, v in hip.items()}
    truth = _oracle_grads(model, rays, target, t_rand, u, torch.float64, near=near, far=far, randomized=rnd)
    ref32 = _oracle_grads(model, rays, target, t_rand, u, torch.float32, near=near, far=far, randomized=rnd)
    for k in NAMES:
        print(f"{case} {k}: |hip - truth| {(hip[k].double() - truth[k]).norm().item():.3e}, |ref32 - truth| {(ref32[k].double() - truth[k]).norm().item():.3e}, "
              f"|truth| {truth[k].norm().item():.3e}")
    _yardstick().assert_as_close_as_fp32(hip, truth, ref32, f"vanilla ray gradients, {case}", factor=5.0, floor=1e-4)


# ---------------------------------------------------------------- bits
def test_repeats_shared_direction_tensor_and_subsets(dev, fold_form):
    """A repeat gives the same bits; one tensor passed as rays_d and viewdirs receives the sum of the two separate results; a subset of the
    rays requiring grad gets the same bits and the others none."""
    model = _model(dev)
    rays, target, t_rand, u = _inputs(model, 37, seed=91)
    g1, _ = _hip_grads(model, dev, rays, target, t_rand, u)
    g2, _ = _hip_grads(model, dev, rays, target, t_rand, u)
    assert set(g1) == set(NAMES)
    for k in NAMES:
        assert torch.isfinite(g1[k]).all() and g1[k].abs().max() > 0 and torch.equal(g1[k], g2[k]), k
    shared, _ = _hip_grads(model, dev, rays, target, t_rand, u, shared_dir=True)
    assert torch.equal(shared["rays_d"], g1["rays_d"] + g1["viewdirs"]) and torch.equal(shared["rays_o"], g1["rays_o"])
    for which in (("rays_d",), ("rays_o", "viewdirs")):
        part, _ = _hip_grads(model, dev, rays, target, t_rand, u, which=which)
        assert set(part) == set(which) and all(torch.equal(part[k], g1[k]) for k in which), which


def test_permuted_and_contained_calls(dev):
    """A ray's gradients do not depend on which rays share the call: a permuted call gives permuted bits, and a 37-ray call equals rows
    0..36 of a 300-ray call that contains them (the 300-ray call spreads over many blocks of both kernels; the 37 rays' samples sit at other
    offsets inside the 32-sample steps and in the other of a lane's two samples)."""
    model = _model(dev, num_coarse_samples=39, num_fine_samples=32)
    rays, target, t_rand, u = _inputs(model, 300, seed=92)
    n = 300

    # the loss is a mean over the rays of the call: weight it so that every ray sees the same upstream gradient in all three calls
    def grads(idx):
        leaves = {k: rays[k][idx].to(dev).clone().requires_grad_(True) for k in NAMES}
        out = model(leaves, True, True, 2.0, 6.0, t_rand=t_rand[idx].to(dev), u=u[idx].to(dev))
        tg = target[idx].to(dev)
        sum(((o[0] - tg) ** 2).sum() / (3 * n) + 0.3 * o[1].sum() / n for o in out).backward()
        return {k: leaves[k].grad.clone() for k in NAMES}

    full = grads(torch.arange(n))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    permuted = grads(perm)
    head = grads(torch.arange(37))
    for k in NAMES:
        assert torch.isfinite(full[k]).all() and full[k].abs().max() > 0
        assert torch.equal(permuted[k], full[k][perm.to(dev)]), k
        assert torch.equal(head[k], full[k][:37]), k


# ---------------------------------------------------------------- routing
def test_forward_routing(dev):
    """Frozen network, the rays requiring grad: the output carries a graph (before this path existed out[-1][0].requires_grad was False and
    the rays got nothing) and it is RenderVanillaInputs'; every other case keeps the function it took."""
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = _model(dev)
    rays, target, t_rand, u = _inputs(model, 16, seed=93)

    def run(ray_grad, net_grad, m=model):
        m.requires_grad_(net_grad)
        leaves = {k: rays[k].to(dev).clone().requires_grad_(ray_grad) for k in NAMES}
        return m(leaves, True, True, 2.0, 6.0, t_rand=t_rand.to(dev), u=u.to(dev)), leaves

    out, leaves = run(True, False)
    assert out[-1][0].requires_grad and type(out[-1][0].grad_fn).__name__ == "RenderVanillaInputsBackward"
    _loss(out, target.to(dev), False).backward()
    g = leaves["rays_o"].grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    assert all(p.grad is None for p in model.parameters())
    for ray_grad in (True, False):
        out, leaves = run(ray_grad, True)
        assert type(out[-1][0].grad_fn).__name__ == "RenderVanillaBackward"
        _loss(out, target.to(dev), False).backward()
        assert all(leaves[k].grad is None for k in NAMES) and all(p.grad is not None for p in model.parameters())
        model.zero_grad(set_to_none=True)
    model.requires_grad_(False)
    # one trainable parameter anywhere: still the training function
    model.fine_mlp.rgb_layer.bias.requires_grad_(True)
    leaves = {k: rays[k].to(dev).clone().requires_grad_(True) for k in NAMES}
    assert type(model(leaves, True, True, 2.0, 6.0, t_rand=t_rand.to(dev), u=u.to(dev))[-1][0].grad_fn).__name__ == "RenderVanillaBackward"
    model.requires_grad_(False)
    out, _ = run(False, False)
    assert not out[-1][0].requires_grad and out[-1][0].grad_fn is None
    with torch.no_grad():
        leaves = {k: rays[k].to(dev).clone().requires_grad_(True) for k in NAMES}
        assert not model(leaves, True, True, 2.0, 6.0, t_rand=t_rand.to(dev), u=u.to(dev))[-1][0].requires_grad
    # what the path does not serve says so
    leaves = {k: rays[k].to(dev).clone().requires_grad_(True) for k in NAMES}
    with pytest.raises(ValueError, match="num_levels=3"):
        _model(dev, num_levels=3)(leaves, False, True, 2.0, 6.0)
    wide = NeRF(max_deg_point=12).to(dev).requires_grad_(False)     # 75 position-encoding columns: the layer-wise engine
    assert wide._general
    with pytest.raises(ValueError, match="layer-wise engine"):
        wide(leaves, False, True, 2.0, 6.0)


# ---------------------------------------------------------------- the C entry point: refusals, what is written
def _c_call(dev, model, rays, target, t_rand, u):
    """A forward through ops.render_fwd_train and the pieces a direct aon_render_bwd_inputs call needs."""
    from aon_amd import ops

    mlps = [model.coarse_mlp, model.fine_mlp]
    packs = model._vanilla_packs(mlps)
    o, d = rays["rays_o"].to(dev), rays["rays_d"].to(dev)
    levels, ws, geometry = ops.render_fwd_train(packs[0][0], packs[1][0], o, d, d, 2.0, 6.0, True, 2, t_rand.to(dev), u.to(dev), opts=model._opts)
    n = d.shape[0]
    g_rgb = [(2.0 / (3 * n)) * (lv[0] - target.to(dev)) for lv in levels]
    return ops, packs, ws, geometry, o, d, g_rgb, [m.ordered_params() for m in mlps]


def test_refusals_come_before_any_launch_and_a_valid_call_writes_its_outputs_only(dev):
    from aon_amd import _lib

    model = _model(dev)
    rays, target, t_rand, u = _inputs(model, 37, seed=94)
    ops, packs, ws, geometry, o, d, g_rgb, params = _c_call(dev, model, rays, target, t_rand, u)
    lib = ops.lib
    n, st = d.shape[0], geometry[0]
    opts = None if st is None else C.byref(st)
    pf, pb = [p[0] for p in packs], [p[1] for p in packs]
    arrs = [ops._vanilla_input_param_array(p, None) for p in params]
    band = torch.full((3, n + 2, 3), -123.456, device=dev)
    good = [o.data_ptr(), d.data_ptr(), band[0, 1].data_ptr(), band[1, 1].data_ptr(), band[2, 1].data_ptr()]
    scratch = ops.train_scratch_inputs_vanilla(dev, n, 2, st)
    assert scratch.numel() == lib.aon_train_scratch_bytes_inputs_vanilla(n, 2, opts)
    ptrs = [ops._pk(pb[0]), ops._pk(pf[0]), ops._pk(pb[1]), ops._pk(pf[1])]

    def hole(arr, i):
        return (C.c_void_p * 24)(*[None if k == i else arr[k] for k in range(24)])

    def call(rg_vals=good, rg_null=False, scratch_bytes=None, n_rays=n, parr=(arrs[0][1], arrs[1][1]), packs4=ptrs):
        rg = None if rg_null else C.byref(_lib.RayGradsC(*rg_vals))
        rc = lib.aon_render_bwd_inputs(*packs4, ops._ptr(d), n_rays, 1, 2, ops._ptr_array(g_rgb), ops._ptr_array([None, None]), ops._ptr_array([None, None]),
                                       parr[0], parr[1], ops._ptr(ws), ws.numel(), ops._ptr(scratch), scratch.numel() if scratch_bytes is None else scratch_bytes,
                                       ops._stream(), opts, rg)
        return rc, lib.aon_last_error()

    for missing in range(5):
        vals = list(good)
        vals[missing] = None
        assert call(rg_vals=vals) == (-1, b"aon_render_bwd_inputs: null member of aon_ray_grads"), missing
    assert call(rg_null=True) == (-1, b"aon_render_bwd_inputs: null aon_ray_grads")
    for lvl, entry in ((0, 0), (1, 10), (0, 16)):
        parr = [arrs[0][1], arrs[1][1]]
        parr[lvl] = hole(parr[lvl], entry)
        assert call(parr=parr) == (-1, b"aon_render_bwd_inputs: null parameter pointer"), (lvl, entry)
    assert call(parr=(arrs[0][1], None)) == (-1, b"aon_render_bwd_inputs: null level pointer")
    assert call(n_rays=0) == (-1, b"aon_render_bwd_inputs: bad size / num_levels")
    assert call(scratch_bytes=scratch.numel() - 1) == (-2, b"aon_render_bwd_inputs: scratch smaller than aon_train_scratch_bytes_inputs_vanilla()")
    # the fine level's forward stream declared in the other form
    form = int(lib.aon_stream_form(pf[1].data_ptr()))
    assert form in (0, 1) and lib.aon_declare_stream_form(pf[1].data_ptr(), 1 - form) == 0
    rc, msg = call()
    assert lib.aon_declare_stream_form(pf[1].data_ptr(), form) == 0
    assert rc == -1 and msg.startswith(b"aon_render_bwd_inputs: forward and transposed streams were packed in different forms")
    torch.cuda.synchronize()
    assert (band == -123.456).all()
    # a valid call: every element of the three outputs is written, the rows around them keep the sentinel; parameters and inputs untouched
    before = [p.detach().clone() for p in model.parameters()]
    o0, d0 = o.clone(), d.clone()
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert (band[:, 0] == -123.456).all() and (band[:, -1] == -123.456).all() and torch.isfinite(band[:, 1:-1]).all()
    assert (band[:, 1:-1] != -123.456).all()
    assert torch.equal(o, o0) and torch.equal(d, d0) and all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    ops.pool_give(scratch)
    # the ops wrapper writes the same three tensors
    g_o, g_d, g_v = ops.render_bwd_inputs(ws, pb, pf, o, d, d, True, 2, g_rgb, [None, None], [None, None], params, geometry=geometry)
    assert torch.equal(g_o, band[0, 1:-1]) and torch.equal(g_d, band[1, 1:-1]) and torch.equal(g_v, band[2, 1:-1])
    ops.pool_give(ws)


# ---------------------------------------------------------------- the memory contract (tests/_guard.py through test_hip_extents.run_case)
GUARD_CASES: list = []
for _n, _kind, _deg in ((1, "default", (0, 10, 4)), (5, "small", (0, 10, 4)), (37, "default", (0, 10, 4)), (37, "small", (0, 10, 4)), (5, "small", (1, 8, 3))):
    def _case(n=_n, kind=_kind, deg=_deg):
        Sc, Sf = _S(kind)

        def make(dev):
            o, d, v = _rays(dev, n)
            params, lat = _net(dev, False, deg)
            return {"pk": _packs(False, params, lat, degrees=deg, bwd=True), "params": params, "o": o, "d": d, "v": v, "t_rand": _uni(160, n, Sc).to(dev),
                    "u": _uni(161, n, Sf - Sc).to(dev), "g_rgb": [(_uni(162 + l, n, 3) - 0.5).to(dev) for l in range(2)], "g_acc": (_uni(164, n) - 0.5).to(dev),
                    "g_depth": (_uni(165, n) - 0.5).to(dev)}

        def call(ops, i):
            pk = i["pk"]
            levels, ws, geometry = ops.render_fwd_train(pk["fwd"][0], pk["fwd"][1], i["o"], i["d"], i["v"], NEAR, FAR, True, 2, i["t_rand"], i["u"],
                                                        opts=_opts(kind, degrees=deg))
            g_rays = ops.render_bwd_inputs(ws, pk["bwd"], pk["fwd"], i["o"], i["d"], i["v"], True, 2, i["g_rgb"], [None, i["g_acc"]], [i["g_depth"], None],
                                           i["params"], geometry=geometry)
            ops.pool_give(ws)
            return _flat(levels) + list(g_rays)
        return Case("vanilla_inputs", f"vanilla_inputs_n{n}_{kind}_deg{'_'.join(map(str, deg))}", make, call,
                    ["aon_render_fwd_train_ex", "aon_render_bwd_inputs", "aon_train_scratch_bytes_inputs_vanilla"])
    GUARD_CASES.append(_case())


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, fold_form, c):
    """Three runs (plain, guarded with 0xFF prefill, guarded with zero prefill): bit-equal outputs, no 0xFFFFFFFF word left, no band touched,
    inputs unchanged, workspace and scratch of exactly the queried sizes."""
    run_case(c, dev, monkeypatch)


# ---------------------------------------------------------------- streams
def test_stream_contract(dev):
    """The whole step enqueued on a side stream while the default stream is kept busy gives the serial call's bits."""
    model = _model(dev)
    rays, target, t_rand, u = _inputs(model, 90, seed=96)
    base, _ = _hip_grads(model, dev, rays, target, t_rand, u)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    busy = torch.randn(2048, 2048, device=dev)
    for _ in range(4):
        busy = busy @ busy * 1e-3    # the default stream has work in flight while the side stream runs the step
    with torch.cuda.stream(side):
        other, _ = _hip_grads(model, dev, rays, target, t_rand, u)
    side.synchronize()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(base[k], other[k]), k


# ---------------------------------------------------------------- fit_pose
FIT = dict(H=8, W=12, steps=60, lr=5e-3, correction=(0.02, -0.025, 0.015, 0.03, -0.03, 0.026),   # a rotation of 2.03 degrees, a translation of 0.0498
           degrees=dict(min_deg_point=0, max_deg_point=3, deg_view=2), seed=5, density_scale=2.0, bias_shift=0.75)


def fit_pose_field():
    """The state dict of the fit_pose tests (shared with tests/test_vanilla_ray_grads_cpu.py)."""
    import aon_amd.synthetic as syn

    sd = syn.make_nerf_state_dict(seed=FIT["seed"], density_scale=FIT["density_scale"], pos_size=21, view_pos_size=15)
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] + FIT["bias_shift"]
    return sd


def pose_errors(p, q):
    R = p[:3, :3].double().cpu() @ q[:3, :3].double().cpu().T
    return math.degrees(math.acos(max(-1.0, min(1.0, (R.trace().item() - 1.0) / 2.0)))), (p[:3, 3].double().cpu() - q[:3, 3].double().cpu()).norm().item()


def oracle_pose_loop(sd, dirs, target, start, dtype, steps):
    """The reference's arithmetic (oracle.nerf_forward) under torch.optim.Adam on one 6-vector -> (losses, fitted pose)."""
    from aon_amd import ops

    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    osd = {k: v.to(dtype) for k, v in sd.items()}
    dd, tg = dirs.cpu().to(dtype), target.cpu().to(dtype)
    corr = torch.zeros(6, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([corr], lr=FIT["lr"])
    out = []
    for _ in range(steps):
        opt.zero_grad()
        ro, rd = ops.rays_from_pose(dd, start.to(dtype), corr)
        r = orc.nerf_forward(osd, {"rays_o": ro, "rays_d": rd, "viewdirs": rd}, False, True, 2.0, 6.0, num_levels=1, num_coarse_samples=32, **FIT["degrees"])
        loss = torch.mean((r[0][0] - tg) ** 2)
        loss.backward()
        opt.step()
        out.append(loss.item())
    with torch.no_grad():
        return out, ops.apply_pose_correction(start.to(dtype), corr)


def test_fit_pose_recovers_a_perturbed_pose(dev):
    """One level, 8 x 12 rays, 32 coarse samples, degrees (0, 3, 2), one view, from a pose perturbed by 2.03 degrees and 0.0498 on the smooth
    field of `fit_pose_field`.  On the CPU the oracle's own loop, fp64 and fp32 alike, ends at 0.023 / 0.053 of the starting rotation /
    translation error after 60 steps (tests/test_vanilla_ray_grads_cpu.py holds it below a quarter).  Here: the first 8 losses against that
    loop in fp64, bar max(2 |oracle32 - oracle64|, 0.02 oracle64) per step -- the rgb of a smooth field is held to 2e-6,
    which moves a mean-square loss of 6e-7 by at most 0.5 %; 0.02 is four times that, for the trajectory --; both errors end below half their
    start; parameters, flags and .grad come back untouched.  Measured on an MI355X: 2.0257 -> 0.0474 degrees, 0.04976 -> 0.00264, loss
    6.3247e-07 -> 7.8125e-10; the 8 losses within 2.0e-11 of the fp64 loop's (bars 7.4e-10 .. 1.3e-08)."""
    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    H, W = FIT["H"], FIT["W"]
    lit = LitNeRF(randomized=False, near=2.0, far=6.0, white_bkgd=True, model_kwargs=dict(num_levels=1, num_coarse_samples=32, **FIT["degrees"])).to(dev)
    sd = fit_pose_field()
    lit.model.load_state_dict(sd)
    true = syn.look_at_pose(4.0, 40.0, 25.0)
    start = ops.apply_pose_correction(true.double(), torch.tensor(FIT["correction"], dtype=torch.float64)).float()
    dirs = ops.ray_directions(H, W, syn.focal_from_fovy(H), device=dev).reshape(-1, 3)
    with torch.no_grad():
        o, d = ops.rays_from_pose(dirs, true.to(dev))
        target = lit.model({"rays_o": o.contiguous(), "rays_d": d, "viewdirs": d}, False, True, 2.0, 6.0)[0][0].clone()
    next(lit.model.coarse_mlp.parameters()).requires_grad_(False)   # a flag the fit must hand back as it found it
    flags = [p.requires_grad for p in lit.model.parameters()]
    before = [p.detach().clone() for p in lit.model.parameters()]
    poses, losses = lit.fit_pose([{"directions": dirs, "target": target}], FIT["steps"], lr=FIT["lr"], poses=[start])
    assert [p.requires_grad for p in lit.model.parameters()] == flags
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, lit.model.parameters())) and all(p.grad is None for p in lit.model.parameters())
    assert losses.shape == (FIT["steps"],) and losses.device.type == "cuda" and torch.isfinite(losses).all()
    e0, e1 = pose_errors(start, true), pose_errors(poses[0], true)
    print(f"fit_pose: rotation {e0[0]:.4f} -> {e1[0]:.4f} degrees, translation {e0[1]:.5f} -> {e1[1]:.5f}; loss {losses[0].item():.4e} -> {losses[-1].item():.4e}")
    assert 1.9 < e0[0] < 2.2 and 0.045 < e0[1] < 0.055
    l64, _ = oracle_pose_loop(sd, dirs, target, start, torch.float64, 8)
    l32, _ = oracle_pose_loop(sd, dirs, target, start, torch.float32, 8)
    hip8 = losses[:8].tolist()
    for i in range(8):
        bar = max(2.0 * abs(l32[i] - l64[i]), 0.02 * l64[i])
        print(f"step {i}: hip {hip8[i]:.6e} oracle64 {l64[i]:.6e} oracle32 {l32[i]:.6e} bar {bar:.1e}")
    for i in range(8):
        assert abs(hip8[i] - l64[i]) <= max(2.0 * abs(l32[i] - l64[i]), 0.02 * l64[i]), (i, hip8[i], l64[i])
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1], (e0, e1)


def test_views_are_independent_fits(dev):
    """Two views fitted in one call are the two views fitted alone, bit for bit: the network is frozen, nothing is drawn, a view's 6-vector
    and moments (columns 6v .. 6v + 5 of the (4, 6 * views) buffer, step count i // views + 1) are touched at its own steps only, and the
    kernels are deterministic.  One level, 32 coarse samples, degrees (0, 3, 2), 7 x 11 rays a view (77 x 33 samples: a padded tail), views
    at azimuths 40 and 75 degrees, each started from FIT's perturbation."""
    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    lit = LitNeRF(randomized=False, near=2.0, far=6.0, white_bkgd=True, model_kwargs=dict(num_levels=1, num_coarse_samples=32, **FIT["degrees"])).to(dev)
    lit.model.load_state_dict(fit_pose_field())
    dirs = ops.ray_directions(7, 11, syn.focal_from_fovy(7), device=dev).reshape(-1, 3)
    views, starts = [], []
    for azimuth in (40.0, 75.0):
        true = syn.look_at_pose(4.0, azimuth, 25.0)
        starts.append(ops.apply_pose_correction(true.double(), torch.tensor(FIT["correction"], dtype=torch.float64)).float())
        with torch.no_grad():
            o, d = ops.rays_from_pose(dirs, true.to(dev))
            views.append({"directions": dirs, "target": lit.model({"rays_o": o.contiguous(), "rays_d": d, "viewdirs": d}, False, True, 2.0, 6.0)[0][0].clone()})
    both, losses = lit.fit_pose(views, 6, poses=starts)
    for v in range(2):
        alone, l = lit.fit_pose([views[v]], 3, poses=[starts[v]])
        assert torch.equal(both[v], alone[0]) and not torch.equal(alone[0].cpu(), starts[v]), v
        assert torch.equal(losses[v::2], l), v
