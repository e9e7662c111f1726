"""Latent-only backward of a frozen articulated network (csrc/aon_train_latent.hip): the three latent gradients
are BIT-EQUAL to the full backward's (ops.art_render_bwd), nothing else is written, the G21 reference yardstick holds, and
LitNeRF_AutoDecoder.fit_latents follows the trajectory of the same loop driven through the full backward."""
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("density", "color", "articulation")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(dev, seed=2, density_scale=10.0, num_levels=2, **kw):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    degrees = {k: kw[k] for k in ("min_deg_point", "max_deg_point", "deg_view") if k in kw}
    model = NeRF_AE_Art(num_levels=num_levels, **kw).to(dev)
    model.load_state_dict(syn.make_art_state_dict(seed=seed, density_scale=density_scale, **degrees))
    return model


def _codes(dev, seed=0, inst=1, art=6):
    import aon_amd.synthetic as syn

    lib = syn.make_code_library_state(seed=seed, n_max_objs=2)
    return {"density": lib["embedding_instance_shape.weight"][inst: inst + 1].to(dev), "color": lib["embedding_instance_appearance.weight"][inst: inst + 1].to(dev),
            "articulation": lib["embedding_instance_articulation.weight"][art: art + 1].to(dev)}


def _inputs(dev, model, n, seed):
    import aon_amd.synthetic as syn

    rays = {k: v.to(dev) for k, v in syn.random_rays(n, seed=seed).items()}
    gen = torch.Generator().manual_seed(seed)
    target = torch.rand(n, 3, generator=gen).to(dev)
    t_rand = torch.rand(n, model.num_coarse_samples + 1, generator=gen).to(dev)
    u = torch.rand(n, model.num_fine_samples, generator=gen).to(dev)
    return rays, target, t_rand, u


def _latent_grads(model, rays, target, t_rand, u, codes, frozen, near=2.0, far=6.0, acc_depth=False):
    """One forward + backward through NeRF_AE_Art: frozen -> the latent-only backward, else the full one (ops.art_render_bwd)."""
    model.requires_grad_(not frozen)
    for p in model.parameters():
        p.grad = None
    lat = {k: v.clone().requires_grad_(True) for k, v in codes.items()}
    out = model(rays, True, True, near, far, lat, t_rand=t_rand, u=u)
    loss = sum(torch.mean((o[0] - target) ** 2) for o in out)
    if acc_depth:   # gradients into acc and depth of every level
        loss = loss + sum(0.3 * torch.mean(o[1]) + 0.1 * torch.mean(o[2] ** 2) for o in out)
    loss.backward()
    return {k: lat[k].grad.clone() for k in KEYS}, loss.detach()


def _assert_same_bits(model, rays, target, t_rand, u, codes, **kw):
    full, loss_full = _latent_grads(model, rays, target, t_rand, u, codes, False, **kw)
    assert all(p.grad is not None for mlp in (model.coarse_mlp, model.fine_mlp)[: model.num_levels] for p in mlp.parameters())   # the full path ran
    only, loss_only = _latent_grads(model, rays, target, t_rand, u, codes, True, **kw)
    assert torch.equal(loss_full, loss_only)
    for k in KEYS:
        assert torch.isfinite(full[k]).all() and full[k].abs().max().item() > 0, k
        assert torch.equal(full[k], only[k]), (k, (full[k] - only[k]).abs().max().item())
    assert all(p.grad is None for p in model.parameters())


# n = 3: 195 / 579 samples, fewer weight-gradient steps than compute units and ONE head segment; n = 37 at 65 + 193: Np = 2,432 / 7,168
# (9,546 valid samples in all, no multiple of 128 or 1,024: the padded tail and ragged work-line segments); n = 300 at 40 / 72 samples: other
# sizes through aon_render_opts, two head segments at the fine level (21,600 samples > 16,384)
@pytest.mark.parametrize("num_levels", [1, 2])
@pytest.mark.parametrize("n,sizes", [(3, None), (37, None), (300, (39, 32))])
def test_latent_gradients_bit_equal_to_full_backward(dev, fold_form, n, sizes, num_levels):
    kw = {} if sizes is None else {"num_coarse_samples": sizes[0], "num_fine_samples": sizes[1]}
    model = _model(dev, num_levels=num_levels, **kw)
    rays, target, t_rand, u = _inputs(dev, model, n, seed=40 + n)
    _assert_same_bits(model, rays, target, t_rand, u, _codes(dev))


# The full backward has two finishing forms for the latent gradients: the merged launch of both levels (art_finish2_kernel, merged
# schedule, with the early head reductions or without) and the per-level form (set_bwd_merge off: art_finish_kernel once per level, level
# 1's into a temporary that is added afterwards).  Sizes as above: n = 3 (one head segment, fewer steps than compute units) and n = 37 at
# the default 65 / 193 samples (Np = 2,432 / 7,168: ragged against 128 and 1,024).
@pytest.mark.parametrize("n", [3, 37])
def test_latent_gradients_across_backward_schedules(dev, fold_form, n):
    from aon_amd import ops

    model = _model(dev)
    rays, target, t_rand, u = _inputs(dev, model, n, seed=60 + n)
    codes = _codes(dev)
    runs = []
    try:
        for merge, early in ((True, True), (False, True), (True, False)):
            ops.set_bwd_merge(merge)
            ops.set_bwd_early_heads(early)
            runs.append(_latent_grads(model, rays, target, t_rand, u, codes, False))
            assert all(p.grad is not None for p in model.parameters())   # the full path ran
    finally:
        ops.set_bwd_merge(True)
        ops.set_bwd_early_heads(True)
    only, loss_only = _latent_grads(model, rays, target, t_rand, u, codes, True)
    model.requires_grad_(True)
    base, loss = runs[0]
    for k in KEYS:
        assert torch.isfinite(base[k]).all() and base[k].abs().max().item() > 0, k
    for grads, other_loss in runs[1:] + [(only, loss_only)]:
        assert torch.equal(loss, other_loss)
        for k in KEYS:
            assert torch.equal(base[k], grads[k]), (k, (base[k] - grads[k]).abs().max().item())


def test_bit_equal_other_degrees(dev):
    model = _model(dev, min_deg_point=0, max_deg_point=6, deg_view=2)
    rays, target, t_rand, u = _inputs(dev, model, 70, seed=7)
    _assert_same_bits(model, rays, target, t_rand, u, _codes(dev))


def test_bit_equal_with_acc_and_depth_gradients(dev):
    model = _model(dev)
    rays, target, t_rand, u = _inputs(dev, model, 70, seed=8)
    _assert_same_bits(model, rays, target, t_rand, u, _codes(dev), acc_depth=True)


def test_bit_equal_with_per_ray_bounds(dev):
    from aon_amd.models.vanilla_nerf import helper

    model = _model(dev)
    rays, target, t_rand, u = _inputs(dev, model, 70, seed=9)
    near, far = helper.get_ray_limits(rays["rays_o"], rays["rays_d"], 2.4)
    assert near.shape == (70, 1) and (far > near).any()
    _assert_same_bits(model, rays, target, t_rand, u, _codes(dev), near=near, far=far)


def test_nothing_else_is_written(dev):
    """The parameter-gradient slots of an arena keep a sentinel, every MLP parameter's .grad stays None, and the scratch is smaller."""
    from aon_amd import ops
    from aon_amd.arena import ParamArena

    model = _model(dev)
    arena = ParamArena([model])
    sentinel = -123.456
    arena.grad.fill_(sentinel)
    rays, target, t_rand, u = _inputs(dev, model, 130, seed=11)
    only, _ = _latent_grads(model, rays, target, t_rand, u, _codes(dev), True)
    torch.cuda.synchronize()
    assert torch.equal(arena.grad, torch.full_like(arena.grad, sentinel))
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.isfinite(only[k]).all() for k in KEYS)
    model.requires_grad_(True)
    for n in (1, 130, 4096):
        for levels in (1, 2):
            small, full = ops.lib.aon_train_scratch_bytes_latents(n, levels, None), ops.lib.aon_train_scratch_bytes_ex(n, 1, levels, None)
            assert 0 < small < full - levels * (90 << 20), (n, levels, small, full)   # no 96 MiB weight-gradient workspace per level


def test_latent_gradients_meet_the_reference_fixture(dev, golden):
    """G21 (4096 rays of BASELINE config 5, the REAL reference's fp32 and fp64 autograd): the latent-only gradients of the three embedding
    tables under the bar tests/test_hip_training_art.py::test_art_training_step_full_size_vs_reference applies to them (tests/_gradcheck.py,
    factor 5, floor 1e-4), and the same loss bar."""
    import aon_amd.synthetic as syn
    from aon_amd.models.code_library import CodeLibraryArticulated

    sys.path.insert(0, os.path.dirname(__file__))
    from _gradcheck import assert_as_close_as_fp32_fixture

    g = golden("g21_config5_step")
    n = int(g["n"])
    model = _model(dev, seed=int(g["seed"]), density_scale=float(g["density_scale"]))
    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=1, N_obj_code_length=128)).to(dev)
    lib.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=1))
    rays = {k: g[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs")}
    gen = torch.Generator().manual_seed(int(g["generator_seed"]))
    assert torch.equal(torch.randint(0, int(g["H"]) * int(g["W"]), (n,), generator=gen), g["idx"])
    target = torch.rand(n, 3, generator=gen)
    t_rand, u = torch.rand(n, 65, generator=gen), torch.rand(n, 128, generator=gen)
    target, t_rand, u = target.to(dev), t_rand.to(dev), u.to(dev)
    model.requires_grad_(False)
    latents = lib({"instance_id": torch.tensor([int(g["instance_id"])], device=dev), "articulation_id": torch.tensor([int(g["articulation_id"])], device=dev)})
    out = model(rays, True, True, 2.0, 6.0, latents, t_rand=t_rand, u=u)
    reg = 1e-4 * sum(torch.mean(torch.norm(latents[k], dim=0)) for k in KEYS)
    loss = torch.mean((out[1][0] - target) ** 2) + torch.mean((out[0][0] - target) ** 2) + reg
    loss.backward()
    loss32, loss64 = float(g["loss32"]), float(g["loss64"])
    assert abs(loss.item() - loss64) <= max(5.0 * abs(loss32 - loss64), 2e-6 * abs(loss64))
    assert all(p.grad is None for p in model.parameters())
    hip = {"lib." + name: p.grad.cpu() for name, p in lib.named_parameters()}
    g_lib = {k: v for k, v in g.items() if k.startswith("lib.")}
    assert len(hip) == 3
    assert_as_close_as_fp32_fixture(hip, g_lib, f"latent-only backward, config 5 step at {n} rays", factor=5.0, floor=1e-4)
    # and at this size too -- every compute unit owns a segment of the weight-gradient work line -- the bits of the full backward
    model.requires_grad_(True)
    lib.zero_grad(set_to_none=True)
    latents = lib({"instance_id": torch.tensor([int(g["instance_id"])], device=dev), "articulation_id": torch.tensor([int(g["articulation_id"])], device=dev)})
    out = model(rays, True, True, 2.0, 6.0, latents, t_rand=t_rand, u=u)
    reg = 1e-4 * sum(torch.mean(torch.norm(latents[k], dim=0)) for k in KEYS)
    (torch.mean((out[1][0] - target) ** 2) + torch.mean((out[0][0] - target) ** 2) + reg).backward()
    assert all(p.grad is not None for p in model.parameters())
    for name, p in lib.named_parameters():
        assert torch.equal(p.grad.cpu(), hip["lib." + name]), name


def test_fit_latents_trajectory(dev):
    """Two 24x32 views rendered with codes L*; from L* + noise, 20 steps of fit_latents equal -- losses and codes, bit for bit -- the same
    loop through the full backward; the loss falls; the network is untouched and its requires_grad flags are restored."""
    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False, near=2.0, far=6.0, white_bkgd=True).to(dev)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=2, density_scale=10.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    star = _codes(dev, inst=1, art=3)
    H, W = 24, 32
    batches = []
    for azim in (20.0, 75.0):
        ro, vd = ops.raygen(syn.look_at_pose(azim_deg=azim), H, W, syn.focal_from_fovy(H), device=dev)
        rays = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
        with torch.no_grad():
            rays["target"] = lit.model(rays, False, True, 2.0, 6.0, star)[1][0].clone()
        batches.append(rays)
    gen = torch.Generator().manual_seed(5)
    start = {k: v + 0.05 * torch.randn(v.shape, generator=gen).to(dev) for k, v in star.items()}
    next(lit.model.fine_mlp.parameters()).requires_grad_(False)   # a flag the fit must hand back as it found it
    flags = [p.requires_grad for p in lit.model.parameters()]
    before = [p.detach().clone() for p in lit.model.parameters()]
    codes, losses = lit.fit_latents(batches, 20, lr=5e-3, init=start, seed=3)
    assert [p.requires_grad for p in lit.model.parameters()] == flags
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, lit.model.parameters()))
    assert all(p.grad is None for p in lit.model.parameters())
    next(lit.model.fine_mlp.parameters()).requires_grad_(True)
    ref_codes, ref_losses = lit.fit_latents(batches, 20, lr=5e-3, init=start, seed=3, full_backward=True)
    assert losses.shape == (20,) and losses.device.type == "cuda"
    print("fit losses", [f"{x:.3e}" for x in losses.tolist()])
    assert torch.equal(losses, ref_losses)
    for k in KEYS:
        assert codes[k].shape == star[k].shape and torch.equal(codes[k], ref_codes[k]), k
        assert not torch.equal(codes[k], start[k]), k
    assert torch.isfinite(losses).all() and losses[-1].item() < losses[0].item()


def test_stream_and_lifetime(dev):
    model = _model(dev)
    rays, target, t_rand, u = _inputs(dev, model, 90, seed=13)
    codes = _codes(dev)
    base, _ = _latent_grads(model, rays, target, t_rand, u, codes, True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other, _ = _latent_grads(model, rays, target, t_rand, u, codes, True)
    side.synchronize()
    for k in KEYS:
        assert torch.equal(base[k], other[k]), k
    # a second backward through a released forward
    lat = {k: v.clone().requires_grad_(True) for k, v in codes.items()}
    out = model(rays, True, True, 2.0, 6.0, lat, t_rand=t_rand, u=u)
    loss = out[1][0].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="released by its first backward"):
        loss.backward()
    # an in-place edit of a latent between forward and backward
    lat = {k: v.clone().requires_grad_(True) for k, v in codes.items()}
    out = model(rays, True, True, 2.0, 6.0, lat, t_rand=t_rand, u=u)
    with torch.no_grad():
        lat["articulation"].add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[1][0].sum().backward()
    model.requires_grad_(True)
