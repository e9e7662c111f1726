"""torch.autograd glue for the HIP render path (SURVEY 8(a) R14, 8(b) "Ownership"): ``NeRF.forward`` under
``torch.is_grad_enabled()`` returns tensors whose graph reaches the module's parameters, so the reference's
``training_step`` (``loss.backward()``, model.py:264-282) works unchanged.  Forward and backward are both HIP kernels
(no eager-PyTorch math): fused forward with activation planes -> composite backward -> fused data-gradient chain ->
grouped split-N weight-gradient GEMMs, each direction ONE C call (aon_render_fwd_train / aon_render_bwd).  Gradients reach only the MLP parameters: the inverse-CDF draws are detached
(helper.py:249) and rays are data -- but for a FROZEN network whose ray tensors require grad: RenderVanillaInputs / RenderArticulatedInputs
return the gradients of rays_o, rays_d and viewdirs (DESIGN.md sections 4.14, 4.15)."""
from __future__ import annotations

import torch

from . import ops
from .arena import arena_of, grad_views


def _arena_plan(ctx, params):
    """Round 6: when every parameter of this forward lives in one ParamArena (aon_amd/arena.py), its backward writes the parameter
    gradients straight into the arena's gradient slots and returns views of them -- autograd adopts a returned tensor as `.grad` without
    copying -- so that the optimiser and the data-parallel mean run on one flat buffer.  Decided here (forward): the arena and a claim on
    the slots (see ParamArena.claim); re-checked in the backward (`_arena_grads`)."""
    ctx.arena_plan = None
    ao = arena_of(params)
    if ao is None:
        return
    tok = ao[0].claim(ao[1])
    if tok is not None:
        ctx.arena_plan = (ao, tok, list(params))


def _arena_grads(ctx, per_level_shapes):
    """-> per level list of gradient-slot views, or None: only if the plan was granted AND no parameter holds a gradient yet (a second
    backward before zero_grad must ADD to the first one's gradients, which live in those very slots)."""
    plan = getattr(ctx, "arena_plan", None)
    if plan is None:
        return None
    (arena, offs), tok, params = plan
    if tok.done or not arena.intact() or any(p.grad is not None for p in params):
        return None
    flat_shapes = [shp for lvl in per_level_shapes for shp in lvl]
    views = grad_views((arena, offs), flat_shapes)
    out, k = [], 0
    for lvl in per_level_shapes:
        out.append(views[k: k + len(lvl)])
        k += len(lvl)
    return out


def _arena_done(ctx):
    plan = getattr(ctx, "arena_plan", None)
    if plan is not None:
        plan[1].done = True
        ctx.arena_plan = None


def _check_not_released(ctx):
    """The activation planes (10-14 KB per sample) are handed back after the first backward, like autograd's own saved
    tensors without retain_graph: a second backward through the same forward gets the error autograd would give."""
    if getattr(ctx, "released", False):
        raise RuntimeError("aon render: the activation workspace of this forward was released by its first backward "
                           "(a second backward / retain_graph=True is not supported; run the forward again)")


def _level_grads(gouts, num_levels, rays_d):
    """The output gradients of a whole-path forward -> per-level lists (g_rgb, g_acc, g_depth); an rgb that got none reads zeros, acc and depth
    stay None (the C calls take NULL for them)."""
    n = rays_d.shape[0]
    g_rgb = [gouts[3 * l] if gouts[3 * l] is not None else torch.zeros((n, 3), dtype=torch.float32, device=rays_d.device) for l in range(num_levels)]
    return g_rgb, [gouts[3 * l + 1] for l in range(num_levels)], [gouts[3 * l + 2] for l in range(num_levels)]


def _release(ctx, ws):
    """After the backward's one C call: the context lets go of the forward's workspace, which goes back to the pool (the backward's launches
    are enqueued: whoever takes the workspace next is ordered behind them)."""
    ctx.fused, ctx.released, ctx.geometry = None, True, None
    ops.pool_give(ws)


def _ray_grads_out(ctx, g_rays, rays):
    """The three ray gradients in their inputs' shapes, None for a ray tensor (the Function's first three inputs) that needs none"""
    return tuple(g.reshape(t.shape) if ctx.needs_input_grad[i] else None for i, (g, t) in enumerate(zip(g_rays, rays)))


def _vanilla_forward(ctx, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, packs, opts, noise):
    """The forward of the two vanilla Functions: ONE C call (aon_render_fwd_train).  near / far: numbers, or per-ray tensors (DESIGN.md
    section 4.11) -- data like the rays: non-differentiable inputs, no gradient returned.  packs: [(packed_fwd, packed_bwd)] per level;
    the backward chain reads the forward stream for its head weights."""
    ctx.white_bkgd, ctx.num_levels = white_bkgd, num_levels
    ctx.set_materialize_grads(False)   # acc / depth carry no gradient in training: None, not four zero-filled tensors per step
    levels, ws, ctx.geometry = ops.render_fwd_train(packs[0][0], packs[1][0] if num_levels == 2 else None, rays_o, rays_d, viewdirs, near, far,
                                                    white_bkgd, num_levels, t_rand, u, opts=opts, noise=noise)
    ctx.fused = (ws, [pk[1] for pk in packs], [pk[0] for pk in packs])
    return tuple(x for lvl in levels for x in lvl)


class RenderVanilla(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):   # rays_o .. noise as _vanilla_forward, then params: 24 tensors per level in ops.VANILLA_PARAM_ORDER
        params = args[12:]
        ctx.rays_d = args[1]
        out = _vanilla_forward(ctx, *args[:12])
        _arena_plan(ctx, params)
        ctx.param_shapes = [tuple(p.shape) for p in params]
        return out

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, packs_bwd, packs_fwd = ctx.fused    # the whole backward is ONE C call too (aon_render_bwd)
        n_per = len(ops.VANILLA_PARAM_ORDER)
        slots = _arena_grads(ctx, [ctx.param_shapes[l * n_per: (l + 1) * n_per] for l in range(ctx.num_levels)])
        per_level = ops.render_bwd(ws, packs_bwd, packs_fwd, ctx.rays_d, ctx.white_bkgd, ctx.num_levels, *_level_grads(gouts, ctx.num_levels, ctx.rays_d),
                                   geometry=ctx.geometry, grads_out=slots)
        _release(ctx, ws)
        _arena_done(ctx)
        return (None,) * 12 + tuple(g[name] for g in per_level for name in ops.VANILLA_PARAM_ORDER)


class RenderVanillaInputs(torch.autograd.Function):
    """NeRF.forward of a FROZEN network with gradients to its rays: rays_o, rays_d, viewdirs -- whichever of them
    requires grad.  RenderVanilla's forward (arguments included) and released-workspace rule; the rays and the parameters, which the
    backward reads again, are saved the autograd way (an in-place update in between raises).  The backward is aon_render_bwd_inputs: no
    weight-gradient stage, the parameters get none.  t is data: nothing flows through the sampler, near / far or the inverse-CDF draws.  A
    tensor passed both as rays_d and as viewdirs (the datasets' convention) receives the sum of the two slots from autograd."""

    @staticmethod
    def forward(ctx, *args):
        ctx.save_for_backward(*args[:3], *args[12:])
        return _vanilla_forward(ctx, *args[:12])

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, packs_bwd, packs_fwd = ctx.fused
        saved = ctx.saved_tensors   # (raises if a ray tensor or a parameter was modified in place since the forward)
        rays_o, rays_d, viewdirs = saved[:3]
        n_per = len(ops.VANILLA_PARAM_ORDER)
        params = [saved[3 + l * n_per: 3 + (l + 1) * n_per] for l in range(ctx.num_levels)]
        g_rays = ops.render_bwd_inputs(ws, packs_bwd, packs_fwd, rays_o, rays_d, viewdirs, ctx.white_bkgd, ctx.num_levels,
                                       *_level_grads(gouts, ctx.num_levels, rays_d), params, geometry=ctx.geometry)
        _release(ctx, ws)
        return _ray_grads_out(ctx, g_rays, saved[:3]) + (None,) * (9 + n_per * ctx.num_levels)


class RenderLevelVanilla(torch.autograd.Function):
    """ONE level of NeRF.forward on given sample positions t (model.py:175-193: cast + encode + NeRFMLP + activations +
    volumetric_rendering), from the stage-level training entry points: aon_mlp_fwd_train -> aon_composite | aon_composite_bwd ->
    aon_mlp_bwd_chain -> aon_vanilla_wgrad.  The drop-in NeRF loops it for `num_levels > 2` in training (the two-call fused step
    covers one or two levels); the weights it returns feed the next level's inverse CDF and carry no gradient (helper.py:249)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, t_vals, white_bkgd, packed_fwd, packed_bwd, *params):
        raw, planes, masks = ops.mlp_fwd_train(packed_fwd, rays_o, rays_d, viewdirs, t_vals)
        comp, acc, weights, depth = ops.composite_raw(raw, t_vals, rays_d, white_bkgd, ops.ACT_VANILLA, True)
        ctx.keep = (raw, planes, masks, t_vals, rays_d, packed_fwd, packed_bwd)
        ctx.white_bkgd = white_bkgd
        ctx.mark_non_differentiable(weights)
        return comp, acc, depth, weights

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth, _g_weights):
        _check_not_released(ctx)
        raw, planes, masks, t_vals, rays_d, packed_fwd, packed_bwd = ctx.keep
        n = t_vals.shape[0]
        if g_rgb is None:
            g_rgb = torch.zeros((n, 3), dtype=torch.float32, device=t_vals.device)
        d_raw = ops.composite_bwd(raw, t_vals, rays_d, g_rgb, g_acc, g_depth, ctx.white_bkgd, ops.ACT_VANILLA, ops.plane_samples(planes))
        dplanes = ops.mlp_bwd_chain(packed_bwd, packed_fwd, d_raw, masks, planes.shape)
        grads = ops.vanilla_wgrad(planes, dplanes, d_raw, packed_bwd)
        ctx.keep, ctx.released = None, True
        return (None,) * 7 + tuple(grads[name] for name in ops.VANILLA_PARAM_ORDER)


class RenderGeneral(torch.autograd.Function):
    """NeRF.forward with a NeRFMLP of non-default geometry: layer-wise GEMM engine (aon_grender_fwd_train / aon_grender_bwd)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, geom, opts, noise, *params):
        n_per = len(geom.param_order)
        ctx.geom, ctx.rays_d, ctx.white_bkgd, ctx.num_levels = geom, rays_d, white_bkgd, num_levels
        # The backward reads the parameter storages again (W^T of the data chain) while the activations in the workspace come from the
        # forward-time weights: save_for_backward, so that an in-place update between this forward and its backward (two live graphs
        # with an optimizer.step() between their backward calls) raises autograd's version error instead of silently mixing two
        # sets of weights (round 3 kept p.detach() aliases, which bypass the check).
        ctx.save_for_backward(*params)
        pd = [dict(zip(geom.param_order, [p.detach() for p in params[l * n_per: (l + 1) * n_per]])) for l in range(num_levels)]
        levels, ws, ctx.geometry = ops.grender_fwd_train(geom, pd[0], pd[1] if num_levels == 2 else None, rays_o, rays_d,
                                                         viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts=opts, noise=noise)
        ctx.fused = (ws,)
        return tuple(x for lvl in levels for x in lvl)

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, = ctx.fused
        n_per = len(ctx.geom.param_order)
        saved = ctx.saved_tensors   # (raises if a parameter was modified in place since the forward)
        params = [dict(zip(ctx.geom.param_order, saved[l * n_per: (l + 1) * n_per])) for l in range(ctx.num_levels)]
        per_level = ops.grender_bwd(ctx.geom, ws, params, ctx.rays_d, ctx.white_bkgd, ctx.num_levels, *_level_grads(gouts, ctx.num_levels, ctx.rays_d),
                                    ctx.geometry)
        _release(ctx, ws)
        return (None,) * 12 + tuple(g[name] for g in per_level for name in ctx.geom.param_order)


def _art_forward(ctx, save_rays, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, packs, opts, noise, lat_density, lat_color,
                 lat_articulation, *params):
    """The forward of the three articulated Functions, whose `forward(ctx, *args)` takes the arguments from rays_o on: ONE C call
    (aon_art_render_fwd_train).  packs: per level (packed_fwd, small, packed_bwd); params: 40 tensors per level in ops.ART_PARAM_ORDER.
    Parameters and latents (and, `save_rays`, the rays) are read again by the backward: saved the autograd way, so an in-place update in
    between raises instead of mixing two sets of weights (as RenderGeneral)."""
    rays, latents = (rays_o, rays_d, viewdirs), (lat_density, lat_color, lat_articulation)
    ctx.white_bkgd, ctx.num_levels = white_bkgd, num_levels
    if not save_rays:
        ctx.rays_d = rays_d
    ctx.set_materialize_grads(False)   # acc / depth carry no gradient in training: None, not four zero-filled tensors per step
    ctx.lat_shapes = tuple(t.shape for t in latents)
    ctx.save_for_backward(*(rays if save_rays else ()), *latents, *params)
    levels, ws, ctx.geometry = ops.render_fwd_train(packs[0][0], packs[1][0] if num_levels == 2 else None, rays_o, rays_d, viewdirs, near, far,
                                                    white_bkgd, num_levels, t_rand, u, small_c=packs[0][1],
                                                    small_f=packs[1][1] if num_levels == 2 else None, opts=opts, noise=noise)
    ctx.fused = (ws, [pk[2] for pk in packs], [pk[1] for pk in packs])
    return tuple(x for lvl in levels for x in lvl)


def _art_saved(ctx, first):
    """-> (saved tensors, per-level dicts of the saved parameters, which start at `first`); raises if one was modified in place since the forward"""
    n_per = len(ops.ART_PARAM_ORDER)
    saved = ctx.saved_tensors
    return saved, [dict(zip(ops.ART_PARAM_ORDER, saved[first + l * n_per: first + (l + 1) * n_per])) for l in range(ctx.num_levels)]


_LATENT_KEYS = tuple(k for k, _ in ops._LATENT_KEYS)


class RenderArticulated(torch.autograd.Function):
    """NeRF_AE_Art.forward with gradients to the 2 x 40 MLP parameters and the three latents."""

    @staticmethod
    def forward(ctx, *args):
        out = _art_forward(ctx, False, *args)
        _arena_plan(ctx, args[15:])
        return out

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, packs_bwd, smalls = ctx.fused       # the whole backward in ONE C call (aon_art_render_bwd)
        saved, params = _art_saved(ctx, 3)
        slots = _arena_grads(ctx, [[tuple(t.shape) for t in p.values()] for p in params])
        per_level, g_lat = ops.art_render_bwd(ws, packs_bwd, smalls, ctx.rays_d, ctx.white_bkgd, ctx.num_levels, *_level_grads(gouts, ctx.num_levels, ctx.rays_d),
                                              params, dict(zip(_LATENT_KEYS, saved[:3])), geometry=ctx.geometry, grads_out=slots)
        _release(ctx, ws)
        _arena_done(ctx)
        lat = tuple(g_lat[k].reshape(shp) for k, shp in zip(_LATENT_KEYS, ctx.lat_shapes))
        return (None,) * 12 + lat + tuple(g[name] for g in per_level for name in ops.ART_PARAM_ORDER)


class RenderArticulatedLatents(torch.autograd.Function):
    """NeRF_AE_Art.forward of a FROZEN network with gradients to the three latents only (fitting codes to observed views, DESIGN.md section
    4.13): RenderArticulated's forward, and a backward without the weight-gradient stage (aon_art_render_bwd_latents).  The latent
    gradients are bit-equal to RenderArticulated's; the parameters get none."""

    @staticmethod
    def forward(ctx, *args):
        return _art_forward(ctx, False, *args)

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, packs_bwd, smalls = ctx.fused
        _, params = _art_saved(ctx, 3)
        g_lat = ops.art_render_bwd_latents(ws, packs_bwd, smalls, ctx.rays_d, ctx.white_bkgd, ctx.num_levels, *_level_grads(gouts, ctx.num_levels, ctx.rays_d),
                                           params, geometry=ctx.geometry)
        _release(ctx, ws)
        lat = tuple(g_lat[k].reshape(shp) for k, shp in zip(_LATENT_KEYS, ctx.lat_shapes))
        return (None,) * 12 + lat + (None,) * (len(ops.ART_PARAM_ORDER) * ctx.num_levels)


class RenderArticulatedInputs(torch.autograd.Function):
    """NeRF_AE_Art.forward of a FROZEN network with gradients to its INPUTS: rays_o, rays_d, viewdirs -- whichever
    of them requires grad -- and the three latents.  RenderArticulatedLatents' forward, saved tensors (plus the rays, which the backward
    reads again) and released-workspace rules; the
    backward is aon_art_render_bwd_inputs: the latent gradients are RenderArticulatedLatents' bits, and with no latent requiring grad its
    latent launches are skipped.  t is data: nothing flows through the sampler, near / far or the inverse-CDF draws.  A tensor passed both
    as rays_d and as viewdirs (the datasets' convention) receives the sum of the two slots from autograd."""

    @staticmethod
    def forward(ctx, *args):
        return _art_forward(ctx, True, *args)

    @staticmethod
    def backward(ctx, *gouts):
        _check_not_released(ctx)
        ws, packs_bwd, smalls = ctx.fused
        saved, params = _art_saved(ctx, 6)
        rays_o, rays_d, viewdirs = saved[:3]
        need = ctx.needs_input_grad
        want_lat = any(need[12:15])
        g_lat, g_o, g_d, g_v = ops.art_render_bwd_inputs(ws, packs_bwd, smalls, rays_o, rays_d, viewdirs, ctx.white_bkgd, ctx.num_levels,
                                                         *_level_grads(gouts, ctx.num_levels, rays_d), params, geometry=ctx.geometry,
                                                         want_latents=want_lat)
        _release(ctx, ws)
        ray = _ray_grads_out(ctx, (g_o, g_d, g_v), saved[:3])
        lat = (None, None, None)
        if want_lat:
            lat = tuple(g_lat[k].reshape(shp) if need[12 + i] else None for i, (k, shp) in enumerate(zip(_LATENT_KEYS, ctx.lat_shapes)))
        return ray + (None,) * 9 + lat + (None,) * (len(ops.ART_PARAM_ORDER) * ctx.num_levels)


class RenderLevelScene(torch.autograd.Function):
    """ONE level of a scene on given sample positions t (P, S), from the stage-level entry points, as
    RenderLevelVanilla is for the vanilla network: per object with pairs, in ascending k, aon_art_mlp_fwd_train on its segment with its own
    per-call block -> aon_scene_composite | aon_scene_composite_bwd -> per object aon_art_bwd_chain -> aon_art_wgrad.  Gradients reach the 40
    parameters (summed over the objects in ascending k) and each object's three codes; the pairs, t and the rays are data.  The merged
    weights it returns feed the next level's inverse CDF and carry no gradient.

    ``apply(pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, *tensors)``: pairs an ops.ScenePairs, rays_d the WORLD
    directions, tensors = (density, color, articulation) of object 0 .. K - 1, then the 40 parameters in ops.ART_PARAM_ORDER.
    -> (rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K), weights (P, S))."""

    @staticmethod
    def forward(ctx, pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, *tensors):
        return _scene_level_forward(ctx, "RenderLevelScene", pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, tensors)

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, _g_weights):
        g_codes, total, _, _ = _scene_level_backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, want_weights=True, rays=None)
        return (None,) * 8 + tuple(g_codes) + tuple(total[name] for name in ops.ART_PARAM_ORDER)


class SceneBackdrop:
    """What one level of a scene's backdrop brings to the scene-level Functions: ``pairs`` = the objects' pairs
    extended by the backdrop's list (ops.ScenePairs.with_background), the WORLD ``rays_o`` / ``viewdirs`` (n, 3) its n rows run on, and the
    vanilla level's forward and transposed streams.  ``train``: its parameters receive gradients (the forward keeps activation planes)."""

    def __init__(self, pairs, rays_o, viewdirs, packed_fwd, packed_bwd, train: bool):
        self.pairs, self.rays_o, self.viewdirs = pairs, rays_o.detach(), viewdirs.detach()
        self.packed_fwd, self.packed_bwd, self.train = packed_fwd, packed_bwd, bool(train)


def _scene_level_forward(ctx, who, pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, tensors, backdrop=None):
    """The forward of the scene-level Functions; tensors = 3 K codes, then the 40 parameters -- and with a ``backdrop`` (a SceneBackdrop)
    its level's parameters in ops.VANILLA_PARAM_ORDER.  ``pairs`` are the OBJECTS' pairs (P rows); with a backdrop t_vals is (P + n, S), its
    n rows go through the vanilla stage into the last n rows of the raw buffer, and the merge is ops.scene_composite_lists."""
    K, n_par = pairs.K, len(ops.ART_PARAM_ORDER)
    n_bg = len(ops.VANILLA_PARAM_ORDER) if backdrop is not None else 0
    if len(tensors) != 3 * K + n_par + n_bg:
        raise ValueError(f"{who}: expected {3 * K} codes and {n_par}{f' + {n_bg}' if n_bg else ''} parameters, got {len(tensors)} tensors")
    # codes and parameters are read again by the backward: saved the autograd way (an in-place update in between raises)
    ctx.save_for_backward(*tensors)
    ctx.set_materialize_grads(False)
    params = dict(zip(ops.ART_PARAM_ORDER, (p.detach() for p in tensors[3 * K: 3 * K + n_par])))
    t = t_vals.detach()
    all_pairs = pairs if backdrop is None else backdrop.pairs
    raw = torch.empty((all_pairs.P, t.shape[1], 4), dtype=torch.float32, device=t.device)
    per_object = []
    for k in range(K):
        seg = pairs.segment(k)
        if seg.stop == seg.start:      # an object without a pair costs no launch
            per_object.append(None)
            continue
        small = ops.art_prepare(params, dict(zip(_LATENT_KEYS, tensors[3 * k: 3 * k + 3])), out=None, degrees=degrees)
        _, planes, masks = ops.art_mlp_fwd_train(packed_fwd, small, pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
        per_object.append((small, planes, masks))
    lists, bg_planes = None, None
    if backdrop is None:
        rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, rays_d, white_bkgd, opts=opts)
    else:
        P = pairs.P
        if pairs.n and backdrop.train:
            _, planes, masks = ops.mlp_fwd_train(backdrop.packed_fwd, backdrop.rays_o, rays_d.detach(), backdrop.viewdirs, t[P:], out=raw[P:])
            bg_planes = (planes, masks)
        elif pairs.n:      # a frozen backdrop keeps no activation planes
            ops.mlp_fwd(backdrop.packed_fwd, backdrop.rays_o, rays_d.detach(), backdrop.viewdirs, t[P:], out=raw[P:])
        lists = [ops.SceneList(ops.ACT_ARTICULATED, False, opts)] * K + [ops.SceneList(ops.ACT_VANILLA, True)]
        rgb, acc, depth, obj_acc, weights = ops.scene_composite_lists(raw, t, all_pairs, rays_d, white_bkgd, lists)
    ctx.keep = (pairs, t, rays_d.detach(), raw, per_object, packed_bwd, opts, tuple(degrees), backdrop, lists, bg_planes)
    ctx.white_bkgd = white_bkgd
    ctx.mark_non_differentiable(weights)
    return rgb, acc, depth, obj_acc, weights


def _scene_level_backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, want_weights, rays):
    """The backward of the scene-level Functions -> (code gradients, parameter gradients, g_pose (K, 12), backdrop gradients), the first two
    None without `want_weights` (no aon_art_wgrad launch), the third None without `rays` = (world rays_o, viewdirs, objects): with them
    every segment's chain is followed by ops.art_ray_grads into one (P, 3) x 3 buffer, and ops.scene_pose_grads reduces that once on the
    objects' pairs.  The last is the dict of a trainable backdrop's parameter gradients (its n rows of d_raw -> ops.mlp_bwd_chain ->
    ops.vanilla_wgrad), None otherwise: a frozen backdrop launches neither."""
    _check_not_released(ctx)
    pairs, t, rays_d, raw, per_object, packed_bwd, opts, degrees, backdrop, lists, bg_planes = ctx.keep
    tensors = ctx.saved_tensors   # (raises if a code or a parameter was modified in place since the forward)
    K, S, dev = pairs.K, t.shape[1], t.device
    params = dict(zip(ops.ART_PARAM_ORDER, tensors[3 * K: 3 * K + len(ops.ART_PARAM_ORDER)]))
    if g_rgb is None:
        g_rgb = torch.zeros((pairs.n, 3), dtype=torch.float32, device=dev)
    if backdrop is None:
        d_raw = ops.scene_composite_bwd(raw, t, pairs, rays_d, g_rgb, g_acc, g_depth, g_obj_acc, ctx.white_bkgd, opts=opts)
    else:
        d_raw = ops.scene_composite_lists_bwd(raw, t, backdrop.pairs, rays_d, g_rgb, g_acc, g_depth, g_obj_acc, ctx.white_bkgd, lists)
    total, g_codes = None, []
    g_pairs = torch.zeros((3, pairs.P, 3), dtype=torch.float32, device=dev) if rays is not None else None
    for k in range(K):
        codes = tensors[3 * k: 3 * k + 3]
        if per_object[k] is None:
            g_codes += [torch.zeros_like(c) for c in codes]
            continue
        if not want_weights and g_pairs is None:      # only the backdrop's weights are asked for: the objects' chains are not needed
            continue
        small, planes, masks = per_object[k]
        seg = pairs.segment(k)
        rows =(seg.stop - seg.start) * S
        d_seg = torch.zeros((ops.plane_samples(planes), 4), dtype=torch.float32, device=dev)   # the chain reads the zero tail
        d_seg[:rows] = d_raw[seg].reshape(rows, 4)
        dplanes, dxp = ops.art_bwd_chain(packed_bwd, small, d_seg, masks, planes)
        if g_pairs is not None:
            for dst, g in zip(g_pairs, ops.art_ray_grads(dplanes, dxp, params, t[seg], pairs.viewdirs[seg], degrees)):
                dst[seg] = g
        if not want_weights:
            continue
        grads, g_lat = ops.art_wgrad(planes, dplanes, d_seg, dxp, params, dict(zip(_LATENT_KEYS, codes)), degrees, packed_bwd=packed_bwd)
        if total is None:
            total = grads
        else:      # plain adds in ascending k: a fixed order
            for name in ops.ART_PARAM_ORDER:
                total[name] += grads[name]
        g_codes += [g_lat[key].reshape(c.shape) for key, c in zip(_LATENT_KEYS, codes)]
    if not want_weights:
        g_codes = None
    elif total is None:
        total = {name: torch.zeros_like(p) for name, p in params.items()}
    g_pose = None
    if rays is not None:
        rays_o, viewdirs, objects = rays
        g_pose = ops.scene_pose_grads(rays_o, rays_d, viewdirs, pairs, objects, g_pairs[0], g_pairs[1], g_pairs[2])
    bg_grads = None
    if bg_planes is not None:
        planes, masks = bg_planes
        rows = pairs.n * S
        d_bg = torch.zeros((ops.plane_samples(planes), 4), dtype=torch.float32, device=dev)   # the chain reads the zero tail
        d_bg[:rows] = d_raw[pairs.P:].reshape(rows, 4)
        dplanes = ops.mlp_bwd_chain(backdrop.packed_bwd, backdrop.packed_fwd, d_bg, masks, planes.shape)
        bg_grads = ops.vanilla_wgrad(planes, dplanes, d_bg, backdrop.packed_bwd)
    elif backdrop is not None and backdrop.train:      # no ray at all
        bg_grads = {name: torch.zeros_like(p) for name, p in zip(ops.VANILLA_PARAM_ORDER, tensors[3 * K + len(ops.ART_PARAM_ORDER):])}
    ctx.keep, ctx.released = None, True
    return g_codes, total, g_pose, bg_grads


class RenderLevelScenePoses(torch.autograd.Function):
    """RenderLevelScene with gradients to the objects' poses too.  The forward is RenderLevelScene's, bit for bit:
    it runs on the pair arrays aon_scene_pairs wrote, and the pose tensors are inputs for autograd's sake only -- their VALUES must be the
    poses `pairs` was built from (`objects`, whose host copies the backward reads).  Backward: after each object's aon_art_bwd_chain,
    aon_art_ray_grads on its segment; aon_scene_pose_grads once; each pose receives the plain derivative with respect to its (3, 4) entries
    (no tangent-space projection), on its own device and dtype.  t, slot, the pairs' existence, near / far and the world direction's norm
    are data.  The code and parameter gradients are RenderLevelScene's bits; when no code and no parameter needs a gradient,
    aon_art_wgrad is not launched.

    ``apply(pairs, t_vals, rays_o, rays_d, viewdirs, objects, white_bkgd, opts, packed_fwd, packed_bwd, degrees, *tensors)``: the WORLD rays,
    objects as ops.scene_pairs took them, tensors = the K poses (3, 4), then as RenderLevelScene.  -> RenderLevelScene's five outputs."""

    N_HEAD = 11

    @staticmethod
    def forward(ctx, pairs, t_vals, rays_o, rays_d, viewdirs, objects, white_bkgd, opts, packed_fwd, packed_bwd, degrees, *tensors):
        K = pairs.K
        poses = tensors[:K]
        if len(list(objects)) != K or any(tuple(p.shape) != (3, 4) for p in poses):
            raise ValueError(f"RenderLevelScenePoses: expected {K} objects and {K} poses of shape (3, 4)")
        ctx.rays = (rays_o.detach(), viewdirs.detach(), list(objects))
        ctx.pose_like = [(p.device, p.dtype) for p in poses]
        return _scene_level_forward(ctx, "RenderLevelScenePoses", pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, tensors[K:])

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, _g_weights):
        K, need = len(ctx.pose_like), ctx.needs_input_grad
        head = RenderLevelScenePoses.N_HEAD
        want_poses, want_weights = any(need[head: head + K]), any(need[head + K:])
        n_rest = len(need) - head - K
        g_codes, total, g_pose, _ = _scene_level_backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, want_weights, ctx.rays if want_poses else None)
        ctx.rays = None
        rest = tuple(g_codes) + tuple(total[name] for name in ops.ART_PARAM_ORDER) if want_weights else (None,) * n_rest
        return (None,) * head + _pose_grads_out(ctx, need, head, want_poses, g_pose) + rest


def _pose_grads_out(ctx, need, head, want_poses, g_pose):
    """(K, 12) rows [dL/dR | dL/dc] -> one (3, 4) gradient per pose input that needs one, on that pose's own device and dtype"""
    if not want_poses:
        return (None,) * len(ctx.pose_like)
    return tuple(torch.cat([g_pose[k, :9].view(3, 3), g_pose[k, 9:].view(3, 1)], dim=1).to(device=dev, dtype=dt) if need[head + k] else None
                 for k, (dev, dt) in enumerate(ctx.pose_like))


class RenderLevelSceneLists(torch.autograd.Function):
    """ONE level of a scene WITH A BACKDROP on given sample positions t (P + n, S): RenderLevelScenePoses' objects
    -- per object with pairs aon_art_mlp_fwd_train into the first P rows of one raw buffer -- plus the backdrop's n rows through the
    vanilla stage into the last n, merged by aon_scene_composite_lists with K articulated closed records and one vanilla open one.
    Backward: aon_scene_composite_lists_bwd, then per object as RenderLevelScenePoses, and for a TRAINABLE backdrop its n rows of d_raw ->
    aon_mlp_bwd_chain -> aon_vanilla_wgrad.  Gradients reach each object's three codes, the 40 articulated parameters, each pose that needs
    one, and the backdrop level's parameters in ops.VANILLA_PARAM_ORDER.  Only what is asked is paid for: no aon_art_wgrad when no code and
    no articulated weight needs a gradient; when no backdrop parameter does, the backdrop's forward is the plane-free ops.mlp_fwd and neither
    its chain nor its weight-gradient kernel is launched.  t, the pairs' existence, near / far, the world rays and the world direction's
    norm are data.

    ``apply(pairs, t_vals, rays_o, rays_d, viewdirs, objects, white_bkgd, opts, packed_fwd, packed_bwd, degrees, bg_pairs, bg_packed_fwd,
    bg_packed_bwd, *tensors)``: pairs the OBJECTS' ops.ScenePairs (ops.ScenePairs.without_objects for none), bg_pairs =
    pairs.with_background(...), the WORLD rays, objects as ops.scene_pairs took them, tensors = the K poses (3, 4), the 3 K codes, the 40
    parameters, the backdrop level's 24.  -> (rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K + 1), weights (P + n, S))."""

    N_HEAD = 14

    @staticmethod
    def forward(ctx, pairs, t_vals, rays_o, rays_d, viewdirs, objects, white_bkgd, opts, packed_fwd, packed_bwd, degrees, bg_pairs, bg_packed_fwd,
                bg_packed_bwd, *tensors):
        K = pairs.K
        poses = tensors[:K]
        if len(list(objects)) != K or any(tuple(p.shape) != (3, 4) for p in poses):
            raise ValueError(f"RenderLevelSceneLists: expected {K} objects and {K} poses of shape (3, 4)")
        if bg_pairs.K != K + 1 or bg_pairs.P != pairs.P + pairs.n or tuple(t_vals.shape[:1]) != (bg_pairs.P,):
            raise ValueError(f"RenderLevelSceneLists: bg_pairs must be pairs.with_background(...) ({K + 1} lists, {pairs.P + pairs.n} rows) and t_vals "
                             f"hold one row per row of it, got {bg_pairs.K} lists, {bg_pairs.P} rows and t_vals {tuple(t_vals.shape)}")
        n_bg = len(ops.VANILLA_PARAM_ORDER)
        ctx.rays = (rays_o.detach(), viewdirs.detach(), list(objects))
        ctx.pose_like = [(p.device, p.dtype) for p in poses]
        train = any(ctx.needs_input_grad[len(ctx.needs_input_grad) - n_bg:]) if len(tensors) >= n_bg else False
        backdrop = SceneBackdrop(bg_pairs, rays_o, viewdirs, bg_packed_fwd, bg_packed_bwd, train)
        return _scene_level_forward(ctx, "RenderLevelSceneLists", pairs, t_vals, rays_d, white_bkgd, opts, packed_fwd, packed_bwd, degrees, tensors[K:],
                                    backdrop)

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, _g_weights):
        K, need = len(ctx.pose_like), ctx.needs_input_grad
        head, n_bg = RenderLevelSceneLists.N_HEAD, len(ops.VANILLA_PARAM_ORDER)
        n_obj = len(need) - head - K - n_bg      # 3 K codes and the 40 parameters
        want_poses, want_weights = any(need[head: head + K]), any(need[head + K: head + K + n_obj])
        g_codes, total, g_pose, bg_grads = _scene_level_backward(ctx, g_rgb, g_acc, g_depth, g_obj_acc, want_weights, ctx.rays if want_poses else None)
        ctx.rays = None
        rest = tuple(g_codes) + tuple(total[name] for name in ops.ART_PARAM_ORDER) if want_weights else (None,) * n_obj
        bg = tuple(bg_grads[name] for name in ops.VANILLA_PARAM_ORDER) if bg_grads is not None else (None,) * n_bg
        return (None,) * head + _pose_grads_out(ctx, need, head, want_poses, g_pose) + rest + bg
