"""Scenes of several posed articulated objects in one frame: one ``NeRF_AE_Art`` and K <= 16 objects, each with its
own codes, rigid object-to-world pose and box, rendered with correct mutual occlusion -- the approach of Neural Scene Graphs (Ost et al.): a
ray-box test per object, samples inside each box, one sorted merge along the ray.  ``render_scene`` is inference only; ``render_scene_grad``
(DESIGN.md sections 4.18, 4.20) is the same frame with gradients to the objects' codes, the network's weights and the objects' poses.

Per chunk of rays: ``ops.scene_pairs`` pairs rays with the boxes they cross (one host read-back: the pair counts), the existing per-ray-bounds
sampler, MLP kernel and inverse-CDF kernel run on the pairs -- the MLP once per object segment with that object's per-call block -- and
``ops.scene_composite`` merges a ray's lists by distance.  The second level's draws come from the MERGED weights, so parts hidden behind
another object get few fine samples.

An object may carry an occupancy grid in its own frame: its samples in empty cells get zero density and skip the MLP.

A vanilla ``NeRF`` may stand behind the objects as the static backdrop (``SceneBackground``): one more sample list
per ray, in world coordinates, merged with the objects' by ``ops.scene_composite_lists``.  ``render_scene_background_grad`` (DESIGN.md
section 4.22) is that frame with gradients: to the objects' codes and poses, the scene network's weights and the backdrop's own."""
from __future__ import annotations

import torch

from . import ops

_LATENT_WIDTHS = dict(ops._LATENT_KEYS)


class SceneObject:
    """One placed object: ``latents`` {"density" (1, 128), "color" (1, 128), "articulation" (1, 32)} as ``NeRF_AE_Art.forward`` takes them,
    ``pose`` the (3, 4) rigid object-to-world matrix [R | c] (orthonormal R, det > 0: no scale), ``box`` the axis-aligned box in the
    object's frame (a side length, or (lo, hi): ``ops._box3``), ``grid`` an optional ``ops.OccupancyGrid`` built under the same latents in the
    object's frame (``occupancy.build_occupancy``).  The grid's extent must contain the box: a sample outside the grid counts as empty, so
    the part of a box that sticks out of it would be silently cut away.

    ``pose`` is validated and kept as a detached fp32 host copy (``ob.pose``), which every kernel reads.  A pose TENSOR that carries autograd
    history (a leaf that requires grad, or the result of ``ops.apply_pose_correction`` on one) is kept beside it as ``ob.pose_tensor``
    (None otherwise): ``render_scene_grad`` hands the pose's gradient back to it.  The copy is taken here: build the
    object again after changing the tensor's values."""

    def __init__(self, latents: dict, pose, box, grid=None):
        if not isinstance(latents, dict) or set(latents) != set(_LATENT_WIDTHS):
            raise ValueError(f"SceneObject: latents needs exactly the keys {sorted(_LATENT_WIDTHS)}")
        for key, width in _LATENT_WIDTHS.items():
            if not isinstance(latents[key], torch.Tensor) or latents[key].numel() != width:
                raise ValueError(f"SceneObject: latents[{key!r}] must be a tensor of {width} values")
        self.latents = latents
        self.pose = ops.check_pose(pose, "SceneObject: pose")
        self.pose_tensor = pose if isinstance(pose, torch.Tensor) and pose.requires_grad else None
        lo, hi = ops._box3(box)      # raises for a malformed box
        self.box = box
        if grid is not None:
            if not isinstance(grid, ops.OccupancyGrid):
                raise TypeError(f"SceneObject: grid must be an ops.OccupancyGrid (occupancy.build_occupancy) or None, got {type(grid)}")
            g_lo = grid.lo
            g_hi = grid.lo + torch.tensor(grid.cells, dtype=torch.float32) * grid.step      # multiply, then add: the last grid point
            b_lo, b_hi = torch.tensor(list(lo), dtype=torch.float32), torch.tensor(list(hi), dtype=torch.float32)
            if not bool(((g_lo <= b_lo) & (b_hi <= g_hi)).all()):
                raise ValueError(f"SceneObject: the grid spans {g_lo.tolist()} .. {g_hi.tolist()} and does not contain the box "
                                 f"{b_lo.tolist()} .. {b_hi.tolist()}: samples outside the grid count as empty, so that part of the box would "
                                 "be cut away; build the grid over bounds that enclose the box")
            if not grid.bits.is_cuda:
                raise ValueError(f"SceneObject: the grid is on {grid.bits.device}; it must be on a cuda (ROCm) device")
        self.grid = grid


class SceneBackground:
    """The static backdrop of a scene: a vanilla ``NeRF`` in WORLD coordinates that every ray samples between
    ``near`` and ``far`` (numbers, or per-ray (N,) / (N, 1) tensors: 0 <= near < far, finite) behind and between the objects.  It is one more
    sample list of the merged composite, read with relu / sigmoid and the reference's open last interval (helper.py:163-167), so it is opaque
    where its last sample has density.  Inference only.  The network must run on the fused kernels at the default geometry and encoding
    degrees (the stage call ``ops.mlp_fwd`` serves no other), condition on the view direction, and take no density noise; its sample counts
    are the scene model's, not its own."""

    def __init__(self, model, near, far):
        from .models.vanilla_nerf.model import NeRF

        if not isinstance(model, NeRF):
            raise TypeError(f"SceneBackground: the backdrop is a vanilla NeRF (models.vanilla_nerf.model.NeRF), got {type(model)}")
        for mlp in (model.coarse_mlp, model.fine_mlp):
            if model._general or not mlp.geometry.is_default:
                raise NotImplementedError("SceneBackground: the backdrop runs on the fused kernels' stage call (ops.mlp_fwd), which serves the default "
                                          "NeRFMLP geometry with encoding degrees (0, 10, 4) only; this network's geometry is served by the layer-wise "
                                          "engine or by padded encoding slots")
        if not model.use_viewdirs:
            raise NotImplementedError("SceneBackground: the fused kernels always condition the colour on the view direction (use_viewdirs=True)")
        if model.noise_std > 0:
            raise NotImplementedError("SceneBackground: the backdrop takes no density noise (noise_std > 0)")
        if model.num_levels not in (1, 2):
            raise NotImplementedError("SceneBackground: the backdrop runs one or two levels")
        self.model = model
        self.near, self.far = self._bound(near, "near"), self._bound(far, "far")
        lo, hi = (x if isinstance(x, torch.Tensor) else torch.tensor(x) for x in (self.near, self.far))
        if lo.dim() and hi.dim() and lo.numel() != hi.numel():
            raise ValueError(f"SceneBackground: per-ray near and far must hold the same number of rays, got {lo.numel()} and {hi.numel()}")
        if not bool((torch.isfinite(lo).all() & torch.isfinite(hi).all() & (lo >= 0).all() & (lo < hi).all()).item()):
            raise ValueError("SceneBackground: near / far must be finite with 0 <= near < far on every ray")

    @staticmethod
    def _bound(x, name):
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float32:
                raise TypeError(f"SceneBackground: a per-ray {name} must be float32, got {x.dtype}")
            return x.detach().reshape(-1)
        return float(x)

    def bounds(self, c0: int, c1: int, n_total: int):
        """near / far of the rays c0 .. c1 - 1 of a frame of n_total rays"""
        out = []
        for x, name in ((self.near, "near"), (self.far, "far")):
            if isinstance(x, torch.Tensor):
                if x.numel() != n_total:
                    raise ValueError(f"SceneBackground: per-ray {name} holds {x.numel()} values, the frame {n_total} rays")
                x = x[c0:c1]
            out.append(x)
        return out


def _check_objects(objects, background=None) -> list:
    objects = list(objects)
    if background is not None:
        if not isinstance(background, SceneBackground):
            raise TypeError(f"render_scene: background must be a scene.SceneBackground or None, got {type(background)}")
        if len(objects) + 1 > ops.SCENE_MAX_OBJECTS:
            raise ValueError(f"a scene with a background holds 0 to {ops.SCENE_MAX_OBJECTS - 1} objects (the backdrop is the merged composite's "
                             f"{ops.SCENE_MAX_OBJECTS}th list), got {len(objects)}")
    elif not 1 <= len(objects) <= ops.SCENE_MAX_OBJECTS:
        raise ValueError(f"a scene holds 1 to {ops.SCENE_MAX_OBJECTS} objects, got {len(objects)}")
    for ob in objects:
        if not isinstance(ob, SceneObject):
            raise TypeError(f"render_scene: expected SceneObject instances, got {type(ob)}")
    return objects


def _check_background_levels(model, K, background):
    """The checks a scene with a backdrop makes beyond _check_objects: matching level counts, (K + 1) * S merged samples within the limit"""
    bg = background.model
    if bg.num_levels != model.num_levels:
        raise ValueError(f"the backdrop runs {bg.num_levels} level(s), the scene model {model.num_levels}: they must match (the backdrop is sampled "
                         "with the scene model's sample counts, level by level)")
    for level in range(model.num_levels):
        S = model._opts.S(level)
        if (K + 1) * S > ops.SCENE_MAX_MERGED:
            raise ValueError(f"{K} objects and a backdrop of {S} samples each at level {level} are {(K + 1) * S} merged samples per ray; the merged "
                             f"composite holds at most {ops.SCENE_MAX_MERGED}: use fewer samples or fewer objects")


def _render_scene_background(model, objects, rays, white_bkgd, chunk, want_occupied, background):
    """render_scene with a backdrop: the objects' pairs as ever (none for an empty object list), extended by the
    backdrop's list; ONE sampler call for all rows; per level the objects' segments through the articulated MLP stage into the first P rows
    of one raw buffer and the backdrop's n rows through ops.mlp_fwd into the last n; the merge is ops.scene_composite_lists, and the fine t
    of all lists alike comes from the merged weights."""
    bg = background.model
    K = len(objects)
    _check_background_levels(model, K, background)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    n = o.shape[0]
    mlps = [model.coarse_mlp, model.fine_mlp][: model.num_levels]
    packed = [m.packed() for m in mlps]
    bg_packed = [m.packed() for m in [bg.coarse_mlp, bg.fine_mlp][: model.num_levels]]
    smalls = [[ops.art_prepare(dict(m.named_parameters()), ob.latents, out=None, degrees=m.degrees) for ob in objects] for m in mlps]
    lists = [ops.SceneList(ops.ACT_ARTICULATED, False, model._opts)] * K + [ops.SceneList(ops.ACT_VANILLA, True)]
    parts = [[] for _ in mlps]
    grids = [ob.grid for ob in objects]
    with_occ = any(g is not None for g in grids)
    occupied = [torch.zeros((K,), dtype=torch.int64, device=o.device) for _ in mlps] if want_occupied and with_occ else None
    host_counts = [[0] * K for _ in mlps] if want_occupied and not with_occ else None
    for c0 in range(0, max(n, 1), chunk):
        co, cd, cv = o[c0: c0 + chunk], d[c0: c0 + chunk], v[c0: c0 + chunk]
        cn = co.shape[0]
        near, far = background.bounds(c0, c0 + cn, n)
        obj_pairs = ops.scene_pairs(co, cd, cv, objects) if K else ops.ScenePairs.without_objects(cn, co.device)
        P = obj_pairs.P
        pairs = obj_pairs.with_background(co, cd, cv, near, far)
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False, lindisp=model.lindisp)
        for level in range(len(mlps)):
            last = level == len(mlps) - 1
            raw = torch.empty((pairs.P, t.shape[1], 4), dtype=torch.float32, device=t.device)
            if K and with_occ:
                _, occ = ops.scene_art_mlp_fwd_occ(packed[level], smalls[level], grids, obj_pairs, t[:P], out=raw[:P])
                if want_occupied:
                    occupied[level] += occ
            elif K:
                ops.scene_art_mlp_fwd(packed[level], smalls[level], obj_pairs, t[:P], out=raw[:P])
                if want_occupied:
                    host_counts[level] = [a + c * t.shape[1] for a, c in zip(host_counts[level], obj_pairs.counts)]
            if cn:
                ops.mlp_fwd(bg_packed[level], co, cd, cv, t[P:], out=raw[P:])
            rgb, acc, depth, obj_acc, weights = ops.scene_composite_lists(raw, t, pairs, cd, white_bkgd, lists, want_weights=not last)
            parts[level].append((rgb, acc, depth, obj_acc))
            if not last:
                t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    levels = [tuple(torch.cat([p[i] for p in lvl]) for i in range(4)) for lvl in parts]
    if host_counts is not None:
        occupied = [torch.tensor(c, dtype=torch.int64).to(o.device) for c in host_counts]
    return (levels, occupied) if want_occupied else levels


def render_scene(model, objects, rays, white_bkgd, chunk: int = 65536, randomized: bool = False, want_occupied: bool = False, background=None):
    """``model``: a NeRF_AE_Art; ``objects``: 1 to 16 SceneObject; ``rays``: {"rays_o", "rays_d", "viewdirs"} (N, 3) in WORLD coordinates.
    -> ``[(rgb (N, 3), acc (N,), depth (N,), obj_acc (N, K))]`` per level, the shape ``forward`` returns with the per-object opacity appended.
    A ray that meets no box returns the background (rgb 1 or 0, acc = depth = 0).
    When an object carries a grid, the levels' MLP stage is ``ops.scene_art_mlp_fwd_occ``; without grids it is ``ops.scene_art_mlp_fwd``, as
    ever.  ``want_occupied``: -> ``(levels, occupied)`` with ``occupied[level]`` the (K,) int64 device tensor of the samples of each object
    that ran through the MLP (all of an object's samples when it has no grid).
    ``background`` (a SceneBackground): a vanilla NeRF behind and between the objects.  Then ``objects`` holds 0 to
    15 objects, ``obj_acc`` is (N, K + 1) with the backdrop's opacity in the last column, ``occupied`` still counts the K objects only, and
    the flat colour shows only where the backdrop is transparent.  None: the calls and the bits of a scene without one."""
    if randomized:
        raise ValueError("scene rendering is inference only: randomized=True is refused")
    if torch.is_grad_enabled():
        raise RuntimeError("scene rendering is inference only: call it under torch.no_grad()")
    if model.noise_std > 0:
        raise NotImplementedError("scene rendering takes no density noise (noise_std > 0)")
    if model.num_levels not in (1, 2):
        raise NotImplementedError("scene rendering runs one or two levels")
    objects = _check_objects(objects, background)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    if background is not None:
        return _render_scene_background(model, objects, rays, white_bkgd, chunk, want_occupied, background)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    n = o.shape[0]
    mlps = [model.coarse_mlp, model.fine_mlp][: model.num_levels]
    packed = [m.packed() for m in mlps]
    # one per-call block per (level, object) and frame; NOT NeRFMLP.prepared, which hands out one cached buffer
    smalls = [[ops.art_prepare(dict(m.named_parameters()), ob.latents, out=None, degrees=m.degrees) for ob in objects] for m in mlps]
    opts = model._opts
    parts = [[] for _ in mlps]
    grids = [ob.grid for ob in objects]
    with_occ = any(g is not None for g in grids)
    # per level: the device tallies of the occupancy call, or -- without grids -- the host's own counts, uploaded once at the end
    occupied = [torch.zeros((len(objects),), dtype=torch.int64, device=o.device) for _ in mlps] if want_occupied and with_occ else None
    host_counts = [[0] * len(objects) for _ in mlps] if want_occupied and not with_occ else None
    for c0 in range(0, max(n, 1), chunk):
        co, cd, cv = o[c0: c0 + chunk], d[c0: c0 + chunk], v[c0: c0 + chunk]
        pairs = ops.scene_pairs(co, cd, cv, objects)
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False, lindisp=model.lindisp)
        for level in range(len(mlps)):
            last = level == len(mlps) - 1
            if with_occ:
                raw, occ = ops.scene_art_mlp_fwd_occ(packed[level], smalls[level], grids, pairs, t)
                if want_occupied:
                    occupied[level] += occ
            else:
                raw = ops.scene_art_mlp_fwd(packed[level], smalls[level], pairs, t)
                if want_occupied:
                    host_counts[level] = [a + c * t.shape[1] for a, c in zip(host_counts[level], pairs.counts)]
            rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, cd, white_bkgd, opts=opts, want_weights=not last)
            parts[level].append((rgb, acc, depth, obj_acc))
            if not last:
                t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    levels = [tuple(torch.cat([p[i] for p in lvl]) for i in range(4)) for lvl in parts]
    if host_counts is not None:
        occupied = [torch.tensor(c, dtype=torch.int64).to(o.device) for c in host_counts]
    return (levels, occupied) if want_occupied else levels


def render_scene_grad(model, objects, rays, white_bkgd, randomized: bool = False, background=None):
    """``render_scene`` with autograd history: -> ``[(rgb (N, 3), acc (N,), depth (N,), obj_acc (N, K))]`` per level,
    the bits ``render_scene`` returns, whose gradients reach every object's three codes (``SceneObject.latents`` may hold leaf tensors that
    require grad), the network's weights and -- for every object whose ``pose_tensor`` is set (``SceneObject``) -- the object's (3, 4) pose
    (the plain derivative with respect to its 12 entries; differentiate ``ops.apply_pose_correction`` for a
    tangent-space step; the levels' contributions add).  The pairs' existence, near / far, the sample positions of both levels (the fine
    draws come from the merged coarse weights, detached: helper.py:249), the world direction's norm and the world rays are data: no
    gradient reaches a ray or the camera.  Without a pose tensor the path and the bits are those of section 4.18.

    One chunk: the activation planes of every pair (13.8 KB per sample) live until the backward, and are released by it -- a second backward
    through the same forward raises.  Dense only: an object carrying a grid is refused (the training forward has no gather instance).  A
    frozen network still pays the full weight-gradient stage, unless a pose tensor is present and no code and no weight requires grad: a
    pose-only backward launches no weight-gradient kernel.  ``background``: refused here -- the frame with a backdrop and gradients is
    ``render_scene_background_grad``."""
    from .autograd import RenderLevelScene, RenderLevelScenePoses

    if background is not None:
        raise NotImplementedError("scene gradients take no background: with a backdrop (scene.SceneBackground) this function is inference only; "
                                  "the gradients through a scene with a backdrop are scene.render_scene_background_grad's")
    if randomized:
        raise ValueError("scene gradients sample without randomness: randomized=True is refused")
    if model.noise_std > 0:
        raise NotImplementedError("scene gradients take no density noise (noise_std > 0)")
    if model.num_levels not in (1, 2):
        raise NotImplementedError("scene gradients run one or two levels")
    objects = _check_objects(objects)
    for k, ob in enumerate(objects):
        if ob.grid is not None:
            raise NotImplementedError(f"scene gradients are dense only: object {k} carries an occupancy grid")
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    mlps = [model.coarse_mlp, model.fine_mlp][: model.num_levels]
    codes = [ob.latents[key] for ob in objects for key in _LATENT_WIDTHS]
    with torch.no_grad():
        pairs = ops.scene_pairs(o, d, v, objects)
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False, lindisp=model.lindisp)
    with_poses = any(ob.pose_tensor is not None for ob in objects)
    poses = [ob.pose_tensor if ob.pose_tensor is not None else ob.pose for ob in objects]
    levels = []
    for level, mlp in enumerate(mlps):
        # fresh streams: the backward reads them again, and a later forward must not overwrite what this graph still needs
        if with_poses:
            rgb, acc, depth, obj_acc, weights = RenderLevelScenePoses.apply(pairs, t, o, d, v, objects, bool(white_bkgd), model._opts, mlp.packed(True),
                                                                            mlp.packed_bwd(True), mlp.degrees, *poses, *codes, *mlp.ordered_params())
        else:
            rgb, acc, depth, obj_acc, weights = RenderLevelScene.apply(pairs, t, d, bool(white_bkgd), model._opts, mlp.packed(True), mlp.packed_bwd(True),
                                                                       mlp.degrees, *codes, *mlp.ordered_params())
        levels.append((rgb, acc, depth, obj_acc))
        if level + 1 < len(mlps):
            with torch.no_grad():
                t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return levels


def render_scene_background_grad(model, objects, rays, white_bkgd, background, randomized: bool = False):
    """``render_scene(..., background=background)`` with autograd history: -> ``[(rgb (N, 3), acc (N,), depth (N,),
    obj_acc (N, K + 1))]`` per level, the bits ``render_scene`` returns with that backdrop, whose gradients reach every object's three codes,
    the scene network's weights, the pose of every object whose ``pose_tensor`` is set (as ``render_scene_grad``) and the backdrop network's
    parameters.  ``objects`` may be empty: the backdrop alone through the lists path.  The pairs' existence, near / far of objects and
    backdrop, the sample positions of both levels (the fine draws of ALL lists come from the merged coarse weights, detached), the world
    rays -- hence the backdrop's rays -- and the world direction's norm are data.

    One chunk, dense objects only, no noise, one or two levels, as ``render_scene_grad``; a second backward through the same forward raises.
    Only what is asked is paid for: no weight-gradient kernel of the scene network when no code and none of its weights requires grad, and a
    backdrop none of whose parameters requires grad runs the plane-free forward (every one of the N rays carries S backdrop samples) and
    launches neither its backward chain nor its weight-gradient kernel."""
    from .autograd import RenderLevelSceneLists

    if randomized:
        raise ValueError("scene gradients sample without randomness: randomized=True is refused")
    if model.noise_std > 0:
        raise NotImplementedError("scene gradients take no density noise (noise_std > 0)")
    if model.num_levels not in (1, 2):
        raise NotImplementedError("scene gradients run one or two levels")
    if background is None:
        raise TypeError("render_scene_background_grad: background must be a scene.SceneBackground (without one, call render_scene_grad)")
    objects = _check_objects(objects, background)
    for k, ob in enumerate(objects):
        if ob.grid is not None:
            raise NotImplementedError(f"scene gradients are dense only: object {k} carries an occupancy grid")
    K = len(objects)
    _check_background_levels(model, K, background)
    bg = background.model
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    n = o.shape[0]
    mlps = [model.coarse_mlp, model.fine_mlp][: model.num_levels]
    bg_mlps = [bg.coarse_mlp, bg.fine_mlp][: model.num_levels]
    codes = [ob.latents[key] for ob in objects for key in _LATENT_WIDTHS]
    poses = [ob.pose_tensor if ob.pose_tensor is not None else ob.pose for ob in objects]
    with torch.no_grad():
        near, far = background.bounds(0, n, n)
        obj_pairs = ops.scene_pairs(o, d, v, objects) if K else ops.ScenePairs.without_objects(n, o.device)
        pairs = obj_pairs.with_background(o, d, v, near, far)
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False, lindisp=model.lindisp)
    levels = []
    for level, (mlp, bg_mlp) in enumerate(zip(mlps, bg_mlps)):
        # fresh streams: the backward reads them again, and a later forward must not overwrite what this graph still needs
        rgb, acc, depth, obj_acc, weights = RenderLevelSceneLists.apply(obj_pairs, t, o, d, v, objects, bool(white_bkgd), model._opts, mlp.packed(True),
                                                                        mlp.packed_bwd(True), mlp.degrees, pairs, bg_mlp.packed(True),
                                                                        bg_mlp.packed_bwd(True), *poses, *codes, *mlp.ordered_params(),
                                                                        *bg_mlp.ordered_params())
        levels.append((rgb, acc, depth, obj_acc))
        if level + 1 < len(mlps):
            with torch.no_grad():
                t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return levels
