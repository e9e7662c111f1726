"""Scenes of several posed articulated objects in one frame: one ``NeRF_AE_Art`` and K <= 16 objects, each with its
own codes, rigid object-to-world pose and box, rendered with correct mutual occlusion -- the approach of Neural Scene Graphs (Ost et al.): a
ray-box test per object, samples inside each box, one sorted merge along the ray.  ``render_scene`` is inference only; ``render_scene_grad``
(DESIGN.md sections 4.18, 4.20) is the same frame with gradients to the objects' codes, the network's weights and the objects' poses.

Per chunk of rays: ``ops.scene_pairs`` pairs rays with the boxes they cross (one host read-back: the pair counts), the existing per-ray-bounds
sampler, MLP kernel and inverse-CDF kernel run on the pairs -- the MLP once per object segment with that object's per-call block -- and
``ops.scene_composite`` merges a ray's lists by distance.  The second level's draws come from the MERGED weights, so parts hidden behind
another object get few fine samples.

An object may carry an occupancy grid in its own frame: its samples in empty cells get zero density and skip the MLP."""
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


def _check_objects(objects) -> list:
    objects = list(objects)
    if not 1 <= len(objects) <= ops.SCENE_MAX_OBJECTS:
        raise ValueError(f"a scene holds 1 to {ops.SCENE_MAX_OBJECTS} objects, got {len(objects)}")
    for ob in objects:
        if not isinstance(ob, SceneObject):
            raise TypeError(f"render_scene: expected SceneObject instances, got {type(ob)}")
    return objects


def render_scene(model, objects, rays, white_bkgd, chunk: int = 65536, randomized: bool = False, want_occupied: bool = False):
    """``model``: a NeRF_AE_Art; ``objects``: 1 to 16 SceneObject; ``rays``: {"rays_o", "rays_d", "viewdirs"} (N, 3) in WORLD coordinates.
    -> ``[(rgb (N, 3), acc (N,), depth (N,), obj_acc (N, K))]`` per level, the shape ``forward`` returns with the per-object opacity appended.
    A ray that meets no box returns the background (rgb 1 or 0, acc = depth = 0).
    When an object carries a grid, the levels' MLP stage is ``ops.scene_art_mlp_fwd_occ``; without grids it is ``ops.scene_art_mlp_fwd``, as
    ever.  ``want_occupied``: -> ``(levels, occupied)`` with ``occupied[level]`` the (K,) int64 device tensor of the samples of each object
    that ran through the MLP (all of an object's samples when it has no grid)."""
    if randomized:
        raise ValueError("scene rendering is inference only: randomized=True is refused")
    if torch.is_grad_enabled():
        raise RuntimeError("scene rendering is inference only: call it under torch.no_grad()")
    if model.noise_std > 0:
        raise NotImplementedError("scene rendering takes no density noise (noise_std > 0)")
    if model.num_levels not in (1, 2):
        raise NotImplementedError("scene rendering runs one or two levels")
    objects = _check_objects(objects)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
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


def render_scene_grad(model, objects, rays, white_bkgd, randomized: bool = False):
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
    pose-only backward launches no weight-gradient kernel."""
    from .autograd import RenderLevelScene, RenderLevelScenePoses

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
