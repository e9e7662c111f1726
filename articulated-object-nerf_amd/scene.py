"""Scenes of several posed articulated objects in one frame: one ``NeRF_AE_Art`` and K <= 16 objects, each with its
own codes, rigid object-to-world pose and box, rendered with correct mutual occlusion -- the approach of Neural Scene Graphs (Ost et al.): a
ray-box test per object, samples inside each box, one sorted merge along the ray.  Inference only.

Per chunk of rays: ``ops.scene_pairs`` pairs rays with the boxes they cross (one host read-back: the pair counts), the existing per-ray-bounds
sampler, MLP kernel and inverse-CDF kernel run on the pairs -- the MLP once per object segment with that object's per-call block -- and
``ops.scene_composite`` merges a ray's lists by distance.  The second level's draws come from the MERGED weights, so parts hidden behind
another object get few fine samples."""
from __future__ import annotations

import torch

from . import ops

_LATENT_WIDTHS = dict(ops._LATENT_KEYS)


class SceneObject:
    """One placed object: ``latents`` {"density" (1, 128), "color" (1, 128), "articulation" (1, 32)} as ``NeRF_AE_Art.forward`` takes them,
    ``pose`` the (3, 4) rigid object-to-world matrix [R | c] (orthonormal R, det > 0: no scale), ``box`` the axis-aligned box in the
    object's frame (a side length, or (lo, hi): ``ops._box3``)."""

    def __init__(self, latents: dict, pose, box):
        if not isinstance(latents, dict) or set(latents) != set(_LATENT_WIDTHS):
            raise ValueError(f"SceneObject: latents needs exactly the keys {sorted(_LATENT_WIDTHS)}")
        for key, width in _LATENT_WIDTHS.items():
            if not isinstance(latents[key], torch.Tensor) or latents[key].numel() != width:
                raise ValueError(f"SceneObject: latents[{key!r}] must be a tensor of {width} values")
        self.latents = latents
        self.pose = ops.check_pose(pose, "SceneObject: pose")
        ops._box3(box)      # raises for a malformed box
        self.box = box


def _check_objects(objects) -> list:
    objects = list(objects)
    if not 1 <= len(objects) <= ops.SCENE_MAX_OBJECTS:
        raise ValueError(f"a scene holds 1 to {ops.SCENE_MAX_OBJECTS} objects, got {len(objects)}")
    for ob in objects:
        if not isinstance(ob, SceneObject):
            raise TypeError(f"render_scene: expected SceneObject instances, got {type(ob)}")
    return objects


def render_scene(model, objects, rays, white_bkgd, chunk: int = 65536, randomized: bool = False) -> list:
    """``model``: a NeRF_AE_Art; ``objects``: 1 to 16 SceneObject; ``rays``: {"rays_o", "rays_d", "viewdirs"} (N, 3) in WORLD coordinates.
    -> ``[(rgb (N, 3), acc (N,), depth (N,), obj_acc (N, K))]`` per level, the shape ``forward`` returns with the per-object opacity appended.
    A ray that meets no box returns the background (rgb 1 or 0, acc = depth = 0)."""
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
    for c0 in range(0, max(n, 1), chunk):
        co, cd, cv = o[c0: c0 + chunk], d[c0: c0 + chunk], v[c0: c0 + chunk]
        pairs = ops.scene_pairs(co, cd, cv, objects)
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False, lindisp=model.lindisp)
        for level in range(len(mlps)):
            last = level == len(mlps) - 1
            raw = ops.scene_art_mlp_fwd(packed[level], smalls[level], pairs, t)
            rgb, acc, depth, obj_acc, weights = ops.scene_composite(raw, t, pairs, cd, white_bkgd, opts=opts, want_weights=not last)
            parts[level].append((rgb, acc, depth, obj_acc))
            if not last:
                t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    return [tuple(torch.cat([p[i] for p in lvl]) for i in range(4)) for lvl in parts]
