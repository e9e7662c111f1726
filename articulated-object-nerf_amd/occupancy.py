"""Occupancy-grid accelerated inference: a bitfield of the cells of a trained field that may hold matter, built once
from the network's density (ops.density_grid, then ops.occupancy_grid), and renders that skip every sample in an empty cell -- the MLP never
runs on it and it gets zero density.  Inference only; the default render path is unchanged.

    from aon_amd.occupancy import build_occupancy, render_image
    grid = build_occupancy(nerf, bounds=(-1.2, 1.2))                                  # vanilla NeRF, 128^3 cells
    out = render_image(nerf, c2w, 480, 640, focal, 2.0, 6.0, grid)                    # {"rgb": (H, W, 3), ..., "occupied": [coarse, fine]}
    grid = build_occupancy(art_nerf, (-1.2, 1.2), latents=latents)                   # NeRF_AE_Art at one articulation state

The box must enclose the object: every sample outside it counts as empty.
"""
from __future__ import annotations

import torch

from . import ops


def _is_articulated(model) -> bool:
    from .models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    return isinstance(model, NeRF_AE_Art)


@torch.no_grad()
def build_occupancy(model, bounds, resolution=128, threshold: float = 0.01, dilate: int = 1, latents: dict | None = None,
                    level: str = "fine") -> ops.OccupancyGrid:
    """Occupancy grid of `resolution` cells per axis (an int or 3 ints) over bounds = (lo, hi) from the activated density of the `level`
    network at the (resolution + 1) grid points per axis (model.density_grid).  A cell is occupied iff one of its corners is above
    `threshold` (or NaN), then the grid is dilated by `dilate` cells.  `latents` (the code library's "density", "color", "articulation"
    rows) are required by NeRF_AE_Art: its density depends on them.  The default uses the fine network for both render levels."""
    lo, hi = bounds
    cells = ops._dims3(resolution)
    dims = [c + 1 for c in cells]
    if _is_articulated(model):
        if latents is None:
            raise ValueError("build_occupancy: NeRF_AE_Art needs latents (its density depends on them)")
        dens = model.density_grid((lo, hi), dims, latents, level=level)
    else:
        dens = model.density_grid((lo, hi), dims, level=level)
    return ops.occupancy_grid(dens, lo, hi, threshold, dilate)


@torch.no_grad()
def render_image(model, c2w, H: int, W: int, focal: float, near: float, far: float, grid: ops.OccupancyGrid | None, latents: dict | None = None,
                 chunk: int = ops.MAX_CHUNK_RAYS, white_bkgd: bool = True, early_stop: float | None = None, round_samples: int | None = None,
                 ray_bounds: bool = False, box=None) -> dict:
    """One H x W view through the occupancy path (deterministic sampling, both levels of the model) -> {"rgb": (H, W, 3), "acc": (H, W),
    "depth": (H, W) of the last level, "occupied": [samples run through the MLP per level] (python ints), "samples": [n * S per level]}.
    ``early_stop`` (eps in [0, 1)): rays stop once their transmittance has fallen to eps, in rounds of
    ``round_samples`` samples (None: ops.DEFAULT_ROUND_SAMPLES); the dict gains "stop", the (H, W) int32 map of the last level's stop
    index (S: the ray ran to its end) -- a heat map of the frame's cost.  `grid` may then be None.
    ``ray_bounds``: per-ray near / far from the rays' intersection with the grid's box (lo, lo + cells * step) -- or
    with ``box`` (a side length, or (lo, hi)) when there is no grid -- computed once over the whole image, and the rays that miss it skipped
    (``ray_live``); the scalar `near` / `far` are then ignored.  The dict gains "live", the number of live rays."""
    if ray_bounds:
        if box is None:
            if grid is None:
                raise ValueError("render_image: ray_bounds without a grid needs box=")
            box = (grid.lo.tolist(), (grid.lo + torch.tensor(grid.cells, dtype=torch.float32) * grid.step).tolist())   # multiply, then add: the last grid point
    elif grid is None and early_stop is None:
        raise ValueError("render_image: needs a grid, early_stop, ray_bounds, or a combination")
    dev = grid.device if grid is not None else next(model.parameters()).device
    rays_o, viewdirs = ops.raygen(c2w, H, W, focal, device=dev)
    n = H * W
    art = _is_articulated(model)
    if art and latents is None:
        raise ValueError("render_image: NeRF_AE_Art needs latents")
    L = model.num_levels
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    occupied = torch.zeros(2, dtype=torch.int64, device=dev)
    pc = model.coarse_mlp.packed()
    pf = model.fine_mlp.packed() if L == 2 else None
    if art:
        sc = model.coarse_mlp.prepared(latents)
        sf = model.fine_mlp.prepared(latents) if L == 2 else None
    stop = torch.empty((n,), dtype=torch.int32, device=dev) if early_stop is not None else None
    limits = ops.ray_limits(rays_o, viewdirs, box) if ray_bounds else None
    for b in range(0, n, chunk):
        e = min(n, b + chunk)
        o, v = rays_o[b:e], viewdirs[b:e]
        if limits is not None:
            pn, pfar, live = (x[b:e] for x in limits)
            if art:
                outs, occ, st = ops.art_render_fwd_stop(pc, sc, pf, sf, o, v, v, pn, pfar, white_bkgd, grid, early_stop or 0.0, round_samples, L,
                                                        opts=model._opts, ray_live=live)
            else:
                outs, occ, st = ops.render_fwd_stop(pc, pf, o, v, v, pn, pfar, white_bkgd, grid, early_stop or 0.0, round_samples, L,
                                                    opts=model._opts, ray_live=live)
            if stop is not None:
                stop[b:e] = st[:, L - 1]
        elif early_stop is not None:
            if art:
                outs, occ, st = ops.art_render_fwd_stop(pc, sc, pf, sf, o, v, v, near, far, white_bkgd, grid, early_stop, round_samples, L,
                                                        opts=model._opts)
            else:
                outs, occ, st = ops.render_fwd_stop(pc, pf, o, v, v, near, far, white_bkgd, grid, early_stop, round_samples, L, opts=model._opts)
            stop[b:e] = st[:, L - 1]
        elif art:
            outs, occ = ops.art_render_fwd_occ(pc, sc, pf, sf, o, v, v, near, far, white_bkgd, grid, L, opts=model._opts)
        else:
            outs, occ = ops.render_fwd_occ(pc, pf, o, v, v, near, far, white_bkgd, grid, L, opts=model._opts)
        rgb[b:e], acc[b:e], depth[b:e] = outs[-1]
        occupied += occ
    S = [model._opts.Sc, model._opts.Sf]
    out = {"rgb": rgb.view(H, W, 3), "acc": acc.view(H, W), "depth": depth.view(H, W), "occupied": [int(x) for x in occupied.tolist()][:L],
           "samples": [n * S[lvl] for lvl in range(L)]}
    if stop is not None:
        out["stop"] = stop.view(H, W)
    if limits is not None:
        out["live"] = int(limits[2].sum())
    return out
