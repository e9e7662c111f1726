"""Mesh extraction from a trained field: the density on a grid (one fused HIP launch, ops.density_grid), marching cubes
on the GPU (ops.marching_cubes), optional per-vertex colour from the full network, and a dependency-free binary PLY writer.

    from aon_amd.mesh import extract_mesh, write_ply
    mesh = extract_mesh(nerf, bounds=(-1.2, 1.2), resolution=256)                       # vanilla NeRF
    mesh = extract_mesh(art_nerf, (-1, 1), 256, latents=latents, color=True)            # NeRF_AE_Art at one articulation state
    write_ply("mesh.ply", mesh)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops

# Default iso levels.  Vanilla: nerf_pl's practice for meshes, sigma = 50 on the relu density.  Articulated: the softplus(raw - 1) density of
# NeRF_AE_Art has the same units (it multiplies the same sample distances in the compositing), but is never exactly zero and its empty
# space sits near softplus(-1) ~ 0.31 rather than at 0; 20 -- nerf_pl's default sigma_threshold -- keeps the surface on the object and off
# the thin low-density haze such models leave in free space.  Both are starting points: tune them per scene.
DEFAULT_THRESHOLD_VANILLA = 50.0
DEFAULT_THRESHOLD_ARTICULATED = 20.0


@dataclass
class Mesh:
    verts: torch.Tensor                    # (V, 3) fp32
    faces: torch.Tensor                    # (F, 3) int32, normals outward (from high density to low)
    colors: torch.Tensor | None = None     # (V, 3) fp32 in [0, 1], or None


def _bounds(bounds):
    lo, hi = bounds
    return ops._vec3(lo, "bounds[0]"), ops._vec3(hi, "bounds[1]")


def _is_articulated(model) -> bool:
    from .models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    return isinstance(model, NeRF_AE_Art)


def extract_mesh(model, bounds, resolution=256, threshold: float | None = None, latents: dict | None = None, level: str = "fine",
                 color: bool = False, chunk: int = 1 << 18) -> Mesh:
    """Iso-surface `density == threshold` of `model` (a NeRF, or a NeRF_AE_Art with its `latents`) over the box bounds = (lo, hi) sampled
    with `resolution` points per axis.  threshold None: DEFAULT_THRESHOLD_VANILLA / DEFAULT_THRESHOLD_ARTICULATED.  color: each vertex gets
    the `level` network's rgb seen by a camera looking at the surface from outside -- view direction +grad(sigma)/|grad(sigma)|, the density
    gradient by central differences on the grid, interpolated trilinearly to the vertex -- through the existing point entries
    (mlp_fwd_enc / the layer-wise engine, art_mlp_fwd_pos), `chunk` vertices at a time."""
    art = _is_articulated(model)
    if art and latents is None:
        raise ValueError("extract_mesh: an articulated model needs its latents")
    lo, hi = _bounds(bounds)
    dims = ops._dims3(resolution)
    if threshold is None:
        threshold = DEFAULT_THRESHOLD_ARTICULATED if art else DEFAULT_THRESHOLD_VANILLA
    grid = model.density_grid((lo, hi), dims, latents, level) if art else model.density_grid((lo, hi), dims, level)
    verts, faces = ops.marching_cubes(grid, float(threshold), lo, hi)
    colors = vertex_colors(model, grid, verts, lo, hi, latents, level, chunk) if color else None
    return Mesh(verts, faces, colors)


def _trilinear(field: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """field (nx, ny, nz, C) at fractional grid indices u (V, 3) -> (V, C)"""
    n = torch.tensor(field.shape[:3], device=u.device)
    i0 = torch.clamp(torch.floor(u).long(), torch.zeros_like(n), n - 2)
    f = (u - i0.to(u.dtype)).clamp(0.0, 1.0)
    out = 0
    for dx in (0, 1):
        wx = f[:, 0] if dx else 1 - f[:, 0]
        for dy in (0, 1):
            wy = f[:, 1] if dy else 1 - f[:, 1]
            for dz in (0, 1):
                wz = f[:, 2] if dz else 1 - f[:, 2]
                out = out + (wx * wy * wz)[:, None] * field[i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz]
    return out


@torch.no_grad()
def vertex_colors(model, grid: torch.Tensor, verts: torch.Tensor, lo, hi, latents=None, level: str = "fine", chunk: int = 1 << 18) -> torch.Tensor:
    art = _is_articulated(model)
    V = verts.shape[0]
    if V == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=verts.device)
    lo32, step = ops.grid_step(list(grid.shape), lo, hi)
    lo32, step = lo32.to(grid.device), step.to(grid.device)
    safe = torch.where(step > 0, step, torch.ones_like(step))
    gx, gy, gz = torch.gradient(grid, spacing=[float(s) for s in safe.tolist()])
    grad = _trilinear(torch.stack([gx, gy, gz], -1), (verts - lo32) / safe)
    norm = grad.norm(dim=-1, keepdim=True)
    d = torch.where(norm > 0, grad / norm.clamp_min(1e-30), torch.tensor([0.0, 0.0, 1.0], device=grad.device)).contiguous()
    mlp = model._level_mlp(level)
    out = torch.empty((V, 3), dtype=torch.float32, device=verts.device)
    for b in range(0, V, chunk):
        e = min(V, b + chunk)
        if art:
            cond = ops.pos_enc(d[b:e], 0, mlp.degrees[2])
            raw_rgb, _ = mlp(verts[b:e, None, :].contiguous(), cond, latents)
            p = model.rgb_padding
            out[b:e] = torch.sigmoid(raw_rgb.reshape(-1, 3)) * (1 + 2 * p) - p
        else:
            enc = ops.pos_enc(verts[b:e, None, :].contiguous(), model.min_deg_point, model.max_deg_point)
            cond = ops.pos_enc(d[b:e], 0, model.deg_view)
            raw_rgb, _ = mlp(enc, cond)
            out[b:e] = torch.sigmoid(raw_rgb.reshape(-1, 3))
    return out.clamp_(0.0, 1.0)


# ---------------------------------------------------------------- PLY (binary little-endian, no third-party dependency)
def write_ply(path, mesh: Mesh) -> None:
    """vertices as float x, y, z (+ uchar red, green, blue when the mesh has colours), faces as a uchar-counted int list"""
    v = mesh.verts.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
    has_c = mesh.colors is not None
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if has_c:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("r", "u1"), ("g", "u1"), ("b", "u1")] if has_c else [])
    vrec = np.empty(len(v), dtype=vdt)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if has_c:
        c = np.clip(np.rint(mesh.colors.detach().cpu().numpy().reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)
        vrec["r"], vrec["g"], vrec["b"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path) -> Mesh:
    """Reads what write_ply writes (binary little-endian, float xyz [+ uchar rgb], triangles) -> Mesh of CPU tensors."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    has_c = "property uchar red" in lines
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("r", "u1"), ("g", "u1"), ("b", "u1")] if has_c else [])
    vrec = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    off = end + vrec.nbytes
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=off)
    if nf and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: only triangle faces are read")
    verts = torch.from_numpy(np.stack([vrec["x"], vrec["y"], vrec["z"]], -1).astype(np.float32).reshape(-1, 3))
    faces = torch.from_numpy(np.ascontiguousarray(frec["i"]).astype(np.int32).reshape(-1, 3))
    colors = torch.from_numpy(np.stack([vrec["r"], vrec["g"], vrec["b"]], -1).astype(np.float32) / 255.0) if has_c else None
    return Mesh(verts, faces, colors)
