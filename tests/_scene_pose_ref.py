"""Pose gradients of scenes restated in torch and numpy, independent of the HIP kernels.

``object_rays``: the object-frame rays of aon_scene_pairs from a (3, 4) pose that may require grad, in the forward's operation order
(include/aon_hip_scene.h): s = o - c, then component a = (R[0][a] s_0 + R[1][a] s_1) + R[2][a] s_2.  ``round32=True`` keeps the forward's fp32
subtraction as part of the function (s = fl32(o - c), with d s / d c = -1), which is what the kernel differentiates; ``round32=False`` subtracts in
the pose's dtype (central differences need a function of the perturbed fp64 pose).
``scene_level_oracle_t``: tests/_scene_grad_ref.scene_level_oracle taking the pair rays as TENSORS, so that autograd reaches the poses.
``pose_grads_closed``: the closed forms of g_R and g_c in numpy fp64.
``ray_grads_fp64``: aon_art_ray_grads' formulas in fp64 from the chain's read-back outputs, with the sums of absolute products."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_grad_ref as gref  # noqa: E402

F = np.float32


def object_rays(M, o, d, v, round32=True):
    """M (3, 4) torch, o / d / v (m, 3) torch of M's dtype holding fp32 values -> (o', d', v') each (m, 3)"""
    R, c = M[:, :3], M[:, 3]
    s = o - c
    if round32:
        s32 = torch.from_numpy((o.detach().numpy().astype(F) - c.detach().numpy().astype(F)[None, :]).astype(F).astype(np.float64)).to(M.dtype)
        s = s + (s32 - s.detach())

    def rot(x):
        return (R[0][None, :] * x[:, 0:1] + R[1][None, :] * x[:, 1:2]) + R[2][None, :] * x[:, 2:3]
    return rot(s), rot(d), rot(v)


def pair_rays(poses, rays, pair_ray, offsets, round32=True):
    """poses: K torch (3, 4); rays: dict of world (n, 3) arrays; pair_ray (P,), offsets (K + 1,) -> (po, pd, pv) torch (P, 3), object-major"""
    dt = poses[0].dtype
    w = {k: torch.from_numpy(np.asarray(rays[k], F).astype(np.float64)).to(dt) for k in ("rays_o", "rays_d", "viewdirs")}
    parts = []
    for k, M in enumerate(poses):
        idx = torch.from_numpy(np.asarray(pair_ray[int(offsets[k]): int(offsets[k + 1])], np.int64))
        parts.append(object_rays(M, w["rays_o"][idx], w["rays_d"][idx], w["viewdirs"][idx], round32))
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def scene_level_oracle_t(sd, prefix, po, pd, pv, offsets, slot, t, latents, rays_d, white, dtype, degrees=(0, 10, 4), opts=None, round32=True):
    """One level of a scene around the oracle's network on pair rays given as torch tensors (P, 3) of `dtype` (they may carry autograd history):
    orc.art_mlp per object segment, then composite_torch.  t (P, S), slot and the world rays_d are data."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as orc

    tt = torch.from_numpy(np.asarray(t, F)).to(dtype)
    pos = orc.cast_rays(tt, po, pd)
    venc = orc.pos_enc(pv, 0, degrees[2])
    parts = []
    for k, lat in enumerate(latents):
        a, b = int(offsets[k]), int(offsets[k + 1])
        if b > a:
            rr, rs = orc.art_mlp(sd, prefix, pos[a:b], venc[a:b], lat, degrees[0], degrees[1])
            parts.append(torch.cat([rr, rs], -1))
    raw = torch.cat(parts) if parts else torch.zeros((0, np.asarray(t).shape[1], 4), dtype=dtype)
    return gref.composite_torch(raw, t, slot, rays_d, white, opts, round32=round32)


def pose_grads_closed(pose, o, d, v, g_o, g_d, g_v):
    """pose (3, 4) fp32 values; o / d / v the WORLD rays of the object's pairs (m, 3) fp32; g_* (m, 3) -> (g_R (3, 3), g_c (3,), sum |terms| (12,))
    in numpy fp64, the pairs in ascending row"""
    pose = np.asarray(pose, F)
    R, c = pose[:, :3].astype(np.float64), pose[:, 3]
    s = (np.asarray(o, F) - c[None, :]).astype(F).astype(np.float64)
    d, v = np.asarray(d, F).astype(np.float64), np.asarray(v, F).astype(np.float64)
    g_o, g_d, g_v = (np.asarray(x, F).astype(np.float64) for x in (g_o, g_d, g_v))
    g_R = s.T @ g_o + d.T @ g_d + v.T @ g_v
    a_R = np.abs(s).T @ np.abs(g_o) + np.abs(d).T @ np.abs(g_d) + np.abs(v).T @ np.abs(g_v)
    so = g_o.sum(0)
    g_c = -(R @ so)
    a_c = np.abs(R) @ np.abs(g_o).sum(0)
    return g_R, g_c, np.concatenate([a_R.reshape(-1), a_c])


def view_backward(part, vd, deg_view, cos=None):
    """the V summed view-encoding partials of one ray pulled back through pos_enc(v, 0, deg_view) at the forward's rounded arguments:
    columns [v ; sin(2^l v) (level-major, xyz-minor) ; sin(2^l v + fp32(pi/2))] -> (g_v (3,), sum |terms| (3,)) in fp64.  cos: the cosine of an
    fp32 argument (default: numpy's in fp64; the kernel's own fp32 polynomial where bits matter)"""
    vd = np.asarray(vd, F)
    g, a = np.zeros(3), np.zeros(3)
    for ci in range(3 + 6 * deg_view):
        ax, coef = ci, 1.0
        if ci >= 3:
            e = ci - 3
            second = e >= 3 * deg_view
            e2 = e - 3 * deg_view if second else e
            ax = e2 % 3
            scale = F(2.0 ** (e2 // 3))
            arg = F(F(vd[ax] * scale) + (F(np.pi / 2) if second else F(0.0)))
            coef = float(scale) * float(np.cos(np.float64(arg)) if cos is None else cos(arg))
        g[ax] += coef * part[ci]
        a[ax] += abs(coef * part[ci])
    return g, a


def ray_grads_fp64(dz_d, dz_v, dxp, w_d0, w_v0, t, viewdirs, deg_view):
    """dz_d, dz_v (128, n * S): the rows aplane_d(0).. and aplane_v(0).. of the read-back gradient planes; dxp (n * S, >= 3); w_d0 (128, 163),
    w_v0 (128, 256 + V + 128); t (n, S); viewdirs (n, 3) -> dict of g_o, g_d, g_v (n, 3) fp64 and abs_o, abs_d, abs_v: the sums of the absolute
    values of every product that enters the output (the bar's scale)."""
    n, S = t.shape
    V = 3 + 6 * deg_view
    dz_d, dz_v = np.asarray(dz_d, np.float64)[:, : n * S], np.asarray(dz_v, np.float64)[:, : n * S]
    wd = np.asarray(w_d0, np.float64)[:, :3]
    wv = np.asarray(w_v0, np.float64)[:, 256: 256 + V]
    dx = np.asarray(dxp, np.float64)[: n * S, :3]
    gx = dx + dz_d.T @ wd                                          # (n S, 3)
    ax = np.abs(dx) + np.abs(dz_d).T @ np.abs(wd)
    pv = dz_v.T @ wv                                               # (n S, V)
    apv = np.abs(dz_v).T @ np.abs(wv)
    tt = np.asarray(t, np.float64).reshape(n * S, 1)
    out = {"g_o": gx.reshape(n, S, 3).sum(1), "abs_o": ax.reshape(n, S, 3).sum(1),
           "g_d": (tt * gx).reshape(n, S, 3).sum(1), "abs_d": (np.abs(tt) * ax).reshape(n, S, 3).sum(1)}
    part, apart = pv.reshape(n, S, V).sum(1), apv.reshape(n, S, V).sum(1)
    gv, av = np.zeros((n, 3)), np.zeros((n, 3))
    for r in range(n):
        gv[r], _ = view_backward(part[r], viewdirs[r], deg_view)
        _, av[r] = view_backward(apart[r], viewdirs[r], deg_view)
    out["g_v"], out["abs_v"] = gv, av
    return out


def fit_poses_oracle(sd, prefix, rays, target, start_poses, boxes, latents, steps, lr, dtype, degrees, num_samples, white=True):
    """The loop of LitNeRF_AutoDecoder.fit_scene_poses (fit_codes off, one level) around the oracle on the CPU: one 6-vector per object, poses
    rebuilt with ops.apply_pose_correction, torch.optim.Adam.  Per step the pairs (tests/_scene_ref.pairs_ref on the fp32 poses) and the
    sampler's t (near (1 - s) + far s in fp32) are data; the object rays come from pair_rays, so autograd reaches the 6-vectors.
    -> (losses, final poses as fp64 (3, 4) tensors)"""
    import _scene_ref as sref
    from aon_amd import ops

    K = len(start_poses)
    osd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    lat = [{k: v.detach().cpu().to(dtype) for k, v in c.items()} for c in latents]
    w = {k: np.asarray(rays[k], F) for k in ("rays_o", "rays_d", "viewdirs")}
    tg = torch.as_tensor(np.asarray(target)).to(dtype)
    start = [torch.as_tensor(np.asarray(p, F)).to(dtype) for p in start_poses]
    corr = torch.zeros(6 * K, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([corr], lr=lr)
    s = np.linspace(0.0, 1.0, num_samples + 1, dtype=F)
    losses = []

    def poses_now():
        return [ops.apply_pose_correction(start[k], corr[6 * k: 6 * k + 6]) for k in range(K)]
    for _ in range(steps):
        opt.zero_grad()
        poses = poses_now()
        pr = sref.pairs_ref(w["rays_o"], w["rays_d"], w["viewdirs"], [(p.detach().numpy().astype(F), b) for p, b in zip(poses, boxes)])
        t = ((pr["near"][:, None] * (F(1.0) - s)[None, :]).astype(F) + (pr["far"][:, None] * s[None, :]).astype(F)).astype(F)
        po, pd, pv = pair_rays(poses, w, pr["ray"], pr["offsets"], round32=dtype == torch.float64)
        out = scene_level_oracle_t(osd, prefix, po, pd, pv, pr["offsets"], pr["slot"], t, lat, w["rays_d"], white, dtype, degrees)
        loss = torch.mean((out["rgb"] - tg) ** 2)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, [p.detach().double() for p in poses_now()]
