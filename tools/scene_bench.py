"""Scenes of several posed objects on a 640x480 frame with the default 65 + 193 samples, K = 1, 3 and 8 objects that
cover different shares of the frame; one JSON line per scene and everything again in profiles/scene_bench.json:

  * frame time of scene.render_scene (median of --reps, host clock around work that ends in a device synchronise, after a warm-up frame);
  * the time of the stages of that frame from device events around each stage call of the same chain written out (pairs, samplers, MLP,
    composite; their sum is the chain without the host's gaps), and the share of the pair and composite kernels in it;
  * pairs per ray, the share of rays that meet a box, the samples that reach the MLP;
  * for comparison, the sum of K whole-frame ops.art_render_fwd calls (what rendering the objects one by one costs before any pasting).

The weights are the synthetic ones (timing does not depend on what the network has learnt).  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/scene_bench.py` and read scene_pair_*_kernel / scene_composite_kernel.

--occupancy adds a leg per scene: the same frame with an occupancy grid on every object -- FULL grids (every cell
set: the three compaction launches and the gather launches against the dense ones, nothing skipped), then grids built from the bench's own
field at section 4.9's defaults (128^3 cells over [-1.2, 1.2]^3, threshold 0.01, dilate 1) -- with the frame without grids re-measured in
the same run, the samples that reached the MLP per level, and the gather-to-dense per-sample rate of the MLP stage.  When the synthetic
field is too hazy for a grid to empty anything, that is reported and the leg is repeated on synthetic.sparsify_nerf_(latents=)'s field.

--grad measures gradients through scenes INSTEAD of the frames above and adds a "grad" list to the file, leaving its
other records as they are: K = 1 and 3 on 4,096 rays of the frame at 65 + 193 samples -- one step of scene.render_scene_grad, a loss on all
four outputs of both levels and its gradients to every code and weight (host clock around work that ends in a device synchronise, and
device events around the whole step), the device time of ops.scene_composite_bwd and ops.scene_composite inside that step and their share
of it, and for K = 1 the step of the same sample count through NeRF_AE_Art.forward + backward on the one object's pairs (its object-frame
rays with their per-ray near / far), measured in the same run.

--grad --poses adds a "grad_poses" list instead: the same rays and objects, a pose-only step on the frozen network
(gradients to every object's (3, 4) pose, no weight-gradient stage) beside the code-and-weight step of --grad in the same run, device
events, and the device time and share of ops.art_ray_grads and ops.scene_pose_grads inside the pose-only step.

--background measures a vanilla NeRF behind the objects INSTEAD and adds a "background" record to the file, leaving
its other records as they are: on the whole frame at K = 0, 1, 3 the frame with the backdrop, the same frame without it (K >= 1), the
backdrop network alone through NeRF.forward at the same 65 + 193 samples, and the device time of ops.scene_composite_lists inside the frame
and its share of it; then an A/B of aon_scene_composite_lists against aon_scene_composite on identical homogeneous closed lists (the K = 3
frame's pairs at 193 samples, seeded raw): the two calls alternate inside one run, each timed by device events around blocks of 20 launches,
and the record holds each side's median and spread, and the A/A spread of the old entry against itself.

--grad --background adds a "background_grad" record instead: one step of scene.render_scene_background_grad on the
4,096 rays of --grad at K = 0, 1, 3 with the backdrop frozen and trainable (host clock and device events, median and spread, and the share of
ops.scene_composite_lists_bwd), then the A/B of aon_scene_composite_lists_bwd against aon_scene_composite_bwd on identical homogeneous closed
lists, alternating in one run as above, with the old entry against itself as the noise floor.

    python tools/scene_bench.py [--reps 5] [--occupancy] [--grad [--poses | --background]] [--background] [--out profiles/scene_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops, scene  # noqa: E402

H, W, NEAR, FAR = 480, 640, 2.0, 6.0


def frame_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def make_scene(K, dev, seed=0):
    """K seeded placements: one object in the middle of the frame, the others around it"""
    rng = np.random.default_rng(seed)
    objects = []
    for k in range(K):
        w = rng.normal(size=3)
        R = ops.so3_exp(torch.tensor(w / np.linalg.norm(w) * rng.uniform(0.2, 1.5), dtype=torch.float64)).float()
        c = torch.zeros(3) if k == 0 else torch.tensor(rng.uniform(-1.3, 1.3, 3), dtype=torch.float32)
        lat = {key: (0.2 * syn.seeded_uniform(60 + 3 * k + i, 1, width) - 0.1).to(dev)
               for i, (key, width) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}
        objects.append(scene.SceneObject(lat, torch.cat([R, c[:, None]], 1), float(rng.uniform(0.7, 1.3))))
    return objects


class Stages:
    """device events around the stage calls of one frame"""

    def __init__(self):
        self.spans = []

    def run(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.spans.append((name, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


def staged_frame(model, objects, rays, st):
    """scene.render_scene's flow for one chunk, every stage under its own pair of events (objects with grids: the occupancy stage call)"""
    grids = [ob.grid for ob in objects]
    occ = any(g is not None for g in grids)
    mlps = [model.coarse_mlp, model.fine_mlp]
    smalls = [[ops.art_prepare(dict(m.named_parameters()), ob.latents, degrees=m.degrees) for ob in objects] for m in mlps]
    pairs = st.run("pairs", lambda: ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects))
    t = st.run("sample", lambda: ops.sample_along_rays(pairs.rays_o, pairs.rays_d, 64, pairs.near, pairs.far, want_coords=False)[0])
    for level, m in enumerate(mlps):
        if occ:
            raw = st.run("mlp", lambda: ops.scene_art_mlp_fwd_occ(m.packed(), smalls[level], grids, pairs, t)[0])
        else:
            raw = st.run("mlp", lambda: ops.scene_art_mlp_fwd(m.packed(), smalls[level], pairs, t))
        out = st.run("composite", lambda: ops.scene_composite(raw, t, pairs, rays["rays_d"], True, want_weights=level == 0))
        if level == 0:
            t = st.run("sample", lambda: ops.sample_pdf_t_n(t, out[4], 128))
    return pairs


def staged_mlp_ms(model, objects, rays, reps):
    """median over `reps` staged frames (after a warm-up) of the MLP stage's device time, both levels"""
    staged_frame(model, objects, rays, Stages())
    runs = []
    for _ in range(reps):
        st = Stages()
        staged_frame(model, objects, rays, st)
        runs.append(st.totals()["mlp"])
    return statistics.median(runs)


def with_grids(objects, grids):
    return [scene.SceneObject(ob.latents, ob.pose, ob.box, g) for ob, g in zip(objects, grids)]


OCC_BOUNDS = (-1.2, 1.2)        # section 4.9's defaults; every box of make_scene (side <= 1.3) lies inside


def occupancy_leg(model, objects, rays, n, reps, ms_dense, mlp_dense, tag):
    """one set of grids on `objects` -> the leg's record; ms_dense / mlp_dense: the frame and MLP stage without grids, same run, same model"""
    _, occupied = scene.render_scene(model, objects, rays, True, chunk=n, want_occupied=True)
    _, total = scene.render_scene(model, with_grids(objects, [None] * len(objects)), rays, True, chunk=n, want_occupied=True)
    ms = frame_time(lambda: scene.render_scene(model, objects, rays, True, chunk=n), reps) * 1e3
    mlp = staged_mlp_ms(model, objects, rays, reps)
    run, tot = [int(o.sum()) for o in occupied], [int(o.sum()) for o in total]
    return {"grids": tag, "ms_frame": round(ms, 3), "frame_vs_no_grids": round(ms / ms_dense, 4), "ms_mlp_stage": round(mlp, 3),
            "samples_run": run, "samples_total": tot, "share_run": [round(r / max(t, 1), 4) for r, t in zip(run, tot)],
            "share_run_per_object_fine": [round(int(r) / max(int(t), 1), 4) for r, t in zip(occupied[-1].tolist(), total[-1].tolist())],
            "cells_occupied_per_object": [round(ob.grid.occupied_fraction(), 4) for ob in objects],
            # samples per millisecond of the MLP stage (compaction launches included) over the dense stage's
            "gather_to_dense_rate": round((sum(run) / mlp) / (sum(tot) / mlp_dense), 4)}


def occupancy_record(model, objects, rays, n, reps, dev):
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art
    from aon_amd.occupancy import build_occupancy

    ms_dense = frame_time(lambda: scene.render_scene(model, objects, rays, True, chunk=n), reps) * 1e3
    mlp_dense = staged_mlp_ms(model, objects, rays, reps)
    full = ops.occupancy_grid(torch.ones(5, 5, 5, device=dev), OCC_BOUNDS[0], OCC_BOUNDS[1], 0.01, 0)
    rec = {"ms_frame_no_grids": round(ms_dense, 3), "ms_mlp_stage_no_grids": round(mlp_dense, 3),
           "legs": [occupancy_leg(model, with_grids(objects, [full] * len(objects)), rays, n, reps, ms_dense, mlp_dense, "full")]}
    field = [build_occupancy(model, OCC_BOUNDS, latents=ob.latents) for ob in objects]
    rec["legs"].append(occupancy_leg(model, with_grids(objects, field), rays, n, reps, ms_dense, mlp_dense, "field (128^3, threshold 0.01, dilate 1)"))
    if min(g.occupied_fraction() for g in field) > 0.99:
        rec["finding"] = "the synthetic articulated field is too hazy for a grid to empty anything; repeated on synthetic.sparsify_nerf_(latents=)'s field"
        sparse = NeRF_AE_Art().to(dev)
        sparse.load_state_dict(model.state_dict())
        syn.sparsify_nerf_(sparse, 0.8, OCC_BOUNDS[1], latents=objects[0].latents)
        ms_sparse = frame_time(lambda: scene.render_scene(sparse, objects, rays, True, chunk=n), reps) * 1e3
        mlp_sparse = staged_mlp_ms(sparse, objects, rays, reps)
        grids = [build_occupancy(sparse, OCC_BOUNDS, latents=ob.latents) for ob in objects]
        leg = occupancy_leg(sparse, with_grids(objects, grids), rays, n, reps, ms_sparse, mlp_sparse, "sparsified field (128^3, threshold 0.01, dilate 1)")
        leg["ms_frame_no_grids"] = round(ms_sparse, 3)
        rec["legs"].append(leg)
    return rec


GRAD_RAYS = 4096


def grad_records(model, ro, vd, reps, dev):
    """the --grad legs -> one record per K"""
    idx = (torch.arange(GRAD_RAYS, device=dev) * (ro.shape[0] // GRAD_RAYS)).long()
    rays = {"rays_o": ro[idx].contiguous(), "rays_d": vd[idx].contiguous(), "viewdirs": vd[idx].contiguous()}
    target = syn.seeded_uniform(5, GRAD_RAYS, 3).to(dev)
    keys = ("density", "color", "articulation")
    nets = [p for m in (model.coarse_mlp, model.fine_mlp) for p in m.ordered_params()]
    recs = []
    for K in (1, 3):
        objects = [scene.SceneObject({k: v.clone().requires_grad_(True) for k, v in ob.latents.items()}, ob.pose, ob.box) for ob in make_scene(K, dev)]
        wrt = [ob.latents[k] for ob in objects for k in keys] + nets

        def step():
            levels = scene.render_scene_grad(model, objects, rays, True)
            loss = sum(torch.mean((lv[0] - target) ** 2) + 0.1 * lv[1].mean() + 0.05 * lv[2].mean() + 0.2 * (lv[3] ** 2).mean() for lv in levels)
            return torch.autograd.grad(loss, wrt)

        ms_host = frame_time(step, reps) * 1e3
        # device events: around the whole step, and around the two composite stage calls inside it
        real_bwd, real_fwd = ops.scene_composite_bwd, ops.scene_composite
        runs = []
        try:
            for _ in range(reps):
                st = Stages()
                ops.scene_composite_bwd = lambda *a, **kw: st.run("composite_bwd", lambda: real_bwd(*a, **kw))
                ops.scene_composite = lambda *a, **kw: st.run("composite", lambda: real_fwd(*a, **kw))
                st.run("step", step)
                runs.append(st.totals())
        finally:
            ops.scene_composite_bwd, ops.scene_composite = real_bwd, real_fwd
        dev_ms = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        with torch.no_grad():
            pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
        rec = {"rays": GRAD_RAYS, "samples": "65 + 193", "objects": K, "reps": reps, "pairs": pairs.P, "mlp_samples": pairs.P * (65 + 193),
               "ms_step_host": round(ms_host, 3), "ms_step_device": round(dev_ms["step"], 3), "ms_composite_bwd": round(dev_ms["composite_bwd"], 4),
               "ms_composite_fwd": round(dev_ms["composite"], 4), "share_composite_bwd": round(dev_ms["composite_bwd"] / dev_ms["step"], 5),
               "share_composite_fwd": round(dev_ms["composite"] / dev_ms["step"], 5),
               "composite_bwd_bytes": pairs.P * (65 + 193) * 36}
        if K == 1:      # the same samples through the one-object step: the object's pairs as a batch of rays with per-ray near / far
            one = {"rays_o": pairs.rays_o.contiguous(), "rays_d": pairs.rays_d.contiguous(), "viewdirs": pairs.viewdirs.contiguous()}
            near, far = pairs.near.reshape(-1, 1).contiguous(), pairs.far.reshape(-1, 1).contiguous()
            lat = objects[0].latents
            tg = target[pairs.ray.long()]

            def single():
                out = model(one, False, True, near, far, lat)
                loss = sum(torch.mean((o[0] - tg) ** 2) + 0.1 * o[1].mean() + 0.05 * o[2].mean() for o in out)
                return torch.autograd.grad(loss, [lat[k] for k in keys] + nets)

            rec["ms_one_object_step_host"] = round(frame_time(single, reps) * 1e3, 3)
            rec["scene_step_vs_one_object_step"] = round(ms_host / rec["ms_one_object_step_host"], 4)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def pose_records(model, ro, vd, reps, dev):
    """the --grad --poses legs -> one record per K: a pose-only step on a frozen network beside the code-and-weight
    step of section 4.18, the same rays and objects in the same run; device events, median of `reps`"""
    idx = (torch.arange(GRAD_RAYS, device=dev) * (ro.shape[0] // GRAD_RAYS)).long()
    rays = {"rays_o": ro[idx].contiguous(), "rays_d": vd[idx].contiguous(), "viewdirs": vd[idx].contiguous()}
    target = syn.seeded_uniform(5, GRAD_RAYS, 3).to(dev)
    keys = ("density", "color", "articulation")
    params = [p for p in model.parameters()]
    nets = [p for m in (model.coarse_mlp, model.fine_mlp) for p in m.ordered_params()]
    loss_of = lambda levels: sum(torch.mean((lv[0] - target) ** 2) + 0.1 * lv[1].mean() + 0.05 * lv[2].mean() + 0.2 * (lv[3] ** 2).mean() for lv in levels)  # noqa: E731
    recs = []
    for K in (1, 3):
        base = make_scene(K, dev)
        coded = [scene.SceneObject({k: v.clone().requires_grad_(True) for k, v in ob.latents.items()}, ob.pose, ob.box) for ob in base]
        posed = [scene.SceneObject(ob.latents, ob.pose.clone().requires_grad_(True), ob.box) for ob in base]

        def weight_step():
            return torch.autograd.grad(loss_of(scene.render_scene_grad(model, coded, rays, True)), [ob.latents[k] for ob in coded for k in keys] + nets)

        def pose_step():
            return torch.autograd.grad(loss_of(scene.render_scene_grad(model, posed, rays, True)), [ob.pose_tensor for ob in posed])

        def timed(step, frozen, spies=()):
            flags = [p.requires_grad for p in params]
            reals = {name: getattr(ops, name) for name in spies}
            runs = []
            try:
                for p in params:
                    p.requires_grad_(not frozen)
                step()                                     # warm-up
                for _ in range(reps):
                    st = Stages()
                    for name, real in reals.items():
                        setattr(ops, name, (lambda real, name: lambda *a, **kw: st.run(name, lambda: real(*a, **kw)))(real, name))
                    st.run("step", step)
                    runs.append(st.totals())
            finally:
                for name, real in reals.items():
                    setattr(ops, name, real)
                for p, f in zip(params, flags):
                    p.requires_grad_(f)
            return {k: statistics.median(r[k] for r in runs) for k in runs[0]}

        w = timed(weight_step, False)
        p = timed(pose_step, True, ("art_ray_grads", "scene_pose_grads"))
        with torch.no_grad():
            pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], base)
        rec = {"rays": GRAD_RAYS, "samples": "65 + 193", "objects": K, "reps": reps, "pairs": pairs.P, "mlp_samples": pairs.P * (65 + 193),
               "ms_code_and_weight_step_device": round(w["step"], 3), "ms_pose_only_step_device": round(p["step"], 3),
               "pose_only_vs_code_and_weight": round(p["step"] / w["step"], 4),
               "ms_art_ray_grads": round(p["art_ray_grads"], 4), "ms_scene_pose_grads": round(p["scene_pose_grads"], 4),
               "share_art_ray_grads": round(p["art_ray_grads"] / p["step"], 5), "share_scene_pose_grads": round(p["scene_pose_grads"] / p["step"], 5)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def background_record(model, rays, n, reps, dev):
    """the --background legs -> {"frames": [one record per K], "composite_ab": {...}}"""
    from aon_amd.models.vanilla_nerf.model import NeRF

    bg_model = NeRF().to(dev)
    bg_model.load_state_dict(syn.make_smooth_nerf_state_dict(seed=7))
    bg = scene.SceneBackground(bg_model, NEAR, FAR)
    ms_alone = frame_time(lambda: bg_model(rays, False, True, NEAR, FAR), reps) * 1e3
    frames = []
    for K in (0, 1, 3):
        objects = make_scene(K, dev)
        with_bg = lambda: scene.render_scene(model, objects, rays, True, chunk=n, background=bg)   # noqa: E731
        ms_with = frame_time(with_bg, reps) * 1e3
        ms_without = frame_time(lambda: scene.render_scene(model, objects, rays, True, chunk=n), reps) * 1e3 if K else None
        real = ops.scene_composite_lists
        runs = []
        try:
            for _ in range(reps):
                st = Stages()
                ops.scene_composite_lists = lambda *a, **kw: st.run("composite", lambda: real(*a, **kw))
                st.run("frame", with_bg)
                runs.append(st.totals())
        finally:
            ops.scene_composite_lists = real
        dev_ms = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        rec = {"frame": f"{W}x{H}", "samples": "65 + 193", "objects": K, "reps": reps, "ms_frame_with_backdrop": round(ms_with, 3),
               "ms_frame_without_backdrop": None if ms_without is None else round(ms_without, 3), "ms_backdrop_alone_nerf_forward": round(ms_alone, 3),
               "frame_vs_sum_of_parts": round(ms_with / ((ms_without or 0.0) + ms_alone), 4), "ms_frame_device": round(dev_ms["frame"], 3),
               "ms_composite_lists": round(dev_ms["composite"], 4), "share_composite_lists": round(dev_ms["composite"] / dev_ms["frame"], 5)}
        print(json.dumps(rec), flush=True)
        frames.append(rec)
    # A/B: the new entry against the old one on identical homogeneous closed lists
    objects = make_scene(3, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
    S = 193
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = (syn.seeded_uniform(9, pairs.P, S, 4).to(dev) * 4.0 - 1.0).contiguous()
    lists = [ops.SceneList(ops.ACT_ARTICULATED, False)] * 3
    old = lambda: ops.scene_composite(raw, t, pairs, rays["rays_d"], True)                         # noqa: E731
    new = lambda: ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], True, lists)            # noqa: E731
    same = all(torch.equal(a, b) for a, b in zip(old(), new()))
    block, rounds = 20, max(4 * reps, 12)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(block):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / block

    for fn in (old, new):
        timed(fn)                                              # warm-up of both
    ms = {"old_a": [], "new": [], "old_b": []}
    for _ in range(rounds):                                    # alternating: old, new, old, new ...
        ms["old_a"].append(timed(old))
        ms["new"].append(timed(new))
        ms["old_b"].append(timed(old))
    stat = lambda x: {"median": round(statistics.median(x), 5), "min": round(min(x), 5), "max": round(max(x), 5)}   # noqa: E731
    ab = {"pairs": pairs.P, "samples": S, "lists": 3, "launches_per_timing": block, "rounds": rounds, "same_bits": bool(same),
          "ms_scene_composite": stat(ms["old_a"]), "ms_scene_composite_lists": stat(ms["new"]), "ms_scene_composite_again": stat(ms["old_b"]),
          "new_vs_old": round(statistics.median(ms["new"]) / statistics.median(ms["old_a"]), 4),
          "old_vs_old": round(statistics.median(ms["old_b"]) / statistics.median(ms["old_a"]), 4)}
    print(json.dumps(ab), flush=True)
    return {"frames": frames, "composite_ab": ab}


def background_grad_record(model, ro, vd, reps, dev):
    """the --grad --background legs -> {"steps": [one record per (K, frozen / trainable backdrop)], "composite_bwd_ab": {...}}"""
    from aon_amd.models.vanilla_nerf.model import NeRF

    idx = (torch.arange(GRAD_RAYS, device=dev) * (ro.shape[0] // GRAD_RAYS)).long()
    rays = {"rays_o": ro[idx].contiguous(), "rays_d": vd[idx].contiguous(), "viewdirs": vd[idx].contiguous()}
    target = syn.seeded_uniform(5, GRAD_RAYS, 3).to(dev)
    keys = ("density", "color", "articulation")
    nets = [p for m in (model.coarse_mlp, model.fine_mlp) for p in m.ordered_params()]
    bg_model = NeRF().to(dev)
    bg_model.load_state_dict(syn.make_smooth_nerf_state_dict(seed=7))
    bg = scene.SceneBackground(bg_model, NEAR, FAR)
    bg_nets = [p for m in (bg_model.coarse_mlp, bg_model.fine_mlp) for p in m.ordered_params()]
    spread = lambda x: {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}   # noqa: E731
    steps = []
    for K in (0, 1, 3):
        objects = [scene.SceneObject({k: v.clone().requires_grad_(True) for k, v in ob.latents.items()}, ob.pose, ob.box) for ob in make_scene(K, dev)]
        codes = [ob.latents[k] for ob in objects for k in keys]
        for trainable in (False, True):
            for p in bg_model.parameters():
                p.requires_grad_(trainable)
            wrt = codes + nets + (bg_nets if trainable else [])

            def step():
                levels = scene.render_scene_background_grad(model, objects, rays, True, bg)
                loss = sum(torch.mean((lv[0] - target) ** 2) + 0.1 * lv[1].mean() + 0.05 * lv[2].mean() + 0.2 * (lv[3] ** 2).mean() for lv in levels)
                return torch.autograd.grad(loss, wrt)

            step()                                             # warm-up
            host = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            real_bwd, real_fwd = ops.scene_composite_lists_bwd, ops.scene_composite_lists
            runs = []
            try:
                for _ in range(reps):
                    st = Stages()
                    ops.scene_composite_lists_bwd = lambda *a, **kw: st.run("composite_bwd", lambda: real_bwd(*a, **kw))
                    ops.scene_composite_lists = lambda *a, **kw: st.run("composite", lambda: real_fwd(*a, **kw))
                    st.run("step", step)
                    runs.append(st.totals())
            finally:
                ops.scene_composite_lists_bwd, ops.scene_composite_lists = real_bwd, real_fwd
            dev_ms = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
            with torch.no_grad():
                P = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects).P if K else 0
            rec = {"rays": GRAD_RAYS, "samples": "65 + 193", "objects": K, "backdrop": "trainable" if trainable else "frozen", "reps": reps,
                   "rows": P + GRAD_RAYS, "mlp_samples": (P + GRAD_RAYS) * (65 + 193), "ms_step_host": spread(host),
                   "ms_step_device": spread([r["step"] for r in runs]), "ms_composite_lists_bwd": round(dev_ms["composite_bwd"], 4),
                   "ms_composite_lists_fwd": round(dev_ms["composite"], 4), "share_composite_lists_bwd": round(dev_ms["composite_bwd"] / dev_ms["step"], 5)}
            print(json.dumps(rec), flush=True)
            steps.append(rec)
    # A/B: the new backward against the old one on identical homogeneous closed lists, alternating in one run
    objects = make_scene(3, dev)
    with torch.no_grad():
        pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects)
        S = 193
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = (syn.seeded_uniform(9, pairs.P, S, 4).to(dev) * 4.0 - 1.0).contiguous()
    g = [syn.seeded_uniform(11 + i, GRAD_RAYS, w).to(dev).reshape(shape) - 0.5 for i, (w, shape) in enumerate(((3, (GRAD_RAYS, 3)), (1, (GRAD_RAYS,)), (1, (GRAD_RAYS,)),
                                                                                                            (3, (GRAD_RAYS, 3))))]
    lists = [ops.SceneList(ops.ACT_ARTICULATED, False)] * 3
    old = lambda: ops.scene_composite_bwd(raw, t, pairs, rays["rays_d"], g[0], g[1], g[2], g[3], True)                        # noqa: E731
    new = lambda: ops.scene_composite_lists_bwd(raw, t, pairs, rays["rays_d"], g[0], g[1], g[2], g[3], True, lists)           # noqa: E731
    same = bool(torch.equal(old().view(torch.int32), new().view(torch.int32)))
    block, rounds = 20, max(4 * reps, 12)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(block):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / block

    for fn in (old, new):
        timed(fn)                                              # warm-up of both
    ms = {"old_a": [], "new": [], "old_b": []}
    for _ in range(rounds):                                    # alternating: old, new, old, new ...
        ms["old_a"].append(timed(old))
        ms["new"].append(timed(new))
        ms["old_b"].append(timed(old))
    stat = lambda x: {"median": round(statistics.median(x), 5), "min": round(min(x), 5), "max": round(max(x), 5)}   # noqa: E731
    ab = {"pairs": pairs.P, "samples": S, "lists": 3, "launches_per_timing": block, "rounds": rounds, "same_bits": same,
          "note": "each launch includes the wrapper's torch.zeros of d_raw, the same in both",
          "ms_scene_composite_bwd": stat(ms["old_a"]), "ms_scene_composite_lists_bwd": stat(ms["new"]), "ms_scene_composite_bwd_again": stat(ms["old_b"]),
          "new_vs_old": round(statistics.median(ms["new"]) / statistics.median(ms["old_a"]), 4),
          "old_vs_old": round(statistics.median(ms["old_b"]) / statistics.median(ms["old_a"]), 4)}
    print(json.dumps(ab), flush=True)
    return {"steps": steps, "composite_bwd_ab": ab}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--occupancy", action="store_true", help="add the occupancy-grid legs (DESIGN.md section 4.17)")
    ap.add_argument("--grad", action="store_true", help="measure gradients through scenes instead (DESIGN.md section 4.18)")
    ap.add_argument("--poses", action="store_true", help="with --grad: the pose-only step beside the code-and-weight step (DESIGN.md section 4.20), key grad_poses")
    ap.add_argument("--background", action="store_true", help="measure a vanilla backdrop behind the objects instead (DESIGN.md section 4.21), key background; "
                    "with --grad: gradients through a scene with a backdrop (DESIGN.md section 4.22), key background_grad")
    ap.add_argument("--objects", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/scene_bench.py measures on the GPU: none found")
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    dev = torch.device("cuda:0")
    model = NeRF_AE_Art().to(dev)
    model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=2.0))
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    rays = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
    n = ro.shape[0]
    if args.grad and args.background:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": "tools/scene_bench.py", "device": torch.cuda.get_device_name(0)}
        doc["background_grad"] = background_grad_record(model, ro, vd, args.reps, dev)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    if args.background:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": "tools/scene_bench.py", "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            doc["background"] = background_record(model, rays, n, args.reps, dev)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    if args.grad:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": "tools/scene_bench.py", "device": torch.cuda.get_device_name(0)}
        if args.poses:
            doc["grad_poses"] = pose_records(model, ro, vd, args.reps, dev)
        else:
            doc["grad"] = grad_records(model, ro, vd, args.reps, dev)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    recs = []
    with torch.no_grad():
        for K in args.objects:
            objects = make_scene(K, dev)
            ms_frame = frame_time(lambda: scene.render_scene(model, objects, rays, True, chunk=n), args.reps) * 1e3
            staged_frame(model, objects, rays, Stages())       # warm-up
            runs = []
            for _ in range(args.reps):
                st = Stages()
                pairs = staged_frame(model, objects, rays, st)
                runs.append(st.totals())
            stages = {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}
            total = sum(stages.values())
            small = [ops.art_prepare(dict(m.named_parameters()), objects[0].latents, degrees=m.degrees) for m in (model.coarse_mlp, model.fine_mlp)]
            one = lambda: ops.art_render_fwd(model.coarse_mlp.packed(), small[0], model.fine_mlp.packed(), small[1], ro, vd, vd, NEAR, FAR, True)  # noqa: E731
            ms_single = frame_time(one, args.reps) * 1e3
            rec = {"frame": f"{W}x{H}", "samples": "65 + 193", "objects": K, "reps": args.reps, "ms_frame": round(ms_frame, 3),
                   "ms_stages": stages, "ms_stages_sum": round(total, 3),
                   "share_pairs": round(stages["pairs"] / total, 4), "share_composite": round(stages["composite"] / total, 4),
                   "pairs": pairs.P, "pairs_per_ray": round(pairs.P / n, 4), "rays_with_a_pair": round(float((pairs.slot >= 0).any(1).float().mean()), 4),
                   "mlp_samples": pairs.P * (65 + 193), "mlp_samples_dense_one_object": n * (65 + 193),
                   "ms_one_whole_frame_art_render_fwd": round(ms_single, 3), "ms_k_whole_frame_renders": round(K * ms_single, 3)}
            if args.occupancy:
                rec["occupancy"] = occupancy_record(model, objects, rays, n, args.reps, dev)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/scene_bench.py", "device": torch.cuda.get_device_name(0), "scenes": recs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
