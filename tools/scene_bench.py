"""Scenes of several posed objects on a 640x480 frame with the default 65 + 193 samples, K = 1, 3 and 8 objects that
cover different shares of the frame; one JSON line per scene and everything again in profiles/scene_bench.json:

  * frame time of scene.render_scene (median of --reps, host clock around work that ends in a device synchronise, after a warm-up frame);
  * the time of the stages of that frame from device events around each stage call of the same chain written out (pairs, samplers, MLP,
    composite; their sum is the chain without the host's gaps), and the share of the pair and composite kernels in it;
  * pairs per ray, the share of rays that meet a box, the samples that reach the MLP;
  * for comparison, the sum of K whole-frame ops.art_render_fwd calls (what rendering the objects one by one costs before any pasting).

The weights are the synthetic ones (timing does not depend on what the network has learnt).  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/scene_bench.py` and read scene_pair_*_kernel / scene_composite_kernel.

    python tools/scene_bench.py [--reps 5] [--out profiles/scene_bench.json]
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
    """scene.render_scene's flow for one chunk, every stage under its own pair of events"""
    mlps = [model.coarse_mlp, model.fine_mlp]
    smalls = [[ops.art_prepare(dict(m.named_parameters()), ob.latents, degrees=m.degrees) for ob in objects] for m in mlps]
    pairs = st.run("pairs", lambda: ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], objects))
    t = st.run("sample", lambda: ops.sample_along_rays(pairs.rays_o, pairs.rays_d, 64, pairs.near, pairs.far, want_coords=False)[0])
    for level, m in enumerate(mlps):
        raw = st.run("mlp", lambda: ops.scene_art_mlp_fwd(m.packed(), smalls[level], pairs, t))
        out = st.run("composite", lambda: ops.scene_composite(raw, t, pairs, rays["rays_d"], True, want_weights=level == 0))
        if level == 0:
            t = st.run("sample", lambda: ops.sample_pdf_t_n(t, out[4], 128))
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/scene_bench.py", "device": torch.cuda.get_device_name(0), "scenes": recs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
