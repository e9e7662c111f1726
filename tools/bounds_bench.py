"""Per-ray near / far from a ray-box intersection on a 640x480 look-at frame, one JSON line per record.

Timing (per field; all modes in the same run, median of --reps device-synchronised whole-frame calls; samples run through the MLP per level):
  exact            scalar near / far, no grid
  bounds           per-ray near / far from the box, every ray rendered
  bounds_live      ... and the rays that miss the box skipped (ray_live)
  grid             scalar near / far, occupancy grid over the box
  grid_bounds_live all three
  limits           ops.ray_limits alone (box + reduce + finish kernels), wall time of the call
plus the PSNR of each frame to the exact one.  Fields: the sparse synthetic field of section 4.9 (box [-4, 4]^3 is its grid; the bounds box is
--sparse-box) and the scene of examples/run_single_scene.py trained for --steps steps (box side 3, its grid's box).  For the three small
kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/bounds_bench.py --no-trained --no-quality` and read
ray_box_kernel / ray_limits_reduce_kernel / ray_limits_finish_kernel / sample_t4_bounds_kernel.

Quality (--no-quality skips it), on the synthetic scene of examples/run_single_scene.py:
  (i)  300 steps with --ray-box unset and set, same seed: held-out PSNR every 50 steps;
  (ii) on the network trained without it, the held-out view at 256 + 512 samples (the yardstick), at 64 + 128, and at 64 + 128 with bounds:
       PSNR of the second and third against the first.

    python tools/bounds_bench.py [--reps 5] [--steps 300] [--no-trained] [--no-quality]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops  # noqa: E402
from aon_amd.occupancy import build_occupancy  # noqa: E402
from early_stop_bench import psnr, sparse_nerf  # noqa: E402
from occupancy_bench import H, W, NEAR, FAR, frame_time  # noqa: E402


def bench(name, model, grid_bound, box, reps, dev):
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    pc, pf = model.coarse_mlp.packed(), model.fine_mlp.packed()
    grid = build_occupancy(model, (-grid_bound, grid_bound))
    n = ro.shape[0]
    with torch.no_grad():
        near, far, live = ops.ray_limits(ro, vd, box)
        modes = {
            "exact": lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, NEAR, FAR, True, None, 0.0),
            "bounds": lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, near, far, True, None, 0.0),
            "bounds_live": lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, near, far, True, None, 0.0, ray_live=live),
            "grid": lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, NEAR, FAR, True, grid, 0.0),
            "grid_bounds_live": lambda: ops.render_fwd_stop(pc, pf, ro, vd, vd, near, far, True, grid, 0.0, ray_live=live),
        }
        rec = {"field": name, "frame": f"{W}x{H}", "box": box, "live_fraction": round(float(live.float().mean()), 4),
               "occupied_cells": round(grid.occupied_fraction(), 4), "samples": [n * 65, n * 193],
               "ms_limits": round(frame_time(lambda: ops.ray_limits(ro, vd, box), reps) * 1e3, 4), "modes": {}}
        ref_rgb = modes["exact"]()[0][1][0]
        for label, fn in modes.items():
            outs, ran, _ = fn()
            rec["modes"][label] = {"ms": round(frame_time(fn, reps) * 1e3, 3), "ran": [int(x) for x in ran.tolist()],
                                   "psnr_vs_exact": psnr(outs[1][0], ref_rgb)}
    print(json.dumps(rec), flush=True)
    return rec


def train_log(exp_dir, steps, ray_box):
    """examples/run_single_scene.py in a child process -> its validation records"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_single_scene.py"), "--synthetic", os.path.join(exp_dir, "scene"), "--steps", str(steps),
           "--val_every", "50", "--exp_dir", exp_dir, "--seed", "0"] + (["--ray-box", str(ray_box)] if ray_box else [])
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    recs = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    return [{"step": r["step"], "val_psnr": round(r["val_psnr"], 3)} for r in recs if "val_psnr" in r], [r for r in recs if "test_psnr" in r]


def quality(steps, box, exp_dir, dev):
    from aon_amd.datasets.sapien import SapienDataset
    from render_occupancy import train_or_load

    plain, plain_test = train_log(os.path.join(exp_dir, "plain"), steps, None)
    boxed, boxed_test = train_log(os.path.join(exp_dir, "boxed"), steps, box)
    print(json.dumps({"quality": "training", "steps": steps, "ray_box": box, "val_psnr_plain": plain, "val_psnr_ray_box": boxed,
                      "test_psnr_plain": plain_test[-1]["test_psnr"], "test_psnr_ray_box": boxed_test[-1]["test_psnr"]}), flush=True)
    root = os.path.join(exp_dir, "plain", "scene")
    lit, _ = train_or_load(os.path.join(exp_dir, "plain", "last.ckpt"), root, steps)
    model = lit.model
    item = SapienDataset(root, "val", (64, 48), white_back=True, device=dev)[0]
    o, d, v = (item[k].reshape(-1, 3) for k in ("rays_o", "rays_d", "viewdirs"))
    gt = item["target"].reshape(-1, 3)
    pc, pf = model.coarse_mlp.packed(), model.fine_mlp.packed()
    with torch.no_grad():
        near, far, live = ops.ray_limits(o, d, box)
        dense = ops.render_fwd(pc, pf, o, d, v, lit.near, lit.far, True, opts=ops.RenderOpts(256, 512))[1][0]
        default = ops.render_fwd(pc, pf, o, d, v, lit.near, lit.far, True)[1][0]
        bounded = ops.render_fwd(pc, pf, o, d, v, near, far, True, ray_live=live)[1][0]
    print(json.dumps({"quality": "sampling", "yardstick": "256+512", "live_fraction": round(float(live.float().mean()), 4),
                      "psnr_default_vs_yardstick": psnr(default, dense), "psnr_bounds_vs_yardstick": psnr(bounded, dense),
                      "psnr_vs_target": {"yardstick": psnr(dense, gt), "default": psnr(default, gt), "bounds": psnr(bounded, gt)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--sparse-box", type=float, default=3.0, help="side of the bounds box on the sparse synthetic field")
    ap.add_argument("--no-trained", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--exp_dir", default="ckpts/bounds_bench")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench("sparse", sparse_nerf(dev, 30.0), 4.0, args.sparse_box, args.reps, dev)
    if not args.no_trained:
        from render_occupancy import train_or_load

        lit, _ = train_or_load(steps=args.steps, exp_dir=os.path.join(args.exp_dir, "trained"))
        bench("trained", lit.model, 1.5, 3.0, args.reps, dev)
    if not args.no_quality:
        quality(args.steps, 3.0, os.path.join(args.exp_dir, "quality"), dev)


if __name__ == "__main__":
    main()
