"""Camera pose of an observed view, refined on a FROZEN single-scene NeRF (iNeRF): train ``LitNeRF`` briefly on
``run_single_scene``'s synthetic scene, take a held-out pose (the observation is the trained model's own render from it: the example shows
the optimiser, not the scene generator), perturb it by a small rotation and translation and recover it with ``LitNeRF.fit_pose``
(gradients of rays_o / rays_d / viewdirs through the HIP backward, one 6-vector stepped by aon_adam_step).  Prints the rotation and
translation error before and after.

    python examples/fit_pose_vanilla.py --synthetic /tmp/scene --img_wh 32 24 --steps 300 --fit-steps 150
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.fit_pose import pose_errors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic scene here (reference on-disk format) and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24))
    ap.add_argument("--steps", type=int, default=300, help="training steps of the model before the fit")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--fit-steps", type=int, default=150)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--azimuth", type=float, default=100.0, help="azimuth of the held-out view (degrees; radius 4, elevation 30)")
    ap.add_argument("--rotation-deg", type=float, default=2.0)
    ap.add_argument("--translation", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.datasets.sapien import SapienDataset, write_synthetic_scene
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    if args.synthetic:
        args.root_dir = write_synthetic_scene(args.synthetic, n_train=8, n_val=1, img_wh=tuple(args.img_wh))
    assert args.root_dir, "--root_dir or --synthetic"
    dev = torch.device("cuda:0")
    train = SapienDataset(args.root_dir, "train", tuple(args.img_wh), white_back=True, device=dev)
    lit = LitNeRF({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.steps}, near=train.near, far=train.far, white_bkgd=True).to(dev)
    opt = lit.configure_optimizers()
    gen = torch.Generator(device=dev).manual_seed(0)
    while lit.global_step < args.steps:     # 1. train briefly
        for batch in train.train_batches(args.batch, generator=gen):
            lit.fit_step({k: v.unsqueeze(0) for k, v in batch.items()}, lit.global_step, opt)
            if lit.global_step >= args.steps:
                break
    lit.finish_fit()
    lit.randomized = False              # the fit samples deterministically
    print(json.dumps({"trained_steps": args.steps, "train_psnr_fine": lit.logged["train/psnr1"][-1]}), flush=True)

    # 2. a held-out look-at pose on the scene's radius-4 sphere, seen by the trained model
    w, h = args.img_wh
    true = syn.look_at_pose(4.0, args.azimuth, 30.0)
    dirs = ops.ray_directions(h, w, syn.focal_from_fovy(h), device=dev).reshape(-1, 3)
    with torch.no_grad():
        o, d = ops.rays_from_pose(dirs, true.to(dev))
        target = lit.model({"rays_o": o.contiguous(), "rays_d": d, "viewdirs": d}, False, lit.white_bkgd, lit.near, lit.far)[-1][0].clone()
    # 3. perturb the pose: a rotation about a fixed axis and a translation along another
    axis = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)
    shift = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    corr = torch.cat([math.radians(args.rotation_deg) * axis / axis.norm(), args.translation * shift / shift.norm()])
    start = ops.apply_pose_correction(true.double(), corr).float()
    # 4. recover it
    poses, losses = lit.fit_pose([{"directions": dirs, "target": target}], args.fit_steps, lr=args.lr, poses=[start], seed=args.seed)
    e0, e1 = pose_errors(start, true), pose_errors(poses[0], true)
    losses = losses.tolist()
    out = {"fit_steps": args.fit_steps, "loss_first": losses[0], "loss_last": losses[-1],
           "rotation_error_deg": {"before": e0[0], "after": e1[0]}, "translation_error": {"before": e0[1], "after": e1[1]}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
