"""Recover the joint states of several objects from ONE observed frame: train ``LitNeRF_AutoDecoder`` briefly on the
synthetic multi-instance set of examples/run_autodecoder.py, render three placements as in examples/render_scene.py, perturb their three
articulation codes, fit them back on the frozen network with ``fit_scene_codes`` -- the poses are known, gradients reach the codes -- and
print every object's code distance to the truth before and after.

    python examples/fit_scene.py --synthetic /tmp/multi --img_wh 32 24 --steps 300
    python examples/fit_scene.py --synthetic /tmp/multi --steps 300 --fit_steps 200 --render_wh 48 36
    python examples/fit_scene.py --synthetic /tmp/multi --steps 300 --background        # ... in front of a vanilla NeRF as the frozen backdrop
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.render_scene import placement, train_backdrop  # noqa: E402
from examples.run_autodecoder import collate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic multi-instance tree here and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24), help="training resolution")
    ap.add_argument("--render_wh", type=int, nargs=2, default=(32, 24), help="resolution of the observed frame (one chunk: its planes live until the backward)")
    ap.add_argument("--steps", type=int, default=300, help="training steps")
    ap.add_argument("--fit_steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--perturbation", type=float, default=0.3, help="standard deviation of the noise added to the articulation codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--background", action="store_true", help="the observed frame shows the objects in front of a vanilla NeRF trained on the synthetic "
                    "single scene, and the fit renders them in front of that frozen backdrop (DESIGN.md section 4.22)")
    ap.add_argument("--background-steps", type=int, default=300, help="training steps of the backdrop's LitNeRF")
    ap.add_argument("--out", default="fit_scene_out", help="where the backdrop's synthetic scene is written without --synthetic")
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.datasets.sapien_multi import SapienDatasetMulti, write_synthetic_multi_scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    if args.synthetic:
        args.root_dir = write_synthetic_multi_scene(args.synthetic, n_instances=2, n_degrees=3, n_views=60, img_wh=tuple(args.img_wh))
    assert args.root_dir, "--root_dir or --synthetic"
    dev = torch.device("cuda:0")
    train = SapienDatasetMulti(args.root_dir, "train", img_wh=tuple(args.img_wh), white_back=True, device=dev)
    lit = LitNeRF_AutoDecoder({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.steps, "N_max_objs": len(train.ids),
                               "N_obj_code_length": 128}).to(dev)
    lit.setup(train)
    opt = lit.configure_optimizers()
    for step in range(args.steps):
        lit.fit_step(collate(train[step], dev), step, opt)
    lit.finish_fit()

    table = lit.code_library.get_interpolated_articulations(max_interpolations=2, device=dev).detach()
    layout = [placement(0, 0, 0.0, (-0.45, -0.3, 0.0), 1.6), placement(1 % len(train.ids), 8, 40.0, (0.45, 0.35, 0.1), 1.6),
              placement(0, 16, -70.0, (-0.2, 1.9, -0.2), 1.6)]
    truth = [table[art].clone() for _, art, _, _ in layout]
    Wr, Hr = args.render_wh
    ro, vd = ops.raygen(syn.look_at_pose(5.0, 35.0, 30.0), Hr, Wr, syn.focal_from_fovy(Hr, 40.0), device=dev)
    batch = {"rays_o": ro, "rays_d": vd, "viewdirs": vd}
    background = train_backdrop(args, dev) if args.background else None
    batch["target"] = lit.render_scene(batch, layout, background=background)["rgb"].clone()
    gen = torch.Generator().manual_seed(args.seed + 1)
    start = [(iid, truth[j] + args.perturbation * torch.randn(32, generator=gen).to(dev), pose, box) for j, (iid, _, pose, box) in enumerate(layout)]
    codes, losses = lit.fit_scene_codes([batch], start, args.fit_steps, lr=args.lr, fit_keys=("articulation",), background=background)
    before = [float((s[1] - t).norm()) for s, t in zip(start, truth)]
    after = [float((c["articulation"].reshape(-1) - t).norm()) for c, t in zip(codes, truth)]
    for j, (b, a) in enumerate(zip(before, after)):
        print(f"object {j}: articulation code distance to the truth {b:.4f} -> {a:.4f}")
    rep = {"trained_steps": args.steps, "fit_steps": args.fit_steps, "frame": [Wr, Hr], "loss_first": float(losses[0]), "loss_last": float(losses[-1]),
           "code_distance_before": [round(b, 4) for b in before], "code_distance_after": [round(a, 4) for a in after]}
    if background is not None:
        rep["backdrop_steps"] = args.background_steps
    print(json.dumps(rep))
    return rep


if __name__ == "__main__":
    main()
