"""Codes of an object state the library has never seen, fitted on the FROZEN network: train
``LitNeRF_AutoDecoder`` briefly with one (instance, articulation) item held out, fit that item's three latent codes from a neighbouring
state's with ``fit_latents`` (latent-only backward: no weight gradient is computed), render a held-out view with the fitted codes.

    python examples/fit_latents.py --synthetic /tmp/multi --img_wh 32 24 --steps 300 --fit-steps 100
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from examples.run_autodecoder import collate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None)
    ap.add_argument("--synthetic", default=None, help="write a small synthetic multi-instance tree here and train on it")
    ap.add_argument("--img_wh", type=int, nargs=2, default=(32, 24))
    ap.add_argument("--steps", type=int, default=300, help="training steps of the whole model before the fit")
    ap.add_argument("--fit-steps", type=int, default=100)
    ap.add_argument("--fit-views", type=int, default=4, help="ray batches of the held-out item the codes are fitted to")
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--held-out", type=int, nargs=2, default=(0, 1), metavar=("INSTANCE", "ARTICULATION"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import random as _random
    _random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    from aon_amd.datasets.sapien_multi import SapienDatasetMulti, write_synthetic_multi_scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    if args.synthetic:
        args.root_dir = write_synthetic_multi_scene(args.synthetic, n_instances=2, n_degrees=3, n_views=60, img_wh=tuple(args.img_wh))
    assert args.root_dir, "--root_dir or --synthetic"
    dev = torch.device("cuda:0")
    kw = dict(img_wh=tuple(args.img_wh), white_back=True, device=dev)
    train = SapienDatasetMulti(args.root_dir, "train", **kw)
    val = SapienDatasetMulti(args.root_dir, "val", **kw)
    held = tuple(args.held_out)

    def draw(ds, want_held, limit=10000):
        """The dataset draws (instance, articulation, view) at random: the next item that is / is not the held-out state."""
        for i in range(limit):
            item = ds[i]
            if ((int(item["instance_id"]), int(item["articulation_id"])) == held) == want_held:
                return item
        raise RuntimeError(f"no {'held-out' if want_held else 'training'} item found for {held}")

    lit = LitNeRF_AutoDecoder({"chunk": 65536, "img_wh": tuple(args.img_wh), "run_max_steps": args.steps, "N_max_objs": len(train.ids),
                               "N_obj_code_length": 128}).to(dev)
    lit.setup(train)
    opt = lit.configure_optimizers()
    for step in range(args.steps):      # 1. train briefly, never on the held-out state
        lit.fit_step(collate(draw(train, False), dev), step, opt)
    lit.finish_fit()
    print(json.dumps({"trained_steps": args.steps, "train_psnr_fine": lit.logged["train/psnr1"][-1]}), flush=True)

    # 2. the held-out item: a few ray batches to fit to, one full view to judge by
    observed = [collate(draw(train, True), dev) for _ in range(args.fit_views)]
    view = collate(draw(val, True), dev)
    # 3. its codes from a neighbour's: the same instance in the nearest articulation state the library was trained on
    neighbour = (held[0], held[1] - 1 if held[1] > 0 else held[1] + 1)
    codes, losses = lit.fit_latents(observed, args.fit_steps, lr=args.lr, init=neighbour, seed=args.seed)
    # 4. the held-out view with the neighbour's codes and with the fitted ones
    start = lit._initial_latents(neighbour, dev)
    batch = lit._unbatch(view)
    with torch.no_grad():
        psnr = {}
        for name, lat in (("neighbour_codes", start), ("fitted_codes", codes)):
            rgb = lit._render_chunks(batch, lat, skip=("img_wh", "src_imgs"))["comp_rgb"]
            psnr[name] = lit.psnr_legacy(rgb, batch["target"]).mean().item()
    losses = losses.tolist()
    print(json.dumps({"held_out": held, "init_from": neighbour, "fit_steps": args.fit_steps, "loss_first": losses[0], "loss_last": losses[-1],
                      "val_psnr": psnr}))
    return psnr, losses


if __name__ == "__main__":
    main()
