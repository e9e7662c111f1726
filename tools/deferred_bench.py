"""The deferred view branch on fields of known live fraction: ms per render of `--rays` rays of bench.py's frame
with ops.set_deferred_view on and off, alternating, and the share of samples with raw sigma > 0 per level (from the stage calls).
    python tools/deferred_bench.py [--rays 76800] [--reps 5] [--fields mixed live dead]
Prints one JSON line per field."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops  # noqa: E402


def state_dict(field):
    sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)
    shift = {"mixed": 0.0, "live": 1e3, "dead": -1e3}[field]
    for lvl in ("coarse_mlp.", "fine_mlp."):
        sd[lvl + "density_layer.bias"] = sd[lvl + "density_layer.bias"] + shift
    return sd


def live_fractions(pc, pf, o, d, v):
    t_c, _ = ops.sample_along_rays(o, d, 64, syn.NEAR, syn.FAR, want_coords=False)
    raw_c = ops.mlp_fwd(pc, o, d, v, t_c)
    _, _, w_c, _ = ops.composite_raw(raw_c, t_c, d, True, ops.ACT_VANILLA, want_weights=True)
    t_f = ops.sample_pdf_t(t_c, w_c)
    raw_f = ops.mlp_fwd(pf, o, d, v, t_f)
    return [float((r.reshape(-1, 4)[:, 3] > 0).float().mean()) for r in (raw_c, raw_f)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=76800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", nargs="+", default=["mixed", "live", "dead"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    frame = syn.make_rays(480, 640, syn.look_at_pose(4.0, 30.0, 30.0), syn.focal_from_fovy(480))
    n = frame["rays_o"].shape[0]
    start = (n - a.rays) // 2          # the middle rows of the frame
    o, d, v = (frame[k][start:start + a.rays].contiguous().to(dev) for k in ("rays_o", "rays_d", "viewdirs"))
    for field in a.fields:
        sd = state_dict(field)
        pc, pf = (ops.pack_vanilla_mlp({k[len(p):]: t.to(dev) for k, t in sd.items() if k.startswith(p)}) for p in ("coarse_mlp.", "fine_mlp."))
        sub = slice(0, a.rays, 16)
        frac = live_fractions(pc, pf, o[sub].contiguous(), d[sub].contiguous(), v[sub].contiguous())
        ms = {True: [], False: []}
        for rep in range(a.reps + 1):       # the first pair is the warm-up
            for on in (True, False):
                ops.set_deferred_view(on)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.render_fwd(pc, pf, o, d, v, syn.NEAR, syn.FAR, True)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[on].append(round(e0.elapsed_time(e1), 3))
        ops.set_deferred_view(True)
        print(json.dumps({"field": field, "rays": a.rays, "live_fraction_coarse": round(frac[0], 4), "live_fraction_fine": round(frac[1], 4),
                          "ms_deferred": ms[True], "ms_single_kernel": ms[False]}), flush=True)


if __name__ == "__main__":
    main()
