"""Occupancy-grid accelerated inference on a 640x480 frame, one JSON line per field:

  * dense MLP and gather MLP: device time of the fused MLP launches (aon_profile_*) and their per-sample rate -- the dense kernel over all
    n * S samples of the exact frame, the gather instance over the samples it ran (the occupied counts) -- and the ratio of the two rates;
  * mark + compact: the accelerated frame with an EMPTY grid (every sample marked, no MLP work) minus its profiled sampling and compositing
    launches, as a share of the dense frame;
  * end-to-end frame time exact vs accelerated (median of --reps, device-synchronised wall time) and the skipped fraction per level.

Fields: the synthetic weights made sparse by synthetic.sparsify_nerf_ (80 % of [-4, 4]^3 empty, "sparse"), and the synthetic scene trained by
examples/run_single_scene.py for --steps steps ("trained"; --no-trained skips it).  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/occupancy_bench.py` and read occ_mark_kernel<1> / occ_scan_kernel<1> / occ_emit_kernel<1> and the
mlp_fwd_kernel instances.

    python tools/occupancy_bench.py [--reps 5] [--steps 300] [--no-trained]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import aon_amd.synthetic as syn  # noqa: E402
from aon_amd import ops  # noqa: E402
from aon_amd.occupancy import build_occupancy  # noqa: E402

H, W, NEAR, FAR = 480, 640, 2.0, 6.0


def sparse_nerf(dev):
    from aon_amd.models.vanilla_nerf.model import NeRF

    model = NeRF().to(dev)
    model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
    return syn.sparsify_nerf_(model, 0.8, 4.0)


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


def profiled(fn):
    """-> {class: (ms, launches, units)} of one call"""
    fn()
    torch.cuda.synchronize()
    ops.profile_begin()
    fn()
    torch.cuda.synchronize()
    ops.profile_end()
    return ops.profile_classes()


def bench(name, model, bound, reps, dev):
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    pc, pf = model.coarse_mlp.packed(), model.fine_mlp.packed()
    grid = build_occupancy(model, (-bound, bound))
    empty = ops.occupancy_grid(torch.zeros(5, 5, 5, device=dev), -bound, bound, 0.01, 0)
    n = ro.shape[0]
    samples = [n * 65, n * 193]
    with torch.no_grad():
        exact = lambda: ops.render_fwd(pc, pf, ro, vd, vd, NEAR, FAR, True)  # noqa: E731
        accel = lambda: ops.render_fwd_occ(pc, pf, ro, vd, vd, NEAR, FAR, True, grid)  # noqa: E731
        blank = lambda: ops.render_fwd_occ(pc, pf, ro, vd, vd, NEAR, FAR, True, empty)  # noqa: E731
        t_exact, t_accel, t_blank = frame_time(exact, reps), frame_time(accel, reps), frame_time(blank, reps)
        _, occupied = accel()
        occupied = [int(x) for x in occupied.tolist()]
        p_exact, p_accel, p_blank = profiled(exact), profiled(accel), profiled(blank)
    ms_dense, ms_gather = p_exact["mlp_fwd"][0], p_accel["mlp_fwd"][0]
    rate_dense = sum(samples) / (ms_dense * 1e-3)
    rate_gather = sum(occupied) / (ms_gather * 1e-3) if ms_gather > 0 else float("nan")
    staged = sum(p_blank[k][0] for k in ("sample_t", "composite", "composite_pdf", "mlp_fwd"))
    mark_ms = t_blank * 1e3 - staged
    rec = {"field": name, "frame": f"{W}x{H}", "occupied_cells": round(grid.occupied_fraction(), 4),
           "skipped_coarse": round(1 - occupied[0] / samples[0], 4), "skipped_fine": round(1 - occupied[1] / samples[1], 4),
           "frame_ms_exact": round(t_exact * 1e3, 3), "frame_ms_accelerated": round(t_accel * 1e3, 3), "speedup": round(t_exact / t_accel, 3),
           "dense_mlp_ms": round(ms_dense, 3), "gather_mlp_ms": round(ms_gather, 3),
           "dense_rate_samples_per_s": round(rate_dense), "gather_rate_samples_per_s": round(rate_gather),
           "gather_over_dense_rate": round(rate_gather / rate_dense, 4),
           "mark_compact_ms": round(mark_ms, 3), "mark_compact_share_of_dense_frame": round(mark_ms / (t_exact * 1e3), 4)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--no-trained", action="store_true")
    ap.add_argument("--exp_dir", default="ckpts/occupancy_bench")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench("sparse", sparse_nerf(dev), 4.0, args.reps, dev)
    if not args.no_trained:
        from render_occupancy import train_or_load

        lit, _ = train_or_load(steps=args.steps, exp_dir=args.exp_dir)
        bench("trained", lit.model, 1.5, args.reps, dev)


if __name__ == "__main__":
    main()
