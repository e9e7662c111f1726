"""Step time of fitting latent codes on a frozen articulated network: LitNeRF_AutoDecoder.fit_latents with the
latent-only backward against the same loop through the full training backward, alternating runs, HIP events around each run, then one
run of each with the library's per-kernel-class timers (aon_profile_class).

    python tools/latent_fit_bench.py --rays 4096 --steps 10 --runs 4
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--runs", type=int, default=4, help="timed runs per mode (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import aon_amd.synthetic as syn
    from aon_amd import ops
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    dev = torch.device("cuda:0")
    lit = LitNeRF_AutoDecoder(randomized=True, near=2.0, far=6.0, white_bkgd=True).to(dev)
    lit.model.load_state_dict(syn.make_art_state_dict(seed=0, density_scale=30.0))
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=1))
    H, W = 480, 640
    ro, vd = ops.raygen(syn.look_at_pose(), H, W, syn.focal_from_fovy(H), device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    idx = torch.randint(0, H * W, (args.rays,), device=dev, generator=g)
    batch = {"rays_o": ro[idx].contiguous(), "rays_d": vd[idx].contiguous(), "viewdirs": vd[idx].contiguous(),
             "target": torch.rand(args.rays, 3, device=dev, generator=g)}

    def run(full, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, losses = lit.fit_latents([batch], steps, lr=5e-3, init=(0, 5), seed=1, full_backward=full)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps, losses

    for full in (True, False):
        run(full, args.warmup)
    times = {True: [], False: []}
    last = {}
    for _ in range(args.runs):
        for full in (True, False):
            ms, losses = run(full, args.steps)
            times[full].append(ms)
            last[full] = losses
    same = bool(torch.equal(last[True], last[False]))
    classes = {}
    for full in (True, False):
        ops.profile_begin()
        run(full, args.steps)
        ops.profile_end()
        classes[full] = {k: round(v[0] / args.steps, 4) for k, v in ops.profile_classes().items() if v[1]}
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    m = lit.model
    samples = sum(-(-args.rays * s // 128) * 128 for s in (m.num_coarse_samples + 1, m.num_coarse_samples + 1 + m.num_fine_samples))
    red_bytes = samples * (256 + 256 + 128 + 128) * 4     # the four dZ row groups the latent-only second stage reads
    red_ms = next((v for k, v in classes[False].items() if "wgrad" in k.lower()), None)
    out = {"rays_per_step": args.rays, "steps_per_run": args.steps, "runs": args.runs,
           "ms_per_step_full": [round(x, 3) for x in times[True]], "ms_per_step_latent": [round(x, 3) for x in times[False]],
           "median_ms_full": round(med[True], 3), "median_ms_latent": round(med[False], 3), "losses_bit_equal": same,
           "classes_ms_per_step_full": classes[True], "classes_ms_per_step_latent": classes[False],
           "latent_stage_bytes": red_bytes, "latent_stage_ms": red_ms,
           "latent_stage_fraction_of_hbm_peak": None if not red_ms else round(red_bytes / (red_ms * 1e-3) / HBM_PEAK, 4),
           "scratch_GB_full": round(ops.lib.aon_train_scratch_bytes_ex(args.rays, 1, 2, None) / 2 ** 30, 3),
           "scratch_GB_latent": round(ops.lib.aon_train_scratch_bytes_latents(args.rays, 2, None) / 2 ** 30, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
