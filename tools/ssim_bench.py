"""Time ops.ssim (csrc/aon_metrics.hip) on the two test-set shapes of the reference: one 640x480 image (the single-scene test view) and
19 images of 320x240 (the autodecoder's test set).  Prints one JSON line per case with the device-event time per call (both launches plus
the host side of the binding).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` and read the two kernels' rows.

    python tools/ssim_bench.py [--reps 50]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aon_amd import ops  # noqa: E402

CASES = {"640x480 x1": (1, 480, 640), "320x240 x19": (19, 240, 320)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, (n, h, w) in CASES.items():
        preds = [torch.rand(h, w, 3, device="cuda", generator=gen) for _ in range(n)]
        gts = [torch.rand(h, w, 3, device="cuda", generator=gen) for _ in range(n)]
        for _ in range(5):
            ops.ssim(preds, gts)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            ops.ssim(preds, gts)
        t1.record()
        torch.cuda.synchronize()
        px = n * (h - 10) * (w - 10) * 3
        print(json.dumps({"case": name, "images": n, "ms_per_call": t0.elapsed_time(t1) / args.reps, "bytes_read": n * h * w * 24,
                          "valid_pixel_channels": px}), flush=True)


if __name__ == "__main__":
    main()
