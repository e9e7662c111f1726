"""tests/_composite_truth.py without a GPU: the long-double truth is finite on every adversarial row, a plain float64 evaluation of the
kernels' own formulas meets the backward bar of tests/test_hip_composite_range.py with room to spare (so a correct fp64 kernel can),
and the project's fp32 oracle is finite on every row (so the forward bar base + 3 |oracle32 - truth| is one)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _composite_truth as ct  # noqa: E402
from oracle import nerf_oracle as orc  # noqa: E402


def test_batches_hold_every_row_the_range_tests_name():
    for S in ct.SIZES:
        b = ct.adversarial_batch(S, 1)
        assert b["raw"].shape == (ct.N_RAYS, S, 4) and b["raw"].dtype == np.float32 and (np.diff(b["t"], axis=1) >= 0).all()
        labels = set(b["labels"])
        for need in ("opaque from the first sample", "empty ray -5", "empty ray -30", "raw_sigma -0.0", "raw_sigma 1e-40", "raw_sigma + bias = 20.0",
                     "raw_sigma + bias = -100.0", "colours 90", "colours -20", "last raw_sigma 1e-20", "last raw_sigma 5.0", "t log-uniform in [1e-3, 1e3]",
                     "|d| = 0.001", "|d| = 1000.0", "|d| = 0.0", "four equal t from 0", "plain"):
            assert need in labels or (S == 1 and need.startswith("raw_sigma + bias")), (S, need)      # (S = 1: no odd sample to carry them)
        if S >= 130:
            assert {f"opaque shell at {p}" for p in (20, 63, 64, 127, 128, S - 2)} <= labels
        again = ct.adversarial_batch(S, 1)
        assert all(np.array_equal(b[k], again[k], equal_nan=True) for k in ("raw", "t", "d", "g_rgb", "g_acc", "g_depth"))
        # the denormal and the signed zero survive as bit patterns
        r = b["labels"].index("raw_sigma 1e-40")
        assert 0 < b["raw"][r, 0, 3] < 1.2e-38
        assert np.signbit(b["raw"][b["labels"].index("raw_sigma -0.0"), 0, 3])


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("S", ct.SIZES)
def test_truth_is_finite_and_the_float64_restatement_meets_the_backward_bar(S, act):
    b = ct.adversarial_batch(S, act)
    worst = 0.0
    for white in (False, True):
        for with_extra in (False, True):
            ga, gd = (b["g_acc"], b["g_depth"]) if with_extra else (None, None)
            truth = ct.composite(b["raw"], b["t"], b["d"], white, act, None, b["g_rgb"], ga, gd)
            for k, v in truth.items():
                bad = ~np.isfinite(v.reshape(ct.N_RAYS, -1)).all(1)
                assert not bad.any(), (k, [b["labels"][i] for i in np.flatnonzero(bad)])
            k64 = ct.composite(b["raw"], b["t"], b["d"], white, act, None, b["g_rgb"], ga, gd, kernel_form=True)
            ratio = ct.backward_ratio(k64["d_raw"], truth["d_raw"])
            i = np.unravel_index(ratio.argmax(), ratio.shape)
            if ratio.max() > worst:
                worst, where = ratio.max(), (b["labels"][i[0]], i, white, with_extra)
            # exact zeros: empty relu rays and d = 0
            for r, lab in enumerate(b["labels"]):
                if lab == "|d| = 0.0" or (act == 1 and lab in ("empty ray -5", "empty ray -30", "raw_sigma 0.0", "raw_sigma -0.0", "raw_sigma -1e-30")):
                    assert (truth["d_raw"][r] == 0).all() and (k64["d_raw"][r] == 0).all(), lab
    print(f"S = {S}, act {act}: float64 restatement against the long-double truth, worst ratio to the backward bar {worst:.3f} at {where}")
    assert worst <= 0.5


@pytest.mark.parametrize("S", ct.SIZES)
def test_fp32_oracle_is_finite_on_every_row(S):
    for act in (0, 1, 2):
        b = ct.adversarial_batch(S, act)
        raw, t, d = (torch.from_numpy(b[k]) for k in ("raw", "t", "d"))
        if act == 2:
            rgb, sig = torch.sigmoid(raw[..., :3]) * (1 + 2 * 0.001) - 0.001, torch.nn.functional.softplus(raw[..., 3:] + (-1.0))
        elif act == 1:
            rgb, sig = torch.sigmoid(raw[..., :3]), torch.relu(raw[..., 3:])
        else:
            rgb, sig = raw[..., :3], raw[..., 3:]
        for white in (False, True):
            for k, v in zip(("rgb", "acc", "weights", "depth"), orc.volumetric_rendering(rgb, sig, t, d, white)):
                bad = ~torch.isfinite(v.reshape(ct.N_RAYS, -1)).all(1)
                assert not bad.any(), (act, k, [b["labels"][i] for i in torch.nonzero(bad).flatten().tolist()])


@pytest.mark.parametrize("S", ct.SIZES)
def test_fully_extreme_rays_are_finite(S):
    """ct.extreme_rows: the truth, its derivative and the fp32 oracle are finite on every ray, under both activations"""
    b = ct.extreme_rows(S)
    raw, t, d = (torch.from_numpy(b[k]) for k in ("raw", "t", "d"))
    for act in (1, 2):
        for white in (False, True):
            for k, v in ct.composite(b["raw"], b["t"], b["d"], white, act, None, b["g_rgb"]).items():
                assert np.isfinite(v).all(), (act, k)
        rgb, sig = ((torch.sigmoid(raw[..., :3]), torch.relu(raw[..., 3:])) if act == 1 else
                    (torch.sigmoid(raw[..., :3]) * (1 + 2 * 0.001) - 0.001, torch.nn.functional.softplus(raw[..., 3:] + (-1.0))))
        assert all(torch.isfinite(v).all() for v in orc.volumetric_rendering(rgb, sig, t, d, True))
