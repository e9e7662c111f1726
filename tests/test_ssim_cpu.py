"""CPU: the fp64 SSIM yardstick (tests/_ssim_ref.py) against an independent scipy formulation and closed forms, the fp32-vs-fp64 gap that
makes the kernel compute its window statistics in fp64, and aon_ssim's argument validation, which needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from _ssim_ref import C1, C2, gaussian_window, ssim_ref, white_background_pair


def ssim_scipy(pred: np.ndarray, gt: np.ndarray) -> float:
    """Independent restatement: scipy.ndimage.correlate1d along both axes, then crop the 5-pixel border the "valid" map drops."""
    from scipy.ndimage import correlate1d

    g = gaussian_window().numpy()
    x, y = np.clip(pred.astype(np.float64), 0, 1), np.clip(gt.astype(np.float64), 0, 1)
    vals = []
    for ch in range(3):
        a, b = x[..., ch], y[..., ch]

        def G(t):
            return correlate1d(correlate1d(t, g, axis=0, mode="constant"), g, axis=1, mode="constant")[5:-5, 5:-5]

        mx, my = G(a), G(b)
        vx, vy, cxy = G(a * a) - mx * mx, G(b * b) - my * my, G(a * b) - mx * my
        vals.append((2 * mx * my + C1) / (mx * mx + my * my + C1) * (2 * cxy + C2) / (vx + vy + C2))
    return float(np.mean(np.stack(vals)))


@pytest.mark.parametrize("h,w", [(11, 11), (24, 32), (37, 53), (12, 40)])
@pytest.mark.parametrize("kind", ["uniform", "outside"])
def test_yardstick_matches_scipy(h, w, kind):
    gen = torch.Generator().manual_seed(h * 1000 + w)
    if kind == "uniform":
        p, g = torch.rand(h, w, 3, generator=gen), torch.rand(h, w, 3, generator=gen)
    else:   # values outside [0,1]: both sides clip before filtering
        p, g = 0.5 + 0.8 * torch.randn(h, w, 3, generator=gen), 0.5 + 0.8 * torch.randn(h, w, 3, generator=gen)
        assert (p < 0).any() and (p > 1).any()
    assert abs(ssim_ref(p, g).item() - ssim_scipy(p.numpy(), g.numpy())) < 1e-12


def test_yardstick_white_background_matches_scipy():
    p, g = white_background_pair(120, 160, seed=3)
    assert abs(ssim_ref(p, g).item() - ssim_scipy(p.numpy(), g.numpy())) < 1e-12


def test_closed_forms():
    x = torch.rand(37, 53, 3, generator=torch.Generator().manual_seed(1))
    assert abs(ssim_ref(x, x).item() - 1.0) < 1e-12
    for a, b in ((0.2, 0.7), (1.0, 0.0), (0.5, 0.5), (0.9, 1.0)):
        ta, tb = torch.full((20, 30, 3), a), torch.full((20, 30, 3), b)
        a, b = ta[0, 0, 0].item(), tb[0, 0, 0].item()   # the fp32 images' values
        want = (2 * a * b + C1) / (a * a + b * b + C1)
        got = ssim_ref(ta, tb).item()
        assert abs(got - want) < 1e-12, (a, b, got, want)
    # constants outside [0,1] are clipped first
    assert abs(ssim_ref(torch.full((11, 11, 3), 1.5), torch.full((11, 11, 3), -0.5)).item() - C1 / (1 + C1)) < 1e-12


def test_fp32_statistics_drift_on_white_background():
    """Why the kernel's window statistics are fp64: G(x^2) - mu^2 cancels on the flat white background against c2 = 9e-4."""
    p, g = white_background_pair()
    d64, d32 = ssim_ref(p, g).item(), ssim_ref(p, g, torch.float32).item()
    x, y = torch.rand(480, 640, 3, generator=torch.Generator().manual_seed(0)), torch.rand(480, 640, 3, generator=torch.Generator().manual_seed(1))
    noise_gap = abs(ssim_ref(x, y).item() - ssim_ref(x, y, torch.float32).item())
    print(f"640x480 white background: SSIM fp64 {d64:.12f}, fp32 statistics {d32:.12f}, |gap| {abs(d64 - d32):.2e}; noise image |gap| {noise_gap:.2e}")
    assert abs(d64 - d32) > 1e-6 > noise_gap


def test_aon_ssim_exported_and_validates_without_gpu():
    from aon_amd import _lib

    lib = _lib.lib
    assert "aon_ssim" in _lib.exported_symbols() and "aon_ssim_workspace_bytes" in _lib.exported_symbols()
    fake = C.c_void_p(4096)   # never dereferenced: every case below fails validation before any HIP call
    ptrs = (C.c_void_p * 2)(fake, fake)
    null_ptrs = (C.c_void_p * 2)(fake, None)
    hs, ws = (C.c_int * 2)(24, 37), (C.c_int * 2)(32, 53)
    nbytes = lib.aon_ssim_workspace_bytes(2, hs, ws)
    assert nbytes == 8 * (1 * 1 + 2 * 2)   # 16 x 32 output tiles: (14 x 22) -> 1 x 1, (27 x 43) -> 2 x 2
    assert lib.aon_ssim(0, None, None, None, None, None, 0, None, None) == 0
    assert lib.aon_ssim(-1, ptrs, ptrs, hs, ws, fake, nbytes, fake, None) == -1
    assert b"n_images" in lib.aon_last_error()
    for args in ((None, ptrs, hs, ws, fake, nbytes, fake), (ptrs, ptrs, hs, ws, fake, nbytes, None), (ptrs, ptrs, hs, ws, None, nbytes, fake)):
        assert lib.aon_ssim(2, *args, None) == -1
        assert b"null pointer" in lib.aon_last_error()
    assert lib.aon_ssim(2, ptrs, null_ptrs, hs, ws, fake, nbytes, fake, None) == -1
    assert b"null image pointer" in lib.aon_last_error()
    for h, w in ((10, 32), (24, 10), (0, 0)):
        small_h, small_w = (C.c_int * 2)(h, 37), (C.c_int * 2)(w, 53)
        assert lib.aon_ssim(2, ptrs, ptrs, small_h, small_w, fake, 1 << 20, fake, None) == -1
        assert b"11 <= h, w" in lib.aon_last_error()
        assert lib.aon_ssim_workspace_bytes(2, small_h, small_w) == -1
    assert lib.aon_ssim(2, ptrs, ptrs, hs, ws, fake, nbytes - 8, fake, None) == -2
    assert b"workspace too small" in lib.aon_last_error()


def test_ops_ssim_rejects_cpu_tensors():
    from aon_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim([torch.zeros(16, 16, 3)], [torch.zeros(16, 16, 3)])
