"""CPU: the early-ray-termination convention through its numpy reference against a brute-force per-ray loop, and
the C ABI / Python surface that needs no GPU: exported symbols, the refusals, the workspace size."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _stop_ref as ref

AON_E_INVALID = -1
NAMES = ("aon_render_stop_workspace_bytes", "aon_render_fwd_stop", "aon_art_render_fwd_stop")


# ---------------------------------------------------------------------------------------------------------------- the numpy reference
def _brute_stop(sigma, delta, eps, R):
    """One ray, python scalars of np.float32: the convention read literally."""
    S = len(sigma)
    ts = np.float32(-math.log(float(np.float32(eps)))) if eps > 0 else np.float32(np.inf)
    tau, k = np.float32(0), 0
    while True:
        s0, s1 = k * R, min(S, (k + 1) * R)
        if s1 == S:
            return S
        for i in range(s0, s1):
            tau = np.float32(tau + np.float32(np.float32(sigma[i]) * np.float32(delta[i])))
        if tau >= ts:
            return s1
        k += 1


@pytest.mark.parametrize("S", [65, 193, 41, 73])
@pytest.mark.parametrize("R", [1, 16, 48, 64, 500])
def test_reference_matches_brute_force(S, R):
    rng = np.random.default_rng(S * 1000 + R)
    n = 60
    t = np.sort(rng.uniform(2, 6, (n, S)).astype(np.float32), axis=1)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    raw = (rng.normal(size=(n, S)) * rng.uniform(0, 40, (n, 1))).astype(np.float32)
    raw[rng.random((n, S)) < 0.2] = -np.inf                  # sentinels
    sigma, delta = ref.relu_sigma(raw), ref.deltas(t, d)
    assert (sigma[np.isneginf(raw)] == 0).all()
    for eps in (1e-2, 1e-4, 0.0):
        got = ref.stops(sigma, delta, eps, R)
        want = [_brute_stop(sigma[r], delta[r], eps, R) for r in range(n)]
        assert got.tolist() == want
        assert all(s == S or (s % R == 0 and s < S) for s in want)
        if eps == 0.0:
            assert (got == S).all()
    if R >= S:
        assert (ref.stops(sigma, delta, 1e-2, R) == S).all()      # one round: nothing decides


def test_reference_details():
    assert ref.tau_stop(0.0) == np.inf
    assert ref.tau_stop(1e-3) == np.float32(-np.log(np.float64(np.float32(1e-3))))
    assert ref.num_rounds(193, 32) == 7 and ref.num_rounds(64, 16) == 4
    d = np.array([[3.0, 4.0, 12.0]], np.float32)
    assert ref.dir_norm(d)[0] == np.float32(13.0)
    t = np.array([[2.0, 2.5, 4.0]], np.float32)
    assert ref.deltas(t, d).tolist() == [[6.5, 19.5, float(np.float32(1e10) * np.float32(13.0))]]
    # NaN never stops and propagates; a stopped ray is not updated
    sigma = np.array([[np.nan, 100, 100, 100, 0], [100, 0, 0, 0, 0]], np.float32)
    delta = np.ones((2, 5), np.float32)
    assert ref.stops(sigma, delta, 1e-2, 2).tolist() == [5, 2]
    b = ref.boundary_tau64(np.ones((1, 5)), np.ones((1, 5)), 2)
    assert b.tolist() == [[2.0, 4.0]]
    assert ref.live_mask(np.array([2, 5]), 5).sum(1).tolist() == [2, 5]
    assert ref.sigma64(np.array([-np.inf, 0.0]), "softplus", -1.0).tolist() == [0.0, math.log1p(math.exp(-1.0))]


# ---------------------------------------------------------------------------------------------------------------- C ABI without a GPU
def test_symbols_exported_and_workspace_size():
    from aon_amd import _lib, ops

    for name in NAMES:
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    lib = _lib.lib
    assert lib.aon_abi_version() == 5
    prev = 0
    for n in (1, 2, 97, 1000, 3840, 100000):
        occ = lib.aon_render_occ_workspace_bytes(n, None)
        stop = lib.aon_render_stop_workspace_bytes(n, None)
        assert stop >= occ + 8 * n            # tau and stop: 8 B per ray
        assert stop <= occ + 8 * n + 2 * 256
        assert stop >= prev
        prev = stop
    st, _ = ops.RenderOpts(num_coarse_samples=40, num_fine_samples=72).c_struct(2.0, 6.0)
    assert lib.aon_render_stop_workspace_bytes(500, ctypes.byref(st)) >= lib.aon_render_occ_workspace_bytes(500, ctypes.byref(st)) + 4000
    st.num_coarse_samples = 1
    assert lib.aon_render_stop_workspace_bytes(500, ctypes.byref(st)) == AON_E_INVALID


def _occ_struct(bits=0x1000):
    from aon_amd import _lib

    st = _lib.OccupancyC()
    st.bits = bits
    for a in range(3):
        st.cells[a], st.lo[a], st.step[a] = 4, -1.0, 0.5
    return st


def _render(fn, art, occ, eps=1e-3, R=32, t_rand=None, opts=None):
    n_ptrs = 4 if art else 2
    fake = ctypes.c_void_p(0x1000)
    args = [fake] * n_ptrs + [fake, fake, fake, 8, 2.0, 6.0, 1, 2, t_rand, fake, 0] + [fake] * 6 + [fake, 1 << 30, None, opts,
                                                                                                  None if occ is None else ctypes.byref(occ), None,
                                                                                                  ctypes.c_float(eps), R, None]
    return fn(*args)


def test_render_refusals_before_any_launch():
    from aon_amd import _lib, ops

    lib = _lib.lib
    for fn, art in ((lib.aon_render_fwd_stop, False), (lib.aon_art_render_fwd_stop, True)):
        for eps in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
            for occ in (None, _occ_struct()):
                assert _render(fn, art, occ, eps=eps) == AON_E_INVALID
                assert b"eps" in lib.aon_last_error()
        for R in (0, -3):
            assert _render(fn, art, None, R=R) == AON_E_INVALID
            assert b"round_samples" in lib.aon_last_error()
        # a grid that is given must be a good one; a null grid is allowed (and gets past these checks to the null-pointer ones)
        assert _render(fn, art, _occ_struct(bits=0)) == AON_E_INVALID
        assert b"null occupancy grid" in lib.aon_last_error()
        bad = _occ_struct()
        bad.step[1] = 0.0
        assert _render(fn, art, bad) == AON_E_INVALID
        for occ in (None, _occ_struct()):
            for eps in (0.0, 1e-3):
                assert _render(fn, art, occ, eps=eps, t_rand=ctypes.c_void_p(0x1000)) == AON_E_INVALID
                assert b"t_rand" in lib.aon_last_error()
                st, _ = ops.RenderOpts(noise_std=1.0).c_struct(2.0, 6.0)
                st.noise_std, st.noise_c = 1.0, 0x1000
                assert _render(fn, art, occ, eps=eps, opts=ctypes.byref(st)) == AON_E_INVALID
                assert b"noise" in lib.aon_last_error()
    st, _ = ops.RenderOpts(degrees=(0, 8, 4)).c_struct(2.0, 6.0)
    assert _render(lib.aon_render_fwd_stop, False, None, opts=ctypes.byref(st)) == AON_E_INVALID
    assert b"degrees" in lib.aon_last_error()


def test_python_wrappers_raise_on_bad_arguments():
    from aon_amd import ops
    from aon_amd.occupancy import render_image

    x = torch.zeros(4, 3)
    with pytest.raises(TypeError):
        ops.render_fwd_stop(None, None, x, x, x, 2.0, 6.0, True, "not a grid", 1e-3)
    for eps in (-1e-3, 1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.render_fwd_stop(None, None, x, x, x, 2.0, 6.0, True, None, eps)
        with pytest.raises(ValueError):
            ops.art_render_fwd_stop(None, None, None, None, x, x, x, 2.0, 6.0, True, None, eps)
    with pytest.raises(ValueError):
        ops.render_fwd_stop(None, None, x, x, x, 2.0, 6.0, True, None, 1e-3, round_samples=0)
    with pytest.raises(ValueError):
        ops.render_fwd_stop(None, None, x, x, x, 2.0, 6.0, True, None, 1e-3, num_levels=3)
    with pytest.raises(ValueError):
        render_image(None, torch.eye(4), 4, 4, 5.0, 2.0, 6.0, None)      # neither a grid nor early_stop
    assert ops.DEFAULT_ROUND_SAMPLES in (16, 32, 48, 64)
