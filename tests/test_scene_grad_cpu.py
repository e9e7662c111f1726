"""Gradients through scenes, what can be checked without a GPU: the torch restatement tests/_scene_grad_ref.py against
tests/_scene_ref.composite_ref and against central differences, the extension header include/aon_hip_scene_grad.h against the library and the
binding, every refusal of aon_scene_composite_bwd -- code, message, rank -- on fake pointers, and the argument rules of
scene.render_scene_grad and LitNeRF_AutoDecoder.fit_scene_codes."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_grad_ref as gref  # noqa: E402
import _scene_ref as sref  # noqa: E402
from test_scene_cpu import INVALID, _Entry, _fake, _latents, _pose  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene_grad.h"


# ---- the torch restatement ----
def tie_case(seed=3):
    """(n, K, S) = (5, 2, 3): rays 0..3 cross object 0, rays 1..4 object 1; on ray 1 a sample of each list has the same t"""
    n, K, S = 5, 2, 3
    rng = np.random.default_rng(seed)
    slot = np.full((n, K), -1, np.int32)
    slot[:4, 0] = np.arange(4)
    slot[1:, 1] = 4 + np.arange(4)
    P = 8
    t = np.sort(rng.uniform(2.0, 6.0, (P, S)), -1).astype(np.float32)
    t[4, 1] = t[1, 1]                                   # ray 1: object 0's row 1, object 1's row 4
    t[4] = np.sort(t[4])
    raw = rng.normal(0.0, 1.5, (P, S, 4)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    return raw, t, slot, dirs


def test_the_restatement_is_composite_ref():
    raw, t, slot, dirs = tie_case()
    assert t[4, list(t[4]).index(t[1, 1])] == t[1, 1]
    order = [(k, i) for _, k, i, _ in sref.merge_order(t, slot[1])]
    idx, kk = gref.merge_index(t, slot[1], 8)
    assert [(int(k), int(f % 3)) for f, k in zip(idx, kk)] == order                      # the tie: object 0's sample first
    for white in (True, False):
        want = sref.composite_ref(raw, t, slot, dirs, white, dtype=np.float64)
        got = gref.composite_torch(torch.from_numpy(raw.astype(np.float64)), t, slot, dirs, white, round32=False)
        for key in ("rgb", "acc", "depth", "obj_acc", "weights"):
            assert np.abs(got[key].numpy() - want[key]).max() <= 1e-12, key
        # the kernel's function (delta and raw + bias rounded in fp32) is the same function up to those roundings
        k32 = gref.composite_torch(torch.from_numpy(raw.astype(np.float64)), t, slot, dirs, white, round32=True)
        for key in ("rgb", "acc", "depth", "obj_acc", "weights"):
            assert np.abs(k32[key].numpy() - want[key]).max() <= 5e-6, key


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
def test_the_restatements_gradient_is_the_central_difference(white, act):
    raw, t, slot, dirs = tie_case()
    if act == 0:
        raw[..., 3] = np.abs(raw[..., 3])               # a raw density, not a pre-activation
    rng = np.random.default_rng(9)
    g = dict(g_rgb=rng.normal(size=(5, 3)), g_acc=rng.normal(size=5), g_depth=rng.normal(size=5), g_obj_acc=rng.normal(size=(5, 2)))
    pairs = (("rgb", g["g_rgb"]), ("acc", g["g_acc"]), ("depth", g["g_depth"]), ("obj_acc", g["g_obj_acc"]))

    def loss(x):      # round32=False: a perturbed fp64 raw has no fp32 value whose rounding of raw + bias could be kept fixed
        out = gref.composite_torch(x, t, slot, dirs, white, act=act, round32=False)
        return sum((out[k] * torch.from_numpy(v)).sum() for k, v in pairs)

    x0 = raw.astype(np.float64)
    xt = torch.from_numpy(x0.copy()).requires_grad_(True)
    got, = torch.autograd.grad(loss(xt), xt)
    got = got.numpy()
    # the kernel's form (delta and raw + bias rounded in fp32) runs the same graph on inputs 1e-7 apart
    k32 = gref.composite_grads(raw, t, slot, dirs, white, act=act, **g).numpy()
    assert np.abs(k32 - got).max() <= 1e-5 * np.abs(got).max()
    h, fd = 1e-6, np.zeros_like(x0)
    for j in np.ndindex(*x0.shape):
        if act == 1 and j[-1] == 3 and abs(x0[j]) < 10 * h:
            continue
        up, dn = x0.copy(), x0.copy()
        up[j] += h
        dn[j] -= h
        fd[j] = (float(loss(torch.from_numpy(up))) - float(loss(torch.from_numpy(dn)))) / (2 * h)
    assert np.abs(got).max() > 1e-2
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(got).max(), np.abs(got - fd).max() / np.abs(got).max()
    assert not got[:, -1].any()                                                          # the last sample of every list: delta = 0


def test_sentinel_records_and_dead_rows_get_zeros():
    raw, t, slot, dirs = tie_case()
    raw[2, 1] = (0.0, 0.0, 0.0, -np.inf)
    slot[3, 0] = -1                                     # row 3 is nobody's now
    g = gref.composite_grads(raw, t, slot, dirs, True, np.ones((5, 3)), np.ones(5), np.ones(5), np.ones((5, 2))).numpy()
    assert np.isfinite(g).all() and not g[2, 1].any() and not g[3].any() and g[2, 0].any()


# ---- header, library, binding ----
GRAD_ARGTYPES = {"aon_scene_composite_bwd": (C.c_int, "p p p p p p p p l i l i i i p p p")}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def grad_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))


def test_scene_grad_header_library_and_binding_agree():
    from aon_amd import _lib
    from test_abi_cpu import declared_symbols
    from test_scene_cpu import scene_declared_symbols
    from test_vanilla_ray_grads_cpu import ext_declared_symbols

    names = grad_declared_symbols()
    assert names == sorted(GRAD_ARGTYPES) == _lib.scene_grad_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = GRAD_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_GRAD_SIGS[n][1]) == list(fn.argtypes), n
    others = (set(declared_symbols()) | set(ext_declared_symbols()) | set(scene_declared_symbols()) | set(_lib.exported_symbols())
              | set(_lib.extension_symbols()) | set(_lib.scene_symbols()) | set(_lib.scene_occ_symbols()))
    occ = set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped("aon_hip_scene_occ.h")))
    assert not set(names) & (others | occ)
    assert '#include "aon_hip_scene.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5


# ---- the refusal table ----
class BwdEntry(_Entry):
    WHO = "aon_scene_composite_bwd"
    ORDER = ["raw", "t_vals", "slot", "rays_d", "g_rgb", "g_acc", "g_depth", "g_obj_acc", "n", "k", "pairs", "s", "white", "act", "opts", "d_raw", "stream"]
    POINTERS = ["raw", "t_vals", "slot", "rays_d", "g_rgb", "d_raw"]

    def __init__(self):
        from aon_amd import _lib

        self.lib = _lib.lib
        a = {k: _fake(i + 40) for i, k in enumerate(self.POINTERS + ["g_acc", "g_depth", "g_obj_acc"])}
        a.update(n=37, k=3, pairs=50, s=65, white=1, act=2, opts=None, stream=None)
        self.base = a

    def rows(self):
        bad, who = "bad size / object count / act (1 <= k <= 16, s >= 2, k * s <= 4096)", self.WHO
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("pairs = -1", {"pairs": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad),
             ("k = 17", {"k": 17}, 1, INVALID, bad), ("s = 1", {"s": 1}, 1, INVALID, bad), ("k * s = 4097", {"k": 1, "s": 4097}, 1, INVALID, bad),
             ("k * s = 4112", {"k": 16, "s": 257}, 1, INVALID, bad), ("act = 3", {"act": 3}, 1, INVALID, bad), ("act = -1", {"act": -1}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS]
        r += [("misaligned raw", {"raw": _fake(40) + 8}, 3, INVALID, "raw must be 16-byte aligned"),
              ("misaligned d_raw", {"d_raw": _fake(45) + 4}, 4, INVALID, "d_raw must be 16-byte aligned")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


def test_every_prelaunch_refusal_of_the_backward():
    e = BwdEntry()
    rows = e.rows()
    assert len(rows) >= 16
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label


def test_the_backwards_refusals_keep_their_rank():
    e = BwdEntry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > 50


def test_empty_backward_calls_succeed_without_a_launch():
    e = BwdEntry()
    for empty in ({"n": 0}, {"pairs": 0}, {"n": 0, "pairs": 0}):
        assert e.call(empty)[0] == 0, empty
    assert e.call({"g_acc": None, "g_depth": None, "g_obj_acc": None, "n": 0})[0] == 0      # the optional three


# ---- scene.render_scene_grad / LitNeRF_AutoDecoder.fit_scene_codes ----
def test_render_scene_grad_argument_errors():
    from aon_amd import ops, scene
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ok = scene.SceneObject(_latents(), _pose(), 2.0)
    model = NeRF_AE_Art()
    rays = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs")}
    with pytest.raises(ValueError, match="randomized=True is refused"):
        scene.render_scene_grad(model, [ok], rays, True, randomized=True)
    with pytest.raises(NotImplementedError, match="no density noise"):
        scene.render_scene_grad(NeRF_AE_Art(noise_std=0.5), [ok], rays, True)
    model.num_levels = 3
    with pytest.raises(NotImplementedError, match="one or two levels"):
        scene.render_scene_grad(model, [ok], rays, True)
    model.num_levels = 2
    with pytest.raises(ValueError, match="1 to 16 objects, got 0"):
        scene.render_scene_grad(model, [], rays, True)
    with pytest.raises(TypeError, match="SceneObject"):
        scene.render_scene_grad(model, [(_pose(), 2.0)], rays, True)
    grid = ops.OccupancyGrid.__new__(ops.OccupancyGrid)
    with_grid = scene.SceneObject(_latents(), _pose(), 2.0)
    with_grid.grid = grid
    with pytest.raises(NotImplementedError, match="dense only: object 1 carries an occupancy grid"):
        scene.render_scene_grad(model, [ok, with_grid], rays, True)
    # render_scene keeps its refusal under grad mode, and its words
    with pytest.raises(RuntimeError, match="scene rendering is inference only: call it under torch.no_grad\\(\\)"):
        scene.render_scene(model, [ok], rays, True)


def test_fit_scene_codes_argument_errors():
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder({"N_max_objs": 2}, randomized=False)
    batch = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs", "target")}
    good = [(0, 4, _pose(), 1.4)]
    flags = [p.requires_grad for p in lit.model.parameters()]
    with pytest.raises(ValueError, match="steps must be a positive int"):
        lit.fit_scene_codes([batch], good, 0)
    with pytest.raises(ValueError, match="no batches"):
        lit.fit_scene_codes([], good, 3)
    with pytest.raises(ValueError, match="lr must be positive"):
        lit.fit_scene_codes([batch], good, 3, lr=0.0)
    with pytest.raises(ValueError, match="fit_keys must name some of"):
        lit.fit_scene_codes([batch], good, 3, fit_keys=("pose",))
    with pytest.raises(ValueError, match="fit_keys must name some of"):
        lit.fit_scene_codes([batch], good, 3, fit_keys=())
    with pytest.raises(ValueError, match="1 to 16 objects, got 0"):
        lit.fit_scene_codes([batch], [], 3)
    with pytest.raises(ValueError, match="fit_scene_codes: placement 0: instance_id 5 outside the library"):
        lit.fit_scene_codes([batch], [(5, 0, _pose(), 1.0)], 3)
    with pytest.raises(ValueError, match="fit_scene_codes: placement 0: articulation row 19 outside"):
        lit.fit_scene_codes([batch], [(0, 19, _pose(), 1.0)], 3)
    with pytest.raises(ValueError, match="fit_scene_codes: placement 0 must be"):
        lit.fit_scene_codes([batch], [(0, 1, _pose())], 3)
    with pytest.raises(ValueError, match="not orthonormal"):
        lit.fit_scene_codes([batch], [(0, 1, _pose(1.01 * torch.eye(3)), 1.0)], 3)
    with pytest.raises(ValueError, match="every batch needs"):
        lit.fit_scene_codes([{k: v for k, v in batch.items() if k != "target"}], good, 3)
    assert [p.requires_grad for p in lit.model.parameters()] == flags
