"""Gradients through scenes with a backdrop, what can be checked without a GPU: the torch restatement
tests/_scene_lists_grad_ref.py against tests/_scene_lists_ref.composite_ref (forward, 1e-12), against tests/_scene_grad_ref.composite_grads
(homogeneous closed lists: exactly) and against central differences; the extension header include/aon_hip_scene_lists_grad.h against the
library and the binding; every refusal of the entry point -- code, message, rank -- on fake pointers; every Python refusal of
scene.render_scene_background_grad; and the harness methods' new keyword."""
import ctypes as C
import inspect
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scene_grad_ref as gref  # noqa: E402
import _scene_lists_grad_ref as lgref  # noqa: E402
import _scene_lists_ref as lref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "aon_hip_scene_lists_grad.h"
CUSTOM = {"rgb_padding": 0.01, "density_bias": 0.5}


# ---- the restatement against what exists ----
def _inputs(seed, n, K, S, dead=True):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(2.0, 6.0, (n * K, S)), -1).astype(np.float32)
    raw = rng.normal(0.0, 1.5, (n * K, S, 4)).astype(np.float32)
    slot = np.stack([np.arange(n) + n * k for k in range(K)], 1).astype(np.int32)
    if dead and K > 1:
        slot[::3, 1] = -1
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    g = dict(g_rgb=rng.normal(size=(n, 3)), g_acc=rng.normal(size=n), g_depth=rng.normal(size=n), g_obj_acc=rng.normal(size=(n, K)))
    return raw, t, slot, dirs, {k: v.astype(np.float32) for k, v in g.items()}


MIXED = [(lref.ACT_NONE, None, False), (lref.ACT_VANILLA, None, False), (lref.ACT_ARTICULATED, CUSTOM, False), (lref.ACT_VANILLA, None, True)]


def test_forward_is_the_numpy_restatement():
    n, S = 6, 9
    raw, t, slot, dirs, _ = _inputs(41, n, 4, S)
    raw[:, :, 3] = np.abs(raw[:, :, 3])                 # act 0 takes raw sigma as it is: keep it a density
    raw[n * 3:, -1, 3] = [0.0, 40.0, -3.0, 1.0, 2.0, 0.5]        # the open list's last sample: exactly 0, large, relu-off, ordinary
    for white in (True, False):
        ref = lref.composite_ref(raw, t, slot, dirs, white, MIXED, np.float64)
        got = lgref.composite_torch(torch.from_numpy(raw.astype(np.float64)), t, slot, dirs, white, MIXED, round32=False)
        for key in ("rgb", "acc", "depth", "obj_acc", "weights"):
            assert np.abs(got[key].numpy() - ref[key]).max() <= 1e-12, (key, white)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_homogeneous_closed_lists_give_the_scene_restatements_gradient_exactly(act):
    n, K, S = 5, 3, 7
    raw, t, slot, dirs, g = _inputs(42 + act, n, K, S)
    slot[1, :] = -1
    for opts in (None, CUSTOM):
        for white in (True, False):
            want = gref.composite_grads(raw, t, slot, dirs, white, g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"], opts=opts, act=act)
            got = lgref.composite_grads(raw, t, slot, dirs, white, [(act, opts, False)] * K, g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"])
            assert torch.equal(got, want) and bool(want.any()), (act, white)
            assert not got[:, S - 1].any()              # the closed last interval: exact zeros


def _fd_case(name):
    """-> (raw, t, slot, dirs, g, lists).  Every vanilla list's raw sigma is kept at |raw| >= 0.1 (the relu kink is out of a step's reach),
    so an open list's last interval is either exactly off (relu: both sides 0) or saturated (exp(-sigma 1e10 N) = 0)."""
    n, S = 3, 5
    if name == "mixed_acts":
        lists = [(0, None, False), (1, None, False), (2, CUSTOM, False)]
    elif name == "tie":
        lists = [(2, None, False), (1, None, True)]
    elif name == "open_in_the_middle":
        lists = [(2, None, False), (1, None, True), (2, CUSTOM, False)]
    else:
        lists = [(1, None, True)]
    K = len(lists)
    raw, t, slot, dirs, g = _inputs(50 + K + len(name), n, K, S, dead=False)
    for k, (act, _o, _e) in enumerate(lists):
        rows = slice(n * k, n * (k + 1))
        if act == 0:
            raw[rows, :, 3] = np.abs(raw[rows, :, 3]) + 0.05
        if act == 1:
            s = raw[rows, :, 3]
            raw[rows, :, 3] = np.where(np.abs(s) < 0.1, np.sign(s + 1e-9) * 0.1, s)
    if name == "tie":
        t[n:] = t[:n]                                   # every backdrop sample ties with the object's
    if name == "open_in_the_middle":
        t[n: 2 * n] = (t[n: 2 * n] - 2.0) * 0.5 + 2.0      # the open list ends at t <= 4: the others reach behind it
        raw[n: 2 * n, -1, 3] = [0.7, -0.4, 2.0]
    if name == "open_vanilla":
        raw[:, -1, 3] = [0.1, -0.1, 40.0]
    return raw, t, slot, dirs, g, lists


@pytest.mark.parametrize("name", ["mixed_acts", "tie", "open_in_the_middle", "open_vanilla"])
def test_gradient_against_central_differences(name):
    raw, t, slot, dirs, g, lists = _fd_case(name)
    n = slot.shape[0]
    h = 1e-4
    # the condition of the docstring, on the inputs actually used
    norm = np.linalg.norm(dirs.astype(np.float64), axis=1)
    for k, (act, _o, open_end) in enumerate(lists):
        s = raw[n * k: n * (k + 1), :, 3].astype(np.float64)
        if act == 1:
            assert np.abs(s).min() >= 0.1 > 10 * h
        if open_end:
            assert act == 1
            last = s[:, -1]
            assert ((last <= -0.1) | (np.maximum(last - h, 0) * 1e10 * norm > 800)).all()        # off, or exp(-x) = 0 in fp64 (x > 745.2)
    x0 = torch.from_numpy(raw.astype(np.float64))

    def loss(x, white):
        return lgref.loss_of(lgref.composite_torch(x, t, slot, dirs, white, lists, round32=False), g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"])

    rng = np.random.default_rng(3)
    directions = [torch.from_numpy(rng.uniform(-1, 1, raw.shape)) for _ in range(4)]
    for comp in range(4):                               # one component at a time too: colours and density separately
        e = torch.zeros(raw.shape, dtype=torch.float64)
        e[..., comp] = torch.from_numpy(rng.uniform(-1, 1, raw.shape[:2]))
        directions.append(e)
    last_only = torch.zeros(raw.shape, dtype=torch.float64)     # the last samples alone (an open list's last interval)
    last_only[:, -1] = 1.0
    directions.append(last_only)
    for white in (True, False):
        x = x0.clone().requires_grad_(True)
        grad, = torch.autograd.grad(loss(x, white), x)
        for i, v in enumerate(directions):
            fd = float(loss(x0 + h * v, white) - loss(x0 - h * v, white)) / (2 * h)
            an = float((grad * v).sum())
            scale = float((grad * v).abs().sum())
            # 1e-6 relative; under it the difference quotient's own rounding: each loss carries about 8 eps |L| from its sums, over 2 h
            floor = 16 * np.finfo(np.float64).eps * abs(float(loss(x0, white))) / (2 * h)
            assert abs(fd - an) <= max(1e-6 * scale, floor), (name, white, i, fd, an, floor)
        # the function the kernel evaluates (fp32 intervals, norm and raw + bias) has this derivative up to those roundings
        g32 = lgref.composite_grads(raw, t, slot, dirs, white, lists, g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"])
        assert float((g32 - grad).abs().max()) <= 2e-5 * float(grad.abs().max())
        # an open list's last density entry: exactly zero on both sides
        for k, (_a, _o, open_end) in enumerate(lists):
            if open_end:
                assert not g32[n * k: n * (k + 1), -1, 3].any() and g32[n * k: n * (k + 1), -1, :3].any()


# ---- header, library, binding ----
# hand-written: p = c_void_p, i = c_int, l = c_int64
ARGTYPES = {
    "aon_scene_composite_lists_bwd": (C.c_int, "p p p p p p p p l i l i i p p p"),
}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_header_library_and_binding_agree():
    from aon_amd import _lib

    names = sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped(HEADER))))
    assert names == sorted(ARGTYPES) == _lib.scene_lists_grad_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in {HEADER} but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._SCENE_LISTS_GRAD_SIGS[n][1]) == list(fn.argtypes), n
    others = (set(_lib.exported_symbols()) | set(_lib.extension_symbols()) | set(_lib.scene_symbols()) | set(_lib.scene_occ_symbols())
              | set(_lib.scene_grad_symbols()) | set(_lib.scene_pose_symbols()) | set(_lib.scene_lists_symbols()))
    assert not set(names) & others
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "aon_hip_scene_lists.h"' in text
    assert _lib.lib.aon_abi_version() == 5 and _lib.ABI_VERSION == 5
    build = open(os.path.join(ROOT, "articulated-object-nerf_amd", "build.py")).read()
    assert '"aon_scene_lists_grad.hip"' in build and '"aon_hip_scene_lists_grad.h"' in build
    tool = open(os.path.join(ROOT, "tools", "kernel_resources.py")).read()
    assert '"aon_scene_lists_grad.hip"' in tool


# ---- the refusal table ----
BASE = 0x7C000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced
INVALID = -1


def _fake(i):
    return BASE + 0x1000 * i


class Entry:
    """ORDER: the argument names in the ABI's order; base: a call that would be valid; rows(): (label, overrides, rank, rc, message)"""
    WHO = "aon_scene_composite_lists_bwd"
    ORDER = ["raw", "t_vals", "slot", "rays_d", "g_rgb", "g_acc", "g_depth", "g_obj_acc", "n", "k", "pairs", "s", "white", "lists", "d_raw", "stream"]
    POINTERS = ["raw", "t_vals", "slot", "rays_d", "g_rgb", "d_raw"]

    def __init__(self):
        from aon_amd import _lib

        self._lib = _lib
        self.lib = _lib.lib
        a = {k: _fake(i + 20) for i, k in enumerate(self.POINTERS + ["g_acc", "g_depth", "g_obj_acc"])}
        a.update(n=37, k=3, pairs=50, s=65, white=1, lists=self.records(), stream=None)
        self.base = a

    def records(self, k=16, **bad):
        arr = (self._lib.SceneListC * k)()
        for j in range(k):
            arr[j].act, arr[j].rgb_scale, arr[j].rgb_shift, arr[j].sigma_bias, arr[j].open_end = 2, 1.002, 0.001, -1.0, 0
        arr[k - 1].act, arr[k - 1].open_end = 1, 1
        for field, (j, value) in bad.items():
            setattr(arr[j], field, value)
        return arr

    def call(self, overrides):
        args = dict(self.base)
        args.update(overrides)
        rc = getattr(self.lib, self.WHO)(*[args[k] for k in self.ORDER])
        return rc, self.lib.aon_last_error().decode()

    def rows(self):
        bad, who = "bad size / list count (1 <= k <= 16, s >= 2, k * s <= 4096)", self.WHO
        rec = "bad list record (act in [0, 2], open_end 0 or 1)"
        r = [("n = -1", {"n": -1}, 1, INVALID, bad), ("pairs = -1", {"pairs": -1}, 1, INVALID, bad), ("k = 0", {"k": 0}, 1, INVALID, bad),
             ("k = 17", {"k": 17}, 1, INVALID, bad), ("s = 1", {"s": 1}, 1, INVALID, bad), ("k * s = 4097", {"k": 1, "s": 4097}, 1, INVALID, bad),
             ("k * s = 4112", {"k": 16, "s": 257}, 1, INVALID, bad)]
        r += [(k + " = NULL", {k: None}, 2, INVALID, "null pointer") for k in self.POINTERS + ["lists"]]
        r += [("act = 3 in record 0", {"lists": self.records(act=(0, 3))}, 3, INVALID, rec),
              ("act = -1 in record 2", {"lists": self.records(act=(2, -1))}, 3, INVALID, rec),
              ("open_end = 2 in record 1", {"lists": self.records(open_end=(1, 2))}, 3, INVALID, rec),
              ("open_end = -1 in record 2", {"lists": self.records(open_end=(2, -1))}, 3, INVALID, rec)]
        r += [("misaligned raw", {"raw": _fake(20) + 8}, 4, INVALID, "raw must be 16-byte aligned"),
              ("misaligned d_raw", {"d_raw": _fake(25) + 4}, 5, INVALID, "d_raw must be 16-byte aligned")]
        return [(label, o, rank, rc, f"{who}: {msg}") for label, o, rank, rc, msg in r]


def test_every_prelaunch_refusal():
    e = Entry()
    rows = e.rows()
    assert len(rows) >= 20
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, msg), label
    # only the k records of the call are read: a bad record past k is nobody's
    assert e.call({"n": 0, "lists": e.records(act=(3, 7))})[0] == 0


def test_refusals_keep_their_rank():
    """Two faults at once: the refusal that ranks first is the one reported."""
    e = Entry()
    pairs = 0
    for a, b in itertools.combinations(e.rows(), 2):
        if a[2] == b[2] or set(a[1]) & set(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], first[4]), (a[0], b[0])
        pairs += 1
    assert pairs > 50


def test_the_empty_calls_succeed_without_a_launch():
    e = Entry()
    assert e.call({"n": 0})[0] == 0
    assert e.call({"pairs": 0})[0] == 0
    assert e.call({"n": 0, "g_acc": None, "g_depth": None, "g_obj_acc": None})[0] == 0     # the nullable three


# ---- scene.render_scene_background_grad / render_scene_grad / the harness ----
def _latents():
    return {"density": torch.zeros(1, 128), "color": torch.zeros(1, 128), "articulation": torch.zeros(1, 32)}


def _pose():
    return torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)


def test_render_scene_background_grad_refusals():
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model import NeRF
    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art

    ob = scene.SceneObject(_latents(), _pose(), 2.0)
    model = NeRF_AE_Art()
    bg = scene.SceneBackground(NeRF(), 2.0, 6.0)
    rays = {k: torch.zeros(4, 3) for k in ("rays_o", "rays_d", "viewdirs")}
    f = scene.render_scene_background_grad
    assert list(inspect.signature(f).parameters)[:5] == ["model", "objects", "rays", "white_bkgd", "background"]
    with pytest.raises(ValueError, match="randomized=True is refused"):
        f(model, [ob], rays, True, bg, randomized=True)
    with pytest.raises(NotImplementedError, match="no density noise"):
        f(NeRF_AE_Art(noise_std=0.5), [ob], rays, True, bg)
    with pytest.raises(NotImplementedError, match="one or two levels"):
        three = NeRF_AE_Art()
        three.num_levels = 3            # (the constructor builds one or two)
        f(three, [ob], rays, True, bg)
    with pytest.raises(TypeError, match="SceneBackground"):
        f(model, [ob], rays, True, None)
    with pytest.raises(TypeError, match="SceneBackground"):
        f(model, [ob], rays, True, NeRF())
    with pytest.raises(ValueError, match="0 to 15 objects.*got 16"):
        f(model, [ob] * 16, rays, True, bg)
    with pytest.raises(TypeError, match="SceneObject instances"):
        f(model, [object()], rays, True, bg)
    with_grid = scene.SceneObject(_latents(), _pose(), 2.0)
    with_grid.grid = object()
    with pytest.raises(NotImplementedError, match="dense only: object 1 carries an occupancy grid"):
        f(model, [ob, with_grid], rays, True, bg)
    with pytest.raises(ValueError, match=r"backdrop runs 1 level\(s\), the scene model 2"):
        f(model, [ob], rays, True, scene.SceneBackground(NeRF(num_levels=1), 2.0, 6.0))
    with pytest.raises(ValueError, match=r"5136 merged samples per ray; the merged composite holds at most 4096"):
        f(NeRF_AE_Art(num_fine_samples=256), [ob] * 15, rays, True, bg)
    with pytest.raises(ValueError, match=r"level 1 are 4248 merged samples"):
        f(NeRF_AE_Art(num_coarse_samples=1023, num_fine_samples=1100), [ob], rays, True, bg)
    # the function without a backdrop keeps refusing one
    with pytest.raises(NotImplementedError, match="inference only"):
        scene.render_scene_grad(model, [ob], rays, True, background=bg)


def test_the_fit_methods_take_a_background():
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    for name in ("fit_scene_codes", "fit_scene_poses"):
        sig = inspect.signature(getattr(LitNeRF_AutoDecoder, name))
        assert list(sig.parameters)[-1] == "background" and sig.parameters["background"].default is None, name
    sig = inspect.signature(LitNeRF_AutoDecoder._scene_fit_loss)
    assert sig.parameters["background"].default is None
    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False, white_bkgd=True)
    for name in ("fit_scene_codes", "fit_scene_poses"):
        with pytest.raises(TypeError, match="background must be a scene.SceneBackground or None"):
            getattr(lit, name)([], [], 1, lr=1e-3, background=object())


def test_mlp_fwd_train_takes_an_out_buffer():
    from aon_amd import ops

    sig = inspect.signature(ops.mlp_fwd_train)
    assert list(sig.parameters) == ["packed", "rays_o", "rays_d", "viewdirs", "t_vals", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(ops.scene_composite_lists_bwd)
    assert list(sig.parameters) == ["raw", "t_vals", "pairs", "rays_d", "g_rgb", "g_acc", "g_depth", "g_obj_acc", "white_bkgd", "lists"]
