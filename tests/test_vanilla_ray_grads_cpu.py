"""Ray gradients of a frozen vanilla network / LitNeRF.fit_pose, what can be checked without a GPU: the extension
header include/aon_hip_inputs.h against the library and the binding (the discipline tests/test_abi_cpu.py, tests/test_bwd_call_cpu.py and
tests/test_guard_cpu.py keep for include/aon_hip.h), every refusal aon_render_bwd_inputs makes before a launch -- code, message, rank -- on
fake pointers, fit_pose's argument rules, and the oracle's own pose loop on the field the GPU test fits."""
import ctypes as C
import itertools
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-written: p = c_void_p, i = c_int, l = c_int64
EXT_ARGTYPES = {
    "aon_render_bwd_inputs": (C.c_int, "p p p p p l i i p p p p p p l p l p p p"),
    "aon_train_scratch_bytes_inputs_vanilla": (C.c_int64, "l i p"),
}


def _stripped(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def ext_declared_symbols():
    return sorted(set(re.findall(r"\b(aon_[a-z_0-9]+)\s*\(", _stripped("aon_hip_inputs.h"))))


def ext_stream_entry_points():
    return sorted({m.group(1) for m in re.finditer(r"\b(aon_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", _stripped("aon_hip_inputs.h"), flags=re.S)
                   if re.search(r"\bstream\b", m.group(2))})


def test_extension_header_library_and_binding_agree():
    from aon_amd import _lib
    from test_abi_cpu import declared_symbols

    names = ext_declared_symbols()
    assert names == sorted(EXT_ARGTYPES) == _lib.extension_symbols()
    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    for n in names:
        assert hasattr(_lib.lib, n), f"{n} declared in aon_hip_inputs.h but not exported"
        fn = getattr(_lib.lib, n)
        res, letters = EXT_ARGTYPES[n]
        assert fn.restype is res and list(fn.argtypes) == [kinds[k] for k in letters.split()], n
        assert list(_lib._EXT_SIGS[n][1]) == list(fn.argtypes), n
    # the main header and its table do not know them
    assert not set(names) & set(declared_symbols()) and not set(names) & set(_lib.exported_symbols())
    assert '#include "aon_hip.h"' in open(os.path.join(ROOT, "include", "aon_hip_inputs.h")).read()
    assert _lib.lib.aon_abi_version() == 5


def test_every_stream_entry_point_of_the_extension_header_is_in_a_guard_case():
    import test_hip_vanilla_ray_grads as gpu

    names = ext_stream_entry_points()
    assert names == ["aon_render_bwd_inputs"]
    reached = set().union(*(set(c.reaches) for c in gpu.GUARD_CASES))
    assert not set(names) - reached
    assert {c.name for c in gpu.GUARD_CASES} >= {"vanilla_inputs_n1_default_deg0_10_4", "vanilla_inputs_n5_small_deg0_10_4", "vanilla_inputs_n37_default_deg0_10_4",
                                                 "vanilla_inputs_n5_small_deg1_8_3"}


# ---- the refusal table (as tests/test_bwd_call_cpu.py) ----
N = 3
BASE = 0x7B000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced, far from the ones other tests declare forms for
ORDER = ["bwd_c", "mate_c", "bwd_f", "mate_f", "rays_d", "n", "white", "levels", "g_rgb", "g_acc", "g_depth", "params_c", "params_f", "ws", "ws_bytes",
         "scratch", "scratch_bytes", "stream", "opts", "rg"]
WHO = "aon_render_bwd_inputs"
FORMS_MSG = "forward and transposed streams were packed in different forms (aon_set_bottleneck_fold changed in between)"
INVALID, WORKSPACE = -1, -2


def _fake(i):
    return BASE + 0x1000 * i


def _array(n, hole=None, start=100):
    return (C.c_void_p * n)(*[0 if i == hole else _fake(start + i) for i in range(n)])


def _only(n, entries, start=100):
    """an array with nothing but `entries` set: what the call reads"""
    return (C.c_void_p * n)(*[_fake(start + i) if i in entries else 0 for i in range(n)])


class Entry:
    def __init__(self):
        from aon_amd import _lib

        self.lib, self._lib = _lib.lib, _lib
        self.rg = _lib.RayGradsC(_fake(40), _fake(41), _fake(42), _fake(43), _fake(44))
        a = {k: None for k in ORDER}
        a.update(bwd_c=_fake(20), mate_c=_fake(21), bwd_f=_fake(22), mate_f=_fake(23), rays_d=_fake(1), n=N, white=1, levels=2, g_rgb=_array(2, start=10),
                 params_c=_only(24, (0, 10, 16), 400), params_f=_array(24, start=500), ws=_fake(2), scratch=_fake(3), rg=C.byref(self.rg))
        a["ws_bytes"] = self.lib.aon_train_workspace_bytes(N, 0, 2)
        a["scratch_bytes"] = self.lib.aon_train_scratch_bytes_inputs_vanilla(N, 2, None)
        assert a["ws_bytes"] > 0 and a["scratch_bytes"] > 0
        self.base = a

    def rows(self):
        """(label, overrides, rank, rc, message)"""
        r = [("n = 0", {"n": 0}, 1, INVALID, "bad size / num_levels"), ("num_levels = 3", {"levels": 3}, 1, INVALID, "bad size / num_levels"),
             ("rg = NULL", {"rg": None}, 2, INVALID, "null aon_ray_grads")]
        for i, member in enumerate(("rays_o", "viewdirs", "g_rays_o", "g_rays_d", "g_viewdirs")):
            vals = [_fake(40 + k) for k in range(5)]
            vals[i] = 0
            hole = self._lib.RayGradsC(*vals)
            r.append((f"null {member} in aon_ray_grads", {"rg": C.byref(hole), "_keep": hole}, 2, INVALID, "null member of aon_ray_grads"))
        r += [(k + " = NULL", {k: None}, 3, INVALID, "null pointer") for k in ("rays_d", "g_rgb", "ws", "scratch")]
        r += [("misaligned scratch", {"scratch": _fake(3) + 16}, 4, INVALID, "workspace / scratch must be 256-byte aligned"),
              ("misaligned workspace", {"ws": _fake(2) + 128}, 4, INVALID, "workspace / scratch must be 256-byte aligned"),
              ("workspace one byte short", {"ws_bytes": self.base["ws_bytes"] - 1}, 5, WORKSPACE, "workspace smaller than aon_train_workspace_bytes()"),
              ("scratch one byte short", {"scratch_bytes": self.base["scratch_bytes"] - 1}, 6, WORKSPACE,
               "scratch smaller than aon_train_scratch_bytes_inputs_vanilla()")]
        level = lambda l, kind: 10 + 10 * l + kind      # noqa: E731  (per level: null level pointer, forms, holes)
        r += [("bwd_c = NULL", {"bwd_c": None}, level(0, 0), INVALID, "null level pointer"),
              ("params_c = NULL", {"params_c": None}, level(0, 0), INVALID, "null level pointer"),
              ("mate_f = NULL", {"mate_f": None}, level(1, 0), INVALID, "null level pointer"),
              ("params_f = NULL", {"params_f": None}, level(1, 0), INVALID, "null level pointer"),
              ("g_rgb[1] = NULL", {"g_rgb": _array(2, 1, 10)}, level(1, 0), INVALID, "null level pointer"),
              ("mate_c in the other form", {"_form_mate_c": 0}, level(0, 1), INVALID, FORMS_MSG),
              ("bwd_f in the other form", {"_form_bwd_f": 0}, level(1, 1), INVALID, FORMS_MSG),
              ("params_c[0] = NULL", {"params_c": _array(24, 0, 400)}, level(0, 2), INVALID, "null parameter pointer"),
              ("params_c[10] = NULL", {"params_c": _array(24, 10, 400)}, level(0, 2), INVALID, "null parameter pointer"),
              ("params_f[16] = NULL", {"params_f": _array(24, 16, 500)}, level(1, 2), INVALID, "null parameter pointer")]
        return r

    def call(self, overrides):
        args = dict(self.base)
        args.update({k: v for k, v in overrides.items() if not k.startswith("_")})
        for key in ORDER[:4]:
            assert self.lib.aon_declare_stream_form(C.c_void_p(self.base[key]), overrides.get("_form_" + key, 1)) == 0
        rc = self.lib.aon_render_bwd_inputs(*[args[k] for k in ORDER])
        return rc, self.lib.aon_last_error().decode()


def _touched(overrides):
    return {k[len("_form_"):] if k.startswith("_form_") else k for k in overrides if k != "_keep"}


def test_every_prelaunch_refusal():
    e = Entry()
    rows = e.rows()
    assert len(rows) >= 26
    for label, overrides, _rank, rc, msg in rows:
        assert e.call(overrides) == (rc, f"{WHO}: {msg}"), label
    # (the coarse level's array of every row holds entries 0, 10 and 16 only: the rows that refuse at the fine level got past it)


def test_refusals_keep_their_rank():
    """Two faults at once: the refusal that ranks first is the one reported."""
    e = Entry()
    rows = e.rows()
    pairs = 0
    for a, b in itertools.combinations(rows, 2):
        if a[2] == b[2] or _touched(a[1]) & _touched(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], f"{WHO}: {first[4]}"), (a[0], b[0])
        pairs += 1
    assert pairs > 150


def test_scratch_query():
    from aon_amd import _lib

    lib = _lib.lib
    two, one = lib.aon_train_scratch_bytes_inputs_vanilla(37, 2, None), lib.aon_train_scratch_bytes_inputs_vanilla(37, 1, None)
    # d_raw (16 B) + gradient planes (2528 rows x 4 B) + record (128 B) per padded sample, 256-byte aligned pieces; no weight-gradient workspace
    per = 16 + 2528 * 4 + 128
    np_c, np_f = -(-37 * 65 // 128) * 128, -(-37 * 193 // 128) * 128
    assert one == np_c * per and two == (np_c + np_f) * per
    assert two < lib.aon_train_scratch_bytes(37, 0, 2) - lib.aon_wgrad_workspace_bytes()
    assert lib.aon_train_scratch_bytes_inputs_vanilla(0, 2, None) == lib.aon_train_scratch_bytes_inputs_vanilla(1, 2, None)


# ---- LitNeRF.fit_pose ----
def test_fit_pose_rejects_bad_arguments():
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    lit = LitNeRF(randomized=False)
    batch = {"directions": torch.zeros(4, 3), "target": torch.zeros(4, 3)}
    pose = syn.look_at_pose()
    for steps in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            lit.fit_pose([batch], steps, poses=[pose])
    with pytest.raises(ValueError, match="no batches"):
        lit.fit_pose([], 3, poses=[])
    with pytest.raises(ValueError, match="one .3, 4. pose per view"):
        lit.fit_pose([batch], 3, poses=[pose, pose])
    with pytest.raises(ValueError, match="one .3, 4. pose per view"):
        lit.fit_pose([batch], 3)
    for lr in (0.0, -1e-3, (1e-3, 1e-3)):
        with pytest.raises(ValueError, match="lr"):
            lit.fit_pose([batch], 3, lr=lr, poses=[pose])
    with pytest.raises(ValueError, match="'directions'"):
        lit.fit_pose([{"rays_o": torch.zeros(4, 3), "target": torch.zeros(4, 3)}], 3, poses=[pose])
    with pytest.raises(ValueError, match=r"\(3, 4\) matrix"):
        lit.fit_pose([batch], 3, poses=[torch.eye(3)])
    with pytest.raises(NotImplementedError, match="ray box"):
        LitNeRF(randomized=False, ray_box=2.0).fit_pose([batch], 3, poses=[pose])
    assert all(p.requires_grad for p in lit.model.parameters())


def test_the_oracle_pose_loop_converges_on_the_fit_pose_field():
    """The bar of the GPU test (both errors below half their start after 60 steps) is one the reference's own arithmetic meets with margin:
    its fp64 loop ends below a quarter of both."""
    import aon_amd.synthetic as syn
    from aon_amd import ops

    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc
    import test_hip_vanilla_ray_grads as gpu

    FIT = gpu.FIT
    H, W = FIT["H"], FIT["W"]
    sd = {k: v.double() for k, v in gpu.fit_pose_field().items()}
    true = syn.look_at_pose(4.0, 40.0, 25.0)
    start = ops.apply_pose_correction(true.double(), torch.tensor(FIT["correction"], dtype=torch.float64))
    # ops.ray_directions is a HIP kernel: the same camera-space directions from their definition (datasets/ray_utils.py get_ray_directions)
    f = syn.focal_from_fovy(H)
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dirs = torch.stack([(i - W / 2) / f, -(j - H / 2) / f, -torch.ones_like(i)], -1).reshape(-1, 3)
    with torch.no_grad():
        o, d = ops.rays_from_pose(dirs, true.double())
        target = orc.nerf_forward(sd, {"rays_o": o, "rays_d": d, "viewdirs": d}, False, True, 2.0, 6.0, num_levels=1, num_coarse_samples=32, **FIT["degrees"])[0][0]
    losses, fitted = gpu.oracle_pose_loop(sd, dirs, target, start, torch.float64, FIT["steps"])
    e0, e1 = gpu.pose_errors(start, true.double()), gpu.pose_errors(fitted, true.double())
    print(f"oracle fp64: rotation {e0[0]:.4f} -> {e1[0]:.4f} degrees, translation {e0[1]:.5f} -> {e1[1]:.5f}; loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert 1.9 < e0[0] < 2.2 and 0.045 < e0[1] < 0.055
    assert e1[0] < 0.25 * e0[0] and e1[1] < 0.25 * e0[1], (e0, e1)
    assert losses[-1] < 0.01 * losses[0]
