"""CPU: the seven whole-path backward entry points (the declarations of include/aon_hip.h with a `scratch_bytes` parameter).  Their ctypes
signatures against hand-written lists, and every refusal they make before a launch -- return code, message and rank among the other
refusals of the same entry point -- on fake pointers: no case reaches a HIP call."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The argtypes as the binding listed them by hand before they were assembled from pieces (_lib._BWD and friends):
# p = c_void_p, i = c_int, l = c_int64.
BWD_ARGTYPES = {
    "aon_render_bwd": "p p p p p l i i p p p p p p l p l p",
    "aon_render_bwd_ex": "p p p p p l i i p p p p p p l p l p p",
    "aon_art_render_bwd": "p p p p p l i i p p p p p p p p p p p p p p l p l p",
    "aon_art_render_bwd_ex": "p p p p p l i i p p p p p p p p p p p p p p l p l p p",
    "aon_art_render_bwd_latents": "p p p p p l i i p p p p p p p p p l p l p p",
    "aon_art_render_bwd_inputs": "p p p p p l i i p p p p p p p p p l p l p p p",
    "aon_grender_bwd": "p p p p l i i p p p p p p l p l p p",
}


def test_backward_argtypes_equal_the_handwritten_lists():
    from aon_amd import _lib

    kinds = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aon_hip.h")).read(), flags=re.S)
    backwards = sorted(re.findall(r"\b(aon_\w+)\s*\([^;]*?\bint64_t scratch_bytes\b[^;]*;", text))
    assert backwards == sorted(BWD_ARGTYPES), set(backwards) ^ set(BWD_ARGTYPES)
    for name, letters in BWD_ARGTYPES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [kinds[k] for k in letters.split()], name
        assert list(_lib._SIGS[name][1]) == list(fn.argtypes), name


# ---- the refusal table ----
N = 3                       # rays
BASE = 0x7A000000           # fake device pointers: non-null, 256-byte aligned, never dereferenced, far from the ones other tests declare forms for
HEAD = ["rays_d", "n", "white", "levels", "g_rgb", "g_acc", "g_depth"]
TAIL = ["ws", "ws_bytes", "scratch", "scratch_bytes", "stream"]
ART_PACKS = ["bwd_c", "mate_c", "bwd_f", "mate_f"]          # transposed stream and its mate (per-call block), per level
FROZEN = ART_PACKS + HEAD + ["params_c", "params_f", "g_shape", "g_app", "g_artic"] + TAIL + ["opts"]
FULL_ART = ART_PACKS + HEAD + ["params_c", "params_f", "shape", "app", "artic", "grads_c", "grads_f", "g_shape", "g_app", "g_artic"] + TAIL
VANILLA = ["bwd_c", "mate_c", "bwd_f", "mate_f"] + HEAD + ["grads_c", "grads_f"] + TAIL      # (mate: the forward stream)
ORDERS = {
    "aon_render_bwd": VANILLA, "aon_render_bwd_ex": VANILLA + ["opts"],
    "aon_art_render_bwd": FULL_ART, "aon_art_render_bwd_ex": FULL_ART + ["opts"],
    "aon_art_render_bwd_latents": FROZEN, "aon_art_render_bwd_inputs": FROZEN + ["rg"],
    "aon_grender_bwd": ["geom", "params_c", "params_f"] + HEAD + ["grads_c", "grads_f"] + TAIL + ["opts"],
}
FORMS_MSG = {False: "forward and transposed streams were packed in different forms (aon_set_bottleneck_fold changed in between)",
             True: "transposed stream and per-call block were made in different forms (aon_set_bottleneck_fold changed in between)"}
ALIGN_MSG = "workspace / scratch must be 256-byte aligned"
INVALID, WORKSPACE = -1, -2


def _fake(i):
    return BASE + 0x1000 * i


def _array(n, hole=None, start=100):
    return (C.c_void_p * n)(*[0 if i == hole else _fake(start + i) for i in range(n)])


class Entry:
    """One entry point (`with_rg`: aon_art_render_bwd_inputs with a ray-gradient struct): a complete argument set that passes every check --
    never called as it is -- and the rows (label, overrides, rank, rc, message, deliberate) that each break one thing."""

    def __init__(self, lib, _lib, name, with_rg=False):
        self.name, self.fn, self.lib = name, getattr(lib, name), lib
        self.general, self.art = name == "aon_grender_bwd", name.startswith("aon_art_")
        self.frozen = name in ("aon_art_render_bwd_latents", "aon_art_render_bwd_inputs")
        # the name the messages carry: the _ex forms report as the plain ones, _inputs without rg IS the _latents call
        self.who = name[:-3] if name.endswith("_ex") else ("aon_art_render_bwd_latents" if self.frozen and not with_rg else name)
        self.nparams = 40 if self.art else 24
        a = {k: None for k in ORDERS[name]}
        a.update(rays_d=_fake(1), n=N, white=1, levels=2, g_rgb=_array(2, start=10), ws=_fake(2), scratch=_fake(3),
                 grads_c=_array(self.nparams, start=200), grads_f=_array(self.nparams, start=300))
        if self.general:
            self.geom = _lib.MlpGeometryC()
            lib.aon_mlp_geometry_init(C.byref(self.geom))
            g = C.byref(self.geom)
            a.update(geom=g, params_c=_array(24, start=400), params_f=_array(24, start=500))
            sizes = (lib.aon_grender_train_workspace_bytes(g, N, 2, None), lib.aon_grender_train_scratch_bytes(g, N, 2, None))
            self.queries = ("aon_grender_train_workspace_bytes()", "aon_grender_train_scratch_bytes()")
        else:
            a.update(bwd_c=_fake(20), mate_c=_fake(21), bwd_f=_fake(22), mate_f=_fake(23))
            if self.art:
                a.update(params_c=_array(40, start=400), params_f=_array(40, start=500), shape=_fake(30), app=_fake(31), artic=_fake(32),
                         g_shape=_fake(33), g_app=_fake(34), g_artic=_fake(35))
            if with_rg:
                self.rg = _lib.RayGradsC(_fake(40), _fake(41), _fake(42), _fake(43), _fake(44))
                a["rg"] = C.byref(self.rg)
            scratch_query = "aon_train_scratch_bytes" + (("_inputs" if with_rg else "_latents") if self.frozen else "")
            sizes = (lib.aon_train_workspace_bytes(N, int(self.art), 2),
                     getattr(lib, scratch_query)(N, 2, None) if self.frozen else lib.aon_train_scratch_bytes(N, int(self.art), 2))
            self.queries = ("aon_train_workspace_bytes()", scratch_query + "()")
        assert sizes[0] > 0 and sizes[1] > 0
        a.update(ws_bytes=sizes[0], scratch_bytes=sizes[1])
        self.base = {k: v for k, v in a.items() if k in ORDERS[name]}
        self.with_rg = with_rg

    def rows(self):
        fused = not self.general
        r = [("n = 0", {"n": 0}, 1, INVALID, "bad size / num_levels", False),
             ("num_levels = 3", {"levels": 3}, 1, INVALID, "bad size / num_levels", False)]
        if self.with_rg:
            hole = type(self.rg)(_fake(40), _fake(41), _fake(42), 0, _fake(44))
            r.append(("null g_rays_d in aon_ray_grads", {"rg": C.byref(hole), "_keep": hole}, 2, INVALID, "null member of aon_ray_grads", False))
        nulls = ["rays_d", "g_rgb", "ws", "scratch"]
        nulls += [] if self.general or self.frozen else ["grads_c"]
        nulls += ["params_c", "shape", "artic", "g_shape", "g_artic"] if self.art and not self.frozen else []
        nulls += ["g_app"] if self.frozen else []          # (one of the three: with rg all three may be null together, never one)
        r += [(k + " = NULL", {k: None}, 3, INVALID, "null pointer", False) for k in nulls]
        # [deliberate change] the fused entry points used to check the scratch only and said "scratch must be 256-byte aligned"
        r += [("misaligned scratch", {"scratch": _fake(3) + 16}, 4, INVALID, ALIGN_MSG, fused),
              ("misaligned workspace", {"ws": _fake(2) + 128}, 4, INVALID, ALIGN_MSG, fused),
              ("workspace one byte short", {"ws_bytes": self.base["ws_bytes"] - 1}, 5, WORKSPACE, "workspace smaller than " + self.queries[0], False),
              ("scratch one byte short", {"scratch_bytes": self.base["scratch_bytes"] - 1}, 6, WORKSPACE, "scratch smaller than " + self.queries[1], False)]
        n = self.nparams
        if self.general:       # level 0 only: level 1 is judged behind level 0's launches
            r += [("params_c = NULL", {"params_c": None}, 10, INVALID, "null parameter pointer", False),
                  ("hole in params_c", {"params_c": _array(n, 7, 400)}, 10, INVALID, "null parameter pointer", False),
                  ("grads_c = NULL", {"grads_c": None}, 11, INVALID, "null level pointer", False),
                  ("g_rgb[0] = NULL", {"g_rgb": _array(2, 0, 10)}, 11, INVALID, "null level pointer", False),
                  ("hole in grads_c", {"grads_c": _array(n, 5, 200)}, 12, INVALID, "null gradient pointer", False)]
            return r
        level = lambda l, kind: 10 + 10 * l + kind      # noqa: E731  (per level: null level pointer, forms, holes)
        r += [("bwd_c = NULL", {"bwd_c": None}, level(0, 0), INVALID, "null level pointer", False),
              ("mate_f = NULL", {"mate_f": None}, level(1, 0), INVALID, "null level pointer", False),
              ("g_rgb[1] = NULL", {"g_rgb": _array(2, 1, 10)}, level(1, 0), INVALID, "null level pointer", False),
              ("mate_c in the other form", {"_form_mate_c": 0}, level(0, 1), INVALID, FORMS_MSG[self.art], False),
              ("bwd_f in the other form", {"_form_bwd_f": 0}, level(1, 1), INVALID, FORMS_MSG[self.art], False)]
        if not self.frozen:
            r.append(("grads_f = NULL", {"grads_f": None}, level(1, 0), INVALID, "null level pointer", False))
        if self.art:
            r.append(("params_f = NULL", {"params_f": None}, level(1, 0), INVALID, "null level pointer", False))
        if self.frozen:        # entries 0, 10, 20, 26 are read; the others may be null
            r += [("params_c[10] = NULL", {"params_c": _array(n, 10, 400)}, level(0, 2), INVALID, "null parameter pointer", False),
                  ("params_f[26] = NULL", {"params_f": _array(n, 26, 500)}, level(1, 2), INVALID, "null parameter pointer", False)]
        else:
            msg = "null parameter / gradient pointer" if self.art else "null gradient pointer"
            r += [("hole in grads_c", {"grads_c": _array(n, 5, 200)}, level(0, 2), INVALID, msg, False),
                  ("hole in grads_f", {"grads_f": _array(n, n - 1, 300)}, level(1, 2), INVALID, msg, False)]
            if self.art:
                r.append(("hole in params_f", {"params_f": _array(n, 0, 500)}, level(1, 2), INVALID, msg, False))
        return r

    def call(self, overrides):
        """-> (rc, message) of the entry point under `overrides`; the four streams / blocks carry the folded form but for `_form_<key>` ones"""
        args = dict(self.base)
        args.update({k: v for k, v in overrides.items() if not k.startswith("_")})
        if not self.general:
            for key in ART_PACKS:
                assert self.lib.aon_declare_stream_form(C.c_void_p(self.base[key]), overrides.get("_form_" + key, 1)) == 0
        rc = self.fn(*[args[k] for k in ORDERS[self.name]])
        return rc, self.lib.aon_last_error().decode()


def _touched(overrides):
    return {k[len("_form_"):] if k.startswith("_form_") else k for k in overrides if k != "_keep"}


CASES = [(name, False) for name in ORDERS] + [("aon_art_render_bwd_inputs", True)]


def entry_rows(name, with_rg, deliberate=True):
    """(entry, its rows) -- `deliberate=False`: without the rows this change moved on purpose, for a run against the build before it."""
    from aon_amd import _lib

    e = Entry(_lib.lib, _lib, name, with_rg)
    return e, [row for row in e.rows() if deliberate or not row[5]]


@pytest.mark.parametrize("name,with_rg", CASES, ids=[n + ("+rg" if rg else "") for n, rg in CASES])
def test_every_prelaunch_refusal(name, with_rg, deliberate=True):
    e, rows = entry_rows(name, with_rg, deliberate)
    assert len(rows) >= 14
    for label, overrides, _rank, rc, msg, _ in rows:
        assert e.call(overrides) == (rc, f"{e.who}: {msg}"), (name, label)


@pytest.mark.parametrize("name,with_rg", CASES, ids=[n + ("+rg" if rg else "") for n, rg in CASES])
def test_refusals_keep_their_rank(name, with_rg, deliberate=True):
    """Two faults at once: the refusal that ranks first is the one reported."""
    e, rows = entry_rows(name, with_rg, deliberate)
    pairs = 0
    for a, b in itertools.combinations(rows, 2):
        if a[2] == b[2] or _touched(a[1]) & _touched(b[1]):
            continue
        first = a if a[2] < b[2] else b
        assert e.call({**a[1], **b[1]}) == (first[3], f"{e.who}: {first[4]}"), (name, a[0], b[0])
        pairs += 1
    assert pairs > 60
