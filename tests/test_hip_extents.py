"""GPU: the memory contract of include/aon_hip.h -- inputs are never written, outputs are written inside their stated extents, a workspace
or scratch of exactly the library's byte count is enough -- for every stream-taking entry point, with the guard bands of tests/_guard.py.

Every case of the table runs three times: plain; guarded with every `torch.empty` of the binding prefilled with 0xFF bytes ("nan") and
every input copied into a guarded slot; guarded with zero prefill.  Then
  1. no band around any output, workspace, scratch, pool buffer or input was touched;
  2. every input has the bits it had before the call, in all three runs;
  3. the outputs of the three runs are equal bit for bit (the result depends neither on neighbouring memory nor on prior contents);
  4. no output of the "nan" run holds a 0xFFFFFFFF word (every element was written);
  5. the recorder saw every entry point the case names in `reaches`.
The last test asserts that the names recorded over the whole table cover every stream-taking entry point of the header outside EXCLUDED
(tests/test_guard_cpu.py holds the static half).  Only valid calls are made here: no undersized buffer, no misaligned or null pointer.

Ray counts 1, 5, 37 and sample counts 64+128 (S = 65 / 193) and 40+72 (S = 41 / 113): 5 x 41 = 205 samples is 1 mod 4 and 77 mod 128,
37 x 65 = 2405 is 1 mod 4, every count is below a workgroup's worth of rays and no multiple of four.

Where an output's documented extent is smaller than its allocation the case slices it and says so: the activation planes / gradient
planes / ReLU masks of the stage-level training calls hold pad rows the header leaves unspecified, so they are handed on to the next stage
but not compared; what is compared is everything computed from them (a read of an unwritten plane element shows there, check 3)."""
import copy
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
SIZES = ((1, "default"), (5, "small"), (37, "default"))       # (rays, sample counts)
DEGREES = ((0, 10, 4), (1, 8, 3))

# entry points no case reaches: (rule, reason); the rules are "probe" (a measurement aid), "older form" (tests/test_hip_entry_ladder.py
# shows it forwarding its arguments unchanged to the covered form the reason names) and "multi-gpu"
EXCLUDED = {
    "aon_wgrad_kind_bench": ("probe", "measurement aid of tools/kernel_bench.py: the grouped weight-gradient kernel alone on arbitrary rows"),
    "aon_render_fwd": ("older form", "the ladder shows it equal to aon_render_fwd_ex without options"),
    "aon_art_render_fwd": ("older form", "the ladder shows it equal to aon_art_render_fwd_ex without options"),
    "aon_render_fwd_train": ("older form", "the ladder shows it equal to aon_render_fwd_train_ex without options"),
    "aon_art_render_fwd_train": ("older form", "the ladder shows it equal to aon_art_render_fwd_train_ex without options"),
    "aon_render_bwd": ("older form", "the ladder shows it equal to aon_render_bwd_ex without options"),
    "aon_art_render_bwd": ("older form", "the ladder shows it equal to aon_art_render_bwd_ex without options"),
}


class Case:
    """`make(dev)` -> dict of inputs (seeded; the entry "inout", if any, holds buffers the call updates in place by contract);
    `call(ops, inputs)` -> flat list of output tensors; `reaches`: the aon_* names the case must hit; `group`: which test runs it."""

    def __init__(self, group, name, make, call, reaches, xfail=None):
        self.group, self.name, self.make, self.call, self.reaches, self.xfail = group, name, make, call, tuple(reaches), xfail

    def __repr__(self):
        return self.name


CASES: list = []


def case(group, name, reaches, xfail=None):
    def deco(fns):
        make, call = fns()
        CASES.append(Case(group, name, make, call, reaches, xfail))
        return fns
    return deco


# ------------------------------------------------------------------ inputs
def _syn():
    import aon_amd.synthetic as syn
    return syn


def _uni(seed, *shape):
    return _syn().seeded_uniform(seed, *shape)


def _rays(dev, n, seed=11):
    r = _syn().random_rays(n, seed=seed)
    return r["rays_o"].to(dev), r["rays_d"].to(dev), r["viewdirs"].to(dev)


def _opts(kind, **kw):
    from aon_amd import ops
    if kind == "small":
        kw = dict(num_coarse_samples=40, num_fine_samples=72, **kw)
    return ops.RenderOpts(**kw)


def _S(kind):
    return (65, 193) if kind == "default" else (41, 113)


def _t_vals(dev, n, S, seed=12):
    return (NEAR + (FAR - NEAR) * torch.sort(_uni(seed, n, S), dim=-1).values).to(dev)


_NETS: dict = {}


def _net(dev, art, degrees=(0, 10, 4)):
    """Both levels' parameters (and the latents) of a seeded network on the device, shared by the cases: inputs are never written."""
    key = (str(dev), art, tuple(degrees))
    if key not in _NETS:
        syn = _syn()
        mn, mx, dv = degrees
        if art:
            sd = syn.make_art_state_dict(seed=0, density_scale=2.0, min_deg_point=mn, max_deg_point=mx, deg_view=dv)
        elif tuple(degrees) == (0, 10, 4):
            sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)
        else:
            sd = syn.make_general_nerf_state_dict(7, min_deg_point=mn, max_deg_point=mx, deg_view=dv)
        params = [{k[len(p):]: v.to(dev) for k, v in sd.items() if k.startswith(p)} for p in ("coarse_mlp.", "fine_mlp.")]
        lat = {k: (0.2 * _uni(30 + i, 1, w) - 0.1).to(dev) for i, (k, w) in enumerate((("density", 128), ("color", 128), ("articulation", 32)))}
        _NETS[key] = (params, lat)
    return _NETS[key]


def _packs(art, params, lat, degrees=(0, 10, 4), bwd=False):
    """Streams of both levels, packed in the form that is current -> dict of lists (made in `make`: inputs of the calls under test)."""
    from aon_amd import ops
    if art:
        out = {"fwd": [ops.pack_art_mlp(p, degrees=degrees) for p in params], "small": [ops.art_prepare(p, lat, degrees=degrees) for p in params]}
        if bwd:
            out["bwd"] = [ops.pack_art_mlp_bwd(p, degrees=degrees) for p in params]
    else:
        out = {"fwd": [ops.pack_vanilla_mlp(p, degrees=degrees) for p in params]}
        if bwd:
            out["bwd"] = [ops.pack_vanilla_mlp_bwd(p, degrees=degrees) for p in params]
    return out


def _half_space_grid(dev):
    """x > 0.2 occupied over [-2, 2]^3, dims (7, 9, 11): the rays from the radius-4 sphere cross occupied and empty cells."""
    from aon_amd import ops
    x = torch.linspace(-2.0, 2.0, 7, device=dev)
    density = (x > 0.2).float()[:, None, None].expand(7, 9, 11).contiguous()
    return ops.occupancy_grid(density, -2.0, 2.0, threshold=0.01, dilate=1)


# ------------------------------------------------------------------ the protocol
def _map(fn, obj):
    """`fn` over every tensor of a nested structure (dicts, lists, tuples, occupancy grids); everything else as it is."""
    if isinstance(obj, torch.Tensor):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: _map(fn, v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(fn, v) for v in obj)
    if hasattr(obj, "bits") and hasattr(obj, "c_struct"):      # ops.OccupancyGrid: its bitfield is an input
        g = copy.copy(obj)
        g.bits = _map(fn, obj.bits)
        return g
    return obj


def _leaves(obj, out=None, path=""):
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append((path, obj))
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _leaves(v, out, f"{path}.{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _leaves(v, out, f"{path}[{i}]")
    elif hasattr(obj, "bits") and hasattr(obj, "c_struct"):
        _leaves(obj.bits, out, path + ".bits")
    return out


def _inputs_unchanged(inputs, before, what):
    frozen = {k: v for k, v in inputs.items() if k != "inout"}
    for (path, t), b in zip(_leaves(frozen), before):
        assert torch.equal(_guard.bits(t), b), f"{what}: input{path} was written"


_SEEN: set = set()
_RAN: set = set()


def _one_run(c, dev, monkeypatch, prefill):
    """-> (outputs as bit images on the host, names recorded or None)"""
    from aon_amd import ops

    inputs = c.make(dev)
    if prefill is None:
        before = [_guard.bits(t) for _, t in _leaves({k: v for k, v in inputs.items() if k != "inout"})]
        outs = c.call(ops, inputs)
        torch.cuda.synchronize()
        _inputs_unchanged(inputs, before, f"{c.name} (plain)")
        return [_guard.bits(t) for t in outs], None
    with _guard.guarded(monkeypatch, prefill) as (alloc, rec):
        inputs = _map(lambda t: _guard.place(alloc, t), inputs)
        before = [_guard.bits(t) for _, t in _leaves({k: v for k, v in inputs.items() if k != "inout"})]
        placed = len(alloc)
        outs = c.call(ops, inputs)
        # the harness is in the loop: the call's own buffers came from the guarded allocator (an in-place update allocates none)
        assert len(alloc) > placed or "inout" in inputs, f"{c.name}: the call allocated nothing through the proxy"
        alloc.check()                                                                     # 1
        _inputs_unchanged(inputs, before, f"{c.name} ({prefill})")                        # 2
        if prefill == "nan":
            unwritten = [f"output {i} {tuple(t.shape)} {t.dtype}" for i, t in enumerate(outs) if _guard.has_unwritten_word(t)]
            assert not unwritten, f"{c.name}: outputs holding an element nobody wrote: {unwritten}"   # 4
        missing = set(c.reaches) - rec.names
        assert not missing, f"{c.name} ({prefill}): never fetched {sorted(missing)}"      # 5
        _SEEN.update(n for n in rec.names)
        return [_guard.bits(t) for t in outs], set(rec.names)


def run_case(c, dev, monkeypatch):
    plain, _ = _one_run(c, dev, monkeypatch, None)
    nan, _ = _one_run(c, dev, monkeypatch, "nan")
    zero, _ = _one_run(c, dev, monkeypatch, "zero")
    assert len(plain) == len(nan) == len(zero) and len(plain) > 0
    for i, (a, b, z) in enumerate(zip(plain, nan, zero)):                                 # 3
        assert a.shape == b.shape == z.shape, f"{c.name}: output {i} shapes {a.shape} / {b.shape} / {z.shape}"
        assert torch.equal(b, z), f"{c.name}: output {i} depends on the prior contents of a buffer ({int((b != z).sum())} of {b.numel()} words differ)"
        assert torch.equal(a, b), f"{c.name}: output {i} of the guarded run differs from the plain run ({int((a != b).sum())} of {a.numel()} words)"
    _RAN.add(c.name)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _group(*groups):
    return [pytest.param(c, id=c.name, marks=[pytest.mark.xfail(strict=True, reason=c.xfail)] if c.xfail else []) for c in CASES if c.group in groups]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arr(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ================================================================== stage calls without a network
@case("stage", "raygen_5x7_pix3_32", ["aon_raygen"])
def _():
    def make(dev):
        return {"dev": dev}

    def call(ops, i):
        syn = _syn()
        return list(ops.raygen(syn.look_at_pose(4.0, 30, 20), 5, 7, syn.focal_from_fovy(5), 3, 32, device=i["dev"]))
    return make, call


@case("stage", "ray_directions_get_rays_radii_5x7", ["aon_ray_directions", "aon_get_rays", "aon_ray_radii"])
def _():
    def make(dev):
        from aon_amd import ops
        return {"dirs": ops.ray_directions(5, 7, _syn().focal_from_fovy(5), device=dev), "dev": dev}

    def call(ops, i):
        syn = _syn()
        c2w = syn.look_at_pose(4.0, 30, 20)
        return [ops.ray_directions(5, 7, syn.focal_from_fovy(5), device=i["dev"]), *ops.get_rays(i["dirs"], c2w), ops.ray_radii(i["dirs"], c2w)]
    return make, call


for _n, _kind in SIZES:
    for _S_ in _S(_kind):
        @case("stage", f"cast_rays_n{_n}_S{_S_}", ["aon_cast_rays"])
        def _(n=_n, S=_S_):
            def make(dev):
                o, d, _v = _rays(dev, n)
                return {"t": _t_vals(dev, n, S), "o": o, "d": d}

            def call(ops, i):
                return [ops.cast_rays(i["t"], i["o"], i["d"])]
            return make, call

    @case("stage", f"ray_limits_n{_n}", ["aon_ray_limits", "aon_ray_limits_box"])
    def _(n=_n):
        def make(dev):
            o, d, _v = _rays(dev, n)
            return {"o": o, "d": d}

        def call(ops, i):
            return [*ops.ray_limits(i["o"], i["d"], 2), *ops.ray_limits_box(i["o"], i["d"], 2), *ops.ray_limits_box(i["o"], i["d"], ((-1, -0.5, -0.7), (0.9, 1, 0.6)))]
        return make, call

    for _var, _reach in (("det_coords_scalar", "aon_sample_along_rays"), ("rand_nocoords_scalar", "aon_sample_along_rays"),
                         ("rand_coords_perray", "aon_sample_along_rays_bounds"), ("det_nocoords_perray_lindisp", "aon_sample_along_rays_bounds"),
                         ("rand_coords_scalar_lindisp", "aon_sample_along_rays_ex")):
        @case("stage", f"sample_along_rays_n{_n}_{_kind}_{_var}", [_reach])
        def _(n=_n, ns=_S(_kind)[0] - 1, var=_var):
            def make(dev):
                o, d, _v = _rays(dev, n)
                i = {"o": o, "d": d}
                if "rand" in var:
                    i["t_rand"] = _uni(13, n, ns + 1).to(dev)
                if "perray" in var:
                    i["near"], i["far"] = (NEAR + 0.1 * _uni(14, n, 1)).to(dev), (FAR - 0.1 * _uni(15, n, 1)).to(dev)
                return i

            def call(ops, i):
                t, coords = ops.sample_along_rays(i["o"], i["d"], ns, i.get("near", NEAR), i.get("far", FAR), t_rand=i.get("t_rand"),
                                                  want_coords="nocoords" not in var, lindisp="lindisp" in var)
                return [t] if coords is None else [t, coords]
            return make, call

    for _deg in ((0, 10), (0, 4), (-2, 8)):
        @case("stage", f"pos_enc_n{_n}_{_kind}_deg{_deg[0]}_{_deg[1]}", ["aon_pos_enc"])
        def _(n=_n, S=_S(_kind)[0], deg=_deg):
            def make(dev):
                return {"x": (2 * _uni(16, n, S, 3) - 1).to(dev)}

            def call(ops, i):
                return [ops.pos_enc(i["x"], *deg), ops.pos_enc(i["x"][0], *deg)]
            return make, call

    for _lat in (False, True):
        @case("stage", f"train_loss_n{_n}_{'latents' if _lat else 'nolatents'}", ["aon_train_loss_fwd", "aon_train_loss_bwd"])
        def _(n=_n, lat=_lat):
            def make(dev):
                i = {"c": _uni(17, n, 3).to(dev), "f": _uni(18, n, 3).to(dev), "target": _uni(19, n, 3).to(dev), "go": torch.tensor([0.7], device=dev)}
                i["lat"] = [(_uni(20 + k, 1, w) - 0.5).to(dev) for k, w in enumerate((128, 128, 32))] if lat else []
                return i

            def call(ops, i):
                loss, stats = ops.train_loss_fwd(i["c"], i["f"], i["target"], i["lat"], 1e-4)
                d_c, d_f, d_l = ops.train_loss_bwd(i["c"], i["f"], i["target"], i["lat"], 1e-4, i["go"])
                loss1, stats1 = ops.train_loss_fwd(None, i["f"], i["target"], i["lat"], 1e-4)
                _, d_f1, _ = ops.train_loss_bwd(None, i["f"], i["target"], i["lat"], 1e-4, i["go"])
                return [loss, stats, d_c, d_f, loss1, stats1, d_f1, *[t for t in d_l if t is not None]]
            return make, call


@case("stage", "ssim_13x17", ["aon_ssim"])
def _():
    def make(dev):
        return {"p": _uni(40, 13, 17, 3).to(dev), "g": _uni(41, 13, 17, 3).to(dev)}

    def call(ops, i):
        return [ops.ssim([i["p"]], [i["g"]])]
    return make, call


@case("stage", "ssim_batch3_image_sizes", ["aon_ssim"])
def _():
    sizes = [(13, 17), (11, 11), (12, 19)]

    def make(dev):
        return {"p": [_uni(42 + k, h * w, 3).to(dev) for k, (h, w) in enumerate(sizes)], "g": [_uni(52 + k, h * w, 3).to(dev) for k, (h, w) in enumerate(sizes)]}

    def call(ops, i):
        return [ops.ssim(i["p"], i["g"], image_sizes=sizes)]
    return make, call


@case("stage", "marching_cubes_7x6x5", ["aon_marching_cubes_count", "aon_marching_cubes"])
def _():
    def make(dev):
        return {"field": _uni(60, 7, 6, 5).to(dev)}

    def call(ops, i):
        verts, faces = ops.marching_cubes(i["field"], 0.5, -1.0, 1.0)
        assert verts.shape[0] > 0 and faces.shape[0] > 0
        return [verts, faces]
    return make, call


for _dil in (0, 1, 2):
    @case("stage", f"occupancy_grid_7x9x11_dilate{_dil}", ["aon_occupancy_build"])
    def _(dil=_dil):
        def make(dev):
            # three corners above the threshold, far enough apart that no 32-cell word fills up even at dilate 2 (an all-ones word is
            # what an unwritten one looks like)
            density = 0.01 * _uni(61, 7, 9, 11)
            for p in ((1, 1, 1), (4, 6, 2), (3, 4, 9)):
                density[p] = 0.5
            return {"density": density.to(dev)}

        def call(ops, i):
            grid = ops.occupancy_grid(i["density"], -2.0, 2.0, threshold=0.017, dilate=dil)
            assert 0 < int(grid.occupied().sum()) < 480
            return [grid.bits]
        return make, call


@case("stage", "code_library_fwd_bwd", ["aon_code_library_fwd", "aon_code_library_bwd"])
def _():
    shapes = [(2, 128), (2, 128), (10, 32)]

    def make(dev):
        return {"tables": [_uni(62 + k, *s).to(dev) for k, s in enumerate(shapes)], "ids": [torch.tensor([v], dtype=torch.int64, device=dev) for v in (1, 1, 6)],
                "g_rows": [_uni(65 + k, 1, s[1]).to(dev) for k, s in enumerate(shapes)]}

    def call(ops, i):
        rows, _ids = ops.code_library_fwd(i["tables"], i["ids"])
        return [*rows, *ops.code_library_bwd(i["g_rows"], i["ids"], shapes)]
    return make, call


_RAGGED = ((dict(max_deg_point=1, deg_view=0, netdepth=1, netwidth=5, netwidth_condition=3), 3, 7),
           (dict(max_deg_point=5, deg_view=1, netdepth=2, netwidth=131, netwidth_condition=257, netdepth_condition=2), 5, 53))
for _k, (_kw, _n, _S_) in enumerate(_RAGGED):
    @case("stage", f"gmlp_fwd_ragged{_k}", ["aon_gmlp_fwd"])
    def _(kw=_kw, n=_n, S=_S_):
        def make(dev):
            from aon_amd import ops
            geom = ops.MlpGeometry(**kw)
            sd = _syn().make_general_nerf_state_dict(11, prefixes=("",), **kw)
            return {"params": {k: t.to(dev) for k, t in sd.items()}, "x": (2 * _uni(3, n, S, geom.pos_size) - 1).to(dev),
                    "v": (2 * _uni(4, n, geom.view_pos_size) - 1).to(dev), "geom": geom}

        def call(ops, i):
            return list(ops.gmlp_fwd(i["geom"], i["params"], i["x"], i["v"]))
        return make, call


# ================================================================== optimiser: the guard is inside the tensor
for _begin, _count in ((0, 1200), (4, 1002), (3, 1001), (8, 1), (8, 3)):
    @case("optimiser", f"adam_step_{_begin}_{_count}", ["aon_adam_step"])
    def _(begin=_begin, count=_count):
        def make(dev):
            return {"g": (_uni(70, 1200) - 0.5).to(dev), "inout": [(_uni(71, 1200) - 0.5).to(dev), (0.1 * _uni(72, 1200) - 0.05).to(dev), (0.01 * _uni(73, 1200)).to(dev)]}

        def call(ops, i):
            p, m, v = i["inout"]
            before = [_guard.bits(t) for t in (p, m, v)]
            ops.adam_step(p, i["g"], m, v, begin, count, 5e-4, 0.9, 0.999, 1e-8, 3)
            for name, t, b in zip("pmv", (p, m, v), before):
                a = _guard.bits(t)
                assert torch.equal(a[:begin], b[:begin]) and torch.equal(a[begin + count:], b[begin + count:]), f"adam_step wrote {name} outside [{begin}, {begin + count})"
                assert bool((a[begin:begin + count] != b[begin:begin + count]).any()), f"adam_step left {name} unchanged"
            return [p, m, v]
        return make, call


# ================================================================== compositing / pdf
for _n, _kind in SIZES:
    for _S_ in _S(_kind):
        @case("composite", f"volumetric_rendering_n{_n}_S{_S_}", ["aon_composite"])
        def _(n=_n, S=_S_):
            def make(dev):
                _o, d, _v = _rays(dev, n)
                return {"rgb": _uni(80, n, S, 3).to(dev), "density": (3 * _uni(81, n, S, 1)).to(dev), "t": _t_vals(dev, n, S), "d": d}

            def call(ops, i):
                return list(ops.volumetric_rendering(i["rgb"], i["density"], i["t"], i["d"], True))
            return make, call

        for _act, _ww, _noise in ((0, True, False), (1, False, False), (2, True, True), (1, False, True), (2, False, False)):
            @case("composite", f"composite_raw_n{_n}_S{_S_}_act{_act}_{'w' if _ww else 'now'}_{'noise' if _noise else 'nonoise'}",
                  ["aon_composite_ex" if _noise else "aon_composite"])
            def _(n=_n, S=_S_, act=_act, ww=_ww, noise=_noise):
                def make(dev):
                    _o, d, _v = _rays(dev, n)
                    i = {"raw": (4 * _uni(82, n, S, 4) - 2).to(dev), "t": _t_vals(dev, n, S), "d": d}
                    if noise:
                        i["noise"] = _uni(83, n, S).to(dev)
                    return i

                def call(ops, i):
                    out = ops.composite_raw(i["raw"], i["t"], i["d"], act != 1, act, ww, opts=_opts("default", noise_std=0.5) if noise else None, noise=i.get("noise"))
                    return [t for t in out if t is not None]
                return make, call

    for _per_ray_u in (False, True):
        @case("composite", f"pdf_n{_n}_{'u_per_ray' if _per_ray_u else 'u_shared'}", ["aon_sample_pdf", "aon_sample_pdf_n", "aon_composite_pdf"])
        def _(n=_n, per_ray=_per_ray_u):
            def make(dev):
                _o, d, _v = _rays(dev, n)
                i = {"bins": _t_vals(dev, n, 64, 84), "w63": _uni(85, n, 63).to(dev), "t65": _t_vals(dev, n, 65, 86), "w65": _uni(87, n, 65).to(dev),
                     "t41": _t_vals(dev, n, 41, 88), "w41": _uni(89, n, 41).to(dev), "raw": (4 * _uni(90, n, 65, 4) - 2).to(dev), "d": d}
                if per_ray:
                    i["u128"], i["u17"] = _uni(91, n, 128).to(dev), _uni(92, n, 17).to(dev)
                else:
                    i["u17"] = torch.sort(_uni(92, 17)).values.to(dev)
                return i

            def call(ops, i):
                u = i.get("u128")
                out = [ops.sorted_piecewise_constant_pdf(i["bins"], i["w63"], u=u), ops.sorted_piecewise_constant_pdf(i["t41"], i["w41"][:, :40].contiguous(), u=i["u17"], num_samples=17),
                       ops.sample_pdf_t(i["t65"], i["w65"], u=u), ops.sample_pdf_t(i["t65"], i["w63"], u=u, bins=i["bins"]),
                       ops.sample_pdf_t_n(i["t41"], i["w41"], 17, u=i["u17"]), ops.sample_pdf_t_n(i["t65"], i["w65"], 128, u=u, force_generic=True)]
                for ww in (False, True):
                    out += [t for t in ops.composite_pdf(i["raw"], i["t65"], i["d"], True, ops.ACT_VANILLA, u=u, want_weights=ww) if t is not None]
                return out
            return make, call

for _n, _S_, _act in ((5, 65, 1), (37, 65, 2), (5, 193, 2), (1, 193, 1), (5, 300, 1), (37, 41, 2), (5, 113, 1)):
    for _given in (True, False):
        @case("composite", f"composite_bwd_n{_n}_S{_S_}_act{_act}_{'acc_depth' if _given else 'null'}", ["aon_composite_bwd"])
        def _(n=_n, S=_S_, act=_act, given=_given):
            def make(dev):
                _o, d, _v = _rays(dev, n)
                i = {"raw": (4 * _uni(93, n, S, 4) - 2).to(dev), "t": _t_vals(dev, n, S), "d": d, "g_rgb": (_uni(94, n, 3) - 0.5).to(dev)}
                if given:
                    i["g_acc"], i["g_depth"] = (_uni(95, n) - 0.5).to(dev), (_uni(96, n) - 0.5).to(dev)
                return i

            def call(ops, i):
                Np = ops.padded_samples(n * S)
                d_raw = ops.composite_bwd(i["raw"], i["t"], i["d"], i["g_rgb"], i.get("g_acc"), i.get("g_depth"), act == 1, act, Np)
                assert d_raw.shape == (Np, 4) and not bool(d_raw[n * S:].any())      # the padded tail carries zero gradient
                return [d_raw]
            return make, call


# ================================================================== packing: outputs are exactly the library's byte counts
for _deg in DEGREES:
    _dn = "deg" + "_".join(str(x) for x in _deg)

    @case("packing", f"pack_vanilla_{_dn}", ["aon_pack_vanilla_mlp" if _deg == (0, 10, 4) else "aon_pack_vanilla_mlp_deg",
                                               "aon_pack_vanilla_mlp_bwd" if _deg == (0, 10, 4) else "aon_pack_vanilla_mlp_bwd_deg", "aon_vanilla_pack_step"])
    def _(deg=_deg):
        def make(dev):
            return {"params": _net(dev, False, deg)[0]}

        def call(ops, i):
            pc, pf = i["params"]
            out = [ops.pack_vanilla_mlp(pc, degrees=deg), ops.pack_vanilla_mlp_bwd(pc, degrees=deg)]
            assert out[0].numel() == ops.packed_bytes() and out[1].numel() == int(ops.lib.aon_bwd_packed_bytes())
            for lvl in ops.vanilla_pack_step(pc, pf, degrees=deg) + ops.vanilla_pack_step(pc, pf, degrees=deg, with_bwd=False):
                out += [t for t in lvl if t is not None]
            return out
        return make, call

    @case("packing", f"pack_art_{_dn}", ["aon_pack_art_mlp_deg", "aon_pack_art_mlp_bwd_deg", "aon_art_prepare_deg", "aon_art_pack_step"])
    def _(deg=_deg):
        def make(dev):
            params, lat = _net(dev, True, deg)
            return {"params": params, "lat": lat}

        def call(ops, i):
            pc, pf = i["params"]
            out = [ops.pack_art_mlp(pc, degrees=deg), ops.pack_art_mlp_bwd(pc, degrees=deg), ops.art_prepare(pf, i["lat"], degrees=deg)]
            assert [t.numel() for t in out] == [int(ops.lib.aon_art_packed_bytes()), int(ops.lib.aon_art_bwd_packed_bytes()), int(ops.lib.aon_art_small_bytes())]
            for lvl in ops.art_pack_step(pc, pf, i["lat"], degrees=deg) + ops.art_pack_step(pc, pf, i["lat"], degrees=deg, with_bwd=False):
                out += [t for t in lvl if t is not None]
            return out
        return make, call


@case("packing", "pack_art_default_degree_forms", ["aon_pack_art_mlp", "aon_pack_art_mlp_bwd", "aon_art_prepare"])
def _():
    """The forms without degrees, which ops.py never calls: through the library directly, on buffers of the proxy."""
    def make(dev):
        params, lat = _net(dev, True)
        return {"params": params[0], "lat": lat}

    def call(ops, i):
        lib, T = ops.lib, ops.torch
        tensors = [i["params"][k] for k in ops.ART_PARAM_ORDER]
        dev = tensors[0].device
        new = lambda nbytes: T.empty(int(nbytes), dtype=torch.uint8, device=dev)   # noqa: E731
        pk, bw, sm = new(lib.aon_art_packed_bytes()), new(lib.aon_art_bwd_packed_bytes()), new(lib.aon_art_small_bytes())
        lat = [i["lat"][k].reshape(-1) for k in ("density", "color", "articulation")]
        with torch.cuda.device(dev):
            ops.check(lib.aon_pack_art_mlp(_arr(tensors), C.c_void_p(pk.data_ptr()), _stream()), "aon_pack_art_mlp")
            ops.check(lib.aon_pack_art_mlp_bwd(_arr(tensors), C.c_void_p(bw.data_ptr()), _stream()), "aon_pack_art_mlp_bwd")
            ops.check(lib.aon_art_prepare(_arr(tensors), *(C.c_void_p(t.data_ptr()) for t in lat), C.c_void_p(sm.data_ptr()), _stream()), "aon_art_prepare")
        return [pk, bw, sm]
    return make, call


# ================================================================== stage calls on a packed network
@case("folded_only", "view_bias", ["aon_view_bias"])
def _():
    def make(dev):
        from aon_amd import ops
        return {"packed": ops.pack_vanilla_mlp(_net(dev, False)[0][1]), "v": _rays(dev, 37)[2]}

    def call(ops, i):
        return [ops.view_bias(i["packed"], i["v"]), ops.view_bias(i["packed"], i["v"][:5].contiguous()), ops.view_bias(i["packed"], i["v"][:1].contiguous())]
    return make, call


for _n, _S_ in ((1, 193), (5, 41), (37, 65)):
    @case("stage_mlp", f"mlp_fwd_n{_n}_S{_S_}", ["aon_mlp_fwd", "aon_mlp_fwd_enc", "aon_mlp_fwd_train"])
    def _(n=_n, S=_S_):
        def make(dev):
            o, d, v = _rays(dev, n)
            return {"pk": _packs(False, *_net(dev, False)), "o": o, "d": d, "v": v, "t": _t_vals(dev, n, S), "enc": (2 * _uni(100, n, S, 63) - 1).to(dev),
                    "venc": (2 * _uni(101, n, 27) - 1).to(dev)}

        def call(ops, i):
            pk = i["pk"]["fwd"][0]
            return [ops.mlp_fwd(pk, i["o"], i["d"], i["v"], i["t"]), ops.mlp_fwd_enc(pk, i["enc"], i["venc"]), ops.mlp_fwd_train(pk, i["o"], i["d"], i["v"], i["t"])[0]]
        return make, call

    @case("stage_mlp", f"art_mlp_fwd_n{_n}_S{_S_}", ["aon_art_mlp_fwd", "aon_art_mlp_fwd_pos", "aon_art_mlp_fwd_train"])
    def _(n=_n, S=_S_):
        def make(dev):
            o, d, v = _rays(dev, n)
            return {"pk": _packs(True, *_net(dev, True)), "o": o, "d": d, "v": v, "t": _t_vals(dev, n, S), "pos": (2 * _uni(102, n, S, 3) - 1).to(dev),
                    "venc": (2 * _uni(103, n, 27) - 1).to(dev)}

        def call(ops, i):
            pk, sm = i["pk"]["fwd"][1], i["pk"]["small"][1]
            return [ops.art_mlp_fwd(pk, sm, i["o"], i["d"], i["v"], i["t"]), ops.art_mlp_fwd_pos(pk, sm, i["pos"], i["venc"]),
                    ops.art_mlp_fwd_train(pk, sm, i["o"], i["d"], i["v"], i["t"])[0]]
        return make, call

for _art in (False, True):
    for _n, _S_ in ((5, 41), (37, 65), (1, 193)):
        @case("stage_mlp", f"{'art' if _art else 'vanilla'}_stage_backward_n{_n}_S{_S_}",
              ["aon_art_mlp_fwd_train", "aon_composite_bwd", "aon_art_bwd_chain", "aon_art_wgrad_deg", "aon_art_wgrad"] if _art else
              ["aon_mlp_fwd_train", "aon_composite_bwd", "aon_mlp_bwd_chain", "aon_vanilla_wgrad"])
        def _(art=_art, n=_n, S=_S_):
            """Forward with planes, compositing backward, data chain, weight gradients.  The planes / gradient planes / masks are handed on,
            not compared (pad rows unspecified); every gradient computed from them is."""
            def make(dev):
                o, d, v = _rays(dev, n)
                params, lat = _net(dev, art)
                return {"pk": _packs(art, params, lat, bwd=True), "params": params[0], "lat": lat, "o": o, "d": d, "v": v, "t": _t_vals(dev, n, S),
                        "g_rgb": (_uni(104, n, 3) - 0.5).to(dev)}

            def call(ops, i):
                pk, pb = i["pk"]["fwd"][0], i["pk"]["bwd"][0]
                if not art:
                    raw, planes, masks = ops.mlp_fwd_train(pk, i["o"], i["d"], i["v"], i["t"])
                    d_raw = ops.composite_bwd(raw, i["t"], i["d"], i["g_rgb"], None, None, True, ops.ACT_VANILLA, ops.plane_samples(planes))
                    dplanes = ops.mlp_bwd_chain(pb, pk, d_raw, masks, planes.shape)
                    grads = ops.vanilla_wgrad(planes, dplanes, d_raw, pb)
                    return [raw, d_raw, *(grads[k] for k in ops.VANILLA_PARAM_ORDER)]
                sm = i["pk"]["small"][0]
                raw, planes, masks = ops.art_mlp_fwd_train(pk, sm, i["o"], i["d"], i["v"], i["t"])
                d_raw = ops.composite_bwd(raw, i["t"], i["d"], i["g_rgb"], None, None, True, ops.ACT_ARTICULATED, ops.plane_samples(planes))
                dplanes, dxp = ops.art_bwd_chain(pb, sm, d_raw, masks, planes)
                grads, g_lat = ops.art_wgrad(planes, dplanes, d_raw, dxp, i["params"], i["lat"], packed_bwd=pb)
                out = [raw, d_raw, dxp[: n * S], *(grads[k] for k in ops.ART_PARAM_ORDER), *(g_lat[k] for k in ("density", "color", "articulation"))]
                # the form without degrees, which ops.py never calls: the same call through the library directly, on buffers of the proxy
                T, dev = ops.torch, planes.device
                ws = T.empty(int(ops.lib.aon_wgrad_workspace_bytes()), dtype=torch.uint8, device=dev)
                g2 = [T.empty(ops.ART_PARAM_SHAPES[k], dtype=torch.float32, device=dev) for k in ops.ART_PARAM_ORDER]
                l2 = [T.empty(w, dtype=torch.float32, device=dev) for w in (128, 128, 32)]
                lat = [i["lat"][k].reshape(-1) for k in ("density", "color", "articulation")]
                p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
                with torch.cuda.device(dev):
                    ops.check(ops.lib.aon_art_wgrad(p(planes), p(dplanes), p(d_raw), p(dxp), ops.plane_samples(planes), _arr([i["params"][k] for k in ops.ART_PARAM_ORDER]),
                                                    *(p(t) for t in lat), _arr(g2), *(p(t) for t in l2), p(ws), ws.numel(), _stream(), ops._pk(pb)), "aon_art_wgrad")
                return out + g2 + l2
            return make, call

for _art in (False, True):
    @case("stage_mlp", f"density_grid_{'art' if _art else 'vanilla'}_5x6x7", ["aon_art_density_grid" if _art else "aon_density_grid"])
    def _(art=_art):
        def make(dev):
            return {"pk": _packs(art, *_net(dev, art))}

        def call(ops, i):
            pk, sm = i["pk"]["fwd"][1], (i["pk"]["small"][1] if art else None)
            act = ops.ACT_ARTICULATED if art else ops.ACT_VANILLA
            return [ops.density_grid(pk, (5, 6, 7), -1.5, 1.5, act, small=sm), ops.density_grid(pk, (5, 6, 7), -1.5, 1.5, ops.ACT_NONE, small=sm, g_begin=11, g_end=97)]
        return make, call


# ================================================================== whole path, inference
def _render(ops, art, pk, *args, **kw):
    if art:
        return ops.art_render_fwd(pk["fwd"][0], pk["small"][0], pk["fwd"][1], pk["small"][1], *args, **kw)
    return ops.render_fwd(pk["fwd"][0], pk["fwd"][1], *args, **kw)


def _flat(levels):
    return [t for lvl in levels for t in lvl]


_INFER = {1: ("L1_det", "bounds_live"), 5: ("L1_det", "L2_det", "L2_rand_noise", "bounds_live", "deg1_8_3", "bounds_rand"), 37: ("L2_det", "L2_rand_noise", "bounds_live")}
for _art in (False, True):
    _stem = "aon_art_render_fwd" if _art else "aon_render_fwd"
    for _n, _kind in SIZES:
        for _var in _INFER[_n]:
            @case("inference", f"{'art_' if _art else ''}render_fwd_n{_n}_{_kind}_{_var}", [_stem + ("_bounds" if "bounds" in _var else "_ex")])
            def _(art=_art, n=_n, kind=_kind, var=_var):
                deg = (1, 8, 3) if var == "deg1_8_3" else (0, 10, 4)
                Sc, Sf = _S(kind)

                def make(dev):
                    o, d, v = _rays(dev, n)
                    i = {"pk": _packs(art, *_net(dev, art, deg), degrees=deg), "o": o, "d": d, "v": v}
                    if "rand" in var:
                        i["t_rand"], i["u"] = _uni(110, n, Sc).to(dev), _uni(111, n, Sf - Sc).to(dev)
                        i["noise"] = [_uni(112, n, Sc).to(dev), _uni(113, n, Sf).to(dev)]
                    if "bounds" in var:
                        i["near"], i["far"] = (NEAR + 0.1 * _uni(114, n, 1)).to(dev), (FAR - 0.1 * _uni(115, n, 1)).to(dev)
                    if "live" in var:
                        live = torch.ones(n, dtype=torch.uint8)
                        live[0] = live[n - 1] = 0
                        i["live"] = live.to(dev)
                    return i

                def call(ops, i):
                    opts = _opts(kind, degrees=deg, noise_std=0.5 if "rand" in var else 0.0)
                    return _flat(_render(ops, art, i["pk"], i["o"], i["d"], i["v"], i.get("near", NEAR), i.get("far", FAR), True, num_levels=1 if "L1" in var else 2,
                                         t_rand=i.get("t_rand"), u=i.get("u"), opts=opts, noise=i.get("noise"), ray_live=i.get("live")))
                return make, call

    for _n, _kind in SIZES[1:]:
        for _var, _form in (("occ", "_occ"), ("stop_eps0", "_stop"), ("stop_eps1e-2", "_stop"), ("stop_eps1e-2_nogrid_live", "_bounds")):
            @case("inference", f"{'art_' if _art else ''}render_fwd_{_var}_n{_n}_{_kind}", [_stem + _form])
            def _(art=_art, n=_n, kind=_kind, var=_var):
                def make(dev):
                    o, d, v = _rays(dev, n)
                    i = {"pk": _packs(art, *_net(dev, art)), "o": o, "d": d, "v": v}
                    if "nogrid" not in var:
                        i["grid"] = _half_space_grid(dev)
                    if "live" in var:
                        live = torch.ones(n, dtype=torch.uint8)
                        live[0] = live[n - 1] = 0
                        i["live"] = live.to(dev)
                    return i

                def call(ops, i):
                    pk = i["pk"]
                    packs = (pk["fwd"][0], pk["small"][0], pk["fwd"][1], pk["small"][1]) if art else (pk["fwd"][0], pk["fwd"][1])
                    rest = (i["o"], i["d"], i["v"], NEAR, FAR, True)
                    if var == "occ":
                        levels, occupied = (ops.art_render_fwd_occ if art else ops.render_fwd_occ)(*packs, *rest, i["grid"], opts=_opts(kind))
                        return _flat(levels) + [occupied]
                    levels, occupied, stop = (ops.art_render_fwd_stop if art else ops.render_fwd_stop)(
                        *packs, *rest, i.get("grid"), 0.0 if "eps0" in var else 1e-2, round_samples=16, opts=_opts(kind), ray_live=i.get("live"))
                    return _flat(levels) + [occupied, stop]
                return make, call


_GEOM = dict(min_deg_point=0, max_deg_point=5, deg_view=1, netdepth=2, netwidth=131, netwidth_condition=72, netdepth_condition=2)


def _gnet(dev):
    from aon_amd import ops
    geom = ops.MlpGeometry(**_GEOM)
    sd = _syn().make_general_nerf_state_dict(21, **_GEOM)
    return geom, [{k[len(p):]: v.to(dev) for k, v in sd.items() if k.startswith(p)} for p in ("coarse_mlp.", "fine_mlp.")]


@case("general", "grender_fwd_n5_small", ["aon_grender_fwd"])
def _():
    def make(dev):
        o, d, v = _rays(dev, 5)
        geom, params = _gnet(dev)
        return {"geom": geom, "params": params, "o": o, "d": d, "v": v, "t_rand": _uni(120, 5, 41).to(dev), "u": _uni(121, 5, 72).to(dev)}

    def call(ops, i):
        pc, pf = i["params"]
        return (_flat(ops.grender_fwd(i["geom"], pc, pf, i["o"], i["d"], i["v"], NEAR, FAR, True, opts=_opts("small")))
                + _flat(ops.grender_fwd(i["geom"], pc, None, i["o"], i["d"], i["v"], NEAR, FAR, False, num_levels=1, t_rand=i["t_rand"], opts=_opts("small"))))
    return make, call


@case("general", "grender_train_n5_small", ["aon_grender_fwd_train", "aon_grender_bwd"])
def _():
    def make(dev):
        o, d, v = _rays(dev, 5)
        geom, params = _gnet(dev)
        return {"geom": geom, "params": params, "o": o, "d": d, "v": v, "t_rand": _uni(120, 5, 41).to(dev), "u": _uni(121, 5, 72).to(dev),
                "g_rgb": [(_uni(122 + k, 5, 3) - 0.5).to(dev) for k in range(2)], "g_acc": (_uni(124, 5) - 0.5).to(dev)}

    def call(ops, i):
        geom = i["geom"]
        levels, ws, geometry = ops.grender_fwd_train(geom, *i["params"], i["o"], i["d"], i["v"], NEAR, FAR, True, 2, i["t_rand"], i["u"], opts=_opts("small"))
        grads = ops.grender_bwd(geom, ws, i["params"], i["d"], True, 2, i["g_rgb"], [None, i["g_acc"]], [None, None], geometry)
        ops.pool_give(ws)
        return _flat(levels) + [g[k] for g in grads for k in geom.param_order]
    return make, call


# ================================================================== whole path, training
_TRAIN = {1: ("L2",), 5: ("L2", "L1", "bounds", "deg1_8_3"), 37: ("L2", "bounds")}
for _art in (False, True):
    _f = "aon_art_render_fwd_train" if _art else "aon_render_fwd_train"
    for _n, _kind in SIZES:
        for _var in _TRAIN[_n]:
            @case("training", f"{'art_' if _art else ''}train_n{_n}_{_kind}_{_var}",
                  [_f + ("_bounds" if _var == "bounds" else "_ex"), "aon_art_render_bwd_ex" if _art else "aon_render_bwd_ex"])
            def _(art=_art, n=_n, kind=_kind, var=_var):
                deg = (1, 8, 3) if var == "deg1_8_3" else (0, 10, 4)
                k = 1 if var == "L1" else 2
                Sc, Sf = _S(kind)

                def make(dev):
                    o, d, v = _rays(dev, n)
                    params, lat = _net(dev, art, deg)
                    i = {"pk": _packs(art, params, lat, degrees=deg, bwd=True), "params": params, "lat": lat, "o": o, "d": d, "v": v,
                         "t_rand": _uni(130, n, Sc).to(dev), "u": _uni(131, n, Sf - Sc).to(dev), "g_rgb": [(_uni(132 + l, n, 3) - 0.5).to(dev) for l in range(k)],
                         "g_acc": (_uni(134, n) - 0.5).to(dev), "g_depth": (_uni(135, n) - 0.5).to(dev)}
                    if var == "bounds":
                        i["near"], i["far"] = (NEAR + 0.1 * _uni(136, n, 1)).to(dev), (FAR - 0.1 * _uni(137, n, 1)).to(dev)
                    return i

                def call(ops, i):
                    pk = i["pk"]
                    sm = pk.get("small", [None, None])
                    levels, ws, geometry = ops.render_fwd_train(pk["fwd"][0], pk["fwd"][1] if k == 2 else None, i["o"], i["d"], i["v"], i.get("near", NEAR), i.get("far", FAR),
                                                                True, k, i["t_rand"], i["u"] if k == 2 else None, small_c=sm[0], small_f=sm[1] if k == 2 else None,
                                                                opts=_opts(kind, degrees=deg))
                    g_acc, g_depth = ([None] * (k - 1) + [i["g_acc"]], [i["g_depth"]] + [None] * (k - 1)) if n != 1 else ([None] * k, [None] * k)
                    if art:
                        # caller-supplied gradient buffers at 5 rays: what a gradient arena hands in
                        shapes = ops.art_param_shapes(deg)
                        outs = [[ops.torch.empty(shapes[nm], dtype=torch.float32, device=i["d"].device) for nm in ops.ART_PARAM_ORDER] for _ in range(k)] if n == 5 else None
                        grads, g_lat = ops.art_render_bwd(ws, pk["bwd"][:k], pk["small"][:k], i["d"], True, k, i["g_rgb"], g_acc, g_depth, i["params"][:k], i["lat"],
                                                          geometry=geometry, grads_out=outs)
                        extra = [g_lat[key] for key in ("density", "color", "articulation")]
                        order = ops.ART_PARAM_ORDER
                    else:
                        grads = ops.render_bwd(ws, pk["bwd"][:k], pk["fwd"][:k], i["d"], True, k, i["g_rgb"], g_acc, g_depth, geometry=geometry)
                        extra, order = [], ops.VANILLA_PARAM_ORDER
                    ops.pool_give(ws)
                    return _flat(levels) + [g[nm] for g in grads for nm in order] + extra
                return make, call

for _n, _kind in SIZES:
    @case("training", f"art_frozen_backwards_n{_n}_{_kind}", ["aon_art_render_fwd_train_ex", "aon_art_render_bwd_latents", "aon_art_render_bwd_inputs"])
    def _(n=_n, kind=_kind):
        Sc, Sf = _S(kind)

        def make(dev):
            o, d, v = _rays(dev, n)
            params, lat = _net(dev, True)
            return {"pk": _packs(True, params, lat, bwd=True), "params": params, "o": o, "d": d, "v": v, "t_rand": _uni(140, n, Sc).to(dev), "u": _uni(141, n, Sf - Sc).to(dev),
                    "g_rgb": [(_uni(142 + l, n, 3) - 0.5).to(dev) for l in range(2)], "g_depth": (_uni(144, n) - 0.5).to(dev)}

        def call(ops, i):
            pk, out = i["pk"], []
            for which in ("latents", "inputs", "inputs_nolatents"):
                levels, ws, geometry = ops.render_fwd_train(pk["fwd"][0], pk["fwd"][1], i["o"], i["d"], i["v"], NEAR, FAR, True, 2, i["t_rand"], i["u"], small_c=pk["small"][0],
                                                            small_f=pk["small"][1], opts=_opts(kind))
                head = (ws, pk["bwd"], pk["small"])
                tail = (True, 2, i["g_rgb"], [None, None], [None, i["g_depth"]], i["params"])
                if which == "latents":
                    g_lat = ops.art_render_bwd_latents(*head, i["d"], *tail, geometry=geometry)
                    out += _flat(levels) + [g_lat[key] for key in ("density", "color", "articulation")]
                else:
                    g_lat, *g_rays = ops.art_render_bwd_inputs(*head, i["o"], i["d"], i["v"], *tail, geometry=geometry, want_latents=which == "inputs")
                    out += ([g_lat[key] for key in ("density", "color", "articulation")] if g_lat is not None else []) + g_rays
                ops.pool_give(ws)
            return out
        return make, call


# ================================================================== one training step per network through the drop-in modules
for _art in (False, True):
    for _n, _kind in SIZES[1:]:
        @case("modules", f"{'NeRF_AE_Art' if _art else 'NeRF'}_step_n{_n}_{_kind}",
              ["aon_art_render_fwd_train_ex", "aon_art_render_bwd_ex", "aon_code_library_fwd", "aon_code_library_bwd", "aon_train_loss_fwd", "aon_train_loss_bwd", "aon_adam_step"]
              if _art else ["aon_render_fwd_train_ex", "aon_render_bwd_ex", "aon_train_loss_fwd", "aon_train_loss_bwd", "aon_adam_step"])
        def _(art=_art, n=_n, kind=_kind):
            Sc, Sf = _S(kind)

            def make(dev):
                o, d, v = _rays(dev, n)
                return {"rays": {"rays_o": o, "rays_d": d, "viewdirs": v}, "target": _uni(150, n, 3).to(dev), "t_rand": _uni(151, n, Sc).to(dev),
                        "u": _uni(152, n, Sf - Sc).to(dev), "dev": dev}

            def call(ops, i):
                from aon_amd.arena import ArenaAdam, ParamArena
                from aon_amd.models.vanilla_nerf.helper import train_loss
                syn, dev = _syn(), i["dev"]
                kw = dict(num_coarse_samples=Sc - 1, num_fine_samples=Sf - Sc)
                if art:
                    from aon_amd.models.code_library import CodeLibraryArticulated
                    from aon_amd.models.vanilla_nerf.model_autodecoder import NeRF_AE_Art
                    model = NeRF_AE_Art(**kw).to(dev)
                    model.load_state_dict(syn.make_art_state_dict(seed=5, density_scale=2.0))
                    lib = CodeLibraryArticulated(types.SimpleNamespace(N_max_objs=2, N_obj_code_length=128)).to(dev)
                    lib.load_state_dict(syn.make_code_library_state(seed=3, n_max_objs=2))
                    mods = [model, lib]
                else:
                    from aon_amd.models.vanilla_nerf.model import NeRF
                    model = NeRF(**kw).to(dev)
                    model.load_state_dict(syn.make_nerf_state_dict(seed=0, density_scale=30.0))
                    mods = [model]
                arena = ParamArena(mods)
                opt = ArenaAdam(arena)
                if art:
                    lat = lib({"instance_id": torch.tensor([1], device=dev), "articulation_id": torch.tensor([6], device=dev)})
                    out = model(i["rays"], True, True, NEAR, FAR, lat, t_rand=i["t_rand"], u=i["u"])
                    loss, _ = train_loss(out, i["target"], (lat["density"], lat["color"], lat["articulation"]), 1e-4)
                else:
                    out = model(i["rays"], True, True, NEAR, FAR, t_rand=i["t_rand"], u=i["u"])
                    loss, _ = train_loss(out, i["target"])
                loss.backward()
                named = [(f"{k}.{nm}", p) for k, m in enumerate(mods) for nm, p in m.named_parameters()]
                assert all(p.grad is not None for _, p in named), [nm for nm, p in named if p.grad is None]
                grads = [p.grad.detach().clone() for _, p in named]
                opt.step()
                return [loss.detach(), *grads, *(p.detach().clone() for _, p in named)]
            return make, call


# ================================================================== the tests
@pytest.mark.parametrize("c", _group("stage"))
def test_stage_calls(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("composite"))
def test_compositing_and_pdf(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("optimiser"))
def test_optimiser(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("packing"))
def test_packing(dev, monkeypatch, fold_form, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("stage_mlp"))
def test_stage_calls_on_a_network(dev, monkeypatch, fold_form, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("folded_only"))
def test_stage_calls_of_the_folded_form(dev, monkeypatch, c):
    from aon_amd import ops
    before = ops.bottleneck_fold()
    ops.set_bottleneck_fold(True)
    try:
        run_case(c, dev, monkeypatch)
    finally:
        ops.set_bottleneck_fold(before)


@pytest.mark.parametrize("c", _group("inference"))
def test_whole_path_inference(dev, monkeypatch, fold_form, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("general"))
def test_whole_path_general_engine(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("training"))
def test_whole_path_training(dev, monkeypatch, fold_form, c):
    run_case(c, dev, monkeypatch)


@pytest.mark.parametrize("c", _group("modules"))
def test_training_step_through_the_modules(dev, monkeypatch, fold_form, c):
    run_case(c, dev, monkeypatch)


def test_every_stream_entry_point_was_reached(dev, monkeypatch):
    """The run-time half of tests/test_guard_cpu.py's completeness test: the names the recorder saw over the whole table.  Cases that did
    not run in this process (a selection with -k) run here once, guarded."""
    from test_guard_cpu import stream_entry_points

    for c in CASES:
        if c.name not in _RAN and not c.xfail:
            _one_run(c, dev, monkeypatch, "nan")
    names = stream_entry_points()
    missing = [n for n in names if n not in _SEEN and n not in EXCLUDED]
    assert not missing, f"stream-taking entry points never fetched by any case: {missing}"
    print(f"\n{len(CASES)} cases, {len([n for n in names if n in _SEEN])} of {len(names)} stream-taking entry points reached, {len(EXCLUDED)} excluded")
