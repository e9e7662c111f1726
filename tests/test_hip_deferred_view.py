"""The deferred view branch of the vanilla whole-path renders (ops.set_deferred_view): with the switch on, the MLP
kernel stops behind the density head, the samples with raw sigma > 0 are compacted and a second kernel runs the view layer and the rgb head
on them alone.  A sample with raw sigma <= 0 has density relu(raw sigma) = 0, weight exactly 0, and its colour is never seen -- so every
output of the call must have the SAME BITS with the switch on and off.  Checked here on fields with mixed, all-dead, all-live and exactly
zero densities, on ray counts that are no multiple of a tile, a pass or a slab, with other sample counts, per-ray bounds, a full occupancy
grid, a side stream, and with the new workspace regions under guard bands."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
RAYS = (1, 7, 333, 4096)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from aon_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _switches_back(ops):
    yield
    ops.set_deferred_view(True)
    ops.lib.aon_test_set_deferred_slab(0)


def _state_dict(field):
    import aon_amd.synthetic as syn
    if field == "smooth":
        return syn.make_smooth_nerf_state_dict()
    sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)      # "mixed": raw sigma of both signs along every ray
    for lvl in ("coarse_mlp.", "fine_mlp."):
        if field == "dead":        # no live sample: the view kernel is launched on an empty list
            sd[lvl + "density_layer.bias"] = sd[lvl + "density_layer.bias"] - 1e3
        elif field == "live":      # every sample live
            sd[lvl + "density_layer.bias"] = sd[lvl + "density_layer.bias"] + 1e3
        elif field == "zero":      # raw sigma is exactly +0.0 everywhere: dead
            sd[lvl + "density_layer.weight"] = torch.zeros_like(sd[lvl + "density_layer.weight"])
            sd[lvl + "density_layer.bias"] = torch.zeros_like(sd[lvl + "density_layer.bias"])
    return sd


_PACKS: dict = {}


def _packs(ops, dev, field):
    if field not in _PACKS:
        sd = _state_dict(field)
        _PACKS[field] = tuple(ops.pack_vanilla_mlp({k[len(p):]: v.to(dev) for k, v in sd.items() if k.startswith(p)}) for p in ("coarse_mlp.", "fine_mlp."))
    return _PACKS[field]


_RAYS: dict = {}


def _rays(dev, n):
    if n not in _RAYS:
        import aon_amd.synthetic as syn
        r = syn.random_rays(n, seed=40 + n % 7)
        _RAYS[n] = tuple(r[k].to(dev) for k in ("rays_o", "rays_d", "viewdirs"))
    return _RAYS[n]


def _flat(levels):
    return [t for lvl in levels for t in lvl]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_guard.bits(a), _guard.bits(b)), f"{what}: output {i} differs in {int((_guard.bits(a) != _guard.bits(b)).sum())} of {a.numel()} words"


def _on_off(ops, fn):
    ops.set_deferred_view(True)
    on = fn()
    ops.set_deferred_view(False)
    off = fn()
    ops.set_deferred_view(True)
    return on, off


@pytest.mark.parametrize("samples", ["default", "32_64"])
@pytest.mark.parametrize("n", RAYS)
@pytest.mark.parametrize("field", ["mixed", "smooth", "dead", "live", "zero"])
def test_same_bits_with_the_switch_on_and_off(ops, dev, field, n, samples):
    pc, pf = _packs(ops, dev, field)
    o, d, v = _rays(dev, n)
    opts = None if samples == "default" else ops.RenderOpts(num_coarse_samples=32, num_fine_samples=64)
    on, off = _on_off(ops, lambda: _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True, opts=opts)))
    _same(on, off, f"{field}, {n} rays, {samples}")
    if field in ("mixed", "smooth", "live"):     # not vacuous: the picture has colour in it
        assert float(on[1].max()) > 0.0


@pytest.mark.parametrize("field", ["mixed", "live"])
def test_slabs_of_128_rays(ops, dev, field):
    """333 rays in slabs of 128: two slab borders per level, the last slab partial."""
    pc, pf = _packs(ops, dev, field)
    o, d, v = _rays(dev, 333)
    whole = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    ops.lib.aon_test_set_deferred_slab(128)
    ops.release_workspaces()
    on, off = _on_off(ops, lambda: _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True)))
    _same(on, off, "slabs of 128, on vs off")
    _same(on, whole, "slabs of 128 vs one slab")


def test_per_ray_bounds_and_one_level(ops, dev):
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, 333)
    import aon_amd.synthetic as syn
    near = (NEAR + 0.3 * syn.seeded_uniform(71, 333)).to(dev)
    far = (FAR - 0.3 * syn.seeded_uniform(72, 333)).to(dev)
    on, off = _on_off(ops, lambda: _flat(ops.render_fwd(pc, pf, o, d, v, near, far, True)))
    _same(on, off, "per-ray near / far")
    on, off = _on_off(ops, lambda: _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, False, num_levels=1)))
    _same(on, off, "one level, black background")


def test_full_grid_occ_call_equals_the_dense_call(ops, dev):
    """The _occ call on a grid whose every cell is occupied lists every sample: the dense call's bits, switch on."""
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, 333)
    grid = ops.occupancy_grid(torch.ones((5, 5, 5), device=dev), -12.0, 12.0, threshold=0.5, dilate=0)
    ops.set_deferred_view(True)
    dense = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    levels, occupied = ops.render_fwd_occ(pc, pf, o, d, v, NEAR, FAR, True, grid)
    assert occupied.tolist() == [333 * 65, 333 * 193]
    _same(_flat(levels), dense, "_occ on a full grid vs dense")


def test_density_noise_keeps_the_single_kernel_bits(ops, dev):
    """Noise can lift a sample with raw sigma <= 0 above zero: a level with noise does not defer, and the bits stay."""
    import aon_amd.synthetic as syn
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, 333)
    noise = [syn.seeded_uniform(81, 333, 65).to(dev), syn.seeded_uniform(82, 333, 193).to(dev)]
    opts = ops.RenderOpts(noise_std=0.5)
    on, off = _on_off(ops, lambda: _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True, opts=opts, noise=noise)))
    _same(on, off, "density noise")


def test_on_a_side_stream(ops, dev):
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, 333)
    want = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    torch.cuda.synchronize()
    # torch hands out its 32 pooled side streams round-robin: a whole round of them, so that the tests behind this file get the streams
    # (and the hardware queues) they get without it -- tests/test_hip_scene_occ.py's overlap check depends on which one it is given
    side = [torch.cuda.Stream(device=dev) for _ in range(32)][0]
    with torch.cuda.stream(side):
        got = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    side.synchronize()
    _same(got, want, "side stream vs default stream")


@pytest.mark.parametrize("prefill", ["nan", "zero"])
def test_under_guard_bands(ops, dev, monkeypatch, prefill):
    """Every buffer of the call -- the workspace with the marks, the live list and the rows at its end among them -- between 0xFF bands,
    allocated at exactly the requested size and pre-filled: no band byte changes, and the outputs do not depend on the prefill."""
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, 333)
    want = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    with _guard.guarded(monkeypatch, prefill) as (alloc, rec):
        got = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
        alloc.check()
        assert "aon_render_deferred_workspace_bytes" in rec.names
        got = [g.clone() for g in got]
    _same(got, want, f"guarded ({prefill}) vs plain")


def test_nothing_is_written_past_the_live_count(ops, dev):
    """The C call on a workspace of exactly aon_render_deferred_workspace_bytes(n), pre-filled with 0xFF and followed by a band.  Behind
    the plain layout lie the marks, the live list and the rows (include/aon_hip.h).  After the call they hold the FINE level: the list is
    the ascending indices of the marked samples and is untouched behind their count; a dead sample's row is untouched (where the coarse
    level, which used the same buffers before, had no sample); a live sample's row is fully written; the band is intact."""
    n, Sf = 333, 193
    pc, pf = _packs(ops, dev, "mixed")
    o, d, v = _rays(dev, n)
    lib = ops.lib
    ops.set_deferred_view(True)
    want = _flat(ops.render_fwd(pc, pf, o, d, v, NEAR, FAR, True))
    plain, need = int(lib.aon_render_workspace_bytes_ex(n, None)), int(lib.aon_render_deferred_workspace_bytes(n, None))
    up = lambda b: (b + 255) // 256 * 256   # noqa: E731
    assert need >= plain + up(n * Sf) + n * Sf * 4 + n * Sf * 1024
    band = 4096
    buf = torch.full((need + band,), 0xFF, dtype=torch.uint8, device=dev)
    call = ops._PathCall(o, d, v, NEAR, FAR, True, 2, None, None, None, None)
    args = list(call.args(buf))
    assert args[-3] == buf.numel()
    args[-3] = need      # (workspace, workspace_bytes, stream, opts): the band is not part of the workspace
    with torch.cuda.device(dev):
        ops.check(lib.aon_render_fwd_ex(ops._pk(pc), ops._pk(pf), *args), "aon_render_fwd_ex")
    torch.cuda.synchronize()
    _same(_flat(call.outs), want, "exact workspace vs ops.render_fwd")
    assert bool((buf[need:] == 0xFF).all()), "the band behind the workspace was written"
    marks = buf[plain:plain + n * Sf]
    assert bool((marks <= 1).all()), "a sample without a mark"
    live = torch.nonzero(marks).flatten().to(torch.int32)
    count = live.numel()
    assert 0 < count < n * Sf
    lst = buf[plain + up(n * Sf):plain + up(n * Sf) + n * Sf * 4].view(torch.int32)
    assert torch.equal(lst[:count], live), "the live list is not the ascending marked samples"
    assert bool((lst[count:] == -1).all()), "the live list was written behind its count"
    rows_at = need - up(n * Sf * 1024)
    rows = buf[rows_at:rows_at + n * Sf * 1024].view(torch.int32).view(n * Sf, 256)
    dead = marks == 0
    fine_only = torch.arange(n * Sf, device=dev) >= n * 65      # (rows below n * 65 may hold a live COARSE sample's values)
    assert int((dead & fine_only).sum()) > 0
    assert bool((rows[dead & fine_only] == -1).all()), "a dead sample's row was written"
    assert not bool((rows[~dead] == -1).any()), "a live sample's row holds an unwritten word"
    assert bool((rows[~dead] >= 0).all()), "a live sample's row holds a negative value behind the ReLU"
