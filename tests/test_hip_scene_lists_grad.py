"""GPU: gradients through scenes with a backdrop (csrc/aon_scene_lists_grad.hip, include/aon_hip_scene_lists_grad.h).

Kernel: aon_scene_composite_lists_bwd against tests/_scene_lists_grad_ref.composite_grads (torch autograd in fp64 on the same raw and the HIP
samplers' t), bar max|got - ref| / max_ray|ref| < 2e-5 -- the project's own for aon_composite_bwd and aon_scene_composite_bwd, computed as
tests/test_hip_scene_grad.py computes it; mixed activations, an open list in the middle, the open list's last sample, ties, sentinels.
Bits: homogeneous closed lists are aon_scene_composite_bwd's; repeat, permuted rays, a sub-batch, a side stream.  Memory: guard bands, rows
past `pairs`, NULL upstream gradients, rows no slot names.  One level through the networks: autograd.RenderLevelSceneLists against the
oracle's autograd (tests/_gradcheck.py).  Whole path: scene.render_scene_background_grad against scene.render_scene(background=...)
(forward bits) and against the chain written out with stage calls (gradient bits).  LitNeRF_AutoDecoder.fit_scene_codes / fit_scene_poses
with a backdrop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guard  # noqa: E402
import _scene_lists_grad_ref as lgref  # noqa: E402
import test_hip_scene_grad as hsg  # noqa: E402
import test_hip_scene_lists as hl  # noqa: E402
from test_hip_extents import Case, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("density", "color", "articulation")
BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def same(a, b):
    return torch.equal(_guard.bits(a), _guard.bits(b))


# ------------------------------------------------------------------ the kernel against the fp64 restatement
#         n   lists S
SHAPES = [(5,  1,  2), (5, 2, 2), (5, 2, 3), (37, 2, 65), (37, 4, 65), (9, 3, 32), (9, 6, 13), (20, 16, 193), (7, 16, 256)]


def chain(dev, rays_cpu, objects, raw_full, S, edit_t=None, far=hl.BG_FAR):
    """pairs + backdrop -> HIP sampler -> seeded raw (named by (ray, list)) -> (pairs, t, raw)"""
    from aon_amd import ops

    rays = hl.to_dev(rays_cpu, dev)
    _, pairs = hl.bg_pairs(ops, rays, objects, hl.BG_NEAR, far)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    if edit_t is not None:
        t = edit_t(pairs, t)
    return pairs, t, hl.gather_raw(raw_full.to(dev), pairs)


def backward(dev, pairs, t, raw, rays_cpu, g, white, lists, nulls=False):
    from aon_amd import ops

    gd = {k: v.to(dev) for k, v in g.items()}
    extra = {} if nulls else {k: gd[k] for k in ("g_acc", "g_depth", "g_obj_acc")}
    return ops.scene_composite_lists_bwd(raw, t, pairs, rays_cpu["rays_d"].to(dev), gd["g_rgb"], white_bkgd=white, lists=lists, **extra)


def reference(pairs, t, raw, rays_cpu, g, white, ref_lists, nulls=False):
    extra = {} if nulls else {k: g[k].numpy() for k in ("g_acc", "g_depth", "g_obj_acc")}
    return lgref.composite_grads(raw.cpu().numpy(), t.cpu().numpy(), pairs.slot.cpu().numpy(), rays_cpu["rays_d"].numpy(), white, ref_lists,
                                 g["g_rgb"].numpy(), **extra)


@pytest.mark.parametrize("nulls", [False, True], ids=["all_four", "rgb_only"])
@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{n}_l{L}_s{S}" for n, L, S in SHAPES])
def test_backward_against_fp64(dev, shape, white, nulls):
    from aon_amd import ops

    n, L, S = shape
    K = L - 1
    objects = hl.layout_objects(K)
    rays_cpu = hl.mixed_rays(n, seed=7)
    pairs, t, raw = chain(dev, rays_cpu, objects, hl.seeded_raw(40 + L + S, n, L, S), S)
    live_lists = (pairs.slot >= 0).sum(1).cpu()
    assert pairs.K == L and pairs.counts[K] == n and (live_lists >= 1).all()
    if K:
        assert (live_lists >= 2).any()
    if shape == (37, 2, 65):
        assert (live_lists * S == 130).any()                                             # two scan blocks and a bit: the carry
    if shape == (7, 16, 256):
        assert L * S == 4096
    last = raw[pairs.segment(K)][:, -1, 3].cpu()
    assert (last == 0).any() and (last == 40).any()
    g = hsg.upstream(3 + n, n, L)
    got = backward(dev, pairs, t, raw, rays_cpu, g, white, hl.scene_lists(ops, K), nulls)
    ref = reference(pairs, t, raw, rays_cpu, g, white, hl.REF_LISTS(K), nulls)
    torch.cuda.synchronize()
    fig = hsg.figure(got, ref, pairs)
    print(f"{shape} white={white} nulls={nulls}: P={pairs.P} of {n * L}, worst |got - ref| / max_ray|ref| = {fig:.2e} (bar {BAR:.0e})")
    assert tuple(got.shape) == (pairs.P, S, 4) and bool(torch.isfinite(got).all())
    assert float(ref.abs().max()) > 1e-3
    assert fig < BAR
    if K:
        assert not got[: pairs.starts[K], S - 1].any()                                   # closed lists: delta = 0, exact zeros
    bg_last = got[pairs.segment(K)][:, S - 1]
    assert bg_last[:, :3].any()                                                          # the open list's last sample has a real colour gradient
    sat = (last == 0) | (last == 40)
    assert not bg_last[sat.to(dev), 3].any() and not torch.signbit(bg_last[sat.to(dev), 3]).any()     # sigma' = 0 or exp underflows: +0


def test_mixed_lists_and_an_open_list_in_the_middle(dev):
    """lists of act 0, 1 (open, in the middle: it ends at t <= 3.6 while the others reach behind it), 2 and the vanilla open backdrop in
    one ray; the middle open list's last raw sigma is exactly 0, 40 and 1e-10 on a third of the rays each"""
    from aon_amd import ops

    n, S = 12, 17
    ob = hl.nested(0, 0)
    rays_cpu = hl.frame_rays(n)
    raw_full = hl.seeded_raw(21, n, 4, S)
    raw_full[:, 0, :, 3] = raw_full[:, 0, :, 3].abs() * 0.3                              # act 0 reads raw sigma as the density
    raw_full[0::3, 1, -1, 3], raw_full[1::3, 1, -1, 3], raw_full[2::3, 1, -1, 3] = 0.0, 40.0, 1e-10

    def squeeze(pairs, t):
        t = t.clone()
        seg = pairs.segment(1)
        lo = t[seg][:, :1]
        t[seg] = lo + (t[seg] - lo) * ((3.0 - lo).clamp_min(0.05) / (t[seg][:, -1:] - lo))     # list 1 ends at t = 3 (in front of the box's end)
        return t
    pairs, t, raw = chain(dev, rays_cpu, [ob, ob, ob], raw_full, S, edit_t=squeeze)
    assert pairs.counts[:3] == [n, n, n]
    lists = [ops.SceneList(ops.ACT_NONE), ops.SceneList(ops.ACT_VANILLA, True), ops.SceneList(ops.ACT_ARTICULATED, False, ops.RenderOpts(rgb_padding=0.01, density_bias=0.5)),
             ops.SceneList(ops.ACT_VANILLA, True)]
    ref_lists = [(0, None, False), (1, None, True), (2, {"rgb_padding": 0.01, "density_bias": 0.5}, False), (1, None, True)]
    g = hsg.upstream(5, n, 4)
    for white in (True, False):
        got = backward(dev, pairs, t, raw, rays_cpu, g, white, lists)
        ref = reference(pairs, t, raw, rays_cpu, g, white, ref_lists)
        fig = hsg.figure(got, ref, pairs)
        print(f"mixed lists white={white}: {fig:.2e}")
        assert bool(torch.isfinite(got).all()) and fig < BAR
        mid = got[pairs.segment(1)][:, -1, 3].cpu()
        assert not mid[0::3].any() and not mid[1::3].any() and not torch.signbit(mid[0::3]).any() and not torch.signbit(mid[1::3]).any()
        big = mid[2::3].abs()
        print(f"  open list's last density entry at raw sigma 1e-10: {big.min():.3e} .. {big.max():.3e}")
        assert bool((big > 1e5).all()) and bool((big < 1e12).all())                      # sigma 1e10 N is O(1): large and finite
        # behind a dense open end (raw sigma 40) everything is at the formula's T <= 1e-10 scale
        rows0 = pairs.slot[1::3, 0].long()
        behind = (t[rows0] > 3.0).cpu()
        assert bool(behind.any(1).all())
        small = got[rows0].cpu()[behind]
        assert bool(torch.isfinite(small).all()) and float(small[:, :3].abs().max()) <= 1e-8 and float(small[:, :3].abs().max()) > 0


def test_ties_and_sentinels(dev):
    from aon_amd import ops

    n, S = 9, 17
    rays_cpu = hl.frame_rays(n)

    def copy_t(pairs, t):
        slot0 = pairs.slot[:, 0].long()
        hit = slot0 >= 0
        assert bool(hit.any())
        t = t.clone()
        t[pairs.segment(1)][hit] = t[slot0[hit]]
        return t
    pairs, t, raw = chain(dev, rays_cpu, [hl.nested(0, 1)], hl.seeded_raw(9, n, 2, S), S, edit_t=copy_t)
    hit = (pairs.slot[:, 0] >= 0)
    assert same(t[pairs.slot[:, 0].long()[hit]], t[pairs.slot[:, 1].long()[hit]])
    g = hsg.upstream(5, n, 2)
    got = backward(dev, pairs, t, raw, rays_cpu, g, True, hl.scene_lists(ops, 1))
    assert hsg.figure(got, reference(pairs, t, raw, rays_cpu, g, True, hl.REF_LISTS(1)), pairs) < BAR
    # sentinel records in both lists: exact zeros, no NaN
    sentinel = torch.tensor([0.0, 0.0, 0.0, float("-inf")], device=dev)
    mask = torch.from_numpy(np.random.default_rng(2).random((pairs.P, S)) < 0.3).to(dev)
    mask[1] = True
    mask[pairs.P - 1] = True                                                             # a whole backdrop list, its open end included
    raw = raw.clone()
    raw[mask] = sentinel
    for white in (True, False):
        got = backward(dev, pairs, t, raw, rays_cpu, g, white, hl.scene_lists(ops, 1))
        assert bool(torch.isfinite(got).all()) and not got[mask].any() and got[~mask].any()
        assert hsg.figure(got, reference(pairs, t, raw, rays_cpu, g, white, hl.REF_LISTS(1)), pairs) < BAR


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("K", [1, 3, 16])
def test_homogeneous_closed_lists_are_scene_composite_bwd_bit_for_bit(dev, K):
    from aon_amd import ops

    n, S = 37, 65
    rays_cpu = hl.mixed_rays(n, seed=7)
    rays = hl.to_dev(rays_cpu, dev)
    pairs = ops.scene_pairs(rays["rays_o"], rays["rays_d"], rays["viewdirs"], hl.layout_objects(K))
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    raw = hl.gather_raw(hl.seeded_raw(5, n, K + 1, S)[:, :K].contiguous().to(dev), pairs)
    g = {k: v.to(dev) for k, v in hsg.upstream(6, n, K).items()}
    custom = ops.RenderOpts(rgb_padding=0.01, density_bias=0.5)
    for act, opts in ((ops.ACT_ARTICULATED, None), (ops.ACT_ARTICULATED, custom), (ops.ACT_VANILLA, None), (ops.ACT_NONE, None)):
        for white in (True, False):
            for extra in ({}, {k: g[k] for k in ("g_acc", "g_depth", "g_obj_acc")}):
                want = ops.scene_composite_bwd(raw, t, pairs, rays["rays_d"], g["g_rgb"], white_bkgd=white, opts=opts, act=act, **extra)
                got = ops.scene_composite_lists_bwd(raw, t, pairs, rays["rays_d"], g["g_rgb"], white_bkgd=white, lists=[ops.SceneList(act, False, opts)] * K,
                                                    **extra)
                assert same(got, want) and bool(want.any()), (K, act, white)


@pytest.mark.parametrize("white", [True, False], ids=["white", "black"])
def test_the_backdrop_alone_is_composite_bwd(dev, white):
    """one open vanilla list against the one-object backward on the same rays: within the bar (whether the bits agree is printed)"""
    from aon_amd import ops

    n, S = 37, 65
    rays_cpu = hl.mixed_rays(n, seed=7)
    pairs, t, raw = chain(dev, rays_cpu, [], hl.seeded_raw(8, n, 1, S), S)
    g = {k: v.to(dev) for k, v in hsg.upstream(7, n, 1).items()}
    d = rays_cpu["rays_d"].to(dev)
    got = ops.scene_composite_lists_bwd(raw, t, pairs, d, g["g_rgb"], g["g_acc"], g["g_depth"], None, white, [ops.SceneList(ops.ACT_VANILLA, True)])
    want = ops.composite_bwd(raw, t, d, g["g_rgb"], g["g_acc"], g["g_depth"], white, ops.ACT_VANILLA, ops.padded_samples(n * S))[: n * S].reshape(n, S, 4)
    fig = hsg.figure(got, want.cpu().double(), pairs)
    print(f"backdrop alone white={white}: |lists bwd - composite_bwd| / max_ray = {fig:.2e}; bit-equal: {same(got, want)}")
    assert fig < BAR and bool(want.any())


def full_rows(d_raw, pairs, n, S):
    out = torch.zeros(n, pairs.K, S, 4)
    slot = pairs.slot.cpu().long()
    r, k = (slot >= 0).nonzero(as_tuple=True)
    out[r, k] = d_raw.cpu()[slot[r, k]]
    return out


def test_bits_do_not_depend_on_the_call(dev):
    from aon_amd import ops

    n, K, S = 37, 3, 65
    objects, rays_cpu, raw_full = hl.layout_objects(K), hl.mixed_rays(n, seed=7), hl.seeded_raw(5, n, K + 1, S)
    g = hsg.upstream(7, n, K + 1)

    def run(rays_cpu, raw_full, g):
        pairs, t, raw = chain(dev, rays_cpu, objects, raw_full, S)
        return full_rows(backward(dev, pairs, t, raw, rays_cpu, g, True, hl.scene_lists(ops, K)), pairs, rays_cpu["rays_o"].shape[0], S), (pairs, t, raw)
    base, (pairs, t, raw) = run(rays_cpu, raw_full, g)
    assert n < pairs.P < n * (K + 1) and base.any()
    assert same(base, run(rays_cpu, raw_full, g)[0])                                                          # repeat
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n))
    assert same(base[perm], run({k: v[perm] for k, v in rays_cpu.items()}, raw_full[perm], {k: v[perm] for k, v in g.items()})[0])
    cut = slice(5, 20)
    assert same(base[cut], run({k: v[cut].contiguous() for k, v in rays_cpu.items()}, raw_full[cut], {k: v[cut].contiguous() for k, v in g.items()})[0])
    side = torch.cuda.Stream(dev, priority=-1)          # (a high-priority stream: see tests/test_hip_scene_lists.py)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = backward(dev, pairs, t, raw, rays_cpu, g, True, hl.scene_lists(ops, K))
    side.synchronize()
    assert same(base, full_rows(got, pairs, n, S))


# ------------------------------------------------------------------ memory
def _guard_case(name, n, K, S):
    def make(dev):
        return {"rays": hl.to_dev(hl.mixed_rays(n, seed=7), dev), "objects": hl.layout_objects(K), "raw_full": hl.seeded_raw(3, n, K + 1, S).to(dev),
                "g": {k: v.to(dev) for k, v in hsg.upstream(8, n, K + 1).items()}}

    def call(ops, i):
        r, g = i["rays"], i["g"]
        _, pairs = hl.bg_pairs(ops, r, i["objects"])
        t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
        return [ops.scene_composite_lists_bwd(hl.gather_raw(i["raw_full"], pairs), t, pairs, r["rays_d"], g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"],
                                              True, hl.scene_lists(ops, K))]
    return Case("scene_lists_grad", name, make, call, ["aon_scene_composite_lists_bwd"])


GUARD_CASES = [_guard_case("scene_lists_grad_n1_bg_s3", 1, 0, 3), _guard_case("scene_lists_grad_n37_k3_s41", 37, 3, 41),
               _guard_case("scene_lists_grad_k15_s256", 7, 15, 256)]


@pytest.mark.parametrize("c", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_memory_contract(dev, monkeypatch, c):
    run_case(c, dev, monkeypatch)


def test_rows_past_pairs_null_gradients_and_unnamed_rows(dev):
    from aon_amd import _lib, ops

    n, S, K = 9, 17, 2
    rays_cpu = hl.mixed_rays(n, seed=7)
    pairs, t, raw = chain(dev, rays_cpu, hl.layout_objects(K), hl.seeded_raw(3, n, K + 1, S), S)
    P = pairs.P
    g = {k: v.to(dev) for k, v in hsg.upstream(9, n, K + 1).items()}
    d = rays_cpu["rays_d"].to(dev)
    lists = hl.scene_lists(ops, K)
    arr = (_lib.SceneListC * (K + 1))()
    for k, x in enumerate(lists):
        x.fill(arr[k])

    def call(slot, pairs_arg, out, nulls=False, stream=None):
        opt = [None] * 3 if nulls else [g[k].data_ptr() for k in ("g_acc", "g_depth", "g_obj_acc")]
        ops.check(ops.lib.aon_scene_composite_lists_bwd(raw.data_ptr(), t.data_ptr(), slot.data_ptr(), d.data_ptr(), g["g_rgb"].data_ptr(), *opt, n, K + 1,
                                                        pairs_arg, S, 1, arr, out.data_ptr(), stream), "aon_scene_composite_lists_bwd")
        torch.cuda.synchronize()
        return out
    want = ops.scene_composite_lists_bwd(raw, t, pairs, d, g["g_rgb"], g["g_acc"], g["g_depth"], g["g_obj_acc"], True, lists)
    for stream in (None, C.c_void_p(torch.cuda.current_stream().cuda_stream)):
        full = call(pairs.slot, P, torch.full((P + 5, S, 4), -7.25, device=dev), stream=stream)
        assert bool((full[P:] == -7.25).all()) and same(full[:P], want)                   # rows past `pairs` keep their prefill
    # NULL g_acc / g_depth / g_obj_acc: zeros
    zeros = ops.scene_composite_lists_bwd(raw, t, pairs, d, g["g_rgb"], torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, K + 1, device=dev),
                                          True, lists)
    assert same(call(pairs.slot, P, torch.zeros((P, S, 4), device=dev), nulls=True), zeros)
    # pairs cut in front of the backdrop's rows: its list is dead on every ray, its rows are never written
    P0 = pairs.starts[K]
    cut = call(pairs.slot, P0, torch.full((P, S, 4), -7.25, device=dev))
    assert bool((cut[P0:] == -7.25).all()) and not bool((cut[:P0] == -7.25).any())
    # a slot that names no row of one ray's lists: those rows are left alone, the other rays keep their bits
    slot = pairs.slot.clone()
    r = int((pairs.slot[:, 0] >= 0).nonzero()[0])
    dropped = int(slot[r, 0])
    slot[r, 0] = -1
    part = call(slot, P, torch.full((P, S, 4), -7.25, device=dev))
    assert bool((part[dropped] == -7.25).all())
    others = torch.ones(P, dtype=torch.bool, device=dev)
    others[pairs.slot[r][pairs.slot[r] >= 0].long()] = False
    assert same(part[others], want[others]) and not bool((part[others] == -7.25).any())


# ------------------------------------------------------------------ one level through the networks
def test_one_level_against_the_oracles_autograd(dev):
    """two objects + backdrop, 8 x 12 rays, S = 16, tests/_gradcheck.py at the factor and floor tests/test_hip_scene_grad.py uses.  The backdrop
    is make_smooth_nerf_state_dict(seed=7): no ray of the fixture sits on the relu kink of the open interval (asserted below on the fp64
    oracle's raw, on every ray: none is left out)."""
    from _gradcheck import assert_as_close_as_fp32
    from aon_amd import ops
    from aon_amd.autograd import RenderLevelSceneLists

    syn = hl._syn()
    sd = syn.make_art_state_dict(seed=0, density_scale=2.0)
    bg_sd = hl.bg_state_dict()
    prefix = "coarse_mlp."
    params = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
    bg_params = {k[len(prefix):]: v.to(dev) for k, v in bg_sd.items() if k.startswith(prefix)}
    specs = [hl.nested(0, 0), (hl.pose(5, (0.3, 0.2, -0.1)), 0.9)]
    rays_cpu = hl.small_frame()
    rays = hl.to_dev(rays_cpu, dev)
    n, S = 96, 16
    obj_pairs, pairs = hl.bg_pairs(ops, rays, specs)
    assert obj_pairs.counts[0] > 0 and obj_pairs.counts[1] > 0 and ((pairs.slot >= 0).sum(1) == 3).any()
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, S - 1, pairs.near, pairs.far, want_coords=False)
    codes = [{k: v.cpu() for k, v in hl.codes("cpu", k).items()} for k in range(2)]
    gen = torch.Generator().manual_seed(31)
    target, w = torch.rand(n, 3, generator=gen), torch.rand(n, 5, generator=gen)
    pr = {"o": pairs.rays_o.cpu().numpy(), "d": pairs.rays_d.cpu().numpy(), "v": pairs.viewdirs.cpu().numpy(), "offsets": np.asarray(pairs.starts),
          "slot": pairs.slot.cpu().numpy()}

    def level_loss(out, target, w):
        rgb, acc, depth, obj_acc = out
        return torch.mean((rgb - target) ** 2) + (0.3 * acc * w[:, 0]).mean() + (0.1 * depth * w[:, 1]).mean() + (0.2 * obj_acc * w[:, 2:5]).mean()

    def oracle(dtype):
        sd_o = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith(prefix)}
        bg_o = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in bg_sd.items() if k.startswith(prefix)}
        lat_o = [{k: v.to(dtype).clone().requires_grad_(True) for k, v in c.items()} for c in codes]
        out = lgref.scene_level_oracle(sd_o, prefix, bg_o, prefix, pr, t.cpu().numpy(), lat_o, rays_cpu["rays_d"].numpy(), True, dtype)
        level_loss((out["rgb"], out["acc"], out["depth"], out["obj_acc"]), target.to(dtype), w.to(dtype)).backward()
        g = {k[len(prefix):]: v.grad for k, v in sd_o.items()}
        g.update({"backdrop." + k[len(prefix):]: v.grad for k, v in bg_o.items()})
        for j, c in enumerate(lat_o):
            g.update({f"object{j}.{k}": v.grad.reshape(-1) for k, v in c.items()})
        return g, out["raw"].detach()

    (g64, raw64), (g32, _) = oracle(torch.float64), oracle(torch.float32)
    last = raw64[pairs.starts[2]:, -1, 3].abs()
    print(f"min |raw sigma_last| of the backdrop in fp64: {float(last.min()):.3e}; rays left out: 0")
    assert last.shape == (n,) and float(last.min()) >= hl.SIGMA_LAST_MARGIN
    leaves = [params[name].clone().requires_grad_(True) for name in ops.ART_PARAM_ORDER]
    bg_leaves = [bg_params[name].clone().requires_grad_(True) for name in ops.VANILLA_PARAM_ORDER]
    lat = [{k: c[k].to(dev).requires_grad_(True) for k in KEYS} for c in codes]
    pd, bd = dict(zip(ops.ART_PARAM_ORDER, leaves)), dict(zip(ops.VANILLA_PARAM_ORDER, bg_leaves))
    out = RenderLevelSceneLists.apply(obj_pairs, t, rays["rays_o"], rays["rays_d"], rays["viewdirs"], specs, True, None, ops.pack_art_mlp(pd),
                                      ops.pack_art_mlp_bwd(pd), (0, 10, 4), pairs, ops.pack_vanilla_mlp(bd), ops.pack_vanilla_mlp_bwd(bd),
                                      *[p for p, _ in specs], *[c[k] for c in lat for k in KEYS], *leaves, *bg_leaves)
    assert not out[4].requires_grad and tuple(out[4].shape) == tuple(t.shape) and tuple(out[3].shape) == (n, 3)
    level_loss(out[:4], target.to(dev), w.to(dev)).backward()
    got = {name: p.grad.cpu() for name, p in pd.items()}
    got.update({"backdrop." + name: p.grad.cpu() for name, p in bd.items()})
    for j, c in enumerate(lat):
        got.update({f"object{j}.{k}": c[k].grad.reshape(-1).cpu() for k in KEYS})
    assert len(got) == 40 + 24 + 6 and all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in got.values())
    assert_as_close_as_fp32(got, g64, g32, "scene + backdrop level, S = 16")


# ------------------------------------------------------------------ the whole path
def _scene_loss(levels, target):
    return hsg._scene_loss(levels, target)


def _pose_objects(dev, specs, code_grads=True, pose_grads=True):
    from aon_amd import scene
    return [scene.SceneObject({k: v.clone().requires_grad_(code_grads) for k, v in hl.codes(dev, j).items()},
                              p.clone().requires_grad_(True) if pose_grads else p, b) for j, (p, b) in enumerate(specs)]


def _fresh_backdrop(dev, levels):
    """a backdrop network of its own (the shared fixture's flags are not touched)"""
    from aon_amd import scene
    from aon_amd.models.vanilla_nerf.model import NeRF

    m = NeRF(num_levels=levels).to(dev)
    m.load_state_dict(hl.bg_state_dict())
    return scene.SceneBackground(m, hl.BG_NEAR, hl.BG_FAR)


def _written_out(model, bg, objects, rays, target, want_poses):
    """render_scene_background_grad's forward and backward with stage-level ops calls; the loss's own derivative from torch on detached leaves
    -> (code gradients, 40 per level, 24 per level, pose gradients or None)"""
    from aon_amd import ops

    K = len(objects)
    obj_pairs, pairs = hl.bg_pairs(ops, rays, objects, bg.near, bg.far)
    P = obj_pairs.P
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, model.num_coarse_samples, pairs.near, pairs.far, want_coords=False)
    lists = [ops.SceneList(ops.ACT_ARTICULATED, False, model._opts)] * K + [ops.SceneList(ops.ACT_VANILLA, True)]
    kept, outs = [], []
    bg_mlps = [bg.model.coarse_mlp, bg.model.fine_mlp]
    for level, mlp in enumerate([model.coarse_mlp, model.fine_mlp][: model.num_levels]):
        params = {k: v.detach() for k, v in mlp.named_parameters()}
        raw = torch.empty((pairs.P, t.shape[1], 4), device=t.device)
        per = []
        for k, ob in enumerate(objects):
            seg = obj_pairs.segment(k)
            if seg.stop > seg.start:
                small = ops.art_prepare(params, ob.latents, degrees=mlp.degrees)
                _, planes, masks = ops.art_mlp_fwd_train(mlp.packed(True), small, pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
                per.append((small, planes, masks))
            else:
                per.append(None)
        bfwd, bbwd = bg_mlps[level].packed(True), bg_mlps[level].packed_bwd(True)
        _, bplanes, bmasks = ops.mlp_fwd_train(bfwd, rays["rays_o"], rays["rays_d"], rays["viewdirs"], t[P:], out=raw[P:])
        rgb, acc, depth, obj_acc, weights = ops.scene_composite_lists(raw, t, pairs, rays["rays_d"], True, lists)
        outs.append([x.detach().requires_grad_(True) for x in (rgb, acc, depth, obj_acc)])
        kept.append((mlp, params, raw, t, per, (bfwd, bbwd, bplanes, bmasks)))
        if level + 1 < model.num_levels:
            t = ops.sample_pdf_t_n(t, weights, model.num_fine_samples)
    up = torch.autograd.grad(_scene_loss(outs, target), [x for lv in outs for x in lv])
    g_codes = [[torch.zeros_like(ob.latents[k]) for k in KEYS] for ob in objects]
    g_params, g_bg, g_pose_total = [], [], None
    for level, (mlp, params, raw, t, per, (bfwd, bbwd, bplanes, bmasks)) in enumerate(kept):
        g_rgb, g_acc, g_depth, g_obj = up[4 * level: 4 * level + 4]
        d_raw = ops.scene_composite_lists_bwd(raw, t, pairs, rays["rays_d"], g_rgb, g_acc, g_depth, g_obj, True, lists)
        bwd, total = mlp.packed_bwd(True), None
        g = torch.zeros((3, P, 3), device=t.device)
        for k, ob in enumerate(objects):
            if per[k] is None:
                continue
            small, planes, masks = per[k]
            seg = obj_pairs.segment(k)
            rows = (seg.stop - seg.start) * t.shape[1]
            buf = torch.zeros((ops.padded_samples(rows), 4), device=t.device)
            buf[:rows] = d_raw[seg].reshape(rows, 4)
            dplanes, dxp = ops.art_bwd_chain(bwd, small, buf, masks, planes)
            for dst, x in zip(g, ops.art_ray_grads(dplanes, dxp, params, t[seg], pairs.viewdirs[seg], mlp.degrees)):
                dst[seg] = x
            grads, g_lat = ops.art_wgrad(planes, dplanes, buf, dxp, params, ob.latents, mlp.degrees, packed_bwd=bwd)
            total = grads if total is None else {name: total[name] + grads[name] for name in ops.ART_PARAM_ORDER}
            for j, key in enumerate(KEYS):
                g_codes[k][j] = g_codes[k][j] + g_lat[key].reshape(g_codes[k][j].shape)
        if total is None:
            total = {name: torch.zeros_like(params[name]) for name in ops.ART_PARAM_ORDER}
        g_params += [total[name] for name in ops.ART_PARAM_ORDER]
        rows = pairs.n * t.shape[1]
        buf = torch.zeros((ops.padded_samples(rows), 4), device=t.device)
        buf[:rows] = d_raw[P:].reshape(rows, 4)
        bgrads = ops.vanilla_wgrad(bplanes, ops.mlp_bwd_chain(bbwd, bfwd, buf, bmasks, bplanes.shape), buf, bbwd)
        g_bg += [bgrads[name] for name in ops.VANILLA_PARAM_ORDER]
        if want_poses and K:
            g_pose = ops.scene_pose_grads(rays["rays_o"], rays["rays_d"], rays["viewdirs"], obj_pairs, objects, g[0], g[1], g[2])
            g_pose_total = g_pose if g_pose_total is None else g_pose_total + g_pose
    poses = None if g_pose_total is None else [torch.cat([g_pose_total[k, :9].view(3, 3), g_pose_total[k, 9:].view(3, 1)], 1).cpu() for k in range(K)]
    return [x for oc in g_codes for x in oc], g_params, g_bg, poses


def _count(monkeypatch, ops, names):
    calls = {name: 0 for name in names}
    for name in names:
        real = getattr(ops, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


BACKDROP_STAGES = ("mlp_fwd_train", "mlp_bwd_chain", "vanilla_wgrad")


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("levels", [1, 2])
def test_render_scene_background_grad_is_render_scene_and_the_written_out_chain(dev, levels, K, monkeypatch):
    from aon_amd import ops, scene

    model, bg = hl.art_model(dev, levels, 16, 16), _fresh_backdrop(dev, levels)
    rays = hl.to_dev(hl.small_frame(), dev)
    specs = hl.THREE()[:K]
    objects = _pose_objects(dev, specs)
    target = hl._syn().seeded_uniform(21, 96, 3).to(dev)
    with torch.no_grad():
        want = scene.render_scene(model, objects, rays, True, background=bg)
    mlps, bg_mlps = [model.coarse_mlp, model.fine_mlp][:levels], [bg.model.coarse_mlp, bg.model.fine_mlp][:levels]
    wrt_codes = [ob.latents[k] for ob in objects for k in KEYS]
    wrt_params = [p for m in mlps for p in m.ordered_params()]
    wrt_bg = [p for m in bg_mlps for p in m.ordered_params()]
    wrt_poses = [ob.pose_tensor for ob in objects]
    got = scene.render_scene_background_grad(model, objects, rays, True, bg)
    assert len(got) == len(want) == levels
    for g, w in zip(got, want):
        assert all(x.requires_grad for x in g) and tuple(g[3].shape) == (96, K + 1)
        for a, b in zip(g, w):
            assert same(a.detach(), b)                                                   # the forward, bit for bit
    assert float(want[-1][3][:, K].max()) > 0.05
    grads = torch.autograd.grad(_scene_loss(got, target), wrt_codes + wrt_params + wrt_bg + wrt_poses)
    ref_codes, ref_params, ref_bg, ref_poses = _written_out(model, bg, objects, rays, target, True)
    ref = ref_codes + ref_params + ref_bg + (ref_poses or [])
    assert len(grads) == len(ref) == 3 * K + 40 * levels + 24 * levels + K
    for i, (a, b) in enumerate(zip(grads, ref)):
        assert same(a, b) and bool(torch.isfinite(a).all()), i                           # the gradients, bit for bit
    assert all(bool(x.any()) for x in grads[3 * K + 40 * levels:])                       # the backdrop's weights and the poses get gradients
    assert all(p.grad is None for p in list(model.parameters()) + list(bg.model.parameters()))
    g_bg_all = grads[3 * K + 40 * levels: 3 * K + 64 * levels]
    # a frozen backdrop: the plane-free forward, no chain and no weight-gradient launch of its own; everything else keeps its bits
    flags = [p.requires_grad for p in bg.model.parameters()]
    for p in bg.model.parameters():
        p.requires_grad_(False)
    calls = _count(monkeypatch, ops, BACKDROP_STAGES + ("mlp_fwd", "art_wgrad"))
    lv = scene.render_scene_background_grad(model, objects, rays, True, bg)
    if K:
        frozen = torch.autograd.grad(_scene_loss(lv, target), wrt_codes + wrt_params + wrt_poses)
        for a, b in zip(frozen, grads[: 3 * K + 40 * levels] + grads[3 * K + 64 * levels:]):
            assert same(a, b)
    else:
        frozen = torch.autograd.grad(_scene_loss(lv, target), wrt_params)                # no object: the scene network's weights get zeros
        assert not any(bool(x.any()) for x in frozen)
    assert [calls[k] for k in BACKDROP_STAGES] == [0, 0, 0] and calls["mlp_fwd"] == levels
    for p, f in zip(bg.model.parameters(), flags):
        p.requires_grad_(f)
    # a trainable backdrop behind frozen objects: the same backdrop gradients, no weight-gradient kernel of the scene network
    m_flags = [p.requires_grad for p in model.parameters()]
    try:
        for p in model.parameters():
            p.requires_grad_(False)
        calls["art_wgrad"] = 0
        still = _pose_objects(dev, specs, code_grads=False, pose_grads=False)
        lv = scene.render_scene_background_grad(model, still, rays, True, bg)
        only_bg = torch.autograd.grad(_scene_loss(lv, target), wrt_bg)
        assert calls["art_wgrad"] == 0 and calls["vanilla_wgrad"] == levels
        for a, b in zip(only_bg, g_bg_all):
            assert same(a, b)
        if K:   # poses alone in front of a frozen backdrop: no weight-gradient kernel at all (as the pose-only case without a backdrop)
            for p in bg.model.parameters():
                p.requires_grad_(False)
            calls.update({k: 0 for k in calls})
            posed = _pose_objects(dev, specs, code_grads=False)
            lv = scene.render_scene_background_grad(model, posed, rays, True, bg)
            g_pose = torch.autograd.grad(_scene_loss(lv, target), [ob.pose_tensor for ob in posed])
            assert calls["art_wgrad"] == 0 and [calls[k] for k in BACKDROP_STAGES] == [0, 0, 0]
            for a, b in zip(g_pose, grads[3 * K + 64 * levels:]):
                assert same(a, b)
    finally:
        for p, f in zip(model.parameters(), m_flags):
            p.requires_grad_(f)
        for p, f in zip(bg.model.parameters(), flags):
            p.requires_grad_(f)


def test_a_second_backward_raises(dev):
    from aon_amd import scene

    model, bg = hl.art_model(dev, 2, 16, 16), _fresh_backdrop(dev, 2)
    rays = hl.to_dev(hl.small_frame(), dev)
    objects = _pose_objects(dev, hl.THREE(), pose_grads=False)
    loss = scene.render_scene_background_grad(model, objects, rays, True, bg)[1][0].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="released by its first backward"):
        loss.backward()
    model.zero_grad(set_to_none=True)
    bg.model.zero_grad(set_to_none=True)


def test_mlp_fwd_train_out(dev):
    """ops.mlp_fwd_train(out=...) writes the same raw as the call without it, into the given rows only"""
    from aon_amd import ops

    bg = hl.backdrop(dev, 1)
    rays = hl.to_dev(hl.frame_rays(9), dev)
    t, _ = ops.sample_along_rays(rays["rays_o"], rays["rays_d"], 16, 2.0, 6.0, want_coords=False)
    packed = bg.model.coarse_mlp.packed(True)
    raw, planes, masks = ops.mlp_fwd_train(packed, rays["rays_o"], rays["rays_d"], rays["viewdirs"], t)
    buf = torch.full((12, 17, 4), -7.0, device=dev)
    raw2, planes2, masks2 = ops.mlp_fwd_train(packed, rays["rays_o"], rays["rays_d"], rays["viewdirs"], t, out=buf[3:])
    assert raw2.data_ptr() == buf[3:].data_ptr() and same(raw, buf[3:]) and bool((buf[:3] == -7.0).all())
    assert planes2.shape == planes.shape and masks2.shape == masks.shape      # (their pad rows are never written: no bit comparison)
    with pytest.raises(ValueError, match="out must be a contiguous float32"):
        ops.mlp_fwd_train(packed, rays["rays_o"], rays["rays_d"], rays["viewdirs"], t, out=buf[:5])


# ------------------------------------------------------------------ the harness
FIT = hsg.FIT


def _fit_fixture(dev, bias_shift=None):
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False, white_bkgd=True,
                              model_kwargs=dict(num_levels=1, num_coarse_samples=32, **FIT["degrees"])).to(dev)
    sd = syn.make_art_state_dict(seed=FIT["seed"], density_scale=FIT["density_scale"], **FIT["degrees"])
    sd["coarse_mlp.density_layer.bias"] = sd["coarse_mlp.density_layer.bias"] - (FIT["bias_shift"] if bias_shift is None else bias_shift)
    lit.model.load_state_dict(sd)
    lit.code_library.load_state_dict(syn.make_code_library_state(seed=0, n_max_objs=2))
    rays = hl.to_dev(syn.make_rays(FIT["H"], FIT["W"], hl.CAM, syn.focal_from_fovy(FIT["H"], 30.0)), dev)
    return lit, sd, rays, _fresh_backdrop(dev, 1)


def test_fit_scene_codes_with_a_background(dev):
    """tests/test_hip_scene_grad.test_fit_scene_codes' setting (K = 2, one 8 x 12 view, one level of 33 samples, 20 Adam steps at lr 5e-3 from
    articulation codes moved by 0.3 x N(0, 1)) in front of the frozen backdrop of tests/test_hip_scene_lists.py.  The first loss against the
    fp64 restatement around the oracle's two networks, bar max(5 |loss32 - loss64|, 2e-6 |loss64|); the loss falls; both networks come
    back untouched."""
    from aon_amd import ops

    lit, sd, rays, bg = _fit_fixture(dev)
    table = lit.code_library.get_interpolated_articulations(max_interpolations=2, device=dev)
    poses = [(hsg.hs.pose(1, (0.35, 0.0, 0.0)), 1.6), (hsg.hs.pose(2, (-0.45, 0.1, 0.1)), 1.4)]
    true_art = [table[4].detach().clone(), table[11].detach().clone()]
    target = lit.render_scene(rays, [(j, true_art[j], *poses[j]) for j in range(2)], background=bg)["rgb"].clone()
    gen = torch.Generator().manual_seed(5)
    start = [(j, true_art[j] + FIT["amp"] * torch.randn(32, generator=gen).to(dev), *poses[j]) for j in range(2)]
    nets = list(lit.model.parameters()) + list(bg.model.parameters())
    next(bg.model.coarse_mlp.parameters()).requires_grad_(False)    # a flag the fit must hand back as it found it
    flags = [p.requires_grad for p in nets]
    before = [p.detach().clone() for p in nets]
    codes, losses = lit.fit_scene_codes([{**rays, "target": target}], start, FIT["steps"], lr=FIT["lr"], background=bg)
    assert [p.requires_grad for p in nets] == flags and all(torch.equal(a, p.detach()) for a, p in zip(before, nets))
    assert all(p.grad is None for p in nets)
    assert losses.shape == (FIT["steps"],) and bool(torch.isfinite(losses).all())
    print("fit_scene_codes(background) losses", [f"{x:.4e}" for x in losses.tolist()])
    assert losses[-1].item() < losses[0].item()
    assert all(not torch.equal(codes[j]["articulation"].reshape(-1), start[j][1]) for j in range(2))
    obj_pairs, pairs = hl.bg_pairs(ops, rays, poses, bg.near, bg.far)
    t, _ = ops.sample_along_rays(pairs.rays_o, pairs.rays_d, 32, pairs.near, pairs.far, want_coords=False)
    pr = {"o": pairs.rays_o.cpu().numpy(), "d": pairs.rays_d.cpu().numpy(), "v": pairs.viewdirs.cpu().numpy(), "offsets": np.asarray(pairs.starts),
          "slot": pairs.slot.cpu().numpy()}
    lib = lit.code_library
    bg_sd = hl.bg_state_dict()

    def first_loss(dtype):
        lat = [{"density": lib.embedding_instance_shape.weight[j: j + 1].detach().cpu().to(dtype),
                "color": lib.embedding_instance_appearance.weight[j: j + 1].detach().cpu().to(dtype), "articulation": start[j][1].cpu().reshape(1, 32).to(dtype)}
               for j in range(2)]
        out = lgref.scene_level_oracle({k: v.to(dtype) for k, v in sd.items()}, "coarse_mlp.", {k: v.to(dtype) for k, v in bg_sd.items()}, "coarse_mlp.", pr,
                                       t.cpu().numpy(), lat, rays["rays_d"].cpu().numpy(), True, dtype, (0, 3, 2))
        reg = 1e-4 * sum(torch.mean(torch.norm(v, dim=0)) for c in lat for v in c.values())
        return float(torch.mean((out["rgb"] - target.cpu().to(dtype)) ** 2) + reg)

    loss64, loss32 = first_loss(torch.float64), first_loss(torch.float32)
    bar = max(5.0 * abs(loss32 - loss64), 2e-6 * abs(loss64))
    print(f"first loss: hip {losses[0].item():.7e} fp64 {loss64:.7e} fp32 {loss32:.7e} bar {bar:.1e}")
    assert abs(losses[0].item() - loss64) <= bar


def test_fit_scene_poses_with_a_background(dev, monkeypatch):
    """tests/test_hip_scene_pose.py's pose fit (its field, boxes and perturbations of about 2 degrees / 0.05) in front of the frozen backdrop,
    100 steps: both errors of both objects fall, and with fit_codes off no weight-gradient kernel of either network runs"""
    from aon_amd import ops
    from test_hip_scene_pose import FIT as PFIT, pose_errors

    lit, sd, rays, bg = _fit_fixture(dev, bias_shift=PFIT["bias_shift"])
    true = [hsg.hs.pose(1, (0.35, 0.0, 0.0)), hsg.hs.pose(2, (-0.45, 0.1, 0.1))]
    start = [ops.apply_pose_correction(p.double(), torch.tensor(c, dtype=torch.float64)).float() for p, c in zip(true, PFIT["corrections"])]
    arts = (4, 11)
    target = lit.render_scene(rays, [(j, arts[j], true[j], PFIT["boxes"][j]) for j in range(2)], background=bg)["rgb"].clone()
    placements = [(j, arts[j], start[j], PFIT["boxes"][j]) for j in range(2)]
    calls = _count(monkeypatch, ops, BACKDROP_STAGES + ("art_wgrad",))
    poses, codes, losses = lit.fit_scene_poses([{**rays, "target": target}], placements, 100, PFIT["lr"], background=bg)
    assert all(v == 0 for v in calls.values()), calls
    assert bool(torch.isfinite(losses).all()) and losses[-1].item() < losses[0].item()
    e0 = [pose_errors(s, t) for s, t in zip(start, true)]
    e1 = [pose_errors(p, t) for p, t in zip(poses, true)]
    print(f"fit_scene_poses(background): (degrees, distance) {e0} -> {e1}; loss {losses[0].item():.4e} -> {losses[-1].item():.4e}")
    for a, b in zip(e0, e1):
        assert b[0] < a[0] and b[1] < a[1], (e0, e1)
    assert all(p.grad is None for p in list(lit.model.parameters()) + list(bg.model.parameters()))
