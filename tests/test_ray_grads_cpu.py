"""Ray gradients / fit_pose, what can be checked without a GPU: the differentiable ray construction
(ops.rays_from_pose) against get_rays' definition and against finite differences, the oracle's own ray gradients against the reference's
(G27), the C ABI of the new entry points and their host-side refusals, and fit_pose's argument rules."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rays_o", "rays_d", "viewdirs")
AON_E_INVALID = -1   # include/aon_hip.h


def _directions(H, W, focal, dtype=torch.float32):
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    return torch.stack([(i - W / 2) / focal, -(j - H / 2) / focal, -torch.ones_like(i)], -1)


def test_rays_from_pose_at_zero_correction_equals_get_rays():
    """datasets/ray_utils.py:118-159 as aon_amd.synthetic.make_rays restates it on the CPU: 2e-7, the bar the directions are held to."""
    import aon_amd.synthetic as syn
    from aon_amd import ops

    H, W = 15, 20
    focal = syn.focal_from_fovy(H)
    for azim, elev in ((30.0, 30.0), (200.0, -15.0)):
        c2w = syn.look_at_pose(4.0, azim, elev)
        want = syn.make_rays(H, W, c2w, focal)
        for corr in (None, torch.zeros(6)):
            o, d = ops.rays_from_pose(_directions(H, W, focal), c2w, corr)
            assert o.shape == d.shape == (H * W, 3)
            assert (o - want["rays_o"]).abs().max().item() == 0.0
            assert (d - want["rays_d"]).abs().max().item() <= 2e-7
    assert torch.equal(ops.so3_exp(torch.zeros(3)), torch.eye(3))


def _taylor_exp(K, terms=30):
    """exp(K) by its power series (|K| < 1: thirty terms are exact to the last bit of fp64)."""
    out, term = torch.eye(3, dtype=K.dtype), torch.eye(3, dtype=K.dtype)
    for k in range(1, terms):
        term = term @ K / k
        out = out + term
    return out


def test_pose_correction_is_a_rigid_motion():
    from aon_amd import ops
    import aon_amd.synthetic as syn

    c2w = syn.look_at_pose(4.0, 40.0, 25.0).double()
    corr = torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4, 0.25], dtype=torch.float64)
    R = ops.so3_exp(corr[:3])
    assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-14 and abs(torch.linalg.det(R).item() - 1.0) < 1e-14
    assert (R - _taylor_exp(torch.tensor([[0, -0.5, -0.2], [0.5, 0, -0.3], [0.2, 0.3, 0]], dtype=torch.float64))).abs().max().item() < 1e-15
    pose = ops.apply_pose_correction(c2w, corr)
    assert torch.allclose(pose[:, :3], R @ c2w[:, :3], atol=1e-15) and torch.allclose(pose[:, 3], c2w[:, 3] + corr[3:], atol=0)
    # both sides of the switch to the series (|omega|^2 = 1e-4) agree with the matrix exponential: a few ulp of entries below one
    for scale in (0.0, 1e-9, 0.0099, 0.0101):
        w = scale * torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
        K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        assert (ops.so3_exp(w) - _taylor_exp(K)).abs().max().item() < 1e-15


@pytest.mark.parametrize("corr", [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.004, -0.003, 0.002, 0.05, 0.0, -0.02), (0.3, -0.2, 0.5, 0.1, -0.4, 0.25)])
def test_rays_from_pose_autograd_against_finite_differences(corr):
    from aon_amd import ops
    import aon_amd.synthetic as syn

    d = _directions(3, 4, 5.0, torch.float64)
    c2w = syn.look_at_pose(4.0, 40.0, 25.0).double().requires_grad_(True)
    c = torch.tensor(corr, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda pose, cc: ops.rays_from_pose(d, pose, cc), (c2w, c), eps=1e-6, atol=1e-8, rtol=1e-6)


def _fixture_case(g):
    import aon_amd.synthetic as syn

    n = int(g["n"])
    rays = syn.random_rays(n, seed=int(g["seed_rays"]))
    target = syn.seeded_uniform(int(g["seed_target"]), n, 3)
    t_rand, u = syn.seeded_uniform(int(g["seed_t"]), n, 65), syn.seeded_uniform(int(g["seed_u"]), n, 128)
    lib = syn.make_code_library_state(seed=0, n_max_objs=2)
    i, a = int(g["instance_id"]), int(g["articulation_id"])
    lat = {"density": lib["embedding_instance_shape.weight"][i: i + 1], "color": lib["embedding_instance_appearance.weight"][i: i + 1],
           "articulation": lib["embedding_instance_articulation.weight"][a: a + 1]}
    sd = syn.make_art_state_dict(seed=int(g["model_seed"]), density_scale=float(g["density_scale"]))
    return rays, target, t_rand, u, lat, sd


def _oracle_grads(g, dtype, acc_depth):
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as orc

    rays, target, t_rand, u, lat, sd = _fixture_case(g)
    leaves = {k: rays[k].to(dtype).clone().requires_grad_(True) for k in NAMES}
    out = orc.nerf_ae_art_forward({k: v.to(dtype) for k, v in sd.items()}, leaves, True, True, 2.0, 6.0, {k: v.to(dtype) for k, v in lat.items()},
                                  t_rand=t_rand.to(dtype), u=u.to(dtype))
    tg = target.to(dtype)
    loss = torch.mean((out[0][0] - tg) ** 2) + torch.mean((out[1][0] - tg) ** 2)
    if acc_depth:
        loss = loss + sum(0.3 * torch.mean(o[1]) + 0.1 * torch.mean(o[2] ** 2) for o in out)
    return dict(zip(NAMES, torch.autograd.grad(loss, [leaves[k] for k in NAMES]))), loss.item()


@pytest.mark.parametrize("draw,acc_depth", [("a", False), ("b", True)])
def test_oracle_ray_gradients_against_the_reference(golden, draw, acc_depth):
    """The oracle differentiates with respect to the rays as it stands (t: coarse from near / far, fine detached).  Both of its evaluations
    are held to the project's gradient yardstick against G27 (tests/_gradcheck.py: as close to the reference's fp64 as the reference's own
    fp32 is, factor 5, floor 1e-4) -- the fp64 one too: it is a second fp64 evaluation whose constants are the fp32 graph's (pi / 2 rounded
    to fp32, helper.py:139) where the reference under a float64 default re-derives them, and on this sharp field the two fp64 gradients
    sit up to 6e-4 apart (printed), two orders inside the reference's fp32 distance of 1e-2."""
    sys.path.insert(0, os.path.dirname(__file__))
    from _gradcheck import assert_as_close_as_fp32_fixture

    g = golden("g27_ray_grads")
    sub = {k[len(draw) + 1:]: v for k, v in g.items() if k.startswith(draw + ".") and "|" in k and not k.endswith("|ref32")}
    g64, l64 = _oracle_grads(g, torch.float64, acc_depth)
    assert abs(l64 - float(g[f"{draw}.loss64"])) <= 1e-7 * abs(l64)
    assert_as_close_as_fp32_fixture(g64, sub, f"oracle fp64 ray gradients, draw {draw}", factor=5.0, floor=1e-4)
    g32, _ = _oracle_grads(g, torch.float32, acc_depth)
    assert_as_close_as_fp32_fixture(g32, sub, f"oracle fp32 ray gradients, draw {draw}", factor=5.0, floor=1e-4)


def test_abi_of_the_new_entry_points():
    from aon_amd import _lib

    text = open(os.path.join(ROOT, "include", "aon_hip.h")).read()
    for name in ("aon_art_render_bwd_inputs", "aon_train_scratch_bytes_inputs"):
        assert name + "(" in text and name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    assert "typedef struct aon_ray_grads" in text
    lat, inp = _lib._SIGS["aon_art_render_bwd_latents"][1], _lib._SIGS["aon_art_render_bwd_inputs"][1]
    assert list(inp) == list(lat) + [C.c_void_p] and _lib._SIGS["aon_art_render_bwd_inputs"][0] is C.c_int
    assert _lib._SIGS["aon_train_scratch_bytes_inputs"] == (C.c_int64, [C.c_int64, C.c_int, C.c_void_p])
    assert [f[0] for f in _lib.RayGradsC._fields_] == ["rays_o", "viewdirs", "g_rays_o", "g_rays_d", "g_viewdirs"]
    assert C.sizeof(_lib.RayGradsC) == 5 * C.sizeof(C.c_void_p)
    assert _lib.lib.aon_abi_version() == 5


def test_scratch_size_and_refusals_without_gpu():
    from aon_amd import _lib

    lib = _lib.lib
    for n, S in ((1, (65, 193)), (37, (65, 193)), (4096, (65, 193))):
        for levels in (1, 2):
            lat, inp = lib.aon_train_scratch_bytes_latents(n, levels, None), lib.aon_train_scratch_bytes_inputs(n, levels, None)
            rec = sum(-(-(-(-n * s // 128) * 128 * 128) // 256) * 256 for s in S[:levels])   # 128 B per padded sample, 256-byte carves
            assert inp == lat + rec, (n, levels, lat, inp, rec)
    nul = [None] * 5
    call = lambda n, levels, rg: lib.aon_art_render_bwd_inputs(None, None, None, None, None, n, 1, levels, None, None, None, None, None, None, None, None,   # noqa: E731
                                                               None, 0, None, 0, None, None, rg)
    # rg == NULL: the latents call, its messages
    assert call(16, 2, None) != 0 and lib.aon_last_error().startswith(b"aon_art_render_bwd_latents")
    rg = _lib.RayGradsC(*nul)
    assert call(0, 2, C.byref(rg)) != 0 and lib.aon_last_error().startswith(b"aon_art_render_bwd_inputs")
    assert call(16, 3, C.byref(rg)) != 0 and lib.aon_last_error().startswith(b"aon_art_render_bwd_inputs")
    # a null member is named before anything else is looked at
    for missing in range(5):
        vals = [C.c_void_p(4096)] * 5
        vals[missing] = None
        rc = call(16, 2, C.byref(_lib.RayGradsC(*vals)))
        assert rc == AON_E_INVALID and lib.aon_last_error() == b"aon_art_render_bwd_inputs: null member of aon_ray_grads", lib.aon_last_error()
    rc = call(16, 2, C.byref(_lib.RayGradsC(*[C.c_void_p(4096)] * 5)))
    assert rc == AON_E_INVALID and lib.aon_last_error() == b"aon_art_render_bwd_inputs: null pointer"


def test_fit_pose_rejects_bad_arguments():
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model_autodecoder import LitNeRF_AutoDecoder

    lit = LitNeRF_AutoDecoder(hparams={"N_max_objs": 2}, randomized=False)
    batch = {"directions": torch.zeros(4, 3), "target": torch.zeros(4, 3)}
    pose = syn.look_at_pose()
    for steps in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            lit.fit_pose([batch], steps, poses=[pose])
    with pytest.raises(ValueError, match="no batches"):
        lit.fit_pose([], 3, poses=[])
    with pytest.raises(ValueError, match="one .3, 4. pose per view"):
        lit.fit_pose([batch], 3, poses=[pose, pose])
    with pytest.raises(ValueError, match="lr"):
        lit.fit_pose([batch], 3, lr=0.0, poses=[pose])
    with pytest.raises(ValueError, match="lr"):
        lit.fit_pose([batch], 3, lr=(1e-3, 1e-3, 1e-3), poses=[pose])
    with pytest.raises(ValueError, match="fit_pose: lr must be positive"):      # a bool is not a rate (it used to run at rate 1.0)
        lit.fit_pose([batch], 3, lr=True, poses=[pose])
    with pytest.raises(ValueError, match="'directions'"):
        lit.fit_pose([{"rays_o": torch.zeros(4, 3), "target": torch.zeros(4, 3)}], 3, poses=[pose])
    with pytest.raises(ValueError, match=r"\(3, 4\) matrix"):
        lit.fit_pose([batch], 3, poses=[torch.eye(3)])
    with pytest.raises(ValueError, match="init"):
        lit.fit_pose([batch], 3, codes="median", poses=[pose])
    assert all(p.requires_grad for p in lit.model.parameters())
