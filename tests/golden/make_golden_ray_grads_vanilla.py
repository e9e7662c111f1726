"""Generate tests/golden/g28_ray_grads_vanilla.npz by importing the REAL reference (as make_golden_ray_grads.py: stubs for the packages that
never touch the arithmetic, only DATA written; weights, rays and draws are rebuilt from aon_amd.synthetic by seed).

    python tests/golden/make_golden_ray_grads_vanilla.py

NeRF.forward (model.py:147-199) on 48 rays, two levels, default sizes, white background, randomized sampling with recorded draws and the
seeded weights (syn.make_nerf_state_dict, seed 2, density scale 10), every parameter frozen.  The reference's own autograd gives dL/d rays_o, dL/d rays_d, dL/d viewdirs (three separate leaf tensors) in fp32 and, the same call under a float64 default, in fp64:

  draw `a`: loss = mse(coarse) + mse(fine)
  draw `b`: ... + sum over the levels of 0.3 mean(acc) + 0.1 mean(depth^2)      (gradients into acc and depth)

Per draw and tensor: `<draw>.<name>|truth` (fp64), `|ref32` (fp32), `|norm` = ||truth||, `|ref32_dist` = ||ref32 - truth|| -- the keys
tests/_gradcheck.assert_as_close_as_fp32_fixture reads.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs, torch.rand patch, save)
from make_golden_full import cast, default_dtype  # noqa: E402

N, SEED_RAYS, SEED_TARGET, SEED_T, SEED_U = 48, 2801, 2802, 2803, 2804
NAMES = ("rays_o", "rays_d", "viewdirs")


def main():
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    os.chdir(mg.REF)
    from models.vanilla_nerf.model import NeRF

    import aon_amd.synthetic as syn

    torch.manual_seed(0)
    torch.set_num_threads(8)
    sd = syn.make_nerf_state_dict(seed=2, density_scale=10.0)
    rays = syn.random_rays(N, seed=SEED_RAYS)
    target = syn.seeded_uniform(SEED_TARGET, N, 3)
    t_rand, u = syn.seeded_uniform(SEED_T, N, 65), syn.seeded_uniform(SEED_U, N, 128)
    arrs = dict(n=N, seed_rays=SEED_RAYS, seed_target=SEED_TARGET, seed_t=SEED_T, seed_u=SEED_U, model_seed=2, density_scale=10.0,
                near=2.0, far=6.0)

    def grads(dtype, acc_depth):
        with default_dtype(dtype):
            model = NeRF().to(dtype)
            model.load_state_dict(cast(sd, dtype), strict=True)
            model.requires_grad_(False)
            leaves = {k: rays[k].to(dtype).clone().requires_grad_(True) for k in NAMES}
            with mg.patched_rand([t_rand.to(dtype), u.to(dtype)]):
                out = model(leaves, True, True, 2.0, 6.0)
            tg = target.to(dtype)
            loss = torch.mean((out[0][0] - tg) ** 2) + torch.mean((out[1][0] - tg) ** 2)
            if acc_depth:
                loss = loss + sum(0.3 * torch.mean(o[1]) + 0.1 * torch.mean(o[2] ** 2) for o in out)
            g = torch.autograd.grad(loss, [leaves[k] for k in NAMES])
        return {k: v.detach() for k, v in zip(NAMES, g)}, loss.item()

    for draw, acc_depth in (("a", False), ("b", True)):
        g32, l32 = grads(torch.float32, acc_depth)
        g64, l64 = grads(torch.float64, acc_depth)
        arrs[f"{draw}.loss32"], arrs[f"{draw}.loss64"] = l32, l64
        for k in NAMES:
            truth = g64[k]
            arrs[f"{draw}.{k}|truth"] = truth
            arrs[f"{draw}.{k}|ref32"] = g32[k]
            arrs[f"{draw}.{k}|norm"] = truth.norm().item()
            arrs[f"{draw}.{k}|ref32_dist"] = (g32[k].double() - truth).norm().item()
            rel = arrs[f"{draw}.{k}|ref32_dist"] / arrs[f"{draw}.{k}|norm"]
            print(f"draw {draw} {k}: |g| {arrs[f'{draw}.{k}|norm']:.3e}, reference fp32 against its fp64: {rel:.2e}")
            assert truth.abs().max() > 0 and torch.isfinite(truth).all()
    mg.save("g28_ray_grads_vanilla", **arrs)


if __name__ == "__main__":
    main()
