"""GPU: the batched SSIM kernel (csrc/aon_metrics.hip) against the fp64 yardstick (tests/_ssim_ref.py) for every image, its determinism (a
mixed-size batch gives the bits of one call per image, and the same bits twice), and the harness's SSIM (LitModel.ssim, test_epoch_end)."""
import json

import pytest
import torch

from _ssim_ref import ssim_ref, ssim_ref_each, white_background_pair

pytestmark = pytest.mark.gpu

SIZES = [(11, 11), (24, 32), (37, 53), (240, 320), (480, 640)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _random_pair(h, w, seed, outside=False):
    gen = torch.Generator().manual_seed(seed)
    if outside:   # pixels outside [0,1] on both sides: the kernel clips on load
        return 0.5 + 0.8 * torch.randn(h, w, 3, generator=gen), 0.5 + 0.8 * torch.randn(h, w, 3, generator=gen)
    x = torch.rand(h, w, 3, generator=gen)
    return x, (x + 0.3 * torch.rand(h, w, 3, generator=gen)).clamp(0, 1)   # correlated, so SSIM is not near 0


def _render_pair(dev, h, w):
    """A white-background synthetic render and a render of the same scene from a camera 2 degrees away, (h, w, 3) each.  The density
    bias is lowered by 8 so that the field is empty along ~40 % of the rays: they composite to exactly 1 (white_bkgd)."""
    import aon_amd.synthetic as syn
    from aon_amd.models.vanilla_nerf.model import NeRF

    sd = syn.make_nerf_state_dict(seed=0, density_scale=30.0)
    for lvl in ("coarse_mlp", "fine_mlp"):
        sd[f"{lvl}.density_layer.bias"] = sd[f"{lvl}.density_layer.bias"] - 8.0
    model = NeRF().to(dev)
    model.load_state_dict(sd)
    imgs = []
    for azim in (30.0, 32.0):
        rays = {k: v.to(dev) for k, v in syn.make_rays(h, w, syn.look_at_pose(azim_deg=azim), syn.focal_from_fovy(h)).items()}
        with torch.no_grad():
            rgb = torch.cat([model({k: v[i: i + 8192] for k, v in rays.items()}, False, True, syn.NEAR, syn.FAR)[1][0]
                             for i in range(0, h * w, 8192)])
        imgs.append(rgb.reshape(h, w, 3))
    return imgs


def _check(dev, preds, gts):
    from aon_amd import ops

    got = ops.ssim([p.to(dev) for p in preds], [g.to(dev) for g in gts])
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (len(preds),)
    want = ssim_ref_each(preds, gts)
    err = (got.double().cpu() - want).abs()
    assert err.max().item() < 1e-6, f"max |HIP - fp64| = {err.max().item():.3e}: got {got.tolist()}, want {want.tolist()}"
    return got


@pytest.mark.parametrize("h,w", SIZES)
def test_ssim_random_matches_fp64(dev, h, w):
    pairs = [_random_pair(h, w, seed) for seed in range(2)] + [_random_pair(h, w, 7, outside=True)]
    _check(dev, [p for p, _ in pairs], [g for _, g in pairs])


@pytest.mark.parametrize("h,w", [(240, 320), (480, 640)])
def test_ssim_white_background_matches_fp64(dev, h, w):
    p, g = white_background_pair(h, w, seed=1)
    got = _check(dev, [p, g], [g, g])
    assert got[1].item() == 1.0


def test_ssim_synthetic_render_matches_fp64(dev):
    pred, gt = _render_pair(dev, 120, 160)
    white = (gt == 1).all(-1).float().mean().item()
    assert 0.1 < white < 0.9, f"expected a white background and an object, {white:.0%} of the pixels are white"
    _check(dev, [pred.cpu(), gt.cpu()], [gt.cpu(), pred.cpu()])


def test_ssim_flat_hwc_with_sizes(dev):
    from aon_amd import ops

    p, g = _random_pair(24, 32, 3)
    a = ops.ssim([p.to(dev)], [g.to(dev)])
    b = ops.ssim([p.reshape(-1, 3).to(dev)], [g.reshape(-1, 3).to(dev)], image_sizes=[(24, 32)])
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.ssim([p.reshape(-1, 3).to(dev)], [g.reshape(-1, 3).to(dev)])
    with pytest.raises(Exception, match="11 <= h, w"):
        ops.ssim([p[:10].contiguous().to(dev)], [g[:10].contiguous().to(dev)])
    assert ops.ssim([], []).shape == (0,)


def test_ssim_batch_is_bit_equal_to_single_calls(dev):
    """40 images of mixed sizes (more than one launch pair's 32-entry table) in one call == one call per image == a second run."""
    from aon_amd import ops

    sizes = [SIZES[i % len(SIZES)] for i in range(40)]
    sizes[5] = (17, 200)
    pairs = [_random_pair(h, w, 100 + i, outside=(i % 3 == 0)) for i, (h, w) in enumerate(sizes)]
    preds, gts = [p.to(dev) for p, _ in pairs], [g.to(dev) for _, g in pairs]
    batch = ops.ssim(preds, gts)
    again = ops.ssim(preds, gts)
    single = torch.cat([ops.ssim([p], [g]) for p, g in zip(preds, gts)])
    assert torch.equal(batch, again) and torch.equal(batch, single)
    for i in (0, 5, 33, 39):
        assert abs(batch[i].item() - ssim_ref(pairs[i][0], pairs[i][1]).item()) < 1e-6


def test_litmodel_ssim_dict(dev):
    from aon_amd.models.interface import LitModel

    pairs = [_random_pair(h, w, 50 + i) for i, (h, w) in enumerate(SIZES[:3])]
    preds, gts = [p.to(dev) for p, _ in pairs], [g.to(dev) for _, g in pairs]
    lit = LitModel()
    each = lit.ssim_each(preds, gts)
    assert each.shape == (3,)
    ret = lit.ssim(preds, gts, None, None, None)
    m = ssim_ref_each([p for p, _ in pairs], [g for _, g in pairs]).mean().item()
    assert set(ret) == {"name", "mean", "test"} and ret["name"] == "SSIM"
    assert ret["mean"] == ret["test"] == each.mean().item()
    assert abs(ret["mean"] - m) < 1e-6


def test_epoch_end_writes_ssim(dev, tmp_path):
    from aon_amd.models.vanilla_nerf.model import LitNeRF

    H, W = 24, 32
    pred, gt = _render_pair(dev, H, W)
    mask = (gt.reshape(-1, 3) < 1).any(-1)
    outs = [{"rgb": pred.reshape(-1, 3), "target": gt.reshape(-1, 3), "instance_mask": mask}]
    lit = LitNeRF({"chunk": 500, "img_wh": (W, H)}).to(dev)
    ret = lit.test_epoch_end(outs, [(H, W)], out_dir=str(tmp_path / "render"))
    assert len(ret) == 2 and ret[0]["name"] == "PSNR" and ret[1]["name"] == "PSNR_obj"
    with open(tmp_path / "render" / "results.json") as f:
        res = json.load(f)
    assert set(res) == {"PSNR", "SSIM", "PSNR_obj"}
    assert res["SSIM"]["test"] == res["SSIM"]["mean"] == lit.logged["test/ssim"][-1]
    assert abs(res["SSIM"]["test"] - ssim_ref(pred, gt).item()) < 1e-6
