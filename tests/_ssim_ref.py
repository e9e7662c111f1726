"""The fp64 yardstick of the SSIM kernel: piqa's SSIM() with its defaults (the reference's LitModel.ssim_each, models/interface.py:102-111),
restated with torch.conv2d.  11-tap Gaussian window with sigma 1.5, "valid" filtering, c1 = 0.01^2, c2 = 0.03^2 (value range 1), inputs clipped
to [0,1], uncentred statistics (sigma_xx = G(x^2) - mu_x^2, sigma_xy = G(xy) - mu_x mu_y), the mean of the map over pixels and channels."""
import torch
import torch.nn.functional as F

WIN, SIGMA, C1, C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2


def gaussian_window(dtype=torch.float64) -> torch.Tensor:
    x = torch.arange(WIN, dtype=dtype) - (WIN - 1) // 2
    g = torch.exp(-(x ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def ssim_ref(pred: torch.Tensor, gt: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """SSIM of one (h, w, 3) pair, computed on the CPU in `dtype` (float64: the yardstick; float32: what an fp32 implementation would see)."""
    x = torch.clip(pred.detach().cpu().to(dtype), 0, 1).permute(2, 0, 1)[None]
    y = torch.clip(gt.detach().cpu().to(dtype), 0, 1).permute(2, 0, 1)[None]
    g = gaussian_window(dtype)
    kh, kv = g.view(1, 1, 1, WIN).repeat(3, 1, 1, 1), g.view(1, 1, WIN, 1).repeat(3, 1, 1, 1)

    def G(t):   # separable window, no padding, per channel
        return F.conv2d(F.conv2d(t, kh, groups=3), kv, groups=3)

    mu_x, mu_y = G(x), G(y)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    sigma_xx, sigma_yy, sigma_xy = G(x ** 2) - mu_xx, G(y ** 2) - mu_yy, G(x * y) - mu_xy
    cs = (2 * sigma_xy + C2) / (sigma_xx + sigma_yy + C2)
    ss = (2 * mu_xy + C1) / (mu_xx + mu_yy + C1) * cs
    return ss.mean()


def ssim_ref_each(preds, gts, dtype=torch.float64) -> torch.Tensor:
    return torch.stack([ssim_ref(p, g, dtype) for p, g in zip(preds, gts)])


def white_background_pair(h: int = 480, w: int = 640, seed: int = 0):
    """A (prediction, target) pair in the shape of a NeRF test render: white background, a textured object in the middle, the prediction a
    slightly perturbed copy (renders leave residues just below 1 on the background).  fp32, (h, w, 3), CPU."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    inside = ((xx / 0.45) ** 2 + (yy / 0.55) ** 2 < 1).float()[..., None]
    tex = 0.5 + 0.3 * torch.sin(12 * xx + 7 * yy)[..., None] * torch.tensor([1.0, 0.6, 0.3]) + 0.05 * torch.rand(h, w, 3, generator=gen)
    gt = inside * tex + (1 - inside)
    pred = gt + 0.02 * inside * (torch.rand(h, w, 3, generator=gen) - 0.5) - 0.003 * (1 - inside) * torch.rand(h, w, 3, generator=gen)
    return pred.float().contiguous(), gt.float().contiguous()
