"""Tensor-level wrappers over the C ABI: torch is used for device memory and streams only.

Every function takes/returns CUDA(HIP) fp32 tensors, allocates its outputs, and enqueues on torch's current
stream.  CPU tensors are rejected: there is no host fallback.
"""
from __future__ import annotations

import collections as _collections
import ctypes as C

import torch

from . import _lib
from ._lib import check, lib

ACT_NONE, ACT_VANILLA, ACT_ARTICULATED = 0, 1, 2


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


STREAM_CACHE_ENTRIES = 8      # (device, stream) entries one scratch cache keeps, least recently used dropped first (as _TRAIN_POOL_SIZES)
_STREAM_CACHES: list = []     # every module-level StreamCache: release_workspaces() clears them all


class StreamCache:
    """Scratch buffers of the whole-path calls, ONE per (device index, stream handle).  Plain Python, no torch and no library call
    (tests/test_stream_cache_cpu.py drives it with fake handles): `get(key, need, alloc)` returns the key's buffer when it holds `need`
    bytes (`.numel()`), else `alloc(need)`, which replaces that key's entry alone.

    Why per stream: a workspace is written and read by the kernels of ONE call, so two calls in flight on two streams of a device must
    never share one (keyed by the device alone, they overwrote each other's t / weights / sample records and -- occupancy and early-stop
    paths -- the int32 gather lists the MLP kernel indexes with).  Why no record_stream: `alloc` runs with the key's stream current and
    the buffer is only ever handed back to that stream, so torch's caching allocator owns the block for the stream that uses it; an entry
    dropped here (grown, evicted, release_workspaces()) is reused by that stream in order, or by another one only after the allocator has
    seen it idle."""

    def __init__(self, max_entries: int = STREAM_CACHE_ENTRIES, register: bool = True):
        self.max_entries = int(max_entries)
        self._entries: "_collections.OrderedDict" = _collections.OrderedDict()
        if register:
            _STREAM_CACHES.append(self)

    def get(self, key, need: int, alloc):
        buf = self._entries.get(key)
        if buf is None or buf.numel() < need:
            buf = self._entries[key] = alloc(need)
        self._entries.move_to_end(key)
        while len(self._entries) > self.max_entries:
            self._entries.popitem(last=False)
        return buf

    def clear(self) -> None:
        self._entries.clear()

    def values(self):
        return list(self._entries.values())

    def __len__(self) -> int:
        return len(self._entries)


def stream_key(device) -> tuple:
    """(device index, handle of torch's current stream on it): the key of every StreamCache."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"workspace requested on {dev}; the HIP path needs a cuda (ROCm) device and has no CPU fallback")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return idx, torch.cuda.current_stream(idx).cuda_stream


def _scratch(cache: StreamCache, device, need: int) -> torch.Tensor:
    """`need` bytes of `cache` for a call on `device`'s current stream."""
    # (torch's allocator takes the block for the current stream of `device`: the stream of the key)
    return cache.get(stream_key(device), need, lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=device))


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path needs a cuda (ROCm) tensor and has no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _tag(out: torch.Tensor) -> torch.Tensor:
    """A freshly packed stream / per-call block remembers the form it was packed in (bottleneck folded or literal) ON THE TENSOR: the
    launchers look the form up by address (csrc/aon_fold.hip), and `_pk` re-declares it from here on every call, so an address the caching
    allocator hands out again can never carry an earlier tenant's form."""
    out._aon_form = int(lib.aon_stream_form(out.data_ptr()))
    return out


def _pk(t: torch.Tensor | None) -> C.c_void_p:
    """Pointer of a packed weight stream / per-call block for a C call, with its form re-declared.  A tensor without a form is not one
    this binding packed (a clone or a moved copy of a packed buffer has none): refused here instead of being run under a guessed form."""
    if t is None:
        return None
    form = getattr(t, "_aon_form", None)
    if form is None:
        raise ValueError("not a packed stream of this binding (tensors returned by ops.pack_* / ops.art_prepare carry their form; a clone or "
                         "copy does not: use ops.clone_packed)")
    check(lib.aon_declare_stream_form(t.data_ptr(), form), "aon_declare_stream_form")
    return C.c_void_p(t.data_ptr())


def clone_packed(t: torch.Tensor) -> torch.Tensor:
    """A copy of a packed stream / per-call block that keeps its form (plain `.clone()` yields a buffer every call refuses)."""
    out = t.clone()
    out._aon_form = t._aon_form
    check(lib.aon_declare_stream_form(out.data_ptr(), out._aon_form), "aon_declare_stream_form")
    return out


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _c2w_host(c2w) -> "C.Array":
    c = torch.as_tensor(c2w, dtype=torch.float32).detach().cpu().reshape(-1)
    if c.numel() < 12:
        raise ValueError("c2w must hold at least (3,4) values")
    return (C.c_float * 12)(*c[:12].tolist())


# ------------------------------------------------------------------ R1/R2 ray generation
def raygen(c2w, H: int, W: int, focal: float, pix_begin: int = 0, pix_end: int | None = None, device=None):
    """Fused get_ray_directions + get_rays for row-major pixels [pix_begin, pix_end).
    Returns (rays_o, viewdirs) with shapes (n,3); the reference's rays_d is the same tensor as viewdirs."""
    pix_end = H * W if pix_end is None else pix_end
    n = pix_end - pix_begin
    dev = torch.device("cuda") if device is None else torch.device(device)
    rays_o = torch.empty((n, 3), dtype=torch.float32, device=dev)
    viewdirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_raygen(_c2w_host(c2w), H, W, float(focal), pix_begin, pix_end, _ptr(rays_o), _ptr(viewdirs), None,
                             _stream()), "aon_raygen")
    return rays_o, viewdirs


# ------------------------------------------------------------------ R13 training losses, two launches
def _loss_args(rgb_c, rgb_f, target, latents):
    rgb_f, target = _f32(rgb_f, "rgb_fine"), _f32(target, "target")
    rgb_c = None if rgb_c is None else _f32(rgb_c, "rgb_coarse")
    n = rgb_f.numel() // 3
    if target.numel() != 3 * n or (rgb_c is not None and rgb_c.numel() != 3 * n):
        raise ValueError("train_loss: rgb / target sizes differ")
    lats = [None, None, None]
    for k, t in enumerate(latents or ()):
        lats[k] = None if t is None else _f32(t, "latent")
    lens = (C.c_int * 3)(*[0 if t is None else t.numel() for t in lats])
    return rgb_c, rgb_f, target, n, lats, lens


def train_loss_fwd(rgb_c, rgb_f, target, latents=(), reg_scale: float = 1e-4):
    """-> (loss (1,), stats (8,) = {loss0, loss1, reg, loss, psnr0, psnr1, 0, 0}); `latents`: up to three one-row codes."""
    rgb_c, rgb_f, target, n, lats, lens = _loss_args(rgb_c, rgb_f, target, latents)
    stats = torch.empty(8, dtype=torch.float32, device=rgb_f.device)
    loss = torch.empty(1, dtype=torch.float32, device=rgb_f.device)
    with torch.cuda.device(rgb_f.device):
        check(lib.aon_train_loss_fwd(_ptr(rgb_c), _ptr(rgb_f), _ptr(target), n, _ptr_array(lats), lens, float(reg_scale), _ptr(stats), _ptr(loss), _stream()),
              "aon_train_loss_fwd")
    return loss, stats


def train_loss_bwd(rgb_c, rgb_f, target, latents, reg_scale: float, grad_loss):
    """-> (d_rgb_c or None, d_rgb_f, [d_latent or None] * 3)"""
    rgb_c, rgb_f, target, n, lats, lens = _loss_args(rgb_c, rgb_f, target, latents)
    go = _f32(grad_loss, "grad_loss")
    d_c = None if rgb_c is None else torch.empty_like(rgb_c)
    d_f = torch.empty_like(rgb_f)
    d_l = [None if t is None else torch.empty_like(t) for t in lats]
    with torch.cuda.device(rgb_f.device):
        check(lib.aon_train_loss_bwd(_ptr(rgb_c), _ptr(rgb_f), _ptr(target), n, _ptr_array(lats), lens, float(reg_scale), _ptr(go), _ptr(d_c), _ptr(d_f),
                                     _ptr_array(d_l), _stream()), "aon_train_loss_bwd")
    return d_c, d_f, d_l


def ray_directions(H: int, W: int, focal: float, device=None):
    dev = torch.device("cuda") if device is None else torch.device(device)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_ray_directions(H, W, float(focal), _ptr(out), _stream()), "aon_ray_directions")
    return out


def get_rays(directions: torch.Tensor, c2w):
    d = _f32(directions, "directions")
    n = d.numel() // 3
    rays_o = torch.empty((n, 3), dtype=torch.float32, device=d.device)
    viewdirs = torch.empty((n, 3), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.aon_get_rays(_ptr(d), _c2w_host(c2w), n, _ptr(rays_o), _ptr(viewdirs), None, _stream()), "aon_get_rays")
    return rays_o, viewdirs


def ray_radii(directions: torch.Tensor, c2w):
    """radii (H*W,) of get_rays(..., output_radii=True) (ray_utils.py:138-143) from (H,W,3) camera-space directions."""
    d = _f32(directions, "directions")
    if d.dim() != 3 or d.shape[-1] != 3 or d.shape[0] < 3:
        raise ValueError(f"output_radii needs directions of shape (H>=3, W, 3) like the reference (it differences image rows), got {tuple(d.shape)}")
    H, W = int(d.shape[0]), int(d.shape[1])
    radii = torch.empty((H * W,), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.aon_ray_radii(_ptr(d), _c2w_host(c2w), H, W, _ptr(radii), _stream()), "aon_ray_radii")
    return radii


# ------------------------------------------------------------------ R3 sampling
def cast_rays(t_vals, origins, directions):
    t, o, d = _f32(t_vals, "t_vals"), _f32(origins, "origins"), _f32(directions, "directions")
    n, S = t.shape
    coords = torch.empty((n, S, 3), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_cast_rays(_ptr(t), _ptr(o), _ptr(d), n, S, _ptr(coords), _stream()), "aon_cast_rays")
    return coords


# ------------------------------------------------------------------ per-ray near / far from a ray-box intersection
_LIMITS_WS = StreamCache()


def _box3(box):
    """A side length (the reference's cube, +-side / 2: helper.py:53-63) or (lo, hi), each a number or 3 numbers -> two float[3]."""
    if isinstance(box, (int, float)):
        half = box / 2                       # Python double, rounded to fp32 once: torch.tensor([bb_min, bb_max], dtype=float32)
        lo, hi = [-1 * half] * 3, [1 * half] * 3
    else:
        lo, hi = _vec3(box[0], "box lo"), _vec3(box[1], "box hi")
    return (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def ray_limits_box(rays_o, rays_d, box):
    """helper.get_ray_limits_box (helper.py:42-102) for `box` (a side length, or (lo, hi)) -> (near, far), each (N, 1): the entry / exit
    distances, (-1, -2) for the rays the reference marks invalid; its NaNs (origin on a face the ray is parallel to) included."""
    o, d = _f32(rays_o.detach(), "rays_o").reshape(-1, 3), _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n = o.shape[0]
    lo, hi = _box3(box)
    near, far = torch.empty((n, 1), dtype=torch.float32, device=o.device), torch.empty((n, 1), dtype=torch.float32, device=o.device)
    with torch.cuda.device(o.device):
        check(lib.aon_ray_limits_box(_ptr(o), _ptr(d), n, lo, hi, _ptr(near), _ptr(far), _stream()), "aon_ray_limits_box")
    return near, far


def ray_limits(rays_o, rays_d, box=2):
    """helper.get_ray_limits (helper.py:29-39) without its host round trip -> (near, far, live): near / far (N, 1) with the invalid rays
    patched by min(near) / max(far) of the valid ones and negatives clamped to 0; live (N,) uint8, 1 iff the ray was valid and far > near
    after the clamp (`ray_live=` of the inference renders).  The min / max belong to the ray set: one call per image, not per chunk."""
    o, d = _f32(rays_o.detach(), "rays_o").reshape(-1, 3), _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n, dev = o.shape[0], o.device
    lo, hi = _box3(box)
    near, far = torch.empty((n, 1), dtype=torch.float32, device=dev), torch.empty((n, 1), dtype=torch.float32, device=dev)
    live = torch.empty((n,), dtype=torch.uint8, device=dev)
    ws = _scratch(_LIMITS_WS, dev, int(lib.aon_ray_limits_workspace_bytes(n)))
    with torch.cuda.device(dev):
        check(lib.aon_ray_limits(_ptr(o), _ptr(d), n, lo, hi, _ptr(near), _ptr(far), _ptr(live), _ptr(ws), ws.numel(), _stream()), "aon_ray_limits")
    return near, far, live


def _ray_bounds(near, far, n: int, dev, ray_live=None):
    """near / far of a whole-path call: two numbers -> (near, far, None, ()); a tensor of N elements ((N,) or (N, 1)) for either, or a
    `ray_live` mask -> (placeholders, placeholders, aon_ray_bounds, tensors to keep alive).  The tensors are data: detached."""
    per_ray = isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor)
    if not per_ray and ray_live is None:
        return float(near), float(far), None, ()

    def vec(x, name):
        if not isinstance(x, torch.Tensor):
            return torch.full((n,), float(x), dtype=torch.float32, device=dev)
        t = _f32(x.detach(), name).reshape(-1)
        if t.numel() == 1 and n != 1:
            t = t.expand(n).contiguous()
        if t.numel() != n or t.device != dev:
            raise ValueError(f"{name}: a per-ray tensor must hold one value per ray ({n}) on {dev}, got shape {tuple(x.shape)} on {x.device}")
        return t

    nt, ft = vec(near, "near"), vec(far, "far")
    lv = None
    if ray_live is not None:
        if not isinstance(ray_live, torch.Tensor) or not ray_live.is_cuda or ray_live.dtype not in (torch.uint8, torch.bool):
            raise TypeError("ray_live: expected a uint8 / bool cuda tensor (ops.ray_limits)")
        lv = ray_live.reshape(-1).to(torch.uint8).contiguous()
        if lv.numel() != n or lv.device != dev:
            raise ValueError(f"ray_live must hold one byte per ray ({n}) on {dev}")
    st = _lib.RayBoundsC(nt.data_ptr(), ft.data_ptr(), None if lv is None else lv.data_ptr())
    return 1.0, 1.0, st, (nt, ft, lv)


def sample_along_rays(rays_o, rays_d, num_samples: int, near, far, t_rand=None, want_coords=True, lindisp=False):
    """``near`` / ``far``: numbers, or tensors of N elements (helper.py:106-133 takes the (N, 1) tensors of get_ray_limits by broadcasting)."""
    o, d = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d")
    n, S = o.shape[0], num_samples + 1
    near, far, bounds, keep = _ray_bounds(near, far, n, o.device)
    tr = None if t_rand is None else _f32(t_rand, "t_rand")
    if tr is not None and tuple(tr.shape) != (n, S):
        raise ValueError(f"t_rand must be ({n},{S}), got {tuple(tr.shape)}")
    t_vals = torch.empty((n, S), dtype=torch.float32, device=o.device)
    coords = torch.empty((n, S, 3), dtype=torch.float32, device=o.device) if want_coords else None
    with torch.cuda.device(o.device):
        if bounds is not None:
            check(lib.aon_sample_along_rays_bounds(_ptr(o), _ptr(d), n, S, _ptr(keep[0]), _ptr(keep[1]), int(bool(lindisp)), _ptr(tr), _ptr(t_vals),
                                                   _ptr(coords), _stream()), "aon_sample_along_rays_bounds")
        elif lindisp:   # helper.py:117 evaluates 1.0 / near in Python double precision; ctypes rounds it to fp32 once, as torch does
            check(lib.aon_sample_along_rays_ex(_ptr(o), _ptr(d), n, S, float(near), float(far), 1, 1.0 / near, 1.0 / far, _ptr(tr),
                                               _ptr(t_vals), _ptr(coords), _stream()), "aon_sample_along_rays_ex")
        else:
            check(lib.aon_sample_along_rays(_ptr(o), _ptr(d), n, S, float(near), float(far), _ptr(tr), _ptr(t_vals), _ptr(coords),
                                            _stream()), "aon_sample_along_rays")
    return t_vals, coords


# ------------------------------------------------------------------ R4 positional encoding (stage-level)
def pos_enc(x, min_deg: int, max_deg: int):
    xc = _f32(x, "x")
    if xc.shape[-1] != 3:
        raise ValueError("pos_enc expects (...,3)")
    n = xc.numel() // 3
    F = 3 + 6 * (max_deg - min_deg)
    out = torch.empty((*xc.shape[:-1], F), dtype=torch.float32, device=xc.device)
    with torch.cuda.device(xc.device):
        check(lib.aon_pos_enc(_ptr(xc), n, min_deg, max_deg, _ptr(out), _stream()), "aon_pos_enc")
    return out


# ------------------------------------------------------------------ R5 MLP
VANILLA_PARAM_ORDER = (
    [f"pts_linears.{i}.{k}" for i in range(8) for k in ("weight", "bias")]
    + [f"{m}.{k}" for m in ("views_linear.0", "bottleneck_layer", "density_layer", "rgb_layer") for k in ("weight", "bias")]
)
VANILLA_PARAM_SHAPES = {
    "pts_linears.0.weight": (256, 63), "pts_linears.5.weight": (256, 319), "views_linear.0.weight": (128, 283),
    "bottleneck_layer.weight": (256, 256), "density_layer.weight": (1, 256), "rgb_layer.weight": (3, 128),
    "views_linear.0.bias": (128,), "bottleneck_layer.bias": (256,), "density_layer.bias": (1,), "rgb_layer.bias": (3,),
}
for _i in (1, 2, 3, 4, 6, 7):
    VANILLA_PARAM_SHAPES[f"pts_linears.{_i}.weight"] = (256, 256)
for _i in range(8):
    VANILLA_PARAM_SHAPES[f"pts_linears.{_i}.bias"] = (256,)


def packed_bytes() -> int:
    return int(lib.aon_mlp_packed_bytes())


def pack_vanilla_mlp(params: dict, out: torch.Tensor | None = None, degrees=(0, 10, 4)) -> torch.Tensor:
    """params: name -> tensor with the reference's NeRFMLP parameter names (no prefix).  Returns the packed
    uint8 weight stream consumed by mlp_fwd / render_fwd (re-pack whenever the parameters change).  ``degrees`` =
    (min_deg_point, max_deg_point, deg_view) of a default-size network with at most 10 / 4 frequency levels: the slots of the
    missing levels get zero weight (aon_pack_vanilla_mlp_deg)."""
    mn, mx, dv = degrees
    shapes = dict(VANILLA_PARAM_SHAPES)
    P, V = 3 + 6 * (mx - mn), 3 + 6 * dv
    shapes.update({"pts_linears.0.weight": (256, P), "pts_linears.5.weight": (256, 256 + P), "views_linear.0.weight": (128, 256 + V)})
    tensors = []
    for name in VANILLA_PARAM_ORDER:
        t = _f32(params[name].detach(), name)
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {shapes[name]} (the fused kernels take the reference's default "
                             f"NeRFMLP sizes with encoding degrees {tuple(degrees)})")
        tensors.append(t)
    dev = tensors[0].device
    if out is None:
        out = torch.empty(packed_bytes(), dtype=torch.uint8, device=dev)
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    with torch.cuda.device(dev):
        if tuple(degrees) == (0, 10, 4):
            check(lib.aon_pack_vanilla_mlp(arr, _ptr(out), _stream()), "aon_pack_vanilla_mlp")
        else:
            check(lib.aon_pack_vanilla_mlp_deg(arr, mn, mx, dv, _ptr(out), _stream()), "aon_pack_vanilla_mlp_deg")
    return _tag(out)


def mlp_fwd(packed, rays_o, rays_d, viewdirs, t_vals, out=None):
    """cast_rays + pos_enc + NeRFMLP.forward fused.  Returns raw (n,S,4) = (raw_rgb, raw_density).
    ``out``: a contiguous fp32 (n, S, 4) tensor to write instead of a fresh one (as art_mlp_fwd: the backdrop's rows of a scene's buffer)."""
    o, d, v, t = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(viewdirs, "viewdirs"), _f32(t_vals, "t_vals")
    n, S = t.shape
    if out is None:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=t.device)
    else:
        raw = out
        if not (isinstance(raw, torch.Tensor) and raw.dtype == torch.float32 and tuple(raw.shape) == (n, S, 4) and raw.device == t.device
                and raw.is_contiguous()):
            raise ValueError(f"mlp_fwd: out must be a contiguous float32 ({n}, {S}, 4) tensor on {t.device}")
    with torch.cuda.device(t.device):
        check(lib.aon_mlp_fwd(_pk(packed), _ptr(o), _ptr(d), _ptr(v), _ptr(t), n, S, _ptr(raw), _stream()), "aon_mlp_fwd")
    return raw


def mlp_fwd_enc(packed, samples_enc, viewdirs_enc):
    x, c = _f32(samples_enc, "samples_enc"), _f32(viewdirs_enc, "viewdirs_enc")
    n, S, F = x.shape
    if F != 63 or tuple(c.shape) != (n, 27):
        raise ValueError("mlp_fwd_enc expects samples_enc (n,S,63) and viewdirs_enc (n,27)")
    raw = torch.empty((n, S, 4), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.aon_mlp_fwd_enc(_pk(packed), _ptr(x), _ptr(c), n, S, _ptr(raw), _stream()), "aon_mlp_fwd_enc")
    return raw


# ------------------------------------------------------------------ constructor arguments beyond the defaults
class RenderOpts:
    """Sampler / activation arguments of ``NeRF.__init__`` (model.py:124-135) and ``NeRF_AE_Art.__init__``
    (model_autodecoder.py:241-257) -> ``aon_render_opts``.  Python numbers become fp32 exactly where torch would round them."""

    def __init__(self, num_coarse_samples=64, num_fine_samples=128, lindisp=False, noise_std=0.0, rgb_padding=0.001, density_bias=-1.0,
                 degrees=(0, 10, 4)):
        self.degrees = tuple(int(x) for x in degrees)   # (min_deg_point, max_deg_point, deg_view) of a default-size network on the fused kernels
        self.num_coarse_samples, self.num_fine_samples = int(num_coarse_samples), int(num_fine_samples)
        self.lindisp, self.noise_std = bool(lindisp), float(noise_std)
        self.rgb_padding, self.density_bias = float(rgb_padding), float(density_bias)
        if not 2 <= self.num_coarse_samples <= 1023 or self.num_fine_samples < 1:
            raise ValueError("num_coarse_samples must be in [2, 1023] and num_fine_samples >= 1")

    @property
    def Sc(self) -> int:
        return self.num_coarse_samples + 1

    @property
    def Sf(self) -> int:
        return self.num_coarse_samples + 1 + self.num_fine_samples

    def S(self, level: int) -> int:
        return self.Sc if level == 0 else self.Sf

    def c_struct(self, near: float, far: float, noise=None):
        """-> (aon_render_opts, tensors to keep alive).  ``noise``: per-level (n,S) uniform draws or None (model.py:184)."""
        st = _lib.RenderOptsC()
        lib.aon_render_opts_init(C.byref(st))
        st.num_coarse_samples, st.num_fine_samples, st.lindisp = self.num_coarse_samples, self.num_fine_samples, int(self.lindisp)
        if self.lindisp:
            st.inv_near, st.inv_far = 1.0 / near, 1.0 / far      # double -> fp32 once (helper.py:117)
        st.rgb_scale, st.rgb_shift, st.sigma_bias = 1 + 2 * self.rgb_padding, self.rgb_padding, self.density_bias
        st.min_deg_point, st.max_deg_point, st.deg_view = self.degrees
        keep = []
        if noise is not None and self.noise_std > 0:
            st.noise_std = self.noise_std
            for lvl, field in enumerate(("noise_c", "noise_f")):
                if lvl < len(noise) and noise[lvl] is not None:
                    t = _f32(noise[lvl], "noise")
                    keep.append(t)
                    setattr(st, field, t.data_ptr())
        return st, keep


DEFAULT_OPTS = RenderOpts()


def _opts(opts):
    return DEFAULT_OPTS if opts is None else opts


# ------------------------------------------------------------------ R8 compositing
def _composite(rgb_t, rgb_stride, sig_t, sig_off, sig_stride, t_vals, dirs, white_bkgd, act, want_weights):
    t, d = _f32(t_vals, "t_vals"), _f32(dirs, "dirs")
    n, S = t.shape
    dev = t.device
    comp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    weights = torch.empty((n, S), dtype=torch.float32, device=dev) if want_weights else None
    sig_ptr = C.c_void_p(sig_t.data_ptr() + 4 * sig_off)
    with torch.cuda.device(dev):
        check(lib.aon_composite(_ptr(rgb_t), rgb_stride, sig_ptr, sig_stride, _ptr(t), _ptr(d), n, S, int(bool(white_bkgd)), act,
                                _ptr(comp), _ptr(acc), _ptr(depth), _ptr(weights), _stream()), "aon_composite")
    return comp, acc, weights, depth


def volumetric_rendering(rgb, density, t_vals, dirs, white_bkgd):
    """helper.volumetric_rendering on activated rgb (n,S,3) / density (n,S,1)."""
    r, s = _f32(rgb, "rgb"), _f32(density, "density")
    return _composite(r, 3, s, 0, 1, t_vals, dirs, white_bkgd, ACT_NONE, True)


def composite_raw(raw, t_vals, dirs, white_bkgd, act=ACT_VANILLA, want_weights=True, opts=None, noise=None):
    """Activation + compositing of the fused kernel's packed raw (n,S,4).  ``opts`` / ``noise`` (n,S): the activation scalars
    and the density noise of a non-default constructor (aon_composite_ex)."""
    r = _f32(raw, "raw")
    if opts is None and noise is None:
        return _composite(r, 4, r, 3, 4, t_vals, dirs, white_bkgd, act, want_weights)
    t, d = _f32(t_vals, "t_vals"), _f32(dirs, "dirs")
    n, S = t.shape
    dev = t.device
    st, keep = _opts(opts).c_struct(1.0, 1.0, [noise])
    comp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    weights = torch.empty((n, S), dtype=torch.float32, device=dev) if want_weights else None
    with torch.cuda.device(dev):
        check(lib.aon_composite_ex(_ptr(r), 4, C.c_void_p(r.data_ptr() + 12), 4, _ptr(t), _ptr(d), n, S, int(bool(white_bkgd)), act,
                                   C.byref(st), _ptr(comp), _ptr(acc), _ptr(depth), _ptr(weights), _stream()), "aon_composite_ex")
    return comp, acc, weights, depth


# ------------------------------------------------------------------ R6/R7 inverse CDF
_U_CACHE: dict = {}


def deterministic_u(device, num_samples: int = 128) -> torch.Tensor:
    """helper.py:229: torch.linspace(0, 1 - 2**-32, num_samples) (fp32; the last element rounds to exactly 1.0).
    Computed once on the host and copied, so it is the same vector the reference builds."""
    key = (str(device), num_samples)
    if key not in _U_CACHE:
        _U_CACHE[key] = torch.linspace(0.0, 1.0 - 2.0 ** -32, num_samples).to(device)
    return _U_CACHE[key]


def _u_args(u, n, device, nf: int = 128):
    if u is None:
        return deterministic_u(device, nf), 0
    uu = _f32(u, "u")
    if tuple(uu.shape) == (nf,):
        return uu, 0
    if tuple(uu.shape) != (n, nf):
        raise ValueError(f"u must be ({nf},) or ({n},{nf}), got {tuple(uu.shape)}")
    return uu, nf


def sorted_piecewise_constant_pdf(bins, weights, u=None, num_samples: int = 128):
    """helper.sorted_piecewise_constant_pdf: bins (n,nb), weights (n,nb-1) -> num_samples draws per ray.  The reference
    geometry (64 bins, 128 draws) runs the specialised kernel, anything else aon_sample_pdf_n (same bits where they overlap)."""
    b, w = _f32(bins, "bins"), _f32(weights, "weights")
    n, nb = b.shape
    if tuple(w.shape) != (n, nb - 1) or nb < 2:
        raise ValueError(f"weights must be ({n},{nb - 1}) for bins ({n},{nb})")
    uu, us = _u_args(u, n, b.device, num_samples)
    samples = torch.empty((n, num_samples), dtype=torch.float32, device=b.device)
    with torch.cuda.device(b.device):
        if (nb, num_samples) == (64, 128):
            check(lib.aon_sample_pdf(_ptr(b), _ptr(w), 63, None, _ptr(uu), us, n, _ptr(samples), None, _stream()), "aon_sample_pdf")
        else:
            check(lib.aon_sample_pdf_n(_ptr(b), _ptr(w), nb - 1, None, _ptr(uu), us, n, nb, num_samples, 0, _ptr(samples), None, _stream()),
                  "aon_sample_pdf_n")
    return samples


def sample_pdf_t_n(t_coarse, coarse_weights, num_samples: int, u=None, bins=None, force_generic=False):
    """sample_pdf_t for any sizes: t_coarse (n,nt), the full coarse weights (n,nt) (the pdf uses weights[...,1:-1]) or explicit
    (bins (n,nb), weights (n,nb-1)) -> t_fine (n, nt + num_samples), through aon_sample_pdf_n."""
    t, w = _f32(t_coarse, "t_coarse"), _f32(coarse_weights, "weights")
    n, nt = t.shape
    b = None if bins is None else _f32(bins, "bins")
    nb = nt - 1 if b is None else b.shape[1]
    if tuple(w.shape) == (n, nb + 1):
        w_ptr, w_stride = C.c_void_p(w.data_ptr() + 4), nb + 1
    elif tuple(w.shape) == (n, nb - 1):
        w_ptr, w_stride = _ptr(w), nb - 1
    else:
        raise ValueError(f"weights must be ({n},{nb + 1}) or ({n},{nb - 1})")
    uu, us = _u_args(u, n, t.device, num_samples)
    t_fine = torch.empty((n, nt + num_samples), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_sample_pdf_n(_ptr(b), w_ptr, w_stride, _ptr(t), _ptr(uu), us, n, nb, num_samples, nt, None, _ptr(t_fine), _stream()),
              "aon_sample_pdf_n")
    return t_fine


def sample_pdf_t(t_coarse, coarse_weights, u=None, bins=None):
    """t_fine (n,193) = sort(cat[t_coarse, inverse-CDF samples]) from the full coarse weights (n,65)
    (the pdf uses weights[...,1:-1]) -- or from explicit (bins (n,64), weights (n,63))."""
    t = _f32(t_coarse, "t_coarse")
    w = _f32(coarse_weights, "weights")
    n = t.shape[0]
    if tuple(t.shape) != (n, 65):
        raise ValueError("t_coarse must be (n,65)")
    if tuple(w.shape) == (n, 65):
        w_ptr, w_stride = C.c_void_p(w.data_ptr() + 4), 65
    elif tuple(w.shape) == (n, 63):
        w_ptr, w_stride = _ptr(w), 63
    else:
        raise ValueError("weights must be (n,65) or (n,63)")
    b = None if bins is None else _f32(bins, "bins")
    uu, us = _u_args(u, n, t.device)
    t_fine = torch.empty((n, 193), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_sample_pdf(_ptr(b), w_ptr, w_stride, _ptr(t), _ptr(uu), us, n, None, _ptr(t_fine), _stream()), "aon_sample_pdf")
    return t_fine


def composite_pdf(raw, t_coarse, dirs, white_bkgd, act=ACT_VANILLA, u=None, want_weights=False):
    """Coarse level of NeRF.forward in ONE kernel (model.py:160-173): compositing of the packed raw (n,65,4) records and the
    fine level's sampling -> (comp_rgb, acc, weights | None, depth, t_fine (n,193)).  Same bits as composite_raw followed by
    sample_pdf_t."""
    r, t, d = _f32(raw, "raw"), _f32(t_coarse, "t_coarse"), _f32(dirs, "dirs")
    n, dev = t.shape[0], t.device
    if tuple(t.shape) != (n, 65) or r.numel() != n * 65 * 4:
        raise ValueError("composite_pdf: t_coarse must be (n,65) and raw (n,65,4)")
    uu, us = _u_args(u, n, dev)
    comp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    weights = torch.empty((n, 65), dtype=torch.float32, device=dev) if want_weights else None
    t_fine = torch.empty((n, 193), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_composite_pdf(_ptr(r), _ptr(t), _ptr(d), n, int(bool(white_bkgd)), act, _ptr(uu), us, _ptr(comp), _ptr(acc),
                                    _ptr(depth), _ptr(weights), _ptr(t_fine), _stream()), "aon_composite_pdf")
    return comp, acc, weights, depth, t_fine


def set_coarse_fusion(on: bool) -> None:
    """Whole-path entry points: coarse compositing + inverse CDF as one kernel (default) or as the two stage kernels."""
    check(lib.aon_set_coarse_fusion(int(bool(on))), "aon_set_coarse_fusion")


# ------------------------------------------------------------------ R9 whole path
_WS_CACHE = StreamCache()
# rays rendered per internal chunk: a whole 640x480 frame (307,200 rays) in one pass -- 4,892 B/ray of per-ray buffers (sample
# records, t, weights, the per-ray view bias) = 1.5 GB of the 288 GB, so that every per-ray kernel is ONE launch per frame (round 2: 65,536-ray chunks, five 30-60 us launches
# each of which spent a fifth of its time ramping up and draining)
MAX_CHUNK_RAYS = 327680


def _workspace(device, n_rays: int, st=None, vanilla=False) -> torch.Tensor:
    """``vanilla``: with room for the deferred view branch (set_deferred_view) while that switch is on."""
    chunk = MAX_CHUNK_RAYS
    if st is not None and (st.min_deg_point, st.max_deg_point, st.deg_view) != (0, 10, 4):
        chunk = 65536      # the encodings of a chunk are materialised (51 KB per ray) for other degrees
    query = "aon_render_deferred_workspace_bytes" if vanilla and lib.aon_get_deferred_view() else "aon_render_workspace_bytes_ex"
    need = int(getattr(lib, query)(min(n_rays, chunk), None if st is None else C.byref(st)))
    if need < 0:
        check(need, query)
    return _scratch(_WS_CACHE, device, need)


def _check_noise(noise, n, op, num_levels):
    if noise is None:
        return None
    out = []
    for lvl in range(num_levels):
        t = noise[lvl] if lvl < len(noise) else None
        if t is not None and t.numel() != n * op.S(lvl):
            raise ValueError(f"noise[{lvl}] must hold ({n},{op.S(lvl)}) values, got {tuple(t.shape)}")
        out.append(t)
    return out


def _level_outs(n, dev, num_levels):
    outs = [(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
             torch.empty((n,), dtype=torch.float32, device=dev)) for _ in range(num_levels)]
    return outs, (outs[1] if num_levels == 2 else (None, None, None))


class _PathCall:
    """The prologue of every whole-path forward, and the Python side of csrc/aon_capi_util.h's PathCall: the
    conversions and shape checks of the common arguments, the per-level outputs and the aon_render_opts struct.  `args(ws)` is the C
    argument list from rays_o up to and including opts, the same for every form; a call is `getattr(lib, name)(*packs, *pc.args(ws),
    *extra)`.  The object holds every tensor those pointers refer to: keep it until the call has returned.
    ``per_ray``: the caller takes near / far tensors (and a `ray_live` mask) -> `bounds` is the aon_ray_bounds struct or None."""

    def __init__(self, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise, per_ray=False, ray_live=None):
        o, d, v = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(viewdirs, "viewdirs")
        self.n, self.dev = n, dev = o.shape[0], o.device
        self.op = op = _opts(opts)
        near, far, self.bounds, bkeep = _ray_bounds(near, far, n, dev, ray_live) if per_ray else (float(near), float(far), None, ())
        tr = None if t_rand is None else _f32(t_rand, "t_rand")
        if tr is not None and tuple(tr.shape) != (n, op.Sc):
            raise ValueError(f"t_rand must be ({n},{op.Sc})")
        self.uu, us = _u_args(u, n, dev, op.num_fine_samples) if num_levels == 2 else (None, 0)
        self.outs, fine = _level_outs(n, dev, num_levels)
        self.st, self.noise_keep = op.c_struct(near, far, _check_noise(noise, n, op, num_levels))
        self._keep = (o, d, v, tr, bkeep)
        self._head = (_ptr(o), _ptr(d), _ptr(v), n, float(near), float(far), int(bool(white_bkgd)), num_levels, _ptr(tr), _ptr(self.uu), us,
                      *(_ptr(x) for x in self.outs[0]), *(_ptr(x) for x in fine))

    def args(self, ws):
        return (*self._head, _ptr(ws), ws.numel(), _stream(), C.byref(self.st))


def _render_call(name, packs, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise, ray_live, workspace_bytes):
    """render_fwd / art_render_fwd: `name` is the C stem ("aon_render_fwd" / "aon_art_render_fwd"), `packs` its network pointers."""
    if isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor) or ray_live is not None:
        return _stop_call(name + "_stop", packs, rays_o, rays_d, viewdirs, near, far, white_bkgd, None, 0.0, None, num_levels, u, opts, workspace_bytes,
                          t_rand=t_rand, noise=noise, ray_live=ray_live, want_stats=False)[0]
    pc = _PathCall(rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise)
    ws = _workspace(pc.dev, pc.n, pc.st, vanilla=name == "aon_render_fwd")
    with torch.cuda.device(pc.dev):
        check(getattr(lib, name + "_ex")(*packs, *pc.args(ws)), name)
    return pc.outs


def render_fwd(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels=2, t_rand=None, u=None,
               opts=None, noise=None, ray_live=None, workspace_bytes=None):
    """NeRF.forward: returns [(rgb, acc, depth)_coarse, (rgb, acc, depth)_fine] (fine omitted if num_levels == 1).
    ``opts`` (RenderOpts): non-default sample counts / lindisp / noise_std; ``noise``: per-level (n,S) uniform draws.
    ``near`` / ``far``: numbers, or per-ray tensors of N elements; ``ray_live`` (N,) uint8: dead rays run no MLP and composite to the
    background (inference only)."""
    return _render_call("aon_render_fwd", (_pk(packed_coarse), _pk(packed_fine)), rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u,
                        opts, noise, ray_live, workspace_bytes)


# ------------------------------------------------------------------ R10/R11 articulated network
ART_PARAM_ORDER = (
    [f"deformations_linear.{i}.{k}" for i in range(4) for k in ("weight", "bias")]
    + [f"deformation_layer.{k}" for k in ("weight", "bias")]
    + [f"pts_linears.{i}.{k}" for i in range(8) for k in ("weight", "bias")]
    + [f"views_linear.{i}.{k}" for i in range(4) for k in ("weight", "bias")]
    + [f"{m}.{k}" for m in ("bottleneck_layer", "density_layer", "rgb_layer") for k in ("weight", "bias")]
)
ART_PARAM_SHAPES = {
    "deformations_linear.0.weight": (128, 163), "deformation_layer.weight": (3, 128), "deformation_layer.bias": (3,),
    "pts_linears.0.weight": (256, 191), "pts_linears.5.weight": (256, 447), "views_linear.0.weight": (128, 411),
    "bottleneck_layer.weight": (256, 256), "bottleneck_layer.bias": (256,), "density_layer.weight": (1, 256),
    "density_layer.bias": (1,), "rgb_layer.weight": (3, 128), "rgb_layer.bias": (3,),
}
for _i in (1, 2, 3):
    ART_PARAM_SHAPES[f"deformations_linear.{_i}.weight"] = (128, 128)
    ART_PARAM_SHAPES[f"views_linear.{_i}.weight"] = (128, 128)
for _i in range(4):
    ART_PARAM_SHAPES[f"deformations_linear.{_i}.bias"] = (128,)
    ART_PARAM_SHAPES[f"views_linear.{_i}.bias"] = (128,)
for _i in (1, 2, 3, 4, 6, 7):
    ART_PARAM_SHAPES[f"pts_linears.{_i}.weight"] = (256, 256)
for _i in range(8):
    ART_PARAM_SHAPES[f"pts_linears.{_i}.bias"] = (256,)


def art_param_shapes(degrees=(0, 10, 4)) -> dict:
    """Parameter shapes of the articulated NeRFMLP built with (min_deg_point, max_deg_point, deg_view) and default widths
    (model_autodecoder.py:60-170): the three concatenating layers follow P = 3 + 6 (max - min), V = 3 + 6 deg_view."""
    lo, hi, dv = (int(x) for x in degrees)
    if not (0 <= hi - lo <= 10 and 0 <= dv <= 4 and -32 <= lo and hi <= 16):
        raise NotImplementedError(f"articulated NeRFMLP with degrees {tuple(degrees)}: the kernels hold up to 10 position and 4 view frequency levels, "
                                  "min_deg_point >= -32 and max_deg_point <= 16 (the in-register encoding's sine holds for arguments below 2^19)")
    P, V = 3 + 6 * (hi - lo), 3 + 6 * dv
    shapes = dict(ART_PARAM_SHAPES)
    shapes["pts_linears.0.weight"] = (256, P + 128)
    shapes["pts_linears.5.weight"] = (256, 256 + P + 128)
    shapes["views_linear.0.weight"] = (128, 256 + V + 128)
    return shapes


def _art_param_array(params: dict, degrees=(0, 10, 4)):
    tensors = []
    shapes = ART_PARAM_SHAPES if tuple(degrees) == (0, 10, 4) else art_param_shapes(degrees)
    for name in ART_PARAM_ORDER:
        t = _f32(params[name].detach(), name)
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {shapes[name]} (the articulated NeRFMLP has HIP kernels for the "
                             f"reference's default widths at degrees {tuple(degrees)})")
        tensors.append(t)
    return tensors, (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def pack_art_mlp(params: dict, out: torch.Tensor | None = None, degrees=(0, 10, 4)) -> torch.Tensor:
    """Packed weight stream of one articulated NeRFMLP (re-pack whenever the parameters change); other ``degrees``: zero weight in the
    63 / 27-wide slots of the levels the network lacks (aon_pack_art_mlp_deg)."""
    tensors, arr = _art_param_array(params, degrees)
    dev = tensors[0].device
    if out is None:
        out = torch.empty(int(lib.aon_art_packed_bytes()), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_pack_art_mlp_deg(arr, int(degrees[0]), int(degrees[1]), int(degrees[2]), _ptr(out), _stream()), "aon_pack_art_mlp_deg")
    return _tag(out)


def _latent(latents: dict, key: str, width: int) -> torch.Tensor:
    t = _f32(latents[key].detach(), f"latents[{key!r}]").reshape(-1)
    if t.numel() != width:
        raise ValueError(f"latents[{key!r}] must hold {width} values (one instance per call, like the reference's "
                         f"'n1 c -> (n1 n2) c' broadcast), got {tuple(latents[key].shape)}")
    return t


def art_prepare(params: dict, latents: dict, out: torch.Tensor | None = None, degrees=(0, 10, 4)) -> torch.Tensor:
    """Per-call block: small vectors + biases with the three latents folded in (latents keys as the reference:
    'density' (1,128), 'color' (1,128), 'articulation' (1,32)) + the ten encoding scales of ``degrees``."""
    tensors, arr = _art_param_array(params, degrees)
    dev = tensors[0].device
    shape, app, art = _latent(latents, "density", 128), _latent(latents, "color", 128), _latent(latents, "articulation", 32)
    if out is None:
        out = torch.empty(int(lib.aon_art_small_bytes()), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_art_prepare_deg(arr, _ptr(shape), _ptr(app), _ptr(art), int(degrees[0]), int(degrees[1]), int(degrees[2]), _ptr(out), _stream()),
              "aon_art_prepare_deg")
    return _tag(out)


def art_pack_step(params_c: dict, params_f: dict, latents: dict, degrees=(0, 10, 4), with_bwd: bool = True, out=None):
    """pack_art_mlp + art_prepare (+ pack_art_mlp_bwd) of the coarse and the fine network in ONE C call (aon_art_pack_step): the four fp64
    fold products as one launch in front.  -> [(packed, small, packed_bwd or None)] per level, tagged with their form; fresh buffers unless
    ``out`` = [(packed, small, packed_bwd or None)] x 2 hands in uint8 buffers of the library's sizes."""
    tens, arrs = [], []
    for params in (params_c, params_f):
        t, arr = _art_param_array(params, degrees)
        tens.append(t)
        arrs.append(arr)
    shape, app, art = _latent(latents, "density", 128), _latent(latents, "color", 128), _latent(latents, "articulation", 32)
    dev = tens[0][0].device
    new = lambda nbytes: torch.empty(int(nbytes), dtype=torch.uint8, device=dev)   # noqa: E731
    if out is not None:
        pk, sm, bw = ([o[i] for o in out] for i in range(3))
        for got, want in zip(pk + sm + bw, [lib.aon_art_packed_bytes()] * 2 + [lib.aon_art_small_bytes()] * 2 + [lib.aon_art_bwd_packed_bytes()] * 2):
            if got is not None and (got.dtype != torch.uint8 or got.numel() != int(want) or got.device != dev or not got.is_contiguous()):
                raise ValueError(f"art_pack_step: out buffers must be contiguous uint8 tensors of the library's sizes on {dev}")
    else:
        pk = [new(lib.aon_art_packed_bytes()) for _ in range(2)]
        sm = [new(lib.aon_art_small_bytes()) for _ in range(2)]
        bw = [new(lib.aon_art_bwd_packed_bytes()) if with_bwd else None for _ in range(2)]
    with torch.cuda.device(dev):
        check(lib.aon_art_pack_step(arrs[0], arrs[1], _ptr(shape), _ptr(app), _ptr(art), int(degrees[0]), int(degrees[1]), int(degrees[2]),
                                    _ptr(pk[0]), _ptr(sm[0]), _ptr(bw[0]), _ptr(pk[1]), _ptr(sm[1]), _ptr(bw[1]), _stream()), "aon_art_pack_step")
    return [(_tag(pk[l]), _tag(sm[l]), None if bw[l] is None else _tag(bw[l])) for l in range(2)]


def vanilla_pack_step(params_c: dict, params_f: dict, degrees=(0, 10, 4), with_bwd: bool = True, out=None):
    """pack_vanilla_mlp (+ pack_vanilla_mlp_bwd) of the coarse and the fine network in ONE C call (aon_vanilla_pack_step): the eight fp64
    fold products as one launch in front.  -> [(packed, packed_bwd or None)] per level, tagged with their form; fresh buffers unless ``out`` =
    [(packed, packed_bwd or None)] x 2 hands in uint8 buffers of the library's sizes."""
    shapes = vanilla_param_shapes(degrees)
    arrs, keep = [], []
    for params in (params_c, params_f):
        tensors = [_f32(params[name].detach(), name) for name in VANILLA_PARAM_ORDER]
        for name, t in zip(VANILLA_PARAM_ORDER, tensors):
            if tuple(t.shape) != shapes[name]:
                raise ValueError(f"{name}: shape {tuple(t.shape)} != {shapes[name]} for encoding degrees {tuple(degrees)}")
        keep.append(tensors)
        arrs.append((C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]))
    dev = keep[0][0].device
    sizes = (packed_bytes(), int(lib.aon_bwd_packed_bytes()))
    if out is not None:
        pk, bw = ([o[i] for o in out] for i in range(2))
        for got, want in zip(pk + bw, [sizes[0]] * 2 + [sizes[1]] * 2):
            if got is not None and (got.dtype != torch.uint8 or got.numel() != want or got.device != dev or not got.is_contiguous()):
                raise ValueError(f"vanilla_pack_step: out buffers must be contiguous uint8 tensors of the library's sizes on {dev}")
    else:
        pk = [torch.empty(sizes[0], dtype=torch.uint8, device=dev) for _ in range(2)]
        bw = [torch.empty(sizes[1], dtype=torch.uint8, device=dev) if with_bwd else None for _ in range(2)]
    with torch.cuda.device(dev):
        check(lib.aon_vanilla_pack_step(arrs[0], arrs[1], int(degrees[0]), int(degrees[1]), int(degrees[2]), _ptr(pk[0]), _ptr(bw[0]), _ptr(pk[1]), _ptr(bw[1]),
                                        _stream()), "aon_vanilla_pack_step")
    return [(_tag(pk[l]), None if bw[l] is None else _tag(bw[l])) for l in range(2)]


def art_mlp_fwd(packed, small, rays_o, rays_d, viewdirs, t_vals, out=None):
    """``out``: a contiguous fp32 (n, S, 4) tensor to write instead of a fresh one (a slice of a larger buffer: ops.scene_pairs' segments)."""
    o, d, v, t = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(viewdirs, "viewdirs"), _f32(t_vals, "t_vals")
    n, S = t.shape
    if out is None:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=t.device)
    else:
        raw = out
        if not (isinstance(raw, torch.Tensor) and raw.dtype == torch.float32 and tuple(raw.shape) == (n, S, 4) and raw.device == t.device
                and raw.is_contiguous()):
            raise ValueError(f"art_mlp_fwd: out must be a contiguous float32 ({n}, {S}, 4) tensor on {t.device}")
    with torch.cuda.device(t.device):
        check(lib.aon_art_mlp_fwd(_pk(packed), _pk(small), _ptr(o), _ptr(d), _ptr(v), _ptr(t), n, S, _ptr(raw), _stream()),
              "aon_art_mlp_fwd")
    return raw


def art_mlp_fwd_pos(packed, small, pos, viewdirs_enc):
    x, c = _f32(pos, "pos"), _f32(viewdirs_enc, "viewdirs_enc")
    n, S, F = x.shape
    if F != 3 or tuple(c.shape) != (n, 27):
        raise ValueError("art_mlp_fwd_pos expects pos (n,S,3) and viewdirs_enc (n,27)")
    raw = torch.empty((n, S, 4), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.aon_art_mlp_fwd_pos(_pk(packed), _pk(small), _ptr(x), _ptr(c), n, S, _ptr(raw), _stream()), "aon_art_mlp_fwd_pos")
    return raw


def art_render_fwd(packed_c, small_c, packed_f, small_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels=2,
                   t_rand=None, u=None, opts=None, noise=None, ray_live=None, workspace_bytes=None):
    """NeRF_AE_Art.forward: [(rgb, acc, depth)_coarse, (rgb, acc, depth)_fine].  Per-ray ``near`` / ``far`` / ``ray_live``: as render_fwd."""
    return _render_call("aon_art_render_fwd", (_pk(packed_c), _pk(small_c), _pk(packed_f), _pk(small_f)), rays_o, rays_d, viewdirs, near, far, white_bkgd,
                        num_levels, t_rand, u, opts, noise, ray_live, workspace_bytes)


# ------------------------------------------------------------------ R14 training (vanilla)
def vanilla_param_shapes(degrees=(0, 10, 4)) -> dict:
    """Shapes of a default-size NeRFMLP with the given encoding degrees (the fused kernels' networks)."""
    mn, mx, dv = degrees
    P, V = 3 + 6 * (mx - mn), 3 + 6 * dv
    shapes = dict(VANILLA_PARAM_SHAPES)
    shapes.update({"pts_linears.0.weight": (256, P), "pts_linears.5.weight": (256, 256 + P), "views_linear.0.weight": (128, 256 + V)})
    return shapes


def pack_vanilla_mlp_bwd(params: dict, out: torch.Tensor | None = None, degrees=(0, 10, 4)) -> torch.Tensor:
    """Transposed weight stream for the backward data chain (re-pack whenever the parameters change)."""
    shapes = vanilla_param_shapes(degrees)
    tensors = [_f32(params[name].detach(), name) for name in VANILLA_PARAM_ORDER]
    for name, t in zip(VANILLA_PARAM_ORDER, tensors):
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {shapes[name]} for encoding degrees {tuple(degrees)}")
    dev = tensors[0].device
    if out is None:
        out = torch.empty(int(lib.aon_bwd_packed_bytes()), dtype=torch.uint8, device=dev)
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    with torch.cuda.device(dev):
        if tuple(degrees) == (0, 10, 4):
            check(lib.aon_pack_vanilla_mlp_bwd(arr, _ptr(out), _stream()), "aon_pack_vanilla_mlp_bwd")
        else:
            check(lib.aon_pack_vanilla_mlp_bwd_deg(arr, degrees[0], degrees[1], degrees[2], _ptr(out), _stream()), "aon_pack_vanilla_mlp_bwd_deg")
    return _tag(out)


def padded_samples(n_samples: int) -> int:
    return (n_samples + 127) // 128 * 128


# Training planes are STEP-MAJOR (include/aon_hip.h, csrc/aon_mlp_core.h): a tensor of shape (Np / 32, rows / 4, 32, 4) =
# [step of 32 samples][feature row / 4][sample in step][feature row % 4].
def _new_planes(rows: int, Np: int, device) -> torch.Tensor:
    return torch.empty((Np // 32, rows // 4, 32, 4), dtype=torch.float32, device=device)


def plane_samples(planes: torch.Tensor) -> int:
    """Np, the padded sample count of a plane buffer."""
    return planes.shape[0] * 32


def plane_rows_view(planes: torch.Tensor) -> torch.Tensor:
    """(rows, Np) view-copy of step-major planes: row f, column s = feature row f of sample s (tests, diagnostics)."""
    nst, ng = planes.shape[0], planes.shape[1]
    return planes.permute(1, 3, 0, 2).reshape(ng * 4, nst * 32)


def mlp_fwd_train(packed, rays_o, rays_d, viewdirs, t_vals, out=None):
    """Fused forward that also stores the step-major activation planes and the ReLU bit masks
    -> (raw (n,S,4), planes (Np/32, rows/4, 32, 4), masks).
    ``out``: as ops.art_mlp_fwd_train's -- a contiguous fp32 (n, S, 4) tensor to write ``raw`` into instead of a fresh one (the backdrop's rows
    of a scene's buffer)."""
    o, d, v, t = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(viewdirs, "viewdirs"), _f32(t_vals, "t_vals")
    n, S = t.shape
    Np = padded_samples(n * S)
    if out is None:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=t.device)
    else:
        raw = out
        if not (isinstance(raw, torch.Tensor) and raw.dtype == torch.float32 and tuple(raw.shape) == (n, S, 4) and raw.device == t.device
                and raw.is_contiguous()):
            raise ValueError(f"mlp_fwd_train: out must be a contiguous float32 ({n}, {S}, 4) tensor on {t.device}")
    # every row the backward consumes is fully written by the kernel (padded columns included); the encoding pad rows
    # (63, and 27..31 of the view block) only ever feed gradient columns that are never emitted -> no zero fill needed
    planes = _new_planes(int(lib.aon_train_plane_rows()), Np, t.device)
    masks = torch.empty(int(lib.aon_train_mask_bytes(Np)), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_mlp_fwd_train(_pk(packed), _ptr(o), _ptr(d), _ptr(v), _ptr(t), n, S, _ptr(raw), _ptr(planes), _ptr(masks), _stream()), "aon_mlp_fwd_train")
    return raw, planes, masks


def composite_bwd(raw, t_vals, dirs, g_rgb, g_acc, g_depth, white_bkgd, act, Np: int):
    """-> d_raw (Np,4): dL/d(raw rgb, raw sigma), zero in the padded tail."""
    r, t, d, g = _f32(raw, "raw"), _f32(t_vals, "t_vals"), _f32(dirs, "dirs"), _f32(g_rgb, "g_rgb")
    ga = None if g_acc is None else _f32(g_acc, "g_acc")
    gd = None if g_depth is None else _f32(g_depth, "g_depth")
    n, S = t.shape
    d_raw = torch.zeros((Np, 4), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_composite_bwd(_ptr(r), _ptr(t), _ptr(d), _ptr(g), _ptr(ga), _ptr(gd), n, S, int(bool(white_bkgd)), act,
                                    _ptr(d_raw), _stream()), "aon_composite_bwd")
    return d_raw


def mlp_bwd_chain(packed_bwd, packed_fwd, d_raw, masks, plane_shape):
    """-> dplanes (layout of the forward planes): pre-activation gradient planes (rows of the encodings are not written / not used)."""
    dplanes = torch.empty(tuple(plane_shape), dtype=torch.float32, device=d_raw.device)
    Np = plane_shape[0] * 32
    with torch.cuda.device(d_raw.device):
        check(lib.aon_mlp_bwd_chain(_pk(packed_bwd), _pk(packed_fwd), _ptr(d_raw), _ptr(masks), _ptr(dplanes), Np, _stream()), "aon_mlp_bwd_chain")
    return dplanes


_WG_WS = StreamCache()


def vanilla_wgrad(planes, dplanes, d_raw, packed_bwd):
    """-> dict name -> gradient (the reference's NeRFMLP parameter names / shapes).  ``packed_bwd`` (required): the transposed stream the
    chain of these planes ran with -- its form (bottleneck folded or literal) is the planes' form, and the folded form's buffer carries the
    raw weights the un-folding reads.  (No default: with the fold on by default, "None = literal planes" would silently mis-read folded ones.)"""
    if packed_bwd is None:
        raise ValueError("vanilla_wgrad: pass the transposed stream (pack_vanilla_mlp_bwd) the backward chain of these planes ran with")
    dev = planes.device
    ws = _scratch(_WG_WS, dev, int(lib.aon_wgrad_workspace_bytes()))
    grads = {name: torch.empty(VANILLA_PARAM_SHAPES[name], dtype=torch.float32, device=dev) for name in VANILLA_PARAM_ORDER}
    arr = (C.c_void_p * len(VANILLA_PARAM_ORDER))(*[grads[n].data_ptr() for n in VANILLA_PARAM_ORDER])
    with torch.cuda.device(dev):
        check(lib.aon_vanilla_wgrad(_ptr(planes), _ptr(dplanes), _ptr(d_raw), plane_samples(planes), arr, _ptr(ws), ws.numel(), _stream(),
                                    _pk(packed_bwd)), "aon_vanilla_wgrad")
    return grads


# ------------------------------------------------------------------ R14 training (articulated)
def pack_art_mlp_bwd(params: dict, out: torch.Tensor | None = None, degrees=(0, 10, 4)) -> torch.Tensor:
    tensors, arr = _art_param_array(params, degrees)
    dev = tensors[0].device
    if out is None:
        out = torch.empty(int(lib.aon_art_bwd_packed_bytes()), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_pack_art_mlp_bwd_deg(arr, int(degrees[0]), int(degrees[1]), int(degrees[2]), _ptr(out), _stream()), "aon_pack_art_mlp_bwd_deg")
    return _tag(out)


def art_mlp_fwd_train(packed, small, rays_o, rays_d, viewdirs, t_vals, out=None):
    """``out``: as ops.art_mlp_fwd's -- a contiguous fp32 (n, S, 4) tensor to write ``raw`` into instead of a fresh one (a scene's segments)."""
    o, d, v, t = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(viewdirs, "viewdirs"), _f32(t_vals, "t_vals")
    n, S = t.shape
    Np = padded_samples(n * S)
    if out is None:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=t.device)
    else:
        raw = out
        if not (isinstance(raw, torch.Tensor) and raw.dtype == torch.float32 and tuple(raw.shape) == (n, S, 4) and raw.device == t.device
                and raw.is_contiguous()):
            raise ValueError(f"art_mlp_fwd_train: out must be a contiguous float32 ({n}, {S}, 4) tensor on {t.device}")
    planes = _new_planes(int(lib.aon_art_train_plane_rows()), Np, t.device)
    masks = torch.empty(int(lib.aon_art_train_mask_bytes(Np)), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.aon_art_mlp_fwd_train(_pk(packed), _pk(small), _ptr(o), _ptr(d), _ptr(v), _ptr(t), n, S, _ptr(raw), _ptr(planes), _ptr(masks), _stream()),
              "aon_art_mlp_fwd_train")
    return raw, planes, masks


def art_bwd_chain(packed_bwd, small, d_raw, masks, planes):
    """-> (dplanes (layout of the forward planes), dxp (Np,4) = dL/d deformed position)."""
    dplanes = torch.empty(planes.shape, dtype=torch.float32, device=planes.device)
    Np = plane_samples(planes)
    dxp = torch.empty((Np, 4), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib.aon_art_bwd_chain(_pk(packed_bwd), _pk(small), _ptr(d_raw), _ptr(masks), _ptr(planes), _ptr(dplanes), _ptr(dxp), Np, _stream()),
              "aon_art_bwd_chain")
    return dplanes, dxp


def art_wgrad(planes, dplanes, d_raw, dxp, params: dict, latents: dict, degrees=(0, 10, 4), *, packed_bwd):
    """-> (dict name -> parameter gradient, dict latent key -> gradient (flat)).  ``packed_bwd`` (required keyword): as vanilla_wgrad."""
    if packed_bwd is None:
        raise ValueError("art_wgrad: pass packed_bwd= the transposed stream (pack_art_mlp_bwd) the backward chain of these planes ran with")
    dev = planes.device
    ws = _scratch(_WG_WS, dev, int(lib.aon_wgrad_workspace_bytes()))
    tensors, parr = _art_param_array(params, degrees)
    shape, app, art = _latent(latents, "density", 128), _latent(latents, "color", 128), _latent(latents, "articulation", 32)
    shapes = art_param_shapes(degrees)
    grads = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in ART_PARAM_ORDER}
    garr = (C.c_void_p * len(ART_PARAM_ORDER))(*[grads[n].data_ptr() for n in ART_PARAM_ORDER])
    g_lat = {"density": torch.empty(128, device=dev), "color": torch.empty(128, device=dev), "articulation": torch.empty(32, device=dev)}
    with torch.cuda.device(dev):
        check(lib.aon_art_wgrad_deg(_ptr(planes), _ptr(dplanes), _ptr(d_raw), _ptr(dxp), plane_samples(planes), parr, _ptr(shape), _ptr(app),
                                    _ptr(art), garr, _ptr(g_lat["density"]), _ptr(g_lat["color"]), _ptr(g_lat["articulation"]), _ptr(ws),
                                    ws.numel(), _stream(), int(degrees[0]), int(degrees[1]), int(degrees[2]), _pk(packed_bwd)), "aon_art_wgrad_deg")
    return grads, g_lat


# ------------------------------------------------------------------ bottleneck_layer folded into views_linear[0] (round 5)
def set_bottleneck_fold(on: bool) -> None:
    """Form of the streams / per-call blocks the pack calls build from now on: folded (default: W' = W_v0[:, :256] W_b, one 256 -> 128
    layer where the reference's graph runs 256 -> 256 then 256 -> 128, model.py:109-114) or the literal two layers.  Buffers already
    packed keep their form (include/aon_hip.h)."""
    check(lib.aon_set_bottleneck_fold(int(bool(on))), "aon_set_bottleneck_fold")


def bottleneck_fold() -> bool:
    return bool(lib.aon_get_bottleneck_fold())


# ------------------------------------------------------------------ R14 training step in two C calls
def set_bwd_overlap(on: bool) -> None:
    """Two-level backward on two library streams (default on) or everything on the caller's stream."""
    check(lib.aon_set_bwd_overlap(2 if on == 2 else int(bool(on))), "aon_set_bwd_overlap")   # 2 (measurements): head reductions on side streams in the merged form


def _sized(nbytes: int, what: str, device) -> torch.Tensor:
    if nbytes < 0:
        check(nbytes, what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def set_fwd_overlap(on: bool) -> None:
    """Training forward of two levels as two ray halves on two library streams (default on) or everything on the caller's stream."""
    check(lib.aon_set_fwd_overlap(int(bool(on))), "aon_set_fwd_overlap")


def set_view_bias(on: bool) -> None:
    """Whole-path calls of the folded vanilla network: the view-encoding term as a per-ray bias (default on; same bits as the chunk form)."""
    check(lib.aon_set_view_bias(int(bool(on))), "aon_set_view_bias")


def set_deferred_view(on: bool) -> None:
    """Dense whole-path renders of the folded vanilla network: the view branch only on the samples with raw sigma > 0, behind a
    compaction (default on; same bits as the single kernel, which ``False`` puts back)."""
    check(lib.aon_set_deferred_view(int(bool(on))), "aon_set_deferred_view")


def deferred_view_enabled() -> bool:
    return bool(lib.aon_get_deferred_view())


def view_bias_enabled() -> bool:
    """True when the whole-path calls of folded networks use the per-ray view bias (needs the fold: bottleneck_fold())."""
    return bool(lib.aon_get_view_bias()) and bottleneck_fold()


def view_bias(packed: torch.Tensor, viewdirs: torch.Tensor) -> torch.Tensor:
    """(n,128) = b' + W_v0[:, 256:] pos_enc(viewdirs, 0, 4) of a folded vanilla stream: what the whole-path calls start the view layer from."""
    v = _f32(viewdirs, "viewdirs")
    n = v.numel() // 3
    out = torch.empty((n, 128), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        check(lib.aon_view_bias(_pk(packed), _ptr(v), n, _ptr(out), _stream()), "aon_view_bias")
    return out


def set_bwd_early_heads(on: bool) -> None:
    """Merged backward: the chain-independent head / bias reductions on a side stream beside the chain launch (default on; same bits)."""
    check(lib.aon_set_bwd_early_heads(int(bool(on))), "aon_set_bwd_early_heads")


def set_bwd_merge(on: bool) -> None:
    """Backward chains of the two levels as ONE persistent launch of two segments (default on; off: one launch per level, round 3)."""
    check(lib.aon_set_bwd_merge(int(bool(on))), "aon_set_bwd_merge")


def set_fwd_merge(on: bool) -> None:
    """Training forward of two levels as three persistent launches, coarse(A) | fine(A) + coarse(B) | fine(B) (default on; off: the
    forms of set_fwd_overlap)."""
    check(lib.aon_set_fwd_merge(2 if on == 2 else int(bool(on))), "aon_set_fwd_merge")   # 2 (tests): merge even when no round is saved


# The two big buffers of a training step -- the forward -> backward workspace (15 GB at 4096 articulated rays) and the backward's scratch
# (11 GB) -- are taken from / given back to a small POOL of this module instead of torch's caching allocator (round 6).  Through the allocator
# they were freed and re-requested every step, and while such a block sat free the step's own 2-7 MB allocations (weight streams, gradient
# buffers) could be carved out of it: the next request for the full size then found no block and the allocator went to the driver -- ONE
# hipMalloc of 11-15 GB, 80-125 ms of host time, once per process at a step that depends on timing (measured: 4 device mallocs and +13.9 GB
# reserved INSIDE the timed loop of every run of tools/train_bench.py; when the stall fell on an early step the device ran dry and the run
# averaged 33-40 ms per step instead of 30.4, tools/slowmode_probe.sh).  A pooled buffer is only handed to the stream it was returned on;
# at most two per (device, size) are kept; release_workspaces() drops them.
_TRAIN_POOL: "_collections.OrderedDict" = _collections.OrderedDict()
_TRAIN_POOL_KEEP = 2          # buffers kept per (device, size)
_TRAIN_POOL_SIZES = 6         # distinct (device, size) keys kept, least recently returned dropped first (a loop whose ray count changes every
                              # step must not pile up buffers: workspace + scratch of the full batch and of an epoch's tail batch are four keys)


def _pool_take(nbytes: int, what: str, device) -> torch.Tensor:
    if nbytes < 0:
        check(nbytes, what)
    dev = torch.device(device)
    if dev.type == "cuda":
        stream = torch.cuda.current_stream(dev).cuda_stream
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), nbytes)
        free = _TRAIN_POOL.get(key)
        if free:
            _TRAIN_POOL.move_to_end(key)
            for i, (t, s) in enumerate(free):
                if s == stream:
                    del free[i]
                    return t
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def pool_give(t) -> None:
    """Hand a training workspace / scratch back (stream-ordered: everything enqueued on the current stream so far may still use it, whatever
    takes it next is enqueued behind).  Called by the backward once it has enqueued its last launch."""
    if t is None or not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 1:
        return
    key = (t.device.index, t.numel())
    free = _TRAIN_POOL.setdefault(key, [])
    _TRAIN_POOL.move_to_end(key)
    if len(free) < _TRAIN_POOL_KEEP:
        free.append((t, torch.cuda.current_stream(t.device).cuda_stream))
    while len(_TRAIN_POOL) > _TRAIN_POOL_SIZES:
        _TRAIN_POOL.popitem(last=False)


def train_workspace(device, n_rays: int, articulated: bool, num_levels: int = 2, st=None) -> torch.Tensor:
    """Workspace of one training forward/backward pair (it carries the forward's planes to the backward, so it is owned by the autograd
    graph until the backward gives it back to the pool: `pool_give`); sized by the levels in use."""
    return _pool_take(int(lib.aon_train_workspace_bytes_ex(n_rays, int(articulated), num_levels, None if st is None else C.byref(st))),
                      "aon_train_workspace_bytes_ex", device)


def _train_scratch(query: str, device, *query_args, st=None) -> torch.Tensor:
    """A backward's temporaries, sized by the C query `query`: taken from the pool when the backward runs and given back right after."""
    return _pool_take(int(getattr(lib, query)(*query_args, None if st is None else C.byref(st))), query, device)


def train_scratch(device, n_rays: int, articulated: bool, num_levels: int = 2, st=None) -> torch.Tensor:
    """The backward's own temporaries (gradient planes, d_raw, weight-gradient partials): taken from the pool when the backward runs and
    given back right after, so a live graph pins the forward's workspace only."""
    return _train_scratch("aon_train_scratch_bytes_ex", device, n_rays, int(articulated), num_levels, st=st)


def render_fwd_train(packed_c, packed_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, small_c=None, small_f=None,
                     opts=None, noise=None):
    """NeRF.forward / NeRF_AE_Art.forward (small blocks given) under grad mode in ONE C call -> (outs, workspace, geometry).
    ``geometry`` = (aon_render_opts struct, tensors it points at): the backward of this forward must be given the same one."""
    art = small_c is not None
    # per-ray near / far: non-differentiable data
    pc = _PathCall(rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise, per_ray=True)
    ws = train_workspace(pc.dev, pc.n, art, num_levels, pc.st)
    packs = (_pk(packed_c), _pk(small_c), _pk(packed_f), _pk(small_f)) if art else (_pk(packed_c), _pk(packed_f))
    stem = "aon_art_render_fwd_train" if art else "aon_render_fwd_train"
    name, extra = (stem + "_ex", ()) if pc.bounds is None else (stem + "_bounds", (C.byref(pc.bounds),))
    with torch.cuda.device(pc.dev):
        check(getattr(lib, name)(*packs, *pc.args(ws), *extra), stem if pc.bounds is None else name)
    return pc.outs, ws, (pc.st, pc.noise_keep)


def _grad_dicts(order, shapes, num_levels, dev, grads_out):
    """Per level {parameter name: tensor the C call writes the gradient into}: fresh tensors, or the caller's (checked: fp32, contiguous,
    right shape and device -- the kernels write every element, 16-byte vector stores included)."""
    if grads_out is None:
        return [{name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in order} for _ in range(num_levels)]
    out = []
    for lvl in range(num_levels):
        d = {}
        for name, t in zip(order, grads_out[lvl]):
            if tuple(t.shape) != tuple(shapes[name]) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or (t.data_ptr() & 15):
                raise ValueError(f"gradient buffer for {name}: expected a contiguous 16-byte aligned float32 {tuple(shapes[name])} tensor on {dev}")
            d[name] = t
        out.append(d)
    return out


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


class _BwdCall:
    """The prologue of every whole-path backward, and the Python side of csrc/aon_capi_util.h's BwdCall: rays_d,
    the per-level g_* pointer arrays, the encoding degrees and aon_render_opts struct of the forward's `geometry`, and the per-level
    parameter arrays (`param_array(params, degrees)` -> (tensors, C array)).  `call` is the C call itself: the network's `packs`, the
    common head, what the network adds (`net`), the common tail for `ws` and `scratch`, `extra`.  The object holds every tensor those
    pointers refer to: keep it until the call has returned."""

    def __init__(self, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry, param_array=None, params_per_level=()):
        self.d = d = _f32(rays_d, "rays_d")
        self.n, self.dev, self.k = d.shape[0], d.device, num_levels
        self.st = st = None if geometry is None else geometry[0]
        self.degrees = (0, 10, 4) if st is None else (int(st.min_deg_point), int(st.max_deg_point), int(st.deg_view))
        made = [param_array(params, self.degrees) for params in params_per_level]
        self._keep = ([m[0] for m in made], [[None if t is None else _f32(t, "grad") for t in g] for g in (g_rgb, g_acc, g_depth)])
        self.parr = self.pad(m[1] for m in made)
        self._head = (_ptr(d), self.n, int(bool(white_bkgd)), num_levels, *(_ptr_array(g) for g in self._keep[1]))

    def pad(self, per_level):
        """per-level entries as the C lists take them: always two, None for a level not in use"""
        return list(per_level) + [None] * (2 - self.k)

    def grad_arrays(self, order, shapes, grads_out=None):
        """-> (per-level dicts the C call writes the parameter gradients into, their two pointer arrays)"""
        grads = _grad_dicts(order, shapes, self.k, self.dev, grads_out)
        return grads, self.pad(_ptr_array([g[nm] for nm in order]) for g in grads)

    def call(self, name, packs, net, ws, scratch, *extra):
        """`scratch` comes from the pool and goes back to it once the call has succeeded (an _ex form reports under the plain name)."""
        with torch.cuda.device(self.dev):
            check(getattr(lib, name)(*packs, *self._head, *net, _ptr(ws), ws.numel(), _ptr(scratch), scratch.numel(), _stream(),
                                     None if self.st is None else C.byref(self.st), *extra), name.removesuffix("_ex"))
        pool_give(scratch)


def render_bwd(ws, packs_bwd, packs_fwd, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry=None, grads_out=None):
    """loss.backward() through render_fwd_train (vanilla): g_* = per-level lists (entries may be None except g_rgb)
    -> per-level dicts of the 24 parameter gradients (shapes of the network's own encoding degrees, read from `geometry`).
    `grads_out`: per level, the 24 tensors to write them into (views of a gradient arena, aon_amd/arena.py) instead of fresh ones."""
    bc = _BwdCall(rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry)
    grads, garr = bc.grad_arrays(VANILLA_PARAM_ORDER, vanilla_param_shapes(bc.degrees), grads_out)
    pb, pf = bc.pad(packs_bwd), bc.pad(packs_fwd)
    bc.call("aon_render_bwd_ex", (_pk(pb[0]), _pk(pf[0]), _pk(pb[1]), _pk(pf[1])), garr, ws,
            train_scratch(bc.dev, bc.n, False, num_levels, bc.st))
    return grads


def train_scratch_inputs_vanilla(device, n_rays: int, num_levels: int = 2, st=None) -> torch.Tensor:
    """The temporaries of the frozen vanilla network's ray-gradient backward (d_raw, gradient planes, one 128-byte record per sample; no
    weight-gradient workspace), pooled as `train_scratch`."""
    return _train_scratch("aon_train_scratch_bytes_inputs_vanilla", device, n_rays, num_levels, st=st)


def _vanilla_input_param_array(params, _degrees):
    """The 24-entry parameter array of aon_render_bwd_inputs from a dict (or an ordered sequence) of the level's parameters: the three
    weights an encoding enters through, in their own nn.Linear layouts; the other entries stay NULL."""
    if isinstance(params, dict):
        params = [params.get(name) for name in VANILLA_PARAM_ORDER]
    params = list(params)
    keep = [_f32(params[i], VANILLA_PARAM_ORDER[i]) if i in (0, 10, 16) else None for i in range(len(VANILLA_PARAM_ORDER))]
    return keep, _ptr_array(keep)


def _ray_grads_call(rays_o, viewdirs, n, dev):
    """-> (g_rays_o, g_rays_d, g_viewdirs) to be written, each (n, 3), and the aon_ray_grads record that points at them and at the rays"""
    g_rays = tuple(torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(3))
    return g_rays, _lib.RayGradsC(rays_o.data_ptr(), viewdirs.data_ptr(), *(g.data_ptr() for g in g_rays))


def render_bwd_inputs(ws, packs_bwd, packs_fwd, rays_o, rays_d, viewdirs, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params, geometry=None):
    """loss.backward() through render_fwd_train of a FROZEN vanilla network, down to its rays -> (g_rays_o, g_rays_d, g_viewdirs), each
    (n, 3), summed over the levels (aon_render_bwd_inputs).  `params`: per level, the network's parameters (a dict
    by name, or the 24 tensors in VANILLA_PARAM_ORDER; only pts_linears.0.weight, pts_linears.5.weight and views_linear.0.weight are read).
    t is data: no gradient through the sampler or near / far.  No parameter gradient is computed or written."""
    ro, vd = _f32(rays_o, "rays_o"), _f32(viewdirs, "viewdirs")
    bc = _BwdCall(rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry, _vanilla_input_param_array, params)
    pb, pf = bc.pad(packs_bwd), bc.pad(packs_fwd)
    g_rays, rg = _ray_grads_call(ro, vd, bc.n, bc.dev)
    bc.call("aon_render_bwd_inputs", (_pk(pb[0]), _pk(pf[0]), _pk(pb[1]), _pk(pf[1])), bc.parr, ws,
            train_scratch_inputs_vanilla(bc.dev, bc.n, num_levels, bc.st), C.byref(rg))
    return g_rays


_LATENT_KEYS = (("density", 128), ("color", 128), ("articulation", 32))


def _art_render_bwd(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, geometry, latents=None,
                    grads_out=None, rays=None, want_latents=True):
    """The three backwards of the articulated network, one body.  `latents` given: the full backward (aon_art_render_bwd_ex) -> (parameter
    gradients, latent gradients); else the frozen network's: latent gradients alone, or with `rays` = (rays_o, viewdirs) -> (latent
    gradients or None, g_rays_o, g_rays_d, g_viewdirs)."""
    rays = None if rays is None else (_f32(rays[0], "rays_o"), _f32(rays[1], "viewdirs"))
    bc = _BwdCall(rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry, _art_param_array, params_per_level)
    n, dev, st = bc.n, bc.dev, bc.st
    pb, sm = bc.pad(packs_bwd), bc.pad(smalls)
    packs = (_pk(pb[0]), _pk(sm[0]), _pk(pb[1]), _pk(sm[1]))
    g_lat = {k: torch.empty(w, device=dev) for k, w in _LATENT_KEYS} if want_latents else None
    lat_ptrs = [None if g_lat is None else _ptr(g_lat[k]) for k, _ in _LATENT_KEYS]
    if latents is not None:
        grads, garr = bc.grad_arrays(ART_PARAM_ORDER, art_param_shapes(bc.degrees), grads_out)
        codes = [_latent(latents, k, w) for k, w in _LATENT_KEYS]
        bc.call("aon_art_render_bwd_ex", packs, (*bc.parr, *(_ptr(t) for t in codes), *garr, *lat_ptrs), ws,
                train_scratch(dev, n, True, num_levels, st))
        return grads, g_lat
    if rays is None:
        bc.call("aon_art_render_bwd_latents", packs, (*bc.parr, *lat_ptrs), ws, train_scratch_latents(dev, n, num_levels, st))
        return g_lat
    g_rays, rg = _ray_grads_call(*rays, n, dev)
    bc.call("aon_art_render_bwd_inputs", packs, (*bc.parr, *lat_ptrs), ws, train_scratch_inputs(dev, n, num_levels, st), C.byref(rg))
    return (g_lat, *g_rays)


def art_render_bwd(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, latents: dict, geometry=None,
                   grads_out=None):
    """Articulated twin -> (per-level dicts of the 40 parameter gradients, dict of latent gradients summed over the levels).
    `grads_out`: as render_bwd."""
    return _art_render_bwd(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, geometry, latents=latents,
                           grads_out=grads_out)


def train_scratch_latents(device, n_rays: int, num_levels: int = 2, st=None) -> torch.Tensor:
    """The latent-only backward's temporaries (gradient planes, d_raw, a few MB of partial sums; no weight-gradient workspace), pooled as
    `train_scratch`."""
    return _train_scratch("aon_train_scratch_bytes_latents", device, n_rays, num_levels, st=st)


def art_render_bwd_latents(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, geometry=None) -> dict:
    """loss.backward() through render_fwd_train of a FROZEN articulated network -> dict of the three latent gradients summed over the
    levels, bit-equal to `art_render_bwd`'s second result for the same workspace and g_*; no parameter gradient is computed or written
    (aon_art_render_bwd_latents)."""
    return _art_render_bwd(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, geometry)


def train_scratch_inputs(device, n_rays: int, num_levels: int = 2, st=None) -> torch.Tensor:
    """`train_scratch_latents` plus the ray gradients' per-sample records (128 B a sample), pooled alike."""
    return _train_scratch("aon_train_scratch_bytes_inputs", device, n_rays, num_levels, st=st)


def art_render_bwd_inputs(ws, packs_bwd, smalls, rays_o, rays_d, viewdirs, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level,
                          geometry=None, want_latents: bool = True):
    """loss.backward() through render_fwd_train of a FROZEN articulated network, down to its inputs -> (dict of the three latent gradients,
    bit-equal to `art_render_bwd_latents`' -- or None when `want_latents` is false: the latent launches are skipped --, g_rays_o, g_rays_d,
    g_viewdirs), each (n, 3), summed over the levels.  t is data: no gradient through the sampler or near / far."""
    return _art_render_bwd(ws, packs_bwd, smalls, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, params_per_level, geometry,
                           rays=(rays_o, viewdirs), want_latents=want_latents)


# ------------------------------------------------------------------ differentiable rays from a camera pose (torch ops on (N, 3): no kernel)
def so3_exp(omega: torch.Tensor) -> torch.Tensor:
    """exp([omega]x), (3,) -> (3, 3), by Rodrigues' formula; differentiable at omega = 0 (the coefficients switch to their Taylor series
    below |omega|^2 = 1e-4, where the closed forms lose their digits and the norm its gradient).  exp(0) is the identity exactly."""
    w = omega.reshape(3)
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    t2 = (w * w).sum()
    small = t2 < 1e-4
    th = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))   # (a safe argument where the series is taken: no 0 * inf in the backward)
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - torch.cos(th)) / (th * th))
    return torch.eye(3, dtype=w.dtype, device=w.device) + a * K + b * (K @ K)


def apply_pose_correction(c2w: torch.Tensor, correction: torch.Tensor) -> torch.Tensor:
    """(3, 4) camera-to-world pose with the 6-vector correction (omega, tau) applied: R = exp([omega]x) R0, t = t0 + tau."""
    c2w = c2w[:3, :4]
    R = so3_exp(correction[:3]) @ c2w[:, :3]
    return torch.cat([R, (c2w[:, 3] + correction[3:6])[:, None]], dim=1)


def rays_from_pose(directions: torch.Tensor, c2w: torch.Tensor, correction: torch.Tensor | None = None):
    """Differentiable `get_rays` (datasets/ray_utils.py:118-159): camera-space directions (..., 3) and a (3, 4) pose -> (rays_o, rays_d),
    both (N, 3); rays_d is normalised and is also the view direction, as the datasets deliver it (pass the SAME tensor as rays_d and as
    viewdirs: autograd then sums the two gradients).  `correction`: see apply_pose_correction.  Plain torch ops on whatever device and
    dtype the inputs have; gradients reach `c2w` and `correction`."""
    pose = c2w[:3, :4] if correction is None else apply_pose_correction(c2w, correction)
    d = directions.reshape(-1, 3) @ pose[:, :3].T
    d = d / torch.norm(d, dim=-1, keepdim=True)
    return pose[:, 3].expand(d.shape), d


# ------------------------------------------------------------------ NeRFMLP of any constructor geometry (csrc/aon_gmlp.hip)
class MlpGeometry:
    """The arguments of ``NeRFMLP.__init__`` (model.py:40-54) -> ``aon_mlp_geometry``; parameter names / shapes / order of the
    module that constructor builds."""

    FIELDS = ("min_deg_point", "max_deg_point", "deg_view", "netdepth", "netwidth", "netdepth_condition", "netwidth_condition",
              "skip_layer", "input_ch", "input_ch_view", "num_rgb_channels", "num_density_channels")
    DEFAULT = (0, 10, 4, 8, 256, 1, 128, 4, 3, 3, 3, 1)

    def __init__(self, min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=8, netwidth=256, netdepth_condition=1,
                 netwidth_condition=128, skip_layer=4, input_ch=3, input_ch_view=3, num_rgb_channels=3, num_density_channels=1):
        vals = (min_deg_point, max_deg_point, deg_view, netdepth, netwidth, netdepth_condition, netwidth_condition, skip_layer, input_ch,
                input_ch_view, num_rgb_channels, num_density_channels)
        for name, v in zip(self.FIELDS, vals):
            setattr(self, name, int(v))
        self.pos_size = ((self.max_deg_point - self.min_deg_point) * 2 + 1) * self.input_ch
        self.view_pos_size = (self.deg_view * 2 + 1) * self.input_ch_view
        st = self.c_struct()
        if lib.aon_gmlp_param_count(C.byref(st)) < 0:     # the C side owns the validity rules
            check(-1, "NeRFMLP geometry")

    def as_tuple(self):
        return tuple(getattr(self, n) for n in self.FIELDS)

    @property
    def is_default(self) -> bool:
        return self.as_tuple() == self.DEFAULT

    @property
    def fits_fused_inference(self) -> bool:
        """Default widths / depths with at most 10 position and 4 view frequency levels: the fused inference kernels take it
        (zero-weight slots for the missing levels, aon_pack_vanilla_mlp_deg)."""
        return (self.as_tuple()[3:] == self.DEFAULT[3:] and 0 <= self.max_deg_point - self.min_deg_point <= 10
                and 0 <= self.deg_view <= 4)

    def c_struct(self):
        st = _lib.MlpGeometryC()
        for n in self.FIELDS:
            setattr(st, n, getattr(self, n))
        return st

    def cat_before(self, l: int) -> bool:
        """layer l reads cat([x, inputs]) (model.py:75-76)"""
        return l >= 2 and (l - 1) % self.skip_layer == 0

    @property
    def param_order(self):
        names = [f"pts_linears.{i}" for i in range(self.netdepth)] + [f"views_linear.{i}" for i in range(self.netdepth_condition)]
        names += ["bottleneck_layer", "density_layer", "rgb_layer"]
        return [f"{m}.{k}" for m in names for k in ("weight", "bias")]

    @property
    def param_shapes(self) -> dict:
        W, Wc, P, V = self.netwidth, self.netwidth_condition, self.pos_size, self.view_pos_size
        out = {}
        for l in range(self.netdepth):
            out[f"pts_linears.{l}.weight"] = (W, P if l == 0 else (W + P if self.cat_before(l) else W))
            out[f"pts_linears.{l}.bias"] = (W,)
        for i in range(self.netdepth_condition):
            out[f"views_linear.{i}.weight"] = (Wc, W + V if i == 0 else Wc)
            out[f"views_linear.{i}.bias"] = (Wc,)
        out.update({"bottleneck_layer.weight": (W, W), "bottleneck_layer.bias": (W,),
                    "density_layer.weight": (self.num_density_channels, W), "density_layer.bias": (self.num_density_channels,),
                    "rgb_layer.weight": (self.num_rgb_channels, Wc), "rgb_layer.bias": (self.num_rgb_channels,)})
        return out


def _gmlp_param_array(geom: MlpGeometry, params: dict):
    shapes = geom.param_shapes
    tensors = []
    for name in geom.param_order:
        t = _f32(params[name].detach(), name)
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {shapes[name]} for NeRFMLP geometry {geom.as_tuple()}")
        tensors.append(t)
    return tensors, (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def gmlp_fwd(geom: MlpGeometry, params: dict, samples_enc, viewdirs_enc):
    """NeRFMLP.forward(x, condition) for any geometry -> (raw_rgb (n,S,C_rgb), raw_density (n,S,C_density))."""
    x, c = _f32(samples_enc, "samples_enc"), _f32(viewdirs_enc, "viewdirs_enc")
    n, S, F = x.shape
    if F != geom.pos_size or tuple(c.shape) != (n, geom.view_pos_size):
        raise ValueError(f"expected samples_enc (n,S,{geom.pos_size}) and viewdirs_enc (n,{geom.view_pos_size})")
    tensors, arr = _gmlp_param_array(geom, params)
    st = geom.c_struct()
    dev = x.device
    rgb = torch.empty((n, S, geom.num_rgb_channels), dtype=torch.float32, device=dev)
    dens = torch.empty((n, S, geom.num_density_channels), dtype=torch.float32, device=dev)
    ws = _sized(int(lib.aon_gmlp_workspace_bytes(C.byref(st), n * S)), "aon_gmlp_workspace_bytes", dev)
    with torch.cuda.device(dev):
        check(lib.aon_gmlp_fwd(C.byref(st), arr, _ptr(x), _ptr(c), n, S, _ptr(rgb), _ptr(dens), _ptr(ws), ws.numel(), _stream()), "aon_gmlp_fwd")
    return rgb, dens


# Workspace of the layer-wise engine's inference call: its activations live in HBM (~ (P + 3 W + 2 Wc) * 4 B per sample) and the C side
# chunks over rays to whatever workspace it is given, so the chunk is sized from a BYTE budget (round 3: a fixed 8,192 rays = ~7 GB
# at 256-wide networks, far more at the widths make_gg accepts, cached per device until release_workspaces(): ADVICE r3).  At 2 GB
# the default-width network gets ~2,400-ray chunks of 193 samples = 460 k-row GEMMs: still hundreds of 128-row tiles per launch.
G_WS_BUDGET_BYTES = 2 << 30
G_CHUNK_RAYS = 8192            # upper bound on rays per chunk
_GWS_CACHE = StreamCache()


def _grender_chunk_rays(gst, st, n: int) -> tuple[int, int]:
    """(rays per chunk, workspace bytes) under G_WS_BUDGET_BYTES; never below 128 rays (then the budget is exceeded, as it must be)."""
    rays = max(1, min(n, G_CHUNK_RAYS))
    while True:
        need = int(lib.aon_grender_workspace_bytes(C.byref(gst), rays, C.byref(st)))
        if need < 0:
            check(need, "aon_grender_workspace_bytes")
        if need <= G_WS_BUDGET_BYTES or rays <= 128:
            return rays, need
        rays = max(128, min(rays // 2, int(rays * G_WS_BUDGET_BYTES / need)))


def _grender_call(geom: MlpGeometry, params_c: dict, params_f, num_levels):
    """-> (aon_mlp_geometry struct, the C prefix of the aon_grender_* forwards, the parameter tensors to keep alive)."""
    gst = geom.c_struct()
    tc, arr_c = _gmlp_param_array(geom, params_c)
    tf, arr_f = _gmlp_param_array(geom, params_f) if num_levels == 2 else (None, None)
    return gst, (C.byref(gst), arr_c, arr_f), (tc, tf)


def grender_fwd(geom: MlpGeometry, params_c: dict, params_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels=2, t_rand=None, u=None,
                opts=None, noise=None):
    """NeRF.forward with a NeRFMLP of any geometry (aon_grender_fwd)."""
    pc = _PathCall(rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise)
    gst, packs, keep = _grender_call(geom, params_c, params_f, num_levels)
    _, need = _grender_chunk_rays(gst, pc.st, pc.n)
    ws = _scratch(_GWS_CACHE, pc.dev, need)
    with torch.cuda.device(pc.dev):
        check(lib.aon_grender_fwd(*packs, *pc.args(ws)), "aon_grender_fwd")
    return pc.outs


def grender_fwd_train(geom: MlpGeometry, params_c: dict, params_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u,
                      opts=None, noise=None):
    """-> (outs, workspace, geometry): the forward of a training step; the workspace carries every layer's output to the backward."""
    pc = _PathCall(rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise)
    gst, packs, keep = _grender_call(geom, params_c, params_f, num_levels)
    ws = _pool_take(int(lib.aon_grender_train_workspace_bytes(C.byref(gst), pc.n, num_levels, C.byref(pc.st))), "aon_grender_train_workspace_bytes",
                    pc.dev)   # (pooled: see _TRAIN_POOL)
    with torch.cuda.device(pc.dev):
        check(lib.aon_grender_fwd_train(*packs, *pc.args(ws)), "aon_grender_fwd_train")
    return pc.outs, ws, (pc.st, pc.noise_keep, pc.uu)


def grender_bwd(geom: MlpGeometry, ws, params_per_level, rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry):
    """loss.backward() through grender_fwd_train -> per-level dicts of parameter gradients."""
    bc = _BwdCall(rays_d, white_bkgd, num_levels, g_rgb, g_acc, g_depth, geometry, lambda params, _: _gmlp_param_array(geom, params), params_per_level)
    gst = geom.c_struct()
    grads, garr = bc.grad_arrays(geom.param_order, geom.param_shapes)
    scratch = _pool_take(int(lib.aon_grender_train_scratch_bytes(C.byref(gst), bc.n, num_levels, C.byref(bc.st))), "aon_grender_train_scratch_bytes", bc.dev)
    bc.call("aon_grender_bwd", (C.byref(gst), *bc.parr), garr, ws, scratch)
    return grads


def release_workspaces() -> None:
    """Drop the per-(device, stream) workspace caches of the inference calls (fused path: up to 1.35 GB, or 3.3 GB with materialised
    encodings; layer-wise engine: G_WS_BUDGET_BYTES = 2 GB; occupancy / early-stop renders; the stage-level weight gradients) back to
    torch's caching allocator.  They are re-made on the next call; and the pool of training workspaces / scratch buffers (`_TRAIN_POOL`:
    up to two of each size in use, 26 GB per pair at 4096 articulated rays).  The per-model packed inference buffers (NeRFMLP._streams)
    belong to their module and are not touched."""
    _TRAIN_POOL.clear()
    for cache in _STREAM_CACHES:     # _WS_CACHE, _GWS_CACHE, _OCC_WS_CACHE, _WG_WS
        cache.clear()


# ------------------------------------------------------------------ measurement aid
def profile_begin() -> None:
    check(lib.aon_profile_begin(), "aon_profile_begin")


def profile_end():
    """-> (mlp_kernel_ms_total, launches, samples) for the fused-MLP launches since profile_begin()."""
    ms, launches, samples = C.c_double(0), C.c_int64(0), C.c_int64(0)
    check(lib.aon_profile_end(C.byref(ms), C.byref(launches), C.byref(samples)), "aon_profile_end")
    return ms.value, launches.value, samples.value


PROF_CLASSES = {"mlp_fwd": 0, "bwd_chain": 1, "wgrad": 2, "composite": 3, "sample_pdf": 4, "composite_bwd": 5, "composite_pdf": 6, "sample_t": 7}


def profile_classes() -> dict:
    """Per kernel class of the interval closed by the last profile_end(): {name: (ms_total, launches, units)}; units are
    samples for mlp_fwd / bwd_chain / wgrad and rays for the per-ray kernels."""
    out = {}
    for name, cls in PROF_CLASSES.items():
        ms, launches, units = C.c_double(0), C.c_int64(0), C.c_int64(0)
        check(lib.aon_profile_class(cls, C.byref(ms), C.byref(launches), C.byref(units)), "aon_profile_class")
        out[name] = (ms.value, launches.value, units.value)
    return out


# ------------------------------------------------------------------ the end of a training step on one parameter arena (csrc/aon_optim.hip)
def adam_step(params_flat, grads_flat, exp_avg, exp_avg_sq, begin: int, count: int, lr: float, beta1: float, beta2: float, eps: float, step: int) -> None:
    """torch.optim.Adam's update (the reference's optimizer: model.py:386-389) on elements [begin, begin + count) of four flat fp32 buffers of
    one layout, ONE launch.  `step` = the count after this update."""
    for name, t in (("params", params_flat), ("grads", grads_flat), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1):
            raise RuntimeError(f"adam_step: {name} must be a flat contiguous float32 cuda tensor (no CPU fallback)")
        if begin < 0 or count < 0 or begin + count > t.numel():
            raise ValueError(f"adam_step: range [{begin}, {begin + count}) outside {name} ({t.numel()} elements)")
    off = 4 * int(begin)
    with torch.cuda.device(params_flat.device):
        check(lib.aon_adam_step(C.c_void_p(params_flat.data_ptr() + off), C.c_void_p(grads_flat.data_ptr() + off), C.c_void_p(exp_avg.data_ptr() + off),
                                C.c_void_p(exp_avg_sq.data_ptr() + off), int(count), float(lr), float(beta1), float(beta2), float(eps), int(step), _stream()),
              "aon_adam_step")


def _code_library_args(tables, ids):
    rows = (C.c_int * 3)(*[int(t.shape[0]) for t in tables])
    dims = (C.c_int * 3)(*[int(t.shape[1]) for t in tables])
    idp = (C.c_void_p * 3)(*[i.data_ptr() for i in ids])
    return rows, dims, idp


def code_library_fwd(tables, ids):
    """CodeLibraryArticulated.forward (code_library.py:36-53) for ids of ONE element each: tables = (shape, appearance, articulation) weight
    matrices, ids = (instance_id, instance_id, articulation_id) int64 device tensors -> three (1, dim) rows, one launch."""
    tabs = [_f32(t, "table") for t in tables]
    idl = [i if (i.dtype == torch.int64 and i.is_cuda) else i.to(device=tabs[0].device, dtype=torch.int64) for i in ids]
    if any(i.numel() != 1 for i in idl):
        raise ValueError("code_library_fwd: one id per table (the reference's batch of one object in one state)")
    outs = [torch.empty((1, t.shape[1]), dtype=torch.float32, device=t.device) for t in tabs]
    rows, dims, idp = _code_library_args(tabs, idl)
    with torch.cuda.device(tabs[0].device):
        check(lib.aon_code_library_fwd(_ptr_array(tabs), idp, rows, dims, _ptr_array(outs), _stream()), "aon_code_library_fwd")
    return outs, idl


def code_library_bwd(g_rows, ids, shapes, outs=None):
    """The dense table gradients of the three lookups (what nn.Embedding's autograd produces), one launch; `outs`: tensors to write into
    (the gradient arena's views) or None."""
    dev = ids[0].device
    gr = [_f32(g, "g_row") if g is not None else torch.zeros((1, shp[1]), dtype=torch.float32, device=dev) for g, shp in zip(g_rows, shapes)]
    if outs is None:
        outs = [torch.empty(tuple(shp), dtype=torch.float32, device=dev) for shp in shapes]
    rows = (C.c_int * 3)(*[int(s[0]) for s in shapes])
    dims = (C.c_int * 3)(*[int(s[1]) for s in shapes])
    idp = (C.c_void_p * 3)(*[i.data_ptr() for i in ids])
    with torch.cuda.device(dev):
        check(lib.aon_code_library_bwd(_ptr_array(gr), idp, rows, dims, _ptr_array(outs), _stream()), "aon_code_library_bwd")
    return outs


# ------------------------------------------------------------------ test-epoch metrics
def ssim(preds, gts, image_sizes=None) -> torch.Tensor:
    """piqa's SSIM() with its defaults for each (pred, gt) pair, both clipped to [0,1] (LitModel.ssim_each, interface.py:102-111), all images in
    one call -> (n,) float32 on the device.  Each image is an (h, w, 3) fp32 cuda tensor, or (h*w, 3) with `image_sizes` = [(h, w), ...]; h, w >= 11
    (the window is applied without padding).  fp64 window statistics and a fixed-order reduction: the same bits on every call and in any batch."""
    preds, gts = list(preds), list(gts)
    if len(preds) != len(gts):
        raise ValueError(f"ssim: {len(preds)} predictions but {len(gts)} targets")
    if image_sizes is not None and len(image_sizes) != len(preds):
        raise ValueError(f"ssim: {len(image_sizes)} image sizes for {len(preds)} images")
    ps, gs, hs, ws = [], [], [], []
    for i, (p, g) in enumerate(zip(preds, gts)):
        p, g = _f32(p, f"preds[{i}]"), _f32(g, f"gts[{i}]")
        if p.shape != g.shape:
            raise ValueError(f"ssim: image {i}: prediction {tuple(p.shape)} and target {tuple(g.shape)} differ")
        if image_sizes is not None:
            h, w = (int(v) for v in image_sizes[i])
        elif p.dim() == 3:
            h, w = int(p.shape[0]), int(p.shape[1])
        else:
            raise ValueError(f"ssim: image {i} has shape {tuple(p.shape)}: give (h, w, 3) images or image_sizes")
        if p.numel() != h * w * 3 or p.shape[-1] != 3:
            raise ValueError(f"ssim: image {i} of shape {tuple(p.shape)} is not an ({h}, {w}, 3) image")
        if g.device != p.device or (ps and p.device != ps[0].device):
            raise ValueError("ssim: images on different devices")
        ps.append(p)
        gs.append(g)
        hs.append(h)
        ws.append(w)
    n = len(ps)
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device="cuda")
    hh, wh = (C.c_int * n)(*hs), (C.c_int * n)(*ws)
    nbytes = int(lib.aon_ssim_workspace_bytes(n, hh, wh))
    if nbytes < 0:
        check(nbytes, "aon_ssim_workspace_bytes")
    dev = ps[0].device
    ws_t = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.aon_ssim(n, _ptr_array(ps), _ptr_array(gs), hh, wh, _ptr(ws_t), nbytes, _ptr(out), _stream()), "aon_ssim")
    return out


# ------------------------------------------------------------------ mesh extraction
def _vec3(v, name: str) -> list:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    if isinstance(v, (int, float)):
        v = [v, v, v]
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError(f"{name}: expected a number or 3 numbers, got {v}")
    return v


def _dims3(dims, name: str = "dims") -> list:
    if isinstance(dims, int):
        dims = (dims, dims, dims)
    dims = [int(d) for d in dims]
    if len(dims) != 3:
        raise ValueError(f"{name}: expected an int or 3 ints, got {dims}")
    return dims


def grid_step(dims, lo, hi):
    """fp32 (lo, step) of an (nx, ny, nz) grid spanning [lo, hi] per axis: step = (hi - lo) / (n - 1) in fp32 (0 for n == 1).  Point
    (i, j, k) lies at lo + idx * step, multiply then add, each rounded to fp32 (grid_points builds the same values)."""
    dims, lo, hi = _dims3(dims), _vec3(lo, "lo"), _vec3(hi, "hi")
    lo32 = torch.tensor(lo, dtype=torch.float32)
    hi32 = torch.tensor(hi, dtype=torch.float32)
    den = torch.tensor([max(n - 1, 1) for n in dims], dtype=torch.float32)
    step = (hi32 - lo32) / den
    step = torch.where(torch.tensor([n > 1 for n in dims]), step, torch.zeros_like(step))
    return lo32, step


def grid_points(dims, lo, hi, g_begin: int = 0, g_end: int | None = None, device="cuda") -> torch.Tensor:
    """(g_end - g_begin, 3) fp32 coordinates of grid points g_begin .. g_end - 1 (C order, k fastest), the values the grid kernels use."""
    dims = _dims3(dims)
    lo32, step = grid_step(dims, lo, hi)
    P = dims[0] * dims[1] * dims[2]
    g_end = P if g_end is None else int(g_end)
    g = torch.arange(int(g_begin), g_end, dtype=torch.int64, device=device)
    idx = torch.stack([g // (dims[1] * dims[2]), (g // dims[2]) % dims[1], g % dims[2]], -1).to(torch.float32)
    return lo32.to(device) + idx * step.to(device)


def density_grid(packed, dims, lo, hi, act: int = ACT_NONE, small=None, g_begin: int = 0, g_end: int | None = None, out=None) -> torch.Tensor:
    """Density of a packed network at the points of an (nx, ny, nz) grid spanning [lo, hi] (grid_points), one fused launch: the trunk of
    mlp_fwd / art_mlp_fwd_pos and the density head, nothing of the view branch.  act 0: raw, 1: relu (vanilla), 2: softplus(raw - 1)
    (articulated).  `small` (art_prepare's per-call block) selects the articulated network.  Vanilla streams must be packed at the default
    degrees (0, 10, 4); NeRF.density_grid routes other geometries to the per-point path.  Returns (nx, ny, nz) for the whole grid, else the
    (g_end - g_begin,) points of the slab (written into `out` when given)."""
    dims = _dims3(dims)
    lo32, step = grid_step(dims, lo, hi)
    P = dims[0] * dims[1] * dims[2]
    whole = g_begin == 0 and (g_end is None or g_end == P)
    g_end = P if g_end is None else int(g_end)
    n = g_end - int(g_begin)
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise RuntimeError("density_grid: packed must be a cuda tensor of ops.pack_vanilla_mlp / ops.pack_art_mlp")
    dev = packed.device
    if out is None:
        out = torch.empty(max(n, 0), dtype=torch.float32, device=dev)
    else:
        out = _f32(out, "out")
        if out.numel() != n:
            raise ValueError(f"density_grid: out holds {out.numel()} values for {n} points")
    d = (C.c_int64 * 3)(*dims)
    lo_h, st_h = (C.c_float * 3)(*lo32.tolist()), (C.c_float * 3)(*step.tolist())
    with torch.cuda.device(dev):
        if small is None:
            check(lib.aon_density_grid(_pk(packed), d, lo_h, st_h, int(g_begin), g_end, int(act), _ptr(out), _stream()), "aon_density_grid")
        else:
            check(lib.aon_art_density_grid(_pk(packed), _pk(small), d, lo_h, st_h, int(g_begin), g_end, int(act), _ptr(out), _stream()),
                  "aon_art_density_grid")
    return out.view(*dims) if whole else out


def marching_cubes(grid, level: float, lo, hi):
    """Marching cubes on an (nx, ny, nz) fp32 cuda grid spanning [lo, hi] (grid_points' coordinates) -> (verts (V, 3) fp32, faces (F, 3) int32).
    Inside is value > level; vertices shared and ordered by (owning grid point, axis), faces by (cell, table order), normals from high values
    to low; the same bits on every call (include/aon_hip.h)."""
    g = _f32(grid, "grid")
    if g.dim() != 3:
        raise ValueError(f"marching_cubes: expected an (nx, ny, nz) grid, got shape {tuple(g.shape)}")
    dims = list(g.shape)
    lo32, step = grid_step(dims, lo, hi)
    d = (C.c_int64 * 3)(*dims)
    nbytes = int(lib.aon_marching_cubes_workspace_bytes(d))
    if nbytes < 0:
        check(nbytes, "aon_marching_cubes_workspace_bytes")
    dev = g.device
    ws = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=dev)
    counts = (C.c_int64 * 2)()
    with torch.cuda.device(dev):
        check(lib.aon_marching_cubes_count(_ptr(g), d, C.c_float(level), _ptr(ws), nbytes, counts, _stream()), "aon_marching_cubes_count")
        V, F = int(counts[0]), int(counts[1])
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        check(lib.aon_marching_cubes(_ptr(g), d, C.c_float(level), (C.c_float * 3)(*lo32.tolist()), (C.c_float * 3)(*step.tolist()), _ptr(ws),
                                     nbytes, _ptr(verts), V, _ptr(faces), F, _stream()), "aon_marching_cubes")
    return verts, faces


# ------------------------------------------------------------------ occupancy-grid accelerated inference
class OccupancyGrid:
    """A bitfield of the cells of a density grid that may hold matter (occupancy_grid): ``bits`` (int32 cuda tensor holding the uint32 words,
    bit c & 31 of word c >> 5 for cell c in C order), ``cells`` (3 ints), fp32 ``lo`` / ``step`` (grid_step's values; the box ends at the last
    grid point lo + cells * step) and the ``threshold`` / ``dilate`` it was built with."""

    def __init__(self, bits: torch.Tensor, cells, lo, step, threshold: float, dilate: int):
        self.bits, self.cells = bits, [int(c) for c in cells]
        self.lo = torch.as_tensor(lo, dtype=torch.float32).cpu()
        self.step = torch.as_tensor(step, dtype=torch.float32).cpu()
        self.threshold, self.dilate = float(threshold), int(dilate)

    @property
    def device(self):
        return self.bits.device

    def c_struct(self):
        st = _lib.OccupancyC()
        st.bits = self.bits.data_ptr()
        for a in range(3):
            st.cells[a], st.lo[a], st.step[a] = self.cells[a], float(self.lo[a]), float(self.step[a])
        return st

    def occupied(self) -> torch.Tensor:
        """(cx, cy, cz) bool tensor of the cells' bits (for inspection and tests)."""
        n = self.cells[0] * self.cells[1] * self.cells[2]
        w = self.bits.to(torch.int64) & 0xFFFFFFFF
        sh = torch.arange(32, device=w.device, dtype=torch.int64)
        b = ((w[:, None] >> sh) & 1).reshape(-1)[:n].to(torch.bool)
        return b.view(*self.cells)

    def occupied_fraction(self) -> float:
        return float(self.occupied().float().mean())


def occupancy_grid(density, lo, hi, threshold: float = 0.01, dilate: int = 1) -> OccupancyGrid:
    """Occupancy bitfield of an ACTIVATED (nx, ny, nz) density grid spanning [lo, hi] (grid_points' coordinates), one launch: a cell (named by
    its lowest corner) is occupied iff one of its 8 corner densities is above `threshold` or NaN, then dilated by `dilate` cells (Chebyshev)."""
    d = _f32(density, "density")
    if d.dim() != 3:
        raise ValueError(f"occupancy_grid: expected an (nx, ny, nz) density grid, got shape {tuple(d.shape)}")
    dims = list(d.shape)
    if min(dims) < 2:
        raise ValueError(f"occupancy_grid: every dimension must be >= 2 (cells = points - 1), got {dims}")
    threshold, dilate = float(threshold), int(dilate)
    if threshold != threshold or not 0 <= dilate <= 8:
        raise ValueError("occupancy_grid: threshold must not be NaN and dilate must be in [0, 8]")
    lo32, step = grid_step(dims, lo, hi)
    if not bool((step > 0).all()):
        raise ValueError(f"occupancy_grid: need lo < hi on every axis, got lo={lo}, hi={hi}")
    cells = [n - 1 for n in dims]
    nbytes = int(lib.aon_occupancy_bytes((C.c_int64 * 3)(*cells)))
    if nbytes < 0:
        check(nbytes, "aon_occupancy_bytes")
    bits = torch.empty(nbytes // 4, dtype=torch.int32, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.aon_occupancy_build(_ptr(d), (C.c_int64 * 3)(*dims), C.c_float(threshold), dilate, _ptr(bits), _stream()), "aon_occupancy_build")
    return OccupancyGrid(bits, cells, lo32, step, threshold, dilate)


_OCC_WS_CACHE = StreamCache()


def _occ_workspace(device, n_rays: int, st, workspace_bytes, query="aon_render_occ_workspace_bytes"):
    """Workspace of the _occ (`query` as given) / _stop / _bounds forms (query aon_render_stop_workspace_bytes)."""
    if workspace_bytes is not None:   # (tests: a workspace small enough to force chunking)
        return torch.empty(int(workspace_bytes), dtype=torch.uint8, device=device)
    need = int(getattr(lib, query)(min(n_rays, MAX_CHUNK_RAYS), C.byref(st)))
    if need < 0:
        check(need, query)
    return _scratch(_OCC_WS_CACHE, device, need)


def render_fwd_occ(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, near, far, white_bkgd, grid: OccupancyGrid, num_levels=2, u=None,
                   opts=None, workspace_bytes=None, ray_live=None):
    """render_fwd (inference: no t_rand, no noise) with every sample in an empty cell of `grid` skipped: zero density, no MLP evaluation.
    Returns (levels, occupied): the level tuples of render_fwd, and an int64 (2,) cuda tensor with the samples each level ran through the MLP.
    Per-ray ``near`` / ``far`` / ``ray_live``: as render_fwd."""
    return _stop_call("aon_render_fwd_occ", (_pk(packed_coarse), _pk(packed_fine)), rays_o, rays_d, viewdirs, near, far, white_bkgd, grid, 0.0, None,
                      num_levels, u, opts, workspace_bytes, ray_live=ray_live)


def art_render_fwd_occ(packed_c, small_c, packed_f, small_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, grid: OccupancyGrid, num_levels=2,
                       u=None, opts=None, workspace_bytes=None, ray_live=None):
    """art_render_fwd with the occupancy skip of render_fwd_occ -> (levels, occupied)."""
    return _stop_call("aon_art_render_fwd_occ", (_pk(packed_c), _pk(small_c), _pk(packed_f), _pk(small_f)), rays_o, rays_d, viewdirs, near, far,
                      white_bkgd, grid, 0.0, None, num_levels, u, opts, workspace_bytes, ray_live=ray_live)


# ------------------------------------------------------------------ early ray termination
DEFAULT_ROUND_SAMPLES = 48   # measured: DESIGN.md section 4.10


def _stop_call(name, packs, rays_o, rays_d, viewdirs, near, far, white_bkgd, grid, eps, round_samples, num_levels, u, opts, workspace_bytes,
               t_rand=None, noise=None, ray_live=None, want_stats=True):
    """The _occ / _stop C calls (`name`: which; the _occ form needs a grid, has no eps / round_samples and returns (levels, occupied)); with
    per-ray near / far tensors or a `ray_live` mask, their common _bounds form (which also serves render_fwd with bounds: no grid and
    eps == 0 without a mask is aon_render_fwd_ex with per-ray planes, t_rand / noise allowed).
    ``want_stats=False`` (render_fwd / art_render_fwd with per-ray planes): no tally, no stop map -- NULL for both, nothing launched for them."""
    occ_form = name.endswith("_occ")
    if not isinstance(grid, OccupancyGrid) and (occ_form or grid is not None):
        raise TypeError(f"{name}: grid must be an ops.OccupancyGrid (ops.occupancy_grid){'' if occ_form else ' or None'}, got {type(grid)}")
    if num_levels not in (1, 2):
        raise ValueError(f"{name}: num_levels must be 1 or 2")
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"{name}: eps must be in [0, 1), got {eps}")
    R = DEFAULT_ROUND_SAMPLES if round_samples is None else int(round_samples)
    if R < 1:
        raise ValueError(f"{name}: round_samples must be >= 1, got {R}")
    per_ray = isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor) or ray_live is not None
    plain = per_ray and grid is None and eps == 0.0 and ray_live is None     # aon_render_fwd_ex with per-ray planes
    pc = _PathCall(rays_o, rays_d, viewdirs, near, far, white_bkgd, num_levels, t_rand, u, opts, noise if plain else None, per_ray=True,
                   ray_live=ray_live)
    n, dev = pc.n, pc.dev
    if grid is not None and grid.device != dev:
        raise ValueError(f"{name}: the grid is on {grid.device}, the rays on {dev}")
    if not plain and (pc.op.noise_std > 0 or t_rand is not None):
        raise ValueError(f"{name}: inference only, density noise (noise_std > 0) and t_rand are refused")
    occ = grid.c_struct() if grid is not None else None
    occupied = torch.zeros(2, dtype=torch.int64, device=dev) if want_stats else None
    extra = (C.byref(occ) if occ is not None else None, _ptr(occupied))
    if occ_form and pc.bounds is None:
        stop, ws = None, _occ_workspace(dev, n, pc.st, workspace_bytes)
    else:
        stop = torch.zeros((n, 2), dtype=torch.int32, device=dev) if want_stats else None
        extra += (C.c_float(eps), R, _ptr(stop))
        if pc.bounds is not None:
            name, extra = name.rsplit("_", 1)[0] + "_bounds", extra + (C.byref(pc.bounds),)
        if plain:
            ws = torch.empty(int(workspace_bytes), dtype=torch.uint8, device=dev) if workspace_bytes is not None else \
                _workspace(dev, n, pc.st, vanilla=name.startswith("aon_render_fwd"))
        else:
            ws = _occ_workspace(dev, n, pc.st, workspace_bytes, "aon_render_stop_workspace_bytes")
    with torch.cuda.device(dev):
        check(getattr(lib, name)(*packs, *pc.args(ws), *extra), name)
    return (pc.outs, occupied) if occ_form else (pc.outs, occupied, stop)


def render_fwd_stop(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, near, far, white_bkgd, grid, eps, round_samples=None, num_levels=2,
                    u=None, opts=None, workspace_bytes=None, ray_live=None):
    """render_fwd_occ with early ray termination: each level runs front to back in rounds of `round_samples` sample indices (default
    DEFAULT_ROUND_SAMPLES) and a ray whose optical depth has reached -ln(eps) after a round is stopped; its remaining samples get zero density
    and never reach the MLP.  `grid` may be None (termination alone); eps == 0 is off (the bits of render_fwd_occ / render_fwd).
    Returns (levels, occupied, stop): the level tuples, the int64 (2,) samples each level ran through the MLP, and the int32 (n, 2) per-level
    stop index of every ray (S of the level: never stopped; a level that was not run: 0)."""
    return _stop_call("aon_render_fwd_stop", (_pk(packed_coarse), _pk(packed_fine)), rays_o, rays_d, viewdirs, near, far, white_bkgd, grid, eps,
                      round_samples, num_levels, u, opts, workspace_bytes, ray_live=ray_live)


def art_render_fwd_stop(packed_c, small_c, packed_f, small_f, rays_o, rays_d, viewdirs, near, far, white_bkgd, grid, eps, round_samples=None,
                        num_levels=2, u=None, opts=None, workspace_bytes=None, ray_live=None):
    """art_render_fwd with the occupancy skip and early termination of render_fwd_stop -> (levels, occupied, stop)."""
    return _stop_call("aon_art_render_fwd_stop", (_pk(packed_c), _pk(small_c), _pk(packed_f), _pk(small_f)), rays_o, rays_d, viewdirs, near, far,
                      white_bkgd, grid, eps, round_samples, num_levels, u, opts, workspace_bytes, ray_live=ray_live)


# ------------------------------------------------------------------ scenes of several posed objects
SCENE_MAX_OBJECTS, SCENE_MAX_MERGED = 16, 4096
_SCENE_WS = StreamCache()


def check_pose(pose, what: str = "pose") -> torch.Tensor:
    """A rigid object-to-world pose -> its (3, 4) fp32 host tensor [R | c].  R must be orthonormal (max |R^T R - I| <= 1e-5) with
    det > 0: there is no scale, so a ray's parameter t means the same distance in every frame."""
    m = torch.as_tensor(pose).detach().to(device="cpu", dtype=torch.float32)
    if tuple(m.shape) != (3, 4):
        raise ValueError(f"{what}: expected a (3, 4) object-to-world matrix, got shape {tuple(m.shape)}")
    R = m[:, :3].double()
    err = float((R.T @ R - torch.eye(3, dtype=torch.float64)).abs().max())
    if not err <= 1e-5:
        raise ValueError(f"{what}: the rotation is not orthonormal (max |R^T R - I| = {err:.3g} > 1e-5; scaled or sheared placements are not supported)")
    if not float(torch.linalg.det(R)) > 0:
        raise ValueError(f"{what}: the rotation has a negative determinant (a reflection)")
    return m.contiguous()


def _scene_objects(objects):
    """[(pose, box) or anything with .pose / .box] -> (aon_scene_object array, K)"""
    objects = list(objects)
    if not 1 <= len(objects) <= SCENE_MAX_OBJECTS:
        raise ValueError(f"a scene holds 1 to {SCENE_MAX_OBJECTS} objects, got {len(objects)}")
    arr = (_lib.SceneObjectC * len(objects))()
    for k, ob in enumerate(objects):
        pose, box = (ob.pose, ob.box) if hasattr(ob, "pose") else ob
        m = check_pose(pose, f"object {k}: pose")
        lo, hi = _box3(box)
        arr[k].rot[:] = m[:, :3].reshape(-1).tolist()
        arr[k].centre[:] = m[:, 3].tolist()
        arr[k].lo[:] = list(lo)
        arr[k].hi[:] = list(hi)
    return arr, len(objects)


class ScenePairs:
    """What aon_scene_pairs wrote for n rays and K objects, the per-pair arrays cut to the P live pairs: `offsets` (K + 1,) int64 on the
    device, `counts` the K segment lengths on the host (read back once: the single synchronisation of a chunk), `slot` (n, K) int32,
    `ray` (P,) int32, `rays_o` / `rays_d` / `viewdirs` (P, 3) in the objects' frames, `near` / `far` (P,).  Object k's rows are
    `segment(k)`.  `capacity`: the same six arrays at the n * K rows they were allocated with (rows from P on are not written)."""

    def __init__(self, n, K, offsets, counts, slot, ray, rays_o, rays_d, viewdirs, near, far):
        self.n, self.K, self.offsets, self.counts, self.slot = n, K, offsets, counts, slot
        self.starts = [sum(counts[:k]) for k in range(K + 1)]
        self.P = P = self.starts[K]
        self.capacity = {"ray": ray, "rays_o": rays_o, "rays_d": rays_d, "viewdirs": viewdirs, "near": near, "far": far}
        self.ray, self.rays_o, self.rays_d, self.viewdirs, self.near, self.far = ray[:P], rays_o[:P], rays_d[:P], viewdirs[:P], near[:P], far[:P]

    def segment(self, k: int) -> slice:
        return slice(self.starts[k], self.starts[k + 1])

    @classmethod
    def without_objects(cls, n: int, device) -> "ScenePairs":
        """The pairs of n rays and NO object (aon_scene_pairs refuses k < 1): K = 0 lists and P = 0 rows, for `with_background`."""
        e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=device)   # noqa: E731
        return cls(int(n), 0, torch.zeros((1,), dtype=torch.int64, device=device), [], e(int(n), 0, dtype=torch.int32), e(0, dtype=torch.int32),
                   e(0, 3), e(0, 3), e(0, 3), e(0), e(0))

    def with_background(self, rays_o, rays_d, viewdirs, near, far) -> "ScenePairs":
        """These pairs with one more list, K, that EVERY ray has (the backdrop): its n rows follow object K - 1's,
        row P + r is world ray r unchanged (`ray` = arange(n), rays_o / rays_d / viewdirs as given) with `near` / `far` as numbers or (n,)
        tensors; `slot` gains the column P + arange(n), `offsets` / `counts` / `starts` one entry, and `segment(K)` is the backdrop.
        Torch operations on the tensors' own device only: no kernel, no host read-back (CPU tensors work)."""
        n, K, P = self.n, self.K, self.P
        dev = self.slot.device
        o, d, v = (x.detach().reshape(-1, 3) for x in (rays_o, rays_d, viewdirs))
        for x, name in ((o, "rays_o"), (d, "rays_d"), (v, "viewdirs")):
            if x.shape[0] != n or x.dtype != torch.float32 or x.device != dev:
                raise ValueError(f"with_background: {name} must be float32 ({n}, 3) on {dev}, got {x.dtype} {tuple(x.shape)} on {x.device}")
        if (P + n) > 0x7fffffff:
            raise ValueError(f"with_background: {P} + {n} rows are more than 2^31 - 1")

        def vec(x, name):
            if not isinstance(x, torch.Tensor):
                return torch.full((n,), float(x), dtype=torch.float32, device=dev)
            t = x.detach().reshape(-1)
            if t.numel() != n or t.dtype != torch.float32 or t.device != dev:
                raise ValueError(f"with_background: a per-ray {name} must be float32 with one value per ray ({n}) on {dev}, got {x.dtype} "
                                 f"{tuple(x.shape)} on {x.device}")
            return t

        nr, fr = vec(near, "near"), vec(far, "far")
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        slot = torch.cat([self.slot, (rows + P)[:, None]], 1).contiguous()
        offsets = torch.cat([self.offsets, self.offsets[-1:] + n])
        return ScenePairs(n, K + 1, offsets, list(self.counts) + [n], slot, torch.cat([self.ray, rows]), torch.cat([self.rays_o, o]),
                          torch.cat([self.rays_d, d]), torch.cat([self.viewdirs, v]), torch.cat([self.near, nr]), torch.cat([self.far, fr]))


def scene_pairs(rays_o, rays_d, viewdirs, objects) -> ScenePairs:
    """Pair every world ray with the objects ([(pose (3, 4) object-to-world, box as ops._box3 takes it)], or scene.SceneObject) whose box
    it crosses, compacted object-major (include/aon_hip_scene.h)."""
    o, d, v = (_f32(x.detach(), nm).reshape(-1, 3) for x, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (viewdirs, "viewdirs")))
    n, dev = o.shape[0], o.device
    if d.shape[0] != n or v.shape[0] != n:
        raise ValueError("rays_o, rays_d and viewdirs must hold the same number of rays")
    arr, K = _scene_objects(objects)
    cap = n * K
    if n == 0:      # nothing to launch (and no pointer to hand over)
        e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
        return ScenePairs(0, K, torch.zeros((K + 1,), dtype=torch.int64, device=dev), [0] * K, e(0, K, dtype=torch.int32), e(0, dtype=torch.int32),
                          e(0, 3), e(0, 3), e(0, 3), e(0), e(0))
    offsets = torch.empty((K + 1,), dtype=torch.int64, device=dev)
    slot = torch.empty((n, K), dtype=torch.int32, device=dev)
    ray = torch.empty((cap,), dtype=torch.int32, device=dev)
    po, pd, pv = (torch.empty((cap, 3), dtype=torch.float32, device=dev) for _ in range(3))
    near, far = (torch.empty((cap,), dtype=torch.float32, device=dev) for _ in range(2))
    ws = _scratch(_SCENE_WS, dev, int(lib.aon_scene_pairs_workspace_bytes(n, K)))
    with torch.cuda.device(dev):
        check(lib.aon_scene_pairs(_ptr(o), _ptr(d), _ptr(v), n, arr, K, _ptr(ws), ws.numel(), _ptr(offsets), _ptr(slot), _ptr(ray), _ptr(po), _ptr(pd),
                                  _ptr(pv), _ptr(near), _ptr(far), _stream()), "aon_scene_pairs")
    starts = offsets.tolist()
    return ScenePairs(n, K, offsets, [starts[k + 1] - starts[k] for k in range(K)], slot, ray, po, pd, pv, near, far)


def scene_composite(raw, t_vals, pairs: ScenePairs, rays_d, white_bkgd, opts=None, want_weights=True, act=ACT_ARTICULATED):
    """Merge the live sample lists of every ray by distance and composite them (include/aon_hip_scene.h): raw (P, S, 4) and t_vals (P, S)
    in `pairs`' row layout, rays_d the WORLD directions (n, 3) -> (rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K), weights (P, S) or None)."""
    d = _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n, K, P, dev = pairs.n, pairs.K, pairs.P, d.device
    t = _f32(t_vals, "t_vals")
    r = _f32(raw, "raw")
    S = t.shape[-1]
    if d.shape[0] != n or tuple(t.shape) != (P, S) or tuple(r.shape) != (P, S, 4):
        raise ValueError(f"scene_composite: expected rays_d ({n}, 3), t_vals ({P}, S) and raw ({P}, S, 4), got {tuple(d.shape)}, {tuple(t.shape)}, {tuple(r.shape)}")
    st, _keep = _opts(opts).c_struct(1.0, 1.0)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc, depth = (torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(2))
    obj_acc = torch.empty((n, K), dtype=torch.float32, device=dev)
    weights = torch.empty((P, S), dtype=torch.float32, device=dev) if want_weights else None
    if n == 0:      # nothing to launch (and no pointer to hand over)
        return rgb, acc, depth, obj_acc, weights
    with torch.cuda.device(dev):
        check(lib.aon_scene_composite(_ptr(r) if P else None, _ptr(t) if P else None, _ptr(pairs.slot), _ptr(d), n, K, P, S, int(bool(white_bkgd)), act,
                                      C.byref(st), _ptr(rgb), _ptr(acc), _ptr(depth), _ptr(obj_acc), _ptr(weights), _stream()), "aon_scene_composite")
    return rgb, acc, depth, obj_acc, weights


class SceneList:
    """How ONE list of a scene's merged composite is read (aon_scene_list, include/aon_hip_scene_lists.h): ``act`` (ACT_*), the
    activation scalars of ``opts`` (a RenderOpts, read for ACT_ARTICULATED only; None: the defaults) and ``open_end`` -- False: the list
    ends where its box ends, True: its last interval is the reference's 1e10 * |d| (a backdrop is opaque where its last sample has density)."""

    def __init__(self, act: int = ACT_ARTICULATED, open_end: bool = False, opts=None):
        if act not in (ACT_NONE, ACT_VANILLA, ACT_ARTICULATED):
            raise ValueError(f"SceneList: act must be 0 (none), 1 (vanilla) or 2 (articulated), got {act!r}")
        self.act, self.open_end, self.opts = int(act), bool(open_end), _opts(opts)

    def fill(self, rec) -> None:
        st, _keep = self.opts.c_struct(1.0, 1.0)      # (the scalars rounded to fp32 exactly as the other calls round them)
        rec.act, rec.open_end = self.act, int(self.open_end)
        rec.rgb_scale, rec.rgb_shift, rec.sigma_bias = st.rgb_scale, st.rgb_shift, st.sigma_bias


def scene_composite_lists(raw, t_vals, pairs: ScenePairs, rays_d, white_bkgd, lists, want_weights=True):
    """scene_composite with one SceneList per list of `pairs` (include/aon_hip_scene_lists.h): each list's samples take ITS activation and
    end rule.  raw (P, S, 4) and t_vals (P, S) in `pairs`' row layout, rays_d the WORLD directions (n, 3)
    -> (rgb (n, 3), acc (n,), depth (n,), obj_acc (n, K), weights (P, S) or None)."""
    d = _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n, K, P, dev = pairs.n, pairs.K, pairs.P, d.device
    t = _f32(t_vals, "t_vals")
    r = _f32(raw, "raw")
    S = t.shape[-1]
    if d.shape[0] != n or tuple(t.shape) != (P, S) or tuple(r.shape) != (P, S, 4):
        raise ValueError(f"scene_composite_lists: expected rays_d ({n}, 3), t_vals ({P}, S) and raw ({P}, S, 4), got {tuple(d.shape)}, {tuple(t.shape)}, "
                         f"{tuple(r.shape)}")
    lists = list(lists)
    if len(lists) != K or not all(isinstance(x, SceneList) for x in lists):
        raise ValueError(f"scene_composite_lists: expected {K} ops.SceneList records, one per list of the pairs")
    if not 1 <= K <= SCENE_MAX_OBJECTS:
        raise ValueError(f"scene_composite_lists: a merged composite takes 1 to {SCENE_MAX_OBJECTS} lists, got {K}")
    arr = (_lib.SceneListC * K)()
    for k, x in enumerate(lists):
        x.fill(arr[k])
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    acc, depth = (torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(2))
    obj_acc = torch.empty((n, K), dtype=torch.float32, device=dev)
    weights = torch.empty((P, S), dtype=torch.float32, device=dev) if want_weights else None
    if n == 0:      # nothing to launch (and no pointer to hand over)
        return rgb, acc, depth, obj_acc, weights
    with torch.cuda.device(dev):
        check(lib.aon_scene_composite_lists(_ptr(r) if P else None, _ptr(t) if P else None, _ptr(pairs.slot), _ptr(d), n, K, P, S, int(bool(white_bkgd)),
                                            arr, _ptr(rgb), _ptr(acc), _ptr(depth), _ptr(obj_acc), _ptr(weights), _stream()),
              "aon_scene_composite_lists")
    return rgb, acc, depth, obj_acc, weights


def scene_composite_bwd(raw, t_vals, pairs: ScenePairs, rays_d, g_rgb, g_acc=None, g_depth=None, g_obj_acc=None, white_bkgd=True, opts=None,
                        act=ACT_ARTICULATED) -> torch.Tensor:
    """The backward of scene_composite on the same raw (P, S, 4), t_vals (P, S), pairs and WORLD rays_d (include/aon_hip_scene_grad.h,
    DESIGN.md section 4.18): upstream gradients g_rgb (n, 3), g_acc / g_depth (n,), g_obj_acc (n, K) -- the last three None for zero --
    -> d_raw (P, S, 4) = dL/d raw.  t, the pairs and rays_d are data: nothing flows to them."""
    d = _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n, K, P, dev = pairs.n, pairs.K, pairs.P, d.device
    t, r, g = _f32(t_vals, "t_vals"), _f32(raw, "raw"), _f32(g_rgb, "g_rgb")
    S = t.shape[-1]
    if d.shape[0] != n or tuple(t.shape) != (P, S) or tuple(r.shape) != (P, S, 4) or tuple(g.shape) != (n, 3):
        raise ValueError(f"scene_composite_bwd: expected rays_d ({n}, 3), t_vals ({P}, S), raw ({P}, S, 4) and g_rgb ({n}, 3), got {tuple(d.shape)}, "
                         f"{tuple(t.shape)}, {tuple(r.shape)}, {tuple(g.shape)}")
    opt = []
    for x, name, shape in ((g_acc, "g_acc", (n,)), (g_depth, "g_depth", (n,)), (g_obj_acc, "g_obj_acc", (n, K))):
        if x is not None:
            x = _f32(x, name)
            if tuple(x.shape) != shape:
                raise ValueError(f"scene_composite_bwd: expected {name} {shape} or None, got {tuple(x.shape)}")
        opt.append(x)
    st, _keep = _opts(opts).c_struct(1.0, 1.0)
    d_raw = torch.zeros((P, S, 4), dtype=torch.float32, device=dev)
    if n == 0 or P == 0:      # nothing to launch (and no pointer to hand over)
        return d_raw
    with torch.cuda.device(dev):
        check(lib.aon_scene_composite_bwd(_ptr(r), _ptr(t), _ptr(pairs.slot), _ptr(d), _ptr(g), _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]), n, K, P, S,
                                          int(bool(white_bkgd)), act, C.byref(st), _ptr(d_raw), _stream()), "aon_scene_composite_bwd")
    return d_raw


def scene_composite_lists_bwd(raw, t_vals, pairs: ScenePairs, rays_d, g_rgb, g_acc=None, g_depth=None, g_obj_acc=None, white_bkgd=True,
                              lists=()) -> torch.Tensor:
    """The backward of scene_composite_lists on the same raw (P, S, 4), t_vals (P, S), pairs, WORLD rays_d and SceneList records
    (include/aon_hip_scene_lists_grad.h): upstream gradients g_rgb (n, 3), g_acc / g_depth (n,), g_obj_acc (n, K)
    -- the last three None for zero -- -> d_raw (P, S, 4) = dL/d raw.  t, the pairs and rays_d are data: nothing flows to them."""
    d = _f32(rays_d.detach(), "rays_d").reshape(-1, 3)
    n, K, P, dev = pairs.n, pairs.K, pairs.P, d.device
    t, r, g = _f32(t_vals, "t_vals"), _f32(raw, "raw"), _f32(g_rgb, "g_rgb")
    S = t.shape[-1]
    if d.shape[0] != n or tuple(t.shape) != (P, S) or tuple(r.shape) != (P, S, 4) or tuple(g.shape) != (n, 3):
        raise ValueError(f"scene_composite_lists_bwd: expected rays_d ({n}, 3), t_vals ({P}, S), raw ({P}, S, 4) and g_rgb ({n}, 3), got "
                         f"{tuple(d.shape)}, {tuple(t.shape)}, {tuple(r.shape)}, {tuple(g.shape)}")
    lists = list(lists)
    if len(lists) != K or not all(isinstance(x, SceneList) for x in lists):
        raise ValueError(f"scene_composite_lists_bwd: expected {K} ops.SceneList records, one per list of the pairs")
    if not 1 <= K <= SCENE_MAX_OBJECTS:
        raise ValueError(f"scene_composite_lists_bwd: a merged composite takes 1 to {SCENE_MAX_OBJECTS} lists, got {K}")
    opt = []
    for x, name, shape in ((g_acc, "g_acc", (n,)), (g_depth, "g_depth", (n,)), (g_obj_acc, "g_obj_acc", (n, K))):
        if x is not None:
            x = _f32(x, name)
            if tuple(x.shape) != shape:
                raise ValueError(f"scene_composite_lists_bwd: expected {name} {shape} or None, got {tuple(x.shape)}")
        opt.append(x)
    arr = (_lib.SceneListC * K)()
    for k, x in enumerate(lists):
        x.fill(arr[k])
    d_raw = torch.zeros((P, S, 4), dtype=torch.float32, device=dev)
    if n == 0 or P == 0:      # nothing to launch (and no pointer to hand over)
        return d_raw
    with torch.cuda.device(dev):
        check(lib.aon_scene_composite_lists_bwd(_ptr(r), _ptr(t), _ptr(pairs.slot), _ptr(d), _ptr(g), _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]), n, K, P, S,
                                                int(bool(white_bkgd)), arr, _ptr(d_raw), _stream()), "aon_scene_composite_lists_bwd")
    return d_raw


def _scene_raw_out(out, P: int, S: int, dev, who: str) -> torch.Tensor:
    """The (P, S, 4) buffer a scene's MLP stage writes: fresh, or the caller's `out` (the first P rows of a larger buffer)."""
    if out is None:
        return torch.empty((P, S, 4), dtype=torch.float32, device=dev)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (P, S, 4) and out.device == dev and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 ({P}, {S}, 4) tensor on {dev}")
    return out


def scene_art_mlp_fwd(packed, smalls, pairs: ScenePairs, t_vals, out=None) -> torch.Tensor:
    """aon_art_mlp_fwd on every object's segment of `pairs` with that object's per-call block (`smalls[k]`, ops.art_prepare) -> one
    (P, S, 4) buffer in the pairs' row layout (``out``: that buffer, to write instead of a fresh one).  An object without a pair costs no
    launch."""
    t = _f32(t_vals, "t_vals")
    if len(smalls) != pairs.K or t.shape[0] != pairs.P:
        raise ValueError(f"scene_art_mlp_fwd: expected {pairs.K} per-call blocks and t_vals of {pairs.P} rows")
    raw = _scene_raw_out(out, pairs.P, t.shape[1], t.device, "scene_art_mlp_fwd")
    for k in range(pairs.K):
        seg = pairs.segment(k)
        if seg.stop > seg.start:
            art_mlp_fwd(packed, smalls[k], pairs.rays_o[seg], pairs.rays_d[seg], pairs.viewdirs[seg], t[seg], out=raw[seg])
    return raw


# ------------------------------------------------------------------ occupancy grids for scenes
_SCENE_OCC_WS = StreamCache()


def scene_art_mlp_fwd_occ(packed, smalls, grids, pairs: ScenePairs, t_vals, out=None):
    """scene_art_mlp_fwd with an optional OccupancyGrid per object (`grids[k]`, in object k's own frame -- the frame of `pairs.rays_o` /
    `pairs.rays_d`; None: dense): a sample in an empty cell of its object's grid gets the record (0, 0, 0, -inf) and never reaches the MLP
    (include/aon_hip_scene_occ.h).  One C call.  -> (raw (P, S, 4), occupied (K,) int64 on the device: the samples of each object that ran
    through the MLP, all of its segment's for a dense object).  With every grid None the bits are scene_art_mlp_fwd's."""
    t = _f32(t_vals, "t_vals")
    K, P, dev = pairs.K, pairs.P, t.device
    grids = list(grids)
    if len(smalls) != K or len(grids) != K or t.dim() != 2 or t.shape[0] != P:
        raise ValueError(f"scene_art_mlp_fwd_occ: expected {K} per-call blocks, {K} grids (or None) and t_vals of {P} rows")
    for k, g in enumerate(grids):
        if g is not None and not isinstance(g, OccupancyGrid):
            raise TypeError(f"scene_art_mlp_fwd_occ: grids[{k}] must be an ops.OccupancyGrid (ops.occupancy_grid) or None, got {type(g)}")
        if g is not None and g.device != dev:
            raise ValueError(f"scene_art_mlp_fwd_occ: grids[{k}] is on {g.device}, the pairs on {dev}")
    S = t.shape[1]
    raw = _scene_raw_out(out, P, S, dev, "scene_art_mlp_fwd_occ")      # (``out``: as scene_art_mlp_fwd)
    occupied = torch.zeros((K,), dtype=torch.int64, device=dev)
    if P == 0:      # nothing to launch (and no pointer to hand over)
        return raw, occupied
    need = int(lib.aon_scene_occ_workspace_bytes(P, K, S))
    if need <= 0:
        raise ValueError(f"scene_art_mlp_fwd_occ: {P} pairs of {S} samples are more than 2^31 - 1 samples: render fewer rays per chunk")
    ws = _scratch(_SCENE_OCC_WS, dev, need)
    structs = [None if g is None else g.c_struct() for g in grids]      # (kept alive until the call has returned)
    grid_arr = (C.c_void_p * K)(*[None if st is None else C.addressof(st) for st in structs])
    small_arr = (C.c_void_p * K)(*[_pk(s).value for s in smalls])
    starts = (C.c_int64 * (K + 1))(*pairs.starts)
    o, d, v = _f32(pairs.rays_o, "pairs.rays_o"), _f32(pairs.rays_d, "pairs.rays_d"), _f32(pairs.viewdirs, "pairs.viewdirs")
    with torch.cuda.device(dev):
        check(lib.aon_scene_art_mlp_fwd_occ(_pk(packed), small_arr, grid_arr, starts, _ptr(o), _ptr(d), _ptr(v), _ptr(t), K, S, _ptr(raw),
                                            _ptr(occupied), _ptr(ws), ws.numel(), _stream()), "aon_scene_art_mlp_fwd_occ")
    return raw, occupied


# ------------------------------------------------------------------ pose gradients of scenes
_RAY_REC = StreamCache()


def art_ray_grads(dplanes, dxp, params: dict, t_vals, viewdirs, degrees=(0, 10, 4)):
    """Stage-level ray gradients of ONE level of ONE block of rays on a frozen articulated network (include/aon_hip_scene_pose.h): dplanes
    and dxp as art_bwd_chain returned them for the block, params the level's 40 parameters, t_vals (n, S) and viewdirs (n, 3) the block's
    own -> (g_rays_o, g_rays_d, g_viewdirs), each (n, 3).  g_rays_d is sum_i t_i g_x_i alone: the norm term of a ray whose own |d| scales
    the compositing is the caller's (a scene has none).  t is data."""
    t, v = _f32(t_vals, "t_vals"), _f32(viewdirs.detach(), "viewdirs").reshape(-1, 3)
    if t.dim() != 2 or v.shape[0] != t.shape[0]:
        raise ValueError(f"art_ray_grads: expected t_vals (n, S) and viewdirs (n, 3), got {tuple(t.shape)} and {tuple(v.shape)}")
    n, S = t.shape
    dev = t.device
    dp, dx = _f32(dplanes, "dplanes"), _f32(dxp, "dxp")
    Np = plane_samples(dp)
    if dp.dim() != 4 or tuple(dx.shape) != (Np, 4):
        raise ValueError(f"art_ray_grads: expected the step-major gradient planes and dxp ({Np}, 4), got {tuple(dp.shape)} and {tuple(dx.shape)}")
    outs = tuple(torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(3))
    if n == 0:      # nothing to launch (and no pointer to hand over)
        return outs
    if S < 1:
        raise ValueError("art_ray_grads: t_vals needs at least one sample per ray")
    tensors, parr = _art_param_array(params, degrees)
    need = int(lib.aon_art_ray_grads_record_bytes(n, S))
    if need < 0:
        raise ValueError(f"art_ray_grads: {n} rays of {S} samples are more than 2^31 - 1 samples")
    rec = _scratch(_RAY_REC, dev, need)
    with torch.cuda.device(dev):
        check(lib.aon_art_ray_grads(_ptr(dp), _ptr(dx), parr, _ptr(t), _ptr(v), n, S, Np, int(degrees[2]), _ptr(rec), rec.numel(), _ptr(outs[0]),
                                    _ptr(outs[1]), _ptr(outs[2]), _stream()), "aon_art_ray_grads")
    return outs


def scene_pose_grads(rays_o, rays_d, viewdirs, pairs: ScenePairs, objects, g_o, g_d, g_v) -> torch.Tensor:
    """The per-pair gradients g_o / g_d / g_v (P, 3) with respect to the pairs' object-frame origins, directions and view directions
    (art_ray_grads on every segment of `pairs`) -> (K, 12): row k = [dL/dR (9, row-major) | dL/dc (3)] of object k's (3, 4) pose, the plain
    derivative with respect to its 12 entries (include/aon_hip_scene_pose.h).  rays_o / rays_d / viewdirs: the WORLD rays `pairs` was built
    from, objects: as scene_pairs took them.  An object without pairs gets zeros."""
    o, d, v = (_f32(x.detach(), nm).reshape(-1, 3) for x, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (viewdirs, "viewdirs")))
    n, K, P, dev = pairs.n, pairs.K, pairs.P, o.device
    gs = [_f32(x, nm) for x, nm in ((g_o, "g_o"), (g_d, "g_d"), (g_v, "g_v"))]
    if any(x.shape[0] != n for x in (o, d, v)) or any(tuple(x.shape) != (P, 3) for x in gs):
        raise ValueError(f"scene_pose_grads: expected world rays ({n}, 3) and per-pair gradients ({P}, 3), got "
                         f"{[tuple(x.shape) for x in (o, d, v)]} and {[tuple(x.shape) for x in gs]}")
    arr, k = _scene_objects(objects)
    if k != K:
        raise ValueError(f"scene_pose_grads: the pairs were built for {K} objects, got {k}")
    g_pose = torch.empty((K, 12), dtype=torch.float32, device=dev)
    some = P > 0
    with torch.cuda.device(dev):
        check(lib.aon_scene_pose_grads(_ptr(o) if some else None, _ptr(d) if some else None, _ptr(v) if some else None, n,
                                       _ptr(pairs.ray) if some else None, _ptr(pairs.offsets), arr, K, P, *(_ptr(x) if some else None for x in gs),
                                       _ptr(g_pose), _stream()), "aon_scene_pose_grads")
    return g_pose
