"""An extended-precision reference of the one-object composite (helper.volumetric_rendering with the activations of the two networks) and of
its derivative with respect to the raw records, and the batch of adversarial rays the CPU and GPU range tests share.

``composite(..., kernel_form=False)`` evaluates in numpy.longdouble with expm1 / log1p: alpha = -expm1(-sigma delta), the transmittance
factor exp(-sigma delta) + 1e-10 (the reference's 1 - alpha + 1e-10 without its cancellation), every sum in long double.  The fp32
operations that are part of the function stay fp32, as in tests/_scene_grad_ref.py with round32=True: delta_i = fl(fl(t[i+1] - t[i]) |d|),
the norm |d| = sqrt(fl(fl(x x + y y) + z z)), fl(raw_sigma + sigma_bias), and the last interval fl(1e10 |d|).  The derivative follows
torch: relu' (0) = 0, softplus with threshold 20 (x > 20: x, derivative 1).

``composite(..., kernel_form=True)`` is the plain float64 restatement of the kernels' own formulas (csrc/aon_composite_grad.h): alpha =
1 - exp(-sigma delta), f = (1 - alpha) + 1e-10, sequential sums -- what a correct fp64 kernel computes before its one rounding to fp32.

acts: 0 = the record is already activated, 1 = sigmoid / relu, 2 = sigmoid * rgb_scale - rgb_shift / softplus(raw + sigma_bias)."""
import numpy as np

F = np.float32
LD = np.longdouble
DEFAULT_OPTS = dict(rgb_padding=0.001, density_bias=-1.0)
SIZES = (1, 2, 65, 193, 300)
N_RAYS = 64


def norm32(d):
    d = np.asarray(d, F)
    return np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)


def norm_candidates(d):
    """The norm as the kernels may hold it.  They take the square root on the hardware's fp32 unit (HIP's __fsqrt_rn is the native
    v_sqrt_f32 unless the correctly rounded device operations are asked for), which is within one ulp of the correctly rounded root:
    the rounded root and its two fp32 neighbours, (3, n); a norm of 0 stays 0.  The bar is held against the FIRST (the reference's norm);
    the other two tell a one-ulp root from any other error: tests/test_hip_composite_range.py admits, as an expected failure, only a ray
    that meets the bar for one of the three, the same for all of its elements."""
    dn = norm32(d)
    lo, hi = np.nextafter(dn, F(0)), np.nextafter(dn, F(np.inf))
    return np.stack([dn, np.where(dn == 0, dn, lo), np.where(dn == 0, dn, hi)]).astype(F)


def intervals32(t, d, dn=None):
    """(n, S) fp32 interval lengths as the kernels form them; the last one is fl(1e10 |d|).  dn: the fp32 norms, if not norm32(d)"""
    t = np.asarray(t, F)
    dn = norm32(d) if dn is None else np.asarray(dn, F)
    out = np.empty_like(t)
    out[:, :-1] = ((t[:, 1:] - t[:, :-1]).astype(F) * dn[:, None]).astype(F)
    with np.errstate(over="ignore"):
        out[:, -1] = (F(1e10) * dn).astype(F)
    return out


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def activate(raw, act, opts, dt):
    """-> colours (n, S, 3), d colour / d raw, sigma (n, S), d sigma / d raw_sigma, all of dtype dt"""
    raw = np.asarray(raw, F)
    c, w = raw[..., :3].astype(dt), raw[..., 3]
    one = dt(1)
    if act == 0:
        return c, np.ones_like(c), w.astype(dt), np.ones(w.shape, dt)
    s = _sigmoid(c)
    if act == 1:
        return s, s * (one - s), np.maximum(w, 0).astype(dt), (w > 0).astype(dt)
    o = DEFAULT_OPTS if opts is None else opts
    scale, shift, bias = dt(F(1 + 2 * o["rgb_padding"])), dt(F(o["rgb_padding"])), F(o["density_bias"])
    xs = (w + bias).astype(F).astype(dt)
    soft = np.where(xs > 20, xs, np.maximum(xs, 0) + np.log1p(np.exp(-np.abs(xs))))
    return s * scale - shift, scale * s * (one - s), soft, np.where(xs > 20, one, _sigmoid(xs))


def composite(raw, t, d, white, act, opts=None, g_rgb=None, g_acc=None, g_depth=None, kernel_form=False, dn=None):
    """-> dict(rgb (n,3), acc, depth (n,), weights (n,S) and, with g_rgb, d_raw (n,S,4)).  kernel_form=False: long double, the truth;
    True: float64 in the kernels' formulas, d_raw rounded to fp32 as a kernel's output is.  dn: see intervals32."""
    dt = np.float64 if kernel_form else LD
    t32 = np.asarray(t, F)
    tt = t32.astype(dt)
    dist = intervals32(t32, d, dn).astype(dt)
    c, dc, sg, dsg = activate(raw, act, opts, dt)
    x = sg * dist
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        ex = np.exp(-x)
        if kernel_form:
            alpha = 1.0 - ex
            f = (1.0 - alpha) + 1e-10
        else:
            alpha = -np.expm1(-x)
            f = ex + dt(1e-10)
        T = np.concatenate([np.ones_like(f[:, :1]), np.cumprod(f[:, :-1], axis=1)], axis=1)
        w = alpha * T
        acc = w.sum(1)
        rgb = (w[..., None] * c).sum(1)
        if white:
            rgb = rgb + (1 - acc)[:, None]
        out = dict(rgb=rgb, acc=acc, depth=(w * tt).sum(1), weights=w)
        if g_rgb is None:
            return out
        gC = np.asarray(g_rgb, F).astype(dt)
        n = t32.shape[0]
        gA = np.zeros(n, dt) if g_acc is None else np.asarray(g_acc, F).astype(dt)
        gD = np.zeros(n, dt) if g_depth is None else np.asarray(g_depth, F).astype(dt)
        const = gA - (gC.sum(1) if white else 0)
        gw = (c * gC[:, None, :]).sum(-1) + const[:, None] + tt * gD[:, None]
        wgw = w * gw
        sfx = np.concatenate([np.cumsum(wgw[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros_like(wgw[:, :1])], axis=1)   # sum over k > i
        dalpha = T * gw - sfx / f
        d_raw = np.concatenate([w[..., None] * gC[:, None, :] * dc, (dalpha * (dist * ex * dsg))[..., None]], axis=-1)
    out["d_raw"] = d_raw.astype(F).astype(np.float64) if kernel_form else d_raw
    return out


def backward_ratio(got, truth):
    """per element |got - truth| / (2^-23 |truth| + 2^-40 max over the ray of |truth|); 0 where both are exactly 0.  got, truth (n, S, 4)."""
    truth = np.asarray(truth, LD)
    err = np.abs(np.asarray(got).astype(LD) - truth)
    bar = LD(2.0) ** -23 * np.abs(truth) + LD(2.0) ** -40 * np.abs(truth).reshape(truth.shape[0], -1).max(1)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, LD(0), err / bar)
    return r.astype(np.float64)


def backward_ratio_any_norm(got, truths):
    """truths: one (n, S, 4) truth per candidate norm -> (n,) the worst ratio of each ray under the candidate that suits it best"""
    per = np.stack([backward_ratio(got, tr).reshape(got.shape[0], -1).max(1) for tr in truths])
    return per.min(0)


# ------------------------------------------------------------------------------------------------ the adversarial rows
def adversarial_batch(S, act, seed=0, opts=None):
    """N_RAYS rays of S samples -> raw (n, S, 4), t (n, S) ascending, d (n, 3), g_rgb (n, 3), g_acc (n,), g_depth (n,), all fp32, and the
    list of row labels.  Everything a row does not set is randn * 3 with t in [2, 6] and a unit direction.  For act 0 the record is the
    act-1 activation of the same raw values (sigmoid / relu in fp64, rounded to fp32).

    Small gradients: the backward bar is relative to the element and to the ray's largest gradient, with no absolute floor, and two things
    cannot meet such a bar on a ray whose EVERY gradient is tiny.  An fp32 output below 1.2e-38 is a denormal and carries fewer than 24
    bits (sigmoid' (+-90) = 8e-40: a ray with all three channels of every sample saturated and no acc / depth gradient has nothing
    larger).  And the kernels' alpha = 1 - exp(-x) in fp64 is 0 for x < 1.1e-16 where the true alpha is x (softplus(-100) = 3.7e-44 over
    the 1e10 interval: x = 3.7e-34), so the colour gradients w gC c' of such a sample come out 0 beside a density gradient of 3.7e-34 g
    that is right.  Neither matters next to any ordinary sample -- the second one is an absolute error below 1.1e-16 |g| -- so the
    saturated colours take two of the three channels and the extreme densities every other sample: each such ray keeps ordinary
    gradients beside them, as a trained field's rays do.  (With S = 1 there is no odd sample: those rows are plain, and labelled so.)
    The same rays WITHOUT that softening are extreme_rows: the forward, finiteness and exact zeros are checked on them."""
    rng = np.random.RandomState(1000 * seed + S)
    n = N_RAYS
    bias = F((DEFAULT_OPTS if opts is None else opts)["density_bias"])
    raw = (rng.randn(n, S, 4) * 3).astype(F)
    t = np.sort(rng.rand(n, S) * 4 + 2, axis=1).astype(F)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    labels = ["plain"] * n
    row = [0]

    def take(label):
        r = row[0]
        assert r < n, "more adversarial rows than rays"
        labels[r] = label
        row[0] += 1
        return r

    raw[take("opaque from the first sample"), :, 3] = 50
    for p in (20, 63, 64, 127, 128, S - 2):
        if 0 <= p <= S - 2:
            raw[take(f"opaque shell at {p}"), p, 3] = 80
    for v in (-5, -30):
        raw[take(f"empty ray {v}"), :, 3] = v
    for v in (0.0, -0.0, 1e-30, -1e-30, 1e-40):
        raw[take(f"raw_sigma {v!r}"), :, 3] = F(v)
    for v in (19.999, 20.0, 20.001, 100.0, -80.0, -100.0):
        # (every other sample: see the note on small gradients; S = 1 has no odd sample, and the row keeps the label of what it is)
        raw[take(f"raw_sigma + bias = {v}" if S > 1 else "plain"), 1::2, 3] = F(v) - bias
    for v in (20, -20, 90, -90):
        raw[take(f"colours {v}"), :, :2] = v                              # (two channels of every sample)
    for v in (1e-20, 0.0, -1e-20, 5.0):
        raw[take(f"last raw_sigma {v!r}"), -1, 3] = F(v)
    for p in (0, S // 2):
        r = take(f"four equal t from {p}")
        t[r, p: p + 4] = t[r, p]
        t[r] = np.sort(t[r])
    for _ in range(4):
        t[take("t log-uniform in [1e-3, 1e3]")] = np.sort(10.0 ** (rng.rand(S) * 6 - 3)).astype(F)
    for scale in (1e-3, 1e3, 0.0):
        for _ in range(2):
            r = take(f"|d| = {scale}")
            d[r] = (d[r].astype(np.float64) * scale).astype(F)
    # combinations: a shell on a log-spaced ray with a long direction; an opaque start under a short one; saturated colours on a shell
    r = take("shell, log t, |d| = 1e3")
    t[r] = np.sort(10.0 ** (rng.rand(S) * 6 - 3)).astype(F)
    d[r] = (d[r].astype(np.float64) * 1e3).astype(F)
    raw[r, S // 2, 3] = 80
    r = take("opaque, |d| = 1e-3")
    raw[r, :, 3] = 50
    d[r] = (d[r].astype(np.float64) * 1e-3).astype(F)
    r = take("shell with colours 90 / -90")
    raw[r, S // 3, 3] = 80
    raw[r, :, :2] = np.where(rng.rand(S, 2) < 0.5, 90, -90)
    if act == 0:
        c64, _, s64, _ = activate(raw, 1, None, np.float64)
        raw = np.concatenate([c64, s64[..., None]], -1).astype(F)
    g_rgb = rng.randn(n, 3).astype(F)
    g_acc = rng.randn(n).astype(F)
    g_depth = (rng.randn(n) * 0.1).astype(F)
    return dict(raw=raw, t=t, d=d, g_rgb=g_rgb, g_acc=g_acc, g_depth=g_depth, labels=labels)


def extreme_rows(S, seed=0):
    """Six rays of S samples, otherwise as adversarial_batch's plain rays: all three colour channels of every sample at 20, -20, 90, -90,
    and raw_sigma + bias = -80, -100 at every sample -> raw, t, d, g_rgb, labels."""
    rng = np.random.RandomState(7000 + 1000 * seed + S)
    n = 6
    raw = (rng.randn(n, S, 4) * 3).astype(F)
    t = np.sort(rng.rand(n, S) * 4 + 2, axis=1).astype(F)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    labels = []
    for r, v in enumerate((20, -20, 90, -90)):
        raw[r, :, :3] = v
        labels.append(f"all colours {v}")
    for r, v in ((4, -80.0), (5, -100.0)):
        raw[r, :, 3] = F(v) - F(DEFAULT_OPTS["density_bias"])
        labels.append(f"every raw_sigma + bias = {v}")
    return dict(raw=raw, t=t, d=d, g_rgb=rng.randn(n, 3).astype(F), labels=labels)


def inf_colour_rows(S=5):
    """Rays with one colour channel at +inf or -inf in every record and an opaque first sample: the forward colour is exactly the
    activation's limit (act 1: 1 / 0; act 2: fl(scale - shift) / -shift), its gradient exactly 0 (sigmoid' = 0 there).  Checked by value,
    outside the truth pipeline."""
    raw = np.zeros((2, S, 4), F)
    raw[..., 3] = 200                       # alpha = 1 at the first sample under relu and softplus
    raw[0, :, 0] = np.inf
    raw[1, :, 0] = -np.inf
    t = np.tile(np.linspace(2, 6, S).astype(F), (2, 1))
    d = np.tile(np.array([[0, 0, 1]], F), (2, 1))
    return dict(raw=raw, t=t, d=d, g_rgb=np.ones((2, 3), F))
