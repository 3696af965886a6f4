"""Float64 numpy restatement of the image reconstruction quality, written from the formulae: direct 2-D
window sums over every valid position (no separable filter, no ring, no shortcut shared with csrc/image_quality.hip), the pooled
levels as strided slices, and beside every value the bound on what float64 rounding can do to it, from its own denominators.

  u = 2^-53, X = max(|x|, |y|, L) of the image pair, gamma = (win^2 + 8) u X^2: the error of a filtered moment in either
  summation order, pooling included; at most 3 gamma f lands in each of var_x, var_y, cov.  Both quotients have |N| <= D, so a
  position's l cs (and l, and cs) is off by at most 12 f gamma (1 / D_l + 1 / D_cs); `bound` is the mean of that over a plane's
  positions and an image's planes.  The tests hold ssim and the level values to 4 x bound;
  mse to 4 C H W u X^2 and mae to 4 C H W u X (n rounded additions of terms <= (2 X)^2 resp. 2 X, and the division);
  psnr through d psnr = (10 / ln 10) d mse / mse, + 4 u |psnr| for the logarithm and the product;
  ms_ssim through ms sum_s w_s d_s / v_s (d_s the bar of level s, v_s its clamped value), + 4 (S + 1) u ms for the powers and
  their product -- meaningful where every v_s is well above 0, which the tests assert (>= 0.05) before they use it."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 2.0 ** -53
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
NAMES = ("mse", "mae", "psnr", "ssim", "ms_ssim", "levels")


def window(win, sigma):
    """the 2-D window, normalised to sum 1: the outer product of a Gaussian with itself, or uniform for sigma None"""
    if sigma is None:
        return np.full((win, win), 1.0 / (win * win))
    i = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    w = np.outer(g, g)
    return w / w.sum()


def pool(a):
    """2 x 2 average pooling of (N, C, h, w), even h and w"""
    assert a.shape[2] % 2 == 0 and a.shape[3] % 2 == 0, a.shape
    return 0.25 * (a[:, :, 0::2, 0::2] + a[:, :, 0::2, 1::2] + a[:, :, 1::2, 0::2] + a[:, :, 1::2, 1::2])


def level_terms(a, b, w, f, c1, c2, gamma):
    """one level of (N, C, h, w) pairs -> the images' (ssim, cs, l, bound), (N,) each: means over positions, then channels;
    gamma (N,)"""
    wa, wb = (sliding_window_view(t, w.shape, axis=(2, 3)) for t in (a, b))
    mx, my = (wa * w).sum((-1, -2)), (wb * w).sum((-1, -2))
    xx, yy, xy = (wa * wa * w).sum((-1, -2)), (wb * wb * w).sum((-1, -2)), (wa * wb * w).sum((-1, -2))
    vx, vy, cxy = f * (xx - mx * mx), f * (yy - my * my), f * (xy - mx * my)
    d_l, d_cs = mx * mx + my * my + c1, vx + vy + c2
    l, cs = (2.0 * mx * my + c1) / d_l, (2.0 * cxy + c2) / d_cs
    bound = 12.0 * f * gamma[:, None, None, None] * (1.0 / d_l + 1.0 / d_cs)
    return tuple(t.mean((2, 3)).mean(1) for t in (l * cs, cs, l, bound))


def image_quality(x, y, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1, weights=None):
    """x, y (N, C, H, W) -> {"mse", "mae", "psnr", "ssim", "ms_ssim": (N,), "levels": (N, S), "values": (N, S) the clamped
    level values, "bar": {the same names: what a float64 implementation may differ by}}"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 4
    N, C, H, W = x.shape
    L, S = float(data_range), int(scales)
    f = win * win / (win * win - 1.0) if sample_covariance else 1.0
    c1, c2, w = (k1 * L) ** 2, (k2 * L) ** 2, window(win, sigma)
    ms_w = np.asarray(MS_WEIGHTS[:S] if weights is None else weights, dtype=np.float64)
    ms_w = ms_w / ms_w.sum() if weights is None else ms_w
    assert ms_w.shape == (S,)
    X = np.maximum(np.maximum(np.abs(x).max((1, 2, 3)), np.abs(y).max((1, 2, 3))), L)
    gamma = (win * win + 8) * U * X * X
    d = x - y
    mse, mae = (d * d).mean((1, 2, 3)), np.abs(d).mean((1, 2, 3))
    with np.errstate(divide="ignore"):
        psnr = np.where(mse > 0.0, 10.0 * np.log10(L * L / np.where(mse > 0.0, mse, 1.0)), np.inf)
    bar = {"mse": 4.0 * C * H * W * U * X * X, "mae": 4.0 * C * H * W * U * X}
    with np.errstate(divide="ignore", invalid="ignore"):
        bar["psnr"] = np.where(mse > 0.0, (10.0 / np.log(10.0)) * bar["mse"] / mse + 4.0 * U * np.abs(psnr), 0.0)
    levels, bounds, a, b = [], [], x, y
    for s in range(S):
        assert min(a.shape[2:]) >= win, f"level {s + 1} is {a.shape[2:]}"
        ssim_s, cs_s, l_s, bound_s = level_terms(a, b, w, f, c1, c2, gamma)
        if s == 0:
            ssim, bar["ssim"] = ssim_s, 4.0 * bound_s
        levels.append(cs_s if s + 1 < S else l_s)
        bounds.append(4.0 * bound_s)
        if s + 1 < S:
            a, b = pool(a), pool(b)
    levels, bar["levels"] = np.stack(levels, 1), np.stack(bounds, 1)
    if S == 1:
        values = np.maximum(ssim, 0.0)[:, None]
        ms, bar["ms_ssim"] = values[:, 0], bar["ssim"]
    else:
        values = np.maximum(levels, 0.0)
        ms = np.prod(values ** ms_w[None, :], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            bar["ms_ssim"] = ms * (ms_w[None, :] * bar["levels"] / values).sum(1) + 4.0 * (S + 1) * U * ms
    return {"mse": mse, "mae": mae, "psnr": psnr, "ssim": ssim, "ms_ssim": ms, "levels": levels, "values": values, "bar": bar}


# ---- the cases the GPU tests share: (N, C, H, W, keyword arguments), computed once and left unchanged ---------------------------
CASES = (
    (1, 1, 11, 11, dict(win=11)),                                                         # one position
    (5, 1, 12, 17, dict(win=3)),                                                          # non-square, smallest window
    (7, 3, 28, 28, dict(win=7, sigma=None, sample_covariance=True, data_range=255.0)),    # scikit-image's default call
    (6, 1, 28, 28, dict(win=11, scales=2)),
    (5, 3, 32, 32, dict(win=11, scales=2)),
    (4, 3, 64, 64, dict(win=11, scales=3)),                                               # the largest plane, every level
    (300, 3, 16, 16, dict(win=5)),                                                        # more planes than CUs
    (2, 2, 64, 64, dict(win=7, scales=4)),                                                # the deepest pyramid
    (3, 4, 40, 24, dict(win=9, sigma=2.0, k1=0.02, k2=0.05, scales=2, weights=(0.3, 0.7))),
    (2, 1, 64, 20, dict(win=5, sigma=None)),                                              # one long side
)
IDS = tuple("{}x{}x{}x{}w{}S{}".format(n, c, h, w, k["win"], k.get("scales", 1)) for n, c, h, w, k in CASES)
MANY = 6
NOISE = (0.02, 0.2)      # the two noise levels: even rows, odd rows


@functools.lru_cache(maxsize=None)
def case(i):
    """-> (x, y fp32 (N, C, H, W), read-only; the keyword arguments; the restatement of the pair)"""
    N, C, H, W, kw = CASES[i]
    rs = np.random.RandomState(100 + i)
    L = kw.get("data_range", 1.0)
    x = rs.uniform(0.0, 1.0, (N, C, H, W))
    sd = np.asarray([NOISE[n % 2] for n in range(N)])[:, None, None, None]
    y = np.clip(x + sd * rs.standard_normal(x.shape), 0.0, 1.0)
    x, y = (np.ascontiguousarray(t * L, dtype=np.float32) for t in (x, y))
    ref = image_quality(x, y, **kw)
    for t in (x, y) + tuple(ref[n] for n in NAMES) + tuple(ref["bar"].values()):
        t.setflags(write=False)
    return x, y, dict(kw), ref


def anti_correlated(N=3, H=28, W=28, seed=7):
    """a high-contrast binary plane and its negative: cov = -var, the mean cs of level 1 is negative, ms_ssim is exactly 0"""
    x = (np.random.RandomState(seed).uniform(size=(N, 1, H, W)) < 0.5).astype(np.float32)
    return x, (1.0 - x).astype(np.float32)
