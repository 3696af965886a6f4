"""Image reconstruction quality (csrc/image_quality.hip): PSNR, SSIM, MS-SSIM; float64, forward only."""
import ctypes
import math

import numpy as np
import torch

from .. import hipops as H
from . import _checks as ck

__all__ = ["MS_SSIM_WEIGHTS", "image_quality_window", "image_quality", "image_quality_plan"]


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003, five scales


def image_quality_window(win=11, sigma=1.5):
    """the 1-D window weights in double, summing to 1 (their outer product is the 2-D window): g[i] ~ exp(-(i - (win - 1) / 2)^2
    / (2 sigma^2)), or 1 / win each for sigma None"""
    if sigma is None:
        return np.full(win, 1.0 / win)
    g = np.exp(-((np.arange(win, dtype=np.float64) - (win - 1) / 2.0) ** 2) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def image_quality(x, y, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1, weights=None):
    """How close the images y are to the images x, pair by pair: x, y floating (N, C, H, W), read as fp32, everything after
    the load in float64, one launch, one workgroup per pair (csrc/image_quality.hip; mmvae_hip.h has the arithmetic).
      mse, mae   means of (x - y)^2 and |x - y| over C H W;  psnr = 10 log10(data_range^2 / mse), +inf for mse = 0;
      ssim       Wang et al. 2004: the mean over the C planes of the mean over the (H - win + 1)(W - win + 1) valid window
                 positions (no padding) of l cs, l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), cs = (2 s_xy + C2) /
                 (s_x^2 + s_y^2 + C2), C1 = (k1 data_range)^2, C2 = (k2 data_range)^2, moments under the window: Gaussian
                 of `sigma` (the paper's: win 11, sigma 1.5), or uniform for sigma None; `sample_covariance` scales the
                 (co)variances by win^2 / (win^2 - 1) (scikit-image's default call: win 7, sigma None, sample_covariance True);
      ms_ssim    `scales` = S levels, level s + 1 the 2 x 2 average pooling of level s (needs even sides; every level sides >=
                 win): prod_{s < S} max(cs_s, 0)^w_s max(l_S, 0)^w_S of the image's per-level means (over positions, then
                 channels), clamped at 0 before the powers; S = 1: max(ssim, 0).  `weights` (S,) default to the first S of
                 (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) divided by their sum -- for S < 5 that is NOT the five-scale
                 standard, whose images must have sides >= 16 win;
      levels     (N, S): cs_1 .. cs_{S-1}, l_S.
    -> {"mse", "mae", "psnr", "ssim", "ms_ssim": (N,) float64, "levels": (N, S) float64} on the device.  No map and no pooled
    plane is written, no atomics, every sum in a fixed order: a row's bits do not depend on the other rows of the call.
    win odd in 3 .. 11, win <= H, W <= 64, 1 <= C <= 4, 1 <= S <= 4, finite inputs."""
    who = "image_quality"
    for what, t in (("x", x), ("y", y)):
        ck.floating(who, what, t, 4, "(N, C, H, W) images")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"{who}: x is {tuple(x.shape)} on {x.device}, y {tuple(y.shape)} on {y.device} (pairs of images: the "
                         f"same shape and device)")
    N, C, Hh, W = x.shape
    plan = image_quality_plan((N, C, Hh, W), win, sigma, data_range, k1, k2, sample_covariance, scales, weights)
    ck.need_gpu(who, "x is", x.device)
    x, y = H.f32c(x.detach()), H.f32c(y.detach())
    ck.finite(who, "x", x)
    ck.finite(who, "y", y)
    win, S = plan["win"], plan["scales"]
    out = torch.empty(N, 5 + S, dtype=torch.float64, device=x.device)
    H.call("mmvae_image_quality", H.ptr(x), H.ptr(y), H.ptr(out), N, C, Hh, W, win, (ctypes.c_double * win)(*plan["window"]),
           plan["data_range"], plan["c1"], plan["c2"], plan["cov_scale"], S, (ctypes.c_double * S)(*plan["weights"]), H.stream())
    return {"mse": out[:, 0], "mae": out[:, 1], "psnr": out[:, 2], "ssim": out[:, 3], "ms_ssim": out[:, 4],
            "levels": out[:, 5:]}


def image_quality_plan(shape, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, sample_covariance=False, scales=1,
                       weights=None):
    """image_quality's checks of its arguments against the images' shape (N, C, H, W), before any device call: ValueError, or
    -> {"win", "scales", "window": win doubles, "weights": S doubles, "data_range", "c1", "c2", "cov_scale"}"""
    who = "image_quality"
    N, C, Hh, W = (int(v) for v in shape)
    win, S = int(win), int(scales)
    if not H.IQ_MIN_WIN <= win <= H.IQ_MAX_WIN or win % 2 == 0:
        raise ValueError(f"{who}: win = {win} (odd, {H.IQ_MIN_WIN} .. {H.IQ_MAX_WIN} are on the MI355X path)")
    if not (win <= Hh <= H.IQ_MAX_SIDE and win <= W <= H.IQ_MAX_SIDE):
        raise ValueError(f"{who}: planes of {Hh} x {W} for win = {win} (sides of win .. {H.IQ_MAX_SIDE} are on the MI355X path)")
    if not 1 <= C <= H.IQ_MAX_CHANNELS or not 1 <= N <= H.IQ_MAX_ROWS:
        raise ValueError(f"{who}: {N} images of {C} channels (at least one image, 1 .. {H.IQ_MAX_CHANNELS} channels are on the "
                         f"MI355X path)")
    if not 1 <= S <= H.IQ_MAX_SCALES:
        raise ValueError(f"{who}: scales = {S} (1 .. {H.IQ_MAX_SCALES} are on the MI355X path)")
    h, w = Hh, W
    for level in range(2, S + 1):
        if h % 2 or w % 2:
            raise ValueError(f"{who}: level {level - 1} is {h} x {w}; pooling it into level {level} needs even sides")
        h, w = h // 2, w // 2
        if h < win or w < win:
            raise ValueError(f"{who}: level {level} is {h} x {w}, smaller than win = {win} ({Hh} x {W} images allow scales <= "
                             f"{level - 1})")
    if sigma is not None and not (math.isfinite(float(sigma)) and float(sigma) > 0.0):
        raise ValueError(f"{who}: sigma = {sigma} (a positive width, or None for the uniform window)")
    L, k1, k2 = float(data_range), float(k1), float(k2)
    if not (math.isfinite(L) and L > 0.0 and math.isfinite(k1) and k1 > 0.0 and math.isfinite(k2) and k2 > 0.0):
        raise ValueError(f"{who}: data_range = {data_range}, k1 = {k1}, k2 = {k2} (positive and finite)")
    if weights is None:
        msw = np.asarray(MS_SSIM_WEIGHTS[:S], dtype=np.float64)
        msw = msw / msw.sum()
    else:
        msw = np.asarray(weights.detach().cpu().double().numpy() if torch.is_tensor(weights) else weights,
                         dtype=np.float64).reshape(-1)
        if msw.shape[0] != S or not np.all(np.isfinite(msw)) or np.any(msw < 0.0):
            raise ValueError(f"{who}: weights holds {msw.shape[0]} values for scales = {S} (one finite exponent >= 0 per level)")
    return {"win": win, "scales": S, "window": image_quality_window(win, sigma).tolist(), "weights": msw.tolist(),
            "data_range": L, "c1": (k1 * L) ** 2, "c2": (k2 * L) ** 2,
            "cov_scale": win * win / (win * win - 1.0) if sample_covariance else 1.0}
