"""Float64 references, error bounds and an fp32 emulation for the kernels of csrc/optim.hip (numpy only, no GPU).

Scalars.  The C ABI takes lr, the betas, eps and grad_scale of the Adam launches as `float`; the kernel forms the gain as
`1.0f - b` (exact for b in [0.5, 1]) and the bias corrections from pow((double)b_float, step).  So the reference is Adam
with every scalar rounded to fp32 first: B = float(np.float32(beta)) throughout -- self-consistent, and what
torch.optim.Adam(betas=(B1, B2)) computes in float64 (tests/test_optim_reference_host.py pins that to 1e-12).  AdaBelief
takes its betas as double: decay float32(beta), gain float32(1.0 - beta) formed in double (comment above
adabelief_update1), bias corrections from pow(double(float32(beta)), step), eps added to the stored s.

Error scales.  u = 2^-24 (fp32 unit roundoff).  Every bound is per element and relative to the magnitude of the TERMS that
were added, never to a tensor maximum or to the value itself.  Counting roundings of the update as the kernel spells it
(gr = g gscale; m = fma(b1, m0, (1-b1) gr); v = fma(b2, v0, ((1-b2) gr) gr); x = max(x0, v); den = fma(sqrt(x), 1/sqrt(bc2),
eps); p = p0 - (lr/bc1 m) / den):
  m    : 3 roundings (gr, the product, the fma)                       -> 3u (|B1 m0| + |(1-B1) gr|)            = 3u Tm
  v    : gr twice (2), two products, the fma                          -> 5u (B2 v0 + (1-B2) gr^2)              = 5u Tv
  vmax : |max(a, b) - max(a, c)| <= |b - c|, and Tv <= vmax            -> 5u vmax
  p    : m (3u of Tm), lr/bc1 -> float (1), its product with m (1), sqrt(x) (2.5 from x + 1), 1/sqrt(bc2) -> float (1),
         the fma (1), the quotient (1) = 11.5, and the final subtraction -> 1/2 ulp(max(|p0|, |p1|)) + 12u S,
         S = (lr/bc1) Tm / den
  sums of R terms in any order: every partial sum is bounded by sum|terms| and there are R - 1 additions
                                                                      -> (R + 1) u sum|terms| per column
RE-DERIVED (the relative bounds above are wrong in the subnormal range): a result below 2^-126 is rounded to a multiple of
2^-149, an ABSOLUTE error of up to 2^-150 per rounding whatever its size.  g = 1e-20 gives (1-b2) gr^2 ~ 1e-43, about 70
subnormal steps: no correct fp32 update can hold 5u of that.  Every bound therefore carries `roundings x 2^-149` as an
absolute floor (TINY below); it is 1e-38 times smaller than any normal-range bound and changes nothing there.

A gradient that is itself a rounded sum (the fused fold + Adam launch) enters with its own error Eg = (R + 2) u sum|terms|
(partial rows + the direct contribution); it is carried through to first order plus the square in v:
  m += (1-B1) gs Eg;  v, vmax += (1-B2) (2 |gr| gs Eg + (gs Eg)^2);
  p += (lr/bc1) (1-B1) gs Eg / den + S dden / den,  dden = min(dx / sqrt(x), sqrt(dx)) / sqrt(bc2)
  (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= both).

AdaBelief (d = gr - m; s = fma(b2, s0, (g2 d) d) + eps): m as above with gain G1 = float32(1 - beta1);
  d    : inherits m's error and gr's rounding, plus its own: Ed = 3u Tm + u |gr| + u |d|
  s    : two products, the fma and the addition of eps (4u of B2 s0 + G2 d^2 + eps) plus what Ed does to G2 d^2
         -> 4u Ts + G2 (2 |d| Ed + Ed^2)
  p    : as Adam's with den's error written out: 1/2 ulp + S (7u + dden/den), dden = ds / (2 sqrt(s)) / sqrt(bc2) + 3u den
         (s >= eps > 0, so the first-order form is safe; m 3, lr/bc1 1, product 1, quotient 1, slack 1 = 7).

Measured with the fp32 emulation below (emulate_adam / emulate_adabelief: numpy float32, fused multiply-adds where the
kernel has them, double-precision bias corrections) on the inputs the GPU tests use (adam_case, every size up to
4 202 499, both states, gscale 1, 0.5, 1/3, steps 1, 7, 42, 43), as a multiple of u times the scale named above --
tests/test_optim_reference_host.py asserts the bounds and prints these:
  Adam     : m 2.32u (bound 3), v 3.43u (5), vmax 3.43u (5), p beyond its 1/2 ulp: 3.82u of S (12)
  AdaBelief: m 2.43u (3), s 0.56 of its bound, p beyond its 1/2 ulp: 0.26 of the rest of its bound
  fold (rows added one by one in fp32) + Adam: m 0.51, v and vmax 0.43 of the propagated bound, p inside it
  edge gradients 0, 1e-20, 1e15 (step 1 from zero state): inside the same bounds WITH the TINY floor; without it v misses
  at g = 1e-20 (emulated error 8.5e4 u of Tv: the subnormal spacing), which is why the floor is there.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149          # spacing of fp32 subnormals: the absolute error of one rounding below 2^-126


def f32(x):
    """a Python float that holds the fp32 rounding of x (how a `float` argument of the C ABI arrives)"""
    return float(np.float32(x))


def _d(a):
    return np.asarray(a, dtype=np.float64)


def ulp32(x):
    """spacing of fp32 at |x| (float64 array)"""
    return _d(np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)))


# ---- Adam (amsgrad) --------------------------------------------------------------------------------------------------
def _adam_scalars(lr, b1, b2, eps, step, gscale):
    B1, B2 = f32(b1), f32(b2)
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    return B1, B2, f32(lr), f32(eps), f32(gscale), bc1, bc2


def adam_amsgrad_step(p, g, m, v, vmax, lr, b1, b2, eps, step, gscale=1.0):
    """one torch.optim.Adam(amsgrad=True) step (1-based `step`) in float64 from fp32 inputs -> (p, m, v, vmax)"""
    B1, B2, lr, eps, gs, bc1, bc2 = _adam_scalars(lr, b1, b2, eps, step, gscale)
    p, g, m, v, vmax = map(_d, (p, g, m, v, vmax))
    gr = g * gs
    m1 = B1 * m + (1.0 - B1) * gr
    v1 = B2 * v + (1.0 - B2) * gr * gr
    x1 = np.maximum(vmax, v1)
    den = np.sqrt(x1) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m1 / den, m1, v1, x1


def adam_bounds(p, g, m, v, vmax, lr, b1, b2, eps, step, gscale=1.0, g_err=None):
    """per-element bounds {p, m, v, vmax} of an fp32 Adam step against adam_amsgrad_step (module docstring); g_err: the
    absolute error of a gradient that is itself a rounded sum.  Also "S", "Tm", "Tv": the scales, for reporting."""
    B1, B2, lr, eps, gs, bc1, bc2 = _adam_scalars(lr, b1, b2, eps, step, gscale)
    p0, g, m0, v0, x0 = map(_d, (p, g, m, v, vmax))
    p1, m1, v1, x1 = adam_amsgrad_step(p, g, m, v, vmax, lr, b1, b2, eps, step, gscale)
    gr = g * gs
    Tm = np.abs(B1 * m0) + np.abs((1.0 - B1) * gr)
    Tv = B2 * v0 + (1.0 - B2) * gr * gr
    den = np.sqrt(x1) / np.sqrt(bc2) + eps
    S = (lr / bc1) * Tm / den
    out = {"m": 3 * U * Tm + 3 * TINY, "v": 5 * U * Tv + 5 * TINY, "vmax": 5 * U * x1 + 5 * TINY,
           "p": 0.5 * ulp32(np.maximum(np.abs(p0), np.abs(p1))) + 12 * U * S + 12 * TINY, "S": S, "Tm": Tm, "Tv": Tv}
    if g_err is not None:
        eg = _d(g_err) * gs
        dm = (1.0 - B1) * eg
        dv = (1.0 - B2) * (2.0 * np.abs(gr) * eg + eg * eg)
        with np.errstate(divide="ignore", invalid="ignore"):
            dsq = np.minimum(np.where(x1 > 0, dv / np.sqrt(x1), np.inf), np.sqrt(dv))
        dden = dsq / np.sqrt(bc2)
        out["m"] = out["m"] + dm
        out["v"] = out["v"] + dv
        out["vmax"] = out["vmax"] + dv
        out["p"] = out["p"] + (lr / bc1) * dm / den + S * dden / den
    return out


def _fma32(a, b, c):
    # the product of two fp32 is exact in double; one double addition, then one rounding to fp32
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate_adam(p, g, m, v, vmax, lr, b1, b2, eps, step, gscale=1.0):
    """adam_update1 of csrc/optim.hip in numpy float32, operation by operation -> (p, m, v, vmax) float32"""
    F = np.float32
    b1, b2, eps, gs = F(b1), F(b2), F(eps), F(gscale)
    lr_bc1 = F(np.float64(F(lr)) / (1.0 - np.float64(b1) ** step))
    isb = F(1.0 / np.sqrt(1.0 - np.float64(b2) ** step))
    P, G, M, V, X = (np.asarray(a, dtype=F) for a in (p, g, m, v, vmax))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        gr = G * gs
        M = _fma32(b1, M, (F(1.0) - b1) * gr)
        V = _fma32(b2, V, ((F(1.0) - b2) * gr) * gr)
        X = np.maximum(X, V)
        den = _fma32(np.sqrt(X), isb, eps)
        P = P - (lr_bc1 * M) / den
    return P, M, V, X


# ---- AdaBelief ---------------------------------------------------------------------------------------------------------
def _belief_scalars(lr, b1, b2, eps, step, gscale):
    B1, B2 = f32(b1), f32(b2)
    return B1, B2, f32(1.0 - b1), f32(1.0 - b2), f32(lr), f32(eps), f32(gscale), 1.0 - B1 ** step, 1.0 - B2 ** step


def adabelief_step(p, g, m, s, lr, b1, b2, eps, step, gscale=1.0):
    """one AdaBelief step (eps inside the stored s, no rectification, no weight decay) in float64 -> (p, m, s)"""
    B1, B2, G1, G2, lr, eps, gs, bc1, bc2 = _belief_scalars(lr, b1, b2, eps, step, gscale)
    p, g, m, s = map(_d, (p, g, m, s))
    gr = g * gs
    m1 = B1 * m + G1 * gr
    d = gr - m1
    s1 = B2 * s + G2 * d * d + eps
    den = np.sqrt(s1) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m1 / den, m1, s1


def adabelief_bounds(p, g, m, s, lr, b1, b2, eps, step, gscale=1.0):
    B1, B2, G1, G2, lr, eps, gs, bc1, bc2 = _belief_scalars(lr, b1, b2, eps, step, gscale)
    p0, g, m0, s0 = map(_d, (p, g, m, s))
    p1, m1, s1 = adabelief_step(p, g, m, s, lr, b1, b2, eps, step, gscale)
    gr = g * gs
    Tm = np.abs(B1 * m0) + np.abs(G1 * gr)
    d = gr - m1
    Ed = 3 * U * Tm + U * np.abs(gr) + U * np.abs(d) + 5 * TINY
    Ts = B2 * s0 + G2 * d * d + eps
    ds = 4 * U * Ts + G2 * (2.0 * np.abs(d) * Ed + Ed * Ed) + 4 * TINY
    den = np.sqrt(s1) / np.sqrt(bc2) + eps
    dden = ds / (2.0 * np.sqrt(s1)) / np.sqrt(bc2) + 3 * U * den
    S = (lr / bc1) * Tm / den
    return {"m": 3 * U * Tm + 3 * TINY, "s": ds,
            "p": 0.5 * ulp32(np.maximum(np.abs(p0), np.abs(p1))) + S * (7 * U + dden / den) + 12 * TINY, "S": S, "Tm": Tm,
            "p_rel": S * (7 * U + dden / den)}


def emulate_adabelief(p, g, m, s, lr, b1, b2, eps, step, gscale=1.0):
    """adabelief_update1 + the host wrapper's scalar conversions in numpy float32 -> (p, m, s) float32"""
    F = np.float32
    fb1, fb2, g1, g2, eps, gs = F(b1), F(b2), F(1.0 - b1), F(1.0 - b2), F(eps), F(gscale)
    lr_bc1 = F(np.float64(F(lr)) / (1.0 - np.float64(fb1) ** step))
    isb = F(1.0 / np.sqrt(1.0 - np.float64(fb2) ** step))
    P, G, M, S = (np.asarray(a, dtype=F) for a in (p, g, m, s))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        gr = G * gs
        M = _fma32(fb1, M, g1 * gr)
        d = gr - M
        S = _fma32(fb2, S, (g2 * d) * d) + eps
        den = _fma32(np.sqrt(S), isb, eps)
        P = P - (lr_bc1 * M) / den
    return P, M, S


# ---- the inputs of the GPU tests (and of the emulation's host test) -------------------------------------------------------
def adam_case(n, state, seed=0):
    """fp32 (p, g, m, v, vmax) of n elements.  state "zero": first step; "mid": a mid-training state with vmax > v on the
    even elements and vmax == v on the odd ones (some of those overtaken by this step's v, some not)"""
    r = np.random.default_rng(1000 + seed)
    p = r.standard_normal(n, dtype=np.float32)
    g = r.standard_normal(n, dtype=np.float32) * np.float32(0.1)
    g[::7] *= np.float32(30.0)
    if state == "zero":
        z = np.zeros(n, np.float32)
        return p, g, z, z.copy(), z.copy()
    m = r.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    v = (r.random(n, dtype=np.float32) * np.float32(0.02) + np.float32(1e-6)).astype(np.float32)
    x = v.copy()
    x[::2] *= (np.float32(1.0) + r.random((n + 1) // 2, dtype=np.float32) * np.float32(3.0))
    return p, g, m, v, x


def belief_case(n, state, seed=0):
    p, g, m, v, _ = adam_case(n, state, seed + 50)
    return p, g, m, v


# ---- folds and sums ------------------------------------------------------------------------------------------------------
def rows_sum(src, rows, length, stride, offset=0):
    """(sum_r src[offset + r stride + i], sum_r |...|) for i < length, float64"""
    src = _d(src)
    idx = offset + np.arange(rows)[:, None] * stride + np.arange(length)[None, :]
    t = src[idx]
    return t.sum(0), np.abs(t).sum(0)


def fold(dst, arena, segments):
    """dst[off + i] += sum_r arena[src + r stride + i] for every segment (src, off, rows, len, stride), chained ones
    (same destination) included -> (dst float64, per-element bound (R + 1) u sum|terms| with R = all terms of the element,
    the destination's own value among them; 0 where nothing was folded)"""
    out = _d(dst).copy()
    mag = np.abs(out)
    cnt = np.zeros(out.shape, np.int64)
    for so, do, rows, ln, sd in segments:
        sm, ab = rows_sum(arena, rows, ln, sd, so)
        out[do:do + ln] += sm
        mag[do:do + ln] += ab
        cnt[do:do + ln] += rows
    bound = np.where(cnt > 0, (cnt + 2) * U * mag + TINY, 0.0)
    return out, bound


def rider(W, rows):
    """out_k = sum_n W[k][n] sum_b rows[n][b] (W as fp32, how the launch receives it) -> (out, bound): the row sums
    carry (B + 1) u sum_b |.|, the weighted sum n_rows products and additions: (B + n_rows + 3) u sum_n |W| sum_b |.|"""
    W = _d(np.asarray(W, dtype=np.float32))
    rows = _d(rows)
    out = W @ rows.sum(1)
    bound = (rows.shape[1] + rows.shape[0] + 3) * U * (np.abs(W) @ np.abs(rows).sum(1)) + TINY
    return out, bound
