"""fp64 reference of the F0 tracker (include/tortoise_mi355x_f0.h) with the element-wise bounds of the device's arithmetic
and the test of whether a frame's decisions could flip inside them.

Bounds (u32 = 2^-24, u64 = 2^-53, gamma_k(u) = k u / (1 - k u)):
  d      every term is one rounded subtraction and one FMA, the 960 non-negative terms are summed in some order: at most W + 2 rounded
         operations on a path, so |d32 - d| <= g d with g = gamma_(W+2)(u32) = 5.73e-5.
  c      a sum of non-negative d32 values in f64: every term is within g of its exact value, the f64 additions add gamma_16(u64).
  d'     d tau / c: relative error at most E = (1 + g)(1 + h) / ((1 - g)(1 - h)) - 1 with h = gamma_32(u64), which also covers the
         product, the division and this reference's own f64 sums (pairwise, far below 32 operations deep).  E = 1.147e-4.
         c = 0 exactly means every term is 0, on the device too: d' = 1 on both sides, bound 0.
  aper   (float)d': E d' + u32 (1 + E) d'.
  P      x^2 is exact in f64, 21 additions on a path: relative gamma_32(u64) with the reference's own.
  delta  num = a - c, den = (a - 2 b) + c with |dnum| <= En = E (a + c) + 4 u64 (a + c), |dden| <= Ed = E (a + 2 b + c) + 8 u64 (a + 2 b + c)
         (an exact entry, d' = 1 where c = 0, contributes no E term).
         For |den| > Ed:  |num'/den' - num/den| = |dnum den - num dden| / |den den'| <= (En |den| + |num| Ed) / (|den| (|den| - Ed)),
         which is the first-order term (En + |num / den| Ed) / |den| and its remainder in one expression; the clamp is 1-Lipschitz;
         0.5 and the f64 roundings of the quotient add 4 u64 (1 + |delta|).
  f0     24000 / (t + delta): |df0| <= 24000 Edelta / ((t + delta)(t + delta - Edelta)) + (u32 + 4 u64) f0.
A frame is ambiguous when a comparison of the pick could flip inside these bounds: d'(tau) against thr for every tau the search for t0
looks at (lo .. t0, or lo .. hi where there is none), d'(tau + 1) against d'(tau) along the descent t0 .. t^, every other lag's d' against
the minimum where the argmin is taken, P against floor_e where a t0 exists - or when |den| <= Ed.  The test is deliberately wide: the errors
of neighbouring lags are strongly correlated (they share almost all of c), and the intervals ignore that."""
import functools

import numpy as np

H, W, T, LEAD = 240, 960, 480, 720
LAG_MIN, LAG_MAX = 24, 480
SR = 24000
U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma(k, u):
    return k * u / (1.0 - k * u)


G_D = gamma(W + 2, U32)
H64 = gamma(32, U64)
E_DP = (1.0 + G_D) * (1.0 + H64) / ((1.0 - G_D) * (1.0 - H64)) - 1.0
G_P = gamma(32, U64)


def frames(n):
    return -(-int(n) // H)


def windows(x):
    """x f32 / f64 [n] -> f64 [F, W + T]: frame f's samples x[f H - 720 ..), 0 outside the clip."""
    x = np.asarray(x, dtype=np.float64)
    n, F = x.shape[0], frames(x.shape[0])
    pad = np.concatenate([np.zeros(LEAD), x, np.zeros(F * H + W + T)])
    idx = (np.arange(F) * H)[:, None] + np.arange(W + T)[None, :]
    return pad[idx]


def difference(X):
    """f64 [F, W + T] -> d f64 [F, T + 1] (d(0) = 0)."""
    d = np.zeros((X.shape[0], T + 1))
    for tau in range(1, T + 1):
        e = X[:, :W] - X[:, tau:tau + W]
        d[:, tau] = np.einsum("fj,fj->f", e, e)
    return d


def difference_f32_sequential(X):
    """The same in f32, every term (a - b) squared and added in ascending j, one rounding each: an emulation of ONE admissible order."""
    X = X.astype(np.float32)
    d = np.zeros((X.shape[0], T + 1), dtype=np.float32)
    for tau in range(1, T + 1):
        e = X[:, :W] - X[:, tau:tau + W]
        d[:, tau] = np.add.accumulate(e * e, axis=1, dtype=np.float32)[:, -1]
    return d


def normalise(d):
    """d [F, T + 1] -> d' f64 [F, T + 1]: d tau / c, 1 where c = 0 and at tau = 0."""
    c = np.cumsum(d[:, 1:].astype(np.float64), axis=1)
    tau = np.arange(1, T + 1, dtype=np.float64)[None, :]
    dp = np.ones((d.shape[0], T + 1))
    nz = c > 0
    dp[:, 1:][nz] = (d[:, 1:].astype(np.float64) * tau)[nz] / c[nz]
    return dp


def pick(dp, P, lo, hi, thr, floor_e):
    """One frame: d' [T + 1], P -> (lag, voiced, t0 or None)."""
    seg = dp[lo:hi + 1]
    below = np.nonzero(seg < thr)[0]
    if below.size == 0:
        return lo + int(np.argmin(seg)), False, None
    t0 = lo + int(below[0])
    t = t0
    while t < hi and dp[t + 1] < dp[t]:
        t += 1
    return t, bool(P >= floor_e), t0


def refine(dp, bound, t):
    """-> (delta, its bound or None where den is within its own error of 0).  bound: the |error| bound of every d' of the frame."""
    if not 2 <= t <= T - 1:
        return 0.0, 0.0
    a, b, c = dp[t - 1], dp[t], dp[t + 1]
    ea, eb, ec = bound[t - 1], bound[t], bound[t + 1]
    num, den = a - c, (a - 2.0 * b) + c
    En = ea + ec + 4 * U64 * (a + c)
    Ed = ea + 2.0 * eb + ec + 8 * U64 * (a + 2.0 * b + c)
    value = lambda: min(1.0, max(-1.0, 0.5 * num / den)) if den > 0 else 0.0
    if ea == 0 and eb == 0 and ec == 0:  # (exact entries, 1 where c = 0: the device computes den from the very same values)
        return value(), 4 * U64 * 2.0
    if abs(den) <= Ed:
        return value(), None
    if den < 0:
        return 0.0, 0.0
    delta = value()
    return delta, 0.5 * (En * den + abs(num) * Ed) / (den * (den - Ed)) + 4 * U64 * (1.0 + abs(delta))


def ambiguous(dp, bound, P, lo, hi, thr, floor_e, t, t0):
    """bound: the frame's |error| bound of every d' (0 where c = 0 and at tau = 0: those are exact)."""
    lo_v, hi_v = dp - bound, dp + bound
    last = hi if t0 is None else t0
    sl = slice(lo, last + 1)
    if np.any((lo_v[sl] <= thr) & (thr <= hi_v[sl]) & (lo_v[sl] != hi_v[sl])):
        return True
    if t0 is None:
        others = np.ones(hi - lo + 1, dtype=bool)
        others[t - lo] = False
        exact = (bound[lo:hi + 1] == 0) & (bound[t] == 0)  # (two exact values compare on the device as they do here)
        if np.any((lo_v[lo:hi + 1] <= hi_v[t]) & others & ~exact):
            return True
    else:
        for tau in range(t0, min(t, hi - 1) + 1):  # the comparisons d'(tau + 1) >= d'(tau) that were made
            if lo_v[tau + 1] <= hi_v[tau] and lo_v[tau] <= hi_v[tau + 1] and dp[tau + 1] != dp[tau]:
                return True
            if dp[tau + 1] == dp[tau] and lo_v[tau] != hi_v[tau]:
                return True
        if P * (1.0 - G_P) <= floor_e <= P * (1.0 + G_P) and P > 0 and floor_e > 0:
            return True
    return False


def track(x, lo=48, hi=400, thr=0.15, floor_e=W * 1e-5):
    """A clip -> dict of per-frame arrays: dprime [F, T + 1], dprime_bound, lag, voiced, f0, f0_bound, aper, aper_bound, power, ambiguous."""
    X = windows(x)
    F = X.shape[0]
    d = difference(X)
    dp = normalise(d)
    P = np.einsum("fj,fj->f", X[:, :W], X[:, :W])
    dp_bound = E_DP * dp
    dp_bound[:, 0] = 0.0
    dp_bound[:, 1:][np.cumsum(d[:, 1:], axis=1) == 0] = 0.0  # (c = 0: every term is 0 on the device too)
    out = dict(dprime=dp, dprime_bound=dp_bound, power=P, lag=np.zeros(F, np.int32), voiced=np.zeros(F, bool), f0=np.zeros(F),
               f0_bound=np.zeros(F), aper=np.zeros(F), aper_bound=np.zeros(F), ambiguous=np.zeros(F, bool), delta=np.zeros(F))
    for f in range(F):
        t, v, t0 = pick(dp[f], P[f], lo, hi, thr, floor_e)
        amb = ambiguous(dp[f], dp_bound[f], P[f], lo, hi, thr, floor_e, t, t0)
        delta, db = refine(dp[f], dp_bound[f], t)
        if db is None:
            amb, db = True, 0.0
        out["lag"][f], out["voiced"][f], out["ambiguous"][f], out["delta"][f] = t, v, amb, delta
        out["aper"][f] = dp[f, t]
        out["aper_bound"][f] = E_DP * dp[f, t] + U32 * (1.0 + E_DP) * dp[f, t]
        if v:
            f0 = SR / (t + delta)
            out["f0"][f] = f0
            out["f0_bound"][f] = SR * db / ((t + delta) * (t + delta - db)) + (U32 + 4 * U64) * f0 * 1.001
    return out


# ------------------------------------------------------------------------------------------------------------------- the test signals
FAMILY_F0 = [62.5 * (490.0 / 62.5) ** (k / 11.0) for k in range(12)]
FAMILY_SNR = (40.0, 20.0)
FAMILY_N = 12000


def harmonic(f0, n=FAMILY_N, snr_db=None, seed=0, harmonics=8, amp=0.25):
    """Eight harmonics at amplitudes 1 / h and seeded phases, white noise at snr_db below the tone's power -> f32 [n]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    ph = rng.uniform(0, 2 * np.pi, harmonics)
    x = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + ph[h]) / (h + 1) for h in range(harmonics))
    x = amp * x / np.sqrt(np.mean(x * x))
    if snr_db is not None:
        x = x + rng.standard_normal(n) * amp * 10.0 ** (-snr_db / 20.0)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def family():
    """[(f0, snr, clip f32, track(clip))] for the 24 clips: computed once and shared (read-only)."""
    out = []
    for k, f0 in enumerate(FAMILY_F0):
        for s, snr in enumerate(FAMILY_SNR):
            x = harmonic(f0, snr_db=snr, seed=100 * s + k)
            x.setflags(write=False)
            out.append((f0, snr, x, track(x)))
    return out


def inner_frames(n):
    """The frames whose W + T samples lie inside a clip of n samples."""
    return [f for f in range(frames(n)) if f * H - LEAD >= 0 and f * H - LEAD + W + T <= n]


def cents(f, ref):
    return 1200.0 * np.log2(f / ref)
