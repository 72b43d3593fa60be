"""Reference of the loudness normalisation (include/tortoise_mi355x_loud.h), the error bounds of every number the device returns, and the
seeded clip family the CPU and GPU tests share.

Nothing here is tuned.  The constants are the header's; the bounds follow from the unit roundoffs U64 = 2^-53 (the filter, the sums of squares,
the gates, L and the gain are f64 on the device) and U32 = 2^-24 (true peak, limiter, samples), with gamma_k(u) = k u / (1 - k u).

The reference filter runs in extended precision (numpy longdouble; unit roundoff REF_U, 2^-64 where the platform has the x87 format): the
device's filter is f64 itself, so an fp64 reference would err as much as the device.  Every f64 bound below is multiplied by
REF_SHARE = 1 + REF_U / U64 for the reference's own error (1 + 2^-11; 2 where longdouble is double).

  filter   (steps 1 - 4 of the issue, laid out for the device's scheme: segments of S = 150 samples, a zero-state pass, a carry, a second pass)
           local     one section's sample is five terms, one fused multiply-add each, with coefficients rounded once to f64: at most 6 roundings
                     touch a term, k = 8 is used:  l[n] = gamma_8 (|b0 x| + |b1 x'| + |b2 x''| + |a1 y'| + |a2 y''|)
           spread    every sample is computed twice: by the zero-state pass, whose local error reaches the LATER segments (through the
                     carried states, exactly as it would travel in a sequential run), and by the second pass, whose local error stays in
                     ITS segment.  With l[n] the larger of the two passes' local errors (their magnitudes differ), e = |g| * l covers
                     both, g the impulse response of the recursive part, followed through SPREAD_TAPS taps
           cascade   the shelf's error e1 enters the high-pass as input: its local error gains |e1[n]| + 2 |e1[n-1]| + |e1[n-2]|
           carry     state' = M state + z is 4 fused multiply-adds per value with an M rounded once from extended precision: each value is
                     off by at most rho = gamma_8 (|M| |state| + |z|) (M is far from normal - the high-pass has a double pole at 0.995:
                     entries up to 95, spectral radius 0.47 - and the products do cancel).  That perturbs the state the NEXT segment
                     starts from; the output feels it through |H|, the cascade's response to a unit start state
           hop       q_h = sum y^2 in sums of at most 150 + 16 terms:  |dq_h| <= sum (2 |y| e + e^2) + gamma_H sum y^2
  blocks   z_j = four q's and a division: the hop bounds add, plus gamma_4 z_j
  L        the mean of nb blocks in any order: the block bounds' mean plus gamma_(nb + 8) mean; 10 log10 carries the relative bound
           (10 / ln 10) and the library's log10, the product and the sum: 16 U64 (|L| + 1)
  gain     10^((T - L) / 20): (ln 10 / 20) of L's bound, the power's few ulps 8 U64 (1 + |T - L|), one rounding to f32
  peak     16 fused multiply-adds per phase with the specification's f32 taps (tabulated in csrc/loudness.hip and held to `taps()` bit for
           bit by tests/test_loudness_cpu.py):  |du_p[n]| <= gamma_16 sum_t |h_p[t] x[n+t]|, and a maximum moves by at most the largest
  limiter  derived in `limiter`, a few U32 per product as the header's roundings go
"""
import functools
import math

import numpy as np
from scipy.signal import fftconvolve
from scipy.ndimage import maximum_filter1d, minimum_filter1d

FS, H, B, S, LH, TAPS, OS = 24000, 2400, 9600, 150, 120, 16, 4   # TT_LOUD_*
NONE, SCALE, LOOKAHEAD = 0, 1, 2
OK, SHORT, SILENT, EMPTY, REFUSED = 0, 1, 2, 3, 4
U64, U32 = 2.0 ** -53, 2.0 ** -24
LD = np.longdouble
REF_U = float(np.finfo(LD).eps) / 2
REF_SHARE = 1.0 + REF_U / U64
ABS_GATE, REL_GATE = -70.0, -10.0
SPREAD_TAPS = 16384  # taps of |g| an error is followed through: the high-pass's double pole at 0.995 leaves (k + 1) 0.995^k, 1e-31 there
GATE_MARGIN = 1e-6   # LU: no family block may lie this close to a gate (tests/test_loudness_cpu.py)


def gamma(k, u):
    return k * u / (1 - k * u)


# ----------------------------------------------------------------------------------------- K-weighting
def coefficients(fs=FS):
    """((shelf b, shelf a), (high-pass b, high-pass a)) in fp64: b = (b0, b1, b2), a = (a1, a2)."""
    K, G, Q = math.tan(math.pi * 1681.974450955533 / fs), 3.999843853973347, 0.7071752369554196
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0),
             (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))
    K, Q = math.tan(math.pi * 38.13547087602444 / fs), 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return shelf, ((1.0, -2.0, 1.0), (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0))


def _rows(x, dtype):
    """x [n] -> [ceil(n / S), S + 2]: every segment behind its two samples of history (zeros before the clip and behind it)."""
    ns = -(-len(x) // S)
    xp = np.zeros(ns * S + 2, dtype=dtype)
    xp[2:2 + len(x)] = x
    return np.lib.stride_tricks.sliding_window_view(xp, S + 2)[::S].copy()


def _run(R, b, a, y1=0, y2=0):
    """One section over every row of R at once: columns 0, 1 are history (the output's: y2, y1), columns 2 .. the segment."""
    Y = np.zeros_like(R)
    Y[:, 1], Y[:, 0] = y1, y2
    for j in range(2, R.shape[1]):
        Y[:, j] = b[0] * R[:, j] + b[1] * R[:, j - 1] + b[2] * R[:, j - 2] - a[0] * Y[:, j - 1] - a[1] * Y[:, j - 2]
    return Y


def _section(x, b, a):
    """One biquad over x (longdouble), exactly the recurrence: zero-state segments, their states carried by the two homogeneous responses.
    -> (y [n], rows of y with history [ns, S + 2], rows of the zero-state pass)."""
    b, a = [LD(v) for v in b], [LD(v) for v in a]
    R = _rows(x, LD)
    Z = _run(R, b, a)
    h1, h2 = _run(np.zeros((1, S + 2), LD), b, a, y1=1)[0], _run(np.zeros((1, S + 2), LD), b, a, y2=1)[0]
    s1, s2 = np.zeros(len(R), LD), np.zeros(len(R), LD)
    p1 = p2 = LD(0)
    for k in range(len(R)):
        s1[k], s2[k] = p1, p2
        p1, p2 = Z[k, -1] + h1[-1] * p1 + h2[-1] * p2, Z[k, -2] + h1[-2] * p1 + h2[-2] * p2
    Y = Z + s1[:, None] * h1[None, :] + s2[:, None] * h2[None, :]
    return Y[:, 2:].reshape(-1)[:len(x)], Y, Z


def kweight(x, fs=FS):
    """The K-weighted signal in extended precision (any fs: the segmenting is only how the recurrence is evaluated)."""
    (sb, sa), (hb, ha) = coefficients(fs)
    return _section(_section(np.asarray(x, dtype=LD), sb, sa)[0], hb, ha)[0]


def kweight_plain(x, fs=FS):
    """The same by the plain loop (short clips: the tests compare the two)."""
    (sb, sa), (hb, ha) = coefficients(fs)
    out = np.asarray(x, dtype=LD)
    for b, a in ((sb, sa), (hb, ha)):
        y = np.zeros(len(out) + 2, LD)
        xp = np.concatenate([np.zeros(2, LD), out])
        for n in range(2, len(xp)):
            y[n] = LD(b[0]) * xp[n] + LD(b[1]) * xp[n - 1] + LD(b[2]) * xp[n - 2] - LD(a[0]) * y[n - 1] - LD(a[1]) * y[n - 2]
        out = y[2:]
    return out


def _impulse_abs(a, count):
    g = np.zeros(count)
    g[0] = 1.0
    for k in range(1, count):
        g[k] = -a[0] * g[k - 1] - (a[1] * g[k - 2] if k >= 2 else 0.0)
    return np.abs(g)


def transition():
    """M [4, 4] over (shelf y[n-1], y[n-2], high-pass y[n-1], y[n-2]): S samples without input."""
    (sb, sa), (hb, ha) = coefficients()
    M = np.zeros((4, 4))
    for q in range(4):
        V = _run(np.zeros((1, S + 2), LD), [LD(v) for v in sb], [LD(v) for v in sa], y1=LD(q == 0), y2=LD(q == 1))
        Y = _run(V, [LD(v) for v in hb], [LD(v) for v in ha], y1=LD(q == 2), y2=LD(q == 3))
        M[:, q] = [float(V[0, -1]), float(V[0, -2]), float(Y[0, -1]), float(Y[0, -2])]
    return M


@functools.lru_cache(maxsize=None)
def _spreads():
    """|g| of the two recursive parts and |H| [taps, 4], the response of the cascade's output to unit start states, SPREAD_TAPS each."""
    (sb, sa), (hb, ha) = coefficients()
    Hm = np.zeros((SPREAD_TAPS, 4))
    for q in range(4):
        v1, v2, y1, y2 = (float(q == i) for i in range(4))
        for n in range(SPREAD_TAPS):
            v = -sa[0] * v1 - sa[1] * v2
            y = v - 2.0 * v1 + v2 - ha[0] * y1 - ha[1] * y2
            v2, v1, y2, y1 = v1, v, y1, y
            Hm[n, q] = abs(y)
    return _impulse_abs(sa, SPREAD_TAPS), _impulse_abs(ha, SPREAD_TAPS), Hm


def _spread(e, taps):
    """sum_t taps[n - t] e[t] for non-negative e and taps, by FFT; the FFT's own rounding (some 1e-16 of the largest value) is covered."""
    out = fftconvolve(e, taps)[:len(e)]
    return np.maximum(out, 0.0) * (1 + 1e-9) + 1e-13 * float(out.max(initial=0.0))


def filter_with_bound(x):
    """x f32 [n] -> (y longdouble [n], e fp64 [n]): the K-weighted clip and the bound of the device's error on every sample (the module docstring)."""
    (sb, sa), (hb, ha) = coefficients()
    n = len(x)
    x = np.asarray(x, dtype=LD)
    v, V, Vz = _section(x, sb, sa)
    y, Y, _ = _section(v, hb, ha)
    Yz = _run(Vz, [LD(c) for c in hb], [LD(c) for c in ha])  # the device's zero-state pass: no history of v either
    X, V, Vz, Y, Yz = (np.abs(np.asarray(A, dtype=np.float64)) for A in (_rows(x, LD), V, Vz, Y, Yz))
    g8 = gamma(8, U64)
    sb_, sa_, ha_ = np.abs(sb), np.abs(sa), np.abs(ha)
    g1, g2, Hm = _spreads()
    flat = lambda A: A.reshape(-1)[:n]
    Vm, Ym = np.maximum(V, Vz), np.maximum(Y, Yz)  # either pass's magnitudes
    l1 = flat(g8 * (sb_[0] * X[:, 2:] + sb_[1] * X[:, 1:-1] + sb_[2] * X[:, :-2] + sa_[0] * Vm[:, 1:-1] + sa_[1] * Vm[:, :-2]))
    e1 = np.concatenate([np.zeros(2), _spread(l1, g1)])
    l2 = flat(g8 * (Vm[:, 2:] + 2 * Vm[:, 1:-1] + Vm[:, :-2] + ha_[0] * Ym[:, 1:-1] + ha_[1] * Ym[:, :-2])) + e1[2:] + 2 * e1[1:-1] + e1[:-2]
    e2 = _spread(l2, g2)
    # the carry's own roundings: segment k's product perturbs the state segment k + 1 starts from
    ns = len(X)
    state = np.stack([V[:, 1], V[:, 0], Y[:, 1], Y[:, 0]], axis=1)
    z = np.stack([Vz[:, -1], Vz[:, -2], Yz[:, -1], Yz[:, -2]], axis=1)
    rho = g8 * (state @ np.abs(transition()).T + z)
    for q in range(4):
        spikes = np.zeros(n)
        at = S * np.arange(1, ns)
        spikes[at[at < n]] = rho[:ns - 1, q][at < n]
        e2 = e2 + _spread(spikes, Hm[:, q])
    return y, e2 * REF_SHARE


# ----------------------------------------------------------------------------------------- blocks, gates, L
def hops(n):
    return -(-n // H)


def blocks(n):
    return (n - B) // H + 1 if n >= B else 0


def _lu(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def gating(q, qb, n):
    """Hop energies and their bounds -> dict(z, zb, l [blocks], above_abs, above_rel (masks), lufs, lufs_bound, status, margin: the least
    distance of a block's loudness, at either end of its bound, from a gate it is compared with)."""
    nb = blocks(n)
    if nb == 0:
        return dict(z=np.zeros(0), zb=np.zeros(0), l=np.zeros(0), above_abs=np.zeros(0, bool), above_rel=np.zeros(0, bool), lufs=-np.inf,
                    lufs_bound=0.0, status=SHORT, margin=np.inf)
    idx = np.arange(nb)
    z = (q[idx] + q[idx + 1] + q[idx + 2] + q[idx + 3]) / B
    zb = (qb[idx] + qb[idx + 1] + qb[idx + 2] + qb[idx + 3]) / B + gamma(4, U64) * z
    l = _lu(z)
    with np.errstate(invalid="ignore"):
        spread = np.maximum(np.abs(_lu(z + zb) - l), np.abs(l - _lu(np.maximum(z - zb, 0))))  # (inf where the bound reaches zero energy)
    spread = np.where(z > 0, spread, 0.0)  # (digital silence is below every gate whatever the bound)
    above_abs = l > ABS_GATE
    margin = float(np.min(np.abs(l - ABS_GATE) - spread))
    out = dict(z=z, zb=zb, l=l, above_abs=above_abs)
    if not above_abs.any():
        out.update(above_rel=above_abs, lufs=-np.inf, lufs_bound=0.0, status=SILENT, margin=margin)
        return out
    gate = _lu(z[above_abs].mean()) + REL_GATE
    gate_b = _mean_bound(z[above_abs], zb[above_abs], nb)
    above_rel = above_abs & (l > gate)
    margin = min(margin, float(np.min(np.abs(l[above_abs] - gate) - spread[above_abs])) - gate_b)
    out.update(above_rel=above_rel, lufs=float(_lu(z[above_rel].mean())), lufs_bound=_mean_bound(z[above_rel], zb[above_rel], nb), status=OK,
               margin=margin)
    return out


def _mean_bound(z, zb, nb):
    """Bound in LU of -0.691 + 10 log10 mean(z) as the device forms it."""
    m = float(z.mean())
    rel = (float(zb.mean()) + gamma(nb + 8, U64) * m) / m
    return 10.0 / math.log(10.0) * rel / (1 - rel) + 16 * U64 * (abs(float(_lu(m))) + 1)


# ----------------------------------------------------------------------------------------- true peak
@functools.lru_cache(maxsize=None)
def taps():
    """h [4, 16] f32: phase p, tap t = -7 .. 8."""
    h = np.zeros((OS, TAPS))
    h[0, 7] = 1.0
    for p in range(1, OS):
        a = np.arange(-7, 9) - p / OS
        h[p] = np.where(np.abs(a) < 8, np.sinc(a) * (0.5 + 0.5 * np.cos(np.pi * a / 8)), 0.0)
        h[p] /= h[p].sum()
    return h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def hann():
    """w [2 Lh + 1] f32, sum 1."""
    w = 0.5 + 0.5 * np.cos(np.pi * np.arange(-LH, LH + 1) / (LH + 1))
    return (w / w.sum()).astype(np.float32)


def peaks(x):
    """x [n] -> (P [n] fp64, bound [n]): max_p |u_p[n]| and the bound of the device's f32 value."""
    x = np.asarray(x, dtype=np.float64)
    xp = np.concatenate([np.zeros(7), x, np.zeros(8)])
    win = np.lib.stride_tricks.sliding_window_view(xp, TAPS)  # win[n, k] = x[n - 7 + k]
    h = taps().astype(np.float64)
    u = np.abs(win @ h.T)
    mag = np.abs(win) @ np.abs(h).T
    return u.max(axis=1), gamma(16, U32) * mag.max(axis=1)


def true_peak(x):
    """-> (TP, bound, A): A = max sum_t |h_p[t] x[n+t]|, the magnitude the bound is made of."""
    P, Pb = peaks(x)
    return float(P.max()), float(Pb.max()), float(Pb.max() / gamma(16, U32))


# ----------------------------------------------------------------------------------------- measure, gain, limiter
def measure(x):
    """One clip -> dict: hop_energy, hop_bound [hops]; gating()'s entries; blocks_abs, blocks_rel; true_peak, tp_bound, tp_mag."""
    n = len(x)
    y, e = filter_with_bound(x)
    pad = hops(n) * H - n
    q = np.asarray(np.concatenate([y * y, np.zeros(pad, LD)]).reshape(-1, H).sum(axis=1), dtype=np.float64)
    eb = np.concatenate([2 * np.abs(np.asarray(y, dtype=np.float64)) * e + e * e, np.zeros(pad)]).reshape(-1, H)
    qb = eb.sum(axis=1) + gamma(H, U64) * REF_SHARE * q
    out = dict(hop_energy=q, hop_bound=qb, **gating(q, qb, n))
    out["blocks_abs"], out["blocks_rel"] = int(out["above_abs"].sum()), int(out["above_rel"].sum())
    out["true_peak"], out["tp_bound"], out["tp_mag"] = true_peak(x)
    return out


def gain(m, target, ceiling, mode):
    """The reference's measurement, a target (LUFS), a linear ceiling -> (g, bound): what the device's f32 gain must be, and how close."""
    if m["status"] != OK:
        return 1.0, 0.0
    T = float(np.float32(target))
    d = (T - m["lufs"]) / 20.0
    g = 10.0 ** d
    rel = math.log(10.0) / 20.0 * m["lufs_bound"] + 8 * U64 * (1 + abs(T - m["lufs"])) + U32
    if mode == SCALE and m["true_peak"] > 0:
        lim = float(np.float32(ceiling)) / m["true_peak"]
        lim_rel = m["tp_bound"] / (m["true_peak"] - m["tp_bound"]) + U32  # the device divides by ITS peak, rounded once
        if lim * (1 + lim_rel) < g * (1 - rel):
            g, rel = lim, lim_rel
        elif lim * (1 - lim_rel) < g * (1 + rel):  # either may be the smaller on the device
            lo, hi = min(lim * (1 - lim_rel), g * (1 - rel)), min(lim * (1 + lim_rel), g * (1 + rel))
            g, rel = (lo + hi) / 2, (hi - lo) / (lo + hi)
    return g, rel * g * (1 + 2 * U32)


def scale_ceiling_bound(m, g, ceiling):
    """SCALE: out_true_peak <= c (1 + this).  out = g' x (1 + d), |d| <= U32, g' <= (c / TP_dev)(1 + U32), TP_dev >= TP - tp_bound; the
    oversampler is linear, so its exact peak on out is within g' (TP + U32 A), and the device's reading within gamma_16 g' A (1 + U32) of that."""
    tp, tb, A = m["true_peak"], m["tp_bound"], m["tp_mag"]
    return U32 + tb / (tp - tb) + (U32 + 1.01 * gamma(16, U32)) * g * A / ceiling + 4 * U32 * U32


def limiter(x, g, ceiling):
    """The LOOKAHEAD limiter in fp64 with the f32 gain g and the f32 tables -> dict(y, bound [n], r, s, free: no device rounding can make
    anything limit within 2 Lh, so y must be f32(g x) exactly).

    The device's values, all f32: P (bound Pb, `peaks`); d = g max(P', P) and c / d, a rounding each, so before the clamp the ratio is off by at
    most rho = Pb / P + 3 U32 relative (second order included), and |min(1, a) - min(1, b)| <= |a - b|: rb = ratio * rho, and 0 where
    ratio (1 - rho) >= 1 (both clamp).  The sliding minimum moves by at most the largest rb in its window.  1 - m is exact for m >= 1/2, else
    one rounding.  The smoothing is 241 fused multiply-adds of non-negative terms with a window the host rounds from fp64 with its own
    libm (two more roundings): gamma_243.  1 - a: one rounding.  min(r, .) moves by at most the larger of its arguments' bounds.  (g x) s: two roundings."""
    x = np.asarray(x, dtype=np.float64)
    g, c = float(np.float32(g)), float(np.float32(ceiling))
    n = len(x)
    P, Pb = peaks(x)
    Pm = np.maximum(np.concatenate([[0.0], P[:-1]]), P)
    Pmb = np.maximum(np.concatenate([[0.0], Pb[:-1]]), Pb)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(Pm > 0, c / (g * Pm), np.inf)
        rho = np.where(Pm > 0, Pmb / np.maximum(Pm - Pmb, 1e-300), 0.0) + 3 * U32
    r = np.minimum(1.0, ratio)
    sure = ratio * (1 - rho) >= 1  # r is 1 on the device too
    rb = np.where(sure, 0.0, np.minimum(ratio, 2.0) * rho)
    m = minimum_filter1d(r, 2 * LH + 1, mode="constant", cval=1.0)
    mb = maximum_filter1d(rb, 2 * LH + 1, mode="constant", cval=0.0)
    # m outside the clip is defined by the same formula (r = 1 there): pad before smoothing
    rp = np.concatenate([np.ones(2 * LH), r, np.ones(2 * LH)])
    rbp = np.concatenate([np.zeros(2 * LH), rb, np.zeros(2 * LH)])
    mp = minimum_filter1d(rp, 2 * LH + 1, mode="constant", cval=1.0)[LH:-LH]      # m[-Lh .. n + Lh)
    mbp = maximum_filter1d(rbp, 2 * LH + 1, mode="constant", cval=0.0)[LH:-LH]
    assert np.array_equal(mp[LH:-LH], m) and np.array_equal(mbp[LH:-LH], mb)
    w = hann().astype(np.float64)
    dd = 1.0 - mp
    ddb = mbp + U32 * dd
    a = np.convolve(dd, w, mode="valid")  # (w is symmetric)
    ab = np.convolve(ddb, w, mode="valid") + gamma(243, U32) * a
    s = np.minimum(r, 1.0 - a)
    sb = np.maximum(rb, ab + U32 * np.abs(1.0 - a))
    y = g * x * s
    yb = np.abs(g * x) * (sb + 3 * U32 * s) + 2.0 ** -149  # (a result below the smallest normal f32 rounds to a subnormal)
    free = minimum_filter1d(np.concatenate([np.ones(2 * LH, bool), sure, np.ones(2 * LH, bool)]).astype(np.uint8), 4 * LH + 1)[2 * LH:-2 * LH] == 1
    return dict(y=y, bound=yb, r=r, s=s, free=free)


# ----------------------------------------------------------------------------------------- the family
LEVELS = (1.0, 0.1, 10.0 ** (-57.0 / 20.0))  # the loud stretch, 20 dB down, near -75 LUFS
TARGETS = (-16.0, -23.0, -30.0)
CEILINGS_DB = (-1.0, -6.0)
# (kind, samples, seed)
FAMILY = tuple([("speech", n, 0) for n in (1, 2399, 2400, 9599, 9600, 9601, 12000, 14999, 15001, 16799, 16800, 19199, 19201)]
               + [("speech", n, s) for n in (72000, 120000) for s in (0, 1)]
               + [("zero", 12000, 0), ("quiet", 16800, 0), ("quiet", 72000, 1)])


def voiced(n, seed):
    """Speech-like f32 audio at 24 kHz as tests/tsm_reference.clip makes it: six gliding harmonics of a 90 - 260 Hz fundamental under a
    syllabic envelope, unvoiced noise in about a quarter of the 100 ms segments, a -40 dB noise floor."""
    rng = np.random.default_rng(9000 + 131 * seed + n)
    t = np.arange(n) / FS
    knots = max(2, int(np.ceil(n / (0.1 * FS))) + 1)
    f0 = np.interp(t, np.arange(knots) * 0.1, rng.uniform(90.0, 260.0, knots))
    phase = 2.0 * np.pi * np.cumsum(f0) / FS
    body = sum(rng.uniform(0.5, 1.0) / h * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 7))
    noisy = (rng.random(knots) < 0.25)[np.minimum((t / 0.1).astype(np.int64), knots - 1)]
    body = np.where(noisy, 0.5 * rng.standard_normal(n), body)
    env = np.maximum(0.55 + 0.45 * np.sin(2.0 * np.pi * rng.uniform(3.5, 5.5) * t + rng.uniform(0, 2 * np.pi)), 0.1)
    return 0.3 * env * body + 0.01 * rng.standard_normal(n)


def clip(kind, n, seed):
    """speech: three stretches in a seeded order - loud, 20 dB down, near -75 LUFS - so that both gates remove blocks of a long clip;
    quiet: all of it below -70 LUFS; zero: digital silence."""
    if kind == "zero":
        return np.zeros(n, dtype=np.float32)
    x = voiced(n, seed)
    if kind == "quiet":
        return (x * 10.0 ** (-70.0 / 20.0)).astype(np.float32)
    order = np.random.default_rng(77 + seed + n).permutation(3)
    level = np.asarray(LEVELS)[order][np.minimum(np.arange(n) * 3 // max(n, 1), 2)]
    return (x * level).astype(np.float32)


def settings(i):
    """Target (LUFS) and ceiling (linear f32) of family member i: every target meets every ceiling."""
    return TARGETS[i % 3], float(np.float32(10.0 ** (CEILINGS_DB[(i // 3) % 2] / 20.0)))


@functools.lru_cache(maxsize=None)
def family_reference():
    """[(x f32, target, ceiling, measure(x))] for FAMILY, computed once per process and shared (read-only)."""
    out = []
    for i, (kind, n, seed) in enumerate(FAMILY):
        x = clip(kind, n, seed)
        x.setflags(write=False)
        out.append((x, *settings(i), measure(x)))
    return tuple(out)


# ----------------------------------------------------------------------------------------- an emulation of the device's arithmetic
def emulate(x, target, ceiling, mode):
    """The device's scheme in the device's formats, with numpy's operations instead of fused ones (another rounding here and there, inside
    the same bounds): the f64 segment passes and the carry, f32 peaks, the f32 limiter -> dict(hop_energy, true_peak, lufs, blocks_abs,
    blocks_rel, status, gain, y, out_true_peak).  The CPU tests run the GPU test's checks on it."""
    (sb, sa), (hb, ha) = coefficients()
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    Xr = _rows(x.astype(np.float64), np.float64)
    Vz = _run(Xr, sb, sa)
    Yz = _run(Vz, hb, ha)
    M, st, states = transition(), np.zeros(4), np.zeros((len(Xr), 4))
    for k in range(len(Xr)):
        states[k] = st
        st = M @ st + np.array([Vz[k, -1], Vz[k, -2], Yz[k, -1], Yz[k, -2]])
    V = _run(Xr, sb, sa, y1=states[:, 0], y2=states[:, 1])
    Y = _run(V, hb, ha, y1=states[:, 2], y2=states[:, 3])
    y = Y[:, 2:].reshape(-1)[:n]
    seg = np.add.reduceat(y * y, np.arange(0, n, S))
    q = np.add.reduceat(seg, np.arange(0, len(seg), H // S))
    nb, out = blocks(n), dict(hop_energy=q, lufs=-np.inf, blocks_abs=0, blocks_rel=0, status=SHORT, gain=np.float32(1))
    if nb:
        z = np.array([(((q[j] + q[j + 1]) + q[j + 2]) + q[j + 3]) / B for j in range(nb)])
        a = z > 10.0 ** (-6.9309)
        out["status"] = SILENT
        if a.any():
            r = a & (z > 0.1 * (z[a].sum() / a.sum()))
            out.update(status=OK, lufs=-0.691 + 10 * np.log10(z[r].sum() / r.sum()), blocks_abs=int(a.sum()), blocks_rel=int(r.sum()))

    def peaks32(s):
        sp = np.concatenate([np.zeros(7, np.float32), s, np.zeros(8, np.float32)])
        win = np.lib.stride_tricks.sliding_window_view(sp, TAPS)
        P = np.abs(s)
        for p in range(1, OS):
            acc = np.zeros(len(s), np.float32)
            for t in range(TAPS):
                acc = acc + taps()[p, t] * win[:, t]
            P = np.maximum(P, np.abs(acc))
        return P

    P = peaks32(x)
    out["true_peak"] = P.max()
    g = np.float32(1)
    if out["status"] == OK:
        g = np.float32(10.0 ** ((float(np.float32(target)) - out["lufs"]) / 20.0))
        if mode == SCALE and out["true_peak"] > 0:
            g = min(g, np.float32(ceiling) / out["true_peak"])
    out["gain"] = g
    if mode == LOOKAHEAD and out["status"] == OK:
        with np.errstate(divide="ignore"):
            r = np.minimum(np.float32(1), np.float32(ceiling) / (g * np.maximum(np.concatenate([[np.float32(0)], P[:-1]]), P)))
        rp = np.concatenate([np.ones(2 * LH, np.float32), r, np.ones(2 * LH, np.float32)])
        d = np.float32(1) - minimum_filter1d(rp, 2 * LH + 1, mode="constant", cval=1.0)[LH:-LH]
        acc = np.zeros(n, np.float32)
        for k in range(2 * LH + 1):
            acc = acc + hann()[k] * d[k:k + n]
        out["y"] = (g * x) * np.minimum(r, np.float32(1) - acc)
    else:
        out["y"] = g * x
    out["out_true_peak"] = peaks32(out["y"]).max()
    return out
