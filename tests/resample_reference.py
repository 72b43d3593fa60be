"""fp64 reference of the arbitrary-ratio resampler (include/tortoise_mi355x_rs.h), the f32 error bound of every output sample, and the
seeded clips the CPU and GPU tests share.

Nothing here is tuned.  The constants and integers are the header's, the table is the header's formula in fp64 rounded to f32 (I0 by its
power series and libm's sin, the operations csrc/resample.hip performs), and the bound follows from the unit roundoff of f32, u = 2^-24,
with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, 3.1):

  tap      the device forms h_j = c32 * fma(a, t1 - t0, t0) from exact f32 inputs (table values, the blend a = (u & 65535) / 65536, c32)
           in three rounded operations: the difference, the fused multiply-add, the product.  The first error reaches the result
           through a (t1 - t0) alone, the other two through the whole value v = t0 + a (t1 - t0):
               |h_f32 - h| <= c32 (gamma_1 (1 + u)^2 |a (t1 - t0)| + gamma_2 |v|) <= gamma_3 c32 (|a (t1 - t0)| + |v|) =: eh_j
  sample   y = sum_j h_j x_j over N = 2 H + 2 taps with one fused multiply-add per term (one rounding each): every term carries at most N
           roundings of the running sum,
               |y_f32 - y| <= sum_j |x_j| (eh_j (1 + gamma_N) + |h_j| gamma_N) + N 2^-149
           (the last term: a result in the subnormal range is rounded to a multiple of 2^-149 instead of relatively).
  fp64     the reference's own error is 2^-29 of these and is ignored.
"""
import functools
import math

import numpy as np

Z, L, BETA = 32, 512, 10                # TT_RS_ZEROS, TT_RS_PER_ZERO, TT_RS_BETA
TABLE = Z * L + 1
RHO_NUM, RHO_DEN = 9, 10
PITCH_ONE = 65536
MAX_TERM, MAX_RATIO = 1 << 20, 8
MAX_SAMPLES = 1 << 23
U = 2.0 ** -24

RATIOS = ((1, 2), (80, 147), (3, 2), (3, 1), (77936, 65536), (55109, 65536))  # the issue's six
EXTREME_RATIOS = ((8, 1), (1, 8))
LENGTHS = (1, 2, 37, 1000, 5000)
EXTREME_LENGTHS = (1, 2, 37, 1000, 2000)


def gamma(k):
    return k * U / (1.0 - k * U)


def i0(x):
    """sum_k ((x / 2)^k / k!)^2, the double operations of csrc/resample.hip's rs_i0 in their order."""
    y, term, total = x / 2, 1.0, 1.0
    for k in range(1, 500):
        f = y / k
        term *= f * f
        total += term
        if term < 1e-17 * total:
            break
    return total


@functools.lru_cache(maxsize=None)
def table():
    """tab[t], t = 0 .. Z L: fp64 values rounded to f32 (returned as float64 holding f32 values)."""
    i0b = i0(float(BETA))
    tab = np.empty(TABLE, dtype=np.float64)
    for t in range(TABLE):
        x, q = t / L, t / (Z * L)
        s = math.sin(math.pi * x) / (math.pi * x) if t else 1.0
        tab[t] = s * i0(BETA * math.sqrt(1.0 - q * q)) / i0b
    out = tab.astype(np.float32).astype(np.float64)
    out.setflags(write=False)
    return out


def ratio_ok(P, Q):
    if not (1 <= P <= MAX_TERM and 1 <= Q <= MAX_TERM and P <= MAX_RATIO * Q and Q <= MAX_RATIO * P):
        return False
    return Q == PITCH_ONE or math.gcd(P, Q) == 1


def out_samples(n, P, Q):
    return -((-n * Q) // P)


def cutoff_q(P, Q):
    """cq = floor(9 L 65536 Qc / (10 Pc)), (Pc, Qc) = (P, Q) for P > Q, else (1, 1)."""
    num = RHO_NUM * L * 65536
    return num * Q // (RHO_DEN * P) if P > Q else num // RHO_DEN


def cutoff_f32(P, Q):
    """c32 = (float)(0.9 * min(1.0, (double)Q / (double)P))."""
    return float(np.float32(0.9 * (Q / P if P > Q else 1.0)))


def half_width(cq):
    return -((-(Z * L * 65536)) // cq)


def resample(x, P, Q, bound=True):
    """x: f32 (or f32-valued) samples [n], ratio (P, Q) -> (y fp64 [n_out], the bound on |y_f32 - y| [n_out] or None): the header's formula
    literally, the division of every tap included."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    assert n >= 1 and ratio_ok(P, Q)
    n_out, cq, c32 = out_samples(n, P, Q), cutoff_q(P, Q), cutoff_f32(P, Q)
    H = half_width(cq)
    N = 2 * H + 2
    tab = table()
    xp = np.concatenate([np.zeros(H), x, np.zeros(H + 2)])  # xp[j + H] = x[j], zeros outside [0, n)
    d = np.arange(-H, H + 2, dtype=np.int64)
    y = np.empty(n_out)
    b = np.empty(n_out) if bound else None
    step = max(1, (1 << 21) // N)  # rows per block: bounded memory
    for m0 in range(0, n_out, step):
        m = np.arange(m0, min(n_out, m0 + step), dtype=np.int64)
        num = m * P
        i, r = num // Q, num % Q
        u = (np.abs(d[None, :] * Q - r[:, None]) * cq) // Q
        k = u >> 16
        a = (u & 65535) / 65536.0
        live = k < Z * L
        kc = np.where(live, k, 0)
        t0, t1 = tab[kc], tab[kc + 1]
        dt = a * (t1 - t0)
        v = np.where(live, t0 + dt, 0.0)
        h = c32 * v
        xs = xp[(i[:, None] + d[None, :]) + H]
        y[m0:m0 + len(m)] = (h * xs).sum(axis=1)
        if bound:
            eh = np.where(live, gamma(3) * c32 * (np.abs(dt) + np.abs(v)), 0.0)
            b[m0:m0 + len(m)] = (np.abs(xs) * (eh * (1.0 + gamma(N)) + np.abs(h) * gamma(N))).sum(axis=1) + N * 2.0 ** -149
    return y, b


def map_sample(s, P, Q, n_out):
    return min(n_out, (s * Q + P // 2) // P)


def clip(n, seed):
    """A seeded f32 test clip of n samples: white noise plus three tones, peak about 1."""
    rng = np.random.default_rng(1000 * seed + n)
    t = np.arange(n)
    x = 0.25 * rng.standard_normal(n)
    for f, amp in ((0.013, 0.3), (0.11, 0.2), (0.31, 0.1)):
        x += amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)
