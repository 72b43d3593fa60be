"""fp64 restatement of include/tortoise_mi355x_sil.h: exact frame energies, the band a device energy must lie in, the labelling as
bridge-then-dilate (NOT the device's closed form), regions, the edit, the segment list and the output with a per-sample bound.

Bounds come from the formats alone.  A device frame energy is the result of at most K = 4 S + 3 rounded f64 operations on non-negative
terms (one FMA per sample of four slots, x^2 being exact in f64, and three additions), so |e_dev - e| <= gamma_K e with
gamma_k = k u / (1 - k u), u = 2^-53.  A cross-faded sample is three rounded f32 operations (the weight's division, the difference, the
FMA), a faded one two (the weight's division, the product); u32 = 2^-24, plus half the smallest subnormal for a result that underflows."""
import math

import numpy as np

S, HOP, FRAME, X = 120, 240, 480, 120
SAMPLE_RATE = 24000
MAX_SAMPLES, MAX_CLIPS, MAX_FRAMES_PARAM = 8388608, 64, 6000
OK, UNCHANGED, SILENT, EMPTY, REFUSED = 0, 1, 2, 3, 4
K_OPS = 4 * S + 3
U64, U32 = 2.0 ** -53, 2.0 ** -24


def gamma(k, u=U64):
    return k * u / (1 - k * u)


def slots(n):
    return -(-n // S)


def frames(n):
    return -(-n // HOP)


def max_regions(n):
    return (frames(n) + 1) // 2


def params(top_db=40.0, floor_db=-70.0, min_sil=10, pad=5, lead=1200, trail=2400, max_pause=-1):
    """The device's per-clip parameters: (rel, floor_e, min_sil, pad, lead, trail, max_pause)."""
    return (10.0 ** (-top_db / 10.0), FRAME * 10.0 ** (floor_db / 10.0), int(min_sil), int(pad), int(lead), int(trail), int(max_pause))


def params_ok(n, p):
    rel, floor_e, min_sil, pad, lead, trail, M = p
    return (0.0 <= rel <= 1.0 and 0.0 <= floor_e < math.inf and 0 <= min_sil <= MAX_FRAMES_PARAM and 0 <= pad <= MAX_FRAMES_PARAM and
            -1 <= lead <= MAX_SAMPLES and -1 <= trail <= MAX_SAMPLES and (M == -1 or X <= M <= MAX_SAMPLES))


def energies(x):
    """Exact frame energies, rounded once: math.fsum over the exact squares (a f32 squared is exact in f64) of the frame's samples."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    sq = x * x
    return np.array([math.fsum(sq[f * HOP:f * HOP + FRAME]) for f in range(frames(len(x)))], dtype=np.float64)


def band(e):
    """|e_dev - e| <= band(e); one more operation than the device's for the reference's own rounding."""
    return gamma(K_OPS + 1) * e


def activity(e, rel, floor_e):
    """Frame energies -> (active flags, undecided flags, E).  A frame is undecided when a device energy inside its band could fall on the
    other side of a threshold computed from a device E inside its band (the product's rounding included)."""
    E = float(e.max()) if len(e) else 0.0
    thr = max(floor_e, rel * E)
    g = gamma(K_OPS + 3)
    thr_lo, thr_hi = max(floor_e, rel * E * (1 - g)), max(floor_e, rel * E * (1 + g))
    active = e > thr
    undecided = (e * (1 + g) > thr_lo) & (e * (1 - g) <= thr_hi)
    return active, undecided, E


def label(active, min_sil, pad):
    """Bridge the gaps between active frames that are shorter than min_sil, then dilate by pad."""
    a = [bool(v) for v in active]
    F = len(a)
    idx = [f for f in range(F) if a[f]]
    for p, q in zip(idx, idx[1:]):
        if q - p - 1 < min_sil:
            for f in range(p + 1, q):
                a[f] = True
    out = [False] * F
    for f in range(F):
        if a[f]:
            for g in range(max(0, f - pad), min(F, f + pad + 1)):
                out[g] = True
    return out


def label_closed(active, min_sil, pad):
    """The device's closed form: prev / next active frame."""
    F = len(active)
    prev, nxt = [-1] * F, [None] * F
    last = -1
    for f in range(F):
        last = f if active[f] else last
        prev[f] = last
    last = None
    for f in range(F - 1, -1, -1):
        last = f if active[f] else last
        nxt[f] = last
    out = []
    for f in range(F):
        p, q = prev[f], nxt[f]
        hp, hq = p >= 0, q is not None
        out.append(bool(active[f]) or (hp and hq and q - p - 1 < min_sil) or (hp and f - p <= pad) or (hq and q - f <= pad))
    return out


def regions(labels, n):
    out, f, F = [], 0, len(labels)
    while f < F:
        if labels[f]:
            g = f
            while g < F and labels[g]:
                g += 1
            out.append((f * HOP, min(g * HOP, n)))
            f = g
        else:
            f += 1
    return out


def cut_lengths(M):
    """(M1, M2): what is kept of a cut gap's head and tail; M1 + M2 - X = M."""
    return (M + X + 1) // 2, (M + X) // 2


def plan(n, regs, lead, trail, M):
    """Regions and the edit's parameters -> (segments [(o, i, l)], n_out, D0, Dt).  Built as a walk over the kept pieces of the input, not
    from prefix sums."""
    if not regs:
        return [(0, 0, n)], n, 0, 0
    G0, Gt = regs[0][0], n - regs[-1][1]
    D0 = G0 - lead if lead >= 0 and G0 > lead else 0
    Dt = Gt - trail if trail >= 0 and Gt > trail else 0
    segs, o, i = [], 0, D0
    for r in range(1, len(regs)):
        b, a = regs[r - 1][1], regs[r][0]
        if M >= 0 and a - b >= M + X:
            M1, M2 = cut_lengths(M)
            end = b + M1
            segs.append((o, i, end - i))
            o += end - i
            i = a - M2 + X
    end = n - Dt
    segs.append((o, i, end - i))
    return segs, o + end - i, D0, Dt


def weight(j):
    return (2 * j + 1) / (2.0 * X)


def render(x, segs, n_out, D0, Dt):
    """-> (y f64, bound f64, ops i32) per output sample.  ops = 0: a copy (bound 0: bit for bit)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y, bound, ops = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int32)
    tiny = 2.0 ** -150
    for k, (o, i, l) in enumerate(segs):
        y[o:o + l] = x[i:i + l]
        if k + 1 < len(segs):
            j = np.arange(X)
            m = o + l - X + j
            head, tail = x[i + l - X + j], x[segs[k + 1][1] - X + j]
            w = weight(j)
            y[m] = head + w * (tail - head)
            bound[m] = gamma(3, U32) * (np.abs(w * (tail - head)) + np.abs(head)) + tiny
            ops[m] = 3
    xe = min(X, n_out)
    m = np.arange(n_out)
    fin = (m < xe) if D0 > 0 else np.zeros(n_out, dtype=bool)
    fout = (m >= n_out - xe) if Dt > 0 else np.zeros(n_out, dtype=bool)
    for sel, wt in ((fin, weight(m)), (fout, weight(n_out - 1 - m))):
        # the value's own error carries through the weight (w <= 1); the weight's division and the product add two operations
        bound[sel] = bound[sel] * (1 + gamma(2, U32)) + gamma(2, U32) * np.abs(y[sel] * wt[sel]) + tiny
        y[sel] *= wt[sel]
        ops[sel] += 2
    return y, bound, ops


def analyse(x, p):
    """A clip and its parameters -> everything the device reports, and what decides it."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    rel, floor_e, min_sil, pad, lead, trail, M = p
    if n == 0:
        return dict(status=EMPTY)
    if n > MAX_SAMPLES or not params_ok(n, p):
        return dict(status=REFUSED)
    e = energies(x)
    active, undecided, E = activity(e, rel, floor_e)
    labels = label(active, min_sil, pad)
    regs = regions(labels, n)
    segs, n_out, D0, Dt = plan(n, regs, lead, trail, M)
    status = SILENT if not active.any() else (OK if len(segs) > 1 or D0 or Dt else UNCHANGED)
    return dict(status=status, e=e, E=E, active=active, undecided=undecided, labels=labels, regions=regs, segments=segs, n_out=n_out,
                D0=D0, Dt=Dt)


def trim(x, p):
    """analyse plus the output: y (f64), bound, ops."""
    r = analyse(x, p)
    if r["status"] in (EMPTY, REFUSED):
        return r
    r["y"], r["bound"], r["ops"] = render(x, r["segments"], r["n_out"], r["D0"], r["Dt"])
    return r


def trim_f32(x, p):
    """The output in f32, by the header's f32 operations (numpy's float32 arithmetic; the FMA through f64, whose product is exact) ->
    (y f32, result dict).  What a reference-backed stage returns."""
    x = np.asarray(x, dtype=np.float32)
    r = analyse(x, p)
    if r["status"] in (EMPTY, REFUSED):
        return None, r
    segs, n_out = r["segments"], r["n_out"]
    y = np.zeros(n_out, dtype=np.float32)
    f32 = np.float32
    for k, (o, i, l) in enumerate(segs):
        y[o:o + l] = x[i:i + l]
        if k + 1 < len(segs):
            j = np.arange(X)
            head, tail = x[i + l - X + j], x[segs[k + 1][1] - X + j]
            w = (2 * j + 1).astype(f32) / f32(2 * X)
            y[o + l - X + j] = (w.astype(np.float64) * (tail - head).astype(np.float64) + head.astype(np.float64)).astype(f32)
    xe = min(X, n_out)
    m = np.arange(n_out)
    fin = (m < xe) & (r["D0"] > 0)
    fout = (m >= n_out - xe) & (r["Dt"] > 0)
    j, jm = m, n_out - 1 - m
    y[fin] = y[fin] * ((2 * j[fin] + 1).astype(f32) / f32(2 * X))
    y[fout] = y[fout] * ((2 * jm[fout] + 1).astype(f32) / f32(2 * X))
    return y, r


def map_sample(s, segs):
    """Brute force: the output position of every kept input sample, a cut sample lands on the next kept one (or the end)."""
    for o, i, l in segs:
        if i <= s < i + l:
            return o + (s - i)
    later = [o for o, i, l in segs if i > s]
    return min(later) if later else segs[-1][0] + segs[-1][2]


# ----------------------------------------------------------------------------------------- test clips
def speech(n, rng, level=0.5):
    """A burst at full level: a tone plus noise, no sample near zero energy over a frame."""
    t = np.arange(n)
    return (level * (0.6 * np.sin(2 * np.pi * 220.0 / SAMPLE_RATE * t + rng.uniform(0, 6.28)) + 0.4 * rng.uniform(-1, 1, n))).astype(np.float32)


def build(parts, seed):
    """parts: [('s', n) speech | ('z', n) exact zeros | ('l', n) noise 60 dB below the speech] -> f32 clip."""
    rng = np.random.default_rng(seed)
    out = []
    for kind, n in parts:
        if kind == "s":
            out.append(speech(n, rng))
        elif kind == "z":
            out.append(np.zeros(n, dtype=np.float32))
        else:
            out.append((0.5e-3 * 0.4 * rng.uniform(-1, 1, n)).astype(np.float32))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)
