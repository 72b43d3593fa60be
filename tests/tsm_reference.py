"""fp64 reference of the WSOLA time-stretch (include/tortoise_mi355x_tsm.h), the f32 error bounds of its scores and output samples, and
the seeded clip family the CPU and GPU tests share.

Nothing here is tuned.  The constants are the header's; the bounds follow from the unit roundoff of f32, u = 2^-24:

  score    the device forms c = sum_j t_j x_j and E = sum_j x_j^2 with one fused multiply-add per term (one rounding each) in sums of depth at
           most W, so |c_f32 - c| <= W u sum_j |t_j x_j| and E_f32 = E (1 + e), |e| <= W u (Higham, Accuracy and Stability, 3.1; any summation
           order of W terms obeys it, and the device's two half-sums of W / 2 + 1 leave the second-order terms to spare).  Adding eps, the
           correctly rounded square root and the correctly rounded division add u / 4 + u / 2 + u / 2 relative, and the error of E reaches the
           score halved by the root:
               |s_f32 - s| <= W u sum_j |t_j x_j| / sqrt(E + eps) + |s| (W u / 2 + 4 u)
  sample   y = w1 x1 + w2 x2 with the window rounded to f32 (u / 2 each), one rounded product and one fused multiply-add:
               |y_f32 - y| <= 4 u (|w1 x1| + |w2 x2|)
  fp64     the reference's own error is 2^-29 of these and is ignored.

Near-ties are real - voiced speech correlates almost as well one pitch period further - so a device choice is judged by `admissible`:
with the device's own previous position, no other offset may beat it by more than the two bounds allow.
"""
import functools

import numpy as np

W, HS, SEARCH = 768, 384, 256          # TT_TSM_WINDOW, TT_TSM_HOP, TT_TSM_SEARCH
RATE_ONE, RATE_MIN, RATE_MAX = 65536, 32768, 131072
SAMPLE_RATE = 24000
EPS = 1e-20
U = 2.0 ** -24
DELTAS = np.arange(-SEARCH, SEARCH)
TIE_ORDER = np.where(DELTAS < 0, -2 * DELTAS - 1, 2 * DELTAS)  # 0, -1, 1, -2, 2, ...: the smaller wins among equal scores

LENGTHS = (1, 300, 767, 768, 769, 1153, 5000, 9001, 12000)
RATES = (0.5, 0.8, 1.25, 2.0)
SEEDS = (0, 1)
FAMILY = tuple((n, r, s) for s in SEEDS for n in LENGTHS for r in RATES)


def rate_q(rate):
    return int(round(float(rate) * RATE_ONE))


def out_samples(n, rq):
    return max(1, (n * RATE_ONE + rq // 2) // rq)


def frames(n, rq):
    return -(-out_samples(n, rq) // HS) + 1


def nominal(k, rq):
    return ((k - 1) * HS * rq + 32768) >> 16


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


def take(x, start, count):
    """x[start : start + count] with zeros outside [0, n)."""
    out = np.zeros(count, dtype=x.dtype)
    lo, hi = max(start, 0), min(start + count, len(x))
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def positions(rq, offsets):
    """p_k of every frame from the chosen offsets (p_0 = -Hs)."""
    return np.array([-HS] + [nominal(k, rq) + int(offsets[k]) for k in range(1, len(offsets))], dtype=np.int64)


def frame_scores(x, rq, k, p_prev):
    """Frame k >= 1 after a frame at p_prev -> (s, bound), fp64 [512] over the offsets -256 .. 255."""
    x = np.asarray(x, dtype=np.float64)
    tpl = take(x, p_prev + HS, W)
    win = np.lib.stride_tricks.sliding_window_view(take(x, nominal(k, rq) - SEARCH, W + 2 * SEARCH - 1), W)
    c = win @ tpl
    e = (win * win).sum(axis=1)
    root = np.sqrt(e + EPS)
    s = c / root
    bound = W * U * (np.abs(win) @ np.abs(tpl)) / root + np.abs(s) * (W * U / 2 + 4 * U)
    return s, bound


def pick(s):
    """argmax with the tie rule: the smaller |d|, and of +-d the negative one."""
    best = np.flatnonzero(s == s.max())
    return int(DELTAS[best[np.argmin(TIE_ORDER[best])]])


def admissible_set(s, bound):
    return (s + bound) >= (s - bound).max()


def admissible(x, rq, k, p_prev, delta):
    s, bound = frame_scores(x, rq, k, p_prev)
    return bool(admissible_set(s, bound)[delta + SEARCH])


def overlap_add(x, rq, offsets, w=None):
    """fp64 overlap-add of the frames at `offsets` -> (y, bound), both [n_out]."""
    x = np.asarray(x, dtype=np.float64)
    w = window() if w is None else w
    n_out, p = out_samples(len(x), rq), positions(rq, offsets)
    K = len(offsets)
    assert K == frames(len(x), rq)
    y, mag = np.zeros((K + 1) * HS), np.zeros((K + 1) * HS)
    for k in range(K):
        seg = w * take(x, int(p[k]), W)
        y[k * HS:k * HS + W] += seg          # frame k covers the output [(k - 1) Hs, (k + 1) Hs): index + Hs here
        mag[k * HS:k * HS + W] += np.abs(seg)
    return y[HS:HS + n_out], 4 * U * mag[HS:HS + n_out]


def stretch(x, rq):
    """The reference: dict(y, offsets, unambiguous [K] - no other offset of the frame is admissible)."""
    x = np.asarray(x, dtype=np.float64)
    K = frames(len(x), rq)
    offsets, unamb, p = [0], [True], -HS
    for k in range(1, K):
        s, bound = frame_scores(x, rq, k, p)
        d = pick(s)
        offsets.append(d)
        unamb.append(int(admissible_set(s, bound).sum()) == 1)
        p = nominal(k, rq) + d
    offsets = np.array(offsets, dtype=np.int32)
    return dict(y=overlap_add(x, rq, offsets)[0], offsets=offsets, unambiguous=np.array(unamb))


def check(x, rq, y_dev, offsets_dev):
    """Steps 1 and 2 of the protocol for one clip: every device choice against the device's own history, every output sample against the
    fp64 overlap-add of the device's offsets -> dict(inadmissible frames, bad samples, the worst shares of the two bounds used)."""
    x64 = np.asarray(x, dtype=np.float64)
    offsets_dev = np.asarray(offsets_dev)
    assert len(offsets_dev) == frames(len(x64), rq) and offsets_dev[0] == 0
    assert np.all((offsets_dev >= -SEARCH) & (offsets_dev < SEARCH))
    p = positions(rq, offsets_dev)
    bad_frames, score_share = [], 0.0
    for k in range(1, len(offsets_dev)):
        s, bound = frame_scores(x64, rq, k, int(p[k - 1]))
        i = int(offsets_dev[k]) + SEARCH
        short = (s - bound).max() - s[i]  # what the device's choice lacks against the best guaranteed score
        if short > bound[i]:
            bad_frames.append(k)
        if short > 0:
            score_share = max(score_share, float(short / bound[i]) if bound[i] > 0 else np.inf)
    y, ybound = overlap_add(x64, rq, offsets_dev)
    err = np.abs(np.asarray(y_dev, dtype=np.float64) - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        y_share = float(np.max(np.where(ybound > 0, err / ybound, np.where(err > 0, np.inf, 0.0))))
    return dict(inadmissible=bad_frames, bad_samples=int((err > ybound).sum()), score_share=score_share, y_share=y_share)


def emulate_f32(x, rq):
    """The algorithm in f32 with another summation order than the device's (BLAS dot products, pairwise sums, no fused operations)."""
    x = np.asarray(x, dtype=np.float32)
    w = window().astype(np.float32)
    n, K, n_out = len(x), frames(len(x), rq), out_samples(len(x), rq)
    offsets, p = [0], -HS
    y = np.zeros((K + 1) * HS, dtype=np.float32)
    y[:W] += w * take(x, -HS, W)
    for k in range(1, K):
        tpl = take(x, p + HS, W)
        win = np.lib.stride_tricks.sliding_window_view(take(x, nominal(k, rq) - SEARCH, W + 2 * SEARCH - 1), W)
        s = (win @ tpl) / np.sqrt((win * win).sum(axis=1, dtype=np.float32) + np.float32(EPS))
        d = pick(s)
        offsets.append(d)
        p = nominal(k, rq) + d
        y[k * HS:k * HS + W] += w * take(x, p, W)
    return y[HS:HS + n_out], np.array(offsets, dtype=np.int32)


def clip(n, seed):
    """Speech-like f32 audio at 24 kHz: six gliding harmonics of a 90 - 260 Hz fundamental under a syllabic envelope, unvoiced noise stretches
    instead of them in about a quarter of the 100 ms segments, and a -40 dB noise floor."""
    rng = np.random.default_rng(7000 + 131 * seed + n)
    t = np.arange(n) / SAMPLE_RATE
    knots = max(2, int(np.ceil(n / (0.1 * SAMPLE_RATE))) + 1)
    at = np.arange(knots) * 0.1
    f0 = np.interp(t, at, rng.uniform(90.0, 260.0, knots))
    phase = 2.0 * np.pi * np.cumsum(f0) / SAMPLE_RATE
    voiced = sum(rng.uniform(0.5, 1.0) / h * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 7))
    unvoiced = rng.random(knots) < 0.25
    noisy = unvoiced[np.minimum((t / 0.1).astype(np.int64), knots - 1)]
    body = np.where(noisy, 0.5 * rng.standard_normal(n), voiced)
    env = np.maximum(0.55 + 0.45 * np.sin(2.0 * np.pi * rng.uniform(3.5, 5.5) * t + rng.uniform(0, 2 * np.pi)), 0.1)
    return (0.3 * env * body + 0.01 * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family_reference():
    """[(x f32, rq, reference dict)] for FAMILY, computed once per process and shared (read-only)."""
    out = []
    for n, rate, seed in FAMILY:
        x, rq = clip(n, seed), rate_q(rate)
        x.setflags(write=False)
        out.append((x, rq, stretch(x, rq)))
    return tuple(out)
