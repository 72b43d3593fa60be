"""fp64 reference of the WSOLA time-stretch along a rate map (include/tortoise_mi355x_tsw.h) and the seeded map family the CPU and GPU tests
share.

Everything but the nominal analysis position is tests/tsm_reference.py's: the clip family, the window, the tie rule, the admissible set, and
the two f32 bounds (the score bound and the 4 u sample bound; the operation counts do not change, a frame sums the same W terms).  The
table's integers are restated here on their own, so that tortoise_tts_amd/stretch.py, the library and this file are three spellings that
the tests compare.
"""
import functools

import numpy as np

from tests.tsm_reference import EPS, HS, RATE_MAX, RATE_MIN, RATE_ONE, SEARCH, U, W, admissible_set, clip, pick, take, window

MAX_SEGMENTS = 64
MIN_SEGMENT = 2

LENGTHS = (769, 1153, 2400, 5000, 9001, 12000)
SEEDS = (0, 1)


def advance(length, rq):
    return (length * rq + 32768) >> 16


def plan(n, segments):
    """Input-domain segments [(b_i, rq_i)] -> the table [(m_i, a_i, rq_i)], every length measured from the achieved a_i."""
    assert 1 <= len(segments) <= MAX_SEGMENTS and segments[0][0] == 0
    ends = [b for b, _ in segments[1:]] + [n]
    assert all(e - b >= MIN_SEGMENT for (b, _), e in zip(segments, ends)) and all(RATE_MIN <= rq <= RATE_MAX for _, rq in segments)
    table, m, a = [], 0, 0
    for (b, rq), end in zip(segments, ends):
        table.append((m, a, rq))
        L = max(1, ((end - a) * RATE_ONE + rq // 2) // rq)
        m, a = m + L, a + advance(L, rq)
    return table


def out_samples(n, table):
    m, a, rq = table[-1]
    return m + max(1, ((n - a) * RATE_ONE + rq // 2) // rq)


def frames(n, table):
    return -(-out_samples(n, table) // HS) + 1


def nominal(k, table):
    m = (k - 1) * HS
    i = max(j for j, row in enumerate(table) if row[0] <= m)
    return table[i][1] + advance(m - table[i][0], table[i][2])


def positions(table, offsets):
    """p_k of every frame from the chosen offsets (p_0 = -Hs)."""
    return np.array([-HS] + [nominal(k, table) + int(offsets[k]) for k in range(1, len(offsets))], dtype=np.int64)


def frame_scores(x, table, k, p_prev):
    """Frame k >= 1 after a frame at p_prev -> (s, bound), fp64 [512] over the offsets -256 .. 255."""
    x = np.asarray(x, dtype=np.float64)
    tpl = take(x, p_prev + HS, W)
    win = np.lib.stride_tricks.sliding_window_view(take(x, nominal(k, table) - SEARCH, W + 2 * SEARCH - 1), W)
    c = win @ tpl
    e = (win * win).sum(axis=1)
    root = np.sqrt(e + EPS)
    s = c / root
    bound = W * U * (np.abs(win) @ np.abs(tpl)) / root + np.abs(s) * (W * U / 2 + 4 * U)
    return s, bound


def overlap_add(x, table, offsets, w=None):
    """fp64 overlap-add of the frames at `offsets` -> (y, bound), both [n_out]."""
    x = np.asarray(x, dtype=np.float64)
    w = window() if w is None else w
    n_out, p = out_samples(len(x), table), positions(table, offsets)
    K = len(offsets)
    assert K == frames(len(x), table)
    y, mag = np.zeros((K + 1) * HS), np.zeros((K + 1) * HS)
    for k in range(K):
        seg = w * take(x, int(p[k]), W)
        y[k * HS:k * HS + W] += seg
        mag[k * HS:k * HS + W] += np.abs(seg)
    return y[HS:HS + n_out], 4 * U * mag[HS:HS + n_out]


def stretch(x, table):
    """The reference: dict(y, offsets, unambiguous [K] - no other offset of the frame is admissible)."""
    x = np.asarray(x, dtype=np.float64)
    K = frames(len(x), table)
    offsets, unamb, p = [0], [True], -HS
    for k in range(1, K):
        s, bound = frame_scores(x, table, k, p)
        d = pick(s)
        offsets.append(d)
        unamb.append(int(admissible_set(s, bound).sum()) == 1)
        p = nominal(k, table) + d
    offsets = np.array(offsets, dtype=np.int32)
    return dict(y=overlap_add(x, table, offsets)[0], offsets=offsets, unambiguous=np.array(unamb))


def check(x, table, y_dev, offsets_dev):
    """tsm_reference.check along a table: every device choice against the device's own history, every output sample against the fp64
    overlap-add of the device's offsets -> dict(inadmissible frames, bad samples, the worst shares of the two bounds used)."""
    x64 = np.asarray(x, dtype=np.float64)
    offsets_dev = np.asarray(offsets_dev)
    assert len(offsets_dev) == frames(len(x64), table) and offsets_dev[0] == 0
    assert np.all((offsets_dev >= -SEARCH) & (offsets_dev < SEARCH))
    p = positions(table, offsets_dev)
    bad_frames, score_share = [], 0.0
    for k in range(1, len(offsets_dev)):
        s, bound = frame_scores(x64, table, k, int(p[k - 1]))
        i = int(offsets_dev[k]) + SEARCH
        short = (s - bound).max() - s[i]
        if short > bound[i]:
            bad_frames.append(k)
        if short > 0:
            score_share = max(score_share, float(short / bound[i]) if bound[i] > 0 else np.inf)
    y, ybound = overlap_add(x64, table, offsets_dev)
    err = np.abs(np.asarray(y_dev, dtype=np.float64) - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        y_share = float(np.max(np.where(ybound > 0, err / ybound, np.where(err > 0, np.inf, 0.0))))
    return dict(inadmissible=bad_frames, bad_samples=int((err > ybound).sum()), score_share=score_share, y_share=y_share)


def rq_of(rate):
    return int(round(rate * RATE_ONE))


def family_maps(n, seed):
    """The maps of a clip of n samples: [(name, input-domain segments)]."""
    maps = [("slow_fast", [(0, rq_of(0.5)), (n // 2, rq_of(2.0))]),
            ("fast_slow", [(0, rq_of(2.0)), (n // 2, rq_of(0.5))]),
            ("thirds", [(0, rq_of(0.8)), (n // 3, rq_of(1.25)), (2 * n // 3, rq_of(1.0))])]
    if n >= 1153:
        maps.append(("borders", [(0, rq_of(1.25)), (2 * HS, rq_of(0.8)), (2 * HS + 100, rq_of(2.0)), (n - 50, rq_of(0.5))]))
    rng = np.random.default_rng(9100 + 17 * seed + n)
    S = min(MAX_SEGMENTS, n // 60)
    cuts = np.sort(rng.choice(np.arange(1, n - 1 - S), S - 1, replace=False)) + np.arange(1, S)  # gaps of at least 2, the last one too
    maps.append(("random", [(int(b), int(rng.integers(RATE_MIN, RATE_MAX + 1))) for b in [0] + cuts.tolist()]))
    return maps


FAMILY = tuple((n, s, name) for s in SEEDS for n in LENGTHS for name, _ in family_maps(n, s))
FAMILY_SEGMENTS = tuple(tuple(segments) for s in SEEDS for n in LENGTHS for _, segments in family_maps(n, s))  # the segments of every FAMILY entry


@functools.lru_cache(maxsize=None)
def family_reference():
    """[(x f32, table, reference dict)] for FAMILY, computed once per process and shared (read-only)."""
    out = []
    for (n, s, _), segments in zip(FAMILY, FAMILY_SEGMENTS):
        x = clip(n, s)
        x.setflags(write=False)
        table = plan(n, list(segments))
        out.append((x, table, stretch(x, table)))
    return tuple(out)
