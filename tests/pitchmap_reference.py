"""fp64 reference of the resampler along a pitch map (include/tortoise_mi355x_rsw.h), the f32 error bound of every output sample, and the
seeded map family the CPU and GPU tests share.

Nothing here is tuned.  The table, cq, H, c32, gamma and the clips are tests/resample_reference.py's; the plan and n_out are the header's
integers in Python integers; resample_map is the header's formula literally, the per-tap division included; and the bound of a sample is
resample_reference.resample's, with the N = 2 H + 2 and c32 of the sample's own segment:
    |y_f32 - y| <= sum_j |x_j| (eh_j (1 + gamma_N) + |h_j| gamma_N) + N 2^-149,   eh_j = gamma_3 c32 (|a (t1 - t0)| + |v|)
(the position is integer arithmetic and exact, so a border adds no error of its own)."""
import functools

import numpy as np

from tests import resample_reference as R

MAX_SEGMENTS, MIN_SEGMENT = 64, 2
P_MIN, P_MAX = 32768, 131072
Q = R.PITCH_ONE


def ratio_ok(P):
    return P_MIN <= P <= P_MAX


def t_of(row):
    return row[1] * 65536 + row[2]


def out_samples(n, table):
    """n_out = m_(S-1) + ceil((n 65536 - t_(S-1)) / P_(S-1)), or 0 for a table that breaks a rule."""
    S = len(table)
    if n < 1 or n > R.MAX_SAMPLES or S < 1 or S > MAX_SEGMENTS:
        return 0
    if tuple(table[0][:3]) != (0, 0, 0):
        return 0
    for i, row in enumerate(table):
        if not ratio_ok(row[3]) or row[1] < 0 or not 0 <= row[2] < 65536:
            return 0
        if i + 1 < S:
            nxt = table[i + 1]
            if nxt[0] <= row[0] or t_of(row) + (nxt[0] - row[0]) * row[3] != t_of(nxt):
                return 0
    m, t, P = table[-1][0], t_of(table[-1]), table[-1][3]
    if t >= n * 65536:
        return 0
    return m + (n * 65536 - t + P - 1) // P


def plan(n, segments):
    """[(b_i, P_i)] -> the table: m_0 = t_0 = 0, L_i = max(1, ceil((b_(i+1) 65536 - t_i) / P_i)), t_(i+1) by continuity."""
    S = len(segments)
    assert 1 <= n <= R.MAX_SAMPLES and 1 <= S <= MAX_SEGMENTS and segments[0][0] == 0
    ends = [b for b, _ in segments[1:]] + [n]
    assert all(e - b >= MIN_SEGMENT and ratio_ok(P) for (b, P), e in zip(segments, ends))
    table, m, t = [], 0, 0
    for i, (b, P) in enumerate(segments):
        table.append((m, t >> 16, t & 65535, P))
        if i + 1 < S:
            L = max(1, (segments[i + 1][0] * 65536 - t + P - 1) // P)
            m, t = m + L, t + L * P
    return table


def table_from_outputs(borders, ratios):
    """A table whose segments start at the OUTPUT samples `borders` (the first one 0): t by continuity."""
    table, t = [], 0
    for i, (m, P) in enumerate(zip(borders, ratios)):
        if i:
            t += (m - borders[i - 1]) * ratios[i - 1]
        table.append((m, t >> 16, t & 65535, P))
    return table


def resample_map(x, table, bound=True):
    """x: f32 (or f32-valued) samples [n] along `table` -> (y fp64 [n_out], the bound on |y_f32 - y| [n_out] or None): the header's formula
    literally - per output its segment, pos = t_i + (m - m_i) P_i, index pos >> 16, phase pos & 65535, then the rs header's taps with the
    cq, H and c32 of (P_i, 65536), the division of every tap included."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    n_out = out_samples(n, table)
    assert n_out > 0
    tab = R.table()
    y = np.empty(n_out)
    b = np.empty(n_out) if bound else None
    HP = R.half_width(R.cutoff_q(P_MAX, Q)) + 2
    xp = np.concatenate([np.zeros(HP), x, np.zeros(HP + 2)])  # xp[j + HP] = x[j], zeros outside [0, n)
    for s, row in enumerate(table):
        m_lo, m_hi = row[0], table[s + 1][0] if s + 1 < len(table) else n_out
        P = row[3]
        cq, c32 = R.cutoff_q(P, Q), R.cutoff_f32(P, Q)
        H = R.half_width(cq)
        N = 2 * H + 2
        d = np.arange(-H, H + 2, dtype=np.int64)
        m = np.arange(m_lo, m_hi, dtype=np.int64)
        pos = t_of(row) + (m - m_lo) * P
        i, r = pos >> 16, pos & 65535
        assert (i < n).all()
        u = (np.abs(d[None, :] * Q - r[:, None]) * cq) // Q
        k = u >> 16
        a = (u & 65535) / 65536.0
        live = k < R.Z * R.L
        kc = np.where(live, k, 0)
        t0, t1 = tab[kc], tab[kc + 1]
        dt = a * (t1 - t0)
        v = np.where(live, t0 + dt, 0.0)
        h = c32 * v
        xs = xp[(i[:, None] + d[None, :]) + HP]
        y[m_lo:m_hi] = (h * xs).sum(axis=1)
        if bound:
            eh = np.where(live, R.gamma(3) * c32 * (np.abs(dt) + np.abs(v)), 0.0)
            b[m_lo:m_hi] = (np.abs(xs) * (eh * (1.0 + R.gamma(N)) + np.abs(h) * R.gamma(N))).sum(axis=1) + N * 2.0 ** -149
    return y, b


# ----------------------------------------------------------------------------------------- the map family
def random_segments(rng, n, S):
    """S input-domain segments of a clip of n >= 2 S samples, each of at least 2 samples, ratios including both ends."""
    cuts = np.sort(rng.choice(np.arange(1, n - S), S - 1, replace=False)) + np.arange(1, S) if S > 1 else np.zeros(0, np.int64)
    pick = lambda: int(rng.choice([P_MIN, P_MAX])) if rng.random() < 0.25 else int(rng.integers(P_MIN, P_MAX + 1))
    return [(int(b), pick()) for b in [0] + cuts.tolist()]


def _family():
    fam = []
    for n in (37, 1000, 5000):
        for S in (1, 2, 3, 8, 64):
            if n >= 2 * S:
                rng = np.random.default_rng(100 * n + S)
                fam.append((f"n{n}_S{S}", n, 1, plan(n, random_segments(rng, n, S))))
    # the extremes on adjacent segments, both ways
    fam.append(("extremes_up_down", 1000, 2, plan(1000, [(125 * i, (P_MAX, P_MIN)[i % 2]) for i in range(8)])))
    fam.append(("extremes_down_up", 5000, 2, plan(5000, [(0, P_MIN), (2500, P_MAX)])))
    # a segment of exactly one output sample
    fam.append(("one_output", 1000, 3, table_from_outputs([0, 400, 401, 700], [65536, P_MAX, P_MIN, 77936])))
    # 64 segments of one output each on a clip of 37 samples (half a sample per output: 32 samples in all)
    fam.append(("n37_64_single_outputs", 37, 3, table_from_outputs(list(range(64)), [P_MIN] * 64)))
    # borders at the outputs 1023, 1024 and 1025: the tile border
    fam.append(("tile_border", 5000, 4, table_from_outputs([0, 1023, 1024, 1025], [55109, P_MAX, P_MIN, 98304])))
    fam.append(("border_at_1024", 5000, 4, table_from_outputs([0, 1024], [P_MAX, P_MIN])))
    fam.append(("border_at_1023", 5000, 5, table_from_outputs([0, 1023, 2047], [77936, 55109, P_MAX])))
    # a last segment that starts two samples before the clip's end
    for n in (37, 1000, 5000):
        fam.append((f"last_of_2_n{n}", n, 6, plan(n, [(0, 77936), (n - 2, P_MAX if n != 1000 else P_MIN)])))
    return fam


FAMILY = _family()


@functools.lru_cache(maxsize=None)
def family_reference():
    """[(name, x f32 [n], table, y fp64, bound)] of FAMILY: computed once, shared, read-only."""
    out = []
    for name, n, seed, table in FAMILY:
        x = R.clip(n, seed)
        y, b = resample_map(x, table)
        for a in (x, y, b):
            a.setflags(write=False)
        out.append((name, x, table, y, b))
    return out
