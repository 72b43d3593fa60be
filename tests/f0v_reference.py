"""fp64 reference of the Viterbi F0 path (include/tortoise_mi355x_f0v.h), built on tests/f0_reference.py: the candidates of a
frame, the recursion in the header's operation order (so that the path kernel is compared bit for bit), the test of whether a frame's
candidate set could differ inside the d' bound, and the margin by which a clip's path wins.

Ambiguity of a frame.  The device's d'(tau) lies within e(tau) = E_DP d'(tau) of the reference's (f0_reference; 0 where it is exact).  A
comparison d'(a) < d'(b) is certain when the two intervals do not meet (or both values are exact).  A lag of [lo, hi] is a CERTAIN dip when
both of its comparisons certainly hold and a POSSIBLE dip when neither certainly fails; the device's dips lie between the two sets.  The
device keeps the 7 of its dips that read smallest.  A possible dip is SURELY KEPT when it is a certain dip and at most 6 other possible dips
have a lower end at or below its upper end; it is SURELY DROPPED when at least 7 certain dips have an upper end below its lower end.  The
possible dips that are neither are IN DOUBT: the device's kept lags and candidates()' can differ in those alone.  The kept set is certain -
the frame unambiguous - iff no dip is in doubt and P does not lie within gamma_32 of floor_e.  That is "any dip comparison could
flip, or the rank of the 7th and 8th dip could", without the comparisons whose flip cannot change the seven kept lags: a flip at a maximum
of d' makes no dip, and a shallow dip with seven certain ones below it is dropped either way.  The states are numbered by lag, so the order
of the kept seven among themselves does not matter.

Margin of a path.  Let a[t][s] be the forward costs and b[t][s] the cheapest completion from (t, s); through(t, s) = a + b is the cost of the
best path through (t, s), and the best path costs `cost`.  The device runs the same recursion on candidate tables whose dp differ from the
reference's by at most E_DP dp each, in f64 with at most 4 rounded operations a frame on a path (the product and the sum of local, the sum
with trans, the sum with local).  For ANY path p: |cost_dev(p) - cost_ref(p)| <= B with
  B = E_DP sum_t max_s dp_t(s)  +  4 F 2^-53 (cost + F max local)
(the first term: every frame contributes one dp, with error at most E_DP of the frame's largest; the second: 4 F roundings, each relative
2^-53 of a partial sum no larger than the total, which is at most cost + F max local for any path within reach of winning - the same
constants bound this reference's own roundings, hence the factor that 2 B below has over B).  So if every off-path (t, s) has
through(t, s) > cost + 2 B, every other path costs more than the best on the device too: the device's states are the reference's, and
|cost_dev - cost| <= B.

Dips in doubt far up the table.  Counting every doubt - "no frame's candidate set is ambiguous" - 29 of the 32 clips of the family below would
be ambiguous, every planted one among them: a harmonic tone's d' carries shallow ripples far up the table (d' of 1 .. 2) whose minimum
cannot be placed to one lag inside E_DP, and where fewer than 7 dips exist every one of them is kept.  Such a dip can change the NUMBER of
a state (states count by ascending lag) but never the path.  List, for every frame, every lag the reference keeps and every lag in doubt,
each at the lower end of its d', and run the recursion forwards and backwards over these wider tables (through_lower): whatever tables the
device has made are part of them with costs no smaller, so through_lower(t, l) bounds from below, up to the f64 roundings that B's second
term counts, what ANY path through (t, l) costs on the device.  The reference's best path costs the device at most cost + B.  So while
through_lower(t, l) > cost + 2 B for every lag l in doubt of frame t, no cheapest path of the device holds a state in doubt - also not one
that holds several of them, since the wider tables hold them all - and the frame is PATH-SAFE.  What is left to compare are paths through
the surely kept states, which the reference's tables hold lag for lag with d' inside E_DP: the margin argument above runs over those, the
first term of B, taken over the reference's states, covers every d' on such a path whatever else the device keeps, and `through` needs
no state the reference lacks.  (A best path that itself passes a lag in doubt fails the condition, as it must.)  A clip is
UNAMBIGUOUS iff every frame is unambiguous or path-safe and the margin holds; on it the device's lag, voicing, f0, aper and cost are
compared on every frame, and its state numbers on the frames with no dip in doubt - the frames that count would cover too.  This compares
more clips (30 of 32 against 3)."""
import functools

import numpy as np

from tests import f0_reference as R
from tortoise_tts_amd import pitch as P

K, S, UNV = 7, 8, 7
L2 = np.asarray(P.LOG2_TABLE, dtype=np.float64)                      # the very doubles the handle is created with
COSTS = tuple(P.smooth_params(True))                                 # (oct, jump, vuv, uv)
DEFAULT = dict(lo=48, hi=400, thr=0.15, floor_e=R.W * 1e-5)
INF = float("inf")


def dip_flags(dp, lo, hi):
    """bool [hi - lo + 1]: lag tau is a dip iff d'(tau) < d'(tau-1) and (tau == T or d'(tau+1) >= d'(tau))."""
    tau = np.arange(lo, hi + 1)
    nxt = np.where(tau < R.T, dp[np.minimum(tau + 1, R.T)] >= dp[tau], True)
    return (dp[tau] < dp[tau - 1]) & nxt


def candidates(dp, Pw, lo, hi, floor_e):
    """One frame -> [(lag, d'(lag))] by ascending lag: the K dips with the smallest d', ties to the smaller lag; [] where P < floor_e."""
    if Pw < floor_e:
        return []
    lags = lo + np.nonzero(dip_flags(dp, lo, hi))[0]
    keep = sorted(lags.tolist(), key=lambda t: (dp[t], t))[:K]
    return [(t, float(dp[t])) for t in sorted(keep)]


def candidate_ambiguous(dp, e, Pw, lo, hi, floor_e):
    """Could the device's kept lags differ from candidates()' (the docstring's rule)? -> (ambiguous, the lags in doubt; None where the
    doubt is P against the floor)."""
    if Pw > 0 and floor_e > 0 and Pw * (1.0 - R.G_P) <= floor_e <= Pw * (1.0 + R.G_P):
        return True, None
    if Pw < floor_e:
        return False, []
    lo_v, hi_v = dp - e, dp + e
    tau = np.arange(lo, hi + 1)
    nx = np.minimum(tau + 1, R.T)
    exact_p, exact_n = (e[tau] == 0) & (e[tau - 1] == 0), (e[tau] == 0) & (e[nx] == 0)
    # d'(tau) < d'(tau-1)
    c1 = np.where(exact_p, dp[tau] < dp[tau - 1], hi_v[tau] < lo_v[tau - 1])
    p1 = np.where(exact_p, dp[tau] < dp[tau - 1], lo_v[tau] < hi_v[tau - 1])
    # d'(tau+1) >= d'(tau)
    c2 = np.where(tau < R.T, np.where(exact_n, dp[nx] >= dp[tau], lo_v[nx] > hi_v[tau]), True)
    p2 = np.where(tau < R.T, np.where(exact_n, dp[nx] >= dp[tau], hi_v[nx] >= lo_v[tau]), True)
    certain, possible = tau[c1 & c2], tau[p1 & p2]
    # of the possible dips: SURELY KEPT - a certain dip that at most 6 possible dips could rank before; SURELY DROPPED - at least 7 certain
    # dips rank before it whatever the device reads; the others are in doubt, and the two kept sets can differ in those alone
    doubt = []
    for l in possible.tolist():
        before = int(np.count_nonzero(lo_v[possible] <= hi_v[l])) - 1          # possible dips (other than l) that could read no larger
        surely_before = int(np.count_nonzero(hi_v[certain] < lo_v[l]))         # certain dips that read smaller whatever happens
        kept = bool((certain == l).any()) and before <= K - 1
        if not kept and surely_before < K:
            doubt.append(l)
    return bool(doubt), doubt


def tables(cands):
    """[[(lag, dp)]] of F frames -> (lag i32 [F, 8], dp f64 [F, 8]) in the device's layout, slots k .. 6 absent (lag 0); slot 7 is left 0."""
    F = len(cands)
    lag, dp = np.zeros((F, S), np.int32), np.zeros((F, S))
    for t, c in enumerate(cands):
        for s, (l, d) in enumerate(c):
            lag[t, s], dp[t, s] = l, d
    return lag, dp


def _costs(lag, dp, lo, costs):
    """Per frame: present bool [F, 8], local f64 [F, 8] (inf where absent), l2 f64 [F, 8] - the header's operations, one rounding each."""
    oct_, _, _, uv = costs
    present = (lag >= 1) & (lag <= R.T)
    present[:, UNV] = True
    l2 = np.where(present, L2[np.clip(lag, 0, R.T)], 0.0)
    l2[:, UNV] = 0.0
    local = dp + oct_ * (l2 - L2[lo])
    local[:, UNV] = uv
    return present, np.where(present, local, INF), l2


def _trans(l2j, l2s, costs):
    """f64 [8 (s), 8 (j)]: trans(j -> s)."""
    _, jump, vuv, _ = costs
    tr = jump * np.abs(l2s[:, None] - l2j[None, :])
    tr[UNV, :] = vuv
    tr[:, UNV] = vuv
    tr[UNV, UNV] = 0.0
    return tr


def viterbi_tables(lag, dp, lo, costs=COSTS, margin=False):
    """The recursion on tables (lag [F, 8], dp [F, 8]) -> (state i32 [F], cost) and, with margin=True, also through f64 [F, 8]."""
    F = lag.shape[0]
    present, local, l2 = _costs(np.asarray(lag), np.asarray(dp, dtype=np.float64), lo, costs)
    a = np.empty((F, S))
    bp = np.zeros((F, S), np.int64)
    a[0] = local[0]
    for t in range(1, F):
        v = a[t - 1][None, :] + _trans(l2[t - 1], l2[t], costs)
        v[:, ~present[t - 1]] = INF
        bp[t] = np.argmin(v, axis=1)  # (the first minimum: the smallest j)
        a[t] = np.where(present[t], local[t] + v[np.arange(S), bp[t]], INF)
    state = np.zeros(F, np.int32)
    state[F - 1] = int(np.argmin(a[F - 1]))
    cost = float(a[F - 1, state[F - 1]])
    for t in range(F - 1, 0, -1):
        state[t - 1] = bp[t, state[t]]
    if not margin:
        return state, cost
    b = np.zeros((F, S))
    for t in range(F - 2, -1, -1):
        w = _trans(l2[t], l2[t + 1], costs) + (local[t + 1] + b[t + 1])[:, None]  # [s' (next), s]
        b[t] = np.min(w, axis=0)
    return state, cost, a + b


def viterbi(cands, lo, costs=COSTS):
    """[[(lag, dp)]] by frame -> (state i32 [F], cost)."""
    return viterbi_tables(*tables(cands), lo, costs)


def through_lower(frames, lo, costs=COSTS):
    """frames: per frame [(lag, a lower end of its d')] of ANY number of voiced states (and "unvoiced", always) -> per frame the list of
    the cheapest cost of a path through each of those states.  With every kept and every doubtful lag of a frame listed at dp - e this is
    a lower bound, up to f64 rounding, of what any path costs on any tables the device can have made."""
    oct_, jump, vuv, uv = costs
    F = len(frames)
    l2 = [np.array([L2[l] for l, _ in fr] + [0.0]) for fr in frames]
    loc = [np.array([d + oct_ * (L2[l] - L2[lo]) for l, d in fr] + [uv]) for fr in frames]

    def trans(t):  # [state of frame t + 1, state of frame t]
        tr = jump * np.abs(l2[t + 1][:, None] - l2[t][None, :])
        tr[-1, :], tr[:, -1] = vuv, vuv
        tr[-1, -1] = 0.0
        return tr
    a, b = [loc[0]], [None] * F
    for t in range(1, F):
        a.append(loc[t] + (a[t - 1][None, :] + trans(t - 1)).min(axis=1))
    b[F - 1] = np.zeros(len(loc[F - 1]))
    for t in range(F - 2, -1, -1):
        b[t] = (trans(t) + (loc[t + 1] + b[t + 1])[:, None]).min(axis=0)
    return [a[t] + b[t] for t in range(F)]


def brute_force(cands, lo, costs=COSTS):
    """Every path over the present states, the recursion's operation order along each; ties to the path whose LAST states are smallest
    (the end state first, then each predecessor), as the backtrace resolves them."""
    lag, dp = tables(cands)
    present, local, l2 = _costs(lag, dp, lo, costs)
    F = lag.shape[0]
    best = {}
    # a[t][s] by exhaustive enumeration of the prefixes that end in (t, s): min over paths equals the recursion's min because + is monotone
    def paths(t, s):
        if t == 0:
            return [(float(local[0, s]), (s,))]
        out = []
        for j in range(S):
            if present[t - 1, j]:
                tr = float(_trans(l2[t - 1], l2[t], costs)[s, j])
                out += [(float(local[t, s]) + (c + tr), p + (s,)) for c, p in paths(t - 1, j)]
        return out
    allp = [cp for s in range(S) if present[F - 1, s] for cp in paths(F - 1, s)]
    cost = min(c for c, _ in allp)
    return cost, [p for c, p in allp if c == cost]


def track_smooth(x, lo=48, hi=400, thr=0.15, floor_e=R.W * 1e-5, costs=COSTS, plain=None):
    """A clip -> dict: plain (f0_reference.track), cands, cand_ambiguous bool [F], state, lag, f0, f0_bound, aper, aper_bound, voiced, cost,
    bound (B), margin (min off-path through - cost), unambiguous."""
    tr = R.track(x, lo, hi, thr, floor_e) if plain is None else plain
    dpr, e, Pw = tr["dprime"], tr["dprime_bound"], tr["power"]
    F = dpr.shape[0]
    cands = [candidates(dpr[f], Pw[f], lo, hi, floor_e) for f in range(F)]
    doubt = [candidate_ambiguous(dpr[f], e[f], Pw[f], lo, hi, floor_e) for f in range(F)]
    amb = np.array([d[0] for d in doubt])
    lag_t, dp_t = tables(cands)
    state, cost, through = viterbi_tables(lag_t, dp_t, lo, costs, margin=True)
    out = dict(thr=thr, floor_e=floor_e, plain=tr, cands=cands, cand_ambiguous=amb, state=state, cost=cost, lag=tr["lag"].copy(), f0=np.zeros(F), f0_bound=np.zeros(F),
               aper=tr["aper"].copy(), aper_bound=tr["aper_bound"].copy(), cand_f0=[[] for _ in range(F)], cand_f0_bound=[[] for _ in range(F)])
    for f in range(F):
        for l, _ in cands[f]:
            delta, db = R.refine(dpr[f], e[f], l)
            f0 = R.SR / (l + delta)
            out["cand_f0"][f].append(f0)
            out["cand_f0_bound"][f].append(None if db is None else R.SR * db / ((l + delta) * (l + delta - db)) + (R.U32 + 4 * R.U64) * f0 * 1.001)
        s = int(state[f])
        if s != UNV:
            l, d = cands[f][s]
            out["lag"][f], out["aper"][f] = l, d
            out["aper_bound"][f] = R.E_DP * d + R.U32 * (1.0 + R.E_DP) * d
            out["f0"][f], fb = out["cand_f0"][f][s], out["cand_f0_bound"][f][s]
            if fb is None:
                amb[f], fb = True, 0.0
            out["f0_bound"][f] = fb
    out["voiced"] = state != UNV
    _, local, _ = _costs(lag_t, dp_t, lo, costs)
    finite = np.where(np.isfinite(local), local, 0.0)
    B = R.E_DP * float(dp_t.max(axis=1).sum()) + 4 * F * R.U64 * (cost + F * float(finite.max()))
    off = np.isfinite(through)
    off[np.arange(F), state] = False
    margin = float((through[off] - cost).min()) if off.any() else INF
    # the frames whose kept set is in doubt only through dips that no cheapest path can hold (module docstring): every kept and every
    # doubtful lag at the lower end of its d', the cheapest path through each doubtful one against cost + 2 B
    wide = []
    for f in range(F):
        lags = sorted({l for l, _ in cands[f]} | set(doubt[f][1] or []))
        wide.append([(l, float(dpr[f][l] - e[f][l])) for l in lags])
    low = through_lower(wide, lo, costs)
    safe = np.ones(F, bool)
    for f in np.nonzero(amb)[0]:
        lags = doubt[f][1]
        at = {l: i for i, (l, _) in enumerate(wide[f])}
        safe[f] = lags is not None and all(low[f][at[l]] > cost + 2 * B for l in lags)
    out.update(bound=B, margin=margin, path_safe=safe, unambiguous=bool(safe.all() and margin > 2 * B))
    return out


def octave_jumps(f0, min_semitones=7.0):
    """pitch.F0Track.octave_jumps on a plain array."""
    return P.F0Track(np.asarray(f0, np.float32), np.zeros(len(f0)), np.zeros(len(f0))).octave_jumps(min_semitones)


# ------------------------------------------------------------------------------------------------------------------- the test signals
FAMILY_N = R.FAMILY_N
PLANT_SNR = 40.0
RUNS = ((9, 1), (22, 3), (37, 2))        # (first frame, frames) of the planted runs of an octave-above clip: separated, inside the clip
RUNS_BELOW = ((12, 1), (23, 1), (34, 1))  # an octave-below run is one frame (the docstring of planted_below says why)
BELOW_THR = 0.05                          # YIN's threshold for the octave-below clips (planted_below says why)
ODD_GAIN = 0.14                           # odd harmonics in an octave-above run
ODD_RAMP = 1200                           # samples of the raised-cosine ramp into and out of an octave-above run
PERIOD_GAIN = 0.7                         # every other period in an octave-below run
BELOW_PLATEAU, BELOW_RAMP = 900, 120      # samples of an octave-below stretch at full depth, and of its ramps


def _window(a, b, n, ramp):
    """f64 [n]: 1 over samples a .. b, a raised-cosine ramp of `ramp` samples on either side, 0 elsewhere."""
    w = np.zeros(n)
    w[a:b] = 1.0
    r = 0.5 - 0.5 * np.cos(np.pi * (np.arange(ramp) + 0.5) / ramp)
    w[a - ramp:a], w[b:b + ramp] = r, r[::-1]
    return w


def planted_above(f0, seed, n=FAMILY_N, snr_db=PLANT_SNR):
    """An eight-harmonic tone whose odd harmonics drop to ODD_GAIN over the samples that the frames of three runs read (x[f H - 720 ..
    + W + T)): there the half period is a dip below YIN's threshold and plain YIN, which takes the first such dip, reads the octave above.
    The drop is a raised-cosine ramp of ODD_RAMP samples (7.5 periods at 150 Hz; neighbouring ramps overlap and add): an amplitude that
    changes inside a window moves the minimum of d near the period, and the slower it changes the less - a step reads 3.6 cents off at
    150 Hz, this ramp 0.53, inside the 0.74 that tests/test_f0_cpu.py asserts at 40 dB."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / R.SR
    ph = rng.uniform(0, 2 * np.pi, 8)
    g = np.ones(n)
    for first, frames in RUNS:
        g -= (1.0 - ODD_GAIN) * _window(first * R.H - R.LEAD, (first + frames - 1) * R.H - R.LEAD + R.W + R.T, n, ODD_RAMP)
    x = sum((g if h % 2 == 0 else 1.0) * np.sin(2 * np.pi * f0 * (h + 1) * t + ph[h]) / (h + 1) for h in range(8))
    x = 0.25 * x / np.sqrt(np.mean(x * x))
    return (x + rng.standard_normal(n) * 0.25 * 10.0 ** (-snr_db / 20.0)).astype(np.float32)


def planted_below(f0, seed, n=FAMILY_N, snr_db=PLANT_SNR):
    """The tone with every other period scaled by PERIOD_GAIN = 0.7 over about the W samples a frame's window sums (BELOW_PLATEAU at full
    depth, centred on the window, ramps of BELOW_RAMP; a period takes the depth at its centre), three times: d'(period) rises there to about
    (1 - 0.7)^2 / (1 + 0.7^2) = 0.06 while the double period stays a perfect one, so a YIN whose threshold lies below that takes the double
    period in those frames and reads the octave below.  These two clips are therefore measured at threshold BELOW_THR = 0.05, inside the
    paper's and the API's range; at the default 0.15 a scaling of 0.7 does not make plain YIN jump.
    Why not a stronger scaling at 0.15: every sample lies in W / H = 4 windows, so a stretch that lifts d'(period) to v in one frame adds
    about 4 v to the path that stays at the period, while a path that leaves pays one octave jump, 0.35, and oct = 0.01 a frame it spends
    an octave down - under 0.6 anywhere in a clip of 50 frames.  At v > 0.15 the path is cheaper an octave down and goes there; at
    v = 0.06 three stretches add about 0.7 and the path stays.  One frame a run: a longer run really is cheaper an octave below.
    What the frames of a stretch read: d'(tau) = tau d(tau) / c(tau) weights d by tau, so where the dip does not reach 0 its minimum stands
    below the period.  With d = d0 + k (tau - T)^2 near T, c(T) / T = 2 P W (the mean of d over a period) and k = P W (2 pi f_rms / 24000)^2,
    f_rms^2 = f0^2 sum h^2 a_h^2 / sum a_h^2 = 5.24 f0^2 for amplitudes 1 / h, the shift is -d'(T) T / (4 pi^2 5.24) samples: 8.4 d'(T)
    cents, 0.5 at d'(T) = 0.06, beside 0.05 .. 0.1 from the noise at 40 dB.  The clips read 0.68 / 0.64 cents at worst: inside 0.74."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / R.SR
    ph = rng.uniform(0, 2 * np.pi, 8)
    x = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + ph[h]) / (h + 1) for h in range(8))
    period = np.floor(t * f0).astype(np.int64)
    centre = np.clip(((period + 0.5) * (R.SR / f0)).astype(np.int64), 0, n - 1)
    g = np.ones(n)
    for first, _ in RUNS_BELOW:
        c = first * R.H - R.LEAD + R.W // 2
        w = _window(c - BELOW_PLATEAU // 2, c + BELOW_PLATEAU // 2, n, BELOW_RAMP)
        g -= (1.0 - PERIOD_GAIN) * w[centre] * (period % 2 == 1)
    x = x * g
    x = 0.25 * x / np.sqrt(np.mean(x * x))
    return (x + rng.standard_normal(n) * 0.25 * 10.0 ** (-snr_db / 20.0)).astype(np.float32)


def gap_tone(f0=150.0, seed=31, n=FAMILY_N):
    """The tone with 100 ms of digital silence in the middle (samples 4800 .. 7200)."""
    x = R.harmonic(f0, n=n, snr_db=40.0, seed=seed).copy()
    x[4800:7200] = 0.0
    return x


def glide(n=FAMILY_N):
    t = np.arange(n) / R.SR
    ph = 2 * np.pi * (100.0 * t + 100.0 * t * t)  # f(t) = 100 + 200 t
    x = sum(np.sin((h + 1) * ph) / (h + 1) for h in range(8))
    return (0.25 * x / np.sqrt(np.mean(x * x))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family():
    """[(name, true f0 or None, planted bool, clip f32, track_smooth(clip))] (the track's "thr" and "floor_e" are what the clip is measured
    with: the defaults but for the octave-below pair): f0_reference's 24 clips, the four planted ones, the gap, the
    glide, white noise and digital silence - computed once and shared (read-only)."""
    out = []
    for f0, snr, x, tr in R.family():
        out.append((f"harmonic {f0:.1f} Hz {snr:g} dB", f0, False, x, track_smooth(x, plain=tr)))
    rng = np.random.default_rng(5)
    more = [("above 150", 150.0, True, planted_above(150.0, 21)), ("above 220", 220.0, True, planted_above(220.0, 22)),
            ("below 150", 150.0, True, planted_below(150.0, 23)), ("below 220", 220.0, True, planted_below(220.0, 24)),
            ("gap", 150.0, False, gap_tone()), ("glide", None, False, glide()),
            ("noise", None, False, (0.1 * rng.standard_normal(FAMILY_N)).astype(np.float32)), ("silence", None, False, np.zeros(FAMILY_N, np.float32))]
    for name, f0, planted, x in more:
        x.setflags(write=False)
        out.append((name, f0, planted, x, track_smooth(x, thr=BELOW_THR if name.startswith("below") else DEFAULT["thr"])))
    return out


def planted_frames(name):
    """The frames of a planted clip's runs."""
    runs = RUNS if name.startswith("above") else RUNS_BELOW
    return [f for first, k in runs for f in range(first, first + k)]
