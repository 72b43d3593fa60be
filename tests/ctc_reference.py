"""fp64 reference of the CTC forced alignment (include/tortoise_mi355x_ctc.h), the bounds its f32 device form is held to, and the
seeded input families the CPU and GPU tests share.

The recurrence, restated:
    states  s = 0 .. 2L; even states are blank, odd state 2l + 1 is token l
    a[0][0] = lp[0][blank], a[0][1] = lp[0][y0], every other state -inf
    a[t][s] = lp[t][lab(s)] + best(a[t-1][s], a[t-1][s-1], a[t-1][s-2]); the skip from s - 2 only for odd s with lab(s) != lab(s-2)
    ties    staying wins over s - 1, s - 1 wins over s - 2 (a move needs a strictly greater value)
    end     state 2L unless a[T-1][2L-1] is strictly greater
"""
import math

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of f32
OK, INFEASIBLE, EMPTY = 0, 1, 2


def log_softmax(logits, dtype=np.float64):
    x = np.asarray(logits, dtype=dtype)
    m = x.max(axis=-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dtype)))).astype(dtype)


def labels(targets, blank):
    lab = np.full(2 * len(targets) + 1, blank, dtype=np.int64)
    lab[1::2] = targets
    return lab


def repeats(targets):
    t = np.asarray(targets, dtype=np.int64)
    return int((t[1:] == t[:-1]).sum())


def status_of(T, targets):
    if T == 0 or len(targets) == 0:
        return EMPTY
    return INFEASIBLE if T < len(targets) + repeats(targets) else OK


def viterbi(logits, targets, blank, dtype=np.float64):
    """-> dict(status, path [T], spans [L][2], conf [L], score, lp [T][V]); for status != 0 only status is set.  dtype float32 runs the same
    recurrence in f32 (what the device does); the default is the fp64 reference."""
    logits = np.asarray(logits)
    targets = [int(t) for t in targets]
    T, L = logits.shape[0], len(targets)
    st = status_of(T, targets)
    if st != OK:
        return dict(status=st)
    lp = log_softmax(logits, dtype)
    lab = labels(targets, blank)
    S = 2 * L + 1
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype=dtype)
    a[0], a[1] = lp[0][blank], lp[0][lab[1]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        s1 = np.concatenate(([ninf], a[:-1]))
        s2 = np.where(skip, np.concatenate(([ninf, ninf], a[:-2])), ninf)
        v, b = a.copy(), np.zeros(S, dtype=np.int8)
        m = s1 > v
        v, b = np.where(m, s1, v), np.where(m, 1, b)
        m = s2 > v
        v, b = np.where(m, s2, v), np.where(m, 2, b)
        a = (lp[t][lab] + v).astype(dtype)
        bp[t] = b
    s = S - 2 if a[S - 2] > a[S - 1] else S - 1
    score = a[s]
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(bp[t][s])
    spans, conf = spans_conf(path, lp, targets)
    return dict(status=OK, path=path, spans=spans, conf=conf, score=float(score), lp=lp)


def spans_conf(path, lp, targets):
    """First / last frame of every token on `path` and the mean of exp(lp[t][token]) over them."""
    L = len(targets)
    spans = np.zeros((L, 2), dtype=np.int64)
    conf = np.zeros(L, dtype=np.float64)
    for l in range(L):
        ts = np.nonzero(path == 2 * l + 1)[0]
        spans[l] = (ts[0], ts[-1])
        conf[l] = np.exp(lp[ts, targets[l]].astype(np.float64)).mean()
    return spans, conf


def is_valid_path(path, targets, blank):
    """A monotone CTC alignment: starts in state 0 or 1, ends in 2L or 2L - 1, moves by 0 / 1, or by 2 onto a token that differs from the
    one two states below."""
    lab = labels(targets, blank)
    S = len(lab)
    p = [int(s) for s in path]
    if not p or p[0] not in (0, 1) or p[-1] not in (S - 1, S - 2) or min(p) < 0 or max(p) >= S:
        return False
    for s0, s1 in zip(p, p[1:]):
        d = s1 - s0
        if d not in (0, 1, 2) or (d == 2 and not (s1 % 2 == 1 and lab[s1] != lab[s0])):
            return False
    return True


def path_score(lp, path, targets, blank):
    """fp64 sum over the frames of lp[t][lab(path[t])]."""
    lab = labels(targets, blank)
    return float(np.asarray(lp, dtype=np.float64)[np.arange(len(path)), lab[np.asarray(path)]].sum())


def brute_force(logits, targets, blank):
    """Every monotone CTC path enumerated -> (best path, its fp64 score).  For tiny T, L only."""
    lp = log_softmax(logits)
    lab = labels(targets, blank)
    T, S = lp.shape[0], len(lab)
    best = (None, -math.inf)

    def walk(prefix, sc):
        nonlocal best
        t = len(prefix)
        if t == T:
            if prefix[-1] in (S - 1, S - 2) and sc > best[1]:
                best = (list(prefix), sc)
            return
        s0 = prefix[-1]
        for d in (0, 1, 2):
            s1 = s0 + d
            if s1 >= S or (d == 2 and not (s1 % 2 == 1 and lab[s1] != lab[s0])):
                continue
            walk(prefix + [s1], sc + lp[t][lab[s1]])

    for s in (0, 1):
        walk([s], lp[0][lab[s]])
    return best


# ----------------------------------------------------------------------------------------- bounds of the f32 device form
def lp_error(lp, logits):
    """Bound on |lp_f32 - lp| of every entry, f32 log-softmax computed as  m = max x;  sum = sum_k exp(x_k - m);  lse = m + log(sum);
    lp = x - lse  with exp / log of at most 1 ulp (<= 2u relative):
      a term   exp(fl(x_k - m)) (1 + 2u): the rounded argument moves it by d_k u exp(-d_k) <= u / e  (d_k = m - x_k)  ->  2u exp(-d_k) + u / e
      the sum  V terms and V - 1 additions, relative to sum >= 1 (the maximum's own term is 1):  (2 + (V - 1) + V / e) u
      log      the sum's relative error, plus 2u |log sum|, log sum <= log V
      lse      one rounding u |lse|;   lp: one rounding u |lp|."""
    lp = np.asarray(lp, dtype=np.float64)
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[-1]
    lse = (x - lp)[..., :1]  # (the same for every entry of a row)
    row = (2 + (V - 1) + V / math.e) + 2 * math.log(V) + np.abs(lse)
    return U32 * (row + np.abs(lp)) * (1 + 64 * U32)  # (second-order terms)


def score_bound(T, lp, logits, frame_labels=None):
    """Bound on |score_f32 - fp64 score of the same path|: the f32 score is the left-to-right f32 sum of the path's f32 log-probs, i.e.
    T - 1 additions, each within u of a partial sum, against the largest |partial score|, plus every frame's own log-softmax error.
    frame_labels [T]: the label the path takes in every frame; None: the bound that holds for EVERY path (per frame the worst label)."""
    lp = np.asarray(lp, dtype=np.float64)
    e = lp_error(lp, logits)
    if frame_labels is None:
        mag, err = np.abs(lp).max(axis=1), e.max(axis=1)
    else:
        idx = (np.arange(T), np.asarray(frame_labels))
        mag, err = np.abs(lp[idx]), e[idx]
    partial = float((mag + err).sum())  # no partial sum is larger in magnitude
    n = max(T - 1, 0)
    gamma = n * U32 / (1 - n * U32)
    return float(err.sum() + gamma * partial)


def conf_bound(lp, logits, targets, spans):
    """Bound on |conf_f32 - conf| per token: exp of an argument off by e_lp moves by that fraction, exp itself 2u, the n - 1 additions,
    the division; every term and the mean are <= 1."""
    e = lp_error(lp, logits)
    out = np.zeros(len(targets))
    for l, (a, b) in enumerate(np.asarray(spans)):
        n = int(b - a + 1)
        out[l] = (e[a:b + 1, targets[l]].max() + (2 + (n - 1) + 1) * U32) * (1 + 64 * U32)
    return out


# ----------------------------------------------------------------------------------------- seeded input families
def random_targets(rng, L, vocab, blank):
    ids = [i for i in range(vocab) if i != blank]
    return [int(ids[i]) for i in rng.integers(0, len(ids), size=L)]


def random_clip(seed, vocab=32, blank=0, tmin=20, tmax=400):
    """N(0, 2^2) logits, a random target of at most T / 3 tokens."""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(tmin, tmax + 1))
    L = int(rng.integers(1, max(2, T // 3)))
    return (2.0 * rng.standard_normal((T, vocab))).astype(np.float32), random_targets(rng, L, vocab, blank)


def planted_clip(seed, vocab=32, blank=0, tmin=20, tmax=400):
    """N(0, 1) logits with + 6 on the labels of a random valid alignment."""
    rng = np.random.default_rng(5000 + seed)
    T = int(rng.integers(tmin, tmax + 1))
    L = int(rng.integers(1, max(2, T // 3)))
    tg = random_targets(rng, L, vocab, blank)
    seq = []  # the label sequence with the blanks that repeats need, stretched to T frames
    for i, y in enumerate(tg):
        if i > 0 and tg[i - 1] == y:
            seq.append(blank)
        seq.append(y)
    extra = rng.multinomial(T - len(seq), np.ones(len(seq)) / len(seq))
    frames = [y for y, n in zip(seq, extra) for _ in range(1 + n)]
    x = rng.standard_normal((T, vocab)).astype(np.float32)
    x[np.arange(T), frames] += 6.0
    return x, tg


def tie_break_path(T, targets):
    """The path the tie-break defines on all-equal logits: every state is entered at the first frame it can be reached and the rest of the
    clip stays in the final blank (written down here independently of the recurrence)."""
    seq = []
    for i, y in enumerate(targets):
        if i > 0 and targets[i - 1] == y:
            seq.append(2 * i)  # the blank a repeat needs
        seq.append(2 * i + 1)
    return seq + [2 * len(targets)] * (T - len(seq))
