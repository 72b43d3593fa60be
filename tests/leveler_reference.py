"""Reference of the streaming leveler (include/tortoise_mi355x_lvs.h), the error bounds of every number the device returns, the streams the
CPU and GPU tests share, and an emulation of the device's scheme in the device's formats.

It restates the header on top of tests/loudness_reference.py (R), which is imported and not edited: the K-weighting in extended precision
and the hop bounds are R.measure's, the gates of a prefix are R.gating's, the peaks are R.peaks'.  Nothing here is tuned; the bounds follow
from the unit roundoffs R.U64 and R.U32.

  q_h    R.measure's hop energies and bounds: the filter is causal, so the complete hops of the whole clip are those of every prefix.
  L_h    R.gating(q[: h + 1], bounds, (h + 1) H): value, bound, status, block counts and the margin to the gates.
  G_h    G_-1 = 20 log10(gain0): the library's log10 and the product, 16 U64 (|G| + 1) as R bounds L's logarithm.
         D = clip(T - L, -cut, boost) moves by at most L's bound plus the subtraction's rounding (a clip never amplifies an error).
         G' = G + clip(D - G, -a, b) = clip(D, G - a, G + b): |dG'| <= max(|dD|, |dG|) - the step never amplifies an error in D or G - plus
         its own roundings U64 (|D - G| + 0.1 max(rise, fall) + |G'|), taken twice because this reference runs the step in f64 as well.
  gl_h   as R.gain: (ln 10 / 20) of G's bound, the power's few ulps 8 U64 (1 + |G|), one rounding to f32.  gl_-1 = gl_-2 = gain0 exactly.
  g[n]   g = a + t (b - a) with a = gl_(h'-2), b = gl_(h'-1), t = k / 2400: (1 - t) da + t db for the ends' bounds, and three f32
         roundings (t, b - a, the fused multiply-add; the emulation's unfused product is a fourth): U32 (3 t |b - a| + |g|).  Where the
         ends are equal and exact, g[n] is that value exactly: bound 0.
  y[n]   R.limiter's derivation with a gain per sample: the ratio c / (g max(P', P)) is off by Pb / P + gb / g + 3 U32 relative; from there
         on R.limiter's text holds word for word.  y = (g x) s: |x| gb (s + sb) + |g x| (sb + 3 U32 s).
"""
import dataclasses
import functools
import math

import numpy as np
from scipy.ndimage import maximum_filter1d, minimum_filter1d

from tests import loudness_reference as R

H, S, LH = R.H, R.S, R.LH
ADAPT, FIXED = 0, 1          # TT_LVS_ADAPT, TT_LVS_FIXED
NONE, LOOKAHEAD = 0, 1       # TT_LVS_NONE, TT_LVS_LOOKAHEAD
DELAY, HIST, TILE = 248, 512, 1024   # TT_LVS_DELAY, TT_LVS_HIST, TT_LVS_TILE
U64, U32 = R.U64, R.U32
f32 = lambda v: float(np.float32(v))


@dataclasses.dataclass(frozen=True)
class Options:
    """One stream's settings as tt_lvs_open takes them (every float is rounded to f32 there)."""
    steer: int
    limit: int
    gain0: float = 1.0
    target: float = -23.0
    ceiling: float = 1.0
    boost: float = 12.0
    cut: float = 24.0
    rise: float = 3.0
    fall: float = 12.0

    def f32(self):
        return dataclasses.replace(self, **{k: f32(getattr(self, k)) for k in ("gain0", "target", "ceiling", "boost", "cut", "rise", "fall")})

    def args(self):
        return (self.steer, self.limit, self.gain0, self.target, self.ceiling, self.boost, self.cut, self.rise, self.fall)


def ready(n_before, n_chunk, limit, flush):
    total = lambda n, fl: n if fl or limit == NONE else max(n - DELAY, 0)
    return total(n_before + n_chunk, flush) - total(n_before, False)


# ----------------------------------------------------------------------------------------- measurement and steering
def hops_trace(x, m=None):
    """x f32 [n] -> per complete hop h: q, qb, L, Lb, status, blocks_abs, blocks_rel, margin (R.gating's, inf for h < 3)."""
    n = len(x)
    nh = n // H
    m = m if m is not None else (R.measure(x) if n else dict(hop_energy=np.zeros(0), hop_bound=np.zeros(0)))
    q, qb = m["hop_energy"][:nh], m["hop_bound"][:nh]
    out = dict(q=q, qb=qb, L=np.full(nh, -np.inf), Lb=np.zeros(nh), status=np.full(nh, R.SHORT, np.int32), blocks_abs=np.zeros(nh, np.int32),
               blocks_rel=np.zeros(nh, np.int32), margin=np.full(nh, np.inf))
    for h in range(3, nh):
        g = R.gating(q[:h + 1], qb[:h + 1], (h + 1) * H)
        out["L"][h], out["Lb"][h], out["status"][h], out["margin"][h] = g["lufs"], g["lufs_bound"], g["status"], g["margin"]
        out["blocks_abs"][h], out["blocks_rel"][h] = int(g["above_abs"].sum()), int(g["above_rel"].sum())
    return out


def steer(tr, o):
    """The dB trajectory and the linear gains with their bounds -> G, Gb [hops] (G_-1, its bound as G0, G0b), gl, glb [hops + 2] (from gl_-2)."""
    o = o.f32()
    nh = len(tr["L"])
    G0 = 20.0 * math.log10(o.gain0)
    G0b = 16 * U64 * (abs(G0) + 1)
    G, Gb = np.zeros(nh), np.zeros(nh)
    gl, glb = np.full(nh + 2, o.gain0), np.zeros(nh + 2)
    g, gb = G0, G0b
    for h in range(nh):
        if o.steer == ADAPT:
            if tr["status"][h] == R.OK:
                d = min(max(o.target - tr["L"][h], -o.cut), o.boost)
                db = tr["Lb"][h] + U64 * abs(o.target - tr["L"][h])
            else:
                d, db = g, gb
            step = min(max(d - g, -(0.1 * o.fall)), 0.1 * o.rise)
            g2 = g + step
            gb = max(db, gb) + 2 * U64 * (abs(d - g) + 0.1 * max(o.rise, o.fall) + abs(g2))
            g = g2
            gl[h + 2] = 10.0 ** (g / 20.0)
            rel = math.log(10.0) / 20.0 * gb + 8 * U64 * (1 + abs(g)) + U32
            glb[h + 2] = rel * gl[h + 2] * (1 + 2 * U32)
        G[h], Gb[h] = g, gb
    return dict(G=G, Gb=Gb, G0=G0, G0b=G0b, gl=gl, glb=glb)


def sample_gain(n, gl, glb):
    """g[n], its bound, for n samples."""
    idx = np.arange(n)
    h = idx // H
    t = (idx - h * H) / 2400.0
    a, b, ab, bb = gl[h], gl[h + 1], glb[h], glb[h + 1]
    g = a + t * (b - a)
    gb = ((1 - t) * ab + t * bb + U32 * (3 * t * np.abs(b - a) + np.abs(g))) * (1 + 4 * U32)
    return g, np.where((a == b) & (ab == 0) & (bb == 0), 0.0, gb)


def limiter(x, g, gb, ceiling):
    """R.limiter with a gain per sample (bound gb) -> dict(y, bound, r, s, free)."""
    x = np.asarray(x, dtype=np.float64)
    c, n = f32(ceiling), len(x)
    if n == 0:
        return dict(y=np.zeros(0), bound=np.zeros(0), r=np.zeros(0), s=np.zeros(0), free=np.zeros(0, bool))
    P, Pb = R.peaks(x)
    Pm = np.maximum(np.concatenate([[0.0], P[:-1]]), P)
    Pmb = np.maximum(np.concatenate([[0.0], Pb[:-1]]), Pb)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(Pm > 0, c / (g * Pm), np.inf)
        rho = np.where(Pm > 0, Pmb / np.maximum(Pm - Pmb, 1e-300), 0.0) + gb / np.maximum(g - gb, 1e-300) + 3 * U32
    r = np.minimum(1.0, ratio)
    sure = ratio * (1 - rho) >= 1
    rb = np.where(sure, 0.0, np.minimum(ratio, 2.0) * rho)
    rp = np.concatenate([np.ones(2 * LH), r, np.ones(2 * LH)])
    rbp = np.concatenate([np.zeros(2 * LH), rb, np.zeros(2 * LH)])
    mp = minimum_filter1d(rp, 2 * LH + 1, mode="constant", cval=1.0)[LH:-LH]
    mbp = maximum_filter1d(rbp, 2 * LH + 1, mode="constant", cval=0.0)[LH:-LH]
    w = R.hann().astype(np.float64)
    dd = 1.0 - mp
    ddb = mbp + U32 * dd
    a = np.convolve(dd, w, mode="valid")
    ab = np.convolve(ddb, w, mode="valid") + R.gamma(243, U32) * a
    s = np.minimum(r, 1.0 - a)
    sb = np.maximum(rb, ab + U32 * np.abs(1.0 - a))
    y = g * x * s
    yb = np.abs(x) * gb * (s + sb) + np.abs(g * x) * (sb + 3 * U32 * s) + 2.0 ** -149
    free = minimum_filter1d(np.concatenate([np.ones(2 * LH, bool), sure, np.ones(2 * LH, bool)]).astype(np.uint8), 4 * LH + 1)[2 * LH:-2 * LH] == 1
    return dict(y=y, bound=yb, r=r, s=s, free=free)


def level(x, o, m=None):
    """One stream, whole -> the per-hop trace (hops_trace, steer), per sample g, gb, y, bound, limited (s < 1), free, s; and P, Pb."""
    o = o.f32()
    x = np.asarray(x, dtype=np.float32)
    tr = hops_trace(x, m)
    out = dict(tr, **steer(tr, o))
    g, gb = sample_gain(len(x), out["gl"], out["glb"])
    out.update(g=g, gb=gb)
    if o.limit == LOOKAHEAD:
        lim = limiter(x, g, gb, o.ceiling)
        out.update(y=lim["y"], bound=lim["bound"], limited=lim["s"] < 1, free=lim["free"], s=lim["s"])
    else:
        xx = x.astype(np.float64)
        out.update(y=g * xx, bound=np.abs(xx) * gb + U32 * np.abs(g * xx) + 2.0 ** -149, limited=np.zeros(len(x), bool), free=np.ones(len(x), bool),
                   s=np.ones(len(x)))
    return out


# ----------------------------------------------------------------------------------------- the streams
SETTINGS = tuple(Options(ADAPT, lim, 1.0, T, 10.0 ** (cdb / 20.0)) for lim, T, cdb in
                 ((LOOKAHEAD, -16.0, -1.0), (LOOKAHEAD, -23.0, -6.0), (NONE, -30.0, -1.0), (LOOKAHEAD, -30.0, -1.0), (NONE, -16.0, -6.0), (LOOKAHEAD, -23.0, -1.0)))
FIXED_SETTINGS = tuple(Options(FIXED, lim, g0, -23.0, 10.0 ** (cdb / 20.0)) for lim, g0, cdb in
                       ((LOOKAHEAD, 2.5, -6.0), (NONE, 0.4, -1.0), (LOOKAHEAD, 1.0, -1.0), (LOOKAHEAD, 6.0, -1.0)))
# lengths around the segment border, D, the history and the tile (speech, seed 2: not family members, held to the same gate margin)
EXTRA = tuple(("speech", n, 2) for n in (149, 150, 151, DELAY - 1, DELAY, DELAY + 1, HIST + 1, TILE + DELAY - 1, TILE + DELAY, TILE + DELAY + 1))


def stream_settings(i):
    """The ADAPT and the FIXED settings of stream i: every clip runs both; targets, ceilings and limit modes rotate."""
    return SETTINGS[i % len(SETTINGS)], FIXED_SETTINGS[i % len(FIXED_SETTINGS)]


@functools.lru_cache(maxsize=None)
def streams():
    """[(x f32, R.measure(x))] for R.FAMILY then EXTRA, computed once per process and shared (read-only)."""
    out = [(x, m) for x, _, _, m in R.family_reference()]
    for kind, n, seed in EXTRA:
        x = R.clip(kind, n, seed)
        x.setflags(write=False)
        out.append((x, R.measure(x)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stream_reference(i, fixed):
    x, m = streams()[i]
    return level(x, stream_settings(i)[int(fixed)], m)


def chunkings(n, seed=0):
    """name -> [(chunk length, flush)] summing to n: the chunkings the issue lists (one sample per push only for n <= 700)."""
    def cut(size):
        sizes = [size] * (n // size) + ([n % size] if n % size else [])
        return [(c, i == len(sizes) - 1) for i, c in enumerate(sizes)] or [(0, True)]
    out = {"whole": [(n, True)]}
    if n <= 700:
        out["ones"] = cut(1)
    for size in (149, 150, 151, 2399, 2400, 2401, DELAY - 1, DELAY, DELAY + 1):
        if n > size and (size > 400 or n <= 20000):
            out[f"by{size}"] = cut(size)
    rng = np.random.default_rng(1000 + seed + n)
    sizes, left = [], n
    while left > 0:
        c = int(min(left, rng.choice([1, 7, 149, 300, HIST - 1, HIST + 1, 1500, 5000, 30000])))
        sizes.append(c)
        left -= c
    out["random"] = [(c, i == len(sizes) - 1) for i, c in enumerate(sizes)] or [(0, True)]
    # pushes of nothing in between, and the flush on its own, without a last chunk
    out["empty"] = [p for c, _ in out["random"] for p in ((0, False), (c, False))] + [(0, True)]
    out["big"] = ([(min(n, 3 * HIST), False)] if n else []) + [(max(n - 3 * HIST, 0), True)]  # chunks larger than the history
    return out


# ----------------------------------------------------------------------------------------- an emulation of the device's arithmetic
def emulate(x, o):
    """The device's scheme in the device's formats, with numpy's operations instead of fused ones (another rounding here and there, inside
    the same bounds): R.emulate's f64 segment passes and carry for q, the gates of every prefix in f64, the f64 steering, the f32 gain ramp
    and the f32 limiter -> dict(q, L, status, blocks_abs, blocks_rel, G, gl [hops + 2], y f32, peak, out_peak, limited)."""
    o = o.f32()
    x = np.asarray(x, dtype=np.float32)
    n, nh = len(x), len(x) // H
    q = R.emulate(x, o.target, o.ceiling, R.NONE)["hop_energy"][:nh] if n else np.zeros(0)
    L, status = np.full(nh, -np.inf), np.full(nh, R.SHORT, np.int32)
    ba, br = np.zeros(nh, np.int32), np.zeros(nh, np.int32)
    z = np.array([(((q[j] + q[j + 1]) + q[j + 2]) + q[j + 3]) / R.B for j in range(max(nh - 3, 0))])
    for h in range(3, nh):
        zz = z[:h - 2]
        a = zz > 10.0 ** (-6.9309)
        status[h] = R.SILENT
        if a.any():
            r = a & (zz > 0.1 * (zz[a].sum() / a.sum()))
            status[h], L[h], ba[h], br[h] = R.OK, -0.691 + 10 * np.log10(zz[r].sum() / r.sum()), a.sum(), r.sum()
    G, gl = np.zeros(nh), np.full(nh + 2, np.float32(o.gain0), np.float32)
    g = 20.0 * math.log10(o.gain0)
    for h in range(nh):
        if o.steer == ADAPT:
            d = min(max(o.target - L[h], -o.cut), o.boost) if status[h] == R.OK else g
            g = g + min(max(d - g, -(0.1 * o.fall)), 0.1 * o.rise)
            gl[h + 2] = np.float32(10.0 ** (g / 20.0))
        G[h] = g
    idx = np.arange(n)
    hh = idx // H
    t = (idx - hh * H).astype(np.float32) / np.float32(2400)
    gs = t * (gl[hh + 1] - gl[hh]) + gl[hh]
    out = dict(q=q, L=L, status=status, blocks_abs=ba, blocks_rel=br, G=G, gl=gl, g=gs)
    if o.limit == NONE or n == 0:
        out.update(y=gs * x, peak=np.float32(0), limited=0)
    else:
        sp = np.concatenate([np.zeros(7, np.float32), x, np.zeros(8, np.float32)])
        win = np.lib.stride_tricks.sliding_window_view(sp, R.TAPS)
        P = np.abs(x)
        for p in range(1, R.OS):
            acc = np.zeros(n, np.float32)
            for k in range(R.TAPS):
                acc = acc + R.taps()[p, k] * win[:, k]
            P = np.maximum(P, np.abs(acc))
        with np.errstate(divide="ignore"):
            r = np.minimum(np.float32(1), np.float32(o.ceiling) / (gs * np.maximum(np.concatenate([[np.float32(0)], P[:-1]]), P)))
        rp = np.concatenate([np.ones(2 * LH, np.float32), r, np.ones(2 * LH, np.float32)])
        d = np.float32(1) - minimum_filter1d(rp, 2 * LH + 1, mode="constant", cval=1.0)[LH:-LH]
        acc = np.zeros(n, np.float32)
        for k in range(2 * LH + 1):
            acc = acc + R.hann()[k] * d[k:k + n]
        s = np.minimum(r, np.float32(1) - acc)
        out.update(y=(gs * x) * s, peak=P.max(), limited=int((s < 1).sum()))
    out["out_peak"] = np.abs(out["y"]).max(initial=np.float32(0))
    return out


# ----------------------------------------------------------------------------------------- the checks both the GPU test and the emulation pass
def share(err, bound):
    """The largest share of its bound any entry uses (inf for an error where the bound is 0)."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0))


def verify(got, ref, x, o):
    """got: a device (or emulated) stream - q, L, G (f64 [hops]), status, blocks_abs, blocks_rel, gl (f32 [hops + 2], optional), y (f32 [n]) -
    against ref = level(x, o): statuses and block counts equal, every q, L, G, gl and y inside its bound, |y| under the ceiling, and
    FIXED samples exactly gain0 x where nothing can limit.  -> the worst share of each bound used."""
    o = o.f32()
    nh = len(ref["q"])
    assert len(got["q"]) == len(got["L"]) == len(got["G"]) == nh and len(got["y"]) == len(x)
    assert np.array_equal(got["status"], ref["status"]), (len(x), got["status"], ref["status"])
    assert np.array_equal(got["blocks_abs"], ref["blocks_abs"]) and np.array_equal(got["blocks_rel"], ref["blocks_rel"]), len(x)
    ok = ref["status"] == R.OK
    assert np.all(got["L"][~ok] == -np.inf)
    worst = dict(q=share(np.abs(got["q"] - ref["q"]), ref["qb"]), L=share(np.abs(got["L"][ok] - ref["L"][ok]), ref["Lb"][ok]),
                 G=share(np.abs(got["G"] - ref["G"]), ref["Gb"]), gl=0.0,
                 y=share(np.abs(got["y"].astype(np.float64) - ref["y"]), ref["bound"]))
    if got.get("gl") is not None:
        worst["gl"] = share(np.abs(got["gl"].astype(np.float64) - ref["gl"]), ref["glb"])
    if o.limit == LOOKAHEAD:
        assert (np.abs(got["y"]) <= np.float32(o.ceiling) * (1 + 4 * U32)).all()
    if o.steer == FIXED:
        gx = np.float32(o.gain0) * np.asarray(x, dtype=np.float32)
        assert got["y"][ref["free"]].tobytes() == gx[ref["free"]].tobytes()  # exactly gain0 x where nothing limits
    assert max(worst.values()) <= 1.0, (len(x), o, worst)
    return worst


# ----------------------------------------------------------------------------------------- a fake stage for host-flow tests
def whole_fake(x, settings):
    """The fake stage's "leveler": gain0 x[n] plus n / 4096 (a value that names its own index)."""
    x = np.asarray(x, dtype=np.float32)
    return (np.float32(settings.gain0) * x + (np.arange(len(x)) / 4096.0).astype(np.float32)).astype(np.float32)


class FakeStreamLevelStage:
    """stages.StreamLevelStage on the host: the real emission rule (loudness.stream_ready), whole_fake as the leveler."""

    made = []

    def __init__(self, max_streams=16, max_hops=36000, device="cpu"):
        self.max_streams, self.slots, self.calls = int(max_streams), {}, []
        FakeStreamLevelStage.made.append(self)

    def open(self, settings):
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError("all leveling streams are open")
        self.slots[free[0]] = dict(settings=settings, x=np.zeros(0, np.float32), m=0, finished=False)
        return free[0]

    def close(self, slot=None):
        if slot is not None:
            self.slots.pop(slot, None)

    def push_many(self, items):
        import torch
        from tortoise_tts_amd import loudness as loud
        assert 1 <= len(items) <= self.max_streams and len({s for s, _, _ in items}) == len(items)
        self.calls.append([(s, int(x.shape[0]), bool(f)) for s, x, f in items])
        out = []
        for slot, x, flush in items:
            st = self.slots[slot]
            assert not st["finished"]
            c = loud.stream_ready(len(st["x"]), x.shape[0], st["settings"].limit, flush)
            st["x"] = np.concatenate([st["x"], x.detach().cpu().numpy().astype(np.float32).reshape(-1)])
            assert st["m"] + c <= len(st["x"])
            out.append(torch.from_numpy(whole_fake(st["x"], st["settings"])[st["m"]:st["m"] + c].copy()))
            st["m"] += c
            st["finished"] = bool(flush)
        return out

    def read(self, slot):
        st = self.slots[slot]
        return dict(lufs=-math.inf, status=R.SHORT, blocks_abs=0, blocks_rel=0, gain_db=0.0, gain=st["settings"].gain0, peak=0.0, out_peak=0.0,
                    limited=0, n_in=len(st["x"]), n_out=st["m"], hops=len(st["x"]) // H)
