"""fp64 restatement of the formant correction (csrc/formant.hip, include/tortoise_mi355x_fmt.h: the seven steps of its header) with
element-wise error bounds, in the style of tests/melfront_reference.py whose STFT bound it reuses, with U, C1, C2 of tests/gemm_reference.py.
Needs no GPU.  Everything is computed in float64 from the f32 values the kernels consume (the clip, the rounded tables).

Every f32 GEMM gets the project's form  gemm_err(S, ref, K) = U (C1 sqrt(K) S + C2 |ref|) + U S,  S the sum of the absolute products.

  log magnitude   p = re^2 + im^2,  e_p = 2 |re| e_re + 2 |im| e_im + e_re^2 + e_im^2 + 4 U (p + delta)   (melfront's e_re, e_im)
                  e_L = 0.5 e_p / max(p - e_p, delta) + 4 U max(|L|, 1)
  log gain        from GIVEN log magnitudes: c = L A with e_c = gemm_err(|L| |A|, c, bins_pad); g = c D with
                  e_g = e_c |D| + gemm_err((|c| + e_c) |D|, g, 64).  The clamp is 1-Lipschitz and adds nothing.
  output          from a GIVEN spectrum and GIVEN gains: Z = (re, im) exp(g) with 4 U |Z| (expf within one ulp = 2 U, one product, one U of
                  slack); y = Z inverse with e_y = e_Z |inverse| + gemm_err(|Z| |inverse|, y, 2 bins_pad); at most four frames are added in
                  f32 (3 U of the absolute sum), the denominator is a sum of at most four positive f32 squares (5 U relative) and the
                  division rounds once: e_out = (sum e_y + 3 U sum |y|) / den + 8 U |out|.
  end to end      e_L goes through |A D|, the composite matrix [bins][bins] (its absolute column sums are about 2 where those of |A| |D|
                  are above 20), plus the log gain's rounding terms; e_Z = (|re| + e_re) exp(g) expm1(e_g) + e_re exp(g) + 4 U (...), then
                  as above.  A clip whose bins reach delta (exact silence, a clean synthetic vowel) has no useful end-to-end bound: e_L is
                  then of order 1.  Such clips are checked through the staged protocol only.
"""
import math

import torch

from tests.gemm_reference import C1, C2, U
from tests.melfront_reference import padded_frames

DELTA = 1e-10


def gemm_err(s, ref, k):
    return U * (C1 * math.sqrt(k) * s + C2 * ref.abs()) + U * s


def gain_limit(max_gain_db):
    """ln(10) G / 20 as the library rounds it to f32 (0: no clamp)"""
    return float(torch.tensor(math.log(10.0) * float(max_gain_db) / 20.0, dtype=torch.float64).float())


class Tables:
    """fp64 views of the f32 tables of formant.tables(), cut to the B bins that are not padding: bc / bs [N][B] (the basis' cos and -sin
    columns), A [B][64], inv_re / inv_im [B][N] (rows 2 b and 2 b + 1 of the inverse basis), window [N] (column 0 of the basis) and
    D(i) [64][B]"""

    def __init__(self, tabs, n_fft, hop):
        self.n_fft, self.hop, self.bins = n_fft, hop, n_fft // 2 + 1
        B = self.bins
        b = tabs["basis"].detach().cpu().double().reshape(n_fft, -1, 2)
        self.bins_pad = b.shape[1]
        self.bc, self.bs = b[:, :B, 0], b[:, :B, 1]
        self.window = b[:, 0, 0].clone()
        self.A = tabs["cepstrum"].detach().cpu().double()[:B]
        inv = tabs["inverse"].detach().cpu().double().reshape(self.bins_pad, 2, n_fft)
        self.inv_re, self.inv_im = inv[:B, 0], inv[:B, 1]
        self.warps = tabs["warps"].detach().cpu().double()[:, :, :B]

    def D(self, i):
        return self.warps[i]


def spectrum(clip, tb):
    """-> re, im, e_re, e_im fp64 [T][B] (melfront's STFT and its bound)"""
    x = clip.detach().cpu().double().reshape(-1)
    fr = padded_frames(x, tb.n_fft, tb.hop)
    re, im = fr @ tb.bc, fr @ tb.bs
    s_re, s_im = fr.abs() @ tb.bc.abs(), fr.abs() @ tb.bs.abs()
    return re, im, gemm_err(s_re, re, tb.n_fft), gemm_err(s_im, im, tb.n_fft)


def log_magnitude(re, im, e_re=None, e_im=None):
    """-> L (and e_L when the spectrum's bounds are given)"""
    p = re * re + im * im
    L = 0.5 * torch.log(p + DELTA)
    if e_re is None:
        return L
    e_p = 2 * re.abs() * e_re + 2 * im.abs() * e_im + e_re ** 2 + e_im ** 2 + 4 * U * (p + DELTA)
    return L, 0.5 * e_p / (p - e_p).clamp(min=DELTA) + 4 * U * L.abs().clamp(min=1.0)


def log_gain(L, tb, warp, limit):
    """L fp64 [T][B] (given: the reference's or the device's) -> (clamped g, unclamped g, rounding bound e_g)"""
    D = tb.D(warp)
    c = L @ tb.A
    e_c = gemm_err(L.abs() @ tb.A.abs(), c, tb.bins_pad)
    g = c @ D
    e_g = e_c @ D.abs() + gemm_err((c.abs() + e_c) @ D.abs(), g, D.shape[0])
    gc = g.clamp(-limit, limit) if limit > 0 else g
    return gc, g, e_g


def overlap_add(y, e_y, tb, n):
    """y, e_y fp64 [T][N] (windowed frames) -> out, e_out fp64 [n]"""
    T, N, H = y.shape[0], tb.n_fft, tb.hop
    total = (T - 1) * H + N
    num, den, e_num, s_abs = (torch.zeros(total, dtype=torch.float64) for _ in range(4))
    w2 = tb.window ** 2
    for t in range(T):
        sl = slice(t * H, t * H + N)
        num[sl] += y[t]
        den[sl] += w2
        e_num[sl] += e_y[t]
        s_abs[sl] += y[t].abs()
    sl = slice(N // 2, N // 2 + n)
    out = num[sl] / den[sl]
    return out, (e_num[sl] + 3 * U * s_abs[sl]) / den[sl] + 8 * U * out.abs(), den[sl]


def synthesis(re, im, g, tb, n, e_re=None, e_im=None, e_g=None):
    """steps 5 to 7 from a spectrum [T][B] and gains [T][B] -> out, e_out fp64 [n].  Without e_*: spectrum and gains are GIVEN (exact)."""
    E = torch.exp(g)
    zre, zim = re * E, im * E
    e_zre, e_zim = 4 * U * zre.abs(), 4 * U * zim.abs()
    if e_g is not None:
        grow = torch.expm1(e_g)
        e_zre = (re.abs() + e_re) * E * grow + e_re * E + 4 * U * (zre.abs() + e_zre + e_re * E) * (1 + grow)
        e_zim = (im.abs() + e_im) * E * grow + e_im * E + 4 * U * (zim.abs() + e_zim + e_im * E) * (1 + grow)
    y = zre @ tb.inv_re + zim @ tb.inv_im
    s = zre.abs() @ tb.inv_re.abs() + zim.abs() @ tb.inv_im.abs()
    e_y = e_zre @ tb.inv_re.abs() + e_zim @ tb.inv_im.abs() + gemm_err(s + (e_zre @ tb.inv_re.abs() + e_zim @ tb.inv_im.abs()), y, 2 * tb.bins_pad)
    out, e_out, _ = overlap_add(y, e_y, tb, n)
    return out, e_out


class FmtRef:
    """re, im, e_re, e_im, L, e_L, g (clamped), e_g_round, e_g (end to end), out, e_out (end to end), peak"""


def formant_reference(clip, tb, warp, limit):
    """clip f32 [n]; the whole chain in fp64 with the end-to-end bound"""
    r = FmtRef()
    n = int(clip.reshape(-1).shape[0])
    r.re, r.im, r.e_re, r.e_im = spectrum(clip, tb)
    r.L, r.e_L = log_magnitude(r.re, r.im, r.e_re, r.e_im)
    r.g, _, r.e_g_round = log_gain(r.L, tb, warp, limit)
    AD = tb.A @ tb.D(warp)                      # the composite [B][B]: the input error goes through |A D|, not |A| |D|
    r.e_g = r.e_L @ AD.abs() + r.e_g_round
    r.out, r.e_out = synthesis(r.re, r.im, r.g, tb, n, r.e_re, r.e_im, r.e_g)
    r.peak = float(clip.detach().abs().max())
    return r


def identity_output(clip, tb):
    """steps 1, 6 and 7 with g = 0: the reconstruction of the clip"""
    re, im, _, _ = spectrum(clip, tb)
    return synthesis(re, im, torch.zeros_like(re), tb, int(clip.reshape(-1).shape[0]))[0]


def liftered_envelope(L, tb, q):
    """the liftered log envelope [T][B] of log magnitudes [T][B]: c_0 + 2 sum_{j=1}^{q-1} h_j c_j cos(j w_b), h the raised-cosine taper of D"""
    c = (L @ tb.A)[:, :q]
    j = torch.arange(q, dtype=torch.float64)
    h = 0.5 * (1.0 + torch.cos(math.pi * j / q))
    w = torch.arange(tb.bins, dtype=torch.float64) * (2.0 * math.pi / tb.n_fft)
    k = 2.0 * h[:, None] * torch.cos(j[:, None] * w[None, :])
    k[0] = 1.0
    return c @ k


def warped_envelope(L, tb, q, alpha):
    """liftered_envelope read at min(alpha w_b, pi)"""
    c = (L @ tb.A)[:, :q]
    j = torch.arange(q, dtype=torch.float64)
    h = 0.5 * (1.0 + torch.cos(math.pi * j / q))
    w = (torch.arange(tb.bins, dtype=torch.float64) * (2.0 * math.pi / tb.n_fft) * float(alpha)).clamp(max=math.pi)
    k = 2.0 * h[:, None] * torch.cos(j[:, None] * w[None, :])
    k[0] = 1.0
    return c @ k


def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound, flat index of it); a zero bound with a zero error counts as 0"""
    err = (got.detach().cpu().double().reshape(-1) - ref.reshape(-1)).abs()
    b = bound.reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
    i = int(ratio.argmax())
    return float(ratio[i]), i


# ----------------------------------------------------------------------------------------------- does it move the formants
def vowel(n, f0, formants, sr=24000.0, seed=0, bandwidths=(80.0, 120.0), noise=0.5e-4):
    """a source-filter vowel: an impulse train at f0 through two resonators (two-pole, at `formants` Hz), white noise 80 dB down (noise=0:
    a clean one, whose bins between the harmonics reach delta); f32 [n], peak 0.5"""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.zeros(n, dtype=torch.float64)
    period = sr / float(f0)
    pos = 0.0
    while pos < n:
        x[int(pos)] = 1.0
        pos += period
    y = x
    for fc, bw in zip(formants, bandwidths):
        r = math.exp(-math.pi * bw / sr)
        a1, a2 = -2.0 * r * math.cos(2.0 * math.pi * fc / sr), r * r
        out = torch.zeros(n, dtype=torch.float64)
        y1 = y2 = 0.0
        yl = y.tolist()
        for i in range(n):
            v = yl[i] - a1 * y1 - a2 * y2
            out[i] = v
            y2, y1 = y1, v
        y = out
    y = 0.5 * y / y.abs().max()
    y = y + noise * torch.randn(n, generator=g, dtype=torch.float64)
    return y.float()


def mean_envelope_db(clip, tb, q):
    """frame-averaged liftered log envelope of a clip in dB, fp64 [B]"""
    re, im, _, _ = spectrum(clip, tb)
    return liftered_envelope(log_magnitude(re, im), tb, q).mean(0) * (20.0 / math.log(10.0))


def envelope_distance(a, b, p):
    """rms over the bins 5 .. 0.9 * 513 / max(p, 1) of the difference of two mean envelopes (dB), mean removed"""
    hi = int(0.9 * 513 / max(float(p), 1.0))
    d = (a - b)[5:hi]
    d = d - d.mean()
    return float(d.pow(2).mean().sqrt())
