"""fp64 restatement of the spectral-subtraction denoiser (csrc/denoise.hip, include/tortoise_mi355x_nr.h: the five steps of its header) with
element-wise error bounds, by the method of tests/formant_reference.py, whose STFT, GEMM and overlap-add bounds it reuses.  Needs no GPU.
Everything is computed in float64 from the f32 values the kernels consume (the clip, the rounded tables, the f32 parameters).

  spectrum        re, im with e_re, e_im: formant_reference.spectrum.
  power           the device computes fl(fl(re'^2) + fl(im'^2)) from ITS re', im' (|re' - re| <= e_re): three roundings, so
                  e_P = 2 |re| e_re + 2 |im| e_im + e_re^2 + e_im^2 + 3 U (P + that) + TINY  (TINY: two products may be subnormal).
  floor, auto     the INTERVAL rule.  Order statistics are monotone: if a_t <= b_t for every t, the k-th smallest of a is at most the k-th
                  smallest of b.  The device's column lies between P - e_P and P + e_P cell by cell, so its k-th order statistic lies between
                  theirs; one product with c adds U.  (A bound from the largest e_P of the column says nothing: the loudest frame sets it.)
  floor, region   a mean of m non-negative f32 in any order is within gamma_m = m U / (1 - m U) of the exact mean of the same numbers, plus
                  U for the division: mean(P - e_P) (1 - gamma_m - 2 U) .. mean(P + e_P) (1 + gamma_m + 2 U).
  smoothed power  W = (2 Rt + 1)(2 Rb + 1) non-negative terms, W - 1 additions and one product with the f32 constant f32(1 / W), which the
                  reference uses as it is: box(P - e_P) (1 - (W + 1) U) .. box(P + e_P) (1 + (W + 1) U).
  gain            G(Pbar, S) = g_min where Pbar <= beta S, else max(g_min, 1 - beta S / Pbar): non-decreasing in Pbar, non-increasing in S
                  and continuous, so it is evaluated at the interval ends: G(Pbar_lo, S_hi) - 4 U .. G(Pbar_hi, S_lo) + 4 U (a product, a
                  division and a subtraction of numbers of at most 1).  The interval holds the fp64 gain and the device's.
  output          from a GIVEN spectrum and GIVEN gains: Z = G (re, im), one product: 2 U |Z|; then formant's synthesis bound.  End to end:
                  e_Z = (G_hi - G_lo) |re| + G_hi e_re + 2 U |Z|.

Cells whose gain interval is wider than 2 * RESOLVED are "unresolved": Pbar sits so close to beta S that f32 cannot say on which side.  The
per-cell gain check leaves them out; tests/test_denoise_cpu.py caps their share at 1 % from this file alone, and G |spectrum| and the output
are checked on every cell all the same.
"""
import math

import torch
import torch.nn.functional as F

from tests import formant_reference as FR
from tests.gemm_reference import U
from tortoise_tts_amd import denoise as nr, engine as E

N, H, B, BP = nr.N_FFT, nr.HOP, nr.BINS, nr.BINS_PAD
TINY = 4.0 * 2.0 ** -149
RESOLVED = 0.05


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float64).float())


def tables():
    """fp64 views of the f32 tables of denoise.tables() (formant_reference.Tables; the cepstral tables it also holds are empty)"""
    t = nr.tables()
    return FR.Tables(dict(t, cepstrum=torch.zeros(BP, E.FMT_Q_PAD), warps=torch.zeros(1, E.FMT_Q_PAD, BP)), N, H)


class Par:
    """what the device runs with: the f32 values of a denoise.Params"""

    def __init__(self, p):
        self.num, self.c, self.beta, self.g_min, self.rt, self.rb = p.quantile_num, f32(p.quantile_scale), f32(p.beta), f32(p.g_min), p.smooth_frames, \
            p.smooth_bins
        self.w = f32(1.0 / ((2 * self.rt + 1) * (2 * self.rb + 1)))
        self.cells = (2 * self.rt + 1) * (2 * self.rb + 1)


def power(re, im, e_re, e_im):
    p = re * re + im * im
    e = 2 * re.abs() * e_re + 2 * im.abs() * e_im + e_re ** 2 + e_im ** 2
    return p, e + 3 * U * (p + e) + TINY


def kth(p, k):
    """k-th smallest over the frames of every bin (k = 0: the minimum); p [T][B]"""
    return torch.sort(p, dim=0).values[k]


def floor_auto(p, e_p, k, c):
    """-> S, S_lo, S_hi fp64 [B]"""
    lo, hi = kth((p - e_p).clamp(min=0.0), k), kth(p + e_p, k)
    return kth(p, k) * c, (lo * c * (1 - U) - TINY).clamp(min=0.0), hi * c * (1 + U) + TINY


def gamma(m):
    return m * U / (1 - m * U)


def floor_region(p, e_p, first, count):
    sl = slice(first, first + count)
    g = gamma(count) + 2 * U
    return p[sl].mean(0), ((p[sl] - e_p[sl]).clamp(min=0.0).mean(0) * (1 - g) - TINY).clamp(min=0.0), (p[sl] + e_p[sl]).mean(0) * (1 + g) + TINY


def smooth(p, par):
    """Pbar [T][B]: the box over clamped neighbours, dt outer, db inner, times f32(1 / W)"""
    T, nb = p.shape
    pad = F.pad(p.reshape(1, 1, T, nb), (par.rb, par.rb, par.rt, par.rt), mode="replicate").reshape(T + 2 * par.rt, nb + 2 * par.rb)
    s = torch.zeros_like(p)
    for dt in range(2 * par.rt + 1):
        for db in range(2 * par.rb + 1):
            s = s + pad[dt:dt + T, db:db + nb]
    return s * par.w


def gain(pbar, s, par):
    bs = par.beta * s
    g = 1.0 - bs / pbar.clamp(min=1e-300)
    return torch.where(pbar <= bs, torch.full_like(pbar, par.g_min), g.clamp(min=par.g_min))


def gain_interval(p_lo, p_hi, s_lo, s_hi, par):
    """G_lo, G_hi [T][B] from the cell-wise power interval and the floor interval [B]"""
    r = (par.cells + 1) * U
    lo = gain(smooth(p_lo, par) * (1 - r), s_hi[None, :], par) - 4 * U
    hi = gain(smooth(p_hi, par) * (1 + r), s_lo[None, :], par) + 4 * U
    return lo.clamp(min=par.g_min), hi.clamp(max=1.0)


def synthesis(re, im, g, tb, n, e_zre=None, e_zim=None):
    """step 5 from a spectrum [T][B] and gains [T][B] -> out, e_out fp64 [n].  Without e_z*: spectrum and gains are GIVEN (exact)."""
    zre, zim = re * g, im * g
    e_zre = 2 * U * zre.abs() if e_zre is None else e_zre
    e_zim = 2 * U * zim.abs() if e_zim is None else e_zim
    y = zre @ tb.inv_re + zim @ tb.inv_im
    s = zre.abs() @ tb.inv_re.abs() + zim.abs() @ tb.inv_im.abs()
    through = e_zre @ tb.inv_re.abs() + e_zim @ tb.inv_im.abs()
    e_y = through + FR.gemm_err(s + through, y, 2 * tb.bins_pad)
    out, e_out, _ = FR.overlap_add(y, e_y, tb, n)
    return out, e_out


class NrRef:
    """re, im, e_re, e_im, P, e_P, k, S, S_lo, S_hi, Pbar, G, G_lo, G_hi, out, e_out (end to end), unresolved (bool [T][B])"""


def denoise_reference(clip, tb, p, region=(0, 0), output=True):
    """clip f32 [n], p a denoise.Params, region (first frame, frames) or (0, 0) for auto: the whole chain in fp64 with its bounds"""
    par = p if isinstance(p, Par) else Par(p)
    r = NrRef()
    n = int(clip.reshape(-1).shape[0])
    r.re, r.im, r.e_re, r.e_im = FR.spectrum(clip, tb)
    r.P, r.e_P = power(r.re, r.im, r.e_re, r.e_im)
    T = r.P.shape[0]
    r.k = nr.rank(par.num, T)
    if region[1]:
        r.S, r.S_lo, r.S_hi = floor_region(r.P, r.e_P, *region)
    else:
        r.S, r.S_lo, r.S_hi = floor_auto(r.P, r.e_P, r.k, par.c)
    r.Pbar = smooth(r.P, par)
    r.G = gain(r.Pbar, r.S[None, :], par)
    r.G_lo, r.G_hi = gain_interval((r.P - r.e_P).clamp(min=0.0), r.P + r.e_P, r.S_lo, r.S_hi, par)
    r.unresolved = (r.G_hi - r.G_lo) > 2 * RESOLVED
    if output:
        w = r.G_hi - r.G_lo
        e_zre = w * r.re.abs() + r.G_hi * r.e_re + 2 * U * (r.G * r.re).abs()
        e_zim = w * r.im.abs() + r.G_hi * r.e_im + 2 * U * (r.G * r.im).abs()
        r.out, r.e_out = synthesis(r.re, r.im, r.G, tb, n, e_zre, e_zim)
    return r


def magnitude_interval(r):
    """G |X| of the device lies in [G_lo max(|X| - e_X, 0), G_hi (|X| + e_X)], e_X = |(e_re, e_im)|: every cell, resolved or not"""
    mag, e = (r.re ** 2 + r.im ** 2).sqrt(), (r.e_re ** 2 + r.e_im ** 2).sqrt()
    return r.G_lo * (mag - e).clamp(min=0.0) * (1 - 4 * U), r.G_hi * (mag + e) * (1 + 4 * U)


# ----------------------------------------------------------------------------------------------- the clip family
SR = 24000.0


def gate(n, sr=SR, active=(0.25, 0.85), ramp=0.02):
    """the vowel's envelope: of every second, `active` is voiced (60 %), with raised-cosine ramps; fp64 [n]"""
    t = (torch.arange(n, dtype=torch.float64) / sr) % 1.0
    up = ((t - active[0]) / ramp).clamp(0.0, 1.0)
    down = ((active[1] - t) / ramp).clamp(0.0, 1.0)
    return 0.25 * (1 - torch.cos(math.pi * up)) * (1 - torch.cos(math.pi * down))


def vowel(n, sr=SR, f0=120.0):
    """a harmonic vowel with vibrato (5 Hz, 3 %) and three formants, gated by gate(); fp64 [n], peak 0.5"""
    t = torch.arange(n, dtype=torch.float64) / sr
    phase = 2.0 * math.pi * torch.cumsum(f0 * (1.0 + 0.03 * torch.sin(2.0 * math.pi * 5.0 * t)), 0) / sr
    x = torch.zeros(n, dtype=torch.float64)
    h = 1
    while h * f0 * 1.03 < 0.45 * sr:
        f = h * f0
        a = sum(g / (1.0 + ((f - fc) / bw) ** 2) for fc, bw, g in ((700.0, 130.0, 1.0), (1200.0, 150.0, 0.6), (2600.0, 200.0, 0.3))) + 0.02 / h
        x += a * torch.sin(h * phase)
        h += 1
    x = x * gate(n, sr)
    return 0.5 * x / x.abs().max()


def gaussian(n, seed, pink=False, sr=SR):
    g = torch.Generator().manual_seed(9100 + seed)
    w = torch.randn(n, generator=g, dtype=torch.float64)
    if pink:
        s = torch.fft.rfft(w)
        f = torch.fft.rfftfreq(n, 1.0 / sr).clamp(min=20.0)
        w = torch.fft.irfft(s / f.sqrt(), n=n)
    return w / w.pow(2).mean().sqrt()


def noisy(n, snr_db, seed, pink=False):
    """-> (clip f32 [n], clean fp64, noise fp64, active bool [n], pause bool [n]); the SNR is that of the active part"""
    clean = vowel(n)
    env = gate(n)
    active, pause = env > 0.99, env == 0.0
    sigma2 = float(clean[active].pow(2).mean()) / 10.0 ** (snr_db / 10.0)
    noise = gaussian(n, seed, pink) * math.sqrt(sigma2)
    clip = (clean + noise).float()
    return clip, clean, clip.double() - clean, active, pause  # (noise as the f32 clip holds it)


def periodic(n=47 * H + 1, seed=5):
    """periodic in hop and even about 0, n = 1 (mod hop): the reflected ends continue the period, every frame holds the same f32 numbers
    and every bin's column is one value T times"""
    assert n % H == 1
    g = torch.Generator().manual_seed(9200 + seed)
    half = torch.randn(H // 2 + 1, generator=g, dtype=torch.float64) * 0.1
    p = torch.cat([half, half[1:-1].flip(0)])  # p[j] = p[hop - j]
    return p.repeat(n // H + 1)[:n].float()


def gated_noisy(n=48000, snr_db=10.0, seed=7, head=12000):
    """a noise-only head of `head` samples, then the noisy vowel with its pauses set to digital zero (a gated recording): zeros in more than
    half of the frames -> (clip f32, head in seconds)"""
    clip, _, _, _, pause = noisy(n, snr_db, seed)
    x = clip.clone()
    x[pause] = 0.0
    lead = (gaussian(head, seed + 1) * float(clip.double()[pause].pow(2).mean().sqrt())).float()
    return torch.cat([lead, x]), head / SR


def family():
    """name -> f32 clip; lengths 0.2 .. 6 s, n mod 256 = 0 and 255 among them"""
    fam = {}
    for name, n, snr, pink in (("white 20 dB", 72000, 20.0, False), ("white 10 dB", 144000, 10.0, False), ("white 0 dB", 48000, 0.0, False),
                               ("pink 20 dB", 48127, 20.0, True), ("pink 10 dB", 36095, 10.0, True), ("pink 0 dB", 24064, 0.0, True)):
        fam[name] = noisy(n, snr, len(fam), pink)[0]
    fam["noise only"] = (gaussian(12000, 20) * 0.05).float()
    fam["clean vowel"] = vowel(24000).float()
    fam["zero pauses"] = gated_noisy()[0]
    fam["all ties"] = periodic()
    fam["short"] = noisy(24000, 10.0, 30)[0][6000:10800].clone()  # 0.2 s of the voiced part: 19 frames, fewer than TT_NR_MIN_FRAMES
    return fam


NOISY = ("white 20 dB", "white 10 dB", "white 0 dB", "pink 20 dB", "pink 10 dB", "pink 0 dB")


def true_floor(noise, tb):
    """the mean periodogram of a noise signal, fp64 [B]"""
    re, im, _, _ = FR.spectrum(noise.float(), tb)
    return (re * re + im * im).mean(0)


def db(x):
    return 10.0 * math.log10(x)
