"""fp64 restatement of the device mel front-end (csrc/melfront.hip, include/tortoise_mi355x_mel.h) with an element-wise error bound, in the
style of tests/gemm_reference.py whose U, C1 and C2 it reuses.  Needs no GPU.  Everything is computed in float64 from the f32 values the
kernels consume (the clip, the rounded tables).

Bounds, chained stage by stage (K = n_fft, S_re = sum_k |x_k b_cos,k|, S_im likewise):
  e_re   = U (C1 sqrt(K) S_re + C2 |re|) + U S_re                     the project's f32-operand GEMM form; e_im likewise
  e_spec = 2 |re| e_re + 2 |im| e_im + e_re^2 + e_im^2 + 4 U spec     power spectrum
         = hypot(e_re, e_im) + 4 U spec                               magnitude spectrum
  e_mel  = fb . e_spec + U (sqrt(bins) (fb . spec) + 4 mel) + U (fb . spec)
  e_log  = (e_mel / max(mel - e_mel, floor) + 4 U max(|log mel|, 1)) |scale|  (+ U |value|: the kernel multiplies by the f32 reciprocal of
           mel_norms where the reference divides)
Resampler: |err| <= U (C1 sqrt(L) S + C2 |ref|), L = 2 width + orig taps, S = sum_j |taps_j x_j|.

Worst |err| / bound so far (CPU only: audio.MelFrontEnd in f32 against this reference, tests/test_melfront_cpu.py): 0.36 for the autoregressive
log mel (elements at the floor: the reciprocal of mel_norms against the division), 0.20 for the diffusion log mel, bounds <= 3.7e-3.  The
kernels' own ratios (tests/test_gpu_melfront.py prints them per stage, with element and shape) have not been recorded on an MI355X yet.
"""
import math

import torch
import torch.nn.functional as F

from tests.gemm_reference import C1, C2, U

FLOOR = 1e-5
LENGTHS = (513, 1024, 1025, 1279, 1280, 4096, 132300, 102400)


def probe_signal(n, seed=0, sr=22050.0):
    """0.3 sin(220 Hz) + 0.2 sin(3 kHz) + 0.05 randn, the first quarter scaled by 1e-3 (quiet bins and the floor are exercised); f32 [n]"""
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    x = 0.3 * torch.sin(2 * math.pi * 220.0 * t) + 0.2 * torch.sin(2 * math.pi * 3000.0 * t) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    x[:n // 4] *= 1e-3
    return x.float()


def padded_frames(x, n_fft, hop):
    """fp64 [1 + n // hop][n_fft]: centred frames of x with reflect padding (torch.stft(center=True, pad_mode='reflect'))"""
    xp = F.pad(x.double().reshape(1, 1, -1), (n_fft // 2, n_fft // 2), mode="reflect").reshape(-1)
    return xp.unfold(0, n_fft, hop)


class MelRef:
    """spec / e_spec [T][bins]; mel (the scaled log mel) / e_log [n_mels][T]; floor_fraction: share of linear-mel elements at the floor"""


def mel_reference(clip, basis, fb, scale, n_fft, hop, power, clamp, floor=FLOOR, reciprocal=True):
    """clip f32 [n]; basis [n_fft][2 * bins_pad] and fb [n_mels][bins_pad] as the kernel consumes them (f32); scale f32 [n_mels] or None."""
    bins = n_fft // 2 + 1
    x = clip.detach().cpu().double().reshape(-1)
    if clamp:
        x = x.clamp(-1.0, 1.0)
    fr = padded_frames(x, n_fft, hop)
    b = basis.detach().cpu().double().reshape(n_fft, -1, 2)[:, :bins]
    bc, bs = b[..., 0], b[..., 1]
    re, im = fr @ bc, fr @ bs
    s_re, s_im = fr.abs() @ bc.abs(), fr.abs() @ bs.abs()
    rk = math.sqrt(n_fft)
    e_re = U * (C1 * rk * s_re + C2 * re.abs()) + U * s_re
    e_im = U * (C1 * rk * s_im + C2 * im.abs()) + U * s_im
    if power == 2:
        spec = re * re + im * im
        e_spec = 2 * re.abs() * e_re + 2 * im.abs() * e_im + e_re ** 2 + e_im ** 2 + 4 * U * spec
    else:
        spec = torch.hypot(re, im)
        e_spec = torch.hypot(e_re, e_im) + 4 * U * spec
    f = fb.detach().cpu().double()[:, :bins]
    lin = f @ spec.t()                       # [n_mels][T]
    fs = f.abs() @ spec.t()
    e_mel = f.abs() @ e_spec.t() + U * (math.sqrt(bins) * fs + 4 * lin.abs()) + U * fs
    logm = torch.log(lin.clamp(min=floor))
    e_log = e_mel / (lin - e_mel).clamp(min=floor) + 4 * U * logm.abs().clamp(min=1.0)
    val = logm
    if scale is not None:
        sc = scale.detach().cpu().double().reshape(-1, 1)
        val = logm * sc
        e_log = e_log * sc.abs()
        if reciprocal:
            e_log = e_log + U * val.abs()
    r = MelRef()
    r.spec, r.e_spec, r.mel, r.e_log = spec, e_spec, val, e_log
    r.frames = fr.shape[0]
    r.floor_fraction = float((lin <= floor).double().mean())
    return r


def resample_reference(x, taps, orig, new, width):
    """fp64 polyphase sum out[n * new + p] = sum_j taps[p][j] xpad[n * orig + j] of f32 x [n] and f32 taps [new][2 width + orig] ->
    (reference [ceil(new n / orig)], bound)"""
    x = x.detach().cpu().double().reshape(-1)
    t = taps.detach().cpu().double()
    L = 2 * width + orig
    assert t.shape == (new, L)
    fr = F.pad(x, (width, width + orig)).unfold(0, L, orig)
    target = -(-new * x.shape[0] // orig)
    ref = (fr @ t.t()).reshape(-1)[:target]
    s = (fr.abs() @ t.abs().t()).reshape(-1)[:target]
    return ref, U * (C1 * math.sqrt(L) * s + C2 * ref.abs())


def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound, flat index of it); a zero bound with a zero error counts as 0"""
    err = (got.detach().cpu().double().reshape(-1) - ref.reshape(-1)).abs()
    b = bound.reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
    i = int(ratio.argmax())
    return float(ratio[i]), i
