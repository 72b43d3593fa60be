"""fp64 references of the row norms (csrc/ops.h RowNormArgs) and of GroupNorm32 (GroupNormArgs) with one element-wise error bound per family,
the deterministic inputs of tests/test_gpu_norm_forms.py, and plain fp32 emulations of the kernels' algorithms.  Needs no GPU.

Row norm.  The updated row t = ((x_in or x) + bias) + slab_0 + ... is a fixed-order chain of fp32 adds (updated_row, compared bit for bit).
From t in fp64, mu the row mean, r = 1 / sqrt(var + eps), z = (t - mu) r:
  LayerNorm  y = z g + b,   S = |g| r (|t - mu| + |mu| + mean_j |t_j|) + |b|,   e = U (C1 sqrt(D) + C2) S
  RMSNorm    y = t / max(||t|| D^-1/2, eps) g,   S = |y|,   e = U (C1 sqrt(D) + C2_RMS) S   (the x-transformers form)
  a second LayerNorm composes: e = e2(y1) + (2 + |z2|) r2 |g2| max_row(e1)
GroupNorm32.  m, q = E[x], E[x^2] over the valid rows of a (sample, group) in fp64, var = q - m^2, r = 1 / sqrt(var + eps), z = (x - m) r.  The
kernel forms var from fp32 partial sums of x^2 over n_part = rows_per_chunk C / 32 values, so the bound carries kappa = q / (var + eps):
  S = |z| + (|x| + |m| + sqrt(q)) r,   e_norm = U (C1 sqrt(n_part) (kappa / 2) |z| + (C1 sqrt(n_part) + C2) S)
  y = z gamma + beta:  e = |gamma| e_norm + C2 U (|y| + |beta|);  y (1 + scale) + shift the same way.  Rows >= vlen are exact zeros.
Both: an activation multiplies e by max |act'| and adds C2 U (|act(y)| + |y|); a T-typed output adds t_round (|ref| + e) + t_abs.

C1 = 1, C2 = 4 are set by the fp32 emulations below (two-pass LayerNorm; row-chunk fp32 partials with an fp64 combine), not by the kernels:
tests/test_norm_reference_cpu.py holds the emulations to <= 0.5 of the bound on every input family of the GPU tests (worst found: 0.21
LayerNorm, 0.09 double LayerNorm, 0.30 GroupNorm); the kernels have to stay <= 1.  C2_RMS = 8: with C2 = 4 the RMSNorm emulation reaches 0.52 at
D = 4 (1027 rows), because behind the reduction its chain rounds seven times (squares, square root, D^-1/2 twice, reciprocal, the row, the
gain: worst case 7 U |y|, more than the (sqrt(4) + 4) U |y| of C2 = 4) where LayerNorm's S carries the slack of its |mu| and mean |t| terms.
Worst |err| / bound measured on the MI355X (tests/test_gpu_norm_forms.py, bf16 / fp16 / f32 outputs together):
  row norm f32 out   narrow kernel 0.271, wave kernel 0.280, generic kernel 0.072
  row norm T out     0.995 on every kernel: there the bound is the round-to-nearest limit itself
  written-back x     bit for bit the fp32 chain (torch.equal, no bound)
  GroupNorm f32 out  C = 128 0.134, 256 0.158, 512 0.164, 1024 0.169 (0.169 on fused statistics), 2048 0.171; T out 0.996
  GroupNorm f32 out at kappa ~ 1e4 (its own, wide bound)  C = 128 0.350, 256 0.209, 512 0.140, 1024 0.074, 2048 0.076
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.gemm_reference import ACT_GELU_ERF, ACT_GELU_TANH, ACT_NONE, ACT_SILU, T_ABS, T_ROUND, U, _LIP, act64

C1 = 1.0
C2 = 4.0
C2_RMS = 8.0
NORM_NONE, NORM_LAYER, NORM_RMS = 0, 1, 2
KAPPA_MAX = 128.0  # every bounded GroupNorm case asserts kappa <= this for its own data


def f32(v):
    """the value a float argument has inside the kernel"""
    return float(np.float32(v))


class Ref:
    """value: the fp64 reference; err: the bound e of the f32 result, per element"""

    def __init__(self, value, err):
        self.value, self.err = value, err


def bound(ref, out_type):
    return ref.err + T_ROUND[out_type] * (ref.value.abs() + ref.err) + T_ABS[out_type]


def worst_ratio(got, ref, out_type):
    g = got.detach().to(ref.value.device).double()
    assert g.shape == ref.value.shape, (tuple(g.shape), tuple(ref.value.shape))
    bd = bound(ref, out_type)
    err = (g - ref.value).abs()
    # a zero bound (the padded rows of a GroupNorm) is an equality
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bd.clamp_min(1e-300))
    return torch.where(torch.isfinite(g), ratio, torch.full_like(err, float("inf")))


def assert_within_bound(name, got, ref, out_type, quiet=False):
    """|got - ref.value| <= bound, element for element; prints and returns the worst ratio |err| / bound"""
    ratio = worst_ratio(got, ref, out_type)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    nbad = int(bad.sum())
    where = ""
    if nbad:
        first = tuple(int(i) for i in torch.nonzero(bad)[0])
        where = (f" first at {first}: got {float(got.detach().to(ref.value.device).double()[first]):.6e} want {float(ref.value[first]):.6e} "
                 f"bound {float(bound(ref, out_type)[first]):.3e}")
    if not quiet:
        print(f"[bound] {name}: worst |err|/bound={worst:.3f} violations={nbad}{where}")
    assert nbad == 0, f"{name}: {nbad} element(s) outside the bound (worst ratio {worst:.3f}){where}"
    return worst


def _activate(y, e, act):
    if act == ACT_NONE:
        return y, e
    ya = act64(y, act)
    return ya, e * _LIP[act] + C2 * U * (ya.abs() + y.abs())


# ------------------------------------------------------------------------------------------------- row norm
def updated_row(x, x_in=None, bias=None, slabs=()):
    """the kernel's fp32 chain ((x_in or x) + bias) + slab_0 + ... in that order; torch fp32"""
    t = (x if x_in is None else x_in).float().clone()
    if bias is not None:
        t = t + bias.float()
    for s in slabs:
        t = t + s.float()
    return t


def _layernorm64(t, g, b, eps):
    D = t.shape[-1]
    mu = t.mean(-1, keepdim=True)
    d = t - mu
    r = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + f32(eps))
    z = d * r
    S = g.abs() * r * (d.abs() + mu.abs() + t.abs().mean(-1, keepdim=True)) + b.abs()
    return z * g + b, U * (C1 * math.sqrt(D) + C2) * S, z, r


def rownorm_reference(t, mode, g1, b1=None, eps1=1e-5, g2=None, b2=None, eps2=0.0, act=ACT_NONE):
    """the normalised rows of the updated rows t [M][D] (fp32 values): Ref"""
    t = t.double()
    D = t.shape[-1]
    g1 = g1.double()
    if mode == NORM_RMS:
        nrm = t.norm(dim=-1, keepdim=True) * D ** -0.5
        y = t / nrm.clamp_min(f32(eps1)) * g1
        return Ref(y, U * (C1 * math.sqrt(D) + C2_RMS) * y.abs())
    assert mode == NORM_LAYER
    y, e, _, _ = _layernorm64(t, g1, b1.double(), eps1)
    if g2 is not None:
        y2, e2, z2, r2 = _layernorm64(y, g2.double(), b2.double(), eps2)
        y, e = y2, e2 + (2.0 + z2.abs()) * r2 * g2.double().abs() * e.amax(-1, keepdim=True)
    return Ref(*_activate(y, e, act))


def _act32(y, act):
    if act == ACT_NONE:
        return y
    if act == ACT_GELU_ERF:
        return F.gelu(y)
    if act == ACT_GELU_TANH:
        return F.gelu(y, approximate="tanh")
    if act == ACT_SILU:
        return F.silu(y)
    raise ValueError(act)


def rownorm_emulate(t, mode, g1, b1=None, eps1=1e-5, g2=None, b2=None, eps2=0.0, act=ACT_NONE, unbiased=False, neighbour=False):
    """plain fp32 emulation of the kernels' algorithm (two-pass variance; every operation in fp32) on the updated rows t.
    unbiased / neighbour: the mutations `variance divided by D - 1` and `a row normalised with its neighbour's statistics`"""
    t = t.float()
    D = t.shape[-1]
    one = torch.tensor(1.0)
    if mode == NORM_RMS:
        nrm = torch.sqrt((t * t).sum(-1, keepdim=True)) * torch.rsqrt(torch.tensor(float(D)))
        return t * (one / torch.clamp_min(nrm, f32(eps1))) * g1.float()
    layers = [(g1, b1, eps1)] + ([(g2, b2, eps2)] if g2 is not None else [])
    for li, (g, b, eps) in enumerate(layers):
        mean = t.sum(-1, keepdim=True) / float(D)
        d = t - mean
        var = (d * d).sum(-1, keepdim=True) / float(D - 1 if unbiased else D)
        rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
        if neighbour and li == 0:
            d, rstd = t - mean.roll(1, 0), rstd.roll(1, 0)
        t = d * rstd * g.float() + b.float()
    return _act32(t, act)


def rownorm_inputs(seed, M, D, nslab=0):
    """deterministic CPU inputs of a row-norm case: rows of spread 0.5 .. 3.5 around offsets in -2 .. 2; split-K slabs and a bias of unit
    scale; two sets of affine parameters"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * (0.5 + 3.0 * torch.rand(M, 1, generator=g)) + (4.0 * torch.rand(M, 1, generator=g) - 2.0)
    return {"x": x, "x_in": torch.randn(M, D, generator=g) * 2.0 + 0.5, "bias": torch.randn(D, generator=g),
            "slabs": torch.randn(max(nslab, 1), M, D, generator=g)[:nslab],
            "g1": torch.randn(D, generator=g), "b1": torch.randn(D, generator=g),
            "g2": 1.0 + 0.3 * torch.randn(D, generator=g), "b2": 0.3 * torch.randn(D, generator=g)}


def rownorm_edge_rows(D, eps):
    """the edge rows: constant (var = 0); 1e-4 spread around 50; 1e-3 spread around 1; RMS rows with ||t|| D^-1/2 below eps (the clamp branch)
    and just above it; an ordinary row"""
    g = torch.Generator().manual_seed(D)
    n = torch.randn(6, D, generator=g)
    unit = n[3:5] / (n[3:5].norm(dim=-1, keepdim=True) * D ** -0.5)  # ||row|| D^-1/2 = 1
    return torch.stack([torch.full((D,), 3.25), 50.0 + 1e-4 * n[1], 1.0 + 1e-3 * n[2], unit[0] * (0.5 * eps), unit[1] * (1.001 * eps), n[5] * 2.0 + 1.0])


# ------------------------------------------------------------------------------------------------- GroupNorm32
def gn_rows_per_chunk(S):
    return max(16, -(-S // 64))


def ss_per_sample(scale_shift, B, C, div, stride):
    """[B][2C]: the scale / shift block sample b reads from the flat buffer (block b / div, stride floats apart; div 0 = 1, stride 0 = shared)"""
    flat = scale_shift.reshape(-1)
    return torch.stack([flat[(b // max(div, 1)) * stride:(b // max(div, 1)) * stride + 2 * C] for b in range(B)])


def _gn_valid(B, S, vlen):
    vl = torch.tensor([S] * B if not vlen else [vlen[b % len(vlen)] for b in range(B)])
    return vl, (torch.arange(S)[None, :] < vl[:, None])


def groupnorm_reference(x, gamma, beta, eps=1e-5, vlen=None, ss=None, act=ACT_NONE):
    """x [B][S][C]; vlen: the valid rows per sample (b % len(vlen)) or None; ss: [B][2C] per-sample scale | shift (ss_per_sample) or None.
    Returns (Ref [B][S][C], kappa [B][32]); rows >= vlen have value 0 and bound 0."""
    B, S, C = x.shape
    cpg = C // 32
    vl, valid = _gn_valid(B, S, vlen)
    xg = x.double().reshape(B, S, 32, cpg)
    w = valid[:, :, None, None].double()
    n = (vl * cpg).double()[:, None]
    m = (xg * w).sum(dim=(1, 3)) / n
    q = (xg * xg * w).sum(dim=(1, 3)) / n
    var = q - m * m
    r = 1.0 / torch.sqrt(var + f32(eps))
    kappa = q / (var + f32(eps))
    mb, qb, rb, kb = (t[:, None, :, None] for t in (m, q, r, kappa))
    z = (xg - mb) * rb
    sn = C1 * math.sqrt(gn_rows_per_chunk(S) * cpg)
    Sab = z.abs() + (xg.abs() + mb.abs() + qb.sqrt()) * rb
    e = (U * (sn * (kb / 2.0) * z.abs() + (sn + C2) * Sab)).reshape(B, S, C)
    gamma, beta = gamma.double(), beta.double()
    y = z.reshape(B, S, C) * gamma + beta
    e = gamma.abs() * e + C2 * U * (y.abs() + beta.abs())
    if ss is not None:
        sc, sh = ss.double()[:, None, :C], ss.double()[:, None, C:]
        y2 = y * (1.0 + sc) + sh
        y, e = y2, (1.0 + sc).abs() * e + C2 * U * (y2.abs() + sh.abs())
    y, e = _activate(y, e, act)
    keep = valid[:, :, None].double()
    return Ref(y * keep, e * keep), kappa


def groupnorm_emulate(x, gamma, beta, eps=1e-5, vlen=None, ss=None, act=ACT_NONE, group_shift=0, count_pad=False):
    """plain fp32 emulation of the kernels' algorithm: per-(chunk of rows, group) fp32 sums of x and x^2 (each column accumulated over the
    chunk's rows in order, then the group's columns added), fp64 combine of the chunks, fp32 rsqrt and apply.
    group_shift / count_pad: the mutations `group boundaries shifted by four channels` and `padded rows counted in the statistics`"""
    B, S, C = x.shape
    cpg = C // 32
    rpc = gn_rows_per_chunk(S)
    nch = -(-S // rpc)
    vl, valid = _gn_valid(B, S, vlen)
    if count_pad:
        stat_valid, nstat = torch.ones_like(valid), torch.full_like(vl, S)
    else:
        stat_valid, nstat = valid, vl
    xs = x.float().roll(-group_shift, -1)
    xp = torch.zeros(B, nch * rpc, C)
    xp[:, :S] = xs * stat_valid[:, :, None]
    xp = xp.reshape(B, nch, rpc, C)
    s = torch.zeros(B, nch, C)
    q = torch.zeros(B, nch, C)
    for i in range(rpc):
        s = s + xp[:, :, i]
        q = q + xp[:, :, i] * xp[:, :, i]
    s = s.reshape(B, nch, 32, cpg).sum(-1).double().sum(1)
    q = q.reshape(B, nch, 32, cpg).sum(-1).double().sum(1)
    inv_n = 1.0 / (nstat.double() * cpg)[:, None]
    m = s * inv_n
    var = (q * inv_n - m * m).clamp_min(0.0)
    mean = m.float()
    rstd = torch.rsqrt(var.float() + torch.tensor(eps, dtype=torch.float32))
    y = (xs.reshape(B, S, 32, cpg) - mean[:, None, :, None]) * rstd[:, None, :, None]
    y = y.reshape(B, S, C).roll(group_shift, -1) * gamma.float() + beta.float()
    if ss is not None:
        y = y * (1.0 + ss.float()[:, None, :C]) + ss.float()[:, None, C:]
    return _act32(y, act) * valid[:, :, None]


def groupnorm_inputs(seed, B, S, C, offset=2.0):
    """deterministic CPU inputs of a GroupNorm case: per-channel spread 0.5 .. 3.5 around per-group offsets in -offset .. offset (kappa =
    q / (var + eps) stays <= 128 with offset 2: asserted by every bounded case); scale / shift blocks for up to B samples"""
    g = torch.Generator().manual_seed(seed)
    cpg = C // 32
    off = ((2.0 * torch.rand(32, generator=g) - 1.0) * offset).repeat_interleave(cpg)
    x = torch.randn(B, S, C, generator=g) * (0.5 + 3.0 * torch.rand(C, generator=g)) + off
    return {"x": x, "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g), "ss": 0.3 * torch.randn(B, 2 * C, generator=g)}


def round_toward_zero(y, tdt):
    """y (fp32) in the 16-bit type tdt, rounded toward zero instead of to nearest (the mutation of a T-typed output)"""
    r = y.to(tdt)
    up = r.float().abs() > y.abs()
    bits = r.view(torch.int16)
    return torch.where(up, bits - 1, bits).view(tdt)


# the GroupNorm shapes of tests/test_gpu_norm_forms.py (the CPU test holds the emulation to half the bound on the same inputs): 4100 rows give
# 64 chunks of 65, 1030 give 61 chunks of 17; the two long shapes run at C = 128 and C = 1024 only
GN_CHANNELS = [128, 256, 512, 1024, 2048]
GN_SHAPES = [(1, 1), (2, 5), (2, 16), (3, 17), (2, 77), (3, 333), (1, 1030), (1, 4100)]


def gn_cases():
    return [(C, B, S) for C in GN_CHANNELS for B, S in GN_SHAPES if S < 1000 or C in (128, 1024)]


def gn_seed(C, B, S):
    return C * 7 + B * 1000 + S
