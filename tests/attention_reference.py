"""fp64 reference of the flash-attention family (csrc/ops.h FlashArgs; csrc/attention.hip, csrc/attention_f32.hip) with one element-wise error
bound, the deterministic inputs and the case tables of tests/test_gpu_flash_forms.py, and a plain fp32 emulation of the kernels' algorithm.
Needs no GPU: every function takes torch tensors on any device and computes from the operand-rounded inputs the kernel consumed.

Operation, per (batch, head) pair with nv valid rows (nv = n without FlashArgs::nv):  s_ij = q_i . k_j + relpos[head][clamp(j - i, -64, 64) + 64]
over the keys j < nv (and j <= i when causal), p = softmax_j(s), o_i = sum_j p_ij v_j for the queries i < nv.  q is pre-scaled; v is given
as vt [pair][64][n_pad].  Columns n .. n_pad of vt and the rows nv .. n of q, k and v are not part of the problem.

Bound (bound, worst_ratio):  |got - o| <= e + t_round (|o| + e) + t_abs, with m = max_j s_ij, A = sum_j p_j |v_j| and
  delta_j = U ((C1 sqrt(64) + C2) sum_d |q_d k_d| + C2 (|s_j - m| + |m| + |bias_j|))      the fp32 score, the exponent's argument
  e = 2 (sum_j p_j delta_j |v_j| + (sum_j p_j delta_j) A)                                    ... carried through the softmax
    + CN t_round A                                                                           the numerators rounded to the operand type
    + 2^-25 sum_{visible j} |v_j|        (fp16 only)                                         a numerator below the fp16 normal range
    + C2 U (A + |o|)                                                                         fp32 accumulation, row sum and the division
The row sum is formed from the UNROUNDED fp32 numerators in every kernel (l_run += psum before q16_pv / the pf conversion), so the numerator
rounding does not cancel between numerator and denominator: its whole t_round A stays, and it is attained - a causal row of two keys, or a
row that one or two keys carry, rounds nearly every numerator by the full half ulp (the emulation reaches 0.92 t_round A at n = 300, causal,
bf16).  Holding the emulation to half of e therefore takes CN = 2 on this term; no constant on an fp32 term can stand in for it.
A numerator is exp(s - running maximum) <= 1, and every later rescale and the key-split merges multiply by factors <= 1 while the row sum
stays >= 1, so an absolute error of half the fp16 subnormal spacing (2^-25) per key is what underflow can cost.  The fp32 verification kernel
(operand type "f32") has neither rounding term.  t_round / t_abs: tests/gemm_reference.py (2^-8 bf16, 2^-11 fp16; half the subnormal spacing).

C1 = 1, C2 = 4 and CN = 2 are set by the fp32 emulation below (emulate: 32-key tiles, online softmax with a running maximum, exp as
exp2((s - m) log2 e), numerators rounded to the operand type for the PV product only, fp32 accumulators, one division, the key-split forms
merged as flash_merge_halves does), not by the kernels: tests/test_attention_reference_cpu.py holds the emulation's fp32 result to <= 0.5 of e
on every family x mode x type x shape of the GPU test, which leaves its typed result within the full bound; the kernels have to stay <= 1.
Worst found, fp32 result / e and typed result / bound: bf16 0.462 / 0.595, fp16 0.465 / 0.543, f32 operands 0.102 (C1 = 1, C2 = 4 alone: a
margin of 4.9 to the half, as the GEMM module's 6.9; the 16-bit figures are the numerator term's).
Worst |err| / bound measured on the MI355X (tests/test_gpu_flash_forms.py; every family, mode and length of a form together):
  flash_kernel<T,1,true>     bf16 0.513   fp16 0.510
  flash_lds_kernel<T,1,2>    bf16 0.517   fp16 0.505
  flash_lds_kernel<T,1,1>    bf16 0.517   fp16 0.505
  flash_lds_kernel<T,2,1>    bf16 0.595   fp16 0.543   (the emulation's own worst, on the same case: 689 pairs x 129, peaked, causal)
  flash32_kernel<T,2>        bf16 0.477   fp16 0.506
  flash32_kernel<T,1>        bf16 0.506   fp16 0.506
  flash_f32_kernel           f32  0.108
A typed output cannot show its fp32-accumulate part alone; the fp32 kernel's 0.108 is that part (its emulation: 0.102).  The typed outputs sit
near 0.5, not near 1: with CN = 2 the numerator term alone is 2 t_round A >= 2 t_round |o|, so the output's own round-to-nearest limit is a
third of the bound at most, and what the figures show is the numerator rounding reaching about its worst case on rows that few keys carry.
"""
import math

import numpy as np
import torch

from tests.gemm_reference import T_ABS, T_ROUND, U

C1 = 1.0
C2 = 4.0
CN = 2.0
LOG2E = float(np.float32(1.4426950408889634))
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PAD_VALUE = 1e4  # exact in bf16 and fp16: what the test data holds wherever the operation says a location is not part of the problem


class Ref:
    """value: the fp64 reference [pairs][n][64]; err: the bound e of the fp32 result; valid [pairs][n]: the query rows the operation computes"""

    def __init__(self, value, err, valid):
        self.value, self.err, self.valid = value, err, valid


def _bias_index(n, device, shift=0):
    pos = torch.arange(n, device=device)
    return (pos[None, :] - pos[:, None] + shift).clamp(-64, 64) + 64  # [query][key]


def reference(q, k, vt, heads, tname, relpos=None, causal=False, nvp=None):
    """q, k [pairs][n][64], vt [pairs][64][n_pad] in the operand type, relpos f32 [heads][129] or None, nvp: valid rows per pair or None"""
    P, n, _ = q.shape
    dev = q.device
    q64, k64 = q.double(), k.double()
    v64 = vt.double()[:, :, :n].transpose(1, 2)
    nvt = torch.as_tensor(list(nvp) if nvp is not None else [n] * P, device=dev)
    pos = torch.arange(n, device=dev)
    vis = (pos[None, None, :] < nvt[:, None, None]).expand(P, n, n)
    if causal:
        vis = vis & (pos[None, None, :] <= pos[None, :, None])
    dot = q64 @ k64.transpose(1, 2)
    sabs = q64.abs() @ k64.abs().transpose(1, 2)
    if relpos is not None:
        bias = relpos.double()[:, _bias_index(n, dev)].repeat(P // heads, 1, 1)  # pair = batch row * heads + head
    else:
        bias = torch.zeros_like(dot)
    s = (dot + bias).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.softmax(s, -1)
    zero = torch.zeros_like(dot)
    delta = torch.where(vis, U * ((C1 * 8.0 + C2) * sabs + C2 * ((s - m).abs() + m.abs() + bias.abs())), zero)
    vabs = v64.abs()
    o = p @ v64
    A = p @ vabs
    pd = p * delta
    e = 2.0 * (pd @ vabs + pd.sum(-1, keepdim=True) * A) + C2 * U * (A + o.abs())
    if tname != "f32":
        e = e + CN * T_ROUND[tname] * A
    if tname == "f16":
        e = e + 2.0 ** -25 * (vis.double() @ vabs)
    return Ref(o, e, pos[None, :] < nvt[:, None])


def naive_reference(q, k, vt, heads, relpos=None, causal=False, nvp=None):
    """softmax(q k^T + bias) v one (pair, query) at a time with Python loops over the keys; shares no code with reference().  Rows a pair does
    not compute are NaN."""
    P, n, _ = q.shape
    out = torch.full((P, n, 64), float("nan"), dtype=torch.float64)
    for p in range(P):
        rows = n if nvp is None else nvp[p]
        for i in range(rows):
            last = min(i, rows - 1) if causal else rows - 1
            sc = []
            for j in range(last + 1):
                x = float(torch.dot(q[p, i].double(), k[p, j].double()))
                if relpos is not None:
                    x += float(relpos[p % heads, max(-64, min(64, j - i)) + 64])
                sc.append(x)
            mx = max(sc)
            w = [math.exp(x - mx) for x in sc]
            tot = sum(w)
            acc = torch.zeros(64, dtype=torch.float64)
            for j, wj in enumerate(w):
                acc += (wj / tot) * vt[p, :, j].double()
            out[p, i] = acc
    return out


def bound(ref, tname):
    return ref.err + T_ROUND[tname] * (ref.value.abs() + ref.err) + T_ABS[tname]


def worst_ratio(got, ref, tname, typed=True):
    """|got - ref| / bound per element of got [pairs][n][64] (typed False: against e alone, the fp32 result before the cast); a non-finite
    output is an infinite ratio; the rows a pair does not compute count as zero"""
    g = got.detach().to(ref.value.device).double()
    assert g.shape == ref.value.shape, (tuple(g.shape), tuple(ref.value.shape))
    bd = bound(ref, tname) if typed else ref.err
    err = (g - ref.value).abs()
    ratio = torch.where(torch.isfinite(g), err / bd.clamp_min(1e-300), torch.full_like(err, float("inf")))
    return torch.where(ref.valid[:, :, None], ratio, torch.zeros_like(ratio))


def rel_l2(got, ref):
    g = torch.where(ref.valid[:, :, None], got.detach().to(ref.value.device).double(), ref.value)
    return float((g - ref.value).norm() / ref.value.norm().clamp_min(1e-300))


def assert_within_bound(name, got, ref, tname, quiet=False):
    """|got - ref.value| <= bound on every element of the computed rows; prints and returns the worst ratio |err| / bound"""
    ratio = worst_ratio(got, ref, tname)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    nbad = int(bad.sum())
    where = ""
    if nbad:
        first = tuple(int(i) for i in torch.nonzero(bad)[0])
        where = (f" first at (pair, query, dim) {first}: got {float(got[first]):.6e} want {float(ref.value[first]):.6e} "
                 f"bound {float(bound(ref, tname)[first]):.3e}")
    if not quiet:
        print(f"[bound] {name}: rel_l2={rel_l2(got, ref):.3e} worst |err|/bound={worst:.3f} violations={nbad}{where}")
    assert nbad == 0, f"{name}: {nbad} element(s) outside the bound (worst ratio {worst:.3f}){where}"
    return worst


def to_pairs(out, B, H):
    """the kernel's out [B][n][H * 64] as [B * H][n][64]"""
    n = out.shape[1]
    return out.reshape(B, n, H, 64).permute(0, 2, 1, 3).reshape(B * H, n, 64)


# ------------------------------------------------------------------------------------------------- fp32 emulation
def emulate(q, k, vt, heads, tname, relpos=None, causal=False, nvp=None, ways=1, dup_last=False, rp_shift=0, skip_rescale=None, causal_off_block=None):
    """plain fp32 emulation of the kernels' algorithm; returns the fp32 result [pairs][n][64] before the final cast.  The keys go in tiles of
    32; tile t belongs to partial state t % ways (ways 1: one state; 2: the two 32-key halves of a 64-key tile, flash_ring_halves with KS = 2;
    4: the four waves of flash_kernel), and the states are merged at the end as flash_merge_halves does.  The row sum adds the unrounded
    numerators, the PV product takes them rounded to the operand type.
    Mutations: dup_last = the last key counted twice (an unmasked clamped load); rp_shift = the relative-position index shifted by that much
    before the saturation; skip_rescale = t: tile t moves the running maximum without rescaling the state; causal_off_block = b: the queries
    of 64-query block b see one key past the diagonal."""
    tdt = TDT[tname]
    P, n, _ = q.shape
    qf, kf = q.float(), k.float()
    vf = vt.float()[:, :, :n].transpose(1, 2)
    nvt = torch.as_tensor(list(nvp) if nvp is not None else [n] * P)
    qpos = torch.arange(n)
    lim = qpos.clone()
    if causal_off_block is not None:
        lim[64 * causal_off_block:64 * causal_off_block + 64] += 1
    keys = torch.arange(n)
    if dup_last:
        assert nvp is None
        keys = torch.cat([keys, torch.tensor([n - 1])])
    m = torch.full((ways, P, n), -1e30)
    l = torch.zeros(ways, P, n)
    acc = torch.zeros(ways, P, n, 64)
    log2e = torch.tensor(LOG2E)
    rp = None if relpos is None else relpos.float()
    for t in range((len(keys) + 31) // 32):
        kidx = keys[t * 32:(t + 1) * 32]
        w = t % ways
        s = qf @ kf[:, kidx].transpose(1, 2)
        if rp is not None:
            bi = (kidx[None, :] - qpos[:, None] + rp_shift).clamp(-64, 64) + 64
            s = s + rp[:, bi].repeat(P // heads, 1, 1)
        vis = (kidx[None, None, :] < nvt[:, None, None]).expand(P, n, len(kidx))
        if causal:
            vis = vis & (kidx[None, None, :] <= lim[None, :, None])
        s = s.masked_fill(~vis, float("-inf"))
        m_new = torch.maximum(m[w], s.amax(-1))
        alpha = torch.exp2((m[w] - m_new) * log2e)
        if skip_rescale != t:
            l[w] = l[w] * alpha
            acc[w] = acc[w] * alpha[..., None]
        m[w] = m_new
        p = torch.exp2(s * log2e - (m_new * log2e)[..., None])
        l[w] = l[w] + p.sum(-1)
        pr = p if tname == "f32" else p.to(tdt).float()
        acc[w] = acc[w] + pr @ vf[:, kidx]
    M = m.amax(0)
    f = torch.exp2((m - M) * log2e)
    L = (f * l).sum(0)
    O = (f[..., None] * acc).sum(0)
    return O * (1.0 / L)[..., None]


# ------------------------------------------------------------------------------------------------- inputs
FAMILIES = ("peaked", "flat", "heavy", "ascending", "descending")
FAMILY_NOTES = {
    "peaked": "The scales of tests/test_gpu_ops.py (q x 0.25, k x 2): a score spread of about 4, a few keys carry each row.",
    "flat": "k x 0.05: every key weighs about 1 / n, so a miscounted or dropped key moves every element of every row.",
    "heavy": "flat with the value row of the last valid key 64 times larger: a tail key counted twice or not at all is far outside the bound even in bf16.",
    "ascending": "Scores rise with the key index up to a row maximum of 16 to 32: a rescale at every tile, and the maximum in the last, ragged tile.",
    "descending": "Scores fall with the key index from 16 to 32: every later tile underflows against the first (the fp16 subnormal term's case).",
}


def _pad_pattern(*shape):
    """+-1e4 in a checkerboard"""
    idx = sum(torch.arange(s).reshape([-1 if i == d else 1 for i in range(len(shape))]) for d, s in enumerate(shape))
    return PAD_VALUE * (1.0 - 2.0 * (idx % 2).float())


def pair_rows(n, B, H, nv=None):
    """valid rows of every (batch row, head) pair: nv[b % len(nv)] (FlashArgs::nv / nv_period) or n"""
    return [nv[(p // H) % len(nv)] if nv else n for p in range(B * H)]


def make_inputs(family, tname, n, B, H, nv=None):
    """deterministic CPU operands of one case in the operand type: q, k [B*H][n][64], vt [B*H][64][n_pad], relpos f32 [H][129], nvp.
    The same fp32 data for every type; +-1e4 in columns n .. n_pad of vt and in the rows nvp .. n of q, k and v."""
    assert family in FAMILIES
    P, n_pad = B * H, (n + 31) // 32 * 32
    g = torch.Generator().manual_seed(1000 * n + 10 * P + FAMILIES.index(family))
    nvp = pair_rows(n, B, H, nv)
    q = torch.randn(P, n, 64, generator=g) * 0.25
    k = torch.randn(P, n, 64, generator=g)
    v = torch.randn(P, n, 64, generator=g)
    relpos = torch.randn(H, 129, generator=g)
    if family == "peaked":
        k = k * 2.0
    elif family in ("flat", "heavy"):
        k = k * 0.05
        if family == "heavy":
            for p in range(P):
                v[p, nvp[p] - 1] *= 64.0
    else:
        # q = alpha_i e + noise, k = beta_j e + noise orthogonal to e (|e| = 1): q . k = alpha_i beta_j up to the noise and the operand rounding
        e = torch.full((64,), 0.125)
        alpha = 2.0 + 2.0 * torch.rand(P, n, 1, generator=g)
        ramp = torch.arange(n, dtype=torch.float32) / max(n - 1, 1)
        beta = 8.0 * (ramp if family == "ascending" else 1.0 - ramp)
        k = k - (k @ e)[..., None] * e
        k = beta[None, :, None] * e + 0.25 * k
        q = alpha * e + 0.08 * q
    vt = _pad_pattern(P, 64, n_pad)
    vt[:, :, :n] = v.transpose(1, 2)
    junk = _pad_pattern(P, n, 64)
    for p in range(P):
        q[p, nvp[p]:] = junk[p, nvp[p]:]
        k[p, nvp[p]:] = -junk[p, nvp[p]:]
        vt[p, :, nvp[p]:n] = junk[p, nvp[p]:].t()
    tdt = TDT[tname]
    return {"q": q.to(tdt), "k": k.to(tdt), "vt": vt.to(tdt), "relpos": relpos, "nvp": nvp if nv else None, "n": n, "n_pad": n_pad, "B": B, "H": H}


def run_reference(inp, tname, mode):
    return reference(inp["q"], inp["k"], inp["vt"], inp["H"], tname, inp["relpos"] if mode == "relpos" else None, mode == "causal", inp["nvp"])


def run_emulation(inp, tname, mode, ways=1, **mutation):
    return emulate(inp["q"], inp["k"], inp["vt"], inp["H"], tname, inp["relpos"] if mode == "relpos" else None, mode == "causal", inp["nvp"], ways, **mutation)


# ------------------------------------------------------------------------------------------------- the forms and cases of the GPU test
# Sequence lengths.  Register-prefetch kernel: one query block / a block of one query, one key more than a tile, fewer key tiles than waves,
# the kernel's upper limit.  Staged kernels: three tiles (the ring depth) with one key in the last; an exactly full lower half (160: the upper
# 32-key half of the last tile is empty for the key-split waves) and one key in the upper half; four, five and seven tiles; ragged query
# blocks of 64 and 128 (257 = 128 + 128 + 1).  The (batch rows, heads) of a length are chosen so that gridDim.x * gridDim.y is no multiple
# of 8 in at least one case per kernel (the remainder branch of flash_xcd_remap).
REG_N = (16, 17, 33, 70, 127, 128)
STAGED_N = (129, 160, 161, 193, 257, 300, 385)
F32_N = (17, 70, 129, 300)
PAIRS = {16: (5, 1), 17: (1, 3), 33: (3, 1), 70: (2, 3), 127: (1, 5), 128: (3, 1),
         129: (1, 3), 160: (2, 2), 161: (5, 1), 193: (2, 3), 257: (3, 1), 300: (2, 2), 385: (1, 5)}
BIG = (129, 53, 13)  # 689 pairs x 3 blocks of 64 queries = 2067 >= 2048: flash_lds_kernel<T,2,1>; its grid 2 x 689 = 8 x 172 + 2
BIG_FAMILIES = ("peaked", "heavy")
REG, LDS, F32W, F32V = 0, 1, 2, 3  # FlashRan::kernel
# form: the record {kernel, NQ, KS} it must leave, the partial states of its emulation, its types, lengths and modes.  No engine stage runs
# causal attention with a relative-position table (GPT-2 prefill: causal, no table; the diffusion / conditioning stages: a table, not
# causal), so that combination is not a case.
FORMS = {
    "flash_kernel<T,1,true>": dict(ran=(REG, 1, 0), ways=4, types=("bf16", "f16"), ns=REG_N, modes=("plain", "relpos", "causal")),
    "flash32_kernel<T,2>": dict(ran=(F32W, 2, 2), ways=2, types=("bf16", "f16"), ns=STAGED_N, modes=("plain", "relpos")),
    "flash32_kernel<T,1>": dict(ran=(F32W, 2, 1), ways=1, types=("bf16", "f16"), ns=STAGED_N, modes=("plain", "relpos")),
    "flash_lds_kernel<T,1,2>": dict(ran=(LDS, 1, 2), ways=2, types=("bf16", "f16"), ns=STAGED_N, modes=("plain", "relpos", "causal")),
    "flash_lds_kernel<T,1,1>": dict(ran=(LDS, 1, 1), ways=1, types=("bf16", "f16"), ns=STAGED_N, modes=("plain", "relpos", "causal")),
    "flash_lds_kernel<T,2,1>": dict(ran=(LDS, 2, 1), ways=1, types=("bf16", "f16"), ns=(BIG[0],), modes=("plain", "relpos", "causal")),
    "flash_f32_kernel": dict(ran=(F32V, 0, 0), ways=1, types=("f32",), ns=F32_N, modes=("plain", "relpos", "causal")),
}


def form_shape(form, n):
    """(batch rows, heads) of a form's case at length n"""
    return BIG[1:] if form == "flash_lds_kernel<T,2,1>" else PAIRS[n]


def form_families(form):
    return BIG_FAMILIES if form == "flash_lds_kernel<T,2,1>" else FAMILIES


def form_steer(form, mode):
    """(variant, TTX_FLASH32 switch) that send a case to its form (flash_attention_launch): the causal cases and n <= 128 need no switch; a
    non-causal case reaches the 16-query-wave staged kernels with the switch off (plain) or with variant 2 (relpos), so both routes run"""
    if form == "flash32_kernel<T,1>":
        return 1, 1
    if form == "flash_lds_kernel<T,1,2>":
        return (0, 1) if mode == "causal" else (0, 0) if mode == "plain" else (2, 1)
    if form in ("flash_lds_kernel<T,1,1>", "flash_lds_kernel<T,2,1>"):
        return (1 if form.endswith("1,1>") else 0), (1 if mode == "causal" else 0)
    return 0, 1


def emulation_cases():
    """every (type, family, n, B, H, mode, ways) the GPU test launches, once"""
    seen = []
    for form, f in FORMS.items():
        for tname in f["types"]:
            for n in f["ns"]:
                B, H = form_shape(form, n)
                for fam in form_families(form):
                    for mode in f["modes"]:
                        c = (tname, fam, n, B, H, mode, f["ways"])
                        if c not in seen:
                            seen.append(c)
    return seen
