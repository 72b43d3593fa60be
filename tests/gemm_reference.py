"""fp64 references of the GEMM forms of csrc/gemm.h (GemmArgs) and one element-wise error bound for them.  Needs no GPU: every function
takes torch tensors on any device and computes in float64 from the operand-rounded inputs the kernel consumed.

Bound (assert_within_bound):  |got - ref| <= e + t_round (|ref| + e) + t_abs,   e = 2^-24 (C1 sqrt(K) S + C2 mag)
  S        sum_k |a_k w_k| of the element (plus |bias|), times the activation's derivative bound: the accumulation error;
  mag      magnitude of what the epilogue rounds after the accumulation (pre-activation value, activation output, skip);
  t_round  rounding of a T-typed output: 2^-8 (bf16), 2^-11 (fp16), 0 for f32 outputs; t_abs: half the subnormal spacing (fp16 2^-25).
fp32 verification operands (operand type "f32") add 2^-24 S to e for the rounding of each product.
C1 = 1, C2 = 4, set from the first MI355X run of tests/test_gpu_gemm_forms.py: the worst ratio |err| / bound over every f32 output was
0.145 with 16-bit operands (256 x 256 16-wave tile, K = 192) and 0.309 in the fp32 verification GEMM, i.e. a margin of 6.9x / 3.2x; the
statistics partials reached 0.041 of their own bound.  T-typed outputs reach 0.995: there the bound is the round-to-nearest limit itself.
"""
import math

import torch

U = 2.0 ** -24
C1 = 1.0
C2 = 4.0
T_ROUND = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}
T_ABS = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25, "f32": 0.0}  # half the subnormal spacing: |x| < 2^-14 rounds absolutely in fp16
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU, ACT_LRELU = 0, 1, 2, 3, 4
_LIP = {ACT_NONE: 1.0, ACT_GELU_TANH: 1.13, ACT_GELU_ERF: 1.13, ACT_SILU: 1.1, ACT_LRELU: 1.0}  # max |act'(x)|


def act64(x, act, slope=0.2):
    if act == ACT_NONE:
        return x
    if act == ACT_GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if act == ACT_GELU_ERF:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_LRELU:
        return torch.where(x > 0, x, x * slope)
    raise ValueError(act)


class Ref:
    """value: the fp64 reference; sabs: the accumulation-error scale S per element; mag: the epilogue magnitude per element; K: k length"""

    def __init__(self, value, sabs, mag, K):
        self.value, self.sabs, self.mag, self.K = value, sabs, mag, K

    def map(self, fn, scale=1.0):
        """the same bound for a re-laid-out output (head scatter, cache layout): fn applied to every field, the value times scale"""
        return Ref(fn(self.value) * scale, fn(self.sabs) * abs(scale), fn(self.mag) * abs(scale), self.K)


def conv_operand(A, M, cin, taps, dilation=1, seq_len=None):
    """the virtual [M][taps * cin] operand of a tap convolution over A [rows][cin]: tap t of row s reads row s + (t - taps // 2) * dilation
    of its own seq_len-row sequence, zero outside it; fp64"""
    seq_len = seq_len or M
    dil = max(dilation, 1)
    A = A.double()[:, :cin]
    X = torch.zeros(M, taps * cin, dtype=torch.float64, device=A.device)
    m = torch.arange(M, device=A.device)
    b, s = m // seq_len, m % seq_len
    for t in range(taps):
        s2 = s + (t - taps // 2) * dil
        ok = (s2 >= 0) & (s2 < seq_len)
        X[ok, t * cin:(t + 1) * cin] = A[(b * seq_len + s2)[ok]]
    return X


def gemm_operand(A, K, A2=None, k_split=None):
    """[A | A2] of the second activation source: k >= k_split reads A2[m][k - k_split] (A2 already offset by its slot); fp64"""
    X = A.double()
    if A2 is not None:
        X = torch.cat([X[:, :k_split], A2.double()[:X.shape[0], :K - k_split]], dim=1)
    return X[:, :K]


def std_reference(X, W, bias=None, act=ACT_NONE, slope=0.2, res=None, act_t=ACT_NONE, slope_t=0.2):
    """standard epilogue: f32 = act(X W^T + bias) + res; T = LeakyReLU(slope_t)(f32) when act_t, else f32.  X: fp64 operand [M][K].
    Returns (f32 Ref, T Ref)."""
    W = W.double()
    K = X.shape[1]
    acc = X @ W.t()
    sabs = X.abs() @ W.abs().t()
    if bias is not None:
        acc = acc + bias.double()
        sabs = sabs + bias.double().abs()
    sabs = sabs * _LIP[act] * (max(1.0, abs(slope)) if act == ACT_LRELU else 1.0)
    y = act64(acc, act, slope)
    mag = y.abs() + acc.abs()
    if res is not None:
        y = y + res.double()
        mag = mag + res.double().abs()
    f32 = Ref(y, sabs, mag, K)
    if act_t != ACT_LRELU:
        return f32, f32
    k = max(1.0, abs(slope_t))
    return f32, Ref(act64(y, ACT_LRELU, slope_t), sabs * k, mag * k, K)


def qkv_heads_reference(x, B, S, heads, q_scale):
    """EPI_QKV_HEADS scatter of the [B*S][3*dmodel] Ref x (bias included): q / k / v [B*heads][S][64] (q times q_scale), vt [B*heads][64][S]"""
    D = heads * 64

    def part(p):
        return lambda t: t[:, p * D:(p + 1) * D].reshape(B, S, heads, 64).permute(0, 2, 1, 3).reshape(B * heads, S, 64)
    v = x.map(part(2))
    return {"q": x.map(part(0), q_scale), "k": x.map(part(1)), "v": v, "vt": v.map(lambda t: t.transpose(1, 2))}


def qkv_decode_reference(x, heads, q_scale):
    """EPI_QKV_DECODE of the [M][3*dmodel] Ref x: qbuf [M][dmodel] (times q_scale) and slot *step of kc [M][heads][8][tmax][8] /
    vc [M][heads][tmax][64], given as [M][heads][8][8] / [M][heads][64]"""
    D = heads * 64
    M = x.value.shape[0]
    return {"qbuf": x.map(lambda t: t[:, :D], q_scale), "kslot": x.map(lambda t: t[:, D:2 * D].reshape(M, heads, 8, 8)),
            "vslot": x.map(lambda t: t[:, 2 * D:].reshape(M, heads, 64))}


def geglu_reference(X, W_interleaved, bias_interleaved=None):
    """EPI_GEGLU on pack.geglu_interleave rows (strips of 16: value, gate, value, ...): out [M][N/2], column j = (value_j + b) * gelu_erf(gate_j + b)"""
    N = W_interleaved.shape[0]
    idx = torch.arange(N).reshape(-1, 2, 16)
    order = torch.cat([idx[:, 0, :].reshape(-1), idx[:, 1, :].reshape(-1)]).to(W_interleaved.device)  # [values | gates]
    b = None if bias_interleaved is None else bias_interleaved[order.to(bias_interleaved.device)]
    pre, _ = std_reference(X, W_interleaved[order], b)
    h = N // 2
    val, gate = pre.value[:, :h], pre.value[:, h:]
    g = act64(gate, ACT_GELU_ERF)
    out = val * g
    sabs = pre.sabs[:, :h] * g.abs() + val.abs() * 1.13 * pre.sabs[:, h:]
    mag = out.abs() + val.abs() * (g.abs() + gate.abs())
    return Ref(out, sabs, mag, X.shape[1])


def bound(ref, out_type, operand_type):
    acc = U * (C1 * math.sqrt(ref.K) * ref.sabs + C2 * ref.mag)
    if operand_type == "f32":
        acc = acc + U * ref.sabs
    # the T rounding is relative to the f32 value the kernel rounds (|ref| + its error), plus half the subnormal spacing
    return acc + T_ROUND[out_type] * (ref.value.abs() + acc) + T_ABS[out_type]


def assert_within_bound(name, got, ref, out_type, operand_type, tile=None, quiet=False):
    """|got - ref.value| <= bound, element for element.  Prints rel-L2, the worst ratio |err| / bound, the violation count and the first
    offending element (for a 2-D GEMM output with tile = (BM, BN) also its row / column tile).  Returns the worst ratio."""
    r, bd = ref.value, bound(ref, out_type, operand_type)
    g = got.detach().to(r.device).double()
    assert g.shape == r.shape, (name, tuple(g.shape), tuple(r.shape))
    err = (g - r).abs()
    ratio = torch.where(torch.isfinite(g), err / bd.clamp_min(1e-300), torch.full_like(err, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    rel = float((g - r).norm() / r.norm().clamp_min(1e-300))
    bad = ratio > 1.0
    nbad = int(bad.sum())
    where = ""
    if nbad:
        first = tuple(int(i) for i in torch.nonzero(bad)[0])
        where = f" first at {first}"
        if tile is not None and len(first) == 2:
            where += f" (row tile {first[0] // tile[0]}, column tile {first[1] // tile[1]})"
        where += f": got {float(g[first]):.6e} want {float(r[first]):.6e} bound {float(bd[first]):.3e}"
    if not quiet:
        print(f"[bound] {name}: rel_l2={rel:.3e} worst |err|/bound={worst:.3f} violations={nbad}{where}")
    assert nbad == 0, f"{name}: {nbad} element(s) outside the bound (worst ratio {worst:.3f}){where}"
    return worst


# ------------------------------------------------------------------------------------------------- GroupNorm statistics partials
def gn_partials_reference(y, rows, seq, vperiod=0, vlen=None):
    """what the statistics epilogue writes for the output y [M][N] (gemm_impl.h run_epilogue): gn_part[row_tile][slot][N/16][2] = (sum, sum
    of squares) over tiles of `rows` rows, fp64; slot 0 = the rows of the sequence the tile's first row is in, slot 1 = the rows after that
    sequence's end (zero when the tile does not straddle); with vperiod, sequence b counts its first vlen[b % vperiod] rows only"""
    M, N = y.shape
    nt = (M + rows - 1) // rows
    yp = torch.zeros(nt * rows, N, dtype=torch.float64, device=y.device)
    yp[:M] = y.double()
    r = torch.arange(nt * rows, device=y.device)
    first = r < ((r // rows) * rows // seq + 1) * seq
    valid = r < M
    if vperiod:
        b_row = r // seq
        vl = torch.as_tensor([vlen[b % vperiod] for b in range(int(b_row.max()) + 1)], device=y.device)
        valid &= (r - b_row * seq) < vl[b_row]
    out = torch.zeros(nt, 2, N // 16, 2, dtype=torch.float64, device=y.device)
    for slot, m in ((0, first & valid), (1, (~first) & valid)):
        v = (yp * m[:, None]).reshape(nt, rows, N // 16, 16)
        out[:, slot, :, 0] = v.sum(dim=(1, 3))
        out[:, slot, :, 1] = (v * v).sum(dim=(1, 3))
    return out


def gn_group_sums(part, B, S, C, rows):
    """the consumer's reduction (norm.hip gn_partial_item / gn_finalize) on the host: [B][32][2] (sum, sum of squares) per (sample, group)
    from gn_part [row_tile][2][C/16][2]; tile t of sample b reads slot 1 when it starts inside sample b - 1"""
    part = part.double().reshape(-1, 2, C // 16, 2)
    spg = C // 32 // 16
    out = torch.zeros(B, 32, 2, dtype=torch.float64, device=part.device)
    for b in range(B):
        for t in range((b * S) // rows, ((b + 1) * S - 1) // rows + 1):
            out[b] += part[t, 1 if t * rows < b * S else 0].reshape(32, spg, 2).sum(1)
    return out


def group_sums_bruteforce(y, B, S, C, vperiod=0, vlen=None):
    """[B][32][2] sum / sum of squares of y [B*S][C] per (sample, group of C/32 channels) over each sample's valid rows"""
    y = y.double().reshape(B, S, 32, C // 32)
    out = torch.zeros(B, 32, 2, dtype=torch.float64, device=y.device)
    for b in range(B):
        n = vlen[b % vperiod] if vperiod else S
        out[b, :, 0] = y[b, :n].sum(dim=(0, 2))
        out[b, :, 1] = (y[b, :n] ** 2).sum(dim=(0, 2))
    return out


def assert_partials(name, got, y, rows, seq, vperiod=0, vlen=None, quiet=False):
    """the kernel's statistics partials against gn_partials_reference of its OWN f32 output y: a partial is a float sum of 16 x rows values,
    so |err| <= 2^-24 * 2 * rows * (sum of |v|, resp. of v^2); slot 1 of a tile that does not straddle a sequence must be exactly zero"""
    want = gn_partials_reference(y, rows, seq, vperiod, vlen)
    absum = gn_partials_reference(y.abs(), rows, seq, vperiod, vlen)[..., 0]
    bd = U * 2 * rows * torch.stack([absum, want[..., 1]], dim=-1) + 1e-30
    nt = want.shape[0]
    g = got.detach().to(want.device).double().reshape(-1, *want.shape[1:])[:nt]
    err = (g - want).abs()
    t = torch.arange(nt, device=want.device)
    straddle = ((t * rows) // seq + 1) * seq < torch.clamp((t + 1) * rows, max=y.shape[0])
    bad = err > bd
    bad[:, 1] |= (~straddle)[:, None, None] & (g[:, 1] != 0)
    worst = float((err / bd).max())
    nbad = int(bad.sum())
    where = ""
    if nbad:
        i = tuple(torch.nonzero(bad)[0].tolist())
        where = (f" first at row tile {i[0]} (rows {i[0] * rows}..), slot {i[1]}, strip {i[2]}, {'sum' if i[3] == 0 else 'sum of squares'}: "
                 f"got {float(g[i]):.6e} want {float(want[i]):.6e}")
    if not quiet:
        print(f"[bound] {name} statistics ({nt} tiles of {rows} rows): worst |err|/bound={worst:.3f} violations={nbad}{where}")
    assert nbad == 0, f"{name}: statistics partials wrong:{where}"
    return worst
