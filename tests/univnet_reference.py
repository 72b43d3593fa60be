"""fp64 references of the audio-rate UnivNet kernels of csrc/univnet.hip (conv1d_direct_kernel<32 / 1>, conv1d_mfma_kernel, convt1d_kernel,
lvc_kernel<., 8 / 64 / 256>, lvc_mfma_kernel<., 64 / 256>), one element-wise error bound for them, deterministic input families, and plain
fp32 emulations of each kernel's summation order.  Needs no GPU: every function takes torch tensors on any device.

Every reference consumes the values the kernel consumed: the input LeakyReLU is the kernel's own fp32 operation (x > 0 ? x : x * float32(slope))
applied before widening, and 16-bit LVC kernels are widened from their rounded values.  A reference works on ONE sequence of its own length;
the ragged batch is the caller's loop over slots (tests/test_gpu_univnet_forms.py).

Bound (the form and the names of tests/gemm_reference.py):  |got - ref| <= e,
    e_acc = U (C1 sqrt(K) S + C2 mag) + U S          U = 2^-24; the last term: fp32 operands, the rounding of each product
  S    sum |w x| + |bias| of the element; K = Cin k (96 dilated convolution and LVC, 448 conv_pre, 224 conv_post, 64 convt1d);
  mag  magnitude of what is rounded after the accumulation (pre-activation value, activation output, residual, result).
  LeakyReLU output (|slope| <= 1): e = e_acc.   tanh output: e = e_acc + TANH_ULPS ulp(tanh)     (Lipschitz constant 1), ulp(v) = 2^-23 |v|.
  gate  x += sigmoid(a) tanh(b):  dg = e_acc(a) / 4 + SIGMOID_ULPS ulp(g),  dt = e_acc(b) + TANH_ULPS ulp(t)  (Lipschitz 1/4 and 1),
        e = |t| dg + |g| dt + dg dt + U C2 (|g t| + |x| + |x + g t|)          (product rule; the product, the residual add)
C1 = 1, C2 = 4: the project's constants.  One exception, forced by a CPU emulation and by no kernel: C1_CONVT = 2 for convt1d.  Its chain is the
shortest here (K = 64: 32 paired-tap sums and 32 accumulator adds, each rounded at the size of the partial sum), so sqrt(K) S = 8 S leaves the
random walk of those roundings the least room, and the fp32 emulation of that order reaches 0.548 of the C1 = 1 bound at one element of 4 10^5
(gauss, stride 4, Tin = 257) - above the 0.5 an emulation may use.  With C1_CONVT = 2 it stands at 0.33.

Activation term.  tanhf and the expf sigmoid 1 / (1 + expf(-a)) are library functions.  Their error is measured with the arithmetic taken out
(activation_probe: one-hot centre taps, zero bias and residual, so the accumulated value is an input element exactly and the other factor of the
gate is exactly 1; conv_post's tanh through a one-hot centre tap) on a dense grid over [-12, 12] (49152 points; 8192 at hop 8), in ulps of the
fp64 result, by tests/test_gpu_univnet_forms.py::test_activation_error on every LVC form and conv1d_direct_kernel<1>:
  measured on the MI355X: tanhf 1.202 ulp, the sigmoid 1.875 ulp (worst over the forms);
  chosen: TANH_ULPS = 3, SIGMOID_ULPS = 4 (twice the worst, rounded up to a whole ulp).  The test asserts twice the measured worst <= the constant.

CPU emulations (tests/test_univnet_reference_cpu.py; every family; fp32 in each form's summation order: the per-sample tap-then-channel chain
of fused multiply-adds, the MFMA's two-k steps (two rounded products summed, then added to the accumulator) with the bias last, the LVC's
three-tap groups, convt's paired taps), worst |err| / bound:
  conv1d_direct_kernel<32> k = 3 0.420, conv1d_mfma_kernel 0.268, conv1d_direct_kernel<32> k = 7 reflect 0.171, conv1d_direct_kernel<1> k = 7
  reflect tanh 0.111, convt1d_kernel 0.326, lvc_kernel 0.115, lvc_mfma_kernel 0.128
Kernels on the MI355X (tests/test_gpu_univnet_forms.py, worst |err| / bound per form over every case of the module):
  conv1d_mfma_kernel 0.528, conv1d_direct_kernel<32> 0.460 (k = 3 and k = 7), conv1d_direct_kernel<1> 0.167, convt1d_kernel 0.335,
  lvc_kernel<f32 / f16 / bf16, 8> 0.089 / 0.090 / 0.086, <., 64> 0.120 / 0.108 / 0.099, <., 256> 0.133 / 0.116 / 0.130,
  lvc_mfma_kernel<f32 / f16 / bf16, 64> 0.158 / 0.175 / 0.169, <., 256> 0.207 / 0.196 / 0.178
The VALU kernels land on their emulations' figures to three digits where the cases coincide (the emulation is the kernel's order); the matrix
cores sum a two-k step in an order of their own, so their figures differ from the emulation's and stay inside the bound.
"""
import math

import torch

from tests.gemm_reference import C1, C2, U

ULP = 2.0 ** -23
C1_CONVT = 2.0  # (the docstring: forced by the emulation of convt1d's summation order)
TANH_ULPS = 3     # twice the measured 1.202 ulp, rounded up (the docstring)
SIGMOID_ULPS = 4  # twice the measured 1.875 ulp, rounded up

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 4, 5
FAMILIES = ("gauss", "offset", "onehot")
KDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


class Ref:
    """value: the fp64 reference of one sequence; bound: the element-wise bound e"""

    def __init__(self, value, bound):
        self.value, self.bound = value, bound


def lrelu32(x, slope):
    """the kernels' input LeakyReLU, their own fp32 operation; slope < 0: none"""
    x = x.float()
    if slope < 0:
        return x
    return torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32, device=x.device))


def e_acc(S, mag, K, c1=C1):
    return U * (c1 * math.sqrt(K) * S + C2 * mag) + U * S


def _out_act(acc, S, K, out_act, out_slope):
    if out_act == ACT_NONE:
        return Ref(acc, e_acc(S, acc.abs(), K))
    if out_act == ACT_LRELU:
        assert abs(out_slope) <= 1.0
        s = float(torch.tensor(out_slope, dtype=torch.float32))
        y = torch.where(acc > 0, acc, acc * s)
        return Ref(y, e_acc(S, acc.abs() + y.abs(), K))
    assert out_act == ACT_TANH
    y = torch.tanh(acc)
    return Ref(y, e_acc(S, acc.abs() + y.abs(), K) + TANH_ULPS * ULP * y.abs())


# ------------------------------------------------------------------------------------------------- conv1d
def conv1d_operand(x, k, dilation, reflect):
    """[Cin][k][T]: tap kk of column t reads column t + (kk - k // 2) * dilation of the sequence's own T columns; outside them zero, or with
    reflect the mirrored column (torch's 'reflect': needs T > (k // 2) * dilation)"""
    Cin, T = x.shape
    t = torch.arange(T, device=x.device)
    X = torch.zeros(Cin, k, T, dtype=x.dtype, device=x.device)
    for kk in range(k):
        idx = t + (kk - k // 2) * dilation
        if reflect:
            assert T > (k // 2) * dilation
            idx = idx.abs()
            idx = torch.where(idx >= T, 2 * (T - 1) - idx, idx)
            X[:, kk] = x[:, idx]
        else:
            ok = (idx >= 0) & (idx < T)
            X[:, kk, ok] = x[:, idx[ok]]
    return X


def conv1d_reference(x, w, bias, k, dilation, reflect, in_slope, out_act=ACT_NONE, out_slope=0.0):
    """x f32 [Cin][T] (one sequence, its own length), w f32 [Cout][Cin][k], bias f32 [Cout] or None -> Ref of y [Cout][T]"""
    X = conv1d_operand(lrelu32(x, in_slope).double(), k, dilation, reflect)
    w = w.double()
    acc = torch.einsum("oik,ikt->ot", w, X)
    S = torch.einsum("oik,ikt->ot", w.abs(), X.abs())
    if bias is not None:
        acc = acc + bias.double()[:, None]
        S = S + bias.double().abs()[:, None]
    return _out_act(acc, S, w.shape[1] * k, out_act, out_slope)


# ------------------------------------------------------------------------------------------------- convt1d
def convt1d_reference(x, w, bias, stride, in_slope):
    """ConvTranspose1d(C -> C, k = 2 stride, stride, padding stride / 2 + stride % 2): x f32 [C][Tin], w f32 [Cin][Cout][2 stride], bias [C]
    -> Ref of y [C][Tin * stride].  Input column j adds x[:, j] w[:, :, r] to output position stride j + r - padding."""
    s = stride
    p = s // 2 + s % 2
    C, Tin = x.shape
    xa = lrelu32(x, in_slope).double()
    w = w.double()

    def scatter(xv, wv):
        c = torch.einsum("ij,ior->ojr", xv, wv)  # [Cout][Tin][2 s]
        full = torch.zeros(C, (Tin + 1) * s, dtype=torch.float64, device=x.device)
        full[:, :Tin * s] += c[:, :, :s].reshape(C, Tin * s)
        full[:, s:] += c[:, :, s:].reshape(C, Tin * s)
        return full[:, p:p + Tin * s]
    acc = scatter(xa, w) + bias.double()[:, None]
    S = scatter(xa.abs(), w.abs()) + bias.double().abs()[:, None]
    return Ref(acc, e_acc(S, acc.abs(), 2 * C, C1_CONVT))


# ------------------------------------------------------------------------------------------------- LVC + gate + residual
def lvc_operand(x, hop):
    """[32][L][hop][3]: the three-tap windows of every frame, zero outside the sequence's own columns"""
    xp = torch.nn.functional.pad(x, (1, 1))
    return xp.unfold(1, hop + 2, hop).unfold(2, 3, 1)


def lvc_preact(x_in, kern, bias, hop, in_slope):
    """x_in f32 [32][L hop]; kern [L][32][64][3] in its (rounded) type; bias f32 [L][64] -> (o, S) fp64 [64][L hop] as oracle/tortoise_oracle.py
    location_variable_convolution: o[c][l hop + s] = bias[l][c] + sum_{i, k} xpad[i][l hop + s + k] kern[l][i][c][k]"""
    L = kern.shape[0]
    win = lvc_operand(lrelu32(x_in, in_slope).double(), hop)
    kd, bd = kern.float().double(), bias.double()
    o = torch.einsum("ilsk,liok->ols", win, kd) + bd.t()[:, :, None]
    S = torch.einsum("ilsk,liok->ols", win.abs(), kd.abs()) + bd.abs().t()[:, :, None]
    return o.reshape(64, L * hop), S.reshape(64, L * hop)


def lvc_reference(x_in, kern, bias, x_res, hop, in_slope):
    """-> Ref of x_res + sigmoid(o[:32]) * tanh(o[32:]) [32][L hop]"""
    o, S = lvc_preact(x_in, kern, bias, hop, in_slope)
    a, b, Sa, Sb = o[:32], o[32:], S[:32], S[32:]
    g, t = torch.sigmoid(a), torch.tanh(b)
    dg = e_acc(Sa, a.abs(), 96) / 4 + SIGMOID_ULPS * ULP * g
    dt = e_acc(Sb, b.abs(), 96) + TANH_ULPS * ULP * t.abs()
    xr = x_res.double()
    y = xr + g * t
    return Ref(y, t.abs() * dg + g * dt + dg * dt + U * C2 * ((g * t).abs() + xr.abs() + y.abs()))


# ------------------------------------------------------------------------------------------------- comparison
def ratio(got, ref):
    """|got - ref| / bound per element; a non-finite output is an infinite ratio"""
    g = got.detach().to(ref.value.device).double()
    assert g.shape == ref.value.shape, (tuple(g.shape), tuple(ref.value.shape))
    r = (g - ref.value).abs() / ref.bound.clamp_min(1e-300)
    r = torch.where((g - ref.value) == 0, torch.zeros_like(r), r)
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def assert_within_bound(name, got, ref, limit=1.0):
    """every element within limit * bound; returns the worst ratio"""
    r = ratio(got, ref)
    worst = float(r.max()) if r.numel() else 0.0
    bad = r > limit
    if bool(bad.any()):
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} element(s) outside {limit} x bound (worst ratio {worst:.3f}), first at {i}: got "
                             f"{float(got[i]):.9e} want {float(ref.value[i]):.9e} bound {float(ref.bound[i]):.3e}")
    return worst


def ulps(got, want64):
    """|got - want| in ulps of the fp32 value nearest want (2^(e - 24) for |want| = m 2^e, 0.5 <= m < 1)"""
    _, e = torch.frexp(want64)
    return (got.double() - want64).abs() / torch.ldexp(torch.ones_like(want64), e - 24)


# ------------------------------------------------------------------------------------------------- input families
def _gen(*key):
    seed = 0
    for v in key:
        for ch in str(v):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _grid(shape, g):
    """a dense grid over [-12, 12] in a deterministic shuffle"""
    n = math.prod(shape)
    v = torch.linspace(-12.0, 12.0, n, dtype=torch.float64)[torch.randperm(n, generator=g)]
    return v.float().reshape(shape)


def _signal(fam, n, C, P, g):
    """[n][C][P]: every channel has its own scale and offset"""
    if fam == "onehot":
        return _grid((n, C, P), g)
    c = torch.arange(C, dtype=torch.float32)
    scale = (0.5 + (c * 7 % 11) / 10.0)[None, :, None]
    off = ((c * 5 % 13) - 6.0)[None, :, None] * (0.05 if fam == "gauss" else 0.4)
    return torch.randn(n, C, P, generator=g) * scale + off + (1.5 if fam == "offset" else 0.0)


def conv_weights(fam, Cout, Cin, k, g, transposed=False):
    """w [Cout][Cin][k] (transposed: [Cin][Cout][k]) and bias [Cout].  onehot: one unit weight per output channel (input channel
    (5 co + 3) % Cin, tap co % k) and zero bias"""
    if fam == "onehot":
        w = torch.zeros(Cout, Cin, k)
        co = torch.arange(Cout)
        w[co, (5 * co + 3) % Cin, co % k] = 1.0
        bias = torch.zeros(Cout)
    else:
        sd = 1.0 / math.sqrt(Cin * k)
        co = torch.arange(Cout, dtype=torch.float32)
        w = torch.randn(Cout, Cin, k, generator=g) * sd * (0.6 + (co * 3 % 7) / 5.0)[:, None, None]
        if fam == "offset":  # mean-shifted with alternating sign along the input channel: the sums cancel
            w = w + 2.0 * sd * (1.0 - 2.0 * (torch.arange(Cin) % 2).float())[None, :, None]
        bias = torch.randn(Cout, generator=g) * 0.3 + ((co % 5) - 2.0) * 0.1
    return (w.transpose(0, 1).contiguous() if transposed else w), bias


def conv1d_inputs(fam, Cin, Cout, k, P, n=1):
    """x [n][Cin][P], w [Cout][Cin][k], bias [Cout] (host tensors, deterministic in the arguments)"""
    g = _gen("conv1d", fam, Cin, Cout, k, P, n)
    x = _signal(fam, n, Cin, P, g)
    w, bias = conv_weights(fam, Cout, Cin, k, g)
    return {"x": x, "w": w, "bias": bias}


def convt1d_inputs(fam, stride, P, n=1):
    """x [n][32][P], w [32][32][2 stride] ([Cin][Cout][tap]), bias [32]"""
    g = _gen("convt1d", fam, stride, P, n)
    x = _signal(fam, n, 32, P, g)
    w, bias = conv_weights(fam, 32, 32, 2 * stride, g, transposed=True)
    return {"x": x, "w": w, "bias": bias}


def lvc_inputs(fam, kname, L, hop, n=1):
    """x_in, x_res [n][32][L hop] f32; kern [n][L][32][64][3] in the type kname (already rounded); bias [n][L][64] f32.  onehot: output channel c
    of frame l reads input channel (5 c + 3 + l) % 32 at tap (c + l) % 3 with weight one, zero bias"""
    g = _gen("lvc", fam, kname, L, hop, n)
    x_in = _signal(fam, n, 32, L * hop, g)
    x_res = torch.randn(n, 32, L * hop, generator=g) * 0.7
    if fam == "onehot":
        kern = torch.zeros(n, L, 32, 64, 3)
        c = torch.arange(64)
        for l in range(L):
            kern[:, l, (5 * c + 3 + l) % 32, c, (c + l) % 3] = 1.0
        bias = torch.zeros(n, L, 64)
    else:
        sd = 1.0 / math.sqrt(96.0)
        c = torch.arange(64, dtype=torch.float32)
        kern = torch.randn(n, L, 32, 64, 3, generator=g) * sd * (0.6 + (c * 3 % 7) / 5.0)[None, None, None, :, None]
        if fam == "offset":
            kern = kern + 2.0 * sd * (1.0 - 2.0 * (torch.arange(32) % 2).float())[None, None, :, None, None]
        bias = torch.randn(n, L, 64, generator=g) * 0.3 + ((c % 5) - 2.0)[None, None, :] * 0.1
    return {"x_in": x_in, "x_res": x_res, "kern": kern.to(KDT[kname]), "bias": bias}


def activation_probe(L, hop):
    """LVC inputs that take the arithmetic out of the gate (one frame sequence of L frames): x_in channel 0 is a dense grid over [-12, 12],
    channel 1 holds 30 (tanhf(30) = 1) and channel 2 holds 88 (1 / (1 + expf(-88)) = 1); centre taps of one; zero bias and residual.  Output
    channel 0 = sigmoid(grid) * 1, output channel 1 = 1 * tanh(grid), each carrying the library's error alone."""
    T = L * hop
    x_in = torch.zeros(32, T)
    x_in[0] = torch.linspace(-12.0, 12.0, T, dtype=torch.float64).float()
    x_in[1], x_in[2] = 30.0, 88.0
    kern = torch.zeros(L, 32, 64, 3)
    kern[:, 0, 0, 1] = 1.0   # a of output 0 = grid
    kern[:, 1, 32, 1] = 1.0  # b of output 0 = 30
    kern[:, 2, 1, 1] = 1.0   # a of output 1 = 88
    kern[:, 0, 33, 1] = 1.0  # b of output 1 = grid
    grid = x_in[0].double()
    return {"x_in": x_in, "x_res": torch.zeros(32, T), "kern": kern, "bias": torch.zeros(L, 64), "sigmoid": torch.sigmoid(grid), "tanh": torch.tanh(grid)}


# ------------------------------------------------------------------------------------------------- fp32 emulations of the summation orders
def _act32(v, out_act, out_slope):
    if out_act == ACT_LRELU:
        return torch.where(v > 0, v, v * torch.tensor(out_slope, dtype=torch.float32))
    return torch.tanh(v) if out_act == ACT_TANH else v


def _fma(a, b, c):
    """fl32(a b + c) with one rounding: the product of two fp32 values is exact in fp64 (the second rounding, fp64 to fp32, moves the result by at
    most 2^-29 ulp).  The VALU kernels' products are fused into the add they feed, as the compiler contracts them (-ffp-contract=fast, HIP's default)"""
    return (a.double() * b.double() + c.double()).float()


def emulate_conv1d_direct(x, w, bias, k, dilation, reflect, in_slope, out_act=ACT_NONE, out_slope=0.0):
    """conv1d_direct_kernel: per sample acc = bias, then taps outermost, channels inside, one fused multiply-add at a time"""
    X = conv1d_operand(lrelu32(x, in_slope), k, dilation, reflect)  # f32 [Cin][k][T]
    Cout, Cin = w.shape[0], w.shape[1]
    acc = (bias if bias is not None else torch.zeros(Cout))[:, None].float().expand(Cout, x.shape[1]).clone()
    for kk in range(k):
        for ci in range(Cin):
            acc = _fma(X[ci, kk][None, :], w[:, ci, kk][:, None], acc)
    return _act32(acc, out_act, out_slope)


def _mfma_chain(A, B):
    """sum over kidx of A[kidx][row] B[kidx][col] as 32x32x2 steps from zero: two products summed, then added to the accumulator (fp32)"""
    acc = torch.zeros(A.shape[1], B.shape[1])
    for p in range(A.shape[0] // 2):
        acc = acc + (A[2 * p][:, None] * B[2 * p][None, :] + A[2 * p + 1][:, None] * B[2 * p + 1][None, :])
    return acc


def emulate_conv1d_mfma(x, w, bias, dilation, in_slope, out_act=ACT_NONE, out_slope=0.0):
    """conv1d_mfma_kernel: kidx = 3 ci + tap in 48 two-k steps from zero, the bias added last"""
    X = conv1d_operand(lrelu32(x, in_slope), 3, dilation, False).reshape(96, -1)
    acc = _mfma_chain(w.reshape(32, 96).t().contiguous(), X)
    if bias is not None:
        acc = acc + bias[:, None]
    return _act32(acc, out_act, out_slope)


def emulate_convt1d(x, w, bias, stride, in_slope):
    """convt1d_kernel: acc = bias, then per input channel acc += x[j] w[r] + x[j - 1] w[r + s] (the paired taps summed first)"""
    s = stride
    p = s // 2
    C, Tin = x.shape
    xa = lrelu32(x, in_slope)
    t = torch.arange(Tin * s)
    j, r = (t + p) // s, (t + p) % s
    x0 = torch.where((j < Tin)[None, :], xa[:, j.clamp(max=Tin - 1)], torch.zeros(()))
    x1 = torch.where((j >= 1)[None, :], xa[:, (j - 1).clamp(min=0)], torch.zeros(()))
    acc = bias[:, None].float().expand(C, Tin * s).clone()
    for ci in range(C):
        acc = acc + _fma(x1[ci][None, :], w[ci][:, r + s], x0[ci][None, :] * w[ci][:, r])
    return acc


def _gate32(a, b, x_res):
    return x_res + (1.0 / (1.0 + torch.exp(-a))) * torch.tanh(b)


def emulate_lvc(x_in, kern, bias, x_res, hop, in_slope):
    """lvc_kernel: acc = bias, then per input channel acc += x0 w0 + x1 w1 + x2 w2 (summed left to right first)"""
    L = kern.shape[0]
    win = lvc_operand(lrelu32(x_in, in_slope), hop)  # [32][L][hop][3]
    kf = kern.float()
    acc = bias.t()[:, :, None].float().expand(64, L, hop).clone()
    for ci in range(32):
        wv = kf[:, ci].permute(1, 0, 2)[:, :, None, :]  # [64][L][1][3]
        xv = win[ci][None]                              # [1][L][hop][3]
        acc = acc + _fma(xv[..., 2], wv[..., 2], _fma(xv[..., 1], wv[..., 1], xv[..., 0] * wv[..., 0]))
    acc = acc.reshape(64, L * hop)
    return _gate32(acc[:32], acc[32:], x_res)


def emulate_lvc_mfma(x_in, kern, bias, x_res, hop, in_slope):
    """lvc_mfma_kernel: per frame kidx = 3 ci + tap in 48 two-k steps from zero, the bias added last"""
    L = kern.shape[0]
    win = lvc_operand(lrelu32(x_in, in_slope), hop)
    kf = kern.float()
    out = []
    for l in range(L):
        A = kf[l].permute(0, 2, 1).reshape(96, 64)          # [3 ci + tap][c]
        B = win[:, l].permute(0, 2, 1).reshape(96, hop)     # [3 ci + tap][s]
        out.append(_mfma_chain(A, B) + bias[l][:, None])
    acc = torch.cat(out, dim=1)
    return _gate32(acc[:32], acc[32:], x_res)
