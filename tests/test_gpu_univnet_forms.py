"""-m gpu: every audio-rate UnivNet kernel form of csrc/univnet.hip one launch at a time through tt_op_conv1d_ex / tt_op_convt1d_ex /
tt_op_lvc_ex, against the fp64 references of tests/univnet_reference.py with an element-wise bound.  Every launch asserts the host-side record
of what started (`ran`: kernel and grid, or kernel, HOP and kernel element type), so a change of the dispatch in conv1d_direct_launch /
lvc_launch cannot silently stop covering a kernel; the form is steered with the TTX_VOC_MFMA switch (restored in a finally).  Outputs are
pre-filled with a sentinel; NaN stands wherever the operation says nothing is read (the x columns of a slot past the sequence's own length,
the kernel and bias rows of frames >= frames[b], the unselected koff / boff blocks), and no element is left out of the bound: a non-finite
output is an infinite ratio.  The one-hot family must come out equal to the selected, LeakyReLU'd input element exactly (indexing apart from
arithmetic).  Ragged batches (VocSeqs) on both forms of every family: the valid range meets the bound, everything of a slot beyond the
sequence's own length keeps the sentinel bit for bit, every sequence is torch.equal to the same sequence launched alone through the n = 0
form, and a second launch reproduces the first.  The LVC guard counter stays 0 on finite kernels and counts the frames with a +inf tap.  The
reflect padding the kernel cannot index is a host refusal (nothing launches).  In situ, VocoderStage.inference runs with the switch at 0 and
at 1 against the oracle - the only place where the VALU forms run inside the stage.  Each launch prints a [parity] line; the last line of a
module run lists the worst |err| / bound per form (the figures in the docstring of tests/univnet_reference.py) and the module's wall time.

Findings: none in the kernels - every form stayed inside the bound, every sentinel, one-hot and batch == alone check held (MI355X).  From
reading the code: conv1d_direct_kernel reflects an index once, so a sequence of T <= (k / 2) * dilation columns would have been read before its
row; conv1d_direct_launch now refuses it (test_reflect_padding_refusal; no launch is ever made at such a length).
"""
import ctypes as C
import functools
import math
import time

import pytest
import torch

from tortoise_tts_amd import engine as E
from tests import univnet_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
KDT_CODE = {"f32": E.TT_F32, "f16": E.TT_F16, "bf16": E.TT_BF16}
WORST = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    t0 = time.time()
    yield E.init()
    for f in (conv1d_operands, conv1d_ref, convt1d_operands, convt1d_ref, lvc_operands, lvc_ref):
        f.cache_clear()
    torch.cuda.empty_cache()
    print("[bound] univnet worst |err|/bound per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + f"; module wall time {time.time() - t0:.1f} s")


def cdiv(a, b):
    return (a + b - 1) // b


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def seq_fields(d, seq):
    """seq: None (n = 0: one sequence that fills the tensor) or (mul, frames)"""
    if seq is not None:
        mul, frames = seq
        assert 1 <= len(frames) <= 32
        d.seq_n, d.seq_mul = len(frames), mul
        for i, f in enumerate(frames):
            d.seq_frames[i] = f


def lengths(seq, P):
    return [P] if seq is None else [f * seq[0] for f in seq[1]]


def switched(lib, switch, fn):
    torch.cuda.synchronize()
    prev = lib.ttx_kernel_variant(E.TTX_VOC_MFMA, switch)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.ttx_kernel_variant(E.TTX_VOC_MFMA, prev)
    return out


def note(form, name, worst):
    print(f"[parity] univnet {form} {name}: worst |err|/bound={worst:.3f}")
    WORST[form] = max(WORST.get(form, 0.0), worst)


# ------------------------------------------------------------------------------------------------- conv1d
CONV_FORMS = {"conv1d_direct_kernel<32>": (0, 256), "conv1d_direct_kernel<1>": (1, 256), "conv1d_mfma_kernel": (2, 128)}  # ran[0], columns per workgroup


@functools.lru_cache(maxsize=None)
def conv1d_operands(fam, Cin, Cout, k, P, seq):
    """device operands of one case, made once (no test writes to them); x columns past a sequence's own length hold NaN"""
    n = 1 if seq is None else len(seq[1])
    i = R.conv1d_inputs(fam, Cin, Cout, k, P, n)
    x = i["x"].clone()
    for b, T in enumerate(lengths(seq, P)):
        assert 1 <= T <= P
        x[b, :, T:] = NAN
    return {"x": x.cuda().contiguous(), "w": i["w"].cuda().contiguous(), "bias": i["bias"].cuda().contiguous()}


@functools.lru_cache(maxsize=None)
def conv1d_ref(fam, Cin, Cout, k, P, seq, d, reflect, in_slope, out_act, out_slope):
    """the fp64 reference and bound of every sequence, computed on the device"""
    o = conv1d_operands(fam, Cin, Cout, k, P, seq)
    return [R.conv1d_reference(o["x"][b, :, :T], o["w"], o["bias"], k, d, reflect, in_slope, out_act, out_slope) for b, T in enumerate(lengths(seq, P))]


def conv1d_launch(lib, form, switch, x, w, bias, Cin, Cout, P, k, d, reflect, in_slope, out_act, out_slope, seq):
    """one launch; asserts `ran`; returns y [n][Cout][P] (sentinel where nothing was written)"""
    n = 1 if seq is None else len(seq[1])
    assert x.shape == (n, Cin, P) and w.shape == (Cout, Cin, k) and bias.shape == (Cout,)
    y = torch.full((n, Cout, P), SENTINEL, device="cuda")
    desc = E.Conv1dDesc(x=E.ptr(x), w=E.ptr(w), bias=E.ptr(bias), y=E.ptr(y), Cin=Cin, Cout=Cout, T=P, k=k, dilation=d, reflect=reflect,
                        in_slope=in_slope, out_act=out_act, out_slope=out_slope)
    seq_fields(desc, seq)
    ran = (C.c_int * 4)(-2, -2, -2, -2)
    switched(lib, switch, lambda: E.check(lib.tt_op_conv1d_ex(C.byref(desc), ran, None)))
    kernel, cols = CONV_FORMS[form]
    assert tuple(ran) == (kernel, cdiv(P, cols), n, 0), f"{form} switch={switch} d={d} P={P} n={n}: launched {E.CONV1D_KERNELS.get(ran[0], ran[0])} grid {ran[1]} x {ran[2]}"
    return y


def conv1d_check(lib, form, switch, fam, Cin, Cout, k, P, d, reflect, in_slope, out_act, out_slope=0.2, seq=None):
    o = conv1d_operands(fam, Cin, Cout, k, P, seq)
    refs = conv1d_ref(fam, Cin, Cout, k, P, seq, d, reflect, in_slope, out_act, out_slope)
    y = conv1d_launch(lib, form, switch, o["x"], o["w"], o["bias"], Cin, Cout, P, k, d, reflect, in_slope, out_act, out_slope, seq)
    name = f"{fam} Cin={Cin} k={k} d={d} P={P} seq={seq} in_slope={in_slope} out_act={out_act}"
    for b, T in enumerate(lengths(seq, P)):
        got = y[b, :, :T]
        note(form, f"{name} b={b}", R.assert_within_bound(f"{form} {name} b={b}", got, refs[b]))
        if fam == "onehot" and out_act == R.ACT_NONE:
            assert torch.equal(got.double(), refs[b].value), f"{form} {name} b={b}: one-hot weights did not select the input element exactly"
        assert bits_equal(y[b, :, T:], torch.full_like(y[b, :, T:], SENTINEL)), f"{form} {name} b={b}: columns past the sequence's own length {T} were written"
    return y


DILATIONS = (1, 2, 3, 9, 26, 27)
K3_T = (1, 26, 127, 128, 129, 300)
K3_ACTS = ((0.2, R.ACT_LRELU), (0.2, R.ACT_NONE), (-1.0, R.ACT_LRELU), (-1.0, R.ACT_NONE))


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("form,switch", [("conv1d_mfma_kernel", 1), ("conv1d_direct_kernel<32>", 0)])
def test_conv1d_k3(lib, form, switch, d):
    """the 32 -> 32 dilated convolution with zero padding on both forms: lengths of one column, below the dilation (the whole input window
    of a T = 26 sequence lies in the padding below d = 27), at and one past the 128-column tile, more than one workgroup"""
    for T in K3_T:
        for in_slope, out_act in K3_ACTS:
            for fam in R.FAMILIES:
                conv1d_check(lib, form, switch, fam, 32, 32, 3, T, d, 0, in_slope, out_act)


def test_conv1d_k3_d28_falls_back(lib):
    """d = 28 is past the MFMA kernel's window: with the switch at 1 `ran` must show conv1d_direct_kernel<32>, whose zero-padding branch runs"""
    for T in K3_T:
        for fam in R.FAMILIES:
            conv1d_check(lib, "conv1d_direct_kernel<32>", 1, fam, 32, 32, 3, T, 28, 0, 0.2, R.ACT_LRELU)


K7_T = (4, 11, 255, 256, 257)


@pytest.mark.parametrize("switch", [0, 1])
def test_conv1d_k7_reflect(lib, switch):
    """conv_pre (64 -> 32) and conv_post (32 -> 1, LeakyReLU in, tanh out) with reflect padding: T = 4 is the shortest the padding can index"""
    for T in K7_T:
        for fam in R.FAMILIES:
            conv1d_check(lib, "conv1d_direct_kernel<32>", switch, fam, 64, 32, 7, T, 1, 1, -1.0, R.ACT_NONE)
            conv1d_check(lib, "conv1d_direct_kernel<1>", switch, fam, 32, 1, 7, T, 1, 1, 0.2, R.ACT_TANH)
            conv1d_check(lib, "conv1d_direct_kernel<1>", switch, fam, 32, 1, 7, T, 1, 1, -1.0, R.ACT_NONE)


def test_reflect_padding_refusal(lib):
    """a sequence of no more than (k / 2) * dilation columns cannot be indexed by one reflection: a negative return with an error text and
    nothing launched, for the n = 0 form and for one short sequence of a batch"""
    i = conv1d_operands("gauss", 64, 32, 7, 64, (1, (64, 3)))
    for P, seq in ((3, None), (64, (1, (64, 3))), (64, (3, (21, 1)))):
        y = torch.full((2, 32, 64), SENTINEL, device="cuda")
        desc = E.Conv1dDesc(x=E.ptr(i["x"]), w=E.ptr(i["w"]), bias=E.ptr(i["bias"]), y=E.ptr(y), Cin=64, Cout=32, T=P, k=7, dilation=1, reflect=1,
                            in_slope=-1.0, out_act=0, out_slope=0.0)
        seq_fields(desc, seq)
        ran = (C.c_int * 4)(-2, -2, -2, -2)
        rc = lib.tt_op_conv1d_ex(C.byref(desc), ran, None)
        torch.cuda.synchronize()
        assert rc < 0 and b"reflect" in lib.tt_last_error(), (rc, lib.tt_last_error())
        assert tuple(ran) == (-1, 0, 0, 0), tuple(ran)
        assert bits_equal(y, torch.full_like(y, SENTINEL))


RAGGED = [(64, (5, 1, 2, 3)), (1, (300, 129, 127, 1)), (51, tuple(1 + (7 * b + 3) % 5 for b in range(32)))]
RAGGED_REFLECT = [(64, (5, 1, 2, 3)), (1, (300, 257, 256, 4)), (51, tuple(1 + (7 * b + 3) % 5 for b in range(32)))]


def ragged_alone(y, y2, alone, seq, P, what):
    """batch == alone, bit for bit, and the second launch reproduces the first"""
    assert bits_equal(y, y2), f"{what}: two launches of one batch differ"
    for b, T in enumerate(lengths(seq, P)):
        a = alone(b, T)
        assert torch.equal(y[b, :, :a.shape[-1]], a), f"{what}: sequence {b} of the batch differs from the same sequence launched alone"


@pytest.mark.parametrize("seq", RAGGED)
@pytest.mark.parametrize("form,switch", [("conv1d_mfma_kernel", 1), ("conv1d_direct_kernel<32>", 0)])
def test_conv1d_k3_ragged(lib, form, switch, seq):
    P = max(lengths(seq, 0))
    for d in (1, 27):
        for fam in ("gauss", "onehot"):
            args = (32, 32, 3, P, d, 0, 0.2, R.ACT_LRELU if fam == "gauss" else R.ACT_NONE)
            y = conv1d_check(lib, form, switch, fam, *args, seq=seq)
            y2 = conv1d_check(lib, form, switch, fam, *args, seq=seq)
            o = conv1d_operands(fam, 32, 32, 3, P, seq)

            def alone(b, T):
                return conv1d_launch(lib, form, switch, o["x"][b:b + 1, :, :T].contiguous(), o["w"], o["bias"], 32, 32, T, 3, d, 0, 0.2, args[-1], 0.2, None)[0]
            ragged_alone(y, y2, alone, seq, P, f"{form} {fam} d={d} seq={seq}")


@pytest.mark.parametrize("seq", RAGGED_REFLECT)
@pytest.mark.parametrize("form,Cin,Cout,in_slope,out_act", [("conv1d_direct_kernel<32>", 64, 32, -1.0, R.ACT_NONE), ("conv1d_direct_kernel<1>", 32, 1, 0.2, R.ACT_TANH)])
def test_conv1d_k7_reflect_ragged(lib, form, Cin, Cout, in_slope, out_act, seq):
    """the reflect padding against each sequence's OWN length (no sequence of one column here: the launcher refuses it)"""
    P = max(lengths(seq, 0))
    for fam in ("gauss", "onehot"):
        args = (Cin, Cout, 7, P, 1, 1, in_slope, out_act)
        y = conv1d_check(lib, form, 1, fam, *args, seq=seq)
        y2 = conv1d_check(lib, form, 1, fam, *args, seq=seq)
        o = conv1d_operands(fam, Cin, Cout, 7, P, seq)

        def alone(b, T):
            return conv1d_launch(lib, form, 1, o["x"][b:b + 1, :, :T].contiguous(), o["w"], o["bias"], Cin, Cout, T, 7, 1, 1, in_slope, out_act, 0.2, None)[0]
        ragged_alone(y, y2, alone, seq, P, f"{form} {fam} seq={seq}")


# ------------------------------------------------------------------------------------------------- convt1d
@functools.lru_cache(maxsize=None)
def convt1d_operands(fam, stride, P, seq):
    n = 1 if seq is None else len(seq[1])
    i = R.convt1d_inputs(fam, stride, P, n)
    x = i["x"].clone()
    for b, T in enumerate(lengths(seq, P)):
        assert 1 <= T <= P
        x[b, :, T:] = NAN
    return {"x": x.cuda().contiguous(), "w": i["w"].cuda().contiguous(), "bias": i["bias"].cuda().contiguous()}


@functools.lru_cache(maxsize=None)
def convt1d_ref(fam, stride, P, seq, in_slope):
    o = convt1d_operands(fam, stride, P, seq)
    return [R.convt1d_reference(o["x"][b, :, :T], o["w"], o["bias"], stride, in_slope) for b, T in enumerate(lengths(seq, P))]


def convt1d_launch(lib, x, w, bias, P, stride, in_slope, seq):
    n = 1 if seq is None else len(seq[1])
    assert x.shape == (n, 32, P) and w.shape == (32, 32, 2 * stride) and bias.shape == (32,)
    y = torch.full((n, 32, P * stride), SENTINEL, device="cuda")
    desc = E.ConvT1dDesc(x=E.ptr(x), w=E.ptr(w), bias=E.ptr(bias), y=E.ptr(y), C=32, Tin=P, stride=stride, in_slope=in_slope)
    seq_fields(desc, seq)
    ran = (C.c_int * 4)(-2, -2, -2, -2)
    E.check(lib.tt_op_convt1d_ex(C.byref(desc), ran, None))
    torch.cuda.synchronize()
    assert tuple(ran) == (0, cdiv(P + 1, 256), stride, n), f"convt1d stride={stride} P={P} n={n}: grid {tuple(ran)[1:]}"
    return y


def convt1d_check(lib, fam, stride, P, in_slope, seq=None):
    o = convt1d_operands(fam, stride, P, seq)
    refs = convt1d_ref(fam, stride, P, seq, in_slope)
    y = convt1d_launch(lib, o["x"], o["w"], o["bias"], P, stride, in_slope, seq)
    name = f"{fam} stride={stride} P={P} seq={seq} in_slope={in_slope}"
    for b, T in enumerate(lengths(seq, P)):
        got = y[b, :, :T * stride]
        note("convt1d_kernel", f"{name} b={b}", R.assert_within_bound(f"convt1d_kernel {name} b={b}", got, refs[b]))
        if fam == "onehot":
            assert torch.equal(got.double(), refs[b].value), f"convt1d_kernel {name} b={b}: one-hot weights did not select the input element exactly"
        assert bits_equal(y[b, :, T * stride:], torch.full_like(y[b, :, T * stride:], SENTINEL)), f"convt1d_kernel {name} b={b}: columns past the sequence's own output were written"
    return y


@pytest.mark.parametrize("stride", [8, 4, 2])
def test_convt1d(lib, stride):
    """Tin of one and two columns, and 255 / 256 / 257: the input j = Tin (the last outputs' second tap) belongs to the second workgroup at 256"""
    for Tin in (1, 2, 255, 256, 257):
        for fam in R.FAMILIES:
            for in_slope in (0.2, -1.0):
                convt1d_check(lib, fam, stride, Tin, in_slope)


@pytest.mark.parametrize("seq", RAGGED)
@pytest.mark.parametrize("stride", [8, 2])
def test_convt1d_ragged(lib, stride, seq):
    P = max(lengths(seq, 0))
    for fam in ("gauss", "onehot"):
        y = convt1d_check(lib, fam, stride, P, 0.2, seq)
        y2 = convt1d_check(lib, fam, stride, P, 0.2, seq)
        o = convt1d_operands(fam, stride, P, seq)

        def alone(b, T):
            return convt1d_launch(lib, o["x"][b:b + 1, :, :T].contiguous(), o["w"], o["bias"], T, stride, 0.2, None)[0]
        ragged_alone(y, y2, alone, seq, P, f"convt1d {fam} stride={stride} seq={seq}")


# ------------------------------------------------------------------------------------------------- LVC + gate + residual
LDK, LDB = 4 * 6144, 256
LVC_OFFS = ((0, 0), (2 * 6144, 128))


@functools.lru_cache(maxsize=None)
def lvc_operands(fam, kname, L, hop, frames, koff, boff):
    """frames: None (n = 0) or the frames of every sequence of L-frame slots.  kernels [n L][LDK] in the type kname with the [6144] block at
    koff, bias [n L][LDB] with the [64] block at boff; NaN in every other block, in the rows of frames >= frames[b] and in the x_in columns
    past a sequence's own length; x_res holds the sentinel there"""
    n = 1 if frames is None else len(frames)
    i = R.lvc_inputs(fam, kname, L, hop, n)
    fr = [L] * n if frames is None else list(frames)
    kern = torch.full((n, L, LDK), NAN, dtype=R.KDT[kname])
    kern[:, :, koff:koff + 6144] = i["kern"].reshape(n, L, 6144)
    bias = torch.full((n, L, LDB), NAN)
    bias[:, :, boff:boff + 64] = i["bias"]
    x_in, x_res = i["x_in"].clone(), i["x_res"].clone()
    for b, f in enumerate(fr):
        assert 1 <= f <= L
        kern[b, f:] = NAN
        bias[b, f:] = NAN
        x_in[b, :, f * hop:] = NAN
        x_res[b, :, f * hop:] = SENTINEL
    return {"x_in": x_in.cuda().contiguous(), "x_res": x_res.cuda().contiguous(), "kernels": kern.cuda().contiguous(), "bias": bias.cuda().contiguous(),
            "kern": i["kern"].cuda(), "b": i["bias"].cuda(), "frames": fr}


@functools.lru_cache(maxsize=None)
def lvc_ref(fam, kname, L, hop, frames, in_slope):
    o = lvc_operands(fam, kname, L, hop, frames, 0, 0)
    return [R.lvc_reference(o["x_in"][b, :, :f * hop], o["kern"][b, :f], o["b"][b, :f], o["x_res"][b, :, :f * hop], hop, in_slope) for b, f in enumerate(o["frames"])]


def lvc_launch(lib, form, switch, kname, x_in, kernels, koff, bias, boff, x_res, L, hop, in_slope, frames, guard=None):
    """one in-place launch on a copy of x_res; asserts `ran`; returns the updated x [n][32][L hop]"""
    n = 1 if frames is None else len(frames)
    ldk, ldb = kernels.shape[-1], bias.shape[-1]
    assert x_in.shape == (n, 32, L * hop) and x_res.shape == x_in.shape and kernels.shape == (n, L, ldk) and bias.shape == (n, L, ldb)
    assert kernels.dtype == R.KDT[kname] and 0 <= koff <= ldk - 6144 and 0 <= boff <= ldb - 64
    x = x_res.clone()
    desc = E.LvcDesc(x_in=E.ptr(x_in), kernels=E.ptr(kernels), ldk=ldk, koff=koff, dtype=KDT_CODE[kname], bias=E.ptr(bias), ldb=ldb, boff=boff, x=E.ptr(x),
                     L=L, hop=hop, in_slope=in_slope, guard=E.ptr(guard))
    seq_fields(desc, None if frames is None else (hop, frames))
    ran = (C.c_int * 4)(-2, -2, -2, -2)
    switched(lib, switch, lambda: E.check(lib.tt_op_lvc_ex(C.byref(desc), ran, None)))
    assert tuple(ran) == (1 if form == "lvc_mfma_kernel" else 0, hop, E.LVC_ELEM[kname], 0), f"{form}<{kname},{hop}> switch={switch} in_slope={in_slope}: launched {E.LVC_KERNELS.get(ran[0], ran[0])}<{ran[2]},{ran[1]}>"
    return x


def lvc_check(lib, form, switch, fam, kname, L, hop, koff, boff, in_slope=-1.0, frames=None):
    o = lvc_operands(fam, kname, L, hop, frames, koff, boff)
    refs = lvc_ref(fam, kname, L, hop, frames, in_slope)
    guard = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = lvc_launch(lib, form, switch, kname, o["x_in"], o["kernels"], koff, o["bias"], boff, o["x_res"], L, hop, in_slope, frames, guard)
    key, name = f"{form}<{kname},{hop}>", f"{fam} L={L} frames={frames} koff={koff} boff={boff} in_slope={in_slope}"
    for b, f in enumerate(o["frames"]):
        note(key, f"{name} b={b}", R.assert_within_bound(f"{key} {name} b={b}", x[b, :, :f * hop], refs[b]))
        assert bits_equal(x[b, :, f * hop:], o["x_res"][b, :, f * hop:]), f"{key} {name} b={b}: columns past the sequence's own length were written"
    assert int(guard) == 0, f"{key} {name}: guard counter {int(guard)} on finite kernels"
    return x


LVC_FORMS = [("lvc_kernel", 0, 8), ("lvc_kernel", 0, 64), ("lvc_kernel", 0, 256), ("lvc_mfma_kernel", 1, 64), ("lvc_mfma_kernel", 1, 256)]


@pytest.mark.parametrize("kname", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("form,switch,hop", LVC_FORMS)
def test_lvc(lib, form, switch, hop, kname):
    """one, two and five frames (L = 1: one frame is both the first and the last), both koff / boff blocks of the KernelPredictor's rows"""
    for L in (1, 2, 5):
        for koff, boff in LVC_OFFS:
            for fam in R.FAMILIES:
                lvc_check(lib, form, switch, fam, kname, L, hop, koff, boff)


@pytest.mark.parametrize("hop", [8, 64, 256])
def test_lvc_in_slope_runs_the_valu_kernel(lib, hop):
    """an input LeakyReLU is not in the MFMA kernel: with the switch at 1 `ran` must show lvc_kernel"""
    for fam in R.FAMILIES:
        lvc_check(lib, "lvc_kernel", 1, fam, "f32", 2, hop, 2 * 6144, 128, in_slope=0.2)


LVC_RAGGED = [(5, (5, 1, 3, 5, 2)), (5, (5, 1, 2, 3)), (5, tuple(1 + (7 * b + 3) % 5 for b in range(32)))]


@pytest.mark.parametrize("L,frames", LVC_RAGGED)
@pytest.mark.parametrize("form,switch,hop", LVC_FORMS)
def test_lvc_ragged(lib, form, switch, hop, L, frames):
    for kname in (("f32", "f16", "bf16") if len(frames) <= 8 else ("f16",)):
        koff, boff = LVC_OFFS[1]
        x = lvc_check(lib, form, switch, "gauss", kname, L, hop, koff, boff, frames=frames)
        x2 = lvc_check(lib, form, switch, "gauss", kname, L, hop, koff, boff, frames=frames)
        assert bits_equal(x, x2), f"{form}<{kname},{hop}> frames={frames}: two launches of one batch differ"
        o = lvc_operands("gauss", kname, L, hop, frames, koff, boff)
        for b, f in enumerate(frames):
            a = lvc_launch(lib, form, switch, kname, o["x_in"][b:b + 1, :, :f * hop].contiguous(), o["kernels"][b:b + 1, :f].contiguous(), koff,
                           o["bias"][b:b + 1, :f].contiguous(), boff, o["x_res"][b:b + 1, :, :f * hop].contiguous(), f, hop, -1.0, None)
            assert torch.equal(x[b, :, :f * hop], a[0]), f"{form}<{kname},{hop}> frames={frames}: sequence {b} differs from the same sequence launched alone"


@pytest.mark.parametrize("form,switch,hop", LVC_FORMS)
def test_lvc_guard_counts_frames_with_an_infinite_tap(lib, form, switch, hop):
    """one +inf tap in the kernels of f frames: at least one and at most four waves of each affected workgroup count, so the counter lies in
    [f, 4 f]; the sequences without one are bit-identical to the clean run"""
    L, frames, kname = 5, (5, 1, 3, 5, 2), "f16"
    koff, boff = LVC_OFFS[1]
    o = lvc_operands("gauss", kname, L, hop, frames, koff, boff)
    clean = lvc_launch(lib, form, switch, kname, o["x_in"], o["kernels"], koff, o["bias"], boff, o["x_res"], L, hop, -1.0, frames)
    kernels = o["kernels"].clone()
    hit = [(0, 4, 17), (2, 0, 6143), (2, 2, 0)]  # (sequence, frame, element of its [6144] block): f = 3 frames of sequences 0 and 2
    for b, l, e in hit:
        kernels[b, l, koff + e] = float("inf")
    guard = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = lvc_launch(lib, form, switch, kname, o["x_in"], kernels, koff, o["bias"], boff, o["x_res"], L, hop, -1.0, frames, guard)
    f = len(hit)
    print(f"[parity] univnet {form}<{kname},{hop}> guard: {int(guard)} for {f} frames with a +inf tap")
    assert f <= int(guard) <= 4 * f, f"{form}<{kname},{hop}>: guard counter {int(guard)} outside [{f}, {4 * f}]"
    for b in (1, 3, 4):
        assert bits_equal(x[b], clean[b]), f"{form}<{kname},{hop}>: sequence {b} changed with a +inf tap in another sequence's kernels"


# ------------------------------------------------------------------------------------------------- the library functions' own error
def test_activation_error(lib):
    """tanhf and the expf sigmoid with the arithmetic taken out (R.activation_probe; conv_post's tanh through a one-hot centre tap), on a dense
    grid over [-12, 12], in ulps of the fp64 result: the activation term of the bound is at least twice the worst found"""
    worst = {"tanh": 0.0, "sigmoid": 0.0}
    for form, switch, hop in LVC_FORMS:
        L = min(49152 // hop, 1024)  # 49152 points (hop 8: 8192)
        p = R.activation_probe(L, hop)
        z = {k: p[k][None].cuda().contiguous() for k in ("x_in", "x_res", "bias")}
        kernels = p["kern"].reshape(1, L, 6144).cuda().contiguous()
        x = lvc_launch(lib, form, switch, "f32", z["x_in"], kernels, 0, z["bias"], 0, z["x_res"], L, hop, -1.0, None)[0]
        us, ut = float(R.ulps(x[0], p["sigmoid"].cuda()).max()), float(R.ulps(x[1], p["tanh"].cuda()).max())
        print(f"[parity] univnet {form}<f32,{hop}> library error on [-12, 12]: sigmoid {us:.3f} ulp, tanh {ut:.3f} ulp")
        worst["sigmoid"], worst["tanh"] = max(worst["sigmoid"], us), max(worst["tanh"], ut)
    T = 49152
    xg = torch.zeros(1, 32, T)
    xg[0, 0] = torch.linspace(-12.0, 12.0, T, dtype=torch.float64).float()
    w = torch.zeros(1, 32, 7)
    w[0, 0, 3] = 1.0
    y = conv1d_launch(lib, "conv1d_direct_kernel<1>", 1, xg.cuda(), w.cuda(), torch.zeros(1, device="cuda"), 32, 1, T, 7, 1, 1, -1.0, R.ACT_TANH, 0.0, None)
    ut = float(R.ulps(y[0, 0], torch.tanh(xg[0, 0].double()).cuda()).max())
    print(f"[parity] univnet conv1d_direct_kernel<1> library error on [-12, 12]: tanh {ut:.3f} ulp")
    worst["tanh"] = max(worst["tanh"], ut)
    print(f"[bound] univnet library error: tanhf {worst['tanh']:.3f} ulp (TANH_ULPS = {R.TANH_ULPS}), sigmoid {worst['sigmoid']:.3f} ulp (SIGMOID_ULPS = {R.SIGMOID_ULPS})")
    assert math.isfinite(worst["tanh"]) and 2 * worst["tanh"] <= R.TANH_ULPS, worst
    assert math.isfinite(worst["sigmoid"]) and 2 * worst["sigmoid"] <= R.SIGMOID_ULPS, worst


# ------------------------------------------------------------------------------------------------- in situ
@pytest.mark.parametrize("switch", [0, 1])
@torch.no_grad()
def test_vocoder_stage_on_both_forms(lib, switch):
    """VocoderStage.inference on 13 mel frames with the switch at 0 (the only place where the VALU forms run inside the stage) and at 1: the
    weights and the bar of tests/test_gpu_stages.py::test_univnet against the oracle"""
    from oracle import make_golden as G
    from oracle import tortoise_oracle as O
    from tortoise_tts_amd import stages
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.config import VocoderConfig
    from tests.gpu_util import DTYPES, quantize_sd, report
    cfg = VocoderConfig()
    g = torch.Generator().manual_seed(13)
    S = 13
    mel = torch.randn(1, 100, S, generator=g) * 2 - 5
    z = torch.randn(1, 64, S + 10, generator=g)
    for name, dt, tdt, tol in DTYPES:
        sd = quantize_sd(W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(cfg), seed=G.VOC_SEED)), tdt)
        want = O.univnet_inference(sd, cfg, mel, z)
        torch.cuda.synchronize()
        prev = lib.ttx_kernel_variant(E.TTX_VOC_MFMA, switch)
        try:
            st = stages.VocoderStage(sd, cfg, dtype=dt, max_frames=64)
            wav = st.inference(mel, z)
            torch.cuda.synchronize()
            st.close()
        finally:
            lib.ttx_kernel_variant(E.TTX_VOC_MFMA, prev)
        assert wav.shape == (1, 1, S * 256)
        report(f"UnivNet waveform {name} TTX_VOC_MFMA={switch} vs oracle", wav, want, tol * 2)
