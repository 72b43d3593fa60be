"""-m gpu: the GEMM forms of csrc/gemm.h one kernel at a time through tt_op_gemm_ex, against the fp64 references of tests/gemm_reference.py
with element-wise bounds.  Every case asserts the host-side record of what launched (tile, standard-epilogue variant, eight-phase 256 x 256
kernel, shared-halo 3-tap kernel), so a change of the tile choice cannot silently stop covering a kernel.  Each case runs for bf16 and
fp16; the fp32 verification GEMM (one 64 x 64 kernel per epilogue, no serial fold) runs every form it supports.  One line per case:
form, what ran, rel-L2, worst |err| / bound; the last line lists the worst ratio per form.

Bound constants C1 = 1, C2 = 4 (tests/gemm_reference.py, with the worst ratios measured on the MI355X: f32 outputs 0.145 with 16-bit
operands, 0.309 in the fp32 verification GEMM; statistics partials 0.041; T-typed outputs 0.995 of the round-to-nearest limit).
Finding: the statistics epilogue wrote partials for wave tiles that start past M (the 128 x 64 tile at M = 600 wrote row tile 19 of 19),
past the cdiv(M, 32) tiles the engine sizes its partials buffers for; test_statistics_forms keeps a sentinel tile past the end.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tortoise_tts_amd import engine as E
from tortoise_tts_amd import pack
from tests import gemm_reference as R

pytestmark = pytest.mark.gpu
DT16 = [("bf16", E.TT_BF16, torch.bfloat16), ("f16", E.TT_F16, torch.float16)]
F32 = ("f32", E.TT_F32, torch.float32)
DIMS = {"64x64": (64, 64), "128x64": (128, 64), "128x128": (128, 128), "256x256": (256, 256), "32x16": (32, 16), "64x16": (64, 16)}
SENTINEL = 8192.0  # exact in bf16 and fp16
WORST = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield E.init()
    print("[bound] worst |err|/bound per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def operands(seed, M, N, K, tdt):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g).to(tdt)
    W = (torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)).to(tdt)
    return A, W, torch.randn(N, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g)


def desc(**kw):
    d = E.GemmDesc()
    d.taps, d.splitk, d.slope, d.slope_t, d.q_scale = 1, 1, 0.2, 0.2, 1.0
    for k, v in kw.items():
        if k == "gn_vlen":
            for i, x in enumerate(v):
                d.gn_vlen[i] = x
        else:
            setattr(d, k, E.ptr(v) if isinstance(v, torch.Tensor) else v)
    return d


def launch(lib, dt, epi, d, p8=None):
    """one tt_op_gemm_ex call (p8: force the eight-phase kernel on / off for it); returns the ran record"""
    ran = (C.c_int * 4)()
    prev = lib.ttx_kernel_variant(E.TTX_GEMM_P8, p8) if p8 is not None else None
    try:
        E.check(lib.tt_op_gemm_ex(dt, epi, C.byref(d), ran, None))
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            lib.ttx_kernel_variant(E.TTX_GEMM_P8, prev)
    return tuple(ran)


def expect(form, ran, tile, variant, p8=0, conv3s=0):
    got = f"{E.GEMM_TILES.get(ran[0], ran[0])} {E.GEMM_VARIANTS.get(ran[1], ran[1])} p8={ran[2]} conv3s={ran[3]}"
    want = f"{tile} {variant} p8={p8} conv3s={conv3s}"
    assert got == want, f"{form}: launched [{got}], expected [{want}]"
    return got


def check(form, ran_s, got, ref, out, op, tile=None):
    w = R.assert_within_bound(f"{form} [{ran_s}]", got, ref, out, op, tile=DIMS.get(tile))
    key = form.split(" M=")[0]
    WORST[key] = max(WORST.get(key, 0.0), w)
    return w


def stat_rows(lib, dt, d):
    return lib.tt_op_gemm_stat_rows(dt, C.byref(d))


def ctypes_ints(v):
    return (C.c_int * len(v))(*v)


def matrix(table, f32_ok):
    """(name, dt, tdt, case) for bf16 and fp16, and for the fp32 verification GEMM where f32_ok(case): it has one 64 x 64 kernel per
    epilogue and no shared-halo kernel, so the small shapes of a table cover it"""
    return [pytest.param(*d, c, id=f"{c[0]}-{d[0]}") for d in DT16 + [F32] for c in table if d[0] != "f32" or f32_ok(c)]


@pytest.mark.parametrize("name,dt,tdt", DT16)
@pytest.mark.parametrize("M", [7, 40])
def test_skinny_tiles(lib, name, dt, tdt, M):
    """decode-batch GEMMs (M <= 64, N >= 1024): 32 x 16 / 64 x 16 tiles, every variant they instantiate"""
    N, K = 1024, 1024
    tile = "32x16" if M <= 32 else "64x16"
    A, W, bias, res = operands(M, M, N, K, tdt)
    X = R.gemm_operand(A, K)
    o32 = torch.zeros(M, N, device="cuda")
    ot = torch.zeros(M, N, device="cuda", dtype=tdt)
    s = expect("gen", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, act=R.ACT_GELU_ERF, out_f32=o32)), tile, "V_GEN")
    check(f"skinny V_GEN gelu_erf {name} M={M}", s, o32, R.std_reference(X, W, bias, R.ACT_GELU_ERF)[0], "f32", name, tile)
    s = expect("none", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, res=res, out_f32=o32)), tile, "V_NONE")
    check(f"skinny V_NONE bias+skip {name} M={M}", s, o32, R.std_reference(X, W, bias, res=res)[0], "f32", name, tile)
    slabs = torch.zeros(2, M, N, device="cuda")
    s = expect("slab", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, splitk=2, out_f32=slabs)), tile, "V_SLAB")
    for z in range(2):
        check(f"skinny V_SLAB {name} M={M} slab {z}", s, slabs[z], R.std_reference(X[:, z * 512:(z + 1) * 512], W[:, z * 512:(z + 1) * 512])[0], "f32", name, tile)
    s = expect("gelu_t", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, act=R.ACT_GELU_TANH, out_t=ot)), tile, "V_GELU_T")
    check(f"skinny V_GELU_T {name} M={M}", s, ot, R.std_reference(X, W, bias, R.ACT_GELU_TANH)[0], name, name, tile)
    s = expect("bias_t", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, out_t=ot)), tile, "V_BIAS_T")
    check(f"skinny V_BIAS_T {name} M={M}", s, ot, R.std_reference(X, W, bias)[0], name, name, tile)


# (form, M, N, K, outputs, expected tile / variant / eight-phase for the 16-bit kernels); every tile's plain forms, ragged M and N
PLAIN = [("64x64 unaligned N gelu+skip+f32+T", 300, 1001, 512, "gelu_all", "64x64", "V_GEN", 0),
         ("64x64 one denoiser pass bias+skip", 1500, 1024, 256, "res", "64x64", "V_NONE", 0),
         ("128x64 ragged M bias+skip", 3000, 256, 512, "res", "128x64", "V_NONE", 0),
         ("128x128 bias->T", 2048, 2048, 256, "bias_t", "128x128", "V_BIAS_T", 0),
         ("256x256 16-wave K=192 bias+skip", 22000, 768, 192, "res", "256x256", "V_NONE", 0),
         ("256x256 eight-phase bias->T", 22000, 768, 256, "bias_t", "256x256", "V_BIAS_T", 1)]


@pytest.mark.parametrize("name,dt,tdt,case", matrix(PLAIN, lambda c: c[1] <= 3000))
def test_plain_forms(lib, name, dt, tdt, case):
    form, M, N, K, outs, tile, variant, p8 = case
    if name == "f32":
        tile, variant, p8 = "64x64", "V_GEN", 0
    A, W, bias, res = operands(M + N, M, N, K, tdt)
    X = R.gemm_operand(A, K)
    o32 = torch.zeros(M, N, device="cuda")
    ot = torch.zeros(M, N, device="cuda", dtype=tdt)
    kw = dict(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias)
    if outs == "gelu_all":
        kw.update(act=R.ACT_GELU_TANH, res=res, out_f32=o32, out_t=ot)
        ref = R.std_reference(X, W, bias, R.ACT_GELU_TANH, res=res)[0]
    elif outs == "res":
        kw.update(res=res, out_f32=o32)
        ref = R.std_reference(X, W, bias, res=res)[0]
    else:
        kw.update(out_t=ot)
        ref = R.std_reference(X, W, bias)[0]
    s = expect(form, launch(lib, dt, 0, desc(**kw)), tile, variant, p8)
    if outs != "bias_t":
        check(f"{form} {name} M={M}", s, o32, ref, "f32", name, tile)
    if outs != "res":
        check(f"{form} (T) {name} M={M}", s, ot, ref, name, name, tile)
    if p8:  # the 16-wave kernel on the same launch: the same bits
        ot2 = torch.zeros_like(ot)
        kw.update(out_t=ot2)
        expect(form + " (16-wave)", launch(lib, dt, 0, desc(**kw), p8=0), tile, variant, 0)
        assert torch.equal(ot, ot2), f"{form}: eight-phase and 16-wave kernels differ"


def run_stats(lib, name, dt, form, kw, M, N, seq, tile, variant, p8=0, conv3s=0, rows=None, vperiod=0, vlen=None, force_p8=None):
    """a statistics GEMM: f32 output + partials; partials checked against the kernel's own output, one sentinel tile past the end untouched"""
    d = desc(**kw)
    rows = rows or stat_rows(lib, dt, desc(**kw, out_f32=1, gn_part=1, gn_seq=seq))
    nt = (M + rows - 1) // rows
    part = torch.full((nt + 1, 2, N // 16, 2), SENTINEL, device="cuda")
    o32 = torch.zeros(M, N, device="cuda")
    d = desc(**kw, out_f32=o32, gn_part=part, gn_seq=seq, gn_vperiod=vperiod, gn_vlen=vlen or [])
    s = expect(form, launch(lib, dt, 0, d, p8=force_p8), tile, variant, p8, conv3s)
    w = R.assert_partials(f"{form} {name} [{s}]", part[:nt], o32, rows, seq, vperiod, vlen)
    WORST[form.split(" M=")[0] + " (statistics)"] = max(WORST.get(form.split(" M=")[0] + " (statistics)", 0.0), w)
    assert (part[nt] == SENTINEL).all(), f"{form}: statistics written past the last row tile"
    return s, o32, part, rows


# (form, M, N, K, seq, skip, tile, variant, eight-phase, statistics rows)
STATS = [("128x64 statistics", 600, 1024, 256, 300, False, "128x64", "V_ST_F32", 0, 32),
         ("128x128 statistics + skip", 4000, 1024, 256, 1000, True, "128x128", "V_ST_RES", 0, 64),
         ("256x256 eight-phase statistics", 22000, 768, 256, 1000, False, "256x256", "V_ST_F32", 1, 64),
         ("256x256 eight-phase statistics + skip", 22000, 768, 256, 1000, True, "256x256", "V_ST_RES", 1, 64)]


@pytest.mark.parametrize("name,dt,tdt,case", matrix(STATS, lambda c: c[1] <= 4000))
def test_statistics_forms(lib, name, dt, tdt, case):
    """GroupNorm statistics epilogues: rows of sequences that straddle the row tiles (seq not a multiple of 32 / 64), ragged last tile"""
    form, M, N, K, seq, skip, tile, variant, p8, rows = case
    if name == "f32":
        tile, variant, p8, rows = "64x64", "V_GEN", 0, 32
    A, W, bias, res = operands(M + 7, M, N, K, tdt)
    kw = dict(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, res=res if skip else None)
    assert stat_rows(lib, dt, desc(**kw, gn_part=1, out_f32=1, gn_seq=seq)) == rows
    s, o32, part, _ = run_stats(lib, name, dt, form, kw, M, N, seq, tile, variant, p8, rows=rows)
    check(f"{form} {name} M={M}", s, o32, R.std_reference(R.gemm_operand(A, K), W, bias, res=res if skip else None)[0], "f32", name, tile)
    if p8:  # the 16-wave kernel on the same launch: the same bits, statistics included
        s2, o2, part2, _ = run_stats(lib, name, dt, form + " (16-wave)", kw, M, N, seq, tile, variant, 0, rows=rows, force_p8=0)
        assert torch.equal(o32, o2) and torch.equal(part, part2), f"{form}: eight-phase and 16-wave kernels differ"


# (form, cin, taps, dilation, N, outputs, tile, variant, conv3s): B * S = 2 * 870 rows; zero padding at every sequence edge
CONV = [("conv3s statistics", 1024, 3, 1, 1024, "stats", "128x64", "V_ST_F32", 1),
        ("conv3s statistics + skip", 1024, 3, 1, 1024, "stats_res", "128x64", "V_ST_RES", 1),
        ("conv taps 3 bias->T", 256, 3, 1, 512, "bias_t", "64x64", "V_BIAS_T", 0),
        ("conv taps 5 dilation 2 statistics", 256, 5, 2, 1024, "stats", "128x64", "V_ST_F32", 0),
        ("conv taps 3 cin 128 statistics + skip", 128, 3, 1, 1024, "stats_res", "128x64", "V_ST_RES", 0)]


@pytest.mark.parametrize("name,dt,tdt,case", matrix(CONV, lambda c: not c[8]))
def test_conv_forms(lib, name, dt, tdt, case):
    form, cin, taps, dil, N, outs, tile, variant, conv3s = case
    if name == "f32":
        tile, variant = "64x64", "V_GEN"
    B, S = 2, 870
    M, K = B * S, taps * cin
    A, W, bias, res = operands(cin + taps, M, N, K, tdt)
    A = A[:, :cin].contiguous()
    X = R.conv_operand(A, M, cin, taps, dil, S)
    skip = res if outs == "stats_res" else None
    kw = dict(A=A, lda=cin, W=W, ldw=K, M=M, N=N, K=K, taps=taps, dilation=dil, seq_len=S, bias=bias, res=skip)
    ref = R.std_reference(X, W, bias, res=skip)[0]
    if outs == "bias_t":
        ot = torch.zeros(M, N, device="cuda", dtype=tdt)
        s = expect(form, launch(lib, dt, 0, desc(**kw, out_t=ot)), tile, variant)
        check(f"{form} {name}", s, ot, ref, name, name, tile)
        return
    s, o32, _, _ = run_stats(lib, name, dt, form, kw, M, N, S, tile, variant, 0, conv3s)
    check(f"{form} {name}", s, o32, ref, "f32", name, tile)


# (form, M, N, K, splitk, tile, variant): fewer k-tiles per K range than ring stages - the clamped re-request goes into a dead ring slot
RING_TAIL = [("ring tail 64x64 K=64 bias+f32", 100, 128, 64, 1, "64x64", "V_NONE"),
             ("ring tail 32x16 K=64 bias+f32", 7, 1024, 64, 1, "32x16", "V_NONE"),
             ("ring tail 32x16 K=128 slabs", 7, 1024, 128, 2, "32x16", "V_SLAB"),
             ("ring tail 64x16 K=128 slabs", 40, 1024, 128, 2, "64x16", "V_SLAB")]


@pytest.mark.parametrize("name,dt,tdt", DT16)
@pytest.mark.parametrize("case", RING_TAIL, ids=[c[0].replace(" ", "_") for c in RING_TAIL])
def test_ring_tail_shorter_than_the_ring(lib, name, dt, tdt, case):
    """one k-tile per K range on the 4- and 8-stage rings: every prologue fill but the first and every refill re-requests that tile"""
    form, M, N, K, splitk, tile, variant = case
    A, W, bias, _ = operands(M + K, M, N, K, tdt)
    X = R.gemm_operand(A, K)
    if splitk == 1:
        o32 = torch.full((M + 1, N), SENTINEL, device="cuda")
        s = expect(form, launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, out_f32=o32)), tile, variant)
        check(f"{form} {name} M={M}", s, o32[:M], R.std_reference(X, W, bias)[0], "f32", name, tile)
        assert (o32[M] == SENTINEL).all(), f"{form}: written past the last row"
        return
    slabs = torch.zeros(splitk, M, N, device="cuda")
    s = expect(form, launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, splitk=splitk, out_f32=slabs)), tile, variant)
    for z in range(splitk):
        check(f"{form} {name} M={M} slab {z}", s, slabs[z], R.std_reference(X[:, z * 64:(z + 1) * 64], W[:, z * 64:(z + 1) * 64])[0], "f32", name, tile)


@pytest.mark.parametrize("name,dt,tdt", DT16)
def test_ring_tail_statistics(lib, name, dt, tdt):
    """K = 64 on the 128 x 64 tile's 4-stage ring through the statistics form, two sequences of 150 rows"""
    M, N, K, seq = 300, 64, 64, 150
    A, W, bias, _ = operands(M + K, M, N, K, tdt)
    kw = dict(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias)
    s, o32, _, _ = run_stats(lib, name, dt, "ring tail 128x64 K=64 statistics", kw, M, N, seq, "128x64", "V_ST_F32")
    check(f"ring tail 128x64 K=64 statistics {name} M={M}", s, o32, R.std_reference(R.gemm_operand(A, K), W, bias)[0], "f32", name, "128x64")


@pytest.mark.parametrize("name,dt,tdt", DT16)
def test_conv_split_k_slab_starts_inside_a_tap(lib, name, dt, tdt):
    """taps 3, cin 128 (6 k-tiles), splitk 4: the slabs start at k-tiles 0, 2, 4, 5, so slab 3 starts at tap 2, slice 1 - the tap cursor's
    one real division.  Every slab against the matching columns of the virtual conv operand."""
    B, S, cin, taps, N, splitk = 2, 70, 128, 3, 128, 4
    M, K = B * S, taps * cin
    A, W, _, _ = operands(cin + splitk, M, N, K, tdt)
    A = A[:, :cin].contiguous()
    X = R.conv_operand(A, M, cin, taps, 1, S)
    slabs = torch.zeros(splitk, M, N, device="cuda")
    d = desc(A=A, lda=cin, W=W, ldw=K, M=M, N=N, K=K, taps=taps, dilation=1, seq_len=S, splitk=splitk, out_f32=slabs)
    s = expect("conv split-K", launch(lib, dt, 0, d), "64x64", "V_NONE")
    for z, (t0, t1) in enumerate(((0, 2), (2, 4), (4, 5), (5, 6))):
        check(f"conv taps 3 cin 128 splitk 4 {name} slab {z}", s, slabs[z], R.std_reference(X[:, t0 * 64:t1 * 64], W[:, t0 * 64:t1 * 64])[0], "f32", name, "64x64")


@pytest.mark.parametrize("name,dt,tdt", DT16)
def test_conv_unaligned(lib, name, dt, tdt):
    """taps 3, cin 64, N = 130 (generic kernel, element-wise epilogue): bias, skip, f32 and T outputs, one sentinel row past each"""
    B, S, cin, taps, N = 2, 70, 64, 3, 130
    M, K = B * S, taps * cin
    A, W, bias, res = operands(cin + N, M, N, K, tdt)
    A = A[:, :cin].contiguous()
    X = R.conv_operand(A, M, cin, taps, 1, S)
    o32 = torch.full((M + 1, N), SENTINEL, device="cuda")
    ot = torch.full((M + 1, N), SENTINEL, device="cuda", dtype=tdt)
    d = desc(A=A, lda=cin, W=W, ldw=K, M=M, N=N, K=K, taps=taps, dilation=1, seq_len=S, bias=bias, res=res, out_f32=o32, out_t=ot)
    s = expect("conv unaligned", launch(lib, dt, 0, d), "64x64", "V_GEN")
    ref = R.std_reference(X, W, bias, res=res)[0]
    check(f"conv taps 3 N=130 f32 {name}", s, o32[:M], ref, "f32", name, "64x64")
    check(f"conv taps 3 N=130 (T) {name}", s, ot[:M], ref, name, name, "64x64")
    assert (o32[M] == SENTINEL).all() and (ot[M] == SENTINEL).all(), "unaligned conv wrote past the last row"


@pytest.mark.parametrize("name,dt,tdt", DT16)
@pytest.mark.parametrize("B,S,N,tile", [(4, 1024, 1024, "128x128"), (26, 870, 768, "256x256")])
def test_conv_on_the_two_stage_tiles(lib, name, dt, tdt, B, S, N, tile):
    """taps 3, cin 64, bias -> T on the 128 x 128 and the 16-wave 256 x 256 tile (a conv never takes the eight-phase kernel)"""
    cin, taps = 64, 3
    M, K = B * S, taps * cin
    A, W, bias, _ = operands(M + N, M, N, K, tdt)
    A = A[:, :cin].contiguous()
    X = R.conv_operand(A, M, cin, taps, 1, S)
    ot = torch.zeros(M, N, device="cuda", dtype=tdt)
    d = desc(A=A, lda=cin, W=W, ldw=K, M=M, N=N, K=K, taps=taps, dilation=1, seq_len=S, bias=bias, out_t=ot)
    s = expect(f"conv {tile}", launch(lib, dt, 0, d), tile, "V_BIAS_T")
    check(f"conv taps 3 cin 64 bias->T {tile} {name} M={M}", s, ot, R.std_reference(X, W, bias)[0], name, name, tile)


@pytest.mark.parametrize("name,dt,tdt", DT16 + [F32])
def test_second_activation_source(lib, name, dt, tdt):
    """[A | A2] without the concatenation: k_split 1024 of 2048 with statistics (slot 2 of A2), and 192 of 320 on the generic kernel (slot 0)"""
    M, N, K, ks = 600, 1024, 2048, 1024
    A, W, bias, _ = operands(11, M, N, K, tdt)
    A2 = torch.randn(3, M, K - ks, device="cuda").to(tdt)
    slot = torch.tensor([2], device="cuda", dtype=torch.int32)
    kw = dict(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, A2=A2, lda2=K - ks, k_split=ks, a2_slot=slot, a2_slot_stride=M * (K - ks))
    tile, variant = ("64x64", "V_GEN") if name == "f32" else ("128x64", "V_ST_A2")
    s, o32, _, _ = run_stats(lib, name, dt, "V_ST_A2 k_split 1024/2048 slot 2", kw, M, N, 300, tile, variant)
    check(f"V_ST_A2 k_split 1024/2048 slot 2 {name}", s, o32, R.std_reference(R.gemm_operand(A, K, A2[2], ks), W, bias)[0], "f32", name, tile)
    M, N, K, ks = 300, 512, 320, 192
    A, W, bias, _ = operands(13, M, N, K, tdt)
    A2 = torch.randn(1, M, K - ks, device="cuda").to(tdt)
    slot = torch.tensor([0], device="cuda", dtype=torch.int32)
    o32 = torch.zeros(M, N, device="cuda")
    d = desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, A2=A2, lda2=K - ks, k_split=ks, a2_slot=slot, a2_slot_stride=M * (K - ks), out_f32=o32)
    s = expect("V_GEN + A2", launch(lib, dt, 0, d), "64x64", "V_GEN")
    check(f"V_GEN + A2 k_split 192/320 slot 0 {name}", s, o32, R.std_reference(R.gemm_operand(A, K, A2[0], ks), W, bias)[0], "f32", name, "64x64")


@pytest.mark.parametrize("name,dt,tdt", DT16)
@pytest.mark.parametrize("M,K,tile", [(1024, 1024, "64x64"), (4096, 4096, "128x128")])
def test_serial_split_k(lib, name, dt, tdt, M, K, tile):
    """serial split-K in place on the skip (the GPT-2 projections of >= 1024 sequences, serial_k 4): bit for bit the split-K slabs of
    256-row chunks folded on the host as ((skip + bias) + P0) + P1 + ..."""
    N, sk = 1024, 4
    A, W, bias, res = operands(M + K, M, N, K, tdt)
    x = res.clone()
    s = expect("serial", launch(lib, dt, 0, desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, serial_k=sk, bias=bias, res=x, out_f32=x)), tile, "V_SERIAL")
    fold = res + bias
    slabs = torch.zeros(sk, 256, N, device="cuda")
    for r0 in range(0, M, 256):
        expect("slabs", launch(lib, dt, 0, desc(A=A[r0:r0 + 256], lda=K, W=W, ldw=K, M=256, N=N, K=K, splitk=sk, out_f32=slabs)), "64x64", "V_SLAB")
        for z in range(sk):
            fold[r0:r0 + 256] += slabs[z]
    assert torch.equal(x, fold), f"serial split-K differs from the folded slabs: {(x - fold).abs().max().item()}"
    check(f"V_SERIAL serial_k {sk} {name} M={M} K={K}", s, x, R.std_reference(R.gemm_operand(A, K), W, bias, res=res)[0], "f32", name, tile)


@pytest.mark.parametrize("name,dt,tdt", DT16 + [F32])
def test_act_t_leaky_relu(lib, name, dt, tdt):
    """bias + skip + both outputs, LeakyReLU on the T copy only: T = lrelu(f32 output) in the operand type"""
    M, N, K = 300, 512, 256
    A, W, bias, res = operands(21, M, N, K, tdt)
    o32 = torch.zeros(M, N, device="cuda")
    ot = torch.zeros(M, N, device="cuda", dtype=tdt)
    d = desc(A=A, lda=K, W=W, ldw=K, M=M, N=N, K=K, bias=bias, res=res, out_f32=o32, out_t=ot, act_t=R.ACT_LRELU, slope_t=0.1)
    s = expect("act_t", launch(lib, dt, 0, d), "64x64", "V_GEN" if name == "f32" else "V_NONE")
    f32, t = R.std_reference(R.gemm_operand(A, K), W, bias, res=res, act_t=R.ACT_LRELU, slope_t=0.1)
    check(f"act_t lrelu f32 out {name}", s, o32, f32, "f32", name, "64x64")
    check(f"act_t lrelu T out {name}", s, ot, t, name, name, "64x64")
    assert torch.equal(ot, torch.where(o32 > 0, o32, o32 * 0.1).to(tdt)), "T output is not lrelu of the f32 output"


@pytest.mark.parametrize("name,dt,tdt", DT16)
def test_padded_statistics_alone_and_batched_and_consumed(lib, name, dt, tdt):
    """gn_vperiod (two utterances of 870 / 801 valid rows in 870-row slots): batched (64 x 64 tile) the partials leave the padded rows out;
    sample 0 alone (128 x 64 tile) gives the same bits for its rows, its partials and its normalised output; the consumer entry on the
    kernel's own statistics equals an fp64 GroupNorm of the kernel's own output and writes zeros past vlen"""
    B, S, C, K, vlen = 2, 870, 1024, 256, [870, 801]
    A, W, bias, _ = operands(31, B * S, C, K, tdt)
    kw = dict(A=A, lda=K, W=W, ldw=K, M=B * S, N=C, K=K, bias=bias)
    s, y, part, rows = run_stats(lib, name, dt, "statistics gn_vperiod batched", kw, B * S, C, S, "64x64", "V_ST_F32", vperiod=2, vlen=vlen)
    kw1 = dict(kw, M=S)
    s1, y1, part1, rows1 = run_stats(lib, name, dt, "statistics alone", kw1, S, C, S, "128x64", "V_ST_F32", vperiod=1, vlen=[S])
    assert rows == rows1 == 32
    assert torch.equal(y[:S], y1), "sample 0 differs alone vs batched"
    nt0 = (S - 1) // rows + 1
    assert torch.equal(part[:nt0, 0], part1[:nt0, 0]), "sample 0's statistics differ alone vs batched"
    g = torch.Generator(device="cuda").manual_seed(32)
    gamma, beta = torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    ws = torch.zeros(lib.tt_op_groupnorm_workspace(B, S) // 4 + 64, device="cuda")
    out = torch.full((B * S, C), SENTINEL, device="cuda")
    E.check(lib.tt_op_groupnorm_part(dt, E.ptr(y), B, S, C, E.ptr(gamma), E.ptr(beta), None, 0, E.ptr(part), rows, 2, ctypes_ints(vlen), None,
                                     E.ptr(out), E.ptr(ws), None))
    out1 = torch.full((S, C), SENTINEL, device="cuda")
    E.check(lib.tt_op_groupnorm_part(dt, E.ptr(y1), 1, S, C, E.ptr(gamma), E.ptr(beta), None, 0, E.ptr(part1), rows, 1, ctypes_ints([S]), None,
                                     E.ptr(out1), E.ptr(ws), None))
    torch.cuda.synchronize()
    assert torch.equal(out[:S], out1), "sample 0's GroupNorm differs alone vs batched"
    for b in range(B):
        n = vlen[b]
        yb = y[b * S:b * S + n].double()
        want = F.group_norm(yb.t().unsqueeze(0), 32, gamma.double(), beta.double(), 1e-5)[0].t()
        err = (out[b * S:b * S + n].double() - want).abs()
        worst = float((err / (2.0 ** -18 * (want.abs() + 1.0))).max())
        print(f"[bound] consumer GroupNorm on the epilogue's statistics {name} sample {b} ({n} valid rows): worst |err|/bound={worst:.3f}")
        assert worst <= 1.0, f"GroupNorm from the GEMM's statistics is off for sample {b}"
        assert (out[b * S + n:(b + 1) * S] == 0).all(), f"rows past vlen of sample {b} are not zero"


# (tile, M, seq_len, dmodel, eight-phase): the head-layout scatter of the prefill / CLVP / denoiser / aligner QKV projections
HEADS = [("64x64", 140, 70, 256, 0), ("128x64", 2580, 129, 256, 0), ("128x128", 3480, 870, 512, 0), ("256x256", 22620, 870, 256, 1)]


@pytest.mark.parametrize("name,dt,tdt,case", matrix(HEADS, lambda c: c[1] <= 140))
def test_qkv_heads(lib, name, dt, tdt, case):
    """q / k / vt (denoiser, CLVP) and q / k / v / vt (GPT-2 prefill into the prefix cache) with q_scale 1/8; every cell outside the
    problem - the vt columns seq_len .. seq_pad and one head slab past each buffer - keeps its sentinel bit for bit"""
    tile, M, S, D, p8 = case
    H, B, K, pad = D // 64, M // S, 256, (S + 31) // 32 * 32
    A, W, bias, _ = operands(M + D, M, 3 * D, K, tdt)
    ref = R.qkv_heads_reference(R.std_reference(R.gemm_operand(A, K), W, bias)[0], B, S, H, 0.125)
    for with_v in (False, True):
        bufs = {p: torch.full((B * H + 1, S, 64), SENTINEL, device="cuda", dtype=tdt) for p in ("q", "k", "v")}
        bufs["vt"] = torch.full((B * H + 1, 64, pad), SENTINEL, device="cuda", dtype=tdt)
        if not with_v:
            bufs["v"] = None
        d = desc(A=A, lda=K, W=W, ldw=K, M=M, N=3 * D, K=K, seq_len=S, bias=bias, dmodel=D, heads=H, seq_pad=pad, q_scale=0.125, **bufs)
        form = f"EPI_QKV_HEADS {'q/k/v/vt' if with_v else 'q/k/vt'} {tile}"
        s = expect(form, launch(lib, dt, 1, d), "64x64" if name == "f32" else tile, "-", 0 if name == "f32" else p8)
        for p in ("q", "k", "v", "vt"):
            if bufs[p] is None:
                continue
            got = bufs[p][:B * H, :, :S] if p == "vt" else bufs[p][:B * H]
            check(f"{form} {p} {name} M={M} S={S}", s, got, ref[p], name, name)
            assert (bufs[p][B * H] == SENTINEL).all(), f"{form}: {p} written past the last head"
        assert (bufs["vt"][:, :, S:] == SENTINEL).all(), f"{form}: vt columns seq_len .. seq_pad written"
        if p8 and name != "f32":
            again = {p: (None if t is None else torch.full_like(t, SENTINEL)) for p, t in bufs.items()}
            d = desc(A=A, lda=K, W=W, ldw=K, M=M, N=3 * D, K=K, seq_len=S, bias=bias, dmodel=D, heads=H, seq_pad=pad, q_scale=0.125, **again)
            expect(form + " (16-wave)", launch(lib, dt, 1, d, p8=0), tile, "-", 0)
            for p in bufs:
                assert bufs[p] is None or torch.equal(bufs[p], again[p]), f"{form}: eight-phase and 16-wave kernels differ in {p}"


@pytest.mark.parametrize("name,dt,tdt,M,tile", [pytest.param(*d, M, t, id=f"M{M}-{d[0]}") for d in DT16 + [F32]
                                                for M, t in ((7, "32x16"), (40, "64x16"), (256, "64x64"), (2048, "128x128")) if d[0] != "f32" or M <= 40])
def test_qkv_decode(lib, name, dt, tdt, M, tile):
    """the decode step's QKV scatter at *step in 0, 63, 64, tmax - 1: only that slot of kc [b][h][8][tmax][8] / vc [b][h][tmax][64] changes;
    the skinny tiles give the bits of the 64 x 64 tile"""
    if name == "f32":
        tile = "64x64"
    D, H, K, tmax = 1024, 16, 1024, 72
    A, W, bias, _ = operands(M + 5, M, 3 * D, K, tdt)
    ref = R.qkv_decode_reference(R.std_reference(R.gemm_operand(A, K), W, bias)[0], H, 0.125)
    for t in (0, 63, 64, tmax - 1):
        step = torch.tensor([t], device="cuda", dtype=torch.int32)
        outs = []
        for skinny in ((1, 0) if tile in ("32x16", "64x16") else (1,)):
            qbuf = torch.full((M + 1, D), SENTINEL, device="cuda", dtype=tdt)
            kc = torch.full((M, H, 8, tmax, 8), SENTINEL, device="cuda", dtype=tdt)
            vc = torch.full((M, H, tmax, 64), SENTINEL, device="cuda", dtype=tdt)
            d = desc(A=A, lda=K, W=W, ldw=K, M=M, N=3 * D, K=K, bias=bias, dmodel=D, heads=H, q_scale=0.125, step=step, qbuf=qbuf, kc=kc, vc=vc, tmax=tmax)
            prev = lib.ttx_kernel_variant(E.TTX_GEMM_SKINNY, skinny)
            try:
                s = expect(f"EPI_QKV_DECODE M={M}", launch(lib, dt, 2, d), tile if skinny else "64x64", "-")
            finally:
                lib.ttx_kernel_variant(E.TTX_GEMM_SKINNY, prev)
            outs.append((qbuf, kc, vc))
            if skinny:
                check(f"EPI_QKV_DECODE {tile} qbuf {name} M={M} step={t}", s, qbuf[:M], ref["qbuf"], name, name)
                check(f"EPI_QKV_DECODE {tile} k slot {name} M={M} step={t}", s, kc[:, :, :, t, :], ref["kslot"], name, name, None)
                check(f"EPI_QKV_DECODE {tile} v slot {name} M={M} step={t}", s, vc[:, :, t, :], ref["vslot"], name, name, None)
                kc2, vc2 = kc.clone(), vc.clone()
                kc2[:, :, :, t, :] = SENTINEL
                vc2[:, :, t, :] = SENTINEL
                assert (kc2 == SENTINEL).all() and (vc2 == SENTINEL).all() and (qbuf[M] == SENTINEL).all(), f"M={M} step={t}: cells outside slot {t} changed"
        if len(outs) == 2:
            assert all(torch.equal(a, b) for a, b in zip(*outs)), f"M={M} step={t}: skinny tile differs from the 64 x 64 tile"


GEGLU = [("64x64", 300, 2048, 512), ("128x128", 2048, 2048, 256), ("256x256", 22000, 768, 256)]


@pytest.mark.parametrize("name,dt,tdt,case", matrix(GEGLU, lambda c: c[1] <= 300))
def test_geglu(lib, name, dt, tdt, case):
    """CLVP's GEGLU feed-forward on pack.geglu_interleave weights: out = (value + b) * gelu_erf(gate + b), N / 2 columns (the 256 x 256 tile:
    the 16-wave kernel only)"""
    tile, M, N, K = case
    A, W, bias, _ = operands(M + N + 1, M, N, K, tdt)
    idx = pack.geglu_interleave(N // 2).cuda()
    Wi, bi = W[idx].contiguous(), bias[idx].contiguous()
    out = torch.full((M + 1, N // 2), SENTINEL, device="cuda", dtype=tdt)
    d = desc(A=A, lda=K, W=Wi, ldw=K, M=M, N=N, K=K, bias=bi, out_t=out, ldot=N // 2)
    s = expect("EPI_GEGLU", launch(lib, dt, 3, d), "64x64" if name == "f32" else tile, "-")
    check(f"EPI_GEGLU {tile} {name} M={M}", s, out[:M], R.geglu_reference(R.gemm_operand(A, K), Wi, bi), name, name, tile)
    assert (out[M] == SENTINEL).all(), "GEGLU wrote past the last row"
