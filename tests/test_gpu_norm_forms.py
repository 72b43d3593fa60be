"""-m gpu: every row-norm and GroupNorm32 kernel form of csrc/norm.hip one launch at a time through tt_op_rownorm_ex / tt_op_groupnorm_ex,
against the fp64 references of tests/norm_reference.py with element-wise bounds.  Every case asserts the host-side record of what launched
(row norm: generic / narrow / wave kernel and the narrow kernel's template arguments; GroupNorm: statistics pass, apply kernel, rows per
block), so a change of the dispatch cannot silently stop covering a kernel.  Every output buffer is allocated with eight pad columns and a
pad row (ld = D + 8) and pre-filled with a sentinel that must survive outside the written region; the written-back residual rows are
compared bit for bit with the fp32 chain.  Each case runs for bf16, fp16 and f32 outputs and prints its worst |err| / bound; the last line
of a module run lists the worst ratio per family (the figures in the docstring of tests/norm_reference.py).
"""
import ctypes as C
import functools

import pytest
import torch

from tortoise_tts_amd import engine as E
from tests import gemm_reference as R
from tests import norm_reference as N

pytestmark = pytest.mark.gpu
DT = [("bf16", E.TT_BF16, torch.bfloat16), ("f16", E.TT_F16, torch.float16), ("f32", E.TT_F32, torch.float32)]
SENTINEL = 8192.0  # exact in bf16 and fp16
PAD = 8
WORST = {}
GENERIC, NARROW, WAVE = 0, 1, 2
LN, RMS, NONE = N.NORM_LAYER, N.NORM_RMS, N.NORM_NONE


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield E.init()
    print("[bound] worst |err|/bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def note(family, w):
    WORST[family] = max(WORST.get(family, 0.0), w)


def padded(t, pad=PAD, dtype=torch.float32):
    """t [..., R, D] inside a sentinel-filled cuda buffer [..., R + 1, D + pad]"""
    buf = torch.full((*t.shape[:-2], t.shape[-2] + 1, t.shape[-1] + pad), SENTINEL, dtype=dtype)
    buf[..., :t.shape[-2], :t.shape[-1]] = t
    return buf.cuda()


def untouched_outside(buf, rows, cols):
    b = buf.clone()
    b[..., :rows, :cols] = SENTINEL
    return bool((b == SENTINEL).all())


def fill(d, **kw):
    for k, v in kw.items():
        setattr(d, k, E.ptr(v) if isinstance(v, torch.Tensor) else v)
    return d


def rows_of(ref, rows):
    return N.Ref(ref.value[rows], ref.err[rows])


# ------------------------------------------------------------------------------------------------- row norm
def run_row(lib, name, dt, tdt, form, d, D, expect, nslab=0, bias=False, mode=LN, write_x=False, x_in=False, g2=False, act=R.ACT_NONE, outs="both",
            eps1=1e-5, eps2=1e-6, slot=None, row_blocks=0, guard=False, check_rows=None):
    """one tt_op_rownorm_ex launch on the inputs d (norm_reference.rownorm_inputs); asserts `ran`, the written-back rows, every bound and
    every sentinel; returns (out_t rows, out_f32 rows, guard count)"""
    M = d["x"].shape[0]
    xb = padded(d["x"])
    x0 = xb.clone()
    xin = padded(d["x_in"], pad=12) if x_in else None
    slabs = padded(d["slabs"][:nslab]) if nslab else None
    dev = {k: d[k].cuda() for k in ("bias", "g1", "b1", "g2", "b2")}
    out_t = torch.full((M + 1, D + PAD), SENTINEL, device="cuda", dtype=tdt) if outs in ("t", "both") else None
    stride = M * D + 64
    if outs not in ("f32", "both"):
        o32 = None
    elif slot:
        o32 = torch.full((5, stride), SENTINEL, device="cuda")
    else:
        o32 = torch.full((M + 1, D + PAD), SENTINEL, device="cuda")
    gcount = torch.zeros(1, device="cuda", dtype=torch.int32) if guard else None
    desc = fill(E.RowNormDesc(), x=xb, ldx=D + PAD, x_in=xin, ldxin=D + 12, M=M, D=D, add_bias=dev["bias"] if bias else None, add_slabs=slabs, nslab=nslab,
                slab_stride=(M + 1) * (D + PAD), ldslab=D + PAD, write_x=int(write_x), mode=mode, g1=dev["g1"], b1=None if mode == RMS else dev["b1"], eps1=eps1,
                g2=dev["g2"] if g2 else None, b2=dev["b2"] if g2 else None, eps2=eps2, out_t=out_t, ldot=D + PAD, out_f32=o32, ldo32=D if slot else D + PAD,
                row_blocks=row_blocks, guard=gcount, act=act)
    slots = None
    if slot == "step":  # device int 2, base 1: block 3
        slots = torch.tensor([2], device="cuda", dtype=torch.int32)
        fill(desc, f32_slot=slots, f32_slot_base=1, f32_slot_stride=stride)
    elif slot == "rows":
        slots = torch.tensor([0, -1, 3, 1, -1], device="cuda", dtype=torch.int32)
        assert M == 5
        fill(desc, f32_row_slot=slots, f32_slot_base=0, f32_slot_stride=stride)
    ran = (C.c_int * 4)()
    E.check(lib.tt_op_rownorm_ex(dt, C.byref(desc), ran, None))
    torch.cuda.synchronize()
    ran = tuple(ran)
    what = f"{form} {name} M={M} D={D} [{E.ROWNORM_KERNELS.get(ran[0], ran[0])} nslab={ran[1]} bias={ran[2]} rms={ran[3]}]"
    assert ran == tuple(expect), f"{what}: expected {tuple(expect)}"
    t = N.updated_row(d["x"], d["x_in"] if x_in else None, d["bias"] if bias else None, d["slabs"][:nslab])
    sel = slice(None) if check_rows is None else check_rows
    if write_x:
        assert torch.equal(xb[:M, :D].cpu()[sel], t[sel]), f"{what}: written-back x differs from the fp32 chain"
        assert untouched_outside(xb, M, D), f"{what}: x written outside the rows"
    else:
        assert torch.equal(xb.view(torch.int32), x0.view(torch.int32)), f"{what}: x changed without write_x"
    if mode == NONE:
        assert (out_t is None or bool((out_t == SENTINEL).all())) and (o32 is None or bool((o32 == SENTINEL).all())), f"{what}: NORM_NONE wrote an output"
        return None, None, 0
    ref = N.rownorm_reference(t, mode, d["g1"], d["b1"], eps1, d["g2"] if g2 else None, d["b2"] if g2 else None, eps2, act)
    got_t = got_32 = None
    fam = E.ROWNORM_KERNELS[ran[0]]
    if out_t is not None:
        got_t = out_t[:M, :D].cpu()
        note(f"row norm T out ({fam})", N.assert_within_bound(what + " T", got_t[sel], rows_of(ref, sel), name))
        assert untouched_outside(out_t, M, D), f"{what}: out_t written outside the rows"
    if o32 is not None and not slot:
        got_32 = o32[:M, :D].cpu()
        note(f"row norm f32 out ({fam})", N.assert_within_bound(what + " f32", got_32[sel], rows_of(ref, sel), "f32"))
        assert untouched_outside(o32, M, D), f"{what}: out_f32 written outside the rows"
    elif o32 is not None:
        blocks = o32[:, :M * D].reshape(5, M, D).cpu()
        if slot == "step":
            note(f"row norm f32 out ({fam})", N.assert_within_bound(f"{what} f32 in block 3", blocks[3][sel], rows_of(ref, sel), "f32"))
            blocks[3] = SENTINEL
        else:
            for r, b in enumerate(slots.cpu().tolist()):
                if b >= 0:
                    note(f"row norm f32 out ({fam})", N.assert_within_bound(f"{what} f32 row {r} in block {b}", blocks[b, r:r + 1], rows_of(ref, slice(r, r + 1)), "f32"))
                    blocks[b, r] = SENTINEL
        assert bool((blocks == SENTINEL).all()) and bool((o32[:, M * D:] == SENTINEL).all()), f"{what}: an f32 row filed outside its block"
    return got_t, got_32, int(gcount.item()) if guard else 0


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("D", [4, 132, 1020, 1024])
def test_narrow_kernel(lib, name, dt, tdt, D):
    """M = 5, D <= 1024: every compiled slab count x bias x LayerNorm / RMSNorm; write_x, a separate x_in (ldxin != ldx) and the output set rotate"""
    i = 0
    for nslab in (0, 1, 2, 4, 8):
        d = N.rownorm_inputs(D * 16 + nslab, 5, D, nslab)
        for bias in (False, True):
            for mode in (LN, RMS):
                run_row(lib, name, dt, tdt, "narrow", d, D, (NARROW, nslab, int(bias), int(mode == RMS)), nslab=nslab, bias=bias, mode=mode, write_x=i % 5 != 4,
                        x_in=(i // 3) % 2 == 1, outs=("t", "f32", "both")[i % 3], eps1=1e-8 if mode == RMS else 1e-5)
                i += 1


@pytest.mark.parametrize("name,dt,tdt", DT)
def test_generic_kernel(lib, name, dt, tdt):
    """run-time slab counts, D > 1024, the double LayerNorm, activations, NORM_NONE, the f32 slots"""
    for nslab in (3, 5):
        d = N.rownorm_inputs(1024 * 16 + nslab, 5, 1024, nslab)
        run_row(lib, name, dt, tdt, f"generic nslab={nslab}", d, 1024, (GENERIC, -1, 1, 0), nslab=nslab, bias=True, write_x=True, x_in=nslab == 3)
        run_row(lib, name, dt, tdt, f"generic nslab={nslab} rms", d, 1024, (GENERIC, -1, 0, 1), nslab=nslab, mode=RMS, eps1=1e-8, outs="f32")
    for D in (1028, 2048, 4096):
        d = N.rownorm_inputs(D * 16 + 2, 5, D, 2)
        run_row(lib, name, dt, tdt, "generic wide", d, D, (GENERIC, -1, 1, 0), nslab=2, bias=True, write_x=True)
        run_row(lib, name, dt, tdt, "generic wide rms", d, D, (GENERIC, -1, 0, 1), mode=RMS, eps1=1e-8, x_in=True, outs="t")
    for D in (1024, 4096):
        d = N.rownorm_inputs(D * 16 + 1, 5, D, 1)
        run_row(lib, name, dt, tdt, "generic double LayerNorm", d, D, (GENERIC, -1, 1, 0), nslab=1, bias=True, write_x=True, g2=True, eps1=1e-5, eps2=1e-6)
    d = N.rownorm_inputs(512 * 16, 5, 512)
    for act in (R.ACT_GELU_ERF, R.ACT_SILU):
        run_row(lib, name, dt, tdt, f"generic act={act}", d, 512, (GENERIC, -1, 0, 0), act=act)
    for D in (1024, 2048):  # NORM_NONE: the residual update alone
        d = N.rownorm_inputs(D * 16 + 2, 5, D, 2)
        run_row(lib, name, dt, tdt, "generic NORM_NONE", d, D, (GENERIC, -1, 1, 0), nslab=2, bias=True, x_in=True, write_x=True, mode=NONE)
    d = N.rownorm_inputs(1024 * 16, 5, 1024)
    run_row(lib, name, dt, tdt, "generic f32_slot", d, 1024, (GENERIC, -1, 0, 0), slot="step")
    run_row(lib, name, dt, tdt, "generic f32_row_slot", d, 1024, (GENERIC, -1, 0, 0), slot="rows", g2=True)
    got_t, _, _ = run_row(lib, name, dt, tdt, "generic f32_row_slot (T rows)", d, 1024, (GENERIC, -1, 0, 0), slot="rows")
    assert not bool((got_t == SENTINEL).any()), "a row with a negative f32_row_slot must still write its out_t row"


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("D", [4, 132, 512, 1024])
def test_wave_kernel(lib, name, dt, tdt, D):
    """M = 1027 (three live waves in the last block): LayerNorm, RMSNorm, the double LayerNorm, an activation, two slabs + bias + write_x"""
    d = N.rownorm_inputs(D * 16 + 2, 1027, D, 2)
    run_row(lib, name, dt, tdt, "wave", d, D, (WAVE, -1, 0, 0))
    run_row(lib, name, dt, tdt, "wave rms", d, D, (WAVE, -1, 0, 1), mode=RMS, eps1=1e-8, x_in=True)
    run_row(lib, name, dt, tdt, "wave double LayerNorm", d, D, (WAVE, -1, 0, 0), g2=True, outs="f32")
    run_row(lib, name, dt, tdt, "wave act", d, D, (WAVE, -1, 0, 0), act=R.ACT_GELU_ERF, outs="t")
    run_row(lib, name, dt, tdt, "wave slabs", d, D, (WAVE, -1, 1, 0), nslab=2, bias=True, write_x=True)


@pytest.mark.parametrize("name,dt,tdt", DT)
def test_f32_slot_never_reaches_the_wave_kernel(lib, name, dt, tdt):
    """M >= 1024, D <= 1024 with an f32 slot and row_blocks = 0: the wave kernel has no slots, so the launch stays on the generic kernel"""
    d = N.rownorm_inputs(77, 1027, 1024)
    run_row(lib, name, dt, tdt, "f32_slot at M=1027", d, 1024, (GENERIC, -1, 0, 0), slot="step")


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("nslab", [0, 4])
def test_row_blocks_rows_do_not_depend_on_the_batch(lib, name, dt, tdt, nslab):
    """row_blocks = 1 at M = 1027: not the wave kernel, and rows 0, 513, 1026 carry the bits of one-row launches (the decode step's promise of
    shard-independent codes)"""
    D = 1024
    d = N.rownorm_inputs(99 + nslab, 1027, D, nslab)
    kw = dict(nslab=nslab, bias=nslab > 0, write_x=True, row_blocks=1)
    got_t, got_32, _ = run_row(lib, name, dt, tdt, "row_blocks", d, D, (NARROW, nslab, int(nslab > 0), 0), **kw)
    for r in (0, 513, 1026):
        one = {k: (v[r:r + 1] if k in ("x", "x_in") else v[:, r:r + 1] if k == "slabs" else v) for k, v in d.items()}
        t1, o1, _ = run_row(lib, name, dt, tdt, f"row_blocks row {r} alone", one, D, (NARROW, nslab, int(nslab > 0), 0), **kw)
        assert torch.equal(t1[0], got_t[r]) and torch.equal(o1[0], got_32[r]), f"row {r} differs between the 1027-row and the one-row launch"


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("D,M,kernel", [(4, 6, NARROW), (1024, 6, NARROW), (4096, 6, GENERIC), (1024, 1027, WAVE)])
def test_edge_rows(lib, name, dt, tdt, D, M, kernel):
    """a constant row, a row of 1e-4 spread around 50, RMS rows on both sides of the eps clamp, eps1 != eps2"""
    eps = 1e-5
    d = N.rownorm_inputs(D + M, M, D)
    d["x"][:6] = N.rownorm_edge_rows(D, eps)
    nk = -1 if kernel != NARROW else 0
    run_row(lib, name, dt, tdt, "edge rows", d, D, (kernel, nk, 0, 0), eps1=eps)
    run_row(lib, name, dt, tdt, "edge rows rms", d, D, (kernel, nk, 0, 1), mode=RMS, eps1=eps)
    run_row(lib, name, dt, tdt, "edge rows double LayerNorm", d, D, (GENERIC if kernel == NARROW else kernel, -1, 0, 0), g2=True, eps1=eps, eps2=1e-3)


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("form,M,D,g2,mode", [("narrow", 9, 1024, False, LN), ("generic", 9, 2048, False, LN), ("generic rms", 9, 2048, False, RMS),
                                              ("generic double LayerNorm", 9, 1024, True, LN), ("wave", 1027, 1024, False, LN),
                                              ("wave double LayerNorm", 1027, 512, True, LN)])
def test_row_guard(lib, name, dt, tdt, form, M, D, g2, mode):
    """+inf, NaN and -inf in three rows: the counter rises by exactly 3 (a second LayerNorm does not count again), a clean launch leaves it at 0,
    and every other row still meets its bound"""
    kernel = {"n": NARROW, "g": GENERIC, "w": WAVE}[form[0]]
    expect = (kernel, 0 if kernel == NARROW else -1, 0, int(mode == RMS))
    d = N.rownorm_inputs(M * 7 + D, M, D)
    kw = dict(g2=g2, mode=mode, guard=True, eps1=1e-8 if mode == RMS else 1e-5)
    assert run_row(lib, name, dt, tdt, form + " clean", d, D, expect, **kw)[2] == 0
    for r, v in ((1, float("inf")), (4, float("nan")), (M - 2, float("-inf"))):
        d["x"][r, (r * 37) % D] = v
    clean = torch.ones(M, dtype=torch.bool)
    clean[[1, 4, M - 2]] = False
    assert run_row(lib, name, dt, tdt, form + " poisoned", d, D, expect, check_rows=clean, **kw)[2] == 3


# ------------------------------------------------------------------------------------------------- GroupNorm32
@functools.lru_cache(maxsize=None)
def gn_data(C_, B, S, seed_shift=0, big_mean=False):
    d = N.groupnorm_inputs(N.gn_seed(C_, B, S) + seed_shift, B, S, C_)
    if big_mean:  # mean / spread = 100: kappa ~ 1e4
        d["x"] = torch.randn(B, S, C_, generator=torch.Generator().manual_seed(C_)) + 100.0
    return d


SS_FORMS = {None: None, "sample": (1, 2), "div2": (2, 2), "shared": (0, 0)}  # (ss_batch_div, ss_batch_stride / C)


@functools.lru_cache(maxsize=None)
def gn_ref(C_, B, S, ss, act, vlen, seed_shift=0, big_mean=False):
    """the fp64 reference of a case, computed once and shared by the three output types"""
    d = gn_data(C_, B, S, seed_shift, big_mean)
    ssb = None if ss is None else N.ss_per_sample(d["ss"], B, C_, SS_FORMS[ss][0], SS_FORMS[ss][1] * C_)
    return N.groupnorm_reference(d["x"], d["gamma"], d["beta"], 1e-5, list(vlen) if vlen else None, ssb, act)


@functools.lru_cache(maxsize=None)
def gn_part(C_, B, S, seed_shift, part_rows, vlen):
    """the statistics partials of a case in the producing GEMM epilogue's layout (tiles of part_rows rows that straddle the samples), from the host"""
    x = gn_data(C_, B, S, seed_shift)["x"].reshape(B * S, C_)
    return R.gn_partials_reference(x, part_rows, S, len(vlen) if vlen else 0, list(vlen) if vlen else None).float()


def run_gn(lib, name, dt, tdt, C_, B, S, ss=None, act=R.ACT_NONE, outs="both", vlen=None, guard=False, seed_shift=0, big_mean=False, x=None, check=None,
           part_rows=0):
    """one tt_op_groupnorm_ex launch; asserts `ran`, kappa <= 128 for the case's own data (big_mean: its own wide bound and finiteness only),
    every bound, the exact zeros past vlen and every sentinel.  part_rows: the statistics come as fused partials (gn_part), no statistics pass"""
    d = gn_data(C_, B, S, seed_shift, big_mean)
    part = gn_part(C_, B, S, seed_shift, part_rows, tuple(vlen) if vlen else None).cuda() if part_rows else None
    xd = (d["x"] if x is None else x).cuda()
    dev = {k: d[k].cuda() for k in ("gamma", "beta", "ss")}
    nws = lib.tt_op_groupnorm_workspace(B, S) // 4
    ws = torch.full((nws + 64,), SENTINEL, device="cuda")
    out_t = torch.full((B * S + 1, C_ + PAD), SENTINEL, device="cuda", dtype=tdt) if outs in ("t", "both") else None
    o32 = torch.full((B * S + 1, C_ + PAD), SENTINEL, device="cuda") if outs in ("f32", "both") else None
    gcount = torch.zeros(1, device="cuda", dtype=torch.int32) if guard else None
    desc = fill(E.GroupNormDesc(), x=xd, B=B, S=S, C=C_, gamma=dev["gamma"], beta=dev["beta"], eps=1e-5, scale_shift=dev["ss"] if ss else None,
                ss_batch_stride=SS_FORMS[ss][1] * C_ if ss else 0, ss_batch_div=SS_FORMS[ss][0] if ss else 0, act=act, out_t=out_t, ldot=C_ + PAD, out_f32=o32,
                ldo32=C_ + PAD, partial=ws, vperiod=len(vlen) if vlen else 0, guard=gcount, gemm_part=part, part_rows=part_rows)
    for i, v in enumerate(vlen or ()):
        desc.vlen[i] = v
    ran = (C.c_int * 4)()
    E.check(lib.tt_op_groupnorm_ex(dt, C.byref(desc), ran, None))
    torch.cuda.synchronize()
    ran = tuple(ran)
    what = f"GroupNorm {name} C={C_} B={B} S={S} ss={ss} act={act} vlen={vlen} [stats={ran[0]} {E.GROUPNORM_APPLY.get(ran[1], ran[1])} rows={ran[2]} fused={ran[3]}]"
    assert ran == (0 if part_rows else 1, int(C_ == 1024), 2 if C_ == 1024 and B * S <= 4096 else 4, int(bool(part_rows) and C_ == 1024)), what
    assert bool((ws[nws:] == SENTINEL).all()), f"{what}: statistics written past the workspace"
    ref, kappa = gn_ref(C_, B, S, ss, act, tuple(vlen) if vlen else None, seed_shift, big_mean)
    if big_mean:
        assert float(kappa.min()) > 5e3
    elif x is None:
        assert float(kappa.max()) <= N.KAPPA_MAX, f"{what}: kappa {float(kappa.max()):.1f}"
    sel = slice(None) if check is None else check
    res = []
    for out, typ in ((out_t, name), (o32, "f32")):
        if out is None:
            continue
        got = out[:B * S, :C_].cpu().reshape(B, S, C_)
        if big_mean:
            assert bool(torch.isfinite(got).all())
        w = N.assert_within_bound(f"{what} {'f32' if out is o32 else 'T'}", got[sel], rows_of(ref, sel), typ)
        note(f"GroupNorm {'f32' if out is o32 else 'T'} out C={C_}" + (" (kappa 1e4)" if big_mean else ""), w)
        for b in range(B):
            if vlen and (check is None or b in check):
                assert bool((got[b, vlen[b % len(vlen)]:] == 0).all()), f"{what}: rows past vlen of sample {b} are not zero"
        assert untouched_outside(out, B * S, C_), f"{what}: output written outside the rows"
        res.append(got)
    return res, int(gcount.item()) if guard else 0


GN_FORMS = [(None, R.ACT_NONE, "f32"), ("sample", R.ACT_SILU, "both"), ("sample", R.ACT_NONE, "t"), (None, R.ACT_SILU, "t")]


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("C_", N.GN_CHANNELS)
def test_groupnorm_shapes(lib, name, dt, tdt, C_):
    """one row, less than one chunk, exactly one, one row more, several chunks, 61 chunks of 17 and 64 chunks of 65 rows; scale / shift
    absent, per sample, shared by pairs of samples (ss_batch_div = 2) and by all (ss_batch_stride = 0); no activation and SiLU; each output set"""
    for i, (B, S) in enumerate((b, s) for c, b, s in N.gn_cases() if c == C_):
        for ss, act, outs in (GN_FORMS if (B, S) == (2, 77) else [GN_FORMS[i % 4]]):
            run_gn(lib, name, dt, tdt, C_, B, S, ss, act, outs)
    run_gn(lib, name, dt, tdt, C_, 4, 77, "div2", R.ACT_SILU, "both")
    run_gn(lib, name, dt, tdt, C_, 3, 17, "shared", R.ACT_NONE, "both")
    run_gn(lib, name, dt, tdt, C_, 2, 77, None, R.ACT_NONE, "both", big_mean=True)


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("C_", N.GN_CHANNELS)
@pytest.mark.parametrize("B,S,vlen", [(4, 77, (77, 9)), (3, 333, (1, 333, 200))])
def test_groupnorm_padded_batches(lib, name, dt, tdt, C_, B, S, vlen):
    """vperiod / vlen on the stand-alone statistics pass: whole chunks past a sample's end, a sample of one valid row; zeros past vlen"""
    run_gn(lib, name, dt, tdt, C_, B, S, "sample", R.ACT_SILU, "both", vlen=vlen, seed_shift=1)


@pytest.mark.parametrize("name,dt,tdt", DT)
def test_groupnorm_rows_per_block_switch(lib, name, dt, tdt):
    """C = 1024: B S = 4096 rows run two rows per block, 4098 run four (S = 2049 leaves a one-row tail block); run_gn asserts it through `ran`"""
    run_gn(lib, name, dt, tdt, 1024, 2, 2048, "sample", R.ACT_SILU, "t" if name != "f32" else "f32")
    run_gn(lib, name, dt, tdt, 1024, 2, 2049, "sample", R.ACT_SILU, "t" if name != "f32" else "f32")


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("C_", [128, 1024])
def test_groupnorm_guard(lib, name, dt, tdt, C_):
    """a clean launch leaves the counter at 0; an inf in one group of sample 1 raises it, and samples 0 and 2 still meet their bound"""
    B, S = 3, 77
    assert run_gn(lib, name, dt, tdt, C_, B, S, guard=True)[1] == 0
    x = gn_data(C_, B, S)["x"].clone()
    x[1, 40, 5] = float("inf")
    assert run_gn(lib, name, dt, tdt, C_, B, S, guard=True, x=x, check=[0, 2])[1] > 0


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("C_", [512, 2048])
def test_groupnorm_fused_statistics_on_the_generic_apply_kernel(lib, name, dt, tdt, C_):
    """fused partials with one and four 16-column strips per group (C = 512, 2048) on the generic apply kernel: 32-row tiles that straddle
    the 77-row samples, a sample of 9 valid rows; run_gn asserts ran == (0, 0, 4, 0), the bound, the zeros past vlen and the sentinels"""
    run_gn(lib, name, dt, tdt, C_, 4, 77, "sample", R.ACT_SILU, "both", vlen=(77, 9), seed_shift=1, part_rows=32)


GN_FUSED_LONG_S = 1100  # 35 tiles of 32 rows = 70 partial items per sample: the loop behind the GN_HEAD requested-ahead items runs


@pytest.mark.parametrize("name,dt,tdt", DT)
@pytest.mark.parametrize("ss", [None, "sample"])
@pytest.mark.parametrize("B", [2, 4])
def test_groupnorm_fused_statistics_remainder_loop(lib, name, dt, tdt, B, ss):
    """C = 1024 on fused partials with more items per thread than are requested ahead: 2200 rows (two rows per block) and 4400 rows (four),
    with and without scale / shift; run_gn asserts ran == (0, 1, 2 | 4, 1) and kappa <= KAPPA_MAX (the data of gn_seed(1024, B, 1100) has
    kappa 1.7 at B = 2 and 2.1 at B = 4, computed on the host)"""
    run_gn(lib, name, dt, tdt, 1024, B, GN_FUSED_LONG_S, ss, R.ACT_SILU, "both", part_rows=32)


@pytest.mark.parametrize("name,dt,tdt", DT)
def test_groupnorm_part_entry_keeps_its_bits(lib, name, dt, tdt):
    """tt_op_groupnorm_part (re-based on the descriptor mapping) and tt_op_groupnorm_ex with the same fused statistics: the same bits, the
    fused-statistics template, and the bound.  Partials in the GEMM epilogue's layout (32-row tiles straddling the samples) from the host."""
    B, S, C_, rows, vlen = 2, 870, 1024, 32, (870, 801)
    d = gn_data(C_, B, S)
    part = R.gn_partials_reference(d["x"].reshape(B * S, C_), rows, S, 2, list(vlen)).float().cuda()
    xd, gam, bet, ssd = d["x"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), d["ss"].cuda()
    ws = torch.zeros(lib.tt_op_groupnorm_workspace(B, S) // 4 + 64, device="cuda")
    a_t, b_t = (torch.full((B * S, C_), SENTINEL, device="cuda", dtype=tdt) for _ in range(2))
    a_32, b_32 = (torch.full((B * S, C_), SENTINEL, device="cuda") for _ in range(2))
    E.check(lib.tt_op_groupnorm_part(dt, E.ptr(xd), B, S, C_, E.ptr(gam), E.ptr(bet), E.ptr(ssd), R.ACT_SILU, E.ptr(part), rows, 2, (C.c_int * 2)(*vlen),
                                     E.ptr(a_t), E.ptr(a_32), E.ptr(ws), None))
    desc = fill(E.GroupNormDesc(), x=xd, B=B, S=S, C=C_, gamma=gam, beta=bet, eps=1e-5, scale_shift=ssd, ss_batch_stride=2 * C_, act=R.ACT_SILU, out_t=b_t,
                ldot=C_, out_f32=b_32, ldo32=C_, partial=ws, gemm_part=part, part_rows=rows, vperiod=2)
    desc.vlen[0], desc.vlen[1] = vlen
    ran = (C.c_int * 4)()
    E.check(lib.tt_op_groupnorm_ex(dt, C.byref(desc), ran, None))
    torch.cuda.synchronize()
    assert tuple(ran) == (0, 1, 2, 1), tuple(ran)
    assert torch.equal(a_t, b_t) and torch.equal(a_32, b_32), "tt_op_groupnorm_part and tt_op_groupnorm_ex differ"
    ref, kappa = gn_ref(C_, B, S, "sample", R.ACT_SILU, vlen)
    assert float(kappa.max()) <= N.KAPPA_MAX
    note("GroupNorm f32 out C=1024 (fused statistics)", N.assert_within_bound(f"GroupNorm on fused statistics {name} f32", a_32.cpu().reshape(B, S, C_), ref, "f32"))
    N.assert_within_bound(f"GroupNorm on fused statistics {name} T", a_t.cpu().reshape(B, S, C_), ref, name)
