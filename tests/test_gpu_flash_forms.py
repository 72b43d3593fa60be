"""-m gpu: every flash-attention kernel form of csrc/attention.hip (and the fp32 verification kernel of csrc/attention_f32.hip) one launch at a
time through tt_op_flash_attention_rows, against the fp64 reference of tests/attention_reference.py with an element-wise bound.  Every launch
reads the host-side record of what started (tt_op_flash_ran: kernel, NQ, KS) and asserts it, so a change of the thresholds in
flash_attention_launch cannot silently stop covering a kernel; the form is steered with `variant` and the TTX_FLASH32 switch (restored in a
finally), which lets three to six (batch, head) pairs reach every kernel but flash_lds_kernel<T,2,1> (689 pairs).  The operands hold +-1e4
wherever the operation says a location is not part of the problem (columns n .. n_pad of vt, the rows past nv of a padded batch), the output
is pre-filled with a sentinel, and no element is left out of the bound: a non-finite output is an infinite ratio.  Beyond the bound: padded
batch rows keep the sentinel bit for bit past nv[b] (nv_period shorter than the batch, entries n, one past a tile edge and 1); one (q, k, v)
pair replicated into every (batch, head) slot gives every slot pair 0's bits (indexing, the XCD remap and cross-workgroup interference, apart
from arithmetic) at grids that are no multiple of 8; a second launch gives the first one's bits.  Each launch prints a [parity] line; the last
line of a module run lists the worst |err| / bound per form and type (the figures in the docstring of tests/attention_reference.py) and the
module's wall time.

Findings: none.  Every form stayed inside the bound, every sentinel and replica check held (MI355X).
"""
import ctypes as C
import functools
import time

import pytest
import torch

from tortoise_tts_amd import engine as E
from tests import attention_reference as A

pytestmark = pytest.mark.gpu
DT = {"bf16": E.TT_BF16, "f16": E.TT_F16, "f32": E.TT_F32}
SENTINEL = -77.0  # exact in both 16-bit types
WORST = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    t0 = time.time()
    yield E.init()
    operands.cache_clear()
    reference.cache_clear()
    torch.cuda.empty_cache()
    print("[bound] flash worst |err|/bound per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + f"; module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def operands(tname, fam, n, B, H, nv=None):
    """the device copies of one case's operands, made once and shared (no test writes to them)"""
    inp = A.make_inputs(fam, tname, n, B, H, nv)
    return {k: v.cuda().contiguous() if isinstance(v, torch.Tensor) else v for k, v in inp.items()}


@functools.lru_cache(maxsize=None)
def reference(tname, fam, n, B, H, mode, nv=None):
    """the fp64 reference and its bound, computed on the device"""
    return A.run_reference(operands(tname, fam, n, B, H, nv), tname, mode)


def launch(lib, form, tname, inp, mode, nv=None):
    """one launch of `form`; asserts the record of what started; returns out [B][n][H * 64] (sentinel where nothing was written)"""
    B, H, n = inp["B"], inp["H"], inp["n"]
    variant, switch = A.form_steer(form, mode)
    out = torch.full((B, n, H * 64), SENTINEL, device="cuda", dtype=A.TDT[tname])
    relpos = inp["relpos"] if mode == "relpos" else None
    nv_arr = (C.c_int * len(nv))(*nv) if nv else None
    ran = (C.c_int * 3)(-2, -2, -2)
    torch.cuda.synchronize()
    prev = lib.ttx_kernel_variant(E.TTX_FLASH32, switch)
    try:
        E.check(lib.tt_op_flash_attention_rows(DT[tname], E.ptr(inp["q"]), E.ptr(inp["k"]), E.ptr(inp["vt"]), E.ptr(out), B, H, n, inp["n_pad"],
                                               int(mode == "causal"), E.ptr(relpos), nv_arr, len(nv) if nv else 0, variant, None))
        E.check(lib.tt_op_flash_ran(ran))
        torch.cuda.synchronize()
    finally:
        lib.ttx_kernel_variant(E.TTX_FLASH32, prev)
    ran = tuple(ran)
    want = A.FORMS[form]["ran"]
    assert ran == want, (f"{form} {tname} {mode} n={n} pairs={B}x{H}: launched {E.FLASH_KERNELS.get(ran[0], ran[0])} NQ={ran[1]} KS={ran[2]}, "
                         f"expected {E.FLASH_KERNELS[want[0]]} NQ={want[1]} KS={want[2]}")
    return out


def check(lib, form, tname, fam, n, B, H, mode, nv=None):
    inp = operands(tname, fam, n, B, H, nv)
    ref = reference(tname, fam, n, B, H, mode, nv)
    out = launch(lib, form, tname, inp, mode, nv)
    got = A.to_pairs(out, B, H)
    ran = A.FORMS[form]["ran"]
    ratio = A.worst_ratio(got, ref, tname)
    worst = float(ratio.max())
    print(f"[parity] flash {form} {tname} {fam} {mode} n={n} pairs={B}x{H}{' nv=' + str(nv) if nv else ''} ran={E.FLASH_KERNELS[ran[0]]} NQ={ran[1]} KS={ran[2]} "
          f"rel_l2={A.rel_l2(got, ref):.3e} worst |err|/bound={worst:.3f}")
    key = f"{form} {tname}"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    A.assert_within_bound(f"{form} {tname} {fam} {mode} n={n} pairs={B}x{H}", got, ref, tname, quiet=True)
    return out


BOUND_CASES = [(form, tname, mode, n) for form, f in A.FORMS.items() for tname in f["types"] for mode in f["modes"] for n in f["ns"]]


@pytest.mark.parametrize("form,tname,mode,n", BOUND_CASES)
def test_form_within_bound(lib, form, tname, mode, n):
    """every input family of the form at this length: the expected kernel launched and every output element is inside the bound"""
    B, H = A.form_shape(form, n)
    for fam in A.form_families(form):
        check(lib, form, tname, fam, n, B, H, mode)


PADDED = {"flash_kernel<T,1,true>": (70, (70, 33, 17, 1)), "flash_lds_kernel<T,1,2>": (300, (300, 129, 65, 1)), "flash32_kernel<T,2>": (300, (300, 129, 65, 1))}


@pytest.mark.parametrize("tname", ["bf16", "f16"])
@pytest.mark.parametrize("form,mode", [(form, mode) for form in PADDED for mode in A.FORMS[form]["modes"]])
def test_padded_rows(lib, form, mode, tname):
    """FlashArgs::nv with a period of 4 under 5 batch rows (b % nv_period wraps): batch row b is attention over its first nv[b % 4] rows; the
    rows of out at and beyond them keep the sentinel bit for bit, the rows before them meet the bound with +-1e4 in the unused operand rows"""
    n, nv = PADDED[form]
    B, H = 5, 2
    for fam in ("peaked", "heavy"):
        out = check(lib, form, tname, fam, n, B, H, mode, nv)
        for b in range(B):
            rows = nv[b % len(nv)]
            tail = out[b, rows:]
            assert torch.equal(tail.view(torch.int16), torch.full_like(tail, SENTINEL).view(torch.int16)), f"{form} {fam} {mode}: batch row {b}: rows past nv = {rows} were written"


def _replica_shape(form):
    return A.BIG if form == "flash_lds_kernel<T,2,1>" else (70, 2, 3) if form == "flash_kernel<T,1,true>" else (300, 1, 3)


def _replicated(form, tname):
    n, B, H = _replica_shape(form)
    src = operands(tname, "peaked", n, 1, 1)
    P = B * H
    inp = dict(src, B=B, H=H)
    for name in ("q", "k", "vt"):
        inp[name] = src[name].expand(P, -1, -1).contiguous()
    inp["relpos"] = src["relpos"].expand(H, -1).contiguous()
    return inp


@pytest.mark.parametrize("form,tname,mode", [(form, tname, mode) for form, f in A.FORMS.items() for tname in f["types"] for mode in f["modes"] if mode != "plain"])
def test_replicated_pairs(lib, form, tname, mode):
    """one (q, k, v) pair in every (batch, head) slot and one relative-position row for every head: every slot's output equals slot 0's in bits.
    Grids: 5 x 6 (flash_kernel), 5 x 3 (flash_lds_kernel<T,1,*>), 3 x 3 (flash32_kernel), 2 x 689 (flash_lds_kernel<T,2,1>): no multiple of 8."""
    inp = _replicated(form, tname)
    got = A.to_pairs(launch(lib, form, tname, inp, mode), inp["B"], inp["H"])
    assert bool(torch.isfinite(got.float()).all()), f"{form} {tname} {mode}: non-finite output"
    bits = got.contiguous().view(torch.int32 if tname == "f32" else torch.int16)
    differ = (bits != bits[:1]).flatten(1).any(1)
    assert not bool(differ.any()), f"{form} {tname} {mode}: slots {torch.nonzero(differ).flatten().tolist()[:8]} differ from slot 0"


@pytest.mark.parametrize("form,tname", [(form, tname) for form, f in A.FORMS.items() for tname in f["types"]])
def test_second_launch_gives_the_same_bits(lib, form, tname):
    n = A.FORMS[form]["ns"][-1]
    B, H = A.form_shape(form, n)
    for mode in A.FORMS[form]["modes"]:
        inp = operands(tname, "peaked", n, B, H)
        a = launch(lib, form, tname, inp, mode)
        b = launch(lib, form, tname, inp, mode)
        view = torch.int32 if tname == "f32" else torch.int16
        assert torch.equal(a.view(view), b.view(view)), f"{form} {tname} {mode} n={n}: two launches of one case differ"
