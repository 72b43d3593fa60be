"""CPU: the element-wise bound of tests/attention_reference.py has margin and can fail.  The plain fp32 emulation of the flash kernels' algorithm
stays at or below 0.5 of the fp32 part e of the bound, and its operand-typed result inside the full bound, on every family x mode x type x
shape that tests/test_gpu_flash_forms.py launches (the kernels have to stay at or below 1); each of five corruptions of the emulation puts at
least one element outside the bound in bf16 and in fp16 on the family designed for it; the fp64 reference agrees with a naive softmax written
with no shared code."""
import functools

import pytest
import torch

from tests import attention_reference as A

HALF = 0.5


@functools.lru_cache(maxsize=None)
def case(tname, fam, n, B, H, mode):
    inp = A.make_inputs(fam, tname, n, B, H)
    return inp, A.run_reference(inp, tname, mode)


@pytest.mark.parametrize("tname", ["bf16", "f16", "f32"])
def test_emulation_is_inside_half_the_bound(tname):
    worst32 = worst_t = 0.0
    for t, fam, n, B, H, mode, ways in A.emulation_cases():
        if t != tname:
            continue
        inp, ref = case(tname, fam, n, B, H, mode)
        emu = A.run_emulation(inp, tname, mode, ways)
        r32 = float(A.worst_ratio(emu, ref, tname, typed=False).max())
        rt = float(A.worst_ratio(emu.to(A.TDT[tname]), ref, tname).max())
        what = f"{tname} {fam} {mode} n={n} pairs={B}x{H} ways={ways}"
        assert r32 <= HALF, f"{what}: the emulation's fp32 result is at {r32:.3f} of e"
        assert rt <= 1.0, f"{what}: the emulation's typed result is at {rt:.3f} of the bound"
        worst32, worst_t = max(worst32, r32), max(worst_t, rt)
    print(f"[bound] flash emulation {tname}: worst fp32 |err|/e={worst32:.3f}, typed |err|/bound={worst_t:.3f}")
    case.cache_clear()


def corrupted_ratio(tname, fam, mode, n=300, ways=1, after=None, **mutation):
    B, H = A.PAIRS[n]
    inp = A.make_inputs(fam, tname, n, B, H)
    ref = A.run_reference(inp, tname, mode)
    clean = A.run_emulation(inp, tname, mode, ways)
    assert float(A.worst_ratio(clean.to(A.TDT[tname]), ref, tname).max()) <= 1.0
    bad = A.run_emulation(inp, tname, mode, ways, **mutation)
    if after is not None:
        after(bad)
    return float(A.worst_ratio(bad.to(A.TDT[tname]), ref, tname).max())


@pytest.mark.parametrize("tname", ["bf16", "f16"])
@pytest.mark.parametrize("ways", [1, 2])
def test_bound_rejects_the_corruptions(tname, ways):
    def other_row(out):
        out[1, 37] = out[1, 38].clone()

    got = {
        "one query row taken from another row (peaked)": corrupted_ratio(tname, "peaked", "plain", ways=ways, after=other_row),
        "the same at equal weights (flat)": corrupted_ratio(tname, "flat", "plain", ways=ways, after=other_row),
        "last key counted twice (heavy)": corrupted_ratio(tname, "heavy", "plain", ways=ways, dup_last=True),
        "last key counted twice, one key in the last tile (heavy, n = 129)": corrupted_ratio(tname, "heavy", "plain", n=129, ways=ways, dup_last=True),
        "relative-position index shifted by one (peaked)": corrupted_ratio(tname, "peaked", "relpos", ways=ways, rp_shift=1),
        "the rescale skipped at the last tile (ascending)": corrupted_ratio(tname, "ascending", "plain", ways=ways, skip_rescale=9),
        "causal mask off by one on the diagonal of a 64-query block (peaked)": corrupted_ratio(tname, "peaked", "causal", ways=ways, causal_off_block=1),
    }
    for what, r in got.items():
        print(f"[bound] {tname} ways={ways} {what}: worst |err|/bound={r:.1f}")
    for what, r in got.items():
        assert r > 1.0, f"{tname}: {what} stays inside the bound ({r:.3f})"


@pytest.mark.parametrize("mode", ["plain", "relpos", "causal"])
def test_reference_agrees_with_the_naive_form(mode):
    """n = 70 reaches the +-64 saturation of the relative-position bucket; the second batch row has 33 valid rows"""
    inp = A.make_inputs("peaked", "f32", 70, 2, 2, nv=(70, 33))
    ref = A.run_reference(inp, "f32", mode)
    rp = inp["relpos"] if mode == "relpos" else None
    want = A.naive_reference(inp["q"], inp["k"], inp["vt"], 2, rp, mode == "causal", inp["nvp"])
    assert torch.equal(torch.isfinite(want).all(-1), ref.valid)
    err = (ref.value - want).abs()[ref.valid]
    assert float(err.max()) < 1e-12, float(err.max())
    assert bool((ref.err[ref.valid] > 0).all())
