"""CPU: the element-wise GEMM bound of tests/gemm_reference.py has teeth at the largest K the GPU matrix uses (4096), and the host reducer
of the GroupNorm statistics partials agrees with a brute-force per-sample sum."""
import math

import pytest
import torch

from tests import gemm_reference as R

M, N, K, BM = 80, 64, 4096, 64  # two row tiles of 64: the last one ragged (rows 64 .. 79)


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).bfloat16().float()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().float()
    bias = torch.randn(N, generator=g)
    got = A @ W.t() + bias  # an fp32 result: what a correct kernel returns
    ref, _ = R.std_reference(R.gemm_operand(A, K), W, bias)
    return A, W, bias, got, ref


def _rejects(got, ref):
    with pytest.raises(AssertionError):
        R.assert_within_bound("corrupted", got, ref, "f32", "bf16", tile=(BM, 64))


def test_valid_result_passes(case):
    A, W, bias, got, ref = case
    assert R.assert_within_bound("fp32 result K=4096", got, ref, "f32", "bf16", tile=(BM, 64)) < 1.0


def test_one_dropped_k_tile_is_caught(case):
    A, W, bias, got, ref = case
    bad = got.clone()
    bad[17, 5] -= A[17, 1024:1088] @ W[5, 1024:1088]
    _rejects(bad, ref)


def test_two_swapped_rows_are_caught(case):
    A, W, bias, got, ref = case
    bad = got.clone()
    bad[[40, 41]] = bad[[41, 40]]
    _rejects(bad, ref)


def test_bias_added_twice_in_one_strip_is_caught(case):
    A, W, bias, got, ref = case
    bad = got.clone()
    bad[:, 16:32] += bias[16:32]
    _rejects(bad, ref)


def test_zero_row_of_the_ragged_last_tile_is_caught(case):
    A, W, bias, got, ref = case
    bad = got.clone()
    bad[M - 1] = 0.0
    _rejects(bad, ref)


def test_t_output_rounding_is_inside_the_bound(case):
    A, W, bias, got, ref = case
    R.assert_within_bound("bf16 copy", got.bfloat16().float(), ref, "bf16", "bf16")
    with pytest.raises(AssertionError):  # the bf16 rounding term does not cover an fp16-typed claim
        R.assert_within_bound("bf16 copy as fp16", got.bfloat16().float(), ref, "f16", "f16", quiet=True)


@pytest.mark.parametrize("rows", [32, 64])
@pytest.mark.parametrize("B,S,vlen", [(3, 100, None), (2, 870, [870, 801]), (4, 64, None), (3, 200, [200, 77, 130])])
def test_statistics_reducer_matches_brute_force(rows, B, S, vlen):
    """partials in the epilogue's layout (tiles straddling a sequence, padded rows with gn_vperiod) reduced as the consumer does =
    per-(sample, group) sums over the valid rows; tiles that do not straddle leave slot 1 at zero"""
    C = 1024
    g = torch.Generator().manual_seed(B * S + rows)
    y = torch.randn(B * S, C, generator=g, dtype=torch.float64)
    vp = len(vlen) if vlen else 0
    part = R.gn_partials_reference(y, rows, S, vp, vlen)
    want = R.group_sums_bruteforce(y, B, S, C, vp, vlen)
    got = R.gn_group_sums(part, B, S, C, rows)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-9)
    t = torch.arange(part.shape[0])
    straddle = ((t * rows) // S + 1) * S < torch.clamp((t + 1) * rows, max=B * S)
    assert (part[~straddle][:, 1] == 0).all()
    if (S % rows) != 0:
        assert straddle.any()
    R.assert_partials("synthetic", part.float(), y, rows, S, vp, vlen, quiet=True)
    wrong = part.clone()
    i = int(torch.nonzero(straddle)[0]) if straddle.any() else 1
    wrong[i, 0], wrong[i, 1] = part[i, 1].clone(), part[i, 0].clone()  # a sum filed under the wrong sequence slot
    if straddle.any():
        with pytest.raises(AssertionError):
            R.assert_partials("slots swapped", wrong.float(), y, rows, S, vp, vlen, quiet=True)
