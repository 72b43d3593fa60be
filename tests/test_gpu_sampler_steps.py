"""-m gpu: the paths of csrc/sampling.hip that the other sampler tests reach only by accident, at operator level (tt_op_sample) against the
oracle's restatement of the HF warpers with injected Exp(1) draws: the fast sampler's counting search with few survivors, the full-sort
sampler (any top_k), its zero fold, and a row of NaN logits on the Philox path."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import tortoise_oracle as O
from tortoise_tts_amd import engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return E.init()


def _seen(ids, B, V):
    seen = np.zeros((B, (V + 31) // 32), dtype=np.uint32)
    if ids is not None:
        for b in range(B):
            for t in ids[b].tolist():
                seen[b, t >> 5] |= np.uint32(1 << (t & 31))
    return torch.from_numpy(seen.view(np.int32)).cuda()


def _sample(lib, logits, k, top_p, penalty=1.0, temperature=1.0, ids=None, q=None, seed=0, stop=None):
    """one tt_op_sample step; returns (tokens, unfinished) on the host"""
    B, V = logits.shape
    s = E.Sampling()
    s.temperature, s.top_p, s.repetition_penalty, s.top_k, s.seed, s.row_offset = temperature, top_p, penalty, k, seed, 0
    qd = None
    if q is not None:
        qd = q.cuda().contiguous()
        s.exp_noise = E.ptr(qd)
    seen = _seen(ids, B, V)
    unfinished = torch.ones(B, dtype=torch.int32, device="cuda")
    codes = torch.zeros(B, 4, device="cuda", dtype=torch.int32)
    ld = logits.cuda().contiguous()
    E.check(lib.tt_op_sample(E.ptr(ld), V, B, V, E.ptr(seen), C.byref(s), 0, E.ptr(unfinished), V - 1 if stop is None else stop, E.ptr(codes), 4, None))
    return codes[:, 0].cpu().long(), unfinished.cpu()


def _oracle(logits, k, top_p, q, penalty=1.0, temperature=1.0, ids=None):
    if ids is None:
        ids = torch.zeros(logits.shape[0], 1, dtype=torch.long)  # (unused at penalty 1)
    scores = O.warp_logits(logits, ids, penalty, temperature, k, top_p)
    return O.multinomial_from_exponential(torch.softmax(scores, -1), q[0]), scores


@pytest.fixture(scope="module")
def few_survivors():
    """600 tokens at 32768 + 0.25 i (i a permutation of 0 .. 599) over randn * 3: all 600 share the upper 16 key bits (the bucket at 2^15 is 256
    wide, the span 150), so the 16-bit lower bound of the k-th key admits 600 > 512 candidates and the counting search over all keys runs."""
    g = torch.Generator().manual_seed(4711)
    B, V = 4, 8194
    logits = torch.randn(B, V, generator=g) * 3
    for b in range(B):
        at = torch.randperm(V, generator=g)[:600]
        logits[b, at] = 32768.0 + 0.25 * torch.randperm(600, generator=g).float()
    q = torch.empty(1, B, V).exponential_(1, generator=g)
    return logits, q


@pytest.mark.parametrize("k", [50, 200])
@pytest.mark.parametrize("top_p", [1.0, 0.8])
def test_counting_search_with_few_survivors(lib, few_survivors, k, top_p):
    """The fast sampler's generic path (counting search, 16 rounds) ending in few survivors - reached otherwise only through the all-ties plateau
    and typical masks: k = 50 ends in the wave tail, k = 200 in the LDS tail.  The probabilities fall by e^-0.25 per place, so the ascending
    cumulative sum crosses 1 - 0.8 between places 6 and 7 (0.223 / 0.174): every cumulative sum is checked to lie >= 1e-3 from the cut."""
    logits, q = few_survivors
    want, scores = _oracle(logits, k, top_p, q)
    assert int(torch.isfinite(scores).sum(-1).max()) <= k
    if top_p < 1.0:
        cum = torch.sort(O.top_k_(logits, k), descending=False)[0].softmax(-1).cumsum(-1)
        margin = float((cum - (1 - top_p)).abs().min())
        print(f"[parity] few survivors k={k}: cumulative sums stay {margin:.3e} from the cut")
        assert margin >= 1e-3
    got, _ = _sample(lib, logits, k, top_p, q=q)
    print(f"[parity] few survivors k={k} top_p={top_p}: tokens", got.tolist(), want.tolist())
    assert torch.equal(got, want)


@pytest.mark.parametrize("V,k", [(8194, 0), (8194, 300), (8194, 8194), (300, 0)])
@pytest.mark.parametrize("top_p", [0.8, 1.0])
def test_full_sort_sampler_matches_oracle(lib, V, k, top_p):
    """sample_wide_kernel (top_k == 0, > 256, or the whole vocabulary) through tt_op_sample: the other tests reach it through generate only."""
    g = torch.Generator().manual_seed(900 + V + 3 * k)
    B = 8
    logits = torch.randn(B, V, generator=g) * 3
    ids = torch.randint(0, V, (B, 24), generator=g)
    q = torch.empty(1, B, V).exponential_(1, generator=g)
    want, scores = _oracle(logits, k, top_p, q, 2.0, 0.8, ids)
    if top_p < 1.0:  # printed, not asserted: random scores come as close to the cut as they come; a mismatch in a row whose margin is of
        # the order of the sum's rounding (V * 2^-24) would be the oracle's summation order, not the kernel
        cum = torch.sort(O.warp_logits(logits, ids, 2.0, 0.8, k, 1.0), descending=False)[0].softmax(-1).cumsum(-1)
        print(f"[parity] full-sort sampler V={V} k={k}: nearest cumulative sum to the cut, per row:", [f"{m:.1e}" for m in (cum - (1 - top_p)).abs().min(-1)[0].tolist()])
    got, _ = _sample(lib, logits, k, top_p, 2.0, 0.8, ids, q)
    print(f"[parity] full-sort sampler V={V} k={k} top_p={top_p}: {int((got == want).sum())} / {B} tokens equal; up to {int(torch.isfinite(scores).sum(-1).max())} kept")
    assert torch.equal(got, want)


def test_full_sort_sampler_keeps_negative_zero_at_the_kth_place(lib):
    """300 distinct positive scores, 100 zeros of alternating sign, the rest negative; k = 350: the k-th value is 0.0, and TopKLogitsWarper's
    `scores < kth` keeps all 100 zeros, -0.0 included.  The noise hands one -0.0 token by far the smallest q, so the oracle returns it.
    (Fails on the commit before the samplers shared sample_score: its full-sort kernel ordered -0.0 below +0.0 and dropped it.)"""
    g = torch.Generator().manual_seed(77)
    V = 8194
    perm = torch.randperm(V, generator=g)
    logits = -(1.0 + torch.rand(1, V, generator=g))
    logits[0, perm[:300]] = torch.linspace(0.01, 3.0, 300)
    zeros = perm[300:400]
    logits[0, zeros[0::2]] = 0.0
    logits[0, zeros[1::2]] = -0.0
    lucky = int(zeros[51])
    assert np.signbit(float(logits[0, lucky])) and float(logits[0, lucky]) == 0.0
    q = torch.empty(1, 1, V).exponential_(1, generator=g).clamp_(min=1e-3)
    q[0, 0, lucky] = 1e-9
    want, scores = _oracle(logits, 350, 1.0, q)
    assert int(torch.isfinite(scores).sum()) == 400 and int(want[0]) == lucky
    got, _ = _sample(lib, logits, 350, 1.0, q=q)
    print("[parity] full-sort sampler, -0.0 at the k-th place: token", got.tolist(), want.tolist())
    assert torch.equal(got, want)


@pytest.mark.parametrize("top_p", [0.8, 1.0])
def test_a_row_of_nan_logits_ends_with_the_stop_token(lib, top_p):
    """Philox path (no injected noise): the poisoned row emits the stop token and is finished; the other rows draw what they draw without it."""
    g = torch.Generator().manual_seed(31)
    B, V, stop = 4, 8194, 8193
    logits = torch.randn(B, V, generator=g) * 3
    ids = torch.randint(0, V, (B, 24), generator=g)
    clean, clean_unf = _sample(lib, logits, 50, top_p, 2.0, 0.8, ids, seed=99, stop=stop)
    poisoned = logits.clone()
    poisoned[2] = float("nan")
    got, unf = _sample(lib, poisoned, 50, top_p, 2.0, 0.8, ids, seed=99, stop=stop)
    print(f"[parity] NaN row top_p={top_p}: tokens", got.tolist(), "clean", clean.tolist(), "unfinished", unf.tolist())
    assert int(got[2]) == stop and int(unf[2]) == 0
    keep = [0, 1, 3]
    assert torch.equal(got[keep], clean[keep]) and torch.equal(unf[keep], clean_unf[keep])
