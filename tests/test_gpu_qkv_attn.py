"""-m gpu: the decode step's QKV projection and attention as ONE launch (csrc/decode_attention.hip decode_qkv_attn_kernel, TT_AR_OPT_FUSED_QKV_ATTN).

  * operator level: `tt_op_decode_qkv_attention` against the composition of the two launches it replaces (the EPI_QKV_DECODE GEMM through
    tt_op_gemm_ex, then tt_op_decode_attention) on the same inputs - BIT for bit on the attention rows, the scaled query rows and the whole
    K / V caches after the call - and against torch fp32 at the bars tests/test_gpu_r6.py::test_decode_attention_operator uses;
  * engine level, full width: the codes of a 256-candidate, 200-token generation do not depend on the option (graph replay and eager), the
    logits of a row at B = 256 (one launch) equal the same row at B = 64 (two launches), tt_ar_stat(h, 2) tells which form a handle takes,
    and the batches the rule excludes (two utterances per batch, session handles narrow and wide, a long prefix, other batch sizes, fp32)
    keep seven launches per layer.
"""
import ctypes as C
import math

import pytest
import torch

from oracle import make_golden_full as GF
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd.config import ARConfig
from tests.gpu_util import DTYPES, report
from tests.test_gpu_r6 import _decode_attention_reference

pytestmark = pytest.mark.gpu
H, D = 16, 1024
TMAX = 208
# rounded-once T outputs from f32 accumulation: the bars of tests/test_gpu_r6.py::test_decode_attention_operator
ATTN_TOL = {"bf16": 4e-3, "f16": 6e-4}


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.fixture(scope="module")
def sds():
    import bench
    return bench.synthetic_weights()


def _qkv_decode_gemm(lib, dt, h, W, bias, step, q, kc, vc, B):
    d = E.GemmDesc()
    d.taps, d.splitk, d.slope, d.slope_t = 1, 1, 0.2, 0.2
    d.A, d.lda, d.W, d.ldw, d.M, d.N, d.K = E.ptr(h), D, E.ptr(W), D, B, 3 * D, D
    d.bias = E.ptr(bias)
    d.dmodel, d.heads, d.tmax, d.q_scale = D, H, TMAX, 0.125
    d.step, d.qbuf, d.kc, d.vc = E.ptr(step), E.ptr(q), E.ptr(kc), E.ptr(vc)
    E.check(lib.tt_op_gemm_ex(dt, 2, C.byref(d), None, None))


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("B", [16, 256, 272])
@pytest.mark.parametrize("P1", [1, 59, 64, 130])
def test_fused_operator_equals_the_two_launches_bit_for_bit(lib, name, dt, tdt, tol, B, P1):
    """Own keys after the step: 1 (no key in the cache yet), 7 / 8 / 9 (the 8-row V sub-rows), 63 / 64 / 65 (the 64-key score slots and the
    two-slot prefetch), 100 (the benchmark's mean), 199 / 200 (its last steps), 207 / 208 (capacity - 1 and the capacity itself: the new
    row goes into the last slot).  P1 = 1 / 59 / 64 / 130: one prefix key, the benchmark's prefix, a full staging slot, three slots.
    B = 16 one workgroup group, 256 the benchmark, 272 one group more than the chip has CUs."""
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + P1)
    W = (torch.randn(3 * D, D, device="cuda", generator=g) / math.sqrt(D) * 2).to(tdt)
    bias = torch.randn(3 * D, device="cuda", generator=g) * 0.5
    kp = (torch.randn(H, P1, 64, device="cuda", generator=g) * 2).to(tdt)
    vp = torch.randn(H, P1, 64, device="cuda", generator=g).to(tdt)
    for tgen in (1, 7, 8, 9, 63, 64, 65, 100, 199, 200, TMAX - 1, TMAX):
        h = torch.randn(B, D, device="cuda", generator=g).to(tdt)
        # slots >= tgen - 1 hold NaN on purpose: the launch writes slot tgen - 1 and nothing of a slot beyond the valid ones may reach
        # the output, not even under a zero weight (own keys = 1: no valid slot at all before the call)
        kc0 = torch.full((B, H, 8, TMAX, 8), float("nan"), device="cuda").to(tdt)
        vc0 = torch.full((B, H, TMAX, 64), float("nan"), device="cuda").to(tdt)
        kc0[:, :, :, :tgen - 1] = (torch.randn(B, H, 8, tgen - 1, 8, device="cuda", generator=g) * 2).to(tdt)
        vc0[:, :, :tgen - 1] = torch.randn(B, H, tgen - 1, 64, device="cuda", generator=g).to(tdt)
        step = torch.tensor([tgen - 1], device="cuda", dtype=torch.int32)
        # the two launches
        kc_a, vc_a = kc0.clone(), vc0.clone()
        q_a = torch.zeros(B, D, device="cuda", dtype=tdt)
        out_a = torch.zeros(B, D, device="cuda", dtype=tdt)
        _qkv_decode_gemm(lib, dt, h, W, bias, step, q_a, kc_a, vc_a, B)
        E.check(lib.tt_op_decode_attention(dt, E.ptr(q_a), E.ptr(kp), E.ptr(vp), P1, E.ptr(kc_a), E.ptr(vc_a), TMAX, tgen, E.ptr(out_a), B, H, 0, None))
        # the one launch
        kc_b, vc_b = kc0.clone(), vc0.clone()
        q_b = torch.zeros(B, D, device="cuda", dtype=tdt)
        out_b = torch.zeros(B, D, device="cuda", dtype=tdt)
        E.check(lib.tt_op_decode_qkv_attention(dt, E.ptr(h), E.ptr(W), E.ptr(bias), 0.125, E.ptr(kp), E.ptr(vp), P1, E.ptr(kc_b), E.ptr(vc_b),
                                               TMAX, tgen, E.ptr(q_b), E.ptr(out_b), B, H, None))
        torch.cuda.synchronize()
        where = f"{name} B={B} P1={P1} own keys={tgen}"
        assert torch.equal(q_b, q_a), f"query rows differ from the QKV GEMM's: {where}"
        # (bit patterns: the untouched slots are NaN, which torch.equal would call different from itself)
        assert torch.equal(kc_b.view(torch.int16), kc_a.view(torch.int16)), f"K cache differs after the call: {where}"
        assert torch.equal(vc_b.view(torch.int16), vc_a.view(torch.int16)), f"V cache differs after the call: {where}"
        assert torch.isfinite(kc_b[:, :, :, :tgen].float()).all() and torch.isfinite(vc_b[:, :, :tgen].float()).all()
        assert torch.isfinite(out_b.float()).all()
        assert torch.equal(out_b, out_a), f"attention rows differ from the two launches': {where}"
        # torch fp32.  The projection from the rounded operands (one rounding to T of an f32 sum of 1024 products) ...
        ref = h.float() @ W.float().t() + bias
        k_new = kc_b[:, :, :, tgen - 1].reshape(B, H * 64).float()
        v_new = vc_b[:, :, tgen - 1].reshape(B, H * 64).float()
        report(f"fused q {where}", q_b.float(), ref[:, :D] * 0.125, ATTN_TOL[name])
        report(f"fused k {where}", k_new, ref[:, D:2 * D], ATTN_TOL[name])
        report(f"fused v {where}", v_new, ref[:, 2 * D:], ATTN_TOL[name])
        # ... and the attention from the rounded q / k / v the launch produced, at the decode-attention operator's bars
        k_own = kc_b[:, :, :, :tgen].permute(0, 1, 3, 2, 4).reshape(B, H, tgen, 64).float()
        v_own = vc_b[:, :, :tgen].float()
        want = _decode_attention_reference(q_b.float().reshape(B, H, 64), kp.float(), vp.float(), k_own, v_own).reshape(B, D)
        report(f"fused decode attention {where}", out_b.float(), want, ATTN_TOL[name])


def test_operator_refuses_what_does_not_fit(lib):
    """A prefix whose staging + score rows exceed the LDS, a batch that is not a multiple of 16 and fp32 operands are errors, not fall-backs."""
    tdt = torch.bfloat16
    B, P1, tmax = 16, 402 + 40, 608
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=tdt)  # noqa: E731
    args = lambda b, p1, dt=E.TT_BF16: (dt, E.ptr(z(b, D)), E.ptr(z(3 * D, D)), None, 0.125, E.ptr(z(H, p1, 64)), E.ptr(z(H, p1, 64)), p1,  # noqa: E731
                                        E.ptr(z(b, H, 8, tmax, 8)), E.ptr(z(b, H, tmax, 64)), tmax, 1, None, E.ptr(z(b, D)), b, H, None)
    assert lib.tt_op_decode_qkv_attention(*args(B, P1)) != 0 and b"LDS" in lib.tt_last_error()
    assert lib.tt_op_decode_qkv_attention(*args(24, 59)) != 0
    assert lib.tt_op_decode_qkv_attention(*args(16, 59, E.TT_F32)) != 0
    assert lib.tt_op_decode_qkv_attention(*args(16, 59)) == 0
    torch.cuda.synchronize()


def _stage(sds, dt, B, new, max_text=80):
    return stages.ArStage(sds["autoregressive"], ARConfig(), dtype=dt, max_batch=B, max_text=max_text, max_new_tokens=new, max_latent_candidates=1)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_codes_do_not_depend_on_the_option(sds, name, dt, tdt, tol):
    """256 candidates x 200 tokens: option on (six launches per layer) and off (seven), kept graph and eager launches, one handle."""
    cfg = ARConfig()
    text, auto, _ = GF.prompt()
    st = _stage(sds, dt, 256, 200)
    runs = {}
    try:
        for replay in (1, 0):
            E.load_library().tt_graph_replay(replay)
            for opt in (1, 0, 1):
                st.set_option(E.TT_AR_OPT_FUSED_QKV_ATTN, opt)
                st.prefill(auto, text)
                codes, n = st.generate(256, 200, seed=77)
                assert st.stat(2) == (6 if opt else 7) * cfg.layers + 4
                runs.setdefault((replay, opt), []).append((codes.clone(), n))
    finally:
        E.load_library().tt_graph_replay(1)
    base, n0 = runs[(1, 0)][0]
    assert n0 == 200
    for key, lst in runs.items():
        for codes, n in lst:
            assert n == n0 and torch.equal(codes, base), f"codes differ from the two-launch graph run: graph replay={key[0]} option={key[1]} ({name})"
    assert st.stat(1) == 0
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_a_row_has_the_same_logits_at_256_and_at_64(sds, name, dt, tdt, tol):
    """Teacher-forced: B = 256 takes the one launch, B = 64 the QKV GEMM (64 x 16 tiles) + the decode attention; a row's logits are the same bits."""
    cfg = ARConfig()
    text, auto, _ = GF.prompt()
    toks = GF.arl_tokens()
    check = (1, 2, 63, 64, 65, 66)
    st = _stage(sds, dt, 256, 72)
    got = {}
    for B in (256, 64):
        st.prefill(auto, text)
        st.begin(B)
        assert st.stat(2) == (6 if B == 256 else 7) * cfg.layers + 4
        for s in range(max(check)):
            st.decode_step(toks[s].repeat(B // GF.ARL_B))
            if s + 1 in check:
                got[(B, s + 1)] = st.logits(B)[:64].clone()
    for n in check:
        assert torch.isfinite(got[(256, n)]).all()
        assert torch.equal(got[(256, n)], got[(64, n)]), f"logits after {n} fed tokens differ between B = 256 and B = 64 ({name})"
    st.close()


@torch.no_grad()
def test_the_rule_keeps_other_batches_on_seven_launches(sds):
    """tt_ar_stat(h, 2) on the handle of tests/test_gpu_r6.py::test_full_width_decode_at_the_benchmarked_contexts (B = 256: one launch, B = 96:
    two), with two utterances per batch, with a prefix too long for the LDS next to the score and activation rows, and in fp32."""
    cfg = ARConfig()
    L = cfg.layers
    text, auto, _ = GF.prompt()
    st = _stage(sds, E.TT_BF16, 256, 508)
    st.prefill(auto, text)
    st.begin(256)
    assert st.stat(2) == 6 * L + 4
    st.begin(96)
    assert st.stat(2) == 7 * L + 4
    st.begin(128)
    assert st.stat(2) == 7 * L + 4
    st.close()
    # two utterances of 128 candidates
    st = stages.ArStage(sds["autoregressive"], cfg, dtype=E.TT_BF16, max_batch=256, max_text=80, max_new_tokens=32, max_latent_candidates=1, max_groups=2)
    st.prefill_group(0, 2, auto, text)
    st.prefill_group(1, 2, auto, text[:, :40])
    codes, n = st.generate(256, 8, seed=3)
    assert n == 8 and st.stat(2) == 7 * L + 4
    st.close()
    # a 400-token text: K + V staging alone is ~110 KB, with 16 score rows of 600 + 440 floats it does not fit 160 KB
    st = _stage(sds, E.TT_BF16, 256, 600, max_text=402)
    long_text = torch.randint(1, cfg.number_text_tokens, (1, 400), dtype=torch.int32)
    st.prefill(auto, long_text)
    codes, n = st.generate(256, 4, seed=3)
    assert n == 4 and st.stat(2) == 7 * L + 4
    st.close()
    st = _stage(sds, E.TT_F32, 256, 32)
    st.prefill(auto, text)
    st.begin(256)
    assert st.stat(2) == 7 * L + 4
    st.close()


@pytest.mark.parametrize("rows,top_k,extra", [(4, 50, 0), (16, 50, 0), (16, 300, 1)])
@torch.no_grad()
def test_session_handles_keep_seven_launches(sds, rows, top_k, extra):
    """A session handle (TT_AR_OPT_SESSIONS = 1 at <= 4 rows, 2 = the wide form at 16) with TT_AR_OPT_FUSED_QKV_ATTN switched on explicitly
    keeps the two-launch layer: tt_ar_stat(h, 2) = 7 * layers + 4, plus the full-sort sampler's launch where a row's top_k needs it."""
    cfg = ARConfig()
    text, auto, _ = GF.prompt()
    st = stages.ArStage(sds["autoregressive"], cfg, dtype=E.TT_BF16, max_batch=rows, max_text=80, max_new_tokens=32, max_latent_candidates=1, sessions=True)
    st.set_option(E.TT_AR_OPT_FUSED_QKV_ATTN, 1)
    assert st.stat(2) == 7 * cfg.layers + 4
    st.admit(0, auto, text, 5)
    st.admit(rows - 1, auto, text[:, :40], 6)
    n_total, finished = st.advance(3, top_k=top_k)
    assert n_total[0] == 3 and n_total[rows - 1] == 3
    assert st.stat(2) == 7 * cfg.layers + 4 + extra
    st.set_option(E.TT_AR_OPT_FUSED_QKV_ATTN, 0)
    assert st.stat(2) == 7 * cfg.layers + 4 + extra
    st.close()


@torch.no_grad()
def test_two_full_rounds_of_workgroups_take_the_launch_with_the_same_codes(sds):
    """512 candidates = two full rounds of 16-sequence workgroups on 256 CUs: measured ahead (profiles/r16_ab_fused_qkv_attn.txt), so the rule
    takes the one launch there too; 496 and 528 (a partly filled round) keep two."""
    cfg = ARConfig()
    text, auto, _ = GF.prompt()
    st = _stage(sds, E.TT_BF16, 528, 72)
    codes = {}
    for opt in (1, 0):
        st.set_option(E.TT_AR_OPT_FUSED_QKV_ATTN, opt)
        st.prefill(auto, text)
        codes[opt], n = st.generate(512, 70, seed=9)
        assert n == 70 and st.stat(2) == (6 if opt else 7) * cfg.layers + 4
    assert torch.equal(codes[1], codes[0])
    st.set_option(E.TT_AR_OPT_FUSED_QKV_ATTN, 1)
    for B in (496, 528):
        st.begin(B)
        assert st.stat(2) == 7 * cfg.layers + 4
    st.close()
