"""-m gpu: ragged batches of the HiFi-GAN decoder (include/tortoise_mi355x_hifi.h, csrc/hifigan.hip) and the fast-path calls built on them.

Every sequence of a batched pass must be bit-identical to decoding it alone: the masked tap convolution equals one launch per sequence,
HifiganStage.inference_many equals inference() per item, tts_many equals tts() per text, read_long_form on the fast path equals tts() per
chunk, and stream_pieces' batched vocoder call keeps the pieces of tts_stream.
"""
import math

import pytest
import torch

from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ARConfig, HifiganConfig
from tests.gpu_util import DTYPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_masked_tap_conv_equals_per_sequence_launches(lib, name, dt, tdt, tol):
    """tt_op_gemm_segv over padded slots (taps 2 / 3 / 7 / 11, dilations 1 / 3 / 5, lengths 1 and shorter than the tap reach among them, the
    last slot cut at its valid rows) is torch.equal, row for row, to tt_op_gemm on each sequence alone."""
    g = torch.Generator().manual_seed(7)
    C, N = 128, 192
    for taps in (2, 3, 7, 11):
        for dil in ((1,) if taps == 2 else (1, 3, 5)):
            lens = [1, 2, taps * dil // 2, 37, 150, 5]
            P = max(lens) + 3
            n = len(lens)
            M = (n - 1) * P + lens[-1]
            A = torch.randn(n * P, C, generator=g).to(tdt).cuda()
            Wt = (torch.randn(N, taps * C, generator=g) / math.sqrt(taps * C)).to(tdt).cuda()
            bias = torch.randn(N, generator=g).cuda()
            res = torch.randn(n * P, N, generator=g).cuda()
            vlen = torch.tensor(lens, dtype=torch.int32).cuda()
            out = torch.zeros(M, N, device="cuda")
            out_t = torch.zeros(M, N, device="cuda", dtype=tdt)
            E.check(lib.tt_op_gemm_segv(dt, E.ptr(A), C, E.ptr(Wt), taps * C, M, N, taps * C, taps, dil, P, E.ptr(vlen), E.ptr(bias), E.ACT_LRELU,
                                        E.ptr(res), E.ptr(out), E.ptr(out_t), None))
            for b, L in enumerate(lens):
                a1 = A[b * P:b * P + L].contiguous()
                r1 = res[b * P:b * P + L].contiguous()
                o1 = torch.zeros(L, N, device="cuda")
                t1 = torch.zeros(L, N, device="cuda", dtype=tdt)
                # (tt_op_gemm has no dilation argument: a dilated tap conv alone is the same launch with the seq_vlen of one sequence)
                one = torch.tensor([L], dtype=torch.int32).cuda()
                if dil == 1:
                    E.check(lib.tt_op_gemm(dt, E.ptr(a1), C, E.ptr(Wt), taps * C, L, N, taps * C, taps, L, 1, E.ptr(bias), E.ACT_LRELU, E.ptr(r1),
                                           E.ptr(o1), E.ptr(t1), None))
                else:
                    E.check(lib.tt_op_gemm_segv(dt, E.ptr(a1), C, E.ptr(Wt), taps * C, L, N, taps * C, taps, dil, L, E.ptr(one), E.ptr(bias),
                                                E.ACT_LRELU, E.ptr(r1), E.ptr(o1), E.ptr(t1), None))
                got, got_t = out[b * P:b * P + L], out_t[b * P:b * P + L]
                assert torch.equal(got, o1) and torch.equal(got_t, t1), f"{name} taps={taps} dil={dil}: sequence {b} ({L} rows) differs"
            # against torch: zero padding at each sequence's own ends
            for b, L in enumerate(lens):
                x = A[b * P:b * P + L].float().t()[None]
                w = Wt.float().reshape(N, taps, C).permute(0, 2, 1)
                ref = torch.nn.functional.conv1d(x, w, padding=(taps // 2) * dil, dilation=dil)[0, :, :L].t() if taps % 2 else None
                if ref is not None:
                    ref = torch.nn.functional.leaky_relu(ref + bias, 0.2) + res[b * P:b * P + L]
                    err = float((out[b * P:b * P + L] - ref).abs().max() / (ref.abs().max() + 1e-6))
                    assert err < 1e-3, f"{name} taps={taps} dil={dil} sequence {b}: rel err {err}"


def _hifi(dt, max_latents):
    cfg = HifiganConfig()
    sd = W.fold_weight_norm(W.synthetic_state_dict(W.hifigan_manifest(cfg), seed=31))
    return cfg, stages.HifiganStage(sd, cfg, dtype=dt, max_latents=max_latents)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_inference_many_equals_inference_alone(name, dt, tdt, tol):
    """Ragged full-width batches (1, 7, 60, 96 latents, mixed, and more than one call's capacity), each sequence with its own g: every
    wav is torch.equal to inference() of that sequence alone."""
    cfg, st = _hifi(dt, 128)
    gen = torch.Generator().manual_seed(32)
    lengths = [1, 7, 60, 96, 60, 3, 96, 60, 60, 7, 1, 33]
    items = [(torch.randn(1, T, cfg.in_channels, generator=gen), torch.randn(1, cfg.cond_channels, generator=gen) * 0.5) for T in lengths]
    groups = st.batch_groups(lengths)
    assert sorted(i for grp in groups for i in grp) == list(range(len(lengths)))
    assert len(groups) > 1 and max(len(grp) for grp in groups) > 1  # (the capacity splits the batch, and batches do form)
    got = st.inference_many(items)
    for i, (lat, g) in enumerate(items):
        want = st.inference(lat, g)
        assert got[i].shape == want.shape and torch.equal(got[i], want), f"{name}: sequence {i} ({lengths[i]} latents) differs from alone"
    # one group of equal lengths and a 1-item call
    same = items[2:3] + items[4:5] + items[7:9]
    for (lat, g), w in zip(same, st.inference_many(same)):
        assert torch.equal(w, st.inference(lat, g))
    assert torch.equal(st.inference_many(items[:1])[0], st.inference(*items[0]))
    st.close()


def _fast_instances(dtype, max_streams, **kw):
    from tortoise_tts_amd.api_fast import TextToSpeech
    a_cfg, h_cfg = ARConfig(), HifiganConfig()
    sds = {"autoregressive": W.synthetic_state_dict(W.ar_manifest(a_cfg), 1234), "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    return TextToSpeech(state_dicts=sds, dtype=dtype, max_mel_tokens=64, kv_cache=True, max_streams=max_streams, **kw)


def _texts(n=20):
    from tests.test_gpu_wide_sessions import _sessions
    s = _sessions(n)
    return [t for _, _, t, _, _, _ in s], [seed for _, _, _, seed, _, _ in s], s[0][1]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@torch.no_grad()
def test_tts_many_on_session_instances_equals_tts(dtype):
    """tts_many over 20 texts on a max_streams=3 instance and on a 16-wide one (texts wait for rows, rows end at different steps) is
    torch.equal per clip to tts() alone on a max_streams=1 instance; so is the max_streams=1 loop itself."""
    texts, seeds, cond = _texts()
    kw = dict(conditioning_latents=(cond,), max_mel_tokens=48)
    one = _fast_instances(dtype, 1)
    want = [one.tts(t, use_deterministic_seed=s, **kw) for t, s in zip(texts, seeds)]
    got1 = one.tts_many(texts[:3], use_deterministic_seed=seeds[:3], **kw)
    assert all(torch.equal(a, b) for a, b in zip(got1, want[:3]))
    del one
    for streams, wide in ((3, False), (16, True)):
        many = _fast_instances(dtype, streams, wide_sessions=wide)
        got = many.tts_many(texts, use_deterministic_seed=seeds, **kw)
        assert len(got) == len(texts)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and torch.equal(a, b), f"{dtype} max_streams={streams}: text {i} differs from tts() alone"
        assert not many._sessions
        del many


@torch.no_grad()
def test_read_long_form_fast_path_equals_per_chunk_tts():
    """read_long_form with a fast-path instance: every part is torch.equal to tts() of that chunk with the agreed seed."""
    from tortoise_tts_amd.longform import read_long_form
    texts, _, cond = _texts(5)
    one = _fast_instances("bf16", 1)
    want = [one.tts(t, use_deterministic_seed=77, conditioning_latents=(cond,), max_mel_tokens=40) for t in texts]
    del one
    wide = _fast_instances("bf16", 4, wide_sessions=True)
    full, parts = read_long_form(wide, texts, texts_are_chunks=True, conditioning_latents=(cond,), seed=77, max_mel_tokens=40)
    assert len(parts) == len(texts) and all(torch.equal(a, b) for a, b in zip(parts, want))
    assert torch.equal(full, torch.cat([p.squeeze(0) for p in want], dim=-1))
