"""The wav2vec2 redaction aligner on the MI355X (csrc/align.hip, include/tortoise_mi355x_align.h): its new kernels against torch fp32, the
whole model at the reference checkpoint's architecture (24 x 1024, 16 heads) against transformers.Wav2Vec2ForCTC in fp32, and redaction end to
end against the transcription of wav2vec_alignment.py (tests/w2v_reference.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import w2v_reference as R
from tortoise_tts_amd import align
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _source(model, cfg):
    return cfg, {k: v.detach().cpu() for k, v in model.state_dict().items()}, R.VOCAB, R.TOK_CFG


@torch.no_grad()
def test_resample_kernel_matches_torchaudio_transcription():
    lib = E.init()
    taps = align.resample_taps().to(DEV)
    for S in (1, 2, 3, 601, 24000, 24001, 223201):
        x = R.test_clip(S / 24000.0, seed=S)[0, :S].contiguous()
        if x.shape[0] < S:
            x = F.pad(x, (0, S - x.shape[0]))
        want = R.resample(x[None].double()).float()[0]
        xd = x.to(DEV)
        y = torch.empty(align.resampled_length(S), device=DEV)
        stats = torch.empty(2, device=DEV)
        ws = torch.empty(lib.tt_op_w2v_resample_workspace(S), dtype=torch.uint8, device=DEV)
        E.check(lib.tt_op_w2v_resample(E.ptr(xd), S, E.ptr(taps), E.ptr(y), E.ptr(stats), E.ptr(ws), E.stream_ptr()))
        assert y.shape == want.shape
        assert float((y.cpu() - want).abs().max()) < 2e-6 * max(1.0, float(want.abs().max()))
        if S > 1:
            yd = want.double()
            assert abs(float(stats[0]) - float(yd.mean())) < 1e-6
            assert abs(float(stats[1]) - float(1 / torch.sqrt(yd.var() + 1e-7))) < 1e-4 * float(1 / torch.sqrt(yd.var() + 1e-7))


@torch.no_grad()
@pytest.mark.parametrize("dt,tol", [(E.TT_F32, 2e-6), (E.TT_F16, 2e-3), (E.TT_BF16, 1.5e-2)])
def test_conv0_layernorm_gelu_kernels(dt, tol):
    lib = E.init()
    g = torch.Generator().manual_seed(3)
    N = 40011
    y = torch.randn(N, generator=g) * 0.3 + 0.1
    stats = torch.tensor([float(y.mean()), float(1 / torch.sqrt(y.var() + 1e-7))])
    w, b = torch.randn(512, 10, generator=g) * 0.3, torch.randn(512, generator=g) * 0.1
    ga, be = 1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    xn = (y - stats[0]) * stats[1]
    want = F.gelu(F.layer_norm(F.conv1d(xn[None, None], w[:, None], b, stride=5)[0].t(), (512,), ga, be, 1e-5))
    Fr = want.shape[0]
    d = {k: v.to(DEV).contiguous() for k, v in dict(y=y, stats=stats, w=w, b=b, ga=ga, be=be).items()}
    tdt = {E.TT_F32: torch.float32, E.TT_F16: torch.float16, E.TT_BF16: torch.bfloat16}[dt]
    out_t = torch.empty(Fr, 512, device=DEV, dtype=tdt)
    out32 = torch.empty(Fr, 512, device=DEV)
    E.check(lib.tt_op_w2v_conv0(dt, E.ptr(d["y"]), E.ptr(d["stats"]), Fr, 10, 5, E.ptr(d["w"]), E.ptr(d["b"]), E.ptr(d["ga"]), E.ptr(d["be"]),
                                E.ptr(out_t), E.ptr(out32), E.stream_ptr()))
    assert _rel(out32, want) < 2e-6 and _rel(out_t.float(), want) < tol
    # LayerNorm + GELU in one row-norm launch (the strided convolutions' epilogue), wave-per-row and block-per-row forms
    for M in (300, 4096):
        x = torch.randn(M, 512, generator=g) * 2 + 0.5
        want = F.gelu(F.layer_norm(x, (512,), ga, be, 1e-5))
        xd = x.to(DEV)
        o_t = torch.empty(M, 512, device=DEV, dtype=tdt)
        o32 = torch.empty(M, 512, device=DEV)
        E.check(lib.tt_op_layernorm_act(dt, E.ptr(xd), M, 512, E.ptr(d["ga"]), E.ptr(d["be"]), 1e-5, E.ACT_GELU_ERF, E.ptr(o_t), E.ptr(o32),
                                        E.stream_ptr()))
        assert _rel(o32, want) < 2e-6 and _rel(o_t.float(), want) < tol


@torch.no_grad()
def test_argmax_kernel_ties_go_to_the_lowest_index():
    lib = E.init()
    g = torch.Generator().manual_seed(4)
    T, V, ld = 1000, 45, 64
    lg = torch.randn(T, ld, generator=g).round()  # many ties
    lg[:, V:] = 100.0  # padding columns are never read
    d = lg.to(DEV)
    ids = torch.empty(T, dtype=torch.int32, device=DEV)
    out = torch.empty(T, V, device=DEV)
    E.check(lib.tt_op_w2v_argmax(E.ptr(d), ld, T, V, E.ptr(ids), E.ptr(out), E.stream_ptr()))
    assert torch.equal(ids.cpu().long(), lg[:, :V].argmax(-1)) and torch.equal(out.cpu(), lg[:, :V])


@pytest.fixture(scope="module")
def large():
    cfg = R.large_config()
    model = R.hf_model(cfg, seed=11).to(DEV)
    return cfg, model


LARGE_TOL = {E.TT_F32: 1e-5, E.TT_F16: 1e-3, E.TT_BF16: 6e-3}  # measured: 5e-7, 1.7e-4, 1.5e-3 (random weights, 1 - 23 s clips)


@torch.no_grad()
def test_full_model_at_the_reference_architecture(large):
    """Logits of the device stage against Wav2Vec2ForCTC fp32 on clips of 1 s, 9.3 s and 23 s; frame-argmax agreement; every disagreeing
    frame has a small fp32 top-2 margin."""
    cfg, model = large
    src = _source(model, cfg)
    clips = {s: R.test_clip(s, seed=int(s * 10)) for s in (1.0, 9.3, 23.0)}
    want = {s: R.model_logits(model, c.to(DEV)).float().cpu() for s, c in clips.items()}
    for dt in (E.TT_F32, E.TT_F16, E.TT_BF16):
        st = stages.AlignerStage(src, DEV, dt, max_samples=24000 * 24)
        for s, c in clips.items():
            ids, lg = st.run(c, logits=True)
            w = want[s]
            assert lg.shape == w.shape, (lg.shape, w.shape)
            r = _rel(lg, w)
            top2 = w.topk(2, dim=-1).values
            margin = top2[:, 0] - top2[:, 1]
            wid = w.argmax(-1)
            dis = (ids.cpu().long() != wid)
            spread = float(w.std())
            print(f"[parity] w2v {E.DTYPE_NAMES[dt]} {s:.1f} s ({w.shape[0]} frames): rel_l2={r:.3e} argmax agree {1 - float(dis.float().mean()):.4f} "
                  f"({int(dis.sum())} frames, max fp32 margin there {float(margin[dis].max()) if dis.any() else 0.0:.3e}; logit std {spread:.2f})")
            assert r < LARGE_TOL[dt], (E.DTYPE_NAMES[dt], s, r)
            assert torch.equal(ids.cpu().long(), lg.cpu().argmax(-1))
            if dis.any():
                assert float(margin[dis].max()) < 8 * LARGE_TOL[dt] * spread
            assert st.guard() == 0
        st.close()


@torch.no_grad()
def test_redact_end_to_end_fp32_is_bit_identical_to_the_transcription(large):
    cfg, model = large
    st = stages.AlignerStage(_source(model, cfg), DEV, E.TT_F32, max_samples=24000 * 24)
    for s in (9.3, 23.0):
        clip = R.test_clip(s, seed=int(s * 10) + 1)
        logits = R.model_logits(model, clip.to(DEV)).float().cpu()
        pred = st.tokenizer.decode(logits.argmax(-1).tolist())
        assert len(pred) >= 6, pred
        text = R.text_from_prediction(pred)
        ids = st.frame_ids(clip)
        assert ids == logits.argmax(-1).tolist()
        want = R.redact(clip, text, lambda a: logits, st.tokenizer)
        got = align.redact(clip, text, st.frame_ids, st.tokenizer)
        assert 0 < got.shape[-1] < clip.shape[-1] and torch.equal(got, want)
    st.close()


class _IdsTokenizer:
    """The text front-end stand-in of this test: every text speaks the same synthetic ids (what bench.py renders)."""

    def __init__(self, ids):
        self.ids = ids

    def encode(self, text):
        return self.ids


@torch.no_grad()
def test_tts_with_brackets_on_the_device():
    """A reduced tts() with a bracketed text: every returned clip is the transcription's redact of the enable_redaction=False render of the
    same seed, aligned with the stage's own frame ids; timings gain redact_s."""
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    sds = bench.synthetic_weights()
    ids, _ = bench.synthetic_prompt()
    cfg = R.small_config()
    model = R.hf_model(cfg, seed=5)
    tts = TextToSpeech(state_dicts=sds, max_candidates=16, max_mel_tokens=48, aligner=_source(model, cfg))
    tts._tokenizer = _IdsTokenizer(ids.tolist())
    text = "[I am so sad,] hello there"
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    tts.enable_redaction = False
    plain = tts.tts(text, k=2, **kw)
    tts.enable_redaction = True
    got = tts.tts(text, k=2, **kw)
    assert tts.aligner is not None and "redact_s" in tts.timings
    for p, g_ in zip(plain, got):
        want = R.redact(p[0], text, lambda a: tts.aligner.run(a).cpu().long(), tts.aligner.tokenizer)[None]
        assert g_.shape[-1] < p.shape[-1] and torch.equal(g_, want)
