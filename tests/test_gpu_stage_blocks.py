"""-m gpu: the model stages at the smallest shapes at which a mis-assembled launch sequence shows (csrc/stage_blocks.h: the norm argument
blocks, the head-split attention pair, the AttentionBlock, the stride-2 convolution front, the pooled-latent tail, the guard reader).
Every case drives a public stage class with synthetic weights at the reduced configurations of oracle/make_golden.py and compares with the
oracle on the same operand-rounded weights, under the measure and tolerance the stage's own test already holds it to for that operand type:
  CLVP          relative L2 of the scores, 2 x tests.gpu_util.DTYPES              (tests/test_gpu_stages.py::test_clvp)
  CVVP          max abs of the scores, tests/test_gpu_cvvp.py MODES                (test_cvvp_scores)
  conditioning  relative L2 of the latent, tests.gpu_util.DTYPES                   (test_conditioning_encoders)
  aligner       relative L2 of the logits, tests/test_gpu_redaction.py LARGE_TOL   (test_full_model_at_the_reference_architecture)
  diffusion     relative L2, tests.gpu_util.DTYPES (x 2 for the sampled mel)       (test_diffusion)
Invariances (a candidate alone / in its batch, an utterance alone / in a padded batch, captured / eager sampler steps) are torch.equal."""
import pytest
import torch

from oracle import make_golden as G
from oracle import tortoise_oracle as O
from tests import w2v_reference as R
from tests.gpu_util import DTYPES, quantize_sd, report
from tests.test_gpu_cvvp import MODES as CVVP_MODES
from tests.test_gpu_redaction import LARGE_TOL as W2V_TOL
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ARConfig, CLVPConfig, CVVPConfig, DiffusionConfig
from tortoise_tts_amd.schedule import Schedule

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_clvp_shortest_candidates_and_a_key_block_crossing(name, dt, tdt, tol):
    """n = 8 codes (the minimum; padded to 32 keys) and n = 33 (two key blocks), one and three candidates; a candidate scores the same
    bits alone as inside its batch."""
    cfg = CLVPConfig(**G.CLVP_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.clvp_manifest(cfg), seed=G.CLVP_SEED), tdt)
    text, _ = G.clvp_inputs()
    g = torch.Generator().manual_seed(41)
    st = stages.ClvpStage(sd, cfg, dtype=dt, max_rows=256)
    for n in (8, 33):
        codes = torch.randint(0, 8192, (3, n), generator=g)
        want = O.clvp_score(sd, cfg, text.repeat(3, 1), codes)
        batch = st.score(text, codes)
        report(f"CLVP {name} n={n} B=3 vs oracle", batch, want, tol * 2)
        alone = [st.score(text, codes[b:b + 1]) for b in range(3)]
        # (the measure of test_clvp is relative to the norm of the score VECTOR - a cosine similarity near zero has no relative error
        # of its own - so the three B = 1 calls are held to it together)
        report(f"CLVP {name} n={n} three B=1 calls vs oracle", torch.cat(alone), want, tol * 2)
        for b in range(3):
            assert torch.equal(alone[b], batch[b:b + 1]), f"n={n}: candidate {b} alone scores other bits than inside the batch"
    assert st.guard() == 0
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", CVVP_MODES)
@torch.no_grad()
def test_cvvp_shortest_clips(name, dt, tdt, tol):
    """T = 29 mel frames (the minimum: 29 -> 15 -> 8 rows through the two stride-2 convolutions) and T = 30 (an even length), n = 8 codes,
    one and three candidates, one and two clips."""
    cfg = CVVPConfig(**G.CVVP_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.cvvp_manifest(cfg), seed=G.CVVP_SEED), tdt)
    g = torch.Generator().manual_seed(43)
    st = stages.CvvpStage(sd, cfg, dtype=dt, max_rows=64, max_cond_frames=32)
    for T, clips, B in ((29, 1, 1), (29, 2, 3), (30, 1, 3), (30, 2, 1)):
        mels = torch.randn(1, clips, 80, T, generator=g) * 2 - 5
        codes = torch.randint(0, 8192, (B, 8), generator=g)
        got = st.score(mels, codes).cpu()
        err = float((got - O.cvvp_score(sd, cfg, mels, codes)).abs().max())
        print(f"[parity] CVVP {name} T={T} clips={clips} B={B} n=8: max abs vs oracle {err:.2e} (tol {tol:.0e})")
        assert err < tol
    assert st.guard() == 0
    st.close()


def _cond_stage(d_cfg, dt):
    a_cfg = ARConfig(**G.AR_CFG)
    a_sd = W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.COND_SEED)
    d_sd = W.synthetic_state_dict(W.diffusion_manifest(d_cfg), seed=G.COND_SEED + 1)
    return a_cfg, a_sd, d_sd, stages.ConditioningStage(a_sd, d_sd, a_cfg, d_cfg, dtype=dt, max_frames=160)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_conditioning_encoders_shortest_and_odd_clips(name, dt, tdt, tol):
    """AR encoder (64-wide heads: the flash path) at T = 1 and T = 33; diffusion embedder (128-wide heads with relative positions: the
    wave-per-query kernel) at T = 4 (one frame after both convolutions) and T = 67 (odd lengths at both convolutions: 67 -> 34 -> 17)."""
    d_cfg = DiffusionConfig(**G.DIFF_CFG)
    a_cfg, a_sd, d_sd, st = _cond_stage(d_cfg, dt)
    assert (2 * d_cfg.model_channels) // d_cfg.num_heads == 128 and any("relative_attention_bias" in k for k in d_sd if k.startswith("contextual_embedder."))
    g = torch.Generator().manual_seed(47)
    for T in (1, 33):
        mel = torch.randn(1, 1, 80, T, generator=g)
        report(f"conditioning auto latent {name} T={T} vs oracle", st.auto_latent(mel).cpu(), O.ar_get_conditioning(quantize_sd(a_sd, tdt), a_cfg, mel), tol)
    for T in (4, 67):
        mel = torch.randn(1, 1, 100, T, generator=g)
        report(f"conditioning diffusion latent {name} T={T} vs oracle", st.diffusion_latent(mel).cpu(),
               O.diffusion_get_conditioning(quantize_sd(d_sd, tdt), d_cfg, mel), tol)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_conditioning_embedder_with_64_wide_heads_and_relative_positions(name, dt, tdt, tol):
    """A reduced embedder whose AttentionBlocks have 64-wide heads (256 channels, 4 heads) AND a relative-position table: the flash path
    with the additive bias, which neither reference configuration reaches through the conditioning stage."""
    d_cfg = DiffusionConfig(**dict(G.DIFF_CFG, num_heads=4))
    a_cfg, a_sd, d_sd, st = _cond_stage(d_cfg, dt)
    assert (2 * d_cfg.model_channels) // d_cfg.num_heads == 64 and any("relative_attention_bias" in k for k in d_sd if k.startswith("contextual_embedder."))
    g = torch.Generator().manual_seed(53)
    for T in (4, 67, 150):  # 150 -> 38 frames: two key blocks
        mel = torch.randn(1, 1, 100, T, generator=g)
        report(f"conditioning diffusion latent, 64-wide heads {name} T={T} vs oracle", st.diffusion_latent(mel).cpu(),
               O.diffusion_get_conditioning(quantize_sd(d_sd, tdt), d_cfg, mel), tol)
    st.close()


@pytest.fixture(scope="module")
def w2v_small():
    cfg = R.small_config()
    model = R.hf_model(cfg, seed=5)
    return (cfg, {k: v.detach().cpu() for k, v in model.state_dict().items()}, R.VOCAB, R.TOK_CFG), model


@pytest.mark.parametrize("dt", [E.TT_BF16, E.TT_F16])
@torch.no_grad()
def test_aligner_one_frame_and_33_frames(w2v_small, dt):
    """The shortest clip tt_w2v_frames maps to one frame (one query, one key) and the shortest that maps to 33 frames (two key blocks)."""
    source, model = w2v_small
    st = stages.AlignerStage(source, "cuda", dt, max_samples=24000)
    for frames in (1, 33):
        S = next(s for s in range(1, 24000) if st.frames(s) == frames)
        assert st.frames(S - 1) == frames - 1
        clip = R.test_clip(S / 24000.0, seed=frames)[:, :S]
        assert clip.shape[-1] == S
        ids, lg = st.run(clip, logits=True)
        want = R.model_logits(model, clip).float().cpu()
        assert lg.shape == want.shape and want.shape[0] == frames
        report(f"w2v {E.DTYPE_NAMES[dt]} {S} samples -> {frames} frame(s) vs Wav2Vec2ForCTC fp32", lg, want, W2V_TOL[dt])
        assert torch.equal(ids.cpu().long(), lg.cpu().argmax(-1))
    assert st.guard() == 0
    st.close()


def _utterance(cfg, M, S, steps, g):
    return (torch.randn(1, M, cfg.in_latent_channels, generator=g), torch.randn(1, 2 * cfg.model_channels, generator=g) * 0.5, S,
            torch.randn(1, 100, S, generator=g), torch.randn(steps, 1, 100, S, generator=g))


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_diffusion_padded_batch_and_captured_steps(name, dt, tdt, tol):
    """Two utterances of 160 (a multiple of 32) and 139 positions in one padded batch: each mel is the same bits as from its solo run (the
    per-utterance lengths reach GroupNorm and the attention pair; both are longer than 128 positions, so neither changes its attention
    kernel inside the batch - tests/test_gpu_parity_r3.py).  The solo runs are held to the oracle, and the captured sampler step to the
    eager one."""
    cfg = DiffusionConfig(**G.DIFF_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=G.DIFF_SEED), tdt)
    N = 3  # the shortest schedule whose step is captured
    g = torch.Generator().manual_seed(59)
    items = [_utterance(cfg, 37, 160, N, g), _utterance(cfg, 32, 139, N, g)]
    sched, osched = Schedule(N, 4000, True, 2.0), O.Schedule(N, 4000, True, 2.0)
    st = stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=192, max_codes=64, max_steps=8, max_batch=2)
    alone = []
    for u, (lat, cond, S, x, nz) in enumerate(items):
        st.condition(lat, cond, S)
        emb = O.diffusion_timestep_independent(sd, cfg, lat, cond, S)
        report(f"diffusion timestep_independent {name} S={S} vs oracle", st.code_emb(), emb, tol)
        captures = st.stat(0)
        mel = st.sample(sched, x, nz).clone()
        assert st.stat(0) == captures + 1, "the sampler step was not captured"
        report(f"diffusion p_sample_loop mel ({N} steps) {name} S={S} vs oracle", mel,
               O.denormalize_tacotron_mel(O.p_sample_loop(sd, cfg, osched, emb, x.clone(), nz)), tol * 2)
        E.load_library().tt_graph_replay(0)
        try:
            eager = st.sample(sched, x, nz)
        finally:
            E.load_library().tt_graph_replay(1)
        assert torch.equal(mel, eager), f"S={S}: captured sampler steps differ from eager launches"
        alone.append(mel)
    many = st.sample_many(sched, items)
    for u, (a, b) in enumerate(zip(many, alone)):
        assert a.shape == b.shape and torch.equal(a, b), f"utterance {u} (S={items[u][2]}) of the padded batch differs from its solo run"
    assert st.guard() == 0
    st.close()


@torch.no_grad()
def test_guard_message_of_a_tripped_stage():
    """The fp16 overflow of tests/test_gpu_r4.py::test_overflow_guards_trip_on_fp16_overflow_only (AR feed-forward scaled beyond 65504): the
    guard's text is the stage's sentence with the count and the fp16 advice, and a null handle is refused with its own text."""
    cfg = ARConfig(**G.AR_CFG)
    hot = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), cfg)
    for k in list(hot):
        if k.endswith("mlp.c_fc.weight") or k.endswith("mlp.c_fc.bias"):
            hot[k] = hot[k] * 1.0e5
        if k.endswith("mlp.c_proj.weight"):
            hot[k] = hot[k] * 1.0e-5
    cond, text = G.ar_inputs(cfg)
    st = stages.ArStage(hot, cfg, dtype=E.TT_F16, max_batch=8, max_text=40, max_new_tokens=16, max_latent_candidates=1)
    st.prefill(cond, text)
    st.generate(8, 8, seed=1)
    lib = E.load_library()
    n = lib.tt_ar_guard(st.h, 0)
    assert n > 0
    assert lib.tt_last_error().decode() == f"autoregressive stage: {n} kernel(s) met non-finite values (operand overflow in fp16: use bf16 operands for this stage)"
    assert st.guard() == n and st.guard() == 0
    st.close()
    assert lib.tt_clvp_guard(None, 0) == -1 and lib.tt_last_error().decode() == "tt_clvp_guard: null handle"
