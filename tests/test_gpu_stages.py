"""-m gpu: each hot-path stage of the HIP engine (through the C-ABI handles) against
  (a) the CPU oracle evaluated on the same operand-rounded weights and the same injected noise, and
  (b) the committed golden vectors produced by the reference's own modules (fp32 weights).
Stated tolerances (relative L2 of the stage output): bf16 2.5e-2 / fp16 4e-3 vs the oracle on rounded
weights; bf16 4e-2 / fp16 6e-3 vs the fp32 reference goldens (adds weight rounding)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import make_golden as G
from oracle import tortoise_oracle as O
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import weights as W
from tortoise_tts_amd import stages
from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, HifiganConfig, VocoderConfig
from tortoise_tts_amd.schedule import Schedule
from tests.gpu_util import DTYPES, quantize_sd, report, rel_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gold(name):
    return np.load(os.path.join(GOLD, name))


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_ar_prefill_and_teacher_forced_steps(name, dt, tdt, tol):
    g = gold("ar.npz")
    cfg = ARConfig(**G.AR_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), tdt)
    cond, text = G.ar_inputs(cfg)
    st = stages.ArStage(sd, cfg, dtype=dt, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=2)
    st.prefill(cond, text)
    prefix = O.ar_prefix(sd, cfg, cond, text)
    lg, kv = O.ar_prefill(sd, cfg, prefix, G.AR_B)
    got = st.logits(1)
    report(f"AR prefill logits {name} vs oracle", got[0], lg[0], tol)
    report(f"AR prefill logits {name} vs reference golden", got[0], torch.from_numpy(g["logits"][0][0]), tol * 1.6)
    st.begin(G.AR_B)
    for s, tk in enumerate(G.AR_TOKENS):
        tk = torch.tensor(tk)
        st.decode_step(tk)
        lg, kv = O.ar_step(sd, cfg, tk, s + 1, kv)
        got = st.logits(G.AR_B)
        report(f"AR cached step {s + 1} logits {name} vs oracle", got, lg, tol)
        report(f"AR cached step {s + 1} logits {name} vs reference golden", got, torch.from_numpy(g["logits"][s + 1]), tol * 1.6)
    st.close()


@torch.no_grad()
def test_ar_long_prompt_multi_slot_prefix():
    """A long prompt (390 text tokens, the reference's limit is < 400: api.py:392): prefix of 394 rows = 7 prefix slots of 64 keys
    in the decode attention's LDS staging, ragged last slot, 5 sequences (a partly filled last workgroup of 4); 70 cached steps
    so that the own keys also span two slots.  Teacher-forced logits vs the oracle."""
    import torch.nn.functional as F_
    cfg = ARConfig(**G.AR_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), torch.bfloat16)
    g = torch.Generator().manual_seed(2)
    cond = torch.randn(1, cfg.model_dim, generator=g)
    text = F_.pad(torch.randint(1, 255, (1, 390), generator=g).int(), (0, 1))
    B, steps = 5, 70
    st = stages.ArStage(sd, cfg, dtype=E.TT_BF16, max_batch=8, max_text=400, max_new_tokens=80, max_latent_candidates=1)
    st.prefill(cond, text)
    lg, kv = O.ar_prefill(sd, cfg, O.ar_prefix(sd, cfg, cond, text), B)
    report("AR long-prompt prefill logits bf16 vs oracle", st.logits(1)[0], lg[0], 2.5e-2)
    st.begin(B)
    toks = torch.randint(0, 8192, (steps, B), generator=g)
    for s in range(steps):
        st.decode_step(toks[s])
        lg, kv = O.ar_step(sd, cfg, toks[s], s + 1, kv)
        if s in (0, 1, 62, 63, 64, steps - 1):
            report(f"AR long-prompt cached step {s + 1} logits bf16 vs oracle", st.logits(B), lg, 2.5e-2)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_ar_latents(name, dt, tdt, tol):
    g = gold("ar.npz")
    cfg = ARConfig(**G.AR_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.LAT_SEED), tdt)
    cond, text, codes = G.latent_inputs(cfg)
    st = stages.ArStage(sd, cfg, dtype=dt, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=2)
    got = st.latents(cond, text, codes)
    want = O.ar_latents(sd, cfg, cond.repeat(G.LAT_K, 1), text.repeat(G.LAT_K, 1), codes)
    report(f"AR latents {name} vs oracle", got, want, tol)
    report(f"AR latents {name} vs reference golden", got, torch.from_numpy(g["latents"]), tol * 1.6)
    st.close()


@torch.no_grad()
def test_ar_generate_injected_noise_and_sharding_invariance():
    cfg = ARConfig(**G.AR_CFG)
    tdt = torch.bfloat16
    sd = W.suppress_stop_token(quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), tdt), cfg)
    cond, text = G.ar_inputs(cfg)
    B, steps = 4, 12
    gen = torch.Generator().manual_seed(0)
    noise = torch.empty(steps, B, cfg.number_mel_codes).exponential_(1, generator=gen)
    want, want_logits = O.ar_sample_loop(sd, cfg, cond, text, B, steps, noise, return_logits=True)
    st = stages.ArStage(sd, cfg, dtype=E.TT_BF16, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=2)
    st.prefill(cond, text)
    got, n = st.generate(B, steps, exp_noise=noise)
    assert n == steps and got.shape == (B, steps)
    agree = float((got.cpu() == want).float().mean())
    first = float((got.cpu()[:, 0] == want[:, 0]).float().mean())
    print(f"[parity] AR free-running codes vs oracle (injected Exp(1) noise): agreement {agree:.3f}, first token {first:.3f}")
    assert got.min() >= 0 and got.max() < cfg.number_mel_codes and (got != cfg.stop_mel_token).all()
    assert first == 1.0 and agree == 1.0  # measured 1.000 on MI355X (profiles/r01_parity_gpu.txt); any flip is a regression
    # every sampled token must lie in the oracle's nucleus when the oracle is teacher-forced with OUR tokens
    ids = torch.full((B, st.P + 1), 1, dtype=torch.long)
    ids[:, -1] = cfg.start_mel_token
    prefix = O.ar_prefix(sd, cfg, cond, text)
    lg, kv = O.ar_prefill(sd, cfg, prefix, B)
    inside = 0
    for s in range(steps):
        scores = O.warp_logits(lg, ids)
        inside += int(torch.isfinite(scores[torch.arange(B), got.cpu()[:, s]]).sum())
        ids = torch.cat([ids, got.cpu()[:, s:s + 1]], dim=1)
        if s + 1 < steps:
            lg, kv = O.ar_step(sd, cfg, got.cpu()[:, s], s + 1, kv)
    print(f"[parity] sampled tokens inside the oracle's top-k/top-p nucleus: {inside}/{B * steps}")
    assert inside >= int(0.95 * B * steps)
    # Philox streams are keyed by the GLOBAL candidate index: sharding 4 = 2 + 2 gives the same codes
    st.prefill(cond, text)
    full, _ = st.generate(4, steps, seed=77)
    st.prefill(cond, text)
    lo, _ = st.generate(2, steps, seed=77, row_offset=0)
    st.prefill(cond, text)
    hi, _ = st.generate(2, steps, seed=77, row_offset=2)
    assert torch.equal(full, torch.cat([lo, hi], dim=0)), "candidate sharding changed the sampled codes"
    again, _ = (st.prefill(cond, text), st.generate(4, steps, seed=77))[1]
    assert torch.equal(full, again)
    st.close()


@torch.no_grad()
def test_ar_generate_stop_token_ragged_rows_and_early_exit():
    """Stop token NOT suppressed (its logit is raised so rows finish at different steps): the decode loop must follow
    GenerationMixin.sample's finished-row rule (stream_generator.py:980-996: `tok * unfinished + pad * (1 - unfinished)`,
    stop when every row is finished) and return exactly the steps the reference would have run, even though the engine
    polls the unfinished counter only every 8 steps."""
    cfg = ARConfig(**G.AR_CFG)
    tdt = torch.float16
    sd = quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), tdt)
    bias = sd["mel_head.bias"].clone()
    bias[cfg.stop_mel_token] += 4.0
    sd["mel_head.bias"] = bias
    cond, text = G.ar_inputs(cfg)
    B, steps = 6, 48
    gen = torch.Generator().manual_seed(3)
    noise = torch.empty(steps, B, cfg.number_mel_codes).exponential_(1, generator=gen)
    want = O.ar_sample_loop(sd, cfg, cond, text, B, steps, noise)
    st = stages.ArStage(sd, cfg, dtype=E.TT_F16, max_batch=8, max_text=40, max_new_tokens=64, max_latent_candidates=2)
    st.prefill(cond, text)
    got, n = st.generate(B, steps, exp_noise=noise)
    got = got.cpu()
    stop = cfg.stop_mel_token

    def first_stop(row):
        idx = (row == stop).nonzero()
        return int(idx[0]) if idx.numel() else len(row)
    fs_got, fs_want = [first_stop(r) for r in got], [first_stop(r) for r in want]
    print(f"[parity] AR ragged stops: engine {fs_got} (n={n}) oracle {fs_want} (n={want.shape[1]})")
    assert got.shape == (B, n) and 1 <= n <= steps
    for r, f in zip(got, fs_got):
        assert (r[f:] == stop).all(), "a finished row emitted something other than the stop token"
    assert min(fs_got) < max(fs_got), "rows did not finish at different steps: the test lost its point"
    if max(fs_got) < steps:  # every row finished: the loop must have stopped exactly one step after the last finisher
        assert n == max(fs_got) + 1
    same = sum(int(a == b) for a, b in zip(fs_got, fs_want))
    assert same >= B // 2, "stop positions disagree with the oracle on most rows"
    if fs_got == fs_want:
        assert n == want.shape[1]
        assert float((got == want).float().mean()) >= 0.9
    # integer post-processing on the ragged rows is bit-exact against the oracle's restatement (api.py:87-114, 425-426)
    from tortoise_tts_amd.api import fix_autoregressive_output
    import torch.nn.functional as F
    padded = F.pad(got, (0, steps + 2 - n), value=stop)
    want_fixed = np.stack([O.fix_autoregressive_output(r.numpy(), stop) for r in padded])
    assert np.array_equal(fix_autoregressive_output(padded.clone(), stop).numpy(), want_fixed)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_clvp(name, dt, tdt, tol):
    cfg = CLVPConfig(**G.CLVP_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.clvp_manifest(cfg), seed=G.CLVP_SEED), tdt)
    text, codes = G.clvp_inputs()
    st = stages.ClvpStage(sd, cfg, dtype=dt, max_rows=4096)
    got = st.score(text, codes)
    want = O.clvp_score(sd, cfg, text.repeat(G.CLVP_B, 1), codes)
    print("[parity] clvp scores", got.cpu().tolist(), want.tolist(), gold("clvp.npz")["scores"].tolist())
    report(f"CLVP scores {name} vs oracle", got, want, tol * 2)
    report(f"CLVP scores {name} vs reference golden", got, torch.from_numpy(gold("clvp.npz")["scores"]), tol * 3)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_diffusion(name, dt, tdt, tol):
    g = gold("diffusion.npz")
    cfg = DiffusionConfig(**G.DIFF_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=G.DIFF_SEED), tdt)
    S, latents, cond, x, step_noise = G.diff_inputs(cfg)
    st = stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=128, max_codes=64, max_steps=16)
    st.condition(latents, cond, S)
    emb = O.diffusion_timestep_independent(sd, cfg, latents, cond, S)
    report(f"diffusion timestep_independent {name} vs oracle", st.code_emb(), emb, tol)
    report(f"diffusion timestep_independent {name} vs reference golden", st.code_emb(), torch.from_numpy(g["code_emb"]), tol * 1.6)
    ts = torch.tensor([G.DIFF_TS])
    out = st.forward(x, G.DIFF_TS, cond_free=True)
    report(f"diffusion forward cond {name} vs oracle", out[0], O.diffusion_forward(sd, cfg, x, ts, emb, False)[0], tol)
    report(f"diffusion forward uncond {name} vs oracle", out[1], O.diffusion_forward(sd, cfg, x, ts, emb, True)[0], tol)
    report(f"diffusion forward cond {name} vs reference golden", out[0], torch.from_numpy(g["eps_cond"][0]), tol * 1.6)
    out1 = st.forward(x, G.DIFF_TS, cond_free=False)
    assert rel_err(out1[0], out[0]) < 1e-6, "batched cond/uncond evaluation changed the conditioned row"
    sched = Schedule(G.DIFF_STEPS, 4000, True, 2.0)
    osched = O.Schedule(G.DIFF_STEPS, 4000, True, 2.0)
    mel = st.sample(sched, x, step_noise)
    want = O.denormalize_tacotron_mel(O.p_sample_loop(sd, cfg, osched, emb, x.clone(), step_noise))
    report(f"diffusion p_sample_loop mel ({G.DIFF_STEPS} steps) {name} vs oracle", mel, want, tol * 2)
    report(f"diffusion p_sample_loop mel {name} vs reference golden", mel, O.denormalize_tacotron_mel(torch.from_numpy(g["x0"])), tol * 3)
    # graph replay and eager launches are the same kernels: results must be bit-identical
    E.load_library().tt_graph_replay(0)
    try:
        mel2 = st.sample(sched, x, step_noise)
    finally:
        E.load_library().tt_graph_replay(1)
    assert torch.equal(mel, mel2), "hipGraph replay differs from eager launches"
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_univnet(name, dt, tdt, tol):
    cfg = VocoderConfig()
    sd = quantize_sd(W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(cfg), seed=G.VOC_SEED)), tdt)
    mel, z = G.voc_inputs()
    st = stages.VocoderStage(sd, cfg, dtype=dt, max_frames=64)
    wav = st.inference(mel, z)
    want = O.univnet_inference(sd, cfg, mel, z)
    assert wav.shape == (1, 1, G.VOC_S * 256)
    report(f"UnivNet waveform {name} vs oracle", wav, want, tol * 2)
    report(f"UnivNet waveform {name} vs reference golden", wav, torch.from_numpy(gold("vocoder.npz")["wav"]), tol * 3)
    st.close()


@torch.no_grad()
def test_diffusion_full_width_short_sequence():
    """1024 channels / 16 heads (the reference width) with 2 layers and a SHORT sequence (S = 43, M = 86 rows): exercises
    the GroupNorm statistics fused into the GEMM epilogue and the C == 1024 GroupNorm fast path against the CPU oracle.
    At M = 86 the 64x64 tile and the 16-query flash variant are selected; the production variants (128x64 conv-GEMM at
    M = 1740, flash 64 queries per wave with key split at n = 870) are compared with the reference in
    tests/test_gpu_fullsize.py::test_full_diffusion_s870."""
    cfg = DiffusionConfig(model_channels=1024, num_layers=2, in_latent_channels=1024, num_heads=16)
    tdt, dt, tol = torch.bfloat16, E.TT_BF16, 2.5e-2
    sd = quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=21), tdt)
    g = torch.Generator().manual_seed(5)
    M = 40
    S = M * 4 * 24000 // 22050
    latents = torch.randn(1, M, 1024, generator=g)
    cond = torch.randn(1, 2048, generator=g)
    x = torch.randn(1, 100, S, generator=g)
    st = stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=256, max_codes=64, max_steps=16)
    st.condition(latents, cond, S)
    emb = O.diffusion_timestep_independent(sd, cfg, latents, cond, S)
    report("full-width timestep_independent vs oracle", st.code_emb(), emb, tol)
    ts = torch.tensor([1234])
    out = st.forward(x, 1234, cond_free=True)
    report("full-width forward cond vs oracle", out[0], O.diffusion_forward(sd, cfg, x, ts, emb, False)[0], tol)
    report("full-width forward uncond vs oracle", out[1], O.diffusion_forward(sd, cfg, x, ts, emb, True)[0], tol)
    N = 4
    step_noise = torch.randn(N, 1, 100, S, generator=g)
    mel = st.sample(Schedule(N, 4000, True, 2.0), x, step_noise)
    want = O.denormalize_tacotron_mel(O.p_sample_loop(sd, cfg, O.Schedule(N, 4000, True, 2.0), emb, x.clone(), step_noise))
    report("full-width p_sample_loop mel vs oracle", mel, want, tol * 2)
    st.close()


@torch.no_grad()
def test_diffusion_split_rows_match_batched_sampling():
    """Split sampling (tt_diff_split_*): two engines stand in for two GPUs, one evaluating the
    conditioned row and one the conditioning-free row of every step, exchanging rows and applying the same update.
    Must agree with the batched single-engine p_sample_loop (and therefore the oracle) and keep both participants'
    states identical.  Full width so the fused-statistics GEMM path is the one exercised."""
    cfg = DiffusionConfig(model_channels=1024, num_layers=2, in_latent_channels=1024, num_heads=16)
    tdt, dt, tol = torch.bfloat16, E.TT_BF16, 2.5e-2
    sd = quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=21), tdt)
    g = torch.Generator().manual_seed(6)
    M = 40
    S = M * 4 * 24000 // 22050
    latents = torch.randn(1, M, 1024, generator=g)
    cond = torch.randn(1, 2048, generator=g)
    x = torch.randn(1, 100, S, generator=g)
    N = 5
    step_noise = torch.randn(N, 1, 100, S, generator=g)
    sched = Schedule(N, 4000, True, 2.0)
    parts = [stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=256, max_codes=64, max_steps=16) for _ in range(2)]
    for st in parts:
        st.condition(latents, cond, S)
    whole = parts[0].sample(sched, x, step_noise)
    for r, st in enumerate(parts):
        assert st.split_begin(sched, x, step_noise, r) == N
    rows = torch.empty(2, S, cfg.out_channels, device="cuda")
    for _ in range(N):
        for r, st in enumerate(parts):
            rows[r].copy_(st.split_forward())  # the all_gather of the two-GPU run
        for st in parts:
            st.split_update(rows)
    mels = [st.split_end() for st in parts]
    assert torch.equal(mels[0], mels[1]), "participants diverged"
    # The conditioned row is bit-identical to the batched run (statistics-emitting GEMMs keep one tile shape); the conditioning-free row sits at batch index 1 there
    # and 0 here, so its GroupNorm partial sums are grouped differently (~1e-7), which flips occasional bf16 roundings
    # of the next GEMM operand; five recursive steps with guidance scale <= 3 amplify that to ~6e-3.  Same bar as the
    # engine-vs-oracle comparison below.
    report("split-row p_sample_loop mel vs batched engine", mels[0], whole, tol)
    emb = O.diffusion_timestep_independent(sd, cfg, latents, cond, S)
    want = O.denormalize_tacotron_mel(O.p_sample_loop(sd, cfg, O.Schedule(N, 4000, True, 2.0), emb, x.clone(), step_noise))
    report("split-row p_sample_loop mel vs oracle", mels[0], want, tol * 2)
    with pytest.raises(E.EngineError):
        parts[0].split_forward()  # ended: must fail loudly, not reuse a stale graph
    for st in parts:
        st.close()



@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_random_conditioning_latents(name, dt, tdt, tol):
    """get_random_conditioning_latents (api.py:301-309) on the engine vs the oracle and the reference golden."""
    g = gold("rlg.npz")
    sds = {ch: W.synthetic_state_dict(W.rlg_manifest(ch), seed=G.RLG_SEED, gain=3.0) for ch in (1024, 2048)}
    st = stages.RandomLatentStage(sds[1024], sds[2048], dtype=dt)
    a, d = st.latents(G.rlg_inputs(1024), G.rlg_inputs(2048))
    for ch, got in ((1024, a), (2048, d)):
        report(f"random latent {ch} {name} vs oracle", got, O.random_latent_converter(quantize_sd(sds[ch], tdt), G.rlg_inputs(ch)), tol)
        report(f"random latent {ch} {name} vs reference golden", got, torch.from_numpy(g[f"latent_{ch}"]), tol * 1.6)


@pytest.mark.parametrize("kv_cache", [True, False])
@torch.no_grad()
def test_ar_position_rule_and_hf_generate_codes(kv_cache):
    """TextToSpeech(kv_cache=...) on the engine = which mel position row a generated token gets (autoregressive.py:134-149).
    (1) teacher-forced logits vs the oracle under the same rule; (2) free-running sampling with the Exp(1) draws HF's
    multinomial consumed must reproduce the codes of the REAL HF generate() run on the reference model
    (tests/golden/sampling.npz), including rows that stop at different steps and the whole-batch early exit."""
    cfg = ARConfig(**G.AR_CFG)
    cond, text = G.ar_inputs(cfg)
    sd = quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), torch.float16)
    st = stages.ArStage(sd, cfg, dtype=E.TT_F16, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=2, kv_cache=kv_cache)
    st.prefill(cond, text)
    prefix = O.ar_prefix(sd, cfg, cond, text)
    lg, kv = O.ar_prefill(sd, cfg, prefix, G.AR_B)
    st.begin(G.AR_B)
    for s_, tk in enumerate(G.AR_TOKENS):
        tk = torch.tensor(tk)
        st.decode_step(tk)
        lg, kv = O.ar_step(sd, cfg, tk, s_ + 1, kv, kv_cache=kv_cache)
        report(f"AR cached step {s_ + 1} logits kv_cache={kv_cache} f16 vs oracle", st.logits(G.AR_B), lg, 4e-3)
    st.close()
    g = gold("sampling.npz")
    noise = G.sampling_noise(cfg)
    for kv, boost in G.SAMPLE_CASES:
        if kv != kv_cache:
            continue
        want = torch.from_numpy(g[f"codes_kv{int(kv)}_eos{boost}"])
        st = stages.ArStage(G.sampling_state_dict(cfg, boost), cfg, dtype=E.TT_F16, max_batch=8, max_text=40, max_new_tokens=32,
                            max_latent_candidates=2, kv_cache=kv_cache)
        st.prefill(cond, text)
        got, n = st.generate(G.SAMPLE_B, G.SAMPLE_N, exp_noise=noise)
        got = got.cpu()
        agree = float((got[:, :want.shape[1]] == want[:, :got.shape[1]]).float().mean()) if n == want.shape[1] else 0.0
        print(f"[parity] AR sampling vs HF generate() golden kv_cache={kv} eos_boost={boost}: steps {n} vs {want.shape[1]}, code agreement {agree:.3f}")
        assert n == want.shape[1], "the engine ran a different number of steps than HF generate()"
        assert agree >= 0.95  # fp16 operands vs fp32 reference: a near-tie in argmax(p/q) may flip a token (measured: see profiles/)
        st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_conditioning_encoders(name, dt, tdt, tol):
    """SURVEY.md 8f-3 on the device: ConditioningEncoder (64-wide heads -> the flash path) and contextual_embedder (stride-2
    convolutions, 128-wide heads with relative positions -> the wave-per-query kernel) vs the oracle on rounded weights and
    vs the reference modules' own get_conditioning outputs (tests/golden/conditioning.npz)."""
    a_cfg, d_cfg = ARConfig(**G.AR_CFG), DiffusionConfig(**G.DIFF_CFG)
    a_sd = W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.COND_SEED)
    d_sd = W.synthetic_state_dict(W.diffusion_manifest(d_cfg), seed=G.COND_SEED + 1)
    mel_ar, mel_diff = G.cond_inputs()
    st = stages.ConditioningStage(a_sd, d_sd, a_cfg, d_cfg, dtype=dt, max_frames=256)
    got_a = st.auto_latent(mel_ar).cpu()
    got_d = st.diffusion_latent(mel_diff).cpu()
    g = gold("conditioning.npz")
    report(f"conditioning auto latent {name} vs reference golden", got_a, torch.from_numpy(g["auto_latent"]), tol * 1.6)
    report(f"conditioning diffusion latent {name} vs reference golden", got_d, torch.from_numpy(g["diffusion_latent"]), tol * 1.6)
    report(f"conditioning auto latent {name} vs oracle", got_a, O.ar_get_conditioning(quantize_sd(a_sd, tdt), a_cfg, mel_ar), tol)
    report(f"conditioning diffusion latent {name} vs oracle", got_d, O.diffusion_get_conditioning(quantize_sd(d_sd, tdt), d_cfg, mel_diff), tol)
    # clips of different lengths, passed as a list (api.py:271-289 stacks equal-length clips; the engine takes them one by one)
    clips = [mel_diff[:, 0], mel_diff[:, 1, :, :37]]
    got = st.diffusion_latent(clips).cpu()
    sdq = quantize_sd(d_sd, tdt)
    outs = []
    for c in clips:
        import torch.nn.functional as F_
        h = F_.conv1d(c.float(), sdq["contextual_embedder.0.weight"], sdq["contextual_embedder.0.bias"], stride=2, padding=1)
        h = F_.conv1d(h, sdq["contextual_embedder.1.weight"], sdq["contextual_embedder.1.bias"], stride=2, padding=1)
        i = 2
        while f"contextual_embedder.{i}.norm.weight" in sdq:
            h = O.attention_block(sdq, f"contextual_embedder.{i}", h, d_cfg.num_heads)
            i += 1
        outs.append(h)
    report(f"conditioning diffusion latent {name}, ragged clips", got, torch.cat(outs, dim=-1).mean(dim=-1), tol)
    st.close()


@torch.no_grad()
def test_conditioning_encoders_full_width():
    """The api.py:217-236 widths (1024 x 16 heads x 6 blocks at 517 frames; 2048-wide embedder, 128-wide heads, 100 frames) vs the oracle."""
    a_cfg, d_cfg = ARConfig(), DiffusionConfig()
    keep_a = lambda k: k.startswith("conditioning_encoder.")
    keep_d = lambda k: k.startswith("contextual_embedder.")
    a_sd = {k: v for k, v in W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=5).items() if keep_a(k)}
    d_sd = {k: v for k, v in W.synthetic_state_dict(W.diffusion_manifest(d_cfg), seed=6).items() if keep_d(k)}
    gen = torch.Generator().manual_seed(8)
    mel_ar = torch.randn(1, 2, 80, 517, generator=gen)
    mel_diff = torch.randn(1, 2, 100, 400, generator=gen)
    st = stages.ConditioningStage(a_sd, d_sd, a_cfg, d_cfg, dtype=E.TT_BF16, max_frames=640)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    report("FULL conditioning auto latent bf16 vs oracle", st.auto_latent(mel_ar).cpu(),
           O.ar_get_conditioning(quantize_sd(a_sd, torch.bfloat16), a_cfg, mel_ar), 2.5e-2)
    report("FULL conditioning diffusion latent bf16 vs oracle", st.diffusion_latent(mel_diff).cpu(),
           O.diffusion_get_conditioning(quantize_sd(d_sd, torch.bfloat16), d_cfg, mel_diff), 2.5e-2)
    st.close()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_hifigan_decoder(name, dt, tdt, tol):
    """HifiganGenerator.inference on the MFMA conv-GEMM path (dilated taps, transposed conv as a 2-tap GEMM,
    channel widths 32 / 16 padded to 64) vs the oracle on rounded weights and vs the reference module's own output."""
    cfg = HifiganConfig(**G.HIFI_CFG)
    sd = W.fold_weight_norm(W.synthetic_state_dict(W.hifigan_manifest(cfg), seed=G.HIFI_SEED))
    lat, g = G.hifi_inputs(cfg)
    st = stages.HifiganStage(sd, cfg, dtype=dt, max_latents=32)
    got = st.inference(lat, g).cpu()
    want = torch.from_numpy(gold("hifigan.npz")["wav"])
    assert got.shape == want.shape == (1, 1, E.load_library().tt_hifi_output_frames(G.HIFI_T) * cfg.hop)
    report(f"hifigan wav {name} vs reference golden", got, want, tol * 1.6)
    report(f"hifigan wav {name} vs oracle", got, O.hifigan_inference(quantize_sd(sd, tdt), cfg, lat, g), tol)
    # a shorter latent sequence on the same handle (streaming chunks grow from call to call)
    got5 = st.inference(lat[:, :5], g).cpu()
    report(f"hifigan wav {name}, 5 latents", got5, O.hifigan_inference(quantize_sd(sd, tdt), cfg, lat[:, :5], g), tol)
    st.close()


@torch.no_grad()
def test_hifigan_decoder_full_width():
    """api_fast.py:222-225 widths (1024 -> 512 -> 256 -> 128 -> 64 -> 32 channels, factors 8, 8, 2, 2) on 40 latents vs the oracle."""
    cfg = HifiganConfig()
    sd = W.fold_weight_norm(W.synthetic_state_dict(W.hifigan_manifest(cfg), seed=31))
    gen = torch.Generator().manual_seed(32)
    lat, g = torch.randn(1, 40, cfg.in_channels, generator=gen), torch.randn(1, cfg.cond_channels, generator=gen) * 0.5
    st = stages.HifiganStage(sd, cfg, dtype=E.TT_BF16, max_latents=64)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    report("FULL hifigan wav bf16 vs oracle", st.inference(lat, g).cpu(), O.hifigan_inference(quantize_sd(sd, torch.bfloat16), cfg, lat, g), 2.5e-2)
    st.close()


@torch.no_grad()
def test_ar_generate_chunks_equal_one_shot_loop():
    """tt_ar_generate_chunk (the streaming path resumes the hipGraph decode loop chunk by chunk) must reproduce tt_ar_generate
    bit for bit: same Philox streams, same device-side state, ragged stop tokens included."""
    cfg = ARConfig(**G.AR_CFG)
    sd = G.sampling_state_dict(cfg, 2.0)
    cond, text = G.ar_inputs(cfg)
    st = stages.ArStage(sd, cfg, max_batch=8, max_text=40, max_new_tokens=40, max_latent_candidates=1)
    st.prefill(cond, text)
    full, n = st.generate(6, 36, seed=5)
    st.prefill(cond, text)
    last, pieces = None, 0
    for codes, done in st.generate_stream(6, 36, 5, first_chunk=7, seed=5):
        last, pieces = codes, pieces + 1
        assert torch.equal(codes, full[:, :codes.shape[1]])
        if pieces == 1:
            # the first chunk consumed the prefill logits: a one-shot generation is rejected before it touches the running stream
            with pytest.raises(E.EngineError):
                st.generate(6, 36, seed=5)
    assert pieces >= 2 and last.shape[1] == n and torch.equal(last, full)
    # the streaming caller runs the teacher-forced latent pass BETWEEN chunks (api_fast.tts_stream): that pass uses the handle's
    # residual-stream buffer, so a resumed chunk must rebuild its input row from the device-side state, not find it there
    st1 = stages.ArStage(sd, cfg, max_batch=1, max_text=40, max_new_tokens=40, max_latent_candidates=1)
    st1.prefill(cond, text)
    one, n1 = st1.generate(1, 36, seed=5)
    st1.prefill(cond, text)
    for codes, done in st1.generate_stream(1, 36, 5, first_chunk=7, seed=5):
        assert torch.equal(codes, one[:, :codes.shape[1]]), "a resumed chunk consumed a stale input row"
        st1.latents(cond, text, codes)
    assert codes.shape[1] == n1
    st1.close()
    st.close()


@pytest.mark.parametrize("top_k,top_p", [(0, 0.8), (300, 0.8), (100000, 0.9), (0, 1.0), (257, 0.3)])
@torch.no_grad()
def test_ar_generate_any_top_k(top_k, top_p):
    """HF accepts any top_k (TopKLogitsWarper clamps it to the vocabulary; top_k == 0 drops the warper: stream_generator.py:43-57 /
    transformers 4.31 _get_logits_warper).  Beyond the 256 of the fast sampler the engine sorts the whole row (sample_wide_kernel):
    the sampled codes must equal the oracle loop's on the same injected Exp(1) draws, token for token."""
    cfg = ARConfig(**G.AR_CFG)
    sd = W.suppress_stop_token(quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), torch.bfloat16), cfg)
    cond, text = G.ar_inputs(cfg)
    B, steps = 4, 10
    gen = torch.Generator().manual_seed(3)
    noise = torch.empty(steps, B, cfg.number_mel_codes).exponential_(1, generator=gen)
    want = O.ar_sample_loop(sd, cfg, cond, text, B, steps, noise, top_k=top_k, top_p=top_p)
    st = stages.ArStage(sd, cfg, dtype=E.TT_BF16, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=1)
    st.prefill(cond, text)
    got, n = st.generate(B, steps, exp_noise=noise, top_k=top_k, top_p=top_p)
    agree = float((got.cpu() == want).float().mean())
    print(f"[parity] AR codes vs oracle with top_k={top_k} top_p={top_p} (full-sort sampler): agreement {agree:.3f}")
    assert n == steps and agree == 1.0
    # and the two samplers agree where both apply: k = 256 (fast kernel) against k = 256 forced through... the same draws with k = 257
    # differ only if the 257th candidate survives top-p, which top_p = 0.3 excludes
    if top_k == 257:
        st.prefill(cond, text)
        fast, _ = st.generate(B, steps, exp_noise=noise, top_k=256, top_p=top_p)
        assert torch.equal(fast, got)
    # Philox path through the wide kernel: reproducible and sharding-invariant like the fast one
    st.prefill(cond, text)
    full, _ = st.generate(4, steps, seed=5, top_k=top_k, top_p=top_p)
    st.prefill(cond, text)
    hi, _ = st.generate(2, steps, seed=5, row_offset=2, top_k=top_k, top_p=top_p)
    assert torch.equal(full[2:], hi)
    st.close()


@pytest.mark.parametrize("eos_boost", [None, 2.0])
@torch.no_grad()
def test_ar_utterance_groups_decode_like_single_utterances(eos_boost):
    """Several utterances in ONE decode batch (tt_ar_prefill_group; long-form reading renders its chunks one after the other in the
    reference, read.py:66-71): every group has its own text / voice / prefix length / Philox key, and its codes must be bit-identical to
    decoding that utterance alone - the batched GEMMs pick other tiles (M = 12 .. 48 rows instead of 4 .. 16) but keep every output
    element's k order, the row norms stay one workgroup per row, attention and sampling are per sequence."""
    cfg = ARConfig(**G.AR_CFG)
    sd = G.sampling_state_dict(cfg, eos_boost) if eos_boost else W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), cfg)
    gen = torch.Generator().manual_seed(21)
    utts = []
    for T_ in (11, 27, 18):
        utts.append((torch.randn(1, cfg.model_dim, generator=gen), F.pad(torch.randint(1, 255, (1, T_), generator=gen).int(), (0, 1))))
    seeds, Bg, max_new = [5, 9, 5], 8, 24
    st = stages.ArStage(sd, cfg, max_batch=len(utts) * Bg, max_text=40, max_new_tokens=32, max_latent_candidates=1, max_groups=4)
    singles = []
    for (cond, text), seed in zip(utts, seeds):
        st.prefill(cond, text)
        codes, n = st.generate(Bg, max_new, seed=seed, row_offset=3)
        singles.append(codes.clone())
    for g, (cond, text) in enumerate(utts):
        st.prefill_group(g, len(utts), cond, text)
    codes, n = st.generate(len(utts) * Bg, max_new, group_seeds=seeds, row_offset=3)
    assert n == max(c.shape[1] for c in singles)
    stop = cfg.stop_mel_token
    for g, single in enumerate(singles):
        mine = codes[g * Bg:(g + 1) * Bg]
        assert torch.equal(mine[:, :single.shape[1]], single), f"utterance {g} decoded differently inside the batch"
        assert (mine[:, single.shape[1]:] == stop).all()  # a group that finished early is padded like any finished row
    assert not torch.equal(singles[0], singles[2])  # same key, different text: different codes
    # and a plain single-utterance call on the same handle afterwards is unaffected by the group state
    st.prefill(*utts[1])
    again, _ = st.generate(Bg, max_new, seed=seeds[1], row_offset=3)
    assert torch.equal(again, singles[1])
    st.close()


@torch.no_grad()
def test_ar_large_group_batches_fold_split_k_in_the_launch():
    """From 1024 sequences per decode batch on, the two projections fold their split-K partial sums inside the launch ("serial
    split-K", gemm.h): ((x + bias) + P0) + P1 + ... in slab order - the same bits as the slab + row-norm path a single utterance takes.
    4 utterances x 256 candidates (1024 rows, serial path) against each utterance alone (256 rows, slab path): identical codes."""
    cfg = ARConfig(**G.AR_CFG)
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), cfg)
    gen = torch.Generator().manual_seed(22)
    utts = [(torch.randn(1, cfg.model_dim, generator=gen), F.pad(torch.randint(1, 255, (1, T_), generator=gen).int(), (0, 1))) for T_ in (9, 30, 17, 22)]
    Bg, max_new = 256, 10
    st = stages.ArStage(sd, cfg, max_batch=len(utts) * Bg, max_text=40, max_new_tokens=16, max_latent_candidates=1, max_groups=4)
    singles = []
    for cond, text in utts:
        st.prefill(cond, text)
        singles.append(st.generate(Bg, max_new, seed=31)[0].clone())
    for g, (cond, text) in enumerate(utts):
        st.prefill_group(g, len(utts), cond, text)
    codes, n = st.generate(len(utts) * Bg, max_new, seed=31)
    assert n == max_new
    for g, single in enumerate(singles):
        assert torch.equal(codes[g * Bg:(g + 1) * Bg], single), f"utterance {g}: the in-launch split-K fold changed the sampled codes"
    st.close()


@pytest.mark.parametrize("kv_cache", [False, True])
@torch.no_grad()
def test_stream_latents_filed_by_the_decode_steps(kv_cache):
    """The (token, latent) pairs of the reference's streaming generator (stream_generator.py:916-1000 -> api_fast.py:402-411): the
    engine's decode steps file final_norm(ln_f(hidden)) themselves (tt_ar_stream_latents).  They must equal one teacher-forced pass
    over the sampled codes - plain mel positions for kv_cache=False, the cached decode's 0, 2, 3, ... for kv_cache=True - on the
    engine (different kernels: M = 1 split-K GEMMs + cached attention vs full GEMMs + flash attention) and in the oracle."""
    cfg = ARConfig(**G.AR_CFG)
    sd = quantize_sd(W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), cfg), torch.bfloat16)
    cond, text = G.ar_inputs(cfg)
    st = stages.ArStage(sd, cfg, max_batch=1, max_text=40, max_new_tokens=40, max_latent_candidates=1, kv_cache=kv_cache)
    st.prefill(cond, text)
    pieces = []
    for codes, done in st.generate_stream(1, 30, 8, first_chunk=12, seed=11):
        pieces.append(st.stream_latents(1, codes.shape[1]).clone())  # read between chunks, as api_fast.tts_stream does
    n = codes.shape[1]
    got = st.stream_latents(1, n)
    assert got.shape == (1, n, cfg.model_dim) and n == 30 and torch.isfinite(got).all()
    for p in pieces:
        assert torch.equal(p, got[:, :p.shape[1]]), "a latent changed after it was filed"
    want_pass = st.latents(cond, text, codes, stream_positions=kv_cache)
    report(f"per-step stream latents (kv_cache={kv_cache}) bf16 vs the engine's teacher-forced pass", got, want_pass, 2.5e-2)
    want = O.ar_latents(sd, cfg, cond, text, codes.cpu(), stream_positions=kv_cache)
    report(f"per-step stream latents (kv_cache={kv_cache}) bf16 vs oracle", got.cpu(), want, 2.5e-2)
    if kv_cache:  # and the position rule matters: the plain-position pass is a different tensor
        assert rel_err(got.cpu(), O.ar_latents(sd, cfg, cond, text, codes.cpu(), stream_positions=False)) > 5e-2
    st.close()


@torch.no_grad()
def test_api_fast_tts_and_stream():
    """tortoise.api_fast.TextToSpeech surface: tts() = generate -> latents -> HiFi-GAN; tts_stream() resumes the
    decode loop per chunk, re-decodes the latents so far and cross-fades (handle_chunks, api_fast.py:275-309)."""
    from tortoise_tts_amd.api_fast import TextToSpeech
    a_cfg = ARConfig(**G.AR_CFG)
    h_cfg = HifiganConfig(in_channels=a_cfg.model_dim, cond_channels=a_cfg.model_dim, upsample_initial_channel=128)
    sds = {"autoregressive": W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.AR_SEED), a_cfg),
           "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), seed=41)}
    tts = TextToSpeech(state_dicts=sds, configs={"ar": a_cfg, "hifigan": h_cfg}, max_mel_tokens=104, max_text_tokens=40, kv_cache=True)
    gen = torch.Generator().manual_seed(3)
    lat = (torch.randn(1, a_cfg.model_dim, generator=gen) * 0.5,)
    text = list(range(5, 25))
    wav = tts.tts(text, conditioning_latents=lat, max_mel_tokens=100, use_deterministic_seed=9)
    frames = E.load_library().tt_hifi_output_frames(100)
    assert wav.shape == (1, 1, frames * h_cfg.hop) and wav.device.type == "cpu" and torch.isfinite(wav).all() and wav.abs().max() <= 1.0
    codes_full = tts.last_codes
    chunks = list(tts.tts_stream(text, conditioning_latents=lat, max_mel_tokens=100, use_deterministic_seed=9, stream_chunk_size=12,
                                 overlap_wav_len=256))
    assert len(chunks) == 5  # 60 (first buffer, api_fast.py:401), then 12 tokens per piece: 72, 84, 96, 100
    total = sum(int(c.shape[0]) for c in chunks)
    assert total == wav.shape[-1] - 256  # everything but the last overlap window is emitted (api_fast.py:277-281)
    assert torch.equal(tts.last_codes, codes_full), "tts_stream sampled different codes from tts() with the same seed"
    # the first piece is the decode of the first 60 codes, minus its overlap tail
    first = tts.hifi_decoder.inference(tts._stream_latents(lat[0].cuda(), F_pad_text(text), codes_full[:, :60]), lat[0]).reshape(-1)
    assert torch.equal(chunks[0].cpu(), first[:-256].cpu())
    # voice_samples on the streaming path: only the autoregressive encoder exists there (api_fast.py:230-247); mel clips in, latent out
    mel_ar, _ = G.cond_inputs()
    sd_c = W.synthetic_state_dict(W.ar_manifest(a_cfg), seed=G.AR_SEED)
    got = tts.get_conditioning_latents([mel_ar[:, 0], mel_ar[:, 1]]).cpu()
    report("api_fast conditioning latent bf16 vs oracle", got, O.ar_get_conditioning(quantize_sd(sd_c, torch.bfloat16), a_cfg, mel_ar), 2.5e-2)
    tts.ar.close(); tts.hifi_decoder.close(); tts.conditioning.close()


def F_pad_text(ids):
    import torch.nn.functional as F_
    return F_.pad(torch.tensor(ids, dtype=torch.int32, device="cuda")[None], (0, 1))


@torch.no_grad()
def test_ar_step_graph_is_kept_between_calls_and_seeds_are_data():
    """The captured decode step is kept on the handle between tt_ar_generate calls (csrc/gpt2.hip ar_step_key): the Philox keys live in
    device memory, so a second call with another seed replays the SAME graph and must sample what eager launches sample for that seed;
    a call that changes what the graph bakes in (batch, prefix length, sampling scalars) must re-capture."""
    cfg = ARConfig(**G.AR_CFG)
    sd = W.suppress_stop_token(quantize_sd(W.synthetic_state_dict(W.ar_manifest(cfg), seed=G.AR_SEED), torch.bfloat16), cfg)
    cond, text = G.ar_inputs(cfg)
    text_short = text[:, : max(2, text.shape[1] // 2)].contiguous()
    st = stages.ArStage(sd, cfg, dtype=E.TT_BF16, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=1)
    steps = 12
    calls = [  # (text, B, seed, sampler kwargs)
        (text, 4, 5, {}), (text, 4, 6, {}), (text, 4, 5, {}),            # same key three times, two seeds
        (text_short, 4, 6, {}),                                           # other prefix length
        (text, 8, 6, {}),                                                 # other batch
        (text, 4, 6, {"temperature": 0.5}), (text, 4, 6, {"top_k": 300}),  # other sampler scalars / the wide sampler kernel
        (text, 4, 5, {}),                                                 # back to the first key
    ]
    got = []
    for t, B, seed, kw in calls:
        st.prefill(cond, t)
        got.append(st.generate(B, steps, seed=seed, **kw)[0].clone())
    E.load_library().tt_graph_replay(0)
    try:
        for (t, B, seed, kw), g in zip(calls, got):
            st.prefill(cond, t)
            eager = st.generate(B, steps, seed=seed, **kw)[0]
            assert torch.equal(eager, g), f"kept step graph differs from eager launches for B={B} seed={seed} {kw} prefix {t.shape[1]}"
    finally:
        E.load_library().tt_graph_replay(1)
    assert torch.equal(got[0], got[2]) and torch.equal(got[0], got[7]) and not torch.equal(got[0], got[1])
    # a fresh handle (first capture) samples the same as the handle that has been through all of the above
    st2 = stages.ArStage(sd, cfg, dtype=E.TT_BF16, max_batch=8, max_text=40, max_new_tokens=32, max_latent_candidates=1)
    st2.prefill(cond, text)
    assert torch.equal(st2.generate(4, steps, seed=6)[0], got[1])
    st2.close()
    st.close()
