"""-m gpu: TextToSpeech(winner_batch=W) on the device, and the batched denoiser it sends the default CLI call through.

  (1) reduced width, where sample_many is bit-identical to sample(): tts(k=3, winner_batch=3) is torch.equal to tts(k=3), with and without
      conditioning-free guidance, bf16 and fp16 - provided every winner keeps more than 128 positions (a shorter sequence gets another
      attention kernel alone than inside a longer batch: tests/test_gpu_parity_r3.py), which the test asserts;
  (2) full width (bench.py's synthetic weights): same ranked winners, every mel within the operand tolerance of its type
      (tests.gpu_util.DTYPES), every waveform within the bar tests/test_gpu_full.py holds tts_many to;
  (3) the full-width batched denoiser against the REFERENCE's p_sample_loop (tests/golden/full_drift.npz): the benchmarked utterance as
      slot 0 of a two- and of a three-utterance batch and as the last slot, beside shorter neighbours, held to the solo run's own
      DRIFT_BOUNDS.
"""
import os

import numpy as np
import pytest
import torch

from oracle import make_golden as G
from oracle import make_golden_full as GF
from oracle import make_golden_drift as GD
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.api import TextToSpeech, calm_trim_length
from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, VocoderConfig
from tortoise_tts_amd.schedule import Schedule
from tests.gpu_util import DTYPES, quantize_sd, rel_err, max_err
from tests.test_gpu_parity_r3 import DRIFT_BOUNDS, GOLD, denorm

pytestmark = pytest.mark.gpu

# reduced-width case: 48 mel tokens give S = 48 * 4 * 24000 // 22050 = 208 positions; SEED is one whose three winners all keep more than
# 128 positions after the calm-token trim (asserted below; with this stop-token boost they run to the full 208, seeds 1 .. 8 all do)
REDUCED_TOKENS, REDUCED_EOS_BOOST, SEED = 48, 1.0, 5


def reduced_instances(tdt, dtype_name):
    a_cfg, c_cfg, d_cfg, v_cfg = ARConfig(**G.AR_CFG), CLVPConfig(**G.CLVP_CFG), DiffusionConfig(**G.DIFF_CFG), VocoderConfig()
    sds = {"autoregressive": quantize_sd(G.sampling_state_dict(a_cfg, REDUCED_EOS_BOOST), tdt),
           "clvp": quantize_sd(W.synthetic_state_dict(W.clvp_manifest(c_cfg), seed=G.CLVP_SEED), tdt),
           "diffusion": quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(d_cfg), seed=G.DIFF_SEED), tdt),
           "vocoder": quantize_sd(W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(v_cfg), seed=G.VOC_SEED)), tdt)}
    kw = dict(state_dicts=sds, configs={"ar": a_cfg, "clvp": c_cfg, "diffusion": d_cfg, "vocoder": v_cfg}, dtype=dtype_name, kv_cache=True,
              max_candidates=8, max_mel_tokens=REDUCED_TOKENS, max_text_tokens=40)
    cond, text = G.ar_inputs(a_cfg)
    dcond = torch.randn(1, 2 * d_cfg.model_channels, generator=torch.Generator().manual_seed(97)) * 0.5
    return TextToSpeech(**kw), TextToSpeech(winner_batch=3, **kw), text[0].tolist(), (cond, dcond)


def winner_positions(tts):
    """Positions of each ranked winner's mel: its calm-token trim times 4 * 24000 / 22050 (api.py:122)."""
    return [calm_trim_length(row) * 4 * 24000 // 22050 for row in tts.last_best_codes.cpu()]


def close(*instances):
    for t in instances:
        for st in (t.ar, t.clvp, t.diffusion, t.vocoder):
            st.close()


@pytest.mark.parametrize("cond_free", [True, False])
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_reduced_width_winner_batch_is_bit_identical_to_the_serial_path(name, dt, tdt, tol, cond_free):
    serial, batched, text, lat = reduced_instances(tdt, {"bf16": "bf16", "f16": "fp16"}[name])
    assert serial.winner_batch == 1 and batched.winner_batch == 3
    kw = dict(conditioning_latents=lat, k=3, num_autoregressive_samples=8, max_mel_tokens=REDUCED_TOKENS, diffusion_iterations=6,
              cond_free=cond_free, use_deterministic_seed=SEED, verbose=False)
    want = serial.tts(text, **kw)
    got = batched.tts(text, **kw)
    pos = winner_positions(serial)
    print(f"[parity] winner_batch=3 reduced width {name} cond_free={cond_free}: winners keep {pos} positions")
    assert torch.equal(batched.last_best_codes, serial.last_best_codes)
    assert min(pos) > 128, f"a winner keeps {min(pos)} <= 128 positions: alone it gets another attention kernel than in the batch (pick another SEED)"
    assert [w.shape[-1] for w in want] == [p * 256 for p in pos]
    for i, (a, b) in enumerate(zip(got, want)):
        same = a.shape == b.shape and torch.equal(a, b)
        print(f"[parity] winner_batch=3 reduced width {name} cond_free={cond_free} winner {i}: equal to the serial clip: {same}")
        assert same, f"winner {i} rendered in the batch differs from the serial path"
    close(serial, batched)


@pytest.fixture(scope="module")
def sds():
    import bench
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    return bench.synthetic_weights()


def _spy_mels(tts, sink):
    """Record every mel handed to the vocoder, by either entry."""
    one, many = tts.vocoder.inference, tts.vocoder.inference_many
    tts.vocoder.inference = lambda mel, z: (sink.append(mel.clone()), one(mel, z))[1]
    tts.vocoder.inference_many = lambda items: (sink.extend(m.clone() for m, _ in items), many(items))[1]


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_full_width_winner_batch_agrees_with_the_serial_path(sds, name, dt, tdt, tol):
    """At the benchmarked width the batched denoiser is another equally valid evaluation (DiffusionStage.sample_many): same winners, mels
    within the operand tolerance of the type (fp16: 8x tighter - what tells a masking error from rounding noise), waveforms within the
    8e-2 rel-L2 tests/test_gpu_full.py holds tts_many to (there is no fp16 waveform bar in the project: the same one, which can only be looser)."""
    import bench
    text, latents = bench.synthetic_prompt()
    kw0 = dict(state_dicts=sds, dtype={"bf16": "bf16", "f16": "fp16"}[name], max_candidates=16, max_mel_tokens=64, kv_cache=True)
    serial, batched = TextToSpeech(**kw0), TextToSpeech(winner_batch=3, **kw0)
    mels_s, mels_b = [], []
    _spy_mels(serial, mels_s)
    _spy_mels(batched, mels_b)
    kw = dict(conditioning_latents=latents, k=3, num_autoregressive_samples=16, diffusion_iterations=5, max_mel_tokens=36,
              use_deterministic_seed=7, verbose=False)
    want = serial.tts(text, **kw)
    got = batched.tts(text, **kw)
    assert torch.equal(batched.last_best_codes, serial.last_best_codes)
    assert len(mels_s) == len(mels_b) == 3 and len(got) == len(want) == 3
    for i in range(3):
        r, m = rel_err(mels_b[i], mels_s[i]), max_err(mels_b[i], mels_s[i])
        rw = rel_err(got[i], want[i])
        print(f"[parity] FULL-WIDTH winner_batch=3 {name} winner {i} S={mels_s[i].shape[-1]}: mel rel_l2={r:.3e} max_abs={m:.3e} (tol {tol:.1e}); "
              f"waveform rel_l2={rw:.3e} (bar 8.0e-02)")
        assert torch.isfinite(got[i]).all() and got[i].shape == want[i].shape
        assert r < tol, f"{name} winner {i}: mel rel_l2 {r:.3e} >= {tol:.1e}"
        assert rw < 8e-2, f"{name} winner {i}: waveform rel_l2 {rw:.3e} >= 8e-2"
    close(serial, batched)


@pytest.mark.parametrize("case", ["std200", "fast80"])
@torch.no_grad()
def test_batched_denoiser_vs_reference_loop(sds, case):
    """tt_diff_sample_batch at full width against the reference's fp32 p_sample_loop: the benchmarked utterance inside ragged batches,
    held to the bounds of the solo run (tests/test_gpu_parity_r3.py DRIFT_BOUNDS: about twice the solo measurement, 8.6e-3 bf16 /
    1.1e-3 fp16 rel-L2)."""
    g = np.load(os.path.join(GOLD, "full_drift.npz"))
    assert case in g.files, f"{case} not in full_drift.npz"
    _, N, cond_free, seed = [c for c in GD.CASES if c[0] == case][0]
    cfg = DiffusionConfig()
    _, _, cond = GF.prompt()
    S, latents, x, step_noise = GF.diff_inputs(cfg, M=GF.DIFF_M, seed=seed, steps=N)
    want = denorm(torch.from_numpy(g[case]))
    main = (latents, cond, S, x, step_noise)

    def neighbour(M, sd_):
        S2, lat2, x2, nz2 = GF.diff_inputs(cfg, M=M, seed=sd_, steps=N)
        return (lat2, cond, S2, x2, nz2)
    nb1, nb2 = neighbour(150, seed + 100), neighbour(90, seed + 200)
    assert nb1[2] < S and nb2[2] < nb1[2]
    sched = Schedule(N, 4000, cond_free, 2.0)
    batches = (("slot 0 of 2", [main, nb1], 0), ("slot 0 of 3", [main, nb1, nb2], 0), ("last slot of 3", [nb2, nb1, main], 2))
    for name, dt, tdt, tol in DTYPES:
        rb, mb = DRIFT_BOUNDS[(case, name)]
        st = stages.DiffusionStage(sds["diffusion"], cfg, dtype=dt, max_seq=S + 8, max_codes=GF.DIFF_M + 8, max_steps=N, max_batch=3)
        failed = []
        for label, items, at in batches:
            mel = st.sample_many(sched, items)[at].cpu()
            r, m = rel_err(mel, want), max_err(mel, want)
            print(f"[parity] FULL-WIDTH batched denoiser {case} ({N} iterations, cond_free={cond_free}) S=870 as {label} {name} vs reference "
                  f"p_sample_loop: mel rel_l2={r:.3e} max_abs={m:.3e} (bounds {rb:.1e} / {mb:.2f})")
            assert torch.isfinite(mel).all()
            if not (r < rb and m < mb):
                failed.append(f"{label}: rel_l2 {r:.3e} (bound {rb:.1e}) max_abs {m:.3e} (bound {mb})")
        st.close()
        assert not failed, f"{case} {name}: " + "; ".join(failed)
