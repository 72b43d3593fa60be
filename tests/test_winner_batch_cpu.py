"""CPU checks of TextToSpeech(winner_batch=W) on the oracle-backed stand-ins: the k winners of tts() rendered in groups of up to W (one
sample_many pass + one inference_many call per group) equal the serial path clip by clip; grouping, the single path for one winner,
noise_override, return_deterministic_state, redaction, the argument range, the fallback without inference_many, and the new header's
symbols.  The device side is tests/test_gpu_univnet_batch.py and tests/test_gpu_winner_batch.py."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import fake_stages
from tests.test_api_flow_cpu import VOCAB, small_setup, voice_latents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = list(range(10, 31))
KW = dict(num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, use_deterministic_seed=5, verbose=False)


class BatchingVocoderStage(fake_stages.FakeVocoderStage):
    """The stand-in vocoder with inference_many, recording every batched call (the mel lengths it was given) and every single call."""
    calls = []
    singles = []

    def inference(self, mel, z):
        BatchingVocoderStage.singles.append(int(mel.shape[-1]))
        return super().inference(mel, z)

    def inference_many(self, items):
        BatchingVocoderStage.calls.append([int(mel.shape[-1]) for mel, _ in items])
        return [fake_stages.FakeVocoderStage.inference(self, mel, z) for mel, z in items]


def install(monkeypatch, batching=True):
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    if batching:
        monkeypatch.setattr(api.stages, "VocoderStage", BatchingVocoderStage)
    BatchingVocoderStage.calls, BatchingVocoderStage.singles = [], []
    return api


def make(api, **kw):
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, **kw)
    return t, voice_latents(cfgs)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@torch.no_grad()
def test_three_winners_in_one_pass_equal_the_serial_path(monkeypatch):
    api = install(monkeypatch)
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    assert not getattr(serial.diffusion, "batched", []) and not BatchingVocoderStage.calls and len(BatchingVocoderStage.singles) == 3
    assert serial.diffusion.max_batch == 1
    batched, _ = make(api, winner_batch=3)
    assert batched.diffusion.max_batch == 3
    got = batched.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    assert isinstance(got, list) and same(got, want)
    assert batched.diffusion.batched == [3]
    assert len(BatchingVocoderStage.calls) == 1 and len(BatchingVocoderStage.calls[0]) == 3 and len(BatchingVocoderStage.singles) == 3
    assert torch.equal(batched.last_best_codes, serial.last_best_codes)
    assert set(batched.timings) >= {"ar_s", "clvp_s", "latents_s", "diffusion_s", "vocoder_s", "total_s"}


@torch.no_grad()
def test_five_winners_two_at_a_time(monkeypatch):
    api = install(monkeypatch)
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=5, **KW)
    batched, _ = make(api, winner_batch=2)
    BatchingVocoderStage.calls, BatchingVocoderStage.singles = [], []
    got = batched.tts(TEXT, conditioning_latents=lat, k=5, **KW)
    assert same(got, want)
    assert batched.diffusion.batched == [2, 2]  # groups of 2, 2 and 1: the last winner alone through sample() / inference()
    assert [len(c) for c in BatchingVocoderStage.calls] == [2, 2] and len(BatchingVocoderStage.singles) == 1


@torch.no_grad()
def test_one_winner_takes_the_single_path(monkeypatch):
    api = install(monkeypatch)
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=1, **KW)
    batched, _ = make(api, winner_batch=3)
    BatchingVocoderStage.calls, BatchingVocoderStage.singles = [], []
    got = batched.tts(TEXT, conditioning_latents=lat, k=1, **KW)
    assert torch.is_tensor(got) and torch.equal(got, want)
    assert not getattr(batched.diffusion, "batched", []) and not BatchingVocoderStage.calls and len(BatchingVocoderStage.singles) == 1


@torch.no_grad()
def test_noise_override_and_deterministic_state_behave_as_in_the_serial_path(monkeypatch):
    api = install(monkeypatch)
    serial, lat = make(api)
    batched, _ = make(api, winner_batch=3)
    # noise_override: every winner gets the SAME supplied draws, which fixes every length to the shortest trim's - so supply z only
    # (its length must match every winner: take the seeds' own lengths first)
    plain = serial.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    S = {w.shape[-1] // 256 for w in plain}
    kw = dict(KW, return_deterministic_state=True)
    if len(S) == 1:  # all winners of this seed trim to one length: x_T / step_noise / z can be supplied
        S = S.pop()
        g = torch.Generator().manual_seed(1)
        noise = {"x_T": torch.randn(1, 100, S, generator=g), "step_noise": torch.randn(3, 1, 100, S, generator=g),
                 "z": torch.randn(1, 64, S + 10, generator=g)}
    else:
        g = torch.Generator().manual_seed(1)
        noise = {"exp_noise": torch.empty(32, 8, serial.ar_cfg.number_mel_codes).exponential_(1, generator=g)}
    want, wstate = serial.tts(TEXT, conditioning_latents=lat, k=3, noise_override=noise, **kw)
    got, gstate = batched.tts(TEXT, conditioning_latents=lat, k=3, noise_override=noise, **kw)
    assert same(got, want) and not same(want, plain)
    assert gstate[0] == wstate[0] == 5 and gstate[1] == TEXT and gstate[3] is lat


def test_winner_batch_range(monkeypatch):
    api = install(monkeypatch)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="winner_batch"):
            make(api, winner_batch=bad)
    t, _ = make(api, winner_batch=16)
    assert t.winner_batch == 16 and t.diffusion.max_batch == 16
    t, _ = make(api, winner_batch=2, utterance_batch=4, candidate_sharding=False)
    assert t.diffusion.max_batch == 4


@torch.no_grad()
def test_stage_without_inference_many_falls_back_to_per_clip_calls(monkeypatch):
    api = install(monkeypatch, batching=False)  # tests/fake_stages.py's vocoder: no inference_many
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    batched, _ = make(api, winner_batch=3)
    assert not hasattr(batched.vocoder, "inference_many")
    got = batched.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    assert same(got, want) and batched.diffusion.batched == [3]


@torch.no_grad()
def test_tts_many_vocodes_a_wave_in_one_call(monkeypatch):
    """_render_wave hands a wave's mels to inference_many when the vocoder has it; the clips equal tts() per text."""
    api = install(monkeypatch)
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, candidate_sharding=False, utterance_batch=2)
    lat = voice_latents(cfgs)
    texts = [list(range(30, 40)), list(range(41, 49)), list(range(10, 31))]
    want = [t.tts(x, conditioning_latents=lat, **KW) for x in texts]
    BatchingVocoderStage.calls = []
    got = t.tts_many(texts, conditioning_latents=lat, **{k: v for k, v in KW.items() if k != "verbose"})
    assert same(got, want)
    assert [len(c) for c in BatchingVocoderStage.calls] == [2]  # a wave of two in one call, the third utterance alone


@torch.no_grad()
def test_bracketed_text_is_redacted_as_in_the_serial_path(monkeypatch):
    """keep_on_device: the batched winners stay where the aligner reads them and every clip loses its [bracketed] passage."""
    pytest.importorskip("transformers")
    from tests.test_redaction_cpu import _flow_tts
    text = "[I am so sad,] hello there"
    kw = dict(num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, use_deterministic_seed=7, verbose=False, k=2)
    serial, _ = _flow_tts(monkeypatch)
    lat = voice_latents(small_setup()[1])
    want = serial.tts(text, conditioning_latents=lat, **kw)
    serial.enable_redaction = False
    plain = serial.tts(text, conditioning_latents=lat, **kw)
    batched, _ = _flow_tts(monkeypatch, winner_batch=2)
    got = batched.tts(text, conditioning_latents=lat, **kw)
    assert batched.diffusion.batched == [2]
    assert same(got, want) and any(a.shape != b.shape for a, b in zip(want, plain))
    assert "redact_s" in batched.timings


def test_univnet_batch_header_symbols_are_exported_and_bound():
    from tortoise_tts_amd import engine as E
    lib = E.load_library()
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_univnet.h")).read()
    names = set(re.findall(r"^(?:int|size_t|void)\s+\*?(tt_\w+)\(", src, re.M))
    assert names == set(E._UNIVNET_PROTOS) == {"tt_voc_batch_abi_version", "tt_voc_batch_struct_size", "tt_voc_batch_capacity", "tt_voc_run_batch"}
    for n in names:
        assert hasattr(lib, n)
    assert lib.tt_voc_batch_abi_version() == 1
    for i, st in enumerate(E.VOC_BATCH_STRUCTS):
        assert C.sizeof(st) == lib.tt_voc_batch_struct_size(i), st.__name__
    assert int(re.search(r"#define TT_VOC_MAX_BATCH (\d+)", src).group(1)) == E.VOC_MAX_BATCH
    # the frozen drop-in header: same ABI number, same entry points
    assert lib.tt_abi_version() == 6 and not names & set(E._PROTOS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", main))
    assert declared == set(E._PROTOS) and len(declared) == 60  # (as before this header existed; tests/test_abi.py caps it at 60)
