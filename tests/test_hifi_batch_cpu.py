"""CPU checks of the host side of batched HiFi-GAN decoding on the oracle-backed stand-ins: api_fast.TextToSpeech.tts_many (rows admitted
as others finish, output order, seeds, random voices, refusals), stream_pieces' one batched vocoder call per round, read_long_form on a
fast-path instance (also over two gloo ranks), and the new header's symbols.  The device side is tests/test_gpu_hifi_batch.py."""
import os
import re

import pytest
import torch

from tests import fake_stages
from tests.test_wide_sessions_cpu import KW, TEXTS, WideSessionArStage, _instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTS_KW = dict(max_mel_tokens=24)


class BatchingHifiganStage(fake_stages.FakeHifiganStage):
    """The stand-in vocoder with inference_many, recording every batched call (the sequence lengths it was given)."""
    calls = []

    def inference_many(self, items):
        BatchingHifiganStage.calls.append([int(lat.shape[1]) for lat, _ in items])
        return [self.inference(lat, g) for lat, g in items]


class LatentSessionArStage(WideSessionArStage):
    """The wide session stand-in with tts()'s latent re-pass (the oracle's teacher-forced pass, as the single-stream stand-in has it)."""

    def latents(self, cond_latent, text_tokens, codes, stream_positions=False):
        sd, cfg, _, _, _ = self.args
        k = codes.shape[0]
        return fake_stages.O.ar_latents(sd, cfg, cond_latent.float().cpu().expand(k, -1), text_tokens.cpu().expand(k, -1), codes.cpu(),
                                        stream_positions=stream_positions)


def _batching(monkeypatch):
    api_fast, make = _instances(monkeypatch)
    monkeypatch.setattr(api_fast.stages, "ArStage", LatentSessionArStage)
    monkeypatch.setattr(api_fast.stages, "HifiganStage", BatchingHifiganStage)
    BatchingHifiganStage.calls = []
    return api_fast, make


@torch.no_grad()
def test_tts_many_on_sixteen_rows_equals_tts_loop(monkeypatch):
    """19 texts on 16 rows: three texts wait for a row, every clip equals tts() alone (same seeds), in text order, and the clips are vocoded
    through inference_many."""
    api_fast, make = _batching(monkeypatch)
    seeds = [40 + i for i in range(len(TEXTS))]
    one = make(1)
    want = [one.tts(t, use_deterministic_seed=s, **TTS_KW) for t, s in zip(TEXTS, seeds)]
    assert [w.shape for w in one.tts_many(TEXTS[:4], use_deterministic_seed=seeds[:4], **TTS_KW)] == [w.shape for w in want[:4]]
    many = make(16, wide_sessions=True)
    BatchingHifiganStage.calls = []
    got = many.tts_many(TEXTS, use_deterministic_seed=seeds, **TTS_KW)
    assert len(got) == len(TEXTS) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert len(many.ar.admits) == len(TEXTS) and [slot for slot, _, _ in many.ar.admits][:16] == list(range(16))
    assert len(BatchingHifiganStage.calls) == 1 and len(BatchingHifiganStage.calls[0]) == len(TEXTS)
    assert not many._sessions


@torch.no_grad()
def test_tts_many_one_seed_and_random_voices_follow_tts_order(monkeypatch):
    """One int seed for all texts and no voice: each text reseeds before its random voice is drawn, as tts() does."""
    api_fast, make = _batching(monkeypatch)
    one = make(1)
    want = [one.tts(t, use_deterministic_seed=9, **TTS_KW) for t in TEXTS[:6]]
    many = make(3)
    got = many.tts_many(TEXTS[:6], use_deterministic_seed=9, **TTS_KW)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_tts_many_refusals(monkeypatch):
    api_fast, make = _batching(monkeypatch)
    many = make(4)
    with pytest.raises(ValueError, match="seeds for"):
        many.tts_many(TEXTS[:3], use_deterministic_seed=[1, 2])
    with pytest.raises(NotImplementedError, match="unsupported generate kwargs"):  # (as tts() refuses it)
        many.tts_many(TEXTS[:3], not_an_argument=1)
    with pytest.raises(ValueError, match="max_mel_tokens"):
        many.tts_many(TEXTS[:3], max_mel_tokens=0)
    assert not many.ar.admits  # (no row was taken)
    many.open_stream(TEXTS[0], **KW)
    with pytest.raises(RuntimeError, match="streaming session"):
        many.tts_many(TEXTS[:2])


@torch.no_grad()
def test_stream_pieces_vocode_each_round_in_one_call(monkeypatch):
    """With a batching vocoder, every round whose pieces are due is one inference_many call holding every due session; the pieces and
    their order equal the one-at-a-time path (a stage without inference_many)."""
    api_fast, make = _instances(monkeypatch)
    seeds = [70 + i for i in range(8)]
    plain = make(16, wide_sessions=True)
    want = list(plain.tts_stream_many(TEXTS[:8], use_deterministic_seed=seeds, **KW))
    monkeypatch.setattr(api_fast.stages, "HifiganStage", BatchingHifiganStage)
    BatchingHifiganStage.calls = []
    many = make(16, wide_sessions=True)
    got = list(many.tts_stream_many(TEXTS[:8], use_deterministic_seed=seeds, **KW))
    assert [(i, d) for i, _, d in got] == [(i, d) for i, _, d in want]
    assert all(torch.equal(a, b) for (_, a, _), (_, b, _) in zip(got, want))
    assert BatchingHifiganStage.calls and max(len(c) for c in BatchingHifiganStage.calls) == 8  # (the first pieces of all eight at once)
    assert sum(len(c) for c in BatchingHifiganStage.calls) <= len(got)


@torch.no_grad()
def test_stream_pieces_mid_round_close_drops_the_computed_piece(monkeypatch):
    """A session closed between the yields of a round gets no piece that was vocoded for it in that round's batched call."""
    api_fast, make = _batching(monkeypatch)
    many = make(4)
    sids = [many.open_stream(t, use_deterministic_seed=5 + i, **KW) for i, t in enumerate(TEXTS[:3])]
    pieces = many.stream_pieces()
    first = next(pieces)
    assert len(BatchingHifiganStage.calls) == 1 and len(BatchingHifiganStage.calls[0]) == 3
    victim = [s for s in sids if s != first[0]][0]
    many.close_stream(victim)
    rest = list(pieces)
    assert all(sid != victim for sid, _, _ in rest)


@torch.no_grad()
def test_read_long_form_renders_fast_path_chunks_with_tts_many(monkeypatch):
    """A fast-path instance goes through one tts_many call with the agreed seed; the parts equal tts() per chunk."""
    from tortoise_tts_amd.longform import read_long_form
    api_fast, make = _batching(monkeypatch)
    one = make(1)
    chunks = [TEXTS[i] for i in range(5)]
    want = [one.tts(c, use_deterministic_seed=31, **TTS_KW) for c in chunks]
    many = make(3)
    seen = []
    orig = many.tts_many

    def spy(texts, **kw):
        seen.append((len(texts), kw.get("use_deterministic_seed")))
        return orig(texts, **kw)
    many.tts_many = spy
    full, parts = read_long_form(many, chunks, texts_are_chunks=True, seed=31, **TTS_KW)
    assert seen == [(5, 31)]
    assert all(torch.equal(a, b) for a, b in zip(parts, want))
    assert torch.equal(full, torch.cat([p.squeeze(0) for p in want], dim=-1))


def _rank(rank, world, port, out):
    import torch.distributed as dist
    from tortoise_tts_amd.longform import read_long_form
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mp = pytest.MonkeyPatch()
        api_fast, make = _batching(mp)
        many = make(2)
        calls = []
        orig = many.tts_many
        many.tts_many = lambda texts, **kw: (calls.append((len(texts), kw.get("use_deterministic_seed"))), orig(texts, **kw))[1]
        full, parts = read_long_form(many, [TEXTS[i] for i in range(5)], texts_are_chunks=True, seed=100 + rank, **TTS_KW)
        torch.save({"calls": calls, "parts": parts}, os.path.join(out, f"rank{rank}.pt"))
        mp.undo()
    finally:
        dist.destroy_process_group()


def test_read_long_form_fast_path_over_two_gloo_ranks(tmp_path, monkeypatch):
    """World size 2: each rank renders its chunks (j % 2) with one tts_many call and rank 0's seed; rank 0 gets every part, equal to
    tts() per chunk."""
    import random
    import torch.multiprocessing as mp
    port = 29500 + random.randint(0, 2000)
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["calls"] == [(3, 100)] and r1["calls"] == [(2, 100)] and r1["parts"] is None
    api_fast, make = _batching(monkeypatch)
    one = make(1)
    want = [one.tts(TEXTS[i], use_deterministic_seed=100, **TTS_KW) for i in range(5)]
    assert all(torch.equal(a, b) for a, b in zip(r0["parts"], want))


def test_hifi_batch_header_symbols_are_exported_and_bound():
    from tortoise_tts_amd import engine as E
    lib = E.load_library()
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_hifi.h")).read()
    names = set(re.findall(r"^(?:int|size_t|void)\s+\*?(tt_\w+)\(", src, re.M))
    assert names == set(E._HIFI_PROTOS)
    for n in names:
        assert hasattr(lib, n)
    assert lib.tt_hifi_batch_abi_version() == 1
    assert "tt_op_gemm_segv" in E._TEST_PROTOS and hasattr(lib, "tt_op_gemm_segv")
    assert int(re.search(r"#define TT_HIFI_MAX_BATCH (\d+)", src).group(1)) == E.HIFI_MAX_BATCH
