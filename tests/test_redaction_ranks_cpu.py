"""Where redaction sits in tts(): after the overflow guards have accepted the utterance (a clip a demotion re-renders is never aligned), with
the fp16 aligner rebuilt in bf16 when its own guard trips, and - with several ranks - an alignment failure on one rank raised on every rank
together (no rank left waiting in a collective, the ranks still in step afterwards).  CPU stand-ins (tests/fake_stages.py), `gloo`."""
import json
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fake_stages
from tests import w2v_reference as R
from tortoise_tts_amd import align
from tortoise_tts_amd import dist as tdist
from tortoise_tts_amd import engine as E

TEXT = "[aa]kab"
KW = dict(num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=12, use_deterministic_seed=9, verbose=False)


class SpellingAligner:
    """Aligner stand-in: hears TEXT spelled CTC-style (so the alignment succeeds) - or only "<unk>" on rank `fail_rank` (the reference's
    alignment then fails).  `trips`: guard() reports that many overflows of an fp16 stage, once per stage built."""
    fail_rank = -1
    trips = 0
    built, calls = [], []

    def __init__(self, source, device="cpu", dtype=E.TT_F16, max_samples=0):
        self.tokenizer = align.CtcTokenizer(R.VOCAB, R.TOK_CFG)
        self.dtype = dtype
        self.tripped = False
        SpellingAligner.built.append(dtype)

    def frame_ids(self, audio):
        SpellingAligner.calls.append(audio.shape[-1])
        if tdist.world()[0] == SpellingAligner.fail_rank:
            return [3]
        ids = [0]
        for ch in TEXT.replace("[", "").replace("]", ""):
            ids += [self.tokenizer.encode(ch)[0], 0]
        return ids

    def guard(self, reset=True):
        if SpellingAligner.trips and not self.tripped and self.dtype == E.TT_F16:
            self.tripped = True
            return SpellingAligner.trips
        return 0

    def close(self):
        pass


class _TextTokenizer:
    def encode(self, text):
        return [10 + (ord(c) % 20) for c in text][:20]


def _tts(mp_, **kw):
    from tests.test_api_flow_cpu import small_setup
    fake_stages.install(mp_)
    from tortoise_tts_amd import api
    mp_.setattr(api.stages, "AlignerStage", SpellingAligner)
    sds, cfgs = small_setup()
    t = api.TextToSpeech(state_dicts=sds, configs=cfgs, max_mel_tokens=16, kv_cache=True, aligner=(R.small_config(), {}, R.VOCAB, R.TOK_CFG),
                         **kw)
    t._tokenizer = _TextTokenizer()
    return t, cfgs


@torch.no_grad()
def test_redaction_runs_after_the_guards_accepted_the_utterance(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents
    SpellingAligner.calls, SpellingAligner.built, SpellingAligner.fail_rank, SpellingAligner.trips = [], [], -1, 0
    t, cfgs = _tts(monkeypatch, max_candidates=8, half=True)
    lat = voice_latents(cfgs)
    t.tts(TEXT, conditioning_latents=lat, k=2, **KW)
    assert len(SpellingAligner.calls) == 2
    # the fp16 decode overflows once: the utterance is rendered again in bf16, and only the accepted clips are aligned
    monkeypatch.setattr(fake_stages.FakeArStage, "trip", 1, raising=False)
    SpellingAligner.calls = []
    got = t.tts(TEXT, conditioning_latents=lat, k=2, **KW)
    assert t.demotions == ["ar"] and len(SpellingAligner.calls) == 2 and all(g.shape[-1] < 12 * 256 * 4 for g in got)


@torch.no_grad()
def test_an_overflowing_fp16_aligner_is_rebuilt_in_bf16_and_aligns_the_same_clip_again(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents
    SpellingAligner.calls, SpellingAligner.built, SpellingAligner.fail_rank, SpellingAligner.trips = [], [], -1, 0
    t, cfgs = _tts(monkeypatch, max_candidates=8)
    lat = voice_latents(cfgs)
    want = t.tts(TEXT, conditioning_latents=lat, k=1, **KW)
    assert SpellingAligner.built == [E.TT_F16] and t.aligner_dtype == E.TT_F16
    t.aligner.close()
    t.aligner = None
    SpellingAligner.calls, SpellingAligner.built, SpellingAligner.trips = [], [], 2
    with pytest.warns(UserWarning, match="aligner"):
        got = t.tts(TEXT, conditioning_latents=lat, k=1, **KW)
    n = want.shape[-1]
    assert SpellingAligner.built == [E.TT_F16, E.TT_BF16] and t.aligner_dtype == E.TT_BF16 and t.aligner.dtype == E.TT_BF16
    assert len(SpellingAligner.calls) == 2 and SpellingAligner.calls[0] == SpellingAligner.calls[1]  # the same clip, not rendered again
    assert torch.equal(got, want) and n > 0
    assert set(t.dtype_names()) == {"ar", "clvp", "diffusion", "vocoder"}
    # a bf16 aligner that still overflows is an error, not a precision choice
    t.aligner.guard = lambda reset=True: 1
    with pytest.raises(E.OperandOverflow):
        t.tts(TEXT, conditioning_latents=lat, k=1, **KW)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    tdist.init_from_env()
    tdist._PAIR = None
    from tests.test_api_flow_cpu import voice_latents
    mp_ = pytest.MonkeyPatch()
    res = {}
    try:
        t, cfgs = _tts(mp_, max_candidates=8 // world)
        lat = voice_latents(cfgs)
        for name, fail_rank, k in (("k1_fail_on_0", 0, 1), ("k2_fail_on_1", 1, 2)):
            SpellingAligner.fail_rank = fail_rank
            try:
                t.tts(TEXT, conditioning_latents=lat, k=k, **KW)
                res[name] = "returned"
            except RuntimeError as ex:
                res[name] = "own" if "could not align" in str(ex) else "other" if "another rank" in str(ex) else str(ex)
        SpellingAligner.fail_rank = -1
        plain = t.tts("aakab", conditioning_latents=lat, k=2, **KW)  # the ranks are still in step
        red = t.tts(TEXT, conditioning_latents=lat, k=2, **KW)
        res["after"] = None if plain is None else [[p.shape[-1], r.shape[-1]] for p, r in zip(plain, red)]
    finally:
        mp_.undo()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    tdist.barrier()
    dist.destroy_process_group()


def test_an_alignment_failure_on_one_rank_raises_on_every_rank(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.time() + 600
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish: a rank is waiting in a collective")
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    # k = 1 with the split diffusion tail: only rank 0 renders (and aligns); rank 1 raises with it
    assert r0["k1_fail_on_0"] == "own" and r1["k1_fail_on_0"] == "other"
    # k = 2 round-robin: rank 1 renders winner 1 and fails; rank 0's alignment succeeded, it raises as well
    assert r0["k2_fail_on_1"] == "other" and r1["k2_fail_on_1"] == "own"
    assert r1["after"] is None and len(r0["after"]) == 2 and all(0 < red < plain for plain, red in r0["after"])
