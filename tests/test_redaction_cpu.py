"""Redaction of [bracketed] text without a GPU: the resampler's tap table, max_alignment, the CTC tokenizer, align / redact, the aligner's
weight source and packing, the boundary header, and the tts() / tts_many() flow with an aligner stand-in backed by transformers'
Wav2Vec2ForCTC - each against the transcription of the reference (tests/w2v_reference.py)."""
import ctypes as C
import json
import os
import random
import re

import pytest
import torch

from tests import fake_stages
from tests import w2v_reference as R
from tortoise_tts_amd import align
from tortoise_tts_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- resampler
def test_resample_taps_and_length_match_torchaudio():
    want, width = R.sinc_resample_kernel()
    assert width == 10 and want.shape == (2, 1, 23)
    assert torch.equal(align.resample_taps(), want.reshape(2, 23))
    g = torch.Generator().manual_seed(0)
    for S in (1, 2, 3, 4, 5, 600, 601, 602, 24000, 24001, 55555):
        x = torch.randn(1, S, generator=g)
        ref = R.resample(x)
        assert ref.shape[-1] == align.resampled_length(S)
        # the polyphase form the device kernel computes: y[2 f + p] = sum_t taps[p][t] x[3 f + t - 10]
        taps = align.resample_taps()
        xp = torch.nn.functional.pad(x[0], (10, 13))
        frames = xp.unfold(0, 23, 3)  # [S // 3 + 1][23]
        y = (frames[:, None, :] * taps[None]).sum(-1).reshape(-1)[: align.resampled_length(S)]
        assert torch.allclose(y, ref[0], atol=1e-6, rtol=1e-5)


def test_frame_count():
    cfg = R.small_config()
    m = R.hf_model(cfg)
    for S in (599, 600, 601, 1000, 24000, 33333):
        assert align.frames_for(S) == R.model_logits(m, R.test_clip(S / 24000.0)[:, :S]).shape[0]
    assert align.frames_for(598) == 0


# ----------------------------------------------------------------------------------------- max_alignment
def test_max_alignment_equals_the_recursive_reference():
    rng = random.Random(1)
    for _ in range(4000):
        a = "".join(rng.choice("abc ") for _ in range(rng.randint(0, 10)))
        b = "".join(rng.choice("abcd ") for _ in range(rng.randint(0, 10)))
        r = rng.random()
        if r < 0.05:
            b = a
        elif r < 0.1:
            a = ""
        elif r < 0.15:
            b = ""
        assert align.max_alignment(a, b) == R.max_alignment(a, b), (a, b)
    # ties: equal scores either way take the skip of s1
    assert align.max_alignment("ab", "ba") == R.max_alignment("ab", "ba")
    # a long text the recursion cannot take (Python's recursion limit) still aligns
    long1 = "the quick brown fox jumps over the lazy dog " * 40
    assert align.max_alignment(long1, long1.replace("o", "")).replace("~", "") == long1.replace("o", "")
    with pytest.raises(ValueError):
        align.max_alignment("a~b", "ab")


# ----------------------------------------------------------------------------------------- CTC tokenizer
@pytest.mark.parametrize("clean_up", [True, False])
def test_ctc_tokenizer_matches_transformers(tmp_path, clean_up):
    hf = R.hf_tokenizer(tmp_path, clean_up)
    ours = align.CtcTokenizer(R.VOCAB, dict(R.TOK_CFG, clean_up_tokenization_spaces=clean_up))
    rng = random.Random(2)
    V = len(R.VOCAB)
    for _ in range(500):
        ids = [rng.choice([0, 0, 0, 4, rng.randrange(V)]) for _ in range(rng.randint(0, 40))]
        assert ours.decode(ids) == hf.decode(ids), ids
        text = "".join(rng.choice("abc de,.'?!~Q ") for _ in range(rng.randint(1, 20)))
        assert ours.encode(text) == hf.encode(text), text
    # tokenizer_config.json without the flag: True (the default of the transformers release the reference ran under)
    assert align.CtcTokenizer(R.VOCAB, {}).cleanup is True
    assert align.CtcTokenizer(R.VOCAB, {}).decode([5, 4, 32]) == "a."


# ----------------------------------------------------------------------------------------- align / redact
def _frames(tok, pieces, rng):
    """frame ids spelling `pieces` CTC-style: every character 1-3 frames, blanks in between."""
    ids = [0, 0]
    for ch in pieces:
        ids += [tok.encode(ch)[0]] * rng.randint(1, 3) + [0] * rng.randint(0, 2)
    return ids


@pytest.mark.parametrize("text,spoken", [
    ("[i am so sad,] hello there", "i am so sad, hello there"),        # leading bracketed span
    ("hello there [said the cat]", "hello there said the cat"),         # trailing
    ("one [two] three [four] five", "one two three four five"),         # two spans
    ("[a][b]c", "abc"),                                                  # empty kept pieces
    ("a[b]", "ab"),
    ("x", "x"),                                                          # no bracket
    ("[hidden] hello wrld", "hidden hello world"),                      # unmatched characters: interpolated
    ("[dog] cat", "dgo ct"),
])
def test_redact_matches_the_reference(text, spoken):
    tok = align.CtcTokenizer(R.VOCAB, R.TOK_CFG)
    rng = random.Random(len(text))
    for trial in range(5):
        ids = _frames(tok, spoken, rng)
        audio = torch.randn(1, len(ids) * 320 + rng.randint(0, 319))
        try:
            want = R.redact(audio, text, lambda a: torch.tensor(ids), tok)
        except AssertionError:
            with pytest.raises((RuntimeError, ValueError)):
                align.redact(audio, text, lambda a: ids, tok)
            continue
        got = align.redact(audio, text, lambda a: ids, tok)
        assert torch.equal(got, want)
        if "[" in text:
            bare = text.replace("[", "").replace("]", "")
            assert align.alignments_from_frames(ids, tok, bare, audio.shape[-1]) == R.align_from_logits(torch.tensor(ids), tok, bare, audio.shape[-1])


def test_single_token_text_and_failure_paths():
    tok = align.CtcTokenizer(R.VOCAB, R.TOK_CFG)
    audio = torch.randn(1, 32000)
    ids = [0, 5, 5, 0, 6, 0] * 10
    assert align.alignments_from_frames(ids, tok, "a", 32000) == R.align_from_logits(torch.tensor(ids), tok, "a", 32000) == [0]
    with pytest.raises(ValueError, match="paired"):
        align.redact(audio, "hello [there", lambda a: ids, tok)
    with pytest.raises(ValueError, match="nothing"):
        align.redact(audio, "[hello there]", lambda a: ids, tok)
    # an alignment the algorithm cannot complete (the aligner heard "<unk>"): the reference asserts (and writes alignment_debug.pth);
    # here RuntimeError, no file
    cwd = os.getcwd()
    with pytest.raises(AssertionError):
        R.redact(audio, "[aa]k", lambda a: torch.tensor([3]), tok)
    with pytest.raises(RuntimeError, match="align"):
        align.redact(audio, "[aa]k", lambda a: [3], tok)
    assert not os.path.exists(os.path.join(cwd, "alignment_debug.pth"))
    assert align.redact(audio, "no brackets here", lambda a: 1 / 0, tok) is audio


# ----------------------------------------------------------------------------------------- weight source
def _write_model(d, cfg, sd, fmt):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    else:
        torch.save(sd, os.path.join(d, "pytorch_model.bin"))


def _write_tokenizer(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(R.VOCAB, f)
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(R.TOK_CFG, f)


def _old_naming(sd):
    """transformers 4.x names of the positional conv's weight norm (weight_g / weight_v)."""
    p = "wav2vec2.encoder.pos_conv_embed.conv."
    out = {k: v for k, v in sd.items() if "parametrizations" not in k}
    out[p + "weight_g"] = sd[p + "parametrizations.weight.original0"]
    out[p + "weight_v"] = sd[p + "parametrizations.weight.original1"]
    return out


def _packed(src):
    from tortoise_tts_amd import pack
    cfg, sd, vocab, tok_cfg = src
    h = pack.pack_w2v(sd, align.check_config(cfg), torch.device("cpu"), E.TT_F16)
    return [t.clone() for t in h.keep]


def test_loader_reads_every_layout_into_the_same_packed_weights(tmp_path, monkeypatch):
    cfg = R.small_config()
    sd = {k: v.detach().clone() for k, v in R.hf_model(cfg).state_dict().items()}
    ref = _packed((cfg, sd, R.VOCAB, R.TOK_CFG))
    for i, (fmt, naming) in enumerate((("safetensors", sd), ("bin", sd), ("bin", _old_naming(sd)), ("safetensors", _old_naming(sd)))):
        md = tmp_path / f"m{i}"
        _write_model(str(md / align.ALIGNER_MODEL), cfg, naming, fmt)
        _write_tokenizer(str(md / align.ALIGNER_TOKENIZER))
        src = align.find_aligner(str(md))
        assert src is not None and src[2] == R.VOCAB and src[3]["word_delimiter_token"] == "|"
        got = _packed(src)
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))
    # nothing under models_dir: the HF hub cache snapshots ($HF_HUB_CACHE, else $HF_HOME/hub)
    hub = tmp_path / "home" / "hub"
    _write_model(str(hub / f"models--jbetker--{align.ALIGNER_MODEL}" / "snapshots" / "abc123"), cfg, sd, "bin")
    _write_tokenizer(str(hub / f"models--jbetker--{align.ALIGNER_TOKENIZER}" / "snapshots" / "def456"))
    monkeypatch.delenv("HF_HUB_CACHE", raising=False)
    monkeypatch.setenv("HF_HOME", str(tmp_path / "home"))
    src = align.find_aligner(str(tmp_path / "empty"))
    assert src is not None and all(torch.equal(a, b) for a, b in zip(_packed(src), ref))
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "nowhere"))
    assert align.find_aligner(str(tmp_path / "empty")) is None


def test_unsupported_configs_are_refused():
    bare = {k: v for k, v in R.large_config().items() if k not in ("feat_extract_norm", "do_stable_layer_norm", "conv_bias")}
    with pytest.raises(ValueError, match="feat_extract_norm"):  # an omitted key is Wav2Vec2Config's default ("group"), not the supported value
        align.check_config(bare)
    with pytest.raises(ValueError, match="conv_dim"):
        align.check_config(R.large_config(conv_dim=None))
    with pytest.raises(ValueError, match="feat_extract_norm"):
        align.check_config(R.large_config(feat_extract_norm="group"))
    with pytest.raises(ValueError, match="do_stable_layer_norm"):
        align.check_config(R.large_config(do_stable_layer_norm=False))
    with pytest.raises(ValueError, match="hidden_act"):
        align.check_config(R.large_config(hidden_act="relu"))
    with pytest.raises(ValueError, match="num_attention_heads"):
        align.check_config(R.large_config(num_attention_heads=8))
    f = align.check_config(R.large_config())
    assert (f["dim"], f["heads"], f["layers"], f["ff_dim"], f["pos_kernel"], f["pos_groups"]) == (1024, 16, 24, 4096, 128, 16)


# ----------------------------------------------------------------------------------------- boundary
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ttx?_[a-z0-9_]+)\s*\(", src)))


def test_align_header_is_exported_and_mirrored():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    lib = E.load_library()
    names = _declared("tortoise_mi355x_align.h")
    assert set(names) == set(E._ALIGN_PROTOS) and all(hasattr(lib, n) for n in names)
    assert not set(names) & set(E._PROTOS)  # the drop-in boundary header is unchanged
    for i, st in enumerate(E.ALIGN_STRUCTS):
        assert C.sizeof(st) == lib.tt_align_struct_size(i), st.__name__
    assert lib.tt_align_abi_version() == 1
    for n in ("tt_op_w2v_resample", "tt_op_w2v_conv0", "tt_op_layernorm_act", "tt_op_w2v_argmax"):
        assert n in _declared("tortoise_mi355x_test.h") and n in E._TEST_PROTOS


# ----------------------------------------------------------------------------------------- tts() flow
class FakeAlignerStage:
    """CPU stand-in of stages.AlignerStage: the frame ids of transformers' Wav2Vec2ForCTC on the reference's resample + normalisation."""
    built = []

    def __init__(self, source, device="cpu", dtype=E.TT_F16, max_samples=0):
        from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
        cfg, sd, vocab, tok_cfg = source
        align.check_config(cfg)
        self.model = Wav2Vec2ForCTC(Wav2Vec2Config(**cfg)).eval()
        self.model.load_state_dict(sd)
        self.model.config._attn_implementation = "eager"
        self.tokenizer = align.CtcTokenizer(vocab, tok_cfg)
        self.dtype = dtype
        FakeAlignerStage.built.append(self)

    def frame_ids(self, audio):
        return R.model_logits(self.model, audio.reshape(1, -1).float().cpu()).argmax(-1).tolist()

    def guard(self, reset=True):
        return 0

    def close(self):
        pass


class _TextTokenizer:
    def encode(self, text):
        return [10 + (ord(c) % 20) for c in text][:20]


def _flow_tts(monkeypatch, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "AlignerStage", FakeAlignerStage)
    sds, cfgs = small_setup()
    cfg = R.small_config()
    m = R.hf_model(cfg, seed=3)
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, aligner=(cfg, m.state_dict(), R.VOCAB, R.TOK_CFG), **kw)
    t._tokenizer = _TextTokenizer()
    return t, m


@torch.no_grad()
def test_tts_redacts_every_candidate_like_the_reference(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    t, m = _flow_tts(monkeypatch)
    lat = voice_latents(small_setup()[1])
    text = "[I am so sad,] hello there"
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, use_deterministic_seed=7,
              verbose=False, k=2)
    assert t.aligner is None  # built on first use
    t.enable_redaction = False
    plain = t.tts(text, **kw)
    assert t.aligner is None and "redact_s" not in t.timings
    t.enable_redaction = True
    got = t.tts(text, **kw)
    assert t.aligner is not None and "redact_s" in t.timings
    tok = align.CtcTokenizer(R.VOCAB, R.TOK_CFG)
    for p, g_ in zip(plain, got):
        want = R.redact(p[0], text, lambda a: R.model_logits(m, a), tok)[None]
        assert torch.equal(g_, want) and g_.shape[-1] < p.shape[-1]
    # text without '[' runs the same path: the aligner is not consulted
    t.aligner.frame_ids = lambda a: 1 / 0
    t.tts("hello there", **kw)
    with pytest.raises(ValueError, match="paired"):
        t.tts("hello [there", **kw)
    with pytest.raises(ValueError, match="nothing"):
        t.tts("[hello there]", **kw)


@torch.no_grad()
def test_tts_many_redacts_per_utterance(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    lat = voice_latents(small_setup()[1])
    kw = dict(num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32)
    texts = ["[so sad] hello", "plain words", "one [two] three"]
    for ub in (1, 2):
        t, _ = _flow_tts(monkeypatch, candidate_sharding=False, utterance_batch=ub)
        many = t.tts_many(texts, conditioning_latents=lat, use_deterministic_seed=5, **kw)
        assert "redact_s" in t.timings
        one = [t.tts(x, conditioning_latents=lat, use_deterministic_seed=5, verbose=False, **kw) for x in texts]
        assert all(torch.equal(a, b) for a, b in zip(many, one))


def test_missing_aligner_files_still_refuse_brackets(monkeypatch):
    from tests.test_api_flow_cpu import VOCAB, small_setup
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setenv("HF_HUB_CACHE", "/nonexistent/hub")
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40)
    with pytest.raises(NotImplementedError, match="bracket") as ei:
        t.tts("[I am so sad,] hello", num_autoregressive_samples=4, diffusion_iterations=3, max_mel_tokens=24)
    assert align.ALIGNER_MODEL in str(ei.value) and "/nonexistent" in str(ei.value)
