"""CTC forced alignment without a GPU: the fp64 reference (tests/ctc_reference.py) against brute force, its tie-break, f32 against fp64 on the
input families the GPU tests use, the host logic of align.py / longform.py, the API flow with a stand-in stage backed by the reference, and
the new header."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from tests import ctc_reference as CR
from tests import fake_stages
from tests import w2v_reference as R
from tests.test_abi import declared_symbols
from tortoise_tts_amd import align
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import longform


# ----------------------------------------------------------------------------------------- the reference
def test_reference_equals_brute_force_enumeration():
    """Every T <= 7, every target of L <= 3 over a 4-symbol vocabulary (blank 0, repeats included): path and score."""
    rng = np.random.default_rng(0)
    n = 0
    for L in (1, 2, 3):
        for tg in itertools.product((1, 2, 3), repeat=L):
            for T in range(1, 8):
                x = rng.standard_normal((T, 4)) * 2
                got = CR.viterbi(x, tg, 0)
                if T < L + CR.repeats(tg):
                    assert got["status"] == CR.INFEASIBLE and CR.brute_force(x, tg, 0)[0] is None
                    continue
                path, score = CR.brute_force(x, tg, 0)
                assert got["status"] == CR.OK and got["path"].tolist() == path, (tg, T)
                assert abs(got["score"] - score) < 1e-12 and abs(CR.path_score(got["lp"], path, tg, 0) - score) < 1e-12
                assert CR.is_valid_path(path, tg, 0)
                n += 1
    assert n > 150
    assert CR.viterbi(np.zeros((0, 4)), [1], 0)["status"] == CR.EMPTY and CR.viterbi(np.zeros((3, 4)), [], 0)["status"] == CR.EMPTY


def test_tie_break_on_all_equal_logits():
    """Stay beats s - 1 beats s - 2: every state is entered as early as it can be, the rest of the clip sits in the final blank."""
    assert CR.viterbi(np.zeros((23, 8)), [1, 2, 3, 4, 5], 0)["path"].tolist() == [1, 3, 5, 7, 9] + [10] * 18
    assert CR.viterbi(np.zeros((7, 8)), [3, 3, 4], 0)["path"].tolist() == [1, 2, 3, 5, 6, 6, 6]
    assert CR.viterbi(np.zeros((4, 8)), [3, 3, 4], 0)["path"].tolist() == [1, 2, 3, 5]  # the single feasible path ends in the token
    for T, tg in ((23, [1, 2, 3, 4, 5]), (40, [2, 2, 2, 5, 5, 1]), (300, list(range(1, 31)) * 5)):
        for dtype in (np.float64, np.float32):
            assert CR.viterbi(np.zeros((T, 32)), tg, 0, dtype)["path"].tolist() == CR.tie_break_path(T, tg)


def test_scores_equal_torchaudio_forced_align():
    ta = pytest.importorskip("torchaudio")
    if not hasattr(ta.functional, "forced_align"):
        pytest.skip("this torchaudio has no forced_align")
    for seed in range(6):
        x, tg = CR.random_clip(seed, tmax=120)
        lp = torch.from_numpy(CR.log_softmax(x, np.float32))[None]
        _, scores = ta.functional.forced_align(lp, torch.tensor([tg], dtype=torch.int32), blank=0)
        assert abs(float(scores.sum()) - CR.viterbi(x, tg, 0)["score"]) < 1e-3


def test_f32_recurrence_takes_the_fp64_path_on_the_test_families():
    """What lets the GPU tests demand exact paths on these seeds: the f32 form of the recurrence already agrees with fp64 on them, and its
    score sits inside score_bound."""
    for fam in (CR.random_clip, CR.planted_clip):
        for seed in range(40):
            x, tg = fam(seed)
            r64, r32 = CR.viterbi(x, tg, 0), CR.viterbi(x, tg, 0, np.float32)
            assert r32["path"].tolist() == r64["path"].tolist(), (fam.__name__, seed)
            lab = CR.labels(tg, 0)[r64["path"]]
            assert abs(r32["score"] - r64["score"]) <= CR.score_bound(len(x), r64["lp"], x, lab)
            assert np.all(np.abs(r32["conf"] - r64["conf"]) <= CR.conf_bound(r64["lp"], x, tg, r64["spans"]))


def test_bounds_come_from_the_format():
    x, tg = CR.random_clip(3)
    r = CR.viterbi(x, tg, 0)
    T = len(x)
    every, own = CR.score_bound(T, r["lp"], x), CR.score_bound(T, r["lp"], x, CR.labels(tg, 0)[r["path"]])
    assert 0 < own <= every < 1e-4 * abs(r["score"])  # a few hundred roundings of 2^-24 against the score
    assert every >= (T - 1) * CR.U32 * abs(r["score"])
    assert np.all(CR.lp_error(r["lp"], x) >= CR.U32 * np.abs(r["lp"]))


# ----------------------------------------------------------------------------------------- host logic
TOK = align.CtcTokenizer(R.VOCAB, R.TOK_CFG)


def test_alignment_targets():
    t = align.alignment_targets("Hi,  it's 42 ok!", align.CtcTokenizer(R.VOCAB, dict(R.TOK_CFG)))
    # 'H' is outside this lower-case vocabulary: dropped like the digits; the double space and the spaces around "42" collapse
    assert "".join(t.chars) == "i, it's ok!" and t.ids == [R.VOCAB[c if c != " " else "|"] for c in "i, it's ok!"]
    assert t.index[0] == -1 and not t.kept[0] and t.index[1] == 0 and t.kept[1]
    assert t.index[4] == t.index[3] and t.kept[3] and not t.kept[4]         # the second space
    assert [t.index[i] for i in (10, 11, 12)] == [t.index[9]] * 3           # "42 " inherits the delimiter before it
    assert all(a <= b for a, b in zip(t.index, t.index[1:])) and len(t.index) == len(t.kept) == 16
    up = align.alignment_targets("ab c", align.CtcTokenizer({"<pad>": 0, "|": 1, "A": 2, "B": 3, "C": 4}, {"do_lower_case": True}))
    assert up.ids == [2, 3, 1, 4] and up.chars == ["a", "b", " ", "c"]
    t = align.alignment_targets("  hello  ", TOK)
    assert "".join(t.chars) == "hello" and t.index == [-1, -1, 0, 1, 2, 3, 4, 4, 4] and t.kept[-2:] == [False, False]
    nothing = align.alignment_targets(" 123 456 ", TOK)
    assert nothing.ids == [] and set(nothing.index) == {-1}
    al = align.empty_alignment(nothing, 5000)
    assert al.chars == [] and [w[:3] for w in al.words] == [("123", 0, 0), ("456", 0, 0)] and all(math.isnan(w[3]) for w in al.words)
    assert align.blank_id(TOK) == 0


def _alignment(text, spans, conf, samples, frame_len=480):
    t = align.alignment_targets(text, TOK)
    assert len(spans) == len(t.ids)
    return align.build_alignment(t, spans, conf, -12.5, samples, frame_len)


def test_sample_mapping_and_word_grouping():
    assert align.frame_samples(align.check_config(R.small_config())) == 480
    assert align.frame_samples(dict(conv_stride=[5, 2, 2, 2, 2, 2, 1])) == 240
    #        h       i       |       7 (dropped)  y        o
    spans = [(1, 2), (3, 3), (6, 6), (8, 8), (9, 11)]
    al = _alignment("hi 7 yo", spans, [0.9, 0.5, 0.8, 0.7, 0.6], samples=5700)
    assert al.chars[0] == ("h", 480, 1440, 0.9) and al.chars[2] == (" ", 2880, 3360, 0.8)
    assert al.chars[-1] == ("o", 4320, 5700, 0.6)  # the last frame ends with the clip
    assert [w[:3] for w in al.words] == [("hi", 480, 1920), ("7", 1920, 1920), ("yo", 3840, 5700)]
    assert al.words[0][3] == 0.5 and math.isnan(al.words[1][3]) and al.words[2][3] == 0.6
    assert al.score == -12.5 and al.samples == 5700
    assert al.seconds()[0][:3] == ("hi", 0.02, 0.08)
    assert al.char_start(0) == 480 and al.char_end(1) == 1920 and al.char_start(3) == 3360 and al.char_end(3) == 3360  # '7' sits at the end of the delimiter
    # frames 0, 4, 5 and 7 are blank: between the characters, nobody's
    covered = sum(b - a for _, a, b, _ in al.chars)
    assert covered == 5700 - 4 * 480


def test_to_srt():
    spans = [(i, i) for i in range(11)]
    al = _alignment("ab cd ef gh", spans, [0.5] * 11, samples=48000, frame_len=2400)
    srt = al.to_srt(max_chars=5)
    assert srt == ("1\n00:00:00,000 --> 00:00:00,500\nab cd\n\n"
                   "2\n00:00:00,600 --> 00:00:01,100\nef gh\n\n")
    assert al.to_srt(max_chars=1).count("-->") == 4 and al.to_srt().count("-->") == 1


def test_merge_alignments():
    a = _alignment("hi", [(0, 0), (2, 3)], [0.9, 0.8], samples=2000)
    b = _alignment("7 yo", [(1, 1), (2, 2)], [0.7, 0.6], samples=1500)
    m = longform.merge_alignments([a, b], [2000, 1500])
    assert m.text == "hi 7 yo" and m.samples == 3500 and m.score == a.score + b.score
    assert m.chars == a.chars + [(c, s + 2000, e + 2000, p) for c, s, e, p in b.chars]
    assert [w[:3] for w in m.words] == [("hi", 0, 1920), ("7", 2000, 2000), ("yo", 2480, 3440)]
    assert m.char_start(0) == 0 and m.char_start(2) == 1920 and m.char_start(3) == 1920 and m.char_start(5) == 2480 and m.char_end(6) == 3440
    assert len(m.index) == len(m.kept) == len(m.text)


def test_redact_forced_cuts_at_character_boundaries():
    text = "[so sad] hello [aside] there"
    bare, keep = align.redaction_plan(text)
    t = align.alignment_targets(bare, TOK)
    spans = [(2 * i, 2 * i) for i in range(len(t.ids))]
    al = align.build_alignment(t, spans, [0.5] * len(t.ids), 0.0, 2 * len(t.ids) * 10, 10)
    audio = torch.arange(al.samples, dtype=torch.float32)[None]
    got = align.redact_forced(audio, text, lambda a, b: al)
    want = torch.cat([audio[:, al.char_start(a):al.char_end(b)] for a, b in keep], dim=-1)
    assert torch.equal(got, want) and 0 < got.shape[-1] < audio.shape[-1]
    # " hello " starts with the delimiter after "sad" and ends with the one before "aside"; " there" runs to the end of its last character
    assert got[0, 0] == al.chars[6][1] and got[0, -1] == al.chars[-1][2] - 1
    assert align.redact_forced(audio, "no brackets", None) is audio


# ----------------------------------------------------------------------------------------- API flow
from tests.test_redaction_cpu import FakeAlignerStage, _TextTokenizer  # noqa: E402


class LogitsAlignerStage(FakeAlignerStage):
    """The CPU aligner stand-in of the redaction tests, with the logits and the fields the forced alignment asks for."""

    def __init__(self, source, device="cpu", dtype=E.TT_F16, max_samples=0):
        super().__init__(source, device, dtype, max_samples)
        self.fields, self.max_samples, self.device = align.check_config(source[0]), max_samples, torch.device("cpu")

    def run(self, audio, logits=False):
        lg = R.model_logits(self.model, audio.reshape(1, -1).float().cpu()).float()
        return (lg.argmax(-1).int(), lg) if logits else lg.argmax(-1).int()


class ReferenceCtcStage:
    """stages.CtcAlignStage backed by tests/ctc_reference.py."""
    calls = []

    def __init__(self, blank):
        self.blank = blank

    @classmethod
    def for_aligner(cls, aligner, max_clips=16):
        return cls(align.blank_id(aligner.tokenizer))

    def align_many(self, logits_list, targets_list):
        ReferenceCtcStage.calls.append(len(logits_list))
        out = []
        for lg, tg in zip(logits_list, targets_list):
            r = CR.viterbi(lg.double().numpy(), tg, self.blank)
            if r["status"] == CR.OK:
                r = dict(status=0, path=torch.from_numpy(r["path"]), spans=torch.from_numpy(r["spans"]), conf=torch.from_numpy(r["conf"]),
                         score=r["score"])
            out.append(r)
        return out

    def close(self):
        pass


def _flow(monkeypatch, fast=False, **kw):
    from tests.test_api_flow_cpu import VOCAB, small_setup
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "AlignerStage", LogitsAlignerStage)
    monkeypatch.setattr(api.stages, "CtcAlignStage", ReferenceCtcStage)
    ReferenceCtcStage.calls = []
    sds, cfgs = small_setup()
    cfg = R.small_config()
    m = R.hf_model(cfg, seed=3)
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, aligner=(cfg, m.state_dict(), R.VOCAB, R.TOK_CFG), **kw)
    t._tokenizer = _TextTokenizer()
    return t, m


def _same(a, b):
    return repr(a) == repr(b)  # (== on the dataclasses, except that a word without characters carries NaN)


def _expected(m, clip, text):
    lg = R.model_logits(m, clip.reshape(1, -1).float().cpu()).double().numpy()
    t = align.alignment_targets(text, TOK)
    r = CR.viterbi(lg, t.ids, 0)
    return align.build_alignment(t, r["spans"].tolist(), r["conf"].tolist(), r["score"], clip.shape[-1], 480)


@torch.no_grad()
def test_align_and_align_many_through_the_api(monkeypatch):
    t, m = _flow(monkeypatch)
    clips = [R.test_clip(s, seed=i) for i, s in enumerate((0.5, 0.8, 0.3))]
    texts = ["hello there", "it's 9 o'clock, ok", "42"]
    one = [t.align(c, x) for c, x in zip(clips, texts)]
    assert ReferenceCtcStage.calls == [1, 1, 1]
    many = t.align_many(clips, texts)
    assert ReferenceCtcStage.calls[-1] == 3  # ONE forced-alignment call for the batch
    assert _same(many, one)
    for al, c, x in zip(one[:2], clips, texts):
        assert _same(al, _expected(m, c, x))
        assert [w[0] for w in al.words] == x.split() and al.samples == c.shape[-1]
        ends = [e for _, _, e, _ in al.chars]
        assert all(a <= b for a, b in zip(ends, ends[1:])) and all(s < e for _, s, e, _ in al.chars)
    assert one[2].chars == [] and math.isnan(one[2].words[0][3])  # nothing alignable: no characters, one empty word
    with pytest.raises(ValueError, match="too few"):
        t.align(R.test_clip(0.05), "a text far too long for a twentieth of a second")
    with pytest.raises(ValueError, match="2 clips with 1 texts"):
        t.align_many(clips[:2], texts[:1])


@torch.no_grad()
def test_tts_with_timings_and_forced_redaction(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    t, m = _flow(monkeypatch)
    lat = voice_latents(small_setup()[1])
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, use_deterministic_seed=7,
              verbose=False)
    plain = t.tts("hello there", **kw)
    res, al = t.tts_with_timings("hello there", **kw)
    assert torch.equal(res, plain) and al == _expected(m, plain, "hello there")
    res2, als = t.tts_with_timings("hello there", k=2, **kw)
    assert isinstance(als, list) and len(als) == 2 and [a == _expected(m, c, "hello there") for a, c in zip(als, res2)] == [True, True]
    assert ReferenceCtcStage.calls[-1] == 2
    (res3, state), al3 = t.tts_with_timings("hello there", return_deterministic_state=True, **kw)
    assert torch.equal(res3, plain) and al3 == al and state[0] == 7
    with pytest.raises(TypeError):
        t.tts_with_timings([1, 2, 3], **kw)
    # bracketed text, default redaction: today's heuristic and bits; the returned (redacted) clip is aligned with the kept text
    text = "[i am so sad,] hello there"
    assert t.redaction == "reference"
    t.enable_redaction = False
    spoken = t.tts(text, **kw)
    t.enable_redaction = True
    want_ref = R.redact(spoken[0], text, lambda a: R.model_logits(m, a), TOK)[None]
    red, al_red = t.tts_with_timings(text, **kw)
    assert torch.equal(red, want_ref) and al_red.text == " hello there" and al_red == _expected(m, red, " hello there")
    # redaction="forced" on the same instance: the kept characters' spans of the forced alignment of the bare text
    t.redaction = "forced"
    forced = t.tts(text, **kw)
    bare, keep = align.redaction_plan(text)
    ex = _expected(m, spoken, bare)
    want = torch.cat([spoken[0][:, ex.char_start(a):ex.char_end(b)] for a, b in keep], dim=-1)[None]
    assert torch.equal(forced, want) and 0 < forced.shape[-1] < spoken.shape[-1] and "redact_s" in t.timings
    # where the heuristic gives up, the forced alignment does not
    t.redaction = "reference"
    t.aligner.frame_ids = lambda a: [3]  # (the aligner heard "<unk>")
    with pytest.raises(RuntimeError, match="could not align"):
        t.tts("[aa] kb", **kw)
    t.redaction = "forced"
    assert 0 < t.tts("[aa] kb", **kw).shape[-1] and torch.equal(t.tts(text, **kw), forced)
    # ... but a clip with too few frames for its text is still an error
    t.aligner.run = lambda a, logits=False: (None, torch.zeros(3, len(R.VOCAB)))
    with pytest.raises(ValueError, match="too few"):
        t.tts(text, **kw)
    with pytest.raises(ValueError, match="redaction="):
        _flow(monkeypatch, redaction="greedy")


@torch.no_grad()
def test_read_long_form_returns_timings(monkeypatch):
    from tests.test_api_flow_cpu import voice_latents, small_setup
    t, m = _flow(monkeypatch, candidate_sharding=False)
    lat = voice_latents(small_setup()[1])
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=8, diffusion_iterations=3, max_mel_tokens=32, seed=5, texts_are_chunks=True,
              preset="ultra_fast")
    full, clips = longform.read_long_form(t, ["hello there", "and on"], **kw)
    full2, al = longform.read_long_form(t, ["hello there", "and on"], return_timings=True, **kw)
    assert torch.equal(full, full2) and ReferenceCtcStage.calls == [2]
    parts = [_expected(m, c, x) for c, x in zip(clips, ["hello there", "and on"])]
    assert al == longform.merge_alignments(parts, [c.shape[-1] for c in clips])
    assert al.samples == full.shape[-1] and [w[0] for w in al.words] == ["hello", "there", "and", "on"]
    assert al.words[2][1] >= clips[0].shape[-1]


def test_missing_aligner_files_refuse_timings_like_brackets(monkeypatch):
    from tests.test_api_flow_cpu import VOCAB, small_setup
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setenv("HF_HUB_CACHE", "/nonexistent/hub")
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40)
    msgs = []
    for call in (lambda: t.align(torch.zeros(24000), "hello"), lambda: t.tts_with_timings("hello", num_autoregressive_samples=4),
                 lambda: t.tts("[so sad] hello", num_autoregressive_samples=4)):
        with pytest.raises(NotImplementedError, match="bracket") as ei:
            call()
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] == msgs[2] and align.ALIGNER_MODEL in msgs[0]


def test_stage_refuses_what_the_handle_cannot_hold():
    from tortoise_tts_amd import stages
    st = object.__new__(stages.CtcAlignStage)  # (no handle: the checks come before any device work)
    st.h = None
    st.vocab, st.blank, st.max_frames, st.max_tokens, st.max_clips = 32, 0, 1499, E.CTC_MAX_TOKENS, 16
    with pytest.raises(ValueError, match="512 tokens"):
        st.align_many([torch.zeros(1499, 32)], [[1] * 512])
    with pytest.raises(ValueError, match="1500 frames"):
        st.align_many([torch.zeros(1500, 32)], [[1] * 5])
    with pytest.raises(ValueError, match="expected"):
        st.align_many([torch.zeros(10, 31)], [[1]])
    assert align.frames_for(24000 * 30) == 1499


# ----------------------------------------------------------------------------------------- ABI
def test_ctc_header_is_exported_and_mirrored():
    import os
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    lib = E.load_library()
    names = declared_symbols("tortoise_mi355x_ctc.h")
    assert set(names) == set(E._CTC_PROTOS) == {"tt_ctc_abi_version", "tt_ctc_create", "tt_ctc_destroy", "tt_ctc_align"}
    assert all(hasattr(lib, n) for n in names)
    assert lib.tt_ctc_abi_version() == 1 == E.CTC_ABI_VERSION
    assert lib.tt_align_abi_version() == 1  # the aligner's own header is untouched
    main = declared_symbols()
    assert len(main) == len(E._PROTOS) <= 60 and set(main) == set(E._PROTOS) and not [n for n in main if n.startswith("tt_ctc")]
    h = E.vp()
    for bad in ((0, 10, 1, 32, 0), (10, 512, 1, 32, 0), (10, 10, 0, 32, 0), (10, 10, 1, 1, 0), (10, 10, 1, 32, 32), (10, 10, 1, 4096, 0)):
        assert lib.tt_ctc_create(*bad, C.byref(h)) == -1 and b"tt_ctc_create" in lib.tt_last_error()
    rc = lib.tt_ctc_create(100, 50, 2, 32, 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.tt_ctc_destroy(h)
    else:  # no silent fallback: the create fails through tt_last_error
        assert rc != 0 and (b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower())
        with pytest.raises(E.EngineError):
            E.check(rc)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tortoise_mi355x_ctc.h")).read()
    import re
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_CTC_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert defines["TT_CTC_MAX_TOKENS"] == E.CTC_MAX_TOKENS
    assert [defines[k] for k in ("TT_CTC_OK", "TT_CTC_INFEASIBLE", "TT_CTC_EMPTY", "TT_CTC_REFUSED")] == [E.CTC_OK, E.CTC_INFEASIBLE, E.CTC_EMPTY, E.CTC_REFUSED]
