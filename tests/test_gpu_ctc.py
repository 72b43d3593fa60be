"""CTC forced alignment on the MI355X (csrc/ctc_align.hip, include/tortoise_mi355x_ctc.h) against the fp64 reference of tests/ctc_reference.py:
paths, spans and statuses exactly, scores and confidences inside the bounds derived there, ragged batches bit-identical to solo calls, and the
API end to end on the small random-weight aligner."""
import numpy as np
import pytest
import torch

from tests import ctc_reference as CR
from tests import w2v_reference as R
from tortoise_tts_amd import align
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7          # what every output holds before the call
C_BT = 64          # kCtcChunk: frames per backtrace chunk
K_MAX_L = {4: 127, 8: 255, 16: 511}  # longest target of each lane-chunk form (64 K - 1 states)

_stages = {}


def _stage(vocab, blank):
    if (vocab, blank) not in _stages:
        _stages[vocab, blank] = stages.CtcAlignStage(vocab, blank, max_frames=1499, max_tokens=E.CTC_MAX_TOKENS, max_clips=16, device=DEV)
    return _stages[vocab, blank]


def device_align(clips, vocab=32, blank=0):
    """One tt_ctc_align call over clips = [(logits f32 [T, vocab], targets)] with every output pre-filled with SENT -> per clip the raw
    status, path, spans, conf, score (SENT where the call wrote nothing)."""
    st = _stage(vocab, blank)
    n = len(clips)
    fo = np.concatenate(([0], np.cumsum([len(x) for x, _ in clips]))).astype(np.int32)
    to = np.concatenate(([0], np.cumsum([len(t) for _, t in clips]))).astype(np.int32)
    F_, L_ = int(fo[-1]), int(to[-1])
    lg = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1, vocab) for x, _ in clips] + [np.zeros((1, vocab), np.float32)])).to(DEV)
    tg = torch.tensor([t for _, tt_ in clips for t in tt_] + [0], dtype=torch.int32, device=DEV)
    fo_d, to_d = torch.from_numpy(fo).to(DEV), torch.from_numpy(to).to(DEV)
    path = torch.full((F_ + 1,), SENT, dtype=torch.int32, device=DEV)
    spans = torch.full((2 * L_ + 1,), SENT, dtype=torch.int32, device=DEV)
    conf = torch.full((L_ + 1,), float(SENT), device=DEV)
    score = torch.full((n,), float(SENT), device=DEV)
    status = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    E.check(st.lib.tt_ctc_align(st.h, n, E.ptr(lg), E.ptr(fo_d), E.ptr(tg), E.ptr(to_d), E.ptr(path), E.ptr(spans), E.ptr(conf), E.ptr(score),
                                E.ptr(status), E.stream_ptr()))
    path, spans, conf, score, status = (t.cpu().numpy() for t in (path, spans, conf, score, status))
    assert path[F_] == SENT and spans[2 * L_] == SENT and conf[L_] == SENT  # nothing beyond the batch
    return [dict(status=int(status[i]), path=path[fo[i]:fo[i + 1]], spans=spans[2 * to[i]:2 * to[i + 1]].reshape(-1, 2), conf=conf[to[i]:to[i + 1]],
                 score=score[i]) for i in range(n)]


def untouched(r):
    return (r["path"] == SENT).all() and (r["spans"] == SENT).all() and (r["conf"] == SENT).all() and r["score"] == SENT


def check(r, x, tg, blank=0, exact=True, worst=None):
    """One clip's device result against the fp64 reference: status, and for a feasible clip path / spans exactly, score and conf inside
    their bounds.  exact=False: the path need only be valid and within 2 score_bound of the optimum (near-tie inputs)."""
    ref = CR.viterbi(x, tg, blank)
    assert r["status"] == ref["status"], (r["status"], ref["status"])
    if ref["status"] != CR.OK:
        assert untouched(r)
        return ref
    T = len(x)
    assert CR.is_valid_path(r["path"], tg, blank)
    own64 = CR.path_score(ref["lp"], r["path"], tg, blank)
    every = CR.score_bound(T, ref["lp"], x)
    assert own64 >= ref["score"] - 2 * every
    if exact:
        assert r["path"].tolist() == ref["path"].tolist()
        assert r["spans"].tolist() == ref["spans"].tolist()
    spans, conf64 = CR.spans_conf(r["path"], ref["lp"], tg)
    assert r["spans"].tolist() == spans.tolist()
    sb = CR.score_bound(T, ref["lp"], x, CR.labels(tg, blank)[r["path"]])
    cb = CR.conf_bound(ref["lp"], x, tg, spans)
    es, ec = abs(float(r["score"]) - own64) / sb, float((np.abs(r["conf"] - conf64) / cb).max())
    if worst is not None:
        worst["score"], worst["conf"] = max(worst["score"], es), max(worst["conf"], ec)
    assert es <= 1 and ec <= 1, (es, ec)
    return ref


def rand_clip(seed, T, L, vocab=32, blank=0, targets=None):
    rng = np.random.default_rng(seed)
    tg = CR.random_targets(rng, L, vocab, blank) if targets is None else targets
    return (2.0 * rng.standard_normal((T, vocab))).astype(np.float32), tg


# ----------------------------------------------------------------------------------------- shapes
BOUNDARY = {
    "L1_T1": (1, [7]), "L1_T2": (2, [7]), "L1_T3": (3, [7]),
    "single_path": (9, [5, 5, 7, 8, 8, 8]),          # T == L + repeats: one feasible path
    "infeasible": (8, [5, 5, 7, 8, 8, 8]),           # one frame less
    "empty_target": (5, []),
    "no_frames": (0, [3, 4]),
    "same_token_9_min": (17, [4] * 9), "same_token_9": (30, [4] * 9),   # no skip is ever allowed
    "alternating": (20, [3, 9] * 6), "alternating_min": (12, [3, 9] * 6),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_boundary_shapes(name):
    T, tg = BOUNDARY[name]
    x, _ = rand_clip(len(name), T, 0, targets=tg)
    ref = check(device_align([(x, tg)])[0], x, tg)
    want = {"infeasible": CR.INFEASIBLE, "empty_target": CR.EMPTY, "no_frames": CR.EMPTY}.get(name, CR.OK)
    assert ref["status"] == want


@pytest.mark.parametrize("K", [4, 8, 16])
def test_lane_chunk_edges(K):
    """2L + 1 at the largest the K form holds (64 K - 1), the odd size below it, and the smallest target that selects the form; T = L + 40."""
    Lmax = K_MAX_L[K]
    smallest = 1 if K == 4 else K_MAX_L[K // 2] + 1
    for L in (smallest, Lmax - 1, Lmax):
        x, tg = rand_clip(100 * K + L, L + 40, L)
        check(device_align([(x, tg)])[0], x, tg)


@pytest.mark.parametrize("vocab,blank,chunk", [(32, 0, C_BT), (37, 17, 55)])
def test_chunk_edges(vocab, blank, chunk):
    """T around the backtrace's LDS chunk (64 frames) and around the emission chunk of a vocabulary of 37 (55 frames)."""
    for T in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        x, tg = rand_clip(T, T, 20, vocab, blank)
        check(device_align([(x, tg)], vocab, blank)[0], x, tg, blank)


@pytest.mark.parametrize("vocab,blank", [(32, 0), (32, 31), (37, 0), (37, 17)])
def test_vocabulary_and_blank(vocab, blank):
    clips = [rand_clip(7 * vocab + blank + i, T, L, vocab, blank) for i, (T, L) in enumerate(((90, 25), (200, 140)))]
    for r, (x, tg) in zip(device_align(clips, vocab, blank), clips):
        check(r, x, tg, blank)


def test_ties_follow_the_tie_break():
    """All-zero logits: stay beats s - 1 beats s - 2, exactly - also across a lane boundary and with repeats."""
    cases = [(23, [1, 2, 3, 4, 5]), (260, [1 + i % 30 for i in range(200)]), (40, [2, 2, 2, 5, 5, 1]), (700, [1 + (i // 2) % 30 for i in range(300)])]
    clips = [(np.zeros((T, 32), np.float32), tg) for T, tg in cases]
    for r, (x, tg) in zip(device_align(clips), clips):
        assert r["status"] == 0 and r["path"].tolist() == CR.tie_break_path(len(x), tg)
        check(r, x, tg)


# ----------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("family", ["random", "planted"])
def test_accuracy_on_the_seeded_families(family):
    """40 clips of the CPU test's family: a valid path, equal to the fp64 path, score and conf inside their bounds."""
    fam = CR.random_clip if family == "random" else CR.planted_clip
    clips = [fam(seed) for seed in range(40)]
    worst = dict(score=0.0, conf=0.0)
    for g in range(0, 40, 16):
        for r, (x, tg) in zip(device_align(clips[g:g + 16]), clips[g:g + 16]):
            check(r, x, tg, worst=worst)
    print(f"[ctc] {family}: worst |score error| / bound {worst['score']:.3f}, worst |conf error| / bound {worst['conf']:.3f}")


def test_near_ties_stay_within_twice_the_bound():
    """Two tokens whose logits differ by one f32 ulp in every frame: which of two paths wins may differ from fp64, never by more than
    2 score_bound in fp64 score."""
    worst = dict(score=0.0, conf=0.0)
    clips = []
    for seed in range(8):
        rng = np.random.default_rng(seed)
        T = 60 + 20 * seed
        x = (2.0 * rng.standard_normal((T, 32))).astype(np.float32)
        x[:, 2] = np.nextafter(x[:, 1], np.float32(np.inf))
        x[:, 0] = x[:, 1]  # and the blank ties with them
        clips.append((x, [1, 2] * (4 + seed)))
    for r, (x, tg) in zip(device_align(clips), clips):
        check(r, x, tg, exact=False, worst=worst)
    print(f"[ctc] near ties: worst |score error| / bound {worst['score']:.3f}, worst |conf error| / bound {worst['conf']:.3f}")


# ----------------------------------------------------------------------------------------- ragged batches
def _bits(r):
    return (r["status"], r["path"].tobytes(), r["spans"].tobytes(), r["conf"].tobytes(), r["score"].tobytes())


def test_ragged_batch_is_bit_identical_to_solo_calls():
    shapes = [(1, 1), (77, 30), (300, 100), (1499, 400), (64, 12)]
    clips = [rand_clip(50 + i, T, L) for i, (T, L) in enumerate(shapes)]
    solo = [device_align([c])[0] for c in clips]
    for r, (x, tg) in zip(solo, clips):
        check(r, x, tg)
    batch = device_align(clips)
    assert [_bits(r) for r in batch] == [_bits(r) for r in solo]
    # an infeasible clip in the middle: its status and nothing else, and its neighbours as before
    bad = rand_clip(99, 20, 0, targets=[6] * 11)
    batch = device_align(clips[:2] + [bad] + clips[2:])
    assert batch[2]["status"] == CR.INFEASIBLE and untouched(batch[2])
    assert [_bits(r) for r in batch[:2] + batch[3:]] == [_bits(r) for r in solo]


def test_stage_align_many_and_host_checks():
    st = _stage(32, 0)
    clips = [rand_clip(200 + i, T, L) for i, (T, L) in enumerate(((40, 10), (5, 9), (33, 0), (150, 130)))]
    res = st.align_many([torch.from_numpy(x) for x, _ in clips], [tg for _, tg in clips])
    assert [r["status"] for r in res] == [E.CTC_OK, E.CTC_INFEASIBLE, E.CTC_EMPTY, E.CTC_OK]
    for r, (x, tg) in zip(res, clips):
        if r["status"] == E.CTC_OK:
            ref = CR.viterbi(x, tg, 0)
            assert r["path"].tolist() == ref["path"].tolist() and r["spans"].tolist() == ref["spans"].tolist()
            assert abs(r["score"] - ref["score"]) <= CR.score_bound(len(x), ref["lp"], x)
    many = st.align_many([torch.from_numpy(clips[0][0])] * 20, [clips[0][1]] * 20)  # more clips than one call holds
    assert len(many) == 20 and all(torch.equal(m["path"], res[0]["path"]) and m["score"] == res[0]["score"] for m in many)
    with pytest.raises(ValueError, match="512 tokens"):
        st.align_many([torch.zeros(1499, 32)], [[1] * 512])
    with pytest.raises(ValueError, match="1500 frames"):
        st.align_many([torch.zeros(1500, 32)], [[1] * 5])
    # what the host cannot see (ids on the device) the kernel refuses: a blank or out-of-range id in a target
    x, _ = rand_clip(1, 30, 0)
    for tg in ([3, 0, 4], [3, 32, 4], [3, -1, 4]):
        r = device_align([(x, tg)])[0]
        assert r["status"] == E.CTC_REFUSED and untouched(r)


# ----------------------------------------------------------------------------------------- end to end
class _IdsTokenizer:
    def __init__(self, ids):
        self.ids = ids

    def encode(self, text):
        return self.ids


@pytest.fixture(scope="module")
def tts():
    import bench
    from tortoise_tts_amd.api import TextToSpeech
    cfg = R.small_config()
    model = R.hf_model(cfg, seed=5)
    src = (cfg, {k: v.detach().cpu() for k, v in model.state_dict().items()}, R.VOCAB, R.TOK_CFG)
    t = TextToSpeech(state_dicts=bench.synthetic_weights(), max_candidates=16, max_mel_tokens=48, aligner=src)
    t._tokenizer = _IdsTokenizer(bench.synthetic_prompt()[0].tolist())
    return t


def _reference_alignment(t, clip, text):
    """The fp64 reference applied to the stage's own logits of the clip."""
    al = t.load_aligner()
    lg = al.run(clip.reshape(1, -1), logits=True)[1].cpu().numpy()
    tg = align.alignment_targets(text, al.tokenizer)
    ref = CR.viterbi(lg, tg.ids, align.blank_id(al.tokenizer))
    return align.build_alignment(tg, ref["spans"].tolist(), ref["conf"].tolist(), ref["score"], clip.shape[-1], 480), ref, lg, tg


def _close(got, want, ref, lg, tg):
    """Same characters, words and samples; confidences and score inside the bounds."""
    assert [c[:3] for c in got.chars] == [c[:3] for c in want.chars] and [w[:3] for w in got.words] == [w[:3] for w in want.words]
    assert got.text == want.text and got.samples == want.samples and got.index == want.index
    cb = CR.conf_bound(ref["lp"], lg, tg.ids, ref["spans"])
    assert all(abs(g[3] - w[3]) <= b for g, w, b in zip(got.chars, want.chars, cb))
    assert abs(got.score - want.score) <= CR.score_bound(len(lg), ref["lp"], lg)


@torch.no_grad()
def test_align_through_the_api(tts):
    assert align.frame_samples(tts.load_aligner().fields) == 480
    clips = [R.test_clip(s, seed=i + 1) for i, s in enumerate((2.0, 1.1, 3.3))]
    texts = ["hello there", "it's 9 o'clock, ok", "well well, who is there?"]
    one = [tts.align(c, x) for c, x in zip(clips, texts)]
    for al, c, x in zip(one, clips, texts):
        _close(al, *_reference_alignment(tts, c, x))
        assert [w[0] for w in al.words] == x.split()
    many = tts.align_many([c.to(DEV) for c in clips], texts)
    assert repr(many) == repr(one)  # bit-identical in a ragged batch
    assert tts.ctc.max_frames == align.frames_for(tts.aligner.max_samples) and tts.ctc.vocab == len(R.VOCAB)
    with pytest.raises(ValueError, match="too few"):
        tts.align(R.test_clip(0.1), "a text far too long for a tenth of a second")


@torch.no_grad()
def test_forced_redaction_and_timings_on_the_device(tts):
    text = "[I am so sad,] hello there"
    g = torch.Generator().manual_seed(6)
    lat = (torch.randn(1, 1024, generator=g) * 0.5, torch.randn(1, 2048, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=16, diffusion_iterations=4, max_mel_tokens=48, use_deterministic_seed=5,
              verbose=False)
    tts.enable_redaction = False
    plain = tts.tts(text, **kw)
    tts.enable_redaction = True
    assert tts.redaction == "reference"
    ref_cut = tts.tts(text, **kw)
    want = R.redact(plain[0], text, lambda a: tts.aligner.run(a).cpu().long(), tts.aligner.tokenizer)[None]
    assert torch.equal(ref_cut, want)  # today's bits
    tts.redaction = "forced"
    try:
        forced = tts.tts(text, **kw)
    finally:
        tts.redaction = "reference"
    bare, keep = align.redaction_plan(text)
    ex = _reference_alignment(tts, plain, bare)[0]
    want = torch.cat([plain[0][:, ex.char_start(a):ex.char_end(b)] for a, b in keep], dim=-1)[None]
    assert torch.equal(forced, want) and 0 < forced.shape[-1] < plain.shape[-1] and "redact_s" in tts.timings
    # tts_with_timings: the clip tts() returns for the seed, and the alignment of its text with it
    res, al = tts.tts_with_timings("hello there", **kw)
    tts.enable_redaction = False
    assert torch.equal(res, plain)  # (the ids stand-in speaks the same tokens for every text)
    tts.enable_redaction = True
    _close(al, *_reference_alignment(tts, res, "hello there"))
    assert [w[0] for w in al.words] == ["hello", "there"] and al.samples == res.shape[-1]
