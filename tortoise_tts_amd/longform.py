"""Long-form reading (BASELINE.json config #4; reference driver: tortoise/read.py:44-99).

The reference splits the text into chunks (`split_and_recombine_text`, utils/text.py), renders them ONE AFTER THE OTHER with
the same seed (read.py:66-71) and concatenates the clips (read.py:87).  Chunks are independent utterances, so on a multi-GPU
node they are spread over the ranks as replicas: chunk j -> rank j % R, every rank runs the complete pipeline
for its chunks on its own GPU (no candidate sharding, no collective on the data path), rank 0 receives the clips point to
point and concatenates them in chunk order.  The audio of a chunk does not depend on R: same seed, same GPU-local pipeline.
With TextToSpeech(utterance_batch=G) a rank renders its chunks G at a time (tts_many): the candidates of G chunks share one decode
batch - per-chunk codes bit-identical to the sequential order - which is what 288 GB of HBM per GPU are for.
"""
import torch

from . import dist as tdist
from .text import split_and_recombine_text


def chunk_owner(j, world):
    return j % world


def merge_alignments(alignments, clip_samples):
    """The alignments of consecutive chunks as one alignment of the concatenated audio: chunk j's samples are offset by the samples of the
    chunks before it, the texts are joined with a space."""
    from .align import Alignment
    chars, words, index, kept, text, off, score = [], [], [], [], "", 0, 0.0
    for j, (al, n) in enumerate(zip(alignments, clip_samples)):
        if j:
            text += " "
            index.append(len(chars) - 1)
            kept.append(False)
        index += [i + len(chars) for i in al.index]  # (-1, nothing before it in its chunk: the last character of the chunks before)
        kept += al.kept
        chars += [(c, a + off, b + off, p) for c, a, b, p in al.chars]
        words += [(w, a + off, b + off, p) for w, a, b, p in al.words]
        text += al.text
        score += al.score
        off += int(n)
    return Alignment(text, chars, words, score, off, index, kept, getattr(alignments[0], "rate", Alignment.rate) if alignments else Alignment.rate)


def read_long_form(tts, text, preset="standard", conditioning_latents=None, voice_samples=None, seed=None, texts_are_chunks=False,
                   return_timings=False, pause=None, **tts_kwargs):
    """tts: a TextToSpeech built with candidate_sharding=False (one complete engine per rank), or a fast-path
    tortoise_tts_amd.api_fast.TextToSpeech (the reference's read_fast.py): each rank then renders its chunks with one tts_many call -
    tts()'s defaults plus tts_kwargs, the agreed seed for every chunk - and `preset` does not apply (read_fast.py passes none; the fast
    path has no diffusion settings).
    text: the whole text (str; '|' splits it like read.py:46-50, else split_and_recombine_text) or, with texts_are_chunks=True,
    a list of chunks (str or pre-tokenised id sequences).
    Returns (full_audio f32 [1, n] or None, parts: list of per-chunk clips [1, 1, n_j]) on rank 0, (None, None) elsewhere.
    return_timings=True (str chunks): (full_audio, align.Alignment of the whole text in the concatenated audio) instead - every chunk is
    aligned with its own clip in one forced-alignment call (tts.align_many) and merge_alignments offsets them.
    loudness= (LUFS; with true_peak= and limit=, see TextToSpeech.normalize_many) brings the reading to a level: loudness_scope='chunk' (the
    default) every chunk to the target, in one normalize_many call per rank - the level no longer moves from chunk to chunk;
    loudness_scope='whole' one gain for the concatenation.
    pitch= goes to the chunks' calls with speaking_rate=, and so do formants= ('keep') / formant_shift= with their options: every chunk's
    spectral envelope is corrected after its pitch shift and before its pauses, with the same warp for all chunks.  sample_rate= (Hz, 8000 .. 96000) is applied here, last: every chunk is converted
    from 24 kHz in one call, after the level and after the alignment, whose positions then count samples of the returned audio (the
    Alignment carries that rate).
    trim_silence= / max_pause= go to the chunks' calls.  pause= (seconds; None: off) sets the silence between two chunks: every chunk is cut
    to its speech at both ends (lead = trail = 0; its own trim_silence= / max_pause= still shape the inside) and `pause` seconds of zeros
    are appended to every part but the last, after the per-chunk level and before the alignment, so the gap between the last speech
    region of one chunk and the first of the next is exactly round(pause * 24000) samples and the full audio is still the parts joined."""
    from . import loudness as loud
    from . import pitch as f0m
    from . import resample as rs
    from . import silence as sil
    from .api_fast import TextToSpeech as FastTextToSpeech
    fast = isinstance(tts, FastTextToSpeech)
    rs.refuse_word_pitches(tts_kwargs, "read_long_form")
    f0m.refuse_long_form(tts_kwargs)
    scope, level = loud.scope_option(tts_kwargs), loud.level_options(tts_kwargs)  # (applied here, to what the chunks' calls return)
    sample_rate = rs.options(dict(sample_rate=tts_kwargs.pop("sample_rate", None)))[1]  # (here too, after the level)
    gap = None if pause is None else sil.for_long_form(tts_kwargs, pause)  # (the chunks' calls get lead = trail = 0)
    if getattr(tts, "world", 1) != 1:
        raise ValueError("read_long_form spreads chunks over the ranks: build TextToSpeech(candidate_sharding=False)")
    if texts_are_chunks:
        texts = list(text)
    elif "|" in text:
        texts = text.split("|")
    else:
        texts = split_and_recombine_text(text)
    rank, world = tdist.world()
    if seed is None:  # read.py:54 uses the wall clock; every rank must agree on it
        import time
        seed = int(time.time())
    seed = tdist.broadcast_int(seed)
    mine = {}
    my_chunks = [j for j in range(len(texts)) if chunk_owner(j, world) == rank]
    if fast and my_chunks:
        wavs = tts.tts_many([texts[j] for j in my_chunks], voice_samples=voice_samples, conditioning_latents=conditioning_latents,
                            use_deterministic_seed=seed, **tts_kwargs)
        mine = {j: w.cpu() for j, w in zip(my_chunks, wavs)}
        my_chunks = []
    elif getattr(tts, "utterance_batch", 1) > 1 and len(my_chunks) > 1:
        # this rank's chunks share decode batches (TextToSpeech.tts_many): same seed, same per-chunk codes as one after the other
        from .config import BASE_SETTINGS, PRESETS
        settings = dict(BASE_SETTINGS)
        settings.update(PRESETS[preset])
        settings.update(tts_kwargs)
        settings.pop("k", None)
        wavs = tts.tts_many([texts[j] for j in my_chunks], voice_samples=voice_samples, conditioning_latents=conditioning_latents,
                            use_deterministic_seed=seed, **settings)
        mine = {j: w.cpu() for j, w in zip(my_chunks, wavs)}
        my_chunks = []
    for j in my_chunks:
        gen = tts.tts_with_preset(texts[j], voice_samples=voice_samples, conditioning_latents=conditioning_latents, preset=preset, k=1,
                                  use_deterministic_seed=seed, **tts_kwargs)  # read.py:70-71
        mine[j] = gen.cpu()
    if level is not None and scope == "chunk" and mine:  # every chunk of this rank to the target, in one call
        mine = tts._at_level(mine, level)
    parts = tdist.collect_on_rank0(mine, len(texts))
    if parts is None:
        return None, None
    clips = [parts[j] for j in range(len(texts))]
    if gap:  # the chosen pause after every chunk but the last
        clips = [torch.cat([c, c.new_zeros(c.shape[:-1] + (gap,))], dim=-1) for c in clips[:-1]] + clips[-1:]
    full = torch.cat([c.squeeze(0) for c in clips], dim=-1)  # read.py:74, 87
    if level is not None and scope == "whole":  # one gain (and one limiter pass) for the concatenation; the parts are its pieces
        full = tts._at_level([full], level)[0]
        clips = [p.reshape(c.shape) for p, c in zip(full.split([c.shape[-1] for c in clips], dim=-1), clips)]
    als = tts.align_many(clips, [tts._spoken_text(t) for t in texts]) if return_timings else None  # (the aligner reads 24 kHz)
    if sample_rate is not None:
        from .align import resample_alignment
        clips = tts._at_sample_rate(clips, sample_rate)
        full = torch.cat([c.squeeze(0) for c in clips], dim=-1)
        als = als and [resample_alignment(al, sample_rate, c.shape[-1]) for al, c in zip(als, clips)]
    if return_timings:
        return full, merge_alignments(als, [c.shape[-1] for c in clips])
    return full, clips
