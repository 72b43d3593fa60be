"""Drop-in surface: `TextToSpeech` with the reference's constructor / tts() / tts_with_preset()
signatures (reference: tortoise/api.py:179-181, 311-332, 334-342), re-hosted on the MI355X engine.

What changed behind the signature
  * all four networks stay resident on the GPU (the reference re-uploads ~5.6 GB per call through
    `temporary_cuda`, api.py:245-249);
  * stage 1 decodes all candidates of this rank together, sharing one prefix evaluation, with
    on-device sampling and a hipGraph per token;
  * candidates shard across the GPUs of a node, one all_gather picks the CLVP top-k (dist.py);
  * stage 2 evaluates conditioned + unconditioned denoiser rows in one pass per step;
  * integer post-processing (api.py:87-114, 547-556) is vectorised on device and bit-exact.
Constructor flags of the reference and what they mean here:
  * kv_cache   the engine always keeps a KV cache; the flag selects the reference's mel POSITION rule, which is the
               only numerical difference between its two code paths (kv_cache=False, the reference default: rows
               0,1,2,...; kv_cache=True: rows 0,2,3,...; autoregressive.py:134-149);
  * half       True selects fp16 MFMA operands (the reference's fp16 autocast), False the engine default (bf16) unless
               the engine-only `dtype=` says otherwise;
  * enable_redaction  [bracketed] text is spoken and then cut out of every returned clip by the wav2vec2 CTC aligner, as
               wav2vec_alignment.py does (align.py + stages.AlignerStage, csrc/align.hip; built on first use from the HF-format files
               under models_dir or the HF hub cache, or the engine-only `aligner=`); text without '[' is unaffected.
cvvp_amount > 0 (api.py:450-472; the CHANGELOG calls CVVP "removed", the call sites and cvvp.pth remain): the CVVP model is built on
first use like upstream (load_cvvp -> stages.CvvpStage, csrc/cvvp.hip) and blended into the CLVP ranking when voice_samples are given.
classify_audio_clip(clip) (api.py; is_this_from_tortoise.py) runs the Tortoise detector on the device (stages.ClassifierStage,
csrc/classify.hip), with classifier.pth read and packed once per (models_dir, device).
Out of scope (raise, never silently fall back): DeepSpeed flag.
"""
import inspect
import math
import os
import random
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

from . import align
from . import denoise as nr
from . import dist as tdist
from . import engine as E
from . import stages
from . import formant as fmt
from . import loudness as loud
from . import pitch as f0m
from . import resample as rs
from . import silence as sil
from . import solver as fastsolver
from . import stretch as tsm
from . import weights as W
from .config import ARConfig, CLVPConfig, CVVPConfig, DiffusionConfig, VocoderConfig, PRESETS, BASE_SETTINGS, CALM_TOKEN
from .schedule import Schedule

MODELS_DIR = os.environ.get("TORTOISE_MODELS_DIR", os.path.join(os.path.expanduser("~"), ".cache", "tortoise", "models"))
MODEL_FILES = {"autoregressive": "autoregressive.pth", "clvp": "clvp2.pth", "diffusion": "diffusion_decoder.pth",
               "vocoder": "vocoder.pth", "rlg_auto": "rlg_auto.pth", "rlg_diffuser": "rlg_diffuser.pth", "cvvp": "cvvp.pth"}


class _StageTimer:
    """Stage boundaries of one tts() call as HIP events on the current stream (no host synchronisation until read)."""

    def __init__(self, n):
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    def mark(self, i):
        self.ev[i].record()

    def seconds(self, i, j):
        return self.ev[i].elapsed_time(self.ev[j]) / 1e3

    @staticmethod
    def synchronize():
        torch.cuda.synchronize()


def sampler_kwargs(hf_generate_kwargs):
    """The **hf_generate_kwargs of tts() the on-device sampler honours -> (top_k, typical_mass); anything else raises instead of
    being dropped.  `top_k`: HF GenerationConfig default 50, which the reference inherits (api.py never overrides it).
    `typical_sampling` / `typical_mass` (api.py:361-364): inference_speech turns them into generate()'s logits_processor list
    [TypicalLogitsWarper(mass=typical_mass)] (autoregressive.py:536, 558); typical_mass is ignored unless typical_sampling is set,
    as upstream.  Returns typical_mass = 0.0 for "off"."""
    kw = dict(hf_generate_kwargs)
    top_k = int(kw.pop("top_k", 50))
    typical = bool(kw.pop("typical_sampling", False))
    mass = float(kw.pop("typical_mass", .9))
    if kw:
        raise NotImplementedError(f"unsupported generate kwargs {sorted(kw)}: the on-device sampler implements temperature / top_k / top_p / "
                                  f"repetition_penalty / typical_sampling + typical_mass (length_penalty is a no-op when sampling)")
    if typical and not 0.0 < mass < 1.0:
        raise ValueError(f"typical_mass={mass} must lie in (0, 1) (the reference's warper indexes past the vocabulary at >= 1)")
    return top_k, (mass if typical else 0.0)


def fix_autoregressive_output(codes, stop_token, calm_token=CALM_TOKEN):
    """Vectorised api.py:87-114 for a batch int tensor [B, n] (any device); rows without a stop token are
    returned unchanged exactly like the reference (which only prints a warning)."""
    codes = codes.clone()
    B, n = codes.shape
    is_stop = codes == stop_token
    has_stop = is_stop.any(dim=1)
    pos = torch.arange(n, device=codes.device)[None, :].expand(B, n)
    first = torch.where(is_stop, pos, torch.full_like(pos, n)).min(dim=1).values  # stm
    tail = (pos >= first[:, None]) & has_stop[:, None]
    codes[tail] = calm_token
    rows = has_stop & (first - 3 < n)
    codes[rows, -3] = 45
    codes[rows, -2] = 45
    codes[rows, -1] = 248
    return codes


def calm_trim_length(codes_row, calm_token=CALM_TOKEN):
    """api.py:547-556: index k at which more than 8 consecutive calm tokens have been seen (latents are cut
    to [:k]); len(codes_row) if there is no such run.  Vectorised, one host read."""
    c = (codes_row == calm_token).to(torch.int32)
    n = c.shape[0]
    if n < 9:
        return n
    run9 = F.avg_pool1d(c[None, None].float(), kernel_size=9, stride=1)[0, 0] >= 1.0 - 1e-6  # windows of 9 calm tokens
    idx = torch.nonzero(run9)
    return int(idx[0, 0]) + 8 if idx.numel() else n


def _load_state_dict(models_dir, name):
    path = os.path.join(models_dir, MODEL_FILES[name])
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found. Put the reference checkpoints in models_dir (or $TORTOISE_MODELS_DIR), or pass "
                                f"state_dicts= to TextToSpeech; there is no network access to download them.")
    sd = torch.load(path, map_location="cpu")
    return sd["model_g"] if name == "vocoder" else sd


def _load_file(models_dir, filename):
    path = os.path.join(models_dir, filename)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found. Put the reference checkpoints in models_dir (or $TORTOISE_MODELS_DIR), or pass "
                                f"state_dicts= to TextToSpeech; there is no network access to download them.")
    return torch.load(path, map_location="cpu")


_CLASSIFIERS = {}  # (models_dir, device) -> ClassifierStage: classifier.pth is read and packed once per process


def classify_audio_clip(clip, *, models_dir=MODELS_DIR):
    """api.py classify_audio_clip: the probability (0-dim CPU tensor) that `clip` [1, T] at 24 kHz (any device) was generated by Tortoise,
    from AudioMiniEncoderWithClassifierHead with classifier.pth from models_dir.  The model runs on the current GPU; an fp16 overflow
    rebuilds it with bf16 operands and classifies the clip again."""
    if not isinstance(clip, torch.Tensor) or clip.dim() != 2 or clip.shape[0] != 1:
        raise ValueError(f"classify_audio_clip takes a [1, T] clip at 24 kHz, got {tuple(clip.shape) if isinstance(clip, torch.Tensor) else type(clip).__name__}")
    if clip.shape[1] < 1:
        raise ValueError("classify_audio_clip: the clip is empty")
    device = E.require_gpu()
    key = (os.path.abspath(models_dir), str(device))
    stage = _CLASSIFIERS.get(key)
    if stage is None:
        sd = _load_file(models_dir, "classifier.pth")
        stage = stages.ClassifierStage(sd, device, E.TT_F16, max_samples=max(220000, clip.shape[1]))
        stage.sd = sd
        _CLASSIFIERS[key] = stage
    while True:
        logits, _ = stage.run(clip)
        logits = logits.cpu()
        if not stage.guard():
            break
        if stage.dtype != E.TT_F16:
            raise E.OperandOverflow("the classifier stage produced non-finite values with bf16 operands (non-finite weights or audio?)")
        import warnings
        warnings.warn("tortoise_tts_amd: the classifier stage overflowed fp16 operands; rebuilding it with bf16 operands")
        sd, cap = stage.sd, stage.max_samples
        stage.close()
        stage = stages.ClassifierStage(sd, device, E.TT_BF16, max_samples=cap)
        stage.sd = sd
        _CLASSIFIERS[key] = stage
    return F.softmax(logits, dim=-1)[0]


def utterance_batch_bytes(utterance_batch, max_candidates, max_mel_tokens, ar_cfg, diff_cfg, max_steps=512):
    """Bytes of the two arenas that grow with TextToSpeech(utterance_batch=): the per-sequence KV cache (layers x model_dim x K,V x 2
    bytes per cached token, utterance_batch x max_candidates sequences of max_mel_tokens + 2 slots) and the conditioning-integrator outputs
    of every sampler step (max_steps x 2 guidance rows x utterances x S x channels x 2 bytes)."""
    max_S = max_mel_tokens * 4 * 24000 // 22050 + 8
    kv = utterance_batch * max_candidates * (max_mel_tokens + 2) * ar_cfg.layers * ar_cfg.model_dim * 2 * 2
    integ = max_steps * 2 * utterance_batch * max_S * diff_cfg.model_channels * 2
    return kv + integ


STAGE_NAMES = ("ar", "clvp", "diffusion", "vocoder")


def resolve_stage_dtypes(dtype, half):
    """MFMA operand type per stage -> {'ar' | 'clvp' | 'diffusion' | 'vocoder': engine dtype code}.

    The reference autocasts ONLY the autoregressive + CLVP stages to fp16, and only under half=True (api.py:413-414, 460-463); its
    diffusion decoder and vocoder always run in fp32 (api.py:225 use_fp16=False, 540-560 no autocast).  Default here (round 6): **fp16 for
    every stage** - the MFMA operand type closest to the reference's fp32 (3 more mantissa bits than bf16) at the same speed.  Measured
    against the reference's own fp32 modules at the benchmarked width (profiles/r06_parity_gpu.txt): decode logits over
    500 teacher-forced steps rel-L2 8e-4 (bf16 6.5e-3), total variation of the sampler's warped distribution mean 0.002 / max 0.020
    (bf16 0.009 / 0.038), CLVP Spearman 0.9999 (0.9993), 200-iteration mel 1.1e-3 (8.6e-3).  fp16 saturates at 65504, so every stage
    counts non-finite values behind its operand casts (tt_*_guard): a tripped stage is rebuilt with bf16 operands - the fp32 exponent
    range - and the utterance re-rendered with the same seed (TextToSpeech._demote).  half=True (the reference's fp16 autocast flag) is
    therefore the default behaviour already; dtype='bf16' (or a dict per stage) selects bf16 operands up front.
    `dtype` may be None (defaults), one name for every stage, or a dict overriding some stages."""
    out = {"ar": "fp16", "clvp": "fp16", "diffusion": "fp16", "vocoder": "fp16"}
    if isinstance(dtype, dict):
        unknown = set(dtype) - set(STAGE_NAMES)
        if unknown:
            raise ValueError(f"dtype: unknown stage(s) {sorted(unknown)}; stages are {STAGE_NAMES}")
        out.update(dtype)
    elif dtype is not None:
        out = {k: dtype for k in STAGE_NAMES}
    if half and any(E.dtype_code(out[k]) != E.TT_F16 for k in ("ar", "clvp")):
        raise ValueError(f"half=True asks for fp16 operands in the autoregressive / CLVP stages but dtype={dtype!r} was also given")
    return {k: E.dtype_code(v) for k, v in out.items()}


DENOISER_SECONDS = 12  # the clip the denoiser is first built for (voice clips are a few seconds each)
ORIG_ALIGNER_SECONDS = 30  # the longest clip the aligner of a path without its own clip cap is built for
LOUDNESS_STAGE_SAMPLES = 16 * 30 * E.LOUD_SAMPLE_RATE  # samples of one call the loudness stage is first built for: sixteen clips of 30 s


class StreamResampler:
    """One stream of a stages.StreamResampleStage (_Common.open_resampler): f32 chunks in, f32 tensors on the device out (possibly
    empty).  An output appears once the H + 1 input samples after its position are in (latency_seconds); finish() ends the stream as
    the clip's end and frees the slot.  A context manager: leaving it closes the stream."""

    def __init__(self, stage, P, Q, from_rate=rs.SAMPLE_RATE):
        self.stage, self.P, self.Q = stage, P, Q
        self.slot = stage.open(P, Q)
        self.n_in = self.n_out = 0
        self.latency_seconds = rs.stream_latency(P, Q) / float(from_rate)

    def _push(self, chunk, flush):
        if self.slot is None:
            raise ValueError("this resampling stream is closed")
        chunk = torch.as_tensor(chunk, dtype=torch.float32).reshape(-1)
        y = self.stage.push_many([(self.slot, chunk, flush)])[0]
        self.n_in += chunk.shape[0]
        self.n_out += y.shape[0]
        return y

    def push(self, chunk):
        return self._push(chunk, False)

    def finish(self, chunk=None):
        """The outputs still due (after an optional last chunk); the stream is over and its slot free."""
        y = self._push(torch.zeros(0) if chunk is None else chunk, True)
        self.close()
        return y

    def close(self):
        if self.slot is not None:
            self.stage.close(self.slot)
            self.slot = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class StreamLeveler:
    """One stream brought to a level (_Common.open_leveler): f32 chunks at 24 kHz in, f32 tensors on the device out (possibly empty) - a
    slot of a stages.StreamLevelStage.  Under the look-ahead limiter an output appears once the 248 input samples behind it are in
    (latency_seconds, 10.3 ms); finish() ends the stream and frees the slot.  reading() is the stream's loudness.StreamLevel so far.  A
    context manager: leaving it closes the stream."""

    def __init__(self, stage, settings):
        self.stage, self.settings = stage, settings
        self.closed = False
        self.slot = stage.open(settings)
        self.n_in = self.n_out = 0
        self._last = None
        self.latency_seconds = (E.LVS_DELAY if settings.limit == E.LVS_LOOKAHEAD else 0) / float(E.LOUD_SAMPLE_RATE)

    def _push(self, chunk, flush):
        if self.closed:
            raise ValueError("this leveling stream is closed")
        x = torch.as_tensor(chunk, dtype=torch.float32).reshape(-1)
        y = self.stage.push_many([(self.slot, x, flush)])[0]
        self.n_in += x.shape[0]
        self.n_out += y.shape[0]
        return y

    def push(self, chunk):
        return self._push(chunk, False)

    def finish(self, chunk=None):
        """The outputs still due (after an optional last chunk); the stream is over and its slot free (reading() keeps the last one)."""
        y = self._push(torch.zeros(0) if chunk is None else chunk, True)
        self._last = self.reading()
        self.close()
        return y

    def reading(self):
        """loudness.StreamLevel of the stream so far.  Synchronises."""
        if self.slot is None:
            if self._last is None:
                raise ValueError("this leveling stream is closed")
            return self._last
        return loud.stream_reading(self.stage.read(self.slot))

    def trace(self):
        """The per-hop history (stages.StreamLevelStage.trace): q, lufs, gain_db, status, blocks_abs, blocks_rel.  Synchronises."""
        if self.slot is None:
            raise ValueError("this leveling stream is closed")
        return self.stage.trace(self.slot)

    def close(self):
        self.closed = True
        if self.slot is not None:
            self.stage.close(self.slot)
            self.slot = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class StreamStretcher:
    """One stream at another speaking rate and / or pitch (_Common.open_stretcher): f32 chunks at 24 kHz in, f32 tensors on the device out
    (possibly empty) - a slot of a stages.StreamStretchStage at rq_eff, then, for a pitch, a slot of a stages.StreamResampleStage at
    (pq, 65536).  An output appears once the 1407 input samples behind the start of its hop's frame are in (latency_seconds; the pitch
    resampler adds its H + 1); finish() ends the stream as the clip's end and frees the slots.  A context manager: leaving it closes the
    stream."""

    def __init__(self, stretch_stage, pitch_stage, rq_eff, pq, keep_map=False):
        self.stretch_stage, self.pitch_stage, self.rq, self.pq = stretch_stage, pitch_stage, int(rq_eff), int(pq)
        self.slot = self.pitch_slot = None
        self.closed = False
        self._offsets = [] if keep_map else None
        try:
            if stretch_stage is not None:
                self.slot = stretch_stage.open(self.rq)
            if pitch_stage is not None:
                self.pitch_slot = pitch_stage.open(self.pq, E.RS_PITCH_ONE)
        except Exception:
            self.close()
            raise
        self.n_in = self.n_out = 0
        late = tsm.stream_latency() if stretch_stage is not None else 0.0
        if pitch_stage is not None:
            late += rs.stream_latency(self.pq, E.RS_PITCH_ONE) * self.rq / E.TSM_RATE_ONE
        self.latency_seconds = late / float(E.TSM_SAMPLE_RATE)

    def _push(self, chunk, flush):
        if self.closed:
            raise ValueError("this time-stretch stream is closed")
        y = torch.as_tensor(chunk, dtype=torch.float32).reshape(-1)
        self.n_in += y.shape[0]
        if self.slot is not None:
            if self._offsets is None:
                y = self.stretch_stage.push_many([(self.slot, y, flush)])[0]
            else:
                (y,), (off,) = self.stretch_stage.push_many([(self.slot, y, flush)], return_offsets=True)
                self._offsets.append(off)
        if self.pitch_slot is not None:
            y = self.pitch_stage.push_many([(self.pitch_slot, y, flush)])[0]
        self.n_out += y.shape[0]
        return y

    def push(self, chunk):
        return self._push(chunk, False)

    def finish(self, chunk=None):
        """The outputs still due (after an optional last chunk); the stream is over and its slots free."""
        y = self._push(torch.zeros(0) if chunk is None else chunk, True)
        self.close()
        return y

    def anchors(self):
        """keep_map=True: int64 [frames so far, 2] anchors (output sample of the time-stretch, input sample) of the frames that have run
        (stretch.anchors; after finish() they are stretch_many(return_map=True)'s).  Synchronises."""
        if self._offsets is None:
            raise ValueError("anchors(): open the stretcher with keep_map=True")
        off = torch.cat([o.cpu() for o in self._offsets]) if self._offsets else torch.zeros(0, dtype=torch.int32)
        return tsm.anchors(self.rq, off) if off.numel() else torch.zeros(0, 2, dtype=torch.int64)

    def close(self):
        self.closed = True
        if self.slot is not None:
            self.stretch_stage.close(self.slot)
            self.slot = None
        if self.pitch_slot is not None:
            self.pitch_stage.close(self.pitch_slot)
            self.pitch_slot = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _Common:
    """What this module's TextToSpeech and api_fast.TextToSpeech share: the lazy tokenizer, the seed, the text front-end."""
    world = 1  # processes that share one utterance's work (TextToSpeech with candidate sharding sets its own)

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            from .text import VoiceBpeTokenizer
            self._tokenizer = VoiceBpeTokenizer(self.tokenizer_args[0], self.tokenizer_args[1], self.models_dir)
        return self._tokenizer

    def deterministic_state(self, seed=None):
        """api.py:598-609."""
        seed = int(torch.seed() % (2 ** 31)) if seed is None else int(seed)
        if self.world > 1:
            seed = tdist.broadcast_int(seed)  # every rank must draw the same noise and key the same Philox streams
        torch.manual_seed(seed)
        random.seed(seed)
        return seed

    def _text_tokens(self, text, max_mel_tokens):
        """One text (str, or ids: int sequence / tensor [T]) to be spoken in max_mel_tokens -> padded int32 tokens [1, T + 1] on the device
        (api.py:388-392)."""
        ids = self.tokenizer.encode(text) if isinstance(text, str) else text
        tokens = F.pad(torch.as_tensor(ids, dtype=torch.int32).reshape(1, -1).to(self.device), (0, 1))  # api.py:391
        if tokens.shape[-1] >= 400:  # api.py:392
            raise ValueError("Too much text provided. Break the text up into separate segments and re-try inference.")
        if max_mel_tokens > self.max_mel_tokens_cap:
            raise ValueError(f"max_mel_tokens={max_mel_tokens} exceeds the capacity this engine was built with "
                             f"(TextToSpeech(max_mel_tokens={self.max_mel_tokens_cap}))")
        return tokens

    # ------------------------------------------------------------------ the wav2vec2 aligner: redaction and word timings
    aligner = None
    _aligner_source = None
    aligner_dtype = E.TT_F16  # (bf16 after an overflow; not one of the four dtype_names() stages)
    ctc = None

    def _aligner_max_samples(self):
        return ORIG_ALIGNER_SECONDS * align.ORIG_SR

    def load_aligner(self):
        """wav2vec_alignment.py:51-58: the wav2vec2 CTC aligner of the redaction path as a device stage, from `aligner=` or the files find_aligner
        locates.  NotImplementedError when there are none (bracketed text cannot be redacted without them)."""
        if self.aligner is None:
            src = self._aligner_source if self._aligner_source is not None else align.find_aligner(self.models_dir)
            if src is None:
                raise NotImplementedError("text with [bracketed] passages is redacted from the audio by the wav2vec2 aligner (api.py:583-587), "
                                          "whose files were not found: " + align.where_to_put_files(self.models_dir) +
                                          "; or construct TextToSpeech(enable_redaction=False) to have the brackets spoken")
            self._aligner_source = src
            self.aligner = stages.AlignerStage(src, self.device, self.aligner_dtype, max_samples=self._aligner_max_samples())
        return self.aligner

    def load_ctc(self):
        """The forced-alignment stage, sized from the aligner (rebuilt with it)."""
        al = self.load_aligner()
        if self.ctc is None or self._ctc_of is not al:
            if self.ctc is not None:
                self.ctc.close()
            self.ctc, self._ctc_of = stages.CtcAlignStage.for_aligner(al), al
        return self.ctc

    def _aligner_run(self, clip, logits):
        """One clip [1, n] through the aligner -> (the stage, frame ids as a host list | logits f32 [T, vocab] on the device).  An fp16
        overflow rebuilds the aligner with bf16 operands and runs the same clip again."""
        while True:
            al = self.load_aligner()
            out = al.run(clip, logits=True)[1] if logits else al.frame_ids(clip)
            if logits and out.is_cuda:
                torch.cuda.current_stream(out.device).synchronize()  # (the guard is read after the run)
            if not al.guard():
                return al, out
            if al.dtype != E.TT_F16:
                raise E.OperandOverflow("the aligner stage produced non-finite values with bf16 operands (non-finite weights or audio?)")
            import warnings
            warnings.warn("tortoise_tts_amd: the aligner stage overflowed fp16 operands; rebuilding it with bf16 operands")
            al.close()
            self.aligner, self.aligner_dtype = None, E.TT_BF16

    @torch.no_grad()
    def align_many(self, audios, texts):
        """Where every text is spoken in its clip: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device), texts in spoken form (numbers
        and abbreviations are not expanded: a character the aligner's vocabulary lacks is given the boundary of the one before it) ->
        [align.Alignment].  The aligner runs clip by clip; the CTC forced alignment of all of them is ONE device call.  ValueError for a
        clip with fewer frames than its text needs."""
        audios, texts = list(audios), list(texts)
        if len(audios) != len(texts):
            raise ValueError(f"{len(audios)} clips with {len(texts)} texts")
        tok = self.load_aligner().tokenizer
        targets = [align.alignment_targets(t, tok) for t in texts]
        clips = [a.reshape(1, -1) for a in audios]
        logits = [self._aligner_run(c, True)[1] for c in clips]
        res = self.load_ctc().align_many(logits, [t.ids for t in targets])
        frame_len = align.frame_samples(self.aligner.fields)
        out = []
        for i, (r, t, c, lg) in enumerate(zip(res, targets, clips, logits)):
            n = c.shape[-1]
            if r["status"] == E.CTC_OK:
                out.append(align.build_alignment(t, r["spans"].tolist(), r["conf"].tolist(), r["score"], n, frame_len))
            elif r["status"] == E.CTC_EMPTY:
                out.append(align.empty_alignment(t, n))
            elif r["status"] == E.CTC_INFEASIBLE:
                raise ValueError(f"forced alignment: clip {i} has {lg.shape[0]} frames ({n} samples), too few for the {len(t.ids)} characters "
                                 f"of its text")
            else:
                raise RuntimeError(f"forced alignment: clip {i} was refused by the device stage (status {r['status']})")
        return out

    def align(self, audio, text):
        """align_many of one clip -> align.Alignment (characters and words with start / end samples and confidences, .seconds(), .to_srt())."""
        return self.align_many([audio], [text])[0]

    def _spoken_text(self, text):
        """What a clip returned for `text` speaks: without the [bracketed] passages when they are redacted."""
        if getattr(self, "redacts_brackets", False) and self.enable_redaction and "[" in text:
            bare, keep = align.redaction_plan(text)
            return " ".join(bare[a:b + 1] for a, b in keep)
        return text

    def tts_with_timings(self, text, **tts_kwargs):
        """tts(text, **tts_kwargs) and where its words are -> (what tts returns, align.Alignment - a list of k of them for k > 1; None where
        tts returns no audio, i.e. on the other ranks of a sharded job).  The text is aligned as spoken (see align_many).  With sample_rate=
        the clip is aligned at 24 kHz and converted afterwards; the Alignment then counts samples of the returned audio and carries its
        rate (.seconds() and .to_srt() use it).
        word_rates= (a list with one speaking rate per word of the text as spoken, None for a word left alone; or a dict {word index:
        rate}; each in [0.5, 2.0]): single words or phrases slower or faster, SSML's <prosody rate>.  It goes with speaking_rate= (the rate
        of everything else: the other words and the pauses) and pitch=.  The clip is rendered without post-processing and aligned at
        24 kHz, which costs ONE EXTRA ALIGNER PASS; the words' spans become a stretch.RateMap (from_words; left in self.rate_maps), and the
        usual chain runs with ONE time-stretch along that map, the pitch folded into every segment's rate: redaction -> stretch and the
        one resampling -> formants -> pauses -> loudness -> sample rate.  The returned timings are those of the returned audio, aligned as always.
        Single-rank instances only.  How natural a jump between neighbouring words sounds nobody has judged on a trained checkpoint.
        word_pitches= (a list with one pitch in semitones per word, None for a word left alone; or a dict {word index: semitones}; each
        within +-12): single words higher or lower, SSML's <prosody pitch>.  It goes with pitch= (the pitch of everything else), word_rates=
        and speaking_rate=; the one aligner pass serves both maps, the segments are the union of their word borders (at most 64 together),
        and the chain runs ONE time-stretch and ONE resampling along them with every word's duration kept (_tts_at_word_pitches; the maps
        are left in self.pitch_maps).  formants='keep' / formant_shift= are refused with it.  Pitch steps between neighbouring words,
        without formant correction, nobody has judged either."""
        if not isinstance(text, str):
            raise TypeError("tts_with_timings aligns the text with the audio: pass it as a str, not as token ids")
        self.load_aligner()  # (missing files are reported before anything renders)
        sample_rate = rs.options(dict(sample_rate=tts_kwargs.pop("sample_rate", None)))[1]  # (the aligner reads 24 kHz: converted after it)
        word_rates, word_pitches = tsm.word_rates(tts_kwargs), rs.word_pitches(tts_kwargs)
        if tts_kwargs.get("pitch_hz") is not None:  # (refused before anything renders; the inner tts() call measures and shifts)
            f0m.options(dict(pitch_hz=tts_kwargs["pitch_hz"], word_pitches=word_pitches), tts_kwargs.get("pitch") or None, "tts_with_timings")
        if "f0_smooth" in tts_kwargs:  # (validated, and refused without pitch_hz, before anything renders)
            f0m.smooth_option(dict(f0_smooth=tts_kwargs["f0_smooth"]), tts_kwargs.get("pitch_hz"), "tts_with_timings")
        if word_pitches is not None:
            res = self._tts_at_word_pitches(text, word_rates, word_pitches, tts_kwargs)
        else:
            res = self.tts(text, **tts_kwargs) if word_rates is None else self._tts_at_word_rates(text, word_rates, tts_kwargs)
        out = res[0] if tts_kwargs.get("return_deterministic_state") else res
        if out is None:
            return res, None
        clips = out if isinstance(out, (list, tuple)) else [out]
        als = self.align_many(clips, [self._spoken_text(text)] * len(clips))
        if sample_rate is not None:  # the returned audio and its timings are at sample_rate
            conv = self._at_sample_rate(list(clips), sample_rate)
            als = [align.resample_alignment(al, sample_rate, c.shape[-1]) for al, c in zip(als, conv)]
            out = conv if isinstance(out, (list, tuple)) else conv[0]
            res = (out,) + tuple(res[1:]) if tts_kwargs.get("return_deterministic_state") else out
        return res, (als if isinstance(out, (list, tuple)) else als[0])

    def _tts_at_word_rates(self, text, word_rates, tts_kwargs):
        """tts(text, **tts_kwargs) with its post-processing run along a rate map of the words -> what tts returns."""
        if getattr(self, "world", 1) > 1:
            raise ValueError("tts_with_timings: word_rates is not available on a sharded job (the ranks that return no audio have nothing to "
                             "align); build a single-rank instance")
        kw = dict(tts_kwargs)
        rate, level = tsm.speaking_rate(kw), loud.level_options(kw)
        pitch = rs.options(kw, rate)[0]
        pauses, formants = sil.options(kw), fmt.options(kw, pitch)
        res = self.tts(text, **kw)  # (rendered and redacted, nothing else)
        state = bool(kw.get("return_deterministic_state"))
        out = res[0] if state else res
        clips = list(out) if isinstance(out, (list, tuple)) else [out]
        als = self.align_many(clips, [self._spoken_text(text)] * len(clips))
        self.rate_maps = [tsm.RateMap.from_words(al, word_rates, base=1.0 if rate is None else rate) for al in als]
        clips = self._voiced(self._at_map(clips, self.rate_maps, pitch), None, None, level, None, pauses, formants)
        out = clips if isinstance(out, (list, tuple)) else clips[0]
        return (out,) + tuple(res[1:]) if state else out

    def _tts_at_word_pitches(self, text, word_rates, word_pitches, tts_kwargs):
        """tts(text, **tts_kwargs) with its post-processing run along a pitch map of the words (and a rate map, with word_rates) -> what
        tts returns.  ONE aligner pass on the plain clip serves both maps; the segments are taken over the union of their word borders
        (at most 64 together); ONE time-stretch at stretch_rq(rq_i, pq_i) per segment and ONE resampling at pq_i along the stretch's own
        borders keep every word's duration len_i / rate_i (resample.WarpChain, resample.duration_bound); then pauses and level as always.
        The maps are left in self.pitch_maps (and self.rate_maps)."""
        if getattr(self, "world", 1) > 1:
            raise ValueError("tts_with_timings: word_pitches is not available on a sharded job (the ranks that return no audio have nothing to "
                             "align); build a single-rank instance")
        kw = dict(tts_kwargs)
        rs.refuse_formants(kw.get("formants"), kw.get("formant_shift"), "tts_with_timings(word_pitches=)")
        rate, level = tsm.speaking_rate(kw), loud.level_options(kw)
        pitch = rs.options(kw, rate)[0]
        pauses = sil.options(kw)
        fmt.options(kw, None)  # (takes the formant keywords out; 'follow' and the lifter options change nothing)
        base_rate, base_pitch = 1.0 if rate is None else rate, 0.0 if pitch is None else pitch
        res = self.tts(text, **kw)  # (rendered and redacted, nothing else)
        state = bool(kw.get("return_deterministic_state"))
        out = res[0] if state else res
        clips = list(out) if isinstance(out, (list, tuple)) else [out]
        als = self.align_many(clips, [self._spoken_text(text)] * len(clips))
        self.pitch_maps = [rs.PitchMap.from_words(al, word_pitches, base=base_pitch) for al in als]
        self.rate_maps = [tsm.RateMap.from_words(al, {} if word_rates is None else word_rates, base=base_rate) for al in als]
        chains = []
        for al, rm, pm in zip(als, self.rate_maps, self.pitch_maps):
            def name(i, b, al=al):
                at = [f"word {k} ({w!r})" for k, (w, a, _, _) in enumerate(al.words) if int(a) == b]
                return f"tts_with_timings: {at[0] if at else 'the segment at sample %d' % b}"
            chains.append(rs.WarpChain(al.samples, *rs.merge_maps(al.samples, list(zip(rm.starts, rm.rqs)), list(zip(pm.starts, pm.pqs)), name)))
        clips = self._at_chains(clips, chains)
        if any(c.stretch is not None for c in chains):
            self._note(stretch_s=self._stretch_s)
        if any(set(c.pqs) != {E.RS_PITCH_ONE} for c in chains):
            self._note(pitch_s=self._resample_s)
        clips = self._voiced(clips, None, None, level, None, pauses, None)
        out = clips if isinstance(out, (list, tuple)) else clips[0]
        return (out,) + tuple(res[1:]) if state else out

    # ------------------------------------------------------------------ what the clip-level calls below share
    def _clip_stage(self, attr, name, max_samples, cap, what, floor):
        """The stages.<name> kept in self.<attr>: refused above `cap` samples (what the library takes), built on first use for clips of at
        least `floor` samples, closed and rebuilt for a longer clip."""
        if max_samples > cap:
            raise ValueError(f"a clip of {max_samples} samples exceeds what the {what} can take ({cap})")
        st = getattr(self, attr)
        if st is None or (st.max_total_samples if hasattr(st, "max_total_samples") else st.max_samples) < max_samples:
            if st is not None:
                st.close()
            setattr(self, attr, getattr(stages, name)(max(int(max_samples), floor), device=self.device))
        return getattr(self, attr)

    def _streaming_stage(self, attr, name, max_streams):
        """The streaming stages.<name> kept in self.<attr>, built on first use."""
        if getattr(self, attr) is None:
            setattr(self, attr, getattr(stages, name)(max_streams, device=self.device))
        return getattr(self, attr)

    @staticmethod
    def _clip(i, a, who):
        """Clip i of a call is [n], [1, n] or [1, 1, n]; ValueError in the name of `who`."""
        if not 1 <= a.dim() <= 3 or a.numel() != a.shape[-1] or a.numel() == 0:
            raise ValueError(f"{who}: clip {i} of shape {tuple(a.shape)}, expected [n], [1, n] or [1, 1, n] with n >= 1")

    def _clips(self, audios, who):
        """The clips of a call as a list, every one checked (_clip)."""
        audios = list(audios)
        for i, a in enumerate(audios):
            self._clip(i, a, who)
        return audios

    @staticmethod
    def _per_clip(v, n):
        """One value for all n clips, or one per clip."""
        return list(v) if isinstance(v, (list, tuple)) else [v] * n

    @staticmethod
    def _like(a, y):
        """The stage's result y in the shape and on the device of the clip a it was made from."""
        return y.to(a.device).reshape(a.shape[:-1] + (-1,))

    @staticmethod
    def _winners(clips, step):
        """What a tts call is about to return, {winner: clip} or a list, through step(list of clips) -> list; given back as it came."""
        keys = sorted(clips) if isinstance(clips, dict) else None
        seq = step([clips[i] for i in keys] if keys is not None else list(clips))
        return dict(zip(keys, seq)) if keys is not None else seq

    def _note(self, **seconds):
        self.timings = dict(getattr(self, "timings", None) or {}, **seconds)

    @staticmethod
    def _subset(seq, todo, fn):
        """fn(the clips of `seq` at the indices `todo`) -> as many clips, put back in their places; no call where `todo` is empty."""
        if todo:
            for i, y in zip(todo, fn([seq[i] for i in todo])):
                seq[i] = y
        return seq

    # ------------------------------------------------------------------ speaking rate: WSOLA time-stretch of finished clips
    stretcher = None
    warp_stretcher = None

    def load_warp_stretch(self, max_samples=0):
        """The time-stretch along a rate map (stages.WarpStretchStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("warp_stretcher", "WarpStretchStage", max_samples, E.TSM_MAX_SAMPLES, "time-stretch",
                                ORIG_ALIGNER_SECONDS * E.TSM_SAMPLE_RATE)

    def load_stretch(self, max_samples=0):
        """The time-stretch stage (stages.TimeStretchStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("stretcher", "TimeStretchStage", max_samples, E.TSM_MAX_SAMPLES, "time-stretch",
                                ORIG_ALIGNER_SECONDS * E.TSM_SAMPLE_RATE)

    @torch.no_grad()
    def stretch_many(self, audios, rates=None, durations=None, return_map=False, rate_maps=None):
        """The same speech at another speed and the same pitch: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device) -> the stretched
        clips, each in the shape and on the device it came in.  Give exactly one of `rates` (2.0: twice as fast; one value or one per clip,
        each in [0.5, 2.0]) and `durations` (seconds the clip shall last: rate = n / (duration * 24000)).  All clips go through ONE device
        call per 16.  return_map=True: also, per clip, int64 [K, 2] anchors (output sample, input sample) of the frames the output was
        assembled from (stretch.anchors), with which a time in the original clip is carried over to the stretched one.
        rate_maps=[...] instead of rates / durations: a speaking rate that changes inside the clip - per clip a stretch.RateMap
        (from_segments, from_anchors, from_words) or a list of (start_seconds, rate); ONE device call per 16 again (csrc/tsm_warp.hip), and
        a map of one segment gives the bits of `rates`."""
        audios = list(audios)
        if rate_maps is not None:
            if rates is not None or durations is not None:
                raise ValueError("stretch: give exactly one of rate, duration and rate_map")
            return self._stretch_maps(audios, rate_maps, return_map)
        if (rates is None) == (durations is None):
            raise ValueError("stretch: give exactly one of rate, duration and rate_map")
        given = rates if durations is None else durations
        given = self._per_clip(given, len(audios))
        if len(given) != len(audios):
            raise ValueError(f"stretch: {len(audios)} clips with {len(given)} {'rates' if durations is None else 'durations'}")
        self._clips(audios, "stretch")
        rqs = [tsm.rate_q(v if durations is None else tsm.rate_for_duration(a.shape[-1], v)) for a, v in zip(audios, given)]
        if not audios:
            return ([], []) if return_map else []
        t0 = time.perf_counter()
        res = self.load_stretch(max(a.shape[-1] for a in audios)).stretch_many([a.reshape(-1) for a in audios], rqs)
        out = [self._like(a, y) for a, (y, _) in zip(audios, res)]  # (the offsets' copy back has synchronised)
        self._stretch_s = time.perf_counter() - t0
        return (out, [tsm.anchors(rq, off) for rq, (_, off) in zip(rqs, res)]) if return_map else out

    def stretch(self, audio, rate=None, duration=None, rate_map=None):
        """stretch_many of one clip -> the stretched clip."""
        return self.stretch_many([audio], rates=rate, durations=duration, rate_maps=None if rate_map is None else [rate_map])[0]

    def _stretch_maps(self, audios, rate_maps, return_map):
        """stretch_many along rate maps."""
        rate_maps = list(rate_maps)
        if len(rate_maps) != len(audios):
            raise ValueError(f"stretch: {len(audios)} clips with {len(rate_maps)} rate maps")
        self._clips(audios, "stretch")
        maps = [tsm.rate_map(a.shape[-1], m) for a, m in zip(audios, rate_maps)]
        if not audios:
            return ([], []) if return_map else []
        t0 = time.perf_counter()
        res = self.load_warp_stretch(max(a.shape[-1] for a in audios)).stretch_many([a.reshape(-1) for a in audios], [m.table for m in maps])
        out = [self._like(a, y) for a, (y, _) in zip(audios, res)]  # (the offsets' copy back has synchronised)
        self._stretch_s = time.perf_counter() - t0
        return (out, [m.anchors(off) for m, (_, off) in zip(maps, res)]) if return_map else out

    @torch.no_grad()
    def retime_many(self, audios, anchors, durations=None, return_map=False):
        """The dubbing call: every clip stretched so that given moments of it sound at given times.  audios as in stretch_many; anchors: per
        clip a list of (src_seconds, dst_seconds) - what is at src in the clip is to sound at dst in the result, both increasing, (0, 0)
        implied; durations (None, one value or one per clip; seconds): the final anchor (the clip's end, duration).  Between two anchors
        the rate is constant and must lie in [0.5, 2.0] (ValueError names the pair); behind a last anchor inside the clip the rest runs
        at rate 1.0.  The plan lands within (dst_(i+1) - m_i) / 65536 + 1 samples of every dst (stretch.RateMap.from_anchors); the audio itself
        sits where WSOLA puts it, within its search range (+-256 samples, 10.7 ms) of that, as for a constant rate.  ONE device call per
        16 clips.  return_map=True: also the anchors of the frames, as in stretch_many."""
        audios, anchors = list(audios), list(anchors)
        if len(anchors) != len(audios):
            raise ValueError(f"retime: {len(audios)} clips with {len(anchors)} anchor lists")
        durations = self._per_clip(durations, len(audios))
        if len(durations) != len(audios):
            raise ValueError(f"retime: {len(audios)} clips with {len(durations)} durations")
        to_s = lambda t: int(round(float(t) * E.TSM_SAMPLE_RATE))
        maps = []
        for i, (a, pts, d) in enumerate(zip(audios, anchors, durations)):
            self._clip(i, a, "retime")
            pts = [(to_s(s_), to_s(t)) for s_, t in (pts or [])]
            if d is not None:
                if not float(d) > 0:
                    raise ValueError(f"retime: duration={d} must be positive (seconds)")
                pts.append((a.shape[-1], to_s(d)))
            if not pts:
                raise ValueError(f"retime: clip {i}: give anchors, a duration or both")
            maps.append(tsm.RateMap.from_anchors(a.shape[-1], pts))
        return self._stretch_maps(audios, maps, return_map)

    def retime(self, audio, anchors=None, duration=None, return_map=False):
        """retime_many of one clip -> the retimed clip (return_map=True: and its anchors)."""
        res = self.retime_many([audio], [anchors], durations=duration, return_map=return_map)
        return (res[0][0], res[1][0]) if return_map else res[0]

    def _at_map(self, clips, maps, semitones):
        """The clips of a tts call (a list) along their rate maps (speaking rates) at pitch `semitones` (None: 0): ONE stretch for all of
        them along the maps with the pitch folded into every segment, rq_i -> round(rq_i 65536 / pq), and ONE resampling by (pq, 65536);
        their time in timings['stretch_s'] / ['pitch_s'].  A clip whose map is rate 1.0 throughout is not stretched."""
        pq = E.RS_PITCH_ONE if semitones is None else rs.pitch(semitones)[0]
        maps = [m.with_pitch(pq) for m in maps]
        self._stretch_s = 0.0
        seq = list(clips)
        todo = [i for i, m in enumerate(maps) if m.rqs != [E.TSM_RATE_ONE]]
        if todo:
            self._subset(seq, todo, lambda sub: self.stretch_many(sub, rate_maps=[maps[i] for i in todo]))
            self._note(stretch_s=self._stretch_s)
        if pq != E.RS_PITCH_ONE:
            seq = self._resample_ratios(seq, [(pq, E.RS_PITCH_ONE)] * len(seq), False)
            self._note(pitch_s=self._resample_s)
        return seq

    stream_stretcher = None
    stream_pitch_resampler = None

    def load_stream_stretch(self, max_streams=16):
        """The streaming time-stretch of open_stretcher (stages.StreamStretchStage), built on first use."""
        return self._streaming_stage("stream_stretcher", "StreamStretchStage", max_streams)

    def load_stream_pitch(self, max_streams=16):
        """The streaming resampler behind open_stretcher's pitch (a stages.StreamResampleStage of its own), built on first use."""
        return self._streaming_stage("stream_pitch_resampler", "StreamResampleStage", max_streams)

    def open_stretcher(self, rate=None, pitch=None, keep_map=False):
        """A StreamStretcher for 24 kHz audio that arrives in chunks: push(chunk) returns the samples that became ready, finish() the rest;
        their concatenation is stretch(whole clip, rate) - with a pitch, the time-stretch and the resampling shift_pitch / tts(pitch=)
        make - to the bit, whatever the chunking.  rate (0.5 .. 2.0) and pitch (semitones, +-12) are validated as speaking_rate= and
        pitch= of tts() are.  keep_map=True: anchors() gives stretch_many(return_map=True)'s anchors.  Up to 16 may be open."""
        if rate is not None:
            tsm.rate_q(rate)
        pq, rq_eff = rs.pitch(0.0 if pitch is None else pitch, rate)
        if rq_eff == E.TSM_RATE_ONE and pq == E.RS_PITCH_ONE:
            raise ValueError("open_stretcher: give a rate other than 1.0 or a pitch other than 0 semitones")
        if keep_map and rq_eff == E.TSM_RATE_ONE:
            raise ValueError("open_stretcher: keep_map=True needs a time-stretch (this rate and pitch need none)")
        return StreamStretcher(self.load_stream_stretch() if rq_eff != E.TSM_RATE_ONE else None,
                               self.load_stream_pitch() if pq != E.RS_PITCH_ONE else None, rq_eff, pq, keep_map)

    def _at_rate(self, clips, rate):
        """The clips a tts call is about to return ({winner: clip} or a list), at speaking_rate `rate`: one stretch_many call for all of
        them, its time in timings['stretch_s']."""
        self._stretch_s = 0.0
        out = self._winners(clips, lambda seq: self.stretch_many(seq, rates=rate))
        self._note(stretch_s=self._stretch_s)
        return out

    # ------------------------------------------------------------------ level: integrated loudness, true peak, gain under a ceiling
    leveller = None

    def load_loudness(self, max_samples=0):
        """The loudness stage (stages.LoudnessStage), built on first use for sixteen clips of 30 s and rebuilt for a longer clip."""
        return self._clip_stage("leveller", "LoudnessStage", max_samples, E.LOUD_MAX_SAMPLES, "loudness stage", LOUDNESS_STAGE_SAMPLES)

    @torch.no_grad()
    def loudness_many(self, audios):
        """Integrated loudness (ITU-R BS.1770-4 / EBU R 128, gated) and 4x oversampled true peak of every clip: audios f32 [n] / [1, n] /
        [1, 1, n] at 24 kHz (any device) -> [loudness.Loudness], all clips in ONE device call per 16."""
        audios = self._clips(audios, "loudness")
        if not audios:
            return []
        res = self.load_loudness(max(a.shape[-1] for a in audios)).measure_many([a.reshape(-1) for a in audios])
        return [loud.reading(r) for r in res]

    def loudness(self, audio):
        """loudness_many of one clip -> loudness.Loudness."""
        return self.loudness_many([audio])[0]

    @torch.no_grad()
    def normalize_many(self, audios, loudness=-23.0, true_peak=-1.0, limit="scale", return_info=False):
        """Every clip brought to `loudness` LUFS under a true-peak ceiling of `true_peak` dBTP, each in the shape and on the device it came
        in; measured and applied on the device without a round trip in between.  loudness / true_peak: one value or one per clip.  limit:
        'scale' (the gain is lowered until the ceiling holds; the shortfall is reported), 'lookahead' (a 5 ms look-ahead limiter takes the
        peaks down instead) or 'none'.  A clip shorter than 400 ms or without a block above -70 LUFS is returned unchanged.
        return_info=True: also [loudness.Loudness]."""
        audios = self._clips(audios, "normalize")
        targets, peaks = self._per_clip(loudness, len(audios)), self._per_clip(true_peak, len(audios))
        if len(targets) != len(audios) or len(peaks) != len(audios):
            raise ValueError(f"normalize: {len(audios)} clips with {len(targets)} targets and {len(peaks)} ceilings")
        levels = [loud.level(T, p, limit) for T, p in zip(targets, peaks)]
        if not audios:
            return ([], []) if return_info else []
        t0 = time.perf_counter()
        res = self.load_loudness(max(a.shape[-1] for a in audios)).normalize_many(
            [a.reshape(-1) for a in audios], [lv.loudness for lv in levels], [lv.ceiling for lv in levels], loud.MODES[limit or "scale"])
        out = [self._like(a, y) for a, (y, _) in zip(audios, res)]  # (the readings' copy back has synchronised)
        self._level_s = time.perf_counter() - t0
        return (out, [loud.reading(r, lv.loudness) for (_, r), lv in zip(res, levels)]) if return_info else out

    def normalize(self, audio, loudness=-23.0, true_peak=-1.0, limit="scale"):
        """normalize_many of one clip -> the clip at its level."""
        return self.normalize_many([audio], loudness, true_peak, limit)[0]

    def _at_level(self, clips, level):
        """The clips a tts call is about to return ({winner: clip} or a list), at `level` (loudness.Level): one normalize_many call for all
        of them, its time in timings['level_s'], the readings in self.loudness_info."""
        self._level_s = 0.0

        def step(seq):
            out, self.loudness_info = self.normalize_many(seq, level.loudness, level.true_peak, level.limit, return_info=True)
            return out
        out = self._winners(clips, step)
        self._note(level_s=self._level_s)
        return out

    # ------------------------------------------------------------------ level a stream: causal loudness, slew-limited gain, limiter
    stream_leveller = None

    def load_stream_level(self, max_streams=16):
        """The streaming leveler of open_leveler / level (stages.StreamLevelStage), built on first use."""
        return self._streaming_stage("stream_leveller", "StreamLevelStage", max_streams)

    def open_leveler(self, loudness=None, gain=None, true_peak=None, limit=None, **options):
        """A StreamLeveler for 24 kHz audio that arrives in chunks: push(chunk) returns the samples that became ready, finish() the rest;
        their concatenation is level(whole clip, ...) to the bit, whatever the chunking.  loudness (LUFS: the gain follows the loudness
        heard so far towards it) or gain (dB, fixed) - exactly one; true_peak (dBTP) and limit ('lookahead' | 'none') as
        stream_true_peak= / stream_limit= of tts_stream; options: assume, boost, cut, rise, fall (loudness.STREAM_LEVEL_DEFAULTS).  Up to 16
        may be open."""
        settings = loud.stream_settings(loudness, gain, true_peak, limit, options or None)  # (validated before a slot is taken)
        return StreamLeveler(self.load_stream_level(), settings)

    @torch.no_grad()
    def level_many(self, audios, loudness=None, gain=None, true_peak=None, limit=None, return_info=False, **options):
        """The CAUSAL leveler applied to finished clips: every clip through one flushed push of a slot of the streaming leveler, each in
        the shape and on the device it came in - what a stream with these settings would have emitted for it.  When the whole clip
        exists, normalize() is the one to use: it measures the clip's integrated loudness first and reaches the target exactly.
        return_info=True: also [loudness.StreamLevel]."""
        audios = self._clips(audios, "level")
        settings = loud.stream_settings(loudness, gain, true_peak, limit, options or None)
        stage = self.load_stream_level()
        out, info = [], []
        for k in range(0, len(audios), stage.max_streams):
            part = audios[k:k + stage.max_streams]
            slots = []
            try:
                for _ in part:
                    slots.append(stage.open(settings))
                ys = stage.push_many([(s, a.reshape(-1), True) for s, a in zip(slots, part)])
                out += [self._like(a, y) for a, y in zip(part, ys)]
                if return_info:
                    info += [loud.stream_reading(stage.read(s)) for s in slots]
            finally:
                for s in slots:
                    stage.close(s)
        return (out, info) if return_info else out

    def level(self, audio, loudness=None, gain=None, true_peak=None, limit=None, **options):
        """level_many of one clip -> the clip as a stream at these settings would have come out."""
        return self.level_many([audio], loudness, gain, true_peak, limit, **options)[0]

    # ------------------------------------------------------------------ pitch and output sample rate: the arbitrary-ratio resampler
    resampler = None

    def load_resample(self, max_samples=0):
        """The resampling stage (stages.ResampleStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("resampler", "ResampleStage", max_samples, E.RS_MAX_SAMPLES, "resampler", ORIG_ALIGNER_SECONDS * rs.SAMPLE_RATE)

    def _resample_ratios(self, audios, ratios, return_info):
        """audios (validated) at (P, Q) each -> the clips, each in the shape and on the device it came in; all of them through ONE device
        call per 16.  A ratio of 1 is no call: the clip is returned as it is (the resampler's P = Q is a low-pass, not a copy)."""
        t0 = time.perf_counter()
        todo = [i for i, (P, Q) in enumerate(ratios) if P != Q]
        out, peaks = list(audios), [None] * len(audios)
        if todo:
            res = self.load_resample(max(audios[i].shape[-1] for i in todo)).resample_many([audios[i].reshape(-1) for i in todo],
                                                                                          [ratios[i] for i in todo])
            for i, (y, pk) in zip(todo, res):  # (the peaks' copy back has synchronised)
                out[i], peaks[i] = self._like(audios[i], y), pk
        if return_info:
            peaks = [float(a.abs().max()) if pk is None else pk for a, pk in zip(audios, peaks)]
        self._resample_s = time.perf_counter() - t0
        return (out, peaks) if return_info else out

    @torch.no_grad()
    def resample_many(self, audios, to_rates, from_rates=rs.SAMPLE_RATE, return_info=False):
        """The same audio at another sample rate: audios f32 [n] / [1, n] / [1, 1, n] (any device) -> the converted clips, each in the shape
        and on the device it came in.  to_rates / from_rates: Hz, one value or one per clip, any positive integers whose reduced ratio has
        terms up to 2^20 and lies in 1/8 .. 8 (24000 -> 8000 / 16000 / 44100 / 48000, or a 44100 Hz voice clip -> 22050).  A Kaiser-windowed
        sinc with its cutoff at 0.9 of the narrower Nyquist frequency (csrc/resample.hip): pass-band within 0.001 dB, everything else below
        -100 dB.  All clips go through ONE device call per 16.  return_info=True: also the sample peak max |y| of every returned clip."""
        audios = self._clips(audios, "resample")
        to_rates, from_rates = self._per_clip(to_rates, len(audios)), self._per_clip(from_rates, len(audios))
        if len(to_rates) != len(audios) or len(from_rates) != len(audios):
            raise ValueError(f"resample: {len(audios)} clips with {len(to_rates)} target rates and {len(from_rates)} source rates")
        return self._resample_ratios(audios, [rs.ratio(f, t) for f, t in zip(from_rates, to_rates)], return_info)

    def resample(self, audio, to_rate, from_rate=rs.SAMPLE_RATE):
        """resample_many of one clip -> the clip at to_rate."""
        return self.resample_many([audio], to_rate, from_rate)[0]

    stream_resampler = None

    def load_stream_resample(self, max_streams=16):
        """The streaming resampler of open_resampler (stages.StreamResampleStage), built on first use."""
        return self._streaming_stage("stream_resampler", "StreamResampleStage", max_streams)

    def open_resampler(self, to_rate, from_rate=rs.SAMPLE_RATE):
        """A StreamResampler for audio that arrives in chunks: push(chunk) returns the samples at to_rate that became ready, finish() the
        rest; their concatenation is resample(whole clip, to_rate, from_rate) to the bit, whatever the chunking.  Up to 16 may be open."""
        P, Q = rs.ratio(from_rate, to_rate)
        return StreamResampler(self.load_stream_resample(), P, Q, int(from_rate))

    @torch.no_grad()
    def shift_pitch_many(self, audios, semitones=None, return_info=False, formants=None, formant_lifter_ms=None, formant_max_gain_db=None,
                         pitch_maps=None, return_map=False, to_hz=None, f0_smooth=None):
        """The same speech at another pitch and the same duration: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device), semitones
        (+: up; one value or one per clip, each within +-12) -> the shifted clips.  Two batched device calls: a time-stretch at rate
        65536^2 / pq (rounded; pq = round(2^(s/12) 65536)), then a resampling by (pq, 65536), which undoes the stretch's change of duration
        (to within the rounding of the two lengths) and moves every frequency by 2^(s/12).  Pitch by resampling moves the formants with
        the pitch: it stays natural for a few semitones, and nobody has rendered a trained checkpoint through it.  0 semitones returns the
        clip as it is.  return_info=True: also the sample peak of every returned clip.  formants='keep': a third batched call, the cepstral
        envelope correction at warp 2^(s/12) (shift_formants_many's kernel and options), puts the formants back where they were; the peaks
        of return_info are then those of the corrected clips.  None or 'follow': the two calls alone.
        pitch_maps=[...] instead of semitones: a pitch that changes inside the clip, SSML's <prosody pitch> - per clip a resample.PitchMap
        (from_segments, from_words) or a list of (start_seconds, semitones).  Every segment keeps its duration: ONE time-stretch along
        the map at rate 65536^2 / pq_i per segment (csrc/tsm_warp.hip), then ONE resampling along it (csrc/resample_warp.hip) whose borders
        are where the stretch put them; the position is continuous across a border, the low-pass changes there.  Every border and the end
        land within resample.duration_bound of where they were.  A map of 0 semitones throughout returns the clip as it is, a map of one
        segment takes the path of `semitones`.  return_map=True: also, per clip, int64 [S + 1, 2] anchors (input sample, output sample) of
        every border and of the end.  The formants move with each segment's pitch: formants='keep' is refused with a map.  Nobody has
        listened to pitch steps between neighbouring words on a trained checkpoint.
        to_hz=H (one value or one per clip, 50 .. 1000 Hz) instead of semitones: an absolute pitch, SSML's <prosody pitch="180Hz">.  ONE
        f0_many call measures the clips (csrc/f0.hip), and every clip is shifted by 12 log2(H / its median F0) through the calls above, a
        ratio per clip; formants='keep' stays allowed.  A shift beyond +-12 semitones is clamped and a clip with fewer than 10 voiced
        frames is returned bit for bit, each with a warning.  return_info=True then gives, per clip, a dict measured_hz (None: no
        median), semitones, clamped and peak; the readings are also left in self.pitch_info.
        f0_smooth= (True, or a dict of costs: pitch.smooth_params) with to_hz: that one f0_many call runs smoothed (f0_many's smooth=), so
        a run of frames read an octave off does not move the median; without to_hz it is refused."""
        audios = self._clips(audios, "shift_pitch")
        if (semitones is None) + (pitch_maps is None) + (to_hz is None) != 2:
            raise ValueError("shift_pitch: give exactly one of semitones and pitch_map, or to_hz")
        smooth = f0m.smooth_option(dict(f0_smooth=f0_smooth), to_hz, "shift_pitch")
        if to_hz is not None:
            if return_map:
                raise ValueError("shift_pitch: return_map=True goes with pitch_map")
            fmt.mode(formants)
            semis, info = self._shifts_to(audios, to_hz, "shift_pitch", smooth)
            out, peaks = self.shift_pitch_many(audios, semis, True, formants, formant_lifter_ms, formant_max_gain_db) if audios else ([], [])
            for d, pk in zip(info, peaks):
                d["peak"] = pk
            return (out, info) if return_info else out
        if pitch_maps is not None:
            rs.refuse_formants(formants, None, "shift_pitch(pitch_map=)")
            return self._shift_maps(audios, pitch_maps, return_info, return_map)
        if return_map:
            raise ValueError("shift_pitch: return_map=True goes with pitch_map")
        semis = self._per_clip(semitones, len(audios))
        if len(semis) != len(audios):
            raise ValueError(f"shift_pitch: {len(audios)} clips with {len(semis)} pitches")
        plans = [rs.pitch(s_) for s_ in semis]
        keep = fmt.mode(formants)
        corr = [fmt.params(s_, keep, None, formant_lifter_ms, formant_max_gain_db) for s_ in semis]
        if any(p is not None for p in corr):
            out = self.shift_pitch_many(audios, semis)
            out = self._correct_formants(out, corr)
            return (out, [float(a.abs().max()) for a in out]) if return_info else out
        t0 = time.perf_counter()
        res = self._resample_ratios(self._stretched(list(audios), plans), [(pq, E.RS_PITCH_ONE) for pq, _ in plans], return_info)
        self._resample_s = time.perf_counter() - t0
        return res

    def shift_pitch(self, audio, semitones=None, formants=None, pitch_map=None, return_map=False, to_hz=None, **options):
        """shift_pitch_many of one clip -> the shifted clip (options: formant_lifter_ms, formant_max_gain_db); pitch_map= instead of
        semitones: a pitch that changes inside the clip (return_map=True: and its anchors); to_hz= instead of either: the clip with its
        median F0 moved to that many Hz (return_info=True: and its reading)."""
        if to_hz is not None:
            info = options.pop("return_info", False)
            res = self.shift_pitch_many([audio], semitones, info, formants, pitch_maps=None if pitch_map is None else [pitch_map],
                                        return_map=return_map, to_hz=to_hz, **options)
            return (res[0][0], res[1][0]) if info else res[0]
        if pitch_map is None and not return_map:
            return self.shift_pitch_many([audio], semitones, formants=formants, **options)[0]
        res = self.shift_pitch_many([audio], semitones, formants=formants, pitch_maps=None if pitch_map is None else [pitch_map],
                                    return_map=return_map, **options)
        return (res[0][0], res[1][0]) if return_map else res[0]

    warp_resampler = None

    def load_warp_resample(self, max_samples=0):
        """The resampling along a pitch map (stages.WarpResampleStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("warp_resampler", "WarpResampleStage", max_samples, E.RS_MAX_SAMPLES, "resampler",
                                2 * ORIG_ALIGNER_SECONDS * rs.SAMPLE_RATE)

    def _shift_maps(self, audios, pitch_maps, return_info, return_map):
        """shift_pitch_many along pitch maps."""
        pitch_maps = list(pitch_maps)
        if len(pitch_maps) != len(audios):
            raise ValueError(f"shift_pitch: {len(audios)} clips with {len(pitch_maps)} pitch maps")
        maps = [rs.pitch_map(a.shape[-1], m) for a, m in zip(audios, pitch_maps)]
        self.pitch_maps = maps
        chains = []
        for m in maps:  # (neighbours at one pitch are one segment: a map that says 3 semitones twice takes the constant path)
            segs = [(b, p) for i, (b, p) in enumerate(zip(m.starts, m.pqs)) if i == 0 or p != m.pqs[i - 1]]
            chains.append(rs.WarpChain(m.n, [b for b, _ in segs], [E.TSM_RATE_ONE] * len(segs), [p for _, p in segs]))
        out = self._at_chains(audios, chains)
        res = (out,)
        if return_info:
            res += ([float(a.abs().max()) for a in out],)
        if return_map:
            res += ([c.anchors for c in chains],)
        return res if len(res) > 1 else out

    def _stretched(self, seq, plans):
        """The list `seq` with every clip whose plan (pq, rq_eff) has a rate other than 1.0 time-stretched at it, in ONE stretch_many call
        (rate 1.0 is the input itself: not stretched)."""
        todo = [i for i, (_, rq) in enumerate(plans) if rq != E.TSM_RATE_ONE]
        return self._subset(seq, todo, lambda sub: self.stretch_many(sub, rates=[plans[i][1] / E.TSM_RATE_ONE for i in todo]))

    def _at_chains(self, audios, chains):
        """audios (validated) each along its resample.WarpChain -> the clips, each in the shape and on the device it came in: ONE
        time-stretch call per 16 for the clips whose speaking rate or pitch changes inside them, and ONE resampling call.  What is
        constant over a clip takes the constant kernels (their bits: a table of one segment gives them anyway), and what is 1.0
        throughout runs nothing; their time in self._stretch_s / self._resample_s."""
        seq = list(audios)
        self._stretch_s = 0.0
        const = [i for i, c in enumerate(chains) if c.stretch is not None and len(c.stretch) == 1]
        warp = [i for i, c in enumerate(chains) if c.stretch is not None and len(c.stretch) > 1]
        self._subset(seq, const, lambda sub: self.stretch_many(sub, rates=[chains[i].rq_effs[0] / E.TSM_RATE_ONE for i in const]))
        spent = self._stretch_s  # (still 0.0 where no clip took that call)
        maps = [tsm.RateMap(chains[i].n, chains[i].starts, chains[i].rq_effs) for i in warp]
        self._subset(seq, warp, lambda sub: self.stretch_many(sub, rate_maps=maps))
        self._stretch_s = spent + self._stretch_s if warp else spent
        t0 = time.perf_counter()
        flat = [i for i, c in enumerate(chains) if len(set(c.pqs)) == 1]
        bent = [i for i, c in enumerate(chains) if len(set(c.pqs)) > 1]
        self._subset(seq, flat, lambda sub: self._resample_ratios(sub, [(chains[i].pqs[0], E.RS_PITCH_ONE) for i in flat], False))

        def along(sub):  # (the peaks' copy back has synchronised)
            stage = self.load_warp_resample(max(a.shape[-1] for a in sub))
            res = stage.resample_many([a.reshape(-1) for a in sub], [chains[i].resample for i in bent])
            return [self._like(a, y) for a, (y, _) in zip(sub, res)]
        self._subset(seq, bent, along)
        self._resample_s = time.perf_counter() - t0
        assert all(y.shape[-1] == c.n_out for y, c in zip(seq, chains)), "the chain's plans and the stages agree on every length"
        return seq

    # ------------------------------------------------------------------ F0: the YIN tracker
    f0_stage = None
    pitch_info = None

    def load_f0(self, max_samples=0):
        """The F0 stage (stages.F0Stage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("f0_stage", "F0Stage", max_samples, E.F0_MAX_SAMPLES, "F0 tracker", ORIG_ALIGNER_SECONDS * f0m.SAMPLE_RATE)

    f0_path_stage = None

    def load_f0_path(self, max_samples=0):
        """The Viterbi F0 stage (stages.F0ViterbiStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("f0_path_stage", "F0ViterbiStage", max_samples, E.F0_MAX_SAMPLES, "F0 tracker", ORIG_ALIGNER_SECONDS * f0m.SAMPLE_RATE)

    @torch.no_grad()
    def f0_many(self, audios, fmin=f0m.DEFAULTS["fmin"], fmax=f0m.DEFAULTS["fmax"], threshold=f0m.DEFAULTS["threshold"],
                floor_db=f0m.DEFAULTS["floor_db"], smooth=None):
        """The fundamental frequency of every clip: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device) -> [pitch.F0Track], a frame
        every 10 ms (hz 0 where unvoiced, aperiodicity, voiced, times(), median_hz(), semitones(ref), range_semitones(), at(seconds),
        for_words(alignment)).  YIN (de Cheveigne & Kawahara 2002) over a 40 ms window: the first dip of the normalised difference
        below `threshold` among the periods of fmin .. fmax Hz (within 50 .. 1000), refined by a parabola; a frame without such a dip, or
        with its power below floor_db dBFS, is unvoiced.  No smoothing over frames: an octave jump in one frame stays in the track (the
        median does not see it).  All clips go through ONE device call per 16 (csrc/f0.hip).  The defaults were chosen from the paper
        and the code: nobody has tuned them on a trained checkpoint's audio.
        smooth= (one value or one per clip; None / False: off, the call and the bits above): True or a dict of costs (octave_cost,
        jump_cost, voicing_cost, unvoiced_cost; pitch.smooth_params) keeps up to seven dips of every frame as candidates and chooses among
        them, and "unvoiced", with a Viterbi path over the whole clip (csrc/f0_viterbi.hip), so a run of frames read an octave high or low
        is pulled back by its neighbours.  The tracks are then `.smoothed`, with `.state` and `.path_cost`; `.octave_jumps()` counts what
        is left on either kind of track.  Clips with smooth off and clips with it on take one call each.  The default costs were chosen
        from the arithmetic: nobody has tuned them on a trained checkpoint's audio either."""
        audios = self._clips(audios, "f0")
        p = f0m.params(fmin, fmax, threshold, floor_db)
        costs = [smooth] * len(audios) if isinstance(smooth, f0m.Costs) else self._per_clip(smooth, len(audios))  # (a Costs is a tuple, and ONE setting)
        if len(costs) != len(audios):
            raise ValueError(f"f0: {len(audios)} clips with {len(costs)} smooth settings")
        costs = [f0m.smooth_params(c) for c in costs]
        if not audios:
            return []
        seq = [a.reshape(-1) for a in audios]
        plain, path = [i for i, c in enumerate(costs) if c is None], [i for i, c in enumerate(costs) if c is not None]
        res = [None] * len(seq)
        if plain:
            sub = [seq[i] for i in plain]
            for i, r in zip(plain, self.load_f0(max(x.shape[0] for x in sub)).track_many(sub, [p] * len(sub))):
                res[i] = r
        if path:
            sub = [seq[i] for i in path]
            for i, r in zip(path, self.load_f0_path(max(x.shape[0] for x in sub)).track_many(sub, [p] * len(sub), [costs[i] for i in path])):
                res[i] = r
        return [f0m.track_of(r, a.shape[-1]) for r, a in zip(res, audios)]

    def f0(self, audio, **options):
        """f0_many of one clip -> pitch.F0Track."""
        return self.f0_many([audio], **options)[0]

    def _shifts_to(self, audios, to_hz, who, smooth=None):
        """audios (validated) and the pitch to land on (Hz: one value or one per clip) -> (semitones per clip, [dict(measured_hz, semitones,
        clamped)]): ONE f0_many call (smoothed with `smooth`, a pitch.Costs), then pitch.shift_to per clip.  The readings are left in
        self.pitch_info."""
        hzs = self._per_clip(to_hz, len(audios))
        if len(hzs) != len(audios):
            raise ValueError(f"{who}: {len(audios)} clips with {len(hzs)} target pitches")
        hzs = [f0m.target_hz("to_hz" if who == "shift_pitch" else "pitch_hz", h) for h in hzs]
        t0 = time.perf_counter()
        tracks = self.f0_many(audios, smooth=smooth)
        semis, info = [], []
        for i, (tr, h) in enumerate(zip(tracks, hzs)):
            med = tr.median_hz()
            s, clamped = f0m.shift_to(med, h, who, i if len(audios) > 1 else None)
            semis.append(s)
            info.append(dict(measured_hz=med, semitones=s, clamped=clamped))
        self.pitch_info = info
        self._f0_s = time.perf_counter() - t0
        return semis, info

    def _pitch_hz_plan(self, clips, hz, formant_kw, who="tts", smooth=None):
        """pitch_hz= of a tts call: the clips it is about to return ({winner: clip} or a list), measured in ONE device call -> (semitones
        per clip in the clips' order, formant.Params or None per clip: formants='keep' takes every clip's own shift back)."""
        seq = [clips[i] for i in sorted(clips)] if isinstance(clips, dict) else clips
        semis, _ = self._shifts_to(self._clips(seq, who), hz, who, smooth)
        self._note(f0_s=self._f0_s)
        kw = dict(formant_kw or {})
        keep = fmt.mode(kw.get("formants"))
        plans = [fmt.params(s_ if s_ != 0.0 else None, keep, kw.get("formant_shift"), kw.get("formant_lifter_ms"), kw.get("formant_max_gain_db"))
                 for s_ in semis]
        return semis, plans

    # ------------------------------------------------------------------ formants: the cepstral envelope correction
    formant_stage = None

    def load_formant(self, max_samples=0, q=None, max_gain_db=None, clips=1):
        """The formant stage (stages.FormantStage), sized from the batch it is first asked for: the longest clip rounded up to whole
        seconds and min(clips, 16) clips per call, 13,056 bytes of intermediates per frame (94 frames a second) and clip slot - 12 MB for
        one clip of 10 s, 196 MB for sixteen.  It is rebuilt, never smaller, for a longer clip, a larger batch or another lifter or clamp."""
        q = fmt.lifter_q() if q is None else int(q)
        g = fmt.max_gain_db() if max_gain_db is None else float(max_gain_db)
        need = max(-(-int(max_samples) // fmt.SAMPLE_RATE), 1) * fmt.SAMPLE_RATE
        slots = max(1, min(int(clips), E.FMT_MAX_CLIPS))
        st = self.formant_stage
        if st is None or st.max_samples < need or st.max_clips < slots or st.q != q or st.max_gain_db != g:
            if st is not None:
                need, slots = max(need, st.max_samples), max(slots, st.max_clips)
                st.close()
            self.formant_stage = stages.FormantStage(need, q, g, max_clips=slots, device=self.device)
        return self.formant_stage

    def _correct_formants(self, audios, plans):
        """audios (validated) with one fmt.Params or None each -> the clips, each in the shape and on the device it came in; the clips of
        one (lifter, clamp) go through ONE device call per 16.  None is no call: the clip is returned as it is."""
        t0 = time.perf_counter()
        out = list(audios)
        for key in sorted({(p.q, p.max_gain_db) for p in plans if p is not None}):
            todo = [i for i, p in enumerate(plans) if p is not None and (p.q, p.max_gain_db) == key]
            for i in todo:
                if audios[i].shape[-1] < fmt.MIN_SAMPLES:
                    raise ValueError(f"formants: clip {i} has {audios[i].shape[-1]} samples; the correction needs at least {fmt.MIN_SAMPLES}")
            stage = self.load_formant(max(audios[i].shape[-1] for i in todo), *key, clips=len(todo))
            res = stage.correct_many([audios[i].reshape(-1) for i in todo], [plans[i].alpha for i in todo])
            for i, y in zip(todo, res):
                out[i] = self._like(audios[i], y)
        self._formant_s = time.perf_counter() - t0
        return out

    @torch.no_grad()
    def shift_formants_many(self, audios, semitones, formant_lifter_ms=None, formant_max_gain_db=None):
        """The same speech at the same pitch and duration with its formants moved: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device,
        n >= 513), semitones (+: up, a smaller speaker; one value or one per clip, each within +-12) -> the clips, each in the shape and on
        the device it came in.  The spectral envelope (the first formant_lifter_ms of the cepstrum, 2 ms by default) of every frame is read
        at 2^(-f / 12) times each frequency and the frame's spectrum gets the difference as a gain of at most formant_max_gain_db (24 dB);
        the harmonics stay where they are (csrc/formant.hip - DESIGN.md 5.32).  All clips go through ONE device call per 16.  0 semitones
        returns the clip as it is.  Nobody has listened to a trained checkpoint through it."""
        audios = self._clips(audios, "shift_formants")
        semis = self._per_clip(semitones, len(audios))
        if len(semis) != len(audios):
            raise ValueError(f"shift_formants: {len(audios)} clips with {len(semis)} shifts")
        return self._correct_formants(audios, [fmt.params(None, False, f, formant_lifter_ms, formant_max_gain_db) for f in semis])

    def shift_formants(self, audio, semitones, **options):
        """shift_formants_many of one clip -> the clip with its formants moved."""
        return self.shift_formants_many([audio], semitones, **options)[0]

    def _at_formants(self, clips, params):
        """The clips a tts call is about to return ({winner: clip} or a list) corrected with `params` (formant.Params): one call for all of
        them, its time in timings['formant_s']."""
        # (params as a list: one per clip, None allowed)
        out = self._winners(clips, lambda seq: self._correct_formants(seq, list(params) if isinstance(params, list) else [params] * len(seq)))
        self._note(formant_s=self._formant_s)
        return out

    def _at_pitch(self, clips, rate, semitones):
        """The clips a tts call is about to return ({winner: clip} or a list) at speaking_rate `rate` (None: 1.0) and pitch `semitones`: ONE
        stretch_many call at rq_eff = round(rq 65536 / pq) and ONE resampling by (pq, 65536) for all of them; their time in
        timings['stretch_s'] / ['pitch_s']."""
        self._stretch_s = 0.0

        def step(seq):
            # a list: one pitch per clip (pitch_hz=), in the clips' order: still ONE stretch and ONE resampling.  rq_eff / 65536 is exact:
            # stretch.rate_q returns rq_eff
            plans = [rs.pitch(s_, rate) for s_ in semitones] if isinstance(semitones, list) else [rs.pitch(semitones, rate)] * len(seq)
            return self._resample_ratios(self._stretched(seq, plans), [(pq, E.RS_PITCH_ONE) for pq, _ in plans], False)
        out = self._winners(clips, step)
        self._note(stretch_s=self._stretch_s, pitch_s=self._resample_s)
        return out

    def _at_sample_rate(self, clips, sample_rate):
        """The clips a tts call is about to return ({winner: clip} or a list) converted from 24 kHz to `sample_rate`: the last step, one
        call for all of them, its time in timings['resample_s'], the sample peaks of the returned clips in self.resample_info."""
        def step(seq):
            seq, self.resample_info = self._resample_ratios(seq, [rs.ratio(rs.SAMPLE_RATE, sample_rate)] * len(seq), True)
            return seq
        out = self._winners(clips, step)
        self._note(resample_s=self._resample_s)
        return out

    # ------------------------------------------------------------------ noisy voice clips: the spectral-subtraction denoiser
    denoiser = None
    denoise_voice_samples = None  # TextToSpeech(denoise_voice_samples=): None | True | dict of denoise_many's options

    def load_denoiser(self, max_samples=0):
        """The denoiser (stages.DenoiseStage), built on first use for clips of 12 s and rebuilt for a longer one."""
        return self._clip_stage("denoiser", "DenoiseStage", max_samples, E.NR_MAX_SAMPLES, "denoiser", DENOISER_SECONDS * nr.VOICE_SAMPLE_RATE)

    @torch.no_grad()
    def denoise_many(self, audios, reduction_db=nr.DEFAULTS["reduction_db"], beta=nr.DEFAULTS["beta"], quantile=nr.DEFAULTS["quantile"],
                     smooth_frames=nr.DEFAULTS["smooth_frames"], smooth_bins=nr.DEFAULTS["smooth_bins"], noise=None, sample_rate=24000,
                     return_info=False):
        """Stationary noise (hiss, room noise) taken out of voice clips by spectral subtraction: audios f32 [n] / [1, n] / [1, 1, n] at any
        sample rate (any device, n >= 513) -> the clips, each in the shape and on the device it came in (csrc/denoise.hip - DESIGN.md
        5.38).  Per clip and frequency bin (frames of 1024 samples every 256) the noise power is the `quantile`-quantile of the bin's power
        over the clip's frames, an exact order statistic, corrected by 1 / (-ln(1 - quantile)), the factor between that quantile and the
        mean of a Gaussian noise bin; where the power, smoothed over 2 smooth_frames + 1 frames and 2 smooth_bins + 1 bins, exceeds
        `beta` times that floor the bin keeps the fraction 1 - beta floor / power of its amplitude, everywhere else, and at least,
        10^(-reduction_db / 20).  noise=(start_s, end_s) - one for all clips or one (or None) per clip, in seconds at `sample_rate`, which
        is used for nothing else - takes the floor as the mean power over the frames that lie whole inside that stretch (at least 8)
        instead.  **A clip with digital silence in more than `quantile` of its frames has an auto floor of exactly 0 and comes back as
        it is: give it a noise= region.**  A clip of fewer than 32 frames (8192 samples) without a region comes back as it is.
        reduction_db=0 or None calls nothing and returns the clips themselves.  All clips go through ONE device call per 16.
        return_info=True -> (clips, [dict(status 'ok' / 'short', noise_floor f32 [513], noise_dbfs, mean_attenuation_db)]).
        **The defaults come from the arithmetic and one synthetic family of vowels in Gaussian noise; nobody has run a real recording or a
        trained checkpoint through them.**"""
        audios = self._clips(audios, "denoise")
        p = nr.params(reduction_db, beta, quantile, smooth_frames, smooth_bins)
        one = noise is None or (isinstance(noise, (tuple, list)) and len(noise) == 2 and all(isinstance(v, (int, float)) for v in noise))
        noises = [noise] * len(audios) if one else list(noise)  # (a pair of numbers is one region for all clips)
        if len(noises) != len(audios):
            raise ValueError(f"denoise: {len(audios)} clips with {len(noises)} noise regions")
        for i, a in enumerate(audios):
            if a.shape[-1] < nr.MIN_SAMPLES:
                raise ValueError(f"denoise: clip {i} has {a.shape[-1]} samples; the denoiser needs at least {nr.MIN_SAMPLES}")
        regions = [nr.region_frames(r, a.shape[-1], sample_rate, "denoise", i) for i, (r, a) in enumerate(zip(noises, audios))]
        if p is None or not audios:
            return (audios, [None] * len(audios)) if return_info else audios
        t0 = time.perf_counter()
        res = self.load_denoiser(max(a.shape[-1] for a in audios)).denoise_many([a.reshape(-1) for a in audios], regions, p)
        out, info = [], []
        for a, (y, d) in zip(audios, res):
            out.append(self._like(a, y))
            if return_info:
                e_in, e_out = float(a.reshape(-1).double().pow(2).sum()), float(y.double().pow(2).sum())
                info.append(dict(status=nr.STATUS[d["status"]], noise_floor=d["floor"], noise_dbfs=nr.noise_dbfs(d["floor"]),
                                 mean_attenuation_db=10.0 * math.log10(e_in / e_out) if e_in > 0 and e_out > 0 else 0.0))
        self._denoise_s = time.perf_counter() - t0
        return (out, info) if return_info else out

    def denoise(self, audio, **options):
        """denoise_many of one clip -> the clip (with return_info=True: (clip, info))."""
        res = self.denoise_many([audio], **options)
        return (res[0][0], res[1][0]) if options.get("return_info") else res[0]

    def _clean_voice_samples(self, voice_samples, denoise, ready=lambda vs: False):
        """The waveform entries of voice_samples through ONE denoise_many call, before any mel front-end; ready mels and (auto_mel,
        diffusion_mel) pairs stay as they are.  denoise: the call's keyword, nr.INHERIT for the constructor's denoise_voice_samples."""
        p = nr.from_option(self.denoise_voice_samples if isinstance(denoise, str) and denoise == nr.INHERIT else denoise)
        todo = [i for i, vs in enumerate(voice_samples) if torch.is_tensor(vs) and not ready(vs)]
        if p is None or not todo:
            return voice_samples
        out = list(voice_samples)
        for i, y in zip(todo, self.denoise_many([out[i] for i in todo], sample_rate=nr.VOICE_SAMPLE_RATE, **nr.keywords(p))):
            out[i] = y
        return out

    # ------------------------------------------------------------------ pauses and silence: speech regions, edge trimming, pause capping
    silencer = None

    def load_silence(self, max_samples=0):
        """The silence stage (stages.SilenceStage), built on first use for clips of 30 s and rebuilt for a longer one."""
        return self._clip_stage("silencer", "SilenceStage", max_samples, E.SIL_MAX_SAMPLES, "silence stage", ORIG_ALIGNER_SECONDS * sil.SAMPLE_RATE)

    @torch.no_grad()
    def speech_regions_many(self, audios, top_db=sil.DEFAULTS["top_db"], floor_db=sil.DEFAULTS["floor_db"],
                            min_silence=sil.DEFAULTS["min_silence"], pad=sil.DEFAULTS["pad"]):
        """Where the speech is: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device) -> per clip (regions, pauses), lists of
        (start, end) in samples: the speech regions in ascending order and the pauses between them (silence.pauses; the silence before the
        first and after the last region is not listed).  A 10 ms frame is active when its energy is within top_db of the clip's loudest
        frame and above floor_db dBFS; pauses shorter than min_silence seconds are bridged and every region is padded by `pad` seconds.
        All clips go through ONE device call per 16.  A clip without an active frame has no region."""
        audios = self._clips(audios, "speech_regions")
        p = sil.params(lead=None, trail=None, max_pause=None, top_db=top_db, floor_db=floor_db, min_silence=min_silence, pad=pad)
        if not audios:
            return []
        res = self.load_silence(max(a.shape[-1] for a in audios)).find_many([a.reshape(-1) for a in audios], [p] * len(audios))
        return [(r["regions"], sil.pauses(r["regions"], a.shape[-1])) for r, a in zip(res, audios)]

    def speech_regions(self, audio, **options):
        """speech_regions_many of one clip -> (regions, pauses)."""
        return self.speech_regions_many([audio], **options)[0]

    def _trim_params(self, audios, params, return_map):
        """audios (validated) through the silence stage with one silence.Params each -> the clips, each in the shape and on the device it
        came in; ONE device call per 16.  The per-clip status and seconds removed are left in self.silence_info."""
        t0 = time.perf_counter()
        out, maps, info = [], [], []
        if audios:
            res = self.load_silence(max(a.shape[-1] for a in audios)).trim_many([a.reshape(-1) for a in audios], params)
            for a, (y, d) in zip(audios, res):  # (the results' copy back has synchronised)
                out.append(self._like(a, y))
                maps.append(d["segments"])
                info.append(dict(status=sil.STATUS[d["status"]], removed_s=(a.shape[-1] - y.shape[-1]) / sil.SAMPLE_RATE, regions=d["regions"]))
        self.silence_info = info
        self._silence_s = time.perf_counter() - t0
        return (out, maps) if return_map else out

    @torch.no_grad()
    def trim_many(self, audios, lead=sil.DEFAULTS["lead"], trail=sil.DEFAULTS["trail"], max_pause=sil.DEFAULTS["max_pause"],
                  top_db=sil.DEFAULTS["top_db"], floor_db=sil.DEFAULTS["floor_db"], min_silence=sil.DEFAULTS["min_silence"],
                  pad=sil.DEFAULTS["pad"], return_map=False):
        """Dead air cut away: audios f32 [n] / [1, n] / [1, 1, n] at 24 kHz (any device) -> the clips, each in the shape and on the device it
        came in.  At most `lead` / `trail` seconds of silence stay before the first / after the last speech region (a cut end is faded
        over 5 ms), and a pause longer than `max_pause` seconds is shortened to exactly that (its two ends cross-faded over 5 ms); None
        leaves that part alone.  Detection as in speech_regions_many.  Everything that is not cut, cross-faded or faded is a bit-for-bit
        copy; a clip without speech is returned as it is, never emptied.  All clips go through ONE device call per 16 (csrc/silence.hip),
        found and edited without a round trip in between.  The defaults were chosen from the code: nobody has run a trained checkpoint's
        audio through them.  return_map=True: also, per clip, the segment list [(output start, input start, length)], with which
        silence.map_sample carries a time in the original clip over to the trimmed one.  Status and seconds removed: self.silence_info."""
        audios = self._clips(audios, "trim")
        p = sil.params(lead=lead, trail=trail, max_pause=max_pause, top_db=top_db, floor_db=floor_db, min_silence=min_silence, pad=pad)
        return self._trim_params(audios, [p] * len(audios), return_map)

    def trim(self, audio, **options):
        """trim_many of one clip -> the trimmed clip."""
        return self.trim_many([audio], **options)[0]

    def _at_pauses(self, clips, params):
        """The clips a tts call is about to return ({winner: clip} or a list) with their pauses shaped by `params` (silence.Params): one
        call for all of them, its time in timings['silence_s'], status and seconds removed in self.silence_info."""
        out = self._winners(clips, lambda seq: self._trim_params(seq, [params] * len(seq), False))
        self._note(silence_s=self._silence_s)
        return out

    def _voiced(self, clips, rate, pitch, level, sample_rate, pauses=None, formants=None):
        """The chain behind redaction: speaking rate and pitch together, then the formants (formant.Params), then the pauses
        (silence.Params: durations are then delivered seconds), then the level (at 24 kHz: the loudness gate sees the final content), then
        the output sample rate."""
        if pitch is not None:
            clips = self._at_pitch(clips, rate, pitch)
        elif rate is not None:
            clips = self._at_rate(clips, rate)
        if formants is not None and not (isinstance(formants, list) and all(p is None for p in formants)):
            clips = self._at_formants(clips, formants)
        if pauses is not None:
            clips = self._at_pauses(clips, pauses)
        if level is not None:
            clips = self._at_level(clips, level)
        return clips if sample_rate is None else self._at_sample_rate(clips, sample_rate)


class TextToSpeech(_Common):
    """Main entry point; see the module docstring.  Engine-only keyword arguments (all optional, after
    the reference's): `state_dicts` (dict of reference-layout state_dicts instead of files in
    models_dir), `dtype` (MFMA operand type: 'bf16' | 'fp16' for every stage, or a dict per stage
    {'ar', 'clvp', 'diffusion', 'vocoder'}; see resolve_stage_dtypes for the defaults), `max_candidates`
    (per-GPU decode batch capacity), `configs` (ARConfig/CLVPConfig/DiffusionConfig/VocoderConfig overrides for tests), `aligner` ((config
    dict, state_dict, vocab dict, tokenizer config dict) of the wav2vec2 redaction aligner instead of its files), `winner_batch` (1 .. 16,
    default 1: the k winners of tts() are rendered one after the other; W >= 2: in groups of up to W, each ONE shared denoiser pass per
    diffusion step and ONE UnivNet call - DESIGN.md 5.20), `redaction` ('reference', the default: the reference's greedy-transcript
    heuristic, bit for bit; 'forced': the bracketed passages are cut at the character boundaries of the CTC forced alignment, which exists
    whenever the clip has enough frames - DESIGN.md 5.23).  Engine-only keyword of tts() / tts_with_preset() / tts_many(), taken out of
    **hf_generate_kwargs: `speaking_rate` (0.5 .. 2.0; None or 1.0: off) - every returned clip is time-stretched at the same pitch after
    redaction (stretch / stretch_many, csrc/tsm.hip - DESIGN.md 5.24); `loudness` (a target in LUFS, -70 .. -5; None: off) with `true_peak`
    (the ceiling in dBTP, default -1) and `limit` ('scale', the default, 'lookahead' or 'none') - every returned clip is then brought to the
    target under the ceiling, the last step after redaction and the speaking rate (normalize / normalize_many, csrc/loudness.hip - DESIGN.md
    5.25; the readings are left in `loudness_info`); `pitch` (semitones, +-12; None or 0: off) - every returned clip is shifted by ONE
    time-stretch at rate speaking_rate / 2^(pitch/12) and ONE resampling by 2^(pitch/12), together with the speaking rate (shift_pitch,
    csrc/resample.hip - DESIGN.md 5.27; pitch by resampling moves the formants with the pitch: natural for a few semitones, and nobody has
    rendered a trained checkpoint through it); `sample_rate` (Hz, an integer in 8000 .. 96000; None or 24000: off) - every returned clip
    is converted from 24 kHz last (resample).  The `true_peak` ceiling is enforced at 24 kHz, before that conversion: down-conversion
    removes content and can move the peak; the sample peaks of the converted clips are left in `resample_info`; `trim_silence` (True: at
    most 0.05 s of silence before and 0.1 s after the speech; or a dict of trim_many's options; None or False: off) and `max_pause`
    (seconds; every longer pause is shortened to it; None: off) - after the rate and the pitch and before the level (trim, csrc/silence.hip
    - DESIGN.md 5.28; the defaults were chosen from the code, nobody has run a trained checkpoint's audio through them; status and seconds
    removed are left in `silence_info`); `formants` ('keep': after a `pitch` the formants are put back where they were; None or 'follow':
    they move with the pitch) and `formant_shift` (semitones, +-12: the formants alone move up, with or without a pitch; the combined
    envelope warp 2^((pitch - formant_shift) / 12) must stay in 0.5 .. 2), with the options `formant_lifter_ms` (2) and
    `formant_max_gain_db` (24) - after the rate and the pitch and before the pauses (shift_formants, csrc/formant.hip - DESIGN.md 5.32;
    downward shifts are corrected less, and nobody has listened to a trained checkpoint through it)."""

    redacts_brackets = True  # tts() cuts [bracketed] passages out of its clips (enable_redaction)

    def __init__(self, autoregressive_batch_size=None, models_dir=MODELS_DIR, enable_redaction=True, kv_cache=False,
                 use_deepspeed=False, half=False, device=None, tokenizer_vocab_file=None, tokenizer_basic=False, *,
                 state_dicts=None, dtype=None, max_candidates=256, configs=None, max_mel_tokens=500, max_text_tokens=402,
                 candidate_sharding=True, utterance_batch=1, aligner=None, winner_batch=1, mel_front_end="torch", redaction="reference", denoise_voice_samples=None):
        nr.from_option(denoise_voice_samples)  # (validated now, used by get_conditioning_latents)
        self.denoise_voice_samples = denoise_voice_samples
        self.models_dir = models_dir
        self.mel_front_end_kind = stages.mel_front_end_kind(mel_front_end)
        if use_deepspeed:
            raise NotImplementedError("use_deepspeed: DeepSpeed kernel injection is a CUDA-only reference option; the MI355X engine "
                                      "always runs its own fused HIP path")
        # enable_redaction (reference default True): every clip of a text with '[' loses its [bracketed] passages (api.py:583-587); the
        # wav2vec2 aligner that finds them is built on first use (load_aligner)
        self.enable_redaction = bool(enable_redaction)
        if redaction not in ("reference", "forced"):
            raise ValueError(f"redaction={redaction!r}: 'reference' (the reference's greedy-transcript heuristic) or 'forced' (CTC forced alignment)")
        self.redaction = redaction
        self._aligner_source = aligner
        self.kv_cache = bool(kv_cache)
        self.half = bool(half)
        # candidate_sharding=False: this instance renders whole utterances on its own GPU even inside a multi-rank job (the
        # long-form driver spreads CHUNKS over the ranks instead: tortoise_tts_amd/longform.py, BASELINE config #4)
        self.rank, self.world = tdist.world() if candidate_sharding else (0, 1)
        # With >= 2 ranks a single winner's diffusion tail is split over ranks 0 and 1 (conditioned / conditioning-free
        # row each, one exchange per step).  TT_SPLIT_DIFFUSION=0 keeps the whole tail on rank 0.
        self.split_diffusion = self.world >= 2 and os.environ.get("TT_SPLIT_DIFFUSION", "1") != "0"
        if self.split_diffusion:
            tdist.pair_group()  # collective over all ranks: create it once, here, where every rank passes
        self.device = E.require_gpu(device)
        self.dtypes = resolve_stage_dtypes(dtype, half)  # half=True is the reference's fp16 autocast (api.py:180, autoregressive.py:561)
        self.dtype = self.dtypes["ar"]  # (conditioning encoders / random-latent MLPs follow the autoregressive stage)
        self.demotions = []             # stages whose overflow guard tripped and that were rebuilt with bf16 operands
        cfgs = configs or {}
        self.ar_cfg = cfgs.get("ar", ARConfig())
        self.clvp_cfg = cfgs.get("clvp", CLVPConfig())
        self.diff_cfg = cfgs.get("diffusion", DiffusionConfig())
        self.voc_cfg = cfgs.get("vocoder", VocoderConfig())
        self.cvvp_cfg = cfgs.get("cvvp", CVVPConfig())
        sds = state_dicts or {}

        def sd(name):
            return sds[name] if name in sds else _load_state_dict(models_dir, name)

        # the reference's default AR batch is 16 on a >=14 GB GPU (api.py:148-172); 288 GB of HBM3E decodes
        # every candidate of this rank in one batch unless the caller asks for smaller batches.
        cap = min(int(autoregressive_batch_size or max_candidates), max_candidates)
        self.autoregressive_batch_size = cap  # never above the handle's decode capacity
        self.tokenizer_args = (tokenizer_vocab_file, tokenizer_basic)
        self._tokenizer = None
        self.max_mel_tokens_cap = max_mel_tokens
        max_S = max_mel_tokens * 4 * 24000 // 22050 + 8
        # utterance_batch > 1 (tts_many, long-form reading): that many utterances share ONE decode batch - the KV caches of
        # utterance_batch x max_candidates sequences are resident (122 880 B per cached token: 8 x 256 x 200 tokens = 50 GB of the 288)
        self.utterance_batch = max(1, int(utterance_batch))
        if self.utterance_batch > 16:
            raise ValueError("utterance_batch is limited to 16 utterances per decode batch")
        if self.utterance_batch > 1 and torch.device(self.device).type == "cuda":
            need = utterance_batch_bytes(self.utterance_batch, cap, max_mel_tokens, self.ar_cfg, self.diff_cfg)
            total = torch.cuda.get_device_properties(self.device).total_memory
            if need > 0.8 * total:
                raise ValueError(f"utterance_batch={self.utterance_batch} x max_candidates={cap} x max_mel_tokens={max_mel_tokens} needs "
                                 f"{need / 2 ** 30:.0f} GiB of KV cache + integrator slices, the device has {total / 2 ** 30:.0f} GiB: "
                                 f"lower utterance_batch or max_mel_tokens")
        # winner_batch = W >= 2: tts(k > 1) renders this rank's winners in groups of up to W - one sample_many pass and one inference_many
        # call per group (_render_winners).  At full width the batched denoiser agrees with the solo run within the operand tolerance, not
        # bit for bit (DiffusionStage.sample_many), so the default stays 1: today's code path and today's bits.
        self.winner_batch = int(winner_batch)
        if not 1 <= self.winner_batch <= 16:
            raise ValueError("winner_batch must lie in 1 .. 16 (winners of one utterance rendered per denoiser / UnivNet pass)")
        # sequences one denoiser / UnivNet pass may hold: the diffusion handle's max_batch and the UnivNet handle's slots of max_S + 10 frames
        self._render_batch = max(self.utterance_batch, self.winner_batch) if self.winner_batch >= 2 else self.utterance_batch
        self._caps = dict(cap=cap, max_text_tokens=max_text_tokens, max_mel_tokens=max_mel_tokens, max_S=max_S)
        self._state_dicts = sds
        # tts_many also pushes utterance_batch utterances through ONE denoiser pass per diffusion step (padded to the longest)
        self.batch_diffusion = self.utterance_batch > 1
        # (Decoding batch i + 1 on a second stream while batch i's denoiser passes run was built and measured: both phases slow down by
        # what the other takes - decode 3.1 -> 4.35 s, rendering 2.85 -> 3.93 s for 15 chunks at 8 per batch, 6.4 -> 6.19 s in total, and
        # one batch of 16 is faster still, 6.06 s: profiles/r03_bench_read_overlap.txt - and removed again.)
        for name in STAGE_NAMES:
            self._build_stage(name)
        self.rlg = None         # random-voice latent MLPs, built lazily like the reference (api.py:301-309)
        self.cvvp = None        # "CVVP model is only loaded if used" (api.py:234): built by the first tts(cvvp_amount > 0)
        self.conditioning = None  # conditioning encoders (voice_samples path), built lazily
        self.mel_front_end = None
        # attributes the reference exposes and callers touch (api.py:408, 523)
        self.stop_mel_token = self.ar_cfg.stop_mel_token
        self.mel_length_compression = self.ar_cfg.mel_length_compression
        self.timings = {}

    def set_candidate_sharding(self, on):
        """Switch an instance inside a multi-rank job between sharding the candidates of ONE utterance over the ranks (on: one
        all_gather per utterance, the winner rendered by ranks 0 / 1) and rendering whole utterances on its own GPU (off: replicas, no
        data-path collective).  The engines need max_candidates >= the candidates a call decodes on this rank in either mode."""
        self.rank, self.world = tdist.world() if on else (0, 1)
        self.split_diffusion = self.world >= 2 and os.environ.get("TT_SPLIT_DIFFUSION", "1") != "0"
        if self.split_diffusion:
            tdist.pair_group()

    def _build_stage(self, name):
        """(Re)build one stage engine with self.dtypes[name] operands."""
        c, dt = self._caps, self.dtypes[name]
        old = getattr(self, {"ar": "ar", "clvp": "clvp", "diffusion": "diffusion", "vocoder": "vocoder"}[name], None)
        if old is not None:
            old.close()
        if name == "ar":
            # (capacity of at least 8 sequences: handles of <= 4 are streaming-size handles whose decode GEMMs run GEMV-shaped - other bits than
            #  the MFMA path - and a candidate's codes must not depend on how few candidates a rank happens to get: csrc/gemv.hip)
            self.ar = stages.ArStage(self._sd("autoregressive"), self.ar_cfg, self.device, dt, max_batch=max(c["cap"], 8) * self.utterance_batch,
                                     max_text=c["max_text_tokens"], max_new_tokens=c["max_mel_tokens"], max_latent_candidates=4,
                                     kv_cache=self.kv_cache, max_groups=self.utterance_batch)
        elif name == "clvp":
            # (tts_many ranks the utterances of a wave in ONE speech-tower pass: capacity for utterance_batch x cap candidates)
            self.clvp = stages.ClvpStage(self._sd("clvp"), self.clvp_cfg, self.device, dt,
                                         max_rows=max(c["cap"], 8) * c["max_mel_tokens"] * self.utterance_batch)
            if getattr(self, "cvvp", None) is not None:  # CVVP runs under the same autocast as CLVP in the reference (api.py:447-449): same operand type
                self.cvvp.close()
                self.cvvp = None
                self.load_cvvp()
        elif name == "diffusion":
            self.diffusion = stages.DiffusionStage(self._sd("diffusion"), self.diff_cfg, self.device, dt, max_seq=c["max_S"],
                                                   max_codes=c["max_mel_tokens"] + 8, max_steps=512, max_batch=self._render_batch)
        elif name == "vocoder":
            voc_sd = self._sd("vocoder")
            if any(k.endswith("weight_v") for k in voc_sd):
                voc_sd = W.fold_weight_norm(voc_sd)  # UnivNetGenerator.eval(inference=True), vocoder.py:284-298
            # (winner_batch >= 2: B clips of the longest length fit one call - B slots of max_S + 10 frames, about 150 KB of HBM per frame,
            #  include/tortoise_mi355x_univnet.h; the default instance keeps today's size)
            B = self._render_batch if self.winner_batch >= 2 else 1
            self.vocoder = stages.VocoderStage(voc_sd, self.voc_cfg, self.device, dt, max_frames=B * (c["max_S"] + 10) - 10)
        else:
            raise ValueError(name)

    def load_cvvp(self):
        """api.py:252-256: the CVVP model (cvvp.pth) as a device stage, with the CLVP stage's operand type."""
        if self.cvvp is None:
            c = self._caps
            self.cvvp = stages.CvvpStage(self._sd("cvvp"), self.cvvp_cfg, self.device, self.dtypes["clvp"],
                                         max_rows=max(c["cap"], 8) * c["max_mel_tokens"])
        return self.cvvp

    def _aligner_max_samples(self):
        return max(self._caps["max_S"] * 256 + 256, super()._aligner_max_samples())  # (its own clips, and align() of a caller's up to 30 s)

    def _redaction_text(self, text):
        """text when its clips are to be redacted (enable_redaction and a str with '['), else None.  Checked before anything renders: an
        unpaired '[' or a text with nothing outside brackets raises ValueError, missing aligner files NotImplementedError."""
        if not (self.enable_redaction and isinstance(text, str) and "[" in text):
            return None
        align.redaction_plan(text)
        self.load_aligner()
        return text

    def _redact(self, audio, text):
        """wav2vec_alignment.py redact on one rendered clip [1, 1, n] (any device) -> the clip without the [bracketed] passages, same device.
        An fp16 overflow rebuilds the aligner with bf16 operands and aligns the same clip again (the audio is not rendered again)."""
        t0 = time.perf_counter()
        clip = audio.reshape(1, -1)
        if self.redaction == "forced":  # cut at the forced alignment's character boundaries: no "could not align"
            out = align.redact_forced(clip, text, self.align).reshape(1, 1, -1)
        else:
            al, ids = self._aligner_run(clip, False)
            out = align.redact(clip, text, lambda _: ids, al.tokenizer).reshape(1, 1, -1)
        self._redact_s += time.perf_counter() - t0
        return out

    def _redact_clips(self, wavs, text):
        """{winner index: clip} this rank rendered -> the same clips redacted, on the CPU.  Runs after _guarded has accepted the utterance (a
        clip that a demotion is about to re-render is never aligned).  Alignment can fail on the data (RuntimeError / ValueError): with
        several ranks the outcome is agreed over them first, so that every rank raises together and none is left waiting in a collective."""
        out, err = {}, None
        try:
            for i, w in wavs.items():
                out[i] = self._redact(w, text).cpu()
        except Exception as ex:  # (any failure: the other ranks must hear of it before this one leaves)
            err = ex
        failed = tdist.any_over_ranks([err is not None])[0] if self.world > 1 else err is not None
        if err is not None:
            raise err
        if failed:
            raise RuntimeError("redaction failed on another rank of this job (its own error says why)")
        return out

    def _tripped_stages(self, wav_ok=True):
        """Stages whose operand-overflow guard counted non-finite values during the utterance that just finished (the caller has
        synchronised); agreed over the ranks so that every rank takes the same decision.  Resets the counters."""
        flags = []
        for name in ("ar", "clvp", "diffusion"):
            g = getattr(getattr(self, name), "guard", None)
            flags.append(bool(g()) if g is not None else False)
            if name == "clvp" and self.cvvp is not None and getattr(self.cvvp, "guard", None) is not None:
                flags[-1] = bool(self.cvvp.guard()) or flags[-1]  # (always read: reading resets the counter)
        vg = getattr(self.vocoder, "guard", None)  # non-finite predicted LVC kernels: the gate and the final tanh would hide them from wav_ok
        voc_tripped = bool(vg()) if vg is not None else False  # (always read: reading resets the counter)
        flags.append((not wav_ok) or voc_tripped)
        if self.world > 1:
            flags = tdist.any_over_ranks(flags)
        # only the FIRST tripped stage in pipeline order is at fault for certain: the later ones may merely have been fed its
        # non-finite output (an overflowed denoiser hands the vocoder a NaN mel); they get their own turn after the re-render
        return [n for n, f in zip(STAGE_NAMES, flags) if f][:1]

    def _demote(self, tripped):
        """fp16 stages among `tripped` are rebuilt with bf16 operands (same weights, fp32 exponent range); a stage that overflows
        in bf16 has non-finite weights or inputs: that is an error, not a precision choice."""
        import warnings
        for name in tripped:
            if self.dtypes[name] != E.TT_F16:
                raise E.OperandOverflow(f"the {name} stage produced non-finite values with bf16 operands (non-finite weights or inputs?)")
            warnings.warn(f"tortoise_tts_amd: the {name} stage overflowed fp16 operands; rebuilding it with bf16 operands and re-rendering")
            self.dtypes[name] = E.TT_BF16
            self.demotions.append(name)
            self._build_stage(name)

    # ------------------------------------------------------------------ reference helpers
    def get_conditioning_latents(self, voice_samples, return_mels=False, denoise=nr.INHERIT):
        """api.py:258-299 on the engine: ConditioningEncoder (autoregressive.py:204-228) and contextual_embedder
        (diffusion_decoder.py:186-192, 222-230) run on the device (csrc/cond.hip).  voice_samples is, as in
        the reference, a list of 22.05 kHz waveform tensors (the mel front-end of api.py:271-287 then runs in torch,
        tortoise_tts_amd/audio.py: restated without torchaudio / librosa, pinned through oracle/audio_oracle.py), or a list of ready
        (auto_mel f32 [1, 80, T_a], diffusion_mel f32 [1, 100, T_d]) pairs, one per clip.  denoise=True | dict | None: the waveform
        entries go through ONE denoise_many call first (its options; the default is the constructor's denoise_voice_samples)."""
        if torch.is_tensor(voice_samples):
            voice_samples = [voice_samples]  # api.py:269-270
        voice_samples = self._clean_voice_samples(voice_samples, denoise)
        if self.conditioning is None:
            self.conditioning = stages.ConditioningStage(self._sd("autoregressive"), self._sd("diffusion"), self.ar_cfg, self.diff_cfg,
                                                         self.device, self.dtype)
        auto_mels, diff_mels = [], []
        device_mels = None
        if self.mel_front_end_kind == "device":  # every waveform entry in one ragged call per mel (stages.MelFrontStage)
            waves = [vs for vs in voice_samples if torch.is_tensor(vs)]
            if waves:
                if self.mel_front_end is None:
                    self.mel_front_end = stages.MelFrontStage(self.models_dir, device=self.device)
                device_mels = iter(self.mel_front_end.many(waves))
        for vs in voice_samples:
            if isinstance(vs, (tuple, list)) and len(vs) == 2:
                am, dm = vs
            elif torch.is_tensor(vs) and device_mels is not None:
                am, dm = next(device_mels)
            elif torch.is_tensor(vs):
                if self.mel_front_end is None:
                    from .audio import MelFrontEnd
                    self.mel_front_end = MelFrontEnd(self.models_dir)
                am, dm = self.mel_front_end(vs.to(self.device))
            else:
                raise TypeError("voice_samples entries must be waveform tensors or (auto_mel, diffusion_mel) pairs")
            auto_mels.append(am.to(self.device).float().reshape(1, am.shape[-2], am.shape[-1]))
            diff_mels.append(dm.to(self.device).float().reshape(1, dm.shape[-2], dm.shape[-1]))
        auto_latent = self.conditioning.auto_latent(auto_mels)
        diffusion_latent = self.conditioning.diffusion_latent(diff_mels)
        if return_mels:
            return auto_latent, diffusion_latent, torch.stack(auto_mels, dim=1), torch.stack(diff_mels, dim=1)
        return auto_latent, diffusion_latent

    def _sd(self, name):
        return self._state_dicts[name] if name in self._state_dicts else _load_state_dict(self.models_dir, name)

    def get_random_conditioning_latents(self):
        """api.py:301-309: two RandomLatentConverter MLPs (random_latent_generator.py:42-55) on the device.  Like the
        reference, the Gaussian inputs are drawn from torch's CPU generator (it evaluates the MLPs on a CPU tensor), so the
        same torch.manual_seed gives the same random voice."""
        if self.rlg is None:
            self.rlg = stages.RandomLatentStage(self._sd("rlg_auto"), self._sd("rlg_diffuser"), self.device, self.dtype)
        ca, cd = self.rlg.channels  # 1024 / 2048 for the released rlg_auto.pth / rlg_diffuser.pth
        return self.rlg.latents(torch.randn(1, ca), torch.randn(1, cd))

    def dtype_names(self):
        """{'ar': 'bf16', ...}: the operand type every stage currently runs with (after any overflow demotion)."""
        return {k: E.DTYPE_NAMES[v] for k, v in self.dtypes.items()}

    def tts_with_preset(self, text, preset="fast", **kwargs):
        """api.py:311-332: same preset table, caller kwargs win."""
        settings = dict(BASE_SETTINGS)
        settings.update(PRESETS[preset])
        settings.update(kwargs)
        return self.tts(text, **settings)

    # ------------------------------------------------------------------ the pipeline
    @torch.no_grad()
    def tts(self, text, voice_samples=None, conditioning_latents=None, k=1, verbose=True, use_deterministic_seed=None,
            return_deterministic_state=False,
            # autoregressive generation parameters follow
            num_autoregressive_samples=512, temperature=.8, length_penalty=1, repetition_penalty=2.0, top_p=.8, max_mel_tokens=500,
            # CVVP parameters follow
            cvvp_amount=.0,
            # diffusion generation parameters follow
            diffusion_iterations=100, cond_free=True, cond_free_k=2, diffusion_temperature=1.0,
            **hf_generate_kwargs):
        if self.world > 1:
            f0m.refuse_sharded(hf_generate_kwargs, "tts")
        o = self._settings(locals())  # (the arguments above, by name)
        redact = self._redaction_text(text)
        tokens = self._text_tokens(text, max_mel_tokens)
        seed = self.deterministic_state(seed=use_deterministic_seed)
        ev = _StageTimer(6)
        ev.mark(0)
        voice = self._voice(voice_samples, conditioning_latents, mels=True)
        if o.cvvp_amount > 0:
            if o.cvvp_amount == 1 and voice[2] is None:
                raise ValueError("cvvp_amount=1 ranks the candidates by CVVP alone, which compares them with the voice's conditioning clips: "
                                 "pass voice_samples (with latents only the reference has nothing to rank by, api.py:462-472)")
            self.load_cvvp()  # api.py:450-453 (loaded even when there are no clips to use it on)
        wavs = self._guarded(lambda: self._utterance(ev, tokens, voice, o, seed, k, keep_on_device=redact is not None))  # (a re-render after a demotion: same seed)
        self.timings = _event_timings(ev)
        if redact is not None:
            self._redact_s = 0.0
            wavs = self._redact_clips(wavs, redact)
            self.timings["redact_s"] = self._redact_s
        # (every rank works on the clips it holds) the chain: redaction -> speaking rate and pitch -> formants -> pauses -> level -> output sample rate
        pitch, formants = o.pitch, o.formants
        if o.pitch_hz is not None:  # measured after redaction, ONE device call for all clips: a shift per clip
            pitch, formants = self._pitch_hz_plan(wavs, o.pitch_hz, o.formant_kw, smooth=o.f0_smooth)
        wavs = self._voiced(wavs, o.speaking_rate, pitch, o.level, o.sample_rate, o.pauses, formants)
        # Rendered winners go to rank 0 only (the reference returns the audio to ONE caller); other ranks get None entries.
        if self.world > 1:
            wavs = tdist.collect_on_rank0(wavs, k)
        res = None if wavs is None else [wavs[i] for i in range(k)] if k > 1 else wavs[0]
        return (res, (seed, text, voice_samples, conditioning_latents)) if return_deterministic_state else res

    def tts_many(self, texts, voice_samples=None, conditioning_latents=None, use_deterministic_seed=None, verbose=False, **kwargs):
        """Several utterances of one voice in one call - what tortoise/read.py:66-71 does chunk after chunk with the same seed.
        Returns [tts(text, ...) for text in texts] (k = 1: one clip f32 [1, 1, n] per text), computed with the autoregressive stage
        batched over `utterance_batch` utterances at a time: their candidates share one decode batch (own prefix, own Philox key per
        utterance), so every weight matrix streams once per step for all of them and the sampled codes of an utterance are
        bit-identical to rendering it alone.  With utterance_batch > 1 the CLVP ranking of a wave is ONE speech-tower pass over all its
        candidates (every score the bits of scoring the utterance alone) and the denoiser runs in shared, padded passes; the latent re-pass
        runs per utterance as in tts() and UnivNet vocodes a wave in one call (every clip the bits of vocoding it alone).  Single-rank instances only (long-form reading spreads whole chunks over the ranks, longform.py).
        speaking_rate= (0.5 .. 2.0): every clip is time-stretched at the same pitch, all of them in ONE stretch_many call.
        loudness= (LUFS; with true_peak= and limit=): after that, every clip is brought to the target, all of them in ONE normalize_many call.
        pitch= (semitones, +-12) goes with the speaking rate - ONE stretch and ONE resampling for all clips - and sample_rate= (Hz, 8000 ..
        96000) converts every clip last, in ONE call.  trim_silence= / max_pause= shape the pauses of every clip after the rate and the
        pitch and before the level, in ONE call (trim_many).  formants= / formant_shift= correct every clip's spectral envelope after the
        pitch and before the pauses, in ONE call (shift_formants_many)."""
        rs.refuse_word_pitches(kwargs, "tts_many")
        rate, level = tsm.speaking_rate(kwargs), loud.level_options(kwargs)
        pitch, sample_rate = rs.options(kwargs, rate)
        pitch_hz, formant_kw = f0m.options(kwargs, pitch, "tts_many"), f0m.formant_keywords(kwargs)
        f0_smooth = f0m.smooth_option(kwargs, pitch_hz, "tts_many")
        pauses, formants = sil.options(kwargs), fmt.options(kwargs, pitch)
        out = self._tts_many(texts, voice_samples=voice_samples, conditioning_latents=conditioning_latents,
                             use_deterministic_seed=use_deterministic_seed, verbose=verbose, **kwargs)
        if pitch_hz is not None:  # pitch_hz= (Hz): every clip's median F0 measured in ONE call, then a shift per clip through the same chain
            pitch, formants = self._pitch_hz_plan(out, pitch_hz, formant_kw, "tts_many", f0_smooth)
        return self._voiced(out, rate, pitch, level, sample_rate, pauses, formants)

    @torch.no_grad()
    def _tts_many(self, texts, voice_samples=None, conditioning_latents=None, use_deterministic_seed=None, verbose=False, **kwargs):
        """tts_many without the speaking rate."""
        if self.world != 1:
            raise ValueError("tts_many batches utterances on one GPU: build TextToSpeech(candidate_sharding=False)")
        args = inspect.signature(self.tts).bind(None, **kwargs)
        args.apply_defaults()
        if int(args.arguments["k"]) != 1:
            raise NotImplementedError("tts_many renders the top-ranked candidate of every utterance (k = 1)")
        if args.arguments["return_deterministic_state"]:
            raise NotImplementedError("tts_many: return_deterministic_state is a per-call option of tts()")
        o = self._settings(args.arguments)
        if o.noise or o.cvvp_amount != 0 or o.N > self.autoregressive_batch_size or o.N % 4 != 0:
            # what the grouped decode cannot hold: tts() renders it, one utterance at a time
            return [self.tts(t, voice_samples=voice_samples, conditioning_latents=conditioning_latents, verbose=verbose,
                             use_deterministic_seed=use_deterministic_seed, **kwargs) for t in texts]
        redacts = [self._redaction_text(t) for t in texts]
        seed = self.deterministic_state(seed=use_deterministic_seed)
        toks = [self._text_tokens(t, o.max_mel_tokens) for t in texts]
        self._redact_s = 0.0
        voice = self._voice(voice_samples, conditioning_latents)
        G = self.utterance_batch
        waves = [toks[w0:w0 + G] for w0 in range(0, len(toks), G)]

        if not self.batch_diffusion:
            # Shared decode batches, then every utterance ranked and rendered with the calls of tts().  An overflowed fp16 autoregressive
            # stage is caught right behind the decode and decoded again: nothing renders from the codes it produced.
            ev = _StageTimer(2)
            ev.mark(0)
            decoded = self._guarded(lambda: ([smp for wave in waves for smp in self._decode_wave(voice[0], wave, o, seed)], True))
            ev.mark(1)
            out, acc = [], {}
            for tokens, samples, redact in zip(toks, decoded, redacts):
                ev_u, ar = _StageTimer(6), self.ar
                ev_u.mark(0)
                # (an overflow in this utterance's latent re-pass rebuilds the stage: its codes are then decoded again, as in tts())
                clip = self._guarded(lambda: self._utterance(ev_u, tokens, voice, o, seed, 1, samples if self.ar is ar else None,
                                                             keep_on_device=redact is not None))[0]
                out.append(clip if redact is None else self._redact_clips({0: clip}, redact)[0])
                for key, v in _event_timings(ev_u).items():
                    acc[key] = acc.get(key, 0.0) + v
            ev.synchronize()
            acc["ar_s"] = acc.get("ar_s", 0.0) + ev.seconds(0, 1)
            acc["total_s"] = acc.get("total_s", 0.0) + ev.seconds(0, 1)
            if any(r is not None for r in redacts):
                acc["redact_s"] = self._redact_s
            self.timings = acc
            return out

        def lap(clock, key, t0):
            _StageTimer.synchronize()
            t1 = time.perf_counter()
            clock[key] += t1 - t0
            return t1

        def attempt():
            clock = dict.fromkeys(("ar_s", "clvp_s", "latents_s", "diffusion_s", "vocoder_s"), 0.0)  # host-clock stage sums
            t_all = time.perf_counter()
            out, ok = [], True
            for wave in waves:
                t0 = time.perf_counter()
                samples = self._decode_wave(voice[0], wave, o, seed)
                t0 = lap(clock, "ar_s", t0)
                # CLVP ranking of the whole wave in ONE speech-tower pass (api.py:460-477 per utterance; read.py:66-71 one call per chunk)
                best = self._rank(wave, samples, 1, grouped=True)
                items, zs = zip(*[self._winner_inputs(b[0], self.ar.latents(voice[0], t, b), voice[1], o, seed, 0) for t, b in zip(wave, best)])
                t0 = lap(clock, "clvp_s", t0)
                wavs, wave_ok = self._render_wave(o.solver if o.solver is not None else o.sched, items, zs)
                clock["diffusion_s"] += time.perf_counter() - t0
                out += wavs
                ok = ok and wave_ok
            return (out, clock, t_all), ok

        out, clock, t_all = self._guarded(attempt)
        out = [w if r is None else self._redact_clips({0: w}, r)[0] for w, r in zip(out, redacts)]  # (after the guards accepted the waves)
        self.timings = dict(clock, total_s=time.perf_counter() - t_all)
        if any(r is not None for r in redacts):
            self.timings["redact_s"] = self._redact_s
        return out

    # ------------------------------------------------------------------ phases of tts() / tts_many()
    def _settings(self, args):
        """tts()'s generation arguments (`args`: its parameters by name), validated -> what the phases read."""
        hf = dict(args["hf_generate_kwargs"])
        noise = hf.pop("noise_override", None) or {}
        speaking_rate, level = tsm.speaking_rate(hf), loud.level_options(hf)
        pitch, sample_rate = rs.options(hf, speaking_rate)
        pitch_hz, formant_kw = f0m.options(hf, pitch), f0m.formant_keywords(hf)
        f0_smooth = f0m.smooth_option(hf, pitch_hz)
        pauses, formants = sil.options(hf), fmt.options(hf, pitch)
        plan = fastsolver.sampler_options(hf, args["diffusion_iterations"], self.diff_cfg.trained_steps, args["cond_free"], args["cond_free_k"])
        top_k, typical_mass = sampler_kwargs(hf)
        if not 0 <= args["cvvp_amount"] <= 1:
            raise ValueError(f"cvvp_amount={args['cvvp_amount']} must lie in [0, 1] (api.py:366-367)")
        return types.SimpleNamespace(
            N=int(args["num_autoregressive_samples"]), max_mel_tokens=args["max_mel_tokens"], cvvp_amount=args["cvvp_amount"], noise=noise,
            sampling=dict(temperature=args["temperature"], top_p=args["top_p"], repetition_penalty=args["repetition_penalty"], top_k=top_k,
                          typical_mass=typical_mass),
            sched=Schedule(args["diffusion_iterations"], self.diff_cfg.trained_steps, args["cond_free"], args["cond_free_k"]),
            solver=plan,  # None: the reference's p sampler over `sched`; a solver.SolverPlan: that solver instead (no step noise)
            diffusion_temperature=args["diffusion_temperature"], speaking_rate=speaking_rate, level=level, pitch=pitch, sample_rate=sample_rate, pauses=pauses, formants=formants,
            pitch_hz=pitch_hz, formant_kw=formant_kw, f0_smooth=f0_smooth)

    def _voice(self, voice_samples, conditioning_latents, mels=False):
        """api.py:393-399 -> (auto_latent, diffusion_latent) f32 on the device, and for mels=True the voice clips' mels (what CVVP compares
        the candidates with; None for a voice given as latents)."""
        auto_conds = None
        if voice_samples is None:
            auto, diff = conditioning_latents if conditioning_latents is not None else self.get_random_conditioning_latents()
        elif mels:
            auto, diff, auto_conds, _ = self.get_conditioning_latents(voice_samples, return_mels=True)
        else:
            auto, diff = self.get_conditioning_latents(voice_samples)
        return auto.to(self.device).float(), diff.to(self.device).float(), auto_conds

    def _decode(self, auto, tokens, o, seed):
        """This rank's share of one utterance's candidates (api.py:407-427) in autoregressive_batch_size batches -> codes [n, max_mel_tokens]."""
        lo, hi = tdist.shard_range(o.N, self.rank, self.world)
        exp_noise = o.noise.get("exp_noise")
        batches = []
        for c0 in range(lo, hi, self.autoregressive_batch_size):
            B = min(self.autoregressive_batch_size, hi - c0)
            self.ar.prefill(auto, tokens)
            en = exp_noise[:, c0 - lo:c0 - lo + B] if exp_noise is not None else None
            codes, _ = self.ar.generate(B, o.max_mel_tokens, seed=seed, row_offset=c0, exp_noise=en, **o.sampling)
            batches.append(F.pad(codes, (0, o.max_mel_tokens - codes.shape[1]), value=self.ar_cfg.stop_mel_token))  # api.py:425-426
        return torch.cat(batches, dim=0)

    def _decode_wave(self, auto, toks, o, seed):
        """One shared decode batch for the utterances `toks` -> their candidates' codes [N, max_mel_tokens], one tensor per utterance."""
        for g, tokens in enumerate(toks):
            self.ar.prefill_group(g, len(toks), auto, tokens)
        codes, _ = self.ar.generate(o.N * len(toks), o.max_mel_tokens, seed=seed, row_offset=0, group_seeds=[seed] * len(toks), **o.sampling)
        return list(F.pad(codes, (0, o.max_mel_tokens - codes.shape[1]), value=self.ar_cfg.stop_mel_token).split(o.N))

    def _rank(self, toks, samples, k, auto_conds=None, cvvp_amount=0.0, grouped=False):
        """api.py:447-477: every utterance's fixed candidates scored by CLVP (score() each, or ONE score_groups() pass for a wave), blended with
        CVVP when there are clips and cvvp_amount > 0, gathered over the ranks -> the k winners' codes per utterance.  Sets last_best_codes."""
        stop = self.ar_cfg.stop_mel_token
        fixed = [fix_autoregressive_output(smp, stop) for smp in samples]
        if grouped:
            scores = self.clvp.score_groups(toks, torch.cat(fixed, dim=0)).split(fixed[0].shape[0])
        else:  # api.py:462-472: CLVP unless cvvp_amount == 1
            scores = [self.clvp.score(tokens, fx) if cvvp_amount != 1 else None for tokens, fx in zip(toks, fixed)]
        best = []
        for sc, fx in zip(scores, fixed):
            if auto_conds is not None and cvvp_amount > 0:
                cvvp = self.cvvp.score(auto_conds, fx)
                sc = cvvp if cvvp_amount == 1 else cvvp * cvvp_amount + sc * (1 - cvvp_amount)
            codes = fx.to(torch.int32)
            if self.world > 1:
                sc, codes = tdist.gather_candidates(sc, codes)
            best.append(codes[tdist.topk_lowest_index(sc, k)].long())
        self.last_best_codes = best[-1]  # the k ranked winners' codes (tests, sharding checks)
        return best

    def _winner_inputs(self, codes, latents, cond, o, seed, i):
        """Winner i (codes [n], re-passed latents [1, n, D]) -> diffusion item (latents cut at the calm run, cond, S, x_T, step_noise) and
        vocoder noise z, drawn in that order from seed + 7919 * (i + 1) unless noise_override supplies them (api.py:122, 547-556).  With a
        solver (o.solver) there is no step noise: x_T, then z, are drawn, nothing is allocated for the steps and a supplied step_noise is
        ignored - so z differs from a p sampler's run at the same seed."""
        dev = self.device
        latents = latents[:, :calm_trim_length(codes)]
        S = latents.shape[1] * 4 * 24000 // 22050
        gen = torch.Generator(device=dev).manual_seed(seed + 7919 * (i + 1))
        x_T, step_noise, z = (o.noise.get(key) for key in ("x_T", "step_noise", "z"))
        x_T = (torch.randn(1, 100, S, device=dev, generator=gen) if x_T is None else x_T.to(dev)) * o.diffusion_temperature
        if o.solver is not None:
            step_noise = None
        elif step_noise is None:
            step_noise = torch.randn(o.sched.num_timesteps, 1, 100, S, device=dev, generator=gen)
        z = torch.randn(1, self.voc_cfg.noise_dim, S + 10, device=dev, generator=gen) if z is None else z.to(dev)
        return (latents, cond, S, x_T, step_noise), z

    def _diffuse(self, sched, item, split=False):
        """Diffusion item -> mel (sched: the p sampler's Schedule or a solver's SolverPlan).  split: ranks 0 and 1 evaluate denoiser row 0 / 1 of every step; rank 1 only lends its GPU and gets None."""
        latents, cond, S, x_T, step_noise = item
        self.diffusion.condition(latents, cond, S)
        if isinstance(sched, fastsolver.SolverPlan):  # (never split: _utterance)
            return self.diffusion.solve(sched, x_T)
        if not split:
            return self.diffusion.sample(sched, x_T, step_noise)
        mel = self.diffusion.sample_split(sched, x_T, step_noise, self.rank, tdist.exchange_rows)
        return mel if self.rank == 0 else None

    def _utterance(self, ev, tokens, voice, o, seed, k, samples=None, keep_on_device=False):
        """One utterance: this rank's candidates (decoded unless given), ranking, the winners' latent re-pass (api.py:516-524) and the winners
        this rank renders (round-robin; a single conditioning-free winner split over ranks 0 and 1), marking `ev` 1-5 between the phases.
        keep_on_device: the clips stay on the device (tts() redacts them there once the utterance is accepted, api.py:583-587).
        -> ({winner index: clip on the CPU (or the device)}, every clip finite)."""
        auto, diff, auto_conds = voice
        if samples is None:
            samples = self._decode(auto, tokens, o, seed)
        ev.mark(1)
        best = self._rank([tokens], [samples], k, auto_conds, o.cvvp_amount)[0]
        ev.mark(2)
        best_latents = self.ar.latents(auto, tokens, best)
        ev.mark(3)
        split = self.split_diffusion and k == 1 and bool(o.sched.cond_free) and o.solver is None  # (a solver's winner renders unsplit on rank 0)
        plan = o.solver if o.solver is not None else o.sched
        wavs, ok = {}, True
        mine = [i for i in range(k) if not ((self.rank > 1) if split else (i % self.world != self.rank))]
        if self.winner_batch >= 2 and len(mine) >= 2:  # (one winner on this rank, the k = 1 split tail included: the single path below)
            return self._render_winners(ev, mine, best, best_latents, diff, o, seed, keep_on_device)
        for i in mine:
            item, z = self._winner_inputs(best[i], best_latents[i:i + 1], diff, o, seed, i)
            mel = self._diffuse(plan, item, split)
            if mel is None:
                continue
            ev.mark(4)
            audio = self.vocoder.inference(mel, z)
            finite = torch.isfinite(audio).all()  # (a NaN survives the final clamp: the vocoder stage's overflow check)
            wavs[i] = audio if keep_on_device else audio.cpu()
            ok = ok and bool(finite)
        if not wavs:  # this rank had no winner to render
            ev.mark(4)
        ev.mark(5)
        return wavs, ok

    def _render_winners(self, ev, mine, best, best_latents, diff, o, seed, keep_on_device):
        """The winners `mine` of one utterance in groups of up to winner_batch: per group ONE shared, padded sample_many pass in length
        order and ONE inference_many call.  Per winner nothing changes: its noise comes from seed + 7919 * (i + 1) in the same order, its
        length from its own calm-token trim.  Marks `ev` 4 after the last denoiser pass and 5 after the vocoder -> ({winner: clip}, all finite)."""
        W = self.winner_batch
        wavs, ok, pending = {}, True, []
        for g0 in range(0, len(mine), W):
            grp = mine[g0:g0 + W]
            items, zs = zip(*[self._winner_inputs(best[i], best_latents[i:i + 1], diff, o, seed, i) for i in grp])
            pending.append((grp, self._diffuse_many(o.solver if o.solver is not None else o.sched, items), zs))
        ev.mark(4)
        for grp, mels, zs in pending:
            for i, audio in zip(grp, self._vocode_many(mels, zs)):
                finite = torch.isfinite(audio).all()  # (a NaN survives the final clamp: the vocoder stage's overflow check)
                wavs[i] = audio if keep_on_device else audio.cpu()
                ok = ok and bool(finite)
        ev.mark(5)
        return wavs, ok

    def _diffuse_many(self, sched, items):
        """Diffusion items -> their mels in order: one item alone, several in ONE shared, padded sample_many pass in length order."""
        if len(items) == 1:
            return [self._diffuse(sched, items[0])]
        order = sorted(range(len(items)), key=lambda u: items[u][2])
        mels = [None] * len(items)
        many = self.diffusion.solve_many if isinstance(sched, fastsolver.SolverPlan) else self.diffusion.sample_many
        for u, mel in zip(order, many(sched, [items[u] for u in order])):
            mels[u] = mel
        return mels

    def _vocode_many(self, mels, zs):
        """UnivNet over several (mel, z): ONE inference_many call when the vocoder stage has it (every clip the bits of inference() alone,
        csrc/vocoder.hip), inference() per clip otherwise."""
        many = getattr(self.vocoder, "inference_many", None)
        if many is not None and len(mels) > 1:
            return many(list(zip(mels, zs)))
        return [self.vocoder.inference(mel, z) for mel, z in zip(mels, zs)]

    def _render_wave(self, sched, items, zs):
        """A wave's winners -> (clips on the CPU, all finite): ONE shared, padded sample_many pass in length order, then ONE UnivNet call."""
        wavs = [w.cpu() for w in self._vocode_many(self._diffuse_many(sched, items), zs)]
        return wavs, all(bool(torch.isfinite(w).all()) for w in wavs)

    def _guarded(self, attempt):
        """Runs attempt() -> (result, wav_ok) until no overflow guard trips, rebuilding the stage at fault with bf16 operands in between.
        Each fp16 stage demotes once and a tripped bf16 stage raises OperandOverflow, so the loop ends."""
        while True:
            result, wav_ok = attempt()
            _StageTimer.synchronize()
            tripped = self._tripped_stages(wav_ok)
            if not tripped:
                return result
            self._demote(tripped)


def _event_timings(ev):
    """Stage seconds of one utterance from its six _StageTimer events."""
    return {"ar_s": ev.seconds(0, 1), "clvp_s": ev.seconds(1, 2), "latents_s": ev.seconds(2, 3), "diffusion_s": ev.seconds(3, 4),
            "vocoder_s": ev.seconds(4, 5), "total_s": ev.seconds(0, 5)}
