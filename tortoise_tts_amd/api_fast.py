"""Drop-in for tortoise.api_fast.TextToSpeech on the MI355X engine: the streaming / low-latency path
(reference tortoise/api_fast.py:180-540).

One autoregressive sample, no CLVP, no diffusion, no UnivNet: GPT latents go straight into the HiFi-GAN decoder
(hifigan_decoder.py:159-294).  The engine pieces are the AR stage of the main path (prefill, hipGraph decode loop,
teacher-forced latent re-pass) and csrc/hifigan.hip.

  * tts(text, ...)          api_fast.py:421-519: inference_speech (1 sequence) -> autoregressive(..., return_latent=True)
                            -> hifi_decoder.inference(latents, auto_conditioning).  Returns wav f32 [1, 1, S] on the CPU.
  * tts_stream(text, ...)   api_fast.py:311-420: a generator of waveform chunks.  The reference pulls (token, latent) pairs out
                            of HF's sampling loop and, every `stream_chunk_size` tokens (first chunk: 60), decodes ALL latents so
                            far and cross-fades the new part in (handle_chunks).  Here the decode loop is resumed chunk by chunk
                            on the device (tt_ar_generate_chunk) and every decode step files its own latent
                            (tt_ar_stream_latents), as the reference's loop does.  Those per-step states equal one teacher-forced
                            pass over the codes - plain mel positions with kv_cache=False (the default), the cached decode's
                            0, 2, 3, ... with kv_cache=True (autoregressive.py:134-149; oracle.ar_latents(stream_positions=True),
                            pinned live against the reference's sample_stream) - which the tests use as the check.
  * handle_chunks           api_fast.py:275-309, restated (host-side tensor slicing / cross-fade).
  * max_streams = 2 .. 4    (engine-only; 2 .. 16 with wide_sessions=True) several streaming sessions share one decode batch:
                            open_stream() admits a session at any time, stream_pieces() yields (session id, wav_chunk, done) with every session on exactly the piece schedule
                            of tts_stream, tts_stream_many() wraps the two.  The AR handle is a session handle (TT_AR_OPT_SESSIONS):
                            one row per session, each with its own state on the device, all advanced by one captured decode step.
                            per_session_sampling=True lets every session keep its own sampling settings (TT_AR_OPT_SESSION_SAMPLING).

Sampling noise comes from the engine's Philox streams keyed by use_deterministic_seed (seeds are not portable between
generators: parity is "same latents -> same waveform", tests/test_gpu_stages.py::test_hifigan_decoder).
"""
import inspect
from dataclasses import dataclass
from typing import Any

import torch

from . import denoise as nr
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
from .api import MODELS_DIR, _Common, _load_state_dict, _load_file, sampler_kwargs
from .config import ARConfig, HifiganConfig


@dataclass
class _Session:
    """One streaming session of a max_streams > 1 instance: its row on the AR handle and the state of tts_stream's loop."""
    sid: int
    slot: int
    cond: Any
    text_tokens: Any
    max_mel_tokens: int
    chunk: int
    stream_chunk_size: int
    overlap: int
    target: int           # token count at which the next piece is due
    n: int = 0            # tokens sampled so far
    emitted: int = 0
    threshold: int = 0
    wav_gen_prev: Any = None
    wav_overlap: Any = None
    rs_slot: Any = None   # stream_sample_rate=: the session's slot on the streaming resampler
    ts_slot: Any = None   # stream_speaking_rate= / stream_pitch=: its slot on the streaming time-stretch
    pitch_slot: Any = None  # stream_pitch=: its slot on the pitch resampler behind the time-stretch
    level_slot: Any = None  # stream_loudness= / stream_gain=: its slot on the streaming leveler, in front of the rate resampler


class TextToSpeech(_Common):
    """api_fast.py:180-229.  Engine-only keyword arguments as in tortoise_tts_amd.api.TextToSpeech: state_dicts
    ('autoregressive', 'hifidecoder', 'rlg_auto'), dtype, configs ('ar', 'hifigan'), max_mel_tokens, and max_streams (1 .. 4):
    streaming sessions served from one shared decode batch (open_stream / stream_pieces / tts_stream_many); 1 keeps the
    single-sequence engine of tts() / tts_stream(); wide_sessions=True allows max_streams = 2 .. 16 (a wide session handle).
    per_session_sampling=True (max_streams > 1): each session samples with the settings it was opened with, whatever the other
    sessions use (else they must all match)."""

    def __init__(self, autoregressive_batch_size=None, models_dir=MODELS_DIR, enable_redaction=True, kv_cache=False,
                 use_deepspeed=False, half=False, device=None, tokenizer_vocab_file=None, tokenizer_basic=False, *,
                 state_dicts=None, dtype=None, configs=None, max_mel_tokens=500, max_text_tokens=402, max_streams=1,
                 per_session_sampling=False, wide_sessions=False, mel_front_end="torch", aligner=None, denoise_voice_samples=None):
        nr.from_option(denoise_voice_samples)  # (validated now, used by get_conditioning_latents)
        self.denoise_voice_samples = denoise_voice_samples
        self.models_dir = models_dir
        self._aligner_source = aligner  # align() / tts_with_timings(): the wav2vec2 aligner's (config, state_dict, vocab, tokenizer config) instead of its files
        self.mel_front_end_kind = stages.mel_front_end_kind(mel_front_end)
        if use_deepspeed:
            raise NotImplementedError("use_deepspeed: DeepSpeed kernel injection is a CUDA-only reference option")
        self.enable_redaction = bool(enable_redaction)
        self.kv_cache = bool(kv_cache)
        self.half = bool(half)
        self.device = E.require_gpu(device)
        if dtype is None:
            dtype = "fp16" if half else "bf16"
        elif half and dtype not in ("fp16", "f16"):
            raise ValueError(f"half=True asks for fp16 operands but dtype={dtype!r} was also given")
        self.dtype = {"bf16": E.TT_BF16, "fp16": E.TT_F16, "f16": E.TT_F16}[dtype]
        cfgs = configs or {}
        self.ar_cfg = cfgs.get("ar", ARConfig())
        self.hifi_cfg = cfgs.get("hifigan", HifiganConfig())
        self._state_dicts = state_dicts or {}
        self.autoregressive_batch_size = 1
        self.tokenizer_args = (tokenizer_vocab_file, tokenizer_basic)
        self._tokenizer = None
        self.max_mel_tokens_cap = max_mel_tokens
        self.wide_sessions = bool(wide_sessions)
        if self.wide_sessions and not 2 <= int(max_streams) <= 16:
            raise ValueError(f"max_streams={max_streams} outside 2 .. 16 (the sessions of one wide decode batch, wide_sessions=True)")
        if not self.wide_sessions and not 1 <= int(max_streams) <= 4:
            raise ValueError(f"max_streams={max_streams} outside 1 .. 4 (the sessions of one decode batch; up to 16 with wide_sessions=True)")
        self.max_streams = int(max_streams)
        self.per_session_sampling = bool(per_session_sampling)
        if self.per_session_sampling and self.max_streams == 1:
            raise ValueError("per_session_sampling=True needs max_streams=2 .. 4 (a single stream has its settings per call)")
        if self.max_streams == 1:
            self.ar = stages.ArStage(self._sd("autoregressive"), self.ar_cfg, self.device, self.dtype, max_batch=1, max_text=max_text_tokens,
                                     max_new_tokens=max_mel_tokens, max_latent_candidates=1, kv_cache=self.kv_cache)
        else:
            own = {"per_session_sampling": True} if self.per_session_sampling else {}
            self.ar = stages.ArStage(self._sd("autoregressive"), self.ar_cfg, self.device, self.dtype, max_batch=self.max_streams,
                                     max_text=max_text_tokens, max_new_tokens=max_mel_tokens, max_latent_candidates=1, kv_cache=self.kv_cache,
                                     sessions=True, **own)
        self._sessions = {}      # slot -> _Session
        self._session_settings = None
        self._next_sid = 0
        hsd = self._sd("hifidecoder")
        if any(k.endswith("weight_v") for k in hsd):
            hsd = W.fold_weight_norm(hsd)
        self.hifi_decoder = stages.HifiganStage(hsd, self.hifi_cfg, self.device, self.dtype, max_latents=max_mel_tokens + 8)
        self.rlg_auto = None
        self.conditioning = None
        self.mel_front_end = None
        self.stream_latents_from = "steps"
        self.stop_mel_token = self.ar_cfg.stop_mel_token
        self.mel_length_compression = self.ar_cfg.mel_length_compression

    def _sd(self, name):
        if name in self._state_dicts:
            return self._state_dicts[name]
        if name == "hifidecoder":
            return _load_file(self.models_dir, "hifidecoder.pth")
        return _load_state_dict(self.models_dir, name)

    # ------------------------------------------------------------------ conditioning (api_fast.py:230-260)
    def get_conditioning_latents(self, voice_samples, return_mels=False, denoise=nr.INHERIT):
        """Only the autoregressive latent exists on this path (there is no diffusion stage).  voice_samples: 22.05 kHz clips
        or ready auto mels f32 [1, 80, T] (see tortoise_tts_amd.api.TextToSpeech.get_conditioning_latents, also for denoise=)."""
        if torch.is_tensor(voice_samples):
            voice_samples = [voice_samples]
        if self.conditioning is None:
            self.conditioning = stages.ConditioningStage(self._sd("autoregressive"), None, self.ar_cfg, None, self.device, self.dtype)
        def ready(vs):
            return torch.is_tensor(vs) and vs.dim() >= 2 and vs.shape[-2] == 80
        voice_samples = self._clean_voice_samples(voice_samples, denoise, ready)

        mels = []
        device_mels = None
        if self.mel_front_end_kind == "device":  # every waveform entry in one ragged call (stages.MelFrontStage; no diffusion mel here)
            waves = [vs for vs in voice_samples if not ready(vs)]
            if waves:
                if self.mel_front_end is None:
                    self.mel_front_end = stages.MelFrontStage(self.models_dir, device=self.device)
                device_mels = iter(self.mel_front_end.auto_many(waves))
        for vs in voice_samples:
            if ready(vs):
                mels.append(vs.reshape(1, 80, vs.shape[-1]))
            elif device_mels is not None:
                mels.append(next(device_mels))
            else:
                if self.mel_front_end is None:
                    from .audio import MelFrontEnd
                    self.mel_front_end = MelFrontEnd(self.models_dir)
                mels.append(self.mel_front_end.auto_mel(vs.to(self.device)))
        return self.conditioning.auto_latent(mels)

    def get_random_conditioning_latents(self):
        if self.rlg_auto is None:
            sd = self._sd("rlg_auto")
            self.rlg_auto = stages.RandomLatentStage(sd, sd, self.device, self.dtype)
        ca = self.rlg_auto.channels[0]
        r = torch.randn(1, ca)
        return self.rlg_auto.latents(r, r)[0]

    def _prepare(self, text, voice_samples, conditioning_latents, max_mel_tokens):
        text_tokens = self._text_tokens(text, max_mel_tokens)  # (api_fast.py:371; no redaction on this path)
        if max_mel_tokens < 1:
            raise ValueError(f"max_mel_tokens={max_mel_tokens} must be at least 1")
        if voice_samples is not None:
            cond = self.get_conditioning_latents(voice_samples)
        elif conditioning_latents is not None:
            cond = conditioning_latents[0] if isinstance(conditioning_latents, (tuple, list)) else conditioning_latents
        else:
            cond = self.get_random_conditioning_latents()
        return text_tokens, cond.to(self.device).float().reshape(1, -1)

    # ------------------------------------------------------------------ non-streaming (api_fast.py:421-519)
    @torch.no_grad()
    def tts(self, text, voice_samples=None, k=1, verbose=True, use_deterministic_seed=None, conditioning_latents=None,
            num_autoregressive_samples=512, temperature=.8, length_penalty=1, repetition_penalty=2.0, top_p=.8, max_mel_tokens=500,
            cvvp_amount=.0, **hf_generate_kwargs):
        # (k and cvvp_amount are accepted and unused as in the reference: its fast path decodes ONE sample, there is nothing to rank)
        self._single("tts")
        speaking_rate, level = tsm.speaking_rate(hf_generate_kwargs), loud.level_options(hf_generate_kwargs)
        pitch, sample_rate = rs.options(hf_generate_kwargs, speaking_rate)
        pitch_hz, formant_kw = f0m.options(hf_generate_kwargs, pitch), f0m.formant_keywords(hf_generate_kwargs)
        f0_smooth = f0m.smooth_option(hf_generate_kwargs, pitch_hz)
        pauses, formants = sil.options(hf_generate_kwargs), fmt.options(hf_generate_kwargs, pitch)
        top_k, typical_mass = sampler_kwargs(hf_generate_kwargs)
        seed = self.deterministic_state(seed=use_deterministic_seed)
        text_tokens, cond = self._prepare(text, voice_samples, conditioning_latents, max_mel_tokens)
        self.ar.prefill(cond, text_tokens)
        codes, _ = self.ar.generate(1, max_mel_tokens, temperature=temperature, top_p=top_p, repetition_penalty=float(repetition_penalty),
                                    top_k=top_k, seed=seed, row_offset=0, typical_mass=typical_mass)
        self.last_codes = codes
        latents = self.ar.latents(cond, text_tokens, codes)          # api_fast.py:510-514 (return_latent=True)
        wav = self.hifi_decoder.inference(latents, cond)             # api_fast.py:517
        out = [wav.cpu()]
        if pitch_hz is not None:  # pitch_hz= (Hz): the clip's median F0 measured, then the shift that lands on it
            pitch, formants = self._pitch_hz_plan(out, pitch_hz, formant_kw, smooth=f0_smooth)
        return self._voiced(out, speaking_rate, pitch, level, sample_rate, pauses, formants)[0]  # (rate and pitch -> formants -> pauses -> level -> sample rate)

    def tts_many(self, texts, voice_samples=None, conditioning_latents=None, use_deterministic_seed=None, **kwargs):
        """Several texts, one clip each: the result equals [tts(t, ...) for t in texts] on a max_streams=1 instance started from the same
        state, clip for clip and bit for bit.  kwargs are tts()'s, shared by all texts; use_deterministic_seed is one seed or a list with
        one per text.  On a max_streams=1 instance this loops tts().  On a session instance (max_streams >= 2) the texts are decoded as
        rows of the shared decode batch - later texts take rows as earlier ones finish - each gets tts()'s latent re-pass, and the clips
        are vocoded in ragged batches (HifiganStage.inference_many).  Returns a list of wav f32 [1, 1, S] on the CPU.
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
        out = self._tts_many(texts, voice_samples, conditioning_latents, use_deterministic_seed, **kwargs)
        if pitch_hz is not None:  # pitch_hz= (Hz): every clip's median F0 measured in ONE call, then a shift per clip
            pitch, formants = self._pitch_hz_plan(out, pitch_hz, formant_kw, "tts_many", f0_smooth)
        return self._voiced(out, rate, pitch, level, sample_rate, pauses, formants)

    @torch.no_grad()
    def _tts_many(self, texts, voice_samples, conditioning_latents, use_deterministic_seed, **kwargs):
        """tts_many without the speaking rate."""
        texts = list(texts)
        seeds = use_deterministic_seed if isinstance(use_deterministic_seed, (list, tuple)) else [use_deterministic_seed] * len(texts)
        if len(seeds) != len(texts):
            raise ValueError(f"tts_many: {len(seeds)} seeds for {len(texts)} texts")
        bound = inspect.signature(TextToSpeech.tts).bind(self, "", **kwargs)  # (a TypeError for an unknown argument, before any work)
        bound.apply_defaults()
        a = bound.arguments
        if self.max_streams == 1:
            return [self.tts(t, voice_samples=voice_samples, conditioning_latents=conditioning_latents, use_deterministic_seed=sd, **kwargs)
                    for t, sd in zip(texts, seeds)]
        if self._sessions:
            raise RuntimeError(f"tts_many: {len(self._sessions)} streaming session(s) are open on this instance; finish or close them first")
        if "exp_noise" in a["hf_generate_kwargs"]:
            raise ValueError("tts_many: injected exp_noise is not available on a session instance (rows draw from their Philox streams)")
        top_k, typical_mass = sampler_kwargs(a["hf_generate_kwargs"])
        settings = dict(temperature=float(a["temperature"]), top_p=float(a["top_p"]), repetition_penalty=float(a["repetition_penalty"]),
                        top_k=int(top_k), typical_mass=float(typical_mass))
        if self.per_session_sampling:
            stages.session_sampling(**settings)  # (invalid settings raise before a row is taken)
        max_mel_tokens = int(a["max_mel_tokens"])
        if max_mel_tokens < 1:
            raise ValueError(f"max_mel_tokens={max_mel_tokens} must be at least 1")
        for t in texts:
            self._text_tokens(t, max_mel_tokens)  # (too long a text raises before a row is taken)
        rows = {}       # slot -> (index, cond, text_tokens)
        n_row = {}      # slot -> tokens that row has sampled
        clips = [None] * len(texts)
        pending = list(range(len(texts)))
        try:
            while pending or rows:
                while pending and len(rows) < self.max_streams:
                    i = pending.pop(0)
                    seed = self.deterministic_state(seed=seeds[i])  # (tts()'s order: reseed, then a random voice may be drawn)
                    text_tokens, cond = self._prepare(texts[i], voice_samples, conditioning_latents, max_mel_tokens)
                    slot = min(r for r in range(self.max_streams) if r not in rows)
                    if self.per_session_sampling:
                        self.ar.admit(slot, cond, text_tokens, seed, **settings)
                    else:
                        self.ar.admit(slot, cond, text_tokens, seed)
                    rows[slot] = (i, cond, text_tokens)
                    n_row[slot] = 0
                step = max(1, min(max_mel_tokens - n_row[r] for r in rows))
                if self.per_session_sampling:
                    n_total, finished = self.ar.advance(step)
                else:
                    n_total, finished = self.ar.advance(step, **settings)
                for slot in sorted(rows):
                    n_row[slot] = n_total[slot]
                    if not (finished[slot] or n_total[slot] >= max_mel_tokens):
                        continue
                    i, cond, text_tokens = rows.pop(slot)
                    codes = self.ar.session_codes(slot)[:, :n_total[slot]]
                    self.ar.close(slot)
                    self.last_codes = codes
                    clips[i] = (self.ar.latents(cond, text_tokens, codes), cond)  # tts()'s latent re-pass (api_fast.py:510-514)
        finally:
            for slot in rows:
                self.ar.close(slot)
        wavs = self.hifi_decoder.inference_many(clips) if hasattr(self.hifi_decoder, "inference_many") else \
            [self.hifi_decoder.inference(lat, cond) for lat, cond in clips]
        return [w.cpu() for w in wavs]

    def tts_with_preset(self, text, preset="fast", **kwargs):
        """api_fast.py:262-273: the preset table of this class only feeds kwargs to tts() (diffusion settings are unused on this
        path); a generator over the result, like the reference."""
        settings = {"temperature": .8, "length_penalty": 1.0, "repetition_penalty": 2.0, "top_p": .8}
        presets = {"ultra_fast": {"num_autoregressive_samples": 1}, "fast": {"num_autoregressive_samples": 32},
                   "standard": {"num_autoregressive_samples": 256}, "high_quality": {"num_autoregressive_samples": 256}}
        settings.update(presets[preset])
        settings.update({k_: v for k_, v in kwargs.items() if k_ not in ("cond_free_k", "diffusion_temperature", "diffusion_iterations", "cond_free")})
        for audio_frame in self.tts(text, **settings):
            yield audio_frame

    # ------------------------------------------------------------------ streaming (api_fast.py:275-420)
    @staticmethod
    def handle_chunks(wav_gen, wav_gen_prev, wav_overlap, overlap_len):
        """api_fast.py:275-309: the part of the newly decoded waveform that has not been emitted yet, cross-faded over the overlap."""
        wav_chunk = wav_gen[:-overlap_len]
        if wav_gen_prev is not None:
            wav_chunk = wav_gen[(wav_gen_prev.shape[0] - overlap_len):-overlap_len]
        if wav_overlap is not None:
            if overlap_len > len(wav_chunk):
                if wav_gen_prev is not None:
                    wav_chunk = wav_gen[(wav_gen_prev.shape[0] - overlap_len):]
                else:
                    wav_chunk = wav_gen[-overlap_len:]
                return wav_chunk, wav_gen, None
            wav_chunk = wav_chunk.clone()
            fade_in = torch.linspace(0.0, 1.0, overlap_len, device=wav_chunk.device)
            crossfade = wav_chunk[:overlap_len] * fade_in
            wav_chunk[:overlap_len] = wav_overlap * torch.linspace(1.0, 0.0, overlap_len, device=wav_overlap.device)
            wav_chunk[:overlap_len] += crossfade
        wav_overlap = wav_gen[-overlap_len:]
        return wav_chunk, wav_gen, wav_overlap

    def _stream_latents(self, cond, text_tokens, codes):
        """The latent half of the (token, latent) pairs of the reference's generator (api_fast.py:405-414): filed by the decode
        steps themselves (tt_ar_stream_latents), exactly where the reference takes them from.  `stream_latents_from="pass"` keeps
        the earlier formulation - one teacher-forced pass over the codes so far (plain positions for kv_cache=False, the cached
        decode's 0, 2, 3, ... for kv_cache=True) - which the tests hold equal to the per-step latents within the operand tolerance."""
        if self.stream_latents_from == "steps":
            return self.ar.stream_latents(1, codes.shape[1])
        return self.ar.latents(cond, text_tokens, codes, stream_positions=self.kv_cache)

    @torch.no_grad()
    def tts_stream(self, text, voice_samples=None, conditioning_latents=None, k=1, verbose=True, use_deterministic_seed=None,
                   return_deterministic_state=False, overlap_wav_len=1024, stream_chunk_size=40,
                   num_autoregressive_samples=512, temperature=.8, length_penalty=1, repetition_penalty=2.0, top_p=.8, max_mel_tokens=500,
                   cvvp_amount=.0, diffusion_iterations=100, cond_free=True, cond_free_k=2, diffusion_temperature=1.0,
                   **hf_generate_kwargs):
        self._single("tts_stream")
        tsm.refuse_streaming(hf_generate_kwargs, "tts_stream")
        tsm.refuse_word_rates(hf_generate_kwargs, "tts_stream")
        loud.refuse_streaming(hf_generate_kwargs, "tts_stream")
        rs.refuse_streaming(hf_generate_kwargs, "tts_stream")
        rs.refuse_word_pitches(hf_generate_kwargs, "tts_stream")
        f0m.refuse_streaming(hf_generate_kwargs, "tts_stream")
        sil.refuse_streaming(hf_generate_kwargs, "tts_stream")
        fmt.refuse_streaming(hf_generate_kwargs, "tts_stream")
        nr.refuse_streaming(hf_generate_kwargs, "tts_stream")
        fastsolver.refuse_streaming(hf_generate_kwargs, "tts_stream")
        stream_rate = rs.stream_options(hf_generate_kwargs)
        stream_voice = tsm.stream_options(hf_generate_kwargs)
        stream_level = loud.stream_options(hf_generate_kwargs)
        top_k, typical_mass = sampler_kwargs(hf_generate_kwargs)
        seed = self.deterministic_state(seed=use_deterministic_seed)
        text_tokens, cond = self._prepare(text, voice_samples, conditioning_latents, max_mel_tokens)
        self.ar.prefill(cond, text_tokens)
        chunk = stream_chunk_size if stream_chunk_size > 0 else max_mel_tokens
        first = max(chunk, 60) if stream_chunk_size > 0 else max_mel_tokens  # first_buffer = 60 (api_fast.py:401, 412)
        wav_gen_prev, wav_overlap = None, None
        emitted = 0          # (token, latent) pairs already decoded into an emitted chunk
        threshold = first    # pairs the reference buffers before the next decode (api_fast.py:412)
        # stream_speaking_rate= / stream_pitch= / stream_loudness= / stream_gain= / stream_sample_rate=: every piece goes through the
        # session's slots of the streaming time-stretch, the pitch resampler, the leveler and the rate resampler, in this order (the
        # whole-clip chain's: the ceiling holds at 24 kHz); the stream's last piece with flush
        chain = self._open_chain(stream_voice, stream_rate, stream_level)
        try:
            for codes, done in self.ar.generate_stream(1, max_mel_tokens, chunk, first_chunk=first, temperature=temperature, top_p=top_p,
                                                       repetition_penalty=float(repetition_penalty), top_k=top_k, seed=seed,
                                                       typical_mass=typical_mass):
                if done and codes.shape[1] > 0 and int(codes[0, -1]) == self.stop_mel_token:
                    codes = codes[:, :-1]  # the reference's generator stops BEFORE yielding the stop token's pair
                if codes.shape[1] == 0:
                    break
                self.last_codes = codes
                latents = self._stream_latents(cond, text_tokens, codes)
                wav_gen = self.hifi_decoder.inference(latents, cond).reshape(-1)
                wav_chunk, wav_gen_prev, wav_overlap = self.handle_chunks(wav_gen, wav_gen_prev, wav_overlap, overlap_wav_len)
                # The reference decodes once per filled buffer AND once more when its generator raises StopIteration
                # (api_fast.py:405-420).  When the sequence ends exactly on a buffer boundary that last pass sees the same latents
                # again and handle_chunks hands out the withheld overlap tail: mirror it.
                extra = done and stream_chunk_size > 0 and codes.shape[1] - emitted == threshold
                yield wav_chunk if chain is None else self._chain_push([(chain, wav_chunk, done and not extra)])[0]
                if done:
                    if extra:
                        wav_chunk, wav_gen_prev, wav_overlap = self.handle_chunks(wav_gen, wav_gen_prev, wav_overlap, overlap_wav_len)
                        yield wav_chunk if chain is None else self._chain_push([(chain, wav_chunk, True)])[0]
                    break
                emitted = codes.shape[1]
                threshold = chunk
        finally:
            self._close_chain(chain)

    _stream_stage = None
    _stretch_stage = None
    _pitch_stage = None
    _level_stage = None

    def _stream_lv(self):
        """The streaming leveler of stream_loudness= / stream_gain= (stages.StreamLevelStage, one slot per session), built on first use."""
        if self._level_stage is None:
            self._level_stage = stages.StreamLevelStage(self.max_streams, device=self.device)
        return self._level_stage

    def _stream_rs(self):
        """The streaming resampler of stream_sample_rate= (stages.StreamResampleStage, one slot per session), built on first use."""
        if self._stream_stage is None:
            self._stream_stage = stages.StreamResampleStage(self.max_streams, device=self.device)
        return self._stream_stage

    def _stream_ts(self):
        """The streaming time-stretch of stream_speaking_rate= / stream_pitch= (stages.StreamStretchStage, one slot per session), built on
        first use."""
        if self._stretch_stage is None:
            self._stretch_stage = stages.StreamStretchStage(self.max_streams, device=self.device)
        return self._stretch_stage

    def _stream_pitch(self):
        """The resampler behind the time-stretch of stream_pitch= (a second stages.StreamResampleStage: the first one's slots belong to
        stream_sample_rate=), built on first use."""
        if self._pitch_stage is None:
            self._pitch_stage = stages.StreamResampleStage(self.max_streams, device=self.device)
        return self._pitch_stage

    def _open_chain(self, stream_voice, stream_rate, stream_level=None):
        """The slots one stream's pieces go through: (time-stretch slot at rq_eff, pitch slot at (pq, 65536), leveler slot, rate slot), None
        where a stage is not needed - or None when none is.  stream_voice: stretch.stream_options' (rq_eff, pq); stream_level:
        loudness.stream_options' settings; stream_rate: Hz.  A rate of exactly 1 is no time-stretch and a ratio of 1 no resampling, as in
        the whole-clip calls.  An open that fails frees the others."""
        if stream_voice is None and stream_rate is None and stream_level is None:
            return None
        chain = [None, None, None, None]
        try:
            if stream_voice is not None and stream_voice[0] != E.TSM_RATE_ONE:
                chain[0] = self._stream_ts().open(stream_voice[0])
            if stream_voice is not None and stream_voice[1] != E.RS_PITCH_ONE:
                chain[1] = self._stream_pitch().open(stream_voice[1], E.RS_PITCH_ONE)
            if stream_level is not None:
                chain[2] = self._stream_lv().open(stream_level)
            if stream_rate is not None:
                chain[3] = self._stream_rs().open(*rs.ratio(rs.SAMPLE_RATE, stream_rate))
        except Exception:
            self._close_chain(tuple(chain))
            raise
        return tuple(chain) if any(c is not None for c in chain) else None

    def _close_chain(self, chain):
        for slot, stage in zip(chain or (), (self._stream_ts, self._stream_pitch, self._stream_lv, self._stream_rs)):
            if slot is not None:
                stage().close(slot)

    def _chain_push(self, items):
        """items = [(chain, piece, flush)] of distinct streams -> what each emits at the end of its chain: ONE push_many per stage for all of
        them (the time-stretch, then the pitch resampler, then the leveler, then the rate resampler; a stream without a slot on a stage passes
        it by)."""
        pieces = [x for _, x, _ in items]
        for which, stage in enumerate((self._stream_ts, self._stream_pitch, self._stream_lv, self._stream_rs)):
            todo = [i for i, (chain, _, _) in enumerate(items) if chain[which] is not None]
            if todo:
                for i, y in zip(todo, stage().push_many([(items[i][0][which], pieces[i], items[i][2]) for i in todo])):
                    pieces[i] = y
        return pieces

    @staticmethod
    def _chain_of(sess):
        chain = (sess.ts_slot, sess.pitch_slot, sess.level_slot, sess.rs_slot)
        return chain if any(c is not None for c in chain) else None

    # ------------------------------------------------------------------ several streams in one decode batch (max_streams > 1)
    def _single(self, name):
        if getattr(self, "max_streams", 1) != 1:
            raise NotImplementedError(f"{name}: this instance serves streaming sessions (max_streams={self.max_streams}); use open_stream / "
                                      f"stream_pieces / tts_stream_many, or an instance with max_streams=1")

    @torch.no_grad()
    def open_stream(self, text, voice_samples=None, conditioning_latents=None, use_deterministic_seed=None, **kwargs):
        """Admit one streaming session (max_streams > 1) and return its id.  Takes tts_stream's arguments; the session's pieces come out
        of stream_pieces() on exactly tts_stream's schedule.  May be called at any time, also between pieces of other sessions.  Raises
        when every slot is busy or when the sampling settings differ from those of the running sessions (they share one sampler) -
        with per_session_sampling any valid settings are taken, and invalid ones raise ValueError before a slot is taken.
        stream_sample_rate=R (also on tts_stream): the session's pieces come at R Hz instead of 24 kHz - the same number of pieces with
        the same done flags, each holding the samples that became ready (possibly none), through one slot of the streaming resampler
        (stages.StreamResampleStage; all pieces due in a round of stream_pieces in ONE push).  Their concatenation is bit for bit
        resample() of the 24 kHz stream; the audio lags by resample.stream_latency input samples (1.5 ms; 4.5 ms to 8 kHz) until the
        last piece flushes it.  None or 24000: nothing is built, today's bits.
        stream_speaking_rate=r (0.5 .. 2.0) and stream_pitch=s (semitones, +-12), also on tts_stream: the session's pieces at another
        speaking rate and pitch, validated as speaking_rate= and pitch= of tts() are - through one slot of the streaming time-stretch
        (stages.StreamStretchStage) at rate r / 2^(s/12) and, for a pitch, one slot of a second streaming resampler at 2^(s/12), in front
        of the stream_sample_rate slot; every stage is ONE push per round of stream_pieces.  The concatenation is bit for bit the
        whole-clip chain (stretch / shift_pitch, then resample) of the 24 kHz stream; the audio lags by 1407 samples (58.6 ms) until the
        last piece flushes it, so early pieces may be short or empty.  None, 1.0 and 0: nothing is built, today's bits.
        stream_loudness=T (LUFS, -70 .. -5) or stream_gain=dB, also on tts_stream: the session's pieces through one slot of the streaming
        leveler (stages.StreamLevelStage) behind the pitch slot and in front of the stream_sample_rate slot - towards T with a
        slew-limited gain steered by the loudness of what the session has said so far, or at a fixed gain; stream_true_peak= (dBTP,
        default -1 with a target) keeps a ceiling with the 5 ms look-ahead limiter (the audio lags by 248 samples, 10.3 ms, until the last
        piece), stream_limit='lookahead' | 'none', stream_level=dict(assume=, boost=, cut=, rise=, fall=) (loudness.STREAM_LEVEL_DEFAULTS).
        The concatenation is bit for bit level() of the stream without the keywords.  None of them: nothing is built, today's bits.
        loudness=, true_peak= and limit= stay refused: an integrated loudness needs the whole clip."""
        tsm.refuse_streaming(kwargs, "open_stream")
        tsm.refuse_word_rates(kwargs, "open_stream")
        loud.refuse_streaming(kwargs, "open_stream")
        rs.refuse_streaming(kwargs, "open_stream")
        rs.refuse_word_pitches(kwargs, "open_stream")
        f0m.refuse_streaming(kwargs, "open_stream")
        sil.refuse_streaming(kwargs, "open_stream")
        fmt.refuse_streaming(kwargs, "open_stream")
        nr.refuse_streaming(kwargs, "open_stream")
        fastsolver.refuse_streaming(kwargs, "open_stream")
        stream_rate = rs.stream_options(kwargs)  # (validated before a slot is taken)
        stream_voice = tsm.stream_options(kwargs)
        stream_level = loud.stream_options(kwargs)
        if self.max_streams == 1:
            raise NotImplementedError("open_stream: create the instance with max_streams=2 .. 4")
        if "exp_noise" in kwargs:
            raise ValueError("open_stream: injected exp_noise is not available for streaming sessions (they draw from their Philox streams)")
        bound = inspect.signature(TextToSpeech.tts_stream).bind(self, text, **kwargs)
        bound.apply_defaults()
        a = bound.arguments
        top_k, typical_mass = sampler_kwargs(a["hf_generate_kwargs"])
        settings = (float(a["temperature"]), float(a["top_p"]), float(a["repetition_penalty"]), int(top_k), float(typical_mass))
        if self.per_session_sampling:
            try:
                stages.session_sampling(*settings)
            except ValueError as err:
                raise ValueError(f"open_stream: {err}") from None
        free = [r for r in range(self.max_streams) if r not in self._sessions]
        if not free:
            raise RuntimeError(f"open_stream: all {self.max_streams} streaming slots are busy")
        if not self.per_session_sampling and self._sessions and settings != self._session_settings:
            raise ValueError(f"open_stream: sampling settings {settings} differ from those of the running sessions {self._session_settings} "
                             f"(temperature, top_p, repetition_penalty, top_k, typical_mass)")
        max_mel_tokens = a["max_mel_tokens"]
        seed = self.deterministic_state(seed=use_deterministic_seed)
        text_tokens, cond = self._prepare(text, voice_samples, conditioning_latents, max_mel_tokens)
        slot = free[0]
        chain = self._open_chain(stream_voice, stream_rate, stream_level)  # (before the row is taken: a refusal here leaves no session behind)
        try:
            if self.per_session_sampling:
                self.ar.admit(slot, cond, text_tokens, seed, **dict(zip(("temperature", "top_p", "repetition_penalty", "top_k", "typical_mass"), settings)))
            else:
                self.ar.admit(slot, cond, text_tokens, seed)
        except Exception:
            self._close_chain(chain)
            raise
        size = a["stream_chunk_size"]
        chunk = size if size > 0 else max_mel_tokens
        first = max(chunk, 60) if size > 0 else max_mel_tokens  # first_buffer = 60 (api_fast.py:401, 412)
        sess = _Session(self._next_sid, slot, cond, text_tokens, max_mel_tokens, chunk, size, a["overlap_wav_len"], min(first, max_mel_tokens),
                        threshold=first)
        if chain is not None:
            sess.ts_slot, sess.pitch_slot, sess.level_slot, sess.rs_slot = chain
        self._next_sid += 1
        self._sessions[slot] = sess
        self._session_settings = settings
        return sess.sid

    def close_stream(self, sid):
        """Retire session `sid` before it ends (a client that went away): its row stops decoding and is free for the next open_stream.
        The other sessions are untouched.  Raises KeyError for an id that is not open."""
        for slot, sess in self._sessions.items():
            if sess.sid == sid:
                del self._sessions[slot]
                self.ar.close(slot)
                self._close_rs(sess)
                return
        raise KeyError(f"close_stream: no open session {sid}")

    def _close_rs(self, sess):
        """Frees every slot of the session's chain."""
        self._close_chain(self._chain_of(sess))
        sess.ts_slot = sess.pitch_slot = sess.level_slot = sess.rs_slot = None

    def _resample_due(self, due, vocoded):
        """stream_speaking_rate= / stream_pitch= / stream_sample_rate=: the pieces of this round's sessions that have a chain, all of them
        through ONE push_many per stage (a session's extra last piece in a second one): slot -> [(chunk at the end of the session's
        chain, done)].  The last piece of a session is pushed with flush.  {} when no session of the round has a chain."""
        pieces = {slot: self._session_piece(sess, n, fin, vocoded.get(slot)) for slot, sess, n, fin in due if self._chain_of(sess) is not None}
        if not pieces:
            return {}
        chains = {slot: self._chain_of(sess) for slot, sess, _, _ in due}
        out = {slot: [] for slot in pieces}
        for k in range(max(len(p) for p in pieces.values())):
            todo = [slot for slot, p in pieces.items() if len(p) > k]
            res = self._chain_push([(chains[slot], pieces[slot][k][0], pieces[slot][k][1]) for slot in todo])
            for slot, y in zip(todo, res):
                out[slot].append((y, pieces[slot][k][1]))
        return out

    def _session_latents(self, sess, n, finished):
        """The first half of tts_stream's loop body for a session whose token count reached its piece boundary (or its end):
        (latents to vocode, or None when there is nothing to decode; done; tokens they cover)."""
        codes = self.ar.session_codes(sess.slot)[:, :n]
        done = finished or n >= sess.max_mel_tokens
        if done and codes.shape[1] > 0 and int(codes[0, -1]) == self.stop_mel_token:
            codes = codes[:, :-1]
        if codes.shape[1] == 0:
            return None, done, 0
        self.last_codes = codes
        if self.stream_latents_from == "steps":
            return self.ar.session_latents(sess.slot, codes.shape[1]), done, codes.shape[1]
        return self.ar.latents(sess.cond, sess.text_tokens, codes, stream_positions=self.kv_cache), done, codes.shape[1]

    def _session_piece(self, sess, n, finished, vocoded=None):
        """tts_stream's loop body for one session whose token count reached its piece boundary (or its end): the wav chunks it yields.
        vocoded: (wav_gen or None, done, tokens) when the caller has vocoded the session already (stream_pieces' batched call)."""
        if vocoded is None:
            latents, done, n_codes = self._session_latents(sess, n, finished)
            wav_gen = None if latents is None else self.hifi_decoder.inference(latents, sess.cond).reshape(-1)
        else:
            wav_gen, done, n_codes = vocoded
        if wav_gen is None:  # (tts_stream yields nothing at all; the session still reports its end)
            return [(torch.zeros(0, device=self.device), True)]
        wav_chunk, sess.wav_gen_prev, sess.wav_overlap = self.handle_chunks(wav_gen, sess.wav_gen_prev, sess.wav_overlap, sess.overlap)
        if not done:
            sess.emitted, sess.threshold = n_codes, sess.chunk
            sess.target = min(n + sess.chunk, sess.max_mel_tokens)
            return [(wav_chunk, False)]
        if sess.stream_chunk_size > 0 and n_codes - sess.emitted == sess.threshold:  # the extra piece (see tts_stream)
            last, sess.wav_gen_prev, sess.wav_overlap = self.handle_chunks(wav_gen, sess.wav_gen_prev, sess.wav_overlap, sess.overlap)
            return [(wav_chunk, False), (last, True)]
        return [(wav_chunk, True)]

    def _vocode_due(self, due):
        """One batched vocoder call (HifiganStage.inference_many) for the sessions of this round whose piece is due: slot -> (wav_gen or
        None, done, tokens).  {} for a stage without inference_many: those sessions are vocoded one at a time at their turn."""
        if not hasattr(self.hifi_decoder, "inference_many"):
            return {}
        prep = {slot: self._session_latents(sess, n, fin) for slot, sess, n, fin in due}
        todo = [(slot, lat, sess.cond) for slot, sess, _, _ in due for lat in [prep[slot][0]] if lat is not None]
        wavs = self.hifi_decoder.inference_many([(lat, cond) for _, lat, cond in todo]) if todo else []
        out = {slot: (None,) + prep[slot][1:] for slot in prep}
        for (slot, _, _), wav in zip(todo, wavs):
            out[slot] = (wav.reshape(-1),) + prep[slot][1:]
        return out

    @torch.no_grad()
    def stream_pieces(self):
        """Generator of (session id, wav_chunk, done) over every open session until none is left.  All running sessions advance in one
        decode batch, by the smallest distance of any of them to its next piece boundary (or its own max_mel_tokens), so none overshoots;
        each session's pieces equal what tts_stream would have yielded for it.  Sessions opened between pieces join the batch."""
        if self.max_streams == 1:
            raise NotImplementedError("stream_pieces: create the instance with max_streams=2 .. 4")
        while self._sessions:
            step = min(sess.target - sess.n for sess in self._sessions.values())
            if self.per_session_sampling:  # (every session with the settings it was opened with)
                n_total, finished = self.ar.advance(max(step, 1))
            else:
                temperature, top_p, repetition_penalty, top_k, typical_mass = self._session_settings
                n_total, finished = self.ar.advance(max(step, 1), temperature=temperature, top_p=top_p, repetition_penalty=repetition_penalty,
                                                    top_k=top_k, typical_mass=typical_mass)
            batch = sorted(self._sessions.items())  # the sessions this advance served (open_stream / close_stream may run between pieces)
            # every session whose piece is due is vocoded in one batched call before the first yield of the round
            vocoded = self._vocode_due([(slot, sess, n_total[slot], finished[slot]) for slot, sess in batch
                                        if finished[slot] or n_total[slot] >= sess.target])
            due = [(slot, sess, n_total[slot], finished[slot]) for slot, sess in batch if finished[slot] or n_total[slot] >= sess.target]
            resampled = self._resample_due(due, vocoded) if any(self._chain_of(sess) is not None for _, sess, _, _ in due) else {}
            for slot, sess in batch:
                if self._sessions.get(slot) is not sess:  # closed while an earlier piece of this round was out
                    continue
                sess.n = n_total[slot]
                if slot not in resampled and not (finished[slot] or n_total[slot] >= sess.target):
                    continue
                pieces = resampled[slot] if slot in resampled else self._session_piece(sess, n_total[slot], finished[slot], vocoded.get(slot))
                if pieces[-1][1]:  # the session is over: its row is free for the next admission
                    del self._sessions[slot]
                    self.ar.close(slot)
                    self._close_rs(sess)
                for wav_chunk, done in pieces:
                    yield sess.sid, wav_chunk, done

    def tts_stream_many(self, texts, **kwargs):
        """Stream several texts at once (max_streams > 1): a generator of (index into texts, wav_chunk, done).  kwargs are tts_stream's,
        shared by all texts; use_deterministic_seed may be a list with one seed per text, and so may temperature, top_p,
        repetition_penalty, top_k, typical_sampling and typical_mass on an instance with per_session_sampling.  Texts beyond the free
        slots are admitted as earlier sessions end.  stream_sample_rate= (Hz, 8000 .. 96000; one value or a list with one per text,
        None allowed): that text's pieces at another rate than 24 kHz, see open_stream.  stream_speaking_rate= and stream_pitch= (one value
        or a list with one per text, None allowed): that text's pieces at another speaking rate and pitch, see open_stream.
        stream_loudness=, stream_gain=, stream_true_peak=, stream_limit= and stream_level= (one value or a list with one per text, None
        allowed): that text's pieces at a level, see open_stream."""
        tsm.refuse_streaming(kwargs, "tts_stream_many")
        tsm.refuse_word_rates(kwargs, "tts_stream_many")
        loud.refuse_streaming(kwargs, "tts_stream_many")
        rs.refuse_streaming(kwargs, "tts_stream_many")
        rs.refuse_word_pitches(kwargs, "tts_stream_many")
        f0m.refuse_streaming(kwargs, "tts_stream_many")
        sil.refuse_streaming(kwargs, "tts_stream_many")
        fmt.refuse_streaming(kwargs, "tts_stream_many")
        nr.refuse_streaming(kwargs, "tts_stream_many")
        fastsolver.refuse_streaming(kwargs, "tts_stream_many")
        seeds = kwargs.pop("use_deterministic_seed", None)
        if not isinstance(seeds, (list, tuple)):
            seeds = [seeds] * len(texts)
        per_text = {}
        if isinstance(kwargs.get("stream_sample_rate"), (list, tuple)):  # one rate per text, None allowed
            if len(kwargs["stream_sample_rate"]) != len(texts):
                raise ValueError(f"tts_stream_many: {len(kwargs['stream_sample_rate'])} stream_sample_rate values for {len(texts)} texts")
            per_text["stream_sample_rate"] = kwargs.pop("stream_sample_rate")
        for r in per_text.get("stream_sample_rate", [kwargs.get("stream_sample_rate")]):
            rs.stream_options({"stream_sample_rate": r})  # (every rate is validated before the first session opens)
        for name in ("stream_speaking_rate", "stream_pitch"):
            if isinstance(kwargs.get(name), (list, tuple)):
                if len(kwargs[name]) != len(texts):
                    raise ValueError(f"tts_stream_many: {len(kwargs[name])} {name} values for {len(texts)} texts")
                per_text[name] = kwargs.pop(name)
        for i in range(len(texts)):  # (every text's rate and pitch are validated together before the first session opens)
            tsm.stream_options({name: per_text[name][i] if name in per_text else kwargs.get(name) for name in ("stream_speaking_rate", "stream_pitch")})
        for name in loud.STREAM_KEYS:  # (stream_loudness=, stream_gain=, ...: one value or one per text, None allowed)
            if isinstance(kwargs.get(name), (list, tuple)):
                if len(kwargs[name]) != len(texts):
                    raise ValueError(f"tts_stream_many: {len(kwargs[name])} {name} values for {len(texts)} texts")
                per_text[name] = kwargs.pop(name)
        for i in range(len(texts)):  # (every text's leveling keywords are validated together before the first session opens)
            loud.stream_options({name: per_text[name][i] if name in per_text else kwargs.get(name) for name in loud.STREAM_KEYS})
        for name in ("temperature", "top_p", "repetition_penalty", "top_k", "typical_sampling", "typical_mass"):
            if isinstance(kwargs.get(name), (list, tuple)):
                if not self.per_session_sampling:
                    raise ValueError(f"tts_stream_many: a list of {name} values needs an instance with per_session_sampling=True")
                if len(kwargs[name]) != len(texts):
                    raise ValueError(f"tts_stream_many: {len(kwargs[name])} {name} values for {len(texts)} texts")
                per_text[name] = kwargs.pop(name)
        pending = list(range(len(texts)))
        index = {}

        def admit():
            while pending and len(self._sessions) < self.max_streams:
                i = pending.pop(0)
                own = {name: values[i] for name, values in per_text.items()}
                index[self.open_stream(texts[i], use_deterministic_seed=seeds[i], **kwargs, **own)] = i

        admit()
        pieces = self.stream_pieces()
        while True:
            try:
                sid, wav_chunk, done = next(pieces)
            except StopIteration:
                if not pending:
                    return
                admit()
                pieces = self.stream_pieces()
                continue
            yield index[sid], wav_chunk, done
            if done:
                admit()
