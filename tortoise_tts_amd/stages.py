"""Host-side stage objects: one per C-ABI handle.  They own the packed weights, translate between
the reference's tensor conventions (channels-first, int64 ids) and the engine's, and keep every
call on the caller's current torch stream.  No model arithmetic happens here beyond embedding
gathers for the once-per-utterance prefix (plumbing).
"""
import ctypes as C
import itertools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import engine as E
from . import denoise as nr
from . import formant as fmt
from . import loudness as loud
from . import pack
from . import pitch as f0m
from . import resample as rs
from . import stretch as tsm
from .config import ARConfig, CLVPConfig, CVVPConfig, DiffusionConfig, VocoderConfig
from .schedule import Schedule


def session_sampling(temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, typical_mass=0.0):
    """One session's sampling settings as the engine takes them: (temperature, top_p, repetition_penalty, top_k, typical_mass), checked
    as tt_ar_generate_chunk checks them (ValueError).  typical_mass 0 = off."""
    v = (float(temperature), float(top_p), float(repetition_penalty), int(top_k), float(typical_mass))
    if not (v[0] > 0 and v[1] > 0 and v[2] > 0):
        raise ValueError(f"temperature={temperature}, top_p={top_p} and repetition_penalty={repetition_penalty} must be positive")
    if not (v[4] == 0.0 or 0.0 < v[4] < 1.0):
        raise ValueError(f"typical_mass={typical_mass} must be 0 (off) or lie in (0, 1)")
    return v


def _i32(t, device):
    return t.to(device=device, dtype=torch.int32).contiguous()


def latent_pass_embeddings(text_emb_w, text_pos_w, mel_emb_w, mel_pos_w, cfg, cond, text_tokens, codes, stream_positions=False):
    """Input rows of the teacher-forced pass (autoregressive.py:454-506): [cond | start text stop | start codes stop] with their
    learned positions -> (emb f32 [k, 1 + T + 2 + n + 2, D], number of mel rows).  Plain tensor indexing (device or host)."""
    k, n = codes.shape
    t = F.pad(text_tokens.long(), (0, 1), value=cfg.stop_text_token)
    t = F.pad(t, (1, 0), value=cfg.start_text_token)
    text_emb = text_emb_w[t] + text_pos_w[: t.shape[1]][None]
    m = F.pad(codes.long(), (0, 1), value=cfg.stop_mel_token)
    m = F.pad(m, (1, 0), value=cfg.start_mel_token)
    pos = torch.arange(m.shape[1], device=m.device)
    if stream_positions:
        pos = torch.where(pos > 0, pos + 1, pos)
    mel_emb = mel_emb_w[m] + mel_pos_w[pos][None]
    if text_emb.shape[0] == 1 and k > 1:
        text_emb = text_emb.expand(k, -1, -1)
    if cond.shape[0] == 1 and k > 1:
        cond = cond.expand(k, -1)
    return torch.cat([cond[:, None, :], text_emb, mel_emb], dim=1).contiguous(), m.shape[1]


class _Handle:
    """A stage that owns one engine handle `h`: made by <api>_create, destroyed by close() or when the stage is collected.
    `api` is the prefix of the stage's C entry points (tt_ar, tt_clvp, ...)."""

    api = None

    def _create(self, *args):
        self.h = E.vp()
        E.check(self._fn("_create")(*args, C.byref(self.h)))

    def _fn(self, suffix):
        return getattr(self.lib, self.api + suffix)

    def close(self):
        if self.h:
            self._fn("_destroy")(self.h)
            self.h = E.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GuardedHandle(_Handle):
    """A stage whose kernels count the non-finite values they meet (operand-overflow guard).  Stages without one have no guard()
    at all: TextToSpeech looks for the attribute."""

    def guard(self, reset=True):
        """Non-finite values this stage's kernels met since the last reset (norms / sampler of the AR and CLVP / CVVP stages, GroupNorm
        statistics / sampler inputs of the diffusion stage, predicted LVC kernels of the vocoder), as of its last finished run: read it
        after a synchronisation (e.g. reading the result)."""
        return E.guard_count(self._fn("_guard")(self.h, int(reset)))


class ArStage(_GuardedHandle):
    """UnifiedVoice hot path: prefill + sampling loop + latent re-pass (autoregressive.py:454-563)."""

    api = "tt_ar"

    def __init__(self, sd, cfg: ARConfig = ARConfig(), device="cuda", dtype=E.TT_BF16, max_batch=256, max_text=402,
                 max_new_tokens=500, max_latent_candidates=4, share_weights_with=None, kv_cache=True, max_groups=1, sessions=False,
                 per_session_sampling=False):
        """sessions=True: a session handle (TT_AR_OPT_SESSIONS) - each of its max_batch <= 4 rows serves one streaming session, admitted,
        advanced and retired on its own (admit / advance / session_codes / session_latents / close(slot)); max_batch = 5 .. 16 opens a
        wide session handle (option value 2).  per_session_sampling=True
        (TT_AR_OPT_SESSION_SAMPLING): every session keeps the sampling settings it was admitted with (admit(..., temperature=...))."""
        if per_session_sampling and not sessions:
            raise ValueError("per_session_sampling=True needs sessions=True")
        self.lib = E.init()
        if sessions:
            max_groups = max(max_groups, max_batch)
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        # several handles (one per concurrent decode stream) can share one packed copy of the weights
        self.w = share_weights_with.w if share_weights_with is not None else pack.pack_ar(sd, cfg, self.device, dtype)
        c = E.ArConfig()
        c.dtype = dtype
        c.layers, c.model_dim, c.heads = cfg.layers, cfg.model_dim, cfg.heads
        c.vocab = cfg.number_mel_codes
        c.start_mel_token, c.stop_mel_token = cfg.start_mel_token, cfg.stop_mel_token
        c.mel_pos_len = cfg.mel_pos_len
        c.max_batch = max_batch
        c.max_prefix = 1 + max_text + 2 + 1
        c.max_new_tokens = max_new_tokens + 2
        c.max_full_rows = max_latent_candidates * (1 + max_text + 2 + max_new_tokens + 2)
        # TextToSpeech(kv_cache=...) only changes WHICH mel position row a generated token gets (autoregressive.py:134-149):
        # the engine always keeps a KV cache; kv_cache=False (the reference default) selects rows 0,1,2,... instead of 0,2,3,...
        c.mel_pos_offset = 2 if kv_cache else 1
        c.max_groups = max_groups  # utterances decoded in one batch (prefill_group); max_batch counts the sequences of all of them
        self.max_groups = max_groups
        self.max_latent_candidates = max_latent_candidates
        self.ccfg = c
        self._create(C.byref(c), C.byref(self.w.weights))
        self.sessions = bool(sessions)
        if self.sessions:
            self.set_option(E.TT_AR_OPT_SESSIONS, 1 if max_batch <= 4 else 2)
            self.per_session_sampling = bool(per_session_sampling)
            if self.per_session_sampling:
                self.set_option(E.TT_AR_OPT_SESSION_SAMPLING, 1)
                self._settings = [session_sampling()] * max_batch
            self.max_batch = max_batch
            self.max_new = max_new_tokens
            self._seeds = [0] * max_batch
            self._n = [0] * max_batch
            self._finished = [False] * max_batch
            self._codes = self._codes_buffer(max_batch, max_new_tokens)
        # A/B switches of the measurement scripts (scripts/ab_stage.py); the product default is what tt_ar_create sets
        for env, opt in (("TT_AR_LOOKAHEAD", E.TT_AR_OPT_LOOKAHEAD), ("TT_AR_FUSED_QKV_ATTN", E.TT_AR_OPT_FUSED_QKV_ATTN)):
            if os.environ.get(env):
                self.set_option(opt, int(os.environ[env]))

    def set_option(self, option, value):
        """tt_ar_set_option: host lookahead of the paced decode loop (no effect on the codes)."""
        E.check(self.lib.tt_ar_set_option(self.h, int(option), int(value)))

    def stat(self, which):
        """tt_ar_stat: 0 decode-step graph captures, 1 queue drains of the launch loop, 2 launches per decode step."""
        return self.lib.tt_ar_stat(self.h, int(which))

    # -- prefix (autoregressive.py:538-544)
    def prefix_embedding(self, cond_latent, text_tokens):
        cfg = self.cfg
        t = F.pad(text_tokens.to(self.device).long(), (0, 1), value=cfg.stop_text_token)
        t = F.pad(t, (1, 0), value=cfg.start_text_token)
        n = t.shape[1]
        text_emb = self.w.text_emb[t] + self.w.text_pos[:n][None]
        return torch.cat([cond_latent.to(self.device).float()[:, None, :], text_emb], dim=1)  # [1, P, D]

    def prefill(self, cond_latent, text_tokens):
        emb = self.prefix_embedding(cond_latent[:1], text_tokens[:1])[0].contiguous()
        self.P = emb.shape[0]
        E.check(self.lib.tt_ar_prefill(self.h, E.ptr(emb), self.P, E.stream_ptr()))

    def prefill_group(self, group, n_groups, cond_latent, text_tokens):
        """Prefix of utterance `group` of a batch of n_groups utterances that generate() then decodes together (sequences
        [group * B / n_groups, (group + 1) * B / n_groups)).  Call for group 0 first."""
        emb = self.prefix_embedding(cond_latent[:1], text_tokens[:1])[0].contiguous()
        self.P = emb.shape[0]
        E.check(self.lib.tt_ar_prefill_group(self.h, group, n_groups, E.ptr(emb), self.P, E.stream_ptr()))

    def logits(self, rows):
        out = torch.empty(rows, self.cfg.number_mel_codes, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_ar_get_logits(self.h, E.ptr(out), rows, E.stream_ptr()))
        return out

    def begin(self, B):
        E.check(self.lib.tt_ar_begin(self.h, B, E.stream_ptr()))

    def decode_step(self, tokens):
        t = _i32(tokens, self.device)
        E.check(self.lib.tt_ar_decode_step(self.h, E.ptr(t), E.stream_ptr()))

    def _codes_buffer(self, B, max_new):
        """int32 [B, max_new] receiving buffer of one call (the sampler itself writes a buffer the handle owns, so this address is
        not part of the kept decode-step graph's key)."""
        return torch.empty(B, max_new, device=self.device, dtype=torch.int32)

    def generate(self, B, max_new, temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, seed=0, row_offset=0,
                 exp_noise=None, group_seeds=None, typical_mass=0.0):
        """Returns (codes int64 [B, n_steps], n_steps).  exp_noise: optional f32 [max_new, B, V] Exp(1) draws.
        group_seeds: after prefill_group calls, one Philox key per utterance (default: `seed` for all of them).
        typical_mass: 0 < mass < 1 = tts(typical_sampling=True, typical_mass=mass) (autoregressive.py:558); 0 = off."""
        s = E.Sampling()
        s.temperature, s.top_p, s.repetition_penalty, s.top_k = temperature, top_p, repetition_penalty, top_k
        s.typical_mass = float(typical_mass)
        s.seed, s.row_offset = seed, row_offset
        if group_seeds is not None:
            gs = (C.c_ulonglong * len(group_seeds))(*[int(v) for v in group_seeds])
            s.group_seeds = C.cast(gs, C.POINTER(C.c_ulonglong))
        if exp_noise is not None:
            exp_noise = exp_noise.to(device=self.device, dtype=torch.float32).contiguous()
            assert exp_noise.shape == (max_new, B, self.cfg.number_mel_codes)
        s.exp_noise = E.ptr(exp_noise)
        codes = self._codes_buffer(B, max_new)
        n = C.c_int(0)
        E.check(self.lib.tt_ar_generate(self.h, B, max_new, C.byref(s), E.ptr(codes), C.byref(n), E.stream_ptr()))
        return codes[:, :n.value].long(), n.value

    def generate_stream(self, B, max_new, chunk, first_chunk=None, temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, seed=0,
                        row_offset=0, typical_mass=0.0):
        """Generator over the sampling loop in pieces (api_fast.py:389-420 pulls get_generator() token by token and decodes every
        `stream_chunk_size` tokens): yields (codes int64 [B, n_so_far], finished) after each chunk."""
        s = E.Sampling()
        s.temperature, s.top_p, s.repetition_penalty, s.top_k = temperature, top_p, repetition_penalty, top_k
        s.seed, s.row_offset = seed, row_offset
        s.typical_mass = float(typical_mass)
        s.exp_noise = None
        codes = self._codes_buffer(B, max_new)
        n, fin = C.c_int(0), C.c_int(0)
        first = True
        while True:
            want = min((first_chunk or chunk) if first else chunk, max_new - n.value)
            if want <= 0:
                return
            E.check(self.lib.tt_ar_generate_chunk(self.h, B, 1 if first else 0, want, max_new, C.byref(s), E.ptr(codes), C.byref(n),
                                                  C.byref(fin), E.stream_ptr()))
            first = False
            done = bool(fin.value) or n.value >= max_new
            yield codes[:, :n.value].long(), done
            if done:
                return

    def stream_latents(self, B, n):
        """f32 [B, n, D]: the per-step latents the decode loop filed for the first n tokens of the running generation - the latent
        half of the (token, latent) pairs of the reference's streaming generator (api_fast.py:402-411); max_batch <= 8 handles."""
        out = torch.empty(B, n, self.cfg.model_dim, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_ar_stream_latents(self.h, B, n, E.ptr(out), E.stream_ptr()))
        return out

    # -- session handles (sessions=True): one streaming session per row
    def admit(self, slot, cond_latent, text_tokens, seed, **settings):
        """Start a session in free row `slot`: its prefix is evaluated now, its first token is drawn at the next advance() with Philox
        key `seed`.  The running sessions are untouched.  With per_session_sampling, `settings` are the session's own (temperature,
        top_p, repetition_penalty, top_k, typical_mass; session_sampling's defaults), validated before the row is taken."""
        if self.per_session_sampling:
            own = session_sampling(**settings)
        elif settings:
            raise TypeError("admit: sampling settings belong to advance() unless the stage was made with per_session_sampling=True")
        emb = self.prefix_embedding(cond_latent[:1], text_tokens[:1])[0].contiguous()
        E.check(self.lib.tt_ar_prefill_group(self.h, int(slot), self.max_batch, E.ptr(emb), emb.shape[0], E.stream_ptr()))
        self._seeds[slot] = int(seed)
        self._n[slot], self._finished[slot] = 0, False
        if self.per_session_sampling:
            self._settings[slot] = own

    def advance(self, n, *args, **scalars):
        """Every running session samples up to n more tokens (a session stops at its stop token).  Returns (n_total, finished), lists
        over the slots.  scalars: temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, typical_mass=0.0 - they belong to the
        handle while a session that has sampled runs.  With per_session_sampling every session samples with its own settings (admit)
        and passing scalars here is a TypeError."""
        S = self.max_batch
        if self.per_session_sampling:
            if args or scalars:
                raise TypeError(f"advance: per-session sampling takes each session's settings at admit(), not {list(args) + sorted(scalars)}")
            s = (E.Sampling * S)()
            for r in range(S):
                v = self._settings[r]
                s[r].temperature, s[r].top_p, s[r].repetition_penalty, s[r].top_k, s[r].typical_mass = v
                s[r].seed, s[r].row_offset, s[r].exp_noise, s[r].group_seeds = self._seeds[r], 0, None, None
            sp = s
        else:
            s, gs = self._shared_sampling(*args, **scalars)
            sp = C.byref(s)
        n_total, fin = (C.c_int * S)(), (C.c_int * S)()
        E.check(self.lib.tt_ar_generate_chunk(self.h, S, 0, int(n), self.max_new, sp, E.ptr(self._codes), n_total, fin, E.stream_ptr()))
        self._n, self._finished = list(n_total), [bool(v) for v in fin]
        return list(self._n), list(self._finished)

    def _shared_sampling(self, temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, typical_mass=0.0):
        """The one tt_sampling of a handle without per-session sampling (and the seed array it points to)."""
        s = E.Sampling()
        s.temperature, s.top_p, s.repetition_penalty, s.top_k = temperature, top_p, repetition_penalty, top_k
        s.typical_mass = float(typical_mass)
        s.seed, s.row_offset, s.exp_noise = 0, 0, None
        gs = (C.c_ulonglong * self.max_batch)(*self._seeds)
        s.group_seeds = C.cast(gs, C.POINTER(C.c_ulonglong))
        return s, gs

    def session_codes(self, slot):
        """int64 [1, n]: the tokens session `slot` has sampled (its stop token included once it has finished)."""
        return self._codes[slot:slot + 1, :self._n[slot]].long()

    def session_latents(self, slot, n):
        """f32 [1, n, D]: latents 0 .. n - 1 of session `slot`, as stream_latents files them for a single generation."""
        out = torch.empty(self.max_batch, n, self.cfg.model_dim, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_ar_stream_latents(self.h, self.max_batch, n, E.ptr(out), E.stream_ptr()))
        return out[slot:slot + 1]

    def close(self, slot=None):
        """close(slot): retire the session in row `slot` (its row is free for the next admit).  close(): release the handle."""
        if slot is None:
            return super().close()
        self.set_option(E.TT_AR_OPT_SESSION_CLOSE, int(slot))
        self._n[slot], self._finished[slot] = 0, False

    # -- latent re-pass (autoregressive.py:454-506 as api.py:521-524 calls it)
    def latents(self, cond_latent, text_tokens, codes, stream_positions=False):
        """stream_positions: mel positions 0, 2, 3, ... instead of 0, 1, 2, ... - the per-step states the reference's streaming
        path collects under kv_cache=True (api_fast.py:389-414 with the cached-decode position rule of autoregressive.py:134-149)."""
        emb, mel_rows = latent_pass_embeddings(self.w.text_emb, self.w.text_pos, self.w.mel_emb, self.w.mel_pos, self.cfg,
                                               cond_latent.to(self.device).float(), text_tokens.to(self.device), codes.to(self.device),
                                               stream_positions)
        k = codes.shape[0]
        outs = []
        for i in range(0, k, self.max_latent_candidates):
            e = emb[i:i + self.max_latent_candidates].contiguous()
            out = torch.empty_like(e)
            E.check(self.lib.tt_ar_latents(self.h, E.ptr(e), e.shape[0], e.shape[1], E.ptr(out), E.stream_ptr()))
            outs.append(out)
        out = torch.cat(outs, dim=0)
        # enc = hidden[:, 1:]; mel part = last mel_rows rows; drop the final two (autoregressive.py:425-431, 503)
        return out[:, -mel_rows:][:, :-2]


class ClvpStage(_GuardedHandle):
    """CLVP.forward(return_loss=False) (clvp.py:99-135)."""

    api = "tt_clvp"

    def __init__(self, sd, cfg: CLVPConfig = CLVPConfig(), device="cuda", dtype=E.TT_BF16, max_rows=256 * 500):
        self.lib = E.init()
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = pack.pack_clvp(sd, cfg, self.device, dtype)
        c = E.ClvpConfig()
        c.dtype, c.dim, c.latent_dim, c.depth, c.heads = dtype, cfg.dim, cfg.dim_latent, cfg.depth, cfg.heads
        c.ff_inner, c.rot_dim, c.max_rows = cfg.dim * cfg.ff_mult, cfg.rotary_dim, max_rows
        self.max_rows = max_rows
        self._create(C.byref(c), C.byref(self.w.text), C.byref(self.w.speech), E.ptr(self.w.temperature))

    def score(self, text_tokens, codes):
        """text_tokens int [1 or B, T] (rows identical), codes int [B, n] -> f32 [B]."""
        text = _i32(text_tokens[0], self.device)
        B, n = codes.shape
        outs = []
        per = max(1, self.max_rows // n)
        for i in range(0, B, per):
            c = _i32(codes[i:i + per], self.device)
            out = torch.empty(c.shape[0], device=self.device, dtype=torch.float32)
            E.check(self.lib.tt_clvp_score(self.h, E.ptr(text), text.shape[0], E.ptr(c), c.shape[0], n, E.ptr(out), E.stream_ptr()))
            outs.append(out)
        return torch.cat(outs)

    def score_groups(self, texts, codes):
        """Several utterances of one voice (long-form reading): texts = list of G int tensors [1, T_g], codes int [G * N, n] with the N
        candidates of utterance g in rows [g * N, (g + 1) * N) -> f32 [G * N].  ONE speech-tower pass for as many utterances as the
        handle's capacity holds (at most 16 per pass); every score equals score() on that utterance alone, bit for bit."""
        G = len(texts)
        GN, n = codes.shape
        assert G >= 1 and GN % G == 0
        N = GN // G
        per = max(1, min(16, self.max_rows // max(1, N * n)))
        if N * n > self.max_rows:  # one utterance's candidates do not fit one pass: fall back to the chunked single-utterance form
            return torch.cat([self.score(texts[g], codes[g * N:(g + 1) * N]) for g in range(G)])
        outs = []
        for g0 in range(0, G, per):
            sel = texts[g0:g0 + per]
            flat = torch.cat([_i32(t.reshape(-1), self.device) for t in sel])
            lens = (C.c_int * len(sel))(*[int(t.numel()) for t in sel])
            c = _i32(codes[g0 * N:(g0 + len(sel)) * N], self.device)
            out = torch.empty(c.shape[0], device=self.device, dtype=torch.float32)
            E.check(self.lib.tt_clvp_score_groups(self.h, E.ptr(flat), lens, len(sel), E.ptr(c), N, n, E.ptr(out), E.stream_ptr()))
            outs.append(out)
        return torch.cat(outs)


def nearest_interp_index(m, s):
    """Source row of F.interpolate(mode='nearest') for each of s outputs given m inputs
    (ATen nearest_neighbor_compute_source_index: floor(dst * float(m / s)), clamped)."""
    scale = np.float32(m) / np.float32(s)
    idx = np.floor(np.arange(s, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, m - 1).astype(np.int32)


class CvvpStage(_GuardedHandle):
    """The CVVP term of the candidate ranking, tts(cvvp_amount > 0) (cvvp.py:107-131 as api.py:464-468 drives it)."""

    api = "tt_cvvp"

    def __init__(self, sd, cfg: CVVPConfig = CVVPConfig(), device="cuda", dtype=E.TT_F16, max_rows=256 * 500, max_cond_frames=520):
        self.lib = E.init()
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = pack.pack_cvvp(sd, cfg, self.device, dtype)
        c = E.CvvpConfig()
        c.dtype, c.dim, c.heads, c.depth, c.rot_dim = dtype, cfg.model_dim, cfg.heads, cfg.depth, cfg.rotary_dim
        c.mel_channels, c.mel_pad, c.max_rows, c.max_cond_frames = cfg.mel_channels, self.w.mel_pad, max_rows, max_cond_frames
        self.max_rows, self.max_cond_frames = max_rows, max_cond_frames
        self._create(C.byref(c), C.byref(self.w.weights))

    def score(self, auto_conds, codes):
        """auto_conds f32 [1, n_clips, 80, T] (the voice's conditioning clips, api.py:262-276), codes int [B, n] -> f32 [B]: the mean over
        the clips of cvvp(clip, codes) (api.py:464-468)."""
        mels = auto_conds.to(self.device).float().reshape(-1, auto_conds.shape[-2], auto_conds.shape[-1]).contiguous()
        n_clips, _, T = mels.shape
        if T > self.max_cond_frames:
            raise ValueError(f"conditioning clips of {T} mel frames exceed this CVVP handle's capacity ({self.max_cond_frames})")
        B, n = codes.shape
        outs = []
        per = max(1, self.max_rows // n)
        for i in range(0, B, per):
            c = _i32(codes[i:i + per], self.device)
            out = torch.empty(c.shape[0], device=self.device, dtype=torch.float32)
            E.check(self.lib.tt_cvvp_score(self.h, E.ptr(mels), n_clips, T, E.ptr(c), c.shape[0], n, E.ptr(out), E.stream_ptr()))
            outs.append(out)
        return torch.cat(outs)


class AlignerStage(_GuardedHandle):
    """The wav2vec2 CTC model of the redaction path (wav2vec_alignment.py:63-72 Wav2VecAlignment.align up to the logits): a 24 kHz clip ->
    the argmax id of every frame.  source = (config dict, state_dict, vocab dict, tokenizer config dict) as align.find_aligner reads them."""

    api = "tt_w2v"

    def __init__(self, source, device="cuda", dtype=E.TT_F16, max_samples=24000 * 30):
        from . import align
        cfg, sd, vocab, tok_cfg = source
        fields = align.check_config(cfg)  # (before the library: a config the stage does not implement is refused on any machine)
        self.lib = E.init()
        self.device = torch.device(device)
        self.dtype = dtype
        self.source = source
        self.tokenizer = align.CtcTokenizer(vocab, tok_cfg)
        self.fields = fields
        self.w = pack.pack_w2v(sd, fields, self.device, dtype)
        c = E.W2vConfig()
        c.dtype, c.dim, c.heads, c.layers, c.ff_dim, c.conv_dim = dtype, fields["dim"], fields["heads"], fields["layers"], fields["ff_dim"], 512
        for i in range(E.W2V_CONV_LAYERS):
            c.conv_kernel[i], c.conv_stride[i] = fields["conv_kernel"][i], fields["conv_stride"][i]
        c.pos_kernel, c.pos_groups, c.vocab, c.vocab_pad = fields["pos_kernel"], fields["pos_groups"], fields["vocab"], self.w.vocab_pad
        c.max_samples, c.eps = int(max_samples), fields["eps"]
        self.max_samples = int(max_samples)
        self._create(C.byref(c), C.byref(self.w.weights))

    def frames(self, samples):
        return self.lib.tt_w2v_frames(self.h, int(samples))

    def run(self, audio, logits=False):
        """audio f32 [S] or [1, S] at 24 kHz -> frame ids int32 [T] on the device (and the logits f32 [T, vocab] with logits=True)."""
        x = audio.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
        S = x.shape[0]
        if S > self.max_samples:
            raise ValueError(f"a clip of {S} samples exceeds the aligner's capacity ({self.max_samples})")
        T = self.frames(S)
        if T < 1:
            raise ValueError(f"a clip of {S} samples is shorter than the aligner's receptive field")
        ids = torch.empty(T, device=self.device, dtype=torch.int32)
        lg = torch.empty(T, self.fields["vocab"], device=self.device, dtype=torch.float32) if logits else None
        E.check(self.lib.tt_w2v_run(self.h, E.ptr(x), S, E.ptr(ids), E.ptr(lg), E.stream_ptr()))
        return (ids, lg) if logits else ids

    def frame_ids(self, audio):
        """-> the frame ids as a host list (synchronises: the overflow guard can be read afterwards)."""
        return self.run(audio).cpu().tolist()


class _Tables:
    """Named flat lists of one dtype laid end to end in one host buffer and copied to the device in one go: p(name) is the device address
    of an array, whatever stands before it."""

    def __init__(self, device, dtype=torch.int32, **arrays):
        self.at, flat = {}, []
        for name, v in arrays.items():
            self.at[name] = len(flat)
            flat += v
        self.t = torch.tensor(flat, dtype=dtype).to(device)

    def p(self, name):
        return self.t.data_ptr() + self.at[name] * self.t.element_size()


class _Results:
    """Result arrays from named sizes, <torch dtype name>=dict(name=elements): one zero-filled device tensor per dtype, its arrays end to
    end and one pad element behind them (an empty array still has an address).  p(name) is an array's device address for the call; after
    cpu(), one copy back per dtype, [name] is the array on the host, a numpy view of that copy."""

    def __init__(self, device, **dtypes):
        self.at, self.buf = {}, {}
        for dt, sizes in dtypes.items():
            o = 0
            for name, k in sizes.items():
                self.at[name] = (dt, o, int(k))
                o += int(k)
            self.buf[dt] = torch.zeros(o + 1, device=device, dtype=getattr(torch, dt))

    def p(self, name):
        dt, o, _ = self.at[name]
        return self.buf[dt].data_ptr() + o * self.buf[dt].element_size()

    def cpu(self):
        self.buf = {dt: b.cpu().numpy() for dt, b in self.buf.items()}

    def __getitem__(self, name):
        dt, o, k = self.at[name]
        return self.buf[dt][o:o + k]


class _ClipStage(_Handle):
    """A stage over ragged batches of clips: every public call checks its clips, splits them into groups the handle takes in one call
    (_groups) and hands each group to the stage's _group, which packs its tables (_Tables), makes ONE library call on the current stream
    and cuts every clip's result out of the result buffers (_Results).  The wording of the shared errors comes from class attributes."""

    noun = None               # "... exceed the <noun> capacity"
    what = None               # "<what>: the device stage refused clips it was handed"
    capacity = "max_samples"  # the attribute that bounds a clip
    least, least_text = 1, "one sample"

    def __init__(self, max_samples, max_clips=16, device="cuda", extra=()):
        """extra: what <api>_create takes after (capacity, max_clips); None: the stage calls _create itself."""
        self.lib = E.init()
        self.device = torch.device(device)
        setattr(self, self.capacity, int(max_samples))
        self.max_clips = int(max_clips)
        if extra is not None:
            self._create(int(max_samples), self.max_clips, *extra)

    def _check_clip(self, i, x):
        if x.dim() != 1 or x.shape[0] < self.least:
            raise ValueError(f"clip {i}: audio of shape {tuple(x.shape)}, expected [samples] with at least {self.least_text}")
        if x.shape[0] > getattr(self, self.capacity):
            raise ValueError(f"clip {i}: {x.shape[0]} samples exceed the {self.noun} capacity ({getattr(self, self.capacity)})")

    def _groups(self, clips):
        """[(first, end)] of the runs of clips that go into one call each."""
        return [(g, min(g + self.max_clips, len(clips))) for g in range(0, len(clips), self.max_clips)]

    def _run(self, clips, *per_clip, **options):
        """_group over every group of `clips` and the matching slices of the per-clip lists (None stays None) -> the results in order."""
        out = []
        for a, b in self._groups(clips):
            out += self._group(clips[a:b], *[None if v is None else v[a:b] for v in per_clip], **options)
        return out

    @staticmethod
    def _offsets(counts):
        """Per-clip counts -> a list of n + 1: where each clip's slice starts and the last one ends."""
        return list(itertools.accumulate(counts, initial=0))

    def _audio(self, clips):
        """The clips end to end on the device, one pad element behind them."""
        return torch.cat([x.to(device=self.device, dtype=torch.float32) for x in clips] + [torch.zeros(1, device=self.device)])

    @staticmethod
    def _host(a):
        """A slice of a result array as a host tensor of its own."""
        return torch.from_numpy(a.copy())

    def _accepted(self, status, ok):
        """The per-clip status as a list; RuntimeError unless every one is in `ok`."""
        status = status.tolist()
        if any(st not in ok for st in status):
            raise RuntimeError(f"{self.what}: the device stage refused clips it was handed (status {status})")
        return status


class CtcAlignStage(_ClipStage):
    """CTC forced alignment of known targets with the aligner's logits (csrc/ctc_align.hip, include/tortoise_mi355x_ctc.h): ragged batches,
    one tt_ctc_align call per max_clips clips, every clip's result bit-identical to aligning it alone."""

    api, capacity = "tt_ctc", "max_frames"

    def __init__(self, vocab, blank, max_frames, max_tokens=E.CTC_MAX_TOKENS, max_clips=16, device="cuda"):
        self.vocab, self.blank, self.max_tokens = int(vocab), int(blank), int(max_tokens)
        super().__init__(max_frames, max_clips, device, extra=None)
        self._create(self.max_frames, self.max_tokens, self.max_clips, self.vocab, self.blank)

    @classmethod
    def for_aligner(cls, aligner, max_clips=16):
        """Sized from an AlignerStage: its vocabulary and blank, the frames of its longest clip."""
        from . import align
        f = aligner.fields
        frames = max(1, align.frames_for(aligner.max_samples, f["conv_kernel"], f["conv_stride"]))
        return cls(f["vocab"], align.blank_id(aligner.tokenizer), frames, max_clips=max_clips, device=aligner.device)

    def align_many(self, logits_list, targets_list):
        """logits f32 [T_i, vocab] (device or host) and target ids of every clip -> one dict per clip: status (E.CTC_*), and for status 0
        path int32 [T_i], spans int32 [L_i, 2], conf f32 [L_i] (host tensors) and score.  ValueError for a target or a clip beyond the handle."""
        if len(logits_list) != len(targets_list):
            raise ValueError(f"{len(logits_list)} clips with {len(targets_list)} targets")
        for i, (lg, tg) in enumerate(zip(logits_list, targets_list)):
            if len(tg) > self.max_tokens:
                raise ValueError(f"clip {i}: a target of {len(tg)} tokens exceeds the forced alignment's capacity ({self.max_tokens})")
            if lg.dim() != 2 or lg.shape[1] != self.vocab:
                raise ValueError(f"clip {i}: logits of shape {tuple(lg.shape)}, expected [frames, {self.vocab}]")
            if lg.shape[0] > self.max_frames:
                raise ValueError(f"clip {i}: {lg.shape[0]} frames exceed the forced alignment's capacity ({self.max_frames})")
        return self._run(logits_list, targets_list)

    def _group(self, logits_list, targets_list):
        n, dev = len(logits_list), self.device
        fo, to = self._offsets(lg.shape[0] for lg in logits_list), self._offsets(len(tg) for tg in targets_list)
        lg = torch.cat([x.to(device=dev, dtype=torch.float32).reshape(-1, self.vocab) for x in logits_list] + [torch.zeros(1, self.vocab, device=dev)])
        t = _Tables(dev, fo=fo, to=to, targets=[t for tg in targets_list for t in tg] + [0])
        r = _Results(dev, int32=dict(path=fo[-1], spans=2 * to[-1], status=n), float32=dict(conf=to[-1], score=n))  # two copies back
        E.check(self.lib.tt_ctc_align(self.h, n, lg.data_ptr(), t.p("fo"), t.p("targets"), t.p("to"), r.p("path"), r.p("spans"), r.p("conf"),
                                      r.p("score"), r.p("status"), E.stream_ptr()))
        r.cpu()
        path, spans, conf, score = r["path"], r["spans"].reshape(-1, 2), r["conf"], r["score"].tolist()
        out = []
        for i, st in enumerate(r["status"].tolist()):
            d = {"status": st}
            if st == E.CTC_OK:
                d.update(path=self._host(path[fo[i]:fo[i + 1]]), spans=self._host(spans[to[i]:to[i + 1]]), conf=self._host(conf[to[i]:to[i + 1]]), score=score[i])
            out.append(d)
        return out


class TimeStretchStage(_ClipStage):
    """WSOLA time-stretch of 24 kHz clips (csrc/tsm.hip, include/tortoise_mi355x_tsm.h): ragged batches, each clip with its own rate, one
    tt_tsm_stretch call per max_clips clips, every clip's result bit-identical to stretching it alone."""

    api, noun, what = "tt_tsm", "time-stretch stage's", "time-stretch"

    def stretch_many(self, clips, rqs):
        """clips f32 [n_i] (device or host) and the 16.16 rate of each (stretch.rate_q) -> one (y f32 [n_out_i] on the stage's device, chosen
        offsets int32 [K_i] on the host) per clip.  ValueError for an empty clip, a clip beyond the handle or a rate outside the range."""
        if len(clips) != len(rqs):
            raise ValueError(f"{len(clips)} clips with {len(rqs)} rates")
        for i, (x, rq) in enumerate(zip(clips, rqs)):
            self._check_clip(i, x)
            if not E.TSM_RATE_MIN <= int(rq) <= E.TSM_RATE_MAX:
                raise ValueError(f"clip {i}: rate {int(rq)} / 65536 is outside the supported range [0.5, 2.0]")
        return self._run(clips, [int(r) for r in rqs])

    def _group(self, clips, rqs):
        lens = [x.shape[0] for x in clips]
        oo = self._offsets(self.lib.tt_tsm_out_samples(m, r) for m, r in zip(lens, rqs))
        fo = self._offsets(self.lib.tt_tsm_frames(m, r) for m, r in zip(lens, rqs))
        return self._stretch(self.lib.tt_tsm_stretch, clips, oo, fo, _Tables(self.device, io=self._offsets(lens), oo=oo, fo=fo, rq=rqs), ("rq",))

    def _stretch(self, entry, clips, oo, fo, t, own):
        """The call of the two time-stretch stages, which differ in the tables `own` between in_off and out: -> (y, offsets) per clip."""
        n = len(clips)
        audio = self._audio(clips)
        y = torch.zeros(oo[-1] + 1, device=self.device, dtype=torch.float32)
        r = _Results(self.device, int32=dict(offsets=fo[-1], status=n))  # one copy back
        E.check(entry(self.h, n, audio.data_ptr(), t.p("io"), *[t.p(k) for k in own], y.data_ptr(), t.p("oo"), r.p("offsets"), t.p("fo"),
                      r.p("status"), E.stream_ptr()))
        r.cpu()
        self._accepted(r["status"], (E.TSM_OK,))  # (E.TSW_OK is the same 0)
        offsets = r["offsets"]
        return [(y[oo[i]:oo[i + 1]], self._host(offsets[fo[i]:fo[i + 1]])) for i in range(n)]


class WarpStretchStage(TimeStretchStage):
    """WSOLA time-stretch along a rate map (csrc/tsm_warp.hip, include/tortoise_mi355x_tsw.h): ragged batches, each clip with its own table
    of segments (stretch.RateMap.table), one tt_tsw_stretch call per max_clips clips, every clip's result bit-identical to stretching it
    alone; the table (0, 0, rq) gives TimeStretchStage's bits."""

    api, what = "tt_tsw", "time-stretch along a rate map"

    def __init__(self, max_samples, max_clips=16, max_segments=E.TSW_MAX_SEGMENTS, device="cuda"):
        self.max_segments = int(max_segments)
        super().__init__(max_samples, max_clips, device, (self.max_segments,))

    def stretch_many(self, clips, tables):
        """clips f32 [n_i] (device or host) and the table [(m, a, rq), ...] of each -> one (y f32 [n_out_i] on the stage's device, chosen
        offsets int32 [K_i] on the host) per clip.  ValueError for an empty clip, a clip beyond the handle or a table that breaks a rule."""
        if len(clips) != len(tables):
            raise ValueError(f"{len(clips)} clips with {len(tables)} rate maps")
        for i, (x, tb) in enumerate(zip(clips, tables)):
            self._check_clip(i, x)
            if not 1 <= len(tb) <= self.max_segments:
                raise ValueError(f"clip {i}: a rate map of {len(tb)} segments (1 .. {self.max_segments})")
            if not tsm.table_out_samples(x.shape[0], tb):
                raise ValueError(f"clip {i}: the rate map's table breaks a rule of include/tortoise_mi355x_tsw.h for a clip of {x.shape[0]} samples")
        return self._run(clips, tables)

    def _group(self, clips, tables):
        lens = [x.shape[0] for x in clips]
        oo = self._offsets(tsm.table_out_samples(m, tb) for m, tb in zip(lens, tables))
        fo = self._offsets(tsm.table_frames(m, tb) for m, tb in zip(lens, tables))
        t = _Tables(self.device, io=self._offsets(lens), so=self._offsets(len(tb) for tb in tables), oo=oo, fo=fo,
                    seg=[v for tb in tables for row in tb for v in row])
        return self._stretch(self.lib.tt_tsw_stretch, clips, oo, fo, t, ("seg", "so"))


class ResampleStage(_ClipStage):
    """Band-limited resampling at an arbitrary ratio (csrc/resample.hip, include/tortoise_mi355x_rs.h): ragged batches, each clip with its own
    (P, Q) input samples per output sample, one tt_rs_resample call per max_clips clips, every clip's result bit-identical to resampling it
    alone."""

    api, noun, what = "tt_rs", "resampling stage's", "resample"

    def resample_many(self, clips, ratios):
        """clips f32 [n_i] (device or host) and the (P, Q) of each (resample.ratio / pitch_ratio) -> one (y f32 [n_out_i] on the stage's
        device, max |y| as a float) per clip.  ValueError for an empty clip, a clip beyond the handle or a ratio the device refuses."""
        if len(clips) != len(ratios):
            raise ValueError(f"{len(clips)} clips with {len(ratios)} ratios")
        for i, (x, (P, Q)) in enumerate(zip(clips, ratios)):
            self._check_clip(i, x)
            if not self.lib.tt_rs_out_samples(x.shape[0], int(P), int(Q)):
                raise ValueError(f"clip {i}: ratio {int(P)}/{int(Q)} is outside what the resampler takes (terms up to {E.RS_MAX_TERM}, "
                                 f"1/{E.RS_MAX_RATIO} .. {E.RS_MAX_RATIO}, reduced unless Q = {E.RS_PITCH_ONE})")
        return self._run(clips, [(int(P), int(Q)) for P, Q in ratios])

    def _group(self, clips, ratios):
        lens = [x.shape[0] for x in clips]
        oo = self._offsets(self.lib.tt_rs_out_samples(m, P, Q) for m, (P, Q) in zip(lens, ratios))
        t = _Tables(self.device, io=self._offsets(lens), oo=oo, P=[P for P, _ in ratios], Q=[Q for _, Q in ratios])
        return self._resample(self.lib.tt_rs_resample, clips, oo, t, ("P", "Q"))

    def _resample(self, entry, clips, oo, t, own):
        """The call of the two resampling stages, which differ in the tables `own` between in_off and out: -> (y, peak) per clip."""
        n = len(clips)
        audio = self._audio(clips)
        y = torch.zeros(oo[-1] + 1, device=self.device, dtype=torch.float32)
        r = _Results(self.device, int32=dict(peak=n, status=n))  # (the peaks as f32 bits: one copy back)
        E.check(entry(self.h, n, audio.data_ptr(), t.p("io"), *[t.p(k) for k in own], y.data_ptr(), t.p("oo"), r.p("peak"), r.p("status"),
                      E.stream_ptr()))
        r.cpu()
        self._accepted(r["status"], (E.RS_OK,))  # (E.RSW_OK is the same 0)
        peaks = r["peak"].view(np.float32).tolist()
        return [(y[oo[i]:oo[i + 1]], float(peaks[i])) for i in range(n)]


class WarpResampleStage(ResampleStage):
    """Band-limited resampling along a pitch map (csrc/resample_warp.hip, include/tortoise_mi355x_rsw.h): ragged batches, each clip with its
    own table of segments (resample.map_plan), one tt_rsw_resample call per max_clips clips, every clip's result bit-identical to resampling
    it alone; the table (0, 0, 0, P) gives ResampleStage's bits at (P, 65536)."""

    api, what = "tt_rsw", "resample along a pitch map"

    def __init__(self, max_samples, max_clips=16, max_segments=E.RSW_MAX_SEGMENTS, device="cuda"):
        self.max_segments = int(max_segments)
        super().__init__(max_samples, max_clips, device, (self.max_segments,))

    def resample_many(self, clips, tables):
        """clips f32 [n_i] (device or host) and the table [(m, thi, tlo, P), ...] of each -> one (y f32 [n_out_i] on the stage's device,
        max |y| as a float) per clip.  ValueError for an empty clip, a clip beyond the handle or a table that breaks a rule."""
        if len(clips) != len(tables):
            raise ValueError(f"{len(clips)} clips with {len(tables)} pitch maps")
        for i, (x, tb) in enumerate(zip(clips, tables)):
            self._check_clip(i, x)
            if not 1 <= len(tb) <= self.max_segments:
                raise ValueError(f"clip {i}: a pitch map of {len(tb)} segments (1 .. {self.max_segments})")
            if not rs.map_out_samples(x.shape[0], tb):
                raise ValueError(f"clip {i}: the pitch map's table breaks a rule of include/tortoise_mi355x_rsw.h for a clip of {x.shape[0]} samples")
        return self._run(clips, tables)

    def _group(self, clips, tables):
        lens = [x.shape[0] for x in clips]
        oo = self._offsets(rs.map_out_samples(m, tb) for m, tb in zip(lens, tables))
        t = _Tables(self.device, io=self._offsets(lens), so=self._offsets(len(tb) for tb in tables), oo=oo,
                    seg=[v for tb in tables for row in tb for v in row])
        return self._resample(self.lib.tt_rsw_resample, clips, oo, t, ("seg", "so"))


class StreamResampleStage(_Handle):
    """The resampler fed in chunks (csrc/resample_stream.hip, include/tortoise_mi355x_rss.h): up to max_streams streams, each with its own
    (P, Q); whatever the chunking, what a stream emits is bit for bit ResampleStage's result for the whole clip.  form: "auto" (a phase
    bank for the few-phase ratios, the table otherwise), "table" or "bank"."""

    api = "tt_rss"
    FORMS = {"auto": E.RSS_AUTO, "table": E.RSS_TABLE, "bank": E.RSS_BANK}

    def __init__(self, max_streams=16, form="auto", device="cuda"):
        if form not in self.FORMS:
            raise ValueError(f"form={form!r}: one of {sorted(self.FORMS)}")
        self.lib = E.init()
        self.device = torch.device(device)
        self.max_streams, self.form = int(max_streams), form
        self.slots = {}  # open slot -> [P, Q, samples pushed, finished]
        self._create(self.max_streams, self.FORMS[form])

    def open(self, P, Q):
        """A free slot opened at ratio (P, Q) (resample.ratio) -> its number.  ValueError for a ratio the device refuses (before a slot is
        taken), RuntimeError when every slot is taken."""
        P, Q = rs.check_ratio(P, Q)
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError(f"all {self.max_streams} resampling streams are open")
        E.check(self.lib.tt_rss_open(self.h, free[0], P, Q, E.stream_ptr()))
        self.slots[free[0]] = [P, Q, 0, False]
        return free[0]

    def close(self, slot=None):
        """close(slot): the slot is free again (whatever it still held is dropped).  close(): the stage."""
        if slot is None:
            self.slots = {}
            return super().close()
        if self.slots.pop(slot, None) is not None and self.h:
            E.check(self.lib.tt_rss_close(self.h, int(slot)))

    def push_many(self, items):
        """items = [(slot, chunk f32 [n] (device or host, n >= 0), flush)], distinct open slots -> what each emits (f32 on the stage's
        device, possibly empty): ONE tt_rss_push, no synchronisation.  A flushed slot is finished: close() it to free it."""
        n = len(items)
        if not 1 <= n <= self.max_streams or len({s for s, _, _ in items}) != n:
            raise ValueError(f"push_many: {n} chunks for {len({s for s, _, _ in items})} slots (1 .. {self.max_streams} distinct slots)")
        counts = []
        for slot, x, flush in items:
            st = self.slots.get(slot)
            if st is None or st[3]:
                raise ValueError(f"push_many: slot {slot} is not open" if st is None else f"push_many: slot {slot} is finished")
            if x.dim() != 1:
                raise ValueError(f"push_many: slot {slot}: a chunk of shape {tuple(x.shape)}, expected [samples]")
            counts.append(rs.stream_ready(st[2], x.shape[0], st[0], st[1], flush))
        dev = self.device
        audio = torch.cat([x.to(device=dev, dtype=torch.float32) for _, x, _ in items] + [torch.zeros(1, device=dev)])
        y = torch.empty(sum(counts) + 1, device=dev, dtype=torch.float32)
        arr = C.c_int * n
        E.check(self.lib.tt_rss_push(self.h, n, arr(*[int(s) for s, _, _ in items]), arr(*[int(x.shape[0]) for _, x, _ in items]),
                                     arr(*[int(bool(f)) for _, _, f in items]), audio.data_ptr(), y.data_ptr(), E.stream_ptr()))
        out, o = [], 0
        for (slot, x, flush), c in zip(items, counts):
            st = self.slots[slot]
            st[2] += x.shape[0]
            st[3] = bool(flush)
            out.append(y[o:o + c])
            o += c
        return out


class StreamStretchStage(_Handle):
    """The WSOLA time-stretch fed in chunks (csrc/tsm_stream.hip, include/tortoise_mi355x_tss.h): up to max_streams streams, each with its
    own rate; whatever the chunking, what a stream emits - samples and chosen offsets - is bit for bit TimeStretchStage's result for the
    whole clip, 1407 input samples late until the flush."""

    api = "tt_tss"

    def __init__(self, max_streams=16, device="cuda"):
        self.lib = E.init()
        self.device = torch.device(device)
        self.max_streams = int(max_streams)
        self.slots = {}  # open slot -> [rq, samples pushed, finished]
        self._create(self.max_streams)

    def open(self, rq):
        """A free slot opened at the 16.16 rate rq (stretch.rate_q) -> its number.  ValueError for a rate outside [0.5, 2.0] (before a slot
        is taken), RuntimeError when every slot is taken."""
        rq = int(rq)
        if not E.TSM_RATE_MIN <= rq <= E.TSM_RATE_MAX:
            raise ValueError(f"rate {rq} / 65536 is outside the supported range [0.5, 2.0]")
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError(f"all {self.max_streams} time-stretch streams are open")
        E.check(self.lib.tt_tss_open(self.h, free[0], rq))
        self.slots[free[0]] = [rq, 0, False]
        return free[0]

    def close(self, slot=None):
        """close(slot): the slot is free again (whatever it still held is dropped).  close(): the stage."""
        if slot is None:
            self.slots = {}
            return super().close()
        if self.slots.pop(slot, None) is not None and self.h:
            E.check(self.lib.tt_tss_close(self.h, int(slot)))

    def push_many(self, items, return_offsets=False):
        """items = [(slot, chunk f32 [n] (device or host, n >= 0), flush)], distinct open slots -> what each emits (f32 on the stage's
        device, possibly empty): ONE tt_tss_push, no synchronisation.  return_offsets=True: (outputs, offsets) with the chosen d_k of the
        frames each slot ran as int32 tensors on the device (stretch.stream_offsets of them).  A flushed slot is finished: close() it to
        free it."""
        n = len(items)
        if not 1 <= n <= self.max_streams or len({s for s, _, _ in items}) != n:
            raise ValueError(f"push_many: {n} chunks for {len({s for s, _, _ in items})} slots (1 .. {self.max_streams} distinct slots)")
        counts, frames = [], []
        for slot, x, flush in items:
            st = self.slots.get(slot)
            if st is None or st[2]:
                raise ValueError(f"push_many: slot {slot} is not open" if st is None else f"push_many: slot {slot} is finished")
            if x.dim() != 1:
                raise ValueError(f"push_many: slot {slot}: a chunk of shape {tuple(x.shape)}, expected [samples]")
            counts.append(tsm.stream_ready(st[1], x.shape[0], st[0], flush))
            frames.append(tsm.stream_offsets(st[1], x.shape[0], st[0], flush) if return_offsets else 0)
        dev = self.device
        audio = torch.cat([x.to(device=dev, dtype=torch.float32) for _, x, _ in items] + [torch.zeros(1, device=dev)])
        y = torch.empty(sum(counts) + 1, device=dev, dtype=torch.float32)
        off = torch.empty(sum(frames) + 1, device=dev, dtype=torch.int32) if return_offsets else None
        arr = C.c_int * n
        E.check(self.lib.tt_tss_push(self.h, n, arr(*[int(s) for s, _, _ in items]), arr(*[int(x.shape[0]) for _, x, _ in items]),
                                     arr(*[int(bool(f)) for _, _, f in items]), audio.data_ptr(), y.data_ptr(),
                                     off.data_ptr() if return_offsets else None, E.stream_ptr()))
        out, offs, o, f = [], [], 0, 0
        for (slot, x, flush), c, k in zip(items, counts, frames):
            st = self.slots[slot]
            st[1] += x.shape[0]
            st[2] = bool(flush)
            out.append(y[o:o + c])
            o += c
            if return_offsets:
                offs.append(off[f:f + k])
                f += k
        return (out, offs) if return_offsets else out


class StreamLevelStage(_Handle):
    """The leveler fed in chunks (csrc/loudness_stream.hip, include/tortoise_mi355x_lvs.h): up to max_streams streams, each with its own
    settings (loudness.StreamSettings); BS.1770 loudness measured on the prefix heard so far, a slew-limited gain towards a target or a
    fixed gain, and the look-ahead limiter.  Whatever the chunking, what a stream emits is bit for bit what one flushed push of the whole
    clip emits, 248 input samples late under the limiter until the flush."""

    api = "tt_lvs"

    def __init__(self, max_streams=16, max_hops=E.LVS_DEFAULT_HOPS, device="cuda"):
        self.lib = E.init()
        self.device = torch.device(device)
        self.max_streams, self.max_hops = int(max_streams), int(max_hops)
        self.slots = {}  # open slot -> [settings, samples pushed, finished]
        self._create(self.max_streams, self.max_hops)

    def open(self, settings):
        """A free slot opened with a loudness.StreamSettings -> its number.  ValueError for settings the device refuses (before a slot is
        taken), RuntimeError when every slot is taken."""
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError(f"all {self.max_streams} leveling streams are open")
        if self.lib.tt_lvs_open(self.h, free[0], *settings.args()):
            raise ValueError(self.lib.tt_last_error().decode())
        self.slots[free[0]] = [settings, 0, False]
        return free[0]

    def close(self, slot=None):
        """close(slot): the slot is free again (whatever it still held is dropped).  close(): the stage."""
        if slot is None:
            self.slots = {}
            return super().close()
        if self.slots.pop(slot, None) is not None and self.h:
            E.check(self.lib.tt_lvs_close(self.h, int(slot)))

    def push_many(self, items):
        """items = [(slot, chunk f32 [n] (device or host, n >= 0), flush)], distinct open slots -> what each emits (f32 on the stage's
        device, possibly empty): ONE tt_lvs_push, no synchronisation.  A flushed slot is finished: close() it to free it."""
        n = len(items)
        if not 1 <= n <= self.max_streams or len({s for s, _, _ in items}) != n:
            raise ValueError(f"push_many: {n} chunks for {len({s for s, _, _ in items})} slots (1 .. {self.max_streams} distinct slots)")
        counts = []
        for slot, x, flush in items:
            st = self.slots.get(slot)
            if st is None or st[2]:
                raise ValueError(f"push_many: slot {slot} is not open" if st is None else f"push_many: slot {slot} is finished")
            if x.dim() != 1:
                raise ValueError(f"push_many: slot {slot}: a chunk of shape {tuple(x.shape)}, expected [samples]")
            if (st[1] + x.shape[0]) // E.LOUD_HOP > self.max_hops:
                raise ValueError(f"push_many: slot {slot}: {st[1]} + {x.shape[0]} samples pass the stage's {self.max_hops} hops of 100 ms")
            counts.append(loud.stream_ready(st[1], x.shape[0], st[0].limit, bool(flush)))
        dev = self.device
        audio = torch.cat([x.to(device=dev, dtype=torch.float32) for _, x, _ in items] + [torch.zeros(1, device=dev)])
        y = torch.empty(sum(counts) + 1, device=dev, dtype=torch.float32)
        arr = C.c_int * n
        E.check(self.lib.tt_lvs_push(self.h, n, arr(*[int(s) for s, _, _ in items]), arr(*[int(x.shape[0]) for _, x, _ in items]),
                                     arr(*[int(bool(f)) for _, _, f in items]), audio.data_ptr(), y.data_ptr(), E.stream_ptr()))
        out, o = [], 0
        for (slot, x, flush), c in zip(items, counts):
            st = self.slots[slot]
            st[1] += x.shape[0]
            st[2] = bool(flush)
            out.append(y[o:o + c])
            o += c
        return out

    def read(self, slot):
        """The slot's latest readings (synchronises): dict(lufs, status, blocks_abs, blocks_rel, gain_db, gain, peak, out_peak, limited,
        n_in, n_out, hops)."""
        d, i, f = C.c_double, C.c_int, C.c_float
        v = dict(lufs=d(), status=i(), blocks_abs=i(), blocks_rel=i(), gain_db=d(), gain=f(), peak=f(), out_peak=f(), limited=i())
        E.check(self.lib.tt_lvs_read(self.h, int(slot), *[C.byref(a) for a in v.values()], E.stream_ptr()))
        c = [i(), i(), i(), i()]
        E.check(self.lib.tt_lvs_state(self.h, int(slot), *[C.byref(a) for a in c]))
        return dict({k: a.value for k, a in v.items()}, n_in=c[0].value, n_out=c[1].value, hops=c[2].value)

    def trace(self, slot, first_hop=0, count=None):
        """The per-hop history of the slot (synchronises): dict of numpy arrays q, lufs, gain_db (f64), status, blocks_abs, blocks_rel (i32)."""
        c = [C.c_int() for _ in range(4)]
        E.check(self.lib.tt_lvs_state(self.h, int(slot), *[C.byref(a) for a in c]))
        count = c[2].value - first_hop if count is None else int(count)
        out = {k: np.zeros(max(count, 0), np.float64) for k in ("q", "lufs", "gain_db")}
        out.update({k: np.zeros(max(count, 0), np.int32) for k in ("status", "blocks_abs", "blocks_rel")})
        E.check(self.lib.tt_lvs_trace(self.h, int(slot), int(first_hop), count, *[a.ctypes.data for a in out.values()], E.stream_ptr()))
        return out


class SilenceStage(_ClipStage):
    """Speech regions, edge trimming and pause capping (csrc/silence.hip, include/tortoise_mi355x_sil.h): ragged batches, each clip with its
    own parameters (silence.Params), one tt_sil_find / tt_sil_trim call per max_clips clips, every clip's result bit-identical to running it
    alone."""

    api, noun, what = "tt_sil", "silence stage's", "silence"

    def _check(self, clips, params):
        if len(clips) != len(params):
            raise ValueError(f"{len(clips)} clips with {len(params)} parameter sets")
        for i, x in enumerate(clips):
            self._check_clip(i, x)

    def find_many(self, clips, params, energies=False):
        """clips f32 [n_i] (device or host) and a silence.Params each -> one dict per clip: status (E.SIL_OK / SIL_SILENT), regions
        [(a, b)] in samples, peak (E, the largest frame energy) and, for energies=True, energies (f64 [F] on the host)."""
        self._check(clips, params)
        return self._run(clips, params, trim=False, energies=energies)

    def trim_many(self, clips, params):
        """clips f32 [n_i] and a silence.Params each -> one (y f32 [n_out_i] on the stage's device, dict) per clip; the dict holds status
        (E.SIL_OK / SIL_UNCHANGED / SIL_SILENT), regions [(a, b)] of the input, segments [(o, i, l)] (silence.map_sample) and peak."""
        self._check(clips, params)
        return self._run(clips, params, trim=True, energies=False)

    def _group(self, clips, params, trim, energies):
        n, dev = len(clips), self.device
        lens = [x.shape[0] for x in clips]
        io, fo = self._offsets(lens), self._offsets(self.lib.tt_sil_frames(m) for m in lens)
        ro = self._offsets(self.lib.tt_sil_max_regions(m) for m in lens)  # (regions and segments alike)
        thr = torch.tensor([[p.rel, p.floor_e] for p in params], dtype=torch.float64).to(dev)
        audio = self._audio(clips)
        t = _Tables(dev, io=io, ro=ro, fo=fo, par=[v for p in params for v in (p.min_sil, p.pad, p.lead, p.trail, p.max_pause)[:5 if trim else 2]])
        r = _Results(dev, int32=dict(n_out=n, n_regions=n, n_segments=n, status=n, regions=2 * ro[-1], segments=3 * ro[-1]), float64=dict(peak=n))
        en = y = None
        if trim:
            y = torch.zeros(io[-1] + 1, device=dev, dtype=torch.float32)
            E.check(self.lib.tt_sil_trim(self.h, n, audio.data_ptr(), t.p("io"), thr.data_ptr(), t.p("par"), t.p("ro"), t.p("ro"), y.data_ptr(),
                                         r.p("n_out"), r.p("n_regions"), r.p("regions"), r.p("n_segments"), r.p("segments"), r.p("peak"),
                                         r.p("status"), E.stream_ptr()))
        else:
            en = torch.zeros(fo[-1] + 1, device=dev, dtype=torch.float64) if energies else None
            E.check(self.lib.tt_sil_find(self.h, n, audio.data_ptr(), t.p("io"), thr.data_ptr(), t.p("par"), t.p("ro"), t.p("fo") if energies else None,
                                         r.p("n_regions"), r.p("regions"), r.p("peak"), en.data_ptr() if energies else None, r.p("status"),
                                         E.stream_ptr()))
        r.cpu()
        status = self._accepted(r["status"], (E.SIL_OK, E.SIL_UNCHANGED, E.SIL_SILENT))
        peaks = r["peak"].tolist()
        n_out, n_reg, n_seg = (r[k].tolist() for k in ("n_out", "n_regions", "n_segments"))
        regs, segs = r["regions"].reshape(-1, 2), r["segments"].reshape(-1, 3)
        en = en.cpu() if en is not None else None
        out = []
        for i in range(n):
            d = dict(status=status[i], peak=peaks[i], regions=[(int(a), int(b)) for a, b in regs[ro[i]:ro[i] + n_reg[i]]])
            if trim:
                d["segments"] = [(int(o), int(s), int(m)) for o, s, m in segs[ro[i]:ro[i] + n_seg[i]]]
                out.append((y[io[i]:io[i] + n_out[i]], d))
            else:
                if en is not None:
                    d["energies"] = en[fo[i]:fo[i + 1]].clone()
                out.append(d)
        return out


class F0Stage(_ClipStage):
    """The YIN fundamental-frequency tracker (csrc/f0.hip, include/tortoise_mi355x_f0.h): ragged batches, each clip with its own parameters
    (pitch.Params), one tt_f0_track call per max_clips clips, every clip's result bit-identical to running it alone."""

    api, noun, what = "tt_f0", "F0 stage's", "f0"

    def track_many(self, clips, params, dprime=False):
        """clips f32 [n_i] (device or host) and a pitch.Params each -> one dict per clip: lag (i32 [F]), f0 (f32 [F], 0 where unvoiced), aper
        (f32 [F]) on the host, n_voiced; dprime=True: also dprime (f64 [F, 481], through the test entry tt_op_f0_track)."""
        if len(clips) != len(params):
            raise ValueError(f"{len(clips)} clips with {len(params)} parameter sets")
        for i, x in enumerate(clips):
            self._check_clip(i, x)
        return self._run(clips, params, dprime=dprime)

    def _group(self, clips, params, dprime):
        n, dev = len(clips), self.device
        lens = [x.shape[0] for x in clips]
        fo = self._offsets(self.lib.tt_f0_frames(m) for m in lens)
        Fs = fo[-1]
        thr = torch.tensor([[p.thr, p.floor_e] for p in params], dtype=torch.float64).to(dev)
        audio = self._audio(clips)
        t = _Tables(dev, io=self._offsets(lens), fo=fo, par=[v for p in params for v in (p.lag_lo, p.lag_hi)])
        r = _Results(dev, int32=dict(n_voiced=n, status=n, lag=Fs), float32=dict(f0=Fs, aper=Fs))
        args = (self.h, n, audio.data_ptr(), t.p("io"), t.p("par"), thr.data_ptr(), t.p("fo"), r.p("lag"), r.p("f0"), r.p("aper"), r.p("n_voiced"),
                r.p("status"))
        dpr = None
        if dprime:
            dpr = torch.zeros(Fs * (E.F0_LAG_MAX + 1) + 1, device=dev, dtype=torch.float64)
            E.check(self.lib.tt_op_f0_track(*args, dpr.data_ptr(), E.stream_ptr()))
        else:
            E.check(self.lib.tt_f0_track(*args, E.stream_ptr()))
        r.cpu()
        self._accepted(r["status"], (E.F0_OK,))
        lag, f0, aper, voiced = r["lag"], r["f0"], r["aper"], r["n_voiced"].tolist()
        dpr = dpr.cpu().numpy()[:-1].reshape(Fs, E.F0_LAG_MAX + 1) if dprime else None
        out = []
        for i in range(n):
            a, b = fo[i], fo[i + 1]
            d = dict(lag=lag[a:b].copy(), f0=f0[a:b].copy(), aper=aper[a:b].copy(), n_voiced=voiced[i])
            if dprime:
                d["dprime"] = dpr[a:b].copy()
            out.append(d)
        return out


class F0ViterbiStage(_ClipStage):
    """The Viterbi path over YIN candidates (csrc/f0_viterbi.hip, include/tortoise_mi355x_f0v.h): ragged batches, each clip with its own
    parameters (pitch.Params) and costs (pitch.Costs), one tt_f0v_track call per max_clips clips, every clip's result bit-identical to
    running it alone.  The handle gets pitch.LOG2_TABLE at create: the device evaluates no logarithm."""

    api, noun, what = "tt_f0v", "F0 path stage's", "f0 path"

    def __init__(self, max_samples, max_clips=16, device="cuda"):
        super().__init__(max_samples, max_clips, device, ((C.c_double * E.F0V_TABLE)(*f0m.LOG2_TABLE),))

    def track_many(self, clips, params, costs):
        """clips f32 [n_i] (device or host), a pitch.Params and a pitch.Costs each -> one dict per clip: lag (i32 [F]), f0 (f32 [F], 0 where
        the path is unvoiced), aper (f32 [F]), state (i32 [F], 0 .. 7) on the host, n_voiced and path_cost."""
        if not len(clips) == len(params) == len(costs):
            raise ValueError(f"{len(clips)} clips with {len(params)} parameter sets and {len(costs)} sets of costs")
        for i, x in enumerate(clips):
            self._check_clip(i, x)
        return self._run(clips, params, costs)

    def _group(self, clips, params, costs):
        n, dev = len(clips), self.device
        lens = [x.shape[0] for x in clips]
        fo = self._offsets(self.lib.tt_f0_frames(m) for m in lens)
        Fs = fo[-1]
        audio = self._audio(clips)
        t = _Tables(dev, io=self._offsets(lens), fo=fo, par=[v for p in params for v in (p.lag_lo, p.lag_hi)])
        d = _Tables(dev, torch.float64, thr=[v for p in params for v in (p.thr, p.floor_e)], cost=[float(v) for k in costs for v in k])
        r = _Results(dev, int32=dict(n_voiced=n, status=n, lag=Fs, state=Fs), float32=dict(f0=Fs, aper=Fs), float64=dict(path_cost=n))
        E.check(self.lib.tt_f0v_track(self.h, n, audio.data_ptr(), t.p("io"), t.p("par"), d.p("thr"), d.p("cost"), t.p("fo"), r.p("lag"), r.p("f0"),
                                      r.p("aper"), r.p("state"), r.p("n_voiced"), r.p("path_cost"), r.p("status"), E.stream_ptr()))
        r.cpu()
        self._accepted(r["status"], (E.F0_OK,))
        lag, f0, aper, state, voiced, cost = r["lag"], r["f0"], r["aper"], r["state"], r["n_voiced"].tolist(), r["path_cost"].tolist()
        return [dict(lag=lag[a:b].copy(), f0=f0[a:b].copy(), aper=aper[a:b].copy(), state=state[a:b].copy(), n_voiced=voiced[i], path_cost=cost[i])
                for i, (a, b) in enumerate(zip(fo, fo[1:]))]


class FormantStage(_ClipStage):
    """Formant-preserving pitch: the cepstral envelope correction of finished clips at 24 kHz (csrc/formant.hip,
    include/tortoise_mi355x_fmt.h): ragged batches, each clip with its own warp alpha, one tt_fmt_run call per max_clips clips, every clip's
    result bit-identical to correcting it alone.  The handle's `warps` table has 16 slots; the stage keeps one D per distinct warp in it and
    replaces the least recently used one when a new warp arrives (a copy on the current stream, ordered before the run that reads it)."""

    api, noun, fmt = "tt_fmt", "formant stage's", fmt
    least, least_text = fmt.MIN_SAMPLES, f"{fmt.MIN_SAMPLES} samples (the frames are centred with reflect padding)"

    def __init__(self, max_samples, q=None, max_gain_db=None, max_clips=E.FMT_MAX_CLIPS, device="cuda"):
        self.q = fmt.lifter_q() if q is None else int(q)
        self.max_gain_db = fmt.max_gain_db() if max_gain_db is None else fmt.max_gain_db(max_gain_db)
        if not fmt.Q_RANGE[0] <= self.q <= fmt.Q_RANGE[1]:
            raise ValueError(f"{self.q} cepstral coefficients; the stage takes {fmt.Q_RANGE[0]} .. {fmt.Q_RANGE[1]}")
        super().__init__(max_samples, max_clips, device, extra=None)
        t = fmt.tables(self.q, [1.0])
        self.t = {k: t[k].to(self.device).contiguous() for k in ("basis", "inverse", "cepstrum")}
        self.t["warps"] = torch.zeros(E.FMT_MAX_WARPS, E.FMT_Q_PAD, fmt.BINS_PAD, device=self.device, dtype=torch.float32)
        self.slots, self.clock = {}, 0  # alpha -> [slot, last use]
        c = E.FmtConfig()
        c.n_fft, c.hop, c.bins_pad, c.q, c.max_gain_db = fmt.N_FFT, fmt.HOP, fmt.BINS_PAD, self.q, self.max_gain_db
        c.max_samples, c.max_clips, c.n_warps = self.max_samples, self.max_clips, E.FMT_MAX_WARPS
        tb = E.FmtTables()
        tb.basis, tb.inverse, tb.cepstrum, tb.warps = (E.ptr(self.t[k]) for k in ("basis", "inverse", "cepstrum", "warps"))
        self._create(C.byref(c), C.byref(tb))

    def _slot(self, alpha, busy):
        """The slot of `warps` that holds D(alpha), filled on first use; `busy`: slots this call already relies on."""
        self.clock += 1
        if alpha in self.slots:
            self.slots[alpha][1] = self.clock
            return self.slots[alpha][0]
        if len(self.slots) < E.FMT_MAX_WARPS:
            slot = len(self.slots)
        else:
            old = min((a for a in self.slots if self.slots[a][0] not in busy), key=lambda a: self.slots[a][1])
            slot = self.slots.pop(old)[0]
        self.t["warps"][slot].copy_(self.fmt.warp_table(alpha, self.q).float())
        self.slots[alpha] = [slot, self.clock]
        return slot

    def correct_many(self, clips, alphas):
        """clips f32 [n] (device or host, n >= 513) and the warp alpha of each (0.5 .. 2) -> the corrected clips f32 [n] on the stage's
        device.  ValueError for a clip the handle does not take or a warp outside the range."""
        if len(clips) != len(alphas):
            raise ValueError(f"{len(clips)} clips with {len(alphas)} warps")
        alphas = [float(a) for a in alphas]
        for i, (x, a) in enumerate(zip(clips, alphas)):
            self._check_clip(i, x)
            if not self.fmt.WARP_RANGE[0] <= a <= self.fmt.WARP_RANGE[1]:
                raise ValueError(f"clip {i}: warp {a!r} is outside {self.fmt.WARP_RANGE}")
        return self._run(clips, alphas)

    def _group(self, clips, alphas):
        k, dev = len(clips), self.device
        busy, idx = set(), []
        for a in alphas:
            idx.append(self._slot(a, busy))
            busy.add(idx[-1])
        lens = [int(x.shape[0]) for x in clips]
        offs = [0] * k
        for i in range(1, k):
            offs[i] = offs[i - 1] + lens[i - 1]
        parts = [x.to(device=dev, dtype=torch.float32) for x in clips]
        wav = (torch.cat(parts) if k > 1 else parts[0]).contiguous()
        y = torch.empty(sum(lens), device=dev, dtype=torch.float32)
        ll, ii = (C.c_longlong * k)(*offs), (C.c_int * k)(*lens)
        E.check(self.lib.tt_fmt_run(self.h, E.ptr(wav), ll, ii, (C.c_int * k)(*idx), k, E.ptr(y), ll, E.stream_ptr()))
        return [y[o:o + n] for o, n in zip(offs, lens)]


class DenoiseStage(_ClipStage):
    """Stationary-noise reduction of voice clips by spectral subtraction (csrc/denoise.hip, include/tortoise_mi355x_nr.h): ragged batches,
    each clip in auto or region mode, one tt_nr_run call per max_clips clips, every clip's samples and floor bit-identical to running it
    alone.  Sample-rate agnostic: regions arrive as frames (denoise.region_frames)."""

    api, noun, what, nr = "tt_nr", "denoiser's", "denoise", nr
    least, least_text = nr.MIN_SAMPLES, f"{nr.MIN_SAMPLES} samples (the frames are centred with reflect padding)"

    def __init__(self, max_samples, max_clips=E.NR_MAX_CLIPS, device="cuda"):
        super().__init__(max_samples, max_clips, device, extra=None)
        self.t = {k: v.to(self.device).contiguous() for k, v in nr.tables().items()}
        c = E.NrConfig()
        c.n_fft, c.hop, c.bins_pad, c.max_samples, c.max_clips = nr.N_FFT, nr.HOP, nr.BINS_PAD, self.max_samples, self.max_clips
        tb = E.NrTables()
        tb.basis, tb.inverse = E.ptr(self.t["basis"]), E.ptr(self.t["inverse"])
        self._create(C.byref(c), C.byref(tb))

    def denoise_many(self, clips, regions, params):
        """clips f32 [n] (device or host, n >= 513), one (first frame, frames) each ((0, 0): auto) and one denoise.Params for all -> one
        (y f32 [n] on the stage's device, dict(status=E.NR_OK / NR_SHORT, floor=f32 [513] on the host)) per clip.  ValueError for a clip
        the handle does not take or a region outside its clip."""
        if len(clips) != len(regions):
            raise ValueError(f"{len(clips)} clips with {len(regions)} noise regions")
        for i, (x, (first, count)) in enumerate(zip(clips, regions)):
            self._check_clip(i, x)
            T = self.nr.frames(x.shape[0])
            if count and not (count >= E.NR_MIN_REGION and 0 <= first <= T - count):
                raise ValueError(f"clip {i}: noise region of frames {first} .. {first + count} in a clip of {T} (at least {E.NR_MIN_REGION}, inside the clip)")
        return self._run(clips, regions, params=params)

    def _group(self, clips, regions, params):
        k, dev = len(clips), self.device
        lens = [int(x.shape[0]) for x in clips]
        offs = self._offsets(lens)
        wav = self._audio(clips)
        y = torch.empty(offs[-1] + 1, device=dev, dtype=torch.float32)
        floor = torch.empty(k, self.nr.BINS_PAD, device=dev, dtype=torch.float32)
        ll, status = (C.c_longlong * k)(*offs[:k]), (C.c_int * k)()
        p = self.nr.c_params(params)
        E.check(self.lib.tt_nr_run(self.h, E.ptr(wav), ll, (C.c_int * k)(*lens), (C.c_int * k)(*[r[0] for r in regions]),
                                   (C.c_int * k)(*[r[1] for r in regions]), C.byref(p), k, E.ptr(y), ll, E.ptr(floor), status, E.stream_ptr()))
        fl = floor[:, :self.nr.BINS].cpu()  # (synchronises)
        return [(y[o:o + n], dict(status=int(status[i]), floor=fl[i].clone())) for i, (o, n) in enumerate(zip(offs, lens))]


class LoudnessStage(_ClipStage):
    """Integrated loudness, true peak and the gain to a target under a ceiling (csrc/loudness.hip, include/tortoise_mi355x_loud.h): ragged
    batches, each clip with its own target and ceiling, one tt_loud_measure / tt_loud_normalize call per group of at most max_clips clips and
    max_total_samples samples, every clip's result bit-identical to running it alone."""

    api, noun, what, capacity = "tt_loud", "loudness stage's", "loudness", "max_total_samples"

    def __init__(self, max_total_samples, max_clips=16, device="cuda"):
        super().__init__(max_total_samples, max_clips, device)

    def measure_many(self, clips):
        """clips f32 [n_i] (device or host) -> one dict per clip: status (E.LOUD_OK / SHORT / SILENT), lufs, true_peak (linear), blocks_abs,
        blocks_rel, hop_energy (f64 host tensor).  ValueError for an empty clip or a clip beyond the handle."""
        return [r for _, r in self._many(clips, None, None, E.LOUD_NONE)]

    def normalize_many(self, clips, targets, ceilings, mode):
        """clips, a target (LUFS) and a ceiling (linear true peak) each, one mode (E.LOUD_NONE / SCALE / LOOKAHEAD_MODE) -> one (y f32 [n_i] on
        the stage's device, dict) per clip: measure_many's entries plus gain and out_true_peak (linear)."""
        if not len(clips) == len(targets) == len(ceilings):
            raise ValueError(f"{len(clips)} clips with {len(targets)} targets and {len(ceilings)} ceilings")
        if mode not in (E.LOUD_NONE, E.LOUD_SCALE, E.LOUD_LOOKAHEAD_MODE):
            raise ValueError(f"mode {mode}: expected E.LOUD_NONE, E.LOUD_SCALE or E.LOUD_LOOKAHEAD_MODE")
        for i, (T, c) in enumerate(zip(targets, ceilings)):
            if not math.isfinite(float(T)) or not (float(c) > 0 and math.isfinite(float(c))):
                raise ValueError(f"clip {i}: target {T} LUFS / ceiling {c} (a finite target and a positive linear ceiling)")
        return self._many(clips, [float(T) for T in targets], [float(c) for c in ceilings], mode)

    def _many(self, clips, targets, ceilings, mode):
        for i, x in enumerate(clips):
            self._check_clip(i, x)
        return self._run(clips, targets, ceilings, mode=mode)

    def _groups(self, clips):
        """The longest runs of clips the handle takes in one call: at most max_clips clips and max_total_samples samples."""
        runs, g0 = [], 0
        while g0 < len(clips):
            g1, total = g0, 0
            while g1 < len(clips) and g1 - g0 < self.max_clips and total + clips[g1].shape[0] <= self.max_total_samples:
                total += clips[g1].shape[0]
                g1 += 1
            runs.append((g0, g1))
            g0 = g1
        return runs

    def _group(self, clips, targets, ceilings, mode):
        n, dev = len(clips), self.device
        io, ho = self._offsets(x.shape[0] for x in clips), self._offsets(self.lib.tt_loud_hops(x.shape[0]) for x in clips)
        audio = self._audio(clips)
        t = _Tables(dev, io=io, ho=ho)
        r = _Results(dev, float64=dict(lufs=n, hop_energy=ho[-1]), float32=dict(true_peak=n, gain=n, out_true_peak=n),
                     int32=dict(blocks_abs=n, blocks_rel=n, status=n))
        head = (self.h, n, audio.data_ptr(), t.p("io"), t.p("ho"))
        measured = (r.p("lufs"), r.p("true_peak"), r.p("blocks_abs"), r.p("blocks_rel"), r.p("hop_energy"))
        y = None
        if targets is None:
            E.check(self.lib.tt_loud_measure(*head, *measured, r.p("status"), E.stream_ptr()))
        else:
            tc = _Tables(dev, torch.float32, target=targets, ceiling=ceilings)
            y = torch.zeros(io[-1] + 1, device=dev, dtype=torch.float32)
            E.check(self.lib.tt_loud_normalize(*head, tc.p("target"), tc.p("ceiling"), int(mode), y.data_ptr(), *measured, r.p("gain"),
                                               r.p("out_true_peak"), r.p("status"), E.stream_ptr()))
        r.cpu()
        status = self._accepted(r["status"], (E.LOUD_OK, E.LOUD_SHORT, E.LOUD_SILENT))
        lufs, true_peak, blocks_abs, blocks_rel, gain, out_true_peak = (
            r[k].tolist() for k in ("lufs", "true_peak", "blocks_abs", "blocks_rel", "gain", "out_true_peak"))
        hop_energy, out = r["hop_energy"], []
        for i in range(n):
            d = dict(status=status[i], lufs=lufs[i], true_peak=true_peak[i], blocks_abs=blocks_abs[i], blocks_rel=blocks_rel[i],
                     hop_energy=self._host(hop_energy[ho[i]:ho[i + 1]]))
            if y is not None:
                d.update(gain=gain[i], out_true_peak=out_true_peak[i])
            out.append((None if y is None else y[io[i]:io[i + 1]], d))
        return out


class ClassifierStage(_GuardedHandle):
    """The Tortoise detector (api.py classify_audio_clip: AudioMiniEncoderWithClassifierHead over one 24 kHz clip) -> the head's two
    logits and the 512-d embedding of frame 0.  The handle is re-created for a longer clip than it was built for."""

    api = "tt_cls"

    def __init__(self, sd, device="cuda", dtype=E.TT_F16, max_samples=220000):
        self.lib = E.init()
        self.device = torch.device(device)
        self.dtype = dtype
        self.w = pack.pack_classifier(sd, self.device, dtype)
        self.h = E.vp()
        self.max_samples = 0
        self._build(max_samples)

    def _build(self, max_samples):
        from .config import ClassifierConfig
        cfg = ClassifierConfig()
        self.close()
        c = E.ClsConfig()
        c.dtype, c.spec_dim, c.base_channels, c.depth, c.resnet_blocks = self.dtype, cfg.spec_dim, cfg.base_channels, cfg.depth, cfg.resnet_blocks
        c.kernel_size, c.downsample_factor, c.embedding_dim = cfg.kernel_size, cfg.downsample_factor, cfg.embedding_dim
        c.attn_blocks, c.heads, c.classes, c.max_samples = cfg.attn_blocks, cfg.heads, cfg.classes, int(max_samples)
        self._create(C.byref(c), C.byref(self.w.weights))
        self.max_samples = int(max_samples)

    def run(self, clip):
        """clip f32 [n] or [1, n] at 24 kHz (any device) -> (logits f32 [2], embedding f32 [512]) on the device."""
        x = clip.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
        n = x.shape[0]
        if n < 1:
            raise ValueError("an empty clip cannot be classified")
        if n > self.lib.tt_cls_max_samples():
            raise ValueError(f"a clip of {n} samples exceeds the classifier's index range ({self.lib.tt_cls_max_samples()} samples)")
        if n > self.max_samples:
            self._build(n)
        logits = torch.empty(2, device=self.device, dtype=torch.float32)
        emb = torch.empty(512, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_cls_run(self.h, E.ptr(x), n, E.ptr(logits), E.ptr(emb), E.stream_ptr()))
        return logits, emb


class DiffusionStage(_GuardedHandle):
    """DiffusionTts + SpacedDiffusion.p_sample_loop (api.py:117-130)."""

    api = "tt_diff"

    def __init__(self, sd, cfg: DiffusionConfig = DiffusionConfig(), device="cuda", dtype=E.TT_BF16, max_seq=2304, max_codes=512,
                 max_steps=512, max_batch=1):
        self.lib = E.init()
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = pack.pack_diffusion(sd, cfg, self.device, dtype)
        c = E.DiffConfig()
        c.dtype, c.channels, c.heads, c.num_layers = dtype, cfg.model_channels, cfg.num_heads, cfg.num_layers
        c.in_channels, c.in_pad, c.out_channels = cfg.in_channels, self.w.in_pad, cfg.out_channels
        c.latent_channels, c.max_seq, c.max_codes, c.max_steps = cfg.in_latent_channels, max_seq, max_codes, max_steps
        c.max_batch = max_batch  # utterances one sample_many() pass may hold
        self.max_batch = max_batch
        self._create(C.byref(c), C.byref(self.w.weights))
        self.S = 0
        if os.environ.get("TT_DIFF_OVERLAP_PREPASS"):  # A/B switch of the measurement scripts
            self.set_option(E.TT_DIFF_OPT_OVERLAP_PREPASS, int(os.environ["TT_DIFF_OVERLAP_PREPASS"]))
        if os.environ.get("TT_DIFF_FUSED_GN"):
            self.set_option(E.TT_DIFF_OPT_FUSED_GN, int(os.environ["TT_DIFF_FUSED_GN"]))

    def set_option(self, option, value):
        E.check(self.lib.tt_diff_set_option(self.h, int(option), int(value)))

    def stat(self, which):
        return self.lib.tt_diff_stat(self.h, int(which))

    def condition(self, latents, cond_latent, S):
        """latents f32 [1, M, latent]; cond_latent f32 [1, 2C] (diffusion_decoder.py:232-260)."""
        lat = latents[0].to(self.device).float().contiguous()
        cond = cond_latent[0].to(self.device).float().contiguous()
        idx = torch.from_numpy(nearest_interp_index(lat.shape[0], S)).to(self.device)
        E.check(self.lib.tt_diff_condition(self.h, E.ptr(lat), lat.shape[0], E.ptr(cond), E.ptr(idx), S, E.stream_ptr()))
        self.S = S

    def code_emb(self):
        out = torch.empty(self.S, self.cfg.model_channels, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_diff_get_code_emb(self.h, E.ptr(out), E.stream_ptr()))
        return out.t()[None]  # [1, C, S] like the reference

    def forward(self, x, timestep, cond_free=True):
        """x f32 [1, 100, S] -> raw model outputs [B, 200, S] (B = 2 with cond_free: row 0 cond, row 1 uncond)."""
        if self.S <= 0:
            raise ValueError("forward() needs condition() first (after sample_many the handle holds a batch)")
        xt = x[0].to(self.device).float().t().contiguous()
        B = 2 if cond_free else 1
        out = torch.empty(B, self.S, self.cfg.out_channels, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_diff_forward(self.h, E.ptr(xt), int(timestep), int(cond_free), E.ptr(out), E.stream_ptr()))
        return out.permute(0, 2, 1)

    @staticmethod
    def _run_order_steps(sched: Schedule):
        """tt_diff_step records in the order the steps run (i = N-1 ... 0) + that order."""
        N = sched.num_timesteps
        steps = (E.DiffStep * N)()
        order = list(reversed(range(N)))
        for j, i in enumerate(order):
            st = steps[j]
            st.timestep = int(sched.timestep_map[i])
            st.min_log = sched.f32(sched.post_logvar_clipped, i)
            st.max_log = sched.f32(sched.log_betas, i)
            st.cfk = float(np.float32(sched.cond_free_k * (1 - i / N)))
            st.sqrt_recip = sched.f32(sched.sqrt_recip_ac, i)
            st.sqrt_recipm1 = sched.f32(sched.sqrt_recipm1_ac, i)
            st.coef1 = sched.f32(sched.coef1, i)
            st.coef2 = sched.f32(sched.coef2, i)
            st.nonzero = 0.0 if i == 0 else 1.0
        return steps, order

    def sample(self, sched: Schedule, x_T, step_noise):
        """x_T f32 [1, 100, S]; step_noise f32 [N, 1, 100, S] with step_noise[i] the draw of spaced index i
        (same convention as the oracle).  Returns the denormalised mel [1, 100, S]."""
        if self.S <= 0:
            raise ValueError("sample() needs condition() first (after sample_many the handle holds a batch)")
        N = sched.num_timesteps
        steps, order = self._run_order_steps(sched)
        x = x_T[0].to(self.device).float().contiguous()
        noise = step_noise.to(self.device).float()[order, 0].contiguous()  # run order
        mel = torch.empty(self.cfg.in_channels, self.S, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_diff_sample(self.h, E.ptr(x), E.ptr(noise), steps, N, int(sched.cond_free), E.ptr(mel), E.stream_ptr()))
        return mel[None]

    def sample_many(self, sched: Schedule, items):
        """Several utterances through one denoiser pass per step (tt_diff_sample_batch).  items: list of
        (latents f32 [1, M_u, latent], cond_latent f32 [1, 2C], S_u, x_T f32 [1, 100, S_u], step_noise f32 [N, 1, 100, S_u]); all of them
        walk `sched`.  Returns the list of denormalised mels [1, 100, S_u].  Each utterance is treated exactly as if it ran alone
        (its own statistics / attention span / zero padding); only the accumulation grouping of the GroupNorm partial sums
        differs from sample(), i.e. results agree within the operand tolerance, not bit for bit."""
        U = len(items)
        if not 1 <= U <= self.max_batch:
            raise ValueError(f"{U} utterances exceed this stage's batch capacity {self.max_batch}")
        N = sched.num_timesteps
        steps, order = self._run_order_steps(sched)
        S_pad = max(int(it[2]) for it in items)
        E.check(self.lib.tt_diff_batch_begin(self.h, U, S_pad, E.stream_ptr()))
        keep = []
        for u, (lat, cond, S, x_T, noise) in enumerate(items):
            lat_ = lat[0].to(self.device).float().contiguous()
            cond_ = cond[0].to(self.device).float().contiguous()
            idx = torch.from_numpy(nearest_interp_index(lat_.shape[0], S)).to(self.device)
            E.check(self.lib.tt_diff_condition_slot(self.h, u, E.ptr(lat_), lat_.shape[0], E.ptr(cond_), E.ptr(idx), int(S), E.stream_ptr()))
            x = x_T[0].to(self.device).float().contiguous()
            nz = noise.to(self.device).float()[order, 0].contiguous()
            mel = torch.empty(self.cfg.in_channels, int(S), device=self.device, dtype=torch.float32)
            keep.append((lat_, cond_, idx, x, nz, mel))
        arr = lambda k: (C.c_void_p * U)(*[E.ptr(t[k]) for t in keep])
        E.check(self.lib.tt_diff_sample_batch(self.h, U, arr(3), arr(4), steps, N, int(sched.cond_free), arr(5), E.stream_ptr()))
        self.S = 0  # the handle holds a batch: condition() again before sample()
        return [t[5][None] for t in keep]

    # ---- deterministic solvers (include/tortoise_mi355x_solver.h; solver.SolverPlan) ---------------------------
    @staticmethod
    def _solver_steps(plan):
        """tt_solver_step records in the order the steps run (i = M-1 ... 0)."""
        M = plan.n_steps
        steps = (E.SolverStep * M)()
        for j, i in enumerate(reversed(range(M))):
            st = steps[j]
            st.timestep = int(plan.timestep_map[i])
            st.cfk = plan.f32(plan.cfk, i)
            st.sqrt_recip = plan.f32(plan.sqrt_recip, i)
            st.sqrt_recipm1 = plan.f32(plan.sqrt_recipm1, i)
            st.a, st.b, st.c = plan.f32(plan.a, i), plan.f32(plan.b, i), plan.f32(plan.c, i)
        return steps

    def solve_stat(self, which):
        return self.lib.tt_diff_solve_stat(self.h, int(which))

    def solve(self, plan, x_T):
        """The plan's solver from x_T f32 [1, 100, S]: no noise is drawn after x_T.  Returns the denormalised mel [1, 100, S]."""
        if self.S <= 0:
            raise ValueError("solve() needs condition() first (after sample_many / solve_many the handle holds a batch)")
        x = x_T[0].to(self.device).float().contiguous()
        mel = torch.empty(self.cfg.in_channels, self.S, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_diff_solve(self.h, E.ptr(x), self._solver_steps(plan), plan.n_steps, int(plan.cond_free), E.ptr(mel), E.stream_ptr()))
        return mel[None]

    def solve_many(self, plan, items):
        """sample_many with the plan's solver (tt_diff_solve_batch): the same item tuples, whose noise entry may be None and is ignored.
        Returns the list of denormalised mels [1, 100, S_u]; each agrees with solve() alone within the operand tolerance, as sample_many
        does with sample()."""
        U = len(items)
        if not 1 <= U <= self.max_batch:
            raise ValueError(f"{U} utterances exceed this stage's batch capacity {self.max_batch}")
        S_pad = max(int(it[2]) for it in items)
        E.check(self.lib.tt_diff_batch_begin(self.h, U, S_pad, E.stream_ptr()))
        keep = []
        for u, (lat, cond, S, x_T, _) in enumerate(items):
            lat_ = lat[0].to(self.device).float().contiguous()
            cond_ = cond[0].to(self.device).float().contiguous()
            idx = torch.from_numpy(nearest_interp_index(lat_.shape[0], S)).to(self.device)
            E.check(self.lib.tt_diff_condition_slot(self.h, u, E.ptr(lat_), lat_.shape[0], E.ptr(cond_), E.ptr(idx), int(S), E.stream_ptr()))
            x = x_T[0].to(self.device).float().contiguous()
            mel = torch.empty(self.cfg.in_channels, int(S), device=self.device, dtype=torch.float32)
            keep.append((lat_, cond_, idx, x, mel))
        arr = lambda k: (C.c_void_p * U)(*[E.ptr(t[k]) for t in keep])
        E.check(self.lib.tt_diff_solve_batch(self.h, U, arr(3), self._solver_steps(plan), plan.n_steps, int(plan.cond_free), arr(4), E.stream_ptr()))
        self.S = 0  # the handle holds a batch: condition() again before solve()
        return [t[4][None] for t in keep]

    # ---- split sampling: this engine evaluates ONE denoiser row per step ---------------------
    def split_begin(self, sched: Schedule, x_T, step_noise, row):
        """row 0 = conditioned, 1 = conditioning-free.  Keeps the run-order noise and the output buffers alive."""
        if not sched.cond_free:
            raise ValueError("split sampling needs conditioning_free (two rows per step)")
        if self.S <= 0:
            raise ValueError("split sampling needs condition() first (the handle holds no single-utterance conditioning)")
        steps, order = self._run_order_steps(sched)
        x = x_T[0].to(self.device).float().contiguous()
        self._split_noise = step_noise.to(self.device).float()[order, 0].contiguous()
        self._split_mel = torch.empty(self.cfg.in_channels, self.S, device=self.device, dtype=torch.float32)
        self._split_row = torch.empty(self.S, self.cfg.out_channels, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_diff_split_begin(self.h, E.ptr(x), steps, sched.num_timesteps, int(row), E.stream_ptr()))
        torch.cuda.current_stream().synchronize()  # `x` and `steps` are consumed
        return sched.num_timesteps

    def split_forward(self):
        """This engine's model row of the current step: f32 [S, out_channels] (valid until the next call)."""
        E.check(self.lib.tt_diff_split_forward(self.h, E.ptr(self._split_row), E.stream_ptr()))
        return self._split_row

    def split_update(self, rows):
        """rows f32 [2, S, out_channels]: row 0 conditioned, row 1 conditioning-free (from both participants)."""
        assert rows.shape == (2, self.S, self.cfg.out_channels) and rows.is_contiguous() and rows.dtype == torch.float32
        E.check(self.lib.tt_diff_split_update(self.h, E.ptr(rows), E.ptr(self._split_noise), E.ptr(self._split_mel), E.stream_ptr()))

    def split_end(self):
        E.check(self.lib.tt_diff_split_end(self.h))
        mel = self._split_mel[None]
        self._split_noise = self._split_row = self._split_mel = None
        return mel

    def sample_split(self, sched: Schedule, x_T, step_noise, row, exchange):
        """p_sample_loop with the two rows on two participants.  `exchange(rows, mine)` fills rows[r] with
        participant r's `mine` (an all_gather over the pair, tortoise_tts_amd/dist.py)."""
        n = self.split_begin(sched, x_T, step_noise, row)
        rows = torch.empty(2, self.S, self.cfg.out_channels, device=self.device, dtype=torch.float32)
        for _ in range(n):
            exchange(rows, self.split_forward())
            self.split_update(rows)
        return self.split_end()


class ConditioningStage(_Handle):
    """Conditioning encoders of the voice_samples path on the device (csrc/cond.hip):
    UnifiedVoice.get_conditioning (ConditioningEncoder, autoregressive.py:204-228, 444-452) and
    DiffusionTts.get_conditioning (contextual_embedder, diffusion_decoder.py:186-192, 222-230).  Inputs are the mel
    spectrograms api.py:271-289 builds from the clips; the per-clip results are combined exactly as the reference does."""

    api = "tt_cond"

    def __init__(self, sd_ar, sd_diff, ar_cfg, diff_cfg, device="cuda", dtype=E.TT_BF16, max_frames=1024):
        self.lib = E.init()
        self.device = torch.device(device)
        self.ar_cfg, self.diff_cfg = ar_cfg, diff_cfg
        self.w = pack.pack_conditioning(sd_ar, sd_diff, ar_cfg, diff_cfg, self.device, dtype)
        sh = self.w.shape
        c = E.CondConfig()
        c.dtype = dtype
        c.ar_dim, c.ar_heads, c.ar_blocks = ar_cfg.model_dim, ar_cfg.heads, sh["ar_blocks"]
        c.ar_mel, c.ar_mel_pad = sh["ar_mel"], sh["mel_pad"]
        c.diff_channels, c.diff_heads, c.diff_blocks = sh["diff_channels"], sh["diff_heads"], sh["diff_blocks"]
        c.diff_mel, c.diff_mel_pad = sh["diff_mel"], sh["mel_pad"]
        c.max_frames = max_frames
        self.cfg = c
        self._create(C.byref(c), C.byref(self.w.weights))

    def _clips(self, mels, n_mel):
        """Accepts [1, n_clips, n_mel, T] (the reference's stacked tensor) or a list of [1, n_mel, T] / [n_mel, T] clips."""
        if torch.is_tensor(mels):
            mels = [mels[0, j] for j in range(mels.shape[1])] if mels.dim() == 4 else [mels]
        out = []
        for m in mels:
            m = m.to(self.device).float()
            m = m.reshape(-1, m.shape[-1]) if m.dim() == 3 else m
            if m.shape[0] != n_mel:
                raise ValueError(f"conditioning clip has {m.shape[0]} mel channels, the encoder takes {n_mel}")
            out.append(m.contiguous())
        if not out:
            raise ValueError("no conditioning clips")
        return out

    def auto_latent(self, mels):
        """mels f32 [1, n_clips, 80, T] (or a list of clips) -> f32 [1, model_dim]: mean over the clips of h[:, :, 0]."""
        clips = self._clips(mels, self.cfg.ar_mel)
        acc = torch.zeros(self.cfg.ar_dim, device=self.device, dtype=torch.float32)
        out = torch.empty(self.cfg.ar_dim, device=self.device, dtype=torch.float32)
        for m in clips:
            E.check(self.lib.tt_cond_ar_clip(self.h, E.ptr(m), m.shape[1], E.ptr(out), E.stream_ptr()))
            acc += out
        return (acc / len(clips))[None]

    def diffusion_latent(self, mels):
        """mels f32 [1, n_clips, 100, T] (or a list of clips) -> f32 [1, 2 * model_channels]: the clips' embedder outputs
        concatenated along time and averaged."""
        clips = self._clips(mels, self.cfg.diff_mel)
        C2 = 2 * self.cfg.diff_channels
        acc = torch.zeros(C2, device=self.device, dtype=torch.float32)
        out = torch.empty(C2, device=self.device, dtype=torch.float32)
        total = 0
        for m in clips:
            frames = C.c_int(0)
            E.check(self.lib.tt_cond_diff_clip(self.h, E.ptr(m), m.shape[1], E.ptr(out), C.byref(frames), E.stream_ptr()))
            acc += out
            total += frames.value
        return (acc / total)[None]


def mel_front_end_kind(value):
    """The mel_front_end= argument of the TextToSpeech classes: 'torch' (audio.MelFrontEnd, the default) or 'device' (MelFrontStage)."""
    if value not in ("torch", "device"):
        raise ValueError(f"mel_front_end={value!r}: 'torch' (audio.MelFrontEnd) or 'device' (stages.MelFrontStage)")
    return value


class MelFrontStage:
    """The wav -> mel front-end of the voice_samples path (api.py:271-287) on the device (csrc/melfront.hip, include/tortoise_mi355x_mel.h):
    what audio.MelFrontEnd computes through torch.stft / F.conv1d / torch.matmul.  Two tt_mel handles - the autoregressive mel (80 HTK mels
    of the 22.05 kHz clip, power spectrum, log / mel_norms) and the diffusion mel (100 Slaney mels of the clip resampled to 24 kHz and
    clamped, magnitude spectrum, log) - and one 147 -> 160 resampler.  Pad, crop, pad-or-truncate and the random crop start stay on the
    host exactly as audio.MelFrontEnd does them, so a caller's RNG stream is consumed identically on both paths.  The log mel is multiplied
    by the f32 reciprocal of mel_norms where the reference divides: one more rounding (2^-24 relative) than audio.MelFrontEnd."""

    def __init__(self, models_dir=None, mel_norms=None, device="cuda", max_clips=E.MEL_MAX_CLIPS):
        from . import audio
        if mel_norms is None:  # (before the library: a missing file is reported on any machine)
            path = audio.find_mel_norms(models_dir)
            if path is None:
                raise FileNotFoundError("mel_norms.pth (tortoise/data/, arch_util.py:290) was not found: pass models_dir= or mel_norms=, "
                                        "or give get_conditioning_latents ready (auto_mel, diffusion_mel) pairs")
            mel_norms = torch.load(path, map_location="cpu")
        self.mel_norms = torch.as_tensor(mel_norms).float()
        self.lib = E.init()
        self.device = torch.device(device)
        self.max_clips = int(max_clips)
        self.holder, self.t = pack.pack_melfront(self.mel_norms, self.device)
        self.auto_samples, self.diff_samples = audio.AUTO_COND_SAMPLES, audio.DIFF_COND_SAMPLES
        self.h_auto, self.h_diff, self.h_rs = E.vp(), E.vp(), E.vp()
        self.h_auto = self._mel_handle(80, 2, 0, self.t["fb_auto"], self.t["scale_auto"], self.auto_samples)
        self.h_diff = self._mel_handle(100, 1, 1, self.t["fb_diff"], None, self.diff_samples)
        taps = self.t["taps"]
        self.rs_new, self.rs_orig, self.rs_width = taps.shape[0], taps.shape[1] - 2 * self.t["width"], self.t["width"]
        # output j < diff_samples reads no input beyond (diff_samples / new) * orig + taps: a longer clip is cut there before the resampler
        self.rs_max_in = -(-self.diff_samples // self.rs_new) * self.rs_orig + taps.shape[1]
        E.check(self.lib.tt_mel_resampler_create(E.ptr(taps), self.rs_orig, self.rs_new, self.rs_width, self.rs_max_in, C.byref(self.h_rs)))

    def _mel_handle(self, n_mels, power, clamp, fb, scale, max_samples):
        c = E.MelConfig()
        c.n_fft, c.hop, c.n_mels, c.bins_pad, c.power, c.clamp_input = pack.MEL_N_FFT, pack.MEL_HOP, n_mels, pack.MEL_BINS_PAD, power, clamp
        c.floor, c.max_samples, c.max_clips = 1e-5, max_samples, self.max_clips
        t = E.MelTables()
        t.basis, t.fb, t.scale = E.ptr(self.t["basis"]), E.ptr(fb), E.ptr(scale)
        h = E.vp()
        E.check(self.lib.tt_mel_create(C.byref(c), C.byref(t), C.byref(h)))
        return h

    def close(self):
        if self.h_auto:
            self.lib.tt_mel_destroy(self.h_auto)
        if self.h_diff:
            self.lib.tt_mel_destroy(self.h_diff)
        if self.h_rs:
            self.lib.tt_mel_resampler_destroy(self.h_rs)
        self.h_auto, self.h_diff, self.h_rs = E.vp(), E.vp(), E.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _auto_clip(self, clip, start=None):
        """format_conditioning's pad / crop (audio.MelFrontEnd.auto_mel): -> f32 [auto_samples] on the device."""
        clip = clip.float().reshape(1, -1)
        gap = clip.shape[-1] - self.auto_samples
        if gap < 0:
            clip = F.pad(clip, (0, -gap))
        elif gap > 0:
            s = int(torch.randint(0, gap + 1, (1,))) if start is None else int(start)
            clip = clip[:, s:s + self.auto_samples]
        return clip.reshape(-1).to(self.device).contiguous()

    def resample(self, clip):
        """f32 [n] at 22.05 kHz -> f32 [ceil(160 n / 147)] at 24 kHz (torchaudio.functional.resample) on the device."""
        x = clip.float().reshape(-1).to(self.device).contiguous()
        n = x.shape[0]
        if not 1 <= n <= self.rs_max_in:
            raise ValueError(f"a clip of {n} samples is outside the resampler's range (1 .. {self.rs_max_in})")
        out = torch.empty(self.lib.tt_mel_resampled_length(self.h_rs, n), device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_mel_resample(self.h_rs, E.ptr(x), n, E.ptr(out), E.stream_ptr()))
        return out

    def _diff_clip(self, clip):
        """resample 22050 -> 24000, pad or truncate (audio.MelFrontEnd.diffusion_mel): -> f32 [diff_samples] on the device."""
        from .audio import pad_or_truncate
        x = clip.float().reshape(-1)
        if x.shape[0] < 1:
            raise ValueError("an empty clip has no mel spectrogram")
        return pad_or_truncate(self.resample(x[:self.rs_max_in]), self.diff_samples)

    def _run(self, h, n_mels, clips):
        """clips: equally prepared f32 device vectors -> [1, n_mels, T] each, max_clips of them per ragged call."""
        out = []
        for i in range(0, len(clips), self.max_clips):
            part = clips[i:i + self.max_clips]
            k = len(part)
            wav = torch.cat(part) if k > 1 else part[0]
            lens = [int(p.shape[0]) for p in part]
            frames = [self.lib.tt_mel_frames(h, n) for n in lens]
            offs, ooffs, a, b = [], [], 0, 0
            for n, T in zip(lens, frames):
                offs.append(a)
                ooffs.append(b)
                a, b = a + n, b + n_mels * T
            mel = torch.empty(b, device=self.device, dtype=torch.float32)
            E.check(self.lib.tt_mel_run(h, E.ptr(wav), (C.c_longlong * k)(*offs), (C.c_int * k)(*lens), k, E.ptr(mel), (C.c_longlong * k)(*ooffs),
                                        E.stream_ptr()))
            out += [mel[o:o + n_mels * T].reshape(1, n_mels, T) for o, T in zip(ooffs, frames)]
        return out

    def auto_many(self, clips):
        """-> [auto_mel f32 [1, 80, 517]] of every clip, one ragged call (the fast path needs no diffusion mel)."""
        return self._run(self.h_auto, 80, [self._auto_clip(c) for c in clips])

    def many(self, clips):
        """-> [(auto_mel f32 [1, 80, 517], diffusion_mel f32 [1, 100, 401])] of every clip: one ragged call per handle."""
        clips = list(clips)
        auto = self._run(self.h_auto, 80, [self._auto_clip(c) for c in clips])
        diff = self._run(self.h_diff, 100, [self._diff_clip(c) for c in clips])
        return list(zip(auto, diff))

    def auto_mel(self, clip, start=None):
        return self._run(self.h_auto, 80, [self._auto_clip(clip, start)])[0]

    def diffusion_mel(self, clip):
        return self._run(self.h_diff, 100, [self._diff_clip(clip)])[0]

    def __call__(self, clip):
        return self.many([clip])[0]


class RandomLatentStage:
    """get_random_conditioning_latents (api.py:301-309): the two RandomLatentConverter MLPs as six M = 1 GEMMs each.
    EqualLinear's constants are folded at pack time: leaky_relu is positively homogeneous, so
    leaky_relu(x W^T s + b l) * sqrt2 == leaky_relu(x (W s sqrt2)^T + b l sqrt2)."""

    def __init__(self, sd_auto, sd_diffuser, device="cuda", dtype=E.TT_BF16, lr_mul=0.1):
        self.lib = E.init()
        self.device = torch.device(device)
        self.dtype = dtype
        self.h = pack.Holder(self.device, dtype)
        self.nets = []
        for sd in (sd_auto, sd_diffuser):
            C_ = sd["layers.0.weight"].shape[0]
            scale = (1.0 / np.sqrt(C_)) * lr_mul * np.sqrt(2.0)
            layers = [(self.h.op(sd[f"layers.{i}.weight"].float() * scale), self.h.f32(sd[f"layers.{i}.bias"].float() * (lr_mul * np.sqrt(2.0))))
                      for i in range(5)]
            layers.append((self.h.op(sd["layers.5.weight"]), self.h.f32(sd["layers.5.bias"])))
            self.nets.append((C_, layers))
        self.channels = tuple(n[0] for n in self.nets)

    def _run(self, net, r):
        C_, layers = net
        x = r.to(self.device).float().reshape(1, C_).to(self.h.tdtype).contiguous()
        out = None
        for i, (w, b) in enumerate(layers):
            last = i == len(layers) - 1
            nxt = None if last else torch.empty(1, C_, device=self.device, dtype=self.h.tdtype)
            out = torch.empty(1, C_, device=self.device, dtype=torch.float32) if last else None
            E.check(self.lib.tt_op_gemm(self.dtype, E.ptr(x), C_, E.ptr(w), C_, 1, C_, C_, 1, 0, 1, E.ptr(b),
                                        E.ACT_NONE if last else E.ACT_LRELU, None, E.ptr(out), E.ptr(nxt), E.stream_ptr()))
            x = nxt
        return out

    def latents(self, r_auto, r_diffuser):
        """r_auto f32 [1, 1024], r_diffuser f32 [1, 2048] standard-normal draws -> (auto latent, diffusion latent)."""
        return self._run(self.nets[0], r_auto), self._run(self.nets[1], r_diffuser)


class HifiganStage(_Handle):
    """HiFi-GAN decoder of the streaming path (csrc/hifigan.hip): hifi_decoder.inference(gpt_latents,
    auto_conditioning) of api_fast.py:420 / 517 (hifigan_decoder.py:259-289)."""

    api = "tt_hifi"

    def __init__(self, sd_folded, cfg, device="cuda", dtype=E.TT_BF16, max_latents=512):
        self.lib = E.init()
        self.device = torch.device(device)
        self.cfg = cfg
        self.w = pack.pack_hifigan(sd_folded, cfg, self.device, dtype)
        c = E.HifiConfig()
        c.dtype = dtype
        c.in_channels, c.cond_channels, c.initial_channel = cfg.in_channels, cfg.cond_channels, cfg.upsample_initial_channel
        c.num_stages = len(cfg.upsample_factors)
        for i, u in enumerate(cfg.upsample_factors):
            c.up_factor[i] = u
        c.num_kernels = len(cfg.resblock_kernel_sizes)
        for i, k in enumerate(cfg.resblock_kernel_sizes):
            c.kernel_size[i] = k
        c.num_dilations = len(cfg.resblock_dilation_sizes)
        for i, d in enumerate(cfg.resblock_dilation_sizes):
            c.dilation[i] = d
        c.lrelu_slope = cfg.lrelu_slope
        c.max_latents = max_latents
        self.c = c
        self._create(C.byref(c), C.byref(self.w.weights))

    def inference(self, latents, g):
        """latents f32 [1, T, in_channels], g f32 [1, cond_channels] -> wav f32 [1, 1, frames * hop] (on the device)."""
        lat = latents.to(self.device).float().reshape(-1, self.cfg.in_channels).contiguous()
        gv = g.to(self.device).float().reshape(-1).contiguous()
        T = lat.shape[0]
        n = self.lib.tt_hifi_output_frames(T) * self.cfg.hop
        wav = torch.empty(n, device=self.device, dtype=torch.float32)
        ns = C.c_int(0)
        E.check(self.lib.tt_hifi_run(self.h, E.ptr(lat), T, E.ptr(gv), E.ptr(wav), C.byref(ns), E.stream_ptr()))
        assert ns.value == n, (ns.value, n)
        return wav[None, None]

    # a padded batch may carry this many idle slot rows beyond a quarter of its real ones (interpolated frames; about 15 latents)
    _PAD_ALLOWANCE = 64

    def batch_groups(self, lengths):
        """Index groups (each one tt_hifi_run_batch call) for sequences of `lengths` latents: longest first, a sequence joins the open
        group while the group fits the handle (n * (longest frames + 1) <= tt_hifi_batch_capacity, n <= TT_HIFI_MAX_BATCH) and its
        padding stays within a quarter of the real rows plus _PAD_ALLOWANCE - so one long sequence is not padded against many short ones."""
        cap = self.lib.tt_hifi_batch_capacity(self.h)
        frames = [self.lib.tt_hifi_output_frames(int(T)) + 1 for T in lengths]
        groups, cur, real = [], [], 0
        for i in sorted(range(len(lengths)), key=lambda i: (-frames[i], i)):
            if cur:
                slot = frames[cur[0]]
                n = len(cur) + 1
                if n > E.HIFI_MAX_BATCH or n * slot > cap or n * slot > 1.25 * (real + frames[i]) + self._PAD_ALLOWANCE:
                    groups.append(cur)
                    cur, real = [], 0
            cur.append(i)
            real += frames[i]
        if cur:
            groups.append(cur)
        return groups

    def inference_many(self, items):
        """items: list of (latents f32 [1, T_i, in_channels], g f32 [1, cond_channels]) -> list of wav f32 [1, 1, frames_i * hop] on the
        device, in order.  Each wav is bit-identical to inference() of that item alone (csrc/hifigan.hip: one ragged batched pass per
        group of batch_groups)."""
        lats = [lat.to(self.device).float().reshape(-1, self.cfg.in_channels) for lat, _ in items]
        gs = [g.to(self.device).float().reshape(-1) for _, g in items]
        lengths = [int(x.shape[0]) for x in lats]
        out = [None] * len(items)
        for grp in self.batch_groups(lengths):
            lat = torch.cat([lats[i] for i in grp], 0).contiguous()
            gv = torch.stack([gs[i] for i in grp], 0).contiguous()
            ns = [self.lib.tt_hifi_output_frames(lengths[i]) * self.cfg.hop for i in grp]
            wav = torch.empty(sum(ns), device=self.device, dtype=torch.float32)
            ln = (C.c_int * len(grp))(*[lengths[i] for i in grp])
            E.check(self.lib.tt_hifi_run_batch(self.h, len(grp), E.ptr(lat), ln, E.ptr(gv), E.ptr(wav), E.stream_ptr()))
            off = 0
            for i, n in zip(grp, ns):
                out[i] = wav[off:off + n][None, None]
                off += n
        return out


class VocoderStage(_GuardedHandle):
    """UnivNetGenerator.inference (vocoder.py:300-312)."""

    api = "tt_voc"

    def __init__(self, sd_folded, cfg: VocoderConfig = VocoderConfig(), device="cuda", dtype=E.TT_BF16, max_frames=2304):
        self.lib = E.init()
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = pack.pack_vocoder(sd_folded, cfg, self.device, dtype)
        c = E.VocConfig()
        c.dtype, c.max_frames, c.mel_channels, c.mel_pad = dtype, max_frames, cfg.n_mel_channels, self.w.mel_pad
        self._create(C.byref(c), C.byref(self.w.weights))

    def inference(self, mel, z):
        """mel f32 [1, 100, S]; z f32 [1, 64, S+10] -> audio [1, 1, S*256]."""
        m = mel[0].to(self.device).float().contiguous()
        S = m.shape[1]
        zz = z[0].to(self.device).float().contiguous()
        assert zz.shape == (self.cfg.noise_dim, S + 10)
        audio = torch.empty(S * self.cfg.hop_length, device=self.device, dtype=torch.float32)
        E.check(self.lib.tt_voc_run(self.h, E.ptr(m), S, E.ptr(zz), E.ptr(audio), E.stream_ptr()))
        return audio.clamp(-1, 1)[None, None]

    # a padded batch may carry this many idle slot frames beyond a quarter of its real ones
    _PAD_ALLOWANCE = 64

    def batch_groups(self, lengths):
        """Index groups (each one tt_voc_run_batch call) for mels of `lengths` frames - the rule of HifiganStage.batch_groups: longest
        first, a sequence joins the open group while the group fits the handle (n * (longest S + 10) <= tt_voc_batch_capacity,
        n <= TT_VOC_MAX_BATCH) and its padding stays within a quarter of the real frames plus _PAD_ALLOWANCE."""
        cap = self.lib.tt_voc_batch_capacity(self.h)
        frames = [int(S) + 10 for S in lengths]
        groups, cur, real = [], [], 0
        for i in sorted(range(len(lengths)), key=lambda i: (-frames[i], i)):
            if cur:
                slot = frames[cur[0]]
                n = len(cur) + 1
                if n > E.VOC_MAX_BATCH or n * slot > cap or n * slot > 1.25 * (real + frames[i]) + self._PAD_ALLOWANCE:
                    groups.append(cur)
                    cur, real = [], 0
            cur.append(i)
            real += frames[i]
        if cur:
            groups.append(cur)
        return groups

    def inference_many(self, items):
        """items: list of (mel f32 [1, 100, S_i], z f32 [1, 64, S_i + 10]) -> list of audio f32 [1, 1, S_i * 256] on the device, in
        order, clamped like inference().  Each clip is bit-identical to inference() of that item alone (csrc/vocoder.hip: one ragged
        batched pass per group of batch_groups)."""
        mels = [mel[0].to(self.device).float().contiguous() for mel, _ in items]
        zs = [z[0].to(self.device).float().contiguous() for _, z in items]
        lengths = [int(m.shape[1]) for m in mels]
        for zz, S in zip(zs, lengths):
            assert zz.shape == (self.cfg.noise_dim, S + 10)
        out = [None] * len(items)
        for grp in self.batch_groups(lengths):
            n = len(grp)
            audio = [torch.empty(lengths[i] * self.cfg.hop_length, device=self.device, dtype=torch.float32) for i in grp]
            arr = lambda ts: (C.c_void_p * n)(*[E.ptr(t) for t in ts])
            ln = (C.c_int * n)(*[lengths[i] for i in grp])
            E.check(self.lib.tt_voc_run_batch(self.h, n, arr([mels[i] for i in grp]), ln, arr([zs[i] for i in grp]), arr(audio), E.stream_ptr()))
            for i, a in zip(grp, audio):
                out[i] = a.clamp(-1, 1)[None, None]
        return out
