"""Several streaming sessions in one decode batch (TT_AR_OPT_SESSIONS): per-token step time with 1 .. 4 running sessions, aggregate
tokens per second, and the first-piece latency of a session admitted while three others run.

    python scripts/stream_sessions.py [--dtype bf16] [--tokens 120] [--out profiles/r07_stream_sessions.json]
    python scripts/stream_sessions.py --per-session [--rounds 3] [--only typical_and_full_sort] [--out ...]
    python scripts/stream_sessions.py --wide [--rounds 3] [--only wide16] [--out profiles/r09_wide_sessions.json]

--per-session: four sessions on a handle with per-session sampling (TT_AR_OPT_SESSION_SAMPLING), per-token step time for four sessions
with the default settings, four different fast-path settings, and a mix with one typical and one full-sort row; the configurations
alternate for --rounds rounds, so each one's spread is measured against the same drift.  --only runs one of them (e.g. under a tracer).

--wide: the wide session handle (TT_AR_OPT_SESSIONS = 2, 16 rows) at 1, 4, 8, 12 and 16 running sessions, alternated with the 4-row
handle at 4 sessions and the max_batch = 1 handle for --rounds rounds; then the first-piece latency of a session admitted while 15 others
run, and the share of stream_pieces' wall time spent in the per-piece HiFi-GAN re-decodes for 16 sessions of 500 tokens.

Full-size synthetic weights with the stop token suppressed (every session runs its whole length).  Warm-up steps are excluded from
every timing; the single-stream figure is the max_batch = 1 handle of api_fast.tts_stream on the same weights."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tokens", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--per-session", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    if args.per_session:
        return per_session(args)
    if args.wide:
        return wide(args)
    from oracle import make_golden_full as GF
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    cfg = ARConfig()
    dt = E.dtype_code(args.dtype)
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg)
    text, auto, _ = GF.prompt()
    N, warm = args.tokens, 20
    res = {"dtype": args.dtype, "timed_tokens": N, "warmup_tokens": warm, "device": torch.cuda.get_device_name(0)}

    single = stages.ArStage(sd, cfg, dtype=dt, max_batch=1, max_text=80, max_new_tokens=warm + N + 8, max_latent_candidates=1)
    single.prefill(auto, text)
    for c, _ in single.generate_stream(1, warm + N, warm, first_chunk=warm, seed=1):
        if c.shape[1] == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
    torch.cuda.synchronize()
    res["single_handle_step_ms"] = (time.perf_counter() - t0) / N * 1e3
    single.close()

    st = stages.ArStage(sd, cfg, dtype=dt, max_batch=4, max_text=80, max_new_tokens=warm + N + 8, max_latent_candidates=1, sessions=True)
    res["sessions"] = {}
    for k in range(1, 5):
        for r in range(k):
            st.admit(r, auto, text, 10 + r)
        st.advance(warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, _ = st.advance(N)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        assert n[:k] == [warm + N] * k, n
        res["sessions"][k] = {"step_ms": dt_s / N * 1e3, "tokens_per_s": k * N / dt_s}
        for r in range(k):
            st.close(r)
    res["graph_captures"] = st.stat(0)
    st.close()
    one = res["sessions"][1]
    res["speedup_4_vs_1_tokens_per_s"] = res["sessions"][4]["tokens_per_s"] / one["tokens_per_s"]
    res["step_4_vs_single_handle"] = res["sessions"][4]["step_ms"] / res["single_handle_step_ms"]

    h_cfg = HifiganConfig()
    sds = {"autoregressive": sd, "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    tts = TextToSpeech(state_dicts=sds, dtype=args.dtype, max_mel_tokens=200, kv_cache=True, max_streams=4)
    lat = []
    for trial in range(3):
        for i in range(3):
            tts.open_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=i + 10 * trial)
        pieces = tts.stream_pieces()
        next(pieces)  # the three running sessions are past their first buffer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sid = tts.open_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=99 + trial)
        for s, wav, _ in pieces:
            if s == sid:
                wav.cpu()
                lat.append(time.perf_counter() - t0)
                break
        for _ in pieces:
            pass
    res["first_piece_latency_ms_with_three_running"] = [x * 1e3 for x in lat]
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


PER_SESSION = {
    "default4": [{}, {}, {}, {}],
    "fast4": [{}, dict(temperature=0.5, top_p=0.95, repetition_penalty=1.0), dict(top_k=1, repetition_penalty=1.3),
              dict(temperature=1.0, top_p=1.0, top_k=100)],
    "typical_and_full_sort": [{}, dict(typical_mass=0.9), dict(top_k=0), {}],
}


def per_session(args):
    from oracle import make_golden_full as GF
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.config import ARConfig
    cfg = ARConfig()
    dt = E.dtype_code(args.dtype)
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg)
    text, auto, _ = GF.prompt()
    N, warm = args.tokens, 20
    names = [args.only] if args.only else list(PER_SESSION)
    res = {"dtype": args.dtype, "timed_tokens": N, "warmup_tokens": warm, "device": torch.cuda.get_device_name(0), "settings": PER_SESSION,
           "step_ms": {k: [] for k in names}}
    st = stages.ArStage(sd, cfg, dtype=dt, max_batch=4, max_text=80, max_new_tokens=warm + N + 8, max_latent_candidates=1, sessions=True,
                        per_session_sampling=True)
    for _ in range(args.rounds):
        for name in names:
            for r, own in enumerate(PER_SESSION[name]):
                st.admit(r, auto, text, 10 + r, **own)
            st.advance(warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n, _ = st.advance(N)
            torch.cuda.synchronize()
            assert n == [warm + N] * 4, n
            res["step_ms"][name].append((time.perf_counter() - t0) / N * 1e3)
            res.setdefault("launches_per_step", {})[name] = st.stat(2)
            for r in range(4):
                st.close(r)
    res["graph_captures"] = st.stat(0)
    st.close()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


WIDE = {"wide1": 1, "wide4": 4, "wide8": 8, "wide12": 12, "wide16": 16, "narrow4": 4, "single": 1}


def wide(args):
    from oracle import make_golden_full as GF
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    from tortoise_tts_amd import weights as W
    from tortoise_tts_amd.api_fast import TextToSpeech
    from tortoise_tts_amd.config import ARConfig, HifiganConfig
    cfg = ARConfig()
    dt = E.dtype_code(args.dtype)
    sd = W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(cfg), 1234), cfg)
    text, auto, _ = GF.prompt()
    N, warm = args.tokens, 20
    names = [args.only] if args.only else list(WIDE)
    res = {"dtype": args.dtype, "timed_tokens": N, "warmup_tokens": warm, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "running_sessions": {k: WIDE[k] for k in names}, "step_ms": {k: [] for k in names}}
    mk = dict(dtype=dt, max_text=80, max_new_tokens=warm + N + 8, max_latent_candidates=1)
    handles = {}
    if any(k.startswith("wide") for k in names):
        handles["wide"] = stages.ArStage(sd, cfg, max_batch=16, sessions=True, **mk)
    if "narrow4" in names:
        handles["narrow"] = stages.ArStage(sd, cfg, max_batch=4, sessions=True, **mk)
    if "single" in names:
        handles["single"] = stages.ArStage(sd, cfg, max_batch=1, **mk)
    for _ in range(args.rounds):
        for name in names:
            k = WIDE[name]
            if name == "single":
                st = handles["single"]
                st.prefill(auto, text)
                for c, _ in st.generate_stream(1, warm + N, warm, first_chunk=warm, seed=1):
                    if c.shape[1] == warm:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                torch.cuda.synchronize()
                res["step_ms"][name].append((time.perf_counter() - t0) / N * 1e3)
                continue
            st = handles["narrow" if name == "narrow4" else "wide"]
            for r in range(k):
                st.admit(r, auto, text, 10 + r)
            st.advance(warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n, _ = st.advance(N)
            torch.cuda.synchronize()
            res["step_ms"][name].append((time.perf_counter() - t0) / N * 1e3)
            assert n[:k] == [warm + N] * k, n
            for r in range(k):
                st.close(r)
    res["graph_captures"] = {h: st.stat(0) for h, st in handles.items() if h != "single"}
    for st in handles.values():
        st.close()
    res["tokens_per_s"] = {k: WIDE[k] * 1e3 / min(v) for k, v in res["step_ms"].items()}
    if "wide16" in names and "narrow4" in names:
        res["wide16_vs_narrow4_tokens_per_s"] = res["tokens_per_s"]["wide16"] / res["tokens_per_s"]["narrow4"]
    if args.only:
        print(json.dumps(res, indent=1))
        return

    h_cfg = HifiganConfig()
    sds = {"autoregressive": sd, "hifidecoder": W.synthetic_state_dict(W.hifigan_manifest(h_cfg), 1238)}
    tts = TextToSpeech(state_dicts=sds, dtype=args.dtype, max_mel_tokens=500, kv_cache=True, max_streams=16, wide_sessions=True)
    lat = []
    for trial in range(3):
        for i in range(15):
            tts.open_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=i + 100 * trial)
        pieces = tts.stream_pieces()
        next(pieces)  # the fifteen running sessions are past their first buffer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sid = tts.open_stream(text, conditioning_latents=(auto,), max_mel_tokens=200, use_deterministic_seed=99 + trial)
        for s, wav, _ in pieces:
            if s == sid:
                wav.cpu()
                lat.append(time.perf_counter() - t0)
                break
        for _ in pieces:
            pass
    res["first_piece_latency_ms_with_fifteen_running"] = [x * 1e3 for x in lat]

    # the per-piece HiFi-GAN re-decodes (every latent so far, api_fast.py:405-420) inside stream_pieces: 16 sessions of 500 tokens
    hifi, inference = [0.0, 0], tts.hifi_decoder.inference

    def timed(*a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = inference(*a, **kw)
        torch.cuda.synchronize()
        hifi[0] += time.perf_counter() - t
        hifi[1] += 1
        return out
    tts.hifi_decoder.inference = timed
    for i in range(16):
        tts.open_stream(text, conditioning_latents=(auto,), max_mel_tokens=500, use_deterministic_seed=200 + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_pieces = sum(1 for _ in tts.stream_pieces())
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tts.hifi_decoder.inference = inference
    res["stream_pieces_16x500"] = {"wall_s": wall, "hifigan_s": hifi[0], "hifigan_calls": hifi[1], "pieces": n_pieces, "hifigan_share": hifi[0] / wall,
                                   "ar_graph_captures": tts.ar.stat(0)}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
