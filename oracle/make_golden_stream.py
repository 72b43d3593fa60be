"""TEST INFRASTRUCTURE - generates tests/golden/stream_pieces.npz: the audio pieces the reference's streaming loop
(tortoise/api_fast.py:399-420) hands out for the cases of tests/test_api_fast_cpu.py::test_stream_decode_points_follow_the_reference_loop.
The loop decodes the latents so far at the decode points below and passes every decode through handle_chunks
(api_fast.py:275-309, overlap 64 samples); the test's stand-in decoder makes sample j of a decode equal to j (256 samples per latent).

handle_chunks is taken from the reference source when the reference tree is present (TORTOISE_REFERENCE_ROOT, as in
oracle/ref_shims.py); elsewhere from tortoise_tts_amd.api_fast.TextToSpeech.handle_chunks, which
tests/test_api_fast_cpu.py::test_handle_chunks_matches_the_reference_method holds equal to it sample for sample.  Where the tree
exists, tests/test_api_fast_cpu.py::test_stream_pieces_golden_follows_the_reference_method re-derives the file from the reference.
    python -m oracle.make_golden_stream"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shims  # noqa: E402

REF = os.path.join(ref_shims.REFERENCE_ROOT, "tortoise", "api_fast.py")
OUT = os.path.join(ROOT, "tests", "golden", "stream_pieces.npz")
CASES = [(70, 5), (64, 5), (61, 40), (60, 40), (100, 40), (99, 40), (140, 40), (30, 40), (59, 20), (120, 20)]  # (latents, stream_chunk_size)
OVERLAP = 64
SAMPLES_PER_LATENT = 256


def reference_method(name):
    """A method of the reference's TextToSpeech, extracted from the source file (the module itself does not import offline)."""
    tree = ast.parse(open(REF).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TextToSpeech"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
    ns = {"torch": torch, "MODELS_DIR": None}  # (a default-argument name of __init__)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "api_fast_excerpt", "exec"), ns)
    return fn, ns[name]


def reference_decode_points(n_pairs, stream_chunk_size):
    """The reference's streaming loop (api_fast.py:399-420) restated over a generator that yields n_pairs (token, latent) pairs:
    the number of latents handed to hifi_decoder.inference at every decode, in order."""
    gen = iter(range(n_pairs))
    points, all_latents, codes_, is_end, first_buffer = [], [], [], False, 60
    while not is_end:
        try:
            all_latents.append(next(gen))
            codes_.append(0)
        except StopIteration:
            is_end = True
        if is_end or (stream_chunk_size > 0 and len(codes_) >= max(stream_chunk_size, first_buffer)):
            first_buffer = 0
            points.append(len(all_latents))
            codes_ = []
    return points


def key(n_pairs, stream_chunk_size, i):
    return f"n{n_pairs}_c{stream_chunk_size}_{i}"


def pieces(handle_chunks, n_pairs, stream_chunk_size):
    """handle_chunks(wav_gen, wav_gen_prev, wav_overlap, overlap_len) (the reference's signature without self) over the decodes."""
    out, prev, over = [], None, None
    for n in reference_decode_points(n_pairs, stream_chunk_size):
        wav = torch.arange(n * SAMPLES_PER_LATENT, dtype=torch.float32)
        chunk, prev, over = handle_chunks(wav, prev, over, OVERLAP)
        out.append(chunk.clone())
    return out


def all_pieces(handle_chunks):
    return {key(n, c, i): p.numpy() for n, c in CASES for i, p in enumerate(pieces(handle_chunks, n, c))}


def main():
    if os.path.exists(REF):
        _, ref_fn = reference_method("handle_chunks")
        fn, src = (lambda *a: ref_fn(None, *a)), REF
    else:
        from tortoise_tts_amd.api_fast import TextToSpeech
        fn, src = TextToSpeech.handle_chunks, "tortoise_tts_amd.api_fast.TextToSpeech.handle_chunks"
    np.savez_compressed(OUT, **all_pieces(fn))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; handle_chunks from", src)


if __name__ == "__main__":
    main()
