"""The Tortoise detector's host side without a GPU: the manifest against the transcription (tests/classifier_reference.py), the packed
layouts applied with torch, the header's exports and struct sizes, classify_audio_clip's argument checks and the .wav loader of the CLI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import classifier_reference as R
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ClassifierConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_manifest_equals_transcription_state_dict():
    man = W.classifier_manifest()
    ref = {k: tuple(v.shape) for k, v in R.build().state_dict().items()}
    assert dict(man) == ref
    sd = W.synthetic_state_dict(man, seed=1)
    m = R.build(sd)
    assert set(m.state_dict()) == set(sd)


def _apply_packed(sd, clip):
    """The engine's layouts applied with torch: token-major rows, convs as [out][tap][in] GEMMs over the padded input, the Downsample
    as overlapping windows of 5 rows every 4, legacy qkv rows, f32 throughout."""
    from tortoise_tts_amd import pack

    class Cap:
        def __init__(self):
            self.t = {}

    store = {}
    real_p = pack._p
    pack._p = lambda t: (store.__setitem__(len(store) + 1, t), len(store))[1] if t is not None else None
    try:
        h = pack.pack_classifier(sd, torch.device("cpu"), E.TT_F32)
    finally:
        pack._p = real_p
    w = h.weights
    T = lambda p: store[p]  # noqa: E731
    cfg = ClassifierConfig()

    def conv5(x, wp, b, stride=1):  # x [L][Cin], wp [Cout][5 Cin]
        L, cin = x.shape
        xp = F.pad(x, (0, 0, 2, 2 + 4))
        Lout = L if stride == 1 else (L + 3) // 4
        win = torch.stack([xp[stride * t: stride * t + 5].reshape(-1) for t in range(Lout)]) if Lout < 4096 else \
            xp.unfold(0, 5, stride)[:Lout].permute(0, 2, 1).reshape(Lout, -1)
        return win @ wp.t() + b

    def gn(x, g, b, groups):
        return F.group_norm(x.t()[None], groups, g, b, eps=1e-5)[0].t()

    x = clip.reshape(-1)
    wi = T(w.w_init)
    x = F.conv1d(x[None, None], wi[:, None, :], T(w.b_init), padding=1)[0].t()
    C = 32
    for lv in range(cfg.depth):
        groups = 16 if C <= 64 else 32
        for r in range(cfg.resnet_blocks):
            rb = w.res[lv][r]
            hh = conv5(F.silu(gn(x, T(rb.gn1_g), T(rb.gn1_b), groups)), T(rb.w1), T(rb.b1))
            x = x + conv5(F.silu(gn(hh, T(rb.gn2_g), T(rb.gn2_b), groups)), T(rb.w2), T(rb.b2))
        x = conv5(x, T(w.w_down[lv]), T(w.b_down[lv]), stride=4)
        C *= 2
    x = F.silu(gn(x, T(w.final_g), T(w.final_b), 32)) @ T(w.w_final).t() + T(w.b_final)
    for a in range(cfg.attn_blocks):
        A = w.attn[a]
        qkv = gn(x, T(A.norm_g), T(A.norm_b), 32) @ T(A.w_qkv).t() + T(A.b_qkv)
        att = R.QKVAttentionLegacy(4)(qkv.t()[None])[0].t()
        x = x + att @ T(A.w_proj).t() + T(A.b_proj)
    emb = x[0]
    return emb @ T(w.w_head).t() + T(w.b_head), emb


@torch.no_grad()
def test_packed_layouts_reproduce_transcription():
    sd = W.synthetic_state_dict(W.classifier_manifest(), seed=2)
    gen = torch.Generator().manual_seed(0)
    for n in (1, 1025, 5000):
        clip = 0.3 * torch.randn(1, n, generator=gen)
        lg, emb = _apply_packed(sd, clip)
        lg_ref, emb_ref = R.forward(R.build(sd, torch.float32), clip)
        assert torch.allclose(emb, emb_ref, rtol=1e-4, atol=1e-4)
        assert torch.allclose(lg, lg_ref, rtol=1e-4, atol=1e-4)


def test_header_symbols_and_struct_sizes():
    lib = E.load_library()
    assert lib.tt_cls_abi_version() == 1
    for i, st in enumerate(E.CLASSIFY_STRUCTS):
        assert lib.tt_cls_struct_size(i) == C.sizeof(st)
    assert lib.tt_cls_struct_size(2) == 0
    assert lib.tt_cls_max_samples() > 60 * 24000
    for name in E._CLASSIFY_PROTOS:
        assert hasattr(lib, name)
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_classify.h")).read()
    for name in E._CLASSIFY_PROTOS:
        assert name + "(" in src


def test_create_refuses_other_architecture():
    lib = E.load_library()
    c = E.ClsConfig(E.TT_F16, 1, 32, 5, 2, 5, 4, 512, 4, 4, 2, 1000)
    c.heads = 8
    h = E.vp()
    assert lib.tt_cls_create(C.byref(c), C.byref(E.ClsWeights()), C.byref(h)) != 0
    assert b"reference classifier" in lib.tt_last_error()


def test_classify_audio_clip_exists_and_refuses_bad_input(tmp_path):
    from tortoise_tts_amd import api
    from tortoise_tts_amd.api import classify_audio_clip
    with pytest.raises(ValueError):
        classify_audio_clip(torch.zeros(2, 100), models_dir=str(tmp_path))
    with pytest.raises(ValueError):
        classify_audio_clip(torch.zeros(1, 0), models_dir=str(tmp_path))
    with pytest.raises(ValueError):
        classify_audio_clip(torch.zeros(100), models_dir=str(tmp_path))
    if not torch.cuda.is_available():  # the GPU check comes before the file: a missing file is reported where a GPU exists
        with pytest.raises(E.EngineError):
            classify_audio_clip(torch.zeros(1, 100), models_dir=str(tmp_path))
    else:
        with pytest.raises(FileNotFoundError):
            classify_audio_clip(torch.zeros(1, 100), models_dir=str(tmp_path))
    assert api._CLASSIFIERS == {}


def _write_wav(path, data, sr):
    from scipy.io import wavfile
    wavfile.write(path, sr, data)


@pytest.mark.parametrize("sr", [22050, 24000])
@pytest.mark.parametrize("kind", ["int16", "float32", "int32"])
def test_cli_loader(tmp_path, sr, kind):
    from tortoise_tts_amd import is_this_from_tortoise as cli
    from tortoise_tts_amd.audio import resample_sinc
    t = np.arange(sr * 2) / sr
    x = 0.5 * np.sin(2 * np.pi * 440 * t)
    if kind == "int16":
        data, want = (x * 32767).astype(np.int16), torch.from_numpy((x * 32767).astype(np.int16).astype(np.float32)) / 32768
    elif kind == "int32":
        data, want = (x * 2 ** 30).astype(np.int32), torch.from_numpy((x * 2 ** 30).astype(np.int32).astype(np.float32)) / 2 ** 31
    else:
        data, want = x.astype(np.float32) * 1.5, torch.from_numpy(x.astype(np.float32) * 1.5)
    stereo = np.stack([data, data[::-1].copy()], axis=1)
    p = os.path.join(str(tmp_path), "c.wav")
    _write_wav(p, stereo, sr)
    got = cli.load_wav(p, 24000)
    if sr != 24000:
        want = resample_sinc(want[None], sr, 24000)[0]
    want = want.clamp(-1, 1)
    assert got.shape == (1, want.shape[0]) and got.dtype == torch.float32
    assert torch.allclose(got[0], want, atol=1e-6)
    assert float(got.abs().max()) <= 1.0
    assert got[:, : cli.CLASSIFIER_SAMPLES].shape[1] == min(cli.CLASSIFIER_SAMPLES, want.shape[0])


def test_cli_truncates_and_refuses_other_formats(tmp_path, monkeypatch):
    from tortoise_tts_amd import api
    from tortoise_tts_amd import is_this_from_tortoise as cli
    p = os.path.join(str(tmp_path), "long.wav")
    _write_wav(p, (np.random.default_rng(0).standard_normal(300000) * 1000).astype(np.int16), 24000)
    seen = []
    monkeypatch.setattr(api, "classify_audio_clip", lambda clip, models_dir: seen.append(clip.shape) or torch.tensor(0.25))
    assert float(cli.main(["--clip", p])) == 0.25
    assert seen == [(1, 220000)]
    with pytest.raises(ValueError, match=r"\.wav"):
        cli.load_wav(os.path.join(str(tmp_path), "x.mp3"))
