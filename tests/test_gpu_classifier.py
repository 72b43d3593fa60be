"""The Tortoise detector on the MI355X (csrc/classify.hip, include/tortoise_mi355x_classify.h): its new kernels against torch fp32 / fp64,
the whole model with synthetic weights at the reference architecture against the transcription (tests/classifier_reference.py), and
api.classify_audio_clip end to end."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import classifier_reference as R
from tests import w2v_reference
from tortoise_tts_amd import api
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 1234
TOL = {E.TT_F32: 1e-4, E.TT_F16: 5e-3, E.TT_BF16: 3e-2}
TDT = {E.TT_F32: torch.float32, E.TT_F16: torch.float16, E.TT_BF16: torch.bfloat16}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _sd():
    return W.synthetic_state_dict(W.classifier_manifest(), seed=SEED)


def _clip(n, seed=0):
    x = w2v_reference.test_clip(n / 24000.0 + 1e-3, seed=seed)[:, :n]
    assert x.shape[1] == n
    return x.contiguous()


def _gn_stats(x, groups=16):
    # x [L][C] -> mean / biased var per group (torch.group_norm's statistics), float64
    L, C = x.shape
    g = x.double().reshape(L, groups, C // groups).permute(1, 0, 2).reshape(groups, -1)
    return g.mean(1), g.var(1, unbiased=False)


@torch.no_grad()
@pytest.mark.parametrize("dtype", [E.TT_F32, E.TT_F16, E.TT_BF16])
def test_narrow_conv_matches_torch(dtype):
    lib = E.init()
    gen = torch.Generator().manual_seed(7)
    for cin, stride in ((32, 1), (64, 1), (32, 4), (64, 4)):
        cout = cin if stride == 1 else 2 * cin
        w = torch.randn(cout, cin, 5, generator=gen) / (5 * cin) ** 0.5
        b = 0.1 * torch.randn(cout, generator=gen)
        gamma = 1 + 0.1 * torch.randn(cin, generator=gen)
        beta = 0.1 * torch.randn(cin, generator=gen)
        wp = w.permute(0, 2, 1).contiguous().to(DEV, TDT[dtype])
        for L in (1, 5, 1023, 1024, 1025, 24000, 220000):
            x = (0.5 + torch.randn(L, cin, generator=gen)).contiguous()
            res = torch.randn(L, cout, generator=gen) if stride == 1 else None
            Lout = L if stride == 1 else (L + 3) // 4
            xd = x.to(DEV)
            stats = torch.empty(32, device=DEV)
            if stride == 1:  # the statistics of x through the kernel's own finaliser, from torch's sums per 128-row block
                blocks = (L + 127) // 128
                xp = F.pad(x.double(), (0, 0, 0, blocks * 128 - L)).reshape(blocks, 128, 16, cin // 16)
                part = torch.stack([xp.sum((1, 3)), (xp * xp).sum((1, 3))], dim=-1).contiguous().to(DEV)
                E.check(lib.tt_op_cls_stats(part.data_ptr(), blocks, L, cin, stats.data_ptr(), E.stream_ptr()))
                mean, var = _gn_stats(x)
                st = stats.cpu().reshape(16, 2).double()
                assert torch.allclose(st[:, 0], mean, rtol=1e-5, atol=1e-6)
                assert torch.allclose(st[:, 1], 1 / (var + 1e-5).sqrt(), rtol=1e-5)
                inp = F.silu(F.group_norm(x.double().t()[None], 16, gamma.double(), beta.double(), eps=1e-5))
            else:
                inp = x.double().t()[None]
            want = F.conv1d(inp, w.double(), b.double(), stride=stride, padding=2)[0].t()
            if res is not None:
                want = want + res.double()
            out = torch.empty(Lout, cout, device=DEV)
            part = torch.empty(lib.tt_op_cls_workspace(Lout), dtype=torch.uint8, device=DEV) if cout <= 64 else None
            gd, bd, biasd = gamma.to(DEV), beta.to(DEV), b.to(DEV)  # (kept alive until the launch has run)
            resd = None if res is None else res.to(DEV)
            E.check(lib.tt_op_cls_conv(dtype, cin, cout, stride, xd.data_ptr(), L, stats.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                       wp.data_ptr(), biasd.data_ptr(), None if resd is None else resd.data_ptr(), out.data_ptr(),
                                       None if part is None else part.data_ptr(), E.stream_ptr()))
            r = _rel(out, want)
            assert r < TOL[dtype], f"cin={cin} stride={stride} L={L} dtype={dtype}: rel {r:.2e}"
            if part is not None:  # the epilogue's partials reduce to torch's statistics of the output
                s2 = torch.empty(32, device=DEV)
                E.check(lib.tt_op_cls_stats(part.data_ptr(), (Lout + 127) // 128, Lout, cout, s2.data_ptr(), E.stream_ptr()))
                mean, var = _gn_stats(out.cpu())
                st = s2.cpu().reshape(16, 2).double()
                assert torch.allclose(st[:, 0], mean, rtol=1e-4, atol=1e-5)
                assert torch.allclose(st[:, 1], 1 / (var + 1e-5).sqrt(), rtol=1e-4)


@torch.no_grad()
def test_init_conv_and_statistics():
    lib = E.init()
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(32, 1, 3, generator=gen)
    b = 0.1 * torch.randn(32, generator=gen)
    for n in (1, 2, 255, 256, 257, 220000):
        x = _clip(n, seed=n)
        want = F.conv1d(x.double()[None], w.double(), b.double(), padding=1)[0].t()
        out = torch.empty(n, 32, device=DEV)
        part = torch.empty(lib.tt_op_cls_workspace(n), dtype=torch.uint8, device=DEV)
        xd, wd, bd = x.to(DEV), w.reshape(32, 3).contiguous().to(DEV), b.to(DEV)
        E.check(lib.tt_op_cls_init(xd.data_ptr(), n, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), part.data_ptr(), E.stream_ptr()))
        assert _rel(out, want) < 1e-6
        stats = torch.empty(32, device=DEV)
        E.check(lib.tt_op_cls_stats(part.data_ptr(), (n + 255) // 256, n, 32, stats.data_ptr(), E.stream_ptr()))
        mean, var = _gn_stats(want)
        st = stats.cpu().reshape(16, 2).double()
        assert torch.allclose(st[:, 0], mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(st[:, 1], 1 / (var + 1e-5).sqrt(), rtol=1e-4)


@torch.no_grad()
@pytest.mark.parametrize("dtype", [E.TT_F32, E.TT_BF16])
def test_attention_matches_torch(dtype):
    lib = E.init()
    gen = torch.Generator().manual_seed(5)
    attn = R.QKVAttentionLegacy(4)
    for n in (1, 7, 215, 256, 1407):
        qkv = torch.randn(n, 1536, generator=gen)
        want = attn(qkv.double().t()[None])[0].t()
        for nq in (n, 1):
            out = torch.empty(n, 512, device=DEV, dtype=TDT[dtype])
            qd = qkv.to(DEV)
            E.check(lib.tt_op_cls_attention(dtype, qd.data_ptr(), n, nq, out.data_ptr(), E.stream_ptr()))
            r = _rel(out[:nq], want[:nq])
            assert r < (1e-5 if dtype == E.TT_F32 else 1e-2), f"n={n} nq={nq}: rel {r:.2e}"


@torch.no_grad()
def test_head_kernel():
    lib = E.init()
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(3, 512, generator=gen)
    w = torch.randn(2, 512, generator=gen) / 512 ** 0.5
    b = torch.randn(2, generator=gen)
    logits, emb = torch.empty(2, device=DEV), torch.empty(512, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    E.check(lib.tt_op_cls_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), logits.data_ptr(), emb.data_ptr(), E.stream_ptr()))
    assert _rel(logits, x[0].double() @ w.double().t() + b.double()) < 1e-6
    assert torch.equal(emb.cpu(), x[0])


_REF_CACHE = {}


def _reference(sd, n):
    if n not in _REF_CACHE:
        clip = _clip(n, seed=n)
        if n <= 220000:
            m = R.build(sd, torch.float64)
        else:
            m = R.build(sd, torch.float32)  # (60 s: fp32 on the host keeps the reference run short)
        _REF_CACHE[n] = (clip,) + R.forward(m, clip)
    return _REF_CACHE[n]


@torch.no_grad()
@pytest.mark.parametrize("dtype", [E.TT_F32, E.TT_F16, E.TT_BF16])
def test_whole_model_matches_transcription(dtype):
    sd = _sd()
    st = stages.ClassifierStage(sd, DEV, dtype, max_samples=24000 * 60)
    try:
        for n in (1, 1023, 1025, 220000, 24000 * 60):
            clip, lg_ref, emb_ref = _reference(sd, n)
            lg, emb = st.run(clip)
            torch.cuda.synchronize()
            re, rl = _rel(emb, emb_ref), _rel(lg, lg_ref)
            print(f"classifier dtype={dtype} n={n}: embedding rel {re:.2e} logits rel {rl:.2e}")
            assert st.guard() == 0
            assert re < TOL[dtype] and rl < TOL[dtype], f"n={n}: embedding rel {re:.2e}, logits rel {rl:.2e}"
    finally:
        st.close()


@torch.no_grad()
def test_repeatable_and_grows_capacity():
    sd = _sd()
    st = stages.ClassifierStage(sd, DEV, E.TT_F16, max_samples=1000)
    try:
        clip = _clip(220000, seed=220000)
        a = [t.clone() for t in st.run(clip)]
        assert st.max_samples == 220000  # re-created for the longer clip
        b = st.run(clip)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert st.guard() == 0
        short = _clip(900, seed=900)
        c = st.run(short)  # a shorter clip after a longer one: the guard rows past the end are cleared
        lg_ref, emb_ref = R.forward(R.build(sd), short)
        assert _rel(c[1], emb_ref) < TOL[E.TT_F16] and _rel(c[0], lg_ref) < TOL[E.TT_F16]
    finally:
        st.close()


@torch.no_grad()
def test_api_classify_audio_clip(tmp_path, monkeypatch):
    sd = _sd()
    torch.save(sd, os.path.join(str(tmp_path), "classifier.pth"))
    loads = []
    real = api._load_file
    monkeypatch.setattr(api, "_load_file", lambda d, f: loads.append(f) or real(d, f))
    clip = _clip(48000, seed=11)
    p1 = api.classify_audio_clip(clip, models_dir=str(tmp_path))
    p2 = api.classify_audio_clip(clip.to(DEV), models_dir=str(tmp_path))
    assert loads == ["classifier.pth"]  # packed once across calls
    assert p1.dim() == 0 and p1.device.type == "cpu"
    assert torch.equal(p1, p2)
    st = stages.ClassifierStage(sd, DEV, E.TT_F16)
    lg, _ = st.run(clip)
    assert torch.equal(p1, F.softmax(lg.cpu(), dim=-1)[0])
    st.close()
    lg_ref, _ = R.forward(R.build(sd), clip)
    assert abs(float(p1) - float(F.softmax(lg_ref, -1)[0])) < 5e-3
    for st in list(api._CLASSIFIERS.values()):
        st.close()
    api._CLASSIFIERS.clear()
