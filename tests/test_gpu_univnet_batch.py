"""-m gpu: ragged UnivNet batches (include/tortoise_mi355x_univnet.h, VocoderStage.inference_many).  Every sequence of a batch must
be bit-identical to inference() on it alone - bf16, fp16 and the fp32 verification mode - whatever its neighbours, its position in the
batch and the tile the KernelPredictor GEMMs pick for the batch's M; and the overflow guard still counts for a batch."""
import pytest
import torch

from oracle import make_golden as G
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import VocoderConfig

pytestmark = pytest.mark.gpu
MAX_FRAMES = 2186  # 500 mel codes + the ten pad frames: capacity 2196 padded frames per call


def _sd(cfg):
    return W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(cfg), seed=G.VOC_SEED))


def _items(cfg, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, 100, S, generator=g) * 2 - 5, torch.randn(1, cfg.noise_dim, S + 10, generator=g)) for S in lengths]


def _one_call(st):
    """Every item in ONE tt_voc_run_batch call (the stage's own grouping would split very different lengths)."""
    st.batch_groups = lambda lengths: [list(range(len(lengths)))]


@pytest.mark.parametrize("name,dt", [("bf16", E.TT_BF16), ("f16", E.TT_F16), ("f32", E.TT_F32)])
@torch.no_grad()
def test_every_sequence_of_a_batch_equals_inference_alone(name, dt):
    cfg = VocoderConfig()
    st = stages.VocoderStage(_sd(cfg), cfg, dtype=dt, max_frames=MAX_FRAMES)
    assert st.lib.tt_voc_batch_capacity(st.h) == MAX_FRAMES + 10
    # one sequence at the handle's full max_frames; two that exactly fill the budget (2 x 1098 = 2196); S = 1; mixed lengths
    lengths = [MAX_FRAMES, 1088, 1088, 1, 300, 150, 77, 513]
    items = _items(cfg, lengths, 11)
    alone = [st.inference(m, z).clone() for m, z in items]
    for a, S in zip(alone, lengths):
        assert a.shape == (1, 1, S * 256) and torch.isfinite(a).all() and float(a.abs().max()) > 0

    def check(idx, label):
        got = st.inference_many([items[i] for i in idx])
        for i, a in zip(idx, got):
            same = torch.equal(a, alone[i])
            print(f"[parity] UnivNet batch {name} {label}: S={lengths[i]} equal to inference() alone: {same}"
                  + ("" if same else f" (max_abs {float((a - alone[i]).abs().max()):.3e})"))
            assert a.shape == alone[i].shape and same, f"{name} {label}: sequence of {lengths[i]} frames differs from inference() alone"

    check([0], "n=1 at max_frames")
    check([3], "n=1 at S=1")
    # the stage's own grouping (by length, within the handle's budget): several calls
    groups = st.batch_groups(lengths)
    assert sorted(i for g in groups for i in g) == list(range(len(lengths)))
    cap = MAX_FRAMES + 10
    assert all(len(g) * (max(lengths[i] for i in g) + 10) <= cap for g in groups)
    check(list(range(len(lengths))), f"grouped {groups}")
    # forced single calls
    _one_call(st)
    check([1, 2], "two that exactly fill the budget")
    check([4, 5, 3, 6], "mixed lengths with S=1")
    check([6, 3, 5, 4], "the same clips, permuted")
    check([7, 3, 4, 6], "four slots of 523 frames (M = 2092 rows: other GEMM tiles than any of them alone)")
    with pytest.raises(E.EngineError, match="exceed the handle"):
        st.inference_many([items[1], items[2], items[3]])
    # and the handle goes back to single-sequence work
    assert torch.equal(st.inference(*items[4]), alone[4])
    st.close()


@torch.no_grad()
def test_overflow_guard_counts_for_a_batch():
    """The weights of tests/test_gpu_r5.py::test_vocoder_overflow_guard_sees_what_the_waveform_hides: an fp16 KernelPredictor operand past
    65504 (finite-arithmetic overflow).  One clean sequence and one batch per handle: 0 without the oversized bias, > 0 with it."""
    cfg = VocoderConfig()
    sd = _sd(cfg)
    items = _items(cfg, [40, 31, 18], 3)
    st = stages.VocoderStage(sd, cfg, dtype=E.TT_F16, max_frames=160)
    wav = st.inference(*items[0])
    torch.cuda.synchronize()
    assert st.guard() == 0 and bool(torch.isfinite(wav).all())
    _one_call(st)
    wavs = st.inference_many(items)
    torch.cuda.synchronize()
    assert st.guard() == 0 and all(bool(torch.isfinite(w).all()) for w in wavs)
    st.close()
    hot = {k: (v + 1e6 if "kernel_predictor.input_conv.0.bias" in k else v) for k, v in sd.items()}
    assert any("kernel_predictor.input_conv.0.bias" in k for k in sd), "the KernelPredictor's input convolution was not found: the test lost its point"
    st = stages.VocoderStage(hot, cfg, dtype=E.TT_F16, max_frames=160)
    st.inference(*items[0])
    torch.cuda.synchronize()
    one = st.guard()
    _one_call(st)
    st.inference_many(items)
    torch.cuda.synchronize()
    many = st.guard()
    print(f"[guard] vocoder with out-of-range predicted kernels: {one} workgroup(s) counted for one sequence, {many} for a batch of three")
    assert one > 0 and many > 0
    st.close()
