"""The classifier transcription (tests/classifier_reference.py) and the manifest against the real reference classes from
$TORTOISE_REFERENCE_ROOT, and a real classifier.pth from the models directory through both paths.  Each skips when its input is absent."""
import os
import sys

import pytest
import torch

from tests import classifier_reference as R
from tortoise_tts_amd import weights as W

REF = os.environ.get("TORTOISE_REFERENCE_ROOT", "")
MODELS = os.environ.get("TORTOISE_MODELS_DIR", os.path.join(os.path.expanduser("~"), ".cache", "tortoise", "models"))


def _reference_classifier():
    if not REF or not os.path.isdir(os.path.join(REF, "tortoise")):
        pytest.skip("TORTOISE_REFERENCE_ROOT does not hold the reference tree")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from tortoise.models.classifier import AudioMiniEncoderWithClassifierHead
    return AudioMiniEncoderWithClassifierHead(2, spec_dim=1, embedding_dim=512, depth=5, downsample_factor=4, resnet_blocks=2, attn_blocks=4,
                                              num_attn_heads=4, base_channels=32, dropout=0, kernel_size=5, distribute_zero_label=False)


@torch.no_grad()
def test_transcription_matches_reference_classes():
    ref = _reference_classifier().eval()
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert shapes == dict(W.classifier_manifest())
    sd = W.synthetic_state_dict(W.classifier_manifest(), seed=4)
    ref.load_state_dict(sd)
    clip = 0.3 * torch.randn(1, 5000, generator=torch.Generator().manual_seed(1))
    want = ref(clip.unsqueeze(0))
    got, _ = R.forward(R.build(sd, torch.float32), clip)
    assert torch.allclose(got, want[0], rtol=1e-4, atol=1e-5)


@torch.no_grad()
def test_real_checkpoint_against_manifest_and_engine():
    path = os.path.join(MODELS, "classifier.pth")
    if not os.path.exists(path):
        pytest.skip(f"{path} is absent")
    sd = torch.load(path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(W.classifier_manifest())
    clip = 0.3 * torch.randn(1, 48000, generator=torch.Generator().manual_seed(2))
    lg_ref, emb_ref = R.forward(R.build(sd, torch.float64), clip)
    if not torch.cuda.is_available():
        return
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    st = stages.ClassifierStage(sd, "cuda", E.TT_F32)
    lg, emb = st.run(clip)
    st.close()
    assert float((emb.cpu().double() - emb_ref).norm() / emb_ref.norm()) < 1e-4
    assert float((lg.cpu().double() - lg_ref).norm() / lg_ref.norm()) < 1e-4
