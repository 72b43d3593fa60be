"""stages.DenoiseStage backed by tests/denoise_reference.py, for the host-flow tests that have no GPU: the same call, the same results'
layout, every call recorded."""
import torch

from tests import denoise_reference as R
from tortoise_tts_amd import denoise as nr, engine as E

_TB = []


def reference(clip, params, region=(0, 0)):
    """-> (y f32 in the clip's shape, status, floor f32 [513])"""
    if not _TB:
        _TB.append(R.tables())
    x = clip.reshape(-1).float()
    if not region[1] and nr.frames(x.shape[0]) < E.NR_MIN_FRAMES:
        return clip.clone(), E.NR_SHORT, torch.zeros(nr.BINS)
    r = R.denoise_reference(x, _TB[0], params, region)
    return r.out.float().reshape(clip.shape), E.NR_OK, r.S.float()


class ReferenceDenoiseStage:
    made = []   # max_samples of every stage built
    calls = []  # per call: (the clips' lengths, the regions, the Params)
    log = None  # a list that gets "denoise" appended per call (the order of a flow)

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceDenoiseStage.made.append(max_samples)

    def denoise_many(self, clips, regions, params):
        ReferenceDenoiseStage.calls.append(([int(x.shape[0]) for x in clips], list(regions), params))
        if ReferenceDenoiseStage.log is not None:
            ReferenceDenoiseStage.log.append("denoise")
        out = []
        for x, reg in zip(clips, regions):
            assert x.dim() == 1 and nr.MIN_SAMPLES <= x.shape[0] <= self.max_samples
            y, status, floor = reference(x, params, reg)
            out.append((y, dict(status=status, floor=floor)))
        return out

    def close(self):
        pass


def install(monkeypatch, api):
    """api.stages.DenoiseStage -> ReferenceDenoiseStage, its records emptied"""
    monkeypatch.setattr(api.stages, "DenoiseStage", ReferenceDenoiseStage)
    ReferenceDenoiseStage.made, ReferenceDenoiseStage.calls, ReferenceDenoiseStage.log = [], [], None
    return ReferenceDenoiseStage
