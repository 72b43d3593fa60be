"""stages.F0Stage backed by tests/f0_reference.py: what the host flow of f0() / shift_pitch(to_hz=) / tts(pitch_hz=) runs on without a GPU."""
import numpy as np

from tests import f0_reference as R


class ReferenceF0Stage:
    made = []
    calls = []

    def __init__(self, max_samples, max_clips=16, device="cpu"):
        self.max_samples, self.max_clips = max_samples, max_clips
        ReferenceF0Stage.made.append(max_samples)

    def track_many(self, clips, params, dprime=False):
        ReferenceF0Stage.calls.append(len(clips))
        out = []
        for x, p in zip(clips, params):
            assert x.dim() == 1 and 1 <= x.shape[0] <= self.max_samples
            tr = R.track(x.cpu().numpy(), p.lag_lo, p.lag_hi, p.thr, p.floor_e)
            out.append(dict(lag=tr["lag"].astype(np.int32), f0=tr["f0"].astype(np.float32), aper=tr["aper"].astype(np.float32),
                            n_voiced=int(tr["voiced"].sum())))
        return out

    def close(self):
        pass


def install(monkeypatch, api):
    monkeypatch.setattr(api.stages, "F0Stage", ReferenceF0Stage, raising=False)
    ReferenceF0Stage.made, ReferenceF0Stage.calls = [], []
    return ReferenceF0Stage
