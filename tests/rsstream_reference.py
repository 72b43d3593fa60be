"""What the CPU and GPU tests of the streaming resampler (include/tortoise_mi355x_rss.h) share: the emission rule by brute force, seeded
chunkings, an fp64 stream built on tests/resample_reference.py, and a fake of stages.StreamResampleStage for host-flow tests.

Nothing here is tuned: the ratios and the clip are resample_reference's, and a streamed sample is held to the whole-clip value."""
import numpy as np

from tests import resample_reference as R

HIST = 576                                                                   # TT_RSS_HIST
RATIOS = R.RATIOS + R.EXTREME_RATIOS + ((147, 160), (160, 147), (320, 147), (3, 4))
LENGTHS = (1, 2, 37, 300, 1000, 5000)
BANK_MAX = 16384                                                             # TT_RSS_BANK_MAX


def half_width(P, Q):
    return R.half_width(R.cutoff_q(P, Q))


def bank_fits(P, Q):
    return Q * (2 * half_width(P, Q) + 2) <= BANK_MAX


def ready_brute(n, P, Q, flush=False):
    """How many outputs m = 0, 1, ... have every tap (the last one is floor(m P / Q) + H + 1) below n; flush: all ceil(n Q / P)."""
    if flush:
        return R.out_samples(n, P, Q)
    H, m = half_width(P, Q), 0
    while (m * P) // Q + H + 1 <= n - 1:
        m += 1
    return m


def chunk_sizes(P, Q):
    H = half_width(P, Q)
    return (0, 1, 2, 5, 37, H, H + 1, 2 * H + 1, 2 * H + 2, 1023, 1025, 4000)


def chunking(n, P, Q, seed):
    """A seeded split of n samples into chunks drawn from chunk_sizes (the last one cut to fit; zero-length chunks stay in)."""
    rng = np.random.default_rng(seed)
    sizes, out, left = chunk_sizes(P, Q), [], n
    while left > 0:
        c = min(int(sizes[rng.integers(len(sizes))]), left)
        out.append(c)
        left -= c
    return out


class Fp64Stream:
    """The stream restated on resample_reference.resample: a push sees only the last HIST inputs and the chunk (everything older is
    replaced by zeros), filters that as a clip, and keeps the outputs that became ready."""

    def __init__(self, P, Q):
        self.P, self.Q, self.H = P, Q, half_width(P, Q)
        self.n, self.m = 0, 0
        self.hist = np.zeros(HIST)

    def push(self, chunk, flush=False):
        chunk = np.asarray(chunk, dtype=np.float64)
        n_end = self.n + len(chunk)
        have = n_end if flush else n_end - self.H - 1
        ready = R.out_samples(have, self.P, self.Q) if have > 0 else 0
        y = np.zeros(0)
        if ready > self.m:
            seen = np.concatenate([np.zeros(max(self.n - HIST, 0)), self.hist[max(HIST - self.n, 0):], chunk])
            assert len(seen) == n_end
            y = R.resample(seen, self.P, self.Q, bound=False)[0][self.m:ready]
        self.hist = np.concatenate([self.hist, chunk])[-HIST:]
        self.n, self.m = n_end, ready
        return y


def whole_hold(x, P, Q):
    """The fake stage's "filter": output m is input floor(m P / Q) plus m / 1024 (a value that names its own index)."""
    n_out = R.out_samples(len(x), P, Q)
    m = np.arange(n_out)
    return (np.asarray(x, dtype=np.float32)[(m * P) // Q] + (m / 1024.0).astype(np.float32)).astype(np.float32)


class FakeStreamResampleStage:
    """stages.StreamResampleStage on the host: the real emission rule (resample.stream_ready), whole_hold as the filter."""

    made = []

    def __init__(self, max_streams=16, form="auto", device="cpu"):
        self.max_streams, self.form, self.slots, self.calls = int(max_streams), form, {}, []
        FakeStreamResampleStage.made.append(self)

    def open(self, P, Q):
        from tortoise_tts_amd import resample as rs
        P, Q = rs.check_ratio(P, Q)
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError("all resampling streams are open")
        self.slots[free[0]] = dict(P=P, Q=Q, x=np.zeros(0, np.float32), m=0, finished=False)
        return free[0]

    def close(self, slot=None):
        if slot is not None:
            self.slots.pop(slot, None)

    def push_many(self, items):
        import torch
        from tortoise_tts_amd import resample as rs
        assert 1 <= len(items) <= self.max_streams and len({s for s, _, _ in items}) == len(items)
        self.calls.append([(s, int(x.shape[0]), bool(f)) for s, x, f in items])
        out = []
        for slot, x, flush in items:
            st = self.slots[slot]
            assert not st["finished"]
            c = rs.stream_ready(len(st["x"]), x.shape[0], st["P"], st["Q"], flush)
            st["x"] = np.concatenate([st["x"], x.detach().cpu().numpy().astype(np.float32).reshape(-1)])
            padded = np.concatenate([st["x"], np.zeros(HIST, np.float32)])  # (outputs not yet ready are not looked at)
            out.append(torch.from_numpy(whole_hold(padded, st["P"], st["Q"])[st["m"]:st["m"] + c].copy()))
            st["m"] += c
            st["finished"] = bool(flush)
        return out
