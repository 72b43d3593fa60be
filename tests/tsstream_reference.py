"""What the CPU and GPU tests of the streaming time-stretch (include/tortoise_mi355x_tss.h) share: the rule by brute force, the chunkings,
an fp64 stream that keeps only what a device slot keeps (the last HIST inputs and the template) built on tests/tsm_reference.py, and a fake
of stages.StreamStretchStage for host-flow tests.

Nothing here is tuned: the constants, the clip family and the reference are tsm_reference's, and a streamed sample is held to the
whole-clip value."""
import numpy as np

from tests import tsm_reference as T

LOOK = 2 * T.SEARCH - 1 + T.HS + T.W - T.SEARCH                             # TT_TSS_LOOK: frame k reads x[a_k - 256 .. a_k + LOOK)
REGION = 2 * T.SEARCH - 1 + T.HS + T.W                                      # 1663
HIST = 1664                                                                  # TT_TSS_HIST
LENGTHS = (1, 300, 1406, 1407, 1408, 1663, 5000, 9001)
RATES = T.RATES
CYCLE = (1, 383, 1407, 0, 1663, 4096)
RQS_8 = (32768, 32769, 52429, 65536, 65537, 81920, 131071, 131072)           # eight rates including both ends
RQS_11 = RQS_8 + (40000, 65535, 100000)


def done_brute(n, rq):
    """The frames k = 1, 2, ... whose whole region x[a_k - 256 .. a_k - 256 + 1663) lies below n."""
    k = 0
    while T.nominal(k + 1, rq) - T.SEARCH + REGION <= n:
        k += 1
    return k


def frames_total(n, rq, flush):
    if flush:
        return T.frames(n, rq) - 1 if n >= 1 else 0
    return done_brute(n, rq)


def ready_total(n, rq, flush):
    if flush:
        return T.out_samples(n, rq) if n >= 1 else 0
    return done_brute(n, rq) * T.HS


def chunkings(n, seed):
    """(chunks, flush with the last chunk?) of a clip of n samples: whole, the cycle, seeded draws; the flush with and without a last chunk."""
    yield [n], True
    yield [n], False
    cyc, left = [], n
    for k in range(10 ** 6):
        if left == 0:
            break
        c = min(CYCLE[k % len(CYCLE)], left)
        cyc.append(c)
        left -= c
    yield cyc, False
    rng = np.random.default_rng(seed)
    sizes, out, left = (0, 1, 2, 383, 384, 385, 1406, 1407, 1408, 1663, 1664, 3000), [], n
    while left > 0:
        c = min(int(sizes[rng.integers(len(sizes))]), left)
        out.append(c)
        left -= c
    yield out, True


class Fp64Stream:
    """The stream restated in fp64 with a device slot's state: a push sees the last HIST inputs, the chunk and the template the previous
    frame left, and nothing else (everything older is replaced by NaN: a read of it would poison the result)."""

    def __init__(self, rq):
        self.rq = rq
        self.n = self.frames = self.m = 0
        self.hist = np.zeros(HIST)
        self.tpl = np.zeros(T.W)
        self.w = T.window()
        self.reach = 0  # the deepest read behind the push's first sample

    def push(self, chunk, flush=False):
        """-> (samples, offsets) the push emits."""
        chunk = np.asarray(chunk, dtype=np.float64)
        rq, n_prev, n_end = self.rq, self.n, self.n + len(chunk)
        k0, k1 = self.frames + 1, frames_total(n_end, rq, flush)
        m1 = ready_total(n_end, rq, flush)
        seen = np.concatenate([np.full(max(n_prev - HIST, 0), np.nan), self.hist[max(HIST - n_prev, 0):], chunk])
        assert len(seen) == n_end
        y, offs = np.zeros(max(k1 - k0 + 1, 0) * T.HS), []
        for k in range(k0, k1 + 1):
            a = T.nominal(k, rq)
            region = T.take(seen, a - T.SEARCH, REGION)
            self.reach = max(self.reach, n_prev - max(a - T.SEARCH, 0))
            assert flush or a + LOOK <= n_end
            if k == 1:
                self.tpl = region[T.SEARCH:T.SEARCH + T.W].copy()  # x[0 .. W)
                offs.append(0)
            win = np.lib.stride_tricks.sliding_window_view(region[:T.W + 2 * T.SEARCH - 1], T.W)
            s = (win @ self.tpl) / np.sqrt((win * win).sum(axis=1) + T.EPS)
            d = T.pick(s)
            offs.append(d)
            cs = d + T.SEARCH
            y[(k - k0) * T.HS:(k - k0 + 1) * T.HS] = self.w[T.HS:] * self.tpl[:T.HS] + self.w[:T.HS] * region[cs:cs + T.HS]
            self.tpl = region[cs + T.HS:cs + T.HS + T.W].copy()
        self.hist = np.concatenate([self.hist, chunk])[-HIST:]
        out = y[:m1 - self.m]
        self.n, self.frames, self.m = n_end, max(k1, self.frames), m1
        return out, np.array(offs, dtype=np.int32)


def stream_fp64(x, rq, chunks, last_with_flush):
    """x in `chunks` through an Fp64Stream -> (y, offsets, deepest reach)."""
    st, ys, offs, at = Fp64Stream(rq), [], [], 0
    assert sum(chunks) == len(x)
    for i, c in enumerate(chunks):
        y, o = st.push(x[at:at + c], last_with_flush and i == len(chunks) - 1)
        ys.append(y), offs.append(o)
        at += c
    if not (last_with_flush and chunks):
        y, o = st.push(x[:0], True)
        ys.append(y), offs.append(o)
    return np.concatenate(ys), np.concatenate(offs), st.reach


def whole_hold(x, rq):
    """The fake stage's "stretch": output m is input min(floor(m rq / 65536), n - 1) plus m / 4096 (a value that names its own index)."""
    x = np.asarray(x, dtype=np.float32)
    m = np.arange(T.out_samples(len(x), rq))
    return (x[np.minimum((m * rq) >> 16, len(x) - 1)] + (m / 4096.0).astype(np.float32)).astype(np.float32)


class FakeStreamStretchStage:
    """stages.StreamStretchStage on the host: the real emission rule (stretch.stream_ready), whole_hold as the stretch."""

    made = []

    def __init__(self, max_streams=16, device="cpu"):
        self.max_streams, self.slots, self.calls = int(max_streams), {}, []
        FakeStreamStretchStage.made.append(self)

    def open(self, rq):
        rq = int(rq)
        if not T.RATE_MIN <= rq <= T.RATE_MAX:
            raise ValueError(f"rate {rq} / 65536 is outside the supported range [0.5, 2.0]")
        free = [s for s in range(self.max_streams) if s not in self.slots]
        if not free:
            raise RuntimeError("all time-stretch streams are open")
        self.slots[free[0]] = dict(rq=rq, x=np.zeros(0, np.float32), m=0, finished=False)
        return free[0]

    def close(self, slot=None):
        if slot is not None:
            self.slots.pop(slot, None)

    def push_many(self, items, return_offsets=False):
        import torch
        from tortoise_tts_amd import stretch as tsm
        assert 1 <= len(items) <= self.max_streams and len({s for s, _, _ in items}) == len(items)
        self.calls.append([(s, int(x.shape[0]), bool(f)) for s, x, f in items])
        out, offs = [], []
        for slot, x, flush in items:
            st = self.slots[slot]
            assert not st["finished"]
            c = tsm.stream_ready(len(st["x"]), x.shape[0], st["rq"], flush)
            k = tsm.stream_offsets(len(st["x"]), x.shape[0], st["rq"], flush)
            st["x"] = np.concatenate([st["x"], x.detach().cpu().numpy().astype(np.float32).reshape(-1)])
            if c:  # (before a flush every ready output's input exists: m rq / 65536 < a_done + 768 < n)
                m = np.arange(st["m"], st["m"] + c)
                idx = (m * st["rq"]) >> 16
                assert flush or idx.max() < len(st["x"])
                y = st["x"][np.minimum(idx, len(st["x"]) - 1)] + (m / 4096.0).astype(np.float32)
            else:
                y = np.zeros(0, np.float32)
            out.append(torch.from_numpy(y.astype(np.float32)))
            offs.append(torch.zeros(k, dtype=torch.int32))
            st["m"] += c
            st["finished"] = bool(flush)
        return (out, offs) if return_offsets else out
