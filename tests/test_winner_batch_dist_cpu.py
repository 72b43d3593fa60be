"""World-size-2 `gloo` run of tts(k=3) on a winner_batch=2 instance with candidate sharding (CPU stand-ins): rank 0 batches its round-robin
share (winners 0 and 2), rank 1 renders winner 1 alone, and rank 0 ends up with the three clips of the one-rank serial run."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dist_cpu import _free_port
from tests.test_winner_batch_cpu import KW, TEXT, BatchingVocoderStage, install, make, same
from tortoise_tts_amd import dist as tdist


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    tdist.init_from_env()
    mp_ = pytest.MonkeyPatch()
    try:
        api = install(mp_)
        t, lat = make(api, winner_batch=2)
        assert (t.rank, t.world) == (rank, world)
        with torch.no_grad():
            got = t.tts(TEXT, conditioning_latents=lat, k=3, **KW)
        torch.save({"clips": got, "batched": getattr(t.diffusion, "batched", []), "many": list(BatchingVocoderStage.calls),
                    "singles": len(BatchingVocoderStage.singles)}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        mp_.undo()
    tdist.barrier()
    dist.destroy_process_group()


@torch.no_grad()
def test_each_rank_batches_its_round_robin_share(tmp_path, monkeypatch):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["batched"] == [2] and [len(c) for c in r0["many"]] == [2]   # winners 0 and 2 in one pass / one call
    assert r1["batched"] == [] and r1["many"] == [] and r1["singles"] == 1  # winner 1 alone: today's single path
    assert r1["clips"] is None
    api = install(monkeypatch)
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=3, **KW)
    assert same(r0["clips"], want)
