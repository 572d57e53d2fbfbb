"""sample_solver='dpm++' on the CFG-pair path of --cfg_split (-m gpu): two processes share cuda:0 as in tests/test_cfg_pair_gpu.py,
each runs ONE branch of a tiny T2V chunk, they exchange the flow predictions every step and both apply the fused CFG + DPM-Solver++
update with host scalars.  Both ranks end with latents bit-identical to each other and to the single-process pipeline (whose steps
run as per-step hipGraphs on the device table)."""
import datetime
import os

import pytest
import torch

from tests.test_cfg_pair_gpu import _free_port, _inputs

pytestmark = pytest.mark.gpu
STEPS = 4


def _pipe():
    from tests.test_pipeline_gpu import _setup
    pipe, *_ = _setup("t2v", steps=STEPS)
    pipe.sample_solver = "dpm++"
    return pipe


def _worker(rank, port, out_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=120))
    try:
        from mmpl_amd.handoff import CfgPair
        pipe = _pipe()
        pipe.cfg_pair, _, _ = CfgPair.build(2, "cuda:0", cfg_split=True)
        noise, _ = _inputs()
        if rank == 1:                                       # the uncond rank's own noise is overwritten by role 0's
            noise = torch.zeros_like(noise)
        torch.manual_seed(1000 + rank)
        _, lat = pipe.inference(noise.cuda(), ["a cat"], return_latents=True, decode=False)
        torch.cuda.synchronize()
        torch.save(lat.cpu(), f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def test_dpmpp_pair_matches_each_other_and_single_process(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "o")
    mp.spawn(_worker, args=(_free_port(), out), nprocs=2, join=True)
    a, b = (torch.load(f"{out}.{r}") for r in range(2))
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    pipe = _pipe()
    noise, _ = _inputs()
    torch.manual_seed(1000)
    _, lat = pipe.inference(noise.cuda(), ["a cat"], return_latents=True, decode=False)
    assert int(pipe.timesteps[0]) == 1000 and len(pipe.timesteps) == STEPS
    assert torch.equal(lat.cpu(), a)
