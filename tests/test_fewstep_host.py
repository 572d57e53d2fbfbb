"""Few-step (Self-Forcing / CausVid) path, host side: the warped step list, block schedules, the causal KV slot map, the errors,
and the entry point's routing between CausalInferencePipeline and CausalFPSInferencePipeline (Wan_fps_inference_1gpu.py:59-64)."""
import os
import types

import pytest
import torch

from mmpl_amd import cli
from mmpl_amd.geometry import Geometry
from mmpl_amd.pipeline import CausalFPSInferencePipeline, CausalInferencePipeline
from mmpl_amd.scheduler import FlowMatchScheduler
from mmpl_amd.wan_wrapper import causal_slots

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DMD_KEYS = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3)


class _Gen:
    """What CausalInferencePipeline.__init__ reads from its generator (no device needed)."""

    def __init__(self, local_attn_size=-1):
        self.geometry = Geometry.named("480p")
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.engine = types.SimpleNamespace(L=30, max_frames=7)
        self.model = types.SimpleNamespace(local_attn_size=local_attn_size, num_frame_per_block=1)

    def get_scheduler(self):
        return self.scheduler


def _pipe(**kw):
    a = dict(DMD_KEYS, independent_first_frame=False, context_noise=0)
    a.update(kw)
    return CausalInferencePipeline(types.SimpleNamespace(**a), "cpu", generator=_Gen(), text_encoder=object(), vae=object())


def test_warped_step_list_matches_reference():
    p = _pipe()
    fx = torch.load(os.path.join(GOLDEN, "fewstep_t2v_tiny.pt"))
    assert p.denoising_step_list.dtype == torch.float32
    assert torch.equal(p.denoising_step_list, fx["step_list"])
    assert float(p.denoising_step_list[0]) == 1000.0 and p.generator.model.num_frame_per_block == 3
    q = _pipe(warp_denoising_step=False)
    assert q.denoising_step_list.dtype == torch.int64 and q.denoising_step_list.tolist() == [1000, 750, 500, 250]


def test_block_schedules():
    p = _pipe()
    assert p.block_schedule(21) == [3] * 7
    lat = torch.zeros(1, 3, 1, 1, 1)
    assert p.block_schedule(6, lat) == [3, 3]
    p.independent_first_frame = True
    assert p.block_schedule(22) == [1] + [3] * 7
    assert p.block_schedule(6, torch.zeros(1, 1, 1, 1, 1)) == [3, 3]
    with pytest.raises(AssertionError):
        p.block_schedule(21)                    # (21 - 1) % 3 != 0
    p.independent_first_frame = False
    with pytest.raises(AssertionError):
        p.block_schedule(22)


def test_causal_slot_map():
    # block 2 of 3 frames, nothing evicted: written at its own frames, sees every frame before its end
    assert causal_slots(6, 3, 21, 21) == ([6, 7, 8], list(range(9)), 9)
    # re-running the same block (the denoise steps / refresh): same slots
    assert causal_slots(6, 3, 21, 21, local_end=9, global_end=9) == ([6, 7, 8], list(range(9)), 9)
    assert causal_slots(0, 1, 21, 21) == ([0], [0], 1)
    # local_attn_size windows
    assert causal_slots(9, 3, 21, 6) == ([9, 10, 11], list(range(6, 12)), 12)
    assert causal_slots(18, 3, 21, 21)[1] == list(range(21))


def test_causal_slot_overflow_raises():
    with pytest.raises(ValueError, match="overflow"):
        causal_slots(18, 3, 20, 21)
    with pytest.raises(ValueError, match="overflow"):
        causal_slots(0, 3, 21, 21, local_end=0, global_end=9)
    with pytest.raises(ValueError):
        causal_slots(0, 0, 21, 21)


def test_too_many_frames_per_block_raises():
    with pytest.raises(ValueError, match="num_frame_per_block"):
        _pipe(num_frame_per_block=9)


def test_cli_routing():
    few = types.SimpleNamespace(**DMD_KEYS)
    fps = cli.load_config(None)
    assert cli.pipeline_class(few) is CausalInferencePipeline
    assert cli.pipeline_class(fps) is CausalFPSInferencePipeline


def test_cli_routing_from_yaml(tmp_path):
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list:\n- 1000\n- 750\n- 500\n- 250\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    assert cli.pipeline_class(cli.load_config(str(cfg))) is CausalInferencePipeline
    plain = tmp_path / "fps.yaml"
    plain.write_text("timestep_shift: 5.0\n")
    assert cli.pipeline_class(cli.load_config(str(plain))) is CausalFPSInferencePipeline


@pytest.mark.parametrize("extra, msg", [(["--duration", "2"], "--duration 2"), (["--duration", "1", "--i2v"], "--i2v"),
                                        ([], "--duration 3")])
def test_cli_fewstep_refusals(tmp_path, capsys, extra, msg):
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["--config_path", str(cfg), "--synthetic", "--model", "tiny"] + extra)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_cli_fewstep_refuses_multirank(monkeypatch, tmp_path, capsys):
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.main(["--config_path", str(cfg), "--synthetic", "--duration", "1"])
    assert "WORLD_SIZE 1" in capsys.readouterr().err
