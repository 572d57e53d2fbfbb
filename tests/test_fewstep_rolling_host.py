"""Rolling KV window of the few-step pipeline, host side: ``rolling_slots`` against a list simulation of evict-the-oldest-non-sink
(tests/fewstep_rolling_ref.py), its rejections, and the entry point's --rolling routing."""
import math
import os
import sys
import types

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fewstep_rolling_ref import schedule_slots  # noqa: E402

from mmpl_amd import cli  # noqa: E402
from mmpl_amd.wan_wrapper import rolling_slots  # noqa: E402

WINDOWS = [(21, 0), (21, 3), (21, 1), (6, 0), (6, 3), (9, 3), (7, 1), (8, 2), (5, 2)]


def _schedule(W, s):
    k = W + (W - s)                                   # >= 3 * W frames, and W - s blocks past the window: every steady pattern
    return ([1] if s == 1 else []) + [3] * k


@pytest.mark.parametrize("W,s", WINDOWS)
def test_rolling_slots_match_evict_oldest_simulation(W, s):
    sched = _schedule(W, s)
    assert sum(sched) >= 3 * W
    steady = set()
    for start, n, write, vis, frames in schedule_slots(W, s, sched):
        got_w, got_v = rolling_slots(start, n, W, s)
        assert got_w == write, (start, got_w, write)
        assert got_v == vis, (start, got_v, vis)
        end = start + n
        # what the block attends to: every frame so far, or the sink frames plus the most recent W - s
        assert frames == (list(range(end)) if end <= W else list(range(s)) + list(range(end - (W - s), end))), (start, frames)
        if start >= W:
            steady.add(tuple(write))
    R = W - s
    assert len(steady) == R // math.gcd(R, 3), (steady, R)


def test_straddling_block_wraps():
    assert rolling_slots(6, 3, 8, 2) == ([6, 7, 2], list(range(8)))
    assert rolling_slots(3, 3, 8, 2) == ([3, 4, 5], list(range(6)))          # below the window: the causal layout
    assert rolling_slots(9, 3, 8, 2) == ([3, 4, 5], list(range(8)))


@pytest.mark.parametrize("args", [(0, 4, 6, 3), (0, 7, 6, 0), (0, 3, 6, 6), (0, 3, 6, 7), (0, 3, 6, -1), (1021, 4, 21, 0),
                                  (1023, 3, 21, 3), (1024, 1, 21, 0)])
def test_rolling_slots_rejections(args):
    with pytest.raises(ValueError):
        rolling_slots(*args)


def test_last_rope_position_is_accepted():
    w, v = rolling_slots(1021, 3, 21, 3)
    assert len(w) == 3 and v == list(range(21))


def _cfg(tmp_path, fewstep=True):
    cfg = tmp_path / ("self_forcing_dmd.yaml" if fewstep else "fps.yaml")
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n" if fewstep
                   else "timestep_shift: 5.0\n")
    return str(cfg)


def test_cli_rolling_passes_the_refusals():
    args = types.SimpleNamespace(duration=2, rolling=True, i2v=False, i2v_model=False, num_output_frames=21, stream=True)
    assert cli.fewstep_refusal(args, 1) is None
    assert cli.rolling_refusal(args, True) is None
    args.rolling = False
    assert "--duration 2" in cli.fewstep_refusal(args, 1)
    assert cli.rolling_refusal(args, True) is None and cli.rolling_refusal(args, False) is None


def test_cli_rolling_needs_a_fewstep_config(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--config_path", _cfg(tmp_path, fewstep=False), "--synthetic", "--model", "tiny", "--rolling"])
    assert e.value.code == 2
    assert "--rolling" in capsys.readouterr().err


def test_cli_duration_still_refused_without_rolling(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--config_path", _cfg(tmp_path), "--synthetic", "--model", "tiny", "--duration", "2"])
    assert e.value.code == 2
    assert "--duration 2" in capsys.readouterr().err


def test_at_entry_points_are_bound_and_validate_before_launching():
    """mmpl_dit_forward_at / mmpl_qknorm_rope_at: the old entry points' checks, reached without a device."""
    from mmpl_amd import _lib
    lib = _lib.load()
    assert lib.mmpl_dit_forward_at(None, None, None, 1, None, None, None, 0, None, None, 15, None, None, 512, None, None, None, None,
                                   None, 0, None, None) != 0
    assert "weights not bound" in lib.mmpl_last_error().decode()
    assert lib.mmpl_qknorm_rope_at(None, None, 0, None, 0, None, 0, None, None, 3, None, None, None, None, None) != 0
    assert "null handle" in lib.mmpl_last_error().decode()


# ------------------------------------------------------------------------------------------------ the pipeline's host logic
class _FakeKV(list):
    def __init__(self, n_slots, S):
        import torch
        super().__init__([{"global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])}])
        self.engine = types.SimpleNamespace(S=S)
        self.k_all = torch.zeros(1, n_slots * S, 8)


class _FakeCross(list):
    def fill(self, pe):
        pass


class _FakeGen:
    """A generator that launches nothing: `flow` records (relative start, base, write, visible) and `fewstep_update` writes each
    frame's ABSOLUTE position (relative start + base) into the x0 it is handed, so the output latent shows where every block ran."""

    def __init__(self, window, sink):
        import torch
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper
        self.geometry = Geometry(16, 24)
        self.engine = types.SimpleNamespace(L=1, max_frames=7, S=self.geometry.frame_seqlen)
        self.model = types.SimpleNamespace(local_attn_size=window, sink_size=sink, num_frame_per_block=1)
        self.window_frames = window
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.calls, self.pos = [], None
        self.slots = types.MethodType(WanDiffusionWrapper.slots, self)
        self.set_cache_ends = WanDiffusionWrapper.set_cache_ends
        self._torch = torch

    def get_scheduler(self):
        return self.scheduler

    def sigma_x0(self, t):
        return 0.5

    def sigma_add_noise(self, t):
        return 0.25

    def new_kv_cache(self):
        return _FakeKV(self.window_frames, self.engine.S)

    def new_crossattn_cache(self):
        return _FakeCross()

    def flow(self, x, t, start, write, vis, kv, cross, out=None, frame_base=None):
        base = None if frame_base is None else int(frame_base)
        assert frame_base is None or (frame_base.dtype == self._torch.int32 and frame_base.numel() == 1)
        self.calls.append((start, base, tuple(write), tuple(vis)))
        self.pos = start + (base or 0)
        return out

    def fewstep_update(self, flow, x, noise, x0_out, sigma_t, sigma_next=0.0):
        for i in range(x0_out.shape[0]):
            x0_out[i].fill_(self.pos + i)


def _fake_pipe(window, sink, rolling=True):
    import torch
    from mmpl_amd.pipeline import CausalInferencePipeline
    a = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                              independent_first_frame=False, context_noise=0, rolling_kv=rolling)
    gen = _FakeGen(window, sink)
    pipe = CausalInferencePipeline(a, "cpu", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": torch.zeros(1, 4, 4)},
                                   vae=object())
    pipe.use_graphs = False
    return pipe, gen


@pytest.mark.parametrize("W,s", [(6, 0), (8, 2)])
def test_pipeline_blocks_past_the_window_run_relative_to_the_device_base(W, s):
    import torch
    pipe, gen = _fake_pipe(W, s)
    S = gen.engine.S
    noise = torch.zeros(1, 18, 16, 16, 24)
    plan = schedule_slots(W, s, [3] * 6)
    with torch.no_grad():
        it = pipe._blocks(noise, ["p"])
        assert next(it)[:2] == (0, 0)
        for start, n, write, vis, _ in plan:
            gen.calls.clear()
            s_, n_, out = next(it)
            assert (s_, n_) == (start, n)
            # 4 denoising forwards + the refresh forward, all on the simulation's slots; past the window: relative ids + base
            want = (0, start) if start + n > W else (start, None)
            assert gen.calls == [want + (tuple(write), tuple(vis))] * 5, (start, gen.calls)
            assert int(pipe.kv_cache1[0]["global_end_index"][0]) == (start + n) * S
            assert int(pipe.kv_cache1[0]["local_end_index"][0]) == min(start + n, W) * S
        assert next(it, None) is None
    # every frame of the output latent was produced at its own absolute position, through the static x0 buffers where rolled
    assert torch.equal(out[0, :, 0, 0, 0].float(), torch.arange(18.0))
    assert len(pipe._roll_bufs) == 2 and all(k[0] == "rolling" and len(k) == 6 for k in pipe._roll_bufs)
    pipe._graphs.clear(), pipe._bufs.clear(), pipe._out.clear(), pipe._roll_bufs.clear()


def test_pipeline_rolling_rejects_before_anything_runs():
    import torch
    pipe, gen = _fake_pipe(21, 0)
    with pytest.raises(ValueError, match="1023"), torch.no_grad():
        next(pipe._blocks(torch.zeros(1, 1026, 16, 16, 24), ["p"]))
    assert not gen.calls
    pipe, gen = _fake_pipe(6, 4)                                    # 3-frame blocks do not fit the 2 rolling slots
    with pytest.raises(ValueError, match="rolling"), torch.no_grad():
        next(pipe._blocks(torch.zeros(1, 6, 16, 16, 24), ["p"]))
    assert not gen.calls
    pipe, gen = _fake_pipe(6, 0, rolling=False)                      # off stays off
    with pytest.raises(ValueError, match="overflow"), torch.no_grad():
        list(pipe._blocks(torch.zeros(1, 9, 16, 16, 24), ["p"]))
