"""bench.py's N > 1 code paths, functionally, on a 1-GPU box (-m gpu): `--gpus 2` makes bench.py start two ranks itself; with
`--dist-backend gloo` they share cuda:0 and stage their exchanges through the host (two RCCL ranks cannot share a device), so
what runs is the real lane layout, the anchor hand-off p2p, the CFG pair's per-step exchange with a hipGraph per forward, the
max-over-ranks timing and rank 0's single JSON line.  The driver's 8-GPU run uses the same code with the nccl backend."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scale_to_50(k, n_chunks, model="tiny", lat=(16, 24)):
    """What a K-step wavefront's wall clock is multiplied by to state it at the reference's 50 steps: the FLOP-weighted ratio of the
    forwards each stage of each chunk runs (2 K + 2; 2 K for the stage that does not persist its K / V, casual_fps_inference.py:283 of
    the build's pipeline; 2 for the first stage of chunks >= 2) -- bench.py `wall_scale_to_50_steps`."""
    from mmpl_amd.stage_plan import T2V_STAGE_SHAPES, dit_forward_flops
    from mmpl_amd.synthetic import WAN_CONFIGS
    S = (lat[0] // 2) * (lat[1] // 2)
    fl = [dit_forward_flops(WAN_CONFIGS[model], S, q, kv) for q, kv in T2V_STAGE_SHAPES]
    tot = lambda K: sum(sum(f * n for f, n in zip(fl, [2 * K + 2 if c == 0 else 2, 2 * K + 2, 2 * K + 2, 2 * K])) for c in range(n_chunks))
    return tot(50) / tot(k)


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--model", "small", "--res", "tiny",
           "--steps", "8", "--warmup", "4", "--full", "--no-cpu-baseline", "--no-vae"] + extra
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_default_two_rank_line_is_a_measured_wavefront():
    """`bench.py --gpus 2` with NO wavefront flag runs one video of 2 x lanes chunks through the real pipeline
    and the real dependency chain and reports its wall clock; the UniPC steps per stage come from the wall-clock budget and the
    scaling to the reference's 50 steps is stated; the occupancy model is printed beside it, not as `value`."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--model", "tiny", "--res", "tiny",
           "--wavefront-budget-s", "20", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["lanes"] == 2 and r["chunks"] == 4 and r["config"]["parallelism"].startswith("measured wavefront")
    k = r["config"]["sampling_steps"]
    assert 2 <= k <= 50 and r["value_modelled"] > 0 and r["ms_per_step"] > 0
    if k < 50:
        assert abs(r["value_shortened_run"] - 21.0 * 4 / r["wall_s"]) < 1e-9 and "value_scaling" in r
        assert abs(r["wall_scale_to_50_steps"] - _scale_to_50(k, 4)) < 1e-9 and 1.0 < r["wall_scale_to_50_steps"] <= 100.0 / (2 * k)
        assert abs(r["value"] - r["value_shortened_run"] / r["wall_scale_to_50_steps"]) < 1e-9
    else:
        assert abs(r["value"] - 21.0 * 4 / r["wall_s"]) < 1e-9


def test_two_chunk_lanes_rotation_line():
    r = _run(["--rotation"])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and "functional_only" in r and "value_is_modelled" in r
    assert "chunk-per-rank x2" in r["config"]["parallelism"] and "hand-off" in r["config"]["parallelism"]
    assert r["value"] > 0 and r["value_independent_chunks"] >= r["value"] and len(r["sec_per_denoise_step_by_stage"]) == 4
    assert r["roofline"]["achieved"] > 0


def test_cfg_pair_with_graphed_forwards():
    r = _run(["--cfg-split", "--rotation"])
    assert r["n_gpus"] == 2 and "CFG split" in r["config"]["parallelism"]
    assert "hipGraph replay per forward" in r["config"]["timed_path"]
    assert r["value"] > 0 and r["roofline"]["achieved"] > 0
    # each rank computes ONE branch per step
    assert r["achieved_pflops_per_gpu"] > 0


def _wavefront(gpus, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--dist-backend", "gloo", "--model", "tiny", "--res", "tiny",
           "--wavefront-chunks", "4", "--sampling-steps", "3"] + extra
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_measured_wavefront_two_lanes():
    """`--wavefront-chunks`: the N > 1 line as a MEASUREMENT -- the real pipeline, the real dependency chain (chunk c + 1 starts from
    chunk c's anchors), wall clock first noise -> last latent; two ranks on one GPU over gloo (functional)."""
    r = _wavefront(2, [])
    assert r["n_gpus"] == 2 and r["chunks"] == 4 and r["lanes"] == 2 and "measured wavefront" in r["config"]["parallelism"]
    assert abs(r["value_shortened_run"] - 21.0 * 4 / r["wall_s"]) < 1e-9 and r["value_modelled"] > 0
    # 3 steps: scaled per stage (2 K + 2 forwards; 2 K in the stage without a refresh pair, the heaviest one: 100 / 6 there; a constant 2
    # in the first stage of chunks >= 2) -- MORE than one 102 / 8 for everything here (that factor over-stated `value` by ~10 %
    # at K = 2)
    assert abs(r["wall_scale_to_50_steps"] - _scale_to_50(3, 4)) < 1e-9 and 102.0 / 8.0 < r["wall_scale_to_50_steps"] < 100.0 / 6.0
    assert abs(r["value"] - r["value_shortened_run"] / r["wall_scale_to_50_steps"]) < 1e-9
    assert len(r["chunk_s"]) == 4 and len(r["stagger_s"]) == 3 and all(s > 0 for s in r["stagger_s"])
    # chunk c + 1 cannot start before chunk c's anchor stage is done (the dependency is real)
    assert all(st >= a - 0.05 for st, a in zip(r["stagger_s"], r["anchor_done_after_s"]))
    # ... and it IS a wavefront: chunk c + 1 starts when chunk c's anchors arrive, not when chunk c has finished (a hand-off that only
    # left at the end of the producer's chunk showed up here as stagger == chunk time)
    # (checked on the first hand-off: later staggers on 2 lanes include waiting for the lane to finish its previous chunk, and chunk 0
    # carries the one-time graph captures)
    assert r["stagger_s"][0] < 0.9 * r["chunk_s"][0], (r["stagger_s"], r["chunk_s"])
    assert set(r["rank_busy_fraction"]) == {"0", "1"} and all(0 < v <= 1.0 for v in r["rank_busy_fraction"].values())
    assert set(r["handoff_latency_s"]) == {"1", "2", "3"} and all(0 <= v < 30 for v in r["handoff_latency_s"].values())
    assert "value_scaling" in r and "functional_only" in r          # 3 sampling steps, shared GPU


def test_measured_wavefront_one_rank_is_the_sequential_chain():
    r = _wavefront(1, [])
    assert r["n_gpus"] == 1 and r["lanes"] == 1 and "sequential chain" in r["config"]["parallelism"]
    assert sum(r["chunk_s"]) <= r["wall_s"] * 1.001 and r["rank_busy_fraction"]["0"] > 0.5


def test_measured_wavefront_two_lanes_of_cfg_pairs():
    """The layout an 8-GPU run uses (N >= 4: N / 2 chunk lanes x (cond, uncond) rank pairs), here 4 ranks on one GPU over gloo: the
    hand-off runs between the lane heads (the cond ranks), each pair exchanges its two flow predictions per step, and the wavefront
    is measured the same way."""
    r = _wavefront(4, ["--cfg-split"])
    assert r["n_gpus"] == 4 and r["chunks"] == 4 and r["lanes"] == 2 and "measured wavefront" in r["config"]["parallelism"]
    assert abs(r["value_shortened_run"] - 21.0 * 4 / r["wall_s"]) < 1e-9
    assert len(r["stagger_s"]) == 3 and all(st >= a - 0.05 for st, a in zip(r["stagger_s"], r["anchor_done_after_s"]))
    # (checked on the first hand-off: later staggers on 2 lanes include waiting for the lane to finish its previous chunk, and chunk 0
    # carries the one-time graph captures)
    assert r["stagger_s"][0] < 0.9 * r["chunk_s"][0], (r["stagger_s"], r["chunk_s"])


def test_default_eight_rank_line_is_four_lanes_of_cfg_pairs():
    """BASELINE configs[4]'s layout end to end on one GPU: `bench.py --gpus 8` starts eight ranks (gloo: they share cuda:0), builds 4 chunk
    lanes x (cond, uncond) pairs -- 4 pair groups, the heads group, the world group and their control groups -- and measures ONE video
    of 2 x lanes = 8 chunks through the real pipeline, chunk c + 4 wrapping around onto lane c.  What the driver's 8-GPU run executes
    with the nccl backend (reference: Wan_fps_inference_parallel_4gpu_5-60s.py:188-381; its wall-clock log
    MMPL_i2v/logs/parallel_i2v_server.log:791-807)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dist-backend", "gloo", "--model", "tiny", "--res", "tiny",
           "--wavefront-budget-s", "30", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["config"]["parallelism"].startswith("measured wavefront: 8 chunks on 4 lane(s) x 2"), r["config"]["parallelism"]
    assert r["n_gpus"] == 8 and r["lanes"] == 4 and r["chunks"] == 8 and len(r["chunk_s"]) == 8 and len(r["stagger_s"]) == 7
    assert set(r["rank_busy_fraction"]) == {"0", "2", "4", "6"}                       # the lane heads (their partners mirror them)
    assert set(r["handoff_latency_s"]) == {str(c) for c in range(1, 8)}               # every hand-off arrived, the wrap-around ones too
    assert all(st >= a - 0.05 for st, a in zip(r["stagger_s"], r["anchor_done_after_s"]))
    k = r["config"]["sampling_steps"]
    assert abs(r["wall_scale_to_50_steps"] - _scale_to_50(k, 8)) < 1e-9 and r["value"] > 0


def test_single_gpu_bench_line_fields_and_heavy_tail_switches():
    """One rank, small model: the default line's contract fields (BASELINE metric, `roofline`, executed vs algorithmic PFLOP/s) and the
    diagnostic switches of the self-attention's pass history (`--heavy-tail [--heavy-tail-heads P]`, `--no-attn-history`): the counters
    add up, and without the history nothing is predicted or remembered."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--model", "small", "--res", "tiny", "--steps", "12", "--warmup", "4", "--full", "--no-cpu-baseline", "--no-vae",
            "--probe-seconds", "0"]

    def run(extra):
        p = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])

    r = run([])
    assert r["metric"] == "video_latent_frames_per_sec" and r["n_gpus"] == 1 and r["dtype"] == "bf16" and r["vs_baseline"] is None
    assert r["roofline"]["bound"] == "mfma" and r["roofline"]["achieved"] > 0 and "attn_history" in r and r["attn_history"].startswith("on")
    assert 0 < r["executed_pflops_per_gpu"] <= r["achieved_pflops_per_gpu"] and "flop_accounting" in r
    assert "attn_blocks" not in r                                        # counters only under --attn-stats / --heavy-tail
    h = run(["--heavy-tail", "--heavy-tail-gain", "12", "--heavy-tail-heads", "0.5"])
    assert "0.5 of every layer's heads" in h["weights"] and h["attn_blocks"] > 0
    parts = h["attn_blocks_redone"] + h["attn_blocks_predicted"] + h["attn_blocks_fast_on_remembered_reference"]
    assert 0 <= parts <= h["attn_blocks"] and h["attn_blocks_redone_fraction"] == h["attn_blocks_redone"] / h["attn_blocks"]
    n = run(["--heavy-tail", "--heavy-tail-gain", "12", "--heavy-tail-heads", "0.5", "--no-attn-history"])
    assert n["attn_history"].startswith("off") and n["attn_blocks_predicted"] == 0 and n["attn_blocks_fast_on_remembered_reference"] == 0
    assert n["attn_blocks_redone"] >= h["attn_blocks_redone"]           # with the history a failing block does not keep paying twice


def test_plain_line_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain one-rank run (no --full) times exactly --steps steps and prints the headline without the measurements that take runs
    of their own (probe, per-kernel eager pass, VAE decode, CPU baseline); `--dump-outputs` writes what the last timed step computed,
    and two runs with the same arguments write the same arrays (seeded inputs, identical launch sequences)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "small", "--res", "tiny", "--steps", "5", "--warmup", "2",
               "--dump-outputs", str(out)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        r = json.loads(lines[0])
        assert r["metric"] == "video_latent_frames_per_sec" and r["value"] > 0 and r["unit"] == "latent-frames/s" and r["higher_is_better"] is True
        assert r["dtype"] == "bf16" and r["steps"] == 5 and r["ms_per_step"] > 0
        assert not {"roofline", "eager", "cpu_baseline", "vae_roofline", "gemm_tflops", "kernel_time_share"} & set(r)
        assert r["vae_decode_s_per_chunk"] is None
        dumps.append({n: np.load(out / f"{n}.npy") for n in ("latents", "flow_cond", "flow_uncond")})
    # 2 warm-up + 5 timed steps rotate s0..s3: the last timed step is stage s2 (6 query frames of 16 x 24 latents)
    for n, a in dumps[0].items():
        assert a.dtype == np.float32 and a.shape == (6, 16, 16, 24) and np.isfinite(a).all() and a.any(), n
        assert np.array_equal(a, dumps[1][n]), n
