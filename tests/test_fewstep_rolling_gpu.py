"""Rolling KV window of the few-step pipeline on the MI355X (CausalInferencePipeline(args.rolling_kv)): blocks past the window
against the oracle on a teacher-forced cache (tests/fewstep_rolling_ref.py), sink frames kept and ring slots overwritten, the
prefix below the window bit-identical to the non-rolling pipeline, a bounded number of hipGraphs, inference_stream, the CLI."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fewstep_rolling_ref import block as ref_block, schedule_slots  # noqa: E402
from util import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)
F = 3
TOL = 2e-2                      # the per-block bound of tests/test_fewstep_gpu.py (a 4-step block + refresh against the oracle)


def _args(**kw):
    a = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=F,
             independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    a.update(kw)
    return types.SimpleNamespace(**a)


class _Ctx(torch.nn.Module):
    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _pipe(window, sink=0, rolling=True, vae=False):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal, vae_state_dict
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper, WanVAEWrapper
    cfg = WAN_CONFIGS["tiny"]
    geo = Geometry(*LAT)
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, local_attn_size=window, sink_size=sink, model_config=cfg,
                              geometry=geo, device=DEV)
    sd = dit_state_dict(cfg, seed=1)
    gen.load_state_dict(sd)
    ctx = philox_normal([1, 512, cfg["text_dim"]], 32)
    ctx[:, 40:] = 0
    v = WanVAEWrapper(geometry=geo, device=DEV, state_dict=vae_state_dict(seed=2)) if vae else _NoVAE()
    pipe = CausalInferencePipeline(_args(rolling_kv=rolling), DEV, generator=gen, text_encoder=_Ctx(ctx.to(DEV)), vae=v)
    return pipe, sd, cfg, ctx


def _noise(n, seed=71):
    from mmpl_amd.synthetic import philox_normal
    return philox_normal([1, n, 16, *LAT], seed).to(DEV)


def _draws(n_blocks, base=80):
    from mmpl_amd.synthetic import philox_normal
    return [philox_normal([F, 16, *LAT], base + k) for k in range(3 * n_blocks)]


# ------------------------------------------------------------------------------------------------ block parity, teacher-forced
_RUNS = {}


def _teacher_forced(window, sink):
    """18 frames through pipe._blocks by hand.  Before each of blocks 2, 3, 4 (the first at or past the window -- the straddling one
    for window 8 --, a steady one, the first after a full revolution of the 6-slot ring) the device cache is copied into an oracle
    cache of the same slots; the block's output and the K it leaves in its write slots are then compared with the oracle's."""
    key = (window, sink)
    if key in _RUNS:
        return _RUNS[key]
    from oracle import wan_dit_ref as W
    pipe, sd, cfg, ctx = _pipe(window, sink)
    gen = pipe.generator
    S, H, L = gen.engine.S, cfg["num_heads"], cfg["num_layers"]
    ocfg = W.DitCfg(**cfg)
    noise, draws = _noise(18), _draws(6)
    pipe.renoise_override = [d.to(DEV) for d in draws]
    plan = schedule_slots(window, sink, [F] * 6)
    ts, sx, sn = pipe._step_scalars()
    rec = dict(blocks={}, plan=plan)
    with torch.no_grad():
        it = pipe._blocks(noise, ["p"])
        next(it)
        kv = pipe.kv_cache1
        assert kv.k_all.shape[1] == window * S
        for b, (start, n, write, vis, _) in enumerate(plan):
            okv = None
            if b in (2, 3, 4):
                torch.cuda.synchronize()
                okv = [{"k": kv.k_all[l].view(1, -1, H, 128).cpu().clone(), "v": kv.v_all[l].view(1, -1, H, 128).cpu().clone()}
                       for l in range(L)]
            s_, n_, out = next(it)
            assert (s_, n_) == (start, n)
            torch.cuda.synchronize()
            if b == 0:
                rec["sink_snapshot"] = (kv.k_all[:, :2 * S].clone(), kv.v_all[:, :2 * S].clone())     # frame 1 is written
            if okv is not None:
                x0 = ref_block(sd, ocfg, okv, [None] * L, noise[0, start:start + n].cpu(), ctx[0], list(range(start, start + n)),
                               write, vis, ts, sx, sn, draws[3 * b:3 * b + 3], 0.0)
                e_out = rel_l2(out[0, start:start + n], x0)
                e_k = max(rel_l2(kv.k_all[l].view(-1, H, 128)[w * S:(w + 1) * S], okv[l]["k"][0, w * S:(w + 1) * S])
                          for l in range(L) for w in write)
                rec["blocks"][b] = (start, write, e_out, e_k)
        assert next(it, None) is None
    rec["k_end"], rec["v_end"] = kv.k_all.clone(), kv.v_all.clone()
    rec["S"] = S
    pipe.release_graphs()
    _RUNS[key] = rec
    return rec


@pytest.mark.parametrize("window,sink", [(6, 0), (8, 2)])
def test_rolling_blocks_vs_oracle(window, sink):
    rec = _teacher_forced(window, sink)
    assert sorted(rec["blocks"]) == [2, 3, 4]
    if window == 8:
        assert rec["blocks"][2][1] == [6, 7, 2], "the straddling block wraps"
    assert rec["blocks"][4][1] == rec["blocks"][2][1], "one revolution of the ring later"
    for b, (start, write, e_out, e_k) in rec["blocks"].items():
        print(f"[rolling] window {window} sink {sink} block at frame {start} -> slots {write}: rel_l2 out {e_out:.3e}, K {e_k:.3e}")
    for b, (start, write, e_out, e_k) in rec["blocks"].items():
        assert e_out < TOL and e_k < TOL, (window, sink, start, e_out, e_k)


def test_sink_slots_keep_their_bits_and_ring_slots_do_not():
    rec = _teacher_forced(8, 2)
    S = rec["S"]
    k0, v0 = rec["sink_snapshot"]
    assert k0.any() and v0.any()
    assert torch.equal(rec["k_end"][:, :2 * S], k0) and torch.equal(rec["v_end"][:, :2 * S], v0)
    rec = _teacher_forced(6, 0)
    k0, v0 = rec["sink_snapshot"]
    assert not torch.equal(rec["k_end"][:, :S], k0[:, :S]) and not torch.equal(rec["v_end"][:, :S], v0[:, :S])


# ------------------------------------------------------------------------------------------------ prefix identity
@pytest.mark.parametrize("use_graphs", [False, True])
def test_prefix_below_the_window_is_bit_identical(use_graphs):
    noise, draws = _noise(6, 72), [d.to(DEV) for d in _draws(2, 90)]
    lats = []
    for rolling in (False, True):
        pipe, *_ = _pipe(6, 0, rolling=rolling)
        pipe.use_graphs = use_graphs
        pipe.renoise_override = draws
        _, lat = pipe.inference(noise, ["p"], return_latents=True)
        lats.append(lat)
        assert not pipe._roll_bufs
        if use_graphs:
            assert all(k[0] != "rolling" for k in pipe._graphs), "today's graph keys below the window"
        pipe.release_graphs()
    assert torch.equal(lats[0], lats[1])


# ------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("window,sink", [(6, 0), (8, 2)])
def test_graph_count_is_bounded_and_second_call_constructs_none(monkeypatch, window, sink):
    pipe, *_ = _pipe(window, sink)
    noise, draws = _noise(18, 73), [d.to(DEV) for d in _draws(6, 100)]
    pipe.renoise_override = draws
    pipe.use_graphs = False
    _, eager = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 0 and not pipe._graphs
    pipe.use_graphs = True
    _, first = pipe.inference(noise, ["p"], return_latents=True)
    R = window - sink
    below = sum(1 for s in range(0, 18, F) if s + F <= window)
    assert 0 < pipe.graph_captures <= below + R // math.gcd(R, F), pipe.graph_captures
    assert len(pipe._graphs) == pipe.graph_captures
    rolled = [k for k in pipe._graphs if k[0] == "rolling"]
    steady = {tuple(w) for start, _, w, _, _ in schedule_slots(window, sink, [F] * 6) if start + F > window}
    # the key of a block past the window: frames per block, the step list, context_noise, write slots, visible slots -- neither the
    # start frame nor the video's length (which sizes the output latent) is in it
    assert {k[4] for k in rolled} == steady and len(rolled) == len(steady)
    assert all(len(k) == 6 and k[1] == F and k[5] == tuple(range(window)) for k in rolled)
    made = []
    real = torch.cuda.CUDAGraph

    class Counting(real):
        def __new__(cls, *a, **k):
            made.append(1)
            return real(*a, **k)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Counting)
    captures = pipe.graph_captures
    _, second = pipe.inference(noise, ["p"], return_latents=True)
    assert not made and pipe.graph_captures == captures
    assert torch.equal(eager, first), "eager == graph"
    assert torch.equal(first, second)
    assert torch.isfinite(first.float()).all() and first[0, 15:].float().abs().max() > 0
    pipe.release_graphs()
    assert not pipe._graphs and not pipe._bufs and not pipe._roll_bufs and not pipe._out and pipe._frame_base is None


def test_longer_video_adds_no_graph():
    """36 frames after 18: the blocks below the window are keyed by the call's length (as without rolling) and are captured again,
    the blocks past it replay the patterns the first call captured."""
    pipe, *_ = _pipe(6, 0)
    torch.manual_seed(3)
    pipe.inference(_noise(18, 74), ["p"])
    rolled = {k for k in pipe._graphs if k[0] == "rolling"}
    assert len(rolled) == 2
    torch.manual_seed(3)
    _, lat = pipe.inference(_noise(36, 75), ["p"], return_latents=True)
    assert {k for k in pipe._graphs if k[0] == "rolling"} == rolled
    assert torch.isfinite(lat.float()).all() and lat[0, 33:].float().abs().max() > 0
    pipe.release_graphs()


# ------------------------------------------------------------------------------------------------ stream
def test_stream_equals_inference_rolling():
    pipe, *_ = _pipe(6, 0, vae=True)
    noise = _noise(12, 76)
    torch.manual_seed(5)
    video = pipe.inference(noise, ["p"])
    assert video.shape == (1, 1 + 4 * 11, 3, 8 * LAT[0], 8 * LAT[1])
    u8 = (video * 255.0).clamp(0, 255).to(torch.uint8)[0].permute(0, 2, 3, 1).contiguous().cpu()
    captures = pipe.graph_captures
    for overlap in (True, False):
        for output in ("float", "uint8"):
            torch.manual_seed(5)
            firsts, parts = [], []
            for first, frames in pipe.inference_stream(noise, ["p"], output=output, overlap=overlap):
                firsts.append(first)
                parts.append(frames)
            assert firsts == [0] + [1 + 4 * (s - 1) for s in (3, 6, 9)], firsts
            got = torch.cat(parts)
            assert torch.equal(got, video[0] if output == "float" else u8), (overlap, output)
    assert pipe.graph_captures == captures
    pipe.release_graphs()


# ------------------------------------------------------------------------------------------------ CLI, and off stays off
def test_cli_rolling_duration_2(tmp_path):
    from mmpl_amd import cli
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    cli.main(["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--num_output_frames", "9", "--duration", "2", "--rolling",
              "--local_attn_size", "6", "--config_path", str(cfg), "--output_folder", str(tmp_path)])
    v = torch.load(tmp_path / "0-0.pt")
    assert tuple(v.shape) == (1 + 4 * 17, 128, 192, 3) and v.dtype == torch.uint8


def test_without_rolling_the_cache_still_overflows():
    pipe, *_ = _pipe(-1, 0, rolling=False)
    pipe.use_graphs = False
    with pytest.raises(ValueError, match="overflow"):
        pipe.inference(_noise(24, 77), ["p"])
