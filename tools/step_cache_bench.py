"""Step caching (TeaCache, mmpl_amd/step_cache.py) measured: one whole-clip sample (BidirectionalDiffusionInferencePipeline) and one
FPS chunk (CausalFPSInferencePipeline, all its stages) with synthetic weights, each with the policy off, with thresh 0 (every step
computed and recorded) and with the identity polynomial at a few thresholds.  Per run: wall time of the denoise loop (second call:
graphs captured), computed / skipped steps, and the relative L2 distance of the final latents to the uncached run.  Also the three
step graphs of the whole-clip pipeline replayed on their own: plain, RECORD, REUSE.  Prints one JSON line.

    python tools/step_cache_bench.py --model 1.3B --resolution 480p
    python tools/step_cache_bench.py --model tiny --latent_hw 16 24 --steps 6 --thresholds 0.05 0.2

Without --thresholds they are 2, 4 and 8 times the median distance between consecutive timestep embeddings on these weights.

Synthetic weights say nothing about picture quality: the distances below show how far the latents move, not what a viewer sees.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, time.perf_counter() - t0


def policies(args):
    from mmpl_amd.step_cache import StepCachePolicy
    return [("off", None), ("thresh_0", StepCachePolicy(0.0))] + [(f"thresh_{t:g}", StepCachePolicy(t)) for t in args.thresholds]


def run_policies(pipe, call, args, dev):
    """`call()` once to capture, once timed, per policy -> {name: seconds, computed, skipped, rel_l2_vs_off}."""
    res, base = {}, None
    for name, policy in policies(args):
        pipe.step_cache = policy
        call()                                             # captures this policy's graphs
        lat, s = timed(call, dev)
        base = lat if base is None else base
        res[name] = dict(seconds=round(s, 4), computed_steps=pipe.computed_steps, skipped_steps=pipe.skipped_steps,
                         rel_l2_vs_off=rel_l2(lat, base), bit_equal_to_off=bool(torch.equal(lat, base)))
        print(f"[step_cache_bench] {type(pipe).__name__} {name}: {s:.3f} s, {pipe.skipped_steps} skipped", file=sys.stderr, flush=True)
    return res


def whole_clip(args, cfg, geo, dev):
    from mmpl_amd.dit import CACHE_OFF, CACHE_RECORD, CACHE_REUSE
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.step_cache import StepCachePolicy
    from mmpl_amd.synthetic import dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=5.0, model_config=cfg, geometry=geo, device=dev)
    gen.load_state_dict(dit_state_dict(cfg, seed=1234, device=dev))
    pargs = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="")
    pipe = BidirectionalDiffusionInferencePipeline(pargs, dev, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), dev),
                                                   vae=_NoVAE())
    pipe.sampling_steps, pipe.shift = args.steps, 5.0
    noise = philox_normal([1, args.frames, 16, geo.lat_h, geo.lat_w], 7).to(torch.bfloat16).to(dev)
    st = pipe._step_state(noise)                           # (policy off) the sampler's timestep table -> the indicator's distances
    rel = gen.engine.rel_l1_rows(gen.engine.time_embed(st["sched"]._t_table)[0]).cpu()
    if not args.thresholds:                                # by default 2, 4 and 8 median distances: about 1/2, 3/4, 7/8 of the steps skipped
        args.thresholds = [round(k * float(rel.median()), 6) for k in (2, 4, 8)]
    res = run_policies(pipe, lambda: pipe.sample(noise, ["a cat running on the grass"]), args, dev)
    # the three step graphs on their own: step 1 on the same latents, replayed
    pipe.step_cache = StepCachePolicy(1e30)
    st = pipe._step_state(noise)
    graphs = {}
    for name, mode in (("plain", CACHE_OFF), ("record", CACHE_RECORD), ("reuse", CACHE_REUSE)):
        st["sched"].reset_step_table(st["t"])
        pipe._step(st, mode)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pipe._step(st, mode)
        times = []
        for i in range(args.warmup + args.reps):
            st["latents"].copy_(noise[0])
            st["sched"].reset_step_table(st["t"])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times.append(a.elapsed_time(b))
        graphs[name] = dict(ms_median=round(statistics.median(times), 3), ms=[round(t, 3) for t in times])
    return dict(frames=args.frames, rows=args.frames * geo.frame_seqlen, steps=args.steps, policies=res, step_graph=graphs,
                record_over_plain=graphs["record"]["ms_median"] / graphs["plain"]["ms_median"],
                indicator_e_rel_l1=dict(min=float(rel.min()), median=float(rel.median()), max=float(rel.max()), sum=float(rel.sum())))


def fps_chunk(args, cfg, geo, dev):
    from mmpl_amd.pipeline import CausalFPSInferencePipeline
    from mmpl_amd.synthetic import dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanFPSWrapper
    gen = WanFPSWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=geo, device=dev)
    gen.load_state_dict(dit_state_dict(cfg, seed=1234, device=dev))
    pargs = types.SimpleNamespace(model_kwargs={}, num_train_timestep=1000, timestep_shift=5.0, guidance_scale=5.0, negative_prompt="",
                                  independent_first_frame=False, sampling_steps=args.steps)
    pipe = CausalFPSInferencePipeline(pargs, dev, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), dev),
                                      vae=types.SimpleNamespace(), save=None, mode="t2v", geometry=geo)
    pipe.renoise_override = {f: philox_normal([1, 16, geo.lat_h, geo.lat_w], 100 + f).to(dev) for f in (4, 9, 13, 18)}
    noise = philox_normal([1, geo.frames_per_chunk, 16, geo.lat_h, geo.lat_w], 7).to(torch.bfloat16).to(dev)
    call = lambda: pipe.inference(noise, ["a cat running on the grass"], return_latents=True, decode=False)[1]
    return dict(stages=[len(s) for s in pipe.plan.stages], steps_per_stage=args.steps, policies=run_policies(pipe, call, args, dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.3B", choices=["1.3B", "14B", "tiny", "small"])
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--latent_hw", type=int, nargs=2, default=None)
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[],
                    help="default: 2, 4 and 8 times the median distance between consecutive timestep embeddings")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe_seconds", type=float, default=2.0)
    ap.add_argument("--skip_fps", action="store_true")
    args = ap.parse_args()

    from mmpl_amd import _lib
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    cfg = WAN_CONFIGS[args.model]
    geo = Geometry(*args.latent_hw) if args.latent_hw else Geometry.named(args.resolution)
    out = dict(metric="step_cache", model=args.model, resolution=args.resolution, weights="synthetic")
    out["whole_clip"] = whole_clip(args, cfg, geo, dev)
    out["thresholds"] = args.thresholds
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if not args.skip_fps:
        out["fps_chunk"] = fps_chunk(args, cfg, geo, dev)
    for shape in (32, 16):
        tf = C.c_double(0.0)
        _lib.check(_lib.load().mmpl_probe_mfma_tflops(shape, args.probe_seconds, C.byref(tf)), "mmpl_probe_mfma_tflops")
        out[f"mfma{shape}_tflops"] = round(tf.value, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
