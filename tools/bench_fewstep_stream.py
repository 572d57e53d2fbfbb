"""Few-step (Self-Forcing / CausVid) latency with the VAE in the loop: time to the first pixel frames and total wall time of
  * one-shot:   CausalInferencePipeline.inference() + the uint8 conversion and host copy mmpl_amd/cli.py does,
  * stream:     inference_stream(output="uint8", overlap=True)  -- block k decodes on a second stream while block k + 1 denoises,
  * in-order:   inference_stream(output="uint8", overlap=False) -- the same work on one stream,
in ONE process, alternating, `--rounds` times, after one untimed warm-up call of each (graph capture, stream / staging / workspace
allocation).  Real WanVAEWrapper and DiT with synthetic weights.  Host clock around work that ends in an event or device
synchronise: a yield follows the synchronise on its block's "ready" event, a total follows the generator's drain of the decode
stream, the one-shot total follows the blocking device-to-host copy.  Prints one JSON line.

Every run also times the denoising blocks by themselves (no decode): device events between the hand-over points of
CausalInferencePipeline._blocks, `--rounds` replays after the warm-up.  With `--rolling` (the rolling KV window; `--frames` may then
exceed the window) only the streamed modes run -- a one-shot decode of a long video is not what the mode is for -- and the JSON
also holds the last full-window block before rolling starts, the median of the steady-state blocks past the window, the hipGraphs
constructed and the seconds of video per second of wall clock; `--preview_vae` decodes the stream with the tiny TAEHV decoder.

    python tools/bench_fewstep_stream.py --model 1.3B --resolution 480p
    python tools/bench_fewstep_stream.py --model 14B --resolution 720p
    python tools/bench_fewstep_stream.py --model 1.3B --frames 63 --rolling [--sink_size 3] [--preview_vae]
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


def _spread(xs):
    """(max - min) / median of the rounds."""
    return (max(xs) - min(xs)) / statistics.median(xs) if len(xs) > 1 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.3B", choices=["1.3B", "14B", "tiny", "small"])
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--latent_hw", type=int, nargs=2, default=None, help="override the latent size (rehearsals)")
    ap.add_argument("--frames", type=int, default=21, help="latent frames of the call")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe_seconds", type=float, default=2.0)
    ap.add_argument("--rolling", action="store_true", help="rolling KV window (args.rolling_kv): --frames may exceed the window")
    ap.add_argument("--local_attn_size", type=int, default=-1, help="the KV window in latent frames (-1 = 21)")
    ap.add_argument("--sink_size", type=int, default=0, help="with --rolling: the first frames that are never evicted")
    ap.add_argument("--preview_vae", action="store_true", help="decode the streamed modes with the tiny TAEHV decoder (seeded weights)")
    args = ap.parse_args()

    from mmpl_amd import _lib
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, vae_state_dict
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper, WanVAEWrapper
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    cfg = WAN_CONFIGS[args.model]
    geo = Geometry(*args.latent_hw) if args.latent_hw else Geometry.named(args.resolution)
    config = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                                   independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0},
                                   rolling_kv=args.rolling)
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, local_attn_size=args.local_attn_size, sink_size=args.sink_size,
                              model_config=cfg, geometry=geo, device=dev)
    gen.load_state_dict(dit_state_dict(cfg, seed=1234, device=dev))
    vae = WanVAEWrapper(geometry=geo, device=dev, state_dict=vae_state_dict(seed=2))
    preview = None
    if args.preview_vae:
        from mmpl_amd.synthetic import taehv_state_dict
        from mmpl_amd.wan_wrapper import TAEHVWrapper
        preview = TAEHVWrapper(geometry=geo, device=dev, state_dict=taehv_state_dict(seed=4))
    decoder = "preview" if args.preview_vae else "vae"
    pipe = CausalInferencePipeline(config, dev, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), dev),
                                   vae=vae, preview_vae=preview)
    noise = torch.randn(1, args.frames, 16, geo.lat_h, geo.lat_w, device=dev, dtype=torch.bfloat16)
    prompt = ["a cat running on the grass"]

    def one_shot():
        torch.manual_seed(0)                                     # the same re-noise draws in every call
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        video = pipe.inference(noise, prompt)
        out = (video * 255.0).clamp(0, 255).to(torch.uint8)[0].permute(0, 2, 3, 1).contiguous().cpu()     # blocks until the frames are on the host
        t = time.perf_counter() - t0
        return dict(first=t, total=t, yields=[t]), out          # the first pixel arrives with the last one

    def stream(overlap):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys, parts = [], []
        for _, frames in pipe.inference_stream(noise, prompt, output="uint8", overlap=overlap, decoder=decoder):
            ys.append(time.perf_counter() - t0)
            parts.append(frames)
        t = time.perf_counter() - t0                             # the generator has drained the decode stream
        return dict(first=ys[0], total=t, yields=ys), torch.cat(parts)

    def block_times():
        """Seconds per denoising block of one call, decode left out: device events at the hand-over points of _blocks."""
        torch.manual_seed(0)
        torch.cuda.synchronize()
        evs = []
        for _ in pipe._blocks(noise, prompt):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)
        torch.cuda.synchronize()
        return [a.elapsed_time(b) / 1e3 for a, b in zip(evs, evs[1:])]

    modes = {"stream_overlap": lambda: stream(True), "stream_in_order": lambda: stream(False)}
    if not (args.rolling or args.preview_vae):
        modes = dict(one_shot=one_shot, **modes)
    outs = {k: f()[1] for k, f in modes.items()}                 # warm-up, untimed; also: the paths give the same bytes
    same = all(torch.equal(outs["stream_overlap"], v) for v in outs.values())
    del outs
    graphs_after_warmup = pipe.graph_captures
    blocks = [block_times() for _ in range(args.rounds)]
    runs = {k: [] for k in modes}
    for _ in range(args.rounds):
        for k, f in modes.items():
            runs[k].append(f()[0])

    # decode seconds per block: the cached decode of each block's 3 latent frames alone on an idle GPU, HIP events
    lat = pipe._out[args.frames]
    dmodel = preview.model if args.preview_vae else vae.model
    dmodel.clear_cache()
    F = pipe.num_frame_per_block
    dec = []
    for s in range(0, args.frames, F):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if args.preview_vae:
            preview.decode_stream(lat[0, s:s + F], out_format="uint8")
        else:
            vae.model.decode_stream(lat[0, s:s + F], vae.mean, vae.std, out_format="uint8")
        b.record()
        b.synchronize()
        dec.append(a.elapsed_time(b) / 1e3)
    dmodel.clear_cache()

    tf = C.c_double(0.0)
    _lib.check(_lib.load().mmpl_probe_mfma_tflops(16, args.probe_seconds, C.byref(tf)), "mmpl_probe_mfma_tflops")
    med = lambda k, f: statistics.median(r[f] for r in runs[k])
    res = dict(metric="fewstep_stream_latency", model=args.model, resolution=f"{8 * geo.lat_h}x{8 * geo.lat_w}",
               latent_frames=args.frames, pixel_frames=1 + 4 * (args.frames - 1), blocks=len(dec), rounds=args.rounds,
               outputs_identical=same, probe_mfma16_tflops=tf.value, decode_s_per_block=[round(t, 4) for t in dec],
               decode_s_total=round(sum(dec), 4), decoder=decoder, rolling=args.rolling, window_frames=gen.window_frames,
               sink_size=args.sink_size, hipgraphs_constructed=pipe.graph_captures,
               hipgraphs_constructed_after_warmup=pipe.graph_captures - graphs_after_warmup)
    # per block: the median over the rounds, and the rounds' spread of the block that attends to the full window for the first time
    nb = len(blocks[0])
    bmed = [statistics.median(r[i] for r in blocks) for i in range(nb)]
    Wf = gen.window_frames
    full = [i for i in range(nb) if (i + 1) * F == min(Wf - Wf % F, args.frames)]        # the last block that ends inside the window
    past = [i for i in range(nb) if (i + 1) * F > Wf]
    res["block_s"] = [round(t, 5) for t in bmed]
    res["block_s_rounds"] = [[round(t, 5) for t in r] for r in blocks]
    if full:
        res["full_window_block"] = dict(index=full[0], s=round(bmed[full[0]], 5), spread=round(_spread([r[full[0]] for r in blocks]), 4))
    if past:
        res["steady_block_s_median"] = round(statistics.median(bmed[i] for i in past), 5)
        res["steady_block_s_min_max"] = [round(min(bmed[i] for i in past), 5), round(max(bmed[i] for i in past), 5)]
    px_frames = 1 + 4 * (args.frames - 1)
    res["video_s_per_wall_s_stream_overlap"] = round((px_frames / 16.0) / statistics.median(r["total"] for r in runs["stream_overlap"]), 4)
    for k in modes:
        res[k] = dict(first_s=round(med(k, "first"), 4), total_s=round(med(k, "total"), 4),
                      first_s_rounds=[round(r["first"], 4) for r in runs[k]], total_s_rounds=[round(r["total"], 4) for r in runs[k]],
                      first_spread=round(_spread([r["first"] for r in runs[k]]), 4),
                      total_spread=round(_spread([r["total"] for r in runs[k]]), 4),
                      yields_s=[round(t, 4) for t in runs[k][-1]["yields"]])
    if "one_shot" in modes:
        res["first_frame_ratio_stream_over_one_shot"] = round(med("stream_overlap", "first") / med("one_shot", "first"), 4)
        res["first_frame_ratio_in_order_over_one_shot"] = round(med("stream_in_order", "first") / med("one_shot", "first"), 4)
        res["total_ratio_stream_over_one_shot"] = round(med("stream_overlap", "total") / med("one_shot", "total"), 4)
    res["total_ratio_stream_over_in_order"] = round(med("stream_overlap", "total") / med("stream_in_order", "total"), 4)
    res["total_spread_max"] = round(max(res[k]["total_spread"] for k in modes), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
