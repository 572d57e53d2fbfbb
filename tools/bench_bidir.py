"""Whole-clip (bidirectional) step time, text-to-video and image-to-video side by side in ONE process: for each model type a
BidirectionalDiffusionInferencePipeline with synthetic weights, step 1 run eagerly and captured (2 forwards + CFG / UniPC = one
hipGraph), then that graph replayed on the same latents and step-table position: warm-up replays first, the median of the timed
ones reported.  One eager forward per model type is timed per kernel class (mmpl_profile_*); the image stream's share of an I2V
forward is its cross-attention time minus the T2V forward's, plus the bf16 add.  Prints one JSON line.

    python tools/bench_bidir.py --model 1.3B --resolution 480p
    python tools/bench_bidir.py --model 14B --resolution 720p --reps 3

--latent_chains: the text-to-video step graph under the two latent chains instead (bfloat16 = the reference pipeline's, float32 =
upstream WanT2V.generate's: `latent_dtype`), same process, same box.  --chain_gap STEPS: both chains run STEPS steps from the same
float32 noise (the bf16 chain from its rounding); reports the rel-L2 between their final latents.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ["gemm", "attn_self", "attn_cross", "layernorm", "qknorm", "elementwise", "unipc", "vae"]


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def measure(model_type, args, cfg, geo, dev, latent_dtype=torch.bfloat16):
    from mmpl_amd import _lib
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.synthetic import dit_i2v_state_dict, dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper
    lib = _lib.load()
    cfg = dict(cfg, model_type=model_type)
    i2v = model_type == "i2v"
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=5.0, model_config=cfg, geometry=geo, device=dev)
    gen.load_state_dict((dit_i2v_state_dict if i2v else dit_state_dict)(cfg, seed=1234, device=dev))
    pargs = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="")
    enc = SyntheticTextEncoder(cfg.get("text_dim", 4096), dev)
    pipe = BidirectionalDiffusionInferencePipeline(pargs, dev, generator=gen, text_encoder=enc, vae=_NoVAE())
    pipe.latent_dtype = latent_dtype
    noise = philox_normal([1, args.frames, 16, geo.lat_h, geo.lat_w], 7, torch.float32).to(latent_dtype).to(dev)
    pipe.crossattn_cache_pos, pipe.crossattn_cache_neg = gen.new_crossattn_cache(), gen.new_crossattn_cache()
    pipe.crossattn_cache_pos.fill(enc(["a cat running on the grass"])["prompt_embeds"][0])
    pipe.crossattn_cache_neg.fill(enc([""])["prompt_embeds"][0])
    st = pipe._step_state(noise)
    if i2v:
        st["y"].copy_(philox_normal([args.frames, 20, geo.lat_h, geo.lat_w], 8).to(torch.bfloat16).to(dev))
        gen.set_image(philox_normal([257, 1280], 9).to(torch.bfloat16).to(dev))

    def rewind():                                          # every run is step 1 on the same latents
        st["latents"].copy_(noise[0])
        if st["latents_bf16"] is not None:
            st["latents_bf16"].copy_(st["latents"])
        st["sched"].reset_step_table(st["t"])

    rewind()
    pipe._step(st)                                         # eager: first launches set their attributes outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pipe._step(st)
    times = []
    for i in range(args.warmup + args.reps):
        rewind()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            times.append(a.elapsed_time(b))
    # one eager forward, per kernel class
    rewind()
    n = len(KINDS)
    ms, fl, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)()
    lib.mmpl_profile_enable(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    gen.flow_full(st["latents"] if st["latents_bf16"] is None else st["latents_bf16"], st["t"], pipe.crossattn_cache_pos, out=st["flow"][0], **({"y": st["y"]} if i2v else {}))
    b.record()
    lib.mmpl_profile_read(n, ms, fl, cnt)
    lib.mmpl_profile_enable(0)
    torch.cuda.synchronize()
    return dict(step_graph_ms_median=statistics.median(times), step_graph_ms=[round(t, 2) for t in times], concurrent_cfg=st["concurrent"],
                eager_forward_ms=a.elapsed_time(b), eager_ms={k: round(ms[i], 3) for i, k in enumerate(KINDS) if cnt[i]},
                eager_launches={k: cnt[i] for i, k in enumerate(KINDS) if cnt[i]})


def chain_gap(args, cfg, geo, dev):
    """Both latent chains over `args.chain_gap` steps of the text-to-video pipeline (UniPC, shift 5, guidance 5) on the same weights,
    prompt and float32 noise -> rel-L2 of the bf16 chain's final latents to the float32 chain's."""
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.synthetic import dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=5.0, model_config=cfg, geometry=geo, device=dev)
    gen.load_state_dict(dit_state_dict(cfg, seed=1234, device=dev))
    pargs = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="")
    pipe = BidirectionalDiffusionInferencePipeline(pargs, dev, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), dev),
                                                   vae=_NoVAE())
    pipe.sampling_steps, pipe.shift = args.chain_gap, 5.0
    noise = philox_normal([1, args.frames, 16, geo.lat_h, geo.lat_w], 7, torch.float32).to(dev)
    out = {}
    for dt in (torch.float32, torch.bfloat16):
        pipe.latent_dtype = dt
        out[dt] = pipe.sample(noise.to(dt), ["a cat running on the grass"]).double()
        torch.cuda.synchronize()
    gap = ((out[torch.bfloat16] - out[torch.float32]).norm() / out[torch.float32].norm()).item()
    return dict(steps=args.chain_gap, solver="unipc", shift=5.0, guidance=5.0, rel_l2_bf16_chain_vs_float32_chain=gap,
                rms_float32_chain=out[torch.float32].pow(2).mean().sqrt().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.3B", choices=["1.3B", "14B", "tiny", "small"])
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--latent_hw", type=int, nargs=2, default=None)
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe_seconds", type=float, default=2.0)
    ap.add_argument("--latent_chains", action="store_true", help="t2v under latent_dtype bfloat16 and float32 instead of t2v and i2v")
    ap.add_argument("--chain_gap", type=int, default=0, metavar="STEPS", help="rel-L2 between the two latent chains' final latents")
    args = ap.parse_args()

    from mmpl_amd import _lib
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    cfg = WAN_CONFIGS[args.model]
    geo = Geometry(*args.latent_hw) if args.latent_hw else Geometry.named(args.resolution)
    res = {}
    if args.chain_gap:
        print(json.dumps(dict(metric="latent_chain_gap", model=args.model, resolution=args.resolution, frames=args.frames,
                              weights="synthetic", **chain_gap(args, cfg, geo, dev))))
        return
    if args.latent_chains:
        for name, dt in (("bfloat16", torch.bfloat16), ("float32", torch.float32), ("bfloat16_again", torch.bfloat16)):
            res[name] = measure("t2v", args, cfg, geo, dev, latent_dtype=dt)
            print(f"[bench_bidir] t2v {name}: step graph {res[name]['step_graph_ms_median']:.1f} ms", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        probe = {}
        for shape in (32, 16):
            tf = C.c_double(0.0)
            _lib.check(_lib.load().mmpl_probe_mfma_tflops(shape, args.probe_seconds, C.byref(tf)), "mmpl_probe_mfma_tflops")
            probe[f"mfma{shape}_tflops"] = round(tf.value, 1)
        print(json.dumps(dict(metric="bidirectional_step_graph_latent_chains", model=args.model, resolution=args.resolution,
                              frames=args.frames, rows=args.frames * geo.frame_seqlen, warmup=args.warmup, reps=args.reps, **res,
                              float32_over_bfloat16_step=res["float32"]["step_graph_ms_median"] / res["bfloat16"]["step_graph_ms_median"],
                              **probe)))
        return
    for mt in ("t2v", "i2v"):
        res[mt] = measure(mt, args, cfg, geo, dev)
        print(f"[bench_bidir] {mt}: step graph {res[mt]['step_graph_ms_median']:.1f} ms", file=sys.stderr, flush=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    probe = {}
    for shape in (32, 16):
        tf = C.c_double(0.0)
        _lib.check(_lib.load().mmpl_probe_mfma_tflops(shape, args.probe_seconds, C.byref(tf)), "mmpl_probe_mfma_tflops")
        probe[f"mfma{shape}_tflops"] = round(tf.value, 1)
    t, i = res["t2v"], res["i2v"]
    img_ms = i["eager_ms"].get("attn_cross", 0.0) - t["eager_ms"].get("attn_cross", 0.0)
    add_ms = i["eager_ms"].get("elementwise", 0.0)
    print(json.dumps(dict(metric="bidirectional_step_graph", model=args.model, resolution=args.resolution, frames=args.frames,
                          rows=args.frames * geo.frame_seqlen, warmup=args.warmup, reps=args.reps, t2v=t, i2v=i,
                          i2v_over_t2v_step=i["step_graph_ms_median"] / t["step_graph_ms_median"],
                          image_attention_ms=round(img_ms, 3), image_add_ms=round(add_ms, 3),
                          image_stream_share_of_i2v_forward=(img_ms + add_ms) / i["eager_forward_ms"], **probe)))


if __name__ == "__main__":
    main()
