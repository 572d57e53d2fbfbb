"""Few-step (Self-Forcing / CausVid) throughput: CausalInferencePipeline with synthetic weights, one call to warm up (it runs
every block eagerly once and captures its hipGraph), then every block's graph replayed once and timed with HIP events.
Prints one JSON line.

    python tools/bench_fewstep.py --model 1.3B --resolution 480p
    python tools/bench_fewstep.py --model 14B --resolution 720p
    python tools/bench_fewstep.py --model 1.3B --resolution 480p --block 1 --num_samples 8

--num_samples B: one batched call (noise [B, frames, ...], B equal prompts): every block's forwards run over B * block frames, the
self-attention as one grouped launch; B * block <= 8.  Times are per block of B samples; frames/s are given per sample and in total.
--lib PATH: load that build of the library instead of the tree's (the same benchmark on another commit's kernels, same process set-up).

Algorithmic FLOPs per forward: the block GEMMs (2 * rows * (6 d^2 + 2 d ffn) per layer), the self-attention against every
visible cached frame (4 * rows * keys * d) and the text cross-attention (4 * rows * 512 * d); a block costs n + 1 forwards.
The VAE decode is not timed.
"""
import argparse
import ctypes as C
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def forward_flops(cfg, S, n_frames, n_keys_frames, text_len=512):
    d, f, L = cfg["dim"], cfg["ffn_dim"], cfg["num_layers"]
    rows = n_frames * S
    per_layer = 2 * rows * (6 * d * d + 2 * d * f) + 4 * rows * n_keys_frames * S * d + 4 * rows * text_len * d
    return L * per_layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.3B", choices=["1.3B", "14B", "tiny", "small"])
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--frames", type=int, default=21, help="latent frames of the call")
    ap.add_argument("--reps", type=int, default=1, help="timed passes over all block graphs")
    ap.add_argument("--probe_seconds", type=float, default=2.0)
    ap.add_argument("--block", type=int, default=3, help="num_frame_per_block")
    ap.add_argument("--num_samples", type=int, default=1, help="samples of the one batched call")
    ap.add_argument("--local_attn_size", type=int, default=-1, help="KV window in latent frames (-1 = 21): a batch's cache holds "
                    "num_samples windows, at 14B / 720p 62 GB of K and V per window of 21")
    ap.add_argument("--lib", type=str, default=None, help="another build of libmmpl_hip.so to load")
    args = ap.parse_args()

    from mmpl_amd import _lib
    if args.lib:                       # (an older build lacks the entries added since: bind what it has)
        _lib.LIB_PATH = args.lib
        have = C.CDLL(args.lib)
        _lib._PROTOS = {k: v for k, v in _lib._PROTOS.items() if hasattr(have, k)}
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    cfg = WAN_CONFIGS[args.model]
    geo = Geometry.named(args.resolution)
    config = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=args.block,
                                   independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    B = args.num_samples
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, local_attn_size=args.local_attn_size, model_config=cfg, geometry=geo, device=dev,
                              **({"max_frames": 8} if B > 1 else {}))
    gen.load_state_dict(dit_state_dict(cfg, seed=1234, device=dev))
    pipe = CausalInferencePipeline(config, dev, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), dev),
                                   vae=_NoVAE())
    noise = torch.randn(B, args.frames, 16, geo.lat_h, geo.lat_w, device=dev, dtype=torch.bfloat16)
    pipe.inference(noise, ["a cat running on the grass"] * B)      # warm-up: eager blocks + graph capture (not timed)
    torch.cuda.synchronize()
    graphs = list(pipe._graphs.items())
    times = [0.0] * len(graphs)
    for _ in range(args.reps):
        for i, (_, g) in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[i] += a.elapsed_time(b) / 1e3 / args.reps
    n = len(pipe.denoising_step_list)
    S = geo.frame_seqlen
    flops = 0
    frames = 0
    for (start, F, *_), _ in graphs:
        keys = min(start + F, gen.window_frames)
        flops += B * (n + 1) * forward_flops(cfg, S, F, keys)
        frames += F
    total = sum(times)
    tf = C.c_double(0.0)
    _lib.check(_lib.load().mmpl_probe_mfma_tflops(16, args.probe_seconds, C.byref(tf)), "mmpl_probe_mfma_tflops")
    print(json.dumps(dict(
        metric="fewstep_block_graph_replay", model=args.model, resolution=args.resolution, latent_frames=frames, num_samples=B,
        window_frames=gen.window_frames,
        latent_frames_per_s_all_samples=B * frames / total,
        blocks=len(graphs), frames_per_block=pipe.num_frame_per_block, steps=n, forwards_per_block=n + 1,
        s_per_block=total / len(graphs), s_per_block_each=[round(t, 4) for t in times], s_total=total,
        latent_frames_per_s=frames / total, pixel_frames_per_s=(1 + 4 * (frames - 1)) / total,
        algorithmic_tflop=flops / 1e12, algorithmic_tflops_per_s=flops / total / 1e12,
        probe_mfma16_tflops=tf.value, frac_of_probe=flops / total / 1e12 / tf.value if tf.value else None)))


if __name__ == "__main__":
    main()
