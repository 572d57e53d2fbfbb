"""Entry point with the reference's CLI (MMPL_t2v/Wan_fps_inference_1gpu.py:21-36 and the `_parallel_4gpu_*` scripts).

    python -m mmpl_amd.cli --config_path configs/self_forcing_df.yaml --checkpoint_path t2v_14B_8k.pt \
           --data_path prompts.txt --output_folder out --duration 2 --seed 0
    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 -m mmpl_amd.cli ... --duration 4     # chunk wavefront, RCCL hand-off

Single process = the reference's sequential rollout (chunk k+1 starts from the last 5 pixel frames of chunk k,
`Wan_fps_inference_1gpu.py:164-203`); several processes = the parallel scripts' wavefront (chunk c on rank c mod W,
anchors handed over right after the anchor stage).  `--bidirectional` = plain Wan2.1 T2V instead: one whole clip per call
(the reference's Bidirectional*InferencePipeline); with `--i2v --i2v_model --image FILE` the Wan2.1-I2V model type sampled the
same way (upstream WanI2V.generate's forward; `--fp32_latents` = upstream's float32 latent chain instead of the reference
pipeline's bf16 one).  `--synthetic` runs without checkpoints (seeded weights and text
embeddings) -- the only mode that can run in this repo's test environments.  Output: per prompt a uint8 tensor
`[T, H, W, 3]` saved with torch.save (mp4 muxing via torchvision is outside the hot path; fps = 16).
"""
from __future__ import annotations

import argparse
import os
import types

import torch
import yaml

from .geometry import Geometry
from .handoff import (CfgPair, ChunkHandoff, handoff_to_initial_latent, rolling_initial_latent, run_chunk_wavefront,
                      stitch_chunks)
from .synthetic import WAN_CONFIGS, dit_state_dict, vae_state_dict

DEFAULTS = dict(num_train_timestep=1000, timestep_shift=5.0, guidance_scale=5.0, independent_first_frame=False,
                negative_prompt="", model_kwargs={"timestep_shift": 5.0})


def load_config(path):
    cfg = dict(DEFAULTS)
    if path:
        with open(path) as f:
            cfg.update(yaml.safe_load(f) or {})
    return types.SimpleNamespace(**cfg)


def is_fewstep(config) -> bool:
    """Wan_fps_inference_1gpu.py:59-64: a config with `denoising_step_list` is a few-step (Self-Forcing / CausVid) checkpoint."""
    return hasattr(config, "denoising_step_list")


def pipeline_class(config, bidirectional: bool = False):
    """The pipeline the reference's entry script builds for `config` (Wan_fps_inference_1gpu.py:59-64); with --bidirectional the
    whole-clip counterpart of either (pipeline/__init__.py of the reference)."""
    from .pipeline import (BidirectionalDiffusionInferencePipeline, BidirectionalInferencePipeline, CausalFPSInferencePipeline,
                           CausalInferencePipeline)
    if bidirectional:
        return BidirectionalInferencePipeline if is_fewstep(config) else BidirectionalDiffusionInferencePipeline
    return CausalInferencePipeline if is_fewstep(config) else CausalFPSInferencePipeline


def bidirectional_refusal(args, world: int):
    """Why --bidirectional cannot run this command line (None = it can, or it was not asked for).  The bidirectional pipelines
    denoise ONE whole clip per call on one process: there is no chunk rollout, no block to stream or to roll a KV window over
    (there is no KV cache), and no second rank to give a CFG branch to.  Image conditioning exists as the Wan-I2V MODEL TYPE only
    (--i2v --i2v_model --image FILE): the whole-clip model has no "image latent as frame 0" mode, which is what --i2v alone means."""
    if not getattr(args, "bidirectional", False):
        return None
    if args.duration > 1:
        return (f"--duration {args.duration}: --bidirectional generates one {args.num_output_frames}-latent-frame clip per call "
                "(use --duration 1)")
    if args.i2v and not args.i2v_model:
        return ("--i2v: --bidirectional has no 'image latent as frame 0' mode; its image-to-video is the Wan-I2V model type "
                "(--i2v --i2v_model --image FILE)")
    if args.i2v_model and not (args.i2v and getattr(args, "image", None)):
        return "--i2v_model needs --i2v --image FILE (with --bidirectional as without)"
    if args.i2v_model and getattr(args, "fewstep", False):
        return "--i2v --i2v_model: the few-step bidirectional pipeline (config with denoising_step_list) is text-to-video only"
    if getattr(args, "sample_shift", None) is not None and getattr(args, "fewstep", False):
        return "--sample_shift: the few-step bidirectional pipeline follows its denoising_step_list and has no sampling shift"
    if getattr(args, "stream", False):
        return "--stream: --bidirectional denoises the whole clip at once; there are no blocks to hand out"
    if getattr(args, "rolling", False):
        return "--rolling: --bidirectional has no KV cache to roll a window over"
    if getattr(args, "preview_vae", None) is not None:
        return "--preview_vae: the tiny preview decoder serves --stream only; --bidirectional decodes with the Wan VAE"
    if getattr(args, "cfg_split", False):
        return "--cfg_split: --bidirectional runs both CFG branches on one process"
    if world > 1:
        return "--bidirectional runs on one process (WORLD_SIZE 1)"
    if args.num_output_frames < 1 or args.num_output_frames > 24:
        return f"--num_output_frames {args.num_output_frames}: the whole-clip forward takes 1 .. 24 latent frames"
    return None


def fewstep_refusal(args, world: int):
    """Why the few-step pipeline cannot run this command line (None = it can).  The reference's rollout loop feeds 2 overlap
    latent frames back and trips `num_input_frames % num_frame_per_block == 0` from rollout 2 on (causal_inference.py:153);
    its I2V image latent is 1 frame; it has no multi-rank few-step path.  With --rolling (the rolling KV window, which the
    reference does not have) --duration N is ONE call of N * num_output_frames latent frames instead."""
    if args.duration > 1 and not getattr(args, "rolling", False):
        return (f"--duration {args.duration}: the few-step pipeline (config with denoising_step_list) generates one "
                f"{args.num_output_frames}-latent-frame call; longer rollouts are not supported (use --duration 1)")
    if args.i2v or args.i2v_model:
        return "--i2v: the few-step pipeline (config with denoising_step_list) is text-to-video only"
    if world > 1:
        return "the few-step pipeline (config with denoising_step_list) runs on one process (WORLD_SIZE 1)"
    return None


def stream_refusal(args, fewstep: bool):
    """Why --stream cannot run this command line (None = it can, or it was not asked for): block-wise output exists for the
    few-step pipeline only (CausalInferencePipeline.inference_stream)."""
    if getattr(args, "stream", False) and not fewstep:
        return ("--stream: block-wise output needs a few-step config (one with denoising_step_list, e.g. self_forcing_dmd.yaml); "
                "the 50-step pipeline does not stream")
    return None


def rolling_refusal(args, fewstep: bool):
    """Why --rolling cannot run this command line (None = it can, or it was not asked for): the rolling KV window belongs to the
    few-step pipeline (CausalInferencePipeline, args.rolling_kv); the 50-step pipeline rolls over chunks by itself."""
    if getattr(args, "rolling", False) and not fewstep:
        return ("--rolling: the rolling KV window needs a few-step config (one with denoising_step_list, e.g. self_forcing_dmd.yaml); "
                "the 50-step pipeline generates --duration chunks without it")
    return None


def preview_refusal(args):
    """Why --preview_vae cannot run this command line (None = it can, or it was not asked for): the tiny TAEHV decoder serves the
    block-wise output only (CausalInferencePipeline.inference_stream(decoder="preview")); a whole video is decoded by the Wan VAE."""
    if getattr(args, "preview_vae", None) is not None and not getattr(args, "stream", False):
        return ("--preview_vae: the tiny preview decoder (TAEHV, taew2_1.pth) decodes the live frames of --stream only; "
                "add --stream, or drop --preview_vae to decode with the Wan VAE")
    return None


def solver_refusal(args, fewstep: bool):
    """Why --sample_solver cannot run this command line (None = it can): the multistep solvers (UniPC, DPM-Solver++) sample the
    50-step pipeline; a few-step config walks its own denoising_step_list and has no solver to choose."""
    if fewstep and getattr(args, "sample_solver", "unipc") != "unipc":
        return (f"--sample_solver {args.sample_solver}: the few-step pipeline (config with denoising_step_list) follows its "
                "denoising_step_list and has no multistep solver; drop --sample_solver or use a 50-step config")
    return None


def fp32_refusal(args, fewstep: bool):
    """Why --fp32_latents cannot run this command line (None = it can, or it was not asked for): upstream Wan2.1's float32 latent
    chain (WanT2V.generate / WanI2V.generate) belongs to the whole-clip multistep sampler alone."""
    if not getattr(args, "fp32_latents", False):
        return None
    if not getattr(args, "bidirectional", False):
        return ("--fp32_latents: the float32 latent chain is upstream WanT2V.generate / WanI2V.generate's, the whole-clip sampler; "
                "add --bidirectional (the causal FPS pipeline keeps the reference's bf16 latents)")
    if fewstep:
        return ("--fp32_latents: the few-step pipeline (config with denoising_step_list) has no multistep solver and keeps its "
                "reference's bf16 latents; use a 50-step config")
    return None


MAX_FORWARD_FRAMES = 8               # the engine's largest forward (MmplDitConfig.max_frames at most): what a batch's samples share


def sample_groups(n_samples: int, num_frame_per_block: int, max_frames: int = MAX_FORWARD_FRAMES):
    """--num_samples N as consecutive slices [lo, hi) of at most ``max_frames // num_frame_per_block`` samples: one
    CausalInferencePipeline.inference call each (a call's samples run as ONE forward of samples x block frames)."""
    g = max(max_frames // max(num_frame_per_block, 1), 1)
    return [(lo, min(lo + g, n_samples)) for lo in range(0, n_samples, g)]


def samples_refusal(args, fewstep: bool):
    """Why --num_samples N cannot run this command line (None = it can, or N is 1): several samples per prompt are the few-step
    causal pipeline's batched inference() (one noise draw [N, F, 16, h, w], as the reference's --num_samples)."""
    n = int(getattr(args, "num_samples", 1))
    if n == 1:
        return None
    if n < 1:
        return f"--num_samples {n}: at least 1"
    if not fewstep:
        return ("--num_samples: batched generation needs a few-step config (one with denoising_step_list, e.g. self_forcing_dmd.yaml); "
                "the 50-step pipeline generates one sample per prompt")
    if getattr(args, "bidirectional", False):
        return "--num_samples: the --bidirectional pipelines denoise one whole clip per call; batched generation is the causal few-step pipeline's"
    if getattr(args, "stream", False):
        return "--num_samples: --stream hands out ONE video block by block (inference_stream keeps batch size 1); drop --stream"
    if getattr(args, "extend", None):
        return "--num_samples: --extend continues one clip on the streaming path, which keeps batch size 1"
    block = int(getattr(args, "num_frame_per_block", 1))
    if block > MAX_FORWARD_FRAMES:
        return f"--num_samples: num_frame_per_block {block} exceeds the engine's largest forward ({MAX_FORWARD_FRAMES} frames)"
    return None


def read_clip(path: str) -> torch.Tensor:
    """A clip as this CLI writes it -> uint8 [T, H, W, 3] on the host: the ``.pt`` tensor, or the MJPEG ``.avi`` of
    utils/video_io.py."""
    if path.lower().endswith(".avi"):
        from .utils.video_io import read_mjpeg_avi
        return torch.from_numpy(read_mjpeg_avi(path).copy())
    clip = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(clip, torch.Tensor) or clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[-1] != 3:
        raise ValueError("not a uint8 [T, H, W, 3] tensor")
    return clip


def extend_context_frames(args) -> int:
    """--extend_context in latent frames (default: one block, num_frame_per_block)."""
    n = getattr(args, "extend_context", None)
    return int(getattr(args, "num_frame_per_block", 1)) if n is None else int(n)


def extend_refusal(args, fewstep: bool):
    """Why --extend FILE cannot run this command line (None = it can, or it was not asked for).  The clip's last 4 N frames are
    encoded by the tiny autoencoder's encoder (TAEHVWrapper.encode_stream) into N latent frames, handed to the few-step pipeline
    as ``initial_latent``, and the new blocks are streamed and decoded by the same autoencoder: hence a few-step config, --stream
    and --preview_vae.  ``main`` puts num_frame_per_block, kv_window (the KV window in latent frames) and pixel_hw on ``args``."""
    path = getattr(args, "extend", None)
    if path is None:
        if getattr(args, "extend_context", None) is not None:
            return "--extend_context: only with --extend FILE"
        return None
    if not fewstep:
        return ("--extend: continuing a clip needs a few-step config (one with denoising_step_list, e.g. self_forcing_dmd.yaml); "
                "the 50-step pipeline rolls over its own chunks")
    if getattr(args, "bidirectional", False):
        return "--extend: --bidirectional denoises one whole clip; there is no earlier video to continue"
    if getattr(args, "i2v", False) or getattr(args, "i2v_model", False):
        return "--extend: the few-step pipeline (config with denoising_step_list) is text-to-video only; drop --i2v"
    if not getattr(args, "stream", False) or getattr(args, "preview_vae", None) is None:
        return ("--extend: the context is encoded, and the new blocks decoded, by the tiny preview autoencoder on the streaming "
                "path: add --stream --preview_vae [PATH] (a Wan-VAE-encoded context is not supported)")
    block = int(getattr(args, "num_frame_per_block", 1))
    n = extend_context_frames(args)
    if n < block or n % block:
        return f"--extend_context {n}: a positive multiple of num_frame_per_block ({block}) latent frames"
    new = int(getattr(args, "num_output_frames", 21)) * int(getattr(args, "duration", 1))
    window = int(getattr(args, "kv_window", 21))
    if not getattr(args, "rolling", False) and n + new > window:
        return (f"--extend: {n} context + {new} new latent frames do not fit the KV window of {window} frames; add --rolling or "
                f"use a smaller --num_output_frames (at most {window - n})")
    if not os.path.isfile(path):
        return f"--extend {path}: no such file"
    try:
        clip = read_clip(path)
    except Exception as e:
        return f"--extend {path}: not a clip this CLI wrote (.pt uint8 [T, H, W, 3], or its MJPEG .avi): {e}"
    if clip.shape[0] < 4 * n:
        return f"--extend {path}: {clip.shape[0]} frames, the context of {n} latent frames needs {4 * n}"
    hw = getattr(args, "pixel_hw", None)
    if hw is not None and tuple(clip.shape[1:3]) != tuple(hw):
        return f"--extend {path}: frames of {clip.shape[1]} x {clip.shape[2]} pixels, this run generates {hw[0]} x {hw[1]}"
    return None


def step_cache_coefficients(text: str):
    """--teacache_coefficients a,b,...: the rescaling polynomial, highest power first."""
    return tuple(float(c) for c in text.split(","))


def step_cache_policy(args):
    """The StepCachePolicy of --teacache_thresh / --teacache_coefficients / --teacache_ret_steps; None without --teacache_thresh
    (step caching off: the pipelines as they are).  --teacache_ret_steps is upstream TeaCache's use_ret_steps: the first 5 steps
    and nothing at the end forced, the indicator e0."""
    thresh = getattr(args, "teacache_thresh", None)
    if thresh is None:
        return None
    from .step_cache import StepCachePolicy
    coeff = getattr(args, "teacache_coefficients", None)
    kw = dict(coefficients=step_cache_coefficients(coeff)) if coeff else {}
    if getattr(args, "teacache_ret_steps", False):
        kw.update(ret_steps=5, cutoff=int(args.sampling_steps), indicator="e0")
    return StepCachePolicy(float(thresh), **kw)


def step_cache_refusal(args, world: int, fewstep: bool):
    """Why --teacache_thresh cannot run this command line (None = it can, or it was not asked for): step caching skips steps of
    the 50-step multistep samplers of one process."""
    if getattr(args, "teacache_thresh", None) is None:
        for flag in ("teacache_coefficients", "teacache_ret_steps"):
            if getattr(args, flag, None):
                return f"--{flag}: only with --teacache_thresh X"
        return None
    if args.teacache_thresh < 0:
        return f"--teacache_thresh {args.teacache_thresh}: at least 0 (0 computes every step)"
    if int(getattr(args, "num_samples", 1)) > 1:
        return "--teacache_thresh: batched generation (--num_samples) runs the grouped forward, which has no cached form"
    if fewstep:
        return ("--teacache_thresh: the few-step pipeline (config with denoising_step_list) runs 4 steps that all differ; step "
                "caching belongs to the 50-step samplers")
    if world > 1 or getattr(args, "cfg_split", False):
        return ("--teacache_thresh: step caching is single-process (the two CFG branches' residuals live on one GPU); run without "
                "torchrun / --cfg_split")
    coeff = getattr(args, "teacache_coefficients", None)
    if coeff:
        try:
            ok = len(step_cache_coefficients(coeff)) >= 1
        except ValueError:
            ok = False
        if not ok:
            return f"--teacache_coefficients {coeff}: comma-separated numbers, highest power first (numpy.poly1d order)"
    return None


def first_refusal(args, world: int, fewstep: bool):
    """The first reason this command line cannot run, asked in ``main``'s order (None = it can).  ``main`` has put fewstep,
    num_frame_per_block, kv_window and pixel_hw on ``args``."""
    checks = (lambda: bidirectional_refusal(args, world), lambda: stream_refusal(args, fewstep), lambda: preview_refusal(args),
              lambda: rolling_refusal(args, fewstep), lambda: solver_refusal(args, fewstep),
              lambda: fp32_refusal(args, fewstep),
              lambda: fewstep_refusal(args, world) if fewstep and not args.bidirectional else None,
              lambda: extend_refusal(args, fewstep), lambda: samples_refusal(args, fewstep),
              lambda: step_cache_refusal(args, world, fewstep))
    return next((why for why in (check() for check in checks) if why is not None), None)


def _prompts(args):
    if args.data_path:
        from .utils.dataset import TextDataset
        ds = TextDataset(args.data_path)
        return [ds[i]["prompts"] for i in range(len(ds))]
    return ["a cat running on the grass"]


def _to_u8(video: torch.Tensor) -> torch.Tensor:
    """[1, T, 3, H, W] in [0, 1] -> uint8 frames (Wan_fps_inference_1gpu.py:209-225 scales by 255 before write_video)"""
    return (video * 255.0).clamp(0, 255).to(torch.uint8)


def _save_clip(frames: torch.Tensor, args, idx: int, what: str = "", sample: int = 0) -> None:
    """uint8 frames, [1, T, 3, H, W] or already the written layout [T, H, W, 3] on the host -> ``idx``-``sample``.pt (torch.save)
    and the video file next to it (Wan_fps_inference_1gpu.py:225)."""
    out = frames[0].permute(0, 2, 3, 1).contiguous().cpu() if frames.dim() == 5 else frames
    path = os.path.join(args.output_folder, f"{idx}-{sample}.pt")
    torch.save(out, path)
    from .utils.video_io import write_video
    vpath = write_video(os.path.join(args.output_folder, f"{idx}-{sample}.mp4"), out, fps=16)
    print(f"[mmpl_amd.cli] {what}prompt {idx}: {tuple(out.shape)} frames @16 fps -> {vpath} (+ {path})")


def _load_image(path: str, geo, dev) -> torch.Tensor:
    """The image at the clip's pixel size, [3, H, W] bf16 in [-1, 1] on the device: Resize -> ToTensor -> Normalize(0.5, 0.5)
    (I2V/Wan_fps_inference_1gpu.py:74-79, image2video.py:186-246)."""
    import numpy as np
    from PIL import Image
    H, W = geo.pixel_hw
    img = Image.open(path).convert("RGB").resize((W, H), Image.BILINEAR)
    px = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float() / 255.0
    return ((px - 0.5) / 0.5).to(device=dev, dtype=torch.bfloat16)


def _build_models(args, dev, geo, mcfg, make_generator, i2v_dir=None):
    """(generator, text encoder, VAE, CLIP tower) of a run.  ``make_generator(model_config)`` builds the wrapper (model_config None:
    from the checkpoint directory).  --synthetic: seeded weights, text embeddings and VAE; otherwise the encoder and the VAE are
    None, i.e. the pipeline's own defaults: the reference checkpoints under ../wan_models (wan_wrapper.local_wan_path).
    ``i2v_dir``: the Wan-I2V model type, whose CLIP ViT-H weights lie in that directory.  --checkpoint_path is loaded last."""
    from .wan_wrapper import SyntheticTextEncoder, WanVAEWrapper
    i2v, clip = i2v_dir is not None, None
    if i2v:
        from .i2v_clip import CLIPVisionTower
        mcfg = dict(mcfg, model_type="i2v")
        tiny_clip = args.synthetic and args.model in ("tiny", "small")      # tests: 3 blocks instead of ViT-H's 32
        clip = CLIPVisionTower(num_layers=3 if tiny_clip else 32, device=dev)
    gen = make_generator(mcfg if args.synthetic else None)
    if i2v and gen.model_type != "i2v":
        raise SystemExit("--i2v_model: the checkpoint directory does not hold a model_type 'i2v' config")
    enc, vae = None, None
    if args.synthetic:
        if i2v:
            from .synthetic import clip_visual_state_dict, dit_i2v_state_dict
            gen.load_state_dict(dit_i2v_state_dict(mcfg, seed=1, device=dev))
            clip.load_state_dict(clip_visual_state_dict(1280, 16, clip.num_layers, seed=3, device=dev))
        else:
            gen.load_state_dict(dit_state_dict(mcfg, seed=1, device=dev))
        enc = SyntheticTextEncoder(mcfg.get("text_dim", 4096), dev)
        vae = WanVAEWrapper(geometry=geo, device=dev, state_dict=vae_state_dict(seed=2))
    elif i2v:
        from .checkpoints import read_clip_visual
        from .wan_wrapper import local_wan_path
        clip.load_state_dict(read_clip_visual(f"{local_wan_path}/{i2v_dir}/models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth"))
    if args.checkpoint_path:
        from .checkpoints import read_mmpl_checkpoint
        gen.load_state_dict(read_mmpl_checkpoint(args.checkpoint_path, use_ema=args.use_ema))
    return gen, enc, vae, clip


def build_preview_vae(args, dev, geo):
    """TAEHVWrapper for --preview_vae [PATH]: the checkpoint at PATH (default ../wan_models/taew2_1.pth), or seeded weights with
    --synthetic (both halves: the decoder, and the encoder --extend needs)."""
    from .wan_wrapper import TAEHVWrapper
    if args.synthetic:
        from .synthetic import taehv_encoder_state_dict, taehv_state_dict
        return TAEHVWrapper(geometry=geo, device=dev, state_dict={**taehv_state_dict(seed=4), **taehv_encoder_state_dict(seed=5)})
    path = args.preview_vae or None
    if path is not None and not os.path.exists(path):
        raise SystemExit(f"--preview_vae {path}: no such file")
    w = TAEHVWrapper(geometry=geo, device=dev, pretrained_path=path)
    if not w.model._weights:
        raise SystemExit("--preview_vae: no TAEHV checkpoint found (pass its path, e.g. --preview_vae ../wan_models/taew2_1.pth)")
    return w


def build_fewstep_pipeline(config, args, dev, geo, mcfg):
    """WanDiffusionWrapper + CausalInferencePipeline (Wan_fps_inference_1gpu.py:61), then `independent_first_frame = False`
    as the entry script sets it (:73)."""
    from .pipeline import CausalInferencePipeline
    from .wan_wrapper import WanDiffusionWrapper
    kw = dict(getattr(config, "model_kwargs", {}) or {})
    for name in ("local_attn_size", "sink_size"):                        # --local_attn_size / --sink_size override the config's
        if getattr(args, name, None) is not None:
            kw[name] = getattr(args, name)
    config.rolling_kv = bool(getattr(args, "rolling", False))
    gen, enc, vae, _ = _build_models(args, dev, geo, mcfg, lambda model_config: WanDiffusionWrapper(
        "Wan2.1-T2V-14B" if args.model == "14B" else "Wan2.1-T2V-1.3B", **kw, is_causal=True, model_config=model_config, geometry=geo,
        device=dev, **({"max_frames": MAX_FORWARD_FRAMES} if int(getattr(args, "num_samples", 1)) > 1 else {})))
    preview = build_preview_vae(args, dev, geo) if getattr(args, "preview_vae", None) is not None else None
    pipe = CausalInferencePipeline(config, dev, generator=gen, text_encoder=enc, vae=vae, preview_vae=preview)
    pipe.independent_first_frame = False
    return pipe


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_path", type=str)
    ap.add_argument("--checkpoint_path", type=str)
    ap.add_argument("--data_path", type=str)
    ap.add_argument("--output_folder", type=str, default="outputs")
    ap.add_argument("--num_output_frames", type=int, default=21)
    ap.add_argument("--use_ema", action="store_true")
    ap.add_argument("--i2v", action="store_true", help="image-to-video: the VAE-encoded image is latent frame 0 (MMPL_i2v)")
    ap.add_argument("--image", type=str, help="input image for --i2v (any PIL-readable file)")
    ap.add_argument("--i2v_model", action="store_true",
                    help="with --i2v: the Wan-I2V MODEL TYPE (in_dim 36, CLIP ViT-H image cross-attention in every block; Wan2.1-I2V-14B, "
                         "BASELINE configs[4]) instead of the T2V backbone MMPL's own I2V scripts run; the conditioning video y and the CLIP "
                         "features are rebuilt per chunk from the chunk's first pixel frame (wan/image2video.py:207-246)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--duration", type=int, default=3, help="number of 21-latent-frame chunks")
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--model", default="14B", choices=list(WAN_CONFIGS))
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights / text embeddings (no checkpoints needed)")
    ap.add_argument("--sampling_steps", type=int, default=None,
                    help="solver steps of the 50-step pipelines: default 50, or 40 for --bidirectional --i2v_model (WanI2V.generate)")
    ap.add_argument("--sample_shift", type=float, default=None,
                    help="--bidirectional only: the sampling schedule's shift; default 8.0 (the reference's text-to-video pipeline), or "
                         "for --i2v_model WanI2V.generate's 5.0 (3.0 at --resolution 480p)")
    ap.add_argument("--sample_solver", default="unipc", choices=["unipc", "dpm++"],
                    help="the multistep solver of the 50-step pipeline: FlowUniPCMultistepScheduler or FlowDPMSolverMultistepScheduler "
                         "(DPM-Solver++(2M)), as in Wan2.1's generate.py")
    ap.add_argument("--fp32_latents", action="store_true",
                    help="--bidirectional with a 50-step config (T2V, or --i2v --i2v_model): upstream WanT2V.generate / WanI2V.generate's "
                         "latent chain -- float32 noise, latents, CFG combine and solver, only the DiT's input rounded to bf16 -- instead "
                         "of the reference pipeline's bf16 chain")
    ap.add_argument("--latent_hw", type=int, nargs=2, default=None, help="override the latent size (tests)")
    ap.add_argument("--cfg_split", action="store_true",
                    help="multi-GPU: WORLD/2 chunk lanes x (cond, uncond) rank pairs -- the reference's device_cond/device_uncond "
                         "seam -- instead of WORLD chunk lanes")
    ap.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (one rank per GPU); gloo stages the hand-off through the host and lets several ranks "
                         "share one GPU (tests on 1-GPU boxes)")
    ap.add_argument("--stream", action="store_true",
                    help="few-step configs: decode and hand out the video block by block while the next block denoises "
                         "(CausalInferencePipeline.inference_stream); prints the time to the first frames and per block")
    ap.add_argument("--preview_vae", type=str, nargs="?", const="", default=None, metavar="PATH",
                    help="with --stream: decode the live frames with the tiny TAEHV preview decoder (taew2_1.pth at PATH, default "
                         "../wan_models/taew2_1.pth; seeded weights with --synthetic) instead of the Wan VAE")
    ap.add_argument("--rolling", action="store_true",
                    help="few-step configs: rolling KV window (evict the oldest frame that is not a sink frame), so that "
                         "--duration N generates N * num_output_frames latent frames in ONE call, with --stream as well")
    ap.add_argument("--bidirectional", action="store_true",
                    help="plain (non-causal) Wan2.1 T2V: the whole --num_output_frames clip per forward, every frame attending to "
                         "every frame -- BidirectionalDiffusionInferencePipeline (--sampling_steps CFG steps of --sample_solver on the "
                         "reference's bf16 latent chain, or on upstream generate.py's float32 one with --fp32_latents), or "
                         "BidirectionalInferencePipeline for a few-step config (one with denoising_step_list).  With --i2v --i2v_model "
                         "--image FILE: the Wan2.1-I2V-14B-480P / -720P model type sampled the same way (WanI2V.generate's forward and "
                         "defaults; its float32 latent chain too with --fp32_latents)")
    ap.add_argument("--local_attn_size", type=int, default=None, help="few-step configs: override model_kwargs.local_attn_size "
                    "(the KV window in latent frames; -1 = 21)")
    ap.add_argument("--sink_size", type=int, default=None, help="few-step configs: override model_kwargs.sink_size (the first "
                    "frames of the video that --rolling never evicts)")
    ap.add_argument("--extend", type=str, default=None, metavar="FILE",
                    help="few-step configs with --stream --preview_vae: continue FILE, a clip this CLI wrote (.pt uint8 [T, H, W, 3] or "
                         "its MJPEG .avi) -- its last frames are encoded by the tiny autoencoder into the pipeline's initial_latent "
                         "and --num_output_frames NEW latent frames follow; the written clip is the context frames plus the new ones")
    ap.add_argument("--num_samples", type=int, default=1, metavar="N",
                    help="few-step configs: N videos per prompt from ONE noise draw [N, F, 16, h, w] (the reference's --num_samples), "
                         "written as {idx}-{sample}; 8 // num_frame_per_block samples run per call as one batched forward.  With more "
                         "samples than that the re-noise draws follow call by call, so they match the reference's order only up to "
                         "that many")
    ap.add_argument("--extend_context", type=int, default=None, metavar="N",
                    help="with --extend: latent frames of context (the clip's last 4 N frames); default num_frame_per_block, a multiple of it")
    ap.add_argument("--teacache_thresh", type=float, default=None, metavar="X",
                    help="50-step pipelines, one process: step caching (TeaCache) -- a denoise step whose timestep embedding moved less "
                         "than X (accumulated relative L1, rescaled by --teacache_coefficients) since the last computed step reuses that "
                         "step's residual and runs only the head; 0 computes every step (bit-identical to no flag)")
    ap.add_argument("--teacache_coefficients", type=str, default=None, metavar="a,b,...",
                    help="with --teacache_thresh: the rescaling polynomial, highest power first (the TeaCache project's per-model fit; "
                         "none is built in: the default is the identity)")
    ap.add_argument("--teacache_ret_steps", action="store_true",
                    help="with --teacache_thresh: upstream TeaCache's use_ret_steps -- the first 5 steps always computed, no forced "
                         "last step, the indicator e0 (the projected embedding) instead of e")
    args = ap.parse_args(argv)
    i2v_clip = bool(args.bidirectional and args.i2v_model)               # the whole-clip Wan-I2V model type: WanI2V.generate's defaults
    if args.sampling_steps is None:
        args.sampling_steps = 40 if i2v_clip else 50
    if args.sample_shift is not None and not args.bidirectional:
        ap.error("--sample_shift: only the --bidirectional pipelines take a sampling shift (the causal ones read timestep_shift "
                 "from the config)")
    if args.sample_shift is None and i2v_clip:
        args.sample_shift = 3.0 if args.resolution == "480p" else 5.0

    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    config = load_config(args.config_path)
    fewstep = is_fewstep(config)
    args.fewstep = fewstep
    geo = Geometry(*args.latent_hw) if args.latent_hw else Geometry.named(args.resolution)
    las = args.local_attn_size if args.local_attn_size is not None else (getattr(config, "model_kwargs", None) or {}).get("local_attn_size", -1)
    args.num_frame_per_block = int(getattr(config, "num_frame_per_block", 1))
    args.kv_window = geo.frames_per_chunk if int(las) == -1 else int(las)
    args.pixel_hw = tuple(geo.pixel_hw)
    why = first_refusal(args, world, fewstep)
    if why is not None:
        ap.error(why)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dist_backend == "gloo":
        local_rank %= max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # ChunkHandoff.recv / CfgPair.broadcast park a rank until the previous lane has finished its anchor stage: minutes per
        # lane at 14B/720p, far beyond the 10-minute default watchdog once there are more than a few lanes
        dist.init_process_group(args.dist_backend, timeout=datetime.timedelta(hours=12))
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    torch.set_grad_enabled(False)

    from .pipeline import CausalFPSInferencePipeline
    from .wan_wrapper import WanFPSWrapper
    mcfg = WAN_CONFIGS[args.model]
    if args.bidirectional:
        return _main_bidirectional(config, args, dev, geo, mcfg)
    if fewstep:
        return _main_fewstep(config, args, dev, geo, mcfg)
    config.sampling_steps = args.sampling_steps
    config.sample_solver = args.sample_solver
    if args.i2v_model and not (args.i2v and args.image):
        ap.error("--i2v_model needs --i2v --image")
    i2v_dir = "Wan2.1-I2V-14B-720P" if args.i2v_model else None
    gen, enc, vae, clip = _build_models(args, dev, geo, mcfg, lambda model_config: WanFPSWrapper(
        i2v_dir or "Wan2.1-T2V-14B", **config.model_kwargs, is_causal=True, model_config=model_config, geometry=geo, device=dev), i2v_dir)
    mode = "i2v" if args.i2v else "t2v"
    pipe = CausalFPSInferencePipeline(config, dev, generator=gen, text_encoder=enc, vae=vae, device_cond=dev, device_uncond=dev, save=None,
                                      mode=mode, geometry=geo)
    pipe.step_cache = step_cache_policy(args)
    image_latent, first_px = None, None
    if args.i2v:                                 # I2V/Wan_fps_inference_1gpu.py:100-104: the image -> vae.encode_to_latent
        first_px = _load_image(args.image, geo, dev)
        image_latent = pipe.vae.encode_to_latent(first_px[None, :, None]).to(torch.bfloat16)         # [1, 3, 1, H, W] -> [1, 1, 16, h, w]

    def image_cond(frame):
        """the Wan-I2V model type's conditioning for a chunk whose first pixel frame is `frame` ([3, H, W] in [-1, 1])"""
        if clip is None:
            return None
        if frame is None:
            # the uncond rank of a CFG pair has no frame: pipeline.inference overwrites both tensors with the cond rank's broadcast,
            # so only the shapes matter -- no CLIP tower, no 81-frame VAE encode of a zero clip on the rank that paces the pair
            return {"clip_fea": torch.empty(257, 1280, device=dev, dtype=torch.bfloat16),
                    "y": torch.empty(20, args.num_output_frames, geo.lat_h, geo.lat_w, device=dev, dtype=torch.bfloat16)}
        from .i2v_condition import build_image_condition
        return build_image_condition(pipe.vae, clip, frame, args.num_output_frames)

    os.makedirs(args.output_folder, exist_ok=True)
    shape = [1, args.num_output_frames, 16, geo.lat_h, geo.lat_w]
    for idx, prompt in enumerate(_prompts(args)):
        # noise for every chunk is drawn in order from one seeded generator on every rank (the reference draws it on the
        # main thread in chunk order, ..._parallel_4gpu_20s.py:170,232-251)
        g = torch.Generator(device="cpu").manual_seed(args.seed)
        noises = [torch.randn(shape, generator=g).to(torch.bfloat16) for _ in range(args.duration)]
        if world == 1:
            videos, initial, frame0 = [], image_latent, first_px
            for c in range(args.duration):
                video, _ = pipe.inference(noises[c].to(dev), [prompt], initial_latent=initial, return_latents=True,
                                          image_condition=image_cond(frame0))
                initial = rolling_initial_latent(pipe.vae, video)
                frame0 = video[0, -5].to(torch.bfloat16) * 2.0 - 1.0       # the next chunk starts at this chunk's 5th-last frame
                videos.append(_to_u8(video))
        else:
            pair, heads, lay = (CfgPair.build(world, dev, True) if args.cfg_split else (None, None, None))
            pipe.cfg_pair = pair
            rank = dist.get_rank()
            ho = (ChunkHandoff((1, 3 if args.i2v else 8, 16, geo.lat_h, geo.lat_w), dev, group=heads)
                  if pair is None or pair.role == 0 else None)

            frame_of = {0: first_px}

            def to_initial(c_recv):
                init, frame = handoff_to_initial_latent(pipe.vae, c_recv.to(dev), return_first_frame=True)
                frame_of["next"] = frame
                return init

            def make_chunk(c, initial, sink):
                pipe.handoff_sink = sink
                pipe.handoff_poll = ho.poll if ho is not None else None
                if c == 0:
                    initial = image_latent
                video, _ = pipe.inference(noises[c].to(dev), [prompt], initial_latent=initial, return_latents=True,
                                          image_condition=image_cond(frame_of[0] if c == 0 else frame_of.get("next")))
                return _to_u8(video)        # quantised on the owner: the device all-gather moves 224 MB per 720p chunk, not 896

            videos = run_chunk_wavefront(make_chunk, args.duration, ho, to_initial,
                                         pair=pair, lane=lay["lane_of"][rank] if lay else rank, n_lanes=world // 2 if lay else world,
                                         initial_like=torch.empty([1, 2, 16, geo.lat_h, geo.lat_w], device=dev, dtype=torch.bfloat16))
        if videos is not None:
            _save_clip(stitch_chunks(videos), args, idx)                     # [1, T, 3, H, W] uint8
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _main_fewstep(config, args, dev, geo, mcfg):
    """Wan_fps_inference_1gpu.py with a few-step config: one CausalInferencePipeline.inference per prompt (--rolling: of
    --duration * num_output_frames latent frames; fewstep_refusal keeps --duration at 1 otherwise)."""
    pipe = build_fewstep_pipeline(config, args, dev, geo, mcfg)
    os.makedirs(args.output_folder, exist_ok=True)
    n_samples = int(getattr(args, "num_samples", 1))
    shape = [n_samples, args.num_output_frames * args.duration, 16, geo.lat_h, geo.lat_w]
    context_px, initial = None, None
    if getattr(args, "extend", None):
        # --extend FILE: the clip's last 4 N frames -> N latent frames (a video of their own, from zero memories) = initial_latent
        if pipe.preview_vae.encoder is None:
            raise SystemExit("--extend: the --preview_vae checkpoint has no 'encoder.*' tensors to encode the context with")
        context_px = read_clip(args.extend)[-4 * extend_context_frames(args):].contiguous()
        pipe.preview_vae.encoder.clear_cache()
        initial = pipe.preview_vae.encode_stream(context_px.to(dev)).unsqueeze(0)                              # [1, N, 16, h, w]
        pipe.preview_vae.encoder.clear_cache()
    for idx, prompt in enumerate(_prompts(args)):
        g = torch.Generator(device="cpu").manual_seed(args.seed)
        noise = torch.randn(shape, generator=g).to(torch.bfloat16)
        torch.manual_seed(args.seed)                         # the re-noise draws: the device generator (set_seed, :44-49)
        if args.stream:
            import time
            parts, t0 = [], time.perf_counter()
            decoder = "preview" if pipe.preview_vae is not None else "vae"
            for first, frames in pipe.inference_stream(noise.to(dev), [prompt], initial_latent=initial, output="uint8", decoder=decoder):
                if context_px is not None and not parts:     # the context's own decode: the clip keeps the file's frames instead
                    parts.append(context_px)
                    continue
                if context_px is not None:                   # frame numbers of the written clip: the context keeps all 4 N frames
                    first = sum(p.shape[0] for p in parts)
                print(f"[mmpl_amd.cli] few-step prompt {idx}: frames {first}..{first + frames.shape[0] - 1} after "
                      f"{time.perf_counter() - t0:.3f} s" + (" (time to the first frames)" if not parts else ""))
                parts.append(frames)
            out = torch.cat(parts)                                                                             # [T, H, W, 3]
        elif n_samples > 1:
            # ONE noise draw for all samples (Wan_fps_inference_1gpu.py:132-155); each call takes the next slice of it and draws its
            # own re-noise [samples, F, 16, h, w] per step from the device generator, call after call
            for lo, hi in sample_groups(n_samples, pipe.num_frame_per_block, pipe.generator.engine.max_frames):
                video = _to_u8(pipe.inference(noise[lo:hi].to(dev), [prompt] * (hi - lo), return_latents=False))
                for k in range(lo, hi):
                    _save_clip(video[k - lo:k - lo + 1], args, idx, "few-step ", sample=k)
            continue
        else:
            out = _to_u8(pipe.inference(noise.to(dev), [prompt], return_latents=False))
        _save_clip(out, args, idx, "few-step ")


def i2v_model_name(args) -> str:
    """The released whole-clip I2V checkpoints' directories under ../wan_models: one per resolution."""
    return "Wan2.1-I2V-14B-480P" if args.resolution == "480p" else "Wan2.1-I2V-14B-720P"


def build_bidirectional_pipeline(config, args, dev, geo, mcfg):
    """WanDiffusionWrapper(is_causal=False) + the bidirectional pipeline `pipeline_class` picks for `config`; with --i2v_model the
    generator is the Wan-I2V model type and the pipeline gets `clip`, the CLIP ViT-H tower its image conditioning needs."""
    from .wan_wrapper import WanDiffusionWrapper
    i2v_dir = i2v_model_name(args) if getattr(args, "i2v_model", False) else None
    kw = {k: v for k, v in dict(getattr(config, "model_kwargs", {}) or {}).items() if k in ("model_name", "timestep_shift")}
    if i2v_dir is not None:
        kw["model_name"] = i2v_dir
    kw.setdefault("model_name", "Wan2.1-T2V-14B" if args.model == "14B" else "Wan2.1-T2V-1.3B")
    gen, enc, vae, clip = _build_models(args, dev, geo, mcfg, lambda model_config: WanDiffusionWrapper(
        **kw, is_causal=False, model_config=model_config, geometry=geo, device=dev), i2v_dir)
    pipe = pipeline_class(config, bidirectional=True)(config, dev, generator=gen, text_encoder=enc, vae=vae)
    pipe.clip = clip
    if not is_fewstep(config):
        pipe.sampling_steps = args.sampling_steps
        pipe.sample_solver = args.sample_solver
        if getattr(args, "fp32_latents", False):
            pipe.latent_dtype = torch.float32
        if getattr(args, "sample_shift", None) is not None:
            pipe.shift = float(args.sample_shift)
        pipe.step_cache = step_cache_policy(args)
    return pipe


def _main_bidirectional(config, args, dev, geo, mcfg):
    """--bidirectional: one whole-clip inference() of --num_output_frames latent frames per prompt."""
    pipe = build_bidirectional_pipeline(config, args, dev, geo, mcfg)
    os.makedirs(args.output_folder, exist_ok=True)
    shape = [1, args.num_output_frames, 16, geo.lat_h, geo.lat_w]
    extra = {}
    if args.i2v_model:
        # image2video.py:186-246: the image at the clip's pixel size in [-1, 1] -> CLIP tokens + the conditioning video y
        from .i2v_condition import build_image_condition
        extra["image_condition"] = build_image_condition(pipe.vae, pipe.clip, _load_image(args.image, geo, dev), args.num_output_frames)
    for idx, prompt in enumerate(_prompts(args)):
        g = torch.Generator(device="cpu").manual_seed(args.seed)
        noise = torch.randn(shape, generator=g).to(getattr(pipe, "latent_dtype", torch.bfloat16))      # (--fp32_latents: as drawn)
        torch.manual_seed(args.seed)                         # the few-step re-noise draws: the device generator
        _save_clip(_to_u8(pipe.inference(noise.to(dev), [prompt], **extra)), args, idx, "bidirectional ")


if __name__ == "__main__":
    main()
