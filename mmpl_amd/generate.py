"""``WanT2V`` / ``WanI2V`` -- the Wan2.1 user's public API (``wan.WanT2V(...).generate(...)`` / ``wan.WanI2V(...).generate(...)``,
wan/text2video.py, wan/image2video.py) on the HIP engine, with upstream's sampling: the noise is drawn in float32 and the latents,
the CFG combine and every tensor operation of the multistep solver stay in float32 (``mmpl_cfg_unipc_step_f32`` /
``mmpl_cfg_dpmpp_step_f32``); only the DiT sees bf16, through the bf16 rounding of the latents that upstream's autocast performs
at the patch embedding.

Each class is a ``BidirectionalDiffusionInferencePipeline`` with ``latent_dtype = torch.float32`` driven with the call's
``shift / sampling_steps / sample_solver / guide_scale``: one hipGraph per denoise step, kept per (frames, solver, steps, guidance,
shift).  Same ``generate()`` signatures, defaults and return value (float32 ``[3, N, H, W]`` in [-1, 1]) as upstream.  Differences:
  * the engine is created for ONE latent geometry (``generator.geometry``); a ``size`` / image + ``max_area`` that asks for another
    is an error, never a silent resize;
  * ``frame_num`` = 4 n + 1 with at most 24 latent frames; batch 1;
  * the forward's output is bf16 (upstream's head output is fp32 under fp32 master weights, which the engine does not keep);
  * ``use_usp`` / ``t5_fsdp`` / ``dit_fsdp`` are refused; ``offload_model``, ``t5_cpu``, ``rank``, ``init_on_cpu`` are accepted and ignored
    (everything lives on the one GPU);
  * keyword-only ``generator= / text_encoder= / vae= / clip= / device= / geometry=`` inject ready parts (synthetic weights, tests), as
    the pipelines' constructors do, and ``generate(..., noise=)`` takes the float32 ``[16, F, h, w]`` noise instead of drawing it.
"""
from __future__ import annotations

import os
import random
import sys
import types
from typing import Optional, Tuple

import numpy as np
import torch

from .pipeline import BidirectionalDiffusionInferencePipeline
from .step_cache import StepCachePolicy

VAE_STRIDE = (4, 8, 8)            # wan/configs/shared_config.py / wan_*_14B.py: the same for every released model
PATCH_SIZE = (1, 2, 2)
MAX_LATENT_FRAMES = 24


def _cfg(config, name: str, default=None):
    """config.name of upstream's EasyDict config, of a plain dict or of any namespace."""
    if isinstance(config, dict):
        return config.get(name, default)
    return getattr(config, name, default)


def latent_frames(frame_num: int) -> int:
    """text2video.py:155-158: the latent frames of `frame_num` pixel frames; 4 n + 1 frames, at most 24 latent frames."""
    if not isinstance(frame_num, int) or frame_num < 1 or (frame_num - 1) % VAE_STRIDE[0]:
        raise ValueError(f"frame_num {frame_num!r}: 4 n + 1 pixel frames (n latent frames after the first)")
    n = (frame_num - 1) // VAE_STRIDE[0] + 1
    if n > MAX_LATENT_FRAMES:
        raise ValueError(f"frame_num {frame_num}: {n} latent frames; the whole-clip forward takes at most {MAX_LATENT_FRAMES} "
                         f"({4 * (MAX_LATENT_FRAMES - 1) + 1} pixel frames)")
    return n


def t2v_latent_hw(size) -> Tuple[int, int]:
    """text2video.py:156-158: size = (width, height) in pixels -> (lat_h, lat_w)."""
    return int(size[1]) // VAE_STRIDE[1], int(size[0]) // VAE_STRIDE[2]


def i2v_latent_hw(img_h: int, img_w: int, max_area: int) -> Tuple[int, int]:
    """image2video.py:179-187, upstream's arithmetic: the latent size of the image's aspect ratio under `max_area` pixels."""
    aspect_ratio = img_h / img_w
    lat_h = round(np.sqrt(max_area * aspect_ratio) // VAE_STRIDE[1] // PATCH_SIZE[1] * PATCH_SIZE[1])
    lat_w = round(np.sqrt(max_area / aspect_ratio) // VAE_STRIDE[2] // PATCH_SIZE[2] * PATCH_SIZE[2])
    return int(lat_h), int(lat_w)


def _image_tensor(img) -> torch.Tensor:
    """`TF.to_tensor(img).sub_(0.5).div_(0.5)` (image2video.py:177) for a PIL image or an HWC uint8 array; a float tensor
    [3, H, W] is taken as already in [-1, 1]."""
    if isinstance(img, torch.Tensor):
        if img.dim() != 3 or img.shape[0] != 3 or not img.is_floating_point():
            raise ValueError(f"img: a float tensor [3, H, W] in [-1, 1], a PIL image or an HWC uint8 array; got {tuple(img.shape)} {img.dtype}")
        return img.float()
    a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"img: an RGB image (HWC uint8); got shape {a.shape} {a.dtype}")
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0).sub_(0.5).div_(0.5)


class _WanGenerate:
    """What WanT2V and WanI2V share: the constructor, the pipeline and one generate call."""

    _model_type = "t2v"

    def __init__(self, config, checkpoint_dir, device_id=0, rank=0, t5_fsdp=False, dit_fsdp=False, use_usp=False, t5_cpu=False, *,
                 generator=None, text_encoder=None, vae=None, clip=None, device=None, geometry=None):
        name = type(self).__name__
        for flag, on, why in (("use_usp", use_usp, "sequence parallelism is not built: the whole clip is denoised on one GPU"),
                              ("t5_fsdp", t5_fsdp, "the umT5 encoder is not sharded: it runs on the one GPU"),
                              ("dit_fsdp", dit_fsdp, "the DiT is not sharded: its bf16 weights live on the one GPU")):
            if on:
                raise ValueError(f"{name}: {flag}=True is not supported ({why})")
        self.device = torch.device(f"cuda:{device_id}" if device is None else device)
        self.config, self.rank, self.t5_cpu = config, rank, t5_cpu
        self.num_train_timesteps = int(_cfg(config, "num_train_timesteps", 1000))
        self.sample_neg_prompt = _cfg(config, "sample_neg_prompt", "")
        self.vae_stride, self.patch_size = VAE_STRIDE, PATCH_SIZE
        dev = str(self.device)
        if generator is None:
            from . import wan_wrapper
            rel = os.path.relpath(os.path.abspath(checkpoint_dir), os.path.abspath(wan_wrapper.local_wan_path))
            generator = wan_wrapper.WanDiffusionWrapper(model_name=rel, is_causal=False, geometry=geometry, device=dev)
        if getattr(generator, "model_type", "t2v") != self._model_type:
            raise ValueError(f"{name}: the generator is model_type {generator.model_type!r}, {name} needs {self._model_type!r}")
        if text_encoder is None:
            from .wan_wrapper import WanTextEncoder
            text_encoder = WanTextEncoder(pretrained_path=os.path.join(checkpoint_dir, _cfg(config, "t5_checkpoint", "models_t5_umt5-xxl-enc-bf16.pth")),
                                          tokenizer_path=os.path.join(checkpoint_dir, _cfg(config, "t5_tokenizer", "google/umt5-xxl")),
                                          text_len=int(_cfg(config, "text_len", 512)), device=dev)
        if vae is None:
            from .wan_wrapper import WanVAEWrapper
            vae = WanVAEWrapper(geometry=generator.geometry, device=dev,
                                pretrained_path=os.path.join(checkpoint_dir, _cfg(config, "vae_checkpoint", "Wan2.1_VAE.pth")))
        if self._model_type == "i2v" and clip is None:
            from .checkpoints import read_clip_visual
            from .i2v_clip import CLIPVisionTower
            clip = CLIPVisionTower(device=dev)
            clip.load_state_dict(read_clip_visual(os.path.join(
                checkpoint_dir, _cfg(config, "clip_checkpoint", "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth"))))
        self.clip = clip
        args = types.SimpleNamespace(num_train_timestep=self.num_train_timesteps, guidance_scale=5.0, negative_prompt=self.sample_neg_prompt)
        self.pipeline = BidirectionalDiffusionInferencePipeline(args, dev, generator=generator, text_encoder=text_encoder, vae=vae)
        self.pipeline.latent_dtype = torch.float32
        self.model, self.text_encoder, self.vae = generator, text_encoder, vae

    def _check_geometry(self, lat_h: int, lat_w: int, asked: str) -> None:
        g = self.pipeline.geometry
        if (lat_h, lat_w) != (g.lat_h, g.lat_w):
            raise ValueError(f"{type(self).__name__}.generate: {asked} asks for {lat_h} x {lat_w} latents ({8 * lat_h} x {8 * lat_w} pixels), "
                             f"this engine was created for {g.lat_h} x {g.lat_w} ({8 * g.lat_h} x {8 * g.lat_w} pixels); build it with "
                             "that geometry -- nothing is resized silently")

    def _noise(self, noise: Optional[torch.Tensor], n_frames: int, seed: int) -> torch.Tensor:
        """Upstream's draw (text2video.py:166-191): float32 [16, F, h, w] from a device generator seeded with `seed` (random if < 0);
        -> the pipeline's layout [1, F, 16, h, w]."""
        g = self.pipeline.geometry
        shape = (16, n_frames, g.lat_h, g.lat_w)
        if noise is None:
            seed = seed if seed >= 0 else random.randint(0, sys.maxsize)
            seed_g = torch.Generator(device=self.device)
            seed_g.manual_seed(seed)
            noise = torch.randn(*shape, dtype=torch.float32, device=self.device, generator=seed_g)
        elif tuple(noise.shape) != shape or noise.dtype != torch.float32:
            raise ValueError(f"noise: float32 {list(shape)} (upstream's layout, channels first); got {noise.dtype} {list(noise.shape)}")
        return noise.to(self.device).permute(1, 0, 2, 3).unsqueeze(0).contiguous()

    def _generate(self, input_prompt, noise, shift, sample_solver, sampling_steps, guide_scale, n_prompt, image_condition=None,
                  teacache_thresh=0.0, teacache_coefficients=None, use_ret_steps=False):
        if sample_solver not in ("unipc", "dpm++"):
            raise NotImplementedError("Unsupported solver.")
        if int(sampling_steps) < 1:
            raise ValueError(f"sampling_steps {sampling_steps}: at least 1")
        p = self.pipeline
        # TeaCache4Wan2.1's arguments: 0 = every step computed -- the sampler as it is (no policy, nothing allocated)
        p.step_cache = None
        if teacache_thresh and float(teacache_thresh) > 0:
            kw = {} if teacache_coefficients is None else {"coefficients": tuple(teacache_coefficients)}
            if use_ret_steps:                                # upstream: the first 5 steps computed, no forced last step, e0 the indicator
                kw.update(ret_steps=5, cutoff=int(sampling_steps), indicator="e0")
            p.step_cache = StepCachePolicy(float(teacache_thresh), **kw)
        p.shift, p.sampling_steps, p.sample_solver = float(shift), int(sampling_steps), sample_solver
        p.args.guidance_scale = float(guide_scale)
        p.args.negative_prompt = self.sample_neg_prompt if n_prompt == "" else n_prompt
        latents = p.sample(noise, [input_prompt], image_condition)                       # float32 [1, F, 16, h, w]
        with torch.no_grad():
            video = self.vae.decode_to_pixel(latents.to(torch.bfloat16))                 # [1, T, 3, H, W] in [-1, 1]
        return video[0].permute(1, 0, 2, 3).float().contiguous(), latents

    def release_graphs(self) -> None:
        self.pipeline.release_graphs()


class WanT2V(_WanGenerate):
    """wan/text2video.py WanT2V: ``WanT2V(config, checkpoint_dir).generate(prompt, size=(1280, 720), ...)``."""

    _model_type = "t2v"

    def generate(self, input_prompt, size=(1280, 720), frame_num=81, shift=5.0, sample_solver='unipc', sampling_steps=50,
                 guide_scale=5.0, n_prompt="", seed=-1, offload_model=True, *, noise: Optional[torch.Tensor] = None,
                 return_latents: bool = False, teacache_thresh: float = 0.0, teacache_coefficients=None, use_ret_steps: bool = False):
        """-> float32 [3, frame_num, H, W] in [-1, 1] (with `return_latents` also the float32 latents [1, F, 16, h, w]).
        `teacache_thresh` > 0: step caching (mmpl_amd/step_cache.py) with the polynomial `teacache_coefficients` (highest power
        first; None = identity); `use_ret_steps`: the first 5 steps computed, no forced last step, the indicator e0."""
        n = latent_frames(frame_num)
        self._check_geometry(*t2v_latent_hw(size), asked=f"size={tuple(size)}")
        video, latents = self._generate(input_prompt, self._noise(noise, n, seed), shift, sample_solver, sampling_steps, guide_scale, n_prompt,
                                        teacache_thresh=teacache_thresh, teacache_coefficients=teacache_coefficients,
                                        use_ret_steps=use_ret_steps)
        return (video, latents) if return_latents else video


class WanI2V(_WanGenerate):
    """wan/image2video.py WanI2V: ``WanI2V(config, checkpoint_dir).generate(prompt, img, max_area=720 * 1280, ...)`` over a
    model_type 'i2v' generator.  The image is resized (bicubic, as image2video.py:239-241) to the clip's pixel size where it has
    another one; the conditioning is ``i2v_condition.build_image_condition``."""

    _model_type = "i2v"

    def __init__(self, config, checkpoint_dir, device_id=0, rank=0, t5_fsdp=False, dit_fsdp=False, use_usp=False, t5_cpu=False,
                 init_on_cpu=True, **injected):
        super().__init__(config, checkpoint_dir, device_id, rank, t5_fsdp, dit_fsdp, use_usp, t5_cpu, **injected)

    def generate(self, input_prompt, img, max_area=720 * 1280, frame_num=81, shift=5.0, sample_solver='unipc', sampling_steps=40,
                 guide_scale=5.0, n_prompt="", seed=-1, offload_model=True, *, noise: Optional[torch.Tensor] = None,
                 return_latents: bool = False, teacache_thresh: float = 0.0, teacache_coefficients=None, use_ret_steps: bool = False):
        """-> float32 [3, frame_num, H, W] in [-1, 1] (with `return_latents` also the float32 latents [1, F, 16, h, w]).
        `teacache_thresh`, `teacache_coefficients`, `use_ret_steps`: step caching, as in `WanT2V.generate`."""
        from .i2v_condition import build_image_condition
        n = latent_frames(frame_num)
        image = _image_tensor(img)
        lat_h, lat_w = i2v_latent_hw(image.shape[1], image.shape[2], max_area)
        self._check_geometry(lat_h, lat_w, asked=f"a {image.shape[1]} x {image.shape[2]} image under max_area={max_area}")
        if tuple(image.shape[1:]) != (8 * lat_h, 8 * lat_w):
            image = torch.nn.functional.interpolate(image[None], size=(8 * lat_h, 8 * lat_w), mode="bicubic")[0]
        condition = build_image_condition(self.vae, self.clip, image.to(self.device), n)
        video, latents = self._generate(input_prompt, self._noise(noise, n, seed), shift, sample_solver, sampling_steps, guide_scale, n_prompt,
                                        image_condition=condition, teacache_thresh=teacache_thresh,
                                        teacache_coefficients=teacache_coefficients, use_ret_steps=use_ret_steps)
        return (video, latents) if return_latents else video
