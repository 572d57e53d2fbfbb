"""``BidirectionalDiffusionInferencePipeline`` -- drop-in for MMPL_t2v/pipeline/bidirectional_diffusion_inference.py: plain
Wan2.1 text-to-video sampling: the whole clip is denoised at once, every frame attending to every frame, by ``sampling_steps``
multistep-solver steps under classifier-free guidance.  The forward and the schedule are upstream ``WanT2V.generate``'s; the latent
chain is chosen by ``latent_dtype``: ``torch.bfloat16`` (default) is the reference pipeline's -- bf16 noise, bf16 latents, a bf16
rounding after every tensor operation of the solver --, ``torch.float32`` is upstream ``WanT2V.generate``'s -- float32 noise, latents,
CFG combine and solver (``mmpl_cfg_*_step_f32``), the forwards reading the bf16 rounding of the latents that the solver kernel writes
next to them (``mmpl_amd.generate.WanT2V`` / ``WanI2V`` wrap that mode in upstream's ``generate()`` signature).

Same constructor / ``inference()`` signature and attributes (``generator``, ``text_encoder``, ``vae``, ``num_train_timesteps``,
``sampling_steps`` = 50, ``sample_solver`` = 'unipc' ('dpm++' accepted), ``shift`` = 8.0 -- hard-coded there too, ``args.timestep_shift``
is not read --, ``args``) and the same semantics.  What changed underneath:
  * a denoise step = the cond forward + the uncond forward (``mmpl_dit_forward_full``: no KV cache, the layer's K / V live in the
    workspace) + the fused CFG / solver update reading its scalars and writing the next timestep on the device
    (``step_cfg_table``), and with ``use_graphs`` that is ONE hipGraph, replayed ``sampling_steps`` times with no host work in
    between.  It is captured once per (frame count, solver, steps, guidance) and kept for the pipeline's lifetime
    (``release_graphs()`` drops it); ``use_graphs = False`` issues the same launches eagerly: the same bits;
  * block 0's self-attention is the same computation in both CFG branches, so the uncond forward takes x after it from the cond
    forward (share_out / share_in) where the two run back to back; where ``concurrent_cfg_pays`` says so they run as parallel
    branches of the graph instead (second stream, private workspace);
  * the frame count is ``noise.shape[1]`` where the reference writes the literal 21; batch size 1;
  * ``step_cache`` (a ``mmpl_amd.step_cache.StepCachePolicy``; None = off: nothing of this exists) runs fewer forwards (TeaCache):
    the steps the policy skips reuse the residual the last computed step left and run only the head.  The indicator is the timestep
    embedding, so the schedule is computed once per step shape before sampling (one ``time_embed`` over the timestep table, one
    ``rel_l1_rows``, one read-back).  Each step kind is its own graph, captured on first use -- two RECORD forwards + the solver
    kernel, two REUSE forwards + the same solver kernel --, and the host replays the one the schedule names.
    ``computed_steps`` / ``skipped_steps`` count the last call's.

Over a ``model_type='i2v'`` generator (the released Wan2.1-I2V-14B-480P / -720P weights) this is upstream ``WanI2V.generate``'s
forward and conditioning (wan/image2video.py): ``inference(..., image_condition={"clip_fea": [257, 1280], "y": [20, F, h, w]})`` from
``i2v_condition.build_image_condition(vae, clip, image, n_latent_frames=F)``, the argument ``CausalFPSInferencePipeline.inference``
has.  The step state gains a static frame-major ``y`` buffer that every forward of the step graph reads next to the latents
(``mmpl_dit_forward_full_i2v``: no concatenation, no copy inside the graph); per call ``y`` is copied in and the generator's
image K / V are rebuilt in place, so another image replays the SAME graph.  Both CFG branches see the image (upstream's
``arg_null`` carries ``clip_fea`` and ``y`` too), so block 0 is still shared.  The latent chain is ``latent_dtype``'s, as for
text-to-video: bf16 by default, upstream ``WanI2V.generate``'s float32 one with ``torch.float32``.  ``shift``
and ``sampling_steps`` keep the defaults above -- ``WanI2V.generate``'s own (40 steps, shift 5.0, or 3.0 at 480p) are the caller's
to set, as ``mmpl_amd.cli`` does.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ..dit import CACHE_OFF, CACHE_RECORD, CACHE_REUSE
from ..step_cache import StepCachePolicy, step_schedule
from ._common import (GeneratorPipeline, cfg_concurrent, cfg_step, cfg_step_buffers, decode_video, eager_then_capture,
                      make_sample_scheduler)


class BidirectionalDiffusionInferencePipeline(GeneratorPipeline):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None):
        super().__init__()
        self._set_generator(args, device, generator, is_causal=False)
        if getattr(self.generator, "is_causal", False):
            raise ValueError("BidirectionalDiffusionInferencePipeline needs WanDiffusionWrapper(is_causal=False)")
        self.i2v = getattr(self.generator, "model_type", "t2v") == "i2v"
        self._set_codecs(text_encoder, vae, device)

        self.num_train_timesteps = args.num_train_timestep
        self.sampling_steps = 50
        self.sample_solver = 'unipc'
        self.shift = 8.0
        # the latent chain: bfloat16 = the reference pipeline's (bf16 noise, latents and solver); float32 = upstream
        # WanT2V.generate / WanI2V.generate's (float32 noise, latents, CFG combine and solver; the forwards read a bf16 shadow)
        self.latent_dtype = torch.bfloat16

        self.args = args

        self.use_graphs = True            # one hipGraph per denoise step (2 forwards + CFG / solver update)
        self.concurrent_cfg: Optional[bool] = None    # None = where concurrent_cfg_pays says so; True / False = always / never
        self.share_block0 = True          # sequential branches: the uncond forward takes block 0's self-attention from the cond one
        self.graph_captures = 0           # hipGraphs constructed so far (tests: none after the first call)
        self.step_cache: Optional[StepCachePolicy] = None    # TeaCache: which steps reuse the last computed step's residual (None = off)
        self.computed_steps = 0           # the last call's steps that ran the blocks / that reused a residual
        self.skipped_steps = 0
        self._steps: Dict[tuple, dict] = {}     # (frames, solver, steps, guidance, concurrent, share, latent dtype, shift) -> static buffers, scheduler, graph
        self._stores = (self._steps,)
        self._side_stream = None
        self.crossattn_cache_pos = None
        self.crossattn_cache_neg = None

    # ------------------------------------------------------------------------------------------------------------
    def _initialize_sample_scheduler(self, noise):
        """bidirectional_diffusion_inference.py:89-110: the solver `sample_solver` names, `self.timesteps` set to its schedule."""
        s, self.timesteps = make_sample_scheduler(self.sample_solver, self.num_train_timesteps, self.sampling_steps, self.shift, noise.device)
        return s

    def _step_state(self, noise: torch.Tensor) -> dict:
        """Static buffers, the scheduler with its device step table and (later) the graph of one step shape."""
        F = noise.shape[1]
        engine, dev = self.generator.engine, self.device
        concurrent = cfg_concurrent(self, engine, F)
        if self.latent_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"latent_dtype {self.latent_dtype}: torch.bfloat16 (the reference pipeline's chain) or torch.float32 (upstream's)")
        key = (F, self.sample_solver, int(self.sampling_steps), float(self.args.guidance_scale), concurrent,
               bool(self.share_block0 and not concurrent), self.latent_dtype, float(self.shift))
        if self.step_cache is not None:                                   # its own buffers, schedule and graphs; off: the key as it was
            key += (self.step_cache.key(),)
        st = self._steps.get(key)
        if st is None:
            g = self.geometry
            shape = (F, 16, g.lat_h, g.lat_w)
            sched = self._initialize_sample_scheduler(noise)
            latents = torch.empty(shape, dtype=self.latent_dtype, device=dev)
            sched._ensure_state(latents)                                  # (first: the state's dtype is the scheduler's mode)
            sched.build_step_table(self.args.guidance_scale, dev)
            # float32 chain: the forwards read the bf16 rounding of the latents, which the solver kernel writes next to them
            shadow = torch.empty(shape, dtype=torch.bfloat16, device=dev) if self.latent_dtype == torch.float32 else None
            st = dict(latents=latents, latents_bf16=shadow, flow=torch.empty((2,) + shape, dtype=torch.bfloat16, device=dev),
                      t=torch.empty(1, dtype=torch.float32, device=dev), sched=sched, n=len(sched.timesteps), graph=None,
                      timesteps=self.timesteps, concurrent=concurrent,
                      # i2v: the conditioning video, frame-major, read by both forwards of every step and never written by them
                      y=torch.empty((F, engine.in_dim - 16, g.lat_h, g.lat_w), dtype=torch.bfloat16, device=dev) if self.i2v else None)
            engine.full_workspace(F)                                      # allocations and the stream: outside any capture
            st["share"], st["ws2"] = cfg_step_buffers(self, engine, F, concurrent, lambda n: engine.full_workspace(n, second=True), dev)
            if self.step_cache is not None:
                # per step True = compute; one residual per CFG branch; one graph per step kind, captured on first use
                st["schedule"] = step_schedule(engine, self.step_cache, sched._t_table)
                st["residual"] = (engine.new_step_cache(F), engine.new_step_cache(F))
                st["graphs"] = {}
            self._steps[key] = st
        return st

    def _step(self, st: dict, cache_mode: int = CACHE_OFF) -> None:
        """One denoise step's launches (bidirectional_diffusion_inference.py:62-76): eager, or recorded into the step graph.
        `cache_mode`: CACHE_RECORD / CACHE_REUSE for a computed / a reused step under `step_cache`."""
        caches = (self.crossattn_cache_pos, self.crossattn_cache_neg)
        kw = {} if st["y"] is None else {"y": st["y"]}                    # i2v: both branches see the image (image2video.py arg_null)
        x_in = st["latents"] if st["latents_bf16"] is None else st["latents_bf16"]
        cache = (lambda bi: {}) if cache_mode == CACHE_OFF else (lambda bi: {"cache_mode": cache_mode, "residual": st["residual"][bi]})
        cfg_step(lambda bi, out, **k: self.generator.flow_full(x_in, st["t"], caches[bi], out=out, **k, **kw, **cache(bi)),
                 st["sched"], st["flow"], st["latents"], st["t"], self.device, self._side_stream if st["concurrent"] else None,
                 st["share"], st["ws2"], latents_bf16=st["latents_bf16"])

    def inference(self, noise: torch.Tensor, text_prompts: List[str], return_latents=False,
                  image_condition: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """noise [1, F, 16, h, w] (F up to 24; with ``latent_dtype = torch.float32`` float32 noise is used unrounded and the returned
        latents are float32).  Returns video [1, T, 3, 8h, 8w] in [0, 1] (and the latents [1, F, 16, h, w]).
        `image_condition`: {"clip_fea": [257, 1280], "y": [20, F, h, w]} (i2v_condition.build_image_condition) -- required over an
        i2v generator, a ValueError over a t2v one."""
        latents = self.sample(noise, text_prompts, image_condition)
        with torch.no_grad():
            video = decode_video(self.vae, latents.to(torch.bfloat16))    # (float32 chain: the decoder reads the bf16 rounding)
        if return_latents:
            return video, latents.to(torch.float32 if self.latent_dtype == torch.float32 else noise.dtype)
        return video

    def sample(self, noise: torch.Tensor, text_prompts: List[str],
               image_condition: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """The denoise loop of `inference` without the decode: noise [1, F, 16, h, w] -> latents [1, F, 16, h, w] in `latent_dtype`."""
        if image_condition is not None and not self.i2v:
            raise ValueError("BidirectionalDiffusionInferencePipeline: image_condition needs a model_type 'i2v' generator; this one is t2v")
        if self.i2v and (image_condition is None or image_condition.get("clip_fea") is None or image_condition.get("y") is None):
            raise ValueError("BidirectionalDiffusionInferencePipeline: a model_type 'i2v' generator needs image_condition = "
                             "{'clip_fea', 'y'} (i2v_condition.build_image_condition)")
        batch_size, num_frames, num_channels, height, width = noise.shape
        assert batch_size == 1, "batch size 1"
        assert (num_channels, height, width) == (16, self.geometry.lat_h, self.geometry.lat_w), tuple(noise.shape)
        dev = self.device
        with torch.no_grad():
            conditional_dict = self.text_encoder(text_prompts=text_prompts)
            unconditional_dict = self.text_encoder(text_prompts=[self.args.negative_prompt] * len(text_prompts))
            if self.crossattn_cache_pos is None:
                self.crossattn_cache_pos = self.generator.new_crossattn_cache()
                self.crossattn_cache_neg = self.generator.new_crossattn_cache()
            self.crossattn_cache_pos.fill(conditional_dict["prompt_embeds"])
            self.crossattn_cache_neg.fill(unconditional_dict["prompt_embeds"])

            st = self._step_state(noise)
            self.timesteps = st["timesteps"]
            st["latents"].copy_(noise[0].to(device=dev, dtype=self.latent_dtype))      # (float32: taken as it is, never rounded)
            if st["latents_bf16"] is not None:
                st["latents_bf16"].copy_(st["latents"])                   # step 1's shadow; the later ones come from the solver kernel
            if self.i2v:                                                  # in place: the step graph holds these addresses
                y = self.generator.frame_major_y(image_condition["y"])
                if y.shape[0] != num_frames:
                    raise ValueError(f"image_condition['y'] holds {y.shape[0]} latent frames, the noise {num_frames}")
                st["y"].copy_(y)
                self.generator.set_image(image_condition["clip_fea"])
            st["sched"].reset_step_table(st["t"])
            n = st["n"]
            self.computed_steps, self.skipped_steps = n, 0
            if "schedule" in st:
                self.computed_steps = sum(st["schedule"])
                self.skipped_steps = n - self.computed_steps
                for compute in st["schedule"]:
                    g = st["graphs"].get(compute)
                    if g is not None:
                        g.replay()
                    else:                                                 # first use of this step kind (without graphs: every use)
                        mode = CACHE_RECORD if compute else CACHE_REUSE
                        st["graphs"][compute] = eager_then_capture(self, lambda: self._step(st, mode))
            elif st["graph"] is not None:
                for _ in range(n):
                    st["graph"].replay()
            else:                                                         # first use: step 1 eagerly, then into the step's graph
                g = st["graph"] = eager_then_capture(self, lambda: self._step(st))
                for _ in range(n - 1):
                    if g is not None:
                        g.replay()
                    else:
                        self._step(st)

            return st["latents"].unsqueeze(0).clone()
