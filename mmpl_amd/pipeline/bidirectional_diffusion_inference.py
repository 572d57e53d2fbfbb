"""``BidirectionalDiffusionInferencePipeline`` -- drop-in for MMPL_t2v/pipeline/bidirectional_diffusion_inference.py: plain
Wan2.1 text-to-video sampling (upstream ``WanT2V.generate``): the whole clip is denoised at once, every frame attending to every
frame, by ``sampling_steps`` multistep-solver steps under classifier-free guidance.

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
  * the frame count is ``noise.shape[1]`` where the reference writes the literal 21; batch size 1.

Over a ``model_type='i2v'`` generator (the released Wan2.1-I2V-14B-480P / -720P weights) this is upstream ``WanI2V.generate``
(wan/image2video.py): ``inference(..., image_condition={"clip_fea": [257, 1280], "y": [20, F, h, w]})`` from
``i2v_condition.build_image_condition(vae, clip, image, n_latent_frames=F)``, the argument ``CausalFPSInferencePipeline.inference``
has.  The step state gains a static frame-major ``y`` buffer that every forward of the step graph reads next to the latents
(``mmpl_dit_forward_full_i2v``: no concatenation, no copy inside the graph); per call ``y`` is copied in and the generator's
image K / V are rebuilt in place, so another image replays the SAME graph.  Both CFG branches see the image (upstream's
``arg_null`` carries ``clip_fea`` and ``y`` too), so block 0 is still shared.  The latent chain stays this project's: bf16 latents
and the fused ``step_cfg_table``, like the text-to-video path; upstream ``WanI2V.generate`` keeps its latents in fp32.  ``shift``
and ``sampling_steps`` keep the defaults above -- ``WanI2V.generate``'s own (40 steps, shift 5.0, or 3.0 at 480p) are the caller's
to set, as ``mmpl_amd.cli`` does.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ..scheduler import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps)
from ..wan_wrapper import WanDiffusionWrapper, WanTextEncoder, WanVAEWrapper


class BidirectionalDiffusionInferencePipeline(torch.nn.Module):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None):
        super().__init__()
        self.device = torch.device(device)
        self.generator = WanDiffusionWrapper(**getattr(args, "model_kwargs", {}), is_causal=False,
                                             device=device) if generator is None else generator
        if getattr(self.generator, "is_causal", False):
            raise ValueError("BidirectionalDiffusionInferencePipeline needs WanDiffusionWrapper(is_causal=False)")
        self.i2v = getattr(self.generator, "model_type", "t2v") == "i2v"
        self.geometry = self.generator.geometry
        self.text_encoder = WanTextEncoder(device=device) if text_encoder is None else text_encoder
        self.vae = WanVAEWrapper(geometry=self.geometry, device=device) if vae is None else vae

        self.num_train_timesteps = args.num_train_timestep
        self.sampling_steps = 50
        self.sample_solver = 'unipc'
        self.shift = 8.0

        self.args = args

        self.use_graphs = True            # one hipGraph per denoise step (2 forwards + CFG / solver update)
        self.concurrent_cfg: Optional[bool] = None    # None = where concurrent_cfg_pays says so; True / False = always / never
        self.share_block0 = True          # sequential branches: the uncond forward takes block 0's self-attention from the cond one
        self.graph_captures = 0           # hipGraphs constructed so far (tests: none after the first call)
        self._steps: Dict[tuple, dict] = {}     # (frames, solver, steps, guidance, concurrent, share) -> static buffers, scheduler, graph
        self._side_stream = None
        self.crossattn_cache_pos = None
        self.crossattn_cache_neg = None

    def to(self, *args, **kwargs):
        return self

    def release_graphs(self) -> None:
        """Drop the captured step graphs (and the static buffers they read)."""
        torch.cuda.synchronize(self.device)
        self._steps.clear()

    # ------------------------------------------------------------------------------------------------------------
    def _initialize_sample_scheduler(self, noise):
        """bidirectional_diffusion_inference.py:89-110 on the device-facing schedulers (mmpl_amd/scheduler.py)."""
        if self.sample_solver == 'unipc':
            s = FlowUniPCMultistepScheduler(num_train_timesteps=self.num_train_timesteps, shift=1, use_dynamic_shifting=False)
            s.set_timesteps(self.sampling_steps, device=noise.device, shift=self.shift)
            self.timesteps = s.timesteps
        elif self.sample_solver == 'dpm++':
            s = FlowDPMSolverMultistepScheduler(num_train_timesteps=self.num_train_timesteps, shift=1, use_dynamic_shifting=False)
            self.timesteps, _ = retrieve_timesteps(s, device=noise.device, sigmas=get_sampling_sigmas(self.sampling_steps, self.shift))
        else:
            raise NotImplementedError("Unsupported solver.")
        return s

    def _step_state(self, noise: torch.Tensor) -> dict:
        """Static buffers, the scheduler with its device step table and (later) the graph of one step shape."""
        F = noise.shape[1]
        engine, dev = self.generator.engine, self.device
        concurrent = self.concurrent_cfg
        if concurrent is None:
            from ..stage_plan import concurrent_cfg_pays
            concurrent = concurrent_cfg_pays(F * engine.S, engine.dim)
        share = bool(self.share_block0 and not concurrent)
        key = (F, self.sample_solver, int(self.sampling_steps), float(self.args.guidance_scale), bool(concurrent), share)
        st = self._steps.get(key)
        if st is None:
            g = self.geometry
            shape = (F, 16, g.lat_h, g.lat_w)
            sched = self._initialize_sample_scheduler(noise)
            latents = torch.empty(shape, dtype=torch.bfloat16, device=dev)
            sched.build_step_table(self.args.guidance_scale, dev)
            sched._ensure_state(latents)
            st = dict(latents=latents, flow=torch.empty((2,) + shape, dtype=torch.bfloat16, device=dev),
                      t=torch.empty(1, dtype=torch.float32, device=dev), sched=sched, n=len(sched.timesteps), graph=None,
                      timesteps=self.timesteps,
                      concurrent=bool(concurrent), share=engine.shared_block0_buffer(F) if share else None, ws2=None,
                      # i2v: the conditioning video, frame-major, read by both forwards of every step and never written by them
                      y=torch.empty((F, engine.in_dim - 16, g.lat_h, g.lat_w), dtype=torch.bfloat16, device=dev) if self.i2v else None)
            engine.full_workspace(F)                                      # allocations and the stream: outside any capture
            if concurrent:
                st["ws2"] = engine.full_workspace(F, second=True)
                if self._side_stream is None:
                    self._side_stream = torch.cuda.Stream(device=dev)
            self._steps[key] = st
        return st

    def _step(self, st: dict) -> None:
        """One denoise step's launches (bidirectional_diffusion_inference.py:62-76): eager, or recorded into the step graph."""
        gen, pos, neg = self.generator, self.crossattn_cache_pos, self.crossattn_cache_neg
        x, t, flow = st["latents"], st["t"], st["flow"]
        kw = {} if st["y"] is None else {"y": st["y"]}                    # i2v: both branches see the image (image2video.py arg_null)
        if st["concurrent"]:
            main, side = torch.cuda.current_stream(self.device), self._side_stream
            side.wait_stream(main)                                        # fork
            gen.flow_full(x, t, pos, out=flow[0], **kw)
            with torch.cuda.stream(side):
                gen.flow_full(x, t, neg, out=flow[1], workspace=st["ws2"], **kw)
            main.wait_stream(side)                                        # join: the CFG / solver update needs both
        else:
            gen.flow_full(x, t, pos, out=flow[0], share_out=st["share"], **kw)
            gen.flow_full(x, t, neg, out=flow[1], share_in=st["share"], **kw)
        # flow = uncond + g (cond - uncond); latents = scheduler.step(flow): one fused kernel, scalars and next t from device tables
        st["sched"].step_cfg_table(flow[0], flow[1], x, t)

    def inference(self, noise: torch.Tensor, text_prompts: List[str], return_latents=False,
                  image_condition: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """noise [1, F, 16, h, w] (F up to 24).  Returns video [1, T, 3, 8h, 8w] in [0, 1] (and the latents [1, F, 16, h, w]).
        `image_condition`: {"clip_fea": [257, 1280], "y": [20, F, h, w]} (i2v_condition.build_image_condition) -- required over an
        i2v generator, a ValueError over a t2v one."""
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
            for cache, d in ((self.crossattn_cache_pos, conditional_dict), (self.crossattn_cache_neg, unconditional_dict)):
                pe = d["prompt_embeds"]
                cache.fill(pe[0] if pe.dim() == 3 else pe)

            st = self._step_state(noise)
            self.timesteps = st["timesteps"]
            st["latents"].copy_(noise[0].to(device=dev, dtype=torch.bfloat16))
            if self.i2v:                                                  # in place: the step graph holds these addresses
                y = self.generator.frame_major_y(image_condition["y"])
                if y.shape[0] != num_frames:
                    raise ValueError(f"image_condition['y'] holds {y.shape[0]} latent frames, the noise {num_frames}")
                st["y"].copy_(y)
                self.generator.set_image(image_condition["clip_fea"])
            st["sched"].reset_step_table(st["t"])
            n = st["n"]
            if st["graph"] is not None:
                for _ in range(n):
                    st["graph"].replay()
            else:
                self._step(st)                                            # first use: step 1 eagerly (the real work) ...
                if self.use_graphs:                                       # ... then the same launches into the step's graph
                    torch.cuda.synchronize(dev)
                    g = torch.cuda.CUDAGraph()
                    self.graph_captures += 1
                    with torch.cuda.graph(g):
                        self._step(st)
                    st["graph"] = g
                    for _ in range(n - 1):
                        g.replay()
                else:
                    for _ in range(n - 1):
                        self._step(st)

            latents = st["latents"].unsqueeze(0).clone()
            video = self.vae.decode_to_pixel(latents)
            video = (video * 0.5 + 0.5).clamp(0, 1)
        if return_latents:
            return video, latents.to(noise.dtype)
        return video
