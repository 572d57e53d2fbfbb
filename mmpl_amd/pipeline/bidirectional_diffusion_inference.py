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
                      concurrent=bool(concurrent), share=engine.shared_block0_buffer(F) if share else None, ws2=None)
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
        if st["concurrent"]:
            main, side = torch.cuda.current_stream(self.device), self._side_stream
            side.wait_stream(main)                                        # fork
            gen.flow_full(x, t, pos, out=flow[0])
            with torch.cuda.stream(side):
                gen.flow_full(x, t, neg, out=flow[1], workspace=st["ws2"])
            main.wait_stream(side)                                        # join: the CFG / solver update needs both
        else:
            gen.flow_full(x, t, pos, out=flow[0], share_out=st["share"])
            gen.flow_full(x, t, neg, out=flow[1], share_in=st["share"])
        # flow = uncond + g (cond - uncond); latents = scheduler.step(flow): one fused kernel, scalars and next t from device tables
        st["sched"].step_cfg_table(flow[0], flow[1], x, t)

    def inference(self, noise: torch.Tensor, text_prompts: List[str], return_latents=False) -> torch.Tensor:
        """noise [1, F, 16, h, w] (F up to 24).  Returns video [1, T, 3, 8h, 8w] in [0, 1] (and the latents [1, F, 16, h, w])."""
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
