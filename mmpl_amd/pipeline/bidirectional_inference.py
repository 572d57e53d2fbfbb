"""``BidirectionalInferencePipeline`` -- drop-in for MMPL_t2v/pipeline/bidirectional_inference.py: the few-step (DMD-distilled)
bidirectional generator, the whole clip per forward.

Same constructor / ``inference()`` signature and attributes (``generator``, ``text_encoder``, ``vae``, ``scheduler``,
``denoising_step_list``) and the same semantics, the loop's quirk included: a trailing 0 is dropped from the step list, the list is
warped through ``timesteps[1000 - list]``, and the generator runs at all but the LAST listed step -- after each forward the
predicted x0 is re-noised to the next listed step with a fresh ``torch.randn_like`` draw (the last draw is consumed although
nothing reads its result) and the last predicted x0 is decoded.  What changed underneath:
  * a forward is ``mmpl_dit_forward_full`` (no KV cache) and the x0 conversion + re-noise one fused kernel
    (``mmpl_fewstep_update``); with ``use_graphs`` the whole call's DiT work is ONE hipGraph, captured on first use per
    (frame count, step list) and replayed by every later ``inference()`` (``release_graphs()`` drops it);
  * the draws are made before the launches, in the reference's order and shape, into a static bank the graph reads
    (``renoise_override`` / ``noise_generator`` as in ``CausalInferencePipeline``).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ._common import GeneratorPipeline, decode_video, eager_then_capture, fewstep_scalars, fill_bank


class BidirectionalInferencePipeline(GeneratorPipeline):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None):
        super().__init__()
        self._set_generator(args, device, generator, is_causal=False)
        if getattr(self.generator, "is_causal", False):
            raise ValueError("BidirectionalInferencePipeline needs WanDiffusionWrapper(is_causal=False)")
        if getattr(self.generator, "model_type", "t2v") != "t2v":
            raise ValueError("BidirectionalInferencePipeline is text-to-video only (no few-step i2v checkpoint exists); sample a "
                             "model_type 'i2v' generator with BidirectionalDiffusionInferencePipeline(image_condition=...)")
        self._set_codecs(text_encoder, vae, device)

        self.scheduler = self.generator.get_scheduler()
        self.denoising_step_list = torch.tensor(args.denoising_step_list, dtype=torch.long)
        if self.denoising_step_list[-1] == 0:
            self.denoising_step_list = self.denoising_step_list[:-1]     # remove the zero timestep for inference (:27-28)
        if getattr(args, "warp_denoising_step", False):                   # :29-31
            timesteps = torch.cat((self.scheduler.timesteps.cpu(), torch.tensor([0], dtype=torch.float32)))
            self.denoising_step_list = timesteps[1000 - self.denoising_step_list]
        self.args = args

        self.use_graphs = True            # one hipGraph per call: every forward and every x0 / re-noise update
        self.renoise_override: Optional[List[torch.Tensor]] = None   # tests: the re-noise draws in order, each [F, 16, h, w]
        self.noise_generator: Optional[torch.Generator] = None       # None = the device's default generator (torch.randn_like)
        self.graph_captures = 0           # hipGraphs constructed so far (tests: none after the first call)
        self._calls: Dict[tuple, dict] = {}     # (frames, step list) -> static buffers and the graph
        self._stores = (self._calls,)
        self.crossattn_cache = None

    def _step_scalars(self):
        """(engine timestep, sigma of the x0 conversion, sigma of add_noise to the NEXT listed step) per forward: one at every
        listed step but the last."""
        return fewstep_scalars(self.generator, self.denoising_step_list, len(self.denoising_step_list) - 1)

    def _run(self, st: dict, scalars) -> None:
        """The call's launches (bidirectional_inference.py:52-67): eager, or recorded into the call's hipGraph."""
        t_eng, sig_x0, sig_next = scalars
        gen = self.generator
        for i in range(len(t_eng)):
            st["t"].fill_(t_eng[i])
            gen.flow_full(st["x"], st["t"], self.crossattn_cache, out=st["flow"])
            # pred = x0(flow, x, t_i); x = add_noise(pred, randn, t_{i+1}) -- after the last forward too, as the reference does
            gen.fewstep_update(st["flow"], st["x"], st["bank"][i], st["x0"], sig_x0[i], sig_next[i])

    def inference(self, noise: torch.Tensor, text_prompts: List[str], return_latents: bool = False) -> torch.Tensor:
        """noise [1, F, 16, h, w] (F up to 24).  Returns video [1, T, 3, 8h, 8w] in [0, 1] (``return_latents``, no counterpart in the
        reference: and the last predicted x0 [1, F, 16, h, w])."""
        batch_size, num_frames, num_channels, height, width = noise.shape
        assert batch_size == 1, "batch size 1"
        assert (num_channels, height, width) == (16, self.geometry.lat_h, self.geometry.lat_w), tuple(noise.shape)
        dev = self.device
        with torch.no_grad():
            conditional_dict = self.text_encoder(text_prompts=text_prompts)
            if self.crossattn_cache is None:
                self.crossattn_cache = self.generator.new_crossattn_cache()
            self.crossattn_cache.fill(conditional_dict["prompt_embeds"])

            scalars = self._step_scalars()
            n_fwd = len(scalars[0])
            if n_fwd < 1:
                raise ValueError("denoising_step_list needs at least two steps: the generator runs at all but the last one")
            key = (num_frames, tuple(scalars[0]), tuple(scalars[2]))
            st = self._calls.get(key)
            if st is None:
                shape = (num_frames, 16, height, width)
                mk = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev)
                st = self._calls[key] = dict(x=mk(*shape), flow=mk(*shape), x0=mk(*shape), bank=mk(n_fwd, *shape),
                                             t=torch.empty(1, dtype=torch.float32, device=dev), graph=None)
                self.generator.engine.full_workspace(num_frames)          # allocated outside the capture
            st["x"].copy_(noise[0].to(device=dev, dtype=torch.bfloat16))
            fill_bank(st["bank"], n_fwd, iter(self.renoise_override) if self.renoise_override is not None else None, self.noise_generator)
            if st["graph"] is not None:
                st["graph"].replay()
            else:                                                         # first use: eagerly, then into the call's graph
                st["graph"] = eager_then_capture(self, lambda: self._run(st, scalars))

            latents = st["x0"].unsqueeze(0).clone()
            video = decode_video(self.vae, latents)
        if return_latents:
            return video, latents.to(noise.dtype)
        return video
