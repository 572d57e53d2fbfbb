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

from ..wan_wrapper import WanDiffusionWrapper, WanTextEncoder, WanVAEWrapper


class BidirectionalInferencePipeline(torch.nn.Module):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None):
        super().__init__()
        self.device = torch.device(device)
        self.generator = WanDiffusionWrapper(**getattr(args, "model_kwargs", {}), is_causal=False,
                                             device=device) if generator is None else generator
        if getattr(self.generator, "is_causal", False):
            raise ValueError("BidirectionalInferencePipeline needs WanDiffusionWrapper(is_causal=False)")
        if getattr(self.generator, "model_type", "t2v") != "t2v":
            raise ValueError("BidirectionalInferencePipeline is text-to-video only (no few-step i2v checkpoint exists); sample a "
                             "model_type 'i2v' generator with BidirectionalDiffusionInferencePipeline(image_condition=...)")
        self.geometry = self.generator.geometry
        self.text_encoder = WanTextEncoder(device=device) if text_encoder is None else text_encoder
        self.vae = WanVAEWrapper(geometry=self.geometry, device=device) if vae is None else vae

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
        self.crossattn_cache = None

    def to(self, *args, **kwargs):
        return self

    def release_graphs(self) -> None:
        """Drop the captured graphs (and the static buffers they read)."""
        torch.cuda.synchronize(self.device)
        self._calls.clear()

    def _step_scalars(self):
        """(engine timestep, sigma of the x0 conversion, sigma of add_noise to the NEXT listed step) per forward, from the step
        list's own dtype the way the reference's tensors carry it (float32 when warped, int64 otherwise)."""
        steps = list(self.denoising_step_list)
        t_eng = [float(t) for t in steps[:-1]]
        sig_x0 = [self.generator.sigma_x0(t) for t in steps[:-1]]
        sig_next = [self.generator.sigma_add_noise(t) for t in steps[1:]]
        return t_eng, sig_x0, sig_next

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
            pe = conditional_dict["prompt_embeds"]
            self.crossattn_cache.fill(pe[0] if pe.dim() == 3 else pe)

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
            draws = iter(self.renoise_override) if self.renoise_override is not None else None
            for i in range(n_fwd):                                        # the reference's torch.randn_like draws, in order
                if draws is not None:
                    st["bank"][i].copy_(next(draws).reshape(st["bank"][i].shape))
                else:
                    st["bank"][i].normal_(0.0, 1.0, generator=self.noise_generator)
            if st["graph"] is not None:
                st["graph"].replay()
            else:
                self._run(st, scalars)                                    # first use: the real work, eagerly ...
                if self.use_graphs:                                       # ... then the same launches into the call's graph
                    torch.cuda.synchronize(dev)
                    g = torch.cuda.CUDAGraph()
                    self.graph_captures += 1
                    with torch.cuda.graph(g):
                        self._run(st, scalars)
                    st["graph"] = g

            latents = st["x0"].unsqueeze(0).clone()
            video = self.vae.decode_to_pixel(latents)
            video = (video * 0.5 + 0.5).clamp(0, 1)
        if return_latents:
            return video, latents.to(noise.dtype)
        return video
