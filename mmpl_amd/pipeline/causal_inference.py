"""``CausalInferencePipeline`` -- drop-in for MMPL_t2v/pipeline/causal_inference.py: few-step, block-causal inference
(Self-Forcing / CausVid checkpoints, configs/self_forcing_{dmd,sid}.yaml) with the denoising loop on the HIP engines.

Same constructor / ``inference()`` signature and attributes (``generator``, ``text_encoder``, ``vae``, ``scheduler``,
``denoising_step_list``, ``num_frame_per_block``, ``independent_first_frame``, ``local_attn_size``, ``kv_cache1``,
``crossattn_cache``) and the same semantics: warped step list, ``[1] + [3] * k`` block schedule, both ``initial_latent``
branches, ``context_noise`` refresh forward, caches reset per call, ``decode_to_pixel`` then ``(x * 0.5 + 0.5).clamp(0, 1)``.
What changed underneath:
  * a block = ``n`` DiT forwards (``mmpl_dit_forward`` on explicit KV slots) + ``n - 1`` fused x0 / re-noise updates
    (``mmpl_fewstep_update``) + the final x0 write into the output latent + the refresh forward, and with ``use_graphs`` all of
    it is ONE hipGraph per block, captured on first use and replayed by every later ``inference()`` call
    (``release_graphs()`` drops them);
  * the re-noise draws (``torch.randn_like`` per non-final step) are drawn before the block, in the reference's order and shape,
    into a static bank the graph reads: the same device generator state gives the reference's draws bit for bit;
  * the literals 30 / 12 / 1560 / 32760 come from the model config and the ``Geometry``;
  * ``inference_stream()`` (no counterpart in the reference) runs the same loop and hands the video out block by block: each
    block is decoded by the VAE's cached decode (``decode_to_pixel(use_cache=True)``'s engine) while the next one denoises --
    or, with ``decoder="preview"``, by the tiny TAEHV decoder handed in as ``preview_vae`` (``TAEHVWrapper``);
  * ``args.rolling_kv`` (no counterpart that runs in the reference, whose ``sink_size`` knob has nothing behind it): the KV cache
    becomes a rolling window -- ``generator.model.sink_size`` sink frames kept, the oldest other frame evicted
    (``wan_wrapper.rolling_slots``) -- so a call may generate more frames than the window holds.  Blocks past the window run on
    frame ids relative to a device scalar (``DitEngine.forward(frame_base=...)``) and write their x0 into a static buffer that is
    then copied into the output latent, so their graphs depend on the slot pattern only, not on the position in time: the
    number of hipGraphs is bounded whatever the video length.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ._common import GeneratorPipeline, decode_video, eager_then_capture, fewstep_scalars, fill_bank


class CausalInferencePipeline(GeneratorPipeline):
    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, preview_vae=None):
        super().__init__()
        self._set_generator(args, device, generator, is_causal=True)
        self._set_codecs(text_encoder, vae, device)
        self.preview_vae = preview_vae    # optional TAEHVWrapper: inference_stream(decoder="preview")

        self.scheduler = self.generator.get_scheduler()
        self.denoising_step_list = torch.tensor(args.denoising_step_list, dtype=torch.long)
        if getattr(args, "warp_denoising_step", False):                  # causal_inference.py:29-31
            timesteps = torch.cat((self.scheduler.timesteps.cpu(), torch.tensor([0], dtype=torch.float32)))
            self.denoising_step_list = timesteps[len(self.scheduler.timesteps) - self.denoising_step_list]

        self.num_transformer_blocks = self.generator.engine.L
        self.frame_seq_length = self.geometry.frame_seqlen

        self.kv_cache1 = None
        self.crossattn_cache = None
        self.args = args
        self.num_frame_per_block = getattr(args, "num_frame_per_block", 1)
        self.independent_first_frame = getattr(args, "independent_first_frame", False)
        self.local_attn_size = self.generator.model.local_attn_size
        self.rolling_kv = bool(getattr(args, "rolling_kv", False))       # rolling KV window with generator.model.sink_size sink frames
        if self.num_frame_per_block > self.generator.engine.max_frames:
            raise ValueError(f"num_frame_per_block {self.num_frame_per_block} > the engine's largest forward "
                             f"({self.generator.engine.max_frames} frames)")
        print(f"KV inference with {self.num_frame_per_block} frames per block")
        if self.num_frame_per_block > 1:
            self.generator.model.num_frame_per_block = self.num_frame_per_block

        self.use_graphs = True            # one hipGraph per block (n forwards + updates + refresh), kept for the pipeline's lifetime
        self.renoise_override: Optional[List[torch.Tensor]] = None   # tests: the re-noise draws in order, each [F, 16, h, w]
        self.noise_generator: Optional[torch.Generator] = None       # None = the device's default generator (torch.randn_like)
        self.graph_captures = 0           # hipGraphs constructed so far (tests: none after the first call)
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._bufs: Dict[object, dict] = {}  # static per-block buffers, by frames per block (a batch: by (frames per block, B))
        self._out: Dict[object, torch.Tensor] = {}                  # static output latents, by frame count (a batch: (frame count, B))
        self._caches: Dict[int, tuple] = {}                         # (kv_cache1, crossattn_cache) by batch: the graphs hold their addresses
        self._roll_bufs: Dict[tuple, torch.Tensor] = {}             # rolling blocks past the window: static x0, by graph key
        self._frame_base: Optional[torch.Tensor] = None             # ... and the int32 device scalar their RoPE positions start from
        self._stores = (self._graphs, self._bufs, self._out, self._roll_bufs)     # (not _caches: kv_cache1 outlives the graphs, as ever)
        self._side: Optional[torch.cuda.Stream] = None              # inference_stream: the decode stream
        self._stage: Optional[torch.Tensor] = None                  # inference_stream: pinned uint8 staging, [2, frames, H, W, 3]

    def release_graphs(self) -> None:
        """Drop every captured block graph (and the static buffers they read)."""
        super().release_graphs()                                      # synchronises: the decode stream of inference_stream included
        self._frame_base = None

    # ------------------------------------------------------------------------------------------------------------
    def block_schedule(self, num_frames: int, initial_latent: Optional[torch.Tensor] = None) -> List[int]:
        """Frames per denoised block (causal_inference.py:68-79, 161-163), with the reference's assertions."""
        F = self.num_frame_per_block
        if not self.independent_first_frame or (self.independent_first_frame and initial_latent is not None):
            assert num_frames % F == 0
            num_blocks = num_frames // F
        else:
            assert (num_frames - 1) % F == 0
            num_blocks = (num_frames - 1) // F
        sched = [F] * num_blocks
        if self.independent_first_frame and initial_latent is None:
            sched = [1] + sched
        return sched

    def _step_scalars(self):
        """(engine timestep, sigma of the x0 conversion, sigma of the next step's add_noise) per step: a forward at every one."""
        return fewstep_scalars(self.generator, self.denoising_step_list, len(self.denoising_step_list))

    def _block_buffers(self, F: int, B: int = 1) -> dict:
        """x / flow [B*F, 16, h, w] and t [B*F], sample-major; the bank [n - 1, B, F, 16, h, w] (one draw of the reference's
        [B, F, 16, h, w] per step: bank[i] viewed [B*F, ...] is the step's noise in x's layout)."""
        key = F if B == 1 else (F, B)
        b = self._bufs.get(key)
        if b is None:
            g, dev = self.geometry, self.device
            n = len(self.denoising_step_list)
            frame = (16, g.lat_h, g.lat_w)
            shape = (B * F,) + frame
            b = dict(x=torch.empty(shape, dtype=torch.bfloat16, device=dev), flow=torch.empty(shape, dtype=torch.bfloat16, device=dev),
                     t=torch.empty(B * F, dtype=torch.float32, device=dev),
                     bank=torch.empty((max(n - 1, 1),) + ((F,) if B == 1 else (B, F)) + frame, dtype=torch.bfloat16, device=dev))
            self._bufs[key] = b
        return b

    def _output(self, T: int, B: int = 1) -> torch.Tensor:
        key = T if B == 1 else (T, B)
        o = self._out.get(key)
        if o is None:
            g = self.geometry
            o = self._out[key] = torch.zeros(B, T, 16, g.lat_h, g.lat_w, dtype=torch.bfloat16, device=self.device)
        return o

    def _run_block(self, b: dict, out_blk: torch.Tensor, start: int, write, vis, scalars, frame_base=None) -> None:
        """One block's launches (causal_inference.py:165-211): eager, or recorded into the block's hipGraph.  ``frame_base``: the
        device scalar `start` is relative to (a rolling block past the window: `start` is 0 and `out_blk` a static buffer)."""
        t_eng, sig_x0, sig_next = scalars
        gen, kv, cross = self.generator, self.kv_cache1, self.crossattn_cache
        n = len(t_eng)
        for i in range(n):
            b["t"].fill_(t_eng[i])
            gen.flow(b["x"], b["t"], start, write, vis, kv, cross, out=b["flow"], frame_base=frame_base)
            if i < n - 1:                           # x0, then add_noise(x0, randn, next t) back into the block's input
                gen.fewstep_update(b["flow"], b["x"], b["bank"][i], out_blk, sig_x0[i], sig_next[i])
            else:                                   # output[:, block] = denoised_pred
                gen.fewstep_update(b["flow"], b["x"], None, out_blk, sig_x0[i])
        b["t"].fill_(float(getattr(self.args, "context_noise", 0)))    # refresh the cache with the clean block (:199-207)
        gen.flow(out_blk, b["t"], start, write, vis, kv, cross, out=b["flow"], frame_base=frame_base)

    def _context_forward(self, lat: torch.Tensor, start: int) -> None:
        """A clean-latent forward at t = 0 that only fills the cache (initial_latent, causal_inference.py:130-159); lat [B, F, ...]."""
        B, F = lat.shape[:2]
        x = lat.to(device=self.device, dtype=torch.bfloat16).reshape((B * F,) + tuple(lat.shape[2:])).contiguous()
        write, vis, le = self.generator.slots(self.kv_cache1, start, F, rolling=self.rolling_kv, **({"batch": B} if B > 1 else {}))
        t = torch.zeros(x.shape[0], dtype=torch.float32, device=self.device)
        self.generator.flow(x, t, start, write, vis, self.kv_cache1, self.crossattn_cache)
        self.generator.set_cache_ends(self.kv_cache1, start + F, le)

    def _blocks(self, noise: torch.Tensor, text_prompts: List[str], initial_latent: Optional[torch.Tensor] = None):
        """The denoising loop ``inference()`` and ``inference_stream()`` share (causal_inference.py:82-211), as a generator over
        its hand-over points: yields ``(start_frame, n_frames, output)`` once after the ``initial_latent`` frames are in the
        static output latent and the cache (``n_frames`` = 0 without one), then after every block's launches -- the block's
        frames ``output[0, start:start + n_frames]`` are complete in stream order on the current stream.  The caller holds
        ``torch.no_grad()`` around every resumption."""
        batch_size, num_frames, num_channels, height, width = noise.shape
        B = batch_size
        if len(text_prompts) != B:
            raise ValueError(f"{len(text_prompts)} prompts for a noise batch of {B}")
        if initial_latent is not None and initial_latent.shape[0] != B:
            raise ValueError(f"initial_latent holds {initial_latent.shape[0]} samples, the noise {B}")
        max_frames = self.generator.engine.max_frames
        if B * self.num_frame_per_block > max_frames:                     # the batch runs as ONE forward over B * F frames
            raise ValueError(f"batch {B} x num_frame_per_block {self.num_frame_per_block} = {B * self.num_frame_per_block} frames "
                             f"per forward exceeds the engine's limit of {max_frames} (max_frames): at most "
                             f"{max_frames // self.num_frame_per_block} samples per call")
        assert (num_channels, height, width) == (16, self.geometry.lat_h, self.geometry.lat_w), tuple(noise.shape)
        schedule = self.block_schedule(num_frames, initial_latent)
        num_input_frames = initial_latent.shape[1] if initial_latent is not None else 0
        num_output_frames = num_frames + num_input_frames
        dev = self.device
        W = self.generator.window_frames
        if self.rolling_kv:
            from ..wan_wrapper import ROPE_POSITIONS, rolling_slots
            if num_output_frames > ROPE_POSITIONS:                        # the last block would fail: say so before anything runs
                raise ValueError(f"rolling KV window: {num_output_frames} frames end past the RoPE tables' last position "
                                 f"({ROPE_POSITIONS - 1})")
            for F in set(schedule) | ({self.num_frame_per_block} if num_input_frames else set()):
                rolling_slots(0, F, W, int(self.generator.model.sink_size))   # sink_size / block size against the window
        conditional_dict = self.text_encoder(text_prompts=text_prompts)

        gen = self.generator
        if self.kv_cache1 is not None:                                    # (the current pair, a caller-installed one included)
            self._caches.setdefault(getattr(self.kv_cache1, "batch", 1), (self.kv_cache1, self.crossattn_cache))
        if B not in self._caches:
            self._caches[B] = (gen.new_kv_cache(), gen.new_crossattn_cache()) if B == 1 else (gen.new_kv_cache(batch=B), gen.new_crossattn_cache(B))
        else:                                                             # :113-123
            for blk in self._caches[B][1]:
                blk["is_init"] = False
            self.generator.set_cache_ends(self._caches[B][0], 0, 0)
        self.kv_cache1, self.crossattn_cache = self._caches[B]
        # one prompt for every sample: sample 0's text K / V serve all, and the text cross-attention stays one launch
        shared = B > 1 and all(p == text_prompts[0] for p in text_prompts)
        if B == 1:
            self.crossattn_cache.fill(conditional_dict["prompt_embeds"])
        else:
            self.crossattn_cache.fill(conditional_dict["prompt_embeds"], shared=shared)

        noise_bf = noise.to(device=dev, dtype=torch.bfloat16).contiguous()
        output = self._output(num_output_frames, B)
        output.zero_()
        current_start_frame = 0
        if initial_latent is not None:                                    # :126-159
            init = initial_latent.to(device=dev, dtype=torch.bfloat16)
            F = self.num_frame_per_block
            if self.independent_first_frame:
                assert (num_input_frames - 1) % F == 0
                num_input_blocks = (num_input_frames - 1) // F
                output[:, :1] = init[:, :1]
                self._context_forward(init[:, :1], current_start_frame)
                current_start_frame += 1
            else:
                assert num_input_frames % F == 0
                num_input_blocks = num_input_frames // F
            for _ in range(num_input_blocks):
                ref = init[:, current_start_frame:current_start_frame + F]
                output[:, current_start_frame:current_start_frame + F] = ref
                self._context_forward(ref, current_start_frame)
                current_start_frame += F
        yield 0, current_start_frame, output

        scalars = self._step_scalars()
        n = len(scalars[0])
        draws = iter(self.renoise_override) if self.renoise_override is not None else None
        for F in schedule:
            s = current_start_frame
            b = self._block_buffers(F, B)
            write, vis, le = self.generator.slots(self.kv_cache1, s, F, rolling=self.rolling_kv,      # (rolling: checks the RoPE range)
                                                  **({"batch": B} if B > 1 else {}))
            b["x"].view((B, F) + tuple(b["x"].shape[1:])).copy_(noise_bf[:, s - num_input_frames:s - num_input_frames + F])
            fill_bank(b["bank"], n - 1, draws, self.noise_generator)
            rolled = self.rolling_kv and s + F > W                        # a frame at or past the window: position-free launches
            # a batch's block is [B*F, ...] sample-major, which is no slice of output [B, T, ...]: like a rolled block it writes its x0
            # into a static buffer of its own that is then copied out; the graph keys of a batch carry B and whether the samples
            # share one context (B == 1: the keys, buffers and graphs this pipeline always had)
            batch_key = (B, shared) if B > 1 else ()
            vis_key = tuple(map(tuple, vis)) if B > 1 else tuple(vis)
            if not rolled:
                out_blk, rel, base = output[0, s:s + F], s, None
                key = (s, F, tuple(scalars[0]), float(getattr(self.args, "context_noise", 0)), num_output_frames, tuple(write),
                       vis_key) + batch_key
            else:
                # the slots say WHERE in the ring the block sits, and that repeats; WHEN it sits there is the device scalar, and
                # its x0 goes to a buffer of the pattern's own: neither the start frame nor an address of `output` is in the launches
                key = ("rolling", F, tuple(scalars[0]), float(getattr(self.args, "context_noise", 0)), tuple(write), vis_key) + batch_key
                if self._frame_base is None:
                    self._frame_base = torch.zeros((), dtype=torch.int32, device=dev)
                rel, base = 0, self._frame_base
                base.fill_(s)                                             # in stream order ahead of the launches that read it
            if rolled or B > 1:
                out_blk = self._roll_bufs.get(key)
                if out_blk is None:
                    out_blk = self._roll_bufs[key] = torch.empty_like(b["x"])
            g = self._graphs.get(key)
            if g is not None:
                g.replay()
            else:                                                         # first use: eagerly, then into the block's graph
                g = eager_then_capture(self, lambda: self._run_block(b, out_blk, rel, write, vis, scalars, base))
                if g is not None:
                    self._graphs[key] = g
            if rolled or B > 1:                                           # on the compute stream: complete before the yield's consumers
                output[:, s:s + F].copy_(out_blk.view((B, F) + tuple(out_blk.shape[1:])))
            self.generator.set_cache_ends(self.kv_cache1, s + F, le)
            current_start_frame += F
            yield s, F, output

    def inference(self, noise: torch.Tensor, text_prompts: List[str], initial_latent: Optional[torch.Tensor] = None,
                  return_latents: bool = False, profile: bool = False, low_memory: bool = False):
        """noise [B, F, 16, h, w]; one prompt per sample; initial_latent [B, n, 16, h, w] or None.  Returns video [B, T, 3, 8h, 8w] in
        [0, 1] (and the latents [B, n + F, 16, h, w]).  The samples of a batch are independent and run as ONE forward over
        B * num_frame_per_block frames per step (DitEngine.forward_groups), so B * num_frame_per_block <= the engine's max_frames;
        the re-noise draws are one [B, F, 16, h, w] per non-final step, the reference's.  low_memory is accepted and has no effect
        (everything stays resident)."""
        dev = self.device
        with torch.no_grad():
            if profile:
                ev = lambda: torch.cuda.Event(enable_timing=True)
                init_start, init_end, diffusion_start, diffusion_end, vae_start, vae_end = (ev() for _ in range(6))
                block_times = []
                init_start.record()

            blocks = self._blocks(noise, text_prompts, initial_latent)
            _, _, output = next(blocks)                                   # text encoder, caches, the initial_latent forwards

            if profile:
                init_end.record()
                torch.cuda.synchronize(dev)
                diffusion_start.record()
                block_start = ev()
                block_start.record()

            for _ in blocks:
                if profile:
                    block_end = ev()
                    block_end.record()
                    torch.cuda.synchronize(dev)
                    block_times.append(block_start.elapsed_time(block_end))
                    block_start = ev()
                    block_start.record()

            if profile:
                diffusion_end.record()
                torch.cuda.synchronize(dev)
                diffusion_time = diffusion_start.elapsed_time(diffusion_end)
                init_time = init_start.elapsed_time(init_end)
                vae_start.record()

            latents = output.clone().to(noise.dtype)
            video = torch.cat([decode_video(self.vae, output[g:g + 1].clone(), use_cache=False) for g in range(output.shape[0])])

            if profile:
                vae_end.record()
                torch.cuda.synchronize(dev)
                vae_time = vae_start.elapsed_time(vae_end)
                total_time = init_time + diffusion_time + vae_time
                print("Profiling results:")
                print(f"  - Initialization/caching time: {init_time:.2f} ms ({100 * init_time / total_time:.2f}%)")
                print(f"  - Diffusion generation time: {diffusion_time:.2f} ms ({100 * diffusion_time / total_time:.2f}%)")
                for i, bt in enumerate(block_times):
                    print(f"    - Block {i} generation time: {bt:.2f} ms ({100 * bt / diffusion_time:.2f}% of diffusion)")
                print(f"  - VAE decoding time: {vae_time:.2f} ms ({100 * vae_time / total_time:.2f}%)")
                print(f"  - Total time: {total_time:.2f} ms")
        if return_latents:
            return video, latents
        return video

    # ------------------------------------------------------------------------------------------------------------
    def _staging(self, n_frames: int) -> torch.Tensor:
        """Two pinned host buffers of n_frames uint8 frames each, used alternately by consecutive yields of inference_stream."""
        g = self.geometry
        st = self._stage
        if st is None or st.shape[1] < n_frames:
            st = self._stage = torch.empty(2, n_frames, 8 * g.lat_h, 8 * g.lat_w, 3, dtype=torch.uint8, pin_memory=True)
        return st

    def _decode_block(self, out_blk: torch.Tensor, fmt: str, compute, side, slot: int, max_frames: int, preview: bool = False):
        """Queue the streamed decode of one block's latent frames on ``side`` behind everything ``compute`` holds now; returns
        (frames, ready event).  uint8 frames land in pinned staging buffer ``slot``; float frames stay on the device.
        ``preview``: the tiny decoder, whose output is in [0, 1] already and is handed out as it is (clamped)."""
        if side is not compute:
            # Everything that writes out_blk is on `compute` before this event.  The launches that follow it there (block k+1, the
            # next call's setup excepted: the generator drains `side` before it ends) write OTHER frame slices of the static
            # output latent and never this one, so `side` may read it while `compute` runs on.
            done = torch.cuda.Event()
            done.record(compute)
            side.wait_event(done)
        with torch.cuda.stream(side):
            if preview:
                px = self.preview_vae.decode_stream(out_blk, out_format=fmt)
            else:
                px = self.vae.model.decode_stream(out_blk, self.vae.mean, self.vae.std, out_format=fmt)
            if fmt == "uint8":
                frames = self._staging(max_frames)[slot, :px.shape[0]]
                frames.copy_(px, non_blocking=True)
            else:
                # the Wan VAE: what inference() does to the decoded video; the preview decoder's [0, 1] output needs the clamp only
                frames = px.clamp(0, 1) if preview else (px * 0.5 + 0.5).clamp(0, 1)
                frames.record_stream(compute)                             # the consumer uses it there
            ready = torch.cuda.Event()
            ready.record(side)
        return frames, ready

    def inference_stream(self, noise: torch.Tensor, text_prompts: List[str], initial_latent: Optional[torch.Tensor] = None,
                         output: str = "uint8", overlap: bool = True, decoder: str = "vae"):
        """``inference()`` handing the video out block by block: a generator of ``(first_pixel_frame_index, frames)``, once for
        the ``initial_latent`` frames (if any) and once per denoised block, as soon as that block's pixels exist.

        ``output="uint8"``: frames are host uint8 [T, 8h, 8w, 3] (the video writer's layout, the caller's to keep);
        ``"float"``: device float32 [T, 3, 8h, 8w] in [0, 1].  Concatenated they are ``inference()``'s video bit for bit (for
        uint8: its ``(video * 255.0).clamp(0, 255).to(torch.uint8)`` conversion).  Same block graphs, buffers, re-noise bank and
        cache bookkeeping as ``inference()``; each block is decoded by the VAE's cached decode (``VaeEngine.decode_stream``),
        eagerly.  ``overlap=True`` decodes block k on a second stream while the first one denoises block k + 1 and yields block
        k once block k + 1 is queued; ``overlap=False`` runs the same work on the current stream, in order.  A call starts a
        new decoded video (``vae.model.clear_cache()``); the generator drains the decode stream when it finishes or is closed.

        ``decoder="preview"`` decodes the blocks with ``preview_vae`` (the tiny TAEHV decoder, ``TAEHVWrapper``) instead: same
        frame indices and counts, its own pixels -- the frames are that decoder's output clamped to [0, 1] (uint8: ``* 255``
        truncated), not ``inference()``'s video.  The latents are the same either way."""
        if output not in ("uint8", "float"):
            raise ValueError(f"output {output!r}: 'uint8' or 'float'")
        if decoder not in ("vae", "preview"):
            raise ValueError(f"decoder {decoder!r}: 'vae' or 'preview'")
        preview = decoder == "preview"
        if noise.shape[0] != 1:
            raise ValueError(f"inference_stream keeps batch size 1 (the noise holds {noise.shape[0]} samples): the block-wise decode "
                             "streams one video; batches run through inference()")
        if preview and self.preview_vae is None:
            raise ValueError("decoder='preview' needs a preview decoder: CausalInferencePipeline(..., preview_vae=TAEHVWrapper(...))")
        compute = torch.cuda.current_stream(self.device)
        if overlap and self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side if overlap else compute
        max_frames = 4 * max(self.num_frame_per_block, initial_latent.shape[1] if initial_latent is not None else 1)
        (self.preview_vae if preview else self.vae).model.clear_cache()

        def finish(first_px, frames, ready):
            ready.synchronize()                                           # this block's event only, never the device
            return first_px, (frames.clone() if output == "uint8" else frames)

        blocks = self._blocks(noise, text_prompts, initial_latent)
        pending, k = None, 0
        try:
            while True:
                with torch.no_grad():
                    step = next(blocks, None)                             # queues block k (or the initial frames) on `compute`
                    if step is None:
                        break
                    s, F, lat = step
                    if F == 0:                                            # no initial_latent
                        continue
                    cur = (0 if s == 0 else 1 + 4 * (s - 1),) + self._decode_block(lat[0, s:s + F], output, compute, side, k & 1,
                                                                                  max_frames, preview)
                    k += 1
                if not overlap:
                    yield finish(*cur)
                    continue
                if pending is not None:                                   # block k is queued behind it: hand out block k - 1
                    yield finish(*pending)
                pending = cur
            if pending is not None:
                yield finish(*pending)
        finally:
            blocks.close()
            side.synchronize()                                            # the static output latent is the next call's too
