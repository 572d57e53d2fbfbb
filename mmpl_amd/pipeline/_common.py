"""What the four pipelines say the same way, said once: the constructor prologue, "eager first, then capture", the solver factory of
the two CFG samplers and one CFG step's launches, the step scalars and the re-noise bank of the two few-step pipelines, and the
decode tail.  Nothing here decides a launch: each helper issues exactly what its callers used to spell out."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from ..scheduler import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas,
                         retrieve_timesteps)
from ..stage_plan import concurrent_cfg_pays
from ..wan_wrapper import WanDiffusionWrapper, WanTextEncoder, WanVAEWrapper


class PipelineBase(torch.nn.Module):
    """What every pipeline's constructor repeats.  No GPU is touched here."""

    def _set_codecs(self, text_encoder, vae, device) -> None:
        """The default text encoder and VAE (``self.geometry`` is set) where none is handed in."""
        self.text_encoder = WanTextEncoder(device=device) if text_encoder is None else text_encoder
        self.vae = WanVAEWrapper(geometry=self.geometry, device=device) if vae is None else vae

    def to(self, *args, **kwargs):
        return self


class GeneratorPipeline(PipelineBase):
    """The three pipelines over a ``WanDiffusionWrapper``, which keep their graphs for their lifetime."""

    _stores: tuple = ()               # the dicts of captured graphs and of the static buffers they read: release_graphs() clears them

    def _set_generator(self, args, device, generator, is_causal: bool) -> None:
        self.device = torch.device(device)
        self.generator = WanDiffusionWrapper(**getattr(args, "model_kwargs", {}), is_causal=is_causal,
                                             device=device) if generator is None else generator
        self.geometry = self.generator.geometry

    def release_graphs(self) -> None:
        """Drop every captured graph (and the static buffers they read)."""
        torch.cuda.synchronize(self.device)                           # a side stream's work included
        for store in self._stores:
            store.clear()


def eager_then_capture(pipe, run: Callable[[], None]) -> Optional["torch.cuda.CUDAGraph"]:
    """First use of a launch sequence: ``run()`` eagerly -- the real work -- and then, with ``pipe.use_graphs``, the same launches
    into a hipGraph (counted in ``pipe.graph_captures``), which is returned for the later uses to replay.  None without graphs."""
    run()
    if not pipe.use_graphs:
        return None
    torch.cuda.synchronize(pipe.device)
    g = torch.cuda.CUDAGraph()                                        # (looked up here, at call time: tests count constructions)
    pipe.graph_captures += 1
    with torch.cuda.graph(g):
        run()
    return g


def decode_video(vae, latents: torch.Tensor, **kw) -> torch.Tensor:
    """latents [1, F, 16, h, w] -> video [1, T, 3, 8h, 8w] in [0, 1]."""
    return (vae.decode_to_pixel(latents, **kw) * 0.5 + 0.5).clamp(0, 1)


# ------------------------------------------------------------------------------------------------ the two CFG samplers
def make_sample_scheduler(solver: str, num_train_timesteps: int, sampling_steps: int, shift: float, device):
    """(scheduler, timesteps) of casual_fps_inference.py:503-524 / bidirectional_diffusion_inference.py:89-110.  Both classes
    offer the same device-facing interface (mmpl_amd/scheduler.py)."""
    if solver == "unipc":
        s = FlowUniPCMultistepScheduler(num_train_timesteps=num_train_timesteps, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(sampling_steps, device=device, shift=shift)
        return s, s.timesteps
    if solver == "dpm++":
        s = FlowDPMSolverMultistepScheduler(num_train_timesteps=num_train_timesteps, shift=1, use_dynamic_shifting=False)
        return s, retrieve_timesteps(s, device=device, sigmas=get_sampling_sigmas(sampling_steps, shift))[0]
    raise NotImplementedError("Unsupported solver.")


def cfg_concurrent(pipe, engine, n_frames: int) -> bool:
    """Whether the cond and the uncond forward of a step run as two parallel branches: ``pipe.concurrent_cfg``, or, with None,
    where it pays (mmpl_amd.stage_plan.concurrent_cfg_pays: small stages / small models)."""
    c = pipe.concurrent_cfg
    return bool(concurrent_cfg_pays(n_frames * engine.S, engine.dim) if c is None else c)


def cfg_step_buffers(pipe, engine, n_frames: int, concurrent: bool, second_workspace: Callable[[int], torch.Tensor], device):
    """(share, ws2) for ``cfg_step``: block 0's hand-over buffer where the branches run back to back with ``pipe.share_block0``,
    the uncond branch's private workspace (and ``pipe._side_stream``) where they run concurrently.  Allocates: outside any capture."""
    share = engine.shared_block0_buffer(n_frames) if (pipe.share_block0 and not concurrent) else None
    ws2 = None
    if concurrent:
        ws2 = second_workspace(n_frames)
        if pipe._side_stream is None:
            pipe._side_stream = torch.cuda.Stream(device=device)
    return share, ws2


def cfg_step(forward: Callable[..., object], sched, flow: torch.Tensor, latents: torch.Tensor, t: torch.Tensor, device,
             side: Optional["torch.cuda.Stream"], share: Optional[torch.Tensor], ws2: Optional[torch.Tensor],
             latents_bf16: Optional[torch.Tensor] = None) -> None:
    """One denoise step's launches, eager or under capture: ``forward(0, flow[0], ...)`` (cond) and ``forward(1, flow[1], ...)``
    (uncond) -- fork / join on ``side`` with the private workspace ``ws2``, or (``side`` None) back to back, the uncond one taking
    block 0's self-attention from the cond one through ``share`` -- then flow = uncond + g (cond - uncond) and
    latents = scheduler.step(flow) as one fused kernel whose scalars and next timestep come from device tables.  ``latents_bf16``:
    the float32 chain's bf16 shadow of ``latents`` (what ``forward`` reads), rewritten by the same kernel."""
    if side is not None:
        main = torch.cuda.current_stream(device)
        side.wait_stream(main)                                        # fork
        forward(0, flow[0])
        with torch.cuda.stream(side):
            forward(1, flow[1], workspace=ws2)
        main.wait_stream(side)                                        # join: the CFG / solver update needs both
    else:
        forward(0, flow[0], share_out=share)
        forward(1, flow[1], share_in=share)
    if latents_bf16 is None:
        sched.step_cfg_table(flow[0], flow[1], latents, t)
    else:
        sched.step_cfg_table(flow[0], flow[1], latents, t, sample_bf16=latents_bf16)


# ------------------------------------------------------------------------------------------------ the two few-step pipelines
def fewstep_scalars(generator, step_list, n_forwards: int):
    """(engine timestep, sigma of the x0 conversion) of the first ``n_forwards`` listed steps and the sigma of add_noise to each
    step after the first, from the step list's own dtype the way the reference's tensors carry it (float32 when warped, int64
    otherwise)."""
    steps = list(step_list)
    return ([float(t) for t in steps[:n_forwards]], [generator.sigma_x0(t) for t in steps[:n_forwards]],
            [generator.sigma_add_noise(t) for t in steps[1:]])


def fill_bank(bank: torch.Tensor, n: int, draws, generator: Optional[torch.Generator]) -> None:
    """The reference's ``torch.randn_like`` draws, in order, into ``bank[:n]``: the next ``n`` items of ``draws`` (the iterator over
    a pipeline's ``renoise_override``), or with None drawn from ``generator`` (None = the device's default one)."""
    for i in range(n):
        if draws is not None:
            bank[i].copy_(next(draws).reshape(bank[i].shape))
        else:
            bank[i].normal_(0.0, 1.0, generator=generator)
