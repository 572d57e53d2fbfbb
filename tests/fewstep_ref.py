"""The few-step block (pipeline/causal_inference.py:165-211) restated on the oracle's DiT forward (oracle/wan_dit_ref.py), for
the tests: PyTorch expressions of the reference's x0 conversion / add_noise, and one block of n forwards + refresh against a
KV cache in the causal layout (frame f in slot f, the window's frames visible)."""
from typing import List, Sequence

import torch


def ref_x0(flow: torch.Tensor, xt: torch.Tensor, sigma_t: float) -> torch.Tensor:
    """WanDiffusionWrapper._convert_flow_pred_to_x0 (utils/wan_wrapper.py:188-199) at one sigma."""
    return (xt.double() - torch.tensor(sigma_t, dtype=torch.float64, device=xt.device) * flow.double()).to(flow.dtype)


def ref_add_noise(x0: torch.Tensor, noise: torch.Tensor, sigma: float) -> torch.Tensor:
    """FlowMatchScheduler.add_noise (utils/scheduler.py:160-176) at one fp32 sigma ([N, 1, 1, 1] broadcast like the reference)."""
    s = torch.full([x0.shape[0], 1, 1, 1], sigma, dtype=torch.float32, device=x0.device)
    return ((1 - s) * x0 + s * noise).type_as(noise)


def block(sd, ocfg, okv, ocross, x: torch.Tensor, ctx: torch.Tensor, start: int, step_ts: Sequence[float], sig_x0: Sequence[float],
          sig_next: Sequence[float], draws: List[torch.Tensor], context_noise: float, window: int, **dit_kw) -> torch.Tensor:
    """One denoised block: x [F, 16, h, w] (pipeline layout) -> the block's output latents; the cache ends up refreshed."""
    from oracle import wan_dit_ref as W
    F = x.shape[0]
    frames = list(range(start, start + F))
    vis = list(range(max(0, start + F - window), start + F))

    def fwd(inp, tv):
        t = torch.full([1, F], float(tv), dtype=torch.float32, device=inp.device)
        return W.dit_forward(sd, ocfg, inp.permute(1, 0, 2, 3), t, ctx, okv, ocross, frames, frames, vis,
                             **dit_kw).permute(1, 0, 2, 3).contiguous()

    n = len(step_ts)
    for i in range(n):
        x0 = ref_x0(fwd(x, step_ts[i]), x, sig_x0[i])
        if i < n - 1:
            x = ref_add_noise(x0, draws[i], sig_next[i])
    fwd(x0, context_noise)
    return x0
