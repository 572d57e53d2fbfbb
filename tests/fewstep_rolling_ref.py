"""The rolling KV window of the few-step pipeline restated for the tests, without the product's formula: the cache as a list of
(slot, frame) entries from which the OLDEST frame that is not a sink frame is evicted -- stated once, in tests/pipeline_chain.py
(`RollingSim`, `schedule_slots`), and re-exported here -- and one denoised block on the oracle's DiT forward (oracle/wan_dit_ref.py)
with explicit RoPE frame ids, write slots and visible slots."""
from typing import List, Sequence

import torch

from fewstep_ref import ref_add_noise, ref_x0
from pipeline_chain import RollingSim, schedule_slots  # noqa: F401


def block(sd, ocfg, okv, ocross, x: torch.Tensor, ctx: torch.Tensor, frame_ids: Sequence[int], write_slots: Sequence[int],
          visible_slots: Sequence[int], step_ts: Sequence[float], sig_x0: Sequence[float], sig_next: Sequence[float],
          draws: List[torch.Tensor], context_noise: float, **dit_kw) -> torch.Tensor:
    """tests/fewstep_ref.block on explicit (frame_ids, write_slots, visible_slots): x [F, 16, h, w] -> the block's output latents;
    the oracle cache `okv` ends up refreshed at `write_slots`."""
    from oracle import wan_dit_ref as W
    F = x.shape[0]

    def fwd(inp, tv):
        t = torch.full([1, F], float(tv), dtype=torch.float32, device=inp.device)
        return W.dit_forward(sd, ocfg, inp.permute(1, 0, 2, 3), t, ctx, okv, ocross, list(frame_ids), list(write_slots),
                             list(visible_slots), **dit_kw).permute(1, 0, 2, 3).contiguous()

    n = len(step_ts)
    for i in range(n):
        x0 = ref_x0(fwd(x, step_ts[i]), x, sig_x0[i])
        if i < n - 1:
            x = ref_add_noise(x0, draws[i], sig_next[i])
    fwd(x0, context_noise)
    return x0
