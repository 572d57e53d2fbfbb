"""The rolling KV window of the few-step pipeline restated for the tests, without the product's formula: the cache as a list of
(slot, frame) entries from which the OLDEST frame that is not a sink frame is evicted, and one denoised block on the oracle's DiT
forward (oracle/wan_dit_ref.py) with explicit RoPE frame ids, write slots and visible slots."""
from typing import List, Sequence, Tuple

import torch

from fewstep_ref import ref_add_noise, ref_x0


class RollingSim:
    """window slots; the first `sink` FRAMES of the video are never evicted.  `put(frame)` returns the slot the frame goes to: a
    free slot while there is one (lowest first), else the slot of the oldest resident frame >= sink."""

    def __init__(self, window: int, sink: int):
        self.window, self.sink = window, sink
        self.entries: List[Tuple[int, int]] = []                     # (slot, frame), oldest first

    def put(self, frame: int) -> int:
        if len(self.entries) < self.window:
            used = {s for s, _ in self.entries}
            slot = min(s for s in range(self.window) if s not in used)
        else:
            victim = next(i for i, (_, f) in enumerate(self.entries) if f >= self.sink)
            slot, _ = self.entries.pop(victim)
        self.entries.append((slot, frame))
        return slot

    def block(self, start: int, n: int):
        """Write frames start .. start+n-1; -> (write_slots, visible slots in slot order, resident frames sorted)."""
        write = [self.put(f) for f in range(start, start + n)]
        return write, sorted(s for s, _ in self.entries), sorted(f for _, f in self.entries)


def schedule_slots(window: int, sink: int, schedule: Sequence[int]):
    """[(start, n, write_slots, visible_slots, visible_frames)] of a block schedule run through the simulation."""
    sim, out, start = RollingSim(window, sink), [], 0
    for n in schedule:
        out.append((start, n) + sim.block(start, n))
        start += n
    return out


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
