"""Step caching (TeaCache) of the 50-step samplers: which denoise steps run the transformer blocks and which reuse the residual
the last computed step left (include/mmpl_hip.h: mmpl_dit_forward_*_cached).

The Wan indicator is the timestep embedding ``e`` (or its projection ``e0``), which depends on the timestep and the weights alone,
never on the latents: the whole schedule is known before sampling starts.  ``step_schedule`` computes it on the device (one
``DitEngine.time_embed`` over the sampler's timesteps, one ``rel_l1_rows``, one small read-back, outside any capture) and
``StepCachePolicy.schedule`` turns the distances into compute / skip on the host.

No fitted coefficients are shipped: the default polynomial is the identity, and a caller who has the TeaCache project's per-model
fit passes it in (highest power first, ``numpy.poly1d`` order).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

INDICATORS = ("e", "e0")


class StepCachePolicy:
    """``thresh``: the accumulated (rescaled) distance from which a step is computed again; 0 = compute every step.
    ``coefficients``: the rescaling polynomial P, highest power first; ``(1.0, 0.0)`` is the identity.
    ``ret_steps``: the first ``ret_steps`` steps are always computed (>= 1: the first step has nothing to reuse).
    ``cutoff``: steps ``i >= cutoff`` are always computed; None = n - 1, the last step.
    ``indicator``: ``"e"`` (the timestep embedding) or ``"e0"`` (its 6 * dim projection, what the blocks' modulation reads)."""

    def __init__(self, thresh: float, coefficients: Sequence[float] = (1.0, 0.0), ret_steps: int = 1, cutoff: Optional[int] = None,
                 indicator: str = "e"):
        if ret_steps < 1:
            raise ValueError(f"StepCachePolicy: ret_steps = {ret_steps}; the first step has no residual to reuse, so ret_steps >= 1")
        if indicator not in INDICATORS:
            raise ValueError(f"StepCachePolicy: indicator {indicator!r}; one of {INDICATORS}")
        if thresh < 0:
            raise ValueError(f"StepCachePolicy: thresh = {thresh} < 0")
        coefficients = tuple(float(c) for c in coefficients)
        if not coefficients:
            raise ValueError("StepCachePolicy: no coefficients")
        self.thresh = float(thresh)
        self.coefficients = coefficients
        self.ret_steps = int(ret_steps)
        self.cutoff = None if cutoff is None else int(cutoff)
        self.indicator = indicator

    def key(self) -> tuple:
        """What the schedule depends on besides the timesteps (pipelines key their cached schedule by it)."""
        return (self.thresh, self.coefficients, self.ret_steps, self.cutoff, self.indicator)

    def rescale(self, r: float) -> float:
        """P(r), Horner from the highest power."""
        acc = 0.0
        for c in self.coefficients:
            acc = acc * r + c
        return acc

    def schedule(self, rel: Sequence[float]) -> List[bool]:
        """rel[i] = distance between step i and step i - 1 (rel[0] is never read) -> per step, True = compute."""
        n = len(rel)
        cutoff = n - 1 if self.cutoff is None else self.cutoff
        out: List[bool] = []
        acc = 0.0
        for i in range(n):
            if i < self.ret_steps or i >= cutoff:
                compute = True
            else:
                acc += self.rescale(float(rel[i]))
                compute = not (acc < self.thresh)
            if compute:
                acc = 0.0
            out.append(compute)
        return out


def step_schedule(engine, policy: StepCachePolicy, timesteps) -> List[bool]:
    """The policy's schedule over `timesteps` (the sampler's table, in step order) on `engine`'s weights: True = compute.  Launches
    and reads back: call it outside any capture."""
    import torch

    t = torch.as_tensor(timesteps).detach().to(device=engine.device, dtype=torch.float32).reshape(-1).contiguous()
    n = t.numel()
    if n < 2:
        return policy.schedule([0.0] * n)
    e, e0 = engine.time_embed(t, want_e0=policy.indicator == "e0")
    rel = engine.rel_l1_rows(e0 if policy.indicator == "e0" else e)
    return policy.schedule([0.0] + [float(v) for v in rel.cpu()])
