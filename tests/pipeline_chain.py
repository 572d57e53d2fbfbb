"""The two few-step pipelines (mmpl_amd/pipeline/causal_inference.py, bidirectional_inference.py) as ORDERED LISTS OF ENTRY CALLS, written
from the reference's loop -- MMPL_t2v/pipeline/causal_inference.py:29-31 (warped step list), :68-79 (block schedule), :82-211 (the
loop), wan/modules/causal_model.py:196-226 (cache indexing), utils/wan_wrapper.py:172-199 (flow -> x0), utils/scheduler.py:160-176
(add_noise), pipeline/bidirectional_inference.py:27-31, 52-67 -- on the contracts of include/mmpl_hip.h, not from mmpl_amd/pipeline or
mmpl_amd/wan_wrapper (neither is imported here).  The loop has no rounding of its own: it decides which forward runs at which timestep on
which buffer, which sigma converts the flow and which re-noises, which draw a step reads, which KV slots a block writes and attends, and
when the refresh forward runs.  `FewstepChain.plan()` states those decisions as records on the host; `run()` executes them through a
small `ops` backend:

  HipOps     each record is exactly ONE ctypes call (mmpl_dit_precompute_context once per distinct context, mmpl_dit_forward_at for one
             sample, mmpl_dit_forward_groups for a batch, mmpl_dit_forward_full for the bidirectional chain, mmpl_fewstep_update), eager
             on the current stream, frame ids absolute, frame_base NULL.  Every buffer (x, flow, x0, t, one poisoned workspace per call,
             the caches) is an allocation of its own with a tail of the 0x7FA5 canary.
  OracleOps  oracle.wan_dit_ref.dit_forward on an oracle cache and tests/fewstep_ref.ref_x0 / ref_add_noise, on the CPU.

The rolling window has no counterpart that runs in the reference; its rule is stated here ONCE (`RollingSim`: evict the oldest frame
that is not a sink frame) and tests/fewstep_rolling_ref.py imports it.

tests/test_pipeline_chain_host.py holds the OracleOps chain to fixtures of the real reference (tests/golden/make_golden_fewstep_chain.py);
tests/test_pipeline_chain_gpu.py demands that the library's pipelines equal the HipOps chain in every bit.  The wiring decisions are the
entries of WIRING; a test hands in an altered copy to build a mutant of the chain.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from fewstep_ref import ref_add_noise, ref_x0
from forward_chain import CANARY, TAIL

BF = torch.bfloat16

# Launch-plan facts the model does not state.  The pipeline's text cross-attention attends over all text_len rows -- no prompt-dependent
# host value enters a launch, so one captured graph serves every prompt; any cross_rows outside [0, text_len - 2] means that.
CROSS_ROWS_ALL = -1

# The wiring of the loop.
WIRING = dict(
    sigma_next_step=lambda i: i + 1,          # after the forward at step i, x0 is re-noised to step i + 1 (causal_inference.py:205-211)
    draw_of_step=lambda i, n: i,              # step i of a block reads the block's i-th draw of n (torch.randn_like in call order)
    refresh=True,                             # the clean block is forwarded once more to rewrite its K / V (:226-235)
    refresh_t=lambda context_noise, step_ts: context_noise,     # ... at t = args.context_noise
    refresh_input="x0",                       # ... reading denoised_pred, not the last noisy input
    visible=lambda entries: entries,          # (slot, age) oldest first: everything in the window is attended (causal_model.py:220-224)
    ring_protect=lambda sink: sink,           # rolling: frames 0 .. sink - 1 are never evicted, so the ring starts at slot `sink`
    bank_rows=lambda d: d.reshape((-1,) + tuple(d.shape[2:])),          # a batch's draw [B, F, ...] is sample-major like x [B * F, ...]
    sample_offset=lambda g, n_slots: g * n_slots,                        # sample g owns slots g * n_slots ..
    initial_forward=True,                     # initial_latent frames are forwarded at t = 0 to fill the cache (:136-169)
)


# ====================================================================================================== scalars
def flow_match_tables(shift: float, n_train: int = 1000) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigmas, timesteps) of FlowMatchScheduler(shift, sigma_min=0, extra_one_step=True).set_timesteps(1000) in float32
    (utils/scheduler.py:118-133): linspace(1, 0, 1001) without its last point, shifted."""
    s = torch.linspace(1.0, 0.0, n_train + 1)[:-1]
    s = shift * s / (1 + (shift - 1) * s)
    return s, s * n_train


def step_scalars(step_list: Sequence[int], warp: bool, shift: float, drop_trailing_zero: bool = False):
    """-> (steps tensor as the reference carries it, engine timesteps, x0 sigmas, add-noise sigmas), one entry per listed step.
    x0: argmin over the float64 timesteps, float64 sigma (wan_wrapper.py:186-195); add_noise: argmin over the float32 timesteps against
    the step in its own dtype, float32 sigma (scheduler.py:172-175)."""
    sig, ts = flow_match_tables(shift)
    steps = torch.tensor(list(step_list), dtype=torch.long)
    if drop_trailing_zero and steps[-1] == 0:                       # bidirectional_inference.py:27-28
        steps = steps[:-1]
    if warp:                                                        # causal_inference.py:29-31
        steps = torch.cat((ts, torch.tensor([0], dtype=torch.float32)))[1000 - steps]
    t_eng, s_x0, s_add = [], [], []
    for t in steps:
        t_eng.append(float(t))
        i64 = torch.argmin((ts.double().unsqueeze(0) - t.reshape(1).double().unsqueeze(1)).abs(), dim=1)
        s_x0.append(float(sig.double()[i64].item()))
        i32 = torch.argmin((ts.unsqueeze(0) - t.reshape(1).unsqueeze(1)).abs(), dim=1)
        s_add.append(float(sig[i32].item()))
    return steps, t_eng, s_x0, s_add


# ====================================================================================================== the rolling window's rule
class RollingSim:
    """`window` slots; the first `sink` FRAMES of the video are never evicted.  `put(frame)` returns the slot the frame goes to: a
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


class _CacheIndex:
    """Where a forward at (start, n) writes and what it attends, in frames, with the bookkeeping the reference keeps per layer.
    Not rolling (causal_model.py:203-226): local_end = local_end_index + current_end - global_end_index, the block is written at
    [local_end - n, local_end) and attends [max(0, local_end - window), local_end).  Rolling: `RollingSim`; every resident frame is
    attended, in slot order, and local_end is the number of resident frames."""

    def __init__(self, window: int, sink: int, rolling: bool, wiring: dict):
        self.window, self.rolling, self.wiring = window, rolling, wiring
        self.ge = self.le = 0
        self.sim = RollingSim(window, wiring["ring_protect"](sink)) if rolling else None

    def place(self, start: int, n: int):
        if self.rolling:
            write = [self.sim.put(f) for f in range(start, start + n)]
            entries = list(self.sim.entries)                                  # (slot, frame): oldest first
            self.ge, self.le = start + n, len(entries)
        else:
            le = self.le + (start + n) - self.ge
            write = list(range(le - n, le))
            entries = [(s, s) for s in range(max(0, le - self.window), le)]   # slot order is age order
            self.ge, self.le = start + n, le
        vis = sorted(s for s, _ in self.wiring["visible"](sorted(entries, key=lambda e: e[1])))
        return write, vis


# ====================================================================================================== backends
class OracleOps:
    """The records on the CPU: oracle.wan_dit_ref.dit_forward with the state dict `sd` (its dtype is the oracle's) on an oracle cache,
    fewstep_ref.ref_x0 / ref_add_noise."""

    def __init__(self, sd, cfg: dict, lat: Tuple[int, int]):
        from oracle import wan_dit_ref as W
        self.W, self.sd, self.cfg, self.ocfg = W, sd, cfg, W.DitCfg(**cfg)
        self.S = (lat[0] // 2) * (lat[1] // 2)
        self.N, self.D = cfg["num_heads"], cfg["dim"] // cfg["num_heads"]

    def caches(self, n_slots: int, kv=None):
        shape = (self.cfg["num_layers"], n_slots * self.S, self.cfg["dim"])
        k, v = (torch.zeros(shape, dtype=BF), torch.zeros(shape, dtype=BF)) if kv is None else (kv[0].clone(), kv[1].clone())
        assert tuple(k.shape) == shape and tuple(v.shape) == shape
        self.k, self.v = k, v
        self.okv = [{"k": k[l].view(1, -1, self.N, self.D), "v": v[l].view(1, -1, self.N, self.D)} for l in range(shape[0])]
        return k, v

    def latent(self, t: torch.Tensor) -> torch.Tensor:
        return t.detach().to("cpu", BF).contiguous().clone()

    def zeros(self, shape) -> torch.Tensor:
        return torch.zeros(shape, dtype=BF)

    def context(self, ctx: torch.Tensor):
        return (ctx.detach().to("cpu"), [None] * self.cfg["num_layers"])

    def _fwd(self, x, tval, frames, write, vis, handle, okv):
        t = torch.full([1, x.shape[0]], float(tval), dtype=torch.float32)
        ctx, ocross = handle
        return self.W.dit_forward(self.sd, self.ocfg, x.permute(1, 0, 2, 3), t, ctx, okv, ocross, list(frames), list(write),
                                  list(vis)).permute(1, 0, 2, 3).contiguous()

    def forward(self, x, tval, start, write, vis, handles, B):
        F = x.shape[0] // B
        frames = list(range(start, start + F))
        if B == 1:
            return self._fwd(x, tval, frames, write, vis, handles[0], self.okv)
        return torch.cat([self._fwd(x[g * F:(g + 1) * F], tval, frames, write[g * F:(g + 1) * F], vis[g], handles[g], self.okv)
                          for g in range(B)])

    def forward_full(self, x, tval, handle):
        """The whole clip: the forward on a zeroed cache of its own with frame_ids = write_slots = visible_slots = 0 .. n - 1
        (mmpl_dit_forward_full's contract)."""
        n = x.shape[0]
        return self._fwd(x, tval, range(n), range(n), range(n), handle, self.W.new_kv_cache(self.ocfg, n, self.S))

    def update(self, flow, x, noise, sigma_x0, sigma_next):
        x0 = ref_x0(flow, x, sigma_x0)
        if noise is not None:
            x.copy_(ref_add_noise(x0, noise.to("cpu", BF), sigma_next))
        return x0

    def finish(self):
        pass


class HipOps:
    """Each record is one call of its C entry on the current stream of `device`; `engine` (a DitEngine) lends the handle and the bound
    weights."""

    def __init__(self, lib, engine, device="cuda:0"):
        from mmpl_amd import _lib
        self.lib, self._lib, self.engine, self.device = lib, _lib, engine, torch.device(device)
        self.S, self.L, self.dim = engine.S, engine.L, engine.dim
        self.buffers: List[torch.Tensor] = []
        self.payload: List[int] = []
        self.calls: List[str] = []                             # the entry of every call, in order

    # ---- buffers
    def _raw(self, n_bytes: int, fill_canary: bool = False) -> torch.Tensor:
        """n_bytes of payload (uint8 view) in an int16 allocation of its own with a canary tail."""
        n = (n_bytes + 1) // 2
        b = torch.full((n + TAIL,), CANARY, dtype=torch.int16, device=self.device)
        self.buffers.append(b)
        self.payload.append(n)
        if not fill_canary:
            b[:n].zero_()
        return b[:n]

    def _bf(self, shape, fill_canary=True) -> torch.Tensor:
        n = 1
        for s in shape:
            n *= int(s)
        return self._raw(2 * n, fill_canary).view(BF).view(tuple(shape))

    def canaries_intact(self) -> bool:
        torch.cuda.synchronize(self.device)
        return all(bool((b[n:] == CANARY).all()) for b, n in zip(self.buffers, self.payload))

    def caches(self, n_slots: int, kv=None):
        shape = (self.L, n_slots * self.S, self.dim)
        self.k, self.v = self._bf(shape, fill_canary=False), self._bf(shape, fill_canary=False)
        if kv is not None:
            assert tuple(kv[0].shape) == shape and tuple(kv[1].shape) == shape
            self.k.copy_(kv[0])
            self.v.copy_(kv[1])
        self.n_slots = n_slots
        return self.k, self.v

    def latent(self, t: torch.Tensor) -> torch.Tensor:
        b = self._bf(t.shape)
        b.copy_(t.to(self.device, BF))
        return b

    def zeros(self, shape) -> torch.Tensor:
        return self._bf(shape, fill_canary=False)

    def _t(self, tval: float, n: int) -> torch.Tensor:
        t = self._raw(4 * n).view(torch.float32)
        t.fill_(float(tval))
        return t

    def _p(self, t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        self.calls.append(name)
        with torch.cuda.device(self.device):
            self._lib.check(getattr(self.lib, name)(*args, self._stream()), name)

    # ---- records
    def context(self, ctx: torch.Tensor):
        e = self.engine
        c = self._bf((e.text_len, e.text_dim), fill_canary=False)
        c[:ctx.shape[0]].copy_(ctx.to(self.device, BF))
        ck, cv = self._bf((self.L, e.text_len, self.dim)), self._bf((self.L, e.text_len, self.dim))
        nb = self.lib.mmpl_dit_context_workspace_bytes(e._h)
        ws = self._raw(nb, fill_canary=True)
        rows = C.c_int(-1)
        self._call("mmpl_dit_precompute_context", e._h, self._p(c), self._p(ck), self._p(cv), self._p(ws), nb, C.byref(rows))
        return ck, cv

    def forward(self, x, tval, start, write, vis, handles, B):
        e, nF = self.engine, x.shape[0]
        F = nF // B
        ia = lambda v: (C.c_int * len(v))(*[int(i) for i in v])
        t = self._t(tval, nF)
        out = self._bf((nF, 16, e.lat_h, e.lat_w))
        nb = self.lib.mmpl_dit_workspace_bytes(e._h, nF)
        ws = self._raw(nb, fill_canary=True)
        ids = [start + i for _ in range(B) for i in range(F)]                    # absolute frame ids, sample-major
        if B == 1:
            ck, cv = handles[0]
            self._call("mmpl_dit_forward_at", e._h, self._p(x), self._p(t), nF, ia(ids), ia(write), ia(vis), len(vis), self._p(self.k),
                       self._p(self.v), self.n_slots, self._p(ck), self._p(cv), CROSS_ROWS_ALL, None, None, None, self._p(out), self._p(ws),
                       nb, None)
        else:
            pa = lambda ts: (C.c_void_p * B)(*[tt.data_ptr() for tt in ts])
            self._call("mmpl_dit_forward_groups", e._h, self._p(x), self._p(t), B, F, ia(ids), ia(write), ia([s for v in vis for s in v]),
                       len(vis[0]), self._p(self.k), self._p(self.v), self.n_slots, pa([h[0] for h in handles]),
                       pa([h[1] for h in handles]), CROSS_ROWS_ALL, None, None, None, self._p(out), self._p(ws), nb, None)
        return out

    def forward_full(self, x, tval, handle):
        e, nF = self.engine, x.shape[0]
        t = self._t(tval, 1)
        out = self._bf((nF, 16, e.lat_h, e.lat_w))
        nb = self.lib.mmpl_dit_full_workspace_bytes(e._h, nF)
        ws = self._raw(nb, fill_canary=True)
        self._call("mmpl_dit_forward_full", e._h, self._p(x), self._p(t), nF, self._p(handle[0]), self._p(handle[1]), CROSS_ROWS_ALL, None,
                   None, None, self._p(out), self._p(ws), nb)
        return out

    def update(self, flow, x, noise, sigma_x0, sigma_next):
        x0 = self._bf(x.shape)
        nz = None
        if noise is not None:
            nz = self._bf(x.shape)
            nz.copy_(noise.to(self.device, BF).reshape(x.shape))
        self._call("mmpl_fewstep_update", self._p(flow), self._p(x), self._p(nz), self._p(x0), x.numel(), float(sigma_x0),
                   0.0 if sigma_next is None else float(sigma_next))
        return x0

    def finish(self):
        torch.cuda.synchronize(self.device)


# ====================================================================================================== the chains
def _distinct(ops, contexts):
    """One handle per DISTINCT context (one precompute each); samples with equal contexts share the handle's tensors."""
    seen, handles = [], []
    for c in contexts:
        for c0, h in seen:
            if c0 is c or (c0.shape == c.shape and torch.equal(c0, c)):
                handles.append(h)
                break
        else:
            h = ops.context(c)
            seen.append((c, h))
            handles.append(h)
    return handles


class FewstepChain:
    """CausalInferencePipeline.inference.  cfg: the model config; lat: (lat_h, lat_w); window: the attention window = the cache's
    frame slots per sample (21 at local_attn_size -1); sink: sink frames of the rolling window; context_noise: the refresh timestep."""

    def __init__(self, cfg: dict, lat: Tuple[int, int], ops, *, step_list, warp: bool, shift: float, frames_per_block: int,
                 independent_first_frame: bool = False, context_noise: float = 0, window: int = 21, sink: int = 0, rolling: bool = False,
                 wiring: Optional[dict] = None):
        self.cfg, self.lat, self.ops = cfg, tuple(lat), ops
        self.wiring = dict(WIRING, **(wiring or {}))
        self.steps, self.t_eng, self.sig_x0, self.sig_add = step_scalars(step_list, warp, shift)
        self.F, self.iff, self.context_noise = int(frames_per_block), bool(independent_first_frame), context_noise
        self.window, self.sink, self.rolling = int(window), int(sink), bool(rolling)

    def schedule(self, num_frames: int, n_initial: int) -> List[int]:
        """Frames per denoised block (causal_inference.py:68-79, 177-179)."""
        F = self.F
        if not self.iff or n_initial:
            assert num_frames % F == 0
            return [F] * (num_frames // F)
        assert (num_frames - 1) % F == 0
        return [1] + [F] * ((num_frames - 1) // F)

    def plan(self, num_frames: int, n_initial: int = 0, B: int = 1) -> List[tuple]:
        """The call as records, in order: ("context", start, n, write, vis), ("forward", step i, t, start, write, vis),
        ("update", i, sigma_x0, sigma_next or None, draw index or None), ("refresh", t, start, write, vis, "x0" | "x"),
        ("ends", global_end, local_end) -- frames and frame slots; a batch's write slots are sample-major, its visible slots one list
        per sample."""
        w, F = self.wiring, self.F
        idx = _CacheIndex(self.window, self.sink, self.rolling, w)
        off = [w["sample_offset"](g, self.window) for g in range(B)]

        def place(start, n):
            write, vis = idx.place(start, n)
            if B == 1:
                return write, vis
            return [s + o for o in off for s in write], [[s + o for s in vis] for o in off]

        recs, start = [], 0
        if n_initial:                                                   # causal_inference.py:136-169
            heads = []
            if self.iff:
                assert (n_initial - 1) % F == 0
                heads = [1]
            else:
                assert n_initial % F == 0
            for n in heads + [F] * ((n_initial - len(heads)) // F):
                if w["initial_forward"]:
                    recs.append(("context", start, n) + place(start, n))
                    recs.append(("ends", idx.ge, idx.le))
                start += n
        n_steps, draw0 = len(self.t_eng), 0
        for n in self.schedule(num_frames, n_initial):                  # :177-244
            write, vis = place(start, n)
            for i in range(n_steps):
                recs.append(("forward", i, self.t_eng[i], start, write, vis))
                last = i == n_steps - 1
                recs.append(("update", i, self.sig_x0[i], None if last else self.sig_add[w["sigma_next_step"](i)],
                             None if last else draw0 + w["draw_of_step"](i, n_steps - 1)))
            draw0 += n_steps - 1
            if w["refresh"]:
                recs.append(("refresh", float(w["refresh_t"](self.context_noise, self.t_eng)), start, write, vis, w["refresh_input"]))
            recs.append(("ends", idx.ge, idx.le))
            start += n
        return recs

    def run(self, noise: torch.Tensor, contexts: Sequence[torch.Tensor], draws: Sequence[torch.Tensor],
            initial_latent: Optional[torch.Tensor] = None, kv=None):
        """noise [B, T, 16, h, w]; contexts: B tensors [<= text_len, text_dim]; draws: one [F, 16, h, w] ([B, F, 16, h, w] for a batch)
        per non-final step, in block order; initial_latent [B, n, 16, h, w]; kv: the (K, V) the caches start from, [L, B * window * S,
        dim] (zeros when None; cloned).  -> (latents [B, n + T, 16, h, w], K cache, V cache, (global_end, local_end) in frames)."""
        ops, w = self.ops, self.wiring
        B, T = noise.shape[:2]
        frame = tuple(noise.shape[2:])
        n_init = 0 if initial_latent is None else initial_latent.shape[1]
        assert len(contexts) == B
        plan = self.plan(T, n_init, B)
        k, v = ops.caches(B * self.window, kv)
        handles = _distinct(ops, contexts)
        out = ops.zeros((B, n_init + T) + frame)
        if n_init:
            out[:, :n_init].copy_(initial_latent.to(out.device, BF))
        x = x0 = flow = None
        ends = (0, 0)
        for rec in plan:
            kind = rec[0]
            if kind == "context":
                _, start, n, write, vis = rec
                ops.forward(ops.latent(initial_latent[:, start:start + n].reshape((B * n,) + frame)), 0.0, start, write, vis, handles, B)
            elif kind == "forward":
                _, i, t, start, write, vis = rec
                if i == 0:
                    n = len(write) // B
                    x = ops.latent(noise[:, start - n_init:start - n_init + n].reshape((B * n,) + frame))
                flow = ops.forward(x, t, start, write, vis, handles, B)
            elif kind == "update":
                _, i, s_x0, s_next, d = rec
                nz = None
                if d is not None:
                    nz = draws[d] if B == 1 else w["bank_rows"](draws[d])
                x0 = ops.update(flow, x, nz, s_x0, s_next)
                if s_next is None:                                      # output[:, block] = denoised_pred (:224)
                    n = x0.shape[0] // B
                    out[:, start:start + n].copy_(x0.view((B, n) + frame))
            elif kind == "refresh":
                _, t, start, write, vis, src = rec
                ops.forward(x0 if src == "x0" else x, t, start, write, vis, handles, B)
            else:
                ends = rec[1:]
        ops.finish()
        return out, k, v, ends


class BidirFewstepChain:
    """BidirectionalInferencePipeline.inference (bidirectional_inference.py:27-31, 52-67): a trailing 0 is dropped from the step list,
    the generator runs at every listed step but the last, the predicted x0 is re-noised to the next listed step after EVERY forward
    (the last one included: its draw is consumed although nothing reads the result), and the last x0 is the result."""

    def __init__(self, cfg: dict, lat: Tuple[int, int], ops, *, step_list, warp: bool, shift: float, wiring: Optional[dict] = None):
        self.cfg, self.lat, self.ops = cfg, tuple(lat), ops
        self.wiring = dict(WIRING, **(wiring or {}))
        self.steps, self.t_eng, self.sig_x0, self.sig_add = step_scalars(step_list, warp, shift, drop_trailing_zero=True)

    def plan(self, num_frames: int) -> List[tuple]:
        w, n = self.wiring, len(self.t_eng) - 1
        recs = []
        for i in range(n):
            recs.append(("forward", i, self.t_eng[i]))
            recs.append(("update", i, self.sig_x0[i], self.sig_add[w["sigma_next_step"](i)], w["draw_of_step"](i, n)))
        return recs

    def run(self, noise: torch.Tensor, context: torch.Tensor, draws: Sequence[torch.Tensor]) -> torch.Tensor:
        """noise [1, F, 16, h, w]; draws: one [F, 16, h, w] per forward.  -> the last x0 [1, F, 16, h, w]."""
        ops = self.ops
        handle = ops.context(context)
        x = ops.latent(noise[0])
        x0 = flow = None
        for rec in self.plan(noise.shape[1]):
            if rec[0] == "forward":
                flow = ops.forward_full(x, rec[2], handle)
            else:
                _, i, s_x0, s_next, d = rec
                x0 = ops.update(flow, x, draws[d], s_x0, s_next)
        ops.finish()
        return x0.unsqueeze(0)
