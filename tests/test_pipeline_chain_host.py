"""tests/pipeline_chain.py IS the reference's loop (CPU): the OracleOps chain against fixtures of the real reference
(tests/golden/make_golden_fewstep_chain.py -> fewstep_chain_tiny.pt), its scalars against the fixtures' step lists, every wiring mutant
against the same bound, the rolling plans against the stated rule, and `plan()` record by record against what the library's pipelines
issue to a recording stub generator -- a readable first failure before tests/test_pipeline_chain_gpu.py demands equal bits.

The bound is the project's convention for trajectories: rel-L2 <= 2 x the case's `order_out` (the reference against itself with its
K / V in reverse frame order).  The causal cases run on sharpened attention (QK-norm gains x 8, `qk_gain` in the fixture's meta): with the
plain synthetic weights a wrong cache moves the trajectory by no more than the order noise (refresh omitted: 3.8e-3 against a bound
of 4.5e-3), so no bound could tell the cache mutants from the loop.  Measured (tiny model in bf16, 16 x 24 latents, CPU oracle;
`pytest -s` prints them) -- rel-L2 against the reference's output:

  case  order_out  bound      chain      mutants on that case (each must EXCEED the bound)
  a     3.418e-03  6.836e-03  0.000e+00  sigma_next_from_step_i 3.888e-01, draws_reversed 1.094e+00, refresh_omitted 3.594e-02,
                                         refresh_at_last_t 1.018e-02, refresh_reads_x 3.581e-02, visible_missing_oldest 3.895e-02
  b     2.875e-03  5.750e-03  0.000e+00
  c     3.168e-03  6.336e-03  0.000e+00  initial_not_forwarded 3.934e-02
  d     2.120e-03  4.240e-03  0.000e+00  initial_not_forwarded 3.470e-02
  e     3.270e-03  6.540e-03  0.000e+00  bank_frame_major 1.156e+00, sample1_on_sample0_slots 3.166e-02
  f     1.717e-03  3.433e-03  0.000e+00  sigma_next_from_step_i 1.742e-01, draws_reversed 2.962e-01

(The chain's 0: the oracle performs the reference's operations in the reference's order on the same CPU kernels.)
"""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pipeline_chain as PC  # noqa: E402
from util import GOLDEN, rel_l2  # noqa: E402

LAT = (16, 24)
S = 96
FRAME = (16,) + LAT
STEPS = [1000, 750, 500, 250]


@functools.lru_cache(maxsize=None)
def _fx():
    return torch.load(os.path.join(GOLDEN, "fewstep_chain_tiny.pt"))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The case's inputs, regenerated from the seeds in its meta the way the generator made them."""
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    m = _fx()[name]["meta"]
    cfg = WAN_CONFIGS[m["cfg"]]
    B = m["batch"]
    ctxs = []
    for s, n in zip(m["ctx_seeds"], m["n_valid"]):
        c = philox_normal([1, 512, cfg["text_dim"]], s)[0]
        c[n:] = 0
        ctxs.append(c)
    noise = philox_normal([B, m["n_noise"], 16, *LAT], m["noise_seed"])
    init = philox_normal([B, m["n_init"], 16, *LAT], m["init_seed"]) if m["n_init"] else None
    if m["kind"] == "bidir":
        draws = [philox_normal([m["n_noise"], 16, *LAT], m["renoise_seed_base"] + k) for k in range(m["n_draws"])]
    else:
        per = len(m["denoising_step_list"]) - 1
        draws = [philox_normal(([B] if B > 1 else []) + [f, 16, *LAT], m["renoise_seed_base"] + k)
                 for k, f in enumerate(f for f in m["schedule"] for _ in range(per))]
    sd = dit_state_dict(cfg, seed=m["weight_seed"])
    for l in range(cfg["num_layers"]):                                  # make_golden_fewstep_chain.sharpen
        for k in (f"blocks.{l}.self_attn.norm_q.weight", f"blocks.{l}.self_attn.norm_k.weight"):
            sd[k] = (sd[k].float() * m["qk_gain"]).to(sd[k].dtype)
    return cfg, sd, ctxs, noise, init, draws


def _chain(name, wiring=None):
    m = _fx()[name]["meta"]
    cfg, sd = _inputs(name)[:2]
    ops = PC.OracleOps(sd, cfg, LAT)
    kw = dict(step_list=m["denoising_step_list"], warp=m["warp_denoising_step"], shift=m["timestep_shift"], wiring=wiring)
    if m["kind"] == "bidir":
        return PC.BidirFewstepChain(cfg, LAT, ops, **kw)
    return PC.FewstepChain(cfg, LAT, ops, frames_per_block=m["num_frame_per_block"], independent_first_frame=m["independent_first_frame"],
                           context_noise=m["context_noise"], window=21, **kw)


def _error(name, wiring=None):
    """rel-L2 of the (mutated) OracleOps chain against the reference's output of the case."""
    _, _, ctxs, noise, init, draws = _inputs(name)
    ch = _chain(name, wiring)
    with torch.no_grad():
        out = ch.run(noise, ctxs[0], draws) if _fx()[name]["meta"]["kind"] == "bidir" else ch.run(noise, ctxs, draws, init)[0]
    return rel_l2(out, _fx()[name]["out"])


# ------------------------------------------------------------------------------------------------ the chain is the reference's loop
@pytest.mark.parametrize("name", list("abcdef"))
def test_oracle_chain_reproduces_the_reference(name):
    fx = _fx()[name]
    e = _error(name)
    print(f"[pipeline chain] case {name}: rel_l2 vs reference {e:.3e} (K/V order noise {fx['order_out']:.3e}, bound {2 * fx['order_out']:.3e})")
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


@pytest.mark.parametrize("name", list("abcdef"))
def test_step_list_and_scalars(name):
    """The chain's own FlowMatchScheduler tables and warped step list, bit for bit: against the reference's step list in the fixture
    and against the library's tables; the x0 sigma is the float64 table's entry, the add-noise sigma the float32 table's."""
    from mmpl_amd.scheduler import FlowMatchScheduler
    ch = _chain(name)
    want = _fx()[name]["step_list"]
    assert ch.steps.dtype == want.dtype == torch.float32 and torch.equal(ch.steps, want)
    s = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    s.set_timesteps(1000, training=True)
    sig, ts = PC.flow_match_tables(5.0)
    assert torch.equal(sig, s.sigmas) and torch.equal(ts, s.timesteps)
    assert ch.t_eng == [1000.0, 937.5, float(torch.tensor(833.3333129882812, dtype=torch.float32)), 625.0]
    for i, t in enumerate(ch.steps):
        j = int(torch.argmin((ts.double() - t.double()).abs()))
        assert ch.sig_x0[i] == float(sig[j].double()) and ch.sig_add[i] == float(sig[j])


def test_unwarped_steps_stay_integers():
    steps, t_eng, s_x0, s_add = PC.step_scalars(STEPS, False, 5.0)
    assert steps.dtype == torch.int64 and t_eng == [1000.0, 750.0, 500.0, 250.0]
    sig, ts = PC.flow_match_tables(5.0)
    assert s_add == [float(sig[int(torch.argmin((ts - t).abs()))]) for t in t_eng]
    assert PC.step_scalars([1000, 500, 0], False, 5.0, drop_trailing_zero=True)[1] == [1000.0, 500.0]


# ------------------------------------------------------------------------------------------------ mutants
MUTANTS = {
    "sigma_next_from_step_i": dict(sigma_next_step=lambda i: i),
    "draws_reversed": dict(draw_of_step=lambda i, n: n - 1 - i),
    "refresh_omitted": dict(refresh=False),
    "refresh_at_last_t": dict(refresh_t=lambda context_noise, step_ts: step_ts[-1]),
    "refresh_reads_x": dict(refresh_input="x"),
    "visible_missing_oldest": dict(visible=lambda entries: entries[1:] if len(entries) > 1 else entries),
    "bank_frame_major": dict(bank_rows=lambda d: d.transpose(0, 1).reshape((-1,) + tuple(d.shape[2:]))),
    "sample1_on_sample0_slots": dict(sample_offset=lambda g, n_slots: 0),
    "initial_not_forwarded": dict(initial_forward=False),
    "ring_without_sink": dict(ring_protect=lambda sink: 0),
}
ON_CASE = [("sigma_next_from_step_i", "a"), ("draws_reversed", "a"), ("refresh_omitted", "a"), ("refresh_at_last_t", "a"),
           ("refresh_reads_x", "a"), ("visible_missing_oldest", "a"), ("bank_frame_major", "e"), ("sample1_on_sample0_slots", "e"),
           ("initial_not_forwarded", "c"), ("initial_not_forwarded", "d"), ("sigma_next_from_step_i", "f"), ("draws_reversed", "f")]


@pytest.mark.parametrize("mutant,name", ON_CASE)
def test_mutant_exceeds_the_bound(mutant, name):
    fx = _fx()[name]
    e = _error(name, MUTANTS[mutant])
    print(f"[pipeline chain] case {name}, mutant {mutant}: rel_l2 vs reference {e:.3e} (bound {2 * fx['order_out']:.3e})")
    assert e > 2.0 * fx["order_out"], (mutant, e, fx["order_out"])


# ------------------------------------------------------------------------------------------------ rolling plans (host only)
def _rolling_chain(W, sink, wiring=None, rolling=True, ops=None, context_noise=0):
    from mmpl_amd.synthetic import WAN_CONFIGS
    return PC.FewstepChain(WAN_CONFIGS["tiny"], LAT, ops, step_list=STEPS, warp=True, shift=5.0, frames_per_block=3, window=W, sink=sink,
                           rolling=rolling, context_noise=context_noise, wiring=wiring)


@pytest.mark.parametrize("W,sink", [(8, 2), (6, 0), (6, 1)])
def test_rolling_plan(W, sink):
    plan = _rolling_chain(W, sink).plan(18)
    blocks = PC.schedule_slots(W, sink, [3] * 6)
    held = {}                                                           # slot -> frame
    fwd = [r for r in plan if r[0] == "forward" and r[1] == 0]
    assert len(fwd) == 6
    R = W - sink
    for (_, _, _, start, write, vis), (b_start, n, b_write, b_vis, _) in zip(fwd, blocks):
        assert (start, write, vis) == (b_start, b_write, b_vis)
        assert write == [f if f < W else sink + (f - sink) % R for f in range(start, start + n)]       # rolling_slots' docstring
        end = start + n
        need = set(range(end)) if end <= W else set(range(sink)) | set(range(end - R, end))
        evicted = {held[s] for s in write if s in held}
        assert not evicted & need, (start, evicted)                     # nothing it still has to see is overwritten
        for s, f in zip(write, range(start, end)):
            held[s] = f
        assert {held[s] for s in vis} == need, (start, vis)             # the sink frames + the most recent W - sink, its own included
    # every forward, update and refresh of a block runs on the block's slots; the ends are (frames so far, resident frames)
    for r in plan:
        if r[0] == "refresh":
            assert (r[3], r[4]) == next((f[4], f[5]) for f in fwd if f[3] == r[2])
    assert [r[1:] for r in plan if r[0] == "ends"] == [(3 * (i + 1), min(3 * (i + 1), W)) for i in range(6)]
    if (W, sink) == (8, 2):
        assert fwd[2][4] == [6, 7, 2]                                   # the docstring's worked example: frames 6, 7, 8


@functools.lru_cache(maxsize=None)
def _rolling_run(W, sink, rolling, mutant=None, frames=9):
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    cfg = WAN_CONFIGS["tiny"]
    ops = PC.OracleOps(dit_state_dict(cfg, seed=211), cfg, LAT)
    ch = _rolling_chain(W, sink, MUTANTS[mutant] if mutant else None, rolling, ops, context_noise=100)
    ctx = philox_normal([512, cfg["text_dim"]], 212)
    ctx[30:] = 0
    noise = philox_normal([1, frames, 16, *LAT], 213)
    draws = [philox_normal([3, 16, *LAT], 220 + k) for k in range(3 * frames // 3)]
    with torch.no_grad():
        out, k, v, ends = ch.run(noise, [ctx], draws)
    return out, k, v, ends


def test_rolling_below_the_window_is_the_causal_layout():
    a = _rolling_run(9, 2, True)
    b = _rolling_run(9, 2, False)
    assert a[3] == b[3] == (9, 9)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("mutant", ["ring_without_sink", "visible_missing_oldest"])
def test_rolling_mutants_change_the_output(mutant):
    good = _rolling_run(5, 2, True)
    bad = _rolling_run(5, 2, True, mutant)
    assert good[3] == (9, 5)
    assert not torch.equal(good[0].view(torch.int16), bad[0].view(torch.int16))


# ------------------------------------------------------------------------------------------------ plan() against the pipelines
class _KV(list):
    def __init__(self, n_slots, batch=1):
        super().__init__([{"global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])}])
        self.engine, self.batch, self.n_slots = types.SimpleNamespace(S=S), batch, n_slots
        self.k_all = torch.zeros(1, batch * n_slots * S, 8)


class _Cross(list):
    def fill(self, pe, shared=False):
        pass


def _tup(v):
    return tuple(_tup(i) for i in v) if isinstance(v, (list, tuple)) else int(v)


class _RecGen:
    """A generator that launches nothing and records what it is asked to launch.  `slots` and the two sigma lookups are the wrapper's
    own (bound to this object): the slot and scalar helpers are part of what is compared."""

    def __init__(self, window, sink=0, is_causal=True):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper as Wd
        self.geometry = Geometry(*LAT)
        self.engine = types.SimpleNamespace(L=1, max_frames=7, S=S, full_workspace=lambda n: None)
        self.model = types.SimpleNamespace(local_attn_size=window, sink_size=sink, num_frame_per_block=1)
        self.window_frames, self.is_causal, self.model_type = window, is_causal, "t2v"
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self._sig64, self._ts64 = self.scheduler.sigmas.double(), self.scheduler.timesteps.double()
        self.slots = types.MethodType(Wd.slots, self)
        self.sigma_x0 = types.MethodType(Wd.sigma_x0, self)
        self.sigma_add_noise = types.MethodType(Wd.sigma_add_noise, self)
        self.events, self._x0_ptr = [], None

    def get_scheduler(self):
        return self.scheduler

    def new_kv_cache(self, batch=1):
        return _KV(self.window_frames, batch)

    def new_crossattn_cache(self, batch=1):
        return _Cross()

    def set_cache_ends(self, kv, ge, le):
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper as Wd
        Wd.set_cache_ends(kv, ge, le)
        self.events.append(("ends", ge, le))

    def flow(self, x, t, start, write, vis, kv, cross, out=None, frame_base=None):
        assert frame_base is None or (frame_base.dtype == torch.int32 and frame_base.numel() == 1)
        assert bool((t == t[0]).all()) and t.numel() == x.shape[0]
        src = "x0" if x.data_ptr() == self._x0_ptr else "x"
        self.events.append(("flow", src, float(t[0]), start + (0 if frame_base is None else int(frame_base)), _tup(write), _tup(vis)))
        return out

    def flow_full(self, x, t, cross, out=None):
        self.events.append(("flow_full", float(t[0])))
        return out

    def fewstep_update(self, flow, x, noise, x0_out, sigma_t, sigma_next=0.0):
        self._x0_ptr = x0_out.data_ptr()
        self.events.append(("update", sigma_t, None if noise is None else sigma_next, None if noise is None else int(noise.reshape(-1)[0])))


def _events(plan):
    """A plan's records in the stub's vocabulary."""
    ev = []
    for r in plan:
        if r[0] == "context":
            ev.append(("flow", "x", 0.0, r[1], _tup(r[3]), _tup(r[4])))
        elif r[0] == "forward":
            ev.append(("flow", "x", r[2], r[3], _tup(r[4]), _tup(r[5])))
        elif r[0] == "refresh":
            ev.append(("flow", r[5], r[1], r[2], _tup(r[3]), _tup(r[4])))
        elif r[0] == "update":
            ev.append(("update",) + tuple(r[2:]))
        else:
            ev.append(tuple(r))
    return ev


# every configuration of tests/test_pipeline_chain_gpu.py: (id, pipeline args, window, sink, batch, noise frames, initial frames)
CONFIGS = [
    ("plain-9", {}, -1, 0, 1, 9, 0),
    ("first-frame-1+3+3", dict(independent_first_frame=True), -1, 0, 1, 7, 0),
    ("context-noise-100", dict(context_noise=100), -1, 0, 1, 9, 0),
    ("initial-3+6", {}, -1, 0, 1, 6, 3),
    ("first-frame-initial-1+3+3", dict(independent_first_frame=True), -1, 0, 1, 3, 4),
    ("rolling-8-sink-2", dict(rolling_kv=True), 8, 2, 1, 18, 0),
    ("rolling-6-sink-0", dict(rolling_kv=True), 6, 0, 1, 18, 0),
    ("batch-2", {}, -1, 0, 2, 6, 0),
    ("batch-2-rolling-6-sink-1", dict(rolling_kv=True), 6, 1, 2, 12, 0),
]


@pytest.mark.parametrize("cid,extra,window,sink,B,T,n_init", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_plan_equals_what_the_pipeline_issues(cid, extra, window, sink, B, T, n_init):
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS
    a = dict(denoising_step_list=STEPS, warp_denoising_step=True, num_frame_per_block=3, independent_first_frame=False, context_noise=0)
    a.update(extra)
    W = 21 if window == -1 else window
    gen = _RecGen(W, sink)
    pipe = CausalInferencePipeline(types.SimpleNamespace(**a), "cpu", generator=gen,
                                   text_encoder=lambda text_prompts: {"prompt_embeds": torch.zeros(len(text_prompts), 4, 4)}, vae=object())
    pipe.use_graphs = False
    chain = PC.FewstepChain(WAN_CONFIGS["tiny"], LAT, None, step_list=STEPS, warp=True, shift=5.0, frames_per_block=3,
                            independent_first_frame=a["independent_first_frame"], context_noise=a["context_noise"], window=W, sink=sink,
                            rolling=bool(a.get("rolling_kv")))
    want = _events(chain.plan(T, n_init, B))
    n_draws = sum(1 for r in want if r[0] == "update" and r[3] is not None)
    sched = chain.schedule(T, n_init)
    assert n_draws == 3 * len(sched)
    for call in range(2):                                               # the second call starts from reset bookkeeping: the same plan
        gen.events.clear()
        pipe.renoise_override = [torch.full(([B] if B > 1 else []) + [f, *FRAME], float(k), dtype=torch.bfloat16)
                                 for k, f in enumerate(f for f in sched for _ in range(3))]
        init = torch.zeros(B, n_init, *FRAME) if n_init else None
        with torch.no_grad():
            for _ in pipe._blocks(torch.zeros(B, T, *FRAME), ["p%d" % g for g in range(B)], init):
                pass
        exp_all = ([("ends", 0, 0)] if call else []) + want           # a later call first resets the bookkeeping (:123-132)
        for i, (got, exp) in enumerate(zip(gen.events, exp_all)):
            assert got == exp, f"{cid}, call {call}, record {i}: the pipeline issued {got}, the chain plans {exp}"
        assert len(gen.events) == len(exp_all)
    for store in pipe._stores:
        store.clear()


@pytest.mark.parametrize("steps", [[1000, 750, 500], [1000, 750, 500, 250, 0]], ids=["3-steps", "ending-in-0"])
def test_bidirectional_plan_equals_what_the_pipeline_issues(steps):
    from mmpl_amd.pipeline import BidirectionalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS
    gen = _RecGen(21, is_causal=False)
    pipe = BidirectionalInferencePipeline(types.SimpleNamespace(denoising_step_list=steps, warp_denoising_step=True), "cpu", generator=gen,
                                          text_encoder=lambda text_prompts: {"prompt_embeds": torch.zeros(1, 4, 4)},
                                          vae=types.SimpleNamespace(decode_to_pixel=lambda lat, **kw: torch.zeros(1, 1, 3, 8, 8)))
    pipe.use_graphs = False
    chain = PC.BidirFewstepChain(WAN_CONFIGS["tiny"], LAT, None, step_list=steps, warp=True, shift=5.0)
    plan = chain.plan(5)
    n_fwd = len([s for s in steps if s != 0]) - 1
    assert len(plan) == 2 * n_fwd
    pipe.renoise_override = [torch.full([5, *FRAME], float(k), dtype=torch.bfloat16) for k in range(n_fwd)]
    pipe.inference(torch.zeros(1, 5, *FRAME), ["p"])
    want = [("flow_full", r[2]) if r[0] == "forward" else ("update",) + tuple(r[2:]) for r in plan]
    assert gen.events == want
    pipe._calls.clear()
