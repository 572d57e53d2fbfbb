"""CausalInferencePipeline.inference and BidirectionalInferencePipeline.inference against THE SAME ENTRY CALLS MADE ONE AT A TIME (-m gpu):
the HipOps chain of tests/pipeline_chain.py, written from the reference's loop (tests/test_pipeline_chain_host.py holds it to the real
reference on the CPU, where it is exact, and compares its plan with the pipelines' record by record).  The loop -- which forward at which
timestep on which buffer, which sigma, which draw, which KV slots (ring, sink, per-sample offsets, frame_base), when the refresh runs,
what initial_latent leaves in the cache, what a replayed hipGraph's static buffers hold -- has no rounding of its own, so the
statement is the strongest there is: EVERY BIT equal.

Set-up of every case: the tiny model at 16 x 24 latents (S = 96: no multiple of the 64-row wave tile or the 256-row query block), 3 frames
per block, [1000, 750, 500, 250] warped, shift 5.  The pipeline runs on a KV cache filled with a seeded non-zero pattern, the chain on
a clone of it; equal bits are demanded of the returned latents, of the whole K and V cache (every layer and slot: unwritten slots keep
their fill) and of every layer's global / local end index, and every HipOps canary must be intact.  Each HipOps record is one ctypes
call, eager, absolute frame ids, frame_base NULL, every buffer an allocation of its own.
"""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pipeline_chain as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LAT = (16, 24)
FRAME = (16,) + LAT
STEPS = [1000, 750, 500, 250]
SHIFT = 5.0
PROMPTS = {"p0": (301, 40), "p1": (302, 17), "p2": (303, 64), "p3": (304, 5)}         # prompt -> (context seed, valid rows)


def bits(t):
    return t.contiguous().view(torch.int16)


def n_diff(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return int((bits(a) != bits(b)).sum())


class _Text(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, text_prompts):
        return {"prompt_embeds": torch.stack([self.table[p] for p in text_prompts])}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


class Rig:
    """The weights, one generator per (causal, window, sink) and one pipeline per argument set, built on first use and kept for the
    module; `close()` releases every pipeline's graphs."""

    def __init__(self):
        from mmpl_amd import _lib
        from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
        self.cfg = WAN_CONFIGS["tiny"]
        self.sd = dit_state_dict(self.cfg, seed=7)
        self.lib = _lib.load()
        self.table = {}
        for p, (seed, n) in PROMPTS.items():
            c = philox_normal([512, self.cfg["text_dim"]], seed)
            c[n:] = 0
            self.table[p] = c.to(DEV)
        self.gens, self.pipes = {}, {}

    def gen(self, causal=True, window=-1, sink=0):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper
        key = (causal, window, sink)
        if key not in self.gens:
            g = WanDiffusionWrapper(is_causal=causal, timestep_shift=SHIFT, local_attn_size=window, sink_size=sink, model_config=self.cfg,
                                    geometry=Geometry(*LAT), device=DEV)
            g.load_state_dict(self.sd)
            self.gens[key] = g
        return self.gens[key]

    def pipe(self, window=-1, sink=0, **kw):
        from mmpl_amd.pipeline import CausalInferencePipeline
        key = (window, sink, tuple(sorted(kw.items())))
        if key not in self.pipes:
            a = dict(denoising_step_list=STEPS, warp_denoising_step=True, num_frame_per_block=3, independent_first_frame=False,
                     context_noise=0, model_kwargs={"timestep_shift": SHIFT})
            a.update(kw)
            self.pipes[key] = CausalInferencePipeline(types.SimpleNamespace(**a), DEV, generator=self.gen(True, window, sink),
                                                      text_encoder=_Text(self.table), vae=_NoVAE())
        return self.pipes[key]

    def bidir(self, steps):
        from mmpl_amd.pipeline import BidirectionalInferencePipeline
        key = ("bidir", tuple(steps))
        if key not in self.pipes:
            a = types.SimpleNamespace(denoising_step_list=list(steps), warp_denoising_step=True, model_kwargs={"timestep_shift": SHIFT})
            self.pipes[key] = BidirectionalInferencePipeline(a, DEV, generator=self.gen(False), text_encoder=_Text(self.table), vae=_NoVAE())
        return self.pipes[key]

    def chain(self, pipe, wiring=None):
        a, g = pipe.args, pipe.generator
        ops = PC.HipOps(self.lib, g.engine, DEV)
        return PC.FewstepChain(self.cfg, LAT, ops, step_list=STEPS, warp=True, shift=SHIFT, frames_per_block=3,
                               independent_first_frame=a.independent_first_frame, context_noise=a.context_noise, window=g.window_frames,
                               sink=int(g.model.sink_size), rolling=bool(getattr(a, "rolling_kv", False)), wiring=wiring), ops

    def close(self):
        for p in self.pipes.values():
            p.release_graphs()
        self.pipes.clear()
        self.gens.clear()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _inputs(rig, pipe, prompts, T, n_init, seed, rng_seed=None):
    """noise, initial latent, contexts, the re-noise draws (seeded, or -- rng_seed -- what a same-seed device generator gives in block
    order) and the seeded fill of the KV cache."""
    from mmpl_amd.synthetic import philox_normal
    B = len(prompts)
    ch, _ = rig.chain(pipe)
    sched = ch.schedule(T, n_init)
    noise = philox_normal([B, T, *FRAME], seed).to(DEV)
    init = philox_normal([B, n_init, *FRAME], seed + 1).to(DEV) if n_init else None
    shapes = [([B] if B > 1 else []) + [f, *FRAME] for f in sched for _ in range(len(STEPS) - 1)]
    if rng_seed is None:
        draws = [philox_normal(s, seed + 10 + k).to(DEV) for k, s in enumerate(shapes)]
    else:
        g = torch.Generator(device=DEV).manual_seed(rng_seed)
        draws = [torch.randn(s, dtype=BF, device=DEV, generator=g) for s in shapes]
    n_slots = B * pipe.generator.window_frames
    eng = pipe.generator.engine
    fill = [philox_normal([eng.L, n_slots * eng.S, eng.dim], seed + 2 + i).to(DEV) for i in range(2)]
    return dict(prompts=list(prompts), noise=noise, init=init, contexts=[rig.table[p] for p in prompts], draws=draws, fill=fill, B=B)


def _library(pipe, inp, use_graphs=True, rng_seed=None):
    """One inference() on a caller-installed, seeded KV cache -> what it returned and left behind."""
    B, gen = inp["B"], pipe.generator
    if B not in pipe._caches:                              # the pipeline accepts a caller-installed pair (and then keeps it: its graphs
        pipe.kv_cache1 = gen.new_kv_cache() if B == 1 else gen.new_kv_cache(batch=B)       # hold the addresses)
        pipe.crossattn_cache = gen.new_crossattn_cache() if B == 1 else gen.new_crossattn_cache(B)
        installed = pipe.kv_cache1
    else:
        installed = pipe._caches[B][0]
    installed.k_all.copy_(inp["fill"][0])
    installed.v_all.copy_(inp["fill"][1])
    pipe.use_graphs = use_graphs
    if rng_seed is None:
        pipe.renoise_override, pipe.noise_generator = inp["draws"], None
    else:
        pipe.renoise_override, pipe.noise_generator = None, torch.Generator(device=DEV).manual_seed(rng_seed)
    _, lat = pipe.inference(inp["noise"].clone(), inp["prompts"], initial_latent=None if inp["init"] is None else inp["init"].clone(),
                            return_latents=True)
    torch.cuda.synchronize()
    kv = pipe.kv_cache1
    assert kv is installed
    S = gen.engine.S
    ends = [(int(b["global_end_index"][0]), int(b["local_end_index"][0])) for b in kv]
    return dict(lat=lat.clone(), k=kv.k_all.clone(), v=kv.v_all.clone(), ends=ends, S=S)


def _chain(rig, pipe, inp, wiring=None):
    ch, ops = rig.chain(pipe, wiring)
    n_init = 0 if inp["init"] is None else inp["init"].shape[1]
    plan = ch.plan(inp["noise"].shape[1], n_init, inp["B"])
    lat, k, v, ends = ch.run(inp["noise"].clone(), inp["contexts"], [d.clone() for d in inp["draws"]],
                             None if inp["init"] is None else inp["init"].clone(), kv=(inp["fill"][0], inp["fill"][1]))
    distinct = len({c.data_ptr() for c in inp["contexts"]})
    assert len(ops.calls) == distinct + sum(1 for r in plan if r[0] != "ends")          # one call per record
    assert ops.canaries_intact()
    return dict(lat=lat, k=k, v=v, ends=ends)


def _same(lib, ch, what=""):
    for name in ("lat", "k", "v"):
        nd = n_diff(lib[name], ch[name])
        assert nd == 0, f"{what}: {nd} of {ch[name].numel()} elements of {name} differ from the chain's"
    ge, le = ch["ends"]
    assert lib["ends"] == [(ge * lib["S"], le * lib["S"])] * len(lib["ends"]), (what, lib["ends"], ch["ends"])
    assert not torch.isnan(lib["lat"].float()).any() and bool((lib["lat"] != 0).any())


def _case(rig, pipe, prompts, T, n_init=0, seed=1000, use_graphs=True, rng_seed=None, what=""):
    inp = _inputs(rig, pipe, prompts, T, n_init, seed, rng_seed)
    lib = _library(pipe, inp, use_graphs, rng_seed)
    ch = _chain(rig, pipe, inp)
    _same(lib, ch, what)
    return inp, lib, ch


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_plain_9_frames(rig, use_graphs):
    inp, lib, _ = _case(rig, rig.pipe(), ["p0"], 9, seed=1000, use_graphs=use_graphs, what="plain")
    S = lib["S"]
    assert n_diff(lib["k"][:, 9 * S:], inp["fill"][0][:, 9 * S:]) == 0               # slots nobody wrote keep their fill
    assert n_diff(lib["k"][:, :9 * S], inp["fill"][0][:, :9 * S]) > 0


def test_independent_first_frame(rig):
    _case(rig, rig.pipe(independent_first_frame=True), ["p1"], 7, seed=1100, what="1 + 3 + 3")


def test_context_noise_100(rig):
    _case(rig, rig.pipe(context_noise=100), ["p0"], 9, seed=1200, what="context_noise 100")


def test_initial_latent(rig):
    inp, lib, _ = _case(rig, rig.pipe(), ["p2"], 6, n_init=3, seed=1300, what="initial 3 + 6")
    assert n_diff(lib["lat"][:, :3], inp["init"]) == 0


def test_independent_first_frame_with_initial_latent(rig):
    _case(rig, rig.pipe(independent_first_frame=True), ["p0"], 3, n_init=4, seed=1400, what="initial 1 + 3, then 3")


@pytest.mark.parametrize("window,sink", [(8, 2), (6, 0)], ids=["window-8-sink-2", "window-6-sink-0"])
def test_rolling_18_frames(rig, window, sink):
    """(8, 2): block 2 straddles the window and its write slots wrap; (6, 0): past one full revolution of the ring.  The blocks past
    the window are the pipeline's position-free ones: relative frame ids on the frame_base scalar, x0 through a static buffer."""
    pipe = rig.pipe(window, sink, rolling_kv=True)
    _case(rig, pipe, ["p0"], 18, seed=1500 + window, what=f"rolling {window}/{sink}")
    assert pipe._frame_base is not None and pipe._roll_bufs


@pytest.mark.parametrize("prompts", [["p0", "p1"], ["p2", "p2"]], ids=["two-prompts", "shared-prompt"])
def test_batch_2(rig, prompts):
    _case(rig, rig.pipe(), prompts, 6, seed=1600 + len(set(prompts)), what="batch 2")


def test_batch_2_rolling(rig):
    _case(rig, rig.pipe(6, 1, rolling_kv=True), ["p1", "p3"], 12, seed=1700, what="batch 2 rolling 6/1")


@pytest.mark.parametrize("which", ["plain", "rolling"])
def test_replay_with_other_inputs(rig, which):
    """A second inference() on a pipeline whose graphs exist, with other noise, another prompt and other draws: the static buffers of
    the replayed graphs hold THIS call's data, and nothing is captured again."""
    pipe, T = (rig.pipe(), 9) if which == "plain" else (rig.pipe(8, 2, rolling_kv=True), 18)
    _case(rig, pipe, ["p0"], T, seed=1800, what=which + ", first call")
    before = pipe.graph_captures
    assert before > 0
    _case(rig, pipe, ["p3"], T, seed=1900, what=which + ", replay")
    assert pipe.graph_captures == before


@pytest.mark.parametrize("prompts", [["p0"], ["p0", "p1"]], ids=["one-sample", "batch-2"])
def test_draws_of_a_seeded_device_generator(rig, prompts):
    """renoise_override None: the pipeline draws from `noise_generator`; the chain is handed what a same-seed generator gives as
    [F, 16, h, w] ([B, F, 16, h, w]) per non-final step, in block order."""
    _case(rig, rig.pipe(), prompts, 6, seed=2000, rng_seed=4321, what="generator draws")


@pytest.mark.parametrize("frames", [5, 21])
@pytest.mark.parametrize("steps", [(1000, 750, 500), (1000, 750, 500, 250, 0)], ids=["3-steps", "ending-in-0"])
def test_bidirectional(rig, frames, steps):
    from mmpl_amd.synthetic import philox_normal
    pipe = rig.bidir(steps)
    ops = PC.HipOps(rig.lib, pipe.generator.engine, DEV)
    ch = PC.BidirFewstepChain(rig.cfg, LAT, ops, step_list=list(steps), warp=True, shift=SHIFT)
    n_fwd = len(ch.plan(frames)) // 2
    assert n_fwd == len([s for s in steps if s]) - 1
    for call, prompt in enumerate(["p0", "p3"]):                        # the second call replays the first one's graph
        noise = philox_normal([1, frames, *FRAME], 2100 + frames + call).to(DEV)
        draws = [philox_normal([frames, *FRAME], 2200 + 10 * call + k).to(DEV) for k in range(n_fwd)]
        pipe.renoise_override = draws
        _, lat = pipe.inference(noise.clone(), [prompt], return_latents=True)
        torch.cuda.synchronize()
        want = ch.run(noise.clone(), rig.table[prompt], [d.clone() for d in draws])
        nd = n_diff(lat, want)
        assert nd == 0, f"bidirectional, {frames} frames, call {call}: {nd} of {want.numel()} elements differ from the chain's"
        assert not torch.isnan(lat.float()).any() and bool((lat != 0).any())
    assert ops.calls.count("mmpl_dit_forward_full") == 2 * n_fwd and ops.canaries_intact()


# ------------------------------------------------------------------------------------------------ power on the device
def test_mutants_differ_on_the_device(rig):
    """What makes the equalities above meaningful: a chain with one wiring decision altered does NOT reproduce the pipeline."""
    pipe = rig.pipe(context_noise=100)
    inp = _inputs(rig, pipe, ["p0"], 6, 0, 2300)
    lib = _library(pipe, inp)
    _same(lib, _chain(rig, pipe, inp), "unmutated")
    bad = _chain(rig, pipe, inp, dict(sigma_next_step=lambda i: i))
    assert n_diff(lib["lat"], bad["lat"]) > 0
    bad = _chain(rig, pipe, inp, dict(refresh=False))                   # the cache bits count: the refresh is what they hold
    print("refresh omitted: latent elements that differ", n_diff(lib["lat"], bad["lat"]), "K elements", n_diff(lib["k"], bad["k"]))
    assert n_diff(lib["k"], bad["k"]) > 0 and n_diff(lib["v"], bad["v"]) > 0
    pipe = rig.pipe(8, 2, rolling_kv=True)
    inp = _inputs(rig, pipe, ["p0"], 12, 0, 2400)
    lib = _library(pipe, inp)
    _same(lib, _chain(rig, pipe, inp), "unmutated rolling")
    bad = _chain(rig, pipe, inp, dict(ring_protect=lambda sink: 0))
    assert n_diff(lib["lat"], bad["lat"]) > 0
