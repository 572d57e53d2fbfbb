"""Batched few-step inference (-m gpu): CausalInferencePipeline.inference on noise [B, T, 16, h, w] with one prompt per sample -- the
samples of a call run as ONE forward of B x num_frame_per_block frames per step (DitEngine.forward_groups, grouped self-attention).

Against the REAL reference at batch 2 (tests/golden/make_golden_fewstep_batch.py: two contexts, one re-noise draw [2, 3, 16, h, w] per
non-final step) under the project's standing rule -- rel-L2 <= 2 x the reference's own K / V summation-order noise, measured by the
reference and stored in the fixture --; eager == hipGraph; no graph constructed on a second call; a B = 1 call on the same object
equals a fresh pipeline's; equal prompts take the single text cross-attention launch and compute what the per-sample launches do;
initial_latent and the rolling KV window at B = 2; the frame limit."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import GOLDEN, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (60, 104)


def _args(**kw):
    a = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
             independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    a.update(kw)
    return types.SimpleNamespace(**a)


class _Ctx(torch.nn.Module):
    """prompt i -> row i of the contexts (a batch of one prompt: row 0)"""

    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx[:len(text_prompts)]}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _contexts(seeds=(52, 53), n_valid=(40, 17)):
    from mmpl_amd.synthetic import WAN_CONFIGS, philox_normal
    out = []
    for s, n in zip(seeds, n_valid):
        c = philox_normal([1, 512, WAN_CONFIGS["tiny"]["text_dim"]], s)
        c[:, n:] = 0
        out.append(c)
    return torch.cat(out)


def _pipe(weight_seed=51, ctx=None, lat=LAT, local_attn_size=-1, sink_size=0, **kw):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    cfg = WAN_CONFIGS["tiny"]
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, local_attn_size=local_attn_size, sink_size=sink_size, model_config=cfg,
                              geometry=Geometry(*lat), device=DEV)
    gen.load_state_dict(dit_state_dict(cfg, seed=weight_seed))
    ctx = _contexts() if ctx is None else ctx
    return CausalInferencePipeline(_args(**kw), DEV, generator=gen, text_encoder=_Ctx(ctx.to(DEV)), vae=_NoVAE())


def _inputs(B, T, lat=LAT, seed=54, n_blocks=None, renoise=600):
    from mmpl_amd.synthetic import philox_normal
    noise = philox_normal([B, T, 16, *lat], seed).to(DEV)
    draws = [philox_normal([B, 3, 16, *lat], renoise + k).to(DEV) for k in range(3 * (T // 3 if n_blocks is None else n_blocks))]
    return noise, draws


def _run(pipe, noise, draws, prompts, **kw):
    pipe.renoise_override = draws
    _, lat = pipe.inference(noise, prompts, return_latents=True, **kw)
    return lat


@pytest.fixture(scope="module")
def batch2():
    """One pipeline, the fixture's inputs, its eager run and its first and second graph run (shared by the tests below)."""
    fx = torch.load(os.path.join(GOLDEN, "fewstep_batch_tiny.pt"))
    m = fx["meta"]
    assert m["batch"] == 2 and m["n_valid"] == (40, 17) and m["schedule"] == [3, 3]
    pipe = _pipe(weight_seed=m["weight_seed"], ctx=_contexts(m["ctx_seeds"], m["n_valid"]))
    noise, draws = _inputs(2, m["n_noise"], seed=m["noise_seed"], renoise=m["renoise_seed_base"])
    runs = {}
    for mode in ("eager", "graph1", "graph2"):
        pipe.use_graphs = mode != "eager"
        before = pipe.graph_captures
        runs[mode] = _run(pipe, noise, draws, ["p0", "p1"]).clone()
        runs[mode + "_captures"] = pipe.graph_captures - before
    return fx, pipe, noise, draws, runs


def test_trajectory_vs_the_reference_at_batch_2(batch2):
    fx, pipe, _, _, runs = batch2
    lat = runs["graph1"]
    assert torch.equal(pipe.denoising_step_list, fx["step_list"]) and lat.shape == (2, 6, 16, 60, 104)
    e = rel_l2(lat[..., ::2, ::2], fx["out_strided"])
    each = [rel_l2(lat[b][..., ::2, ::2], fx["out_strided"][b]) for b in range(2)]
    print(f"[fewstep batch] rel_l2 vs the reference at batch 2: {e:.3e} (per sample {each[0]:.3e}, {each[1]:.3e}; K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(lat.float()).all()
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])
    assert max(each) <= 2.0 * fx["order_out"], each


def test_graph_equals_eager_and_second_call_replays(batch2):
    _, _, _, _, runs = batch2
    assert runs["graph1_captures"] == 2 and runs["graph2_captures"] == 0          # one per block, then replays only
    assert torch.equal(runs["eager"], runs["graph1"]) and torch.equal(runs["graph1"], runs["graph2"])


def test_no_graph_constructed_on_a_later_call(batch2, monkeypatch):
    _, pipe, noise, draws, runs = batch2
    made = []
    real = torch.cuda.CUDAGraph

    class Counting(real):
        def __new__(cls, *a, **k):
            made.append(1)
            return real(*a, **k)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Counting)
    pipe.use_graphs = True
    assert torch.equal(_run(pipe, noise, draws, ["p0", "p1"]), runs["graph1"]) and not made


def test_batch_1_on_the_same_object_equals_a_fresh_pipeline(batch2):
    fx, pipe, noise, draws, _ = batch2
    m = fx["meta"]
    one = [d[:1].contiguous() for d in draws]
    pipe.use_graphs = True
    a = _run(pipe, noise[:1], one, ["p0"]).clone()
    fresh = _pipe(weight_seed=m["weight_seed"], ctx=_contexts(m["ctx_seeds"], m["n_valid"]))
    b = _run(fresh, noise[:1], one, ["p0"])
    assert a.shape == (1, 6, 16, 60, 104) and torch.equal(a, b)
    assert set(fresh._graphs) == {k for k in pipe._graphs if len(k) == 7}          # the batch-1 keys are the ones it always had
    # ... and it is sample 0 of the batch up to what the launchers choose from the row count
    e = rel_l2(a[0], batch2[4]["graph1"][0])
    print(f"[fewstep batch] sample 0 of the batch vs the same sample alone: rel_l2 {e:.3e}")
    assert e <= 2.0 * fx["order_out"]


def _cross_launches(pipe, noise, draws, prompts):
    from mmpl_amd import _lib
    lib = _lib.load()
    pipe.use_graphs = False
    n = 8
    ms, fl, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)()
    lib.mmpl_profile_enable((1 << 2) << 1)                 # kind 2: the text cross-attention
    try:
        lat = _run(pipe, noise, draws, prompts).clone()
        lib.mmpl_profile_read(n, ms, fl, cnt)
    finally:
        lib.mmpl_profile_enable(0)
    return lat, cnt[2]


def test_equal_prompts_take_one_cross_attention_launch():
    """Both samples on context 0.  Prompts that are equal strings share sample 0's text K / V: one cross-attention launch per layer
    and forward.  Different strings (here with the same embedding) take one launch per sample.  Same numbers, bit for bit."""
    ctx = _contexts()
    pipe = _pipe(ctx=torch.cat([ctx[:1], ctx[:1]]))
    noise, draws = _inputs(2, 3, seed=91, renoise=700)
    forwards, layers = 5, pipe.generator.engine.L          # 4 steps + the cache refresh
    shared, n_shared = _cross_launches(pipe, noise, draws, ["p", "p"])
    assert pipe.crossattn_cache.shared
    apart, n_apart = _cross_launches(pipe, noise, draws, ["p", "q"])
    assert not pipe.crossattn_cache.shared
    print(f"[fewstep batch] cross-attention launches of one block: {n_shared} shared, {n_apart} per sample")
    assert n_shared == forwards * layers and n_apart == 2 * forwards * layers
    assert torch.equal(shared, apart)


def test_initial_latent_at_batch_2():
    """3 context frames per sample + 1 block.  Sample b equals the batch-1 run on its own slices of the noise, the context frames and the
    re-noise draws, bit for bit: at these shapes (2 x 3 frames of 96 tokens) the launchers choose the same kernels at 576 and at 288
    rows, which tests/test_dit_forward_groups_gpu.py (c) establishes from their plans."""
    from mmpl_amd.synthetic import philox_normal
    pipe = _pipe(lat=(16, 24))
    noise, draws = _inputs(2, 3, lat=(16, 24), seed=92, renoise=710)
    init = philox_normal([2, 3, 16, 16, 24], 93).to(DEV)
    both = _run(pipe, noise, draws, ["p0", "p1"], initial_latent=init).clone()
    assert both.shape == (2, 6, 16, 16, 24) and torch.equal(both[:, :3], init)
    for b in range(2):
        solo = _pipe(lat=(16, 24), ctx=_contexts()[b:b + 1])
        one = _run(solo, noise[b:b + 1], [d[b:b + 1].contiguous() for d in draws], ["p"], initial_latent=init[b:b + 1])
        e = rel_l2(both[b], one[0])
        print(f"[fewstep batch] initial_latent, sample {b}: rel_l2 vs batch 1 {e:.3e}")
        assert torch.equal(both[b], one[0])


def test_rolling_window_at_batch_2():
    """window 6, sink 1, 12 frames: blocks 2 and 3 run past the window (ring slots, frame ids relative to the device scalar).  Bit-equal
    to the batch-1 runs, as above."""
    kw = dict(lat=(16, 24), local_attn_size=6, sink_size=1, rolling_kv=True)
    pipe = _pipe(**kw)
    noise, draws = _inputs(2, 12, lat=(16, 24), seed=94, renoise=720)
    both = _run(pipe, noise, draws, ["p0", "p1"]).clone()
    again = _run(pipe, noise, draws, ["p0", "p1"])
    assert torch.equal(both, again) and torch.isfinite(both.float()).all()
    assert pipe.kv_cache1.batch == 2 and pipe.kv_cache1.k_all.shape[1] == 2 * 6 * pipe.generator.engine.S
    for b in range(2):
        solo = _pipe(ctx=_contexts()[b:b + 1], **kw)
        one = _run(solo, noise[b:b + 1], [d[b:b + 1].contiguous() for d in draws], ["p"])
        e = rel_l2(both[b], one[0])
        print(f"[fewstep batch] rolling window, sample {b}: rel_l2 vs batch 1 {e:.3e}")
        assert torch.equal(both[b], one[0])


def test_too_many_frames_per_forward_raises():
    pipe = _pipe(lat=(16, 24), ctx=torch.cat([_contexts(), _contexts()[:1]]))
    noise, _ = _inputs(3, 3, lat=(16, 24))
    with pytest.raises(ValueError, match=r"exceeds the engine's limit of 7 \(max_frames\)"):
        pipe.inference(noise, ["a", "b", "c"])
    with pytest.raises(ValueError, match="batch size 1"):
        next(pipe.inference_stream(noise[:2], ["a", "b"]))
