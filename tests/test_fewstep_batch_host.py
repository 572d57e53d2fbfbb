"""Host logic of batched few-step generation (no GPU): the grouped slot arithmetic against the list simulation of
tests/fewstep_rolling_ref.py, the re-noise bank's layout and draw order against tests/fewstep_ref.py's expressions on a generator that
launches nothing, the CLI's refusals and its slicing of --num_samples into calls, and the batched caches' views."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fewstep_ref import ref_add_noise, ref_x0  # noqa: E402
from fewstep_rolling_ref import schedule_slots  # noqa: E402

LAT = (4, 6)


class _KV(list):
    def __init__(self, n_slots, S, batch):
        super().__init__([{"global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])}])
        self.engine = types.SimpleNamespace(S=S)
        self.n_slots, self.batch = n_slots, batch
        self.k_all = torch.zeros(1, batch * n_slots * S, 8)


class _Cross(list):
    shared = False

    def fill(self, pe, shared=False):
        self.shared = shared


class _Gen:
    """A generator that launches nothing: `flow` is a fixed elementwise function of (x, t) and records its slots; `fewstep_update`
    is tests/fewstep_ref.py's two expressions."""

    def __init__(self, window, sink=0, max_frames=8):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper
        self.geometry = Geometry(*LAT)
        self.engine = types.SimpleNamespace(L=1, max_frames=max_frames, S=self.geometry.frame_seqlen)
        self.model = types.SimpleNamespace(local_attn_size=window, sink_size=sink, num_frame_per_block=1)
        self.window_frames = window
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.calls = []
        self.slots = types.MethodType(WanDiffusionWrapper.slots, self)
        self.set_cache_ends = WanDiffusionWrapper.set_cache_ends
        self.sigma_x0 = types.MethodType(WanDiffusionWrapper.sigma_x0, self)
        self.sigma_add_noise = types.MethodType(WanDiffusionWrapper.sigma_add_noise, self)
        self._sig64, self._ts64 = self.scheduler.sigmas.double(), self.scheduler.timesteps.double()

    def get_scheduler(self):
        return self.scheduler

    def new_kv_cache(self, batch=1):
        return _KV(self.window_frames, self.engine.S, batch)

    def new_crossattn_cache(self, batch=1):
        return _Cross()

    @staticmethod
    def flow_of(x, t):
        return (x.float() * 0.25 + t.view(-1, 1, 1, 1) / 1000.0).to(torch.bfloat16)

    def flow(self, x, t, start, write, vis, kv, cross, out=None, frame_base=None):
        self.calls.append((start, None if frame_base is None else int(frame_base), list(write), [list(v) for v in vis] if kv.batch > 1 else list(vis)))
        f = self.flow_of(x, t)
        return f if out is None else out.copy_(f)

    @staticmethod
    def fewstep_update(flow, x, noise, x0_out, sigma_t, sigma_next=0.0):
        x0 = ref_x0(flow, x, sigma_t)
        x0_out.copy_(x0)
        if noise is not None:
            x.copy_(ref_add_noise(x0, noise.reshape(x0.shape), sigma_next))


def _pipe(window=21, sink=0, rolling=False, F=3, max_frames=8):
    from mmpl_amd.pipeline import CausalInferencePipeline
    a = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=F,
                              independent_first_frame=False, context_noise=0, rolling_kv=rolling)
    gen = _Gen(window, sink, max_frames)
    pipe = CausalInferencePipeline(a, "cpu", generator=gen, vae=object(),
                                   text_encoder=lambda text_prompts: {"prompt_embeds": torch.zeros(len(text_prompts), 4, 4)})
    pipe.use_graphs = False
    return pipe, gen


# ---------------------------------------------------------------------------------------------------------------- slots
@pytest.mark.parametrize("W,sink", [(6, 0), (6, 1), (8, 2)])
@pytest.mark.parametrize("G", [2, 3])
def test_grouped_rolling_slots_are_the_simulation_plus_g_windows(G, W, sink):
    """every sample is a rolling cache of its own in slots g * W .. of the one allocation"""
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    gen = _Gen(W, sink)
    kv = gen.new_kv_cache(batch=G)
    for start, n, write, vis, _ in schedule_slots(W, sink, [2] * 7):
        w, v, le = WanDiffusionWrapper.slots(gen, kv, start, n, rolling=True, batch=G)
        assert w == [s + g * W for g in range(G) for s in write]
        assert v == [[s + g * W for s in vis] for g in range(G)]
        assert le == min(start + n, W)
        assert len(set(w)) == len(w) and all(g * W <= s < (g + 1) * W for g in range(G) for s in v[g] + w[g * n:(g + 1) * n])


def test_grouped_causal_slots_and_batch_mismatch():
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper, causal_slots
    gen = _Gen(21)
    kv = gen.new_kv_cache(batch=2)
    le = 0
    for start in (0, 3, 6):
        write, vis, le1 = causal_slots(start, 3, 21, 21, le, start)
        w, v, le2 = WanDiffusionWrapper.slots(gen, kv, start, 3, batch=2)
        assert (w, v, le2) == (write + [s + 21 for s in write], [vis, [s + 21 for s in vis]], le1)
        WanDiffusionWrapper.set_cache_ends(kv, start + 3, le2)
        le = le1
    with pytest.raises(ValueError, match="batch 1 against a KV cache for 2"):
        WanDiffusionWrapper.slots(gen, kv, 9, 3)
    one = gen.new_kv_cache()
    assert WanDiffusionWrapper.slots(gen, one, 0, 3) == causal_slots(0, 3, 21, 21, 0, 0)        # batch 1: the plain lists


# ---------------------------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("rolling", [False, True])
def test_bank_layout_and_draw_order(rolling):
    """B = 2, two blocks of 3: per non-final step ONE draw of [B, F, 16, h, w] from the generator (the reference's order), sample b's
    noise being its slice [b]; each sample's trajectory is tests/fewstep_ref.py's block on that slice."""
    B, F, T = 2, 3, 6 if not rolling else 9
    pipe, gen = _pipe(window=21 if not rolling else 6, sink=1 if rolling else 0, rolling=rolling)
    pipe.noise_generator = torch.Generator().manual_seed(7)
    g0 = torch.Generator().manual_seed(3)
    noise = torch.randn(B, T, 16, *LAT, generator=g0).to(torch.bfloat16)
    with torch.no_grad():
        steps = list(pipe._blocks(noise, ["a", "b"]))
    out = steps[-1][2]
    assert out.shape == (B, T, 16, *LAT) and [s[:2] for s in steps] == [(0, 0)] + [(s, F) for s in range(0, T, F)]
    assert pipe._bufs[(F, B)]["bank"].shape == (3, B, F, 16, *LAT) and pipe._bufs[(F, B)]["x"].shape == (B * F, 16, *LAT)
    t_eng, sig_x0, sig_next = pipe._step_scalars()
    g = torch.Generator().manual_seed(7)
    for s in range(0, T, F):
        draws = [torch.empty(B, F, 16, *LAT, dtype=torch.bfloat16).normal_(0.0, 1.0, generator=g) for _ in range(3)]
        for b in range(B):
            x = noise[b, s:s + F].clone()
            for i in range(4):
                x0 = ref_x0(gen.flow_of(x, torch.full([F], t_eng[i])), x, sig_x0[i])
                if i < 3:
                    x = ref_add_noise(x0, draws[i][b], sig_next[i])
            assert torch.equal(out[b, s:s + F], x0), (s, b)
    # every forward of a block ran on both samples' slots at once: 4 steps + the refresh, B * F write slots, one visible list per sample
    assert len(gen.calls) == 5 * (T // F) and all(len(c[2]) == B * F and len(c[3]) == B for c in gen.calls)
    assert pipe.kv_cache1.batch == B and int(pipe.kv_cache1[0]["global_end_index"][0]) == T * gen.engine.S
    keys = list(pipe._roll_bufs)
    assert all(k[-2:] == (B, False) for k in keys) and len(keys) == T // F     # a batch's x0 goes through a static block buffer


def test_equal_prompts_share_the_context_and_batch_1_keeps_its_keys():
    pipe, gen = _pipe()
    noise = torch.zeros(2, 3, 16, *LAT, dtype=torch.bfloat16)
    with torch.no_grad():
        list(pipe._blocks(noise, ["p", "p"]))
        assert pipe.crossattn_cache.shared and list(pipe._roll_bufs)[0][-2:] == (2, True)
        list(pipe._blocks(noise, ["p", "q"]))
        assert not pipe.crossattn_cache.shared
        two = pipe.kv_cache1
        list(pipe._blocks(noise[:1], ["p"]))
    assert pipe.kv_cache1 is not two and pipe.kv_cache1.batch == 1 and pipe._caches[2][0] is two
    assert set(pipe._bufs) == {(3, 2), 3} and set(pipe._out) == {(3, 2), 3}      # batch 1: the integer keys it always had
    assert len(pipe._roll_bufs) == 2                                             # ... and no static x0 buffer


def test_limits_are_named():
    pipe, gen = _pipe(max_frames=7)
    with pytest.raises(ValueError, match=r"3 x num_frame_per_block 3 = 9 frames per forward exceeds the engine's limit of 7"), torch.no_grad():
        next(pipe._blocks(torch.zeros(3, 3, 16, *LAT), ["a", "b", "c"]))
    with pytest.raises(ValueError, match="1 prompts for a noise batch of 2"), torch.no_grad():
        next(pipe._blocks(torch.zeros(2, 3, 16, *LAT), ["a"]))
    with pytest.raises(ValueError, match="initial_latent holds 1 samples"), torch.no_grad():
        next(pipe._blocks(torch.zeros(2, 3, 16, *LAT), ["a", "b"], initial_latent=torch.zeros(1, 3, 16, *LAT)))
    with pytest.raises(ValueError, match="inference_stream keeps batch size 1"):
        next(pipe.inference_stream(torch.zeros(2, 3, 16, *LAT), ["a", "b"]))
    assert not gen.calls


def test_initial_latent_at_batch_2_fills_every_samples_cache():
    pipe, gen = _pipe()
    init = torch.arange(2 * 3, dtype=torch.float32).view(2, 3, 1, 1, 1).expand(2, 3, 16, *LAT).to(torch.bfloat16)
    with torch.no_grad():
        steps = list(pipe._blocks(torch.zeros(2, 3, 16, *LAT, dtype=torch.bfloat16), ["a", "b"], initial_latent=init))
    assert steps[0][:2] == (0, 3) and torch.equal(steps[-1][2][:, :3], init)
    assert gen.calls[0] == (0, None, [0, 1, 2, 21, 22, 23], [[0, 1, 2], [21, 22, 23]])             # the context forward
    assert gen.calls[1][2:] == ([3, 4, 5, 24, 25, 26], [list(range(6)), list(range(21, 27))])


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli_args(**kw):
    a = dict(num_samples=2, bidirectional=False, stream=False, extend=None, extend_context=None, num_frame_per_block=3, preview_vae=None,
             rolling=False, sample_solver="unipc", fp32_latents=False, duration=1, i2v=False, i2v_model=False, num_output_frames=21)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_cli_refusals():
    from mmpl_amd import cli
    assert cli.samples_refusal(_cli_args(), True) is None and cli.first_refusal(_cli_args(), 1, True) is None
    assert cli.samples_refusal(_cli_args(num_samples=1, stream=True), True) is None                 # not asked for
    assert "few-step config" in cli.samples_refusal(_cli_args(), False)                              # the 50-step pipeline
    assert "few-step config" in cli.first_refusal(_cli_args(), 1, False)
    assert "--bidirectional" in cli.samples_refusal(_cli_args(bidirectional=True), True)
    assert "--stream" in cli.samples_refusal(_cli_args(stream=True), True)
    assert "--extend" in cli.samples_refusal(_cli_args(extend="x.pt", stream=False), True)
    assert "at least 1" in cli.samples_refusal(_cli_args(num_samples=0), True)
    assert "largest forward" in cli.samples_refusal(_cli_args(num_frame_per_block=9), True)


def test_cli_slices_the_samples_into_calls():
    from mmpl_amd import cli
    assert cli.sample_groups(2, 3) == [(0, 2)]                     # 8 // 3 = 2 samples per call
    assert cli.sample_groups(5, 3) == [(0, 2), (2, 4), (4, 5)]
    assert cli.sample_groups(8, 1) == [(0, 8)] and cli.sample_groups(9, 1) == [(0, 8), (8, 9)]
    assert cli.sample_groups(3, 7) == [(0, 1), (1, 2), (2, 3)]
    assert cli.sample_groups(4, 3, max_frames=7) == [(0, 2), (2, 4)]
    for n, f in ((5, 3), (9, 1), (17, 2)):
        gs = cli.sample_groups(n, f)
        assert [lo for lo, _ in gs] == [0] + [hi for _, hi in gs[:-1]] and gs[-1][1] == n and all((hi - lo) * f <= 8 for lo, hi in gs)


# ---------------------------------------------------------------------------------------------------------------- caches
class _Engine:
    L, S, dim, text_len, device = 2, 6, 256, 8, torch.device("cpu")
    cfg = {"num_heads": 2}

    def new_kv_cache(self, n_slots):
        shape = (self.L, n_slots * self.S, self.dim)
        return torch.zeros(shape, dtype=torch.bfloat16), torch.zeros(shape, dtype=torch.bfloat16)

    def precompute_context(self, ctx, out):
        out[0].fill_(float(ctx[0, 0]))
        out[1].fill_(-float(ctx[0, 0]))
        return types.SimpleNamespace(rows=int(ctx[0, 1]))


def test_kv_cache_views_alias_the_one_allocation():
    from mmpl_amd.wan_wrapper import KVCache
    e = _Engine()
    kv = KVCache(e, 5, batch=3)
    assert kv.k_all.shape == (2, 3 * 5 * 6, 256) and (kv.n_slots, kv.batch) == (5, 3) and len(kv) == 2
    assert kv[1]["k"].shape == (3, 5 * 6, 2, 128) and kv[1]["v"].shape == (3, 5 * 6, 2, 128)      # the reference's [B, W * S, H, 128]
    kv[1]["k"][2, 7, 1, 5] = 3.0                           # sample 2, token 7 of its window = slot 2 * 5 + 1, row 1
    assert float(kv.k_all[1, (2 * 5 + 1) * 6 + 1, 128 + 5]) == 3.0 and int((kv.k_all != 0).sum()) == 1
    one = KVCache(e, 5)
    assert one.batch == 1 and one[0]["k"].shape == (1, 5 * 6, 2, 128) and one.k_all.shape == (2, 30, 256)


def test_cross_attn_cache_per_sample_or_shared():
    from mmpl_amd.wan_wrapper import CrossAttnCache
    e = _Engine()
    c = CrossAttnCache(e, batch=2)
    assert c[0]["k"].shape == (2, 8, 2, 128) and c.k_all.data_ptr() == c.k_b[0].data_ptr() and not c.is_init
    pe = torch.tensor([[[1.0, 4.0]], [[2.0, 6.0]]])
    c.fill(pe)
    assert c.is_init and not c.shared and c.rows == 6 and float(c.k_b[1, 1, 0, 0]) == 2.0 and float(c[1]["v"][1, 3, 1, 7]) == -2.0
    k0, k1 = c.pairs()
    assert k0[0].data_ptr() != k1[0].data_ptr() and k1[0].data_ptr() == c.k_b[1].data_ptr()
    c.fill(pe, shared=True)
    assert c.shared and c.rows == 4 and all(p[0].data_ptr() == c.k_b[0].data_ptr() and p[1].data_ptr() == c.v_b[0].data_ptr() for p in c.pairs())
    with pytest.raises(ValueError, match="1 prompts for a batch of 2"):
        c.fill(pe[:1])
    one = CrossAttnCache(e)
    one.fill(pe[:1])
    assert one.shared and one[0]["k"].shape == (1, 8, 2, 128) and one.k_all.shape == (2, 8, 256) and one.rows == 4
