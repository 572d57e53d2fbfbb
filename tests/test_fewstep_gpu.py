"""Few-step (Self-Forcing / CausVid) inference on the MI355X: mmpl_fewstep_update bit for bit against PyTorch's CPU evaluation of
the reference's expressions, WanDiffusionWrapper's block forward and the full CausalInferencePipeline against the oracle and the
reference's fixtures (tests/golden/make_golden_fewstep.py), graph == eager, graph lifetime, the re-noise draws, and one 1.3B / 480p
block at full depth against the oracle evaluated on the device."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fewstep_ref import block as ref_block, ref_add_noise, ref_x0  # noqa: E402
from util import GOLDEN, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-2                      # per-forward parity bound of tests/test_dit_forward_gpu.py


def _args(**kw):
    a = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
             independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    a.update(kw)
    return types.SimpleNamespace(**a)


class _Ctx(torch.nn.Module):
    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _pipe(cfg_name="tiny", weight_seed=1, lat=(60, 104), ctx=None, n_valid=40, ctx_seed=32, sd=None, **kw):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    cfg = WAN_CONFIGS[cfg_name]
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=Geometry(*lat), device=DEV)
    sd = dit_state_dict(cfg, seed=weight_seed) if sd is None else sd
    gen.load_state_dict(sd)
    if ctx is None:
        ctx = philox_normal([1, 512, cfg["text_dim"]], ctx_seed)
        ctx[:, n_valid:] = 0
    return CausalInferencePipeline(_args(**kw), DEV, generator=gen, text_encoder=_Ctx(ctx.to(DEV)), vae=_NoVAE()), sd, cfg, ctx


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n", [8, 4096 * 3 + 5, 1, 77])
@pytest.mark.parametrize("sigma_t", [0.0, 1.0, 0.8333333333333334, 0.0625])
def test_fewstep_update_bit_identical(n, sigma_t):
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    g = torch.Generator().manual_seed(n * 7 + int(sigma_t * 1000))
    flow = (torch.randn(n, generator=g) * torch.logspace(-30, 30, n).to(torch.float32)[torch.randperm(n, generator=g)]).bfloat16()
    x = (torch.randn(n, generator=g) * 3).bfloat16()
    x[: n // 4] = (torch.randn(n // 4, generator=g) * 1e-30).bfloat16()           # tiny magnitudes
    noise = torch.randn(n, generator=g).bfloat16()
    sig_next = 0.640625
    exp_x0 = ref_x0(flow.view(1, -1), x.view(1, -1), sigma_t).view(-1)
    exp_x = ref_add_noise(exp_x0.view(1, -1), noise.view(1, -1), sig_next).view(-1)
    # x0 written at an offset into a bigger buffer (odd element offset: the unaligned path), with and without noise
    for off in (0, 3, 8):
        big = torch.zeros(n + 16, dtype=torch.bfloat16, device=DEV)
        xd = x.to(DEV)
        WanDiffusionWrapper.fewstep_update(flow.to(DEV), xd, noise.to(DEV), big[off:off + n], sigma_t, sig_next)
        torch.cuda.synchronize()
        assert torch.equal(big[off:off + n].cpu().view(torch.int16), exp_x0.view(torch.int16)), off
        assert torch.equal(xd.cpu().view(torch.int16), exp_x.view(torch.int16)), off
        assert not big[:off].any() and not big[off + n:].any()
        xd = x.to(DEV)
        out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        WanDiffusionWrapper.fewstep_update(flow.to(DEV), xd, None, out, sigma_t)      # noise = NULL: x untouched
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int16), exp_x0.view(torch.int16))
        assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))


def test_wrapper_x0_matches_reference_fixture():
    """_convert_flow_pred_to_x0 as the reference computed it (per-frame timestep lookup included)."""
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(os.path.join(GOLDEN, "fewstep_t2v_tiny.pt"))
    pipe, *_ = _pipe()
    gen = pipe.generator
    flow = philox_normal([4, 16, 8, 8], fx["x0_flow_seed"])
    xt = philox_normal([4, 16, 8, 8], fx["x0_xt_seed"])
    for i, t in enumerate(fx["x0_timesteps"]):
        out = torch.empty(16, 8, 8, dtype=torch.bfloat16, device=DEV)
        gen.fewstep_update(flow[i].to(DEV), xt[i].to(DEV).contiguous(), None, out, gen.sigma_x0(t))
        assert torch.equal(out.cpu(), fx["x0"][i]), i


# ---------------------------------------------------------------------------------------------------------------- forward
def test_block_forward_vs_oracle():
    """WanDiffusionWrapper.forward (reference call shape) on block 2 of a cache holding blocks 0 and 1, vs the oracle."""
    from mmpl_amd.synthetic import philox_normal
    from oracle import wan_dit_ref as W
    pipe, sd, cfg, ctx = _pipe(lat=(16, 24))
    gen = pipe.generator
    kv, cross = gen.new_kv_cache(), gen.new_crossattn_cache()
    assert kv.k_all.shape[1] == 21 * gen.engine.S
    ocfg = W.DitCfg(**cfg)
    okv, ocross = W.new_kv_cache(ocfg, 21, gen.engine.S), [None] * cfg["num_layers"]
    S = gen.engine.S
    for blk, tv in ((0, 0.0), (1, 0.0), (2, 937.5)):
        x = philox_normal([1, 3, 16, 16, 24], 60 + blk)
        t = torch.full([1, 3], tv, dtype=torch.float32)
        flow, x0 = gen(x.to(DEV), {"prompt_embeds": ctx.to(DEV)}, t.to(DEV), kv, cross, current_start=3 * blk * S)
        frames = [3 * blk + i for i in range(3)]
        fo = W.dit_forward(sd, ocfg, x[0].permute(1, 0, 2, 3), t, ctx[0], okv, ocross, frames, frames,
                           list(range(0, frames[-1] + 1))).permute(1, 0, 2, 3)
        e = rel_l2(flow[0], fo)
        assert e < TOL, (blk, e)
        assert torch.equal(x0[0].cpu(), ref_x0(flow[0].cpu(), x[0], gen.sigma_x0(torch.tensor(tv))))
    assert int(kv[0]["global_end_index"][0]) == 9 * S and int(kv[0]["local_end_index"][0]) == 9 * S
    with pytest.raises(ValueError, match="overflow"):
        gen(x.to(DEV), {"prompt_embeds": ctx.to(DEV)}, t.to(DEV), kv, cross, current_start=19 * S)


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _fixture_run(name, use_graphs=True):
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(os.path.join(GOLDEN, name))
    m = fx["meta"]
    pipe, *_ = _pipe(weight_seed=m["weight_seed"], n_valid=m["n_valid"], ctx_seed=m["ctx_seed"],
                     independent_first_frame=m["independent_first_frame"], context_noise=m["context_noise"])
    pipe.use_graphs = use_graphs
    noise = philox_normal([1, m["n_noise"], 16, 60, 104], m["noise_seed"])
    init = philox_normal([1, m["n_init"], 16, 60, 104], m["init_seed"]) if m["n_init"] else None
    draws = [philox_normal([F, 16, 60, 104], m["renoise_seed_base"] + k)
             for k, F in enumerate(f for f in m["schedule"] for _ in range(len(m["denoising_step_list"]) - 1))]
    pipe.renoise_override = [d.to(DEV) for d in draws]
    _, lat = pipe.inference(noise.to(DEV), ["p"], initial_latent=None if init is None else init.to(DEV), return_latents=True)
    return fx, pipe, lat


@pytest.mark.parametrize("name", ["fewstep_t2v_tiny.pt", "fewstep_ext_tiny.pt"])
def test_trajectory_vs_reference(name):
    fx, pipe, lat = _fixture_run(name)
    assert torch.equal(pipe.denoising_step_list, fx["step_list"])
    e = rel_l2(lat[..., ::2, ::2], fx["out_strided"])
    print(f"[fewstep] {name}: rel_l2 vs reference {e:.3e} (K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(lat.float()).all()
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


def test_graph_equals_eager_and_second_call_replays():
    from mmpl_amd.synthetic import philox_normal
    pipe, *_ = _pipe()
    noise = philox_normal([1, 9, 16, 60, 104], 71).to(DEV)
    draws = [philox_normal([3, 16, 60, 104], 80 + k).to(DEV) for k in range(9)]
    outs = {}
    for mode in ("eager", "graph1", "graph2"):
        pipe.use_graphs = mode != "eager"
        pipe.renoise_override = draws
        before = pipe.graph_captures
        _, outs[mode] = pipe.inference(noise, ["p"], return_latents=True)
        if mode == "graph1":
            assert pipe.graph_captures - before == 3             # one per block, captured on first use
        if mode == "graph2":
            assert pipe.graph_captures == before                 # the second call only replays
    assert torch.equal(outs["eager"], outs["graph1"])
    assert torch.equal(outs["graph1"], outs["graph2"])
    pipe.release_graphs()
    assert not pipe._graphs


def test_no_graph_constructed_after_first_call(monkeypatch):
    from mmpl_amd.synthetic import philox_normal
    pipe, *_ = _pipe()
    noise = philox_normal([1, 6, 16, 60, 104], 72).to(DEV)
    torch.manual_seed(5)
    _, a = pipe.inference(noise, ["p"], return_latents=True)
    made = []
    real = torch.cuda.CUDAGraph

    class Counting(real):
        def __new__(cls, *a, **k):
            made.append(1)
            return real(*a, **k)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Counting)
    torch.manual_seed(5)
    _, b = pipe.inference(noise, ["p"], return_latents=True)
    assert not made
    assert torch.equal(a, b)


def test_renoise_draws_match_a_same_seed_generator():
    """The bank holds what torch.randn_like(denoised_pred.flatten(0, 1)) draws in the reference's order (last block's 3)."""
    from mmpl_amd.synthetic import philox_normal
    pipe, *_ = _pipe()
    noise = philox_normal([1, 3, 16, 60, 104], 73).to(DEV)
    torch.cuda.manual_seed(1234)
    pipe.inference(noise, ["p"])
    torch.cuda.synchronize()
    g = torch.Generator(device=DEV).manual_seed(1234)
    like = torch.empty(3, 16, 60, 104, dtype=torch.bfloat16, device=DEV)
    for i in range(3):
        exp = torch.randn(like.shape, dtype=like.dtype, device=DEV, generator=g)
        assert torch.equal(pipe._bufs[3]["bank"][i], exp), i
    torch.cuda.manual_seed(1234)
    assert torch.equal(pipe._bufs[3]["bank"][0], torch.randn_like(like))


# ---------------------------------------------------------------------------------------------------------------- full size
def test_fullsize_1p3b_block_after_two_cached_blocks():
    """Wan 1.3B at 480p, all 30 layers: blocks 0 and 1 cached (refresh forwards), then block 2 denoised in 4 steps, the
    oracle evaluated by PyTorch on the device (grouped SDPA, as tests/test_fullsize_gpu.py)."""
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    from oracle import wan_dit_ref as W
    from test_fullsize_gpu import _grouped_sdpa
    cfg = WAN_CONFIGS["1.3B"]
    g = torch.Generator(device=DEV).manual_seed(91)
    ctx = torch.randn(1, 512, cfg["text_dim"], generator=g, device=DEV).bfloat16()
    ctx[:, 64:] = 0
    sd = dit_state_dict(cfg, seed=92, device=DEV)
    pipe, _, _, _ = _pipe("1.3B", ctx=ctx, sd=sd)
    gen = pipe.generator
    S = gen.engine.S
    lat = torch.randn(1, 6, 16, 60, 104, generator=g, device=DEV).bfloat16()
    noise = torch.randn(3, 16, 60, 104, generator=g, device=DEV).bfloat16()
    draws = [torch.randn(3, 16, 60, 104, generator=g, device=DEV).bfloat16() for _ in range(3)]
    # product: the pipeline with a 6-frame initial latent (two cached blocks) and one denoised block
    pipe.renoise_override = draws
    _, out = pipe.inference(noise.unsqueeze(0), ["p"], initial_latent=lat, return_latents=True)
    # oracle on the device
    ocfg = W.DitCfg(**cfg)
    okv = [{n: t.to(DEV) for n, t in d.items()} for d in W.new_kv_cache(ocfg, 21, S)]
    ocross = [None] * cfg["num_layers"]
    for b in range(2):
        fr = [3 * b + i for i in range(3)]
        W.dit_forward(sd, ocfg, lat[0, 3 * b:3 * b + 3].permute(1, 0, 2, 3), torch.zeros(1, 3, device=DEV), ctx[0], okv, ocross,
                      fr, fr, list(range(0, fr[-1] + 1)), attn_fn=_grouped_sdpa)
    ts, sx, sn = pipe._step_scalars()
    x0 = ref_block(sd, ocfg, okv, ocross, noise, ctx[0], 6, ts, sx, sn, draws, 0.0, 21, attn_fn=_grouped_sdpa)
    torch.cuda.synchronize()
    assert torch.equal(out[0, :6], lat[0])
    e = rel_l2(out[0, 6:], x0)
    print(f"[fewstep] 1.3B/480p block 2 after 2 cached blocks: rel_l2 vs device oracle {e:.3e}")
    assert torch.isfinite(out.float()).all() and e < TOL, e


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_fewstep_synthetic(tmp_path):
    """A config with denoising_step_list runs the few-step pipeline end to end (VAE decode included): 9 latent frames -> 33."""
    from mmpl_amd import cli
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    cli.main(["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--num_output_frames", "9",
              "--config_path", str(cfg), "--output_folder", str(tmp_path)])
    v = torch.load(tmp_path / "0-0.pt")
    assert tuple(v.shape) == (33, 128, 192, 3) and v.dtype == torch.uint8
