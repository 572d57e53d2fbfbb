"""GPU tests of the two bidirectional pipelines (-m gpu): BidirectionalDiffusionInferencePipeline (CFG sampling of a whole clip,
both solvers) and BidirectionalInferencePipeline (few-step) against the REAL reference's latents (tests/golden/make_golden_bidir.py),
graph == eager, graph reuse, and the CLI.  Tiny synthetic config, 21 frames at 16 x 24 latents.

Tolerance: rel-L2(HIP, reference) <= 2 x the fixture's `order_out` -- the reference's own change when its self-attention sums the
keys in reverse frame order (the convention of tests/test_fewstep_gpu.py for whole trajectories)."""
import os
import types

import pytest
import torch

from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)


class _Text(torch.nn.Module):
    """prompt -> seeded context; the negative prompt "NEG" -> the other one."""

    def __init__(self, ctx, neg=None):
        super().__init__()
        self.ctx, self.neg = ctx, neg

    def forward(self, text_prompts):
        return {"prompt_embeds": self.neg if text_prompts[0] == "NEG" else self.ctx}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _context(cfg, seed, n_valid):
    from mmpl_amd.synthetic import philox_normal
    c = philox_normal([1, 512, cfg["text_dim"]], seed)
    c[:, n_valid:] = 0
    return c.to(torch.bfloat16).to(DEV)


def _generator(m):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    cfg = WAN_CONFIGS[m["cfg"]]
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=m["timestep_shift"], model_config=cfg, geometry=Geometry(*LAT), device=DEV)
    gen.load_state_dict(dit_state_dict(cfg, seed=m["weight_seed"]))
    assert gen.uniform_timestep is True and gen.model.num_frame_per_block == 1
    return gen, cfg


def _diffusion(tag, **attrs):
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(os.path.join(GOLDEN, f"bidir_diffusion_{tag}_tiny.pt"))
    m = fx["meta"]
    gen, cfg = _generator(m)
    args = types.SimpleNamespace(num_train_timestep=m["num_train_timestep"], guidance_scale=m["guidance_scale"], negative_prompt="NEG",
                                 timestep_shift=3.0)
    text = _Text(_context(cfg, m["ctx_seed"], m["n_valid"]), _context(cfg, m["neg_seed"], m["n_valid_neg"]))
    pipe = BidirectionalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=text, vae=_NoVAE())
    pipe.sampling_steps, pipe.sample_solver = m["sampling_steps"], m["sample_solver"]
    for k, v in attrs.items():
        setattr(pipe, k, v)
    noise = philox_normal([1, m["F"], 16, LAT[0], LAT[1]], m["noise_seed"]).to(torch.bfloat16).to(DEV)
    return fx, pipe, noise


def _fewstep():
    from mmpl_amd.pipeline import BidirectionalInferencePipeline
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(os.path.join(GOLDEN, "bidir_fewstep_tiny.pt"))
    m = fx["meta"]
    gen, cfg = _generator(m)
    args = types.SimpleNamespace(denoising_step_list=m["denoising_step_list"], warp_denoising_step=m["warp_denoising_step"])
    pipe = BidirectionalInferencePipeline(args, DEV, generator=gen, text_encoder=_Text(_context(cfg, m["ctx_seed"], m["n_valid"])),
                                          vae=_NoVAE())
    noise = philox_normal([1, m["F"], 16, LAT[0], LAT[1]], m["noise_seed"]).to(torch.bfloat16).to(DEV)
    draws = [philox_normal([m["F"], 16, LAT[0], LAT[1]], m["renoise_seed_base"] + k).to(torch.bfloat16).to(DEV) for k in range(m["n_draws"])]
    return fx, pipe, noise, draws


@pytest.mark.parametrize("tag", ["unipc", "dpmpp"])
def test_diffusion_trajectory_vs_reference(tag):
    """6 CFG steps of the whole 21-frame clip against the reference's BidirectionalDiffusionInferencePipeline.inference; the eager
    path gives the graph path's bits; a second call constructs no graph and returns the first call's bits; release_graphs()
    then recaptures."""
    fx, pipe, noise = _diffusion(tag)
    _, lat = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 1
    assert [float(t) for t in pipe.timesteps] == [float(t) for t in fx["timesteps"]]
    e = rel_l2(lat[..., ::2, ::2], fx["out_strided"])
    print(f"[bidir] diffusion {tag}: rel_l2 vs reference {e:.3e} (K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(lat.float()).all()
    _, again = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 1                                       # the second call only replays
    assert torch.equal(again, lat)
    pipe.release_graphs()
    _, recaptured = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 2 and torch.equal(recaptured, lat)
    _, pipe_e, _ = _diffusion(tag, use_graphs=False)
    _, eager = pipe_e.inference(noise, ["p"], return_latents=True)
    assert pipe_e.graph_captures == 0 and torch.equal(eager, lat)
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


def test_diffusion_concurrent_branches_give_the_sequential_bits():
    """The two CFG branches as parallel graph branches (second stream, private workspace) or back to back with block 0 shared,
    or back to back without sharing: the same bits."""
    outs = []
    for attrs in (dict(concurrent_cfg=True), dict(concurrent_cfg=False), dict(concurrent_cfg=False, share_block0=False)):
        _, pipe, noise = _diffusion("unipc", **attrs)
        pipe.sampling_steps = 3
        outs.append(pipe.inference(noise, ["p"], return_latents=True)[1])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def test_fewstep_trajectory_vs_reference():
    fx, pipe, noise, draws = _fewstep()
    assert torch.equal(pipe.denoising_step_list, fx["step_list"])
    pipe.renoise_override = draws
    _, lat = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 1                                       # the whole call's DiT work is one hipGraph
    e = rel_l2(lat[..., ::2, ::2], fx["out_strided"])
    print(f"[bidir] few-step: rel_l2 vs reference {e:.3e} (K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(lat.float()).all()
    _, again = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 1 and torch.equal(again, lat)
    pipe.release_graphs()
    _, recaptured = pipe.inference(noise, ["p"], return_latents=True)
    assert pipe.graph_captures == 2 and torch.equal(recaptured, lat)
    _, pipe_e, _, _ = _fewstep()
    pipe_e.use_graphs, pipe_e.renoise_override = False, draws
    _, eager = pipe_e.inference(noise, ["p"], return_latents=True)
    assert pipe_e.graph_captures == 0 and torch.equal(eager, lat)
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


def test_fewstep_draws_match_a_same_seed_generator():
    """The bank holds what torch.randn_like draws in the reference's order: one per forward, the last one included."""
    fx, pipe, noise, _ = _fewstep()
    torch.cuda.manual_seed(4321)
    pipe.inference(noise, ["p"])
    torch.cuda.synchronize()
    (st,) = pipe._calls.values()
    g = torch.Generator(device=DEV).manual_seed(4321)
    assert st["bank"].shape[0] == len(pipe.denoising_step_list) - 1 == fx["meta"]["n_draws"]
    for i in range(st["bank"].shape[0]):
        assert torch.equal(st["bank"][i], torch.randn(st["bank"][i].shape, dtype=torch.bfloat16, device=DEV, generator=g)), i


def test_wrapper_forward_reference_call_shape():
    """WanDiffusionWrapper(is_causal=False).forward(noisy, conditional_dict, timestep) -> (flow_pred, pred_x0): the engine's whole-clip
    forward at timestep[:, 0] and _convert_flow_pred_to_x0 at that timestep's sigma; seq_len is the call's token count."""
    from mmpl_amd.synthetic import philox_normal
    from tests.fewstep_ref import ref_x0
    fx = torch.load(os.path.join(GOLDEN, "bidir_fewstep_tiny.pt"))
    gen, cfg = _generator(fx["meta"])
    ctx = _context(cfg, 32, 40)
    x = philox_normal([1, 9, 16, LAT[0], LAT[1]], 5).to(torch.bfloat16).to(DEV)
    t = torch.full([1, 9], 833.0, device=DEV)
    flow, x0 = gen(x, {"prompt_embeds": ctx}, t)
    kv = gen.engine.precompute_context(ctx[0])
    direct = gen.engine.forward_full(x[0], t[0, :1].float(), kv[0], kv[1], cross_rows=kv.rows)
    torch.cuda.synchronize()
    assert flow.shape == x0.shape == x.shape and gen.seq_len == 9 * gen.engine.S
    assert torch.equal(flow[0], direct)
    assert torch.equal(x0[0].cpu(), ref_x0(flow[0].cpu(), x[0].cpu(), gen.sigma_x0(torch.tensor(833.0))))


def test_cli_bidirectional(tmp_path, capsys):
    from mmpl_amd import cli
    base = ["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--bidirectional", "--sampling_steps", "3"]
    for name, extra in (("unipc", []), ("dpmpp", ["--sample_solver", "dpm++"])):
        cli.main(base + extra + ["--output_folder", str(tmp_path / name)])
        v = torch.load(tmp_path / name / "0-0.pt")
        assert v.dtype == torch.uint8 and tuple(v.shape) == (81, 128, 192, 3)
    assert not torch.equal(torch.load(tmp_path / "unipc" / "0-0.pt"), torch.load(tmp_path / "dpmpp" / "0-0.pt"))
    with pytest.raises(SystemExit):
        cli.main(base + ["--stream"])
    assert "--bidirectional denoises the whole clip at once" in capsys.readouterr().err
