"""GPU tests of BidirectionalDiffusionInferencePipeline over the Wan-I2V model type (-m gpu): 6 CFG steps of a whole 21-frame clip,
both solvers, against the REAL reference's latents (tests/golden/make_golden_bidir_i2v.py), the modes' bit-identity, a second image
through the same graph, the wrapper's reference call shape and the CLI.  Tiny synthetic config at 16 x 24 latents.

Tolerance: rel-L2(HIP, reference) <= 2 x the fixture's `order_out` -- the reference's own change when its self-attention sums the
keys in reverse frame order, doubled because two independent orders differ (the margin of every whole-trajectory row of
DESIGN.md section 7d)."""
import os
import types

import pytest
import torch

from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)
BF = torch.bfloat16


class _Text(torch.nn.Module):
    """prompt -> a seeded context; the negative prompt "NEG" -> the other one; "q" -> a third."""

    def __init__(self, **ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx[text_prompts[0]]}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _context(cfg, seed, n_valid):
    from mmpl_amd.synthetic import philox_normal
    c = philox_normal([1, 512, cfg["text_dim"]], seed)
    c[:, n_valid:] = 0
    return c.to(BF).to(DEV)


def _image(clip_seed, y_seed, F_=21):
    from mmpl_amd.synthetic import philox_normal
    return {"clip_fea": philox_normal([257, 1280], clip_seed).to(BF).to(DEV), "y": philox_normal([20, F_, LAT[0], LAT[1]], y_seed).to(BF).to(DEV)}


def _generator(m):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    cfg = dict(WAN_CONFIGS[m["cfg"]], model_type="i2v")
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=m["timestep_shift"], model_config=cfg, geometry=Geometry(*LAT), device=DEV)
    gen.load_state_dict(dit_i2v_state_dict(cfg, seed=m["weight_seed"]))
    assert gen.model_type == "i2v" and gen.engine.in_dim == 36 and gen.uniform_timestep is True
    return gen, cfg


_FX = {}


def _fixture(tag):
    if tag not in _FX:
        _FX[tag] = torch.load(os.path.join(GOLDEN, f"bidir_i2v_diffusion_{tag}_tiny.pt"))
    return _FX[tag]


def _diffusion(tag, **attrs):
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.synthetic import philox_normal
    fx = _fixture(tag)
    m = fx["meta"]
    gen, cfg = _generator(m)
    args = types.SimpleNamespace(num_train_timestep=m["num_train_timestep"], guidance_scale=m["guidance_scale"], negative_prompt="NEG",
                                 timestep_shift=3.0)
    text = _Text(p=_context(cfg, m["ctx_seed"], m["n_valid"]), NEG=_context(cfg, m["neg_seed"], m["n_valid_neg"]), q=_context(cfg, 222, 29))
    pipe = BidirectionalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=text, vae=_NoVAE())
    pipe.sampling_steps, pipe.sample_solver = m["sampling_steps"], m["sample_solver"]
    for k, v in attrs.items():
        setattr(pipe, k, v)
    noise = philox_normal([1, m["F"], 16, LAT[0], LAT[1]], m["noise_seed"]).to(BF).to(DEV)
    return fx, pipe, noise, _image(m["clip_seed"], m["y_seed"], m["F"])


@pytest.mark.parametrize("tag", ["unipc", "dpmpp"])
def test_i2v_diffusion_trajectory_vs_reference(tag):
    """6 CFG steps against the reference's BidirectionalDiffusionInferencePipeline.inference around WanModel(model_type='i2v'); the
    eager path gives the graph path's bits.  Measured on an MI355X: UniPC 8.307e-03 (bound 1.345e-02), DPM-Solver++ 6.945e-03
    (bound 1.357e-02); DESIGN.md section 7e."""
    fx, pipe, noise, cond = _diffusion(tag)
    _, lat = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)
    assert pipe.graph_captures == 1
    assert [float(t) for t in pipe.timesteps] == [float(t) for t in fx["timesteps"]]
    e = rel_l2(lat[..., ::2, ::2], fx["out_strided"])
    print(f"[bidir i2v] diffusion {tag}: rel_l2 vs reference {e:.3e} (K/V order noise {fx['order_out']:.3e}, bound {2 * fx['order_out']:.3e})")
    assert torch.isfinite(lat.float()).all()
    _, pipe_e, _, _ = _diffusion(tag, use_graphs=False)
    _, eager = pipe_e.inference(noise, ["p"], return_latents=True, image_condition=cond)
    assert pipe_e.graph_captures == 0 and torch.equal(eager, lat)
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


def test_i2v_concurrent_branches_give_the_sequential_bits():
    """The two CFG branches as parallel graph branches (second stream, private workspace), back to back with block 0 shared, or back
    to back without sharing: the same bits -- both branches see the same image, so block 0 is still one computation."""
    outs = []
    for attrs in (dict(concurrent_cfg=True), dict(concurrent_cfg=False), dict(concurrent_cfg=False, share_block0=False)):
        _, pipe, noise, cond = _diffusion("unipc", **attrs)
        pipe.sampling_steps = 3
        outs.append(pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)[1])
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])


def test_second_image_and_prompt_replay_the_same_graph():
    """y and the image K / V are refreshed in place: another image and prompt construct no graph and give the bits of a fresh
    pipeline's eager run on them; the first image again gives the first result."""
    _, pipe, noise, cond = _diffusion("unipc")
    pipe.sampling_steps = 3
    _, first = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)
    assert pipe.graph_captures == 1
    cond2 = _image(301, 302)
    _, second = pipe.inference(noise, ["q"], return_latents=True, image_condition=cond2)
    assert pipe.graph_captures == 1
    _, fresh, _, _ = _diffusion("unipc", use_graphs=False)
    fresh.sampling_steps = 3
    _, want = fresh.inference(noise, ["q"], return_latents=True, image_condition=cond2)
    assert fresh.graph_captures == 0
    assert torch.equal(second, want) and not torch.equal(second, first)
    # the image alone matters (same prompt, other image), and going back gives the first bits
    _, third = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond2)
    _, again = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)
    assert pipe.graph_captures == 1
    assert not torch.equal(third, first) and torch.equal(again, first)
    # a clip_fea tensor written in place is noticed by its version counter
    cond["clip_fea"].copy_(cond2["clip_fea"])
    cond["y"].copy_(cond2["y"])
    _, rewritten = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)
    assert torch.equal(rewritten, third)
    with pytest.raises(ValueError, match="image_condition"):
        pipe.inference(noise, ["p"])
    with pytest.raises(ValueError, match="latent frames"):
        pipe.inference(noise, ["p"], image_condition=_image(301, 302, F_=9))


def test_wrapper_forward_reference_call_shape():
    """WanDiffusionWrapper(is_causal=False).forward over an i2v config: clip_fea / y from conditional_dict -> the engine's whole-clip
    forward; the image K / V are rebuilt only when the clip_fea tensor or its version changed."""
    from mmpl_amd.synthetic import philox_normal
    gen, cfg = _generator(_fixture("unipc")["meta"])
    ctx = _context(cfg, 32, 40)
    cond = _image(41, 42, F_=9)
    x = philox_normal([1, 9, 16, LAT[0], LAT[1]], 5).to(BF).to(DEV)
    t = torch.full([1, 9], 833.0, device=DEV)
    calls = []
    real = gen.engine.precompute_image_context
    gen.engine.precompute_image_context = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    d = {"prompt_embeds": ctx, "clip_fea": cond["clip_fea"], "y": cond["y"]}
    flow, x0 = gen(x, d, t)
    flow_b, _ = gen(x, d, t)
    assert len(calls) == 1                                                # same tensor, same version: kept
    kv = gen.engine.precompute_context(ctx[0])
    direct = gen.engine.forward_full(x[0], t[0, :1].float(), kv[0], kv[1], cross_rows=kv.rows, y=cond["y"].permute(1, 0, 2, 3).contiguous())
    torch.cuda.synchronize()
    assert flow.shape == x0.shape == x.shape and gen.seq_len == 9 * gen.engine.S
    assert torch.equal(flow[0], direct) and torch.equal(flow_b, flow)
    pair = gen._img_kv
    cond["clip_fea"].mul_(-1)                                             # written in place: rebuilt, into the same pair
    flow_c, _ = gen(x, d, t)
    assert len(calls) == 2 and gen._img_kv[0].data_ptr() == pair[0].data_ptr() and not torch.equal(flow_c, flow)
    with pytest.raises(ValueError, match="clip_fea and y"):
        gen(x, {"prompt_embeds": ctx}, t)
    with pytest.raises(ValueError, match="frames"):
        gen(x[:, :3], d, t[:, :3])


def test_causal_wrapper_still_refuses_an_i2v_config():
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    with pytest.raises(ValueError, match="t2v model"):
        WanDiffusionWrapper(is_causal=True, model_config=dict(WAN_CONFIGS["tiny"], model_type="i2v"), geometry=Geometry(*LAT), device=DEV)


def test_cli_bidirectional_i2v(tmp_path, capsys):
    """--bidirectional --i2v --i2v_model --image FILE on the tiny model: image -> CLIP tower + VAE encode -> 3 CFG steps of the whole clip."""
    import numpy as np
    from PIL import Image
    from mmpl_amd import cli
    rng = np.random.default_rng(1)
    img = tmp_path / "in.png"
    Image.fromarray(rng.integers(0, 255, (90, 130, 3), dtype=np.uint8)).save(img)
    base = ["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--bidirectional", "--sampling_steps", "3"]
    cli.main(base + ["--i2v", "--i2v_model", "--image", str(img), "--output_folder", str(tmp_path / "i2v")])
    v = torch.load(tmp_path / "i2v" / "0-0.pt")
    assert v.dtype == torch.uint8 and tuple(v.shape) == (81, 128, 192, 3) and v.float().std() > 1.0
    with pytest.raises(SystemExit):
        cli.main(base + ["--i2v", "--image", str(img)])
    assert "--i2v" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ["--i2v", "--i2v_model"])
    assert "--i2v_model needs --i2v --image" in capsys.readouterr().err
