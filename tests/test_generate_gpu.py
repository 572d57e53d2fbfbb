"""GPU tests of mmpl_amd.generate (-m gpu): WanT2V.generate / WanI2V.generate, upstream's float32 latent chain on the HIP engine,
tiny synthetic config, 21 latent frames at 16 x 24 latents.

  reference      WanT2V.generate(noise = the fixture's noise) against the REAL `WanT2V.generate`'s final latents
                 (tests/golden/fp32_chain.pt, make_golden_fp32_chain.py), 6 steps, both solvers.  Tolerance: rel-L2 <= 2 x the
                 fixture's `order_out` -- the reference's own change when its self-attention sums the keys in reverse frame order,
                 doubled because two independent orders differ (the convention of DESIGN.md sections 7d / 7e);
  modes          eager == hipGraph; parallel CFG branches == back to back == back to back without block-0 sharing; a second call
                 constructs no graph; `latent_dtype = bfloat16` on the same pipeline object still gives a fresh bf16 pipeline's bits
                 and float32 afterwards the first float32 bits: the modes do not leak into each other;
  i2v            WanI2V.generate == the pipeline with latent_dtype = float32 on build_image_condition's condition, bit for bit;
  output         float32 [3, 81, 128, 192] in [-1, 1] through the real VAE.
Measured on an MI355X: see DESIGN.md section 7f.
"""
import hashlib
import os
import types

import pytest
import torch

from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)
SIZE = (LAT[1] * 8, LAT[0] * 8)                       # upstream's (width, height)
BF = torch.bfloat16
TAGS = {"unipc": "unipc", "dpmpp": "dpm++"}
_FX = {}


def _fixture():
    if not _FX:
        _FX.update(torch.load(os.path.join(GOLDEN, "fp32_chain.pt")))
    return _FX


class _Text(torch.nn.Module):
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


def _parts(m, i2v=False):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    cfg = dict(WAN_CONFIGS[m["cfg"]], model_type="i2v") if i2v else WAN_CONFIGS[m["cfg"]]
    gen = WanDiffusionWrapper(is_causal=False, timestep_shift=5.0, model_config=cfg, geometry=Geometry(*LAT), device=DEV)
    gen.load_state_dict((dit_i2v_state_dict if i2v else dit_state_dict)(cfg, seed=m["weight_seed"]))
    text = _Text(p=_context(cfg, m["ctx_seed"], m["n_valid"]), NEG=_context(cfg, m["neg_seed"], m["n_valid_neg"]))
    return gen, text


def _noise(m):
    from mmpl_amd.synthetic import philox_normal
    return philox_normal([16, m["F"], LAT[0], LAT[1]], m["noise_seed"], torch.float32)


def _t2v(m, vae=None, **attrs):
    from mmpl_amd.generate import WanT2V
    gen, text = _parts(m)
    wan = WanT2V(dict(num_train_timesteps=m["num_train_timesteps"], sample_neg_prompt="NEG"), "", generator=gen, text_encoder=text,
                 vae=_NoVAE() if vae is None else vae, device=DEV)
    for k, v in attrs.items():
        setattr(wan.pipeline, k, v)
    return wan


def _call(wan, m, steps=None, **kw):
    return wan.generate("p", size=SIZE, frame_num=4 * (m["F"] - 1) + 1, shift=m["shift"], sample_solver=m["sample_solver"],
                        sampling_steps=m["sampling_steps"] if steps is None else steps, guide_scale=m["guide_scale"], n_prompt="",
                        seed=1, offload_model=False, noise=_noise(m), return_latents=True, **kw)[1]


@pytest.mark.parametrize("tag", ["unipc", "dpmpp"])
def test_generate_vs_the_real_generate(tag):
    """Measured on an MI355X: DESIGN.md section 7f (the figure is printed before the assertion)."""
    fx = _fixture()["generate"][TAGS[tag]]
    m = fx["meta"]
    noise = _noise(m)
    assert hashlib.sha256(noise.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() == fx["noise_sha"]
    wan = _t2v(m)
    lat = _call(wan, m)
    assert lat.dtype == torch.float32 and tuple(lat.shape) == (1, m["F"], 16, LAT[0], LAT[1]) and torch.isfinite(lat).all()
    assert wan.pipeline.graph_captures == 1
    out = lat[0].permute(1, 0, 2, 3)                                       # upstream's layout [16, F, h, w]
    e = rel_l2(out[..., ::2, ::2], fx["out_strided"])
    print(f"[generate] {tag}: rel_l2 vs the real WanT2V.generate {e:.3e} (K/V order noise {fx['order_out']:.3e}, bound {2 * fx['order_out']:.3e})")
    again = _call(wan, m)
    assert wan.pipeline.graph_captures == 1 and torch.equal(again, lat)   # the second call only replays
    eager_wan = _t2v(m, use_graphs=False)
    eager = _call(eager_wan, m)
    assert eager_wan.pipeline.graph_captures == 0 and torch.equal(eager, lat)
    assert e <= 2.0 * fx["order_out"], (e, fx["order_out"])


def test_cfg_branch_modes_give_the_same_bits():
    m = _fixture()["generate"]["unipc"]["meta"]
    outs = [_call(_t2v(m, **attrs), m, steps=3)
            for attrs in (dict(concurrent_cfg=True), dict(concurrent_cfg=False), dict(concurrent_cfg=False, share_block0=False))]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def test_the_two_latent_dtypes_do_not_leak_into_each_other():
    """One pipeline object serves both chains: bf16 after float32 gives a fresh bf16 pipeline's bits, float32 after that the first
    float32 bits, and each mode keeps its own graph."""
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    m = _fixture()["generate"]["unipc"]["meta"]
    noise32 = _noise(m).permute(1, 0, 2, 3).unsqueeze(0).to(DEV)
    noise16 = noise32.to(BF)

    def pipeline():
        gen, text = _parts(m)
        args = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=m["guide_scale"], negative_prompt="NEG")
        p = BidirectionalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=text, vae=_NoVAE())
        p.sampling_steps, p.sample_solver, p.shift = 3, "unipc", m["shift"]
        return p

    fresh = pipeline()
    assert fresh.latent_dtype == BF
    _, want16 = fresh.inference(noise16, ["p"], return_latents=True)
    p = pipeline()
    p.latent_dtype = torch.float32
    _, first32 = p.inference(noise32, ["p"], return_latents=True)
    p.latent_dtype = BF
    _, got16 = p.inference(noise16, ["p"], return_latents=True)
    p.latent_dtype = torch.float32
    _, second32 = p.inference(noise32, ["p"], return_latents=True)
    assert p.graph_captures == 2 and len(p._steps) == 2
    assert first32.dtype == torch.float32 and got16.dtype == BF
    assert torch.equal(got16, want16) and torch.equal(second32, first32)
    assert not torch.equal(first32.to(BF), want16)                          # two different samplers


def test_i2v_generate_is_the_float32_pipeline_on_the_built_condition():
    from mmpl_amd.generate import WanI2V
    from mmpl_amd.i2v_clip import CLIPVisionTower
    from mmpl_amd.i2v_condition import build_image_condition
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    from mmpl_amd.synthetic import clip_visual_state_dict, philox_normal, vae_state_dict
    from mmpl_amd.wan_wrapper import WanVAEWrapper
    m = dict(_fixture()["generate"]["unipc"]["meta"], F=5)
    gen, text = _parts(m, i2v=True)
    vae = WanVAEWrapper(geometry=Geometry(*LAT), device=DEV, state_dict=vae_state_dict(seed=2))
    clip = CLIPVisionTower(num_layers=3, device=DEV)
    clip.load_state_dict(clip_visual_state_dict(1280, 16, clip.num_layers, seed=3, device=DEV))
    image = philox_normal([3, 8 * LAT[0], 8 * LAT[1]], 91, torch.float32).clamp_(-1, 1)
    wan = WanI2V(dict(num_train_timesteps=1000, sample_neg_prompt="NEG"), "", init_on_cpu=False, generator=gen, text_encoder=text, vae=vae,
                 clip=clip, device=DEV)
    noise = _noise(m)
    max_area = (8 * LAT[0] + 2) * (8 * LAT[1] + 2)                         # upstream's floor arithmetic lands on 16 x 24 with room to spare
    video, lat = wan.generate("p", image, max_area=max_area, frame_num=4 * (m["F"] - 1) + 1, shift=3.0, sample_solver="unipc", sampling_steps=3,
                              guide_scale=5.0, seed=1, offload_model=False, noise=noise, return_latents=True)
    assert video.dtype == torch.float32 and tuple(video.shape) == (3, 17, 128, 192) and float(video.abs().max()) <= 1.0
    args = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="NEG")
    p = BidirectionalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=text, vae=vae)
    p.sampling_steps, p.sample_solver, p.shift, p.latent_dtype = 3, "unipc", 3.0, torch.float32
    cond = build_image_condition(vae, clip, image.to(DEV), m["F"])
    _, want = p.inference(noise.permute(1, 0, 2, 3).unsqueeze(0).to(DEV), ["p"], return_latents=True, image_condition=cond)
    assert want.dtype == torch.float32 and torch.equal(lat, want)
    with pytest.raises(ValueError, match="created for 16 x 24"):
        wan.generate("p", image, max_area=720 * 1280, noise=noise)


def test_generate_output_is_upstreams():
    """float32 [3, 81, 128, 192] in [-1, 1] through the real VAE; without `noise=` the draw is the device generator's, seeded."""
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import vae_state_dict
    from mmpl_amd.wan_wrapper import WanVAEWrapper
    m = _fixture()["generate"]["unipc"]["meta"]
    wan = _t2v(m, vae=WanVAEWrapper(geometry=Geometry(*LAT), device=DEV, state_dict=vae_state_dict(seed=2)))
    video = wan.generate("p", size=SIZE, sampling_steps=2, seed=7, offload_model=False)
    assert video.dtype == torch.float32 and tuple(video.shape) == (3, 81, 128, 192)
    assert torch.isfinite(video).all() and float(video.min()) >= -1.0 and float(video.max()) <= 1.0 and float(video.std()) > 0
    same = wan.generate("p", size=SIZE, sampling_steps=2, seed=7, offload_model=False)
    other = wan.generate("p", size=SIZE, sampling_steps=2, seed=8, offload_model=False)
    assert torch.equal(same, video) and not torch.equal(other, video)
