"""Golden fixtures of the bidirectional Wan2.1 IMAGE-to-video path from the REAL reference, on the CPU in bf16: one
WanModel(model_type="i2v", in_dim=36) forward with `clip_fea` and `y` (wan/modules/model.py:626-760) and the reference's own
BidirectionalDiffusionInferencePipeline.inference (pipeline/bidirectional_diffusion_inference.py) once per solver around that model,
tiny config on `dit_i2v_state_dict`, 21 frames at 16 x 24 latents (S = 96).  Build-container only (the reference never travels to
the GPU box).

    python tests/golden/make_golden_bidir_i2v.py

Writes tests/golden/bidir_i2v_forward_tiny.pt and bidir_i2v_diffusion_{unipc,dpmpp}_tiny.pt.  The reference's pipeline knows no
image: `bind_image` below binds `clip_fea` / `y` into `model.forward` for the run, the way `with_reversed_keys` binds the key
order, so both CFG branches see the image as in upstream WanI2V.generate (wan/image2video.py: `arg_c` and `arg_null` both carry
`clip_fea` and `y`).  Inputs are regenerated from seeds by the tests (mmpl_amd.synthetic.philox_normal).  The forward output is
stored whole, the pipelines' strided, each with a sha256 of the full tensor and `order_out`: the rel-L2 of the same run with the
self-attention keys in reverse frame order (softmax is permutation invariant, only the fp32 summation order changes) -- the unit
of the GPU tolerance.
"""
import functools
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import REF  # noqa: E402
from make_golden_bidir import F_, H, S, SHIFT, Wd, _load, with_reversed_keys  # noqa: E402
from make_golden_fewstep import _NoVAE, load_fewstep_reference, make_context, rel_l2, sha  # noqa: E402
from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, philox_normal  # noqa: E402

torch.set_grad_enabled(False)


def tiny_i2v_wrapper(model, ww, seed):
    cfg = WAN_CONFIGS["tiny"]
    m = model.WanModel(model_type="i2v", in_dim=36, dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"],
                       num_layers=cfg["num_layers"], text_dim=cfg["text_dim"], freq_dim=cfg["freq_dim"]).eval()
    m.load_state_dict(dit_i2v_state_dict(cfg, seed=seed), strict=True)
    m = m.to(torch.bfloat16)
    w = ww.WanDiffusionWrapper.__new__(ww.WanDiffusionWrapper)          # __init__ would read wan_models/
    torch.nn.Module.__init__(w)
    w.model = m
    w.uniform_timestep = True
    w.scheduler = ww.FlowMatchScheduler(shift=SHIFT, sigma_min=0.0, extra_one_step=True)
    w.scheduler.set_timesteps(1000, training=True)
    w.seq_len = F_ * S
    w.post_init()
    return w, cfg


def image_inputs(clip_seed, y_seed):
    """(clip_fea [257, 1280], y [20, F, h, w]) in bf16 -- regenerated bit-identically by the tests"""
    return (philox_normal([257, 1280], clip_seed).to(torch.bfloat16), philox_normal([20, F_, H, Wd], y_seed).to(torch.bfloat16))


def bind_image(m, clip_fea, y):
    """Every later m(...) gets clip_fea / y (batch of one), whoever calls it."""
    m.forward = functools.partial(m.forward, clip_fea=clip_fea.unsqueeze(0), y=[y])


def gen_forward(model, ww):
    meta = dict(cfg="tiny", weight_seed=91, x_seed=92, ctx_seed=93, clip_seed=94, y_seed=95, n_valid=40, t=673.0, F=F_, lat_hw=(H, Wd))
    w, cfg = tiny_i2v_wrapper(model, ww, meta["weight_seed"])
    x = philox_normal([16, F_, H, Wd], meta["x_seed"]).to(torch.bfloat16)
    ctx = philox_normal([meta["n_valid"], cfg["text_dim"]], meta["ctx_seed"]).to(torch.bfloat16)
    clip_fea, y = image_inputs(meta["clip_seed"], meta["y_seed"])

    def run():
        out = w.model([x], t=torch.tensor([meta["t"]], dtype=torch.float32), context=[ctx], seq_len=F_ * S,
                      clip_fea=clip_fea.unsqueeze(0), y=[y])
        out = out[0] if isinstance(out, (list, tuple)) else out
        return out.squeeze(0) if out.dim() == 5 else out                # [16, F, h, w]

    out = run()
    order = rel_l2(with_reversed_keys(model, run), out)
    print(f"[i2v forward] out {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}")
    return dict(out=out.clone(), out_sha=sha(out), order_out=order, meta=meta)


def gen_diffusion(model, ww, bd, solver):
    seeds = dict(weights=101, ctx=102, n_valid=40, neg=103, n_valid_neg=17, noise=104, clip=105, y=106)
    w, cfg = tiny_i2v_wrapper(model, ww, seeds["weights"])
    ctx = make_context(cfg, seeds["ctx"], seeds["n_valid"]).to(torch.bfloat16)
    neg = make_context(cfg, seeds["neg"], seeds["n_valid_neg"]).to(torch.bfloat16)
    noise = philox_normal([1, F_, 16, H, Wd], seeds["noise"]).to(torch.bfloat16)
    bind_image(w.model, *image_inputs(seeds["clip"], seeds["y"]))
    args = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="NEG", model_kwargs={})

    class Text(torch.nn.Module):
        def forward(self, text_prompts):
            return {"prompt_embeds": neg if text_prompts[0] == "NEG" else ctx}

    def run():
        pipe = bd.BidirectionalDiffusionInferencePipeline(args, device="cpu", generator=w, text_encoder=Text(), vae=_NoVAE())
        pipe.sampling_steps = 6
        pipe.sample_solver = solver
        _, lat = pipe.inference(noise, ["p"], return_latents=True)
        return lat, pipe

    out, pipe = run()
    out_perm, _ = with_reversed_keys(model, run)
    order = rel_l2(out_perm, out)
    print(f"[i2v diffusion {solver}] out {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  "
          f"K/V order noise rel_l2={order:.3e}")
    return dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order,
                timesteps=torch.as_tensor(pipe.timesteps).clone().cpu(),
                meta=dict(cfg="tiny", weight_seed=seeds["weights"], ctx_seed=seeds["ctx"], n_valid=seeds["n_valid"],
                          neg_seed=seeds["neg"], n_valid_neg=seeds["n_valid_neg"], noise_seed=seeds["noise"], clip_seed=seeds["clip"],
                          y_seed=seeds["y"], F=F_, lat_hw=(H, Wd), guidance_scale=5.0, sampling_steps=6, sample_solver=solver, shift=8.0,
                          num_train_timestep=1000, timestep_shift=SHIFT))


def main():
    _, ww, _ = load_fewstep_reference()                 # diffusers stubs, wan packages, utils.wan_wrapper
    model = sys.modules["wan.modules.model"]
    from make_golden_dpmpp import load_dpm_reference
    load_dpm_reference()                                # wan.utils.fm_solvers (DPM-Solver++), which the diffusion pipeline imports
    bd = _load("_ref_bidir_diffusion", REF + "/pipeline/bidirectional_diffusion_inference.py")
    torch.save(gen_forward(model, ww), os.path.join(HERE, "bidir_i2v_forward_tiny.pt"))
    for solver, tag in (("unipc", "unipc"), ("dpm++", "dpmpp")):
        torch.save(gen_diffusion(model, ww, bd, solver), os.path.join(HERE, f"bidir_i2v_diffusion_{tag}_tiny.pt"))


if __name__ == "__main__":
    main()
