"""Golden fixtures of the bidirectional (non-causal) Wan2.1 path from the REAL reference, on the CPU in bf16: one
WanModel(model_type="t2v") forward (wan/modules/model.py), BidirectionalDiffusionInferencePipeline.inference
(pipeline/bidirectional_diffusion_inference.py) once per solver and BidirectionalInferencePipeline.inference
(pipeline/bidirectional_inference.py), all around a tiny WanModel at 16 x 24 latents (S = 96) and 21 frames.  Build-container only
(the reference never travels to the GPU box).

    python tests/golden/make_golden_bidir.py

Writes tests/golden/bidir_forward_tiny.pt, bidir_diffusion_{unipc,dpmpp}_tiny.pt and bidir_fewstep_tiny.pt.  Inputs are regenerated
from seeds by the tests (mmpl_amd.synthetic.philox_normal); the few-step re-noise draws replace torch.randn_like in the
reference's call order.  Outputs are stored strided with a sha256 of the full tensor.  Each pipeline fixture also holds the
reference run again with its self-attention keys in reverse frame order (`order_out`: softmax is permutation invariant, only the
fp32 summation order changes) -- the unit of the GPU tolerance.  The wrapper's seq_len is the call's token count: nothing is padded.
"""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import REF  # noqa: E402
from make_golden_fewstep import _NoVAE, _Text, load_fewstep_reference, make_context, rel_l2, sha  # noqa: E402
from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal  # noqa: E402

torch.set_grad_enabled(False)
H, Wd, F_ = 16, 24, 21
S = (H // 2) * (Wd // 2)
SHIFT = 5.0            # timestep_shift of the wrapper's FlowMatchScheduler (the few-step fixture's re-noise sigmas)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def tiny_wrapper(model, ww, seed):
    cfg = WAN_CONFIGS["tiny"]
    m = model.WanModel(model_type="t2v", dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"],
                       num_layers=cfg["num_layers"], text_dim=cfg["text_dim"], freq_dim=cfg["freq_dim"]).eval()
    m.load_state_dict(dit_state_dict(cfg, seed=seed), strict=True)
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


def with_reversed_keys(model, fn):
    """Run fn() with the self-attention's keys / values in reverse frame order (the text cross-attention, 512 keys, untouched)."""
    real = model.flash_attention

    def permuted(*a, **kw):
        if "k" in kw and kw["k"].shape[1] == F_ * S:
            idx = torch.arange(F_ * S).view(F_, S).flip(0).reshape(-1)
            kw = dict(kw, k=kw["k"][:, idx], v=kw["v"][:, idx])
        return real(*a, **kw)

    model.flash_attention = permuted
    try:
        return fn()
    finally:
        model.flash_attention = real


def gen_forward(model, ww):
    meta = dict(cfg="tiny", weight_seed=61, x_seed=62, ctx_seed=63, n_valid=40, t=673.0, F=F_, lat_hw=(H, Wd))
    w, cfg = tiny_wrapper(model, ww, meta["weight_seed"])
    x = philox_normal([16, F_, H, Wd], meta["x_seed"]).to(torch.bfloat16)
    ctx = philox_normal([meta["n_valid"], cfg["text_dim"]], meta["ctx_seed"]).to(torch.bfloat16)
    run = lambda: w.model([x], t=torch.tensor([meta["t"]], dtype=torch.float32), context=[ctx], seq_len=F_ * S)
    out = run()
    out = (out[0] if isinstance(out, (list, tuple)) else out)
    out = out.squeeze(0) if out.dim() == 5 else out                     # [16, F, h, w]
    perm = with_reversed_keys(model, run)
    perm = (perm[0] if isinstance(perm, (list, tuple)) else perm)
    perm = perm.squeeze(0) if perm.dim() == 5 else perm
    order = rel_l2(perm, out)
    print(f"[forward] out {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}")
    return dict(out=out.clone(), out_sha=sha(out), order_out=order, meta=meta)


def gen_diffusion(model, ww, bd, solver):
    seeds = dict(weights=71, ctx=72, n_valid=40, neg=73, n_valid_neg=17, noise=74)
    w, cfg = tiny_wrapper(model, ww, seeds["weights"])
    ctx = make_context(cfg, seeds["ctx"], seeds["n_valid"]).to(torch.bfloat16)
    neg = make_context(cfg, seeds["neg"], seeds["n_valid_neg"]).to(torch.bfloat16)
    noise = philox_normal([1, F_, 16, H, Wd], seeds["noise"]).to(torch.bfloat16)
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
    print(f"[diffusion {solver}] out {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  "
          f"K/V order noise rel_l2={order:.3e}")
    return dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order,
                timesteps=torch.as_tensor(pipe.timesteps).clone().cpu(),
                meta=dict(cfg="tiny", weight_seed=seeds["weights"], ctx_seed=seeds["ctx"], n_valid=seeds["n_valid"],
                          neg_seed=seeds["neg"], n_valid_neg=seeds["n_valid_neg"], noise_seed=seeds["noise"], F=F_, lat_hw=(H, Wd),
                          guidance_scale=5.0, sampling_steps=6, sample_solver=solver, shift=8.0, num_train_timestep=1000,
                          timestep_shift=SHIFT))


def gen_fewstep(model, ww, bi):
    seeds = dict(weights=81, ctx=82, n_valid=40, noise=83, renoise=600)
    w, cfg = tiny_wrapper(model, ww, seeds["weights"])
    ctx = make_context(cfg, seeds["ctx"], seeds["n_valid"]).to(torch.bfloat16)
    noise = philox_normal([1, F_, 16, H, Wd], seeds["noise"]).to(torch.bfloat16)
    steps = [1000, 750, 500, 250]
    args = types.SimpleNamespace(denoising_step_list=steps, warp_denoising_step=True, model_kwargs={})
    n_draws = len(steps) - 1                                            # one per forward, the last one consumed unused
    draws = [philox_normal([F_, 16, H, Wd], seeds["renoise"] + k).to(torch.bfloat16) for k in range(n_draws)]
    last = {}

    class VAE:
        def decode_to_pixel(self, latent, use_cache=False):
            last["x0"] = latent.clone()
            return torch.zeros(1, 1, 3, 8, 8)

    def run():
        pipe = bi.BidirectionalInferencePipeline(args, device="cpu", generator=w, text_encoder=_Text(ctx), vae=VAE())
        queue = list(draws)
        real = torch.randn_like
        torch.randn_like = lambda x, *a, **k: queue.pop(0).reshape(x.shape).to(x)
        try:
            pipe.inference(noise, ["p"])
        finally:
            torch.randn_like = real
        assert not queue, len(queue)
        return last["x0"], pipe

    out, pipe = run()
    out_perm, _ = with_reversed_keys(model, run)
    order = rel_l2(out_perm, out)
    print(f"[fewstep] out {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}  "
          f"steps {pipe.denoising_step_list.tolist()}")
    return dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order, step_list=pipe.denoising_step_list.clone().cpu(),
                meta=dict(cfg="tiny", weight_seed=seeds["weights"], ctx_seed=seeds["ctx"], n_valid=seeds["n_valid"],
                          noise_seed=seeds["noise"], renoise_seed_base=seeds["renoise"], n_draws=n_draws, F=F_, lat_hw=(H, Wd),
                          denoising_step_list=steps, warp_denoising_step=True, timestep_shift=SHIFT))


def main():
    _, ww, _ = load_fewstep_reference()                 # diffusers stubs, wan packages, utils.wan_wrapper
    model = sys.modules["wan.modules.model"]
    from make_golden_dpmpp import load_dpm_reference
    load_dpm_reference()                                # wan.utils.fm_solvers (DPM-Solver++), which the diffusion pipeline imports
    bd = _load("_ref_bidir_diffusion", REF + "/pipeline/bidirectional_diffusion_inference.py")
    bi = _load("_ref_bidir", REF + "/pipeline/bidirectional_inference.py")
    torch.save(gen_forward(model, ww), os.path.join(HERE, "bidir_forward_tiny.pt"))
    for solver, tag in (("unipc", "unipc"), ("dpm++", "dpmpp")):
        torch.save(gen_diffusion(model, ww, bd, solver), os.path.join(HERE, f"bidir_diffusion_{tag}_tiny.pt"))
    torch.save(gen_fewstep(model, ww, bi), os.path.join(HERE, "bidir_fewstep_tiny.pt"))


if __name__ == "__main__":
    main()
