"""Golden fixture of the BATCHED few-step path: the real reference's CausalInferencePipeline.inference at batch 2 (two prompts, one
noise tensor [2, F, 16, h, w], one re-noise draw [2, 3, 16, h, w] per non-final step) around the tiny CausalWanModel, on the CPU in
bf16.  Build-container only, like make_golden_fewstep.py, whose helpers it uses.

    python tests/golden/make_golden_fewstep_batch.py

Writes tests/golden/fewstep_batch_tiny.pt: 6 latent frames = 2 blocks of 3 per sample, warped [1000, 750, 500, 250], context_noise 0,
contexts with 40 and 17 valid rows.  `order_out`: the same run with the attention keys in reverse frame order (the fp32 summation
order only), the unit of the GPU tolerance.
"""
import os
import types

import torch

from make_golden_fewstep import (H, HERE, S480, Wd, _NoVAE, _Text, load_fewstep_reference, make_context, rel_l2, sha, tiny_wrapper,
                                 with_reversed_keys)
from mmpl_amd.synthetic import philox_normal

torch.set_grad_enabled(False)
B, N_NOISE, F = 2, 6, 3
SEEDS = dict(weights=51, ctx=(52, 53), n_valid=(40, 17), noise=54, renoise=600)


def run_reference(ci, w, cfg, args, noise, ctx, draws):
    pipe = ci.CausalInferencePipeline(args, device="cpu", generator=w, text_encoder=_Text(ctx), vae=_NoVAE())
    L, Hh = cfg["num_layers"], cfg["num_heads"]
    pipe.num_transformer_blocks = L
    pipe.frame_seq_length = S480
    z = lambda rows: torch.zeros(B, rows, Hh, 128, dtype=torch.bfloat16)
    pipe.kv_cache1 = [{"k": z(21 * S480), "v": z(21 * S480), "global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])}
                      for _ in range(L)]
    pipe.crossattn_cache = [{"k": z(512), "v": z(512), "is_init": False} for _ in range(L)]
    queue = list(draws)
    real = torch.randn_like
    torch.randn_like = lambda x, *a, **k: queue.pop(0).reshape(x.shape).to(x)
    try:
        _, out = pipe.inference(noise, ["p0", "p1"], return_latents=True)
    finally:
        torch.randn_like = real
    assert not queue, len(queue)
    return out, pipe


def main():
    causal, ww, ci = load_fewstep_reference()
    w, cfg = tiny_wrapper(causal, ww, SEEDS["weights"])
    args = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=F,
                                 independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    ctx = torch.cat([make_context(cfg, s, n) for s, n in zip(SEEDS["ctx"], SEEDS["n_valid"])])
    noise = philox_normal([B, N_NOISE, 16, H, Wd], SEEDS["noise"]).to(torch.bfloat16)
    draws = [philox_normal([B, F, 16, H, Wd], SEEDS["renoise"] + k).to(torch.bfloat16) for k in range(3 * (N_NOISE // F))]
    out, pipe = run_reference(ci, w, cfg, args, noise, ctx, draws)
    out_perm, _ = with_reversed_keys(causal, lambda: run_reference(ci, w, cfg, args, noise, ctx, draws))
    order = rel_l2(out_perm, out)
    print(f"[batch] output {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}")
    fx = dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order, step_list=pipe.denoising_step_list.clone(),
              meta=dict(cfg="tiny", batch=B, weight_seed=SEEDS["weights"], ctx_seeds=SEEDS["ctx"], n_valid=SEEDS["n_valid"],
                        noise_seed=SEEDS["noise"], n_noise=N_NOISE, renoise_seed_base=SEEDS["renoise"], schedule=[F] * (N_NOISE // F),
                        independent_first_frame=False, context_noise=0, denoising_step_list=[1000, 750, 500, 250],
                        warp_denoising_step=True, num_frame_per_block=F, timestep_shift=5.0, lat_hw=(H, Wd)))
    torch.save(fx, os.path.join(HERE, "fewstep_batch_tiny.pt"))


if __name__ == "__main__":
    main()
