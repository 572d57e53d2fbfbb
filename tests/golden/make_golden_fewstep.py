"""Golden fixtures of the few-step (Self-Forcing / CausVid) path: the REAL reference's CausalInferencePipeline.inference
(MMPL_t2v/pipeline/causal_inference.py) and WanDiffusionWrapper.forward / _convert_flow_pred_to_x0 (utils/wan_wrapper.py)
around a tiny CausalWanModel, on the CPU in bf16.  Build-container only (the reference never travels to the GPU box).

    python tests/golden/make_golden_fewstep.py

Writes tests/golden/fewstep_t2v_tiny.pt (9 latent frames = 3 blocks of 3, warped [1000, 750, 500, 250], context_noise 0) and
tests/golden/fewstep_ext_tiny.pt (independent_first_frame with a 1-frame initial latent + 2 blocks of 3, context_noise 37).
Inputs are regenerated from seeds by the tests (mmpl_amd.synthetic.philox_normal): the re-noise draws replace torch.randn_like
in the reference's call order.  Each fixture also holds the reference run again with its attention keys in reverse frame order
(`order_out`: softmax is permutation invariant, only the fp32 summation order changes) -- the unit of the GPU tolerance.
"""
import hashlib
import importlib
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import REF, load_reference  # noqa: E402
from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal  # noqa: E402

torch.set_grad_enabled(False)
S480, H, Wd = 1560, 60, 104


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_fewstep_reference():
    load_reference()                                     # diffusers stubs, wan packages, SDPA cross-attention
    causal = importlib.import_module("wan.modules.causal_model")
    causal.attention = sys.modules["wan.modules.attention"].attention
    # utils/wan_wrapper.py imports the tokenizer, T5 and VAE builders at module level; none of them runs here
    _stub("wan.modules.tokenizers", HuggingfaceTokenizer=object)
    _stub("wan.modules.t5", umt5_xxl=None)
    # demo_utils.memory calls torch.cuda.current_device() at import
    _stub("demo_utils")
    _stub("demo_utils.memory", gpu=None, get_cuda_free_memory_gb=None, DynamicSwapInstaller=None,
          move_model_to_device_with_memory_preservation=None)
    pkg = types.ModuleType("utils")
    pkg.__path__ = [REF + "/utils"]
    sys.modules["utils"] = pkg
    ww = importlib.import_module("utils.wan_wrapper")
    spec = importlib.util.spec_from_file_location("_ref_causal_inference", REF + "/pipeline/causal_inference.py")
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    return causal, ww, ci


def tiny_wrapper(causal, ww, seed):
    cfg = WAN_CONFIGS["tiny"]
    m = causal.CausalWanModel(model_type="t2v", dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"],
                              num_layers=cfg["num_layers"], text_dim=cfg["text_dim"], freq_dim=cfg["freq_dim"]).eval()
    sd = dit_state_dict(cfg, seed=seed)
    m.load_state_dict(sd, strict=True)
    m = m.to(torch.bfloat16)
    w = ww.WanDiffusionWrapper.__new__(ww.WanDiffusionWrapper)          # __init__ would read ../wan_models
    torch.nn.Module.__init__(w)
    w.model = m
    w.uniform_timestep = False
    w.scheduler = ww.FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    w.scheduler.set_timesteps(1000, training=True)
    w.seq_len = 32760
    w.post_init()
    return w, cfg


class _Text(torch.nn.Module):
    def __init__(self, ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8)


def make_context(cfg, seed, n_valid):
    c = philox_normal([1, 512, cfg["text_dim"]], seed)
    c[:, n_valid:] = 0
    return c


def run_reference(ci, w, cfg, args, noise, ctx, draws, initial_latent=None):
    pipe = ci.CausalInferencePipeline(args, device="cpu", generator=w, text_encoder=_Text(ctx), vae=_NoVAE())
    # the reference allocates 1.3B-shaped caches when kv_cache1 is None (12 heads, 30 blocks): hand it the tiny ones
    L, Hh = cfg["num_layers"], cfg["num_heads"]
    pipe.num_transformer_blocks = L
    pipe.frame_seq_length = S480
    pipe.kv_cache1 = [{"k": torch.zeros(1, 21 * S480, Hh, 128, dtype=torch.bfloat16),
                       "v": torch.zeros(1, 21 * S480, Hh, 128, dtype=torch.bfloat16),
                       "global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])} for _ in range(L)]
    pipe.crossattn_cache = [{"k": torch.zeros(1, 512, Hh, 128, dtype=torch.bfloat16),
                             "v": torch.zeros(1, 512, Hh, 128, dtype=torch.bfloat16), "is_init": False} for _ in range(L)]
    queue = list(draws)
    real = torch.randn_like
    torch.randn_like = lambda x, *a, **k: queue.pop(0).reshape(x.shape).to(x)
    try:
        _, out = pipe.inference(noise, ["p"], initial_latent=initial_latent, return_latents=True)
    finally:
        torch.randn_like = real
    assert not queue, len(queue)
    return out, pipe


def with_reversed_keys(causal, fn):
    real = causal.attention

    def permuted(q, k, v, *a, **kw):
        n = k.shape[1] // S480
        idx = torch.arange(n * S480).view(n, S480).flip(0).reshape(-1)
        return real(q, k[:, idx], v[:, idx], *a, **kw)

    causal.attention = permuted
    try:
        return fn()
    finally:
        causal.attention = real


def gen_case(name, causal, ww, ci, *, independent_first_frame, n_init, n_noise, context_noise, seeds):
    w, cfg = tiny_wrapper(causal, ww, seeds["weights"])
    args = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                                 independent_first_frame=independent_first_frame, context_noise=context_noise,
                                 model_kwargs={"timestep_shift": 5.0})
    ctx = make_context(cfg, seeds["ctx"], seeds["n_valid"])
    noise = philox_normal([1, n_noise, 16, H, Wd], seeds["noise"]).to(torch.bfloat16)
    init = philox_normal([1, n_init, 16, H, Wd], seeds["init"]).to(torch.bfloat16) if n_init else None
    sched = ([1] if independent_first_frame and init is None else []) + [3] * ((n_noise - (1 if independent_first_frame and init is None else 0)) // 3)
    draws = [philox_normal([F, 16, H, Wd], seeds["renoise"] + k).to(torch.bfloat16)
             for k, F in enumerate(f for f in sched for _ in range(3))]
    out, pipe = run_reference(ci, w, cfg, args, noise, ctx, draws, init)
    out_perm, _ = with_reversed_keys(causal, lambda: run_reference(ci, w, cfg, args, noise, ctx, draws, init))
    order = rel_l2(out_perm, out)
    print(f"[{name}] output {tuple(out.shape)} rms={out.float().pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}")
    fx = dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order, step_list=pipe.denoising_step_list.clone(),
              meta=dict(cfg="tiny", weight_seed=seeds["weights"], ctx_seed=seeds["ctx"], n_valid=seeds["n_valid"],
                        noise_seed=seeds["noise"], init_seed=seeds["init"] if n_init else None, n_init=n_init, n_noise=n_noise,
                        renoise_seed_base=seeds["renoise"], schedule=sched, independent_first_frame=independent_first_frame,
                        context_noise=context_noise, denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True,
                        num_frame_per_block=3, timestep_shift=5.0, lat_hw=(H, Wd)))
    return fx, (w, cfg)


def gen_wrapper_x0(ww, w, cfg):
    """_convert_flow_pred_to_x0 alone on seeded data at every warped step (the device kernel's fp64 chain)."""
    flow = philox_normal([4, 16, 8, 8], 901).to(torch.bfloat16)
    xt = philox_normal([4, 16, 8, 8], 902).to(torch.bfloat16)
    ts = torch.tensor([1000.0, 937.5, 833.3333, 625.0])
    x0 = w._convert_flow_pred_to_x0(flow, xt, ts)
    return dict(x0_flow_seed=901, x0_xt_seed=902, x0_timesteps=ts, x0=x0)


def main():
    causal, ww, ci = load_fewstep_reference()
    fx, (w, cfg) = gen_case("t2v", causal, ww, ci, independent_first_frame=False, n_init=0, n_noise=9, context_noise=0,
                            seeds=dict(weights=31, ctx=32, n_valid=40, noise=33, init=None, renoise=400))
    fx.update(gen_wrapper_x0(ww, w, cfg))
    torch.save(fx, os.path.join(HERE, "fewstep_t2v_tiny.pt"))
    fx, _ = gen_case("ext", causal, ww, ci, independent_first_frame=True, n_init=1, n_noise=6, context_noise=37,
                     seeds=dict(weights=41, ctx=42, n_valid=24, noise=43, init=44, renoise=500))
    torch.save(fx, os.path.join(HERE, "fewstep_ext_tiny.pt"))


if __name__ == "__main__":
    main()
