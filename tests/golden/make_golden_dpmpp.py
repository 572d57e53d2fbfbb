"""Golden fixtures of the DPM-Solver++ sampler (sample_solver='dpm++'): the REAL reference's FlowDPMSolverMultistepScheduler
(MMPL_t2v/wan/utils/fm_solvers.py), built the way its pipeline builds it (pipeline/casual_fps_inference.py:512-521), on the CPU
in bf16.  Build-container only (the reference never travels to the GPU box).

    python tests/golden/make_golden_dpmpp.py [sched] [chunk]

sched -> tests/golden/dpmpp_sched.pt, for the schedules (50 steps, shift 5) and (10 steps, shift 5):
    timesteps, sigmas; the per-step scalars (sigma_cur, c1, c2, inv_r0, order) from the reference's expressions on ITS sigmas --
    checked here by running the kernel's chain with them against the reference's step, bit for bit, on every step;
    the toy-field trajectory of make_golden.gen_sched's kind (x0 from seed 5, target from seed 6): the flow fed to every step and the
    sample after it (the sample before step i is the one after step i - 1), under CPU scalar semantics (the reference as is) and
    under the scalar semantics of its native platform (`scheduler.sigmas` carrying make_golden._GpuScalar).
chunk -> tests/golden/chunk_t2v_tiny_dpmpp.pt: the T2V first chunk of make_golden.gen_chunk's kind (tiny model, seeds of its meta)
    through make_golden._ref_stage_loop with the DPM-Solver++ scheduler in place of UniPC, 10 steps per stage, `_GpuScalar`
    semantics, at 60x104 -- the one latent size the reference model runs at (frame_seqlen 1560 is a literal in
    causal_fps_model.py:194-256) -- stored strided; and the same run with only the K/V gather order of its self-attention
    reversed (make_golden.gen_chunk50_deep's `perm`): the reference's own noise floor, the unit of the GPU test's bound.
"""
import importlib
import os
import sys
import time
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from _ref_import import load_reference  # noqa: E402
from mmpl_amd.synthetic import philox_normal  # noqa: E402

torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHEDULES = ((50, 5.0), (10, 5.0))
TOY_SHAPE = [1, 3, 4, 6, 8]


def load_dpm_reference():
    """wan.utils.fm_solvers next to what load_reference() imports; it also wants diffusers.utils.torch_utils.randn_tensor (the SDE
    variants' noise, never called here)."""
    load_reference()
    m = types.ModuleType("diffusers.utils.torch_utils")
    m.randn_tensor = None
    sys.modules["diffusers.utils.torch_utils"] = m
    return importlib.import_module("wan.utils.fm_solvers")


def build_scheduler(fm, steps, shift, gpu_scalars=False):
    """casual_fps_inference.py:512-521, literally."""
    s = fm.FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    timesteps, _ = fm.retrieve_timesteps(s, device="cpu", sigmas=fm.get_sampling_sigmas(steps, shift))
    assert timesteps is s.timesteps
    if gpu_scalars:
        s.sigmas = s.sigmas.as_subclass(MG._GpuScalar)
    return s


def rbf(t):
    return t.to(BF).to(torch.float32)


def step_scalars(sigmas, i, n):
    """The scalars of step i from the reference's expressions (fm_solvers.py:457-468, 529-553) on plain fp32 0-dim tensors."""
    lam = lambda q: torch.log(1 - q) - torch.log(q)
    sigma_t, sigma_s0 = sigmas[i + 1], sigmas[i]
    h = lam(sigma_t) - lam(sigma_s0)
    order = 1 if i == 0 or i == n - 1 else 2
    inv_r0 = (1.0 / ((lam(sigma_s0) - lam(sigmas[i - 1])) / h)).item() if order == 2 else 0.0
    return dict(sigma_cur=sigma_s0.item(), c1=(sigma_t / sigma_s0).item(), c2=((1 - sigma_t) * (torch.exp(-h) - 1.0)).item(), inv_r0=inv_r0,
                order=order)


def chain(sc, flow, x, m0, gpu):
    """The fused kernel's chain in torch fp32 (gpu: scalars in fp32; else rounded to bf16 where the CPU kernels round them)."""
    q = (lambda v: torch.tensor(v, dtype=torch.float32)) if gpu else (lambda v: rbf(torch.tensor(v, dtype=torch.float32)))
    f, xe = flow.float(), x.float()
    x0 = rbf(xe - rbf(q(sc["sigma_cur"]) * f))
    m1, m0 = m0, x0
    acc = torch.tensor(sc["c1"], dtype=torch.float32) * xe - rbf(q(sc["c2"]) * m0)
    if sc["order"] == 2:
        half_c2 = (0.5 * torch.tensor(sc["c2"], dtype=torch.float32)).item()
        acc = acc - rbf(q(half_c2) * rbf(q(sc["inv_r0"]) * rbf(m0 - m1)))
    return acc.to(BF), m0


def gen_sched():
    fm = load_dpm_reference()
    out = dict(produced_by="the REAL reference (wan/utils/fm_solvers.py FlowDPMSolverMultistepScheduler, unedited, built as "
                           "casual_fps_inference.py:512-521 builds it); make_golden_dpmpp.py sched",
               toy=dict(shape=TOY_SHAPE, x_seed=5, target_seed=6))
    x_init, target = philox_normal(TOY_SHAPE, 5, BF), philox_normal(TOY_SHAPE, 6, BF)
    for steps, shift in SCHEDULES:
        s = build_scheduler(fm, steps, shift)
        sig = s.sigmas.clone()
        sc = [step_scalars(sig, i, steps) for i in range(steps)]
        e = dict(steps=steps, shift=shift, timesteps=s.timesteps.clone(), sigmas=sig,
                 **{k: torch.tensor([c[k] for c in sc], dtype=torch.int32 if k == "order" else torch.float32) for k in sc[0]})
        for gpu in (False, True):
            s = build_scheduler(fm, steps, shift, gpu_scalars=gpu)
            x, m0, flows, traj = x_init.clone(), torch.zeros(TOY_SHAPE), [], []
            for i, t in enumerate(s.timesteps):
                v = (x - target) * (1.0 + 0.1 * torch.sin(x.float() * 3 + i).to(BF))
                xr = s.step(v, t, x, return_dict=False)[0]
                assert type(xr) is torch.Tensor and xr.dtype == BF and torch.isfinite(xr.float()).all()
                xe, m0 = chain(sc[i], v, x, m0, gpu)
                assert torch.equal(xe.view(torch.int16), xr.view(torch.int16)), (steps, gpu, i)
                flows.append(v.clone())
                traj.append(xr.clone())
                x = xr
            key = "gpu" if gpu else "cpu"
            e[f"flow_{key}"], e[f"traj_{key}"] = torch.stack(flows), torch.stack(traj)
        d = (e["traj_gpu"].float() - e["traj_cpu"].float()).abs().max().item()
        assert d > 0, "the shim changed nothing"
        print(f"[dpmpp sched] {steps} steps, shift {shift}: timesteps {e['timesteps'][:3].tolist()} .. {e['timesteps'][-2:].tolist()}; the kernel's chain "
              f"equals the reference's step bit for bit on all {steps} steps under both scalar semantics; GPU- vs CPU-semantics trajectory max|d| = {d:.3e}")
        out[f"s{steps}"] = e
    torch.save(out, os.path.join(HERE, "dpmpp_sched.pt"))


class _DpmAsTheStageLoopBuildsIt:
    """What make_golden._ref_stage_loop asks of its `unipc` module, answered with the reference's DPM-Solver++ scheduler: the
    constructor call and `set_timesteps(steps, device=, shift=)` become casual_fps_inference.py:512-521; `sigmas`, `timesteps` and
    `step` are the reference object's own."""

    fm = None

    def __init__(self, **kw):
        self._s = self.fm.FlowDPMSolverMultistepScheduler(**kw)

    def set_timesteps(self, steps, device=None, shift=None):
        self.fm.retrieve_timesteps(self._s, device=device, sigmas=self.fm.get_sampling_sigmas(steps, shift))

    sigmas = property(lambda self: self._s.sigmas, lambda self, v: setattr(self._s, "sigmas", v))
    timesteps = property(lambda self: self._s.timesteps)

    def step(self, *a, **kw):
        return self._s.step(*a, **kw)


def gen_chunk(steps=10):
    fm = load_dpm_reference()
    fps, _, _, _, _, sched = load_reference()
    _DpmAsTheStageLoopBuildsIt.fm = fm
    solver = types.SimpleNamespace(FlowUniPCMultistepScheduler=_DpmAsTheStageLoopBuildsIt)
    meta = dict(cfg="tiny", weight_seed=2, ctx_seeds=(21, 22), n_valid=(40, 12), noise_seed=23, renoise_seed_base=100, steps=steps,
                guidance=5.0, shift=5.0, sample_solver="dpm++", lat=(MG.H, MG.Wd), out_stride=(4, 4), handoff_stride=(4, 4))
    cfg, ctxs, noise, renoise = MG._chunk_inputs(meta)
    mdl, _, _ = MG.build_ref_model(fps, meta["cfg"], seed=meta["weight_seed"])
    t0 = time.time()
    tick = lambda tag: (lambda si: print(f"[dpmpp chunk] {tag}: stage {si} done at {time.time() - t0:.0f}s", flush=True))
    out, hand = MG._ref_stage_loop(mdl, fps, solver, sched, cfg, noise.clone(), renoise, ctxs, steps, progress=tick("reference"), gpu_scalars=True)
    real_attention = fps.attention

    def permuted_attention(q, k, v, *a, **kw):
        n = k.shape[1] // MG.S480
        idx = torch.arange(n * MG.S480).view(n, MG.S480).flip(0).reshape(-1)
        return real_attention(q, k[:, idx], v[:, idx], *a, **kw)

    fps.attention = permuted_attention
    p_out, p_hand = MG._ref_stage_loop(mdl, fps, solver, sched, cfg, noise.clone(), renoise, ctxs, steps, progress=tick("K/V order reversed"),
                                       gpu_scalars=True)
    fps.attention = real_attention
    assert torch.isfinite(out.float()).all() and hand.shape == (1, 8, 16, MG.H, MG.Wd)
    nf = dict(order_out=MG.rel_l2(p_out, out), order_handoff=MG.rel_l2(p_hand, hand))
    print(f"[dpmpp chunk] {steps} steps per stage at {MG.H}x{MG.Wd}: {time.time() - t0:.0f}s  rms={out.float().pow(2).mean().sqrt().item():.3f}  the reference vs "
          f"itself with the K/V frame order reversed: out={nf['order_out']:.3e} handoff={nf['order_handoff']:.3e}", flush=True)
    torch.save(dict(out_sha=MG.sha(out), out_strided=out[..., ::4, ::4].clone(), handoff_sha=MG.sha(hand), handoff_strided=hand[..., ::4, ::4].clone(),
                    noise_floor=nf, meta=meta,
                    produced_by="the REAL reference (CausalFPSWanModel + FlowDPMSolverMultistepScheduler.step, unedited, built as "
                                "casual_fps_inference.py:512-521 builds it) with scheduler.sigmas carrying make_golden._GpuScalar; "
                                "make_golden_dpmpp.py chunk"),
               os.path.join(HERE, "chunk_t2v_tiny_dpmpp.pt"))


if __name__ == "__main__":
    what = sys.argv[1:] or ["sched", "chunk"]
    if "sched" in what:
        gen_sched()
    if "chunk" in what:
        gen_chunk()
