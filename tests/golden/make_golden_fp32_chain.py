"""Golden fixture of upstream Wan2.1's float32 latent chain from the REAL reference, on the CPU: its two multistep schedulers on
float32 samples (wan/utils/fm_solvers_unipc.py, wan/utils/fm_solvers.py), `WanT2V.generate` (wan/text2video.py) around a tiny
WanModel, and the latent geometry `WanI2V.generate` (wan/image2video.py) derives.  Build-container only (the reference never
travels to the GPU box).

    python tests/golden/make_golden_fp32_chain.py

Writes tests/golden/fp32_chain.pt (tensors, numbers and short labels only):
  sched[solver][f"s{steps}"]   open-loop solver trajectories, solver in ('unipc', 'dpm++'), (steps, shift) in ((50, 5.0), (6, 8.0)),
      guidance 5, n = 768 elements: `x0` the float32 start, `flow_cond` / `flow_uncond` bf16 [steps, n] as fed to every step, `x`
      float32 [steps, n] the REAL scheduler's sample after every step, built and called the way text2video.py:202-250 does
      (float32 CFG combine, `step(noise_pred.unsqueeze(0), t, latents.unsqueeze(0))`).  The flows are a deterministic toy field
      evaluated on the trajectory itself and recorded, so a replay is open-loop and can be exact.  `rho_c` float32 [steps, 2]: what
      the scheduler's `torch.linalg.solve(R, b)` returned at each step that called it (UniPC's order-2 corrector; zeros elsewhere)
      -- its float32 bits depend on the machine (LAPACK picks its kernels by CPU).  `rows` {field: [steps]}: every per-step scalar
      of the schedule (the fields of MmplUniPCStepF32 / MmplDpmppStep) as the reference's 0-dim float32 expressions give them ON
      THE MACHINE THAT MADE THIS FIXTURE -- torch.log / torch.expm1 / torch.exp are dispatched by CPU too, and their last bits
      (amplified by the cancellation in lambda_t - lambda_s) differ between hosts -- computed by mmpl_amd/scheduler.py and checked
      here to reproduce the trajectory bit for bit, so that a replay elsewhere can use the bits this trajectory was made with.
  generate[solver]             the real `WanT2V.generate` on an object made with object.__new__: the tiny WanModel of
      make_golden_bidir.py (weights from seed) behind the two casts autocast performs at the model's boundary (input -> bf16,
      output -> float32), a text encoder returning fixed contexts, a VAE whose decode returns its input, offload_model=False, 21
      latent frames at 16 x 24 latents, 6 steps, shift 5.0, guidance 5.  `torch.randn` inside generate() is answered with
      mmpl_amd.synthetic.philox_normal(shape, noise_seed) in float32 (the tests regenerate it; `noise_sha` is the sha256 of the
      model's first input, which is checked here to be that noise); `out_strided` / `out_sha`: the final float32 latents
      [16, 21, 16, 24]; `order_out`: rel-L2 to the same run with the self-attention's keys in reverse frame order, the
      reference's own order noise.
  i2v_geometry                 rows (img_h, img_w, max_area, lat_h, lat_w): the noise shape the real `WanI2V.generate` draws
      (image2video.py:177-205) for each image size and max_area.
"""
import importlib
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import load_reference  # noqa: E402
from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal  # noqa: E402

torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHEDULES = ((50, 5.0), (6, 8.0))
GUIDANCE = 5.0
TOY_SHAPE = [16, 3, 4, 4]                              # 768 elements
H, Wd, F_ = 16, 24, 21
S = (H // 2) * (Wd // 2)
I2V_IMAGES = ((720, 1280), (1280, 720), (480, 832), (1024, 1024), (333, 500))
I2V_AREAS = (720 * 1280, 480 * 832)


def sha(t):
    import hashlib
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_upstream():
    """wan.text2video / wan.image2video next to what load_reference() imports."""
    load_reference()
    _stub("diffusers.utils.torch_utils", randn_tensor=None)             # fm_solvers: the SDE variants' noise, never called
    for name in ("ftfy", "easydict"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                _stub(name)
    fm = importlib.import_module("wan.utils.fm_solvers")
    unipc = importlib.import_module("wan.utils.fm_solvers_unipc")
    real_current = torch.cuda.current_device                           # wan/modules/t5.py:478 calls it in a default argument
    torch.cuda.current_device = lambda: 0
    try:
        t2v = importlib.import_module("wan.text2video")
    finally:
        torch.cuda.current_device = real_current
    try:                                                              # (after transformers, which looks torchvision up by its spec)
        importlib.import_module("torchvision.transforms.functional")
    except ImportError:
        _stub("torchvision")
        _stub("torchvision.transforms")
        sys.modules["torchvision.transforms"].functional = _stub("torchvision.transforms.functional", to_tensor=None)
    i2v = importlib.import_module("wan.image2video")
    return fm, unipc, t2v, i2v


def build_scheduler(fm, unipc, solver, steps, shift):
    """text2video.py:202-221, literally."""
    if solver == "unipc":
        s = unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(steps, device="cpu", shift=shift)
        return s, s.timesteps
    s = fm.FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    timesteps, _ = fm.retrieve_timesteps(s, device="cpu", sigmas=fm.get_sampling_sigmas(steps, shift))
    return s, timesteps


def gen_sched(fm, unipc):
    out = {}
    x_init = philox_normal(TOY_SHAPE, 5, torch.float32)
    tc, tu = philox_normal(TOY_SHAPE, 6, torch.float32), philox_normal(TOY_SHAPE, 7, torch.float32)
    for solver in ("unipc", "dpm++"):
        out[solver] = {}
        for steps, shift in SCHEDULES:
            s, timesteps = build_scheduler(fm, unipc, solver, steps, shift)
            x, fcs, fus, traj = x_init.clone(), [], [], []
            solved, rho_c = [], torch.zeros(steps, 2)
            real_solve = torch.linalg.solve
            torch.linalg.solve = lambda A, B: (solved.append(real_solve(A, B).clone()), solved[-1])[1]
            for i, t in enumerate(timesteps):
                n_solved = len(solved)
                wob = 1.0 + 0.1 * torch.sin(x * 3 + i)
                fc, fu = ((x - tc) * wob).to(BF), ((x - tu) * (2.0 - wob)).to(BF)
                cond, uncond = fc.float(), fu.float()                     # the forward's output, `.float()`ed
                noise_pred = uncond + GUIDANCE * (cond - uncond)          # text2video.py:241-242
                x = s.step(noise_pred.unsqueeze(0), t, x.unsqueeze(0), return_dict=False)[0].squeeze(0)
                assert x.dtype == torch.float32 and torch.isfinite(x).all()
                if len(solved) > n_solved:                                # the order-2 corrector's rhos_c, as LAPACK returned them here
                    assert len(solved) == n_solved + 1 and solved[-1].dtype == torch.float32 and solved[-1].shape == (2,)
                    rho_c[i] = solved[-1]
                fcs.append(fc.reshape(-1).clone())
                fus.append(fu.reshape(-1).clone())
                traj.append(x.reshape(-1).clone())
            torch.linalg.solve = real_solve
            assert len(solved) == (max(steps - 2, 0) if solver == "unipc" else 0)
            rows = scalar_rows(solver, steps, shift, fcs, fus, x_init.reshape(-1), traj, rho_c)
            out[solver][f"s{steps}"] = dict(steps=steps, shift=shift, guidance=GUIDANCE, x0=x_init.reshape(-1).clone(), rho_c=rho_c, rows=rows,
                                            timesteps=torch.as_tensor(timesteps).clone(), flow_cond=torch.stack(fcs),
                                            flow_uncond=torch.stack(fus), x=torch.stack(traj))
            print(f"[sched {solver}] {steps} steps, shift {shift}: |x_final| rms {traj[-1].pow(2).mean().sqrt().item():.3f}, "
                  f"timesteps {torch.as_tensor(timesteps)[:2].tolist()} .. {torch.as_tensor(timesteps)[-1:].tolist()}")
    return out


def scalar_rows(solver, steps, shift, fcs, fus, x0, traj, rho_c):
    """The per-step float32 scalars of this schedule as computed ON THIS MACHINE (mmpl_amd/scheduler.py: the reference's own 0-dim
    torch expressions), {field: tensor [steps]}.  They are the reference's: checked here by replaying tests/fp32_chain_ref.py with
    them against the reference's trajectory, bit for bit at every step, and against the rhos its `torch.linalg.solve` returned."""
    from mmpl_amd.pipeline._common import make_sample_scheduler
    from tests import fp32_chain_ref as R
    s, _ = make_sample_scheduler(solver, 1000, steps, shift, "cpu")
    s._ensure_state(torch.zeros(1, dtype=torch.float32))
    rows = [s.step_scalars(GUIDANCE) for _ in range(steps)]
    x = x0.clone()
    m0, m1, last = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for i, st in enumerate(rows):
        if solver == "unipc":
            x, m0, m1, last = R.unipc_f32(st, fcs[i], fus[i], x, m0, m1, last)
            if st.use_corrector and st.corr_order == 2:
                assert (st.c_rho0, st.c_rho_last) == (rho_c[i, 0].item(), rho_c[i, 1].item()), i
        else:
            x, m0, m1 = R.dpmpp_f32(st, fcs[i], fus[i], x, m0, m1)
        assert torch.equal(x.view(torch.int32), traj[i].view(torch.int32)), (solver, steps, i)
    return {f: torch.tensor([getattr(r, f) for r in rows], dtype=torch.int32 if isinstance(getattr(rows[0], f), int) else torch.float32)
            for f, _ in rows[0]._fields_}


class _AutocastBoundary(torch.nn.Module):
    """The two casts autocast performs at the model's boundary: the float32 latents enter the patch embedding as bf16, the output is
    `.float()`ed (wan/modules/model.py's forward ends in `[u.float() for u in x]`)."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.first_input = None

    def forward(self, x, t, context, seq_len, **kw):
        if self.first_input is None:
            self.first_input = x[0].clone()
        out = self.model([u.to(BF) for u in x], t=t.to(torch.float32), context=[c.to(BF) for c in context], seq_len=seq_len, **kw)
        return [u.float() for u in out]


def tiny_model(model, seed):
    """The tiny WanModel as make_golden_bidir.tiny_wrapper builds it."""
    cfg = WAN_CONFIGS["tiny"]
    m = model.WanModel(model_type="t2v", dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"],
                       num_layers=cfg["num_layers"], text_dim=cfg["text_dim"], freq_dim=cfg["freq_dim"]).eval()
    m.load_state_dict(dit_state_dict(cfg, seed=seed), strict=True)
    return m.to(BF), cfg


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


def gen_generate(model, t2v, solver):
    seeds = dict(weights=71, ctx=72, n_valid=40, neg=73, n_valid_neg=17, noise=75)
    steps, shift = 6, 5.0
    m, cfg = tiny_model(model, seeds["weights"])
    ctx = philox_normal([512, cfg["text_dim"]], seeds["ctx"])[:seeds["n_valid"]]
    neg = philox_normal([512, cfg["text_dim"]], seeds["neg"])[:seeds["n_valid_neg"]]
    noise = philox_normal([16, F_, H, Wd], seeds["noise"], torch.float32)

    class Text:
        model = torch.nn.Identity()

        def __call__(self, texts, device):
            return [neg.clone() if texts[0] == "NEG" else ctx.clone()]

    class VAE:
        model = types.SimpleNamespace(z_dim=16)

        def decode(self, zs):
            return zs

    def run():
        wan = object.__new__(t2v.WanT2V)
        wan.device, wan.rank, wan.t5_cpu, wan.sp_size = torch.device("cpu"), 0, False, 1
        wan.num_train_timesteps, wan.param_dtype = 1000, BF
        wan.vae_stride, wan.patch_size = (4, 8, 8), (1, 2, 2)
        wan.text_encoder, wan.vae, wan.model = Text(), VAE(), _AutocastBoundary(m)
        wan.sample_neg_prompt = "NEG"
        real = torch.randn
        torch.randn = lambda *shape, **kw: philox_normal(list(shape), seeds["noise"], kw["dtype"])
        try:
            out = wan.generate("p", size=(Wd * 8, H * 8), frame_num=(F_ - 1) * 4 + 1, shift=shift, sample_solver=solver,
                               sampling_steps=steps, guide_scale=GUIDANCE, n_prompt="", seed=1, offload_model=False)
        finally:
            torch.randn = real
        return out, wan.model.first_input

    out, first = run()
    assert out.dtype == torch.float32 and out.shape == (16, F_, H, Wd) and torch.isfinite(out).all()
    assert first.dtype == torch.float32 and torch.equal(first, noise), "the model's first input is not the noise"
    perm, _ = with_reversed_keys(model, run)
    order = rel_l2(perm, out)
    print(f"[generate {solver}] out {tuple(out.shape)} rms={out.pow(2).mean().sqrt().item():.3f}  K/V order noise rel_l2={order:.3e}")
    return dict(out_strided=out[..., ::2, ::2].clone(), out_sha=sha(out), order_out=order, noise_sha=sha(noise),
                meta=dict(cfg="tiny", weight_seed=seeds["weights"], ctx_seed=seeds["ctx"], n_valid=seeds["n_valid"], neg_seed=seeds["neg"],
                          n_valid_neg=seeds["n_valid_neg"], noise_seed=seeds["noise"], F=F_, lat_hw=(H, Wd), guide_scale=GUIDANCE,
                          sampling_steps=steps, sample_solver=solver, shift=shift, num_train_timesteps=1000))


class _NoiseDrawn(Exception):
    pass


def gen_i2v_geometry(i2v):
    """(lat_h, lat_w) of the noise the real WanI2V.generate draws: its own arithmetic (image2video.py:177-205) up to torch.randn."""
    wan = object.__new__(i2v.WanI2V)
    wan.device, wan.vae_stride, wan.patch_size, wan.sp_size = torch.device("cpu"), (4, 8, 8), (1, 2, 2), 1
    rows = []

    def randn(*shape, **kw):
        raise _NoiseDrawn(shape)

    real_randn, real_tf = torch.randn, i2v.TF.to_tensor
    torch.randn, i2v.TF.to_tensor = randn, (lambda img: img)
    try:
        for ih, iw in I2V_IMAGES:
            for area in I2V_AREAS:
                try:
                    wan.generate("p", torch.zeros(3, ih, iw), max_area=area, sampling_steps=1, seed=1, offload_model=False)
                    raise AssertionError("generate() drew no noise")
                except _NoiseDrawn as e:
                    c, f, lat_h, lat_w = e.args[0]
                    assert (c, f) == (16, 21)
                    rows.append((ih, iw, area, lat_h, lat_w))
    finally:
        torch.randn, i2v.TF.to_tensor = real_randn, real_tf
    print("[i2v geometry]", rows)
    return torch.tensor(rows, dtype=torch.int64)


def main():
    fm, unipc, t2v, i2v = load_upstream()
    model = sys.modules["wan.modules.model"]
    out = dict(produced_by="the REAL reference (wan/utils/fm_solvers_unipc.py, wan/utils/fm_solvers.py, wan/text2video.py WanT2V.generate, "
                           "wan/image2video.py WanI2V.generate, unedited); make_golden_fp32_chain.py",
               sched=gen_sched(fm, unipc), i2v_geometry=gen_i2v_geometry(i2v),
               generate={solver: gen_generate(model, t2v, solver) for solver in ("unipc", "dpm++")})
    path = os.path.join(HERE, "fp32_chain.pt")
    torch.save(out, path)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
