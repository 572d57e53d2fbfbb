"""Flow-matching samplers of the denoise loop, MI355X host side.

``FlowUniPCMultistepScheduler`` keeps the reference's name and call shape
(MMPL_t2v/wan/utils/fm_solvers_unipc.py:20-800 as configured by
pipeline/casual_fps_inference.py:503-511: order 2, bh2, predict_x0, flow_prediction, lower_order_final,
final sigma 0) but splits the work the MI355X way: the per-step *scalars* (sigma ratios, h, expm1 terms,
rho coefficients -- a handful of fp32 values) are computed on the host exactly as the reference computes
them, and the whole tensor update (CFG combine, x0 conversion, UniC corrector, UniP predictor, solver-state
rotation) is ONE fused HIP kernel (``mmpl_cfg_unipc_step``) instead of ~25 tiny PyTorch launches.

``FlowDPMSolverMultistepScheduler`` (with ``get_sampling_sigmas`` / ``retrieve_timesteps``) is the reference's other solver,
``sample_solver = 'dpm++'`` (MMPL_t2v/wan/utils/fm_solvers.py as configured by pipeline/casual_fps_inference.py:512-521), split the
same way around ``mmpl_cfg_dpmpp_step`` and with the same device-facing interface, so the stage loop drives either object.

Both classes have two modes, chosen by the dtype of the sample their solver state is built for (``_solver_state``): bfloat16 is
the reference pipelines' chain (a bf16 rounding after every tensor operation), float32 is upstream Wan2.1's ``WanT2V.generate`` /
``WanI2V.generate`` chain -- float32 sample and solver state, ``mmpl_cfg_unipc_step_f32`` / ``mmpl_cfg_dpmpp_step_f32``, the same
scalar expressions with ``rk`` itself in place of ``1 / rk`` and rhos that are not rounded to bf16.

``FlowMatchScheduler`` is the train-time schedule the pipeline uses for ``add_noise``
(MMPL_t2v/utils/scheduler.py:103-176).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib


def _solver_state(sched, sample: torch.Tensor, n_tensors: int) -> None:
    """THE place where a scheduler's mode is chosen: by the dtype of the sample its solver state is built for.  bfloat16 = the
    reference pipelines' chain (a bf16 rounding after every tensor operation); float32 = upstream Wan2.1's (`WanT2V.generate`:
    float32 latents and solver state, ``mmpl_cfg_*_step_f32``).  `step_scalars` and `build_step_table` read `sched.latent_dtype`, so
    a table is built after the state (`_ensure_state(sample)` first)."""
    if sample.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{type(sched).__name__}: the sample is {sample.dtype}; bfloat16 or float32")
    st = sched._state
    if st is None or st[0].shape != sample.shape or st[0].device != sample.device or st[0].dtype != sample.dtype:
        sched._state = [torch.zeros_like(sample) for _ in range(n_tensors)]
    sched.latent_dtype = sample.dtype


def _shadow_ptr(sample: torch.Tensor, sample_bf16: Optional[torch.Tensor]):
    """The bf16 shadow of a float32 sample (None = not wanted) as the x_bf16 argument."""
    if sample_bf16 is not None:
        assert sample_bf16.dtype == torch.bfloat16 and sample_bf16.is_contiguous() and sample_bf16.numel() == sample.numel()
    return _lib.ptr(sample_bf16)


def _table_rows(sched, guidance: float, device) -> None:
    """`build_step_table` of both solvers: the scalars of every remaining step from a copy of `sched` (its own bookkeeping does not
    advance), in the struct of its mode, and the timestep of every step."""
    import copy
    probe = copy.copy(sched)
    probe._state = None
    n = len(sched.timesteps) - sched.step_index
    first = probe.step_scalars(guidance)
    rows = (type(first) * n)()
    rows[0] = first
    for i in range(1, n):
        rows[i] = probe.step_scalars(guidance)
    raw = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).clone()
    sched._table = raw.to(device)
    sched._table_dtype = sched.latent_dtype
    t_host = [float(t) for t in sched.timesteps[sched.step_index:]]
    sched._t_table = torch.tensor(t_host, dtype=torch.float32, device=device)
    sched._t_first = t_host[0]          # host copy: reset_step_table must not read the device table (a sync inside timed loops)
    sched._counter = torch.zeros(1, dtype=torch.int32, device=device)
    sched._table_n = n


def _check_table_call(sched, sample: torch.Tensor, timestep: torch.Tensor) -> None:
    assert sample.is_contiguous() and timestep.dtype == torch.float32 and timestep.is_contiguous()
    if sched._table_dtype != sample.dtype:
        raise TypeError(f"{type(sched).__name__}: the step table was built for a {sched._table_dtype} sample, this one is {sample.dtype}")


class _DeviceSolver:
    """The device-facing half of both schedulers: the solver state, the fused step and the device-resident step table.  A subclass
    sets `_n_state` (state tensors of the sample's shape and dtype: m0, m1 and, for UniPC, last_sample) and `_stem` -- the C entry is
    ``mmpl_cfg_{_stem}_step{_f32}{_table}`` -- and has `step_scalars(guidance)`, `sigmas`, `timesteps` and `step_index`."""
    order = 1
    latent_dtype = torch.bfloat16         # the mode: set by _ensure_state from the sample (see _solver_state)
    _n_state: int
    _stem: str

    def _train_sigmas(self, num_train_timesteps: int, shift: float) -> None:
        """The constructor's schedule: the train-time sigmas under `shift`, until `set_timesteps` replaces them."""
        alphas = np.linspace(1, 1 / num_train_timesteps, num_train_timesteps)[::-1].copy()
        sigmas = torch.from_numpy(1.0 - alphas).to(dtype=torch.float32)
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)               # shift 1: unchanged, bit for bit
        self.num_train_timesteps = num_train_timesteps
        self.sigmas = sigmas
        self.sigma_min = self.sigmas[-1].item()
        self.sigma_max = self.sigmas[0].item()
        self.timesteps = sigmas * num_train_timesteps
        self.num_inference_steps = None
        self._state = None

    def _inference_sigmas(self, sigmas: np.ndarray, shift: float) -> None:
        """`set_timesteps`: `sigmas` (numpy, without the trailing 0) under `shift` become the schedule; the step count rewinds."""
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        timesteps = sigmas * self.num_train_timesteps
        sigmas = np.concatenate([sigmas, [0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas)                       # stays on the host, like the reference
        self.timesteps = torch.from_numpy(timesteps).to(dtype=torch.int64)      # truncated: the first one is 1000
        self.num_inference_steps = len(timesteps)
        self.step_index = 0
        self._state = None

    @staticmethod
    def _lam(sigma):
        return torch.log(1 - sigma) - torch.log(sigma)

    # -- device update -----------------------------------------------------------------------------
    def _ensure_state(self, sample: torch.Tensor):
        _solver_state(self, sample, self._n_state)

    def _call(self, table: bool, flow_cond, flow_uncond, sample: torch.Tensor, sample_bf16, *tail) -> None:
        """One of the four entries of this solver: `tail` is what follows n in its signature, without the stream."""
        f32 = sample.dtype == torch.float32
        assert f32 or sample_bf16 is None, "sample_bf16 is the shadow of a float32 sample"
        name = f"mmpl_cfg_{self._stem}_step" + ("_f32" if f32 else "") + ("_table" if table else "")
        shadow = (_shadow_ptr(sample, sample_bf16),) if f32 else ()
        _lib.check(getattr(_lib.load(), name)(_lib.ptr(flow_cond), _lib.ptr(flow_uncond), _lib.ptr(sample),
                                              *[_lib.ptr(t) for t in self._state], *shadow, sample.numel(), *tail, _lib.stream_ptr()), name)

    def step_cfg(self, flow_cond: torch.Tensor, flow_uncond: Optional[torch.Tensor], guidance: float,
                 sample: torch.Tensor, sample_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
        """CFG combine + scheduler step, fused; `sample` is updated in place and returned.  The flows are bf16.  A float32 `sample`
        takes the float32 chain (DPM-Solver++: the same scalars, the reference multiplies by 1.0 / r0 there too); `sample_bf16`
        (optional) then receives the bf16 rounding of the new sample."""
        assert sample.is_contiguous() and flow_cond.is_contiguous() and flow_cond.dtype == torch.bfloat16
        self._ensure_state(sample)
        st = self.step_scalars(guidance)
        self._call(False, flow_cond, flow_uncond, sample, sample_bf16, C.byref(st))
        return sample

    # -- device-resident step table: one hipGraph per denoise step, replayed with no host work in between --------------
    def build_step_table(self, guidance: float, device) -> None:
        """Upload the scalars of ALL remaining steps (they depend only on the step index, never on data) plus the timestep
        of every step; `step_cfg_table` then reads entry *counter on the device.  The host-side step bookkeeping of THIS
        object is not advanced (the scalars come from a copy): after the table's last step the device kernel does nothing
        (the counter is clamped), `reset_step_table` rewinds it for another pass over the same schedule.  The rows are those of
        the mode `_ensure_state` chose (bf16 unless it has been called with a float32 sample)."""
        _table_rows(self, guidance, device)

    def reset_step_table(self, timestep: torch.Tensor) -> None:
        """Rewind the device step counter, the solver history and `timestep` to the first entry of the uploaded table."""
        self._counter.zero_()
        if self._state is not None:
            for t in self._state:
                t.zero_()
        timestep.fill_(self._t_first)

    def step_cfg_table(self, flow_cond: torch.Tensor, flow_uncond: torch.Tensor, sample: torch.Tensor, timestep: torch.Tensor,
                       sample_bf16: Optional[torch.Tensor] = None) -> None:
        """CFG combine + scheduler step with device-resident scalars (capturable: no host value enters the launch);
        advances the device step counter and writes the next step's timestep into `timestep` (float32, contiguous).  A float32
        `sample` (the table was built for one) takes the float32 chain and writes its bf16 rounding to `sample_bf16`."""
        _check_table_call(self, sample, timestep)
        self._ensure_state(sample)
        self._call(True, flow_cond, flow_uncond, sample, sample_bf16, _lib.ptr(self._table), _lib.ptr(self._counter), _lib.ptr(timestep),
                   _lib.ptr(self._t_table), timestep.numel(), self._table_n)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True):
        """Reference call shape (fm_solvers_unipc.py:655, fm_solvers.py:706).  `timestep` is accepted and ignored: the steps are
        counted, as the reference's internal step counter does after the first call."""
        out = self.step_cfg(model_output.to(torch.bfloat16).contiguous(), None, 0.0, sample.contiguous().clone())   # (flows are bf16)
        return (out,) if not return_dict else {"prev_sample": out}


class FlowUniPCMultistepScheduler(_DeviceSolver):
    _n_state, _stem = 3, "unipc"          # m0, m1, last_sample

    def __init__(self, num_train_timesteps: int = 1000, solver_order: int = 2, shift: float = 1.0,
                 use_dynamic_shifting: bool = False):
        assert solver_order == 2 and not use_dynamic_shifting
        self.solver_order = solver_order
        self.shift = shift
        self._train_sigmas(num_train_timesteps, shift)

    def set_timesteps(self, num_inference_steps: int, device=None, shift: Optional[float] = None):
        sigmas = np.linspace(self.sigma_max, self.sigma_min, num_inference_steps + 1).copy()[:-1]
        self._inference_sigmas(sigmas, self.shift if shift is None else shift)
        self.lower_order_nums = 0
        self.this_order = 1
        self._have_last = False

    # -- host scalars ------------------------------------------------------------------------------
    def _corrector_scalars(self, order: int):
        """fm_solvers_unipc.py:549-618."""
        si = self.step_index
        sigma_t, sigma_s0 = self.sigmas[si], self.sigmas[si - 1]
        alpha_t = 1 - sigma_t
        h = self._lam(sigma_t) - self._lam(sigma_s0)
        rks = []
        inv_rk, rk_f = 0.0, 1.0
        if order == 2:
            rk = (self._lam(self.sigmas[si - 2]) - self._lam(sigma_s0)) / h
            rks.append(rk)
            inv_rk, rk_f = (1.0 / rk).item(), rk.item()
        rks.append(1.0)
        rks = torch.tensor(rks)
        hh = -h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = torch.expm1(hh)
        factorial_i = 1
        R, b = [], []
        for i in range(1, order + 1):
            R.append(torch.pow(rks, i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1 / factorial_i
        if order == 1:                                                 # `.to(x.dtype)`: float32 rhos for a float32 sample
            rhos = torch.tensor([0.5], dtype=self.latent_dtype)
        else:
            rhos = torch.linalg.solve(torch.stack(R), torch.tensor(b)).to(self.latent_dtype)
        return dict(c1=(sigma_t / sigma_s0).item(), c2=(alpha_t * h_phi_1).item(), c3=(alpha_t * B_h).item(), inv_rk=inv_rk, rk=rk_f,
                    rho0=rhos[0].float().item() if order == 2 else 0.0, rho_last=rhos[-1].float().item())

    def _predictor_scalars(self, order: int):
        """fm_solvers_unipc.py:402-476."""
        si = self.step_index
        sigma_t, sigma_s0 = self.sigmas[si + 1], self.sigmas[si]
        alpha_t = 1 - sigma_t
        h = self._lam(sigma_t) - self._lam(sigma_s0)
        inv_rk, rk_f = 0.0, 1.0
        if order == 2:
            rk = (self._lam(self.sigmas[si - 1]) - self._lam(sigma_s0)) / h
            inv_rk, rk_f = (1.0 / rk).item(), rk.item()
        hh = -h
        h_phi_1 = torch.expm1(hh)
        B_h = torch.expm1(hh)
        return dict(c1=(sigma_t / sigma_s0).item(), c2=(alpha_t * h_phi_1).item(), c3=(alpha_t * B_h).item(), inv_rk=inv_rk, rk=rk_f)

    def step_scalars(self, guidance: float):
        """Scalars of the step at the current step_index; advances the host-side order bookkeeping (:686-730).  A MmplUniPCStep, or
        in float32 mode a MmplUniPCStepF32: the same expressions, but rk itself where the bf16 struct carries 1 / rk (the kernel
        divides, as the reference does) and rhos that were never rounded to bf16."""
        si = self.step_index
        use_corr = si > 0 and self._have_last
        f32 = self.latent_dtype == torch.float32
        rk = "rk" if f32 else "inv_rk"
        st = (_lib.MmplUniPCStepF32 if f32 else _lib.MmplUniPCStep)()
        st.guidance = float(guidance)
        st.sigma_cur = self.sigmas[si].item()
        st.use_corrector = int(use_corr)
        st.corr_order = self.this_order
        if use_corr:
            c = self._corrector_scalars(self.this_order)
            st.c_c1, st.c_c2, st.c_c3, st.c_rho0, st.c_rho_last = c["c1"], c["c2"], c["c3"], c["rho0"], c["rho_last"]
            setattr(st, "c_" + rk, c[rk])
        this_order = min(self.solver_order, len(self.timesteps) - si)
        self.this_order = min(this_order, self.lower_order_nums + 1)
        p = self._predictor_scalars(self.this_order)
        st.pred_order = self.this_order
        st.p_c1, st.p_c2, st.p_c3 = p["c1"], p["c2"], p["c3"]
        setattr(st, "p_" + rk, p[rk])
        self._have_last = True
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return st


def get_sampling_sigmas(sampling_steps: int, shift: float) -> np.ndarray:
    """fm_solvers.py:22-26: the shifted sigmas of a `sampling_steps`-step schedule from 1 down (fp64, without the trailing 0)."""
    sigma = np.linspace(1, 0, sampling_steps + 1)[:sampling_steps]
    return shift * sigma / (1 + (shift - 1) * sigma)


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, sigmas=None, **kwargs):
    """fm_solvers.py:29-66 for the one form the pipeline uses: custom `sigmas`.  -> (timesteps, number of steps).  `device` is
    passed on and ignored there: the timesteps stay on the host."""
    if timesteps is not None:
        raise ValueError("retrieve_timesteps: custom `timesteps` are not supported, pass `sigmas`")
    if sigmas is None:
        raise ValueError("retrieve_timesteps: pass `sigmas` (get_sampling_sigmas(steps, shift))")
    scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
    return scheduler.timesteps, len(scheduler.timesteps)


class FlowDPMSolverMultistepScheduler(_DeviceSolver):
    """DPM-Solver++(2M) for flow matching: the reference's second sampler (MMPL_t2v/wan/utils/fm_solvers.py:69-797) in the one
    configuration its pipeline builds (pipeline/casual_fps_inference.py:512-521: order 2, dpmsolver++, midpoint, flow_prediction,
    final sigma 0, no thresholding, config shift 1 with the schedule's shift applied by `get_sampling_sigmas`).  Every other
    constructor value raises.

    Split like the UniPC class above: the per-step scalars (sigma ratio, alpha_t (exp(-h) - 1), 1 / r0) are computed on the host with
    the reference's own torch fp32 0-dim tensor operations, the tensor update (CFG combine, x0 conversion, history rotation, first /
    second order update) is ONE fused HIP kernel (``mmpl_cfg_dpmpp_step``), and the device-facing interface is the UniPC class's, so
    the stage loop drives either object.  The solver state is two tensors of the sample's dtype (m0, m1); there is no corrector and no last sample."""
    _n_state, _stem = 2, "dpmpp"          # m0, m1
    _SUPPORTED = dict(solver_order=2, prediction_type="flow_prediction", shift=1.0, use_dynamic_shifting=False, thresholding=False,
                      algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                      final_sigmas_type="zero", lambda_min_clipped=-float("inf"), variance_type=None, invert_sigmas=False)

    def __init__(self, num_train_timesteps: int = 1000, solver_order: int = 2, prediction_type: str = "flow_prediction",
                 shift: Optional[float] = 1.0, use_dynamic_shifting: bool = False, thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, euler_at_final: bool = False,
                 final_sigmas_type: Optional[str] = "zero", lambda_min_clipped: float = -float("inf"),
                 variance_type: Optional[str] = None, invert_sigmas: bool = False):
        given = dict(solver_order=solver_order, prediction_type=prediction_type, shift=shift, use_dynamic_shifting=use_dynamic_shifting,
                     thresholding=thresholding, algorithm_type=algorithm_type, solver_type=solver_type,
                     lower_order_final=lower_order_final, euler_at_final=euler_at_final, final_sigmas_type=final_sigmas_type,
                     lambda_min_clipped=lambda_min_clipped, variance_type=variance_type, invert_sigmas=invert_sigmas)
        for k, v in given.items():                    # (the two thresholding parameters have no effect without thresholding)
            if v != self._SUPPORTED[k]:
                raise NotImplementedError(f"FlowDPMSolverMultistepScheduler: {k}={v!r} is not supported (only {self._SUPPORTED[k]!r}: "
                                          "the configuration the pipeline builds)")
        self.solver_order = solver_order
        self._train_sigmas(num_train_timesteps, 1.0)
        self.step_index = 0

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, sigmas=None, mu=None, shift: Optional[float] = None):
        """fm_solvers.py:226-287.  `sigmas` (fp64, from get_sampling_sigmas: already shifted) are taken as they are -- the config's
        shift is 1; without them the schedule is the linear one from sigma_max to sigma_min under `shift`.  `device` is accepted for
        the reference's call shape and ignored: `sigmas` and `timesteps` stay on the host (as in the UniPC class above), the stage
        loop reads them there without a device sync."""
        if mu is not None:
            raise NotImplementedError("FlowDPMSolverMultistepScheduler: dynamic shifting (mu) is not supported")
        if sigmas is None:
            if num_inference_steps is None:
                raise ValueError("set_timesteps: pass num_inference_steps or sigmas")
            sigmas = np.linspace(self.sigma_max, self.sigma_min, num_inference_steps + 1).copy()[:-1]
        sigmas = np.asarray(sigmas, dtype=np.float64)
        self._inference_sigmas(sigmas, 1.0 if shift is None else shift)

    # -- host scalars ------------------------------------------------------------------------------
    def step_scalars(self, guidance: float) -> _lib.MmplDpmppStep:
        """Scalars of the step at the current step_index (fm_solvers.py:457-468, 529-553, 746-783), then step_index += 1.
        The reference's own fp32 0-dim tensor operations, so the values are its bits; its three infinities stay on the host:
          step 0      sigma_s0 = 1: lambda_s0 = -inf, h = +inf, exp(-h) = 0                 -> c2 = -(1 - sigma_t)
          step 1      lambda_s1 = -inf: h_0 = +inf, r0 = +inf                               -> inv_r0 = 0 (D1 = +-0)
          last step   sigma_t = 0: lambda_t = +inf, h = +inf, c1 = 0                        -> c2 = -1: the result is m0
        Order: 1 on the first step (no history) and on the last (final sigma 0), else 2; with solver order 2 the reference's
        `lower_order_second` selects the branch that is taken anyway."""
        i, n = self.step_index, len(self.timesteps)
        if i >= n:
            raise IndexError(f"FlowDPMSolverMultistepScheduler: step {i} of a {n}-step schedule")
        sigma_t, sigma_s0 = self.sigmas[i + 1], self.sigmas[i]
        alpha_t = 1 - sigma_t
        lambda_t, lambda_s0 = self._lam(sigma_t), self._lam(sigma_s0)
        h = lambda_t - lambda_s0
        st = _lib.MmplDpmppStep()
        st.guidance = float(guidance)
        st.sigma_cur = sigma_s0.item()
        st.order = 1 if i == 0 or i == n - 1 else 2
        st.c1 = (sigma_t / sigma_s0).item()
        st.c2 = (alpha_t * (torch.exp(-h) - 1.0)).item()
        st.inv_r0 = 0.0
        if st.order == 2:
            h_0 = lambda_s0 - self._lam(self.sigmas[i - 1])
            st.inv_r0 = (1.0 / (h_0 / h)).item()
        if not all(np.isfinite(v) for v in (st.sigma_cur, st.c1, st.c2, st.inv_r0)):
            raise FloatingPointError(f"FlowDPMSolverMultistepScheduler: non-finite scalar at step {i}: "
                                     f"c1={st.c1} c2={st.c2} inv_r0={st.inv_r0}")
        self.step_index += 1
        return st


class FlowMatchScheduler:
    """utils/scheduler.py:103-176 (shift, sigma_min, extra_one_step) -- host-side, tiny."""

    def __init__(self, num_inference_steps=100, num_train_timesteps=1000, shift=3.0, sigma_max=1.0, sigma_min=0.003 / 1.002,
                 extra_one_step=False):
        self.num_train_timesteps, self.shift, self.sigma_max, self.sigma_min = num_train_timesteps, shift, sigma_max, sigma_min
        self.extra_one_step = extra_one_step
        self.set_timesteps(num_inference_steps)

    def set_timesteps(self, num_inference_steps=100, denoising_strength=1.0, training=False):
        sigma_start = self.sigma_min + (self.sigma_max - self.sigma_min) * denoising_strength
        if self.extra_one_step:
            self.sigmas = torch.linspace(sigma_start, self.sigma_min, num_inference_steps + 1)[:-1]
        else:
            self.sigmas = torch.linspace(sigma_start, self.sigma_min, num_inference_steps)
        self.sigmas = self.shift * self.sigmas / (1 + (self.shift - 1) * self.sigmas)
        self.timesteps = self.sigmas * self.num_train_timesteps

    def add_noise(self, original_samples, noise, timestep):
        if timestep.ndim == 2:
            timestep = timestep.flatten(0, 1)
        sig = self.sigmas.to(noise.device)
        ts = self.timesteps.to(noise.device)
        tid = torch.argmin((ts.unsqueeze(0) - timestep.to(noise.device).unsqueeze(1)).abs(), dim=1)
        sigma = sig[tid].reshape(-1, 1, 1, 1)
        return ((1 - sigma) * original_samples + sigma * noise).type_as(noise)
