"""The DPM-Solver++ sampler (sample_solver='dpm++'), host side: FlowDPMSolverMultistepScheduler's schedules and per-step scalars
against what the REAL reference produced (tests/golden/dpmpp_sched.pt, make_golden_dpmpp.py), the numpy emulation of the fused
kernel (tests/dpmpp_ref.py) against the reference's trajectory, the teeth of its mutants, the entry points' argument checks, and
the pipeline's / the entry point's routing of the solver choice."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from mmpl_amd import _lib, cli
from mmpl_amd.scheduler import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas,
                                retrieve_timesteps)
from tests import dpmpp_ref as D
from tests.util import GOLDEN

SCHEDULES = ((50, 5.0), (10, 5.0))


def _fixture():
    return torch.load(f"{GOLDEN}/dpmpp_sched.pt")


def _scheduler(steps, shift):
    """the way the reference's pipeline builds it (pipeline/casual_fps_inference.py:512-521)"""
    s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    ts, n = retrieve_timesteps(s, device="cpu", sigmas=get_sampling_sigmas(steps, shift))
    assert ts is s.timesteps and n == steps == s.num_inference_steps
    return s


def _bits32(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def _bf(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


# ------------------------------------------------------------------ schedules and scalars
@pytest.mark.parametrize("steps,shift", SCHEDULES)
def test_schedule_equals_the_reference(steps, shift):
    fx = _fixture()
    assert "REAL reference" in fx["produced_by"]
    e = fx[f"s{steps}"]
    s = _scheduler(steps, shift)
    assert s.timesteps.dtype == torch.int64 and s.sigmas.dtype == torch.float32 and s.sigmas.device.type == "cpu"
    assert torch.equal(s.timesteps, e["timesteps"]) and torch.equal(s.sigmas, e["sigmas"])
    assert int(s.timesteps[0]) == 1000 and float(s.sigmas[0]) == 1.0 and float(s.sigmas[-1]) == 0.0 and len(s.sigmas) == steps + 1
    u = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    u.set_timesteps(steps, shift=shift)
    assert int(u.timesteps[0]) == 999                      # UniPC's schedule starts below sigma 1: the two classes are not interchangeable


@pytest.mark.parametrize("steps,shift", SCHEDULES)
def test_step_scalars_equal_the_reference_bit_for_bit(steps, shift):
    e = _fixture()[f"s{steps}"]
    s = _scheduler(steps, shift)
    rows = [s.step_scalars(5.0) for _ in range(steps)]
    assert s.step_index == steps
    with pytest.raises(IndexError):
        s.step_scalars(5.0)
    for k in ("sigma_cur", "c1", "c2", "inv_r0"):
        got = [getattr(r, k) for r in rows]
        assert all(math.isfinite(v) for v in got), k
        assert np.array_equal(_bits32(got), _bits32(e[k].numpy())), k
    assert [r.order for r in rows] == e["order"].tolist() == [1] + [2] * (steps - 2) + [1]
    assert all(r.guidance == 5.0 for r in rows)
    # the three places where the reference's host arithmetic passes through an infinity
    sig = s.sigmas
    first, second, last = rows[0], rows[1], rows[-1]
    assert first.sigma_cur == 1.0 and first.c2 == float(-(1 - sig[1])) and first.c1 == float(sig[1])       # h = +inf: exp(-h) = 0
    assert second.order == 2 and second.inv_r0 == 0.0                                                       # r0 = +inf: D1 = +-0
    assert last.c1 == 0.0 and last.c2 == -1.0 and last.order == 1                                           # sigma_t = 0: the result is m0
    for step in D.STEPS_50 if steps == 50 else D.STEPS_10:       # the steps the GPU test launches take the order its table says
        assert D.ORDERS[(steps, step)] == rows[step].order


def test_unsupported_configurations_raise():
    for kw in (dict(solver_order=3), dict(solver_order=1), dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver++"),
               dict(solver_type="heun"), dict(prediction_type="epsilon"), dict(final_sigmas_type="sigma_min"), dict(thresholding=True),
               dict(use_dynamic_shifting=True), dict(shift=5.0), dict(euler_at_final=True), dict(lower_order_final=False),
               dict(lambda_min_clipped=-5.0), dict(variance_type="learned"), dict(invert_sigmas=True)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            FlowDPMSolverMultistepScheduler(**kw)
    s = FlowDPMSolverMultistepScheduler()
    with pytest.raises(NotImplementedError):
        s.set_timesteps(10, mu=0.8)
    with pytest.raises(ValueError):
        retrieve_timesteps(s, device="cpu", timesteps=[999, 500])
    with pytest.raises(ValueError):
        retrieve_timesteps(s, 10, device="cpu")


def test_sigmas_are_not_shifted_twice():
    s = _scheduler(10, 5.0)
    want = np.concatenate([get_sampling_sigmas(10, 5.0), [0]]).astype(np.float32)
    assert np.array_equal(s.sigmas.numpy(), want)
    assert np.array_equal(get_sampling_sigmas(10, 5.0), 5.0 * np.linspace(1, 0, 11)[:10] / (1 + 4.0 * np.linspace(1, 0, 11)[:10]))


# ------------------------------------------------------------------ the emulation against the reference's trajectory
def _walk(e, steps, shift, key, mutation=None):
    """dpmpp_chain over the fixture's toy trajectory, each step fed the reference's own sample and flow; the history is the chain's.
    -> the steps on which the sample after the step differs from the reference's."""
    s = _scheduler(steps, shift)
    from mmpl_amd.synthetic import philox_normal
    toy = _fixture()["toy"]
    x = _bf(philox_normal(toy["shape"], toy["x_seed"], torch.bfloat16))
    m0 = m1 = np.zeros_like(x)
    bad = []
    for i in range(steps):
        st = s.step_scalars(0.0)
        (xo, m0, m1), _ = D.dpmpp_chain(st, _bf(e[f"flow_{key}"][i]), None, x, m0, m1, mutation)
        want = _bf(e[f"traj_{key}"][i])
        if not np.array_equal(xo, want):
            bad.append(i)
        x = want
    return bad


@pytest.mark.parametrize("steps,shift", SCHEDULES)
def test_emulation_reproduces_the_reference_under_its_native_scalar_semantics(steps, shift):
    e = _fixture()[f"s{steps}"]
    assert _walk(e, steps, shift, "gpu") == []
    # ... and the fixture tells the two scalar semantics apart: the fp32-scalar chain is not the CPU run, the bf16-scalar chain is
    assert _walk(e, steps, shift, "cpu") != []
    assert _walk(e, steps, shift, "cpu", "scalar_rounded") == []
    assert not torch.equal(e["traj_gpu"], e["traj_cpu"])


# ------------------------------------------------------------------ the mutants have teeth on the GPU test's operands
def _rows(steps):
    s = _scheduler(steps, 5.0)
    return [s.step_scalars(5.0) for _ in range(steps)]


@pytest.mark.parametrize("with_u", [True, False], ids=["cfg", "combined"])
@pytest.mark.parametrize("n", D.MUTANT_SIZES)
def test_every_mutant_changes_an_output_element(n, with_u):
    ops = [o[:D.MUTANT_SLICE] for o in D.operands(n)]             # the elements the GPU test holds the mutants to
    for steps, picks in ((50, D.STEPS_50), (10, D.STEPS_10)):
        rows = _rows(steps)
        for step in picks:
            st = rows[step]
            base, mids = D.dpmpp_chain(st, ops[0], ops[1] if with_u else None, *ops[2:])
            assert all(np.isfinite(m).all() for m in mids)
            assert np.array_equal(base[2], ops[3])                      # m1 <- the old m0
            for mut in D.MUTATIONS:
                got, _ = D.dpmpp_chain(st, ops[0], ops[1] if with_u else None, *ops[2:], mutation=mut)
                changed = sum(D.differs(got, base))
                if D.bites(mut, st) is True:
                    assert changed > 0, (steps, step, mut)
                elif D.bites(mut, st) is False:
                    assert changed == 0, (steps, step, mut)
    # every mutant applies on at least one of the steps the GPU test launches
    for mut in D.MUTATIONS:
        assert any(D.bites(mut, _rows(50)[s]) for s in D.STEPS_50) and any(D.bites(mut, _rows(10)[s]) for s in D.STEPS_10)


# ------------------------------------------------------------------ entry points
def test_struct_layout():
    assert C.sizeof(_lib.MmplDpmppStep) == 6 * 4
    assert [f[0] for f in _lib.MmplDpmppStep._fields_] == list(D.FIELDS)
    assert {"mmpl_cfg_dpmpp_step", "mmpl_cfg_dpmpp_step_table"} <= set(_lib.SYMBOLS)


def test_entry_points_reject_null_arguments_without_a_device():
    lib = _lib.load()
    P = C.c_void_p(0x1000)                                   # never dereferenced: every call below fails before a launch

    def err(rc):
        assert rc != 0
        return lib.mmpl_last_error().decode()

    st = _lib.MmplDpmppStep()
    st.order = 1
    for bad in (0, 2, 3, 4):                                 # flow_uncond (1) may be NULL
        a = [P] * 5
        a[bad] = None
        assert "mmpl_cfg_dpmpp_step: null argument" in err(lib.mmpl_cfg_dpmpp_step(*a, 16, C.byref(st), None))
        assert "mmpl_cfg_dpmpp_step_table: null argument" in err(lib.mmpl_cfg_dpmpp_step_table(*a, 16, P, P, P, P, 1, 50, None))
    assert "null step" in err(lib.mmpl_cfg_dpmpp_step(*[P] * 5, 16, None, None))
    st.order = 3
    assert "order" in err(lib.mmpl_cfg_dpmpp_step(*[P] * 5, 16, C.byref(st), None))
    for a in ((None, P, P, P, 1, 50), (P, None, P, P, 1, 50), (P, P, None, P, 1, 50), (P, P, P, None, 1, 50), (P, P, P, P, 0, 50), (P, P, P, P, 1, 0)):
        assert "bad arguments" in err(lib.mmpl_cfg_dpmpp_step_table(*[P] * 5, 16, *a, None))


# ------------------------------------------------------------------ pipeline and entry script
class _FakeGen:
    """A generator that launches nothing: enough of WanFPSWrapper for CausalFPSInferencePipeline's constructor."""

    def __init__(self):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        self.geometry = Geometry(16, 24)
        self.engine = types.SimpleNamespace(L=1)
        self.model = types.SimpleNamespace(num_frame_per_block=3)
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)

    def get_scheduler(self):
        return self.scheduler


def _fake_pipe(**extra):
    from mmpl_amd.pipeline import CausalFPSInferencePipeline
    a = types.SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, guidance_scale=5.0, negative_prompt="NEG",
                              independent_first_frame=False, sampling_steps=10, **extra)
    return CausalFPSInferencePipeline(a, "cpu", generator=_FakeGen(), text_encoder=object(), vae=object(), device_cond="cpu",
                                      device_uncond="cpu", save=None)


def test_pipeline_builds_the_solver_its_attribute_names():
    noise = torch.zeros(1)
    pipe = _fake_pipe()
    assert pipe.sample_solver == "unipc"
    s = pipe._initialize_sample_scheduler(noise)
    assert type(s) is FlowUniPCMultistepScheduler and int(pipe.timesteps[0]) == 999 and len(pipe.timesteps) == 10
    pipe = _fake_pipe(sample_solver="dpm++")
    assert pipe.sample_solver == "dpm++"
    s = pipe._initialize_sample_scheduler(noise)
    assert type(s) is FlowDPMSolverMultistepScheduler and pipe.timesteps is s.timesteps
    assert torch.equal(s.timesteps, _fixture()["s10"]["timesteps"]) and torch.equal(s.sigmas, _fixture()["s10"]["sigmas"])
    pipe.sample_solver = "unipc"                                 # the reference's way: set the attribute on the built pipeline
    assert type(pipe._initialize_sample_scheduler(noise)) is FlowUniPCMultistepScheduler
    pipe.sample_solver = "euler"
    with pytest.raises(NotImplementedError, match="Unsupported solver."):
        pipe._initialize_sample_scheduler(noise)
    # the stage loop's whole use of the object, on either class
    for name in ("timesteps", "step_scalars", "_ensure_state", "step_cfg", "build_step_table", "reset_step_table", "step_cfg_table", "step"):
        assert hasattr(FlowDPMSolverMultistepScheduler, name) or name == "timesteps", name
        assert hasattr(FlowUniPCMultistepScheduler, name) or name == "timesteps", name


def _cfg(tmp_path, fewstep):
    cfg = tmp_path / ("self_forcing_dmd.yaml" if fewstep else "fps.yaml")
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n" if fewstep
                   else "timestep_shift: 5.0\n")
    return str(cfg)


def test_cli_solver_refusal():
    args = types.SimpleNamespace(sample_solver="dpm++")
    assert "--sample_solver dpm++" in cli.solver_refusal(args, True) and cli.solver_refusal(args, False) is None
    args.sample_solver = "unipc"
    assert cli.solver_refusal(args, True) is None and cli.solver_refusal(args, False) is None
    assert cli.solver_refusal(types.SimpleNamespace(), True) is None


def test_cli_refuses_dpmpp_with_a_fewstep_config(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--config_path", _cfg(tmp_path, True), "--synthetic", "--model", "tiny", "--duration", "1", "--sample_solver", "dpm++"])
    assert e.value.code == 2
    assert "--sample_solver dpm++" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                          # an unknown solver never reaches the pipeline
        cli.main(["--config_path", _cfg(tmp_path, False), "--synthetic", "--model", "tiny", "--sample_solver", "euler"])
    assert e.value.code == 2
    assert "invalid choice" in capsys.readouterr().err


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flag,want", [(["--sample_solver", "dpm++"], FlowDPMSolverMultistepScheduler), ([], FlowUniPCMultistepScheduler)])
def test_cli_flag_reaches_the_pipeline(tmp_path, monkeypatch, flag, want):
    """cli.main up to the pipeline's construction, nothing launched: the wrappers are stand-ins, the pipeline is the real class
    around the fake generator, built from the config object the entry point hands over."""
    import mmpl_amd.pipeline as P
    import mmpl_amd.wan_wrapper as W
    real, built = P.CausalFPSInferencePipeline, {}

    class _Wrapper:
        model_type = "t2v"

        def __init__(self, *a, **kw):
            pass

        def load_state_dict(self, sd):
            pass

    def pipeline(config, dev, **kw):
        built["pipe"] = real(config, "cpu", generator=_FakeGen(), text_encoder=object(), vae=object(), device_cond="cpu",
                             device_uncond="cpu", save=None, mode=kw["mode"])
        raise _Reached

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for name in ("WanFPSWrapper", "SyntheticTextEncoder", "WanVAEWrapper"):
        monkeypatch.setattr(W, name, _Wrapper)
    monkeypatch.setattr(cli, "dit_state_dict", lambda *a, **kw: {})
    monkeypatch.setattr(cli, "vae_state_dict", lambda *a, **kw: {})
    monkeypatch.setattr(P, "CausalFPSInferencePipeline", pipeline)
    with pytest.raises(_Reached):
        cli.main(["--config_path", _cfg(tmp_path, False), "--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--sampling_steps", "10"] + flag)
    pipe = built["pipe"]
    assert pipe.sample_solver == (flag[1] if flag else "unipc") and pipe.sampling_steps == 10
    assert type(pipe._initialize_sample_scheduler(torch.zeros(1))) is want
