"""Host tests of upstream Wan2.1's float32 latent chain (no GPU):

  restatement    tests/fp32_chain_ref.py (the two float32 solvers of csrc/sampler.hip per element, one torch float32 operation per IEEE
                 operation), driven by the float32 scalars of mmpl_amd/scheduler.py, reproduces the REAL reference's schedulers
                 (tests/golden/fp32_chain.pt, make_golden_fp32_chain.py) bit for bit at EVERY step, for both solvers and both
                 schedules.  The scalars the replay carries are the fixture's record of them (`rows`): the reference's 0-dim
                 float32 expressions cannot be matched bitwise ACROSS MACHINES -- torch.log / torch.expm1 / torch.exp and
                 torch.linalg.solve (LAPACK) are dispatched by CPU, and an MI355X host was seen to differ from the fixture's machine
                 in the last bits of rk, c2 / c3 and the rhos (first at step 3 of the 6-step schedule), which the cancellation in
                 lambda_t - lambda_s amplifies.  Those are the named operations; everything else -- every tensor operation, the
                 sigmas, the orders, the one-term `einsum` (an exact single product) -- is held bit for bit.  1 / rk in place of
                 rk, or a rho rounded to bf16, fails the replay;
  scalars        mmpl_amd/scheduler.py's float32 scalars computed on THIS host equal the recorded ones: bitwise where no such
                 function is involved, within a bound derived from the schedule in float64 (`host_scalar_bounds`) elsewhere;
  geometry       generate.i2v_latent_hw reproduces the latent sizes the real WanI2V.generate derives;
  CLI            --fp32_latents is refused without --bidirectional and with a few-step config, each with its reason;
  generate()     argument errors (frame_num, size, solver, noise shape, the distributed flags), raised before any GPU work.
"""
import os
import types

import pytest
import torch

from mmpl_amd import cli
from mmpl_amd.pipeline._common import make_sample_scheduler
from tests import fp32_chain_ref as R
from tests.util import GOLDEN

FX = torch.load(os.path.join(GOLDEN, "fp32_chain.pt"))


def f32_scheduler(solver, steps, shift):
    """The pipeline's scheduler in float32 mode (the mode is the dtype of the sample the state is built for)."""
    s, _ = make_sample_scheduler(solver, 1000, steps, shift, "cpu")
    s._ensure_state(torch.zeros(1, dtype=torch.float32))
    assert s.latent_dtype == torch.float32
    return s


def recorded_rows(solver, e):
    """The fixture's record of the per-step scalars as the machine that made the trajectory computed them -> ctypes rows."""
    from mmpl_amd import _lib
    cls = _lib.MmplUniPCStepF32 if solver == "unipc" else _lib.MmplDpmppStep
    assert sorted(e["rows"]) == sorted(f for f, _ in cls._fields_)
    return [cls(**{f: (int if ty is _lib.C.c_int else float)(e["rows"][f][i]) for f, ty in cls._fields_}) for i in range(e["steps"])]


U = 2.0 ** -24
EXACT = {"unipc": ("guidance", "sigma_cur", "use_corrector", "corr_order", "pred_order", "c_c1", "p_c1"),
         "dpm++": ("guidance", "sigma_cur", "order", "c1")}
RHOS = ("c_rho0", "c_rho_last")


def host_scalar_bounds(sigmas, i):
    """How far two hosts may lie apart, relatively, in the scalars of step i that pass through torch.log / torch.expm1 / torch.exp
    or torch.linalg.solve -- from the float64 schedule alone, not from any code under test.  Each elementary function is accurate
    to 1 ulp in either implementation (two results differ by at most 2 ulp) and at most 16 such results and roundings enter one
    scalar: 32 u.  Two amplifications multiply that: the cancellation in h = lambda_a - lambda_b, lambda = log(1 - s) - log(s), by
    A = (|log(1 - s_a)| + |log s_a| + |log(1 - s_b)| + |log s_b|) / |h| (the worst of the adjacent pairs among steps i - 2 .. i + 1),
    and, for the rhos only, the cancellation in expm1(-h) / (-h) - 1 ~ -h / 2 by 2 / |h| and the 2 x 2 elimination by
    cond_inf([[1, 1], [rk, 1]]) = max(2, |rk| + 1)^2 / |1 - rk|.  -> (bound of the other scalars, bound of the rhos)."""
    import math
    sg = [float(v) for v in sigmas.double().tolist()]
    lam = lambda v: math.log(1 - v) - math.log(v)
    amp, inv_h, rk = 1.0, 0.0, -1.0
    pairs = [(a, a + 1) for a in range(max(i - 2, 0), min(i + 1, len(sg) - 1)) if 0.0 < sg[a] < 1.0 and 0.0 < sg[a + 1] < 1.0]
    for a, b in pairs:
        h = abs(lam(sg[b]) - lam(sg[a]))
        amp = max(amp, sum(abs(math.log(v)) for v in (1 - sg[a], sg[a], 1 - sg[b], sg[b])) / h)
        inv_h = max(inv_h, 2.0 / h)
    if i >= 2 and (i - 2, i - 1) in pairs and (i - 1, i) in pairs:
        rk = (lam(sg[i - 2]) - lam(sg[i - 1])) / (lam(sg[i]) - lam(sg[i - 1]))
    cond = max(2.0, abs(rk) + 1.0) ** 2 / abs(1.0 - rk)
    return 32 * U * amp, cond * 32 * U * (amp + inv_h)


def replay(solver, e, mutation=None):
    """The restatement over the fixture's recorded flows, free running from its start -> x after every step, float32 [steps, n]."""
    x = e["x0"].clone()
    m0, m1, last = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    out = []
    for i, st in enumerate(recorded_rows(solver, e)):
        if solver == "unipc":
            x, m0, m1, last = R.unipc_f32(st, e["flow_cond"][i], e["flow_uncond"][i], x, m0, m1, last, mutation=mutation)
        else:
            x, m0, m1 = R.dpmpp_f32(st, e["flow_cond"][i], e["flow_uncond"][i], x, m0, m1)
        out.append(x)
    return torch.stack(out)


@pytest.mark.parametrize("key", ["s50", "s6"])
@pytest.mark.parametrize("solver", ["unipc", "dpm++"])
def test_restatement_equals_the_reference_at_every_step(solver, key):
    e = FX["sched"][solver][key]
    assert e["x"].dtype == torch.float32 and e["x"].shape == (e["steps"], 768) and e["flow_cond"].dtype == torch.bfloat16
    got = replay(solver, e)
    differ = [int((got[i].view(torch.int32) != e["x"][i].view(torch.int32)).sum()) for i in range(e["steps"])]
    print(f"{solver} {key}: elements of 768 that differ from the reference, per step: {differ}")
    assert not any(differ), differ


@pytest.mark.parametrize("key", ["s50", "s6"])
@pytest.mark.parametrize("solver", ["unipc", "dpm++"])
def test_this_hosts_scalars_agree_with_the_recorded_ones(solver, key):
    """mmpl_amd/scheduler.py's float32 scalars, computed here, against the fixture's record: the orders, the sigmas and the sigma
    ratios in every bit; whatever passes through torch.log / expm1 / exp / linalg.solve within `host_scalar_bounds` (bitwise on a
    host like the one that made the fixture).  A reciprocal in place of rk, or a rho rounded to bf16 (up to 2^-9 off), is far outside."""
    e = FX["sched"][solver][key]
    s = f32_scheduler(solver, e["steps"], e["shift"])
    assert [int(t) for t in s.timesteps] == [int(t) for t in e["timesteps"]]
    worst = 0.0
    for i, rec in enumerate(recorded_rows(solver, e)):
        st = s.step_scalars(e["guidance"])
        assert type(st) is type(rec)
        other, rho = host_scalar_bounds(s.sigmas, i)
        for f, _ in st._fields_:
            a, b = getattr(st, f), getattr(rec, f)
            if f in EXACT[solver] or a == b:
                assert a == b, (i, f, a, b)
                continue
            bound = rho if f in RHOS else other
            worst = max(worst, abs(a - b) / abs(b) / bound)
            assert abs(a - b) <= bound * abs(b), (i, f, a, b, bound)
    print(f"{solver} {key}: largest |live - recorded| / bound = {worst:.3f}")


def test_float32_scalars_carry_rk_and_unrounded_rhos():
    """The float32 struct holds rk itself and float32 rhos; the bf16 struct of the same schedule holds 1 / rk and bf16 rhos."""
    from mmpl_amd import _lib
    a = f32_scheduler("unipc", 50, 5.0)
    b, _ = make_sample_scheduler("unipc", 1000, 50, 5.0, "cpu")
    rows_a = [a.step_scalars(5.0) for _ in range(50)]
    rows_b = [b.step_scalars(5.0) for _ in range(50)]
    assert all(type(r) is _lib.MmplUniPCStepF32 for r in rows_a) and all(type(r) is _lib.MmplUniPCStep for r in rows_b)
    assert [f for f, _ in _lib.MmplUniPCStepF32._fields_] == [f.replace("inv_rk", "rk") for f, _ in _lib.MmplUniPCStep._fields_]
    unrounded = 0
    for i, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        assert (ra.use_corrector, ra.corr_order, ra.pred_order) == (rb.use_corrector, rb.corr_order, rb.pred_order)
        for f in ("guidance", "sigma_cur", "c_c1", "c_c2", "c_c3", "p_c1", "p_c2", "p_c3"):
            assert getattr(ra, f) == getattr(rb, f), (i, f)
        if ra.pred_order == 2:
            assert rb.p_inv_rk == (1.0 / torch.tensor(ra.p_rk, dtype=torch.float32)).item()
        if ra.use_corrector and ra.corr_order == 2:
            assert rb.c_inv_rk == (1.0 / torch.tensor(ra.c_rk, dtype=torch.float32)).item()
            for f in ("c_rho0", "c_rho_last"):
                v = torch.tensor(getattr(ra, f), dtype=torch.float32)
                assert getattr(rb, f) == v.to(torch.bfloat16).float().item()
                unrounded += int(v.to(torch.bfloat16).float().item() != v.item())
        if ra.use_corrector and ra.corr_order == 1:
            assert ra.c_rho_last == rb.c_rho_last == 0.5
    assert unrounded > 40                                                  # the float32 rhos are not bf16 values


@pytest.mark.parametrize("mutation", ["inv_rk", "bf16_rho"])
def test_a_wrong_scalar_path_fails_the_fixture(mutation):
    """The fixture has teeth: multiplying by 1 / rk, or rounding the rhos to bf16, changes the 50-step UniPC trajectory."""
    e = FX["sched"]["unipc"]["s50"]
    got = replay("unipc", e, mutation=mutation)
    assert int((got.view(torch.int32) != e["x"].view(torch.int32)).sum()) > 0


def test_i2v_geometry_is_upstreams():
    from mmpl_amd.generate import i2v_latent_hw
    rows = FX["i2v_geometry"].tolist()
    assert len(rows) == 10
    for ih, iw, area, lat_h, lat_w in rows:
        assert i2v_latent_hw(ih, iw, area) == (lat_h, lat_w), (ih, iw, area)
    # upstream's own arithmetic, quirks included: a 480 x 832 image under 480 * 832 gives 58 rows (sqrt(max_area * h / w) lands just
    # below 480 in floating point), not the 60 of the '480p' preset
    assert i2v_latent_hw(720, 1280, 720 * 1280) == (90, 160) and i2v_latent_hw(480, 832, 480 * 832) == (58, 104)


def test_cli_fp32_refusal():
    a = types.SimpleNamespace(fp32_latents=True, bidirectional=False)
    assert "add --bidirectional" in cli.fp32_refusal(a, False)
    a.bidirectional = True
    assert cli.fp32_refusal(a, False) is None
    assert "few-step pipeline" in cli.fp32_refusal(a, True) and "50-step config" in cli.fp32_refusal(a, True)
    a.fp32_latents = False
    assert cli.fp32_refusal(a, True) is None and cli.fp32_refusal(types.SimpleNamespace(), False) is None


@pytest.mark.parametrize("fewstep, extra, text", [
    (False, [], "--fp32_latents: the float32 latent chain is upstream"),
    (True, ["--bidirectional"], "--fp32_latents: the few-step pipeline"),
])
def test_cli_refuses_fp32_latents(tmp_path, capsys, fewstep, extra, text):
    cfg = tmp_path / "config.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n" if fewstep
                   else "timestep_shift: 5.0\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["--config_path", str(cfg), "--synthetic", "--model", "tiny", "--duration", "1", "--fp32_latents"] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ generate(): argument errors
class _FakeGenerator:
    def __init__(self, model_type="t2v"):
        from mmpl_amd.geometry import Geometry
        self.model_type, self.geometry, self.is_causal = model_type, Geometry(16, 24), False


def _wan(cls, model_type="t2v", **kw):
    cfg = dict(num_train_timesteps=1000, sample_neg_prompt="NEG")
    return cls(cfg, "/nowhere", generator=_FakeGenerator(model_type), text_encoder=object(), vae=object(), clip=object(), device="cpu", **kw)


def test_generate_argument_errors():
    from mmpl_amd.generate import WanI2V, WanT2V, latent_frames
    assert latent_frames(81) == 21 and latent_frames(1) == 1 and latent_frames(93) == 24
    for flag in ("use_usp", "t5_fsdp", "dit_fsdp"):
        with pytest.raises(ValueError, match=f"{flag}=True is not supported"):
            _wan(WanT2V, **{flag: True})
    _wan(WanT2V, t5_cpu=True)                                              # accepted and ignored
    with pytest.raises(ValueError, match="needs 'i2v'"):
        _wan(WanI2V, "t2v")
    with pytest.raises(ValueError, match="needs 't2v'"):
        _wan(WanT2V, "i2v")
    w = _wan(WanT2V)
    assert w.pipeline.latent_dtype == torch.float32 and w.pipeline.args.negative_prompt == "NEG"
    for bad in (80, 0, 82):
        with pytest.raises(ValueError, match="4 n \\+ 1"):
            w.generate("p", size=(192, 128), frame_num=bad)
    with pytest.raises(ValueError, match="at most 24"):
        w.generate("p", size=(192, 128), frame_num=97)
    with pytest.raises(ValueError, match="created for 16 x 24"):
        w.generate("p")                                                    # the default 1280 x 720 on a 16 x 24 engine
    with pytest.raises(ValueError, match=r"noise: float32 \[16, 21, 16, 24\]"):
        w.generate("p", size=(192, 128), noise=torch.zeros(1, 21, 16, 16, 24))
    with pytest.raises(ValueError, match="noise: float32"):
        w.generate("p", size=(192, 128), noise=torch.zeros(16, 21, 16, 24, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="Unsupported solver"):
        w.generate("p", size=(192, 128), sample_solver="euler", noise=torch.zeros(16, 21, 16, 24))
    i = _wan(WanI2V, "i2v", init_on_cpu=False)
    with pytest.raises(ValueError, match="created for 16 x 24"):
        i.generate("p", torch.zeros(3, 720, 1280))
    with pytest.raises(ValueError, match="img:"):
        i.generate("p", torch.zeros(1, 3, 128, 192))


def test_generate_signatures_are_upstreams():
    import inspect
    from mmpl_amd.generate import WanI2V, WanT2V
    t = inspect.signature(WanT2V.generate).parameters
    assert [(k, v.default) for k, v in t.items() if v.kind is v.POSITIONAL_OR_KEYWORD][1:] == [
        ("input_prompt", inspect.Parameter.empty), ("size", (1280, 720)), ("frame_num", 81), ("shift", 5.0), ("sample_solver", "unipc"),
        ("sampling_steps", 50), ("guide_scale", 5.0), ("n_prompt", ""), ("seed", -1), ("offload_model", True)]
    i = inspect.signature(WanI2V.generate).parameters
    assert [(k, v.default) for k, v in i.items() if v.kind is v.POSITIONAL_OR_KEYWORD][1:] == [
        ("input_prompt", inspect.Parameter.empty), ("img", inspect.Parameter.empty), ("max_area", 720 * 1280), ("frame_num", 81),
        ("shift", 5.0), ("sample_solver", "unipc"), ("sampling_steps", 40), ("guide_scale", 5.0), ("n_prompt", ""), ("seed", -1),
        ("offload_model", True)]
    assert t["noise"].kind is inspect.Parameter.KEYWORD_ONLY and i["noise"].kind is inspect.Parameter.KEYWORD_ONLY
