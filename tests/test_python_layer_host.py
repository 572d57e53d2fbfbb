"""The seams of the Python layer that the wrappers, the pipelines and the entry point share (CPU, no GPU): CrossAttnCache.fill's two
input shapes, "built from this very tensor, unwritten since", the validated conditioning video, the pipelines' common helpers
(mmpl_amd/pipeline/_common.py) and the entry point's refusal order."""
import types

import pytest
import torch

from mmpl_amd import cli, wan_wrapper as W
from mmpl_amd.pipeline import _common as P
from mmpl_amd.scheduler import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler
from tests.util import GOLDEN


# ------------------------------------------------------------------------------------------------ wan_wrapper
class _FakeEngine:
    """What CrossAttnCache touches of a DitEngine; precompute_context records its call."""
    L, text_len, dim, device, cfg = 2, 8, 128, torch.device("cpu"), {"num_heads": 1}

    def __init__(self):
        self.calls = []

    def precompute_context(self, context, out=None):
        self.calls.append((context.clone(), out))
        return types.SimpleNamespace(rows=5)


def test_crossattn_cache_fill_takes_both_shapes():
    eng = _FakeEngine()
    cache = W.CrossAttnCache(eng)
    pe = torch.arange(8 * 4, dtype=torch.float32).reshape(8, 4)
    assert not cache.is_init and cache.rows == 8
    cache.fill(pe)
    assert cache.is_init and cache.rows == 5
    cache.fill(pe.unsqueeze(0))
    (a, out_a), (b, out_b) = eng.calls
    assert a.shape == b.shape == (8, 4) and torch.equal(a, b) and torch.equal(a, pe)
    assert out_a[0] is cache.k_all and out_a[1] is cache.v_all and out_b[0] is cache.k_all and out_b[1] is cache.v_all


def test_built_from_is_identity_and_version():
    t = torch.zeros(3, 4)
    src = W._source(t)
    assert W._built_from(src, t) and not W._built_from(None, t)
    assert not W._built_from(src, t.clone()), "an equal but different tensor"
    assert not W._built_from(src, torch.zeros(3, 4))
    t.add_(1)                                                           # in place: _version moved
    assert not W._built_from(src, t)
    assert W._built_from(W._source(t), t)


def test_conditioning_video_shapes():
    eng = types.SimpleNamespace(in_dim=36, lat_h=4, lat_w=6)
    y = torch.arange(20 * 3 * 4 * 6, dtype=torch.float32).reshape(20, 3, 4, 6)
    for form in (y, [y], (y,), y.unsqueeze(0)):
        got = W._conditioning_video(form, eng, "who")
        assert got.shape == (20, 3, 4, 6) and torch.equal(got, y)
    for bad in (y[:19], y[:, :, :3], y[..., :5], y[0], y.unsqueeze(0).unsqueeze(0), torch.zeros(16, 3, 4, 6)):
        with pytest.raises(ValueError, match=r"who: y is .*expected \[20, F, 4, 6\]"):
            W._conditioning_video(bad, eng, "who")


def test_both_wrappers_refuse_a_malformed_y_with_value_error():
    eng = types.SimpleNamespace(in_dim=36, lat_h=4, lat_w=6, device=torch.device("cpu"))
    fps = W.WanFPSWrapper.__new__(W.WanFPSWrapper)                      # __init__ creates the engine on a GPU
    torch.nn.Module.__init__(fps)
    fps.engine, fps.model_type = eng, "i2v"
    clip_fea = torch.zeros(257, 1280)
    fps._clip_src = W._source(clip_fea)                                 # the image K / V count as built: no engine call
    good = torch.zeros(20, 5, 4, 6)
    assert fps._image_stream([1, 3], {}, clip_fea, good).shape == (2, 20, 4, 6)
    with pytest.raises(ValueError, match="WanFPSWrapper: y is"):
        fps._image_stream([1, 3], {}, clip_fea, torch.zeros(20, 5, 4, 7))
    dif = W.WanDiffusionWrapper.__new__(W.WanDiffusionWrapper)
    torch.nn.Module.__init__(dif)
    dif.engine = eng
    assert dif.frame_major_y([good]).shape == (5, 20, 4, 6)
    with pytest.raises(ValueError, match="WanDiffusionWrapper: y is"):
        dif.frame_major_y(torch.zeros(19, 5, 4, 6))


# ------------------------------------------------------------------------------------------------ pipeline/_common.py
def test_sample_scheduler_factory():
    s, ts = P.make_sample_scheduler("unipc", 1000, 50, 5.0, "cpu")
    fx = torch.load(f"{GOLDEN}/sched.pt")
    assert type(s) is FlowUniPCMultistepScheduler and ts is s.timesteps
    assert torch.equal(ts, fx["timesteps"]) and torch.equal(s.sigmas, fx["sigmas"])
    assert ts[:6].tolist() == [999, 995, 991, 987, 982, 978] and ts[-4:].tolist() == [302, 241, 172, 92]
    s, ts = P.make_sample_scheduler("unipc", 1000, 10, 5.0, "cpu")
    assert int(ts[0]) == 999 and len(ts) == 10
    s, ts = P.make_sample_scheduler("dpm++", 1000, 10, 5.0, "cpu")
    fx = torch.load(f"{GOLDEN}/dpmpp_sched.pt")["s10"]
    assert type(s) is FlowDPMSolverMultistepScheduler and ts is s.timesteps
    assert torch.equal(ts, fx["timesteps"]) and torch.equal(s.sigmas, fx["sigmas"])
    with pytest.raises(NotImplementedError, match="Unsupported solver."):
        P.make_sample_scheduler("euler", 1000, 10, 5.0, "cpu")


class _Sigmas:
    """sigma_x0 / sigma_add_noise that show which step they were asked about, and in which dtype."""

    def sigma_x0(self, t):
        return ("x0", float(t), t.dtype)

    def sigma_add_noise(self, t):
        return ("add", float(t), t.dtype)


def test_fewstep_scalars_for_both_pipelines():
    """The warped list [1000, 750, 500, 250] (float32, as `timesteps[1000 - list]` leaves it): the causal pipeline runs a forward
    at every step, the bidirectional one at all but the last; both re-noise to every step after the first."""
    from mmpl_amd.scheduler import FlowMatchScheduler
    fm = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    fm.set_timesteps(1000, training=True)
    steps = torch.cat((fm.timesteps, torch.tensor([0], dtype=torch.float32)))[1000 - torch.tensor([1000, 750, 500, 250])]
    assert steps.dtype == torch.float32 and len(steps) == 4
    v = [float(t) for t in steps]
    f32 = torch.float32
    t_eng, sx, sn = P.fewstep_scalars(_Sigmas(), steps, 4)
    assert t_eng == v and sx == [("x0", t, f32) for t in v] and sn == [("add", t, f32) for t in v[1:]]
    t_eng, sx, sn = P.fewstep_scalars(_Sigmas(), steps, 3)
    assert t_eng == v[:3] and sx == [("x0", t, f32) for t in v[:3]] and sn == [("add", t, f32) for t in v[1:]]
    # through the pipelines' own _step_scalars, on a generator with the real sigma lookups
    from mmpl_amd.pipeline import BidirectionalInferencePipeline, CausalInferencePipeline
    gen = types.SimpleNamespace(scheduler=fm, _sig64=fm.sigmas.double(), _ts64=fm.timesteps.double())
    gen.sigma_x0 = types.MethodType(W.WanDiffusionWrapper.sigma_x0, gen)
    gen.sigma_add_noise = types.MethodType(W.WanDiffusionWrapper.sigma_add_noise, gen)
    want_x0 = [gen.sigma_x0(t) for t in steps]
    want_add = [gen.sigma_add_noise(t) for t in steps[1:]]
    for cls, n in ((CausalInferencePipeline, 4), (BidirectionalInferencePipeline, 3)):
        pipe = types.SimpleNamespace(generator=gen, denoising_step_list=steps)
        assert cls._step_scalars(pipe) == (v[:n], want_x0[:n], want_add)
    assert want_x0[0] == 1.0 and all(a > b for a, b in zip(want_x0, want_x0[1:]))


def test_fill_bank_takes_the_override_in_order_or_draws():
    bank = torch.zeros(3, 2, 4)
    draws = iter([torch.full((8,), float(k)) for k in range(5)])        # any shape of the right size
    P.fill_bank(bank, 2, draws, None)
    assert bank[0].eq(0).all() and bank[1].eq(1).all() and bank[2].eq(0).all()
    P.fill_bank(bank, 3, draws, None)                                   # the next block goes on where the last one stopped
    assert [float(bank[i, 0, 0]) for i in range(3)] == [2.0, 3.0, 4.0]
    g = torch.Generator().manual_seed(7)
    P.fill_bank(bank, 2, None, g)
    g2 = torch.Generator().manual_seed(7)
    want = [torch.empty(2, 4).normal_(0.0, 1.0, generator=g2) for _ in range(2)]
    assert torch.equal(bank[0], want[0]) and torch.equal(bank[1], want[1]) and bank[2].eq(4).all()


# ------------------------------------------------------------------------------------------------ cli
def _cli_args(**kw):
    a = dict(bidirectional=False, duration=1, num_output_frames=21, i2v=False, i2v_model=False, stream=False, rolling=False,
             preview_vae=None, cfg_split=False, sample_solver="unipc", sample_shift=None, extend=None, extend_context=None,
             num_frame_per_block=3, kv_window=21, pixel_hw=(128, 192), image=None)
    a.update(kw)
    a.setdefault("fewstep", False)
    return types.SimpleNamespace(**a)


def test_first_refusal_lets_a_plain_command_line_through():
    assert cli.first_refusal(_cli_args(), 1, False) is None
    assert cli.first_refusal(_cli_args(duration=3), 4, False) is None
    assert cli.first_refusal(_cli_args(fewstep=True, stream=True, preview_vae=""), 1, True) is None
    assert cli.first_refusal(_cli_args(bidirectional=True), 1, False) is None


@pytest.mark.parametrize("kw, world, fewstep, first", [
    # two or more refusals apply; `first` is the one main has always asked first
    (dict(bidirectional=True, stream=True, rolling=True), 1, False, lambda a, w, f: cli.bidirectional_refusal(a, w)),
    (dict(stream=True, rolling=True, preview_vae=""), 1, False, lambda a, w, f: cli.stream_refusal(a, f)),
    (dict(preview_vae="", rolling=True), 1, False, lambda a, w, f: cli.preview_refusal(a)),
    (dict(rolling=True, sample_solver="dpm++", extend="x.pt"), 1, False, lambda a, w, f: cli.rolling_refusal(a, f)),
    (dict(sample_solver="dpm++", duration=2), 2, True, lambda a, w, f: cli.solver_refusal(a, f)),
    (dict(duration=2, extend_context=3), 1, True, lambda a, w, f: cli.fewstep_refusal(a, w)),
    (dict(i2v=True, extend="x.pt", stream=True, preview_vae=""), 1, True, lambda a, w, f: cli.fewstep_refusal(a, w)),
    (dict(extend_context=3), 1, True, lambda a, w, f: cli.extend_refusal(a, f)),
    (dict(extend="x.pt"), 1, False, lambda a, w, f: cli.extend_refusal(a, f)),
    # --bidirectional with a few-step config: fewstep_refusal is not asked (one clip per call, no rollout)
    (dict(bidirectional=True, extend_context=3), 1, True, lambda a, w, f: cli.extend_refusal(a, f)),
])
def test_first_refusal_order(kw, world, fewstep, first):
    args = _cli_args(fewstep=fewstep, **kw)
    want = first(args, world, fewstep)
    assert want is not None
    assert cli.first_refusal(args, world, fewstep) == want


@pytest.mark.parametrize("fewstep, extra, text", [
    # the command lines of tests/test_fewstep_host.py, tests/test_bidir_host.py and tests/test_taehv_enc_host.py, and pairs of them
    (True, ["--duration", "2"], "--duration 2: the few-step pipeline"),
    (True, ["--duration", "1", "--i2v"], "--i2v: the few-step pipeline"),
    (True, [], "--duration 3: the few-step pipeline"),
    (True, ["--bidirectional", "--duration", "2", "--stream"], "--duration 2: --bidirectional generates one"),
    (True, ["--bidirectional", "--duration", "1", "--stream", "--rolling"], "--stream: --bidirectional denoises the whole clip"),
    (False, ["--bidirectional", "--duration", "1", "--num_output_frames", "25"], "--num_output_frames 25"),
    (False, ["--stream", "--rolling"], "--stream: block-wise output needs a few-step config"),
    (False, ["--preview_vae", "--rolling"], "--preview_vae: the tiny preview decoder (TAEHV"),
    (False, ["--rolling", "--sample_solver", "dpm++"], "--rolling: the rolling KV window needs a few-step config"),
    (True, ["--sample_solver", "dpm++", "--duration", "2"], "--sample_solver dpm++"),
    (True, ["--duration", "1", "--extend", "CLIP", "--stream"], "--extend: the context is encoded"),
    (True, ["--duration", "1", "--extend", "CLIP", "--stream", "--preview_vae", "--num_output_frames", "21"], "add --rolling"),
    (True, ["--duration", "1", "--extend", "CLIP", "--stream", "--preview_vae", "--i2v", "--num_output_frames", "3"],
     "--i2v: the few-step pipeline"),
    (True, ["--duration", "1", "--extend_context", "3"], "--extend_context: only with --extend FILE"),
])
def test_cli_reports_the_first_refusal(tmp_path, capsys, fewstep, extra, text):
    cfg = tmp_path / "config.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n" if fewstep
                   else "timestep_shift: 5.0\n")
    clip = tmp_path / "clip.pt"
    torch.save(torch.zeros(12, 128, 192, 3, dtype=torch.uint8), clip)
    argv = ["--config_path", str(cfg), "--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--output_folder", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + [str(clip) if a == "CLIP" else a for a in extra])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err and err.count("error:") == 1
