"""Host-side facts of the bidirectional (non-causal) Wan2.1 path: the oracle's identity-slot forward against the reference's
WanModel(model_type="t2v") fixture, the few-step step list, the CLI's choices and refusals, the wrapper's argument errors and
the C ABI's declarations.  No GPU."""
import os
import types

import pytest
import torch

from tests.util import GOLDEN


def _ns(**kw):
    a = dict(duration=1, num_output_frames=21, i2v=False, i2v_model=False, stream=False, rolling=False, preview_vae=None,
             cfg_split=False, bidirectional=True)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_oracle_identity_slots_reproduce_the_reference_forward():
    """oracle dit_forward with frame_ids = write_slots = visible_slots = range(21) == WanModel(model_type='t2v').forward, bit for
    bit (fixture: tests/golden/make_golden_bidir.py): the oracle under oracle/ serves the whole-clip forward unchanged."""
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    from oracle import wan_dit_ref as W
    fx = torch.load(os.path.join(GOLDEN, "bidir_forward_tiny.pt"))
    m = fx["meta"]
    cfg = WAN_CONFIGS[m["cfg"]]
    F_, (h, w) = m["F"], m["lat_hw"]
    S = (h // 2) * (w // 2)
    sd = dit_state_dict(cfg, seed=m["weight_seed"])
    x = philox_normal([16, F_, h, w], m["x_seed"]).to(torch.bfloat16)
    ctx = philox_normal([m["n_valid"], cfg["text_dim"]], m["ctx_seed"]).to(torch.bfloat16)
    ocfg = W.DitCfg(**cfg)
    ident = list(range(F_))
    out = W.dit_forward(sd, ocfg, x, torch.full([1, F_], m["t"], dtype=torch.float32), ctx, W.new_kv_cache(ocfg, F_, S),
                        [None] * ocfg.num_layers, ident, ident, ident)
    assert out.shape == fx["out"].shape == (16, F_, h, w)
    assert torch.equal(out, fx["out"])


class _Gen:
    """What BidirectionalInferencePipeline reads off its generator at construction."""
    is_causal = False

    def __init__(self, shift):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        self.geometry = Geometry(16, 24)
        self.scheduler = FlowMatchScheduler(shift=shift, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)

    def get_scheduler(self):
        return self.scheduler


def test_fewstep_step_list_matches_the_reference():
    from mmpl_amd.pipeline import BidirectionalInferencePipeline
    fx = torch.load(os.path.join(GOLDEN, "bidir_fewstep_tiny.pt"))
    m = fx["meta"]
    mk = lambda steps, warp: BidirectionalInferencePipeline(
        types.SimpleNamespace(denoising_step_list=steps, warp_denoising_step=warp), "cpu", generator=_Gen(m["timestep_shift"]),
        text_encoder=object(), vae=object())
    p = mk(m["denoising_step_list"], m["warp_denoising_step"])
    assert torch.equal(p.denoising_step_list, fx["step_list"])
    assert torch.equal(mk(m["denoising_step_list"] + [0], True).denoising_step_list, fx["step_list"])     # trailing zero removed
    plain = mk([1000, 750, 500, 250, 0], False).denoising_step_list
    assert plain.dtype == torch.long and plain.tolist() == [1000, 750, 500, 250]
    assert p.use_graphs and p.graph_captures == 0 and p.renoise_override is None and p.noise_generator is None


def test_diffusion_pipeline_attributes():
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    args = types.SimpleNamespace(num_train_timestep=1000, timestep_shift=3.0, guidance_scale=5.0, negative_prompt="")
    p = BidirectionalDiffusionInferencePipeline(args, "cpu", generator=_Gen(5.0), text_encoder=object(), vae=object())
    assert (p.sampling_steps, p.sample_solver, p.shift, p.num_train_timesteps) == (50, "unipc", 8.0, 1000)   # shift is not args.timestep_shift
    assert p.use_graphs and p.graph_captures == 0
    causal = _Gen(5.0)
    causal.is_causal = True
    with pytest.raises(ValueError, match="is_causal=False"):
        BidirectionalDiffusionInferencePipeline(args, "cpu", generator=causal, text_encoder=object(), vae=object())


def test_pipeline_class_selection():
    from mmpl_amd import cli
    from mmpl_amd.pipeline import (BidirectionalDiffusionInferencePipeline, BidirectionalInferencePipeline, CausalFPSInferencePipeline,
                                   CausalInferencePipeline)
    few, plain = types.SimpleNamespace(denoising_step_list=[1000, 500]), types.SimpleNamespace()
    assert cli.pipeline_class(few, bidirectional=True) is BidirectionalInferencePipeline
    assert cli.pipeline_class(plain, bidirectional=True) is BidirectionalDiffusionInferencePipeline
    assert cli.pipeline_class(few) is CausalInferencePipeline and cli.pipeline_class(plain) is CausalFPSInferencePipeline


@pytest.mark.parametrize("kw, world, text", [
    (dict(duration=2), 1, "--duration 2"), (dict(i2v=True), 1, "--i2v"), (dict(i2v_model=True), 1, "--i2v"),
    (dict(stream=True), 1, "--stream"), (dict(rolling=True), 1, "--rolling"), (dict(preview_vae=""), 1, "--preview_vae"),
    (dict(cfg_split=True), 1, "--cfg_split"), (dict(), 2, "WORLD_SIZE"), (dict(num_output_frames=25), 1, "--num_output_frames 25")])
def test_bidirectional_refusal(kw, world, text):
    from mmpl_amd import cli
    why = cli.bidirectional_refusal(_ns(**kw), world)
    assert why is not None and text in why


def test_bidirectional_refusal_lets_the_plain_command_line_through():
    from mmpl_amd import cli
    assert cli.bidirectional_refusal(_ns(), 1) is None
    assert cli.bidirectional_refusal(_ns(num_output_frames=9), 1) is None
    assert cli.bidirectional_refusal(_ns(bidirectional=False, duration=3, stream=True), 4) is None     # not asked for


def _bare_wrapper(is_causal):
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    w = WanDiffusionWrapper.__new__(WanDiffusionWrapper)                 # __init__ creates the engine on a GPU
    torch.nn.Module.__init__(w)
    w.is_causal = is_causal
    return w


def test_wrapper_value_errors():
    x, t = torch.zeros(1, 3, 16, 16, 24), torch.zeros(1, 3)
    with pytest.raises(ValueError, match="kv_cache"):
        _bare_wrapper(False)(x, {}, t, kv_cache=[{}])
    with pytest.raises(ValueError, match="kv_cache"):
        _bare_wrapper(False)(x, {}, t, crossattn_cache=[{}])
    with pytest.raises(ValueError, match="KV-cached"):
        _bare_wrapper(True)(x, {}, t)
    for causal in (False, True):
        kw = dict(kv_cache=[{}], crossattn_cache=[{}]) if causal else {}
        with pytest.raises(ValueError, match="training-only"):
            _bare_wrapper(causal)(x, {}, t, classify_mode=True, **kw)
        with pytest.raises(ValueError, match="training-only"):
            _bare_wrapper(causal)(x, {}, t, clean_x=x, **kw)


def test_header_declares_and_lib_binds_the_full_forward():
    import ctypes as C
    from mmpl_amd import _lib
    src = open(_lib.HEADER_PATH).read()
    for name in ("mmpl_dit_full_workspace_bytes", "mmpl_dit_forward_full"):
        assert f" {name}(" in src
        assert name in _lib.SYMBOLS
    restype, argtypes = _lib._PROTOS["mmpl_dit_full_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_void_p, C.c_int]
    restype, argtypes = _lib._PROTOS["mmpl_dit_forward_full"]
    v, i = C.c_void_p, C.c_int
    assert restype is C.c_int and argtypes == [v, v, v, i, v, v, i, v, v, v, v, v, C.c_size_t, v]
