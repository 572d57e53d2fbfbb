"""Host-side facts of the bidirectional Wan2.1 image-to-video path: the oracle's identity-slot forward with `clip_fea` against the
reference's WanModel(model_type="i2v") fixture, the fixtures' own conditions, the CLI's refusals and defaults, the wrapper's and the
pipelines' argument errors, the C ABI's declarations and the rejections that need no device.  No GPU."""
import ctypes as C
import hashlib
import os
import types

import pytest
import torch

from tests.util import GOLDEN, rel_l2

FIXTURES = ("bidir_i2v_forward_tiny.pt", "bidir_i2v_diffusion_unipc_tiny.pt", "bidir_i2v_diffusion_dpmpp_tiny.pt")
P = 0x100000                       # a made-up 16-byte aligned "device pointer" that nothing dereferences


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _ns(**kw):
    a = dict(duration=1, num_output_frames=21, i2v=False, i2v_model=False, image=None, stream=False, rolling=False, preview_vae=None,
             cfg_split=False, bidirectional=True)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_oracle_identity_slots_with_clip_fea_reproduce_the_reference_forward():
    """oracle dit_forward(cat([x, y]), clip_fea=...) with frame_ids = write_slots = visible_slots = range(21) against
    WanModel(model_type='i2v').forward (fixture: tests/golden/make_golden_bidir_i2v.py): the same sha256, or within the fixture's
    own `order_out` -- what the reference itself moves by when its self-attention sums the keys in another order."""
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, philox_normal
    from oracle import wan_dit_ref as W
    fx = torch.load(os.path.join(GOLDEN, FIXTURES[0]))
    m = fx["meta"]
    cfg = WAN_CONFIGS[m["cfg"]]
    F_, (h, w) = m["F"], m["lat_hw"]
    S = (h // 2) * (w // 2)
    sd = dit_i2v_state_dict(cfg, seed=m["weight_seed"])
    x = philox_normal([16, F_, h, w], m["x_seed"]).to(torch.bfloat16)
    y = philox_normal([20, F_, h, w], m["y_seed"]).to(torch.bfloat16)
    clip_fea = philox_normal([257, 1280], m["clip_seed"]).to(torch.bfloat16)
    ctx = philox_normal([m["n_valid"], cfg["text_dim"]], m["ctx_seed"]).to(torch.bfloat16)
    ocfg = W.DitCfg(**dict(cfg, in_dim=36))
    ident = list(range(F_))
    out = W.dit_forward(sd, ocfg, torch.cat([x, y], dim=0), torch.full([1, F_], m["t"], dtype=torch.float32), ctx,
                        W.new_kv_cache(ocfg, F_, S), [None] * ocfg.num_layers, ident, ident, ident, clip_fea=clip_fea)
    assert out.shape == fx["out"].shape == (16, F_, h, w)
    e = rel_l2(out, fx["out"])
    print(f"[bidir i2v] oracle vs reference forward: rel_l2 {e:.3e} (order_out {fx['order_out']:.3e}), sha equal: {_sha(out) == fx['out_sha']}")
    assert _sha(out) == fx["out_sha"] or e <= fx["order_out"]


def test_fixture_conditions():
    """What the issue asks of the fixtures: the tiny i2v model at 21 frames of 16 x 24 latents, 6 CFG steps at guidance 5 per solver,
    a sha256 of the full output, a positive `order_out` below the per-forward bound, and files within the committed-file limit."""
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20, name
        fx = torch.load(os.path.join(GOLDEN, name))
        m = fx["meta"]
        assert (m["cfg"], m["F"], tuple(m["lat_hw"])) == ("tiny", 21, (16, 24)), name
        assert {"weight_seed", "ctx_seed", "clip_seed", "y_seed", "n_valid"} <= set(m), name
        assert len(fx["out_sha"]) == 64 and 0.0 < fx["order_out"] < 2e-2, (name, fx["order_out"])
    fwd = torch.load(os.path.join(GOLDEN, FIXTURES[0]))
    assert fwd["out"].dtype == torch.bfloat16 and _sha(fwd["out"]) == fwd["out_sha"]
    for name, solver in zip(FIXTURES[1:], ("unipc", "dpm++")):
        fx = torch.load(os.path.join(GOLDEN, name))
        m = fx["meta"]
        assert (m["sampling_steps"], m["guidance_scale"], m["sample_solver"], m["shift"]) == (6, 5.0, solver, 8.0)
        assert tuple(fx["out_strided"].shape) == (1, 21, 16, 8, 12) and len(fx["timesteps"]) == 6
        assert torch.isfinite(fx["out_strided"].float()).all()


def test_bidirectional_refusal_lets_the_i2v_model_type_through():
    from mmpl_amd import cli
    assert cli.bidirectional_refusal(_ns(i2v=True, i2v_model=True, image="cat.png"), 1) is None
    for kw in (dict(i2v=True), dict(i2v_model=True), dict(image="cat.png", i2v=True), dict(i2v=True, i2v_model=True),
               dict(i2v_model=True, image="cat.png")):
        why = cli.bidirectional_refusal(_ns(**kw), 1)
        assert why is not None and "--i2v" in why, kw
    # the other refusals still hold with the image flags on, and nothing is refused when --bidirectional was not asked for
    on = dict(i2v=True, i2v_model=True, image="cat.png")
    assert "--stream" in cli.bidirectional_refusal(_ns(stream=True, **on), 1)
    assert "WORLD_SIZE" in cli.bidirectional_refusal(_ns(**on), 2)
    assert "--i2v" in cli.bidirectional_refusal(_ns(fewstep=True, **on), 1)                  # no few-step i2v checkpoint exists
    assert cli.bidirectional_refusal(_ns(bidirectional=False, **on), 1) is None


class _Gen:
    """What the bidirectional pipelines read off their generator at construction."""
    is_causal = False

    def __init__(self, model_type):
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.scheduler import FlowMatchScheduler
        self.model_type = model_type
        self.geometry = Geometry(16, 24)
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)

    def get_scheduler(self):
        return self.scheduler


def test_pipeline_value_errors():
    """image_condition over a t2v generator, none (or half of one) over an i2v generator: ValueError before any work; the few-step
    pipeline refuses an i2v generator at construction."""
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline, BidirectionalInferencePipeline
    args = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="")
    noise = torch.zeros(1, 21, 16, 16, 24)
    cond = {"clip_fea": torch.zeros(257, 1280), "y": torch.zeros(20, 21, 16, 24)}
    t2v = BidirectionalDiffusionInferencePipeline(args, "cpu", generator=_Gen("t2v"), text_encoder=object(), vae=object())
    assert t2v.i2v is False
    with pytest.raises(ValueError, match="image_condition"):
        t2v.inference(noise, ["p"], image_condition=cond)
    i2v = BidirectionalDiffusionInferencePipeline(args, "cpu", generator=_Gen("i2v"), text_encoder=object(), vae=object())
    assert i2v.i2v is True and (i2v.sampling_steps, i2v.shift) == (50, 8.0)
    for bad in (None, {"clip_fea": cond["clip_fea"]}, {"y": cond["y"]}):
        with pytest.raises(ValueError, match="image_condition"):
            i2v.inference(noise, ["p"], image_condition=bad)
    few = types.SimpleNamespace(denoising_step_list=[1000, 500])
    with pytest.raises(ValueError, match="text-to-video only"):
        BidirectionalInferencePipeline(few, "cpu", generator=_Gen("i2v"), text_encoder=object(), vae=object())
    BidirectionalInferencePipeline(few, "cpu", generator=_Gen("t2v"), text_encoder=object(), vae=object())


def _bare_wrapper(model_type):
    from mmpl_amd.wan_wrapper import WanDiffusionWrapper
    w = WanDiffusionWrapper.__new__(WanDiffusionWrapper)                 # __init__ creates the engine on a GPU
    torch.nn.Module.__init__(w)
    w.is_causal, w.model_type = False, model_type
    return w


def test_wrapper_value_errors():
    x, t = torch.zeros(1, 3, 16, 16, 24), torch.zeros(1, 3)
    pe, fea, y = torch.zeros(1, 512, 256), torch.zeros(257, 1280), torch.zeros(20, 3, 16, 24)
    for d in ({"prompt_embeds": pe}, {"prompt_embeds": pe, "clip_fea": fea}, {"prompt_embeds": pe, "y": y}):
        with pytest.raises(ValueError, match="clip_fea and y"):
            _bare_wrapper("i2v")(x, d, t)
    with pytest.raises(ValueError, match="t2v model"):
        _bare_wrapper("t2v").set_image(fea)


def test_header_declares_and_lib_binds_the_new_symbols():
    from mmpl_amd import _lib
    src = open(_lib.HEADER_PATH).read()
    for name in ("mmpl_patchify2", "mmpl_dit_forward_full_i2v"):
        assert f" {name}(" in src
        assert name in _lib.SYMBOLS
    v, i = C.c_void_p, C.c_int
    restype, argtypes = _lib._PROTOS["mmpl_patchify2"]
    assert restype is C.c_int and argtypes == [v, v, v, i, i, i, i, i, i, v]
    restype, argtypes = _lib._PROTOS["mmpl_dit_forward_full_i2v"]
    assert restype is C.c_int and argtypes == [v, v, v, v, i, v, v, i, v, v, v, v, v, C.c_size_t, v]
    lib = _lib.load()                                                    # load() raises for a declared symbol the library lacks
    for name in ("mmpl_patchify2", "mmpl_dit_forward_full_i2v"):
        assert getattr(lib, name).argtypes == _lib._PROTOS[name][1]
    assert "mmpl_launch_patchify2(" in open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "csrc", "kernels.h")).read()


def test_patchify2_rejects_before_any_hip_call():
    """Each call is wrong in exactly one way; the pointers are made-up addresses, so a launch would fault rather than pass."""
    from mmpl_amd import _lib
    lib = _lib.load()

    def e(rc):
        assert rc != 0
        return lib.mmpl_last_error().decode()

    ok = dict(x=P, y=P, a=P, lda=192, F=3, Cx=16, Cy=20, h=4, w=6)

    def call(**kw):
        a = dict(ok, **kw)
        return e(lib.mmpl_patchify2(a["x"], a["y"], a["a"], a["lda"], a["F"], a["Cx"], a["Cy"], a["h"], a["w"], None))

    for kw in (dict(x=None), dict(y=None), dict(a=None)):
        assert "mmpl_patchify2: null argument" in call(**kw), kw
    for kw in (dict(F=0), dict(Cx=0), dict(Cy=0), dict(h=0), dict(w=-2)):
        assert "non-positive" in call(**kw), kw
    assert "odd h or w" in call(h=5)
    assert "odd h or w" in call(w=7)
    assert "lda < 4 (Cx + Cy)" in call(lda=143)
    assert "lda < 4 (Cx + Cy)" in call(lda=64)                           # enough for x alone, as mmpl_patchify would take it
    assert "lda < 4 (Cx + Cy)" in call(Cx=1 << 30)
    assert "too many pixels" in call(F=2, h=1 << 16, w=1 << 14)
    for kw in (dict(x=P + 1), dict(y=P + 1), dict(a=P + 1)):
        assert "misaligned" in call(**kw), kw


def test_forward_full_i2v_rejects_a_null_handle_before_any_hip_call():
    """Without a device there is no handle to make (mmpl_dit_create allocates the RoPE tables): the null handle is the one rejection a
    host can reach; tests/test_bidir_i2v_forward_gpu.py makes every other one."""
    from mmpl_amd import _lib
    lib = _lib.load()
    rc = lib.mmpl_dit_forward_full_i2v(None, P, P, P, 3, P, P, 512, None, None, None, P, P, 1 << 20, None)
    assert rc != 0 and "mmpl_dit_forward_full_i2v: null handle" in lib.mmpl_last_error().decode()


def test_cli_defaults_follow_wan_i2v_generate(monkeypatch, tmp_path):
    """--bidirectional --i2v --i2v_model with nothing else said: 40 steps and shift 3.0 at 480p / 5.0 at 720p (WanI2V.generate); what
    the user gives wins; text-to-video keeps 50 steps and the pipeline's own 8.0; --sample_shift needs --bidirectional."""
    from mmpl_amd import cli
    seen = {}

    def stop(config, args, dev, geo, mcfg):
        seen.update(steps=args.sampling_steps, shift=args.sample_shift)
        raise SystemExit(0)

    monkeypatch.setattr(cli, "_main_bidirectional", stop)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    base = ["--synthetic", "--model", "tiny", "--duration", "1", "--bidirectional"]
    img = ["--i2v", "--i2v_model", "--image", str(tmp_path / "x.png")]
    for extra, want in ((img, (40, 3.0)), (img + ["--resolution", "720p"], (40, 5.0)),
                        (img + ["--sampling_steps", "7", "--sample_shift", "4.5"], (7, 4.5)), ([], (50, None)),
                        (["--sample_shift", "6"], (50, 6.0))):
        with pytest.raises(SystemExit) as ex:
            cli.main(base + extra)
        assert ex.value.code == 0 and (seen["steps"], seen["shift"]) == want, (extra, seen)
    with pytest.raises(SystemExit) as ex:
        cli.main(["--synthetic", "--model", "tiny", "--sample_shift", "6"])
    assert ex.value.code != 0
