"""The HIP TAEHV encoder end to end (mmpl_taehv_encode behind TaehvEncoderEngine / TAEHVWrapper), the few-step pipeline fed by it
and the CLI's --extend.

Accuracy bound: rel L2 <= 2 x ref_bf16_rel_l2 of tests/golden/taehv_enc_tiny.pt -- twice the distance of the reference's own
all-bf16 evaluation from its fp32 one, the project's bf16 bound -- against the real reference's output where the fixture holds it
and against the fp32 restatement (tests/taehv_enc_ref.py, itself held to the fixture in tests/test_taehv_enc_host.py) elsewhere.
Streaming, the input formats and graph replay are checked bit for bit."""
import os
import types

import pytest
import torch

import taehv_enc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taehv_enc_tiny.pt")
WEIGHT_SEED = 7
_cache = {}


def _fixture():
    if "fx" not in _cache:
        _cache["fx"] = torch.load(GOLDEN, weights_only=True)
    return _cache["fx"]


def _sd():
    from mmpl_amd.synthetic import taehv_encoder_state_dict
    if "sd" not in _cache:
        _cache["sd"] = taehv_encoder_state_dict(seed=WEIGHT_SEED)
    return _cache["sd"]


def _engine(lat):
    from mmpl_amd.taehv import TaehvEncoderEngine
    if lat not in _cache:
        eng = TaehvEncoderEngine(*lat, device=DEV)
        eng.load_state_dict(_sd())
        _cache[lat] = eng
    return _cache[lat]


def _pixels(shape, seed):
    """sigmoid of seeded normals, rounded to bf16: float32 [T, 3, H, W] in (0, 1)"""
    from mmpl_amd.synthetic import philox_normal
    return torch.sigmoid(philox_normal(list(shape), seed).float()).to(torch.bfloat16).float()


def test_engine_matches_the_reference():
    fx = _fixture()
    m = fx["meta"]
    assert m["weight_seed"] == WEIGHT_SEED
    px = _pixels(m["px_shape"], m["px_seed"])
    z = _engine((4, 6)).encode(px.to(DEV))
    assert z.dtype == torch.bfloat16 and tuple(z.shape) == (3, 16, 4, 6)
    err = R.rel_l2(z.float().cpu(), fx["exact"])
    print(f"engine vs the reference: rel L2 {err:.3e}, bound {2 * fx['ref_bf16_rel_l2']:.3e}")
    assert err <= 2 * fx["ref_bf16_rel_l2"]


def test_any_split_is_bit_identical():
    """16 frames cross the 3-latent group boundary inside one call and between calls"""
    eng = _engine((4, 6))
    px = _pixels([16, 3, 32, 48], 46).to(DEV)
    whole = eng.encode(px).clone()
    assert tuple(whole.shape) == (4, 16, 4, 6)
    for split in ([4, 12], [12, 4], [4, 4, 4, 4]):
        eng.clear_cache()
        parts, f0 = [], 0
        for n in split:
            parts.append(eng.encode_stream(px[f0:f0 + n]).clone())
            f0 += n
        assert torch.equal(torch.cat(parts), whole), split
    # clear_cache() restarts the video; without it the same frames continue it
    cont = eng.encode_stream(px[:4]).clone()
    assert not torch.equal(cont, whole[:1])
    eng.clear_cache()
    assert torch.equal(eng.encode_stream(px[:4]), whole[:1])


def test_uint8_input_equals_float_input():
    eng = _engine((4, 6))
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (8, 32, 48, 3), generator=g, dtype=torch.uint8)
    a = eng.encode(u.to(DEV)).clone()
    b = eng.encode((u.float() / 255).permute(0, 3, 1, 2).contiguous().to(DEV))
    assert torch.equal(a, b)
    assert float(a.float().std()) > 0.1


def test_bad_frame_counts_raise_before_the_device():
    eng = _engine((4, 6))
    for T in (0, 5, 6):
        with pytest.raises(ValueError, match="multiple of 4"):
            eng.encode_stream(torch.zeros(T, 3, 32, 48))
        with pytest.raises(ValueError, match="multiple of 4"):
            eng.encode(torch.zeros(T, 32, 48, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        eng.encode(torch.zeros(4, 3, 32, 40))


def test_workspace_may_not_change_between_resets():
    import ctypes as C
    from mmpl_amd import _lib
    eng = _engine((4, 6))
    lib, px = eng._lib, _pixels([4, 3, 32, 48], 51).to(DEV)
    want = eng.encode(px).clone()                                           # binds eng._ws for this video
    other = torch.empty_like(eng._ws)
    z = torch.empty_like(want)
    call = lambda ws: lib.mmpl_taehv_encode(eng._h, _lib.ptr(px), 0, 4, _lib.ptr(z), None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())  # noqa: E731
    assert call(other) != 0 and "reset first" in lib.mmpl_last_error().decode()
    eng.clear_cache()
    assert call(other) == 0                                                 # after a reset another workspace starts a new video
    torch.cuda.synchronize()
    assert torch.equal(z, want)
    eng.clear_cache()


@pytest.mark.parametrize("lat,T", [((5, 7), 8), ((9, 13), 8), ((60, 104), 4)], ids=["5x7", "9x13", "480p"])
def test_ragged_and_full_size(lat, T):
    """sizes that are no multiple of any patch, and the production size, against the fp32 restatement (on the device through
    PyTorch where the CPU would take long)"""
    fx = _fixture()
    px = _pixels([T, 3, 8 * lat[0], 8 * lat[1]], 47)
    big = lat[0] * lat[1] > 1000
    from mmpl_amd.taehv import TaehvEncoderEngine
    eng = TaehvEncoderEngine(*lat, device=DEV) if big else _engine(lat)
    if big:
        eng.load_state_dict(_sd())
    z = eng.encode(px.to(DEV)).float().cpu()
    ref = R.encode_video({k: v.float() for k, v in _sd().items()}, px, device=DEV if big else "cpu").cpu()
    err = R.rel_l2(z, ref)
    print(f"lat {lat}, {T} frames: rel L2 {err:.3e}, bound {2 * fx['ref_bf16_rel_l2']:.3e}")
    assert tuple(z.shape) == (T // 4, 16, *lat)
    assert err <= 2 * fx["ref_bf16_rel_l2"]


def test_streamed_call_is_capturable():
    eng = _engine((4, 6))
    px = _pixels([12, 3, 32, 48], 48).to(DEV)
    eng.clear_cache()
    eager = [eng.encode_stream(px[4 * i:4 * i + 4]).clone() for i in range(3)]
    eng.clear_cache()
    first = eng.encode_stream(px[:4])                                       # a video's first call clears the workspace: eager
    assert torch.equal(first, eager[0])
    buf = px[4:8].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.encode_stream(buf)
    for i in (1, 2):
        buf.copy_(px[4 * i:4 * i + 4])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), f"replay {i}"
    del g
    eng.clear_cache()


def _wrapper(lat, encoder=True):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import taehv_state_dict
    from mmpl_amd.wan_wrapper import TAEHVWrapper
    sd = dict(taehv_state_dict(seed=4))
    if encoder:
        sd.update(_sd())
    return TAEHVWrapper(geometry=Geometry(*lat), device=DEV, state_dict=sd)


def test_wrapper_encode_to_latent():
    w = _wrapper((4, 6))
    px = _pixels([13, 3, 32, 48], 49).to(DEV)
    video = (px * 2 - 1).permute(1, 0, 2, 3).unsqueeze(0)                    # [1, 3, 13, H, W] in [-1, 1]
    a = w.encode_to_latent(video[:, :, :12])
    b = w.encode_to_latent(video)
    assert tuple(a.shape) == (1, 3, 16, 4, 6) and tuple(b.shape) == (1, 4, 16, 4, 6) and a.dtype == torch.float32
    # T = 4k is the engine's encode; T = 1 + 4k repeats the first frame three times in front
    v = (video[0].permute(1, 0, 2, 3).float() + 1) * 0.5                    # what the wrapper hands the engine
    assert torch.equal(a[0], w.encoder.encode(v[:12]).float())
    assert torch.equal(b[0], w.encoder.encode(torch.cat([v[:1]] * 3 + [v])).float())
    with pytest.raises(ValueError):
        w.encode_to_latent(video[:, :, :6])
    # encode -> decode gives the input's frame count back (the decoder drops the video's first 3 frames)
    assert w.decode_to_pixel(b).shape[1] == 13
    dec_only = _wrapper((4, 6), encoder=False)
    assert dec_only.encoder is None
    with pytest.raises(RuntimeError, match="encoder"):
        dec_only.encode_to_latent(video)


LAT = (16, 24)


def _pipe():
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, vae_state_dict
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper, WanVAEWrapper
    cfg = WAN_CONFIGS["tiny"]
    geo = Geometry(*LAT)
    args = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                                 independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=geo, device=DEV)
    gen.load_state_dict(dit_state_dict(cfg, seed=1, device=DEV))
    vae = WanVAEWrapper(geometry=geo, device=DEV, state_dict=vae_state_dict(seed=2))
    return CausalInferencePipeline(args, DEV, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), DEV), vae=vae,
                                   preview_vae=_wrapper(LAT))


def test_pipeline_continues_an_encoded_context():
    from mmpl_amd.synthetic import philox_normal
    pipe = _pipe()
    px = _pixels([12, 3, 8 * LAT[0], 8 * LAT[1]], 50).to(DEV)
    initial = pipe.preview_vae.encode_to_latent((px * 2 - 1).permute(1, 0, 2, 3).unsqueeze(0))
    assert tuple(initial.shape) == (1, 3, 16, *LAT)
    noise = philox_normal([1, 6, 16, *LAT], 76).to(DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        firsts, counts = [], []
        for first, frames in pipe.inference_stream(noise, ["p"], initial_latent=initial, output="uint8", decoder="preview"):
            firsts.append(first)
            counts.append(frames.shape[0])
        assert firsts == [0, 9, 21] and counts == [9, 12, 12]              # the context's frames first, then every block
        runs.append(pipe._out[9].clone())
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(runs[0][0, :3], initial[0].to(runs[0].dtype)), "the context latents lead the video"
    pipe.release_graphs()


def test_cli_extend(tmp_path, monkeypatch):
    from mmpl_amd import cli
    from mmpl_amd.pipeline import CausalInferencePipeline
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    common = ["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--config_path", str(cfg), "--stream",
              "--preview_vae"]
    first = tmp_path / "first"
    cli.main(common + ["--num_output_frames", "6", "--output_folder", str(first)])
    clip = torch.load(first / "0-0.pt")
    assert tuple(clip.shape) == (21, 128, 192, 3) and clip.dtype == torch.uint8

    seen = {}
    stream = CausalInferencePipeline.inference_stream

    def spy(self, noise, prompts, initial_latent=None, **kw):
        seen["initial"], seen["pipe"] = initial_latent.clone(), self
        return stream(self, noise, prompts, initial_latent=initial_latent, **kw)

    monkeypatch.setattr(CausalInferencePipeline, "inference_stream", spy)
    second = tmp_path / "second"
    cli.main(common + ["--num_output_frames", "3", "--output_folder", str(second), "--extend", str(first / "0-0.pt")])
    out = torch.load(second / "0-0.pt")
    assert tuple(out.shape) == (4 * (3 + 3), 128, 192, 3) and out.dtype == torch.uint8
    assert torch.equal(out[:12], clip[-12:]), "the context frames are the file's"
    assert float(out[12:].float().std()) > 1.0, "a picture, not a constant"
    enc = seen["pipe"].preview_vae.encoder
    assert tuple(seen["initial"].shape) == (1, 3, 16, 16, 24)
    assert torch.equal(seen["initial"][0], enc.encode(clip[-12:].to(DEV)))
