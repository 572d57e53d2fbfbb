"""TAEHV preview decoder on the MI355X (-m gpu): parity with the real reference's output (tests/golden/taehv_tiny.pt), streaming
as the same function as the one-shot decode, the uint8 format, ragged and full-size shapes against tests/taehv_ref.py, hipGraph
capture of a streamed call, TAEHVWrapper's frame contract, and inference_stream(decoder="preview").

Parity bound: 2 x ref_bf16_rel_l2, the distance of the reference's OWN all-bf16 evaluation to its fp32 one, read from the fixture
(6.2e-3 when it was generated).  Two independent bf16 roundings of one network sit about sqrt(2) of one rounding's distance apart;
2 x a measured noise floor is the factor this project uses for bf16 bounds (tests/test_trajectory_gpu.py)."""
import os
import types

import pytest
import torch

import taehv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPLITS = [[5], [1, 4], [3, 2], [1, 1, 1, 1, 1], [2, 2, 1]]


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "taehv_tiny.pt"))


def _engine(lat, seed=5):
    from mmpl_amd.synthetic import taehv_state_dict
    from mmpl_amd.taehv import TaehvEngine
    sd = taehv_state_dict(seed=seed)
    eng = TaehvEngine(lat[0], lat[1], DEV)
    eng.load_state_dict(sd)
    return eng, sd


def _to_u8(x):
    """float [T, 3, H, W] -> uint8 [T, H, W, 3] the way the header states it: (x.clamp(0, 1) * 255) truncated"""
    return (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_parity_with_the_reference(fx):
    from mmpl_amd.synthetic import philox_normal
    m = fx["meta"]
    eng, _ = _engine(m["z_shape"][2:], seed=m["weight_seed"])
    z = philox_normal(m["z_shape"], m["z_seed"]).to(DEV)
    out = eng.decode(z)
    assert out.shape == (12, 3, 64, 96) and out.dtype == torch.float32 and torch.isfinite(out).all()
    d = taehv_ref.rel_l2(out.cpu(), fx["exact"])
    bound = 2 * fx["ref_bf16_rel_l2"]
    print(f"engine vs reference (fp32): rel L2 {d:.3e}; the reference's own bf16: {fx['ref_bf16_rel_l2']:.3e}; bound {bound:.3e}")
    assert d <= bound
    assert float(out.min()) < 0 and float(out.max()) > 1, "the float output is the network's, unclamped"


def test_patch_tgrow_layers(fx):
    """A checkpoint whose first TGrow has 2 * 256 rows: the engine keeps the last 256, like the reference's loader."""
    from mmpl_amd.synthetic import philox_normal, taehv_state_dict
    from mmpl_amd.taehv import TaehvEngine
    tg = fx["tgrow"]
    sd = taehv_state_dict(seed=fx["meta"]["weight_seed"])
    g = torch.Generator().manual_seed(tg["extra_seed"])
    extra = (torch.randn(256, 256, 1, 1, generator=g) * (1.0 / 16)).to(torch.bfloat16)
    big = dict(sd)
    big["decoder.7.conv.weight"] = torch.cat([extra, sd["decoder.7.conv.weight"]], 0)
    big["encoder.0.weight"] = torch.zeros(64, 3, 3, 3)                      # encoder keys are ignored
    eng = TaehvEngine(tg["z_shape"][2], tg["z_shape"][3], DEV)
    eng.load_state_dict(big)
    out = eng.decode(philox_normal(tg["z_shape"], tg["z_seed"]).to(DEV))
    d = taehv_ref.rel_l2(out.cpu(), tg["out"])
    print(f"patch_tgrow case: rel L2 {d:.3e}")
    assert d <= 2 * fx["ref_bf16_rel_l2"]


def test_streaming_is_the_same_function():
    from mmpl_amd.synthetic import philox_normal
    eng, _ = _engine((8, 12))
    z = philox_normal([5, 16, 8, 12], 47).to(DEV)
    one = {f: eng.decode(z, out_format=f).clone() for f in ("float", "uint8")}
    assert one["float"].shape == (20, 3, 64, 96) and one["uint8"].shape == (20, 64, 96, 3) and one["uint8"].dtype == torch.uint8
    for fmt in ("float", "uint8"):
        for split in SPLITS:
            eng.clear_cache()
            parts, f0 = [], 0
            for n in split:
                parts.append(eng.decode_stream(z[f0:f0 + n], out_format=fmt))
                assert parts[-1].shape[0] == 4 * n
                f0 += n
            assert torch.equal(torch.cat(parts), one[fmt]), (fmt, split)
    # without clear_cache() a call continues the video; after it the video starts over
    eng.clear_cache()
    eng.decode_stream(z[:4])
    cont = eng.decode_stream(z[4:5])
    assert cont.shape[0] == 4 and torch.equal(cont, one["float"][16:])
    assert not torch.equal(eng.decode_stream(z[:1]), one["float"][:4])       # latent 0 behind latent 4: not a first frame
    eng.clear_cache()
    assert torch.equal(eng.decode_stream(z[:1]), one["float"][:4])


def test_uint8_is_the_float_output_converted(fx):
    from mmpl_amd.synthetic import philox_normal
    eng, _ = _engine((8, 12))
    z = philox_normal([3, 16, 8, 12], fx["meta"]["z_seed"]).to(DEV)
    f = eng.decode(z, out_format="float")
    u = eng.decode(z, out_format="uint8")
    assert torch.equal(u, _to_u8(f))
    assert 0 < int((u == 0).sum()) and 0 < int((u == 255).sum()) and int(((u > 0) & (u < 255)).sum()) > u.numel() // 2


def _device_reference(sd, z):
    """tests/taehv_ref.py in fp32 on the device, on the bf16-rounded weights and input the engine sees"""
    with torch.no_grad():
        return taehv_ref.decode_video(sd, z.float(), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("lat,frames", [((9, 13), 3), ((8, 12), 3), ((60, 104), 2)])
def test_ragged_and_fullsize_shapes(fx, lat, frames):
    from mmpl_amd.synthetic import philox_normal
    eng, sd = _engine(lat)
    z = philox_normal([frames, 16, *lat], 48).to(DEV)
    out = eng.decode(z)
    assert out.shape == (4 * frames, 3, 8 * lat[0], 8 * lat[1])
    assert torch.isfinite(out).all(), "NaN / Inf in the decoded frames"
    ref = _device_reference(sd, z)
    d = taehv_ref.rel_l2(out, ref)
    bound = 2 * fx["ref_bf16_rel_l2"]
    print(f"latents {lat} x {frames}: rel L2 to the fp32 restatement {d:.3e} (bound {bound:.3e})")
    assert d <= bound
    # streamed, one latent per call, is the same function at this size too
    eng.clear_cache()
    parts = [eng.decode_stream(z[i:i + 1]) for i in range(frames)]
    assert torch.equal(torch.cat(parts), out)


def test_streamed_call_is_capturable():
    from mmpl_amd.synthetic import philox_normal
    eng, _ = _engine((8, 12))
    z = philox_normal([3, 2, 16, 8, 12], 49).to(DEV)                        # three calls of 2 latents
    eng.clear_cache()
    eager = [eng.decode_stream(z[i]).clone() for i in range(3)]
    eng.clear_cache()
    first = eng.decode_stream(z[0])                                         # a video's first call clears the workspace: eager
    assert torch.equal(first, eager[0])
    buf = z[1].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.decode_stream(buf)
    for i in (1, 2):
        buf.copy_(z[i])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), f"replay {i}"
    del g


def test_wrapper_frame_contract():
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import philox_normal, taehv_state_dict, vae_state_dict
    from mmpl_amd.wan_wrapper import TAEHVWrapper, WanVAEWrapper
    geo = Geometry(8, 12)
    tiny = TAEHVWrapper(geometry=geo, device=DEV, state_dict=taehv_state_dict(seed=5))
    wan = WanVAEWrapper(geometry=geo, device=DEV, state_dict=vae_state_dict(seed=2))
    z = philox_normal([1, 5, 16, 8, 12], 50).to(DEV)
    raw = tiny.model.decode(z[0]).clone()                                    # the engine: 20 frames, untrimmed
    assert raw.shape[0] == 20
    want = (raw * 2 - 1).clamp(-1, 1)
    for w in (tiny, wan):
        w.model.clear_cache()
    shapes = {}
    for name, w in (("tiny", tiny), ("wan", wan)):
        a = w.decode_to_pixel(z[:, :2], use_cache=True)
        b = w.decode_to_pixel(z[:, 2:5], use_cache=True)
        c = w.decode_to_pixel(z, use_cache=False)
        w.model.clear_cache()
        d = w.decode_to_pixel(z[:, :1], use_cache=True)
        shapes[name] = [tuple(t.shape) for t in (a, b, c, d)]
        if name == "tiny":
            assert all(t.dtype == torch.float32 for t in (a, b, c, d))
            assert torch.equal(torch.cat([a, b], 1)[0], want[3:]) and torch.equal(c[0], want[3:]) and torch.equal(d[0], want[3:4])
            assert float(c.min()) >= -1 and float(c.max()) <= 1
    assert shapes["tiny"] == shapes["wan"] == [(1, 5, 3, 64, 96), (1, 12, 3, 64, 96), (1, 17, 3, 64, 96), (1, 1, 3, 64, 96)]


LAT = (16, 24)


def _pipe():
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, taehv_state_dict, vae_state_dict
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, TAEHVWrapper, WanDiffusionWrapper, WanVAEWrapper
    cfg = WAN_CONFIGS["tiny"]
    geo = Geometry(*LAT)
    args = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                                 independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=geo, device=DEV)
    gen.load_state_dict(dit_state_dict(cfg, seed=1, device=DEV))
    vae = WanVAEWrapper(geometry=geo, device=DEV, state_dict=vae_state_dict(seed=2))
    tiny = TAEHVWrapper(geometry=geo, device=DEV, state_dict=taehv_state_dict(seed=4))
    return CausalInferencePipeline(args, DEV, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), DEV), vae=vae,
                                   preview_vae=tiny)


def _collect(pipe, noise, output, overlap, decoder):
    torch.manual_seed(5)
    firsts, parts = [], []
    for first, frames in pipe.inference_stream(noise, ["p"], output=output, overlap=overlap, decoder=decoder):
        firsts.append(first)
        parts.append(frames)
    return firsts, parts


def test_pipeline_preview_decoder():
    from mmpl_amd.synthetic import philox_normal
    pipe = _pipe()
    noise = philox_normal([1, 9, 16, *LAT], 75).to(DEV)
    torch.manual_seed(5)
    _, lat = pipe.inference(noise, ["p"], return_latents=True)
    v_firsts, v_parts = _collect(pipe, noise, "uint8", True, "vae")
    captures = pipe.graph_captures
    eng = pipe.preview_vae.model
    for output in ("uint8", "float"):
        got = {}
        for overlap in (True, False):
            firsts, parts = _collect(pipe, noise, output, overlap, "preview")
            assert firsts == v_firsts == [0, 9, 21]
            assert [p.shape[0] for p in parts] == [p.shape[0] for p in v_parts] == [9, 12, 12]
            assert torch.equal(pipe._out[9].to(lat.dtype), lat), "the latents do not depend on the decoder"
            got[overlap] = torch.cat(parts)
        assert torch.equal(got[True], got[False]), output
        one = eng.decode(pipe._out[9][0], out_format=output)[3:]              # the engine's one-shot decode, first 3 frames dropped
        if output == "uint8":
            assert not got[True].is_cuda and got[True].dtype == torch.uint8
            assert torch.equal(got[True], one.cpu())
        else:
            assert got[True].is_cuda and got[True].dtype == torch.float32
            assert torch.equal(got[True], one.clamp(0, 1))
    assert pipe.graph_captures == captures, "the preview decoder constructs no hipGraph"
    # and the Wan VAE's stream is what it was
    again_firsts, again = _collect(pipe, noise, "uint8", True, "vae")
    assert again_firsts == v_firsts and torch.equal(torch.cat(again), torch.cat(v_parts))
    pipe.release_graphs()


def test_cli_stream_with_preview_vae(tmp_path):
    from mmpl_amd import cli
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    cli.main(["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--num_output_frames", "9",
              "--config_path", str(cfg), "--output_folder", str(tmp_path), "--stream", "--preview_vae"])
    a = torch.load(tmp_path / "0-0.pt")
    assert tuple(a.shape) == (33, 128, 192, 3) and a.dtype == torch.uint8
    assert float(a.float().std()) > 1.0, "a picture, not a constant"
