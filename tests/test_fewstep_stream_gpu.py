"""Block-wise output of the few-step pipeline on the MI355X (-m gpu): CausalInferencePipeline.inference_stream hands out the
video ``inference()`` returns, bit for bit, in every mode (decode overlapped on a second stream or in order, float or uint8
frames, with / without initial_latent, independent_first_frame); graph reuse; early close; one Wan 1.3B / 480p case where both
streams carry long kernels; the CLI's --stream."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)


def _args(**kw):
    a = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
             independent_first_frame=False, context_noise=0, model_kwargs={"timestep_shift": 5.0})
    a.update(kw)
    return types.SimpleNamespace(**a)


def _pipe(cfg_name="tiny", lat=LAT, **kw):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, vae_state_dict
    from mmpl_amd.wan_wrapper import SyntheticTextEncoder, WanDiffusionWrapper, WanVAEWrapper
    cfg = WAN_CONFIGS[cfg_name]
    geo = Geometry(*lat)
    gen = WanDiffusionWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=geo, device=DEV)
    gen.load_state_dict(dit_state_dict(cfg, seed=1, device=DEV))
    vae = WanVAEWrapper(geometry=geo, device=DEV, state_dict=vae_state_dict(seed=2))
    return CausalInferencePipeline(_args(**kw), DEV, generator=gen, text_encoder=SyntheticTextEncoder(cfg.get("text_dim", 4096), DEV),
                                   vae=vae)


def _to_u8(video):
    """What mmpl_amd/cli.py does to inference()'s video: [1, T, 3, H, W] in [0, 1] -> uint8 [T, H, W, 3] on the host."""
    return (video * 255.0).clamp(0, 255).to(torch.uint8)[0].permute(0, 2, 3, 1).contiguous().cpu()


def _collect(pipe, noise, init, output, overlap, seed=5):
    torch.manual_seed(seed)
    firsts, parts = [], []
    for first, frames in pipe.inference_stream(noise, ["p"], initial_latent=init, output=output, overlap=overlap):
        assert first == sum(p.shape[0] for p in parts), "yields are consecutive pixel frames"
        firsts.append(first)
        parts.append(frames)
    return firsts, parts


CASES = {   # name: (independent_first_frame, initial latent frames, noise frames, pixel frames per yield)
    "plain": (False, 0, 21, [9] + [12] * 6),
    "initial_latent": (False, 3, 18, [9] + [12] * 6),
    "independent_first_frame": (True, 0, 19, [1] + [12] * 6),
    "independent_first_frame_initial": (True, 1, 18, [1] + [12] * 6),
}


@pytest.mark.parametrize("case", list(CASES))
def test_stream_equals_inference(case):
    from mmpl_amd.synthetic import philox_normal
    iff, n_init, n_noise, per_yield = CASES[case]
    pipe = _pipe(independent_first_frame=iff)
    noise = philox_normal([1, n_noise, 16, *LAT], 71).to(DEV)
    init = philox_normal([1, n_init, 16, *LAT], 72).to(DEV) if n_init else None
    torch.manual_seed(5)
    video, lat = pipe.inference(noise, ["p"], initial_latent=init, return_latents=True)
    T = n_init + n_noise
    assert video.shape == (1, 1 + 4 * (T - 1), 3, 8 * LAT[0], 8 * LAT[1])
    u8 = _to_u8(video)
    captures = pipe.graph_captures
    for overlap in (True, False):
        for output in ("float", "uint8"):
            firsts, parts = _collect(pipe, noise, init, output, overlap)
            assert [int(p.shape[0]) for p in parts] == per_yield, (overlap, output)
            got = torch.cat(parts)
            if output == "float":
                assert got.is_cuda and got.dtype == torch.float32
                assert torch.equal(got, video[0]), (case, overlap, output, float((got - video[0]).abs().max()))
            else:
                assert not got.is_cuda and got.dtype == torch.uint8
                assert torch.equal(got, u8), (case, overlap, output)
            assert torch.equal(pipe._out[T].to(lat.dtype), lat), "the two paths' latents"
    assert pipe.graph_captures == captures, "inference_stream replays inference()'s block graphs"
    # and inference() itself is unchanged by the streamed calls in between
    torch.manual_seed(5)
    again = pipe.inference(noise, ["p"], initial_latent=init)
    assert torch.equal(again, video)
    pipe.release_graphs()


def test_second_stream_call_constructs_no_graph():
    from mmpl_amd.synthetic import philox_normal
    pipe = _pipe()
    noise = philox_normal([1, 9, 16, *LAT], 73).to(DEV)
    _, a = _collect(pipe, noise, None, "uint8", True)
    assert pipe.graph_captures == 3
    _, b = _collect(pipe, noise, None, "uint8", True)
    assert pipe.graph_captures == 3
    assert torch.equal(torch.cat(a), torch.cat(b))
    assert a[0].data_ptr() != a[2].data_ptr(), "yields are the consumer's own copies, not the staging buffers"
    pipe.release_graphs()
    assert not pipe._graphs


def test_early_close_then_inference():
    from mmpl_amd.synthetic import philox_normal
    noise = philox_normal([1, 21, 16, *LAT], 74).to(DEV)
    fresh = _pipe()
    torch.manual_seed(5)
    want = fresh.inference(noise, ["p"])
    pipe = _pipe()
    torch.manual_seed(9)
    it = pipe.inference_stream(noise, ["p"], output="uint8", overlap=True)
    first0, f0 = next(it)
    first1, f1 = next(it)
    assert (first0, first1) == (0, 9) and f0.shape[0] == 9 and f1.shape[0] == 12
    it.close()                                                       # drains the decode stream
    torch.manual_seed(5)
    got = pipe.inference(noise, ["p"])
    assert torch.equal(got, want)
    # and a streamed call after the aborted one starts a new decoded video
    _, parts = _collect(pipe, noise, None, "uint8", True)
    assert torch.equal(torch.cat(parts), _to_u8(want))


def test_fullsize_1p3b_480p_two_blocks_overlapped():
    """Wan 1.3B at 480p, all 30 layers, 2 blocks: block 1's denoise (long GEMM / attention kernels) runs while block 0 decodes."""
    pipe = _pipe("1.3B", lat=(60, 104))
    g = torch.Generator(device=DEV).manual_seed(91)
    noise = torch.randn(1, 6, 16, 60, 104, generator=g, device=DEV).bfloat16()
    torch.manual_seed(5)
    video = pipe.inference(noise, ["p"])
    assert video.shape == (1, 21, 3, 480, 832) and torch.isfinite(video).all()
    u8 = _to_u8(video)
    for overlap in (True, False):
        firsts, parts = _collect(pipe, noise, None, "uint8", overlap)
        assert firsts == [0, 9] and torch.equal(torch.cat(parts), u8), overlap
    firsts, parts = _collect(pipe, noise, None, "float", True)
    assert torch.equal(torch.cat(parts), video[0])


def test_cli_stream_writes_the_same_file(tmp_path):
    from mmpl_amd import cli
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n"
                   "model_kwargs:\n  timestep_shift: 5.0\n")
    base = ["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--num_output_frames", "9",
            "--config_path", str(cfg)]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    cli.main(base + ["--output_folder", str(tmp_path / "a")])
    cli.main(base + ["--output_folder", str(tmp_path / "b"), "--stream"])
    a, b = torch.load(tmp_path / "a" / "0-0.pt"), torch.load(tmp_path / "b" / "0-0.pt")
    assert tuple(a.shape) == (33, 128, 192, 3) and a.dtype == torch.uint8
    assert torch.equal(a, b)


def test_cli_stream_refused_on_50_step_config(capsys):
    from mmpl_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--synthetic", "--model", "tiny", "--latent_hw", "16", "24", "--duration", "1", "--stream"])
    assert "--stream" in capsys.readouterr().err
