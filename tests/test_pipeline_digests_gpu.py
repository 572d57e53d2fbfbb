"""The four pipelines, pinned by the bytes of the latents they produce (-m gpu).

The Python layer above the engines (mmpl_amd/wan_wrapper.py, mmpl_amd/dit.py, mmpl_amd/pipeline/) decides which launches run, in
which order, on which buffers and from which RNG draws; a change there that is meant to leave all of that alone is held to the
sha256 of each case's latents (and of the hand-off tensor where the pipeline has one), recorded on an MI355X before that change
(tests/golden/pipeline_digests.json).  The tiny synthetic config at 16 x 24 latents, the set-ups of the existing pipeline tests,
``torch.manual_seed(0)`` before anything is built and ``renoise_override`` wherever a pipeline draws; every case ran twice in
separate processes when it was recorded and gave the same digests both times.  A kernel change that moves bits on purpose records
the file again.
"""
import hashlib
import json
import os

import pytest
import torch

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
LAT = (16, 24)
DEV = "cuda:0"


def _fps_inputs(seed=23):
    from mmpl_amd.synthetic import philox_normal
    noise = philox_normal([1, 21, 16, *LAT], seed).cuda()
    renoise = {f: philox_normal([1, 16, *LAT], 100 + f).cuda() for f in (4, 9, 13, 18)}
    return noise, renoise


def _fps_chunk(pipe, noise, **kw):
    got = {}
    pipe.handoff_sink = lambda t: got.__setitem__("h", t.clone())
    _, lat = pipe.inference(noise, ["a cat"], return_latents=True, decode=False, **kw)
    return {"latents": lat, "handoff": got["h"]}


def _fps_t2v(chunk2=False, solver=None, **attrs):
    """Chunk 1 of the 50-step pipeline at 2 steps; `chunk2`: then chunk 2 (initial_latent) on the same pipeline."""
    from mmpl_amd.synthetic import philox_normal
    from tests.test_pipeline_gpu import _setup
    pipe, *_ = _setup("t2v")
    noise, pipe.renoise_override = _fps_inputs()
    if solver is not None:
        pipe.sample_solver = solver
    for k, v in attrs.items():
        setattr(pipe, k, v)
    out = _fps_chunk(pipe, noise)
    if chunk2:
        out = _fps_chunk(pipe, noise, initial_latent=philox_normal([1, 2, 16, *LAT], 55).cuda())
    return out


def _fps_i2v_mode():
    from mmpl_amd.synthetic import philox_normal
    from tests.test_pipeline_gpu import _setup
    pipe, *_ = _setup("i2v")
    return _fps_chunk(pipe, _fps_inputs(24)[0], initial_latent=philox_normal([1, 1, 16, *LAT], 56).cuda())


def _fps_i2v_model():
    """The Wan-I2V model type under the 50-step pipeline: clip_fea and y from the HIP CLIP tower and VAE."""
    from mmpl_amd.i2v_condition import build_image_condition
    from mmpl_amd.synthetic import philox_normal
    from tests.test_i2v_pipeline_gpu import _setup
    pipe, clip, *_ = _setup()
    img = philox_normal([3, LAT[0] * 8, LAT[1] * 8], 71).clamp(-1, 1).cuda()
    cond = build_image_condition(pipe.vae, clip, img)
    image_latent = pipe.vae.encode_to_latent(img[None, :, None]).to(torch.bfloat16)
    return _fps_chunk(pipe, _fps_inputs(24)[0], initial_latent=image_latent, image_condition=cond)


def _draws(n, frames=3, base=80):
    from mmpl_amd.synthetic import philox_normal
    return [philox_normal([frames, 16, *LAT], base + k).to(DEV) for k in range(n)]


def _fewstep(stream=False, init_frames=0):
    """9 latent frames in blocks of 3 (4 steps each, 3 re-noise draws per block); `stream`: through inference_stream, the latents
    then read from the static output latent; `init_frames`: that many of the 9 come in as initial_latent."""
    from mmpl_amd.synthetic import philox_normal
    from tests.test_fewstep_stream_gpu import _pipe
    pipe = _pipe()
    n_noise = 9 - init_frames
    pipe.renoise_override = _draws(n_noise)
    noise = philox_normal([1, n_noise, 16, *LAT], 71).to(DEV)
    init = philox_normal([1, init_frames, 16, *LAT], 72).to(DEV) if init_frames else None
    if stream:
        for _ in pipe.inference_stream(noise, ["p"], initial_latent=init, output="float", decoder="vae"):
            pass
        return {"latents": pipe._out[9]}
    return {"latents": pipe.inference(noise, ["p"], initial_latent=init, return_latents=True)[1]}


def _fewstep_rolling():
    """Window 6, sink 0, 18 frames: the blocks from frame 6 on replay position-free graphs."""
    from tests.test_fewstep_rolling_gpu import _noise, _pipe
    pipe, *_ = _pipe(6, 0)
    pipe.renoise_override = _draws(18)
    lat = pipe.inference(_noise(18), ["p"], return_latents=True)[1]
    assert any(k[0] == "rolling" for k in pipe._graphs)
    return {"latents": lat}


def _bidir_fewstep():
    from tests.test_bidir_pipeline_gpu import _fewstep as setup
    _, pipe, noise, draws = setup()
    pipe.renoise_override = draws
    return {"latents": pipe.inference(noise, ["p"], return_latents=True)[1]}


def _bidir_diffusion(tag):
    from tests.test_bidir_pipeline_gpu import _diffusion
    _, pipe, noise = _diffusion(tag)
    return {"latents": pipe.inference(noise, ["p"], return_latents=True)[1]}


def _bidir_i2v():
    """Two images on one pipeline: the second call replays the first call's step graph."""
    from tests.test_bidir_i2v_pipeline_gpu import _diffusion, _image
    _, pipe, noise, cond = _diffusion("unipc")
    first = pipe.inference(noise, ["p"], return_latents=True, image_condition=cond)[1]
    second = pipe.inference(noise, ["q"], return_latents=True, image_condition=_image(301, 302))[1]
    assert pipe.graph_captures == 1
    return {"first_image": first, "second_image": second}


CASES = {
    "fps_t2v_chunk1": _fps_t2v,
    "fps_t2v_chunk2_initial_latent": lambda: _fps_t2v(chunk2=True),
    "fps_t2v_dpmpp": lambda: _fps_t2v(solver="dpm++"),
    "fps_t2v_concurrent_cfg": lambda: _fps_t2v(concurrent_cfg=True),
    "fps_t2v_no_share_block0": lambda: _fps_t2v(share_block0=False),
    "fps_t2v_no_graphs": lambda: _fps_t2v(use_graphs=False),
    "fps_i2v_mode": _fps_i2v_mode,
    "fps_i2v_model_type": _fps_i2v_model,
    "fewstep": _fewstep,
    "fewstep_stream": lambda: _fewstep(stream=True),
    "fewstep_rolling": _fewstep_rolling,
    "fewstep_initial_latent": lambda: _fewstep(init_frames=3),
    "bidir_fewstep": _bidir_fewstep,
    "bidir_diffusion_unipc": lambda: _bidir_diffusion("unipc"),
    "bidir_diffusion_dpmpp": lambda: _bidir_diffusion("dpmpp"),
    "bidir_diffusion_i2v_two_images": _bidir_i2v,
}
SAME_AS_CHUNK1 = ("fps_t2v_concurrent_cfg", "fps_t2v_no_share_block0", "fps_t2v_no_graphs")   # what the existing tests promise in-process


def digest(name):
    """{what: "dtype[shape]:sha256"} of the case's tensors."""
    torch.manual_seed(0)                # CausalFPSInferencePipeline.__init__ draws ddpm_index from the device generator
    outs = CASES[name]()
    torch.cuda.synchronize()
    res = {}
    for what, out in outs.items():
        raw = out.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        res[what] = f"{out.dtype}{list(out.shape)}:{hashlib.sha256(raw).hexdigest()}"
    return res


def _recorded():
    return json.load(open(os.path.join(GOLDEN, "pipeline_digests.json")))


@pytest.mark.parametrize("name", sorted(CASES))
def test_pipeline_digest(name):
    want = _recorded()
    got = digest(name)
    print(f"[digest] {name}: {got}")
    assert got == want[name]


def test_recorded_launch_modes_equal_chunk1():
    want = _recorded()
    for name in SAME_AS_CHUNK1:
        assert want[name] == want["fps_t2v_chunk1"], name
    assert want["fewstep_stream"] == want["fewstep"]
