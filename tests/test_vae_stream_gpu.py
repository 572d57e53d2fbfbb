"""Streaming VAE decode on the MI355X (-m gpu): VaeEngine.decode_stream / clear_cache and WanVAEWrapper.decode_to_pixel(use_cache=True)
against the one-shot decode (bit for bit: the same kernels see the same inputs in the same order) and against the reference's
cached_decode fixture (tests/golden/make_golden_vae_stream.py; rel-L2 <= 3e-2, the VAE bound of tests/test_vae_gpu.py), and the
fused uint8 output against PyTorch's evaluation of the pipeline's and the CLI's conversion."""
import pytest
import torch

from tests.util import GOLDEN, max_abs, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508, 0.4134, -0.0715, 0.5517, -0.3632, -0.1922,
        -0.9497, 0.2503, -0.2921]
STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743, 3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253,
       2.8251, 1.9160]


def _engine(lat):
    from mmpl_amd.synthetic import vae_state_dict
    from mmpl_amd.vae import VaeEngine
    eng = VaeEngine(lat[0], lat[1], DEV)
    eng.load_state_dict(vae_state_dict(seed=3))
    return eng


def _stream(eng, z, split, out_format="float"):
    """clear_cache, then decode_stream over `split`; returns (concatenated frames, frames per call)."""
    eng.clear_cache()
    parts, f0 = [], 0
    for n in split:
        parts.append(eng.decode_stream(z[f0:f0 + n], MEAN, STD, out_format=out_format))
        f0 += n
    assert f0 == z.shape[0]
    return torch.cat(parts), [int(p.shape[0]) for p in parts]


def _fixture():
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(f"{GOLDEN}/vae_stream_tiny.pt")
    z = philox_normal(fx["meta"]["z_shape"], fx["meta"]["z_seed"])[0].permute(1, 0, 2, 3).contiguous()     # [7, 16, 8, 12]
    return fx, z


def test_splits_bit_identical_to_one_shot():
    fx, z = _fixture()
    eng = _engine((8, 12))
    one = eng.decode(z, MEAN, STD)
    assert one.shape == (25, 3, 64, 96)
    for split, counts in zip(fx["splits"], fx["counts"]):
        got, n = _stream(eng, z, split)
        assert n == counts, (split, n)
        assert torch.equal(got, one), (split, max_abs(got, one))
    assert torch.equal(eng.decode(z, MEAN, STD), one)                      # and the one-shot path is what it was


@pytest.mark.parametrize("split", [[1, 2], [1, 1, 1]])
def test_splits_bit_identical_ragged_geometry(split):
    from mmpl_amd.synthetic import philox_normal
    eng = _engine((6, 10))
    z = philox_normal([3, 16, 6, 10], 77)
    one = eng.decode(z, MEAN, STD)
    got, n = _stream(eng, z, split)
    assert n == [1 + 4 * (k - 1) if i == 0 else 4 * k for i, k in enumerate(split)]
    assert torch.equal(got, one), max_abs(got, one)


def test_stream_vs_reference_cached_decode():
    fx, z = _fixture()
    eng = _engine((8, 12))
    ref = fx["dec_out"][0].permute(1, 0, 2, 3).float().clamp(-1, 1)         # [25, 3, 64, 96], == the reference's cached_decode
    for split in fx["splits"]:
        got, _ = _stream(eng, z, split)
        e = rel_l2(got, ref)
        print(f"decode_stream {split}: rel_l2(HIP, reference cached_decode) = {e:.3e}, max|d| = {max_abs(got, ref):.3e}")
        assert torch.isfinite(got).all() and e < 3e-2
    # a call without clear_cache continues the video, as the reference's stale-cache call does
    assert eng.decode_stream(z[:1], MEAN, STD).shape[0] == fx["stale_count"] == 4


@pytest.mark.parametrize("lat, n_lat, split", [((8, 12), 4, [1, 3]), ((6, 10), 3, [2, 1])])
def test_uint8_output_equals_pytorch_conversion(lat, n_lat, split):
    """out_format=1 == the pipeline's (x * 0.5 + 0.5).clamp(0, 1) and the CLI's (v * 255.0).clamp(0, 255).to(uint8) on the float
    frames of the same decode, byte for byte; the latent is scaled up so that both clamps see saturated pixels."""
    from mmpl_amd.synthetic import philox_normal
    eng = _engine(lat)
    z = philox_normal([n_lat, 16, lat[0], lat[1]], 55) * 4.0
    f, _ = _stream(eng, z, split)
    u, n = _stream(eng, z, split, out_format="uint8")
    T = 1 + 4 * (n_lat - 1)
    assert u.dtype == torch.uint8 and u.shape == (T, 8 * lat[0], 8 * lat[1], 3) and sum(n) == T
    exp = (((f.clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1)) * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    diff = (u.int() - exp.int()).abs()
    print(f"uint8 {lat}: max byte difference {int(diff.max())}, differing {int((diff > 0).sum())} of {diff.numel()}; "
          f"zeros {int((u == 0).sum())}, 255s {int((u == 255).sum())}")
    assert (u == 0).any() and (u == 255).any(), "the input must saturate both clamps"
    assert torch.equal(u, exp)


def test_stream_is_isolated_from_one_shot_calls():
    from mmpl_amd.synthetic import philox_normal
    fx, z = _fixture()
    eng = _engine((8, 12))
    one = eng.decode(z, MEAN, STD)
    eng.clear_cache()
    a = eng.decode_stream(z[:2], MEAN, STD)
    other = eng.decode(philox_normal([2, 16, 8, 12], 5), MEAN, STD)         # a one-shot decode and an encode in between
    lat = eng.encode(philox_normal([3, 5, 64, 96], 6).clamp(-1, 1), MEAN, STD)
    assert other.shape[0] == 5 and lat.shape[0] == 2
    b = eng.decode_stream(z[2:], MEAN, STD)
    assert a.shape[0] == 5 and b.shape[0] == 20
    assert torch.equal(torch.cat([a, b]), one)
    # clear_cache mid-video: the next call decodes a first frame again
    eng.decode_stream(z[:2], MEAN, STD)
    eng.clear_cache()
    c = eng.decode_stream(z[:3], MEAN, STD)
    assert c.shape[0] == 9 and torch.equal(c, one[:9])


def test_wrong_workspace_is_an_error():
    import ctypes as C
    from mmpl_amd import _lib
    fx, z = _fixture()
    eng = _engine((8, 12))
    eng.clear_cache()
    eng.decode_stream(z[:1], MEAN, STD)
    lib, ws = eng._lib, eng._stream_ws
    zz = z[1:2].to(DEV, torch.bfloat16).contiguous()
    out = torch.empty(4, 3, 64, 96, dtype=torch.float32, device=DEV)
    m, inv = eng._scales(MEAN, STD)
    n = C.c_int(0)
    other = torch.empty_like(ws)
    args = (eng._stream, _lib.ptr(zz), 1, m, inv, _lib.ptr(out), 0, C.byref(n))
    with pytest.raises(RuntimeError, match="workspace differs"):
        _lib.check(lib.mmpl_vae_stream_decode(*args, _lib.ptr(other), other.numel(), _lib.stream_ptr()), "mmpl_vae_stream_decode")
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.check(lib.mmpl_vae_stream_decode(*args, _lib.ptr(ws), ws.numel() - 1, _lib.stream_ptr()), "mmpl_vae_stream_decode")
    # the refused calls changed nothing: the video continues in its own workspace
    _lib.check(lib.mmpl_vae_stream_decode(*args, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "mmpl_vae_stream_decode")
    torch.cuda.synchronize()
    assert n.value == 4 and torch.equal(out, eng.decode(z[:2], MEAN, STD)[1:5])


def test_wrapper_use_cache_continues_the_video():
    """WanVAEWrapper.decode_to_pixel(use_cache=True) (utils/wan_wrapper.py:90-113): 1 latent then 3 more -> 1 then 12 frames, the
    one-shot frames 0 and 1..12.  (Ignoring use_cache gave 9 frames decoded from an empty cache.)"""
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import vae_state_dict
    from mmpl_amd.wan_wrapper import WanVAEWrapper
    fx, z = _fixture()
    vae = WanVAEWrapper(geometry=Geometry(8, 12), device=DEV, state_dict=vae_state_dict(seed=3))
    zb = z.unsqueeze(0).to(DEV)                                               # [1, 7, 16, 8, 12]
    one = vae.decode_to_pixel(zb[:, :4], use_cache=False)
    assert one.shape == (1, 13, 3, 64, 96) and one.dtype == torch.float32
    vae.model.clear_cache()
    a = vae.decode_to_pixel(zb[:, :1], use_cache=True)
    b = vae.decode_to_pixel(zb[:, 1:4], use_cache=True)
    assert a.shape == (1, 1, 3, 64, 96) and b.shape == (1, 12, 3, 64, 96) and b.dtype == torch.float32
    assert torch.equal(a, one[:, :1]) and torch.equal(b, one[:, 1:13])
    assert float(b.min()) >= -1.0 and float(b.max()) <= 1.0
    # use_cache=False returns what it always did and leaves the cache cleared: the next cached call is a first frame
    again = vae.decode_to_pixel(zb[:, :4], use_cache=False)
    assert torch.equal(again, one)
    c = vae.decode_to_pixel(zb[:, :2], use_cache=True)
    assert c.shape[1] == 5 and torch.equal(c, one[:, :5])
    # encode_to_latent ends the cached video too (vae.py:542)
    vae.encode_to_latent(torch.zeros(1, 3, 1, 64, 96, device=DEV))
    d = vae.decode_to_pixel(zb[:, :1], use_cache=True)
    assert d.shape[1] == 1 and torch.equal(d, one[:, :1])
    with pytest.raises(AssertionError, match="Batch size"):
        vae.decode_to_pixel(torch.cat([zb[:, :1], zb[:, :1]]), use_cache=True)
