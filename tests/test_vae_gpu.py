"""HIP Wan 3D-VAE decode / encode vs the oracle and the reference's golden outputs (-m gpu).
Stated tolerance: rel-L2 <= 3e-2 against the reference's bf16 CPU run (the VAE is ~60 bf16 convs deep; the measured
value is printed).  That bound is a whole-network one; what a single launch computes -- every conv kernel bit for bit against
float64 in the exact integer regime, halo / ring-slot / border handling, the norm, resampling and softmax passes -- is checked
per launch in tests/test_vae_kernels_gpu.py (and tests/test_taehv_kernels_gpu.py for the preview decoder)."""
import pytest
import torch

from tests.util import GOLDEN, max_abs, rel_l2

pytestmark = pytest.mark.gpu
MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508, 0.4134, -0.0715, 0.5517, -0.3632, -0.1922,
        -0.9497, 0.2503, -0.2921]
STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743, 3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253,
       2.8251, 1.9160]


def _engine(lat):
    from mmpl_amd.synthetic import vae_state_dict
    from mmpl_amd.vae import VaeEngine
    sd = vae_state_dict(seed=3)
    eng = VaeEngine(lat[0], lat[1], "cuda:0")
    eng.load_state_dict(sd)
    return eng, sd


def test_decode_vs_reference_golden():
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(f"{GOLDEN}/vae_tiny.pt")
    eng, sd = _engine((8, 12))
    z = philox_normal(fx["meta"]["z_shape"], fx["meta"]["z_seed"])          # [1,16,4,8,12]
    out = eng.decode(z[0].permute(1, 0, 2, 3), MEAN, STD)                     # [13,3,64,96]
    torch.cuda.synchronize()
    ref = fx["dec_out"][0].permute(1, 0, 2, 3).float().clamp(-1, 1)
    e = rel_l2(out, ref)
    print(f"decode: rel_l2(HIP, reference golden) = {e:.3e}, max|d| = {max_abs(out, ref):.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert e < 3e-2
    # causal prefix property: decoding only the first two latents gives the first five frames
    out2 = eng.decode(z[0].permute(1, 0, 2, 3)[:2], MEAN, STD)
    assert torch.equal(out2, out[:5])


def test_encode_vs_reference_golden():
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(f"{GOLDEN}/vae_tiny.pt")
    eng, sd = _engine((8, 12))
    x = philox_normal(fx["meta"]["x_shape"], fx["meta"]["x_seed"]).clamp(-1, 1)     # [1,3,9,64,96]
    lat = eng.encode(x[0], MEAN, STD)                                                # [3,16,8,12]
    torch.cuda.synchronize()
    ref = fx["enc_out"][0].permute(1, 0, 2, 3).float()
    e = rel_l2(lat, ref)
    print(f"encode: rel_l2(HIP, reference golden) = {e:.3e}, max|d| = {max_abs(lat, ref):.3e}")
    assert e < 3e-2
    lat2 = eng.encode(x[0][:, :5], MEAN, STD)
    assert torch.equal(lat2, lat[:2])


def test_decode_vs_oracle_other_geometry():
    from mmpl_amd.synthetic import philox_normal
    from oracle import vae_ref
    eng, sd = _engine((6, 10))
    z = philox_normal([3, 16, 6, 10], 77)
    out = eng.decode(z, MEAN, STD)
    torch.cuda.synchronize()
    ref = vae_ref.decode_to_pixel(sd, z.unsqueeze(0), MEAN, STD)[0]
    e = rel_l2(out, ref)
    print(f"decode 6x10: rel_l2 = {e:.3e}")
    assert e < 3e-2


def test_decode_real_handoff_artefact_vs_oracle():
    """Realistic latent statistics: a spatial crop of the reference tree's real left-over hand-off tensor
    (MMPL_i2v/latents_chunk4.pt: frame 0 + the last two anchors, mean -0.13 / std 0.96; tests/golden/make_golden_vae.py)
    decoded by the HIP VAE and by the oracle."""
    from oracle import vae_ref
    art = torch.load(f"{GOLDEN}/handoff_artefact_crop.pt")          # bf16 [1, 3, 16, 16, 24]
    assert art.shape == (1, 3, 16, 16, 24) and art.dtype == torch.bfloat16
    eng, sd = _engine((16, 24))
    out = eng.decode(art[0], MEAN, STD)                               # [9, 3, 128, 192]
    torch.cuda.synchronize()
    ref = vae_ref.decode_to_pixel(sd, art, MEAN, STD)[0]
    e = rel_l2(out, ref)
    print(f"decode of the real hand-off artefact crop: rel_l2(HIP, oracle) = {e:.3e}")
    assert out.shape == (9, 3, 128, 192) and e < 3e-2


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_vae_gpu import _engine, MEAN, STD
from mmpl_amd.synthetic import philox_normal
eng, sd = _engine((6, 10))
z = philox_normal([3, 16, 6, 10], 77)
px = philox_normal([3, 9, 48, 80], 78).clamp(-1, 1)
torch.save({{"dec": eng.decode(z, MEAN, STD).cpu(), "enc": eng.encode(px, MEAN, STD).cpu()}}, sys.argv[1])
"""


def test_norm_fused_into_conv_epilogue_vs_separate_pass(tmp_path):
    """The RMS_norm + SiLU in front of every 96-channel conv runs in the PRODUCING conv's epilogue (conv_halo_kernel, ConvArgs.ngamma;
    vae.py:51-54, 186-220).  Same arithmetic and rounding points as the separate pass (MMPL_VAE_NO_FUSE_NORM=1, run in a child
    process because the switch is read once); only the order of the fp32 sum of squares differs, which moves a pixel's bf16 norm
    by one ulp now and then.  In the decoder those layers are the LAST stage (measured distance between the two builds 1.9e-4); in
    the encoder they are the FIRST, and the bf16 network behind them amplifies any perturbation to its own rounding-noise level
    (3.3e-3; the reference's bf16-vs-fp32 distance for an encode is 7.7e-3) -- so the statement that matters is the second one:
    both builds are equally close to the oracle.  Geometry 48 x 80: ragged 8 x 32 patches."""
    import os
    import subprocess
    import sys
    from mmpl_amd.synthetic import philox_normal
    from oracle import vae_ref
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = tmp_path / "unfused.pt"
    env = dict(os.environ, MMPL_VAE_NO_FUSE_NORM="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=root), str(f)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    ref = torch.load(f)
    eng, sd = _engine((6, 10))
    z = philox_normal([3, 16, 6, 10], 77)
    px = philox_normal([3, 9, 48, 80], 78).clamp(-1, 1)
    dec = eng.decode(z, MEAN, STD).cpu()
    enc = eng.encode(px, MEAN, STD).cpu()
    ed, ee = rel_l2(dec, ref["dec"]), rel_l2(enc, ref["enc"])
    o_dec = vae_ref.decode_to_pixel(sd, z.unsqueeze(0), MEAN, STD)[0]
    o_enc = vae_ref.encode_to_latent(sd, px.unsqueeze(0).to(torch.bfloat16), MEAN, STD)[0]
    fd, ud = rel_l2(dec, o_dec), rel_l2(ref["dec"], o_dec)
    fe, ue = rel_l2(enc, o_enc), rel_l2(ref["enc"], o_enc)
    print(f"fused vs separate norm pass: decode rel_l2 = {ed:.3e}, encode rel_l2 = {ee:.3e}; vs the oracle: decode fused {fd:.3e} / separate "
          f"{ud:.3e}, encode fused {fe:.3e} / separate {ue:.3e}")
    assert ed < 1e-3 and ee < 6e-3
    assert fd < 1.1 * ud + 5e-4 and fe < 1.1 * ue + 5e-4
