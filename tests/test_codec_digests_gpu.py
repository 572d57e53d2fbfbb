"""The VAE and TAEHV compositions, pinned by the bytes they produce (-m gpu).

No launch chain restates these two host orchestrations (the kernels under them are tested one launch at a time in
tests/test_vae_kernels_gpu.py, tests/test_taehv_kernels_gpu.py and tests/test_taehv_enc_kernels_gpu.py), so a change to the host code
that is meant to leave the launches alone is held to the sha256 of each output, recorded on an MI355X before that change
(tests/golden/codec_digests.json).  Synthetic weights of seed 0, philox inputs; every case ran twice in separate processes when it
was recorded and gave the same digest both times.  A kernel change that moves bits on purpose records the file again.
"""
import hashlib
import json
import os

import pytest
import torch

from tests.test_vae_gpu import MEAN, STD
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

TAEHV_LAT = (3, 5)      # 24 x 40 pixels: ragged against the 8 x 32 patch
VAE_LAT = (6, 10)       # the smallest geometry of tests/test_vae_gpu.py


def _taehv_decode(out_format):
    """4 latent frames = one full group of 3 and a group of 1: the MemBlock memories carry across groups."""
    from mmpl_amd.synthetic import philox_normal, taehv_state_dict
    from mmpl_amd.taehv import TaehvEngine
    eng = TaehvEngine(*TAEHV_LAT, "cuda:0")
    eng.load_state_dict(taehv_state_dict(seed=0))
    return eng.decode(philox_normal([4, 16, *TAEHV_LAT], 101), out_format=out_format)


def _taehv_encode(u8):
    """16 pixel frames = 4 latent frames, again a group of 3 and a group of 1."""
    from mmpl_amd.synthetic import philox_normal, taehv_encoder_state_dict
    from mmpl_amd.taehv import TaehvEncoderEngine
    eng = TaehvEncoderEngine(*TAEHV_LAT, "cuda:0")
    eng.load_state_dict(taehv_encoder_state_dict(seed=0))
    px = (philox_normal([16, 3, 8 * TAEHV_LAT[0], 8 * TAEHV_LAT[1]], 102).float() * 0.25 + 0.5).clamp(0, 1)
    if u8:
        px = (px * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return eng.encode(px)


def _vae(what):
    from mmpl_amd.synthetic import philox_normal, vae_state_dict
    from mmpl_amd.vae import VaeEngine
    eng = VaeEngine(*VAE_LAT, "cuda:0")
    eng.load_state_dict(vae_state_dict(seed=0))
    if what == "encode":                                    # 1 + 4 pixel frames: the first-chunk branch and the later-chunk one
        return eng.encode(philox_normal([3, 5, 8 * VAE_LAT[0], 8 * VAE_LAT[1]], 104).clamp(-1, 1), MEAN, STD)
    z = philox_normal([2, 16, *VAE_LAT], 103)               # 2 latent frames: the first-frame layout branch and the later-frame one
    if what == "decode":
        return eng.decode(z, MEAN, STD)
    eng.clear_cache()
    return eng.decode_stream(z, MEAN, STD)


CASES = {
    "taehv_decode_float": lambda: _taehv_decode("float"),
    "taehv_decode_uint8": lambda: _taehv_decode("uint8"),
    "taehv_encode_float": lambda: _taehv_encode(False),
    "taehv_encode_uint8": lambda: _taehv_encode(True),
    "vae_decode": lambda: _vae("decode"),
    "vae_stream_decode": lambda: _vae("stream"),
    "vae_encode": lambda: _vae("encode"),
}


def digest(name):
    out = CASES[name]()
    torch.cuda.synchronize()
    raw = out.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return f"{out.dtype}{list(out.shape)}:{hashlib.sha256(raw).hexdigest()}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_digest(name):
    want = json.load(open(os.path.join(GOLDEN, "codec_digests.json")))
    assert digest(name) == want[name]
