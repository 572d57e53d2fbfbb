"""Streaming-decode fixture from the REAL reference (build container only): WanVAE_.cached_decode over several splits of
one 7-latent video against WanVAE_.decode of the whole, tiny-spatial, bf16 on the CPU.  The fixture holds data only: the
one-shot frames, and per split the per-call frame counts and whether the concatenated calls equal the one-shot frames."""
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ref_import import load_reference  # noqa: E402
from make_golden_vae import MEAN, STD  # noqa: E402
from mmpl_amd.synthetic import philox_normal, vae_state_dict  # noqa: E402

SPLITS = [[1, 3, 3], [3, 3, 1], [1] * 7, [2, 5]]


def gen_vae_stream():
    torch.set_grad_enabled(False)
    vae = load_reference()[3]
    m = vae.WanVAE_(dim=96, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=2, attn_scales=[], temperal_downsample=[False, True, True],
                    dropout=0.0).eval()
    m.load_state_dict(vae_state_dict(seed=3), strict=True)
    m = m.to(torch.bfloat16)
    scale = [torch.tensor(MEAN, dtype=torch.bfloat16), 1.0 / torch.tensor(STD, dtype=torch.bfloat16)]
    z = philox_normal([1, 16, 7, 8, 12], 41)
    t0 = time.time()
    px = m.decode(z, scale)                                                   # [1, 3, 25, 64, 96]
    print(f"[vae stream] one-shot decode {time.time() - t0:.1f}s -> {tuple(px.shape)}")
    out = {"dec_out": px.clone(), "splits": SPLITS, "counts": [], "equal": [], "max_abs": []}
    for split in SPLITS:
        m.clear_cache()
        parts, f0 = [], 0
        for n in split:
            parts.append(m.cached_decode(z[:, :, f0:f0 + n], scale))
            f0 += n
        cat = torch.cat(parts, 2)
        out["counts"].append([int(p.shape[2]) for p in parts])
        out["equal"].append(bool(torch.equal(cat, px)))
        out["max_abs"].append(float((cat.float() - px.float()).abs().max()))
        print(f"[vae stream] split {split}: frames per call {out['counts'][-1]}, equal to one-shot: {out['equal'][-1]}, "
              f"max|d| = {out['max_abs'][-1]}")
    # a call WITHOUT clear_cache continues the last video: its one latent is no first frame
    out["stale_count"] = int(m.cached_decode(z[:, :, :1], scale).shape[2])
    print(f"[vae stream] 1 latent on a stale cache -> {out['stale_count']} frames")
    m.clear_cache()
    out["meta"] = dict(weight_seed=3, z_seed=41, z_shape=[1, 16, 7, 8, 12])
    torch.save(out, os.path.join(HERE, "vae_stream_tiny.pt"))


if __name__ == "__main__":
    gen_vae_stream()
