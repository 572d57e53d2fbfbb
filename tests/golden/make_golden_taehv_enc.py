"""TAEHV encoder fixture from the REAL reference (build container only): demo_utils/taehv.py's ``TAEHV.encode_video`` on seeded
weights (mmpl_amd.synthetic.taehv_encoder_state_dict), 12 frames of 32 x 48 pixels, on the CPU.  Data only -- weights and input are
regenerated from the seeds, never stored:

  taehv_enc_tiny.pt   "exact": the reference in fp32 on bf16-rounded weights and a bf16-rounded input, [3, 16, 4, 6] float32;
                      "ref_bf16_rel_l2": the relative L2 distance of the reference's own all-bf16 output to it (the noise yardstick);
                      "parallel_rel_l2": the reference's two evaluation orders against each other;
                      "prefix": for the first 4 and 8 frames, the latent count and max |d| to the same latents of the whole video;
                      "mem_effect": per MemBlock, the relative change of the output when the `past` half of its first conv is zeroed;
                      "tpool_swap": the relative change when the two frame halves of the first TPool's weight are swapped;
                      "no_memory_rel_l2": every 4-frame group encoded with empty memories, against the video's encode
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden_taehv import load_taehv, rel_l2  # noqa: E402
from mmpl_amd.synthetic import philox_normal, taehv_encoder_state_dict  # noqa: E402

WEIGHT_SEED, PX_SEED, PX_SHAPE = 7, 45, [12, 3, 32, 48]
MEMBLOCKS = [4, 5, 6, 9, 10, 11, 14, 15, 16]


def pixels():
    """the fixture's input: sigmoid of seeded normals, rounded to bf16 (values in (0, 1))"""
    return torch.sigmoid(philox_normal(PX_SHAPE, PX_SEED).float()).to(torch.bfloat16)


def build(taehv, sd, dtype=torch.float32):
    m = taehv.TAEHV(checkpoint_path=None).eval()
    full = m.state_dict()
    full.update({k: v.clone() for k, v in sd.items()})                      # the decoder keeps its default init: unused
    m.load_state_dict(full, strict=True)
    return m.to(dtype)


def gen_taehv_enc():
    torch.set_grad_enabled(False)
    taehv = load_taehv()
    sd = taehv_encoder_state_dict(seed=WEIGHT_SEED)
    m = build(taehv, sd)
    n_enc = sum(p.numel() for p in m.encoder.parameters())
    assert n_enc == 1470928, n_enc
    assert list(sd) == ["encoder." + k for k in m.encoder.state_dict()], "synthetic keys != the reference encoder's"
    px = pixels()
    enc = lambda mod, x, **kw: mod.encode_video(x[None], show_progress_bar=False, **kw)[0]      # noqa: E731
    exact = enc(m, px.float())                                              # [3, 16, 4, 6]
    assert list(exact.shape) == [3, 16, 4, 6], exact.shape
    out = {"meta": dict(weight_seed=WEIGHT_SEED, px_seed=PX_SEED, px_shape=PX_SHAPE), "exact": exact.clone(),
           "parallel_rel_l2": rel_l2(enc(m, px.float(), parallel=False), exact)}
    bf = enc(build(taehv, sd, torch.bfloat16), px)
    out["ref_bf16_rel_l2"] = rel_l2(bf.float(), exact)
    print(f"[taehv enc] latent {tuple(exact.shape)} std {float(exact.std()):.3f} |max| {float(exact.abs().max()):.2f}; "
          f"ref_bf16_rel_l2 = {out['ref_bf16_rel_l2']:.3e}; parallel vs sequential {out['parallel_rel_l2']:.2e}")
    out["prefix"] = []
    for n in (4, 8):
        p = enc(m, px[:n].float())
        out["prefix"].append(dict(frames=n, latents=int(p.shape[0]), max_abs=float((p - exact[:p.shape[0]]).abs().max())))
        print(f"[taehv enc] first {n} of 12 frames -> {p.shape[0]} latents, max|d| to the whole video's = {out['prefix'][-1]['max_abs']:.2e}")
    out["mem_effect"] = []
    for i in MEMBLOCKS:
        cut = dict(sd)
        w = sd[f"encoder.{i}.conv.0.weight"].clone()
        w[:, w.shape[1] // 2:] = 0
        cut[f"encoder.{i}.conv.0.weight"] = w
        out["mem_effect"].append(rel_l2(enc(build(taehv, cut), px.float()), exact))
    print("[taehv enc] relative change with one MemBlock's memory cut:", " ".join(f"{e:.3f}" for e in out["mem_effect"]))
    assert min(out["mem_effect"]) > 2 * out["ref_bf16_rel_l2"], "a MemBlock's memory does not matter"
    swap = dict(sd)
    w = sd["encoder.2.conv.weight"]
    swap["encoder.2.conv.weight"] = torch.cat([w[:, 64:], w[:, :64]], 1)
    out["tpool_swap"] = rel_l2(enc(build(taehv, swap), px.float()), exact)
    print(f"[taehv enc] the first TPool's frame halves swapped: {out['tpool_swap']:.3f}")
    assert out["tpool_swap"] > 2 * out["ref_bf16_rel_l2"], "TPool's frame order does not matter"
    solo = torch.cat([enc(m, px[i:i + 4].float()) for i in range(0, PX_SHAPE[0], 4)])
    out["no_memory_rel_l2"] = rel_l2(solo, exact)
    print(f"[taehv enc] 4-frame groups encoded one by one with empty memories: {out['no_memory_rel_l2']:.3f} from the video's encode")
    path = os.path.join(HERE, "taehv_enc_tiny.pt")
    torch.save(out, path)
    print(f"[taehv enc] taehv_enc_tiny.pt: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    gen_taehv_enc()
