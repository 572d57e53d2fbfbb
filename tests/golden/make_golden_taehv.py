"""TAEHV decoder fixture from the REAL reference (build container only): demo_utils/taehv.py's ``TAEHV.decode_video`` on seeded
weights (mmpl_amd.synthetic.taehv_state_dict), a 3-latent video at 8 x 12 latents, on the CPU.  Data only -- weights are regenerated
from the seed, never stored:

  taehv_tiny.pt       "exact": the reference in fp32 on bf16-rounded weights and a bf16-rounded input, [12, 3, 64, 96] float32;
                      "ref_bf16_rel_l2": the relative L2 distance of the reference's own all-bf16 output to it (the noise yardstick);
                      "prefix": for the first 1 and 2 latents, the frame count and max |d| to the same frames of the whole video;
                      "parallel_rel_l2": the reference's two evaluation orders against each other;
                      "mem_effect": per MemBlock, the relative change of the output when the `past` half of its first conv is zeroed;
                      "tgrow": a state dict whose first TGrow weight has 2 * 256 rows (seed of the extra rows, latent seed / shape,
                      output [4, 3, 32, 48] float32)
  taehv_tiny_bf16.pt  the all-bf16 output itself, bfloat16 (a file of its own: the two together would pass the 1 MiB a committed
                      file may have)
"""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402
from mmpl_amd.synthetic import philox_normal, taehv_state_dict  # noqa: E402

WEIGHT_SEED, Z_SEED, Z_SHAPE = 5, 43, [3, 16, 8, 12]
TG_SEED, TG_Z_SEED, TG_Z_SHAPE = 6, 44, [1, 16, 4, 6]
MEMBLOCKS = [3, 4, 5, 9, 10, 11, 15, 16, 17]


def load_taehv():
    try:
        import tqdm.auto  # noqa: F401
    except ImportError:                                                     # the progress bar is all the reference wants from it
        m, a = types.ModuleType("tqdm"), types.ModuleType("tqdm.auto")

        class _Bar:
            def __init__(self, it=None, **kw):
                self.it = it

            def __iter__(self):
                return iter(self.it)

            def update(self, n):
                pass

            def close(self):
                pass
        a.tqdm = _Bar
        m.auto = a
        sys.modules["tqdm"], sys.modules["tqdm.auto"] = m, a
    spec = importlib.util.spec_from_file_location("_ref_taehv", REF + "/demo_utils/taehv.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def build(taehv, sd, dtype=torch.float32, patch=False):
    m = taehv.TAEHV(checkpoint_path=None).eval()
    full = m.state_dict()
    full.update({k: v.clone() for k, v in sd.items()})                      # the encoder keeps its default init: unused
    if patch:
        full = m.patch_tgrow_layers(full)
    m.load_state_dict(full, strict=True)
    return m.to(dtype)


def gen_taehv():
    torch.set_grad_enabled(False)
    taehv = load_taehv()
    sd = taehv_state_dict(seed=WEIGHT_SEED)
    m = build(taehv, sd)
    n_dec = sum(p.numel() for p in m.decoder.parameters())
    assert n_dec == 9844611, n_dec
    assert sorted(sd) == sorted("decoder." + k for k in m.decoder.state_dict()), "synthetic keys != the reference decoder's"
    z = philox_normal(Z_SHAPE, Z_SEED)                                      # bf16
    exact = m.decode_video(z.float()[None])[0]                              # [12, 3, 64, 96]
    seq = m.decode_video(z.float()[None], parallel=False)[0]
    out = {"meta": dict(weight_seed=WEIGHT_SEED, z_seed=Z_SEED, z_shape=Z_SHAPE), "exact": exact.clone(),
           "parallel_rel_l2": rel_l2(seq, exact)}
    bf = build(taehv, sd, torch.bfloat16).decode_video(z[None])[0]
    out["ref_bf16_rel_l2"] = rel_l2(bf.float(), exact)
    inside = float(((exact > 0) & (exact < 1)).float().mean())
    beyond = float(((exact < -1) | (exact > 2)).float().mean())
    print(f"[taehv] output {tuple(exact.shape)} std {float(exact.std()):.3f}, {100 * inside:.1f} % inside (0, 1), {100 * beyond:.2f} % beyond "
          f"[-1, 2]; ref_bf16_rel_l2 = {out['ref_bf16_rel_l2']:.3e}; parallel vs sequential {out['parallel_rel_l2']:.2e}")
    assert inside >= 0.5 and beyond < 0.05, "the fixture's output does not sit where clamp / uint8 cannot hide an error"
    out["prefix"] = []
    for n in (1, 2):
        p = m.decode_video(z[:n].float()[None])[0]
        out["prefix"].append(dict(latents=n, frames=int(p.shape[0]), max_abs=float((p - exact[:p.shape[0]]).abs().max())))
        print(f"[taehv] first {n} of 3 latents -> {p.shape[0]} frames, max|d| to the whole video's = {out['prefix'][-1]['max_abs']:.2e}")
    out["mem_effect"] = []
    for i in MEMBLOCKS:
        cut = dict(sd)
        w = sd[f"decoder.{i}.conv.0.weight"].clone()
        w[:, w.shape[1] // 2:] = 0
        cut[f"decoder.{i}.conv.0.weight"] = w
        out["mem_effect"].append(rel_l2(build(taehv, cut).decode_video(z.float()[None])[0], exact))
    print("[taehv] relative change with one MemBlock's memory cut:", " ".join(f"{e:.3f}" for e in out["mem_effect"]))
    assert min(out["mem_effect"]) > 2 * out["ref_bf16_rel_l2"], "a MemBlock's memory does not matter"
    solo = torch.cat([m.decode_video(z[i:i + 1].float()[None])[0] for i in range(Z_SHAPE[0])])
    out["no_memory_rel_l2"] = rel_l2(solo, exact)
    print(f"[taehv] latents decoded one by one with empty memories: {out['no_memory_rel_l2']:.3f} from the video's decode")
    # patch_tgrow_layers: the first TGrow (decoder.7) with 2 * 256 rows -- the model keeps the last 256
    g = torch.Generator().manual_seed(TG_SEED)
    extra = (torch.randn(256, 256, 1, 1, generator=g) * (1.0 / 16)).to(torch.bfloat16)
    big = dict(sd)
    big["decoder.7.conv.weight"] = torch.cat([extra, sd["decoder.7.conv.weight"]], 0)
    zt = philox_normal(TG_Z_SHAPE, TG_Z_SEED)
    tg = build(taehv, big, patch=True).decode_video(zt.float()[None])[0]
    assert torch.equal(tg, m.decode_video(zt.float()[None])[0])              # the extra rows are dropped, the last 256 kept
    out["tgrow"] = dict(extra_seed=TG_SEED, z_seed=TG_Z_SEED, z_shape=TG_Z_SHAPE, out=tg.clone())
    torch.save(out, os.path.join(HERE, "taehv_tiny.pt"))
    torch.save({"ref_bf16": bf.clone()}, os.path.join(HERE, "taehv_tiny_bf16.pt"))
    for f in ("taehv_tiny.pt", "taehv_tiny_bf16.pt"):
        print(f"[taehv] {f}: {os.path.getsize(os.path.join(HERE, f))} bytes")


if __name__ == "__main__":
    gen_taehv()
