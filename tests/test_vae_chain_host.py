"""The chain of tests/vae_chain.py IS the model (CPU, no GPU): VaeRefOps(float64, round=False) against the oracle (oracle/vae_ref.py
decode / encode) on float64 copies of the weights and the same inputs.  Latents 6 x 10: three latent frames for the decoder (the
video's first frame -- 'Rep' -- and two later ones through the upsamplers' time_conv), nine pixel frames for the encoder (the first
chunk, which only fills the time_conv caches, and two chunks of four).  Weights: mmpl_amd.synthetic.vae_state_dict(seed 3).

The bound.  NOISE = rel_l2(VaeRefOps(float32), VaeRefOps(float64)) of the same quantity is the float32 noise of this computation,
measured in the test itself; the oracle, which sums in another order, is allowed MULT = 8 times that.
Measured (x86-64, torch CPU): NOISE decode 2.3e-6, encode 6.7e-7; rel_l2(chain float64, oracle float64) decode 5.1e-8, encode
2.8e-9, i.e. 0.022 x and 0.0041 x NOISE.  Both sides are float64; what is left is the attention scale, which the chain states as
the float32 quotient 1 / sqrtf(C) the launch is given (relative 3e-8 off 1 / sqrt(384)) while the oracle's sdpa computes it in float64.
The chain's stream over the splits [1, 2], [2, 1], [1, 1, 1] equals its one-shot decode exactly.
Every mutant of the chain (MUTANTS) misses the oracle by far more than the bound 8 x NOISE (1.8e-5 decode, 5.4e-6 encode): by
1.1e4 x (gamma of the first norm used for the second; the head's gamma taken from the last block) to 1.1e5 x the bound (ZeroPad2d
on the wrong side); none stays below it.  The multiples are printed and listed in DESIGN.md 4.4.
"""
import functools

import pytest
import torch

from mmpl_amd.synthetic import philox_normal, vae_state_dict
from mmpl_amd.vae import VaeEngine
from oracle import vae_ref
from tests import vae_chain as VC

MULT = 8.0
LAT = (6, 10)
F64, F32 = torch.float64, torch.float32
MEAN, STD = VC.MEAN, VC.STD


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _inputs():
    sd = vae_state_dict(seed=3)
    z = philox_normal([3, 16, LAT[0], LAT[1]], 77)
    px = philox_normal([3, 9, 8 * LAT[0], 8 * LAT[1]], 78).clamp(-1, 1)
    mean, inv = VC.latent_scales(MEAN, STD)
    return sd, z, px, mean, inv


def _chain(dtype, wiring=None):
    sd = _inputs()[0]
    return VC.VaeChain(sd, LAT[0], LAT[1], VC.VaeRefOps(dtype, round=False), wiring)


@functools.lru_cache(maxsize=None)
def _decode(dtype):
    _, z, _, mean, inv = _inputs()
    return _chain(dtype).decode(z, mean, inv)


@functools.lru_cache(maxsize=None)
def _encode(dtype):
    _, _, px, mean, inv = _inputs()
    return _chain(dtype).encode(px, mean, inv)


@functools.lru_cache(maxsize=None)
def _oracle(which):
    sd, z, px, mean, inv = _inputs()
    p = {k: v.double() for k, v in sd.items()}
    m, i = torch.tensor(mean, dtype=F64), torch.tensor(inv, dtype=F64)
    with torch.no_grad():
        if which == "decode":
            return vae_ref.decode(p, z.double().permute(1, 0, 2, 3).unsqueeze(0), m, i).clamp(-1, 1)[0].permute(1, 0, 2, 3).contiguous()
        return vae_ref.encode(p, px.double().unsqueeze(0), m, i)[0].permute(1, 0, 2, 3).contiguous()


def test_packers_match_the_products():
    """pack_conv / pack_frag, written from the header's description of the operands, give the bytes VaeEngine._repack / _frag_pack
    bind -- for every conv of the state dict, the padded head and the 3- and 16-channel first convs included."""
    sd = _inputs()[0]
    n = 0
    for key, t in sd.items():
        if not key.endswith(".weight") or key in ("conv1.weight", "conv2.weight") or ".to_qkv." in key or ".proj." in key:
            continue
        w = t.unsqueeze(2) if t.dim() == 4 else t
        if key == "decoder.head.2.weight":
            w = torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))])
        mine = VC.pack_conv(w)
        theirs = VaeEngine._repack(key, t).contiguous()
        assert mine.shape == theirs.shape and torch.equal(mine, theirs), key
        cin = (t.shape[1] + 31) // 32 * 32
        assert torch.equal(VC.pack_frag(mine, cin), VaeEngine._frag_pack(theirs, cin)), key
        n += 1
    assert n > 60


@pytest.mark.parametrize("which", ["decode", "encode"])
def test_chain_is_the_model(which):
    run = _decode if which == "decode" else _encode
    c64, c32, o = run(F64), run(F32), _oracle(which)
    assert c64.shape == o.shape and bool(torch.isfinite(c64).all())
    noise = rel_l2(c32, c64)
    d = rel_l2(c64, o)
    print(f"{which}: NOISE = {noise:.3e}, rel_l2(chain float64, oracle float64) = {d:.3e} = {d / noise:.3e} x NOISE")
    assert 1e-8 < noise < 1e-5, "the float32 noise of a ~60-conv network"
    assert d <= MULT * noise


@pytest.mark.parametrize("split", [(1, 2), (2, 1), (1, 1, 1)], ids=lambda s: "-".join(map(str, s)))
def test_stream_equals_one_shot(split):
    """Float64, the same operations in the same order: exactly equal, frame for frame."""
    _, z, _, mean, inv = _inputs()
    one = _decode(F64)
    s = _chain(F64).stream()
    outs, f0 = [], 0
    for n in split:
        outs.append(s.decode(z[f0:f0 + n], mean, inv))
        f0 += n
    assert [o.shape[0] for o in outs] == [4 * n - (3 if i == 0 else 0) for i, n in enumerate(split)]
    assert torch.equal(torch.cat(outs), one)


def test_rounded_chain_stays_at_the_network_tolerance():
    """VaeRefOps(round=True) -- the bf16 roundings of the per-launch references -- against the oracle: the whole-network 3e-2 of
    tests/test_vae_gpu.py.  (This is the arithmetic the VaeHipOps chain runs; nothing tighter holds for ~60 bf16 convs.)"""
    sd, z, _, mean, inv = _inputs()
    out = VC.VaeChain(sd, LAT[0], LAT[1], VC.VaeRefOps(F64, round=True)).decode(z[:2], mean, inv)
    d = rel_l2(out, _oracle("decode")[:5])
    print(f"rounded chain, decode of two latent frames: rel_l2 vs the oracle = {d:.3e}")
    assert d < 3e-2


# name -> (wiring override, which product shows it)
MUTANTS = {
    "cache_of_one_frame": (dict(cache_frames=1), "decode"),
    "first_frame_through_time_conv": (dict(first_frame="time_conv"), "decode"),
    "enc_time_conv_before_resample": (dict(enc_down_order=("time_conv", "resample")), "encode"),
    "gamma0_for_second_norm": (dict(norm2_gamma=lambda pre, cin, cout: pre + ("residual.0.gamma" if cin == cout else "residual.3.gamma")),
                               "decode"),
    "shortcut_from_the_activation": (dict(shortcut_src="act"), "decode"),
    "attention_scale_missing": (dict(attn_scale=lambda c: 1.0), "decode"),
    "zero_pad_on_the_wrong_side": (dict(down_pad=(1, 1)), "encode"),
    "head_gamma_from_the_last_block": (dict(dec_head_gamma="decoder.upsamples.14.residual.3.gamma"), "decode"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_of_the_chain_misses_the_oracle(name):
    """A chain with one wiring decision altered is farther from the oracle than 8 x NOISE, by the printed multiple of that bound."""
    wiring, which = MUTANTS[name]
    _, z, px, mean, inv = _inputs()
    ch = _chain(F64, wiring)
    got = ch.decode(z, mean, inv) if which == "decode" else ch.encode(px, mean, inv)
    run = _decode if which == "decode" else _encode
    bound = MULT * rel_l2(run(F32), run(F64))
    d = rel_l2(got, _oracle(which))
    print(f"mutant {name} ({which}): rel_l2 vs the oracle = {d:.3e} = {d / bound:.3e} x the bound {bound:.3e}")
    assert d > bound
