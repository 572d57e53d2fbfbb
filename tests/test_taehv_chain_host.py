"""The chain of tests/taehv_chain.py IS the model (CPU, no GPU): TaehvRefOps(float64, round=False) against the restatements of the
reference (tests/taehv_ref.py TaehvRef, tests/taehv_enc_ref.py TaehvEncRef) in float64, on the same weights
(mmpl_amd.synthetic.taehv_state_dict / taehv_encoder_state_dict, seed 5) and inputs.  Latents 3 x 5 and 9 x 13; 5 latent frames
decoded in calls of [3, 2], [1, 4] and [5]; 20 pixel frames encoded in calls of [12, 8], [4, 16] and [20]: every split but the last
continues a video, so the memories carried from call to call are exercised in both directions (a long call after a short one and
the reverse).  One more decoder case takes the checkpoint of test_patch_tgrow_layers, whose first TGrow has 2 * 256 rows.

The bound.  Both sides are float64 and differ only in the order of their sums (the chain convolves channels-last copies, splits
TGrow into one conv per frame and concatenates x and past itself).  d32 = rel_l2(restatement in float32, restatement in float64) on
the same inputs is the float32 noise of the reference itself, far above float64 re-ordering noise and far below any wiring
mistake; the chain must be within d32.  Measured (x86-64, torch CPU), d32 and the chain's worst split:

    decode 3 x 5   d32 4.6e-7   chain 1.5e-15        encode 3 x 5   d32 4.2e-7   chain 1.4e-15
    decode 9 x 13  d32 5.8e-7   chain 1.9e-15        encode 9 x 13  d32 4.0e-7   chain 1.3e-15
    decode 3 x 5, over-sized TGrow: d32 4.6e-7, chain 1.5e-15

Every mutant of the chain (MUTANTS: one or two per WIRING entry, 16 in all) misses the restatement in the same assertion, by
4.4e4 x (Clamp on the pixels too) to 3.0e6 x d32 (TGrow's frames reversed); the multiples are printed and listed in DESIGN.md 4.5.
No mutant is equivalent at these cases; what makes each visible:
`memory_from` and `past_offset` need a call of more than one frame that is continued ([3, 2], [12, 8]); `initial_memory` shows in
a video's first frame; `tgrow_block` needs a TGrow of stride 2 (levels 1 and 2); `tgrow_rows` needs the over-sized checkpoint.
"""
import functools
import os

import pytest
import torch

import taehv_enc_ref
import taehv_ref
from mmpl_amd.synthetic import philox_normal, taehv_encoder_state_dict, taehv_state_dict
from tests import taehv_chain as TC

F64, F32 = torch.float64, torch.float32
LATS = [(3, 5), (9, 13)]
DEC_SPLITS = [(3, 2), (1, 4), (5,)]
ENC_SPLITS = [(12, 8), (4, 16), (20,)]
SEED = 5
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _sd(big=False):
    sd = dict(taehv_state_dict(seed=SEED))
    sd.update(taehv_encoder_state_dict(seed=SEED))
    if big:                                                   # the checkpoint of tests/test_taehv_gpu.py::test_patch_tgrow_layers
        g = torch.Generator().manual_seed(97)
        extra = (torch.randn(256, 256, 1, 1, generator=g) * (1.0 / 16)).to(torch.bfloat16)
        sd["decoder.7.conv.weight"] = torch.cat([extra, sd["decoder.7.conv.weight"]], 0)
    return sd


@functools.lru_cache(maxsize=None)
def _input(which, lat):
    if which == "decode":
        return philox_normal([5, 16, lat[0], lat[1]], 47) * 1.5
    return philox_normal([20, 3, 8 * lat[0], 8 * lat[1]], 48).mul(0.25).add(0.5).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _model(which, lat, dtype, big=False):
    """The restatement, one-shot (its own split invariance is tests/test_taehv_host.py's and test_taehv_enc_host.py's)."""
    with torch.no_grad():
        if which == "decode":
            return taehv_ref.decode_video(_sd(big), _input(which, lat), dtype=dtype)
        return taehv_enc_ref.encode_video(_sd(big), _input(which, lat), dtype=dtype)


def _chain_run(which, lat, split, wiring=None, big=False, dtype=F64):
    ch = TC.TaehvChain(_sd(big), lat[0], lat[1], TC.TaehvRefOps(dtype, round=False), wiring)
    x = _input(which, lat)
    parts, f0 = [], 0
    with torch.no_grad():
        for n in split:
            parts.append(ch.decode(x[f0:f0 + n]) if which == "decode" else ch.encode(x[f0:f0 + n]))
            f0 += n
    return torch.cat(parts, 0)


def _check(which, lat, split, big=False):
    m64, m32 = _model(which, lat, F64, big), _model(which, lat, F32, big)
    got = _chain_run(which, lat, split, big=big)
    assert got.shape == m64.shape and bool(torch.isfinite(got).all())
    d32, d = rel_l2(m32, m64), rel_l2(got, m64)
    print(f"{which} {lat[0]} x {lat[1]} in calls of {list(split)}{' (over-sized TGrow)' if big else ''}: d32 = {d32:.3e}, "
          f"rel_l2(chain float64, restatement float64) = {d:.3e}")
    assert 1e-9 < d32 < 1e-5, "the float32 noise of a ~40-conv network"
    assert d <= d32


@pytest.mark.parametrize("split", DEC_SPLITS, ids=_id)
@pytest.mark.parametrize("lat", LATS, ids=_id)
def test_decode_chain_is_the_model(lat, split):
    _check("decode", lat, split)


@pytest.mark.parametrize("split", ENC_SPLITS, ids=_id)
@pytest.mark.parametrize("lat", LATS, ids=_id)
def test_encode_chain_is_the_model(lat, split):
    _check("encode", lat, split)


def test_decode_chain_is_the_model_oversized_tgrow():
    _check("decode", (3, 5), (3, 2), big=True)


def test_uint8_pixels_are_u_over_255():
    """The chain on uint8 pixels is the chain on float pixels u / 255 (float64: the same quotient)."""
    lat = (3, 5)
    u = (_input("encode", lat)[:8] * 255).to(torch.uint8)
    ch = lambda: TC.TaehvChain(_sd(), lat[0], lat[1], TC.TaehvRefOps(F64, round=False))
    a = ch().encode(u.permute(0, 2, 3, 1).contiguous())
    b = ch().encode(u.to(F64) / 255.0)
    assert torch.equal(a, b)


def test_reset_starts_a_new_video():
    lat = (3, 5)
    z = _input("decode", lat)
    ch = TC.TaehvChain(_sd(), lat[0], lat[1], TC.TaehvRefOps(F64, round=False))
    first = ch.decode(z[:2])
    cont = ch.decode(z[:2])
    ch.reset()
    again = ch.decode(z[:2])
    assert torch.equal(first, again) and not torch.equal(first, cont)


def test_rounded_chain_stays_at_the_network_tolerance():
    """TaehvRefOps(round=True) -- one bf16 rounding per launch, as the kernels do -- against the restatement: the whole-network
    bound of tests/test_taehv_gpu.py (2 x ref_bf16_rel_l2, about 1.2e-2).  Nothing tighter holds for 35 bf16 convolutions, which is
    why the GPU test compares bits with the launch chain instead."""
    lat = (3, 5)
    ch = TC.TaehvChain(_sd(), lat[0], lat[1], TC.TaehvRefOps(F64, round=True))
    d = rel_l2(ch.decode(_input("decode", lat)[:2]), _model("decode", lat, F64)[:8])
    bound = 2 * torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taehv_tiny.pt"))["ref_bf16_rel_l2"]
    print(f"rounded chain, decode of two latent frames: rel_l2 vs the restatement = {d:.3e}; bound {bound:.3e}")
    assert d <= bound


# ---------------------------------------------------------------------------------------------------- the packers
class _PackOps(TC.TaehvRefOps):
    def param(self, t):
        return t.detach().to(torch.bfloat16).contiguous()


def test_packers_match_the_products():
    """The chain's operands, packed from the header's description, are the bytes TaehvEngine._repack / TaehvEncoderEngine._repack
    bind: every conv of both halves, the padded head and bias, the input layer's 27-of-32 chunk; a TGrow block is its 16-row groups
    of the product's one matrix (after patch_tgrow_layers, on the over-sized checkpoint)."""
    from mmpl_amd.taehv import TaehvEncoderEngine, TaehvEngine, patch_tgrow_layers
    sd = _sd(big=True)
    ch = TC.TaehvChain(sd, 3, 5, _PackOps())
    psd = patch_tgrow_layers(sd)
    n = 0
    for key in sd:
        if not key.endswith(".weight"):
            continue
        name, eng = key[:-len(".weight")], TaehvEngine if key.startswith("decoder.") else TaehvEncoderEngine
        theirs = eng._repack(key, psd[key])
        if key in ("decoder.7.conv.weight", "decoder.13.conv.weight", "decoder.19.conv.weight"):
            S = {"decoder.7": 1, "decoder.13": 2, "decoder.19": 2}[name[:-len(".conv")]]
            C_ = psd[key].shape[0] // S
            groups = theirs.reshape(C_ // 32, 1, S * C_ // 16, 512)
            for j in range(S):
                mine = ch.cv_tgrow(name, C_, S, j).Wfrag
                assert torch.equal(mine.reshape(C_ // 32, 1, C_ // 16, 512), groups[:, :, j * C_ // 16:(j + 1) * C_ // 16]), (key, j)
        else:
            has_bias = name + ".bias" in sd
            cv = ch.cv_in() if key == "encoder.0.weight" else ch.cv(name, ntaps=psd[key].shape[-1] ** 2, bias=has_bias)
            assert cv.Wfrag.shape == theirs.shape and torch.equal(cv.Wfrag, theirs), key
            if has_bias:
                assert torch.equal(cv.bias, eng._repack(name + ".bias", sd[name + ".bias"])), key
        n += 1
    assert n == 35 + 35


# ---------------------------------------------------------------------------------------------------- mutants of the chain
# name -> (wiring override, which product shows it, the over-sized checkpoint?)
MUTANTS = {
    "cat_past_first": (dict(cat_order=("past", "x")), "decode", False),
    "past_is_the_frame_itself": (dict(past_offset=0), "encode", False),
    "memory_from_the_first_frame": (dict(memory_from=0), "decode", False),
    "memory_starts_at_one": (dict(initial_memory=1.0), "encode", False),
    "tgrow_frames_reversed": (dict(tgrow_block=lambda S, j: S - 1 - j), "decode", False),
    "tgrow_keeps_first_rows": (dict(tgrow_rows="first"), "decode", True),
    "tpool_pairs_overlap": (dict(tpool_pair=lambda t: (t, t + 1)), "encode", False),
    "tpool_odd_frame_first": (dict(tpool_order=(1, 0)), "encode", False),
    "no_relu_after_the_first_conv": (dict(relu_after_in=False), "decode", False),
    "relu_after_every_level_conv": (dict(relu_after_level=lambda half, lvl: True), "encode", False),
    "no_relu_in_front_of_the_head": (dict(relu_after_level=lambda half, lvl: False), "decode", False),
    "bias_on_the_level_conv": (dict(level_bias=lambda key: "decoder.9.conv.0.bias" if key == "decoder.8" else None), "decode", False),
    "bias_on_tgrow": (dict(level_bias=lambda key: "decoder.9.conv.0.bias" if key == "decoder.13.conv" else None), "decode", False),
    "bias_on_tpool": (dict(level_bias=lambda key: "encoder.0.bias" if key == "encoder.2.conv" else None), "encode", False),
    "no_clamp": (dict(clamp=()), "decode", False),
    "clamp_on_the_pixels_too": (dict(clamp=("decoder", "encoder")), "encode", False),
}


def test_every_wiring_entry_has_a_mutant():
    assert {k for w, _, _ in MUTANTS.values() for k in w} == set(TC.WIRING)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_of_the_chain_misses_the_model(name):
    """A chain with one wiring decision altered is farther from the restatement than d32, by the printed multiple."""
    wiring, which, big = MUTANTS[name]
    lat, split = (3, 5), (3, 2) if which == "decode" else (12, 8)
    m64 = _model(which, lat, F64, big)
    bound = rel_l2(_model(which, lat, F32, big), m64)
    d = rel_l2(_chain_run(which, lat, split, wiring, big), m64)
    print(f"mutant {name} ({which}): rel_l2 vs the restatement = {d:.3e} = {d / bound:.3e} x the bound {bound:.3e}")
    assert d > bound
