"""The chains of tests/encoder_chain.py ARE the model (CPU, no GPU): EncRefOps(float64, round=False) against the oracle run unrounded
on float64 copies of the weights (oracle/t5_ref.py, clip_ref.py, i2v_ref.py with acc=float64 and a float64 attention), on the same
inputs: umT5 "tiny" (2 layers) and "small" (3 layers) at text_len 64 with 37 valid tokens, the CLIP tower of the clip_visual_tiny
geometry (56 px, 17 tokens, dim 320, 4 heads of 80 padded to 128, 2 blocks run), MLPProj 257 x 1280 -> 256, the image and the text
K / V, WanI2VCrossAttention at Lq 200 over 257 image and 512 text tokens, and the per-layer image K / V of the tiny i2v DiT.

The bound.  NOISE = rel_l2(EncRefOps(float32), EncRefOps(float64)) of the same quantity is the float32 noise of this computation,
measured in the test itself; the oracle sums in another order (F.linear, F.layer_norm, einsum), so it is allowed MULT = 8 times that,
the project's bound for this statement (tests/test_forward_chain_host.py).  Measured (x86-64, torch CPU):

  quantity                                   NOISE              chain float64 vs oracle float64
  umT5 output, tiny / small                  2.8e-6 / 4.4e-6    0 (the same float64 operations in the same order)
  CLIP tokens                                4.5e-7             4.0e-9 = 0.009 x NOISE
  MLPProj, image K / V (also per DiT layer)  4.4e-7 .. 5.3e-7   4.5e-16 .. 6.6e-16
  text K / V                                 5.8e-8 / 1.0e-7    0
  WanI2VCrossAttention output                7.4e-7             6.4e-9 = 0.009 x NOISE
  CLIP heads padded to 128 against native 80, both float64: 7.8e-16.

Mutants of the chains, as multiples of the bound 8 x NOISE (umT5: tiny / small): position table of layer 0 in every layer
8.4e3 / 9.4e3, of the previous layer 8.4e3 / 9.5e3 (on two layers the same mistake, on three another one), norm2 with norm1's gain
1.2e4 / 1.2e4, GELU on fc1 4.2e4 / 3.1e4, eps 1e-5 251 / 249; CLIP scale 1 / sqrt(128) 2.0e4, norm2 with norm1's gain 2.7e4,
eps 1e-6 39; img_kv norming V 4.5e6, norm_k for norm_k_img 3.6e4, text and image K swapped 4.3e4, MLPProj eps 1e-6 3.0; layer 0's
k_img / v_img / norm_k_img weights in every slot 3.3e5 / 3.4e5 / 3.0e4.

The token embedding is scaled by 0.05 here so that the rows entering the first norm have a mean square of 2.5e-3: with the synthetic
table's unit-variance rows eps 1e-5 instead of 1e-6 moves a norm by 4.5e-6 of itself, the size of the bound; at 2.5e-3 it moves it by
1.8e-3.  The per-layer position tables are independent draws of std 0.5, so a block that reads another layer's table is far off.
Every wiring mutant of a chain exceeds the bound; by what factor is printed and recorded in DESIGN.md.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mmpl_amd.synthetic import (T5_CONFIGS, WAN_CONFIGS, clip_visual_state_dict, dit_i2v_state_dict, i2v_cross_state_dict, philox_normal,
                                t5_state_dict)
from oracle import clip_ref, i2v_ref, t5_ref
from oracle.wan_dit_ref import rms_norm
from tests import encoder_chain as EC

MULT = 8.0
F64, F32 = torch.float64, torch.float32
BF = torch.bfloat16


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def attn64(q, k, v):
    """[B, L, N, D] in and out, softmax(q k^T / sqrt(D)) v in the inputs' own dtype (attention.py:170-185 without its bf16 casts)."""
    q, k, v = (u.transpose(1, 2) for u in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).contiguous()


def check(name, q32, q64, qo):
    """Every quantity: finite, float32 noise of a sane size, chain float64 within MULT x noise of the oracle."""
    for k in q64:
        noise, err = rel_l2(q32[k], q64[k]), rel_l2(q64[k], qo[k])
        print(f"{name} {k}: noise {noise:.3e}  chain-vs-oracle {err:.3e}  ({err / noise:.3g} x)")
        assert torch.isfinite(q64[k]).all() and q64[k].shape == qo[k].shape
        assert 1e-8 < noise < 1e-5, (name, k, noise)
        assert err <= MULT * noise, (name, k, err, noise)


def check_mutant(name, qm, q32, q64, qo):
    worst = max((rel_l2(qm[k], qo[k]) / (MULT * rel_l2(q32[k], q64[k])), k) for k in qm)
    print(f"MUTANT {name}: worst quantity {worst[1]} at {worst[0]:.3g} x the bound")
    assert worst[0] > 1.0
    return worst[0]


# ------------------------------------------------------------------------------------------------ umT5
T5_L, T5_VALID = 64, 37


@functools.lru_cache(maxsize=None)
def _t5_inputs(cfg_name):
    cfg = T5_CONFIGS[cfg_name]
    sd = dict(t5_state_dict(cfg, seed=21))
    sd["token_embedding.weight"] = (sd["token_embedding.weight"].float() * 0.05).to(BF)     # small-variance rows: see the docstring
    ids = torch.randint(0, cfg["vocab"], (T5_L,), generator=torch.Generator().manual_seed(22))
    ids[0], ids[1] = cfg["vocab"] - 1, 0
    mask = torch.zeros(T5_L, dtype=torch.long)
    mask[:T5_VALID] = 1
    return cfg, sd, ids, mask


def _t5_chain(cfg_name, dtype, wiring=None):
    cfg, sd, ids, mask = _t5_inputs(cfg_name)
    return dict(out=EC.T5Chain(sd, cfg, T5_L, EC.EncRefOps(dtype), wiring).encode(ids, mask).clone())


@functools.lru_cache(maxsize=None)
def _t5_reference(cfg_name):
    cfg, sd, ids, mask = _t5_inputs(cfg_name)
    p = {k: v.double() for k, v in sd.items()}
    o = t5_ref.text_encoder_forward(p, ids[None], mask[None], cfg["num_heads"], cfg["num_buckets"], cfg["num_layers"], acc=F64)[0]
    return _t5_chain(cfg_name, F32), _t5_chain(cfg_name, F64), dict(out=o)


@pytest.mark.parametrize("cfg_name", ["tiny", "small"])
def test_t5_chain_equals_oracle(cfg_name):
    q32, q64, qo = _t5_reference(cfg_name)
    check("umT5 " + cfg_name, q32, q64, qo)
    assert q64["out"][T5_VALID:].abs().sum() == 0 and bool((q64["out"][:T5_VALID].abs().amax(dim=1) > 0).all())


T5_MUTANTS = {
    "position table of layer 0 in every layer": dict(t5_bias_layer=lambda l: 0),
    "position table of the previous layer": dict(t5_bias_layer=lambda l: max(l - 1, 0)),
    "norm2 with norm1's gain": dict(t5_norm2_gain="norm1"),
    "GELU on fc1 instead of gate": dict(t5_gelu_on="fc1"),
    "eps 1e-5": dict(t5_eps=1e-5),
}


@pytest.mark.parametrize("name", T5_MUTANTS)
@pytest.mark.parametrize("cfg_name", ["tiny", "small"])
def test_t5_chain_mutant_exceeds_the_bound(cfg_name, name):
    q32, q64, qo = _t5_reference(cfg_name)
    check_mutant(f"umT5 {cfg_name}: {name}", _t5_chain(cfg_name, F64, T5_MUTANTS[name]), q32, q64, qo)


def test_t5_the_two_position_table_mutants_differ_with_three_layers():
    """With three layers "layer 0's table everywhere" and "the previous layer's table" are different mistakes (with two they are one)."""
    a, b = (_t5_chain("small", F64, T5_MUTANTS[k])["out"] for k in list(T5_MUTANTS)[:2])
    assert rel_l2(a, b) > 1e-3
    a, b = (_t5_chain("tiny", F64, T5_MUTANTS[k])["out"] for k in list(T5_MUTANTS)[:2])
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ CLIP
CLIP_GEOM = dict(image_size=56, patch_size=14, dim=320, num_heads=4, num_layers=3)


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    g = CLIP_GEOM
    sd = clip_visual_state_dict(g["dim"], g["num_heads"], g["num_layers"], g["image_size"], g["patch_size"], seed=31)
    return sd, philox_normal([3, g["image_size"], g["image_size"]], 32)


def _clip_chain(dtype, wiring=None, pad_heads=True):
    sd, px = _clip_inputs()
    ops = EC.EncRefOps(dtype)
    ch = EC.ClipChain(sd, ops=ops, wiring=wiring, pad_heads=pad_heads, **CLIP_GEOM)
    assert (ch.n, ch.pk, ch.hd, ch.hp, ch.n_blocks) == (17, 640, 80, 128 if pad_heads else 80, 2)
    return dict(out=ch.forward(ops.tensor(ch.im2col(px))).clone())


@functools.lru_cache(maxsize=None)
def _clip_reference():
    sd, px = _clip_inputs()
    g = CLIP_GEOM
    o = clip_ref.clip_visual({k: v.double() for k, v in sd.items()}, px.double()[None], g["num_heads"], g["num_layers"], g["patch_size"],
                             attn_fn=attn64, acc=F64)[0]
    return _clip_chain(F32), _clip_chain(F64), dict(out=o)


def test_clip_chain_equals_oracle():
    check("CLIP", *_clip_reference())


def test_clip_padded_heads_equal_native_heads():
    """Heads of 80 zero-padded to 128 columns (zero rows and biases in to_qkv, zero columns in proj) against the chain at the native
    width, float64: the pad adds exact zeros to every sum, so the two agree to summation noise."""
    a, b = _clip_chain(F64)["out"], _clip_chain(F64, pad_heads=False)["out"]
    e = rel_l2(a, b)
    print(f"CLIP heads padded to 128 vs native 80, float64: rel_l2 {e:.3e}")
    assert e < 1e-13


CLIP_MUTANTS = {
    "softmax scale 1 / sqrt(128)": dict(clip_scale=lambda head_dim: 128.0 ** -0.5),
    "norm2 with norm1's gain": dict(clip_norm2_gain="norm1"),
    "eps 1e-6": dict(clip_eps=1e-6),
}


@pytest.mark.parametrize("name", CLIP_MUTANTS)
def test_clip_chain_mutant_exceeds_the_bound(name):
    q32, q64, qo = _clip_reference()
    check_mutant("CLIP: " + name, _clip_chain(F64, CLIP_MUTANTS[name]), q32, q64, qo)


# ------------------------------------------------------------------------------------------------ Wan-I2V
I2V_DIM, I2V_HEADS, I2V_LQ = 256, 2, 200


@functools.lru_cache(maxsize=None)
def _i2v_inputs():
    ca, mp = i2v_cross_state_dict(I2V_DIM, seed=41)
    clip = philox_normal([257, 1280], 42)
    txt = philox_normal([512, I2V_DIM], 43)
    txt[33:] = 0
    x = philox_normal([I2V_LQ, I2V_DIM], 44)
    return ca, mp, clip, txt, x


def _i2v_chain(dtype, wiring=None):
    ca, mp, clip, txt, x = _i2v_inputs()
    ops = EC.EncRefOps(dtype)
    ctx_img = EC.img_proj(mp, ops.tensor(clip), ops, wiring)
    k_img, v_img = EC.img_kv(ca, ctx_img, ops, "img", wiring)
    k_txt, v_txt = EC.img_kv(ca, ops.tensor(txt), ops, "txt", wiring)
    out = EC.i2v_cross_attn(ca, ops.tensor(x), k_txt, v_txt, k_img, v_img, ops, wiring)
    return dict(ctx_img=ctx_img, k_img=k_img, v_img=v_img, k_txt=k_txt, v_txt=v_txt, out=out)


@functools.lru_cache(maxsize=None)
def _i2v_reference():
    ca, mp, clip, txt, x = _i2v_inputs()
    ca64, mp64 = {k: v.double() for k, v in ca.items()}, {k: v.double() for k, v in mp.items()}
    ctx_img = i2v_ref.mlp_proj(mp64, clip.double())
    lin = lambda t, n: F.linear(t, ca64[n + ".weight"], ca64[n + ".bias"])
    qo = dict(ctx_img=ctx_img,
              k_img=rms_norm(lin(ctx_img, "k_img"), ca64["norm_k_img.weight"], 1e-6, F64), v_img=lin(ctx_img, "v_img"),
              k_txt=rms_norm(lin(txt.double(), "k"), ca64["norm_k.weight"], 1e-6, F64), v_txt=lin(txt.double(), "v"),
              out=i2v_ref.i2v_cross_attention(ca64, x.double()[None], torch.cat([ctx_img, txt.double()])[None], I2V_HEADS, attn_fn=attn64,
                                              acc=F64)[0])
    return _i2v_chain(F32), _i2v_chain(F64), qo


def test_i2v_chains_equal_oracle():
    check("I2V", *_i2v_reference())


I2V_MUTANTS = {
    "img_kv norms V instead of K": dict(i2v_normed="v"),
    "norm_k instead of norm_k_img": dict(i2v_img_gain="norm_k"),
    "text and image K swapped (their V kept)": dict(i2v_swap_k=True),
    "MLPProj eps 1e-6": dict(proj_eps=1e-6),
}


@pytest.mark.parametrize("name", I2V_MUTANTS)
def test_i2v_chain_mutant_exceeds_the_bound(name):
    q32, q64, qo = _i2v_reference()
    qm = _i2v_chain(F64, I2V_MUTANTS[name])
    check_mutant("I2V: " + name, qm, q32, q64, qo)
    assert rel_l2(qm["out"], qo["out"]) > MULT * rel_l2(q32["out"], q64["out"])           # and it shows in the block's output itself


# ------------------------------------------------------------------------------------------------ image context of the i2v DiT
@functools.lru_cache(maxsize=None)
def _ctx_inputs():
    cfg = dict(WAN_CONFIGS["tiny"], in_dim=36)
    return cfg, dit_i2v_state_dict(cfg, seed=6), philox_normal([257, 1280], 9)


def _ctx_chain(dtype, wiring=None):
    cfg, sd, clip = _ctx_inputs()
    ops = EC.EncRefOps(dtype)
    img_k, img_v = EC.image_context(sd, cfg, ops.tensor(clip), ops, wiring)
    return {f"{n}{l}": t[l] for n, t in (("img_k", img_k), ("img_v", img_v)) for l in range(cfg["num_layers"])}


@functools.lru_cache(maxsize=None)
def _ctx_reference():
    cfg, sd, clip = _ctx_inputs()
    p = {k: v.double() for k, v in sd.items()}
    ctx_img = i2v_ref.mlp_proj({k[len("img_emb."):]: v for k, v in p.items() if k.startswith("img_emb.")}, clip.double())
    qo = {}
    for l in range(cfg["num_layers"]):
        c = f"blocks.{l}.cross_attn."
        qo[f"img_k{l}"] = rms_norm(F.linear(ctx_img, p[c + "k_img.weight"], p[c + "k_img.bias"]), p[c + "norm_k_img.weight"], 1e-6, F64)
        qo[f"img_v{l}"] = F.linear(ctx_img, p[c + "v_img.weight"], p[c + "v_img.bias"])
    return _ctx_chain(F32), _ctx_chain(F64), qo


def test_image_context_chain_equals_oracle():
    q32, q64, qo = _ctx_reference()
    check("image context", q32, q64, qo)
    assert not torch.equal(q64["img_k0"], q64["img_k1"]) and not torch.equal(q64["img_v0"], q64["img_v1"])


CTX_MUTANTS = {
    "k_img weights of layer 0 in every slot": dict(img_layer=lambda l, part: 0 if part == "k" else l),
    "v_img weights of layer 0 in every slot": dict(img_layer=lambda l, part: 0 if part == "v" else l),
    "norm_k_img gain of layer 0 in every slot": dict(img_layer=lambda l, part: 0 if part == "norm" else l),
}


@pytest.mark.parametrize("name", CTX_MUTANTS)
def test_image_context_chain_mutant_exceeds_the_bound(name):
    q32, q64, qo = _ctx_reference()
    check_mutant("image context: " + name, _ctx_chain(F64, CTX_MUTANTS[name]), q32, q64, qo)
