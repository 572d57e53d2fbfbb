"""mmpl_t5_encode, mmpl_clip_visual, mmpl_i2v_img_proj / _img_kv / _cross_attn and DitEngine.precompute_image_context against the SAME
LAUNCHES MADE ONE AT A TIME (-m gpu): the EncHipOps chains of tests/encoder_chain.py, written from the model
(tests/test_encoder_chain_host.py holds them to the oracle on the CPU) on the single-launch entries whose kernels the exact tests prove
one by one.  The host code that joins the launches -- which layer's position table a block reads, which projection the GELU takes,
which gain and eps a norm uses, the CLIP softmax scale, the padded-head packing, norm_k_img against norm_k, which layer's image
weights fill which slot -- has no rounding of its own, so the statement is the strongest there is: EVERY BIT equal.

Each case runs the product twice and the chain once, on the same inputs:
  1. through the Python engine, with every buffer the engine allocates for the call (its workspace, its `out`) arriving filled with
     the 0x7FA5 NaN pattern (torch.empty / torch.empty_like are wrapped for the duration of the call);
  2. through the C entry with the engine's own weight pointers, a workspace of exactly *_workspace_bytes filled with another NaN
     pattern (0x7F91) in front of a guard region, and an `out` pre-filled with NaN in front of a canary tail;
  3. the chain, every intermediate in a canary-tailed buffer of its own.
Demanded: equal bits of every output of 1 and 2 to 3's, no NaN left in an output, guard regions and tails untouched, every EncHipOps
canary intact, and the launch plans (plan_out of the chain's GEMM and attention launches) as the docstrings state them.
"""
import contextlib
import ctypes as C
import functools

import pytest
import torch

from tests import encoder_chain as EC
from tests import forward_chain as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 4096                              # bytes behind a workspace
POISON = (FC.CANARY, 0x7F91)              # two bf16 NaN patterns (as fp32 pairs: NaN too)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t


def n_diff(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return int((bits(a) != bits(b)).sum())


@contextlib.contextmanager
def poisoned_allocations(pattern):
    """What an engine allocates per call with torch.empty / torch.empty_like arrives filled with `pattern` (16 bits)."""
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_cuda and t.dtype in (torch.uint8, BF) and t.is_contiguous() and (t.numel() * t.element_size()) % 2 == 0:
            t.view(torch.int16).fill_(pattern)
        return t
    torch.empty = lambda *a, **k: fill(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


class Guarded:
    """nbytes of workspace filled with `pattern`, in front of GUARD bytes that must stay as they are."""

    def __init__(self, nbytes, pattern):
        assert nbytes % 2 == 0
        self.nbytes = nbytes
        self.full = torch.full(((nbytes + GUARD) // 2,), pattern, dtype=torch.int16, device=DEV)
        self.ws = self.full.view(torch.uint8)[:nbytes]
        self.pattern = pattern

    def intact(self):
        return bool((self.full[self.nbytes // 2:] == self.pattern).all())


class NanOut:
    """[*shape] bf16 pre-filled with the NaN canary in front of a canary tail."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.raw = torch.full((n + FC.TAIL,), FC.CANARY, dtype=torch.int16, device=DEV)
        self.t = self.raw[:n].view(BF).view(*shape)

    def intact(self):
        return bool((self.raw[self.n:] == FC.CANARY).all())


def _lib():
    from mmpl_amd import _lib
    return _lib, _lib.load()


def _ops():
    return EC.EncHipOps(_lib()[1], None, DEV)


def _agree(want, *gots, what="out"):
    torch.cuda.synchronize()
    assert not torch.isnan(want.float()).any() and bool((want != 0).any())
    for i, got in enumerate(gots):
        nd = n_diff(got, want)
        assert nd == 0, f"{what}, product run {i + 1}: {nd} of {want.numel()} elements differ from the chain's"


def _plans(ops):
    """name -> the set of plans its launches reported."""
    out = {}
    for name, plan in ops.plans:
        out.setdefault(name, set()).add(tuple(plan))
    print("launch plans:", {k: sorted(v) for k, v in sorted(out.items())})
    return out


def _arr(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ------------------------------------------------------------------------------------------------ umT5
@functools.lru_cache(maxsize=None)
def _t5(cfg_name, L):
    from mmpl_amd.synthetic import T5_CONFIGS, t5_state_dict
    from mmpl_amd.t5 import T5Engine
    cfg = T5_CONFIGS[cfg_name]
    sd = t5_state_dict(cfg, seed=21)
    eng = T5Engine(cfg, text_len=L, device=DEV)
    eng.load_state_dict(sd)
    return cfg, sd, eng


@pytest.mark.parametrize("cfg_name,L,n_valid", [("tiny", 64, 1), ("tiny", 64, 37), ("tiny", 64, 64), ("tiny", 128, 1), ("tiny", 128, 37),
                                                ("tiny", 128, 128), ("small", 128, 37)])
def test_t5_encode(cfg_name, L, n_valid):
    """T5Engine.encode and mmpl_t5_encode against T5Chain.encode: "tiny" (dim 256, 4 heads of 64, ffn 512, 2 layers) at text_len 64
    (one K tile of the PV GEMM) and 128 with 1, 37 and text_len valid tokens, "small" (8 heads, 3 layers: a block that reads layer 0's
    position table differs from one that reads the previous layer's) at 128; ids at both ends of the table.
    Plans: every GEMM -- qkv, the batched fp32 scores, the batched PV, o, gate, fc1, fc2 -- runs gemm_bf16_kernel (kernel 1, no tail)."""
    lib_mod, lib = _lib()
    cfg, sd, eng = _t5(cfg_name, L)
    ids = torch.randint(0, cfg["vocab"], (L,), generator=torch.Generator().manual_seed(100 + n_valid))
    ids[0], ids[1] = cfg["vocab"] - 1, 0
    mask = torch.zeros(L, dtype=torch.long)
    mask[:n_valid] = 1
    nb = lib.mmpl_t5_workspace_bytes(eng._h)
    g1 = Guarded(nb, POISON[0])
    eng._ws = g1.ws
    try:
        with poisoned_allocations(POISON[0]):
            out1 = eng.encode(ids[None], mask[None])[0]
        torch.cuda.synchronize()
    finally:
        eng._ws = None
    g2, o2 = Guarded(nb, POISON[1]), NanOut(L, cfg["dim"])
    ids_d, mask_d = ids.to(device=DEV, dtype=torch.int32), mask.to(device=DEV, dtype=torch.int32)
    with torch.cuda.device(DEV):
        lib_mod.check(lib.mmpl_t5_encode(eng._h, lib_mod.ptr(ids_d), lib_mod.ptr(mask_d), lib_mod.ptr(eng._bucket), lib_mod.ptr(o2.t),
                                         lib_mod.ptr(g2.ws), nb, lib_mod.stream_ptr()), "mmpl_t5_encode")
    ops = _ops()
    want = EC.T5Chain(sd, cfg, L, ops).encode(ids.clone(), mask.clone())
    _agree(want, out1, o2.t)
    assert g1.intact() and g2.intact() and o2.intact() and ops.canaries_intact()
    assert bool((want[n_valid:] == 0).all()) and bool((want[:n_valid].float().abs().amax(dim=1) > 0).all())
    plans = _plans(ops)
    assert set(plans) == {"t5_qkv", "t5_scores", "t5_pv", "t5_o", "t5_gate", "t5_fc1", "t5_fc2"}
    assert all(p[0] == 1 and p[1] == 0 for ps in plans.values() for p in ps)


# ------------------------------------------------------------------------------------------------ CLIP
CLIP_CASES = {"17-tokens-heads-of-80": dict(image_size=56, patch_size=14, dim=320, num_heads=4, num_layers=3),
              "257-tokens-heads-of-128": dict(image_size=224, patch_size=14, dim=256, num_heads=2, num_layers=2)}


@pytest.mark.parametrize("case", CLIP_CASES)
def test_clip_visual(case):
    """CLIPVisionTower.forward_pixels and mmpl_clip_visual against ClipChain.forward: the clip_visual_tiny geometry (56 px, patch 14:
    17 tokens; dim 320, 4 heads of 80 padded to 128; 3 layers built, 2 run) and the real tower's row count (224 px: 257 tokens, no
    multiple of 64 or 256; dim 256, 2 heads of 128: no padding; one block run).
    Plans: every GEMM runs gemm_bf16_kernel (kernel 1, no tail); the attention is a cross launch of ONE page on the lock-step
    kernels: attn_cross_kernel<1> (kernel 2) over the 17-row page, attn_fwd_kernel (kernel 1) over the 257-row page."""
    from mmpl_amd.i2v_clip import CLIPVisionTower
    from mmpl_amd.synthetic import clip_visual_state_dict, philox_normal
    lib_mod, lib = _lib()
    g = CLIP_CASES[case]
    sd = clip_visual_state_dict(g["dim"], g["num_heads"], g["num_layers"], g["image_size"], g["patch_size"], seed=31)
    tower = CLIPVisionTower(g["image_size"], g["patch_size"], g["dim"], 4, g["num_heads"], g["num_layers"], device=DEV)
    tower.load_state_dict(sd)
    px = philox_normal([1, 3, g["image_size"], g["image_size"]], 32)
    with poisoned_allocations(POISON[0]):
        out1 = tower.forward_pixels(px.to(DEV))[0]
    torch.cuda.synchronize()
    ops = _ops()
    ch = EC.ClipChain(sd, ops=ops, **g)
    patches = ops.tensor(ch.im2col(px[0]))
    n, d = ch.n, g["dim"]
    assert n == {"17-tokens-heads-of-80": 17, "257-tokens-heads-of-128": 257}[case] and tuple(patches.shape) == (n - 1, 640)
    nb = lib.mmpl_clip_visual_workspace_bytes(n, d, 4 * d, g["num_heads"])
    g2, o2 = Guarded(nb, POISON[1]), NanOut(n, d)
    with torch.cuda.device(DEV):
        lib_mod.check(lib.mmpl_clip_visual(lib_mod.ptr(patches.clone()), n - 1, ch.pk, d, 4 * d, g["num_heads"], d // g["num_heads"],
                                           g["num_layers"] - 1, _arr(tower._gw), _arr(tower._lw), 1e-5, lib_mod.ptr(o2.t), lib_mod.ptr(g2.ws), nb,
                                           lib_mod.stream_ptr()), "mmpl_clip_visual")
    want = ch.forward(patches)
    _agree(want, out1, o2.t)
    assert g2.intact() and o2.intact() and ops.canaries_intact()
    plans = _plans(ops)
    assert set(plans) == {"clip_patch", "clip_qkv", "clip_proj", "clip_mlp0", "clip_mlp2", "cross_attn"}
    assert all(p[0] == 1 and p[1] == 0 for k, ps in plans.items() if k != "cross_attn" for p in ps)
    assert {p[0] for p in plans["cross_attn"]} == ({2} if n == 17 else {1}) and all(p[1] == 1 for p in plans["cross_attn"])


# ------------------------------------------------------------------------------------------------ Wan-I2V
I2V_DIM, I2V_HEADS = 256, 2


@functools.lru_cache(maxsize=None)
def _i2v():
    from mmpl_amd.i2v_clip import MLPProj, WanI2VCrossAttention
    from mmpl_amd.synthetic import i2v_cross_state_dict, philox_normal
    ca_sd, mp_sd = i2v_cross_state_dict(I2V_DIM, seed=41)
    proj = MLPProj(1280, I2V_DIM, device=DEV)
    proj.load_state_dict(mp_sd)
    ca = WanI2VCrossAttention(I2V_DIM, I2V_HEADS, device=DEV)
    ca.load_state_dict(ca_sd)
    ctx = philox_normal([257 + 512, I2V_DIM], 43)
    ctx[257 + 77:] = 0                                     # the zero-padded tail of the text
    return ca_sd, mp_sd, proj, ca, ctx.to(DEV)


def test_i2v_img_proj():
    """MLPProj.__call__ and mmpl_i2v_img_proj at 257 x 1280 -> 256 against img_proj.
    Plans: both GEMMs (1280 -> 1280, 1280 -> 256 over 257 rows) run gemm_bf16_kernel (kernel 1, no tail)."""
    from mmpl_amd.synthetic import philox_normal
    lib_mod, lib = _lib()
    ca_sd, mp_sd, proj, ca, ctx = _i2v()
    clip = philox_normal([257, 1280], 42).to(DEV)
    with poisoned_allocations(POISON[0]):
        out1 = proj(clip[None])[0]
    torch.cuda.synchronize()
    nb = lib.mmpl_i2v_img_proj_workspace_bytes(257, 1280, I2V_DIM)
    g2, o2 = Guarded(nb, POISON[1]), NanOut(257, I2V_DIM)
    with torch.cuda.device(DEV):
        lib_mod.check(lib.mmpl_i2v_img_proj(lib_mod.ptr(clip.clone()), 257, 1280, I2V_DIM, _arr(proj._w), lib_mod.ptr(o2.t), lib_mod.ptr(g2.ws),
                                            nb, lib_mod.stream_ptr()), "mmpl_i2v_img_proj")
    ops = _ops()
    want = EC.img_proj(mp_sd, clip.clone(), ops)
    _agree(want, out1, o2.t)
    assert g2.intact() and o2.intact() and ops.canaries_intact()
    plans = _plans(ops)
    assert set(plans) == {"proj_fc1", "proj_fc2"} and all(p[0] == 1 and p[1] == 0 for ps in plans.values() for p in ps)


@pytest.mark.parametrize("which", ["img", "txt"], ids=["image-tokens-257-rows", "text-tokens-512-rows"])
def test_i2v_img_kv(which):
    """WanI2VCrossAttention.prepare and mmpl_i2v_img_kv against img_kv: the entry's two uses, on the 257 image tokens (k_img, v_img,
    norm_k_img) and on the 512 text tokens (k, v, norm_k).
    Plans: both GEMMs run gemm_bf16_kernel (kernel 1, no tail)."""
    lib_mod, lib = _lib()
    ca_sd, mp_sd, proj, ca, ctx = _i2v()
    with poisoned_allocations(POISON[0]):
        k_txt, v_txt, k_img, v_img = ca.prepare(ctx)
    torch.cuda.synchronize()
    src = ctx[:257].contiguous() if which == "img" else ctx[257:].contiguous()
    kn, vn, gn = ("k_img", "v_img", "norm_k_img") if which == "img" else ("k", "v", "norm_k")
    n = src.shape[0]
    k2, v2 = NanOut(n, I2V_DIM), NanOut(n, I2V_DIM)
    P = ca._p
    with torch.cuda.device(DEV):
        lib_mod.check(lib.mmpl_i2v_img_kv(lib_mod.ptr(src.clone()), n, I2V_DIM, lib_mod.ptr(P[kn + ".weight"]), lib_mod.ptr(P[kn + ".bias"]),
                                          lib_mod.ptr(P[vn + ".weight"]), lib_mod.ptr(P[vn + ".bias"]), lib_mod.ptr(P[gn + ".weight"]), 1e-6,
                                          lib_mod.ptr(k2.t), lib_mod.ptr(v2.t), lib_mod.stream_ptr()), "mmpl_i2v_img_kv")
    ops = _ops()
    want_k, want_v = EC.img_kv(ca_sd, src.clone(), ops, which)
    _agree(want_k, k_img if which == "img" else k_txt, k2.t, what="K")
    _agree(want_v, v_img if which == "img" else v_txt, v2.t, what="V")
    assert k2.intact() and v2.intact() and ops.canaries_intact()
    plans = _plans(ops)
    assert set(plans) == {"img_k", "img_v"} and all(p[0] == 1 and p[1] == 0 for ps in plans.values() for p in ps)


@pytest.mark.parametrize("Lq", [200, 288])
def test_i2v_cross_attn(Lq):
    """WanI2VCrossAttention.forward and mmpl_i2v_cross_attn at dim 256, 2 heads, over 512 text and 257 image keys, against
    i2v_cross_attn: Lq 200 (no multiple of 64) and 288 (3 frames of 96).
    Plans: both GEMMs run gemm_bf16_kernel (kernel 1, no tail); both attentions are cross launches of ONE page (512 and 257 rows,
    more than 128) on attn_fwd_kernel (kernel 1)."""
    from mmpl_amd.synthetic import philox_normal
    lib_mod, lib = _lib()
    ca_sd, mp_sd, proj, ca, ctx = _i2v()
    kv = ca.prepare(ctx)
    torch.cuda.synchronize()
    k_txt, v_txt, k_img, v_img = kv
    x = philox_normal([Lq, I2V_DIM], 44 + Lq).to(DEV)
    with poisoned_allocations(POISON[0]):
        out1 = ca(x[None], None, None, kv=kv)[0]
    torch.cuda.synchronize()
    nb = lib.mmpl_i2v_cross_attn_workspace_bytes(Lq, I2V_DIM)
    g2, o2 = Guarded(nb, POISON[1]), NanOut(Lq, I2V_DIM)
    P = ca._p
    with torch.cuda.device(DEV):
        lib_mod.check(lib.mmpl_i2v_cross_attn(lib_mod.ptr(x.clone()), Lq, I2V_DIM, lib_mod.ptr(P["q.weight"]), lib_mod.ptr(P["q.bias"]),
                                              lib_mod.ptr(P["norm_q.weight"]), 1e-6, lib_mod.ptr(k_txt), lib_mod.ptr(v_txt), 512, lib_mod.ptr(k_img),
                                              lib_mod.ptr(v_img), 257, lib_mod.ptr(P["o.weight"]), lib_mod.ptr(P["o.bias"]), lib_mod.ptr(o2.t),
                                              lib_mod.ptr(g2.ws), nb, lib_mod.stream_ptr()), "mmpl_i2v_cross_attn")
    ops = _ops()
    want = EC.i2v_cross_attn(ca_sd, x.clone(), k_txt.clone(), v_txt.clone(), k_img.clone(), v_img.clone(), ops)
    _agree(want, out1, o2.t)
    assert g2.intact() and o2.intact() and ops.canaries_intact()
    plans = _plans(ops)
    assert set(plans) == {"i2v_q", "i2v_o", "cross_attn"}
    assert all(p[0] == 1 and p[1] == 0 for k in ("i2v_q", "i2v_o") for p in plans[k])
    assert {(p[0], p[1]) for p in plans["cross_attn"]} == {(1, 1)}


def test_precompute_image_context():
    """DitEngine(model_type='i2v').precompute_image_context on the tiny config (2 layers, dim 256) against image_context: the freshly
    allocated pair and the out= in-place form (NaN-filled buffers with canary tails).  The loop over the layers is Python: which
    layer's k_img / v_img / norm_k_img weights fill which slot of img_k / img_v is decided there.
    Plans: img_emb's two GEMMs and every layer's k_img / v_img GEMM run gemm_bf16_kernel (kernel 1, no tail)."""
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, philox_normal
    cfg = dict(WAN_CONFIGS["tiny"], model_type="i2v", in_dim=36)
    sd = dit_i2v_state_dict(cfg, seed=6)
    eng = DitEngine(cfg, 16, 24, DEV)
    eng.load_state_dict(sd)
    L, d = cfg["num_layers"], cfg["dim"]
    clip = philox_normal([257, 1280], 9).to(DEV)
    with poisoned_allocations(POISON[0]):
        k1, v1 = eng.precompute_image_context(clip)
    torch.cuda.synchronize()
    k2, v2 = NanOut(L, 257, d), NanOut(L, 257, d)
    with poisoned_allocations(POISON[1]):
        rk, rv = eng.precompute_image_context(clip.clone(), out=(k2.t, v2.t))
    assert rk is k2.t and rv is v2.t
    ops = _ops()
    want_k, want_v = EC.image_context(sd, cfg, clip.clone(), ops)
    _agree(want_k, k1, k2.t, what="img_k")
    _agree(want_v, v1, v2.t, what="img_v")
    assert k2.intact() and v2.intact() and ops.canaries_intact()
    assert n_diff(want_k[0], want_k[1]) > 0 and n_diff(want_v[0], want_v[1]) > 0          # (the layers' slots do differ)
    plans = _plans(ops)
    assert set(plans) == {"proj_fc1", "proj_fc2", "img_k", "img_v"} and all(p[0] == 1 and p[1] == 0 for ps in plans.values() for p in ps)
