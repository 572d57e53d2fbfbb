"""The chain of tests/forward_chain.py IS the model (CPU, no GPU): RefOps(float64, round=False) against the oracle run unrounded
(oracle/wan_dit_ref.py in float32 with sdpa_fp32), on the same inputs -- tiny config, lat 16 x 24 (S = 96): the four stages of
stage_ref.T2V_CLEAN_STEPS on one live cache (nF 2, 7, 6, 6; the last one is the non-persisting stage: write_slots all -1), the
outputs and every layer's K / V cache after each stage, and one i2v forward (in_dim 36, 257 image tokens).

The bound.  NOISE = rel_l2(RefOps(float32), RefOps(float64)) of the same quantity is the float32 noise of this computation, measured
in the test itself; the oracle sums in another order (F.linear, F.layer_norm, softmax of torch) and rounds its own float32 operations,
so it is allowed MULT = 8 times that.  Measured (x86-64, torch CPU): NOISE of the four outputs and of every layer's K / V cache after
every stage 3.0e-7 .. 3.1e-7 (i2v output: 4.0e-7); rel_l2(chain float64, oracle float32) 0.99 .. 1.08 x NOISE (i2v: 1.02 x).
The six chain mutants miss the oracle by far more than the bound 8 x NOISE = 2.4e-6: norm1 scale / shift swapped 5.6e4 x the bound,
self-attention gate from chunk 5 1.6e4 x, cross K from layer 0 2.4e3 x, head modulation from e0 2.9e4 x, image V from layer 0
2.1e5 x, and last_row_copies one short 5.8 x (1.4e-5 on the last stage's flow).  That last figure is why the prompt here has 500 valid
rows (12 copies of the padded key): with 20 valid rows (492 copies) one copy short moves the flow by 2.0e-6, 0.83 x the bound -- and
by 1e-4 of the 2e-2 that tests/test_dit_forward_gpu.py allows.  A wiring mistake of these kinds cannot hide in this comparison, and
the chain that passes it is the description tests/test_forward_chain_gpu.py holds the library's forward to, bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict, philox_normal
from oracle import stage_ref
from oracle import wan_dit_ref as W
from tests import forward_chain as FC

MULT = 8.0
LAT = (16, 24)
N_VALID = 500                 # 12 copies of the padded text key: one copy short moves its weight by 8 %
TVALS = [999.0, 640.0, 250.0, 0.0]
F64, F32 = torch.float64, torch.float32


def rel_l2(a, b):
    """In float64 (tests.util.rel_l2 compares in float32, which is the size of what is measured here)."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _stage_plan():
    vis = stage_ref.VisIndex()
    plan = []
    for si, frames in enumerate(stage_ref.stage_frames(stage_ref.T2V_CLEAN_STEPS)):
        if si == 2:
            vis.hide()
        if si == 3:
            vis.show()
        vis.on_forward(frames)
        plan.append((frames, stage_ref.write_slots_for(frames), list(vis.slots())))
    return plan


@functools.lru_cache(maxsize=None)
def _inputs():
    cfg = WAN_CONFIGS["tiny"]
    sd = dit_state_dict(cfg, seed=3)
    ctx = philox_normal([512, cfg["text_dim"]], 4)
    ctx[N_VALID:] = 0
    noise = philox_normal([1, 21, 16, LAT[0], LAT[1]], 5)
    return cfg, sd, ctx, noise


def _run_chain(dtype, wiring=None, collapse=True):
    """-> ([out per stage], [(K cache, V cache) after each stage], rows)."""
    cfg, sd, ctx, noise = _inputs()
    ops = FC.RefOps(dtype, round=False)
    ch = FC.ForwardChain(sd, cfg, LAT[0], LAT[1], ops, wiring)
    L, S, d = ch.L, ch.S, ch.dim
    ck, cv = torch.zeros(L, 512, d, dtype=dtype), torch.zeros(L, 512, d, dtype=dtype)
    rows = ch.precompute_context(ops.tensor(ctx), ck, cv)
    kc, vc = torch.zeros(L, 15 * S, d, dtype=dtype), torch.zeros(L, 15 * S, d, dtype=dtype)
    outs, caches = [], []
    for si, (frames, ws, vis) in enumerate(_stage_plan()):
        x = ops.tensor(noise[0, frames])
        t = torch.full([len(frames)], TVALS[si], dtype=F32)
        outs.append(ch.forward(x, t, frames, ws, vis, kc, vc, ck, cv, cross_rows=rows if collapse else None).clone())
        caches.append((kc.clone(), vc.clone()))
    return outs, caches, rows


@functools.lru_cache(maxsize=None)
def _chain(dtype):
    return _run_chain(dtype)


@functools.lru_cache(maxsize=None)
def _oracle():
    cfg, sd, ctx, noise = _inputs()
    ocfg = W.DitCfg(**cfg)
    p = {k: v.float() for k, v in sd.items()}
    S = (LAT[0] // 2) * (LAT[1] // 2)
    okv = W.new_kv_cache(ocfg, 15, S, dtype=F32)
    ocross = [None] * cfg["num_layers"]
    outs, caches = [], []
    for si, (frames, ws, vis) in enumerate(_stage_plan()):
        x = noise[0, frames].float()
        t = torch.full([1, len(frames)], TVALS[si], dtype=F32)
        y = W.dit_forward(p, ocfg, x.permute(1, 0, 2, 3), t, ctx.float(), okv, ocross, frames, ws, vis, attn_fn=W.sdpa_fp32)
        outs.append(y.permute(1, 0, 2, 3).clone())
        caches.append((torch.stack([c["k"].reshape(15 * S, -1) for c in okv]).clone(), torch.stack([c["v"].reshape(15 * S, -1) for c in okv]).clone()))
    return outs, caches


def _quantities(outs, caches):
    """name -> tensor, for every compared quantity of a four-stage run."""
    q = {}
    for si, (o, (k, v)) in enumerate(zip(outs, caches)):
        q[f"s{si}.out"] = o
        for l in range(k.shape[0]):
            q[f"s{si}.k{l}"], q[f"s{si}.v{l}"] = k[l], v[l]
    return q


def test_chain_equals_oracle_four_stages_live_cache():
    o64, c64, rows = _chain(F64)
    o32, c32, rows32 = _chain(F32)
    oo, co = _oracle()
    assert rows == rows32 == N_VALID
    q64, q32, qo = _quantities(o64, c64), _quantities(o32, c32), _quantities(oo, co)
    plan = _stage_plan()
    assert [len(p[0]) for p in plan] == [2, 7, 6, 6] and plan[3][1] == [-1] * 6          # (the last stage does not persist its K / V)
    for name in q64:
        noise = rel_l2(q32[name], q64[name])
        err = rel_l2(q64[name], qo[name])
        print(f"{name}: noise {noise:.3e}  chain-vs-oracle {err:.3e}  ({err / noise:.2f} x)")
        assert torch.isfinite(q64[name]).all()
        assert 1e-8 < noise < 1e-5, (name, noise)                  # float32 noise, neither zero (nothing compared) nor large
        assert err <= MULT * noise, (name, err, noise)
    # unwritten slots keep their fill in the chain as in the oracle: the set of non-zero slots is the same
    S = (LAT[0] // 2) * (LAT[1] // 2)
    for (k, v), (ko, vo) in zip(c64, co):
        assert torch.equal(k.reshape(k.shape[0], 15, S, -1).abs().amax(dim=(2, 3)) > 0, ko.reshape(k.shape[0], 15, S, -1).abs().amax(dim=(2, 3)) > 0)
        assert torch.equal(v.reshape(k.shape[0], 15, S, -1).abs().amax(dim=(2, 3)) > 0, vo.reshape(k.shape[0], 15, S, -1).abs().amax(dim=(2, 3)) > 0)


def test_collapsed_text_attention_equals_all_512_keys():
    """round=False: cross_rows = n attends over n + 1 keys, the last weighted 512 - n times -- the full softmax to float64 noise."""
    o_c, c_c, rows = _chain(F64)
    o_f, c_f, _ = _run_chain(F64, collapse=False)
    assert rows == N_VALID
    for si, (a, b) in enumerate(zip(o_c, o_f)):
        e = rel_l2(a, b)
        print(f"stage {si}: rel_l2(collapsed, all 512 keys) = {e:.3e}")
        assert e < 1e-12
        assert not torch.equal(a, b)                  # (the two really are different computations)


MUTANTS = {
    "norm1 scale / shift swapped": dict(norm1=(0, 1)),
    "self-attention gate from chunk 5": dict(gate1=5),
    "cross K from layer 0": dict(cross_k_layer=lambda l: 0),
    "last_row_copies one short": dict(copies=lambda T, n: T - n - 1),
    "head modulation from e0": dict(head_from="e0"),
}


@pytest.mark.parametrize("name", MUTANTS)
def test_chain_mutant_exceeds_the_bound(name):
    o64, c64, _ = _chain(F64)
    o32, c32, _ = _chain(F32)
    oo, co = _oracle()
    om, cm, _ = _run_chain(F64, wiring=MUTANTS[name])
    q64, q32, qo, qm = _quantities(o64, c64), _quantities(o32, c32), _quantities(oo, co), _quantities(om, cm)
    worst = max((rel_l2(qm[k], qo[k]) / (MULT * rel_l2(q32[k], q64[k])), k) for k in qm)
    print(f"{name}: worst quantity {worst[1]} at {worst[0]:.3g} x the bound; final output rel_l2 {rel_l2(om[-1], oo[-1]):.3e}")
    assert worst[0] > 1.0
    assert rel_l2(om[-1], oo[-1]) > MULT * rel_l2(o32[-1], o64[-1])              # and it shows in the flow of the last stage itself


# ------------------------------------------------------------------------------------------------ i2v
def _rms64(x, w, eps):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w


@functools.lru_cache(maxsize=None)
def _i2v_inputs():
    cfg = dict(WAN_CONFIGS["tiny"], in_dim=36)
    sd = dit_i2v_state_dict(cfg, seed=6)
    ctx = philox_normal([512, cfg["text_dim"]], 7)
    ctx[33:] = 0
    x = philox_normal([3, 36, LAT[0], LAT[1]], 8)
    clip = philox_normal([257, 1280], 9)
    return cfg, sd, ctx, x, clip


def _run_i2v_chain(dtype, wiring=None):
    from oracle.i2v_ref import mlp_proj
    cfg, sd, ctx, x, clip = _i2v_inputs()
    ops = FC.RefOps(dtype, round=False)
    ch = FC.ForwardChain(sd, cfg, LAT[0], LAT[1], ops, wiring)
    assert ch.in_dim == 36 and ch.pe_k == 192
    L, S, d = ch.L, ch.S, ch.dim
    p = {k: v.to(dtype) for k, v in sd.items()}
    ctx_img = mlp_proj({k[len("img_emb."):]: v for k, v in p.items() if k.startswith("img_emb.")}, clip.to(dtype))
    lin = lambda l, n: torch.nn.functional.linear(ctx_img, p[f"blocks.{l}.cross_attn.{n}.weight"], p[f"blocks.{l}.cross_attn.{n}.bias"])
    img_k = torch.stack([_rms64(lin(l, "k_img"), p[f"blocks.{l}.cross_attn.norm_k_img.weight"], ch.eps) for l in range(L)])
    img_v = torch.stack([lin(l, "v_img") for l in range(L)])
    ck, cv = torch.zeros(L, 512, d, dtype=dtype), torch.zeros(L, 512, d, dtype=dtype)
    rows = ch.precompute_context(ops.tensor(ctx), ck, cv)
    kc, vc = torch.zeros(L, 15 * S, d, dtype=dtype), torch.zeros(L, 15 * S, d, dtype=dtype)
    t = torch.full([3], 700.0, dtype=F32)
    return ch.forward(ops.tensor(x), t, [4, 5, 6], [4, 5, 6], [4, 5, 6], kc, vc, ck, cv, cross_rows=rows, img_k=img_k, img_v=img_v).clone()


@functools.lru_cache(maxsize=None)
def _i2v_reference():
    cfg, sd, ctx, x, clip = _i2v_inputs()
    ocfg = W.DitCfg(**cfg)
    p = {k: v.float() for k, v in sd.items()}
    S = (LAT[0] // 2) * (LAT[1] // 2)
    okv = W.new_kv_cache(ocfg, 15, S, dtype=F32)
    y = W.dit_forward(p, ocfg, x.float().permute(1, 0, 2, 3), torch.full([1, 3], 700.0), ctx.float(), okv, [None] * cfg["num_layers"], [4, 5, 6],
                      [4, 5, 6], [4, 5, 6], attn_fn=W.sdpa_fp32, clip_fea=clip.float())
    return y.permute(1, 0, 2, 3), _run_i2v_chain(F64), _run_i2v_chain(F32)


def test_chain_equals_oracle_i2v():
    yo, y64, y32 = _i2v_reference()
    noise, err = rel_l2(y32, y64), rel_l2(y64, yo)
    print(f"i2v: noise {noise:.3e}  chain-vs-oracle {err:.3e}  ({err / noise:.2f} x)")
    assert 1e-8 < noise < 1e-5 and err <= MULT * noise


def test_chain_mutant_image_v_from_layer_0():
    yo, y64, y32 = _i2v_reference()
    ym = _run_i2v_chain(F64, wiring=dict(img_v_layer=lambda l: 0))
    e = rel_l2(ym, yo)
    print(f"image V from layer 0: rel_l2 {e:.3e} = {e / (MULT * rel_l2(y32, y64)):.3g} x the bound")
    assert e > MULT * rel_l2(y32, y64)


# ------------------------------------------------------------------------------------------------ RoPE tables
def test_rope_table_rule_and_count():
    """The float32 table of the reference's formula, under the rule of forward_chain.rope_table_rule: 7 of its 131 072 entries lie
    within the angle's error bound of a float32 rounding boundary, so a table built by the same formula with another libm may differ
    in those 7 and in no other, by one float32 ulp (the library's own, on an MI355X host: 0 differ, tests/test_forward_chain_gpu.py).
    The oracle's own table (torch, complex128) rounded to float32 obeys the rule; a table whose frame and grid-row parts are
    exchanged, one built with theta 1e4 + 1 and one with a single entry moved by one ulp do not."""
    cs, sn, ang = FC.rope_tables_f64()
    may, differ, bad = FC.rope_table_rule(cs.astype(np.float32), sn.astype(np.float32))
    print(f"RoPE tables: {may} of {2 * cs.size} entries may differ by one float32 ulp")
    assert (differ, bad) == (0, 0) and may <= 8
    fr = W.rope_table(128)
    may2, differ2, bad2 = FC.rope_table_rule(fr.real.numpy().astype(np.float32), fr.imag.numpy().astype(np.float32))
    print(f"oracle's table: {differ2} entries differ, {bad2} outside the rule")
    assert bad2 == 0 and differ2 <= may
    swapped = np.concatenate([cs[:, 22:43], cs[:, :22], cs[:, 43:]], axis=1).astype(np.float32)
    assert FC.rope_table_rule(swapped, sn.astype(np.float32))[2] > 1000
    ang2 = ang * (np.log(10000.0) / np.log(10001.0))
    assert FC.rope_table_rule(np.cos(ang2).astype(np.float32), np.sin(ang2).astype(np.float32))[2] > 1000
    one_ulp = cs.astype(np.float32).copy()
    one_ulp[517, 3] = np.nextafter(one_ulp[517, 3], np.float32(2.0))             # one ulp where the rule allows none
    assert FC.rope_table_rule(one_ulp, sn.astype(np.float32))[2] == 1
