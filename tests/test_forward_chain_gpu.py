"""mmpl_dit_forward_at and mmpl_dit_precompute_context against the SAME LAUNCHES MADE ONE AT A TIME (-m gpu): the HipOps chain of
tests/forward_chain.py, written from the model (tests/test_forward_chain_host.py holds it to the oracle on the CPU) on the
single-launch entries whose kernels the exact tests prove one by one.  The code that joins the kernels -- which modulation chunk
feeds which norm and gate, which layer's slice of emod / cross_k / img_k / the history a block reads, where K and V go, which pages
are attended in which group, last_row_copies, the q prescale, the aliased buffers (xn as split-KV scratch, ksc as the image
attention's output) -- has no rounding of its own, so the statement is the strongest there is: EVERY BIT equal.

Each case fills the caches with seeded data, poisons the forward's workspace with the 0x7FA5 canary, runs DitEngine.forward, runs the
chain on clones of the same inputs, and demands equal bits of the output, the whole K and V cache (every layer and slot: unwritten
slots keep their fill), share_out, the history bytes, the five attention counters, cross_k / cross_v and the reported rows; every
HipOps canary intact and every GEMM scratch header zero again; and the same bits from a second forward whose workspace was poisoned
with another pattern.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import forward_chain as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_GEMMS = ("qkv", "o", "cross_q", "cross_o", "ffn0", "ffn2")


def bits(t):
    """A tensor's bytes as integers (NaN canaries compare equal to themselves)."""
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.uint8) if t.dtype == torch.uint8 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def n_diff(a, b):
    return int((bits(a) != bits(b)).sum())


class Model:
    """One engine and the chain that describes it."""

    def __init__(self, cfg_name="tiny", lat=(16, 24), seed=3, i2v=False, gain=1.0, self_variant="w64", cross_w64=False):
        from mmpl_amd import _lib
        from mmpl_amd.dit import DitEngine
        from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict
        cfg = dict(WAN_CONFIGS[cfg_name])
        if i2v:
            cfg.update(model_type="i2v", in_dim=36)
            sd = dit_i2v_state_dict(cfg, seed=seed)
        else:
            sd = dit_state_dict(cfg, seed=seed)
        if gain != 1.0:                                    # (tests/test_dit_forward_gpu.py::test_attention_redo_counters_blocks_and_waves)
            for l in range(cfg["num_layers"]):
                for k in ("self_attn.norm_q.weight", "self_attn.norm_k.weight"):
                    sd[f"blocks.{l}.{k}"] = (sd[f"blocks.{l}.{k}"].float() * gain).to(BF)
        self.cfg, self.sd, self.lat = cfg, sd, lat
        self.eng = DitEngine(cfg, lat[0], lat[1], DEV)
        self.eng.load_state_dict(sd)
        self.lib = _lib.load()
        self.variant = dict(self_variant=self_variant, cross_w64=cross_w64)
        self.stats = self.eng.enable_attn_stats()
        self.L, self.S, self.d, self.in_dim = self.eng.L, self.eng.S, self.eng.dim, self.eng.in_dim

    def chain(self):
        ops = FC.HipOps(self.lib, self.eng, DEV)
        return FC.ForwardChain(self.sd, self.cfg, self.lat[0], self.lat[1], ops), ops

    def caches(self, seed, n_slots=15):
        from mmpl_amd.synthetic import philox_normal
        kc, vc = self.eng.new_kv_cache(n_slots)
        kc.copy_(philox_normal(list(kc.shape), seed).to(DEV))
        vc.copy_(philox_normal(list(vc.shape), seed + 1).to(DEV))
        return kc, vc

    def context(self, n_valid, seed=4):
        """-> (ck, cv, rows) of the library, compared with the context chain in every bit."""
        from mmpl_amd.synthetic import philox_normal
        ctx = philox_normal([512, self.cfg["text_dim"]], seed)
        ctx[n_valid:] = 0
        ctx = ctx.to(DEV)
        outs = []
        for poison in (0xA5, 0xFF):
            nb = self.lib.mmpl_dit_context_workspace_bytes(self.eng._h)
            self.eng._ctx_ws = torch.full((nb,), poison, dtype=torch.uint8, device=DEV)
            kv = self.eng.precompute_context(ctx)
            torch.cuda.synchronize()
            outs.append((kv[0].clone(), kv[1].clone(), kv.rows))
        ch, ops = self.chain()
        ck = ops.new(self.L * 512, self.d).view(self.L, 512, self.d)
        cv = ops.new(self.L * 512, self.d).view(self.L, 512, self.d)
        rows = ch.precompute_context(ctx, ck, cv)
        for k_, v_, r_ in outs:
            assert r_ == rows == (n_valid if n_valid <= 510 else 512), (r_, rows, n_valid)
            assert same(k_, ck) and same(v_, cv), (n_diff(k_, ck), n_diff(v_, cv))
        assert ops.canaries_intact()
        return outs[0]

    def check(self, x, t, frames, ws_slots, vis, kc0, vc0, ck, cv, cross_rows=None, share=None, share_in=None, img=None, hist0=None,
              frame_base=None, want_plans=False):
        """One forward from the state (kc0, vc0, hist0), twice with differently poisoned workspaces, against the chain on clones.
        share = True: a share_out forward.  -> dict(out, kc, vc, share, hist, stats[, plans]) as the forward left them."""
        eng, nF = self.eng, len(frames)
        runs = []
        for poison in (FC.CANARY, 0x7F91):
            kc, vc = kc0.clone(), vc0.clone()
            hist = None if hist0 is None else hist0.clone()
            sh = torch.full((nF * self.S * self.d,), float("nan"), dtype=BF, device=DEV) if share else None
            ws = eng.workspace(nF)
            ws.view(torch.int16).fill_(poison)
            self.stats.zero_()
            out = eng.forward(x, t, frames, ws_slots, vis, kc, vc, ck, cv, cross_rows=cross_rows, share_out=sh, share_in=share_in,
                              attn_history=hist, frame_base=frame_base)
            torch.cuda.synchronize()
            runs.append(dict(out=out.clone(), kc=kc, vc=vc, share=sh, hist=hist, stats=self.stats.clone()))
        ch, ops = self.chain()
        kc, vc = kc0.clone(), vc0.clone()
        hist = None if hist0 is None else hist0.clone()
        sh = torch.full((nF * self.S * self.d,), float("nan"), dtype=BF, device=DEV) if share else None
        stats = torch.zeros(5, dtype=torch.int64, device=DEV)
        out = ch.forward(x, t, frames, ws_slots, vis, kc, vc, ck, cv, cross_rows=cross_rows, share_out=sh, share_in=share_in,
                         img_k=None if img is None else img[0], img_v=None if img is None else img[1], attn_history=hist, stats=stats,
                         frame_base=frame_base, **self.variant)
        want = dict(out=out, kc=kc, vc=vc, share=sh, hist=hist, stats=stats)
        for i, r in enumerate(runs):
            for name in ("out", "kc", "vc", "share", "hist", "stats"):
                if want[name] is None:
                    assert r[name] is None
                    continue
                nd = n_diff(r[name], want[name])
                assert nd == 0, f"forward run {i}: {nd} of {want[name].numel()} elements of {name} differ from the chain's"
        assert not torch.isnan(out.float()).any() and bool((out != 0).any())
        assert ops.canaries_intact()
        res = runs[0]
        if want_plans:
            res["plans"] = ops.plans
        return res


def _inputs(m, nF, seed, tval=700.0):
    from mmpl_amd.synthetic import philox_normal
    x = philox_normal([nF, m.in_dim, m.lat[0], m.lat[1]], seed).to(DEV)
    t = torch.full([nF], tval, dtype=torch.float32, device=DEV)
    return x, t


@pytest.fixture(scope="module")
def tiny():
    m = Model()
    m.kv37 = m.context(37)
    return m


# ------------------------------------------------------------------------------------------------ the cases
def test_persisting_stages_on_one_live_cache(tiny):
    """nF 1, 3, 7 and 2 in sequence; the visible list is unsorted and includes the slots just written; the cache starts from a
    seeded fill, so a slot nobody wrote must still hold it."""
    m = tiny
    ck, cv, rows = m.kv37
    kc, vc = m.caches(10)
    stages = [([0], [0], [0]),
              ([1, 2, 3], [1, 2, 3], [3, 0, 2, 1]),
              ([4, 5, 6, 7, 8, 9, 10], [4, 5, 6, 7, 8, 9, 10], [10, 4, 0, 7, 5, 1, 9, 6, 8]),
              ([19, 20], [13, 14], [14, 2, 13, 9, 0])]
    fill_k = kc.clone()
    for si, (frames, ws_slots, vis) in enumerate(stages):
        x, t = _inputs(m, len(frames), 20 + si, [999.0, 640.0, 250.0, 0.0][si])
        r = m.check(x, t, frames, ws_slots, vis, kc, vc, ck, cv, cross_rows=rows)
        kc, vc = r["kc"], r["vc"]
    S = m.S
    assert same(kc[:, 11 * S:13 * S], fill_k[:, 11 * S:13 * S]) and not same(kc[:, :S], fill_k[:, :S])


def test_non_persisting_stage_scratch_pages_in_group_1(tiny):
    """write_slots all -1: the stage's own K / V are scratch pages of another allocation (page group 1) behind the visible cache slots,
    adjacent ones (0 1 2, 9 10: merged) and one that is not (5)."""
    m = tiny
    ck, cv, rows = m.kv37
    kc, vc = m.caches(30)
    x, t = _inputs(m, 3, 31, 433.0)
    r = m.check(x, t, [13, 14, 15], [-1, -1, -1], [9, 0, 5, 2, 10, 1], kc, vc, ck, cv, cross_rows=rows)
    assert same(r["kc"], kc) and same(r["vc"], vc)        # nothing persisted


@pytest.mark.parametrize("cross_rows", [None, 0, 1, 37, 510, 511, 512])
def test_cross_rows_and_precompute_context(tiny, cross_rows):
    """The context chain for n_valid = cross_rows (text embedding, row comparison, host-side count, per-layer K / norm / V), then a
    forward told that count: collapsed up to 510, all 512 keys from 511 on and for None."""
    m = tiny
    n_valid = 37 if cross_rows is None else cross_rows
    ck, cv, rows = m.kv37 if n_valid == 37 else m.context(n_valid, seed=40 + n_valid)
    kc, vc = m.caches(50)
    x, t = _inputs(m, 2, 51)
    m.check(x, t, [0, 1], [0, 1], [1, 0], kc, vc, ck, cv, cross_rows=cross_rows)


@pytest.mark.parametrize("persist", [True, False])
def test_shared_block0(tiny, persist):
    """A share_out forward, then a share_in forward: the chain skips what the header says is skipped (block 0's attention and output
    projection) and still writes layer 0's K / V when the stage persists."""
    m = tiny
    ck, cv, rows = m.kv37
    ck_u, cv_u, rows_u = m.context(9, seed=61)
    kc, vc = m.caches(60)
    frames, ws_slots, vis = ([4, 5, 6], [4, 5, 6], [6, 0, 1, 4, 5]) if persist else ([4, 5, 6], [-1, -1, -1], [0, 1, 2])
    x, t = _inputs(m, 3, 62, 433.0)
    prod = m.check(x, t, frames, ws_slots, vis, kc, vc, ck, cv, cross_rows=rows, share=True)
    kc_u, vc_u = m.caches(64)
    kc_u[0].copy_(kc[0])                                   # the precondition: layer 0 of the two caches agrees
    vc_u[0].copy_(vc[0])
    kc_u[0, 4 * m.S:7 * m.S] = 0                           # ... and the consumer's own layer-0 slots are to be written by IT
    cons = m.check(x, t, frames, ws_slots, vis, kc_u, vc_u, ck_u, cv_u, cross_rows=rows_u, share_in=prod["share"])
    if persist:
        assert same(cons["kc"][0, 4 * m.S:7 * m.S], prod["kc"][0, 4 * m.S:7 * m.S])
    assert not same(cons["out"], prod["out"])


def test_i2v_image_kv_per_layer():
    from mmpl_amd.synthetic import philox_normal
    m = Model(i2v=True, seed=6)
    assert m.in_dim == 36 and m.lib.mmpl_dit_workspace_bytes(m.eng._h, 1) > 0
    img_k = philox_normal([m.L, 257, m.d], 70).to(DEV)
    img_v = philox_normal([m.L, 257, m.d], 71).to(DEV)
    assert not same(img_k[0], img_k[1])
    m.eng.set_image_kv(img_k, img_v)
    ck, cv, rows = m.context(33, seed=7)
    kc, vc = m.caches(72)
    x, t = _inputs(m, 3, 73)
    m.check(x, t, [4, 5, 6], [4, 5, 6], [0, 5, 4, 6], kc, vc, ck, cv, cross_rows=rows, img=(img_k, img_v))


@pytest.mark.parametrize("base,ids", [(5, [0, 1, 2]), (1020, [0, 2, 5])], ids=["base-5", "base-1020-clamped"])
def test_frame_base_device_scalar(tiny, base, ids):
    """frame_ids relative to a device scalar; 1020 + 5 passes 1023, so the clamp is exercised."""
    m = tiny
    ck, cv, rows = m.kv37
    kc, vc = m.caches(80)
    x, t = _inputs(m, 3, 81)
    fb = torch.tensor([base], dtype=torch.int32, device=DEV)
    r = m.check(x, t, ids, [1, 2, 3], [0, 1, 2, 3], kc, vc, ck, cv, cross_rows=rows, frame_base=fb)
    r0 = m.check(x, t, [min(i + base, 1023) for i in ids], [1, 2, 3], [0, 1, 2, 3], kc, vc, ck, cv, cross_rows=rows)
    assert same(r["out"], r0["out"]) and same(r["kc"], r0["kc"])
    other = m.check(x, t, ids, [1, 2, 3], [0, 1, 2, 3], kc, vc, ck, cv, cross_rows=rows)
    assert not same(other["kc"], r["kc"])                  # (the base does move the rotation)


def test_attn_history_consecutive_forwards_on_one_buffer():
    """QK-norm gains x 12: blocks fail their FAST pass, so the history leaves the zero state, and every forward starts from what the one
    before left (oracle/attn_history_ref.py: first failure -> references stored; FAST on them; a second failure -> straight to the
    GENERAL pass).  Three consecutive forwards; history bytes and counters after each equal the chain's."""
    m = Model(gain=12.0)
    ck, cv, rows = m.context(37)
    kc, vc = m.caches(90)
    hist = m.eng.new_attn_history(2)
    assert hist.numel() == m.L * m.lib.mmpl_attn_history_bytes(2 * m.S, m.cfg["num_heads"])
    seen = []
    for step in range(3):
        x, t = _inputs(m, 2, 91 + step, 700.0 - 100.0 * step)
        r = m.check(x, t, [0, 1], [0, 1], [0, 1], kc, vc, ck, cv, cross_rows=rows, hist0=hist)
        kc, vc, hist = r["kc"], r["vc"], r["hist"]
        seen.append([int(v) for v in r["stats"].cpu()])
        hb = hist.numel() // m.L
        assert bool((hist[:hb] != 0).any()) and bool((hist[hb:] != 0).any()) and not same(hist[:hb], hist[hb:])     # both layers' slices, each its own
    print("attention counters per forward {blocks, redone, waves, straight to GENERAL, held on remembered}:", seen)
    assert seen[0][1] > 0 and seen[0][3] == seen[0][4] == 0            # blocks were redone: the history left the zero state
    # the later forwards used it: a block's FAST pass held on the remembered references, or it failed again and the next forward
    # sent the block straight to the GENERAL pass
    assert seen[1][4] + seen[2][4] + seen[2][3] > 0


def test_small_config():
    m = Model("small", (12, 20), seed=8)
    ck, cv, rows = m.context(33, seed=9)
    kc, vc = m.caches(100)
    x, t = _inputs(m, 3, 101, 500.0)
    m.check(x, t, [2, 3, 10], [2, 3, 10], [10, 0, 3, 2, 1], kc, vc, ck, cv, cross_rows=rows)


def test_large_case_runs_256x256_kernels_with_a_tail_launch():
    """lat 60 x 104, 7 frames (M = 10 920 rows): the block GEMMs run a 256 x 256 kernel and at least one of them a tail launch for its
    partial last round, so the tile tickets and the scratch are part of the comparison."""
    m = Model(lat=(60, 104))
    ck, cv, rows = m.context(20)
    kc, vc = m.caches(110)
    x, t = _inputs(m, 7, 111, 640.0)
    frames = [2, 3, 10, 11, 12, 19, 20]
    r = m.check(x, t, frames, [2, 3, 10, 11, 12, 13, 14], [14, 0, 1, 2, 3, 10, 11, 12, 13], kc, vc, ck, cv, cross_rows=rows, want_plans=True)
    plans = [(n, p) for n, p in r["plans"] if n in BLOCK_GEMMS]
    print("block GEMM plans:", sorted({(n, tuple(p)) for n, p in plans}))
    assert all(p[0] in (3, 4) for _, p in plans)
    assert any(p[1] != 0 and p[4] > 0 for _, p in plans)


def test_rope_tables_of_the_handle(tiny):
    """mmpl_dit_rope_tables against the float64 table of the reference's formula, under the rule of the host test: only entries within
    the angle's error bound of a float32 rounding boundary may differ, and then by one float32 ulp."""
    cs, sn = FC.HipOps(tiny.lib, tiny.eng, DEV).rope_tables()
    may, differ, bad = FC.rope_table_rule(cs.cpu().numpy(), sn.cpu().numpy())
    print(f"RoPE tables of the handle: {differ} entries differ from float32(float64 table), {may} may, {bad} break the rule")
    assert bad == 0 and differ <= may


# ------------------------------------------------------------------------------------------------ environment switches
def _child(kind):
    """Runs in a fresh process whose environment holds the switch (read once per process): one persisting and one non-persisting
    forward against the chain told the same setting."""
    m = Model(self_variant="lockstep" if kind == "attn_v1" else "w64", cross_w64=kind == "cross_w64")
    ck, cv, rows = m.context(37)
    kc, vc = m.caches(120)
    x, t = _inputs(m, 3, 121)
    r = m.check(x, t, [1, 2, 3], [1, 2, 3], [3, 0, 2, 1], kc, vc, ck, cv, cross_rows=rows)
    m.check(x, t, [13, 14, 15], [-1, -1, -1], [0, 3, 1, 2], r["kc"], r["vc"], ck, cv, cross_rows=rows)
    print("CHILD-OK", kind)


@pytest.mark.parametrize("kind,env", [("attn_v1", "MMPL_ATTN_V1"), ("cross_w64", "MMPL_CROSS_W64")])
def test_environment_switch_in_a_fresh_process(kind, env):
    e = dict(os.environ, **{env: "1"})
    r = subprocess.run([sys.executable, "-c", f"from tests.test_forward_chain_gpu import _child; _child({kind!r})"], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"CHILD-OK {kind}" in r.stdout


def test_environment_switches_change_the_bits(tiny):
    """(What makes the two child runs meaningful: told the OTHER setting, the chain does not reproduce this process's forward.)"""
    m = tiny
    ck, cv, rows = m.kv37
    kc, vc = m.caches(120)
    x, t = _inputs(m, 3, 121)
    for other in (dict(self_variant="lockstep", cross_w64=False), dict(self_variant="w64", cross_w64=True)):
        keep, m.variant = m.variant, other
        try:
            with pytest.raises(AssertionError, match="differ from the chain's"):
                m.check(x, t, [1, 2, 3], [1, 2, 3], [3, 0, 2, 1], kc, vc, ck, cv, cross_rows=rows)
        finally:
            m.variant = keep
