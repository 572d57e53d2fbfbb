"""Step caching (TeaCache) on the GPU (-m gpu): the cached forward entries, the indicator's two entries, the two 50-step pipelines and
WanT2V.generate.  Tiny synthetic config at 16 x 24 latents (96 rows per frame: 1 and 3 frames are 96 and 288 rows, neither a
multiple of the 256-row query block or of a GEMM tile).

Every forward statement is an equality of bits: OFF and RECORD against the uncached entry, the RECORD residual against
bf16(x_L - x_0) computed on the host from the ForwardChain trace of the same forward, REUSE against the public launches made one at
a time.  mmpl_rel_l1_rows: exact on small-integer data; on normal data within 2 (d + 1) 2^-24 relative of float64 -- two d-term
float32 sums of non-negative terms (each at most (d - 1) u in any order, u = 2^-24) and one division, to first order 2 (d - 1) u + u.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import forward_chain as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LAT = (16, 24)
OFF, RECORD, REUSE = 0, 1, 2


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def ints(v):
    return (C.c_int * max(len(v), 1))(*[int(i) for i in v])


class Model:
    """One engine, its weights as the chain reads them, one prompt's cross K / V."""

    def __init__(self, i2v=False, seed=3):
        from mmpl_amd import _lib
        from mmpl_amd.dit import DitEngine
        from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict, philox_normal
        cfg = dict(WAN_CONFIGS["tiny"])
        if i2v:
            cfg.update(model_type="i2v", in_dim=36)
        self.sd = (dit_i2v_state_dict if i2v else dit_state_dict)(cfg, seed=seed)
        self.cfg, self._lib, self.lib = cfg, _lib, _lib.load()
        self.eng = DitEngine(cfg, LAT[0], LAT[1], DEV)
        self.eng.load_state_dict(self.sd)
        self.stats = self.eng.enable_attn_stats()
        self.L, self.S, self.d, self.in_dim = self.eng.L, self.eng.S, self.eng.dim, self.eng.in_dim
        ctx = philox_normal([512, cfg["text_dim"]], 4)
        ctx[37:] = 0
        kv = self.eng.precompute_context(ctx.to(DEV))
        self.ck, self.cv, self.rows = kv[0], kv[1], kv.rows
        self.img = None
        if i2v:
            self.img = (philox_normal([self.L, 257, self.d], 70).to(DEV), philox_normal([self.L, 257, self.d], 71).to(DEV))
            self.eng.set_image_kv(*self.img)

    def chain(self):
        ops = FC.HipOps(self.lib, self.eng, DEV)
        return FC.ForwardChain(self.sd, self.cfg, LAT[0], LAT[1], ops), ops

    def caches(self, seed):
        from mmpl_amd.synthetic import philox_normal
        kc, vc = self.eng.new_kv_cache(15)
        kc.copy_(philox_normal(list(kc.shape), seed).to(DEV))
        vc.copy_(philox_normal(list(vc.shape), seed + 1).to(DEV))
        return kc, vc

    def residual(self, nF, fill=float("nan")):
        r = self.eng.new_step_cache(nF)
        assert r.data_ptr() % 256 == 0 and r.numel() * 2 == self.lib.mmpl_dit_step_cache_bytes(self.eng._h, nF) >= nF * self.S * self.d * 2
        r.fill_(fill)
        return r

    def at_cached(self, x, t, frames, ws_slots, vis, kc, vc, out, mode, residual, share_out=None, share_in=None, ck="own", cv="own"):
        """mmpl_dit_forward_at_cached itself (DitEngine.forward routes OFF to the uncached entry) -> its return code."""
        ws = self.eng.workspace(len(frames))
        ck, cv = (self.ck if ck == "own" else ck), (self.cv if cv == "own" else cv)
        with torch.cuda.device(DEV):
            return self.lib.mmpl_dit_forward_at_cached(
                self.eng._h, P(x), P(t), len(frames), ints(frames), ints(ws_slots), ints(vis), len(vis), P(kc), P(vc), kc.shape[1] // self.S,
                P(ck), P(cv), self.rows, P(share_out), P(share_in), None, P(out), P(ws), ws.numel(), None, self._lib.stream_ptr(),
                mode, P(residual))

    def reuse_chain(self, x_in, t, residual):
        """A REUSE forward as public launches, one at a time: patchify, mmpl_gemm with epilogue 4 and the residual, then the timestep
        embedding, the head modulation and the head as ForwardChain makes them.  x_in [nF, in_dim, h, w]; t [nT] (one row per frame,
        or ONE row for a whole clip: every frame then reads row 0)."""
        ch, ops = self.chain()
        p, d, S = ch.p, self.d, self.S
        nF, nT = x_in.shape[0], t.numel()
        Lq = nF * S
        patch = ops.new(Lq, ch.pe_k)
        ops.patchify(patch, x_in, self.in_dim, LAT[0], LAT[1])
        x = ops.new(Lq, d)
        with torch.cuda.device(DEV):
            self._lib.check(self.lib.mmpl_gemm(P(patch), ch.pe_k, P(p["patch_w"]), ch.pe_k, P(p["patch_b"]), P(x), d, Lq, d, ch.pe_k, FC.EPI_RES,
                                               P(residual), d, None, 0, 1, self._lib.stream_ptr()), "mmpl_gemm")
        sinu = ops.new(nT, ch.freq_dim)
        ops.sinusoid(sinu, t, ch.freq_dim)
        t1 = ops.new(nT, d)
        ops.gemm("time0", t1, sinu, p["time0_w"], p["time0_b"], epi=FC.EPI_SILU)
        e = ops.new(nT, d)
        ops.gemm("time2", e, t1, p["time2_w"], p["time2_b"])
        emod_head = ops.new(nT, 2 * d)
        ops.modulation(emod_head, p["head_mod"], e, 1, 1, nT, 2, d)
        xh = ops.new(Lq, d)
        ops.layernorm(xh, x, ch.eps, scale=emod_head[:, d:], shift=emod_head[:, :d], rpf=S if nT == nF else Lq)
        yh = ops.new(Lq, 64)
        ops.gemm("head", yh, xh, p["head_w"], p["head_b"])
        out = ops.new(nF, 16 * LAT[0] * LAT[1])
        ops.unpatchify(out, yh, 16, LAT[0], LAT[1])
        assert ops.canaries_intact()
        return out.view(nF, 16, LAT[0], LAT[1]), x


def host_residual(x_last, x_embed):
    """bf16(float(x_L) - float(x_0)) on the host: one fp32 subtraction, one rounding."""
    return (x_last.cpu().float() - x_embed.cpu().float()).to(BF)


def small_int_residual(n, d):
    from mmpl_amd.synthetic import philox_normal
    return (philox_normal([n, d], 17, torch.float32) * 3).round().clamp_(-8, 8).to(BF).to(DEV)


@pytest.fixture(scope="module")
def tiny():
    return Model()


@pytest.fixture(scope="module")
def tiny_i2v():
    return Model(i2v=True, seed=6)


def _inputs(m, nF, seed, tval=700.0, C_=None):
    from mmpl_amd.synthetic import philox_normal
    x = philox_normal([nF, m.in_dim if C_ is None else C_, LAT[0], LAT[1]], seed).to(DEV)
    return x, torch.full([nF], tval, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ the cached stage forward
@pytest.mark.parametrize("nF", [1, 3])
def test_stage_forward_off_record_reuse(tiny, nF):
    m = tiny
    frames = list(range(4, 4 + nF))
    vis = [0, 1] + frames
    x, t = _inputs(m, nF, 20 + nF, 640.0)
    kc0, vc0 = m.caches(10)

    def uncached(**kw):
        kc, vc = kc0.clone(), vc0.clone()
        out = m.eng.forward(x, t, frames, frames, vis, kc, vc, m.ck, m.cv, cross_rows=m.rows, **kw)
        torch.cuda.synchronize()
        return out, kc, vc

    def cached(mode, res, **kw):
        kc, vc = kc0.clone(), vc0.clone()
        out = torch.full((nF, 16, *LAT), float("nan"), dtype=BF, device=DEV)
        assert m.at_cached(x, t, frames, frames, vis, kc, vc, out, mode, res, **kw) == 0, m.lib.mmpl_last_error()
        torch.cuda.synchronize()
        return out, kc, vc

    want = uncached()
    # OFF: the uncached entry, the residual ignored (NULL, or left as it was)
    assert all(same(a, b) for a, b in zip(cached(OFF, None), want))
    res = m.residual(nF)
    assert all(same(a, b) for a, b in zip(cached(OFF, res), want)) and bool(torch.isnan(res.float()).all())
    # RECORD: the same bits, and the residual of this very forward
    got = cached(RECORD, res)
    assert all(same(a, b) for a, b in zip(got, want))
    ch, ops = m.chain()
    kc, vc = kc0.clone(), vc0.clone()
    ch_out = ch.forward(x, t, frames, frames, vis, kc, vc, m.ck, m.cv, cross_rows=m.rows)
    trace = dict(ch.trace)
    assert same(ch_out, want[0])
    want_res = host_residual(trace[f"{m.L - 1}.x_ffn"], trace["x_embed"])
    n = nF * m.S * m.d
    assert same(res[:n].cpu().view(nF * m.S, m.d), want_res) and bool((want_res.float() != 0).any())
    # ... with share_out / share_in too
    sh_want = torch.empty(n, dtype=BF, device=DEV)
    sh_got = torch.empty(n, dtype=BF, device=DEV)
    prod_want = uncached(share_out=sh_want)
    res2 = m.residual(nF)
    prod_got = cached(RECORD, res2, share_out=sh_got)
    assert all(same(a, b) for a, b in zip(prod_got, prod_want)) and same(sh_got, sh_want) and same(res2, res)
    cons_want = uncached(share_in=sh_want)
    res3 = m.residual(nF)
    cons_got = cached(RECORD, res3, share_in=sh_got)
    assert all(same(a, b) for a, b in zip(cons_got, cons_want)) and same(res3, res)
    # REUSE: the public launches, for a zero residual, a small-integer one and the one RECORD left
    for name, r in (("zero", m.residual(nF, 0.0)), ("small integers", small_int_residual(nF * m.S, m.d).reshape(-1)), ("recorded", res)):
        rr = m.residual(nF, 0.0)
        rr[:n].copy_(r[:n])
        m.stats.zero_()
        out, kc, vc = cached(REUSE, rr, ck=None, cv=None)                       # cross K / V may be NULL
        want_out, x_reuse = m.reuse_chain(x, t, rr[:n].view(nF * m.S, m.d))
        assert same(out, want_out), name
        assert int(m.stats[0]) == 0, "a REUSE forward ran a self-attention block"
        assert same(kc, kc0) and same(vc, vc0), "a REUSE forward wrote K / V"      # the write slots of every layer included
        assert bool(torch.isfinite(out.float()).all())
        if name == "zero":
            assert same(x_reuse, trace["x_embed"])                               # + 0: the patch embedding itself
    m.stats.zero_()
    cached(RECORD, m.residual(nF))
    assert int(m.stats[0]) > 0                                                   # (the counter does move when a block runs)


def test_rejections(tiny):
    m = tiny
    x, t = _inputs(m, 1, 30)
    kc, vc = m.caches(12)
    res = m.residual(1)
    sentinel = torch.full((1, 16, *LAT), 123.0, dtype=BF, device=DEV)
    seen = set()

    def rejected(rc, text):
        msg = m.lib.mmpl_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and text in msg, (rc, msg)
        assert bool((sentinel == 123.0).all())
        seen.add(msg)

    for mode in (-1, 3):
        rejected(m.at_cached(x, t, [0], [0], [0], kc, vc, sentinel, mode, res), "cache_mode outside 0 .. 2")
    for mode in (RECORD, REUSE):
        rejected(m.at_cached(x, t, [0], [0], [0], kc, vc, sentinel, mode, None), "needs a residual buffer")
        rejected(m.at_cached(x, t, [0], [0], [0], kc, vc, sentinel, mode, res[64:]), "256-byte aligned")
    rejected(m.at_cached(x, t, [0], [99], [0], kc, vc, sentinel, REUSE, res), "write slot out of range")     # validated, nothing persisted
    # the whole-clip entry: the same three, and a missing cross K / V where blocks run
    ws = m.eng.full_workspace(1)

    def full(mode, residual, ck=m.ck):
        with torch.cuda.device(DEV):
            return m.lib.mmpl_dit_forward_full_cached(m.eng._h, P(x), P(t), 1, P(ck), P(m.cv), m.rows, None, None, None, P(sentinel), P(ws),
                                                      ws.numel(), m._lib.stream_ptr(), None, mode, P(residual))

    rejected(full(7, res), "cache_mode outside 0 .. 2")
    rejected(full(RECORD, None), "needs a residual buffer")
    rejected(full(REUSE, res[8:]), "256-byte aligned")
    rejected(full(RECORD, res, ck=None), "null argument")
    assert len(seen) >= 5


# ------------------------------------------------------------------------------------------------ the cached whole-clip forward
@pytest.mark.parametrize("kind", ["t2v", "i2v"])
def test_whole_clip_forward_off_record_reuse(kind, tiny, tiny_i2v):
    from mmpl_amd.synthetic import philox_normal
    m = tiny if kind == "t2v" else tiny_i2v
    nF = 2
    x, _ = _inputs(m, nF, 40, C_=16)
    y = philox_normal([nF, 20, *LAT], 41).to(DEV) if kind == "i2v" else None
    t1 = torch.full([1], 433.0, dtype=torch.float32, device=DEV)
    kw = dict(cross_rows=m.rows, y=y)
    want = m.eng.forward_full(x, t1, m.ck, m.cv, **kw)
    ws = m.eng.full_workspace(nF)

    def raw(mode, residual):                               # OFF through the cached entry itself
        out = torch.full_like(want, float("nan"))
        with torch.cuda.device(DEV):
            rc = m.lib.mmpl_dit_forward_full_cached(m.eng._h, P(x), P(t1), nF, P(m.ck), P(m.cv), m.rows, None, None, None, P(out), P(ws), ws.numel(),
                                                    m._lib.stream_ptr(), P(y), mode, P(residual))
        assert rc == 0, m.lib.mmpl_last_error()
        return out

    assert same(raw(OFF, None), want)
    res = m.residual(nF)
    assert same(m.eng.forward_full(x, t1, m.ck, m.cv, cache_mode=RECORD, residual=res, **kw), want)
    share = torch.empty(nF * m.S * m.d, dtype=BF, device=DEV)
    res_p, res_c = m.residual(nF), m.residual(nF)
    assert same(m.eng.forward_full(x, t1, m.ck, m.cv, cache_mode=RECORD, residual=res_p, share_out=share, **kw), want)
    assert same(m.eng.forward_full(x, t1, m.ck, m.cv, cache_mode=RECORD, residual=res_c, share_in=share, **kw), want)
    assert same(res_p, res) and same(res_c, res)
    # the chain: the whole clip is the stage forward on a zeroed cache with frame i in slot i (include/mmpl_hip.h)
    ch, ops = m.chain()
    kc, vc = m.eng.new_kv_cache(15)
    x_cat = x if y is None else torch.cat([x, y], dim=1).contiguous()
    tN = t1.expand(nF).contiguous()
    img = (None, None) if m.img is None else m.img
    ch_out = ch.forward(x_cat, tN, list(range(nF)), list(range(nF)), list(range(nF)), kc, vc, m.ck, m.cv, cross_rows=m.rows,
                        img_k=img[0], img_v=img[1])
    trace = dict(ch.trace)
    assert same(ch_out, want)
    n = nF * m.S * m.d
    assert same(res[:n].cpu().view(nF * m.S, m.d), host_residual(trace[f"{m.L - 1}.x_ffn"], trace["x_embed"]))
    for name, r in (("zero", m.residual(nF, 0.0)), ("small integers", small_int_residual(nF * m.S, m.d).reshape(-1)), ("recorded", res)):
        rr = m.residual(nF, 0.0)
        rr[:n].copy_(r[:n])
        m.stats.zero_()
        out = m.eng.forward_full(x, t1, None, None, cache_mode=REUSE, residual=rr, y=y)
        want_out, _ = m.reuse_chain(x_cat, t1, rr[:n].view(nF * m.S, m.d))
        assert same(out, want_out), name
        assert int(m.stats[0]) == 0


# ------------------------------------------------------------------------------------------------ the indicator
@pytest.mark.parametrize("rows", [2, 4])
@pytest.mark.parametrize("d", [8, 264, 1536, 6 * 1536])
def test_rel_l1_rows(tiny, rows, d):
    from mmpl_amd.synthetic import philox_normal
    eng = tiny.eng
    ld = d + 8                                             # a row stride of its own; the gap holds NaN
    # small integers: every |difference| and every sum is an integer below 2^24, exact in float32 in any order
    xi = (philox_normal([rows, d], 50 + rows, torch.float32) * 3).round().clamp_(-8, 8)
    xi[:, 0] = 1.0                                         # (no zero row)
    buf = torch.full((rows, ld), float("nan"), dtype=BF, device=DEV)
    buf[:, :d] = xi.to(BF).to(DEV)
    got = eng.rel_l1_rows(buf[:, :d]).cpu().numpy()
    a = xi.numpy().astype(np.float64)
    for i in range(rows - 1):
        num, den = np.abs(a[i + 1] - a[i]).sum(), np.abs(a[i]).sum()
        assert num < 2 ** 24 and den < 2 ** 24
        assert got[i].view(np.uint32) == (np.float32(num) / np.float32(den)).view(np.uint32), (i, got[i], num, den)
    # normal data: the worst case of two d-term float32 sums of non-negative terms and one division
    xn = philox_normal([rows, d], 60 + rows).to(BF)
    buf[:, :d] = xn.to(DEV)
    got = eng.rel_l1_rows(buf[:, :d]).cpu().numpy().astype(np.float64)
    again = eng.rel_l1_rows(buf[:, :d]).cpu().numpy().astype(np.float64)
    a = xn.double().numpy()
    want = np.abs(a[1:] - a[:-1]).sum(axis=1) / np.abs(a[:-1]).sum(axis=1)
    err = np.abs(got - want) / want
    print(f"[rel_l1_rows] rows {rows} d {d}: max relative error {err.max():.3e}, bound {2 * (d + 1) * 2.0 ** -24:.3e}")
    assert np.array_equal(got, again)
    assert (err <= 2 * (d + 1) * 2.0 ** -24).all(), (err, want)


def test_rel_l1_rows_rejections(tiny):
    lib, x, out = tiny.lib, torch.zeros(4, 16, dtype=BF, device=DEV), torch.full((3,), 5.0, device=DEV)
    S = tiny._lib.stream_ptr()
    for args, text in (((None, 16, 4, 16, P(out), S), "null argument"), ((P(x), 16, 4, 16, None, S), "null argument"),
                       ((P(x), 16, 1, 16, P(out), S), "rows < 2"), ((P(x), 16, 4, 0, P(out), S), "non-positive size"),
                       ((P(x), 8, 4, 16, P(out), S), "ld < d")):
        assert lib.mmpl_rel_l1_rows(*args) != 0 and text in lib.mmpl_last_error().decode(), text
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def test_time_embed_rows_are_the_forwards(tiny):
    m = tiny
    ts = torch.tensor([999.0, 640.25, 3.0], dtype=torch.float32, device=DEV)
    e3, e03 = m.eng.time_embed(ts)
    e_only, none = m.eng.time_embed(ts, want_e0=False)
    assert none is None and same(e_only, e3)
    x, _ = _inputs(m, 1, 70)
    for i in range(3):
        e1, e01 = m.eng.time_embed(ts[i:i + 1].contiguous())
        assert same(e1[0], e3[i]) and same(e01[0], e03[i]), i
        ch, ops = m.chain()
        kc, vc = m.eng.new_kv_cache(15)
        ch.forward(x, ts[i:i + 1].contiguous(), [0], [0], [0], kc, vc, m.ck, m.cv, cross_rows=m.rows)
        trace = dict(ch.trace)
        assert same(trace["e"][0], e3[i]) and same(trace["e0"][0], e03[i]), i
    assert not same(e3[0], e3[1])
    rel = m.eng.rel_l1_rows(e3).cpu()
    assert rel.shape == (2,) and bool((rel > 0).all()) and bool(torch.isfinite(rel).all())


# ------------------------------------------------------------------------------------------------ the whole-clip pipeline
class _Text(torch.nn.Module):
    def __init__(self, **ctx):
        super().__init__()
        self.ctx = ctx

    def forward(self, text_prompts):
        return {"prompt_embeds": self.ctx[text_prompts[0]]}


class _NoVAE:
    def decode_to_pixel(self, latent, use_cache=False):
        return torch.zeros(1, 1, 3, 8, 8, device=latent.device)


def _context(cfg, seed, n_valid):
    from mmpl_amd.synthetic import philox_normal
    c = philox_normal([1, 512, cfg["text_dim"]], seed)
    c[:, n_valid:] = 0
    return c.to(BF).to(DEV)


N_STEPS, F_CLIP = 6, 3
_PARTS = {}


def _clip_parts(kind):
    """(generator, text encoder) per model type, shared by the pipelines of this module (weights are read-only)."""
    if kind not in _PARTS:
        from mmpl_amd.geometry import Geometry
        from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict
        from mmpl_amd.wan_wrapper import WanDiffusionWrapper
        i2v = kind == "i2v"
        cfg = dict(WAN_CONFIGS["tiny"], model_type="i2v") if i2v else WAN_CONFIGS["tiny"]
        gen = WanDiffusionWrapper(is_causal=False, timestep_shift=5.0, model_config=cfg, geometry=Geometry(*LAT), device=DEV)
        gen.load_state_dict((dit_i2v_state_dict if i2v else dit_state_dict)(cfg, seed=5))
        _PARTS[kind] = (gen, _Text(p=_context(cfg, 31, 40), NEG=_context(cfg, 32, 12)))
    return _PARTS[kind]


def _clip_pipeline(kind, dtype, policy, use_graphs=True):
    from mmpl_amd.pipeline import BidirectionalDiffusionInferencePipeline
    gen, text = _clip_parts(kind)
    args = types.SimpleNamespace(num_train_timestep=1000, guidance_scale=5.0, negative_prompt="NEG")
    p = BidirectionalDiffusionInferencePipeline(args, DEV, generator=gen, text_encoder=text, vae=_NoVAE())
    p.sampling_steps, p.sample_solver, p.shift, p.latent_dtype, p.use_graphs, p.step_cache = N_STEPS, "unipc", 5.0, dtype, use_graphs, policy
    return p


@pytest.mark.parametrize("kind,dtype", [("t2v", BF), ("t2v", torch.float32), ("i2v", BF)], ids=["t2v-bf16", "t2v-fp32", "i2v-bf16"])
def test_whole_clip_pipeline(kind, dtype):
    from mmpl_amd.step_cache import StepCachePolicy
    from mmpl_amd.synthetic import philox_normal
    noise = philox_normal([1, F_CLIP, 16, *LAT], 33, torch.float32).to(dtype).to(DEV)
    kw = {}
    if kind == "i2v":
        kw["image_condition"] = {"clip_fea": philox_normal([257, 1280], 34).to(BF).to(DEV), "y": philox_normal([20, F_CLIP, *LAT], 35).to(BF).to(DEV)}

    def run(p):
        return p.sample(noise, ["p"], **kw)

    off = _clip_pipeline(kind, dtype, None)
    want = run(off)
    assert off.graph_captures == 1 and (off.computed_steps, off.skipped_steps) == (N_STEPS, 0)      # one step graph, as before
    assert all("residual" not in st and "schedule" not in st for st in off._steps.values())
    # thresh 0: every step computed, the same bits, graphs on and off
    for graphs in (True, False):
        p0 = _clip_pipeline(kind, dtype, StepCachePolicy(0.0), use_graphs=graphs)
        got = run(p0)
        assert torch.equal(got, want) and (p0.computed_steps, p0.skipped_steps) == (N_STEPS, 0)
        assert p0.graph_captures == (1 if graphs else 0)
    # a thresh above the sum of the distances: only the forced steps are computed
    for ret_steps, cutoff in ((1, None), (2, 4)):
        policy = StepCachePolicy(1e9, ret_steps=ret_steps, cutoff=cutoff)
        forced = ret_steps + (N_STEPS - (N_STEPS - 1 if cutoff is None else cutoff))
        pg = _clip_pipeline(kind, dtype, policy)
        lat = run(pg)
        assert (pg.computed_steps, pg.skipped_steps) == (forced, N_STEPS - forced)
        assert bool(torch.isfinite(lat.float()).all()) and not torch.equal(lat, want)
        assert pg.graph_captures == 2                      # a computed step's graph and a reused step's
        again = run(pg)
        assert pg.graph_captures == 2 and torch.equal(again, lat)               # the second call captures nothing
        pe = _clip_pipeline(kind, dtype, policy, use_graphs=False)
        assert torch.equal(run(pe), lat) and pe.graph_captures == 0             # eager == graph
    # the policy's own schedule on this model: between the two extremes, the last step computed
    (st,) = [s for s in pg._steps.values()]
    rel = pg.generator.engine.rel_l1_rows(pg.generator.engine.time_embed(st["sched"]._t_table)[0]).cpu()
    mid = _clip_pipeline(kind, dtype, StepCachePolicy(float(rel.max()) * 1.5))
    lat = run(mid)
    assert mid.skipped_steps >= 1 and mid.computed_steps >= 2 and bool(torch.isfinite(lat.float()).all())


def test_generate_with_teacache_thresh_zero_is_generate():
    from mmpl_amd.generate import WanT2V
    from mmpl_amd.synthetic import philox_normal
    gen, text = _clip_parts("t2v")
    wan = WanT2V(dict(num_train_timesteps=1000, sample_neg_prompt="NEG"), "", generator=gen, text_encoder=text, vae=_NoVAE(), device=DEV)
    noise = philox_normal([16, F_CLIP, *LAT], 36, torch.float32)
    call = lambda **kw: wan.generate("p", size=(LAT[1] * 8, LAT[0] * 8), frame_num=4 * (F_CLIP - 1) + 1, shift=5.0, sampling_steps=N_STEPS,
                                     seed=1, offload_model=False, noise=noise, return_latents=True, **kw)[1]
    want = call()
    assert torch.equal(call(teacache_thresh=0.0), want) and wan.pipeline.graph_captures == 1
    skipping = call(teacache_thresh=1e9, use_ret_steps=True)               # ret_steps 5, cutoff n: step 6 alone reuses
    assert (wan.pipeline.computed_steps, wan.pipeline.skipped_steps) == (5, 1) and wan.pipeline.step_cache.indicator == "e0"
    assert bool(torch.isfinite(skipping).all()) and not torch.equal(skipping, want)
    assert torch.equal(call(), want) and wan.pipeline.step_cache is None


# ------------------------------------------------------------------------------------------------ the FPS pipeline
def _fps_pipeline(steps=4):
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalFPSInferencePipeline
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    from mmpl_amd.wan_wrapper import WanFPSWrapper, WanTextEncoder
    cfg, geo = WAN_CONFIGS["tiny"], Geometry(*LAT)
    gen = WanFPSWrapper(is_causal=True, timestep_shift=5.0, model_config=cfg, geometry=geo, device=DEV)
    gen.load_state_dict({"model." + k: v for k, v in dit_state_dict(cfg, seed=2).items()})
    ctx = {"NEG": _context(cfg, 22, 12), "p": _context(cfg, 21, 40)}
    enc = WanTextEncoder(lambda prompts: ctx[prompts[0]])
    args = types.SimpleNamespace(model_kwargs={}, num_train_timestep=1000, timestep_shift=5.0, guidance_scale=5.0, negative_prompt="NEG",
                                 independent_first_frame=False, sampling_steps=steps)
    pipe = CausalFPSInferencePipeline(args, DEV, generator=gen, text_encoder=enc, vae=types.SimpleNamespace(), save=None, mode="t2v", geometry=geo)
    pipe.renoise_override = {f: philox_normal([1, 16, *LAT], 100 + f).to(DEV) for f in (4, 9, 13, 18)}
    return pipe


def test_fps_pipeline():
    from mmpl_amd.step_cache import StepCachePolicy
    from mmpl_amd.synthetic import philox_normal
    noise = philox_normal([1, 21, 16, *LAT], 23).to(BF).to(DEV)
    pipe = _fps_pipeline()
    run = lambda: pipe.inference(noise, ["p"], return_latents=True, decode=False)[1]
    want = run()
    n_stages = len(pipe.plan.stages)
    assert (pipe.computed_steps, pipe.skipped_steps) == (4 * n_stages, 0)
    for step_graphs, use_graphs in ((True, True), (False, True), (False, False)):      # the step graph, forward graphs, eager
        pipe.step_graphs, pipe.use_graphs = step_graphs, use_graphs
        pipe.step_cache = None
        assert torch.equal(run(), want)
        pipe.step_cache = StepCachePolicy(0.0)
        assert torch.equal(run(), want), (step_graphs, use_graphs)
        assert (pipe.computed_steps, pipe.skipped_steps) == (4 * n_stages, 0)
    # a skipping policy on a fresh pipeline (zeroed caches): steps 2 and 3 of every stage reuse step 1's residual
    outs = []
    for step_graphs, use_graphs in ((True, True), (False, True), (False, False)):
        p = _fps_pipeline()
        p.step_graphs, p.use_graphs, p.step_cache = step_graphs, use_graphs, StepCachePolicy(1e9)
        lat = p.inference(noise, ["p"], return_latents=True, decode=False)[1]
        assert (p.computed_steps, p.skipped_steps) == (2 * n_stages, 2 * n_stages)
        assert bool(torch.isfinite(lat.float()).all()) and not torch.equal(lat, want)
        S = p.frame_seq_length
        for frames in p.plan.stages:                       # every persisting stage's slots hold K / V after its t = 0 refresh
            for slot in (s for s in p.plan.write_slots(frames) if s >= 0):
                for kv in (p.kv_cache_pos, p.kv_cache_neg):
                    for l in (0, p.num_transformer_blocks - 1):
                        assert bool((kv.k_all[l, slot * S:(slot + 1) * S] != 0).any()) and bool((kv.v_all[l, slot * S:(slot + 1) * S] != 0).any())
        outs.append(lat)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    pair_pipe = _fps_pipeline()
    pair_pipe.step_cache, pair_pipe.cfg_pair = StepCachePolicy(0.1), types.SimpleNamespace(role=0)
    with pytest.raises(ValueError, match="single-process"):
        pair_pipe.inference(noise, ["p"], decode=False)
