"""mmpl_dit_forward_groups (-m gpu): a batch of G samples x F frames in the launches of ONE forward over G * F frames, the
self-attention block-diagonal (grouped launch of attn_w64_kernel), each sample on slots of its own of the one cache.

Tiny config, latents 16 x 24 (S = 96), G x F in {2 x 3, 8 x 1, 1 x 3}:
  (a) every bit of the output and of the whole cache against the launch chain of tests/forward_chain.py at G * F frames, whose
      self-attention is made one launch per sample on that sample's rows and pages (and its text cross-attention likewise where the
      samples' contexts differ);
  (b) isolation: with sample 1's latents, cache contents and context replaced, sample 0's output and every byte of its slots are what
      they were, and slots nobody writes keep their fill;
  (c) against G calls of mmpl_dit_forward_at on per-sample caches: equal bits where the GEMM launcher's plan (mmpl_gemm_ex's plan_out:
      kernel, tail kind, epilogue, split-K parts) is the same at G * F * S and at F * S rows for every GEMM of the forward, else within
      the project's per-forward bound of 2e-2 rel-L2; the case that applied is printed;
  (d) G = 1 is mmpl_dit_forward_at: same sha256;
  (e) every rejection the header lists, before anything is launched.
"""
import ctypes as C
import hashlib

import pytest
import torch

from tests import forward_chain as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
W = 5                                  # slots of a sample's window
SHAPES = [(2, 3), (8, 1), (1, 3)]


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(bits(t).cpu().numpy().tobytes())
    return h.hexdigest()


class PerSampleAttention:
    """The chain's ops with every attention launch over all rows replaced by one launch per sample: the self-attention on the sample's
    rows and ITS pages (the chain is told sample 0's visible slots; the scratch pages of a non-persisting stage are each sample's own
    frames'), the text cross-attention on the sample's context where the contexts differ."""

    def __init__(self, ops, G, S, vis, k_cache, v_cache, cross):
        self.ops, self.G, self.S, self.vis, self.kc, self.vc, self.cross = ops, G, S, vis, k_cache, v_cache, cross
        self.one_context = all(c[0] is cross[0][0] for c in cross)
        self.n_self = self.n_cross = 0

    def __getattr__(self, name):
        return getattr(self.ops, name)

    def attention(self, out, q, k_pages, v_pages, H, scale, groups=None, cross=0, **kw):
        G, S = self.G, self.S
        Lg = q.shape[0] // G
        rows = lambda t, g: t[g * Lg:(g + 1) * Lg]
        if cross:
            l, self.n_cross = self.n_cross, self.n_cross + 1
            if self.one_context:
                return self.ops.attention(out, q, k_pages, v_pages, H, scale, groups=groups, cross=cross, **kw)
            n = k_pages[0].shape[0]
            for g in range(G):
                self.ops.attention(rows(out, g), rows(q, g), [self.cross[g][0][l][:n]], [self.cross[g][1][l][:n]], H, scale, cross=cross, **kw)
            return
        l, self.n_self = self.n_self, self.n_self + 1
        nv, Fg = len(self.vis[0]), Lg // S
        page = lambda cache, slot: cache[l, slot * S:(slot + 1) * S]
        for g in range(G):
            own = slice(nv + g * Fg, nv + (g + 1) * Fg) if len(k_pages) > nv else slice(0, 0)
            kp = [page(self.kc, s) for s in self.vis[g]] + k_pages[own]
            vp = [page(self.vc, s) for s in self.vis[g]] + v_pages[own]
            self.ops.attention(rows(out, g), rows(q, g), kp, vp, H, scale, groups=[0] * nv + [1] * (len(kp) - nv), **kw)


class Model:
    def __init__(self):
        from mmpl_amd import _lib
        from mmpl_amd.dit import DitEngine
        from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
        self.cfg, self.lat = dict(WAN_CONFIGS["tiny"]), (16, 24)
        self.sd = dit_state_dict(self.cfg, seed=3)
        self.eng = DitEngine(self.cfg, 16, 24, DEV, max_frames=8)
        self.eng.load_state_dict(self.sd)
        self.lib = _lib.load()
        self.L, self.S, self.d = self.eng.L, self.eng.S, self.eng.dim
        self.ctx = []
        for n_valid, seed in ((40, 4), (17, 5), (29, 6)):
            c = philox_normal([512, self.cfg["text_dim"]], seed)
            c[n_valid:] = 0
            self.ctx.append(self.eng.precompute_context(c.to(DEV)))
        torch.cuda.synchronize()

    def chain(self):
        ops = FC.HipOps(self.lib, self.eng, DEV)
        return FC.ForwardChain(self.sd, self.cfg, 16, 24, ops), ops

    def caches(self, G, seed):
        from mmpl_amd.synthetic import philox_normal
        kc, vc = self.eng.new_kv_cache(G * W)
        kc.copy_(philox_normal(list(kc.shape), seed).to(DEV))
        vc.copy_(philox_normal(list(vc.shape), seed + 1).to(DEV))
        return kc, vc

    def inputs(self, G, F, seed):
        from mmpl_amd.synthetic import philox_normal
        x = philox_normal([G * F, 16, 16, 24], seed).to(DEV)
        t = torch.tensor([[999.0, 750.0, 500.0, 250.0, 640.0, 433.0, 120.0, 0.0][g] for g in range(G) for _ in range(F)], dtype=torch.float32, device=DEV)
        return x, t

    def case(self, G, F, persist=True, one_context=False):
        """sample g: frames at positions 1 .. F (every sample its own RoPE positions would do as well), written to slots 1 .. F of its
        window, attending to its slot 0 and the written ones, listed out of order"""
        frames = [1 + i + (g % 2) for g in range(G) for i in range(F)]
        if persist:
            write = [g * W + 1 + i for g in range(G) for i in range(F)]
            vis = [[g * W + s for s in ([F, 0] + list(range(1, F)))] for g in range(G)]
        else:
            write = [-1] * (G * F)
            vis = [[g * W + s for s in (4, 0, 1)] for g in range(G)]
        cross = [self.ctx[0] if one_context else self.ctx[g % 2] for g in range(G)]
        rows = max(c.rows for c in cross)
        return frames, write, vis, cross, rows


@pytest.fixture(scope="module")
def m():
    return Model()


def _forward(m, G, x, t, frames, write, vis, kc, vc, cross, rows, poison=FC.CANARY):
    ws = m.eng.workspace(x.shape[0])
    ws.view(torch.int16).fill_(poison)
    out = m.eng.forward_groups(x, t, G, frames, write, vis, kc, vc, cross, cross_rows=rows)
    torch.cuda.synchronize()
    return out.clone()


@pytest.mark.parametrize("persist,one_context", [(True, False), (False, False), (True, True)], ids=["persist", "scratch", "one-context"])
@pytest.mark.parametrize("G,F", SHAPES)
def test_a_equals_the_chain_with_per_sample_attention(m, G, F, persist, one_context):
    frames, write, vis, cross, rows = m.case(G, F, persist, one_context)
    kc0, vc0 = m.caches(G, 10 * G + F)
    x, t = m.inputs(G, F, 20 + G)
    runs = []
    for poison in (FC.CANARY, 0x7F91):
        kc, vc = kc0.clone(), vc0.clone()
        runs.append((_forward(m, G, x, t, frames, write, vis, kc, vc, cross, rows, poison), kc, vc))
    ch, ops = m.chain()
    kc, vc = kc0.clone(), vc0.clone()
    ch.ops = PerSampleAttention(ops, G, m.S, vis, kc, vc, cross)
    want = ch.forward(x, t, frames, write, vis[0], kc, vc, cross[0][0], cross[0][1], cross_rows=rows)
    for out, kc_r, vc_r in runs:
        for name, a, b in (("out", out, want), ("k cache", kc_r, kc), ("v cache", vc_r, vc)):
            nd = int((bits(a) != bits(b)).sum())
            assert nd == 0, f"{nd} of {b.numel()} elements of {name} differ from the chain's"
    assert ops.canaries_intact() and not torch.isnan(want.float()).any() and bool((want != 0).any())
    assert same(kc, kc0) == (not persist)


def test_b_samples_are_isolated(m):
    G, F = 2, 3
    frames, write, vis, cross, rows = m.case(G, F)
    kc0, vc0 = m.caches(G, 30)
    x, t = m.inputs(G, F, 31)
    kc, vc = kc0.clone(), vc0.clone()
    out = _forward(m, G, x, t, frames, write, vis, kc, vc, cross, rows)
    # sample 1: other latents, other cache contents (its whole window), another context
    x2, _ = m.inputs(G, F, 32)
    x2[:F] = x[:F]
    kc2, vc2 = m.caches(G, 33)
    kc2[:, :W * m.S], vc2[:, :W * m.S] = kc0[:, :W * m.S], vc0[:, :W * m.S]
    cross2 = [cross[0], m.ctx[2]]
    fill_k, fill_v = kc2.clone(), vc2.clone()
    out2 = _forward(m, G, x2, t, frames, write, vis, kc2, vc2, cross2, max(rows, m.ctx[2].rows))
    assert same(out2[:F], out[:F]) and not same(out2[F:], out[F:])
    assert same(kc2[:, :W * m.S], kc[:, :W * m.S]) and same(vc2[:, :W * m.S], vc[:, :W * m.S])
    S = m.S
    for g in range(G):                                     # slots 0 and F + 1 .. W - 1 of every window: written by nobody
        for s in [0] + list(range(F + 1, W)):
            r = slice((g * W + s) * S, (g * W + s + 1) * S)
            assert same(kc2[:, r], fill_k[:, r]) and same(vc2[:, r], fill_v[:, r])
        r = slice((g * W + 1) * S, (g * W + F + 1) * S)
        assert not same(kc2[:, r], fill_k[:, r])


def _gemm_plans(m, n_frames, x, t, frames, write, vis, kc, vc, cross, rows):
    ch, ops = m.chain()
    ch.forward(x, t, frames, write, vis, kc.clone(), vc.clone(), cross[0], cross[1], cross_rows=rows)
    return {(n, tuple(p[i] for i in (0, 1, 2, 5))) for n, p in ops.plans if n not in ("self_attn", "cross_attn")}


@pytest.mark.parametrize("G,F", SHAPES)
def test_c_equals_one_forward_per_sample(m, G, F):
    frames, write, vis, cross, rows = m.case(G, F)
    kc0, vc0 = m.caches(G, 40 + G)
    x, t = m.inputs(G, F, 41 + G)
    kc, vc = kc0.clone(), vc0.clone()
    out = _forward(m, G, x, t, frames, write, vis, kc, vc, cross, rows)
    outs, kcs, vcs = [], [], []
    for g in range(G):
        win = slice(g * W * m.S, (g + 1) * W * m.S)
        kg, vg = kc0[:, win].contiguous(), vc0[:, win].contiguous()
        fr = slice(g * F, (g + 1) * F)
        o = m.eng.forward(x[fr].contiguous(), t[fr].contiguous(), frames[fr], [s - g * W for s in write[fr]], [s - g * W for s in vis[g]], kg, vg,
                          cross[g][0], cross[g][1], cross_rows=rows)
        torch.cuda.synchronize()
        outs.append(o.clone()); kcs.append(kg); vcs.append(vg)
    want, want_k, want_v = torch.cat(outs), torch.cat(kcs, dim=1), torch.cat(vcs, dim=1)
    # the plans of the GEMMs at both row counts (a chain run each, on this case's own arguments)
    both = _gemm_plans(m, G * F, x, t, frames, write, vis[0], kc0, vc0, cross[0], rows)
    one = _gemm_plans(m, F, x[:F].contiguous(), t[:F].contiguous(), frames[:F], write[:F], vis[0], kc0, vc0, cross[0], rows)
    rel = float((out.double() - want.double()).norm() / want.double().norm())
    if both == one:
        print(f"{G} x {F}: the GEMM plans agree at {G * F * m.S} and {F * m.S} rows -> bit equality required; rel-L2 {rel:.3e}")
        assert same(out, want) and same(kc, want_k) and same(vc, want_v)
    else:
        print(f"{G} x {F}: the GEMM plans differ ({sorted(both ^ one)}) -> rel-L2 {rel:.3e} against the bound 2e-2")
        assert rel <= 2e-2


def test_d_one_group_is_forward_at(m):
    G, F = 1, 3
    frames, write, vis, cross, rows = m.case(G, F)
    kc0, vc0 = m.caches(G, 50)
    x, t = m.inputs(G, F, 51)
    kc, vc = kc0.clone(), vc0.clone()
    out = _forward(m, G, x, t, frames, write, vis, kc, vc, cross, rows)
    kc1, vc1 = kc0.clone(), vc0.clone()
    m.eng.workspace(F).view(torch.int16).fill_(0x7F91)
    out1 = m.eng.forward(x, t, frames, write, vis[0], kc1, vc1, cross[0][0], cross[0][1], cross_rows=rows)
    torch.cuda.synchronize()
    assert sha(out, kc, vc) == sha(out1, kc1, vc1)


def _raw_call(m, **kw):
    from mmpl_amd import _lib
    G, F = 2, 3
    frames, write, vis, cross, rows = m.case(G, F)
    kc, vc = m.caches(G, 60)
    fill = kc.clone()
    x, t = m.inputs(G, F, 61)
    out = torch.full((G * F, 16, 16, 24), float("nan"), dtype=BF, device=DEV)
    ws = m.eng.workspace(8)
    ia = lambda v: (C.c_int * len(v))(*v)
    pa = lambda ts: (C.c_void_p * len(ts))(*[tt.data_ptr() for tt in ts])
    a = dict(h=m.eng._h, x=_lib.ptr(x), t=_lib.ptr(t), n_groups=G, frames_per_group=F, frame_ids=ia(frames), write_slots=ia(write),
             visible_slots=ia([s for v in vis for s in v]), n_visible=len(vis[0]), k_cache=_lib.ptr(kc), v_cache=_lib.ptr(vc), n_slots=G * W,
             cross_k=pa([c[0] for c in cross]), cross_v=pa([c[1] for c in cross]), cross_rows=rows, share_out=None, share_in=None,
             attn_history=None, out=_lib.ptr(out), workspace=_lib.ptr(ws), workspace_bytes=ws.numel(), frame_base=None)
    for k, v in kw.items():
        a[k] = ia(v) if isinstance(v, list) else v
    rc = m.lib.mmpl_dit_forward_groups(*a.values(), _lib.stream_ptr())
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(out.float()).all()) and same(kc, fill)
    return rc, m.lib.mmpl_last_error().decode(), untouched


def test_e_rejects(m):
    from mmpl_amd import _lib
    some = torch.zeros(16, dtype=torch.uint8, device=DEV)
    G, F = 2, 3
    _, write, vis, _, _ = m.case(G, F)
    flat = [s for v in vis for s in v]
    rejects = [
        (dict(n_groups=0), "n_groups < 1"),
        (dict(n_groups=3), "exceeds max_frames"),                             # 3 x 3 > 8
        (dict(share_out=_lib.ptr(some)), "share_out"), (dict(share_in=_lib.ptr(some)), "share_in"),
        (dict(attn_history=_lib.ptr(some)), "attn_history"),
        (dict(visible_slots=flat[:-1] + [G * W]), "visible slot out of range"), (dict(visible_slots=[-1] + flat[1:]), "visible slot out of range"),
        (dict(write_slots=write[:-1] + [G * W]), "write slot out of range"),
        (dict(write_slots=write[:F] + [write[0]] + write[F + 1:]), "two groups write the same slot"),
    ]
    for kw, msg in rejects:
        rc, text, untouched = _raw_call(m, **kw)
        assert rc != 0 and text.startswith("mmpl_dit_forward_groups:") and msg in text, (kw.keys(), rc, text)
        assert untouched, msg
    rc, text, untouched = _raw_call(m)
    assert rc == 0 and not untouched                                          # (the unmodified call is a valid one)


def test_e_rejects_an_i2v_handle():
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, philox_normal
    cfg = dict(WAN_CONFIGS["tiny"], model_type="i2v", in_dim=36)
    eng = DitEngine(cfg, 16, 24, DEV, max_frames=8)
    eng.load_state_dict(dit_i2v_state_dict(cfg, seed=6))
    img = philox_normal([eng.L, 257, eng.dim], 70).to(DEV)
    eng.set_image_kv(img, img.clone())
    c = philox_normal([512, cfg["text_dim"]], 4)
    c[30:] = 0
    kv = eng.precompute_context(c.to(DEV))
    kc, vc = eng.new_kv_cache(2 * W)
    x = philox_normal([2, 36, 16, 24], 71).to(DEV)
    t = torch.full([2], 500.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="i2v handle"):
        eng.forward_groups(x, t, 2, [0, 0], [0, W], [[0], [W]], kc, vc, [kv, kv], cross_rows=kv.rows)
