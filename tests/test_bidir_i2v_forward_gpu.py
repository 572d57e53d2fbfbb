"""GPU tests of the whole-clip forward of the Wan-I2V model type (-m gpu): the two-source patch embedding input (mmpl_patchify2) and
C ABI mmpl_dit_forward_full_i2v behind DitEngine.forward_full(y=...), bit for bit against mmpl_dit_forward_full on the 36-channel
concatenation and against mmpl_dit_forward with identity slots and the same image K / V, then against the reference's own
WanModel(model_type="i2v") output at 21 frames, and its argument errors.  Tiny synthetic config at 16 x 24 latents: S = 96 rows
per frame, not a multiple of the 64-row wave tile."""
import os

import numpy as np
import pytest
import torch

from tests.test_dit_forward_gpu import TOL
from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)
BF = torch.bfloat16


def _engine(weight_seed=8, clip_seed=6, attach=True, model_type="i2v"):
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_i2v_state_dict, dit_state_dict, philox_normal
    cfg = dict(WAN_CONFIGS["tiny"], model_type=model_type)
    eng = DitEngine(cfg, LAT[0], LAT[1], DEV)
    eng.load_state_dict((dit_i2v_state_dict if model_type == "i2v" else dit_state_dict)(cfg, seed=weight_seed))
    if attach and model_type == "i2v":
        eng.set_image_kv(*eng.precompute_image_context(philox_normal([257, 1280], clip_seed).to(BF).to(DEV)))
    return eng, cfg


def _inputs(cfg, n, x_seed=11, y_seed=12, ctx_seed=4, n_valid=40):
    from mmpl_amd.synthetic import philox_normal
    x = philox_normal([n, 16, LAT[0], LAT[1]], x_seed).to(BF).to(DEV)
    y = philox_normal([n, 20, LAT[0], LAT[1]], y_seed).to(BF).to(DEV)
    ctx = philox_normal([n_valid, cfg["text_dim"]], ctx_seed).to(BF).to(DEV)
    return x, y, ctx


def _t(v):
    return torch.full([1], float(v), dtype=torch.float32, device=DEV)


def _full_on_cat(eng, xy, t, kv, share_out=None, share_in=None):
    """mmpl_dit_forward_full on the i2v handle, given the 36-channel concatenation (DitEngine.forward_full no longer goes there)."""
    from mmpl_amd import _lib
    n = xy.shape[0]
    assert xy.is_contiguous() and xy.shape[1] == 36
    ws = eng.full_workspace(n)
    out = torch.empty(n, 16, LAT[0], LAT[1], dtype=BF, device=DEV)
    _lib.check(eng._lib.mmpl_dit_forward_full(eng._h, _lib.ptr(xy), _lib.ptr(t), n, _lib.ptr(kv[0]), _lib.ptr(kv[1]), kv.rows,
                                              _lib.ptr(share_out), _lib.ptr(share_in), None, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr()), "mmpl_dit_forward_full")
    return out


@pytest.mark.parametrize("F_, h, w", [(3, 4, 6), (1, 2, 2)])
def test_patchify2_equals_patchify_of_the_concatenation(F_, h, w):
    """mmpl_patchify2(x, y) == mmpl_patchify(cat([x, y])) bit for bit, Cx 16, Cy 20, lda 192: every row's columns 0 .. 143 and the
    zeroed padding columns 144 .. 191, which the poisoned (0xFFFF) buffers show to be written; the rows behind the last stay
    poisoned and the inputs untouched.  Random 16-bit patterns, NaNs included: the kernel moves bits."""
    from mmpl_amd import _lib
    lib = _lib.load()
    Cx, Cy, lda = 16, 20, 192
    rows, guard = F_ * (h // 2) * (w // 2), 2
    rng = np.random.default_rng(100 + F_)
    bits = lambda *s: torch.from_numpy(rng.integers(0, 1 << 16, size=s, dtype=np.uint16).view(np.int16)).to(DEV)
    x, y = bits(F_, Cx, h, w), bits(F_, Cy, h, w)
    xy = torch.cat([x, y], dim=1).contiguous()
    a1 = torch.full([rows + guard, lda], -1, dtype=torch.int16, device=DEV)       # 0xFFFF
    a2 = a1.clone()
    x0, y0 = x.clone(), y.clone()
    s = _lib.stream_ptr()
    _lib.check(lib.mmpl_patchify(_lib.ptr(xy), _lib.ptr(a1), lda, F_, Cx + Cy, h, w, s), "mmpl_patchify")
    _lib.check(lib.mmpl_patchify2(_lib.ptr(x), _lib.ptr(y), _lib.ptr(a2), lda, F_, Cx, Cy, h, w, s), "mmpl_patchify2")
    torch.cuda.synchronize()
    assert torch.equal(a2, a1)
    assert bool((a2[:rows, 4 * (Cx + Cy):] == 0).all()) and bool((a2[rows:] == -1).all())
    # the reference's layout, spelled out on the host: column c * 4 + ph * 2 + pw of token (f, gy, gx)
    want = xy.cpu().view(F_, Cx + Cy, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(rows, 4 * (Cx + Cy))
    assert torch.equal(a2[:rows, :4 * (Cx + Cy)].cpu(), want)
    assert torch.equal(x, x0) and torch.equal(y, y0)


@pytest.fixture(scope="module")
def engine():
    return _engine()


@pytest.mark.parametrize("n", [3, 9, 21])
def test_two_source_forward_equals_the_forward_on_the_concatenation(engine, n):
    """mmpl_dit_forward_full_i2v(x, y) == mmpl_dit_forward_full(cat([x, y])) on the same handle, bit for bit -- also with block 0's
    self-attention handed over (share_out, then share_in under another text context) against the unshared forward."""
    eng, cfg = engine
    x, y, ctx = _inputs(cfg, n, x_seed=20 + n)
    _, _, ctx2 = _inputs(cfg, n, ctx_seed=77, n_valid=13)
    kv, kv2 = eng.precompute_context(ctx), eng.precompute_context(ctx2)
    t = _t(640.0)
    ref = _full_on_cat(eng, torch.cat([x, y], dim=1).contiguous(), t, kv)
    out = eng.forward_full(x, t, kv[0], kv[1], cross_rows=kv.rows, y=y)
    share = eng.shared_block0_buffer(n)
    other = eng.forward_full(x, t, kv2[0], kv2[1], cross_rows=kv2.rows, y=y, share_out=share)
    shared = eng.forward_full(x, t, kv[0], kv[1], cross_rows=kv.rows, y=y, share_in=share)
    other_plain = eng.forward_full(x, t, kv2[0], kv2[1], cross_rows=kv2.rows, y=y)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref)
    assert torch.equal(shared, out) and torch.equal(other, other_plain) and not torch.equal(other, out)
    # y enters the result: another conditioning video is another function
    assert not torch.equal(eng.forward_full(x, t, kv[0], kv[1], cross_rows=kv.rows, y=y.flip(0).contiguous()), out)


@pytest.mark.parametrize("n", [3, 7])
def test_two_source_forward_equals_the_cached_forward_with_the_image_stream(engine, n):
    """The whole-clip identity with the image stream in the loop: == mmpl_dit_forward on a zeroed cache with frame_ids = write_slots =
    visible_slots = range(n), the same t in every frame and the same image K / V.  There the image cross-attention's output goes
    to workspace pages that never held K (the cache did); here it overwrites the layer's own K, dead by then -- a K page that was
    still needed would change the bits."""
    eng, cfg = engine
    x, y, ctx = _inputs(cfg, n, x_seed=30 + n)
    kv = eng.precompute_context(ctx)
    kc, vc = eng.new_kv_cache(n)
    ident = list(range(n))
    ref = eng.forward(torch.cat([x, y], dim=1).contiguous(), torch.full([n], 500.0, device=DEV), ident, ident, ident, kc, vc, kv[0], kv[1],
                      cross_rows=kv.rows)
    out = eng.forward_full(x, _t(500.0), kv[0], kv[1], cross_rows=kv.rows, y=y)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref)


def test_21_frames_vs_reference_fixture():
    """rel-L2 against the reference's WanModel(model_type='i2v') forward (tests/golden/make_golden_bidir_i2v.py) <= 2e-2, the
    project's per-forward bound.  Measured on an MI355X: 3.614e-03 (the fixture's order_out: 3.263e-03)."""
    from mmpl_amd.synthetic import WAN_CONFIGS, philox_normal
    fx = torch.load(os.path.join(GOLDEN, "bidir_i2v_forward_tiny.pt"))
    m = fx["meta"]
    cfg = WAN_CONFIGS[m["cfg"]]
    eng, _ = _engine(weight_seed=m["weight_seed"], clip_seed=m["clip_seed"])
    F_ = m["F"]
    x = philox_normal([16, F_, LAT[0], LAT[1]], m["x_seed"]).to(BF)                 # [C, F, h, w], the reference's layout
    y = philox_normal([20, F_, LAT[0], LAT[1]], m["y_seed"]).to(BF)
    ctx = philox_normal([m["n_valid"], cfg["text_dim"]], m["ctx_seed"]).to(BF)
    kv = eng.precompute_context(ctx.to(DEV))
    out = eng.forward_full(x.permute(1, 0, 2, 3).contiguous().to(DEV), _t(m["t"]), kv[0], kv[1], cross_rows=kv.rows,
                           y=y.permute(1, 0, 2, 3).contiguous().to(DEV)).cpu().permute(1, 0, 2, 3)
    e = rel_l2(out, fx["out"])
    print(f"[bidir i2v] 21 frames: rel_l2(HIP, reference WanModel i2v) = {e:.3e} (the reference's own K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(out.float()).all()
    assert e <= TOL


def test_image_kv_refreshed_in_place_is_what_a_captured_forward_reads():
    """precompute_image_context(out=) writes the attached pair in place: a graph captured before replays on the new image."""
    from mmpl_amd.synthetic import philox_normal
    eng, cfg = _engine(clip_seed=6)
    n = 3
    x, y, ctx = _inputs(cfg, n)
    kv = eng.precompute_context(ctx)
    t = _t(700.0)
    out = torch.empty(n, 16, LAT[0], LAT[1], dtype=BF, device=DEV)
    first = eng.forward_full(x, t, kv[0], kv[1], y=y).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_full(x, t, kv[0], kv[1], y=y, out=out)
    g.replay()
    assert torch.equal(out, first)
    pair = eng._img_kv
    ptrs = (pair[0].data_ptr(), pair[1].data_ptr())
    got = eng.precompute_image_context(philox_normal([257, 1280], 55).to(BF).to(DEV), out=pair)
    assert (got[0].data_ptr(), got[1].data_ptr()) == ptrs
    g.replay()
    torch.cuda.synchronize()
    fresh, _ = _engine(clip_seed=55)
    assert not torch.equal(out, first)
    assert torch.equal(out, fresh.forward_full(x, t, kv[0], kv[1], y=y))


def test_argument_errors_stop_on_the_host():
    """Every argument error of mmpl_dit_forward_full_i2v: non-zero and a message, nothing launched; and DitEngine's own."""
    from mmpl_amd import _lib
    n = 3
    eng, cfg = _engine()
    lib, h = eng._lib, eng._h
    need = lib.mmpl_dit_full_workspace_bytes(h, n)
    buf = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p, null = _lib.ptr(buf), None
    T = eng.text_len

    def call(hh=h, x=p, y=p, t=p, nf=n, ck=p, cv=p, so=null, si=null, out=p, ws=p, nbytes=need):
        rc = lib.mmpl_dit_forward_full_i2v(hh, x, y, t, nf, ck, cv, T, so, si, null, out, ws, nbytes, null)
        return rc, lib.mmpl_last_error().decode()

    for kw in (dict(x=null), dict(y=null), dict(t=null), dict(ck=null), dict(cv=null), dict(out=null), dict(ws=null)):
        rc, msg = call(**kw)
        assert rc != 0 and "mmpl_dit_forward_full_i2v" in msg and "null" in msg, (kw, msg)
    rc, msg = call(hh=None)
    assert rc != 0 and "null handle" in msg
    for nf in (0, -1, 25):
        rc, msg = call(nf=nf)
        assert rc != 0 and "n_frames out of range" in msg, (nf, msg)
    rc, msg = call(nbytes=need - 1)
    assert rc != 0 and "workspace too small" in msg
    rc, msg = call(so=p, si=p)
    assert rc != 0 and "exclusive" in msg
    bare, _ = _engine(attach=False)
    rc, msg = call(hh=bare._h)
    assert rc != 0 and "set_image_kv first" in msg
    t2v, _ = _engine(model_type="t2v", weight_seed=3)
    rc, msg = call(hh=t2v._h)
    assert rc != 0 and "in_dim must be 36" in msg
    torch.cuda.synchronize()
    # the engine: y is required by i2v and refused by t2v; image K / V first
    x, y, ctx = _inputs(cfg, n)
    kv = eng.precompute_context(ctx)
    with pytest.raises(ValueError, match="needs y"):
        eng.forward_full(x, _t(1.0), kv[0], kv[1])
    with pytest.raises(RuntimeError, match="set_image_kv"):
        bare.forward_full(x, _t(1.0), kv[0], kv[1], y=y)
    kv3 = t2v.precompute_context(ctx)
    with pytest.raises(ValueError, match="i2v model type"):
        t2v.forward_full(x, _t(1.0), kv3[0], kv3[1], y=y)
