"""GPU tests of the whole-clip (bidirectional) DiT forward, C ABI mmpl_dit_forward_full behind DitEngine.forward_full (-m gpu):
bit for bit against mmpl_dit_forward where that can run (up to 7 frames), against the CPU oracle and the reference's own
WanModel(model_type="t2v") output past that, and its destinations, workspace bound, reproducibility and argument errors.
Tiny / small synthetic configs at 16 x 24 latents: S = 96 rows per frame, not a multiple of the 64-row wave tile."""
import os

import pytest
import torch

from tests.test_dit_forward_gpu import TOL
from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAT = (16, 24)
BF = torch.bfloat16


def _engine(cfg_name="tiny", weight_seed=3, load=True):
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    cfg = WAN_CONFIGS[cfg_name]
    eng = DitEngine(cfg, LAT[0], LAT[1], DEV)
    sd = dit_state_dict(cfg, seed=weight_seed)
    if load:
        eng.load_state_dict(sd)
    return eng, cfg, sd


def _inputs(cfg, n, x_seed=11, ctx_seed=4, n_valid=40):
    from mmpl_amd.synthetic import philox_normal
    x = philox_normal([n, 16, LAT[0], LAT[1]], x_seed).to(BF)
    ctx = philox_normal([n_valid, cfg["text_dim"]], ctx_seed).to(BF)
    return x, ctx


def _t(v):
    return torch.full([1], float(v), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("cfg_name", ["tiny", "small"])
@pytest.mark.parametrize("n", [3, 7])
def test_full_forward_equals_the_cached_forward_bit_for_bit(cfg_name, n):
    """mmpl_dit_forward_full == mmpl_dit_forward on a zeroed cache with frame_ids = write_slots = visible_slots = range(n) and the
    same t in every frame, stateless attention: same kernels on the same values (the one-row timestep embedding read through a
    frame stride of 0 included)."""
    eng, cfg, _ = _engine(cfg_name, weight_seed=8)
    x, ctx = _inputs(cfg, n)
    kv = eng.precompute_context(ctx.to(DEV))
    kc, vc = eng.new_kv_cache(n)
    ident = list(range(n))
    ref = eng.forward(x.to(DEV), torch.full([n], 640.0, device=DEV), ident, ident, ident, kc, vc, kv[0], kv[1], cross_rows=kv.rows)
    out = eng.forward_full(x.to(DEV), _t(640.0), kv[0], kv[1], cross_rows=kv.rows)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ref)


@pytest.fixture(scope="module")
def fixture_forward():
    """The reference-made forward fixture, the HIP forward on its inputs and the oracle's identity-slot forward: computed once."""
    from mmpl_amd.synthetic import WAN_CONFIGS, philox_normal
    fx = torch.load(os.path.join(GOLDEN, "bidir_forward_tiny.pt"))
    m = fx["meta"]
    cfg = WAN_CONFIGS[m["cfg"]]
    eng, _, sd = _engine(m["cfg"], weight_seed=m["weight_seed"])
    F_ = m["F"]
    x = philox_normal([16, F_, LAT[0], LAT[1]], m["x_seed"]).to(BF)               # [C, F, h, w], the reference's layout
    ctx = philox_normal([m["n_valid"], cfg["text_dim"]], m["ctx_seed"]).to(BF)
    kv = eng.precompute_context(ctx.to(DEV))
    out = eng.forward_full(x.permute(1, 0, 2, 3).contiguous().to(DEV), _t(m["t"]), kv[0], kv[1], cross_rows=kv.rows).cpu()
    return fx, out.permute(1, 0, 2, 3)


def test_past_the_old_limit_vs_reference_fixture(fixture_forward):
    fx, out = fixture_forward
    e = rel_l2(out, fx["out"])
    print(f"[bidir] 21 frames: rel_l2(HIP, reference WanModel) = {e:.3e} (the reference's own K/V order noise {fx['order_out']:.3e})")
    assert torch.isfinite(out.float()).all()
    assert e < TOL


@pytest.mark.parametrize("n", [9, 21])
def test_past_the_old_limit_vs_oracle(n):
    from oracle import wan_dit_ref as W
    eng, cfg, sd = _engine("tiny", weight_seed=3)
    x, ctx = _inputs(cfg, n, x_seed=20 + n)
    kv = eng.precompute_context(ctx.to(DEV))
    out = eng.forward_full(x.to(DEV), _t(500.0), kv[0], kv[1], cross_rows=kv.rows).cpu()
    ocfg = W.DitCfg(**cfg)
    ident = list(range(n))
    ref = W.dit_forward(sd, ocfg, x.permute(1, 0, 2, 3), torch.full([1, n], 500.0), ctx, W.new_kv_cache(ocfg, n, eng.S),
                        [None] * ocfg.num_layers, ident, ident, ident).permute(1, 0, 2, 3)
    e = rel_l2(out, ref)
    print(f"[bidir] {n} frames: rel_l2(HIP, oracle identity slots) = {e:.3e}")
    assert torch.isfinite(out.float()).all()
    assert e < TOL


@pytest.mark.parametrize("cfg_name", ["tiny", "small"])
def test_rows_past_frame_8_equal_the_cached_forward_on_explicit_indices(cfg_name):
    """Row-exactness across the old limit of 8 frames.  mmpl_dit_forward cannot RUN 21 frames, but it can ATTEND to 21 cache slots:
    run it over the clip in chunks of 8 frames (8, 8, 5) with explicit frame_ids = write_slots = the frames' absolute indices and
    visible_slots = range(21), num_layers + 1 rounds over all chunks.  After round r the cache's layers 0 .. r-1 hold every frame's
    K / V as the whole-clip forward computes them (layer l's K / V of a frame depend on the layers before, whose attention by then
    saw the correct K / V of all 21 frames), so the last round's outputs are the whole-clip forward's -- computed with every frame
    >= 8 rotated and written through an index the caller spelled out, in arrays of at most 8 entries.  mmpl_dit_forward_full must
    give the same bits.  Why this catches a frame >= 8 rotated at, or written to, another frame's position: that frame's K rows
    (or the page they land in) change, through the self-attention every output row changes, and the comparison is exact.  (The
    clip has one timestep, so gating has no per-frame index to get wrong: every frame reads the same modulation row; the 3- and
    7-frame identities above pin that row against the per-frame computation.)
    The chunk is 8 frames because 8 * S = 768 rows is a multiple of the self-attention's 256-row query block: the chunks' query
    blocks are then the whole clip's, and each row sees the same KV tiles in the same order.  With chunks of 7 frames (672 rows) the
    blocks straddle differently and the outputs differ by bf16 rounding (max |d| 2^-7 on the device), which says nothing about
    indices."""
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict
    n, chunk = 21, 8
    cfg = WAN_CONFIGS[cfg_name]
    eng = DitEngine(cfg, LAT[0], LAT[1], DEV, max_frames=chunk)
    eng.load_state_dict(dit_state_dict(cfg, seed=5))
    assert (chunk * eng.S) % 256 == 0
    x, ctx = _inputs(cfg, n, x_seed=31)
    kv = eng.precompute_context(ctx.to(DEV))
    xd = x.to(DEV)
    full = eng.forward_full(xd, _t(750.0), kv[0], kv[1], cross_rows=kv.rows)
    kc, vc = eng.new_kv_cache(n)
    ref = torch.empty_like(full)
    for _ in range(cfg["num_layers"] + 1):
        for c0 in range(0, n, chunk):
            ids = list(range(c0, min(c0 + chunk, n)))
            eng.forward(xd[c0:c0 + len(ids)].contiguous(), torch.full([len(ids)], 750.0, device=DEV), ids, ids, list(range(n)), kc, vc,
                        kv[0], kv[1], cross_rows=kv.rows, out=ref[c0:c0 + len(ids)])
    torch.cuda.synchronize()
    assert torch.isfinite(full.float()).all()
    assert torch.equal(full, ref)


def test_destinations_and_workspace_bound():
    """`out` is overwritten completely and nothing is written behind mmpl_dit_full_workspace_bytes."""
    n, guard = 9, 1 << 16
    eng, cfg, _ = _engine("tiny")
    x, ctx = _inputs(cfg, n)
    kv = eng.precompute_context(ctx.to(DEV))
    need = eng._lib.mmpl_dit_full_workspace_bytes(eng._h, n)
    assert need > 0 and need % 256 == 0
    ws = torch.full([need + guard], 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full([n, 16, LAT[0], LAT[1]], float("nan"), dtype=BF, device=DEV)      # the sentinel: no forward leaves a NaN
    plain = eng.forward_full(x.to(DEV), _t(300.0), kv[0], kv[1])
    eng.forward_full(x.to(DEV), _t(300.0), kv[0], kv[1], out=out, workspace=ws[:need])
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()                                  # every element was written
    assert torch.equal(out, plain)
    assert bool((ws[need:] == 0xA5).all())


def test_reproducible_eager_and_graph_and_shared_block0():
    n = 9
    eng, cfg, _ = _engine("tiny")
    x, ctx = _inputs(cfg, n)
    _, ctx2 = _inputs(cfg, n, ctx_seed=77, n_valid=13)
    kv, kv2 = eng.precompute_context(ctx.to(DEV)), eng.precompute_context(ctx2.to(DEV))
    xd, t = x.to(DEV), _t(820.0)
    a = eng.forward_full(xd, t, kv[0], kv[1])
    b = eng.forward_full(xd, t, kv[0], kv[1])
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_full(xd, t, kv[0], kv[1], out=out)
    replays = []
    for _ in range(2):
        out.zero_()
        g.replay()
        replays.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, replays[0]) and torch.equal(a, replays[1])
    # block 0's self-attention handed from a forward with ANOTHER context (share_out) to this one (share_in)
    share = eng.shared_block0_buffer(n)
    other = eng.forward_full(xd, t, kv2[0], kv2[1], share_out=share)
    shared = eng.forward_full(xd, t, kv[0], kv[1], share_in=share)
    torch.cuda.synchronize()
    assert torch.equal(shared, a)
    assert not torch.equal(other, a)                                          # the other context is another function
    assert torch.equal(other, eng.forward_full(xd, t, kv2[0], kv2[1]))        # and share_out changes nothing of its own result


def test_argument_errors_stop_on_the_host():
    """Every argument error of mmpl_dit_forward_full: non-zero and a message, on null or undersized arguments (nothing is launched)."""
    from mmpl_amd import _lib
    n = 3
    eng, cfg, _ = _engine("tiny")
    lib, h = eng._lib, eng._h
    need = lib.mmpl_dit_full_workspace_bytes(h, n)
    buf = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p, null = _lib.ptr(buf), None
    T = eng.text_len

    def call(hh=h, x=p, t=p, nf=n, ck=p, cv=p, so=null, si=null, out=p, ws=p, nbytes=need):
        rc = lib.mmpl_dit_forward_full(hh, x, t, nf, ck, cv, T, so, si, null, out, ws, nbytes, null)
        return rc, lib.mmpl_last_error().decode()

    for kw in (dict(x=null), dict(t=null), dict(ck=null), dict(cv=null), dict(out=null), dict(ws=null)):
        rc, msg = call(**kw)
        assert rc != 0 and "mmpl_dit_forward_full" in msg and "null" in msg, (kw, msg)
    rc, msg = call(hh=None)
    assert rc != 0 and "null" in msg
    for nf in (0, -1, 25):
        rc, msg = call(nf=nf)
        assert rc != 0 and "n_frames out of range" in msg, (nf, msg)
        assert lib.mmpl_dit_full_workspace_bytes(h, nf) == 0
    rc, msg = call(nbytes=need - 1)
    assert rc != 0 and "workspace too small" in msg
    rc, msg = call(so=p, si=p)
    assert rc != 0 and "exclusive" in msg
    unbound, _, _ = _engine("tiny", load=False)
    rc, msg = call(hh=unbound._h)
    assert rc != 0 and "weights not bound" in msg
    # the frame count is independent of cfg.max_frames (7 here), and the size grows with it
    assert lib.mmpl_dit_full_workspace_bytes(h, 24) > lib.mmpl_dit_full_workspace_bytes(h, 21) > lib.mmpl_dit_full_workspace_bytes(h, 8) > 0
    torch.cuda.synchronize()
