"""The RoPE position base as device data (mmpl_qknorm_rope_at / mmpl_dit_forward_at, DitEngine.forward(frame_base=...)) on the
MI355X: relative frame ids plus a device int give the bits of absolute ids, the sum is clamped to the tables' last position, a NULL
base is the old entry point, and ONE captured forward is replayed at another position in time by rewriting the int."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"

# the shapes of tests/test_kernels_gpu.py::test_qknorm_rope_kvwrite that cover every path of qknorm_kernel: NIT 1 not FULL; 15 rows per
# frame and a row count that is no multiple of 4; NIT 10 FULL; several row groups per block
SHAPES = [(2, (8, 12), 3), (12, (6, 10), 3), (40, (4, 8), 3), (4, (70, 86), 5)]


class _Case:
    """One qkv matrix and its launch arguments; run(ids, base) -> (q, K pages, V pages) of a fresh launch on zeroed caches."""

    def __init__(self, H, lat, nF):
        from mmpl_amd.dit import DitEngine
        torch.manual_seed(H)
        self.d = d = H * 128
        self.eng = DitEngine(dict(dim=d, ffn_dim=256, num_heads=H, num_layers=1, text_dim=64), lat[0], lat[1], DEV)
        self.S, self.nF = (lat[0] // 2) * (lat[1] // 2), nF
        self.qkv = torch.randn(nF * self.S, 3 * d, device=DEV).to(BF)
        self.wq = (1 + 0.1 * torch.randn(d, device=DEV)).to(BF)
        self.wk = (1 + 0.1 * torch.randn(d, device=DEV)).to(BF)
        self.slots = [7, 3, 5, 4, 9][:nF]                   # not contiguous, not ascending: a wrapped ring write

    def run(self, lib, ids, base):
        from mmpl_amd import _lib
        d, S, nF = self.d, self.S, self.nF
        qkv = self.qkv.clone()
        kc = torch.zeros(12 * S, d, device=DEV, dtype=BF)
        vc = torch.zeros(12 * S, d, device=DEV, dtype=BF)
        kd = (C.c_void_p * nF)(*[kc[s * S:].data_ptr() for s in self.slots])
        vd = (C.c_void_p * nF)(*[vc[s * S:].data_ptr() for s in self.slots])
        fi = (C.c_int * nF)(*ids)
        args = (self.eng._h, _lib.ptr(qkv), 3 * d, _lib.ptr(qkv[:, d:]), 3 * d, _lib.ptr(qkv[:, 2 * d:]), 3 * d, _lib.ptr(self.wq),
                _lib.ptr(self.wk), nF, fi, kd, vd)
        if base == "old":
            _lib.check(lib.mmpl_qknorm_rope(*args, _lib.stream_ptr()), "mmpl_qknorm_rope")
        else:
            b = None if base is None else torch.tensor(base, dtype=torch.int32, device=DEV)
            _lib.check(lib.mmpl_qknorm_rope_at(*args, _lib.ptr(b), _lib.stream_ptr()), "mmpl_qknorm_rope_at")
        torch.cuda.synchronize()
        assert torch.equal(qkv[:, d:], self.qkv[:, d:]), "k, v inputs untouched"
        free = [s for s in range(12) if s not in self.slots]
        for c in (kc, vc):                                  # nothing outside the destination pages is written
            assert not c.view(12, S * d)[free].any()
        return qkv[:, :d].clone(), kc, vc


def _same(a, b):
    return all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))


@pytest.mark.parametrize("H,lat,nF", SHAPES)
def test_qknorm_rope_device_base(lib, H, lat, nF):
    c = _Case(H, lat, nF)
    rel = list(range(nF))
    seen = []
    for base in (0, 18, 1020, 1022):                        # 1020 + 4 (the 5-frame shape) and 1022 + 1, + 2 run into the clamp
        want = c.run(lib, [min(base + i, 1023) for i in rel], "old")
        got = c.run(lib, rel, base)
        assert _same(got, want), (H, base)
        assert want[1].any() and want[2].any()
        seen.append(want[0])
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]), "the position changes q"
    # a base that is not the whole position: ids 2.. relative to 16 == ids 18..
    assert _same(c.run(lib, [2 + i for i in rel], 16), c.run(lib, [18 + i for i in rel], "old"))
    # NULL base: the old entry point
    ids = [3, 10, 11, 19, 20][:nF]
    assert _same(c.run(lib, ids, None), c.run(lib, ids, "old"))


def test_qknorm_rope_negative_sum_clamps_to_zero(lib):
    c = _Case(2, (8, 12), 3)
    assert _same(c.run(lib, [0, 1, 2], -1), c.run(lib, [0, 0, 1], "old"))


# ------------------------------------------------------------------------------------------------------------------ DiT forward
@pytest.fixture(scope="module")
def dit():
    """The tiny DiT at lat (16, 24) with a 9-slot cache whose slots 0..5 hold two context blocks."""
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS, dit_state_dict, philox_normal
    cfg = WAN_CONFIGS["tiny"]
    eng = DitEngine(cfg, 16, 24, DEV)
    eng.load_state_dict(dit_state_dict(cfg, seed=5))
    ctx = philox_normal([512, cfg["text_dim"]], 6)
    ctx[24:] = 0
    cross = eng.precompute_context(ctx.to(DEV))
    kc, vc = eng.new_kv_cache(9)
    t0 = torch.zeros(3, device=DEV)
    for b in range(2):
        fr = [3 * b, 3 * b + 1, 3 * b + 2]
        eng.forward(philox_normal([3, 16, 16, 24], 40 + b).to(DEV), t0, fr, fr, list(range(fr[-1] + 1)), kc, vc, cross[0], cross[1])
    x = philox_normal([3, 16, 16, 24], 50).to(DEV)
    t = torch.full([3], 750.0, device=DEV)
    torch.cuda.synchronize()
    yield eng, cross, kc, vc, x, t
    del eng


def _fwd(dit, ids, base, caches=None, out=None):
    eng, cross, kc, vc, x, t = dit
    k, v = (kc.clone(), vc.clone()) if caches is None else caches
    b = None if base is None else torch.tensor(base, dtype=torch.int32, device=DEV)
    flow = eng.forward(x, t, ids, [6, 7, 8], list(range(9)), k, v, cross[0], cross[1], out=out, frame_base=b)
    torch.cuda.synchronize()
    return flow, k, v


def test_dit_forward_relative_ids_plus_base(dit):
    want = _fwd(dit, [6, 7, 8], None)
    got = _fwd(dit, [0, 1, 2], 6)
    assert _same(got, want)
    other = _fwd(dit, [0, 1, 2], 9)
    assert not torch.equal(other[0], want[0]) and not torch.equal(other[1], want[1]), "the base reaches the kernel"
    assert torch.equal(other[2][0], want[2][0]), "layer 0's V is cached unrotated (deeper layers see the rotated attention)"


def test_one_captured_forward_replayed_at_another_position(dit):
    eng, cross, kc, vc, x, t = dit
    k, v = kc.clone(), vc.clone()
    base = torch.tensor(6, dtype=torch.int32, device=DEV)
    out = torch.empty(3, 16, 16, 24, dtype=BF, device=DEV)
    eng.forward(x, t, [0, 1, 2], [6, 7, 8], list(range(9)), k, v, cross[0], cross[1], out=out, frame_base=base)   # warm, eager
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward(x, t, [0, 1, 2], [6, 7, 8], list(range(9)), k, v, cross[0], cross[1], out=out, frame_base=base)
    for pos in (6, 9):
        base.fill_(pos)                                                        # in stream order ahead of the replay
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = _fwd(dit, [pos, pos + 1, pos + 2], None)
        assert _same((out, k, v), want), pos
