"""The GEMM (csrc/gemm.hip) pinned by the bytes it produces on real-valued inputs (-m gpu).

tests/test_gemm_forms_gpu.py feeds integers, which make every order of summation exact: a change of the MFMA operand order, of the
k order per accumulator, of the order in which split-K parts are summed or of an epilogue's rounding points can pass it.  Here the
inputs are seeded real-valued bf16 (A ~ N(0, 1), W ~ N(0, 1) / sqrt(K), bias, residual and gate ~ N(0, 1)), so any such change moves
bits, and a change to gemm.hip that is meant to leave the arithmetic alone is held to the sha256 of C's whole buffer and of the
pages' whole buffer after one launch (tests/golden/gemm_digests.json, recorded on an MI355X before that change).  Every case of
tests/gemm_ref.CASES, with that module's buffer geometry, canaries and pages, plus four shapes whose tile lists have dealt groups
(XCD x works through M-groups x, x + 8, ...) with group 8 and group 4, launched with and without tile tickets.  Every case ran twice
in separate processes when it was recorded and gave the same digest both times: every kernel path computes a tile the same way
whoever draws it, and split-K sums in part order.  A kernel change that moves bits on purpose records the file again.
"""
import ctypes as C
import hashlib
import json
import math
import os

import pytest
import torch

from tests import gemm_ref as R
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (99 row panels, N < 8192, K < 8192: group 8, one dealt round of 8 groups, persistent with tickets); (36 row panels: group 4, one dealt
# round, one block per tile); (16 row panels, K >= 4096: tickets and a split-K tail); (13 x 3 tiles, one block per tile)
EXTRA = [
    R.Case("dealt-g8-tickets-25200x5120x1024-epi3", 25200, 5120, 1024, 3, R.V6, staged=1, main="percu", rpf=3600, inplace=True, scratch=True),
    R.Case("dealt-g4-9000x2560x512-epi0", 9000, 2560, 512, 0, R.V6, staged=1),
    R.Case("splitk-tickets-4096x5120x5120-epi1", 4096, 5120, 5120, 1, R.V6, tail=R.SPLITK, staged=1, splitk_s=4, main="percu", scratch=True),
    R.Case("ragged-3120x768x256-epi4", 3120, 768, 256, 4, R.V6, staged=1, inplace=True),
]
CASES = {c.name: c for c in R.CASES + EXTRA}


def _normal(g, n, scale=1.0):
    return (torch.randn(n, generator=g, dtype=torch.float32) * scale).to(R.BF)


def inputs(c):
    """A, W (whole buffers, as gemm_ref.operands sizes them), bias, gate, res of a case: seeded on the CPU, real-valued."""
    g = torch.Generator().manual_seed(1000003 * c.M + 1009 * c.N + c.K + 17 * c.epi + c.batch)
    a = _normal(g, (c.batch - 1) * c.sA + (c.M - 1) * c.LDA + c.K)
    w = _normal(g, (c.batch - 1) * c.sW + (c.N - 1) * c.LDW + c.K, 1.0 / math.sqrt(c.K))
    bias = _normal(g, c.N) if c.bias and c.epi != R.EPI_F32_SCALE else None
    gate = _normal(g, c.n_frames * c.GATE_STRIDE) if c.epi == R.EPI_GATE_RES else None
    res = _normal(g, c.M * c.N).view(c.M, c.N) if c.epi in (R.EPI_GATE_RES, R.EPI_RES) else None
    return [None if t is None else t.to(DEV) for t in (a, w, bias, gate, res)]


def digest(lib, c):
    """One launch of case c (the call of tests/test_gemm_forms_gpu.py) -> (plan, digest of C's buffer and the pages' buffer)."""
    from mmpl_amd import _lib
    a, w, bias, gate, res = inputs(c)
    sbytes = lib.mmpl_gemm_scratch_bytes()
    sbuf = torch.zeros(sbytes, dtype=torch.uint8, device=DEV) if c.scratch else None
    tickets = torch.zeros(8, dtype=torch.int32, device=DEV) if c.tickets else None
    cb, vb = R.initial_buffers(c, res, DEV)
    c_ptr = cb.data_ptr() + (4 if c.epi == R.EPI_F32_SCALE else 2) * c.c_off
    res_ptr, ldres = 0, 0
    if res is not None:
        res_ptr, ldres = (c_ptr, c.LDC) if c.inplace else (res.data_ptr(), c.N)
    gate_ptr = gate.data_ptr() + 2 * R.gate_off(c) if gate is not None else 0
    pages, n_pages = None, 0
    if vb is not None:
        n_pages = c.n_frames
        pages = (C.c_void_p * n_pages)(*[vb.data_ptr() + 2 * o for o in R.page_layout(c)[0]])
    plan = (C.c_int * 6)(*([-1] * 6))
    _lib.check(lib.mmpl_gemm_ex(_lib.ptr(a), c.LDA, _lib.ptr(w), c.LDW, _lib.ptr(bias), C.c_void_p(c_ptr), c.LDC, c.M, c.N, c.K, c.epi,
                                C.c_void_p(res_ptr), ldres, C.c_void_p(gate_ptr), c.GATE_STRIDE if gate is not None else 0, c.rpf,
                                c.alpha, c.batch, c.sA, c.sW, c.sC, pages, n_pages, c.v_col0, c.V_LD if vb is not None else 0,
                                _lib.ptr(sbuf), sbytes if c.scratch else 0, _lib.ptr(tickets), plan, _lib.stream_ptr()), c.name)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for buf in (cb, vb):
        if buf is not None:
            h.update(R.bits(buf).cpu().numpy().tobytes())
    return list(plan), h.hexdigest()


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_digest(lib, name):
    want = json.load(open(os.path.join(GOLDEN, "gemm_digests.json")))
    c = CASES[name]
    plan, got = digest(lib, c)
    print(f"{name}: plan {plan} digest {got}")
    assert plan[:3] == [c.kernel, c.tail, c.staged] and plan[5] == c.splitk_s, (plan, "the shape no longer reaches the path it is here for")
    assert got == want[name]
