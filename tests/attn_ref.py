"""Exact-input reference of the attention kernels (csrc/attention.hip, csrc/attn_w64.hip), one launch at a time through
mmpl_attn_fwd_ex: the case table of tests/test_attn_exact_gpu.py, a seeded operand generator, the buffer geometry around every operand
(canaries, gaps, page placement), a float64 reference, and the criterion.  Importable without a GPU (tests/test_attn_ref.py proves,
on the CPU, every condition the comparison rests on).

The construction.  head_dim 128.  An ORDINARY query row holds three non-zero integers of magnitude 1 or 2 with sum |q| <= 5, in the
first 96 dimensions; K holds {-1, 0, 1} there, V integers with |v| <= 3: all exact in bf16.  Scores s = q.k are integers in
[-5, 5] (spread <= SPREAD = 10), exact in fp32 in any MFMA order.  Every launch (but the `-c8` ones, below) passes softmax_scale = float32(ln 2), for which
c = scale * 1.4426950408889634f rounds to exactly 1.0f: the lock-step kernels' fmaf(s, c, -m c), variant 3's rescaling of q and
the split tail's mref / c ... * c round trip all see integer scores in log2 units, and variant 4 takes the same q as "prescaled".
Then p = exp2(integer) is a power of two (cvt_pk_bf16 of it is exact, also when v_exp is an ulp off a power of two it rounds
back), every rescale by exp2(integer) is exact, and O = sum p v and l = sum p are integer multiples of the smallest p below
2^24 of it as long as n_keys * 3 * 2^SPREAD < 2^24 (n_keys < 5461; `exactness_bounds`): exact in fp32 whatever reference a pass
subtracts (0, the row max, max + 64, a remembered one), whatever the tile size and the order of the tiles.  Only the final
normalisation o = bf16(O * (1 / l)) is left to tolerate.

Criterion.  x = O / l in float64; the kernel's element g must satisfy bf16_rne(x - d) <= g <= bf16_rne(x + d), d = eps * A, with
A = |x| for an unsplit row: g equals one of the two candidates bf16_rne(x (1 -+ eps)); for x == 0 either sign of zero passes and
nothing else.  No element is excluded.  An element is AMBIGUOUS when its two candidates differ; at most AMBIGUITY_CAP of a case.

eps is derived, not measured (`eps`), in units of u = 2^-24:
    unsplit           (n_keys + 8) u    each p within 1 ulp of v_exp_f32 (1), n_keys - 1 fp32 adds of l of at most u relative each if
                                        the p were not exact, the reciprocal (1, correctly rounded division), the product O * inv (1);
                                        the remaining 6 u are head room for the final bf16 pack's input and were not needed by any bound
    split-KV tail     + (3 sp + 1) u    attn_merge_kernel: l = sum_p w_p l_p is 2 sp - 1 roundings (products and adds of positive terms,
                                        relative), inv one, w_p * inv one: every term t_p = (w_p inv) O_p carries (2 sp + 1) u relative;
                                        the product one more and the sp - 1 adds of the element one each on partial sums bounded by
                                        sum_p |t_p|.  The parts can cancel, so this error is absolute: for a row of the tail round
                                        A = sum_p |t_p| >= |x| (`reference` returns it; the parts are the kernel's: tile ranges
                                        [p T / sp, (p + 1) T / sp) of the walk over the pages in address order).
    last_row_copies   + COPIES_EPS      the last key's weight is exp2(s + __logf(copies) / scale - m): __logf is an approximation for
                                        which the ROCm documentation installed with the toolchain states no error.  Measured instead
                                        (tests/test_attn_exact_gpu.py prints it per case): the smallest eps under which every element
                                        of every copies case passes.  On an MI355X it was 0 u in all 16 cases -- every element
                                        equals bf16_rne(x) -- so COPIES_MEASURED = 0 and the allowance, 4 x that (capped at 2^-12),
                                        is 0: the copies cases are held to the unsplit (n_keys + 8) u, the weighted key counting as
                                        one key.  (bf16(copies 2^k (1 + d)) is copies 2^k, so O stays exact; l carries
                                        d p_last / l, which 8 u hold for any d up to 2^-21.)
                                        The weighted score is no integer for copies = 3, 448, so there it must not become the row
                                        maximum m -- every p would stop being a power of two and be rounded to bf16 at 2^-9, as
                                        in production.  In those cases the last key scores TAIL_SCORE = -8 on every ordinary row
                                        (-8 + log2 448 < 1) and key 0 scores HEAD_SCORE = 3 (two more reserved dimensions); with a
                                        single key the weight cancels.  copies = 2 has the integer bias 1: the `-max` cases put the
                                        weighted key at 5, ABOVE every other key, so that last_bias takes part in the row maximum
                                        and, with two tiles, in the rescale of the running one, and everything stays exact.
c != 1.  float32(ln 2) / 8 gives c = 0.125 exactly; the `-c8` cases pass that scale and, on a raw q (variants 1, 3), q times 8, so the
raw scores are multiples of 8 and s c, m c, mref / c and (m_p - m) c are all exact: the same reference, the same eps, and a c that is
dropped, doubled or applied on the wrong side changes the result.  This pair of split cases (and four unsplit ones) stands in for
the pair at the production scale 1 / sqrt(128), which is NOT built: with q = bf16(q_int * c) the scores are no integers, every p is
rounded to bf16 (2^-9 relative) before the PV MFMA and O is a sum with cancellation, so the honest bound there is of the order of
n_keys 2^-9 |v|max / |x| per element -- no candidate criterion; tests/test_kernels_gpu.py and tests/test_attn_history_gpu.py keep
judging that scale by rel_l2.
PROBE rows.  A fixed subset of the query rows (`probe_rows`) is zero in the first 96 dimensions and addresses ONE key through the
last 32: K row n holds there the four base-8 digits of its index n, one-hot in four groups of 8, and the probe holds +10 on its
target's digits and -30 elsewhere: the target scores 40, every other key <= 0.  Such a row must return the target's V row (whose
elements are non-zero): the other keys weigh at most n_keys 2^-40 together, which fp32 drops and float64 keeps -- a relative
difference of at most 6 n_keys 2^-40 < 2^-26 that eps covers (asserted on the CPU).  Across a case the targets sweep the first and
last row of every page and then the positions mod 64; the three variants of a shape start the sweep at different positions, and
tests/test_attn_ref.py asserts that together they visit every position a shape has.  Rows that share a lane of attn_w64_kernel
(r and r ^ 32) are of the same kind, so that the FAST pass's shared reference holds both and no block of a plain case is redone.

BEYOND the exact class (`spike`): one 256-row block, one page of 448 rows (7 tiles).  Row SPIKE_A addresses a key in tile 6 with 200
(everything else <= 0): the FAST reference (first four tiles + 64) cannot hold it, the block is redone by the GENERAL pass, which
meets the key on its slow rescale.  Row SPIKE_B = SPIKE_A ^ 32 (the same lane) scores 20 on a key of tile 3 and 35 on the same
position of tile 5, everything else <= -70: the GENERAL pass accepts tile 3 on its running reference and redoes tile 5, whose
partial sum 2^35 exceeds 2^30.  What fp32 drops here is at most n_keys 2^-70 < 2^-60 relative (asserted on the CPU); criterion and
eps are unchanged.  With a history the second launch runs FAST on the remembered references (mean log-sum-exp of the lane: ~120).

"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
HD, ORD, KVB, QB = 128, 96, 64, 256
SPREAD = 10
U = 2.0 ** -24
AMBIGUITY_CAP = 0.10
SCALE_LN2 = float(np.float32(math.log(2.0)))
LOCKSTEP, CROSS1, CROSS2, W64 = 1, 2, 3, 4           # plan[0]: AttnKernel (csrc/kernels.h)
CANARY_BF16 = 0x7FA5                                 # a NaN pattern no kernel produces
K_CANARY = 2.0 ** 100
GAP_ROWS, END_ROWS = 3, 64
PROBE_HIT, PROBE_MISS = 10, -30                      # 4 digits: the target scores 40, one wrong digit 0
SPIKE_A, SPIKE_B = 77, 77 ^ 32
HEAD_SCORE, TAIL_SCORE = 3, -8                       # last_row_copies cases: what the first and (Case.tail) the weighted last key score on an ordinary row
COPIES_MEASURED = 0.0                                # measured on an MI355X (docstring): every element of every copies case equals bf16_rne(x)
COPIES_EPS = min(4.0 * COPIES_MEASURED, 2.0 ** -12)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    variant: int                   # mmpl_attn_fwd_ex: 1 lock-step, 3 w64 on a raw q, 4 w64 on a prescaled q
    n_pages: int
    page_rows: int
    Lq: int = 64
    H: int = 1
    layout: str = "gaps"           # "gaps": shuffled pages, GAP_ROWS canary rows behind each; "contig": back to back in list order;
                                   # "groups": 4 + 5 pages of two allocations that lie back to back, listed alternately
    split_groups: bool = False     # "groups" only: every page its own group (the same keys, presented unmerged)
    ldq_mult: int = 1              # q lies in a [Lq, ldq_mult * H * 128] matrix (3: the fused qkv)
    kpad: int = 0                  # ldk = ldv = H * 128 + kpad
    cross: int = 0
    copies: int = 0
    workspace: bool = False
    history: bool = False
    spike: bool = False
    cdiv: int = 1                  # softmax_scale = float32(ln 2) / cdiv, so c = 1 / cdiv exactly; a raw q (variants 1, 3) is handed in times cdiv
    tail: int = -8                 # copies cases: what the weighted last key scores on every ordinary row (TAIL_SCORE; 5: it is the row maximum)
    # expected path at 32 CUs per XCD (plan_restated gives it for any device)
    kernel: int = LOCKSTEP
    pages_walked: int = 0          # 0 = n_pages
    split: bool = False            # the plan must report sp > 1
    stats: tuple = ()              # w64: per launch (redone, held on remembered references); () = (0, 0) on every launch
    why: str = ""

    @property
    def n_keys(self): return self.n_pages * self.page_rows
    @property
    def d(self): return self.H * HD
    @property
    def ldq(self): return self.ldq_mult * self.d
    @property
    def ldo(self): return self.d + 8
    @property
    def ldk(self): return self.d + self.kpad
    @property
    def w64(self): return self.variant in (3, 4)
    @property
    def n_qb(self): return (self.Lq + QB - 1) // QB
    @property
    def scale(self): return float(np.float32(SCALE_LN2) / np.float32(self.cdiv))
    @property
    def operand_key(self): return (self.n_pages, self.page_rows, self.Lq, self.H, self.spike, self.variant, self.tail)      # (the probes' targets depend on the variant)


def _cases():
    c = []
    def add(name, variant, n_pages, page_rows, **kw):
        kw.setdefault("kernel", W64 if variant in (3, 4) else LOCKSTEP)
        c.append(Case(f"{name}-v{variant}", variant, n_pages, page_rows, **kw))
    for v in (1, 3, 4):
        # ---- KV stream: H = 1, Lq = 64.  One page: T = 1, ragged tiles, a tile plus one row, T = 4 against 5 (the FAST reference is
        # sampled from the first 4 tiles only when T > 4), a wrap of the ring of 4
        for S in (1, 30, 63, 64, 65, 256, 257, 320, 577):
            add(f"kv-1x{S}", v, 1, S, why="one page")
        for n, S in ((24, 10), (21, 72), (5, 40), (3, 64)):
            add(f"kv-{n}x{S}", v, n, S, why="pages by rows")
        add("kv-3x100-contig", v, 3, 100, layout="contig", pages_walked=1 if v != 1 else 3, why="w64 merges back-to-back pages")
        add("kv-4+5x40-groups", v, 9, 40, layout="groups", pages_walked=2 if v != 1 else 9, why="two allocations, merged per group")
        add("kv-4+5x40-unmerged", v, 9, 40, layout="groups", split_groups=True, why="the same keys, every page its own group")
        # ---- query side: clamped rows past Lq; head counts, q inside a fused qkv, grid padding on the last XCD when H % 8 != 0
        for Lq in (1, 255, 256, 257, 513):
            add(f"q-Lq{Lq}", v, 2, 72, Lq=Lq, why="rows past Lq")
        for H, kw in ((2, dict(ldq_mult=3)), (3, dict(kpad=8)), (8, {}), (12, {})):
            add(f"q-H{H}", v, 2, 72, Lq=513, H=H, why="heads / grid padding", **kw)
    # ---- beyond the exact class
    add("spike", 4, 1, 448, Lq=256, spike=True, stats=((1, 0), (1, 0)), why="FAST fails, GENERAL slow rescale")
    add("spike-raw", 3, 1, 448, Lq=256, spike=True, stats=((1, 0), (1, 0)), why="the same on a raw q")
    add("spike-history", 4, 1, 448, Lq=256, spike=True, history=True, stats=((1, 0), (0, 1)), why="FAST held on remembered references")
    # ---- split-KV tail (variant 4): b = n_qb * H / 8 work items per XCD, the b mod 32 of the last round run as sp parts
    add("split-H8", 4, 3, 520, Lq=256 * 40 + 1, H=8, workspace=True, split=True, why="tail of 9 items per XCD in 3 parts")
    add("split-H12", 4, 3, 520, Lq=256 * 40 + 1, H=12, workspace=True, why="62 items per XCD: a tail of 30 is not split")
    add("split-H12-tail10", 4, 5, 330, Lq=256 * 27 + 1, H=12, workspace=True, split=True, why="H % 8 != 0, parts cut inside pages")
    add("split-H8-nows", 4, 3, 520, Lq=256 * 40 + 1, H=8, why="no workspace: sp = 1")
    # ---- c != 1: scale = float32(ln 2) / 8, c = 0.125 exactly, raw q times 8 (scores in multiples of 8): a dropped, doubled or misplaced c
    # in the split tail's mref / c and the merge's (m_p - m) c, variant 3's rescale of q, the lock-step fmaf(s, c, -m c) or last_bias shows
    add("split-H8-c8", 4, 3, 520, Lq=256 * 40 + 1, H=8, workspace=True, split=True, cdiv=8, why="the split pair at c = 1/8")
    add("split-H12-tail10-c8", 4, 5, 330, Lq=256 * 27 + 1, H=12, workspace=True, split=True, cdiv=8, why="the split pair at c = 1/8")
    for v in (1, 3, 4):
        add("kv-21x72-c8", v, 21, 72, cdiv=8, why="c = 1/8")
    add("spike-raw-c8", 3, 1, 448, Lq=256, spike=True, cdiv=8, stats=((1, 0), (1, 0)), why="GENERAL pass on a raw q at c = 1/8")
    # ---- lock-step only: the weighted padded text key, and the LDS-resident cross kernels
    for copies in (2, 3, 448):
        for S in (1, 13, 64, 65):
            add(f"copies{copies}-1x{S}", 1, 1, S, copies=copies, why="last_row_copies")
    add("copies448-1x65-c8", 1, 1, 65, copies=448, cdiv=8, why="last_bias = ln(copies) / scale at c = 1/8")
    for S in (13, 64, 65):
        add(f"copies2-1x{S}-max", 1, 1, S, copies=2, tail=5, why="the weighted key is the row maximum (integer bias: still exact)")
    for S, kern in ((40, CROSS1), (100, CROSS2)):
        for H, Lq in ((40, 7 * 256 - 100), (36, 9 * 256 - 100)):
            for copies in (0, 448):
                add(f"cross-1x{S}-H{H}" + ("-copies" if copies else ""), 1, 1, S, Lq=Lq, H=H, cross=1, copies=copies, kernel=kern,
                    why="query blocks per block 2, the last block ragged")
    return c


CASES = _cases()


def eps(c: Case, sp: int = 1) -> float:
    return (c.n_keys + 8 + (3 * sp + 1 if sp > 1 else 0)) * U + (COPIES_EPS if c.copies > 1 else 0.0)


def exactness_bounds(c: Case):
    """(quantum, bound) of O and l relative to the row's smallest p, from the input ranges alone: exact in fp32 iff bound < 2^24."""
    if c.copies > 1:            # the plain keys span [min(tail, -5), 5] above the smallest p; the weighted one is `copies` times 2^tail
        lo = min(c.tail, -5)
        n = (c.n_keys - 1) * 2.0 ** (5 - lo) + c.copies * 2.0 ** (c.tail - lo)
        return [("l", 1.0, n), ("O", 1.0, 3 * n)]
    n = c.n_keys
    return [("l", 1.0, n * 2.0 ** SPREAD), ("O", 1.0, 3 * n * 2.0 ** SPREAD)]


# ---------------------------------------------------------------------------------------------------------------- launch plan
WS_BYTES = 256 * QB * 130 * 4        # mmpl_attn_workspace_bytes() today; the GPU test hands in what the library reports


def plan_restated(c: Case, per: int = 32, ws_bytes: int = WS_BYTES):
    """[kernel, pages, KV tiles, main blocks, tail items per XCD, parts, query blocks per block, blocks per head] for `per` CUs per XCD."""
    n_qb, tpp = c.n_qb, -(-c.page_rows // KVB)
    if not c.w64:
        if c.cross and c.n_pages == 1 and c.page_rows <= 2 * KVB:
            bph = min(max(8 * per // c.H, 1), n_qb)
            qpb = -(-n_qb // bph)
            bph = -(-n_qb // qpb)
            return [CROSS1 if tpp == 1 else CROSS2, 1, tpp, bph * c.H, 0, 1, qpb, bph]
        return [LOCKSTEP, c.n_pages, c.n_pages * tpp, n_qb * c.H, 0, 1, 0, 0]
    walk = layout(c).walk
    tiles = sum(-(-len(p) // KVB) for p in walk)
    total = n_qb * c.H
    b = total // 8 if c.H % 8 == 0 else -(-total // 8)
    tb, sp = b % per, 1
    if c.workspace and b > per and tb > 0 and per // tb >= 2:
        sp = min(4, per // tb)
        if tiles // sp < 8 or 8 * tb * sp * QB * 130 * 4 > ws_bytes:
            sp = 1
    tail = tb if sp > 1 else 0
    return [W64, len(walk), tiles, 8 * (b - tail), tail, sp, 0, 0]


def tail_items(c: Case, per: int, tail: int):
    """(head, query block) of the work items of the split tail round (csrc/kernels.h: mmpl_attn_item)."""
    total = c.n_qb * c.H
    b = total // 8 if c.H % 8 == 0 else -(-total // 8)
    out = []
    for xcd in range(8):
        for local in range(b - tail, b):
            if c.H % 8 == 0:
                head, qb = xcd + 8 * (local // c.n_qb), local % c.n_qb
                if head < c.H:
                    out.append((head, qb))
            else:
                item = xcd * b + local
                if item < total:
                    out.append((item // c.n_qb, item % c.n_qb))
    return out


# ---------------------------------------------------------------------------------------------------------------- geometry
@dataclasses.dataclass(frozen=True)
class Layout:
    page_row0: tuple          # first buffer row of page p (list order)
    rows: int                 # rows of the K (and V) buffer, canaries included
    groups: tuple             # page_group byte per page
    walk: tuple               # attn_w64_kernel's pages after sorting by (group, address) and merging: tuples of key indices


@functools.lru_cache(maxsize=None)
def layout(c: Case) -> Layout:
    n, S = c.n_pages, c.page_rows
    if c.layout == "gaps":
        order = list(np.random.RandomState(1000 * n + S).permutation(n))
        row0, cur = [0] * n, 0
        for p in order:
            row0[p] = cur
            cur += S + GAP_ROWS
        groups = [0] * n
    elif c.layout == "contig":
        row0, cur, groups = [p * S for p in range(n)], n * S, [0] * n
    else:
        assert n == 9
        # list order B0 A0 B1 A1 B2 A2 B3 A3 B4; allocation A (group 0) = 4 pages at rows [0, 4 S), B (group 1) = 5 pages right behind
        row0 = [(4 + p // 2) * S if p % 2 == 0 else (p // 2) * S for p in range(n)]
        groups = list(range(n)) if c.split_groups else [1 if p % 2 == 0 else 0 for p in range(n)]
        cur = n * S
    keys = lambda p: tuple(range(p * S, (p + 1) * S))
    walk = []
    if c.w64:
        order = sorted(range(n), key=lambda p: (groups[p], row0[p]))
        for p in order:
            q = walk[-1] if walk else None
            if q is not None and groups[q[0]] == groups[p] and row0[p] == row0[q[1]] + S:
                walk[-1] = (q[0], p, q[2] + keys(p))
            else:
                walk.append((p, p, keys(p)))
        walk = [w[2] for w in walk]
    else:
        walk = [keys(p) for p in range(n)]
    return Layout(tuple(row0), cur + END_ROWS, tuple(groups), tuple(walk))


def canary(n, device="cpu"):
    return torch.full((n,), CANARY_BF16, dtype=torch.int16, device=device).view(BF)


def bits(t):
    return t.view(torch.int16)


def kv_buffers(c: Case, K, V, device):
    """K / V [n_keys, d] -> the two buffers [rows, ldk] with the pages at their places; everything else is canary: 2^100 in K, NaN in V."""
    lay = layout(c)
    kb = torch.full((lay.rows, c.ldk), K_CANARY, dtype=BF, device=device)
    vb = canary(lay.rows * c.ldk, device).view(lay.rows, c.ldk)
    for p, r0 in enumerate(lay.page_row0):
        kb[r0:r0 + c.page_rows, :c.d] = K[p * c.page_rows:(p + 1) * c.page_rows].to(device)
        vb[r0:r0 + c.page_rows, :c.d] = V[p * c.page_rows:(p + 1) * c.page_rows].to(device)
    return kb, vb


def q_buffer(c: Case, q, device):
    """q [Lq, d] (log2 score units) -> [Lq + 3, ldq] with the q the launch takes in the first d columns and NaN everywhere else: a raw q
    (variants 1, 3) is q * cdiv, which the kernel's c = 1 / cdiv undoes exactly; variant 4's q is "already multiplied by c"."""
    qb = canary((c.Lq + 3) * c.ldq, device).view(c.Lq + 3, c.ldq)
    qb[:c.Lq, :c.d] = (q.to(device).float() * (1 if c.variant == 4 else c.cdiv)).to(BF)
    return qb


def o_buffer(c: Case, device):
    return canary((c.Lq + 3) * c.ldo, device).view(c.Lq + 3, c.ldo)


# ---------------------------------------------------------------------------------------------------------------- inputs
def probe_rows(c: Case):
    """Query rows (of every head) that are probes.  KV-stream shapes (Lq = 64): three rows in four; else r % 32 in {5, 12, 21}.  A row
    whose lane partner in attn_w64_kernel (r ^ 32, clamped to Lq - 1 like the kernel's loads) is of the other kind is ordinary, and so
    is row Lq - 1 when the kernel reads it in place of rows past Lq."""
    want = (lambda r: r % 32 >= 8) if c.Lq == 64 else (lambda r: r % 32 in (5, 12, 21))
    kind = [want(r) for r in range(c.Lq)]
    if c.Lq % 64:
        kind[c.Lq - 1] = False
    return [r for r in range(c.Lq) if kind[r] and kind[min(r ^ 32, c.Lq - 1)]]


def target_pool(c: Case):
    """Keys worth aiming at: the first and last row of every page, then one key per position mod 64 (of the row within its page),
    taken from the pages in turn."""
    S, n = c.page_rows, c.n_pages
    pool = []
    for p in range(n):
        pool += [p * S, p * S + S - 1]
    for i in range(min(S, 64)):
        rows = range(i, S, 64)
        pool.append(((5 * i) % n) * S + rows[i % len(rows)])
    return list(dict.fromkeys(pool))


def probe_targets(c: Case, n_probes: int):
    """The key every probe (in order of head, then row) aims at: the pool in order, started a third of the way further per variant, so
    that the three variants of a shape with fewer probes than keys worth aiming at visit all of them together."""
    pool = target_pool(c)
    start = len(pool) * {1: 0, 3: 1, 4: 2}[c.variant] // 3
    return [pool[(start + i) % len(pool)] for i in range(n_probes)]


def _digits(n):
    return [(n >> (3 * g)) & 7 for g in range(4)]


def _address(weights_hit, miss, target):
    """the 32 reserved entries of a q row: per digit group `hit` on the target's digit and `miss` elsewhere"""
    v = torch.full((32,), float(miss))
    for g, dg in enumerate(_digits(target)):
        v[8 * g + dg] = float(weights_hit[g])
    return v


@functools.lru_cache(maxsize=2)
def operands(key, c: Case):
    """q [Lq, d], K, V [n_keys, d] (bf16, CPU) and the probe table {(head, row): key}."""
    g = torch.Generator().manual_seed(hash(key) % (2 ** 31))
    N, d, H, Lq = c.n_keys, c.d, c.H, c.Lq
    assert N <= 4096
    K = torch.zeros(N, H, HD)
    K[:, :, :ORD] = torch.randint(-1, 2, (N, H, ORD), generator=g).float()
    code = torch.zeros(N, 32)
    for n in range(N):
        for gi, dg in enumerate(_digits(n)):
            code[n, 8 * gi + dg] = 1.0
    K[:, :, ORD:] = code[:, None, :]
    V = torch.randint(-3, 4, (N, H, HD), generator=g).float()
    q = torch.zeros(Lq, H, HD)
    free = ORD - 2 if c.copies > 1 else ORD
    pos = torch.rand(Lq, H, free, generator=g).argsort(dim=-1)[..., :3]
    mag = torch.randint(1, 3, (Lq, H, 3), generator=g).float()
    mag[..., 2] = torch.where(mag.sum(-1) == 6, torch.ones(()), mag[..., 2])
    sign = torch.randint(0, 2, (Lq, H, 3), generator=g).float() * 2 - 1
    q.scatter_(2, pos, mag * sign)
    if c.copies > 1:
        # the weighted key must stay under the row maximum (see the docstring): it scores TAIL_SCORE on every ordinary row, key 0 scores HEAD_SCORE
        K[:, :, free:ORD] = 0
        K[N - 1, :, :free] = 0
        K[N - 1, :, free + 1] = 1
        q[:, :, free + 1] = c.tail
        if N > 1:
            K[0, :, :free] = 0
            K[0, :, free] = 1
            q[:, :, free] = HEAD_SCORE
    rows = probe_rows(c) if not c.spike else [r for r in probe_rows(c) if r not in (SPIKE_A, SPIKE_B)]
    table = {}
    targets = probe_targets(c, len(rows) * H)
    for i, (h, r) in enumerate((h, r) for h in range(H) for r in rows):
        t = targets[i]
        table[(h, r)] = t
        q[r, h] = 0
        q[r, h, ORD:] = _address([PROBE_HIT] * 4, PROBE_MISS, t)
        V[t, h] = torch.where(V[t, h] == 0, torch.ones(()), V[t, h])
    if c.spike:
        a_key, b_lo, b_hi = 6 * 64 + 17, 3 * 64 + 29, 5 * 64 + 29
        q[SPIKE_A, 0] = 0
        q[SPIKE_A, 0, ORD:] = _address([50] * 4, -150, a_key)           # 200 on a_key, <= 0 elsewhere (three digits right: 150 - 150)
        wq = _address([5, 5, 0, 5], -100, b_hi)                         # digit group 2 = the tile index: 20 on tile 5, 5 on tile 3
        wq[8 * 2 + 5], wq[8 * 2 + 3] = 20.0, 5.0
        q[SPIKE_B, 0] = 0
        q[SPIKE_B, 0, ORD:] = wq
        for t in (a_key, b_lo, b_hi):
            V[t, 0] = torch.where(V[t, 0] == 0, torch.ones(()), V[t, 0])
        assert _digits(b_lo)[2] == 3 and _digits(b_hi)[2] == 5 and _digits(b_lo)[:2] == _digits(b_hi)[:2]
    return q.reshape(Lq, d).to(BF), K.reshape(N, d).to(BF), V.reshape(N, d).to(BF), table


def case_operands(c: Case):
    return operands(c.operand_key, c)


# ---------------------------------------------------------------------------------------------------------------- reference
def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; ONE rounding (a detour through fp32 would round twice), done on the
    bits: 8 of the 53 significant bits stay.  (Finite values inside bf16's exponent range, which is fp32's.)"""
    b = x.contiguous().view(torch.int64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    return b.view(torch.float64)


def window(x, delta):
    return bf16_rne(x - delta), bf16_rne(x + delta)


def outside(got, x, delta):
    """bool mask: elements of the kernel's output (bf16) that are none of their candidates."""
    lo, hi = window(x, delta)
    g = got.double()
    return ~((g >= lo) & (g <= hi))


def ambiguous(x, delta):
    lo, hi = window(x, delta)
    return lo != hi


def needed_eps(got, x, A, hi=2.0 ** -8):
    """the smallest eps (to 1 %) under which no element is outside; inf if `hi` is not enough"""
    if bool(outside(got, x, hi * A).any()):
        return float("inf")
    lo = 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if bool(outside(got, x, mid * A).any()):
            lo = mid
        else:
            hi = mid
        if hi - lo < 0.01 * hi:
            break
    return hi


def scores(c: Case, q, K, head, rows=None):
    """float64 [rows, n_keys] scores of one head (log2 units: the launches' c is 1)"""
    qh = q[:, head * HD:(head + 1) * HD].double()
    if rows is not None:
        qh = qh[rows]
    return qh @ K[:, head * HD:(head + 1) * HD].double().T


def key_weights(c: Case, device):
    w = torch.ones(c.n_keys, dtype=torch.float64, device=device)
    if c.copies > 1:
        w[-1] = float(c.copies)
    return w


def softmax_ref(c: Case, s, Vh, w, parts=None):
    """s [R, N] float64, Vh [N, 128], w [N] -> (x [R, 128], A [R, 128]): A = |x|, or sum over `parts` (lists of key indices) of the
    parts' |contribution| for rows that the kernel computes in parts."""
    m = s.max(dim=1, keepdim=True).values
    p = torch.exp2(s - m) * w
    l = p.sum(dim=1, keepdim=True)
    x = (p @ Vh.double()) / l
    if parts is None:
        return x, x.abs()
    A = torch.zeros_like(x)
    for idx in parts:
        idx = torch.as_tensor(idx, device=s.device)
        A += (p[:, idx] @ Vh[idx].double()).abs() / l
    return x, A


def split_parts(c: Case, sp: int):
    """key indices of the sp KV ranges of a tail block: tiles [p T / sp, (p + 1) T / sp) of the walk"""
    tiles = [pg[i:i + KVB] for pg in layout(c).walk for i in range(0, len(pg), KVB)]
    T = len(tiles)
    return [sum((list(t) for t in tiles[p * T // sp:(p + 1) * T // sp]), []) for p in range(sp)]


def reference(c: Case, q, K, V, plan=None, per: int = 32):
    """x and A [Lq, d] float64 on the operands' device; plan = the launch plan (plan_restated's form; None = restated at `per`)."""
    plan = plan or plan_restated(c, per)
    sp, tail = plan[5], plan[4]
    w = key_weights(c, q.device)
    x = torch.empty(c.Lq, c.d, dtype=torch.float64, device=q.device)
    A = torch.empty_like(x)
    parts = split_parts(c, sp) if sp > 1 else None
    tails = {}
    for h, qb in (tail_items(c, per, tail) if sp > 1 else []):
        tails.setdefault(h, []).append(qb)
    for h in range(c.H):
        s = scores(c, q, K, h)
        Vh = V[:, h * HD:(h + 1) * HD]
        xh, Ah = softmax_ref(c, s, Vh, w)
        for qb in tails.get(h, []):
            r = slice(qb * QB, min((qb + 1) * QB, c.Lq))
            _, Ah[r] = softmax_ref(c, s[r], Vh, w, parts)
        x[:, h * HD:(h + 1) * HD], A[:, h * HD:(h + 1) * HD] = xh, Ah
    return x, A


def fast_pass_fails(c: Case, s, keys_tiles):
    """Would attn_w64_kernel's FAST pass fail on a block?  s: float64 [256, n_keys] scores of the block's rows (rows past Lq clamped to
    Lq - 1, as the kernel loads them); keys_tiles: the block's KV tiles in the kernel's order (lists of key indices).  The reference
    of rows r and r ^ 32 is the largest score either has in the sampled tiles (the first four when there are more than four, else
    the first) + 64; every row sum must end within [2^-100, 2^100]."""
    T = len(keys_tiles)
    sample = [k for t in keys_tiles[:4 if T > 4 else 1] for k in t]
    allk = [k for t in keys_tiles for k in t]
    mx = s[:, sample].max(dim=1).values
    if T > 4 and any(len(t) < KVB for t in keys_tiles[1:4]):
        # tiles 1 .. 3 are sampled under tile 0's mask: the zero-filled rows behind a page's end score 0 there.  (Harmless: any reference
        # inside the window gives the exact softmax; it only moves which blocks the window sends to the GENERAL pass.)
        mx = mx.clamp(min=0.0)
    ref = torch.maximum(mx, mx[torch.arange(s.shape[0]) ^ 32]) + 64
    e = s[:, allk] - ref[:, None]
    l = torch.where(e < -126, torch.zeros_like(e), torch.exp2(e)).sum(dim=1)       # (v_exp_f32 flushes what would be a denormal)
    return bool(((l < 2.0 ** -100) | (l > 2.0 ** 100)).any())


def predict_redone(c: Case, q, K, plan, per: int = 32, heads=None):
    """blocks of a stateless launch that the GENERAL pass redoes (the counter stats[1]), over `heads` (default all)"""
    tiles = [list(pg[i:i + KVB]) for pg in layout(c).walk for i in range(0, len(pg), KVB)]
    sp, T = plan[5], len(tiles)
    tails = set(tail_items(c, per, plan[4])) if sp > 1 else set()
    n = 0
    for h in (range(c.H) if heads is None else heads):
        sh = scores(c, q, K, h)
        for qb in range(c.n_qb):
            rows = torch.clamp(torch.arange(qb * QB, (qb + 1) * QB), max=c.Lq - 1)
            parts = [tiles[p * T // sp:(p + 1) * T // sp] for p in range(sp)] if (h, qb) in tails else [tiles]
            n += sum(fast_pass_fails(c, sh[rows], part) for part in parts)
    return n
