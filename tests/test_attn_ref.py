"""What tests/test_attn_exact_gpu.py rests on, proven on the CPU for every case of tests/attn_ref.py's table (no GPU, default suite):
integer scores within the spread, the fp32 exactness bounds, an fp32 emulation of the kernels' accumulation that reproduces the
float64 O and l exactly under several references, tile sizes and tile orders (and per split part, with attn_merge_kernel's merge in
part order), the ambiguity cap, c == 1.0f, the probes, the geometry, and -- so that the criterion can see each error class -- that every
reference-side mutation moves at least one element outside its candidates.

Large cases are checked on a sample of their rows (the first and last rows of two heads, and rows of the split tail round)."""
import numpy as np
import pytest
import torch

from tests import attn_ref as R

F32 = np.float32
IDS = [c.name for c in R.CASES]


def _sample(c, plan):
    """[(head, rows tensor, rows are computed in parts)]"""
    heads = sorted({0, c.H - 1})
    rows = torch.arange(c.Lq) if c.Lq <= 320 else torch.cat([torch.arange(160), torch.arange(c.Lq - 96, c.Lq)])
    out = [(h, rows, False) for h in heads]
    if plan[5] > 1:
        h, qb = R.tail_items(c, 32, plan[4])[3]
        out = [(h, torch.arange(qb * R.QB, min(qb * R.QB + 96, c.Lq)), True), (heads[0], rows[:96], False)]
    return out


def _bf16(a32):
    return torch.from_numpy(np.ascontiguousarray(a32)).to(R.BF).float().numpy()


def _emulate(s, Vh, w, ref, keys, ts):
    """fp32 accumulation of O and l over the keys `keys` in tiles of ts, against the per-row reference `ref` (float64 integers):
    p = exp2(s + log2 w - ref) in fp32, O += bf16(p) . V as the PV MFMA does, l += p."""
    R_, O, l = s.shape[0], None, None
    O = np.zeros((R_, R.HD), F32)
    l = np.zeros(R_, F32)
    lw = np.log2(w).astype(F32)
    for i in range(0, len(keys), ts):
        t = np.asarray(keys[i:i + ts])
        arg = (s[:, t].astype(F32) + lw[t][None, :]) - ref.astype(F32)[:, None]
        plain = lw[t] == 0
        p = np.where(plain[None, :], np.ldexp(F32(1), np.clip(arg, -149, 127).astype(np.int32)).astype(F32), np.exp2(arg, dtype=F32))
        l = (l + p.sum(axis=1, dtype=F32)).astype(F32)
        O = (O + (_bf16(p) @ Vh[t]).astype(F32)).astype(F32)
    return O, l


def _finish(O, l):
    inv = (F32(1) / l).astype(F32)
    return torch.from_numpy((O * inv[:, None]).astype(F32)).to(R.BF)


def _merge(parts, refs):
    """attn_merge_kernel in fp32, parts in order: w_p = exp2(m_p - m), l = sum w_p l_p, wgt = w_p / l, acc += wgt_p * O_p."""
    m = np.max(np.stack(refs), axis=0)
    wp = [np.exp2((r - m).astype(F32), dtype=F32) for r in refs]
    l = np.zeros_like(parts[0][1])
    for (O, lp), w in zip(parts, wp):
        l = (l + (w * lp).astype(F32)).astype(F32)
    inv = (F32(1) / l).astype(F32)
    acc = np.zeros_like(parts[0][0])
    for (O, lp), w in zip(parts, wp):
        acc = (acc + ((w * inv).astype(F32)[:, None] * O).astype(F32)).astype(F32)
    return torch.from_numpy(acc).to(R.BF)


def _kinds(c, table, h, rows):
    """bool [rows]: ordinary rows (not a probe, not a spike row)"""
    special = {r for (hh, r) in table if hh == h} | ({R.SPIKE_A, R.SPIKE_B} if c.spike and h == 0 else set())
    return torch.tensor([int(r) not in special for r in rows])


def test_scale_folds_to_one():
    c = np.float32(R.SCALE_LN2) * np.float32(1.4426950408889634)
    assert c.dtype == np.float32 and c == np.float32(1.0)
    assert np.float32(np.log(2)) == np.float32(R.SCALE_LN2)
    for case in R.CASES:                          # c = 1 / cdiv exactly, and a raw q times cdiv is still exact in bf16
        cc = np.float32(case.scale) * np.float32(1.4426950408889634)
        assert cc.dtype == np.float32 and cc * np.float32(case.cdiv) == np.float32(1.0) and case.cdiv in (1, 8)
        if case.cdiv > 1:
            q = R.case_operands(case)[0]
            qd = R.q_buffer(case, q, "cpu")[:case.Lq, :case.d].float()
            assert torch.equal(qd, q.float() * (1 if case.variant == 4 else case.cdiv))
    assert {c.variant for c in R.CASES if c.cdiv > 1} == {1, 3, 4} and any(c.cdiv > 1 and c.split for c in R.CASES)


def test_bf16_rne_is_one_rounding_to_nearest_even():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(200000, dtype=torch.float64, generator=g) * torch.exp2(torch.randint(-30, 30, (200000,), generator=g).double())
    m, e = torch.frexp(x)
    assert torch.equal(R.bf16_rne(x), torch.ldexp(torch.round(m * 256.0), e - 8))           # (torch.round: half to even)
    t = torch.tensor([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8 - 2.0 ** -40], dtype=torch.float64)
    assert R.bf16_rne(t).tolist() == [0.0, -0.0, 1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7, 1.0]
    assert torch.equal(R.bf16_rne(x).float().to(R.BF).double(), R.bf16_rne(x))                 # on the bf16 grid


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_case_is_exact(c):
    q, K, V, table = R.case_operands(c)
    plan = R.plan_restated(c, 32)
    assert plan[0] == c.kernel and plan[1] == (c.pages_walked or c.n_pages) and (plan[5] > 1) == c.split, (plan, "the shape no longer reaches the path it is here for")
    for name, quantum, bound in R.exactness_bounds(c):
        assert bound / quantum < 2.0 ** 24, (name, bound)
    for t in (q, K, V):
        assert torch.equal(t.float().to(R.BF), t) and bool((t.float() == t.float().round()).all())
    assert float(K.float().abs().max()) <= 1 and float(V.float().abs().max()) <= 3
    w = R.key_weights(c, "cpu")
    eps = R.eps(c, plan[5])
    parts = R.split_parts(c, plan[5]) if plan[5] > 1 else None
    walk = [k for pg in R.layout(c).walk for k in pg]
    assert sorted(walk) == list(range(c.n_keys))
    n_amb = n_all = 0
    for h, rows, in_parts in _sample(c, plan):
        s = R.scores(c, q, K, h, rows)
        Vh = V[:, h * R.HD:(h + 1) * R.HD]
        x, A = R.softmax_ref(c, s, Vh, w, parts if in_parts else None)
        delta = eps * A
        amb = R.ambiguous(x, delta)
        n_amb, n_all = n_amb + int(amb.sum()), n_all + amb.numel()
        ordinary = _kinds(c, table, h, rows)
        # ---- integer scores within the spread
        assert bool((s == s.round()).all())
        so = s[ordinary]
        if len(so) and c.copies > 1:
            # the weighted key stays under the row maximum, so the maximum stays an integer
            # (or it is the maximum and its bias log2(copies) is an integer)
            assert bool((so[:, -1] == c.tail).all()) and (c.tail + np.log2(c.copies) < 1 or (c.copies == 2 and c.tail == 5))
            assert c.n_keys == 1 or (bool((so[:, 0] == R.HEAD_SCORE).all()) and float(so[:, :-1].abs().max()) <= R.SPREAD / 2)
        elif len(so):
            assert float(so.abs().max()) <= R.SPREAD / 2 and float((so.max(1).values - so.min(1).values).max()) <= R.SPREAD
        # ---- what fp32 drops on the special rows
        for i, r in enumerate(rows.tolist()):
            if (h, r) in table:
                t = table[(h, r)]
                rest = torch.cat([s[i, :t], s[i, t + 1:]])
                assert s[i, t] == 40 and (rest.numel() == 0 or float(rest.max()) <= 0)
                assert 6 * c.n_keys * 2.0 ** -40 < 2.0 ** -26
                assert torch.equal(R.bf16_rne(x[i]), Vh[t].double()) and bool((Vh[t] != 0).all()), (h, r, t)
        if c.spike and h == 0:
            ia, ib = rows.tolist().index(R.SPIKE_A), rows.tolist().index(R.SPIKE_B)
            top_a, top_b = s[ia].topk(2).values, s[ib].topk(3).values
            assert top_a[0] == 200 and top_a[1] <= 0 and top_b.tolist()[:2] == [35, 20] and top_b[2] <= -70
            assert c.n_keys * 2.0 ** -70 < 2.0 ** -60
            first4 = s[ia, :4 * R.KVB].max()
            assert s[ia].argmax() // R.KVB == 6 and s[ia].max() - max(first4, s[ib, :4 * R.KVB].max()) - 64 > 100      # FAST cannot hold it
            assert s[ib].topk(2).indices.tolist() == [5 * 64 + 29, 3 * 64 + 29]
        # ---- fp32 emulation: O and l exact under every reference, tile size and order (ordinary rows); the normalised result of every
        # row inside its candidates
        sn, Vn, wn = s.numpy(), Vh.float().numpy(), w.numpy()
        mx = sn.max(axis=1)
        O64 = (np.exp2(sn - mx[:, None]) * wn) @ Vn.astype(np.float64)
        l64 = (np.exp2(sn - mx[:, None]) * wn).sum(axis=1)
        om = ordinary.numpy()
        exact = c.copies <= 1                       # (the weighted key's p is an approximation: attn_ref's COPIES_EPS)
        for ts in (32, 64):
            for keys in (walk, walk[::-1]):
                for ref in ((np.zeros_like(mx), mx, mx + 64) if not c.spike else (mx, mx + 64)):
                    if in_parts:
                        done, refs = [], []
                        for pk in parts:
                            rp = sn[:, pk].max(axis=1) + 64
                            kk = [k for k in keys if k in set(pk)]
                            Op, lp = _emulate(sn, Vn, wn, rp, kk, ts)
                            O64p = np.exp2(sn[:, pk] - rp[:, None]) @ Vn[pk].astype(np.float64)
                            assert np.array_equal(Op[om].astype(np.float64), O64p[om]) and np.array_equal(lp[om].astype(np.float64), np.exp2(sn[:, pk] - rp[:, None]).sum(1)[om])
                            done.append((Op, lp))
                            refs.append(rp)
                        got = _merge(done, refs)
                    else:
                        use = np.where(om, ref, mx)                 # probe / spike rows: the row max (anything else only drops less)
                        O, l = _emulate(sn, Vn, wn, use, keys, ts)
                        if exact:
                            scale = np.exp2(use - mx)
                            assert np.array_equal(O[om].astype(np.float64) * scale[om, None], O64[om])
                            assert np.array_equal(l[om].astype(np.float64) * scale[om], l64[om])
                        got = _finish(O, l)
                    bad = R.outside(got, x, delta)
                    assert int(bad.sum()) == 0, (ts, int(bad.sum()), bad.nonzero()[:4].tolist())
        # ---- each error class moves at least one element outside its candidates
        as_out = lambda xm: R.bf16_rne(xm).float().to(R.BF)
        moved = lambda xm: int(R.outside(as_out(xm), x, delta).sum())
        if ordinary.any() and c.n_keys > 1:
            keep = [k for k in range(c.n_keys) if k != c.n_keys // 2]
            assert moved(R.softmax_ref(c, s[:, keep], Vh[keep], w[keep])[0]) > 0, "one key dropped"
            Vs = Vh.clone()
            j = next(j for j in range(c.n_keys - 1) if not torch.equal(Vh[j], Vh[j + 1]) and j // R.KVB == (j + 1) // R.KVB)
            Vs[[j, j + 1]] = Vh[[j + 1, j]]
            assert moved(R.softmax_ref(c, s, Vs, w)[0]) > 0, "two V rows of one tile swapped"
        if ordinary.any() and any(len(pg) % R.KVB for pg in R.layout(c).walk):
            s0 = torch.cat([s, torch.zeros(len(rows), 1, dtype=s.dtype)], 1)
            V0 = torch.cat([Vh, torch.zeros(1, R.HD, dtype=Vh.dtype)])
            assert moved(R.softmax_ref(c, s0, V0, torch.cat([w, torch.ones(1, dtype=w.dtype)]))[0]) > 0, "one zero row admitted after a ragged page"
        if c.copies > 1 and c.n_keys > 1:           # (a single key: its weight cancels)
            w1 = w.clone()
            w1[-1] += 1
            assert moved(R.softmax_ref(c, s, Vh, w1)[0]) > 0, "copies off by one"
        if in_parts:
            p = torch.exp2(s - s.max(1, keepdim=True).values)
            l_less = p.sum(1, keepdim=True) - p[:, parts[0]].sum(1, keepdim=True)
            assert moved((p @ Vh.double()) / l_less) > 0, "one split part's l omitted from the merge"
    assert n_amb <= R.AMBIGUITY_CAP * n_all, (n_amb, n_all)


def test_probes_of_the_three_variants_visit_every_target():
    shapes = {}
    for c in R.CASES:
        if c.Lq == 64 and c.H == 1 and not c.copies and not c.split_groups and c.cdiv == 1:
            shapes.setdefault((c.n_pages, c.page_rows, c.layout), []).append(c)
    assert len(shapes) == 15
    for cs in shapes.values():
        assert sorted(c.variant for c in cs) == [1, 3, 4]
        seen = set()
        for c in cs:
            seen |= set(R.case_operands(c)[3].values())
        pool = set(R.target_pool(cs[0]))
        assert seen == pool, (cs[0].name, sorted(pool - seen))
        S = cs[0].page_rows
        assert {k % S % 64 for k in pool} == set(range(min(S, 64)))
        assert {p * S for p in range(cs[0].n_pages)} | {p * S + S - 1 for p in range(cs[0].n_pages)} <= pool


@pytest.mark.parametrize("c", [c for c in R.CASES if c.w64], ids=[c.name for c in R.CASES if c.w64])
def test_lane_partners_are_of_one_kind(c):
    """attn_w64_kernel's FAST reference is shared by rows r and r ^ 32 (clamped to Lq - 1): a probe next to an ordinary row would push
    the ordinary row's sum under the window and the block into the GENERAL pass."""
    probes = set(R.probe_rows(c))
    for r in range(-(-c.Lq // 64) * 64):
        a, b = min(r, c.Lq - 1), min(r ^ 32, c.Lq - 1)
        assert (a in probes) == (b in probes), (r, a, b)


@pytest.mark.parametrize("c", [c for c in R.CASES if c.w64], ids=[c.name for c in R.CASES if c.w64])
def test_fast_pass_holds_where_the_case_says_so(c):
    """The counter of redone blocks, predicted from the scores: no block of a plain case is redone (probes, their lane partners and the
    rows clamped past Lq included), the spike block is.  A split tail block is different: a probe whose target lies in another part
    sees nothing above -30 in its own while its lane partner may hold 40, so such parts go to the GENERAL pass -- and only those (the
    GPU test asserts the counter against this prediction over all heads).  (Large cases: the first and the last head.)"""
    q, K, _, _ = R.case_operands(c)
    plan = R.plan_restated(c, 32)
    heads = None if c.Lq < 2000 else sorted({0, c.H - 1})
    got = R.predict_redone(c, q, K, plan, heads=heads)
    if plan[5] == 1:
        assert got == (c.stats[0][0] if c.stats else 0)
    else:
        assert 0 < got <= plan[5] * sum(h in heads for h, _ in R.tail_items(c, 32, plan[4]))
        assert R.predict_redone(c, q, K, plan[:4] + [0, 1, 0, 0], heads=heads) == 0


@pytest.mark.parametrize("c", R.CASES[::7], ids=IDS[::7])
def test_geometry(c):
    """Pages do not overlap, every page is followed by canary rows ("gaps") or by the next page ("contig", "groups"), the allocation ends
    in END_ROWS canary rows, and the canaries are non-finite in V and huge in K."""
    q, K, V, _ = R.case_operands(c)
    kb, vb = R.kv_buffers(c, K, V, "cpu")
    lay = R.layout(c)
    owner = torch.full((lay.rows,), -1)
    for p, r0 in enumerate(lay.page_row0):
        assert bool((owner[r0:r0 + c.page_rows] == -1).all())
        owner[r0:r0 + c.page_rows] = p
        assert torch.equal(kb[r0:r0 + c.page_rows, :c.d], K[p * c.page_rows:(p + 1) * c.page_rows])
        if c.layout == "gaps":
            assert bool((owner[r0 + c.page_rows:r0 + c.page_rows + R.GAP_ROWS] == -1).all())
    assert bool((owner[-R.END_ROWS:] == -1).all())
    free = owner == -1
    assert bool(torch.isnan(vb[free].float()).all()) and bool((kb[free].float() == R.K_CANARY).all())
    assert bool(torch.isnan(vb[:, c.d:].float()).all())
    qb = R.q_buffer(c, q, "cpu")
    assert bool(torch.isnan(qb[c.Lq:].float()).all()) and bool(torch.isnan(qb[:, c.d:].float()).all())
    assert c.ldq % 8 == 0 and c.ldo % 8 == 0 and c.ldk % 8 == 0 and all((r0 * c.ldk * 2) % 16 == 0 for r0 in lay.page_row0)
