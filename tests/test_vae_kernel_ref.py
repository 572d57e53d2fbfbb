"""Self-test of tests/vae_kernel_ref.py (CPU): the bf16 arithmetic, the layout builders, the references against plain conv3d /
conv2d, the product's fragment packer against the formula of include/mmpl_hip.h, and the input conditions of every parametrised
case of the GPU files (exact regime below 2^24, ambiguous set under 1 %, every kernel covered)."""
import pytest
import torch
import torch.nn.functional as F

import vae_kernel_ref as R
from mmpl_amd.vae import VaeEngine


def test_rbf_is_bf16_round_to_nearest_even():
    g = R._rng("rbf")
    x = torch.cat([torch.randn(20000, generator=g) * 100, torch.tensor([0.0, 257.0, 259.0, -257.0, 1.00390625, 3.0e38, 1e-30])])
    assert torch.equal(R.rbf(x.double()), x.to(torch.bfloat16).double())
    # midpoints are flagged, representable values and clear misses are not
    t = torch.tensor([257.0, 257.0 + 2.0 ** -12, 256.0, 258.0, 257.5, 0.0], dtype=R.F64)
    assert R.near_tie(t).tolist() == [True, True, False, False, False, False]
    # one exact fp32 operation: the midpoint itself is decided by ties-to-even, only its open neighbourhood is ambiguous
    t = torch.tensor([257.0, 257.0 + 2.0 ** -16, 257.0 - 2.0 ** -16, 257.0 + 2.0 ** -14, 256.0], dtype=R.F64)
    assert R.near_tie(t, R.TIE_REL_FP32, exact_ok=True).tolist() == [False, True, True, False, False]
    assert R.rbf(torch.tensor([257.0, 259.0], dtype=R.F64)).tolist() == [256.0, 260.0]
    a = torch.tensor([1.0, -1.0, 0.0, 2.0], dtype=torch.bfloat16)
    b = torch.tensor([1.0078125, -1.0078125, -0.0, 1.9921875], dtype=torch.bfloat16)
    assert (R.bf16_line(a) - R.bf16_line(b)).abs().tolist() == [1, 1, 0, 1]


def test_layout_builders_round_trip():
    g = R._rng("layout")
    x = R._ints(g, (1, 8, 3, 4, 5), 255)
    v = R.to_cl(x)
    assert v.shape == (3, 4, 5, 8) and torch.equal(R.from_cl(v), x)
    vol = R.embed(v, 6, 7, 9, 16, 2, 1, 3, fill=7.0)
    assert torch.equal(R.extract(vol, 3, 4, 5, 8, 2, 1, 3), v) and R.outside_is(vol, 3, 4, 5, 8, 2, 1, 3, fill=7.0)
    vol[0, 0, 0, 0] = 1.0
    assert not R.outside_is(vol, 3, 4, 5, 8, 2, 1, 3, fill=7.0)
    assert R.ring_slots(6, 4, 6) == [4, 5, 0, 1, 2, 3]
    ring = R.to_ring(v, 5, 3, fill=7.0)
    assert torch.equal(R.from_ring(ring, 3, 3), v) and bool((ring[[1, 2]].double() == 7.0).all())
    assert torch.equal(ring[3], v[0]) and torch.equal(ring[0], v[2])
    p = R.to_plain(x, 12, fill=7.0)
    assert p.shape == (60, 12) and torch.equal(p[:, :8], v.reshape(-1, 8)) and bool((p[:, 8:].double() == 7.0).all())
    f = R._ints(g, (2, 8, 4, 5), 255)
    fr = R.pad_frames(f)
    assert fr.shape == (2, 6, 7, 8) and torch.equal(R.unpad_frames(fr), f) and float(fr[:, 0].abs().max()) == 0.0


def test_reference_on_padded_layout_equals_plain_conv():
    g = R._rng("conv")
    x, w, bias = R._ints(g, (1, 32, 3, 6, 10), 3), R._ints(g, (8, 32, 3, 3, 3), 1), R._ints(g, (8,), 16)
    # a video's first chunk through the layouts: causal padding = two zero frames in front, one zero pixel all round, frames in ring slots
    xp = F.pad(x, (1, 1, 1, 1, 2, 0))
    ring = R.to_ring(R.to_cl(xp), 7, 5)
    y, acc = R.vae_conv_ref(R.from_cl(R.from_ring(ring, 5, 5)), w, bias)
    plain = F.conv3d(F.pad(x, (0, 0, 0, 0, 2, 0)), w, bias, padding=(0, 1, 1))
    assert torch.equal(acc + bias.view(1, -1, 1, 1, 1), plain) and torch.equal(y, R.rbf(plain))
    # the down-sampler: ZeroPad2d((0, 1, 0, 1)) + Conv2d(3, stride 2) per frame
    w2 = R._ints(g, (8, 32, 1, 3, 3), 1)
    y2, _ = R.vae_conv_ref(F.pad(x, (0, 1, 0, 1)), w2, bias, (1, 2, 2))
    per_frame = torch.stack([F.conv2d(F.pad(x[:, :, t], (0, 1, 0, 1)), w2[:, :, 0], bias, stride=2) for t in range(3)], dim=2)
    assert torch.equal(y2, R.rbf(per_frame))
    # TAEHV: nearest x2 folded in front of a padded 3x3, two sources as one K axis, skip and ReLU before the one rounding
    x0, x1, wt = R._ints(g, (2, 32, 3, 4), 3), R._ints(g, (2, 32, 3, 4), 3), R._ints(g, (64, 64, 3, 3), 1)
    skip = R._ints(g, (2, 64, 6, 8), 255)
    yt, _ = R.taehv_conv_ref(x0, x1, wt, None, skip, True, True)
    up = F.interpolate(torch.cat([x0, x1], 1), scale_factor=2, mode="nearest")
    assert torch.equal(yt, R.rbf(torch.relu(F.conv2d(up, wt, None, padding=1) + skip)))


def test_frag_pack_matches_header_formula():
    """element (n, tap, c) at ((((c / 32) * taps + tap) * (Npad / 16) + n / 16) * 4 + (c % 32) / 8) * 16 + n % 16) * 8 + c % 8"""
    N, taps, Cin = 40, 9, 64
    w2d = torch.arange(N * taps * Cin, dtype=torch.float32).reshape(N, taps * Cin)
    packed = VaeEngine._frag_pack(w2d, Cin)
    npad = 48
    assert packed.numel() == Cin // 32 * taps * npad * 32
    n, tap, c = torch.meshgrid(torch.arange(N), torch.arange(taps), torch.arange(Cin), indexing="ij")
    idx = ((((c // 32) * taps + tap) * (npad // 16) + n // 16) * 4 + (c % 32) // 8) * 16 + n % 16
    idx = idx * 8 + c % 8
    assert torch.equal(packed[idx.reshape(-1)], w2d.reshape(-1))
    rest = torch.ones(packed.numel(), dtype=torch.bool)
    rest[idx.reshape(-1)] = False
    assert float(packed[rest].abs().max()) == 0.0


@pytest.mark.parametrize("c", R.CONV_CASES, ids=lambda c: c.name)
def test_conv_case_conditions(c):
    b = R.build_conv(c)                                            # asserts integers and sum|a||w| + |bias| + |res| < 2^24
    assert b["y"].shape == (1, c.N, c.To, c.Ho, c.Wo)
    if c.regime != "gauss":
        assert b["exact_max"] < R.EXACT_LIMIT
        assert float(b["x"].min()) < 0 < float(b["x"].max()) and float(b["y"].min()) < 0 < float(b["y"].max())
        if c.regime in ("act8", "w8"):                             # full 8-bit mantissas on one operand
            full = b["x"] if c.regime == "act8" else b["w"]
            assert float(full.abs().max()) == 255.0
    if c.fuse:
        assert float(b["norm_amb"].double().mean()) < 0.01
        assert float(b["norm"].min()) < 0 < float(b["norm"].max())
    if c.ring:
        assert c.ring[0] >= b["Tp"] and c.To + c.k[0] - 1 <= 8


def test_conv_cases_cover_every_kernel_and_the_ring_wrap():
    exact = [c for c in R.CONV_CASES if c.regime != "gauss"]
    for k in (R.K_IGEMM3, R.K_IGEMM4, R.K_HALO6, R.K_HALO1):
        regimes = {c.regime for c in exact if c.kernel == k}
        assert {"act8", "w8"} <= regimes, (k, regimes)
        assert any(c.kernel == k for c in R.CONV_CASES if c.regime == "gauss")
    assert R.ring_slots(6, 4, 6) == [4, 5, 0, 1, 2, 3] and any(c.ring == (6, 4) and c.To == 4 for c in exact)
    assert any(c.fuse and R.ring_slots(c.fuse[0], c.fuse[1] + 2, c.To) != sorted(R.ring_slots(c.fuse[0], c.fuse[1] + 2, c.To)) for c in exact)


@pytest.mark.parametrize("c", R.TAEHV_CASES, ids=lambda c: c.name)
def test_taehv_case_conditions(c):
    b = R.build_taehv(c)
    assert b["y"].shape == (c.T, 3 if c.head else c.Nw, c.Ho, c.Wo)
    if c.regime != "gauss":
        assert b["exact_max"] < R.EXACT_LIMIT
        pre = b["y"] if not c.relu else b["xin"]
        assert float(pre.min()) < 0 < float(pre.max())
        if c.relu:
            assert 0.2 < float((b["y"] == 0).double().mean()) < 0.8          # ReLU sees both sides
        full = b["run"] if c.regime == "act8" else b["w"]
        assert float(full.abs().max()) == 255.0


@pytest.mark.parametrize("C_,npix,mode", R.NORM_CASES)
def test_norm_case_conditions(C_, npix, mode):
    b = R.build_norm(C_, npix, mode)
    assert float(b["amb"].double().mean()) < 0.01
    assert float(b["x"].abs().max()) >= 240.0 and float(b["ref"].min()) < 0 < float(b["ref"].max())
    if mode == "copy":
        assert torch.equal(b["ref"], b["x"]) and not b["amb"].any()


def test_zprep_case_conditions():
    b = R.build_zprep()
    assert float(b["amb"].double().mean()) < 0.01
    assert float(b["z"].abs().max()) == 15.0 and float(b["ref"].min()) < 0 < float(b["ref"].max())
    # the case does meet exact midpoints in + mean (decided by ties-to-even, not ambiguous) and inexact quotients in channels 0 and 1
    q = R.rbf(b["z"].permute(0, 2, 3, 1) / b["inv"])
    assert R.near_tie(q + b["mean"], 0.0).any()
    assert not torch.equal(q[..., :2] * b["inv"][:2], b["z"].permute(0, 2, 3, 1)[..., :2])


def test_mu_out_case_conditions():
    b = R.build_mu_out()
    assert float(b["amb"].double().mean()) < 0.01
    assert b["ref"].shape == (b["F"], 16, b["h"], b["w"]) and float(b["ref"].min()) < 0 < float(b["ref"].max())
    assert float(b["enc"].abs().max()) == 255.0


@pytest.mark.parametrize("h,w", R.TAEHV_PREP_CASES)
def test_taehv_prep_case_conditions(h, w):
    b = R.build_taehv_prep(h, w)
    assert float(b["amb"].double().mean()) < 0.01
    assert float(b["ref"].min()) < -2.5 and float(b["ref"].max()) > 2.5            # into the saturated part of tanh, both signs
    assert float(b["ref"].abs().max()) <= 3.0


def test_norm_reference_against_float32_torch():
    """the chain of vae.py:51-54 in torch bf16 tensors agrees with the float64 reference outside the ambiguous set"""
    b = R.build_norm(96, 297, "norm")
    x = R.bf16_exact(b["x"])
    y = torch.nn.functional.normalize(x, dim=-1) * (96 ** 0.5) * R.bf16_exact(b["gamma"])
    d = (R.bf16_line(y) - R.bf16_line(R.bf16_exact(b["ref"]))).abs()
    assert float((d > 1).double().mean()) < 0.01                    # torch's own normalize rounds at other points: a sanity check only


def _gauss_rounding_share(y64, acc_bound):
    """the share of |y - y64| <= 2^-9 |y64| + acc_bound that the correctly rounded bf16(y64) uses, worst element"""
    return float(((R.rbf(y64) - y64).abs() / (2.0 ** -9 * y64.abs() + acc_bound).clamp_min(1e-300)).max())


def test_gaussian_bound_is_satisfiable_on_the_deep_cases_only():
    """The Gaussian-data bound's 2^-9 |y| is half of what round-to-nearest bf16 can cost (2^-8 |y|, 8 significant bits).  On the small
    cases the correctly rounded float64 result breaks it whatever a kernel does; on the deep-K cases, where the GPU files assert
    it, bf16(y64) stays under GAUSS_DEEP_MARGIN of it on every element."""
    for c in [c for c in R.CONV_CASES if c.regime == "gauss"]:
        b = R.build_conv(c)
        y64 = b["acc"] + b["bias"].view(1, -1, 1, 1, 1)
        share = _gauss_rounding_share(y64, R.accum_bound(b["xp"], b["w"], c.s))
        assert float(((R.rbf(y64) - y64).abs() / (2.0 ** -8 * y64.abs()).clamp_min(1e-300)).max()) <= 1.0
        if R.is_deep(c):
            assert share <= R.GAUSS_DEEP_MARGIN, (c.name, share)
        elif c.N > 4:
            assert share > 1.0, (c.name, share)
    for c in [c for c in R.TAEHV_CASES if c.regime == "gauss"]:
        b = R.build_taehv(c)
        y64 = F.conv2d(b["xin"], b["w"], None) + (b["bias"].view(1, -1, 1, 1) if c.bias else 0.0)
        y64 = y64.clamp_min(0.0) if c.relu else y64
        share = _gauss_rounding_share(y64, R.accum_bound(b["xin"], b["w"]))
        assert (share <= R.GAUSS_DEEP_MARGIN) if R.is_deep(c) else (share > 1.0), (c.name, share)
    for k in (R.K_IGEMM3, R.K_IGEMM4, R.K_HALO6, R.K_HALO1):
        assert any(c.kernel == k and R.is_deep(c) for c in R.CONV_CASES)
    assert any(R.is_deep(c) and c.Nw % 64 == 0 for c in R.TAEHV_CASES) and any(R.is_deep(c) and c.Nw == 16 for c in R.TAEHV_CASES)
