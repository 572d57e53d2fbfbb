"""mmpl_taehv_decode and mmpl_taehv_encode -- through TaehvEngine.decode / decode_stream, TaehvEncoderEngine.encode / encode_stream
and through the C entries -- against the launch chain of tests/taehv_chain.py, bit for bit (-m gpu).

Every case runs the product twice on a CALLER-MADE workspace that is larger than mmpl_taehv[_enc]_workspace_bytes and is filled as a
whole with a NaN pattern before the video's first call: through the engine on 0x7FA5 and through the C entry on 0xFFB3.  The only
clearing is the library's own once-per-video clearing.  Every call of both runs must equal the same call of the TaehvHipOps chain
(one single-launch entry per op, every intermediate in a canary-tailed buffer of its own, one frame of memory per MemBlock, a
call's frames in one launch per layer) in EVERY BIT; the bytes past the stated workspace size must come back untouched and the
chain's canaries intact.  That the chain is the model is shown on the CPU (tests/test_taehv_chain_host.py).

Latents: 1 x 1 (every level a single clamped patch, the stride-2 conv at Ho = 1, 8 x 8 pixels), 3 x 5 (ragged at every level, 24 x
40 pixels = two patch columns), 9 x 13 (two patch rows already at the latent level, 104 pixel columns ragged against the 32-wide
patch).  Latent frames per call: 1, 2, 3, 4, 5, 7 one-shot (a partial group, a full one, 3 + 1, 3 + 3 + 1) and the streams [3, 1]
(a 1-frame call over the stale frames of a full group), [1, 3] (the reverse), [2, 2, 1], [1, 1, 1, 1, 1], [3, 2]; the encoder takes
the same times 4 pixel frames."""
import ctypes as C
import functools

import pytest
import torch

from mmpl_amd import _lib
from mmpl_amd.synthetic import philox_normal, taehv_encoder_state_dict, taehv_state_dict
from tests import taehv_chain as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT_A, PAT_B = 0x7FA5, 0xFFB3 - 0x10000        # two bf16 NaN patterns, as int16
EXTRA = 12288                                   # bytes the workspaces are larger by
LATS = [(1, 1), (3, 5), (9, 13)]
SPLITS = [(1,), (2,), (3,), (4,), (5,), (7,), (3, 1), (1, 3), (2, 2, 1), (1, 1, 1, 1, 1), (3, 2)]
_id = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _sd(big=False):
    sd = dict(taehv_state_dict(seed=5))
    sd.update(taehv_encoder_state_dict(seed=5))
    if big:                                     # the checkpoint of tests/test_taehv_gpu.py::test_patch_tgrow_layers: 2 * 256 TGrow rows
        g = torch.Generator().manual_seed(97)
        extra = (torch.randn(256, 256, 1, 1, generator=g) * (1.0 / 16)).to(torch.bfloat16)
        sd["decoder.7.conv.weight"] = torch.cat([extra, sd["decoder.7.conv.weight"]], 0)
    return sd


@functools.lru_cache(maxsize=None)
def _engine(kind, lat, big=False):
    from mmpl_amd.taehv import TaehvEncoderEngine, TaehvEngine
    eng = (TaehvEngine if kind == "dec" else TaehvEncoderEngine)(lat[0], lat[1], DEV)
    eng.load_state_dict(_sd(big))
    return eng


def _chain(lat, big=False):
    ops = TC.TaehvHipOps(_lib.load(), DEV)
    return TC.TaehvChain(_sd(big), lat[0], lat[1], ops), ops


def _latents(lat, n, seed=47):
    return (philox_normal([n, 16, lat[0], lat[1]], seed) * 1.5).to(torch.bfloat16)


def _pixels(lat, n, u8, seed=48):
    px = philox_normal([n, 3, 8 * lat[0], 8 * lat[1]], seed).mul(0.25).add(0.5).clamp(0, 1)
    return (px * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() if u8 else px


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _nan_ws(kind, eng, pattern):
    """-> (a workspace EXTRA bytes larger than the library asks for, filled as a whole with `pattern`; the size it asks for)"""
    lib = _lib.load()
    need = (lib.mmpl_taehv_workspace_bytes if kind == "dec" else lib.mmpl_taehv_enc_workspace_bytes)(eng._h)
    assert need > 0 and need % 2 == 0
    return torch.full(((need + EXTRA) // 2,), pattern, dtype=torch.int16, device=DEV).view(torch.uint8), need


def _tail_ok(ws, need, pattern):
    return bool((ws[need:].view(torch.int16) == pattern).all())


def _calls(x, split, mult=1):
    out, f0 = [], 0
    for n in split:
        out.append(x[f0:f0 + mult * n])
        f0 += mult * n
    assert f0 == x.shape[0]
    return out


# ------------------------------------------------------------------------------------------------ the three routes
def _chain_calls(kind, ch, calls, fmt=0):
    outs = [ch.decode(c, fmt) if kind == "dec" else ch.encode(c) for c in calls]
    assert ch.ops.canaries_intact(), "a launch of the chain wrote past its buffer"
    return outs


def _engine_calls(kind, eng, calls, fmt=0, reset=True):
    """One video through the engine: one call -> the one-shot method, several -> clear_cache and the streamed method.  With
    reset=False the calls continue the engine's current video."""
    outs = []
    if reset and len(calls) == 1:
        outs.append(eng.decode(calls[0], out_format=("float", "uint8")[fmt]) if kind == "dec" else eng.encode(calls[0]))
    else:
        if reset:
            eng.clear_cache()
        for c in calls:
            outs.append(eng.decode_stream(c, out_format=("float", "uint8")[fmt]) if kind == "dec" else eng.encode_stream(c))
    torch.cuda.synchronize()
    return outs


def _c_calls(kind, eng, calls, ws, fmt=0, reset=True):
    """One video through mmpl_taehv_decode / mmpl_taehv_encode on the engine's handle and the workspace `ws`."""
    lib, lat = _lib.load(), (eng.lat_h, eng.lat_w)
    H, W = 8 * lat[0], 8 * lat[1]
    if reset:
        _lib.check((lib.mmpl_taehv_reset if kind == "dec" else lib.mmpl_taehv_enc_reset)(eng._h), "reset")
    outs = []
    for c in calls:
        n = c.shape[0]
        n_out = C.c_int(0)
        if kind == "dec":
            x = c.to(device=DEV, dtype=torch.bfloat16).contiguous()
            out = torch.zeros((4 * n, H, W, 3), dtype=torch.uint8, device=DEV) if fmt == 1 else \
                torch.full((4 * n, 3, H, W), float("nan"), dtype=torch.float32, device=DEV)
            _lib.check(lib.mmpl_taehv_decode(eng._h, _lib.ptr(x), n, _lib.ptr(out), fmt, C.byref(n_out), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()), "mmpl_taehv_decode")
            assert n_out.value == 4 * n
        else:
            u8 = c.dtype == torch.uint8
            x = c.to(device=DEV, dtype=torch.uint8 if u8 else torch.float32).contiguous()
            out = torch.full((n // 4, 16, lat[0], lat[1]), float("nan"), dtype=torch.bfloat16, device=DEV)
            _lib.check(lib.mmpl_taehv_encode(eng._h, _lib.ptr(x), int(u8), n, _lib.ptr(out), C.byref(n_out), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()), "mmpl_taehv_encode")
            assert n_out.value == n // 4
        torch.cuda.synchronize()
        outs.append(out)
    return outs


def _both_routes_equal_chain(kind, lat, calls, fmt=0, big=False):
    eng = _engine(kind, lat, big)
    ch, _ = _chain(lat, big)
    want = _chain_calls(kind, ch, calls, fmt)
    if not (kind == "dec" and fmt == 1):
        assert all(bool(torch.isfinite(w.float()).all()) for w in want), "the chain read something no launch wrote"
    try:
        ws, need = _nan_ws(kind, eng, PAT_A)
        eng.clear_cache()
        eng._ws = ws
        got = _engine_calls(kind, eng, calls, fmt)
        for i, (g, w) in enumerate(zip(got, want)):
            assert _same_bits(g, w), f"engine, call {i} of {[c.shape[0] for c in calls]} differs from the launch chain"
        assert _tail_ok(ws, need, PAT_A), "bytes past the stated workspace size were written"
        ws, need = _nan_ws(kind, eng, PAT_B)
        got = _c_calls(kind, eng, calls, ws, fmt)
        for i, (g, w) in enumerate(zip(got, want)):
            assert _same_bits(g, w), f"C entry, call {i} of {[c.shape[0] for c in calls]} differs from the launch chain"
        assert _tail_ok(ws, need, PAT_B), "bytes past the stated workspace size were written"
    finally:
        eng._ws = None
        eng.clear_cache()


# ------------------------------------------------------------------------------------------------ decode / encode, one-shot and streamed
@pytest.mark.parametrize("fmt", [0, 1], ids=["float", "uint8"])
@pytest.mark.parametrize("split", SPLITS, ids=_id)
@pytest.mark.parametrize("lat", LATS, ids=lambda v: "x".join(map(str, v)))
def test_decode_equals_chain(lat, split, fmt):
    _both_routes_equal_chain("dec", lat, _calls(_latents(lat, sum(split)), split), fmt)


@pytest.mark.parametrize("u8", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("split", SPLITS, ids=_id)
@pytest.mark.parametrize("lat", LATS, ids=lambda v: "x".join(map(str, v)))
def test_encode_equals_chain(lat, split, u8):
    _both_routes_equal_chain("enc", lat, _calls(_pixels(lat, 4 * sum(split), u8), split, 4))


@pytest.mark.parametrize("split", [(3, 1), (4,)], ids=_id)
def test_decode_oversized_tgrow_equals_chain(split):
    """A checkpoint whose first TGrow has 2 * 256 rows: the engine's patch_tgrow_layers and the chain's own row choice agree."""
    lat = (3, 5)
    _both_routes_equal_chain("dec", lat, _calls(_latents(lat, sum(split)), split), 0, big=True)
    ch, _ = _chain(lat, big=False)
    chb, _ = _chain(lat, big=True)
    z = _latents(lat, 1)
    assert _same_bits(ch.decode(z), chb.decode(z)), "the kept rows are the original weight"


# ------------------------------------------------------------------------------------------------ two videos in one engine
@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_reset_starts_over_and_no_reset_continues(kind):
    """Video 1 in calls of [2, 1]; then, WITHOUT reset, a further call continues it and equals the continued chain; then reset and
    a second video in calls of [1, 2] on the same engine and workspace pointer equals a FRESH chain."""
    lat, mult = (3, 5), 1 if kind == "dec" else 4
    eng = _engine(kind, lat)
    x1 = _latents(lat, 5, 51) if kind == "dec" else _pixels(lat, 20, False, 52)
    x2 = _latents(lat, 3, 53) if kind == "dec" else _pixels(lat, 12, True, 54)
    c1, c2 = _calls(x1, (2, 1, 2), mult), _calls(x2, (1, 2), mult)
    ch, _ = _chain(lat)
    want1 = _chain_calls(kind, ch, c1)
    fresh, _ = _chain(lat)
    want2 = _chain_calls(kind, fresh, c2)
    ch.reset()
    want2_reset = _chain_calls(kind, ch, c2)
    assert all(_same_bits(a, b) for a, b in zip(want2, want2_reset)), "the chain's reset() is a fresh chain"
    try:
        for route in ("engine", "c"):
            ws, need = _nan_ws(kind, eng, PAT_A if route == "engine" else PAT_B)
            if route == "engine":
                eng.clear_cache()
                eng._ws = ws
                got1 = _engine_calls(kind, eng, c1[:2]) + _engine_calls(kind, eng, c1[2:], reset=False)
                got2 = _engine_calls(kind, eng, c2)
            else:
                got1 = _c_calls(kind, eng, c1[:2], ws) + _c_calls(kind, eng, c1[2:], ws, reset=False)
                got2 = _c_calls(kind, eng, c2, ws)
            for i, (g, w) in enumerate(zip(got1, want1)):
                assert _same_bits(g, w), f"{route}: video 1, call {i}"
            for i, (g, w) in enumerate(zip(got2, want2)):
                assert _same_bits(g, w), f"{route}: video 2 after reset, call {i}"
            assert _tail_ok(ws, need, PAT_A if route == "engine" else PAT_B)
    finally:
        eng._ws = None
        eng.clear_cache()


def test_uint8_pixels_equal_float_u_over_255():
    lat = (3, 5)
    eng = _engine("enc", lat)
    u = _pixels(lat, 8, True)
    a = eng.encode(u)
    b = eng.encode(u.permute(0, 3, 1, 2).to(torch.float32) / 255.0)
    torch.cuda.synchronize()
    assert _same_bits(a, b)
    ch, ops = _chain(lat)
    assert _same_bits(a, ch.encode(u)) and ops.canaries_intact()
