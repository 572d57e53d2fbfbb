"""mmpl_vae_decode, mmpl_vae_encode and mmpl_vae_stream_decode against the launch chain of tests/vae_chain.py, bit for bit (-m gpu).

Every case runs the product twice -- through VaeEngine, whose workspace arrives filled with the NaN pattern 0x7FA5, and through the
C entry with a LARGER workspace filled with another NaN pattern (0xFFB3), whose bytes past mmpl_vae_workspace_bytes must come back
untouched -- and demands that both outputs equal the VaeHipOps chain (one single-launch entry per op, every intermediate in a
canary-tailed buffer of its own, the temporal caches kept as two frames per conv) in EVERY BIT, with the chain's canaries intact.
That the chain is the model is shown on the CPU (tests/test_vae_chain_host.py).

Geometries: 6 x 10 (the suite's ragged one), 8 x 12, 8 x 8 (64 tokens = no score padding, every stage a multiple of the 8 x 32 halo
tile up to 64 x 64) and 3 x 5 (partial halo tiles in both directions at every stage, 15 attention tokens: padded to 64 for the P . V
GEMM and to 16 keys for the scores GEMM, whose N must be a multiple of 4)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from mmpl_amd import _lib
from mmpl_amd.synthetic import philox_normal, vae_state_dict
from tests import vae_chain as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = VC.MEAN, VC.STD
PAT_A, PAT_B = 0x7FA5, 0xFFB3 - 0x10000        # two bf16 NaN patterns, as int16
EXTRA = 12288                                   # bytes the second workspace is larger by


@functools.lru_cache(maxsize=None)
def _sd():
    return vae_state_dict(seed=3)


@functools.lru_cache(maxsize=None)
def _engine(lat):
    from mmpl_amd.vae import VaeEngine
    eng = VaeEngine(lat[0], lat[1], DEV)
    eng.load_state_dict(_sd())
    return eng


def _scales():
    return VC.latent_scales(MEAN, STD)


def _chain(lat, fuse=None):
    ops = VC.VaeHipOps(_lib.load(), DEV)
    return VC.VaeChain(_sd(), lat[0], lat[1], ops, fuse=fuse), ops


def _nan_ws(nbytes, pattern):
    assert nbytes % 2 == 0
    return torch.full((nbytes // 2,), pattern, dtype=torch.int16, device=DEV).view(torch.uint8)


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _tail_ok(ws, need):
    return bool((ws[need:].view(torch.int16) == PAT_B).all())


def _f16(v):
    return (C.c_float * 16)(*v)


def _latents(lat, n, seed):
    return philox_normal([n, 16, lat[0], lat[1]], seed)


def _pixels(lat, n, seed):
    return philox_normal([3, n, 8 * lat[0], 8 * lat[1]], seed).clamp(-1, 1)


# ------------------------------------------------------------------------------------------------ decode / encode
@pytest.mark.parametrize("lat,n", [((6, 10), 3), ((8, 12), 2), ((8, 8), 2), ((3, 5), 2)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_decode_equals_chain(lat, n):
    lib, eng = _lib.load(), _engine(lat)
    mean, inv = _scales()
    z = _latents(lat, n, 77)
    ch, ops = _chain(lat)
    want = ch.decode(z, mean, inv)
    assert ops.canaries_intact()
    need = lib.mmpl_vae_workspace_bytes(eng._h, 0)
    eng._ws[0] = _nan_ws(need, PAT_A)
    got = eng.decode(z, MEAN, STD)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got, want), "VaeEngine.decode differs from the launch chain"
    ws = _nan_ws(need + EXTRA, PAT_B)
    zd = z.to(device=DEV, dtype=torch.bfloat16).contiguous()
    out = torch.full_like(got, float("nan"))
    _lib.check(lib.mmpl_vae_decode(eng._h, _lib.ptr(zd), n, _f16(mean), _f16(inv), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "mmpl_vae_decode")
    torch.cuda.synchronize()
    assert _same_bits(out, want), "mmpl_vae_decode on another workspace differs from the launch chain"
    assert _tail_ok(ws, need), "bytes past mmpl_vae_workspace_bytes were written"


@pytest.mark.parametrize("lat,n", [((6, 10), 9), ((8, 8), 5), ((3, 5), 1)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_encode_equals_chain(lat, n):
    lib, eng = _lib.load(), _engine(lat)
    mean, inv = _scales()
    px = _pixels(lat, n, 78)
    ch, ops = _chain(lat)
    want = ch.encode(px, mean, inv)
    assert ops.canaries_intact()
    need = lib.mmpl_vae_workspace_bytes(eng._h, 1)
    eng._ws[1] = _nan_ws(need, PAT_A)
    got = eng.encode(px, MEAN, STD)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    assert _same_bits(got, want), "VaeEngine.encode differs from the launch chain"
    ws = _nan_ws(need + EXTRA, PAT_B)
    pd = px.to(device=DEV, dtype=torch.bfloat16).contiguous()
    out = torch.full_like(got, float("nan"))
    _lib.check(lib.mmpl_vae_encode(eng._h, _lib.ptr(pd), n, _f16(mean), _f16(inv), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "mmpl_vae_encode")
    torch.cuda.synchronize()
    assert _same_bits(out, want), "mmpl_vae_encode on another workspace differs from the launch chain"
    assert _tail_ok(ws, need), "bytes past mmpl_vae_workspace_bytes were written"


# ------------------------------------------------------------------------------------------------ stream
LAT_S = (6, 10)


def _chain_stream_calls(z, split, fmt, stream=None):
    """The chain's stream over `split` -> the output of every call."""
    mean, inv = _scales()
    if stream is None:
        ch, ops = _chain(LAT_S)
        stream = ch.stream()
    outs, f0 = [], 0
    for n in split:
        outs.append(stream.decode(z[f0:f0 + n], mean, inv, fmt))
        f0 += n
    assert stream.chain.ops.canaries_intact()
    return outs, stream


def _c_stream_calls(eng, z, split, fmt, pattern, extra, handle=None):
    """mmpl_vae_stream_decode over `split` on a NaN-filled workspace of its own -> (the output of every call, workspace, handle)."""
    lib = _lib.load()
    mean, inv = _scales()
    need = lib.mmpl_vae_workspace_bytes(eng._h, 0)
    if handle is None:
        handle = C.c_void_p()
        _lib.check(lib.mmpl_vae_stream_create(eng._h, C.byref(handle)), "mmpl_vae_stream_create")
    ws = _nan_ws(need + extra, pattern)
    H, W = 8 * LAT_S[0], 8 * LAT_S[1]
    outs, f0 = [], 0
    for n in split:
        zd = z[f0:f0 + n].to(device=DEV, dtype=torch.bfloat16).contiguous()
        out = torch.zeros((4 * n, H, W, 3), dtype=torch.uint8, device=DEV) if fmt == "uint8" else \
            torch.full((4 * n, 3, H, W), float("nan"), dtype=torch.float32, device=DEV)
        n_out = C.c_int(0)
        _lib.check(lib.mmpl_vae_stream_decode(handle, _lib.ptr(zd), n, _f16(mean), _f16(inv), _lib.ptr(out), int(fmt == "uint8"),
                                              C.byref(n_out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "mmpl_vae_stream_decode")
        torch.cuda.synchronize()
        outs.append(out[:n_out.value])
        f0 += n
    return outs, ws, handle


@pytest.mark.parametrize("fmt", ["float", "uint8"])
@pytest.mark.parametrize("split", [(1, 2), (2, 1), (1, 1, 1)], ids=lambda s: "-".join(map(str, s)))
def test_stream_equals_chain_stream(split, fmt):
    """Each call's output equals the same call of the chain's stream, whose caches are frames in buffers of their own."""
    lib, eng = _lib.load(), _engine(LAT_S)
    z = _latents(LAT_S, 3, 77)
    want, _ = _chain_stream_calls(z, split, fmt)
    need = lib.mmpl_vae_workspace_bytes(eng._h, 0)
    eng.clear_cache()
    eng._stream_ws = _nan_ws(need, PAT_A)
    f0 = 0
    for i, n in enumerate(split):
        got = eng.decode_stream(z[f0:f0 + n], MEAN, STD, fmt)
        torch.cuda.synchronize()
        assert _same_bits(got, want[i]), f"decode_stream call {i} of {split} differs from the chain's stream"
        f0 += n
    outs, ws, handle = _c_stream_calls(eng, z, split, fmt, PAT_B, EXTRA)
    try:
        for i, o in enumerate(outs):
            assert _same_bits(o, want[i]), f"mmpl_vae_stream_decode call {i} of {split} differs from the chain's stream"
        assert _tail_ok(ws, need)
    finally:
        lib.mmpl_vae_stream_destroy(handle)


def test_stream_continues_and_starts_over():
    """A call without clear_cache continues the video (a fourth and fifth latent frame after [2, 1]); clear_cache, then a second
    video on the same stream object and ANOTHER workspace starts from a first frame again.  Every call equals the chain's."""
    lib, eng = _lib.load(), _engine(LAT_S)
    mean, inv = _scales()
    z1, z2 = _latents(LAT_S, 5, 81), _latents(LAT_S, 2, 82)
    split1, split2 = (2, 1, 2), (1, 1)
    want1, cs = _chain_stream_calls(z1, split1, "float")
    cs.clear_cache()
    want2, _ = _chain_stream_calls(z2, split2, "float", cs)
    need = lib.mmpl_vae_workspace_bytes(eng._h, 0)
    # through VaeEngine
    eng.clear_cache()
    eng._stream_ws = _nan_ws(need, PAT_A)
    f0 = 0
    for i, n in enumerate(split1):
        assert _same_bits(eng.decode_stream(z1[f0:f0 + n], MEAN, STD), want1[i]), f"video 1, call {i}"
        f0 += n
    eng.clear_cache()
    eng._stream_ws = _nan_ws(need + EXTRA, PAT_B)
    f0 = 0
    for i, n in enumerate(split2):
        assert _same_bits(eng.decode_stream(z2[f0:f0 + n], MEAN, STD), want2[i]), f"video 2, call {i}"
        f0 += n
    assert _tail_ok(eng._stream_ws, need)
    eng.clear_cache()
    eng._stream_ws = None
    # through the C entries: one stream handle, reset between the videos, two workspaces of two sizes
    outs1, _, handle = _c_stream_calls(eng, z1, split1, "float", PAT_B, EXTRA)
    try:
        _lib.check(lib.mmpl_vae_stream_reset(handle), "mmpl_vae_stream_reset")
        outs2, _, _ = _c_stream_calls(eng, z2, split2, "float", PAT_A, 0, handle)
        for i, o in enumerate(outs1):
            assert _same_bits(o, want1[i]), f"C entry, video 1, call {i}"
        for i, o in enumerate(outs2):
            assert _same_bits(o, want2[i]), f"C entry, video 2, call {i}"
    finally:
        lib.mmpl_vae_stream_destroy(handle)


# ------------------------------------------------------------------------------------------------ the switch
_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_vae_chain_gpu import _engine, _latents, _pixels, MEAN, STD
eng = _engine((6, 10))
torch.save({{"dec": eng.decode(_latents((6, 10), 3, 77), MEAN, STD).cpu(), "enc": eng.encode(_pixels((6, 10), 9, 78), MEAN, STD).cpu()}}, sys.argv[1])
"""


def test_no_fuse_norm_switch_equals_chain_without_fusing(tmp_path):
    """MMPL_VAE_NO_FUSE_NORM=1 (read once per process: a fresh child) against the chain with every edge of FUSE off."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = tmp_path / "unfused.pt"
    env = dict(os.environ, MMPL_VAE_NO_FUSE_NORM="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(root=root), str(f)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = torch.load(f)
    mean, inv = _scales()
    lat = (6, 10)
    ch, ops = _chain(lat, fuse=False)
    dec = ch.decode(_latents(lat, 3, 77), mean, inv)
    enc = ch.encode(_pixels(lat, 9, 78), mean, inv)
    assert ops.canaries_intact()
    assert _same_bits(got["dec"], dec), "decode with the switch differs from the chain without fused norms"
    assert _same_bits(got["enc"], enc), "encode with the switch differs from the chain without fused norms"
    # and the switch matters: the fused chain is another function at the 1e-3 level (tests/test_vae_gpu.py)
    chf, _ = _chain(lat)
    assert not _same_bits(chf.encode(_pixels(lat, 9, 78), mean, inv), enc)
