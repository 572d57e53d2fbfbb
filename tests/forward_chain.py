"""The DiT forward (mmpl_dit_forward_at) and the context precompute (mmpl_dit_precompute_context) as ORDERED LISTS OF LAUNCHES, written
from the model -- oracle/wan_dit_ref.py, i.e. the reference's causal_fps_model.py:312-364 (block), :708-837 (forward), :384-395 (head),
model.py:161-194 / :238-266 (text / image cross-attention) -- on the launch contracts of include/mmpl_hip.h, not from csrc/api.hip.

`ForwardChain(sd, cfg, lat_h, lat_w, ops)` takes the REFERENCE state dict (the keys of mmpl_amd.synthetic.dit_state_dict): it packs
q | k | v and the block modulations itself and pads the patch weight to pe_k itself (it never calls mmpl_amd.dit.slot_tensors).  Every
launch goes through a small `ops` backend:

  HipOps   each op is exactly ONE call of the matching single-launch C entry (mmpl_gemm_ex, mmpl_attn_fwd_ex, mmpl_layernorm_ex,
           mmpl_qknorm_ex, mmpl_modulation, mmpl_patchify, mmpl_unpatchify, mmpl_sinusoid, mmpl_silu, mmpl_add,
           mmpl_rows_equal_last; `copy` is a device-to-device memcpy).  Every intermediate is a buffer of its own (nothing aliases),
           allocated with a tail filled with the 0x7FA5 canary; every GEMM that takes scratch gets a fresh zeroed one.
  RefOps   each op is its documented contract in plain torch on the CPU, in float64 or float32; `round=True` rounds to bf16 where the
           header says a kernel rounds its OUTPUT (the roundings inside a kernel -- P of the attention, the norm before its gain --
           are not restated: the per-kernel references tests/*_ref.py do that), `round=False` never rounds.

tests/test_forward_chain_host.py shows on the CPU that the chain is the model (RefOps against the oracle, both unrounded);
tests/test_forward_chain_gpu.py demands that the library's forward equals the HipOps chain in every bit.

The wiring decisions a forward makes are the entries of WIRING; a test hands in an altered copy to build a mutant of the chain.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

BF = torch.bfloat16
CANARY = 0x7FA5                       # the NaN pattern of the exact tests (tests/rowpass_ref.py)
TAIL = 128                            # canary elements behind every HipOps buffer
EPI_BIAS, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_RES, EPI_F32, EPI_VPAGES = range(7)     # mmpl_gemm_ex's `epi`
ATTN_AUTO, ATTN_LOCKSTEP, ATTN_W64 = 0, 1, 3                                             # mmpl_attn_fwd_ex's `variant`

# Which GEMM launches are given the tile tickets and the split-K scratch.  This is a fact about the LAUNCH PLAN (what the forward
# decided to schedule dynamically), not about wiring: the model does not say it, the header's mmpl_gemm_scratch does.
GEMM_SCRATCH = {"qkv": True, "o": True, "cross_q": True, "cross_o": True, "ffn0": True, "ffn2": True,
                "patch": False, "time0": False, "time2": False, "time_proj": False, "head": False,
                "text0": False, "text2": False, "ctx_k": False, "ctx_v": False}
# The encoder compositions (tests/encoder_chain.py: mmpl_t5_encode, mmpl_clip_visual, mmpl_i2v_*) pass neither to any of their GEMMs.
GEMM_SCRATCH.update({name: False for name in (
    "t5_qkv", "t5_scores", "t5_pv", "t5_o", "t5_gate", "t5_fc1", "t5_fc2",
    "clip_patch", "clip_qkv", "clip_proj", "clip_mlp0", "clip_mlp2",
    "proj_fc1", "proj_fc2", "img_k", "img_v", "i2v_q", "i2v_o")})

# The wiring of one forward (causal_fps_model.py:338-360: e = (modulation + e0).chunk(6); norm1 * (1 + e[1]) + e[0]; y * e[2];
# norm2 * (1 + e[4]) + e[3]; y * e[5]; :393: head e = (head.modulation + e).chunk(2), norm * (1 + e[1]) + e[0]).
WIRING = dict(
    norm1=(1, 0),                         # (scale chunk, shift chunk)
    gate1=2,
    norm2=(4, 3),
    gate2=5,
    cross_k_layer=lambda l: l,            # the layer whose text K block l attends
    cross_v_layer=lambda l: l,            # ... and whose text V
    img_v_layer=lambda l: l,              # the layer whose image V block l attends (its image K is always its own)
    copies=lambda T, n: T - n,            # weight of the collapsed text key: rows n .. T-1 are T - n copies of row n
    head_from="e",                        # the head's modulation adds e (the time embedding), not e0 (its projection)
)


def softmax_scale() -> float:
    """1 / sqrt(128) as one fp32 division of an fp32 square root."""
    return float(np.float32(1.0) / np.sqrt(np.float32(128.0)))


def q_prescale() -> float:
    """softmax_scale * log2(e) as one fp32 product: what a q that feeds the 64-rows-per-wave kernel is multiplied by before its rounding."""
    return float(np.float32(softmax_scale()) * np.float32(1.4426950408889634))


def rope_tables_f64():
    """cos, sin [1024][64] float64 by the reference's formula (model.py:29-36 rope_params, theta 1e4; causal_fps_model.py:510-516:
    dims 44 | 42 | 42 of the 128-wide head -> 22 | 21 | 21 rotary pairs), and the angles."""
    d = 128
    parts = (d - 4 * (d // 6), 2 * (d // 6), 2 * (d // 6))
    pos = np.arange(1024, dtype=np.float64)[:, None]
    ang = np.concatenate([pos * (1.0 / np.power(10000.0, np.arange(0, n, 2, dtype=np.float64) / n))[None, :] for n in parts], axis=1)
    assert ang.shape == (1024, 64)
    return np.cos(ang), np.sin(ang), ang


def rope_table_rule(cos32, sin32):
    """The rule a float32 RoPE table is held to: it equals float32(float64 table of the reference's formula) except where the float64
    value lies within the angle's error bound of a float32 rounding boundary -- there, and only there, it may be the neighbouring
    float32.  The bound on |d cos|, |d sin| <= |d angle|: 4 ulp of the float64 angle pos * freq (pow, the division and the product
    are one rounding each, in whichever libm), at most 1023 * 2^-50, plus 2 ulp of the value for cos / sin themselves.
    -> (entries that may differ, entries that do differ, entries that break the rule), over both tables."""
    cs, sn, ang = rope_tables_f64()
    err_a = np.minimum(4.0 * np.spacing(ang), 1023.0 * 2.0 ** -50)
    may = differ = bad = 0
    for v64, got in ((cs, np.asarray(cos32, dtype=np.float32)), (sn, np.asarray(sin32, dtype=np.float32))):
        want = v64.astype(np.float32)
        err = err_a + 2.0 * np.spacing(np.abs(v64))
        up, dn = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
        d_up = np.abs((want.astype(np.float64) + up.astype(np.float64)) / 2.0 - v64)        # distance to the two rounding boundaries
        d_dn = np.abs((want.astype(np.float64) + dn.astype(np.float64)) / 2.0 - v64)
        amb_up, amb_dn = d_up <= err, d_dn <= err
        ne = got != want
        ok = (~ne) | (amb_up & (got == up)) | (amb_dn & (got == dn))
        may += int((amb_up | amb_dn).sum())
        differ += int(ne.sum())
        bad += int((~ok).sum())
    return may, differ, bad


# ====================================================================================================== backends
class RefOps:
    """Every op as its documented contract, in plain torch on the CPU."""

    def __init__(self, dtype=torch.float64, round: bool = False):
        self.dtype, self.round = dtype, round
        cs, sn, _ = rope_tables_f64()
        if round:                                          # the library's tables are float32
            cs, sn = cs.astype(np.float32), sn.astype(np.float32)
        self._tables = (torch.from_numpy(cs.astype(np.float64)).to(dtype), torch.from_numpy(sn.astype(np.float64)).to(dtype))

    # ---- buffers
    def _r(self, x):
        return x.to(BF).to(self.dtype) if self.round else x

    def new(self, rows, cols):
        return torch.full((rows, cols), float("nan"), dtype=self.dtype)

    def param(self, t):
        return t.detach().to("cpu").to(self.dtype).contiguous()

    def tensor(self, t):
        return self.param(t)

    def ints(self, v):
        return None if v is None else torch.tensor([int(v)], dtype=torch.int32)

    def rope_tables(self):
        return self._tables

    def history_bytes(self, Lq, H):
        return 0

    def finish(self):
        pass

    # ---- ops
    def gemm(self, name, out, A, W, bias, epi=EPI_BIAS, res=None, gate=None, rpf=1, v_pages=None, v_col0=0):
        M, K = A.shape[0], W.shape[1]
        y = self._r(A[:, :K] @ W.t() + (0 if bias is None else bias))
        if epi == EPI_GELU:
            u = math.sqrt(2.0 / math.pi) * (y + 0.044715 * y * y * y)
            y = self._r(y / (1.0 + torch.exp(-2.0 * u)))              # == 0.5 y (1 + tanh u)
        elif epi == EPI_SILU:
            y = self._r(y / (1.0 + torch.exp(-y)))
        elif epi in (EPI_GATE_RES, EPI_RES):
            if epi == EPI_GATE_RES:
                rows = torch.arange(M) // rpf
                y = self._r(y * gate[rows])
            y = self._r(res + y)
        if epi == EPI_VPAGES:
            for f, page in enumerate(v_pages):
                page.copy_(y[f * rpf:(f + 1) * rpf, v_col0:])
            out[:, :v_col0].copy_(y[:, :v_col0])
        else:
            out.copy_(y)

    def layernorm(self, out, x, eps, scale=None, shift=None, rpf=1, w=None, b=None):
        mean = x.mean(dim=1, keepdim=True)
        var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
        n = (x - mean) * torch.rsqrt(var + eps)
        if w is not None:
            out.copy_(self._r(n * w + b))
        else:
            f = torch.arange(x.shape[0]) // rpf
            out.copy_(self._r(self._r(self._r(n) * self._r(1 + scale[f])) + shift[f]))

    def qknorm(self, q, wq, eps, q_scale=0.0, k=None, wk=None, k_pages=None, rope=None):
        def norm(x, w):
            return self._r(self._r(x * torch.rsqrt((x * x).mean(dim=1, keepdim=True) + eps)) * w)

        def rot(x):
            if rope is None:
                return x
            rows, d = x.shape
            S, gw = rope["rpf"], rope["grid_w"]
            r = torch.arange(rows)
            tok = r % S
            base = 0 if rope["frame_base"] is None else int(rope["frame_base"].reshape(-1)[0])
            fpos = torch.tensor([min(max(int(i) + base, 0), 1023) for i in rope["frame_ids"]])[r // S]
            pos = torch.cat([fpos[:, None].expand(rows, 22), (tok // gw)[:, None].expand(rows, 21), (tok % gw)[:, None].expand(rows, 21)], dim=1)
            pair = torch.arange(64)[None, :]
            cs, sn = rope["cos"][pos, pair][:, None, :], rope["sin"][pos, pair][:, None, :]
            v = x.reshape(rows, d // 128, 64, 2)
            re, im = v[..., 0], v[..., 1]
            return torch.stack([re * cs - im * sn, re * sn + im * cs], dim=-1).reshape(rows, d)

        qn = rot(norm(q, wq))
        q.copy_(self._r(qn * (q_scale if q_scale else 1.0)))
        if k is not None:
            kn = self._r(rot(norm(k, wk)))
            if rope is None:
                k_pages[0].copy_(kn)
            else:
                S = rope["rpf"]
                for f, page in enumerate(k_pages):
                    page.copy_(kn[f * S:(f + 1) * S])

    def attention(self, out, q, k_pages, v_pages, H, scale, groups=None, workspace_bytes=0, variant=ATTN_AUTO, q_prescaled=0, cross=0,
                  last_row_copies=0, history=None, stats=None):
        K, V = torch.cat(list(k_pages)), torch.cat(list(v_pages))
        mult = math.log(2.0) if q_prescaled else scale                   # a prescaled q carries scale * log2(e): exp2(K.q) = exp(ln 2 K.q)
        for h in range(H):
            c = slice(128 * h, 128 * (h + 1))
            s = (q[:, c] @ K[:, c].t()) * mult
            if last_row_copies > 1:
                s[:, -1] += math.log(last_row_copies)
            out[:, c].copy_(self._r(torch.softmax(s, dim=1) @ V[:, c]))

    def modulation(self, out, mod, e, bcast, n_layers, n_frames, nmod, d):
        m = mod.reshape(n_layers, 1, nmod, d)
        ev = e[:, None, :d] if bcast else e.reshape(n_frames, nmod, d)
        out.copy_(self._r(m + ev[None]).reshape(out.shape))

    def patchify(self, out, x, C_, h, w):
        F = x.shape[0]
        v = x.reshape(F, C_, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(F * (h // 2) * (w // 2), 4 * C_)
        out.zero_()
        out[:, :4 * C_].copy_(v)

    def unpatchify(self, out, y, C_, h, w):
        F = out.numel() // (C_ * h * w)
        v = y[:, :4 * C_].reshape(F, h // 2, w // 2, 2, 2, C_).permute(0, 5, 1, 3, 2, 4)
        out.copy_(v.reshape(out.shape))

    def sinusoid(self, out, t, freq_dim):
        half = freq_dim // 2
        a = t.to(torch.float64)[:, None] * torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(half, dtype=torch.float64) / half)
        out.copy_(self._r(torch.cat([torch.cos(a), torch.sin(a)], dim=1).to(self.dtype)))

    def silu(self, out, x):
        out.copy_(self._r(x / (1.0 + torch.exp(-x))))

    def add(self, a, b):
        a.copy_(self._r(a + b))

    def rows_equal_last(self, x):
        return (x == x[-1:]).all(dim=1).to(torch.int32)

    def copy(self, dst, src):
        dst.copy_(src.reshape(-1)[:dst.numel()].view(dst.shape))


class HipOps:
    """Every op is one call of the matching single-launch entry of libmmpl_hip.so on the current stream of `device`."""

    def __init__(self, lib, engine=None, device="cuda:0"):
        from mmpl_amd import _lib
        self.lib, self._lib, self.device = lib, _lib, torch.device(device)
        self.engine = engine
        self.buffers: List[torch.Tensor] = []              # (flat int16 buffer, payload elements)
        self.payload: List[int] = []
        self.plans: List[tuple] = []                       # (name, plan_out) of every GEMM and attention launch
        self.scratch: List[torch.Tensor] = []
        self._tables = None

    # ---- buffers
    def _raw(self, n_elems):
        b = torch.full((n_elems + TAIL,), CANARY, dtype=torch.int16, device=self.device)
        self.buffers.append(b)
        self.payload.append(n_elems)
        return b

    def new(self, rows, cols):
        return self._raw(rows * cols)[:rows * cols].view(BF).view(rows, cols)

    def param(self, t):
        return t.detach().to(device=self.device, dtype=BF).contiguous()

    def tensor(self, t):
        return t.detach().to(self.device).contiguous()

    def ints(self, v):
        return None if v is None else torch.tensor([int(v)], dtype=torch.int32, device=self.device)

    def rope_tables(self):
        """The HANDLE's tables (mmpl_dit_rope_tables): what the forward's own qknorm launch reads."""
        if self._tables is None:
            cs = torch.full((1024 * 64 + TAIL,), float("nan"), dtype=torch.float32, device=self.device)
            sn = cs.clone()
            with torch.cuda.device(self.device):
                self._lib.check(self.lib.mmpl_dit_rope_tables(self.engine._h, self._lib.ptr(cs), self._lib.ptr(sn), self._lib.stream_ptr()),
                                "mmpl_dit_rope_tables")
            torch.cuda.synchronize(self.device)
            assert bool(torch.isnan(cs[1024 * 64:]).all()) and bool(torch.isnan(sn[1024 * 64:]).all())
            self._tables = (cs[:1024 * 64].view(1024, 64), sn[:1024 * 64].view(1024, 64))
        return self._tables

    def history_bytes(self, Lq, H):
        return self.lib.mmpl_attn_history_bytes(Lq, H)

    def finish(self):
        torch.cuda.synchronize(self.device)

    def canaries_intact(self) -> bool:
        """Every tail still holds the canary, and every scratch header (tickets, split-K counters) is zero again."""
        torch.cuda.synchronize(self.device)
        want = CANARY
        tails = all(bool((b[n:] == want).all()) for b, n in zip(self.buffers, self.payload))
        heads = all(int(s[:2048].to(torch.int32).sum()) == 0 for s in self.scratch)
        return tails and heads

    # ---- helpers
    def _p(self, t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ld(self, t):
        assert t.dim() == 2 and t.stride(1) == 1, (tuple(t.shape), t.stride())
        return t.stride(0)

    def _call(self, rc, what):
        self._lib.check(rc, what)

    # ---- ops
    def gemm(self, name, out, A, W, bias, epi=EPI_BIAS, res=None, gate=None, rpf=1, v_pages=None, v_col0=0):
        M, N, K = A.shape[0], W.shape[0], W.shape[1]
        scratch, sbytes = None, 0
        if GEMM_SCRATCH[name]:
            sbytes = self.lib.mmpl_gemm_scratch_bytes()
            scratch = torch.zeros(sbytes, dtype=torch.uint8, device=self.device)
            self.scratch.append(scratch)
        pages, n_pages, v_ld = None, 0, 0
        if epi == EPI_VPAGES:
            n_pages = len(v_pages)
            pages = (C.c_void_p * n_pages)(*[p.data_ptr() for p in v_pages])
            v_ld = self._ld(v_pages[0])
        plan = (C.c_int * 6)(*([-1] * 6))
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_gemm_ex(self._p(A), self._ld(A), self._p(W), self._ld(W), self._p(bias), self._p(out), self._ld(out), M, N, K,
                                             epi, self._p(res), 0 if res is None else self._ld(res), self._p(gate),
                                             0 if gate is None else self._ld(gate), rpf, 1.0, 1, 0, 0, 0, pages, n_pages, v_col0, v_ld,
                                             self._p(scratch), sbytes, None, plan, self._stream()), "gemm " + name)
        self.plans.append((name, list(plan)))

    def layernorm(self, out, x, eps, scale=None, shift=None, rpf=1, w=None, b=None):
        rows, d = x.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_layernorm_ex(self._p(x), self._ld(x), self._p(out), self._ld(out), rows, d, eps, self._p(scale), self._p(shift),
                                                  0 if scale is None else self._ld(scale), rpf, self._p(w), self._p(b), -1, 0, None,
                                                  self._stream()), "layernorm")

    def qknorm(self, q, wq, eps, q_scale=0.0, k=None, wk=None, k_pages=None, rope=None):
        rows, d = q.shape
        n_frames = len(rope["frame_ids"]) if rope is not None else 1
        kp = None if k is None else (C.c_void_p * len(k_pages))(*[p.data_ptr() for p in k_pages])
        ids = None if rope is None else (C.c_int * n_frames)(*[int(i) for i in rope["frame_ids"]])
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_qknorm_ex(self._p(q), self._ld(q), self._p(k), 0 if k is None else self._ld(k), None, 0, self._p(wq), self._p(wk),
                                               rows, d, eps, q_scale, 0 if rope is None else 1,
                                               None if rope is None else self._p(rope["cos"]), None if rope is None else self._p(rope["sin"]),
                                               n_frames, ids, None if rope is None else self._p(rope["frame_base"]), kp, None,
                                               rope["rpf"] if rope is not None else rows, rope["grid_w"] if rope is not None else 1, 0, None,
                                               self._stream()), "qknorm")

    def attention(self, out, q, k_pages, v_pages, H, scale, groups=None, workspace_bytes=0, variant=ATTN_AUTO, q_prescaled=0, cross=0,
                  last_row_copies=0, history=None, stats=None):
        n = len(k_pages)
        kp = (C.c_void_p * n)(*[p.data_ptr() for p in k_pages])
        vp = (C.c_void_p * n)(*[p.data_ptr() for p in v_pages])
        grp = None if groups is None else (C.c_ubyte * n)(*groups)
        ws = None
        if workspace_bytes:
            assert workspace_bytes % 2 == 0
            ws = self._raw(workspace_bytes // 2)[:workspace_bytes // 2]
        plan = (C.c_int * 8)(*([-1] * 8))
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_attn_fwd_ex(self._p(q), self._ld(q), self._p(out), self._ld(out), kp, vp, grp, self._ld(k_pages[0]),
                                                 self._ld(v_pages[0]), n, k_pages[0].shape[0], q.shape[0], H, scale, self._p(ws), workspace_bytes,
                                                 variant, q_prescaled, cross, last_row_copies, self._p(history), self._p(stats), plan,
                                                 self._stream()), "attention")
        self.plans.append(("cross_attn" if cross else "self_attn", list(plan)))

    def modulation(self, out, mod, e, bcast, n_layers, n_frames, nmod, d):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_modulation(self._p(mod), 0 if n_layers == 1 else nmod * d, self._p(e), self._ld(e), bcast, self._p(out), n_layers,
                                                n_frames, nmod, d, self._stream()), "modulation")

    def patchify(self, out, x, C_, h, w):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_patchify(self._p(x), self._p(out), self._ld(out), x.shape[0], C_, h, w, self._stream()), "patchify")

    def unpatchify(self, out, y, C_, h, w):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_unpatchify(self._p(y), self._ld(y), self._p(out), out.numel() // (C_ * h * w), C_, h, w, self._stream()),
                       "unpatchify")

    def sinusoid(self, out, t, freq_dim):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_sinusoid(self._p(t), self._p(out), t.numel(), freq_dim, self._stream()), "sinusoid")

    def silu(self, out, x):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_silu(self._p(x), self._p(out), x.numel(), self._stream()), "silu")

    def add(self, a, b):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_add(self._p(a), self._p(b), a.numel(), self._stream()), "add")

    def rows_equal_last(self, x):
        rows, d = x.shape
        flags = torch.full((rows + 4,), -7, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_rows_equal_last(self._p(x), self._ld(x), rows, d, self._p(flags), self._stream()), "rows_equal_last")
        torch.cuda.synchronize(self.device)
        assert bool((flags[rows:] == -7).all())
        return flags[:rows].cpu()

    def copy(self, dst, src):
        dst.copy_(src.reshape(-1)[:dst.numel()].view(dst.shape))


# ====================================================================================================== the chain
class ForwardChain:
    def __init__(self, sd: Dict[str, torch.Tensor], cfg: dict, lat_h: int, lat_w: int, ops, wiring: Optional[dict] = None):
        self.ops, self.wiring = ops, dict(WIRING, **(wiring or {}))
        self.dim, self.ffn, self.H, self.L = cfg["dim"], cfg["ffn_dim"], cfg["num_heads"], cfg["num_layers"]
        self.text_len, self.text_dim = cfg.get("text_len", 512), cfg.get("text_dim", 4096)
        self.freq_dim, self.eps = cfg.get("freq_dim", 256), cfg.get("eps", 1e-6)
        self.in_dim = sd["patch_embedding.weight"].shape[1]
        self.lat_h, self.lat_w = lat_h, lat_w
        self.gh, self.gw = lat_h // 2, lat_w // 2
        self.S = self.gh * self.gw
        self.pe_k = (4 * self.in_dim + 63) // 64 * 64
        L, d = self.L, self.dim
        p = {}
        g = lambda k: sd[k].detach().to("cpu")
        # Conv3d(in_dim, dim, kernel (1, 2, 2), stride (1, 2, 2)) as a Linear over (c, ph, pw) -- patchify's column order -- zero-padded to pe_k
        pw = g("patch_embedding.weight").reshape(d, 4 * self.in_dim)
        p["patch_w"] = torch.nn.functional.pad(pw, (0, self.pe_k - 4 * self.in_dim))
        p["patch_b"] = g("patch_embedding.bias")
        for name, key in (("text0", "text_embedding.0"), ("text2", "text_embedding.2"), ("time0", "time_embedding.0"), ("time2", "time_embedding.2"),
                          ("time_proj", "time_projection.1"), ("head", "head.head")):
            p[name + "_w"], p[name + "_b"] = g(key + ".weight"), g(key + ".bias")
        p["head_mod"] = g("head.modulation").reshape(2, d)
        p["block_mod"] = torch.stack([g(f"blocks.{l}.modulation").reshape(6 * d) for l in range(L)])           # [L, 6 d]
        for l in range(L):
            b = f"blocks.{l}."
            p[f"{l}.qkv_w"] = torch.cat([g(b + f"self_attn.{x}.weight") for x in "qkv"])
            p[f"{l}.qkv_b"] = torch.cat([g(b + f"self_attn.{x}.bias") for x in "qkv"])
            for name, key in (("o", "self_attn.o"), ("cq", "cross_attn.q"), ("ck", "cross_attn.k"), ("cv", "cross_attn.v"), ("co", "cross_attn.o"),
                              ("f0", "ffn.0"), ("f2", "ffn.2")):
                p[f"{l}.{name}_w"], p[f"{l}.{name}_b"] = g(b + key + ".weight"), g(b + key + ".bias")
            for name, key in (("nq", "self_attn.norm_q"), ("nk", "self_attn.norm_k"), ("cnq", "cross_attn.norm_q"), ("cnk", "cross_attn.norm_k")):
                p[f"{l}.{name}"] = g(b + key + ".weight")
            p[f"{l}.n3_w"], p[f"{l}.n3_b"] = g(b + "norm3.weight"), g(b + "norm3.bias")
        self.p = {k: ops.param(v) for k, v in p.items()}
        self.trace: List[tuple] = []                       # (name, tensor) of every intermediate of the last forward, in launch order

    def _keep(self, name, t):
        self.trace.append((name, t))
        return t

    # ------------------------------------------------------------------------------------------ mmpl_dit_precompute_context
    def precompute_context(self, context, cross_k, cross_v):
        """context [text_len, text_dim] (zero-padded) -> cross_k, cross_v [L, text_len, dim] (written), returns distinct_rows:
        text_embedding (Linear, GELU(tanh), Linear: causal_fps_model.py:780-786), the count of leading rows distinct from the repeated
        tail (the header's `distinct_rows`), then per layer K = norm_k(k(ctx)), V = v(ctx) (model.py:175-180)."""
        ops, p, T, d = self.ops, self.p, self.text_len, self.dim
        t0 = ops.new(T, d)
        ops.gemm("text0", t0, context, p["text0_w"], p["text0_b"], epi=EPI_GELU)
        ctx = ops.new(T, d)
        ops.gemm("text2", ctx, t0, p["text2_w"], p["text2_b"])
        rows = T
        if T >= 2:
            flags = [int(v) for v in ops.rows_equal_last(ctx)]
            n = T - 1
            while n > 0 and flags[n - 1]:
                n -= 1                                     # rows n .. T-1 are identical
            if T - n >= 2:
                rows = n
        for l in range(self.L):
            ops.gemm("ctx_k", cross_k[l], ctx, p[f"{l}.ck_w"], p[f"{l}.ck_b"])
            ops.qknorm(cross_k[l], p[f"{l}.cnk"], self.eps)
            ops.gemm("ctx_v", cross_v[l], ctx, p[f"{l}.cv_w"], p[f"{l}.cv_b"])
        ops.finish()
        return rows

    # ------------------------------------------------------------------------------------------ mmpl_dit_forward_at
    def forward(self, x_in, t, frame_ids: Sequence[int], write_slots: Sequence[int], visible_slots: Sequence[int], k_cache, v_cache,
                cross_k, cross_v, cross_rows: Optional[int] = None, share_out=None, share_in=None, img_k=None, img_v=None,
                attn_history=None, stats=None, frame_base=None, self_variant: str = "w64", cross_w64: bool = False):
        """One forward.  x_in [nF, in_dim, h, w]; t [nF] float32; k_cache / v_cache [L, n_slots * S, dim], laid out as
        DitEngine.new_kv_cache lays them out (one allocation each: page addresses, adjacency and merging as in the forward), written
        in place; cross_k / cross_v [L, text_len, dim]; img_k / img_v [L, n_img, dim] or None; attn_history: uint8, per-layer slices of
        history_bytes(Lq, H); stats: int64 [5]; frame_base: int32 device scalar or None.
        self_variant "w64": 64 rows per wave on a q prescaled by softmax_scale * log2(e) (the default); "lockstep": MMPL_ATTN_V1=1.
        cross_w64: MMPL_CROSS_W64=1 (only with "w64").  Returns out [nF, 16, h, w]."""
        ops, p, w = self.ops, self.p, self.wiring
        self.trace = []
        S, d, H, L, T, eps = self.S, self.dim, self.H, self.L, self.text_len, self.eps
        nF = len(frame_ids)
        Lq = nF * S
        persist = all(s >= 0 for s in write_slots)
        assert persist or all(s < 0 for s in write_slots)
        assert share_out is None or share_in is None
        scale = softmax_scale()
        prescale = self_variant == "w64"
        cross_w64 = cross_w64 and prescale
        cos, sin = ops.rope_tables()

        # ---- embeddings (causal_fps_model.py:757-776)
        patch = self._keep("patch", ops.new(Lq, self.pe_k))
        ops.patchify(patch, x_in, self.in_dim, self.lat_h, self.lat_w)
        x = self._keep("x_embed", ops.new(Lq, d))
        ops.gemm("patch", x, patch, p["patch_w"], p["patch_b"])
        sinu = self._keep("sinusoid", ops.new(nF, self.freq_dim))
        ops.sinusoid(sinu, t, self.freq_dim)
        t1 = self._keep("time0", ops.new(nF, d))
        ops.gemm("time0", t1, sinu, p["time0_w"], p["time0_b"], epi=EPI_SILU)
        e = self._keep("e", ops.new(nF, d))
        ops.gemm("time2", e, t1, p["time2_w"], p["time2_b"])
        se = self._keep("silu_e", ops.new(nF, d))
        ops.silu(se, e)
        e0 = self._keep("e0", ops.new(nF, 6 * d))
        ops.gemm("time_proj", e0, se, p["time_proj_w"], p["time_proj_b"])
        # e = modulation + e0 for every block (causal_fps_model.py:338) and head.modulation + e for the head (:393)
        emod = self._keep("emod", ops.new(L * nF, 6 * d))
        ops.modulation(emod, p["block_mod"], e0, 0, L, nF, 6, d)
        emod_head = self._keep("emod_head", ops.new(nF, 2 * d))
        ops.modulation(emod_head, p["head_mod"], e if w["head_from"] == "e" else e0, 1, 1, nF, 2, d)

        page = lambda cache, l, slot: cache[l, slot * S:(slot + 1) * S]
        for l in range(L):
            chunk = lambda k, l=l: emod[l * nF:(l + 1) * nF, k * d:(k + 1) * d]       # [nF, d], one row per frame
            take_shared = l == 0 and share_in is not None
            ksc = vsc = None
            if not persist:                                # the stage's own K / V: scratch pages of one allocation each (:254-264)
                ksc, vsc = ops.new(Lq, d), ops.new(Lq, d)
            if not take_shared or persist:
                # -- self-attention input: norm1(x) * (1 + e[1]) + e[0]; q | k | v; RMSNorm(q), RMSNorm(k), RoPE; K / V slot write (:342-348, 209-217)
                xn = self._keep(f"{l}.norm1", ops.new(Lq, d))
                ops.layernorm(xn, x, eps, scale=chunk(w["norm1"][0]), shift=chunk(w["norm1"][1]), rpf=S)
                qkv = self._keep(f"{l}.qkv", ops.new(Lq, 3 * d))
                if persist:
                    k_dst = [page(k_cache, l, s) for s in write_slots]
                    v_dst = [page(v_cache, l, s) for s in write_slots]
                else:
                    k_dst = [ksc[i * S:(i + 1) * S] for i in range(nF)]
                    v_dst = [vsc[i * S:(i + 1) * S] for i in range(nF)]
                ops.gemm("qkv", qkv, xn, p[f"{l}.qkv_w"], p[f"{l}.qkv_b"], epi=EPI_VPAGES, rpf=S, v_pages=v_dst, v_col0=2 * d)
                ops.qknorm(qkv[:, :d], p[f"{l}.nq"], eps, q_scale=q_prescale() if prescale else 0.0, k=qkv[:, d:2 * d], wk=p[f"{l}.nk"],
                           k_pages=k_dst, rope=dict(cos=cos, sin=sin, frame_ids=list(frame_ids), frame_base=frame_base, rpf=S, grid_w=self.gw))
            if take_shared:
                # the other CFG branch computed block 0's self-attention residual on the same inputs: x continues from it
                x = self._keep("0.x_shared", ops.new(Lq, d))
                ops.copy(x, share_in)
            else:
                kp = [page(k_cache, l, s) for s in visible_slots]
                vp = [page(v_cache, l, s) for s in visible_slots]
                groups = [0] * len(kp)
                if not persist:
                    kp += [ksc[i * S:(i + 1) * S] for i in range(nF)]
                    vp += [vsc[i * S:(i + 1) * S] for i in range(nF)]
                    groups += [1] * nF                     # another allocation than the cache
                attn = self._keep(f"{l}.self_attn", ops.new(Lq, d))
                hist = None
                if attn_history is not None:
                    hb = ops.history_bytes(Lq, H)
                    hist = attn_history[l * hb:(l + 1) * hb]
                ops.attention(attn, qkv[:, :d], kp, vp, H, scale, groups=groups, workspace_bytes=Lq * d * 2,
                              variant=ATTN_W64 if prescale else ATTN_LOCKSTEP, q_prescaled=int(prescale), history=hist, stats=stats)
                x1 = self._keep(f"{l}.x_self", ops.new(Lq, d))
                ops.gemm("o", x1, attn, p[f"{l}.o_w"], p[f"{l}.o_b"], epi=EPI_GATE_RES, res=x, gate=chunk(w["gate1"]), rpf=S)
                x = x1
                if l == 0 and share_out is not None:
                    ops.copy(share_out.reshape(-1)[:Lq * d].view(Lq, d), x)
            # -- cross-attention: x + o(attention(norm_q(q(norm3(x))), K_text, V_text) [+ attention(q, K_img, V_img)]) (:352-353, model.py:161-194, 254-263)
            xn3 = self._keep(f"{l}.norm3", ops.new(Lq, d))
            ops.layernorm(xn3, x, eps, w=p[f"{l}.n3_w"], b=p[f"{l}.n3_b"])
            cq = self._keep(f"{l}.cross_q", ops.new(Lq, d))
            ops.gemm("cross_q", cq, xn3, p[f"{l}.cq_w"], p[f"{l}.cq_b"])
            ops.qknorm(cq, p[f"{l}.cnq"], eps, q_scale=q_prescale() if cross_w64 else 0.0)
            ckl, cvl = w["cross_k_layer"](l), w["cross_v_layer"](l)
            rows_k, copies = T, 0
            if not cross_w64 and cross_rows is not None and 0 <= cross_rows <= T - 2:
                rows_k, copies = cross_rows + 1, w["copies"](T, cross_rows)      # rows cross_rows .. T-1 are one key, weighted
            ca = self._keep(f"{l}.cross_attn", ops.new(Lq, d))
            cross_kind = dict(variant=ATTN_W64, q_prescaled=1) if cross_w64 else dict(variant=ATTN_AUTO, q_prescaled=0)
            ops.attention(ca, cq, [cross_k[ckl][:rows_k]], [cross_v[cvl][:rows_k]], H, scale, cross=1, last_row_copies=copies, **cross_kind)
            if img_k is not None:
                il = w["img_v_layer"](l)
                ia = self._keep(f"{l}.img_attn", ops.new(Lq, d))
                ops.attention(ia, cq, [img_k[l]], [img_v[il]], H, scale, cross=1, **cross_kind)
                ops.add(ca, ia)
            x2 = self._keep(f"{l}.x_cross", ops.new(Lq, d))
            ops.gemm("cross_o", x2, ca, p[f"{l}.co_w"], p[f"{l}.co_b"], epi=EPI_RES, res=x)
            # -- FFN: x + ffn(norm2(x) * (1 + e[4]) + e[3]) * e[5] (:354-360)
            xn2 = self._keep(f"{l}.norm2", ops.new(Lq, d))
            ops.layernorm(xn2, x2, eps, scale=chunk(w["norm2"][0]), shift=chunk(w["norm2"][1]), rpf=S)
            hid = self._keep(f"{l}.ffn0", ops.new(Lq, self.ffn))
            ops.gemm("ffn0", hid, xn2, p[f"{l}.f0_w"], p[f"{l}.f0_b"], epi=EPI_GELU)
            x3 = self._keep(f"{l}.x_ffn", ops.new(Lq, d))
            ops.gemm("ffn2", x3, hid, p[f"{l}.f2_w"], p[f"{l}.f2_b"], epi=EPI_GATE_RES, res=x2, gate=chunk(w["gate2"]), rpf=S)
            x = x3
        # ---- head: Linear(norm(x) * (1 + e[1]) + e[0]), unpatchify (:384-395, 1007-1030)
        xh = self._keep("head_norm", ops.new(Lq, d))
        ops.layernorm(xh, x, eps, scale=emod_head[:, d:], shift=emod_head[:, :d], rpf=S)
        yh = self._keep("head", ops.new(Lq, 64))
        ops.gemm("head", yh, xh, p["head_w"], p["head_b"])
        out = self._keep("out", ops.new(nF, 16 * self.lat_h * self.lat_w))
        ops.unpatchify(out, yh, 16, self.lat_h, self.lat_w)
        ops.finish()
        return out.view(nF, 16, self.lat_h, self.lat_w)
