"""The umT5 encoder (mmpl_t5_encode), the CLIP vision tower (mmpl_clip_visual), the three Wan-I2V entries (mmpl_i2v_img_proj,
mmpl_i2v_img_kv, mmpl_i2v_cross_attn) and DitEngine.precompute_image_context as ORDERED LISTS OF LAUNCHES, written from the model --
the reference's wan/modules/t5.py:45-145, 267-312, clip.py:120-155, 209-327, model.py:224-266, 469-481, as restated in
oracle/t5_ref.py, oracle/clip_ref.py, oracle/i2v_ref.py -- on the launch contracts of include/mmpl_hip.h, not from csrc/t5.hip,
csrc/i2v.hip or the Python engines.

Every chain takes the REFERENCE state dict (mmpl_amd.synthetic.t5_state_dict, clip_visual_state_dict, i2v_cross_state_dict,
dit_i2v_state_dict) and packs it itself: q | k | v of umT5 into one operand, the CLIP heads zero-padded from head_dim to 128 columns
in to_qkv and proj, the im2col in (c, ky, kx) order padded to a multiple of 64, the bucket table from
oracle/t5_ref.relative_position_bucket.  It never calls T5Engine.load_state_dict, CLIPVisionTower.load_state_dict,
relative_position_buckets or slot_tensors.

The launches go through the two backends of tests/forward_chain.py, extended here with the ops these compositions add (the batched
and the fp32-output GEMM, the five umT5 glue launches, gelu_erf):

  EncHipOps  one call of the matching single-launch entry per op, every intermediate in a canary-tailed buffer of its own.
  EncRefOps  the documented contract of each op in plain torch on the CPU, float64 or float32.

None of these compositions passes tile tickets or split-K scratch to a GEMM (forward_chain.GEMM_SCRATCH: all "no").
tests/test_encoder_chain_host.py shows on the CPU that the chains are the model; tests/test_encoder_chain_gpu.py demands that the
library equals the EncHipOps chains in every bit.  The wiring decisions are the entries of WIRING; a test hands in an altered copy to
build a mutant of a chain.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from tests import forward_chain as FC
from tests.forward_chain import BF, EPI_BIAS, EPI_F32, EPI_RES

BF16_MIN = float(torch.finfo(torch.bfloat16).min)

WIRING = dict(
    # umT5 (t5.py:267-312, shared_pos=False: every block has a position table of its own)
    t5_bias_layer=lambda l: l,            # the layer whose relative-position table block l's softmax reads
    t5_gelu_on="gate",                    # fc1(x) * GELU(gate(x)) (t5.py:139): which of the two projections goes through the GELU
    t5_norm2_gain="norm2",                # the gain of the norm in front of the FFN
    t5_eps=1e-6,                          # T5LayerNorm's eps (t5.py:55)
    # CLIP (clip.py:52-86, 120-155)
    clip_scale=lambda head_dim: float(np.float32(1.0) / np.sqrt(np.float32(head_dim))),   # of the NATIVE head_dim, not the padded 128
    clip_norm2_gain="norm2",              # the gain of the norm in front of the MLP
    clip_eps=1e-5,
    # Wan-I2V (model.py:224-266, 469-481)
    proj_eps=1e-5,                        # MLPProj's two LayerNorms: torch default
    i2v_eps=1e-6,
    i2v_img_gain="norm_k_img",            # the gain that norms k_img(context_img) (norm_k norms k(context))
    i2v_normed="k",                       # of the (K, V) pair, the one that is normed
    i2v_swap_k=False,                     # True: the text attention reads the image K and the image attention the text K
    img_layer=lambda l, part: l,          # the layer whose k_img ("k") / v_img ("v") / norm_k_img ("norm") weights fill slot l
)


def ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


# ====================================================================================================== backends
class EncRefOps(FC.RefOps):
    """forward_chain.RefOps plus the contracts of the ops the encoders add, restated from include/mmpl_hip.h."""

    def new_f32(self, rows, cols):
        return torch.full((rows, cols), float("nan"), dtype=self.dtype)

    def int_tensor(self, t):
        return t.detach().to("cpu").to(torch.int64).contiguous()

    def bgemm(self, name, outs, As, Ws, epi=EPI_BIAS):
        """Problem b: outs[b] = As[b] . Ws[b]^T; epi 5 leaves the fp32 accumulator (alpha 1), epi 0 rounds it."""
        for o, a, w in zip(outs, As, Ws):
            y = a @ w.t()
            if epi == EPI_F32:
                o.copy_(y.to(torch.float32).to(self.dtype) if self.round else y)
            else:
                o.copy_(self._r(y))

    def attention(self, out, q, k_pages, v_pages, H, scale, head_dim=128, **kw):
        """forward_chain's contract at a head width other than 128 too (the unpadded CLIP chain of the host test)."""
        if head_dim == 128:
            return super().attention(out, q, k_pages, v_pages, H, scale, **kw)
        K, V = torch.cat(list(k_pages)), torch.cat(list(v_pages))
        for h in range(H):
            c = slice(head_dim * h, head_dim * (h + 1))
            out[:, c].copy_(self._r(torch.softmax((q[:, c] @ K[:, c].t()) * scale, dim=1) @ V[:, c]))

    def t5_gather(self, out, ids, emb):
        out.copy_(emb[ids])

    def t5_softmax(self, p, sc, pos_emb, bucket, mask, H, L):
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        table = pos_emb[bucket[j - i + L - 1]]                                 # [L, L, H]
        for h in range(H):
            bias = torch.where(mask[None, :] != 0, table[:, :, h], torch.full_like(table[:, :, h], BF16_MIN))
            s = self._r(self._r(sc[h * L:(h + 1) * L]) + bias)
            p[h * L:(h + 1) * L].copy_(self._r(torch.softmax(s, dim=1)))

    def t5_transpose(self, vt, v, L, c, H):
        for h in range(H):
            vt[h * c:(h + 1) * c].copy_(v[:, h * c:(h + 1) * c].t())

    def t5_gated(self, f, g):
        r = self._r
        u = r(g + r(0.044715 * r(g * g * g)))
        gelu = r(r(0.5 * g) * r(1.0 + r(torch.tanh(r(math.sqrt(2.0 / math.pi) * u)))))
        f.copy_(r(f * gelu))

    def t5_zero_pad(self, out, mask):
        out[mask == 0] = 0.0

    def gelu_erf(self, x):
        x.copy_(self._r(0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))))


class EncHipOps(FC.HipOps):
    """forward_chain.HipOps plus one call of mmpl_gemm_ex (batched, fp32), mmpl_t5_*, mmpl_gelu_erf per added op."""

    def new_f32(self, rows, cols):
        n = 2 * rows * cols
        return self._raw(n)[:n].view(torch.float32).view(rows, cols)

    def int_tensor(self, t):
        return t.detach().to(device=self.device, dtype=torch.int32).contiguous()

    def _batch_stride(self, ts):
        """Element stride from one problem's operand to the next: the views must be evenly spaced and alike."""
        steps = {b.data_ptr() - a.data_ptr() for a, b in zip(ts, ts[1:])}
        assert len(steps) == 1 and len({(tuple(t.shape), t.stride()) for t in ts}) == 1
        step = steps.pop()
        assert step >= 0 and step % ts[0].element_size() == 0
        return step // ts[0].element_size()

    def bgemm(self, name, outs, As, Ws, epi=EPI_BIAS):
        import ctypes as C
        assert not FC.GEMM_SCRATCH[name] and len(outs) == len(As) == len(Ws) > 1
        (M, K), N = As[0].shape, Ws[0].shape[0]
        assert Ws[0].shape[1] == K and tuple(outs[0].shape) == (M, N)
        assert outs[0].dtype == (torch.float32 if epi == EPI_F32 else BF)
        plan = (C.c_int * 6)(*([-1] * 6))
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_gemm_ex(self._p(As[0]), self._ld(As[0]), self._p(Ws[0]), self._ld(Ws[0]), None, self._p(outs[0]),
                                             self._ld(outs[0]), M, N, K, epi, None, 0, None, 0, 1, 1.0, len(outs), self._batch_stride(As),
                                             self._batch_stride(Ws), self._batch_stride(outs), None, 0, 0, 0, None, 0, None, plan,
                                             self._stream()), "gemm " + name)
        self.plans.append((name, list(plan)))

    def attention(self, out, q, k_pages, v_pages, H, scale, head_dim=128, **kw):
        assert head_dim == 128                             # the kernels' head width: narrower heads arrive padded
        return super().attention(out, q, k_pages, v_pages, H, scale, **kw)

    def t5_gather(self, out, ids, emb):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_t5_gather(self._p(ids), self._p(emb), self._p(out), out.shape[0], out.shape[1], self._stream()), "t5_gather")

    def t5_softmax(self, p, sc, pos_emb, bucket, mask, H, L):
        assert tuple(sc.shape) == tuple(p.shape) == (H * L, L) and tuple(pos_emb.shape)[1] == H and bucket.numel() == 2 * L - 1
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_t5_softmax(self._p(sc), self._p(pos_emb), self._p(bucket), self._p(mask), self._p(p), H, L,
                                                self._stream()), "t5_softmax")

    def t5_transpose(self, vt, v, L, c, H):
        assert tuple(vt.shape) == (H * c, L) and tuple(v.shape) == (L, H * c)
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_t5_transpose(self._p(v), self._ld(v), self._p(vt), L, c, H, self._stream()), "t5_transpose")

    def t5_gated(self, f, g):
        assert f.is_contiguous() and g.is_contiguous() and f.numel() == g.numel()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_t5_gated(self._p(f), self._p(g), f.numel(), self._stream()), "t5_gated")

    def t5_zero_pad(self, out, mask):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_t5_zero_pad(self._p(out), self._p(mask), out.shape[0], out.shape[1], self._stream()), "t5_zero_pad")

    def gelu_erf(self, x):
        assert x.is_contiguous()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_gelu_erf(self._p(x), x.numel(), self._stream()), "gelu_erf")


# ====================================================================================================== umT5
class T5Chain:
    """T5Encoder.forward behind WanTextEncoder (t5.py:267-312, wan_wrapper.py:38-51) for ONE prompt of text_len tokens."""

    def __init__(self, sd: Dict[str, torch.Tensor], cfg: dict, text_len: int, ops, wiring: Optional[dict] = None):
        from oracle.t5_ref import relative_position_bucket
        self.ops, self.wiring = ops, dict(WIRING, **(wiring or {}))
        self.L, self.d, self.da, self.df = text_len, cfg["dim"], cfg["dim_attn"], cfg["dim_ffn"]
        self.H, self.n_layers = cfg["num_heads"], cfg["num_layers"]
        g = lambda k: sd[k].detach().to("cpu")
        p = {"emb": g("token_embedding.weight"), "norm": g("norm.weight")}
        for l in range(self.n_layers):
            b = f"blocks.{l}."
            p[f"{l}.qkv"] = torch.cat([g(b + f"attn.{x}.weight") for x in "qkv"])
            for name, key in (("norm1", "norm1"), ("o", "attn.o"), ("pos", "pos_embedding.embedding"), ("norm2", "norm2"),
                              ("gate", "ffn.gate.0"), ("fc1", "ffn.fc1"), ("fc2", "ffn.fc2")):
                p[f"{l}.{name}"] = g(b + key + ".weight")
        self.p = {k: ops.param(v) for k, v in p.items()}
        # bucket of rel = j - i at index j - i + L - 1 (t5.py:240-264)
        self.bucket = ops.int_tensor(relative_position_bucket(torch.arange(-(text_len - 1), text_len), cfg["num_buckets"]))
        assert self.bucket.numel() == 2 * text_len - 1
        self.trace = []

    def _keep(self, name, t):
        self.trace.append((name, t))
        return t

    def _norm(self, name, x, gain):
        """T5LayerNorm (t5.py:52-67): RMS norm with a gain, into a buffer of its own."""
        y = self._keep(name, self.ops.new(self.L, self.d))
        self.ops.copy(y, x)
        self.ops.qknorm(y, gain, self.wiring["t5_eps"])
        return y

    def encode(self, ids, mask):
        """ids, mask: integer [text_len] -> [text_len, dim], rows of masked tokens zeroed."""
        ops, p, w = self.ops, self.p, self.wiring
        L, d, da, df, H = self.L, self.d, self.da, self.df, self.H
        hc = da // H
        self.trace = []
        ids, mask = ops.int_tensor(ids), ops.int_tensor(mask)
        x = self._keep("embed", ops.new(L, d))
        ops.t5_gather(x, ids, p["emb"])
        for l in range(self.n_layers):
            # -- x + o(softmax(q k^T + position bias, masked keys at finfo.min) v) (t5.py:70-121, 169-172): no score scaling
            xn = self._norm(f"{l}.norm1", x, p[f"{l}.norm1"])
            qkv = self._keep(f"{l}.qkv", ops.new(L, 3 * da))
            ops.gemm("t5_qkv", qkv, xn, p[f"{l}.qkv"], None)
            sc = self._keep(f"{l}.scores", ops.new_f32(H * L, L))
            ops.bgemm("t5_scores", [sc[h * L:(h + 1) * L] for h in range(H)], [qkv[:, h * hc:(h + 1) * hc] for h in range(H)],
                      [qkv[:, da + h * hc:da + (h + 1) * hc] for h in range(H)], epi=EPI_F32)
            pr = self._keep(f"{l}.p", ops.new(H * L, L))
            ops.t5_softmax(pr, sc, p[f"{w['t5_bias_layer'](l)}.pos"], self.bucket, mask, H, L)
            vt = self._keep(f"{l}.vt", ops.new(H * hc, L))
            ops.t5_transpose(vt, qkv[:, 2 * da:], L, hc, H)
            attn = self._keep(f"{l}.attn", ops.new(L, da))
            ops.bgemm("t5_pv", [attn[:, h * hc:(h + 1) * hc] for h in range(H)], [pr[h * L:(h + 1) * L] for h in range(H)],
                      [vt[h * hc:(h + 1) * hc] for h in range(H)])
            x1 = self._keep(f"{l}.x_attn", ops.new(L, d))
            ops.gemm("t5_o", x1, attn, p[f"{l}.o"], None, epi=EPI_RES, res=x)
            # -- x + fc2(fc1(h) * GELU(gate(h))), h = norm2(x) (t5.py:124-145, 173)
            xn2 = self._norm(f"{l}.norm2", x1, p[f"{l}.{w['t5_norm2_gain']}"])
            gt = self._keep(f"{l}.gate", ops.new(L, df))
            ops.gemm("t5_gate", gt, xn2, p[f"{l}.gate"], None)
            f1 = self._keep(f"{l}.fc1", ops.new(L, df))
            ops.gemm("t5_fc1", f1, xn2, p[f"{l}.fc1"], None)
            if w["t5_gelu_on"] == "gate":
                ops.t5_gated(f1, gt)
                hid = f1
            else:
                ops.t5_gated(gt, f1)
                hid = gt
            x2 = self._keep(f"{l}.x_ffn", ops.new(L, d))
            ops.gemm("t5_fc2", x2, hid, p[f"{l}.fc2"], None, epi=EPI_RES, res=x1)
            x = x2
        out = self._norm("out", x, p["norm"])
        ops.t5_zero_pad(out, mask)
        ops.finish()
        return out


# ====================================================================================================== CLIP
class ClipChain:
    """VisionTransformer.forward(x, use_31_block=True) (clip.py:209-327): every block but the last, no post_norm, no head."""

    def __init__(self, sd: Dict[str, torch.Tensor], image_size: int, patch_size: int, dim: int, num_heads: int, num_layers: int, ops,
                 wiring: Optional[dict] = None, pad_heads: bool = True):
        self.ops, self.wiring = ops, dict(WIRING, **(wiring or {}))
        self.P, self.d, self.H, self.hd = patch_size, dim, num_heads, dim // num_heads
        self.n_blocks = num_layers - 1
        self.n_patch = (image_size // patch_size) ** 2
        self.n = self.n_patch + 1
        self.pk = ceil64(3 * patch_size * patch_size)
        self.hp = 128 if pad_heads else self.hd                                # a head's columns in to_qkv's output and proj's input
        H, hd, hp, d = self.H, self.hd, self.hp, dim
        g = lambda k: sd[k].detach().to("cpu")
        p = {}
        # Conv2d(3, dim, P, stride P, bias=False) as a Linear over (c, ky, kx), K zero-padded to a multiple of 64
        p["patch_w"] = torch.nn.functional.pad(g("patch_embedding.weight").reshape(d, 3 * patch_size * patch_size), (0, self.pk - 3 * patch_size ** 2))
        p["cls"], p["pos"] = g("cls_embedding").reshape(1, d), g("pos_embedding").reshape(self.n, d)
        p["pre_w"], p["pre_b"] = g("pre_norm.weight"), g("pre_norm.bias")
        for i in range(self.n_blocks):
            b = f"transformer.{i}."
            # to_qkv's rows are (q | k | v, head, column of the head) (clip.py:75: view(b, s, 3, n, d)); proj's columns (head, column)
            qw = torch.zeros(3, H, hp, d, dtype=g(b + "attn.to_qkv.weight").dtype)
            qw[:, :, :hd] = g(b + "attn.to_qkv.weight").reshape(3, H, hd, d)
            qb = torch.zeros(3, H, hp, dtype=qw.dtype)
            qb[:, :, :hd] = g(b + "attn.to_qkv.bias").reshape(3, H, hd)
            pw = torch.zeros(d, H, hp, dtype=qw.dtype)
            pw[:, :, :hd] = g(b + "attn.proj.weight").reshape(d, H, hd)
            p[f"{i}.qkv_w"], p[f"{i}.qkv_b"], p[f"{i}.proj_w"] = qw.reshape(3 * H * hp, d), qb.reshape(-1), pw.reshape(d, H * hp)
            p[f"{i}.proj_b"] = g(b + "attn.proj.bias")
            for name in ("norm1", "norm2", "mlp.0", "mlp.2"):
                p[f"{i}.{name}_w"], p[f"{i}.{name}_b"] = g(b + name + ".weight"), g(b + name + ".bias")
        self.mlp = p["0.mlp.0_w"].shape[0] if self.n_blocks else 4 * d
        self.p = {k: ops.param(v) for k, v in p.items()}
        self.trace = []

    def _keep(self, name, t):
        self.trace.append((name, t))
        return t

    def im2col(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels [3, S, S] -> [n_patch, pk]: patch (gy, gx) in row gy * g + gx (the conv output flattened, clip.py:313), its pixels in
        (c, ky, kx) order like the conv weight, zero-padded to pk."""
        P, g = self.P, int(round(math.sqrt(self.n_patch)))
        cols = pixels.reshape(3, g, P, g, P).permute(1, 3, 0, 2, 4).reshape(g * g, 3 * P * P)
        return torch.nn.functional.pad(cols, (0, self.pk - 3 * P * P)).contiguous()

    def forward(self, patches):
        """patches [n_patch, pk] (im2col) -> tokens [n_patch + 1, dim]."""
        ops, p, w = self.ops, self.p, self.wiring
        n, d, H, hw = self.n, self.d, self.H, self.H * self.hp
        eps, scale = w["clip_eps"], w["clip_scale"](self.hd)
        self.trace = []
        # x = [cls; patch embedding] + pos, pre_norm (clip.py:313-317)
        x0 = self._keep("embed", ops.new(n, d))
        ops.copy(x0[0:1], p["cls"])
        ops.gemm("clip_patch", x0[1:], patches, p["patch_w"], None)
        ops.add(x0, p["pos"])
        x = self._keep("pre_norm", ops.new(n, d))
        ops.layernorm(x, x0, eps, w=p["pre_w"], b=p["pre_b"])
        for i in range(self.n_blocks):
            # x + proj(attention(to_qkv(norm1(x)))) (clip.py:52-86, 150-151)
            h1 = self._keep(f"{i}.norm1", ops.new(n, d))
            ops.layernorm(h1, x, eps, w=p[f"{i}.norm1_w"], b=p[f"{i}.norm1_b"])
            qkv = self._keep(f"{i}.qkv", ops.new(n, 3 * hw))
            ops.gemm("clip_qkv", qkv, h1, p[f"{i}.qkv_w"], p[f"{i}.qkv_b"])
            att = self._keep(f"{i}.attn", ops.new(n, hw))
            ops.attention(att, qkv[:, :hw], [qkv[:, hw:2 * hw]], [qkv[:, 2 * hw:]], H, scale, head_dim=self.hp, cross=1)
            x1 = self._keep(f"{i}.x_attn", ops.new(n, d))
            ops.gemm("clip_proj", x1, att, p[f"{i}.proj_w"], p[f"{i}.proj_b"], epi=EPI_RES, res=x)
            # x + mlp.2(GELU(mlp.0(norm2(x)))) (clip.py:152-153), GELU in its erf form
            h2 = self._keep(f"{i}.norm2", ops.new(n, d))
            ops.layernorm(h2, x1, eps, w=p[f"{i}.{w['clip_norm2_gain']}_w"], b=p[f"{i}.norm2_b"])
            m = self._keep(f"{i}.mlp0", ops.new(n, self.mlp))
            ops.gemm("clip_mlp0", m, h2, p[f"{i}.mlp.0_w"], p[f"{i}.mlp.0_b"])
            ops.gelu_erf(m)
            x2 = self._keep(f"{i}.x_mlp", ops.new(n, d))
            ops.gemm("clip_mlp2", x2, m, p[f"{i}.mlp.2_w"], p[f"{i}.mlp.2_b"], epi=EPI_RES, res=x1)
            x = x2
        ops.finish()
        return x


# ====================================================================================================== Wan-I2V
def img_proj(mp_sd: Dict[str, torch.Tensor], clip_fea, ops, wiring: Optional[dict] = None, prefix: str = ""):
    """MLPProj (model.py:469-481): LayerNorm, Linear, GELU (erf), Linear, LayerNorm.  clip_fea [n, clip_dim] -> [n, dim]."""
    w = dict(WIRING, **(wiring or {}))
    p = {k: ops.param(mp_sd[prefix + k]) for k in ("proj.0.weight", "proj.0.bias", "proj.1.weight", "proj.1.bias", "proj.3.weight",
                                                    "proj.3.bias", "proj.4.weight", "proj.4.bias")}
    n, cd, d = clip_fea.shape[0], p["proj.1.weight"].shape[1], p["proj.3.weight"].shape[0]
    t0 = ops.new(n, cd)
    ops.layernorm(t0, clip_fea, w["proj_eps"], w=p["proj.0.weight"], b=p["proj.0.bias"])
    t1 = ops.new(n, cd)
    ops.gemm("proj_fc1", t1, t0, p["proj.1.weight"], p["proj.1.bias"])
    ops.gelu_erf(t1)
    t2 = ops.new(n, d)
    ops.gemm("proj_fc2", t2, t1, p["proj.3.weight"], p["proj.3.bias"])
    out = ops.new(n, d)
    ops.layernorm(out, t2, w["proj_eps"], w=p["proj.4.weight"], b=p["proj.4.bias"])
    ops.finish()
    return out


def _kv(ops, w, ctx, wk, bk, wv, bv, gain, k_out, v_out):
    """K = norm(k(ctx)), V = v(ctx) (model.py:248-252) into k_out / v_out [n, dim]."""
    ops.gemm("img_k", k_out, ctx, wk, bk)
    if w["i2v_normed"] == "k":
        ops.qknorm(k_out, gain, w["i2v_eps"])
    ops.gemm("img_v", v_out, ctx, wv, bv)
    if w["i2v_normed"] != "k":
        ops.qknorm(v_out, gain, w["i2v_eps"])


def img_kv(ca_sd: Dict[str, torch.Tensor], ctx, ops, which: str = "img", wiring: Optional[dict] = None):
    """which "img": (norm_k_img(k_img(ctx)), v_img(ctx)) of the image tokens; "txt": (norm_k(k(ctx)), v(ctx)) of the text tokens."""
    w = dict(WIRING, **(wiring or {}))
    kn, vn, gn = ("k_img", "v_img", w["i2v_img_gain"]) if which == "img" else ("k", "v", "norm_k")
    g = lambda k: ops.param(ca_sd[k])
    n, d = ctx.shape[0], ca_sd[kn + ".weight"].shape[0]
    k_out, v_out = ops.new(n, d), ops.new(n, d)
    _kv(ops, w, ctx, g(kn + ".weight"), g(kn + ".bias"), g(vn + ".weight"), g(vn + ".bias"), g(gn + ".weight"), k_out, v_out)
    ops.finish()
    return k_out, v_out


def i2v_cross_attn(ca_sd: Dict[str, torch.Tensor], x, k_txt, v_txt, k_img, v_img, ops, wiring: Optional[dict] = None):
    """WanI2VCrossAttention.forward on prepared K / V (model.py:238-266): o(attention(q, K, V) + attention(q, K_img, V_img)),
    q = norm_q(q(x)); heads of 128, scale 1 / sqrt(128)."""
    w = dict(WIRING, **(wiring or {}))
    g = lambda k: ops.param(ca_sd[k])
    Lq, d = x.shape
    H = d // 128
    q = ops.new(Lq, d)
    ops.gemm("i2v_q", q, x, g("q.weight"), g("q.bias"))
    ops.qknorm(q, g("norm_q.weight"), w["i2v_eps"])
    if w["i2v_swap_k"]:                                   # (each attention keeps its V; both are cut to the rows the two K share)
        n = min(k_txt.shape[0], k_img.shape[0])
        k_txt, k_img, v_txt, v_img = k_img[:n], k_txt[:n], v_txt[:n], v_img[:n]
    at, ai = ops.new(Lq, d), ops.new(Lq, d)
    ops.attention(ai, q, [k_img], [v_img], H, FC.softmax_scale(), cross=1)
    ops.attention(at, q, [k_txt], [v_txt], H, FC.softmax_scale(), cross=1)
    ops.add(at, ai)
    out = ops.new(Lq, d)
    ops.gemm("i2v_o", out, at, g("o.weight"), g("o.bias"))
    ops.finish()
    return out


def image_context(dit_sd: Dict[str, torch.Tensor], cfg: dict, clip_fea, ops, wiring: Optional[dict] = None):
    """DitEngine.precompute_image_context: img_emb once (model.py:684-685), then every block's own k_img / norm_k_img / v_img on it
    (model.py:251-252) into slot l of img_k / img_v [num_layers, n, dim]."""
    w = dict(WIRING, **(wiring or {}))
    L, d, n = cfg["num_layers"], cfg["dim"], clip_fea.shape[0]
    ctx_img = img_proj(dit_sd, clip_fea, ops, wiring, prefix="img_emb.")
    img_k, img_v = ops.new(L * n, d).view(L, n, d), ops.new(L * n, d).view(L, n, d)
    for l in range(L):
        g = lambda part, name: ops.param(dit_sd[f"blocks.{w['img_layer'](l, part)}.cross_attn.{name}"])
        _kv(ops, w, ctx_img, g("k", "k_img.weight"), g("k", "k_img.bias"), g("v", "v_img.weight"), g("v", "v_img.bias"),
            g("norm", w["i2v_img_gain"] + ".weight"), img_k[l], img_v[l])
    ops.finish()
    return img_k, img_v
