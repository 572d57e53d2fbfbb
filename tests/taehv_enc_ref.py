"""Restatement of the TAEHV encoder (the reference's demo_utils/taehv.py, ``TAEHV.encode_video``) for tests at sizes the committed
fixture does not hold.  Written from the layer list, plain ``torch.nn.functional`` on a state dict in the reference's keys:

    conv 3->64 + ReLU -> TPool(2) -> conv 64->64 stride 2 (no bias) -> 3 MemBlock(64) -> TPool(2) -> conv stride 2 -> 3 MemBlock(64)
    -> TPool(1) -> conv stride 2 -> 3 MemBlock(64) -> conv 64->16
    MemBlock(x, past) = ReLU(conv(ReLU(conv(ReLU(conv(cat[x, past]))))) + x), past = the block's input one frame earlier
    TPool(stride): `stride` consecutive frames concatenated on the channel axis (frame 2t first) -> bias-free 1x1 conv to 64

tests/test_taehv_enc_host.py holds it against the real reference's output (tests/golden/taehv_enc_tiny.pt).
"""
import torch
import torch.nn.functional as F

POOL = [2, 2, 1]
MEMBLOCKS = [4, 5, 6, 9, 10, 11, 14, 15, 16]


class TaehvEncRef:
    """encode(px [T, 3, H, W] in [0, 1], T % 4 == 0) -> [T / 4, 16, H / 8, W / 8] continuing the current video; reset() starts a
    new one."""

    def __init__(self, sd, dtype=torch.float32, device="cpu"):
        self.sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items() if k.startswith("encoder.")}
        self.dtype, self.device = dtype, device
        self.mem = {}

    def reset(self):
        self.mem = {}

    def _conv(self, x, key, bias=True, stride=1):
        return F.conv2d(x, self.sd[key + ".weight"], self.sd[key + ".bias"] if bias else None, padding=1, stride=stride)

    def _memblock(self, x, i):
        """x [T, C, H, W]: consecutive frames of the video at this level"""
        first = self.mem.get(i)
        if first is None:
            first = torch.zeros_like(x[:1])
        past = torch.cat([first, x[:-1]], 0)
        self.mem[i] = x[-1:].clone()
        h = F.relu(self._conv(torch.cat([x, past], 1), f"encoder.{i}.conv.0"))
        h = F.relu(self._conv(h, f"encoder.{i}.conv.2"))
        return F.relu(self._conv(h, f"encoder.{i}.conv.4") + x)

    def encode(self, px):
        if px.shape[0] % 4:
            raise ValueError(f"{px.shape[0]} frames: not a multiple of 4")
        x = F.relu(self._conv(px.to(device=self.device, dtype=self.dtype), "encoder.0"))
        i = 2
        for s in POOL:
            t, c, h, w = x.shape
            x = F.conv2d(x.reshape(t // s, s * c, h, w), self.sd[f"encoder.{i}.conv.weight"])
            x = self._conv(x, f"encoder.{i + 1}", bias=False, stride=2)
            i += 2
            for _ in range(3):
                x = self._memblock(x, i)
                i += 1
        return self._conv(x, "encoder.17")


def encode_video(sd, px, dtype=torch.float32, device="cpu", split=None):
    """One video from zero memories, optionally in several calls (``split``: pixel frames per call)."""
    m = TaehvEncRef(sd, dtype, device)
    parts, f0 = [], 0
    for n in (split or [px.shape[0]]):
        parts.append(m.encode(px[f0:f0 + n]))
        f0 += n
    return torch.cat(parts, 0)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
