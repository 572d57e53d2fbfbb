"""Restatement of the TAEHV decoder (the reference's demo_utils/taehv.py, ``TAEHV.decode_video``) for tests at sizes the committed
fixture does not hold.  Written from the layer list, plain ``torch.nn.functional`` on a state dict in the reference's keys:

    Clamp (tanh(x / 3) * 3) -> conv 16->256 + ReLU -> 3 MemBlock(256) -> Upsample x2 -> TGrow(256, 1) -> conv 256->128 (no bias)
    -> 3 MemBlock(128) -> Upsample x2 -> TGrow(128, 2) -> conv 128->64 (no bias) -> 3 MemBlock(64) -> Upsample x2 -> TGrow(64, 2)
    -> conv 64->64 (no bias) -> ReLU -> conv 64->3
    MemBlock(x, past) = ReLU(conv(ReLU(conv(ReLU(conv(cat[x, past]))))) + x), past = the block's input one frame earlier
    TGrow(stride): 1x1 conv to stride * C channels, re-read as `stride` consecutive frames

tests/test_taehv_host.py holds it against the real reference's output (tests/golden/taehv_tiny.pt).
"""
import torch
import torch.nn.functional as F

CH = [256, 128, 64, 64]
GROW = [1, 2, 2]
TGROW_KEYS = {"decoder.7.conv.weight": 256, "decoder.13.conv.weight": 256, "decoder.19.conv.weight": 128}


def patch_tgrow(sd):
    """A TGrow weight with more rows than the model keeps its LAST channels * stride rows."""
    sd = dict(sd)
    for k, rows in TGROW_KEYS.items():
        if sd[k].shape[0] > rows:
            sd[k] = sd[k][-rows:]
    return sd


class TaehvRef:
    """decode(z [T, 16, h, w]) -> [4T, 3, 8h, 8w] continuing the current video; reset() starts a new one."""

    def __init__(self, sd, dtype=torch.float32, device="cpu"):
        self.sd = {k: v.to(device=device, dtype=dtype) for k, v in patch_tgrow(sd).items() if k.startswith("decoder.")}
        self.dtype, self.device = dtype, device
        self.mem = {}

    def reset(self):
        self.mem = {}

    def _conv(self, x, key, bias=True):
        return F.conv2d(x, self.sd[key + ".weight"], self.sd[key + ".bias"] if bias else None, padding=1)

    def _memblock(self, x, i):
        """x [T, C, H, W]: consecutive frames of the video at this level"""
        first = self.mem.get(i)
        if first is None:
            first = torch.zeros_like(x[:1])
        past = torch.cat([first, x[:-1]], 0)
        self.mem[i] = x[-1:].clone()
        h = F.relu(self._conv(torch.cat([x, past], 1), f"decoder.{i}.conv.0"))
        h = F.relu(self._conv(h, f"decoder.{i}.conv.2"))
        return F.relu(self._conv(h, f"decoder.{i}.conv.4") + x)

    def decode(self, z):
        x = torch.tanh(z.to(device=self.device, dtype=self.dtype) / 3) * 3
        x = F.relu(self._conv(x, "decoder.1"))
        i = 3
        for lvl in range(3):
            for _ in range(3):
                x = self._memblock(x, i)
                i += 1
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            i += 1
            t, c, h, w = x.shape
            x = F.conv2d(x, self.sd[f"decoder.{i}.conv.weight"]).reshape(t * GROW[lvl], c, h, w)
            x = self._conv(x, f"decoder.{i + 1}", bias=False)
            i += 2
        return self._conv(F.relu(x), "decoder.22")


def decode_video(sd, z, dtype=torch.float32, device="cpu", split=None):
    """One video from zero memories, optionally in several calls (``split``: latent frames per call)."""
    m = TaehvRef(sd, dtype, device)
    parts, f0 = [], 0
    for n in (split or [z.shape[0]]):
        parts.append(m.decode(z[f0:f0 + n]))
        f0 += n
    return torch.cat(parts, 0)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
