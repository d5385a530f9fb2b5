"""TEST INFRASTRUCTURE — the VideoCrafter depth adapter and its injection into the LVDM UNet as plain torch, written from the
formulas (lvdm/models/modules/adapter.py:39-105, ddpm3d.py:1463-1464, openaimodel3d.py:654-663).  The reference itself is not on
the GPU machine; tests/test_adapter_cpu.py pins this file against the live reference where it is present and against the committed
goldens everywhere.  Nothing under sd-webui-text2video_amd/ imports it.
"""
import math

import torch
import torch.nn.functional as F

from oracle import torch_port as tp

OPTION_SETS = {                      # the three configurations the reference can run (tests/golden/make_golden_adapter.py)
    "t2i": dict(nums_rb=2, ksize=1, sk=True, use_conv=False),
    "full": dict(nums_rb=3, ksize=3, sk=True, use_conv=True),
    "conv": dict(nums_rb=2, ksize=1, sk=True, use_conv=True),
}


def normalise_depth(d: torch.Tensor) -> torch.Tensor:
    """[n, 1, H, W]: 2 (d - min) / (max - min + 1e-7) - 1 over each frame, in the reference's operation order."""
    mn, mx = torch.amin(d, dim=[1, 2, 3], keepdim=True), torch.amax(d, dim=[1, 2, 3], keepdim=True)
    return 2. * (d - mn) / (mx - mn + 1e-7) - 1.


def adapter_forward(sd, x, *, channels, nums_rb, ksize, sk, use_conv, cin=64):
    """x [n, 1, H, W] -> list of [n, c_i, h_i, w_i]."""
    ps = ksize // 2

    def conv(key, v, k, stride=1):
        return F.conv2d(v, sd[key + ".weight"].float(), sd[key + ".bias"].float(), stride=stride, padding=k // 2)

    x = F.pixel_unshuffle(x.float(), 8)
    assert x.shape[1] == cin and ps in (0, 1)
    x = conv("conv_in", x, 3)
    feats = []
    for i, c in enumerate(channels):
        for j in range(nums_rb):
            p = f"body.{i * nums_rb + j}"
            in_c = channels[i - 1] if (i and j == 0) else c
            if i and j == 0:
                x = conv(p + ".down_opt.op", x, 3, stride=2) if use_conv else F.avg_pool2d(x, 2, 2)
            if in_c != c or not sk:
                x = conv(p + ".in_conv", x, ksize)
            h = conv(p + ".block2", F.relu(conv(p + ".block1", x, 3)), ksize)
            x = h + (x if sk else conv(p + ".skep", x, ksize))
        feats.append(x)
    return feats


def lvdm_unet_forward_features(sd, cfg, x, t, context, feats):
    """oracle.torch_port.lvdm_unet_forward with `features_adapter`: feats[k] ([b', c, t, h, w], b' = b or broadcastable) is added to the
    result of the k-th input block with (id + 1) % 3 == 0, before it goes on the skip stack."""
    mc, heads, rel = cfg["model_channels"], cfg["num_heads"], cfg["temporal_length"]
    half = mc // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    emb = tp._lin(sd, "time_embed.2", F.silu(tp._lin(sd, "time_embed.0", torch.cat([torch.cos(args), torch.sin(args)], dim=-1))))
    inputs, middle, outputs = tp._lvdm_layout(cfg)

    def run(prefix, parts, h):
        for j, (kind, cin, cout) in enumerate(parts):
            p = f"{prefix}.{j}"
            if kind == "stem":
                h = tp._conv3d(sd, p, h)
            elif kind == "res":
                h = tp._lvdm_res(sd, p, h, emb)
            elif kind == "st":
                h = tp._lvdm_st(sd, p, h, context, heads, rel)
            elif kind == "down":
                h = tp._conv3d(sd, p + ".op", h, stride=2)
            else:
                h = F.interpolate(h, (h.shape[2], h.shape[3] * 2, h.shape[4] * 2), mode="nearest")
                h = tp._conv3d(sd, p + ".conv", h)
        return h

    hs, h, k = [], x.float(), 0
    for idx, (prefix, parts) in enumerate(inputs):
        h = run(prefix, parts, h)
        if (idx + 1) % 3 == 0 and feats is not None:
            f = feats[k].float()
            h = h + (f if f.shape[0] == h.shape[0] else f.repeat(h.shape[0] // f.shape[0], 1, 1, 1, 1))
            k += 1
        hs.append(h)
    assert feats is None or k == len(feats), "Mismatch features adapter"
    h = run("middle_block", middle, h)
    for prefix, parts in outputs:
        h = run(prefix, parts, torch.cat([h, hs.pop()], dim=1))
    return tp._conv3d(sd, "out.2", F.silu(tp._gn(sd, "out.0", h, 1e-5)))


# ---- seeded inputs shared by tests/golden/make_golden_adapter.py and the tests -----------------------------------------------------
SMALL = dict(channels=[32, 64, 64], cin=64)          # case 1: 5 frames of 64 x 48 (not square)
RELEASED = dict(channels=[320, 640, 1280, 1280], cin=64, **OPTION_SETS["t2i"])     # the 77 M-parameter T2I-Adapter shape
STRIDES = (5, 8, 2, 2)                               # case 4: stored samples feat[::5, ::8, ::2, ::2] of every [16, c, h, w] feature


def small_depth() -> torch.Tensor:
    """Raw (un-normalised) depth [5, 1, 64, 48]; frame 2 is constant (normalises to exactly -1)."""
    g = torch.Generator().manual_seed(31)
    d = torch.rand(5, 1, 64, 48, generator=g) * 7.5 + 0.25
    d[2] = 3.7
    return d


def tiny_feature() -> torch.Tensor:
    """One feature for TINY_LVDM_UNET's single site (input block 2: 320 channels at half the 8 x 8 latent), two samples."""
    return torch.randn(2, 320, 5, 4, 4, generator=torch.Generator().manual_seed(41)) * 0.5


def released_depth() -> torch.Tensor:
    """Raw depth clip [1, 1, 16, 256, 256]."""
    return torch.rand(1, 1, 16, 256, 256, generator=torch.Generator().manual_seed(51)) * 10.0 + 1.0


def subsample(f: torch.Tensor) -> torch.Tensor:
    a, b, c, d = STRIDES
    return f[::a, ::b, ::c, ::d]
