"""TEST INFRASTRUCTURE — Pillow's 8-bit separable resize as plain numpy integer arithmetic.

`Image.resize(size, Image.LANCZOS)` on an RGB image is a horizontal pass into a uint8 intermediate followed by a vertical pass
(a pass whose sizes are equal is left out); per pass and output index o, with the table of `packing.resample_table`:
    acc = 2^21 + sum_j src[first(o) + j] * coef[o][j]   (int32),   value = clamp(acc >> 22, 0, 255)   (arithmetic shift)
This file gives the whole expected image, so that a failing comparison can say where it differs.  Nothing under
sd-webui-text2video_amd/ imports it.
"""
import hashlib

import numpy as np

from sd_webui_text2video_amd import packing as pk


def resample_pass(src: np.ndarray, coef: np.ndarray, bounds: np.ndarray, axis: int) -> np.ndarray:
    """src uint8 [N, H, W, 3]; axis 0 = horizontal (W -> len(coef)), 1 = vertical (H -> len(coef))."""
    a = src if axis == 0 else src.transpose(0, 2, 1, 3)                  # resampled axis at position 2
    out = np.empty(a.shape[:2] + (coef.shape[0], 3), dtype=np.uint8)
    for o in range(coef.shape[0]):
        first, count = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (a[:, :, first:first + count, :].astype(np.int64) * coef[o, :count].astype(np.int64)[None, None, :, None]).sum(axis=2)
        acc = (acc + (1 << 21)).astype(np.int32)                         # (wraps like the C int; never happens for Lanczos tables)
        out[:, :, o, :] = np.clip(acc >> 22, 0, 255)
    return out if axis == 0 else np.ascontiguousarray(out.transpose(0, 2, 1, 3))


def resample_ref(frames: np.ndarray, height: int, width: int) -> np.ndarray:
    """uint8 [N, H, W, 3] (or one image [H, W, 3]) -> uint8 [N, height, width, 3]: what Pillow's Lanczos resize gives per frame."""
    single = frames.ndim == 3
    x = np.ascontiguousarray(frames[None] if single else frames)
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[-1] == 3
    if x.shape[2] != width:
        x = resample_pass(x, *pk.resample_table(x.shape[2], width), axis=0)
    if x.shape[1] != height:
        x = resample_pass(x, *pk.resample_table(x.shape[1], height), axis=1)
    return x[0] if single else x


def make_input(kind: str, seed: int, h: int, w: int, block: int = 0) -> np.ndarray:
    """The fixture's inputs, reproducible without storing them: the frozen legacy random stream, or a checkerboard of 0 / 255 blocks."""
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checkerboard":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy // block + xx // block) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    raise ValueError(kind)


def case_input(case: dict) -> np.ndarray:
    """-> uint8 [N, H, W, 3]: frame f of a clip comes from seed + f."""
    h, w = case["src"]
    return np.stack([make_input(case["kind"], case["seed"] + f, h, w, case.get("block", 0)) for f in range(case["frames"])])


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
