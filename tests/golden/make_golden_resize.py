"""Generator of tests/golden/resize_lanczos.npz — run ONCE on a machine where Pillow is installed:

    python tests/golden/make_golden_resize.py

Per case it records what `Image.fromarray(frame).resize((W', H'), Image.LANCZOS)` returns for reproducible inputs
(tests/resample_ref.make_input: numpy's frozen legacy random stream, or a 0 / 255 checkerboard): the SHA-256 of the output bytes
of all frames, the first 256 output bytes, and whether any output byte is saturated (0 or 255).  The Pillow version is recorded.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

CASES = [
    dict(name="zeroscope_up", kind="random", seed=101, src=(320, 576), dst=(576, 1024), frames=1),
    dict(name="down_aspect", kind="random", seed=102, src=(576, 1024), dst=(256, 256), frames=1),
    dict(name="odd_sizes", kind="random", seed=103, src=(187, 333), dst=(256, 256), frames=1),
    dict(name="small", kind="random", seed=104, src=(75, 100), dst=(64, 64), frames=1),
    dict(name="width_only", kind="random", seed=105, src=(80, 144), dst=(80, 256), frames=1),
    dict(name="height_only", kind="random", seed=106, src=(80, 144), dst=(144, 144), frames=1),
    dict(name="checker3_up", kind="checkerboard", seed=0, block=3, src=(320, 576), dst=(576, 1024), frames=1),
    dict(name="checker5_down", kind="checkerboard", seed=0, block=5, src=(576, 1024), dst=(320, 576), frames=1),
    dict(name="wide_rows", kind="random", seed=109, src=(1080, 1920), dst=(576, 1024), frames=1),
    dict(name="up16", kind="random", seed=110, src=(64, 64), dst=(1024, 1024), frames=1),
    dict(name="clip24", kind="random", seed=200, src=(320, 576), dst=(576, 1024), frames=24),
]


def main():
    import PIL
    from PIL import Image
    import resample_ref as rr
    meta, heads = [], []
    for case in CASES:
        x = rr.case_input(case)
        h2, w2 = case["dst"]
        out = np.stack([np.asarray(Image.fromarray(f).resize((w2, h2), Image.LANCZOS)) for f in x])
        sat = bool(((out == 0) | (out == 255)).any())
        meta.append(dict(case, sha256=rr.digest(out), saturates=sat))
        heads.append(out.reshape(-1)[:256].copy())
        print(f"{case['name']:14s} {case['src']} -> {case['dst']} x{case['frames']}  saturates={sat}  {meta[-1]['sha256'][:16]}")
    np.savez(os.path.join(HERE, "resize_lanczos.npz"), meta=np.array(json.dumps(dict(pillow=PIL.__version__, cases=meta))),
             head=np.stack(heads))


if __name__ == "__main__":
    main()
