"""Generate the torch_to_np golden FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_frames.py          # torch_to_np_designed.npz, a second on a CPU

The reference's own `torch_to_np` (videocrafter/sample_utils.py:98-107), unmodified, converts the designed inputs of
tests/frames_inputs.py.  sample_utils.py imports its LoRA and config helpers at module top; they import under the stubs of
oracle/ref_bootstrap.py, and none of them is called.  Stored, per element (the function is elementwise; the layout is the tests'):
  f32_in / f32_out        the fp32 inputs and their bytes
  f32_half_out            the bytes of the same inputs rounded to fp16 first (`.half().float()`): an fp32 token tensor of an fp16 model
  f16_in / f16_out        every non-NaN fp16 value (stored as its bit pattern) and the bytes of its `.float()` — what the product's
                          `torch_to_np` hands the arithmetic for an fp16 video."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frames_inputs as FI  # noqa: E402
from oracle import ref_bootstrap as rb  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    rb.bootstrap()
    su = importlib.import_module("videocrafter.sample_utils")

    def ref(flat: torch.Tensor) -> np.ndarray:
        """The reference function on a [n, 1, 1, 1] 'batch of images' -> its bytes [n]."""
        out = su.torch_to_np(flat.view(-1, 1, 1, 1))
        assert out.dtype == torch.uint8 and out.shape == (flat.numel(), 1, 1, 1)
        return out.reshape(-1).numpy()

    f32 = torch.from_numpy(FI.f32_inputs())
    f16 = torch.from_numpy(FI.f16_inputs())
    out = dict(f32_in=f32.numpy(), f32_out=ref(f32), f32_half_out=ref(f32.half().float()),
               f16_in=f16.numpy().view(np.uint16), f16_out=ref(f16.float()))
    for k in ("f32_out", "f32_half_out", "f16_out"):
        print(k, out[k].shape, "distinct bytes:", len(np.unique(out[k])))
    np.savez_compressed(os.path.join(OUT, "torch_to_np_designed.npz"), **out)


if __name__ == "__main__":
    main()
