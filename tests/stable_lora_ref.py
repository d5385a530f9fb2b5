"""The arithmetic contract of the Stable LoRA merge (T2V_OP_LORA_MERGE, include/t2v_hip.h) in numpy, independent of the
package: the fp16 contract step by step (sequential fp32 sums, one rounding per step — numpy's float32 ops and its float32 -> float16
conversion are IEEE round-to-nearest-even), a float64 evaluation with the magnitude sum that the fp32 tolerance is built from, and the
golden file's contents in the form the tests use."""
import hashlib
import json
import os

import numpy as np

DIRECT, TEMPORAL = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stable_lora_tiny.npz")


def merge_f16(W, A, B, alpha, form=DIRECT):
    """W fp16 (any shape, N J elements), A fp16 [r, Jf], B fp16 [N, r] -> the merged fp16 weight (a new array)."""
    assert W.dtype == A.dtype == B.dtype == np.float16
    N, r = B.shape
    Jf = A.shape[1]
    s = np.zeros((N, Jf), dtype=np.float32)
    for k in range(r):                                   # ascending k; the fp16 x fp16 product is exact in fp32: one rounding, the add's
        s = s + B[:, k:k + 1].astype(np.float32) * A[k:k + 1, :].astype(np.float32)
    d = s.astype(np.float16)
    if form == TEMPORAL:
        d3 = d.astype(np.float32).reshape(N, Jf // 3, 3)
        d = (((d3[..., 0] + d3[..., 1]) + d3[..., 2]) / np.float32(3)).astype(np.float16)
    e = (d.astype(np.float32) * np.float32(alpha)).astype(np.float16)
    return (W.reshape(N, -1).astype(np.float32) + e.astype(np.float32)).astype(np.float16).reshape(W.shape)


def merge_f64(W, A, B, alpha, form=DIRECT):
    """float64 evaluation -> (w*, S): the exact merged weight and S = sum_k |B| |A| per element (temporal form: the mean of the three)."""
    N, r = B.shape
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    d, S = B64 @ A64, np.abs(B64) @ np.abs(A64)
    if form == TEMPORAL:
        d, S = d.reshape(N, -1, 3).mean(-1), S.reshape(N, -1, 3).mean(-1)
    alpha = np.float64(np.float32(alpha))
    return (W.reshape(N, -1).astype(np.float64) + alpha * d).reshape(W.shape), S.reshape(W.shape)


def f32_bound(w_star, S, alpha, r):
    """2 x [(r + 5) 2^-24 |alpha| S + 2^-24 |w*|]: twice the first-order bound of the r + 5 roundings of the fp32 path (r - 1 adds and r products
    of the sum folded into <= r, the rounding of d, the mean's two adds and division, the product with alpha; then the final add's own)."""
    u = 2.0 ** -24
    return 2.0 * ((r + 5) * u * abs(float(np.float32(alpha))) * S + u * np.abs(w_star))


def digest(arr) -> str:
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def golden():
    """-> dict: file1 / file2 {key: numpy array} in key order, touched, untouched, alpha, sha_* lists over touched + untouched, eps_merged,
    call_sequence."""
    z = np.load(GOLDEN)
    out = {k: z[k] for k in ("eps_merged", "separation_over_gate")}
    out["file1"] = {str(k): z[f"a{i}"] for i, k in enumerate(z["keys1"])}
    out["file2"] = {str(k): z[f"b{i}"] for i, k in enumerate(z["keys2"])}
    out["touched"], out["untouched"] = [str(n) for n in z["touched"]], [str(n) for n in z["untouched"]]
    out["alpha"] = float(z["alpha"])
    for k in ("sha_original", "sha_merged", "sha_undone", "sha_two_files"):
        out[k] = [str(s) for s in z[k]]
    out["call_sequence"] = json.loads(str(z["call_sequence"]))
    return out
