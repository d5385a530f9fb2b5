"""Context windows: the float64 restatement of the schedule, the gather and the blend in plain torch, and the designed operands of
tests/test_context_windows_cpu.py and tests/test_gpu_context_windows.py.

The restatement follows include/t2v_hip.h (T2V_OP_LINCOMB forms i[9] = 2 and 1) and `samplers.ContextWindows`, not their code:
  starts      0, stride, 2 * stride, ... while start + length < F, then F - length
  batch row   v * nW + w is window w of video v
  gather      xw[row, c, j] = x[v, c, starts[w] + j]
  blend       out[role, v, c, f] = sum_w wgt[f - starts[w]] * e[role, v * nW + w, c, f - starts[w]] / sum_w wgt[f - starts[w]]
              over the windows that hold f
  forwards    the rows go in ascending chunks; a guided forward returns [cond (rows of the chunk) | uncond (rows of the chunk)]

The shapes are the smallest at which the kernels can still go wrong: V = 2, C = 4, F = 11 with windows of 4 frames and overlap 1, 2, 3
(a frame lies in 1 to 4 windows; with overlap 1 and 2 the flush-right last window overlaps its neighbour by 3 frames, more than `overlap`;
with overlap 3 the stride is 1 and the last window sits on the stride grid), HW = 6 (12 or 24 bytes per frame: the scalar paths) and
HW = 16 (the 16-byte paths), eps fp16 and fp32, guided and not, and forwards of all, 1 and 3 windows.

Operands carry their coordinates: every eps element is a distinct fp16-representable value, a function of (role, v, w, c, j, pixel) alone,
so that any mix-up of indices lands on another value; the weights are a designed table without symmetry (the pyramid reads the same
from both ends, which would hide a reversed index)."""
import itertools

import torch

V, C, F, LENGTH = 2, 4, 11, 4
OVERLAPS = (1, 2, 3)
HWS = ((2, 3), (4, 4))              # (h, w): HW = 6 and 16
BATCHES = (None, 1, 3)
DESIGNED_WEIGHTS = (1.0, 2.5, 0.75, 4.0)
PAD = 64                            # fence elements either side of a dense tensor (keeps 16-byte alignment for both dtypes)
TOL = 8 * 2.0 ** -24                # |out - ref| <= TOL * (sum_w wgt |e|) / (sum_w wgt)

BLEND_SHAPES = [dict(overlap=o, hw=hw, dtype=dt, guided=g) for o, hw, dt, g in
                itertools.product(OVERLAPS, HWS, (torch.float16, torch.float32), (True, False))]
GATHER_SHAPES = [dict(overlap=o, hw=hw, dtype=dt, batch=b) for o, hw, dt, b in
                 itertools.product(OVERLAPS, HWS, (torch.float16, torch.float32), BATCHES)]


def shape_id(s):
    return "-".join(f"{k}{'x'.join(map(str, v)) if isinstance(v, tuple) else str(v).replace('torch.', '')}" for k, v in s.items())


# ---- the schedule ------------------------------------------------------------------------------------------------------------------------
def starts_ref(frames, length, overlap):
    stride, out, s = length - overlap, [], 0
    while s + length < frames:
        out.append(s)
        s += stride
    last = max(frames - length, 0)
    if not out or out[-1] != last:
        out.append(last)
    return out


def weights_ref(length, kind):
    return [float(min(j + 1, length - j)) if kind == "pyramid" else 1.0 for j in range(length)]


def chunks_ref(rows, batch):
    b = rows if batch is None else batch
    return [(r, min(b, rows - r)) for r in range(0, rows, b)]


# ---- gather and blend ----------------------------------------------------------------------------------------------------------------------
def gather_ref(x, starts, length, row0, rows):
    nW = len(starts)
    return torch.stack([x[r // nW, :, starts[r % nW]:starts[r % nW] + length] for r in range(row0, row0 + rows)])


def assemble_ref(chunks, roles, n_rows, uncond_at="chunk"):
    """The forwards' eps, each [roles * rows_k, ...] = [cond (rows_k) | uncond (rows_k)], -> [roles, n_rows, ...].
    uncond_at="batch" is the mutation: the unconditional half is looked for n_rows rows behind the conditional one, where it would lie
    had all windows gone through one forward (the rows of all forwards as one buffer, wrapping at its end)."""
    flat = torch.cat(list(chunks), dim=0)
    out = torch.empty((roles, n_rows) + tuple(flat.shape[1:]), dtype=flat.dtype)
    base = row0 = 0
    for e in chunks:
        r = e.shape[0] // roles
        for role in range(roles):
            off = role * (r if uncond_at == "chunk" else n_rows)
            idx = [(base + off + i) % flat.shape[0] for i in range(r)]
            out[role, row0:row0 + r] = flat[idx]
        base, row0 = base + roles * r, row0 + r
    return out


def blend_ref(e, starts, weights, videos, frames, *, shift=0, normalise="weights", reverse=False, order="vw", swap_roles=False):
    """e [roles, videos * nW, C, length, h, w] -> (out [roles, videos, C, frames, h, w] float64, bound: the same shape).
    The keywords are the mutations of tests/test_context_windows_cpu.py: `shift` moves every start, normalise="count" divides by the
    number of windows, `reverse` reads the weight table backwards, order="wv" takes batch row w * videos + v, `swap_roles` exchanges
    the conditional and unconditional halves."""
    roles, nW, length = e.shape[0], len(starts), e.shape[3]
    e64 = e.double()
    wg = [float(w) for w in (reversed(weights) if reverse else weights)]
    out = torch.zeros((roles, videos, e.shape[2], frames) + tuple(e.shape[4:]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for f in range(frames):
        wsum = count = 0.0
        for w, s in enumerate(starts):
            j = f - (s + shift)
            if not 0 <= j < length:
                continue
            for v in range(videos):
                row = v * nW + w if order == "vw" else w * videos + v
                for role in range(roles):
                    src = e64[(roles - 1 - role) if swap_roles else role, row, :, j]
                    out[role, v, :, f] += wg[j] * src
                    mag[role, v, :, f] += wg[j] * src.abs()
            wsum, count = wsum + wg[j], count + 1
        div = wsum if normalise == "weights" else count
        if div == 0:                   # (a mutated table may leave a frame out: the restatement says NaN, as a division by zero would)
            out[:, :, :, f] = float("nan")
            continue
        out[:, :, :, f] /= div
        mag[:, :, :, f] /= wsum
    return out, TOL * mag


# ---- designed operands ---------------------------------------------------------------------------------------------------------------------
def _coded(n, salt):
    """n distinct fp16 values between 0.125 and 8192 in a scrambled order, signs mixed: value k of a tensor is a function of k alone."""
    assert n <= 0x8000
    k = torch.arange(n, dtype=torch.int64)
    code = (k * 5003 + salt) % 0x8000               # 5003 is odd: a permutation of the 2^15 codes = 2^14 magnitudes x 2 signs
    bits = (0x3000 + (code >> 1)).to(torch.int16)
    val = bits.view(torch.float16).float()
    return torch.where((code & 1) == 1, -val, val)


def latent_operand(hw, dtype):
    """x [V, C, F, h, w]: a distinct value per (v, c, f, pixel)."""
    n = V * C * F * hw[0] * hw[1]
    return _coded(n, 17).reshape(V, C, F, *hw).to(dtype)


def eps_operand(roles, n_windows, hw, dtype):
    """e [roles, V * nW, C, LENGTH, h, w]: a distinct value per (role, v, w, c, j, pixel)."""
    shape = (roles, V * n_windows, C, LENGTH) + tuple(hw)
    n = 1
    for d in shape:
        n *= d
    return _coded(n, 911).reshape(shape).to(dtype)


def split_chunks(e, batch):
    """e [roles, N, ...] -> the eps of the forwards, each [roles * rows_k, ...] = [cond (rows_k) | uncond (rows_k)]."""
    return [torch.cat([e[r, r0:r0 + n] for r in range(e.shape[0])], dim=0).contiguous() for r0, n in chunks_ref(e.shape[1], batch)]


def fenced(t, device=None, skew=0, fill=True):
    """-> (big, view): a dense view shaped like `t`, PAD + skew elements inside a NaN-filled allocation (skew = 1 takes the base off
    every 16-byte boundary); fill=False leaves the view NaN too (an output)."""
    big = torch.full((t.numel() + 2 * PAD + skew,), float("nan"), dtype=t.dtype, device=device or t.device)
    view = big[PAD + skew:PAD + skew + t.numel()].view(t.shape)
    if fill:
        view.copy_(t)
    return big, view


def fence_intact(big, n, skew=0):
    return bool(torch.isnan(big[:PAD + skew]).all()) and bool(torch.isnan(big[PAD + skew + n:]).all())


# ---- the two kernel helpers of samplers.py on the CPU --------------------------------------------------------------------------------------
def window_gather_cpu(xw, x, starts_d, row0):
    xw.copy_(gather_ref(x, starts_d.tolist(), xw.shape[2], row0, xw.shape[0]))
    return xw


def window_blend_cpu(out, chunks, starts_d, weights_d, roles):
    starts = starts_d.tolist()
    videos = out.shape[0] // roles
    e = assemble_ref(chunks, roles, videos * len(starts))
    ref, _ = blend_ref(e, starts, weights_d.tolist(), videos, out.shape[2])
    out.copy_(ref.reshape(out.shape).to(out.dtype))
    return out
