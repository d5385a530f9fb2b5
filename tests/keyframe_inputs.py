"""Keyframe inpainting of DDIM_Gaussian (T2V_OP_DDIM_STEP mode 4, `GaussianDiffusion.sample(inpaint="legacy")`): what the tests share.

  * the torch restatement of the record (include/t2v_hip.h): the mode-0 update in fp32, every operation rounded by itself, then
        bin = mask <= v ? 0 : 1;   known = f6 * orig + f7 * n;   out = known * (1 - bin) + x1 * bin
    with the wrong implementations a kernel or a binding could be (MUTANTS);
  * designed operands for the kernel (`kernel_case`): mask weights at, just above and just below the threshold, 0 and 1, negative and
    above 1, infinite and NaN, and non-finite fences in `original` under free elements and in the step's own operands under held ones;
  * the cases and inputs of the golden runs of the reference's legacy loop (tests/golden/make_golden_inpaint.py).
No GPU and no reference is needed to import this."""
import os
import struct

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelscope_inpaint_tiny.npz")
F32 = torch.float32


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _t(v):
    return torch.tensor(float(v), dtype=F32)


def guided_eps(eps_pair, guided: int, gscale, videos: int):
    """e = e_u + g (e_c - e_u) over each video's first `guided` channels, the conditional prediction elsewhere."""
    e = eps_pair[0:videos].float()
    if guided:
        u = eps_pair[videos:2 * videos].float()
        e = torch.cat([u[:, :guided] + _t(gscale) * (e[:, :guided] - u[:, :guided]), e[:, guided:]], dim=1)
    return e


def plain_step(xt, eps_pair, noise, coef, guided: int):
    """Mode 0 in fp32, every operation rounded by itself (the kernel of the plain record may contract: equal to rounding, not bits)."""
    f = [_t(c) for c in coef]
    e = guided_eps(eps_pair, guided, coef[5], xt.shape[0])
    ax = f[0] * xt.float()
    x0 = ax - f[1] * e
    eps = (ax - x0) / f[1]
    r = f[2] * x0 + f[3] * eps
    if noise is not None and float(coef[4]) != 0.0:
        r = r + f[4] * noise
    return r


def f32_bits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def keyframe_blend(x1, original, mask, qnoise, qcoef, v: float, mutant=None, xt=None):
    """The blend of the record on a given x1.  `mutant`: one of MUTANTS (a wrong implementation), None: the contract."""
    thr = _t(v)                                           # the fp32 threshold the record carries
    if mutant == "threshold compared in float64":
        held = mask.double() <= float(v)
    elif mutant == "< instead of <=":
        held = mask < thr
    else:
        held = mask <= thr                                # a NaN weight compares false: free
    if mutant == "the mask of the next sample in the batch":
        held = torch.roll(held, -1, dims=0)
    bin_ = torch.where(held, torch.zeros_like(mask), torch.ones_like(mask))
    if mutant == "inverted polarity":
        bin_ = 1 - bin_
    src = xt if mutant == "known taken from xt" else original
    f6, f7 = (_t(qcoef[1]), _t(qcoef[0])) if mutant == "f6 and f7 swapped" else (_t(qcoef[0]), _t(qcoef[1]))
    known = f6 * src
    if qnoise is not None:
        known = known + f7 * qnoise
    return known * (1 - bin_) + x1 * bin_


def keyframe_step(xt, eps_pair, noise, coef, guided, original, mask, qnoise, qcoef, v, mutant=None, x1=None):
    """The whole record.  `x1`: the update part taken from elsewhere (a plain mode-0 launch on the GPU) instead of `plain_step`."""
    if mutant == "blend before the eta noise":
        quiet = list(coef)
        quiet[4] = 0.0
        r = keyframe_blend(plain_step(xt, eps_pair, None, quiet, guided), original, mask, qnoise, qcoef, v, xt=xt)
        return r + _t(coef[4]) * noise if (noise is not None and float(coef[4]) != 0.0) else r
    if x1 is None:
        x1 = plain_step(xt, eps_pair, noise, coef, guided)
    return keyframe_blend(x1, original, mask, qnoise, qcoef, v, mutant, xt=xt)


MUTANTS = ("< instead of <=", "inverted polarity", "known taken from xt", "f6 and f7 swapped", "blend before the eta noise",
           "threshold compared in float64", "the mask of the next sample in the batch")


def keyframe_update_cpu(out, xt, eps_pair, noise, coef, guided, original, mask, qnoise, qcoef, v):
    """Stands in for `samplers._ddim_update_keyframe` on the host."""
    out.copy_(keyframe_step(xt, eps_pair, noise, coef, guided, original, mask, qnoise, qcoef, v))
    return out


# ---- designed operands for the kernel ----------------------------------------------------------------------------------------------
V = 0.6          # (5 - 1 - 1) / 5: not an fp32 number, so fp32(V) > V and a weight of fp32(V) separates the two precisions
KERNEL_SHAPES = [(1, 4, 45), (2, 4, 200), (1, 4, 1792)]      # [videos, channels, inner]
COEF = (1.7320508, 1.4142135, 0.8660254, 0.4330127, 0.25, 3.0)       # f[0..5] of a mid-schedule step with eta noise (f4) and scale 3
QCOEF = (0.8, 0.6)


def special_weights():
    v32 = np.float32(V)
    up, down = np.nextafter(v32, np.float32(np.inf)), np.nextafter(v32, np.float32(-np.inf))
    #        weight                held?
    return [(float(v32), True), (float(up), False), (float(down), True), (0.0, True), (1.0, False), (-0.25, True), (1.5, False),
            (float("nan"), False), (float("inf"), False), (float("-inf"), True)]


def kernel_case(shape, eps_dtype=torch.float32, eta=True, seed=0):
    """-> dict of operands [videos, channels, inner] and what the case expects per element:
      held        where the weight is <= fp32(V)
      fence_orig  free elements whose `original` is NaN or +-inf: the arithmetic blend gives NaN there (inf * 0)
      fence_x1    held elements whose step is not finite (x_t or the eta noise inf / NaN): NaN there as well
    The second video of a batch has its own mask and original; the special weights stand in every channel's row at other columns."""
    B, C, inner = shape
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    xt, original, qnoise, noise = r(B, C, inner), r(B, C, inner) * 2 + 0.5, r(B, C, inner), r(B, C, inner)
    eps_pair = r(2 * B, C, inner).to(eps_dtype)
    mask = torch.rand(B, C, inner, generator=g)                                      # both sides of V, none by accident within 0.025 of it
    mask = torch.where((mask - V).abs() < 0.025, torch.full_like(mask, 0.3), mask)
    sp = special_weights()
    for b in range(B):
        for c in range(C):
            for k, (w, _) in enumerate(sp):
                mask[b, c, (3 * c + 7 * b + 4 * k) % inner] = w
    held = mask <= torch.tensor(V, dtype=F32)
    flat = lambda t: t.view(-1)
    free_idx, held_idx = (~held).view(-1).nonzero().view(-1), held.view(-1).nonzero().view(-1)
    fence_orig, fence_x1 = torch.zeros(B * C * inner, dtype=torch.bool), torch.zeros(B * C * inner, dtype=torch.bool)
    bad = [float("nan"), float("inf"), float("-inf")]
    for k in range(3):
        i = int(free_idx[(5 * k + 1) % len(free_idx)])
        flat(original)[i] = bad[k]
        fence_orig[i] = True
        j = int(held_idx[(7 * k + 2) % len(held_idx)])
        if k == 2 and eta:
            flat(noise)[j] = float("inf")
        else:
            flat(xt)[j] = bad[k]
        fence_x1[j] = True
    return dict(xt=xt.contiguous(), eps_pair=eps_pair.contiguous(), noise=noise if eta else None,
                coef=COEF if eta else COEF[:4] + (0.0,) + COEF[5:], original=original, mask=mask, qnoise=qnoise, qcoef=QCOEF, v=V,
                held=held, fence_orig=fence_orig.view(B, C, inner), fence_x1=fence_x1.view(B, C, inner))


def step_args(case, guided):
    return (case["xt"], case["eps_pair"], case["noise"], case["coef"], guided, case["original"], case["mask"], case["qnoise"],
            case["qcoef"], case["v"])


# ---- the golden runs of the reference's legacy loop --------------------------------------------------------------------------------
SHAPE = (1, 4, 5, 8, 8)
GUIDANCE = 2.0       # moderate: at 9 the tiny UNet's synthetic weights blow the latent up to std 5-13
SEED = 7             # torch.manual_seed before every run
CASES = {            # name: steps, eta, mask kind
    "frames_eta0": (4, 0.0, "frames"),        # per-frame weights, 0.25 / 0.5 / 0.75 are exactly v_2 / v_1 / v_0 at S = 4
    "frames_eta1": (4, 1.0, "frames"),
    "spatial": (5, 0.0, "spatial"),           # a mask that also varies inside a frame
    "plain": (4, 0.0, None),                  # mask=None through the same legacy loop: the baseline
}
FRAME_WEIGHTS = (0.0, 0.25, 0.5, 0.75, 1.0)


def case_mask(kind):
    """-> fp32 [1, 4, 5, 8, 8] or None"""
    if kind is None:
        return None
    m = np.ones(SHAPE)
    if kind == "frames":
        for i, w in enumerate(FRAME_WEIGHTS):
            m[:, :, i] = w
    else:
        rng = np.random.RandomState(11)
        for i, w in enumerate((0.0, 0.2, 0.4, 0.8, 1.0)):          # left half: per-frame weights, some of them a v_i of S = 5 in fp32
            m[:, :, i, :, :4] = w
            m[:, :, i, :, 4:] = rng.uniform(size=(8, 4))             # right half: every pixel its own release step
    return torch.tensor(m).float()


def case_inputs(name):
    """-> (latents fp32, mask fp32 or None, c, uc): the latents as process_modelscope builds them — one image latent repeated over the
    frames, blended with seeded numpy normal noise by the mask (the plain case: by the per-frame mask) — and fp16-representable contexts
    (the legacy loop casts them to fp16, t2v_model.py:1538-1539)."""
    S, eta, kind = CASES[name]
    g = torch.Generator().manual_seed(5)
    image = (torch.randn(1, 4, 1, 8, 8, generator=g) * 0.8).expand(SHAPE).double().numpy()
    c = torch.randn(1, 7, 1024, generator=g).half().float()
    uc = torch.randn(1, 7, 1024, generator=g).half().float()
    noise = np.random.RandomState(3).normal(size=SHAPE)
    mask = case_mask(kind)
    m = (mask if mask is not None else case_mask("frames")).double().numpy()
    latents = torch.tensor(image * (1 - m) + noise * m).float()
    return latents, mask, c, uc
