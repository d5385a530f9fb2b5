"""GPU: context windows — the gather and blend kernels (T2V_OP_LINCOMB forms i[9] = 2 and 1) on the designed operands of
tests/context_window_inputs.py, and the windowed samplers end to end on the tiny UNet.

Gather: bit-exact against the restatement.  Blend: per element |out - ref| <= 8 * 2^-24 * (sum_w wgt |e|) / (sum_w wgt) against the
float64 restatement — the fp32 bound of at most 4 fused multiply-adds, one sum of at most 4 weights and one division (the fp16 -> fp32
load is exact) — and bit-identical results however the windows were chunked over forwards.  Every operand sits between NaN fences and
every output starts as NaN.  What the operands expose is shown on the CPU (tests/test_context_windows_cpu.py).

End to end (6 frames, windows of 4 with overlap 2, 4 steps, CFG 9, eta 0): each sampler against the REAL reference run through windows
(tests/golden/context_windows.npz) at the gates tests/test_gpu_e2e.py applies to the same sampler against tiny.npz; DDIM_Gaussian
against a composition of single-window (B = 1) forwards of the same model, a float64 blend and the existing step kernel, at the gate of
test_several_videos_per_batch_match_single_video_runs for batch-dependent GEMM tiling (3e-3)."""
import os

import numpy as np
import pytest
import torch

import context_window_inputs as CW
from harness import rel_l2
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import samplers

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "context_windows.npz")
DEV = "cuda:0"
FRAMES, WINDOWS, STEPS, SCALE = 6, dict(length=4, overlap=2), 4, 9.0


def _tables(overlap, weights=CW.DESIGNED_WEIGHTS):
    starts = CW.starts_ref(CW.F, CW.LENGTH, overlap)
    return starts, torch.tensor(starts, dtype=torch.int32, device=DEV), torch.tensor(weights, dtype=torch.float32, device=DEV)


# ---- 1. gather -----------------------------------------------------------------------------------------------------------------------------
def _check_gather(shape, skew=0):
    starts, starts_d, _ = _tables(shape["overlap"])
    x = CW.latent_operand(shape["hw"], shape["dtype"])
    xbig, xv = CW.fenced(x, DEV, skew)
    rows_all = CW.V * len(starts)
    for row0, rows in CW.chunks_ref(rows_all, shape["batch"]):
        want = CW.gather_ref(x, starts, CW.LENGTH, row0, rows)
        big, xw = CW.fenced(want, DEV, skew, fill=False)
        assert bool(torch.isnan(xw).all())
        samplers._window_gather(xw, xv, starts_d, row0)
        torch.cuda.synchronize()
        got = xw.cpu()
        assert not bool(torch.isnan(got).any()) and torch.equal(got, want), (row0, rows)
        assert CW.fence_intact(big, want.numel(), skew) and CW.fence_intact(xbig, x.numel(), skew)
    assert torch.equal(xv.cpu(), x)


@pytest.mark.parametrize("shape", CW.GATHER_SHAPES, ids=CW.shape_id)
def test_gather_is_bit_exact(shape):
    _check_gather(shape)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_gather_from_a_base_off_the_16_byte_grid(dtype):
    """HW = 16 allows the 16-byte path, the bases do not: the scalar path on a vector-sized frame."""
    _check_gather(dict(overlap=2, hw=(4, 4), dtype=dtype, batch=3), skew=1)


# ---- 2. blend ------------------------------------------------------------------------------------------------------------------------------
def _check_blend(shape, weights=CW.DESIGNED_WEIGHTS, skew=0):
    starts, starts_d, weights_d = _tables(shape["overlap"], weights)
    nW, roles = len(starts), 2 if shape["guided"] else 1
    e = CW.eps_operand(roles, nW, shape["hw"], shape["dtype"])
    ref, bound = CW.blend_ref(e, starts, weights, CW.V, CW.F)
    ref, bound = ref.reshape(roles * CW.V, *ref.shape[2:]), bound.reshape(roles * CW.V, *bound.shape[2:])
    outs, worst = [], 0.0
    for batch in CW.BATCHES:
        chunks = [CW.fenced(ch, DEV, skew) for ch in CW.split_chunks(e, batch)]
        big, out = CW.fenced(ref.float(), DEV, skew, fill=False)
        samplers._window_blend(out, [v for _, v in chunks], starts_d, weights_d, roles)
        torch.cuda.synchronize()
        got = out.cpu()
        assert not bool(torch.isnan(got).any())
        err = (got.double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (batch, float((err / bound.clamp_min(1e-300)).max()))
        assert CW.fence_intact(big, ref.numel(), skew)
        for (cbig, cv), ch in zip(chunks, CW.split_chunks(e, batch)):
            assert CW.fence_intact(cbig, ch.numel(), skew) and torch.equal(cv.cpu(), ch)
        outs.append(got)
    print(f"{CW.shape_id(shape)}: largest error {worst:.3f} of the bound")
    assert all(torch.equal(o, outs[0]) for o in outs[1:])          # the chunking does not reach the value
    return outs[0]


@pytest.mark.parametrize("shape", CW.BLEND_SHAPES, ids=CW.shape_id)
def test_blend_against_the_float64_restatement(shape):
    _check_blend(shape)


@pytest.mark.parametrize("kind", ["pyramid", "flat"])
def test_blend_with_the_schedule_weights(kind):
    for overlap in CW.OVERLAPS:
        _check_blend(dict(overlap=overlap, hw=(4, 4), dtype=torch.float32, guided=True), weights=tuple(CW.weights_ref(CW.LENGTH, kind)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_blend_from_a_base_off_the_16_byte_grid(dtype):
    shape = dict(overlap=2, hw=(4, 4), dtype=dtype, guided=True)
    assert torch.equal(_check_blend(shape, skew=1), _check_blend(shape))          # the scalar path gives the vector path's bits


# ---- 3. end to end on the tiny UNet --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from sd_webui_text2video_amd import unet as U
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, betas


def _cond():
    g = torch.Generator().manual_seed(5)
    torch.randn(2, 4, 3, 16, 16, generator=g); torch.randn(2, 7, 1024, generator=g); torch.randn(2, 4, 8, 8, generator=g)
    return torch.randn(1, 7, 1024, generator=g).to(DEV), torch.randn(1, 7, 1024, generator=g).to(DEV)


def _noise(seeds, frames=FRAMES):
    out = []
    for seed in seeds:
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        out.append(torch.randn((1, 4, frames, 16, 16), generator=g))
    return torch.cat(out).to(DEV)


def _sample(net, betas, name, noise, **kw):
    c, uc = _cond()
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name=name)
    smp.progress = False
    return smp.sample_loop(steps=STEPS, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=noise.shape[0],
                           shape=tuple(noise.shape), noise=noise, guidance_scale=SCALE, eta=0.0, sampler_name=name, **kw).float().cpu()


GATES = {"DDIM_Gaussian": 2e-2, "DDIM": 3e-2, "UniPC": 3e-2}          # tests/test_gpu_e2e.py, the same samplers against tiny.npz


@pytest.mark.parametrize("seeds", [(1234,), (1234, 1235)], ids=["V1", "V2"])
@pytest.mark.parametrize("name", list(GATES))
def test_windowed_samplers_match_the_reference_through_windows(tiny, name, seeds):
    net, betas = tiny
    gold = np.load(GOLD)
    x0 = _sample(net, betas, name, _noise(seeds), context_windows=WINDOWS)
    assert tuple(x0.shape) == (len(seeds), 4, FRAMES, 16, 16)
    for v, seed in enumerate(seeds):
        r = rel_l2(x0[v:v + 1], torch.from_numpy(gold[f"{name}_x0_{seed}"]))
        print(f"{name}, video {v} of {len(seeds)} (seed {seed}): rel-L2 {r:.3e} against the reference through windows (gate {GATES[name]:.0e})")
        assert r < GATES[name], (name, seed, r)
    if len(seeds) == 1:                # chunked forwards: the same run to rounding (the GEMM tiling differs with the batch)
        x1 = _sample(net, betas, name, _noise(seeds), context_windows=dict(WINDOWS, batch=1))
        r = rel_l2(x1, torch.from_numpy(gold[f"{name}_x0_{seeds[0]}"]))
        print(f"{name}, forwards of one window: rel-L2 {r:.3e}")
        assert r < GATES[name], (name, r)


class _Composed:
    """model(x, t, c): every window of every video through its own B = 1 forward of the net, blended per frame in float64 — the
    composition the windowed run must equal, with no code of the feature in it."""

    def __init__(self, net):
        self.net, self.device = net, torch.device(DEV)

    def __call__(self, x, t, c):
        length, starts = WINDOWS["length"], CW.starts_ref(x.shape[2], WINDOWS["length"], WINDOWS["overlap"])
        wg = CW.weights_ref(length, "pyramid")
        acc = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
        wsum = torch.zeros(x.shape[2], dtype=torch.float64, device=x.device)
        for s in starts:
            for v in range(x.shape[0]):
                cv = c if c.shape[0] == 1 else c[v:v + 1]
                eps = self.net(x[v:v + 1, :, s:s + length].contiguous(), t[:1], cv).double()
                for j in range(length):
                    acc[v, :, s + j] += wg[j] * eps[0, :, j]
            for j in range(length):
                wsum[s + j] += wg[j]
        return (acc / wsum.view(1, 1, -1, 1, 1)).float()


@pytest.mark.parametrize("extra", [{}, dict(percentile=0.995)], ids=["plain", "percentile"])
def test_ddim_gaussian_equals_its_composition_from_single_window_forwards(tiny, extra):
    net, betas = tiny
    c, uc = _cond()
    noise = _noise((1234, 1235) if not extra else (1234,))
    kw = dict(S=STEPS, conditioning=c, unconditional_conditioning=uc, shape=tuple(noise.shape), unconditional_guidance_scale=SCALE, eta=0.0, **extra)
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM_Gaussian")
    got = smp.sampler.sample(x_T=noise, context_windows=WINDOWS, **kw).float().cpu()
    ref = samplers.GaussianDiffusion(_Composed(net), betas).sample(x_T=noise, **kw).float().cpu()
    for v in range(noise.shape[0]):
        r = rel_l2(got[v:v + 1], ref[v:v + 1])
        print(f"DDIM_Gaussian {extra or 'plain'}, video {v}: rel-L2 {r:.3e} against the composition (gate 3e-3)")
        assert r < 3e-3, (v, r)
    plain = smp.sampler.sample(x_T=noise, **kw).float().cpu()
    assert rel_l2(got, plain) > 1e-2               # windows of 4 out of 6 frames are not the full-clip run


# ---- 4. inert on the device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GATES))
def test_a_clip_no_longer_than_a_window_is_the_run_without_the_keyword(tiny, name):
    net, betas = tiny
    noise = _noise((1234,), frames=4)
    base = _sample(net, betas, name, noise)
    for win in (WINDOWS, dict(length=5, overlap=1, weights="flat", batch=1)):
        assert torch.equal(_sample(net, betas, name, noise, context_windows=win), base)
