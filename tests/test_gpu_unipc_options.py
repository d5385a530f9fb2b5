"""GPU (-m gpu): T2V_OP_DDIM_STEP mode 2, the thresholded data prediction of UniPC, against the torch restatement of its documented
semantics (tests/unipc_ref.py) bit for bit; the UniPC sampler's options against golden runs of the REAL reference's UniPC class
(tests/golden/make_golden_unipc.py); several videos per batch in the "UniPC" and "DDIM" samplers.  Measured figures:
profiles/unipc_options.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

import unipc_ref as UR
import x0_threshold_ref as XR
from harness import rel_l2
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers as S, unet as U
from test_samplers_cpu import _ddim_update_cpu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "unipc_options_tiny.npz")
DEV = "cuda:0"

# whole-output rel-L2 of each golden case on the tiny UNet (3 frames @ 128x128) against the reference's latent: measured on the MI355X
# (profiles/unipc_options.txt) + 10 %, the project's convention for few-step parity; none above the 3e-2 tests/test_gpu_e2e.py allows
# the tiny UniPC run
LOOP_GATES = {                                   # measured
    "bh2": 2.76e-3,                              # 2.517e-3
    "time_quadratic": 2.75e-3,                   # 2.506e-3
    "logSNR": 2.69e-3,                           # 2.453e-3
    "order2": 2.86e-3,                           # 2.604e-3
    "order1": 2.80e-3,                           # 2.548e-3
    "order2_bh2_2steps": 2.88e-3,                # 2.620e-3
    "no_lower_order_final": 4.15e-3,             # 3.775e-3  (order 3 up to the last step: the history differences weigh more)
    "no_initial_corrector": 2.80e-3,             # 2.549e-3
    "denoise_to_zero": 2.80e-3,                  # 2.549e-3
    "thresholding": 4.94e-3,                     # 4.492e-3  (q of every evaluation within 1.21e-3 of the golden's)
    "thresholding_bh2_s07_dtz": 6.16e-3,         # 5.602e-3  (q within 1.39e-3)
    "thresholding_unguided": 7.67e-4,            # 6.980e-4  (guidance 1: no amplification of the UNet's fp16 rounding; q within 4.08e-4)
}
LOOP_CAP = 3e-2


def _record(out, x, eps, sigma, alpha, g, guided, *, i8, table=None, f6=0.0, mode=2, inner=None):
    op = L.T2VOp()
    op.kind = L.OP_DDIM_STEP
    B, C = x.shape[0], x.shape[1]
    op.i[0], op.i[1], op.i[2], op.i[6] = B * C, (x.numel() // (B * C)) if inner is None else inner, guided, C
    op.i[3], op.i[4], op.i[5], op.i[8] = S._dt_tag(eps), S._dt_tag(x), mode, i8
    op.f[0], op.f[1], op.f[5], op.f[6] = float(sigma), float(alpha), float(g), f6
    op.p[0], op.p[1] = x.data_ptr(), eps.data_ptr()
    op.p[3] = out.data_ptr() if out is not None else 0
    op.p[7] = table.data_ptr() if table is not None else 0
    return op


def _launch(*ops):
    arr = (L.T2VOp * len(ops))(*ops)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    return L.load().t2v_run_ops(arr, len(ops), None, 0, ctypes.c_void_p(stream))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit-equal, a NaN matching any NaN (the payload of a propagated NaN is not part of the contract)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


Q = float(np.float32(UR.QUANTILE))


def _both_passes(x, eps, sigma, alpha, g, guided):
    """measure + apply in ONE t2v_run_ops call, as the sampler sends them -> (out, table) on the host; the output and the table start
    from sentinels."""
    xd, ed = x.to(DEV), eps.to(DEV)
    out = torch.full(x.shape, 123.0, device=DEV)
    table = torch.full((x.shape[0], 4), -7.0, device=DEV)
    C = x.shape[1]
    rc = _launch(_record(None, xd, ed, sigma, alpha, g, C if guided else 0, i8=3, table=table, f6=Q),
                 _record(out, xd, ed, sigma, alpha, g, C if guided else 0, i8=2, table=table))
    assert rc == 0, L.load().t2v_last_error()
    torch.cuda.synchronize()
    return out.cpu(), table.cpu()


@pytest.mark.parametrize("videos", [1, 3])
@pytest.mark.parametrize("shape", UR.SHAPES, ids=["n256", "n3072", "n11520"])
def test_mode2_equals_the_restatement_bit_for_bit(shape, videos):
    """Per video 256 (fewer keys than threads), 3072, 11520 (two 8192-key trips, the second partial); 1 and 3 videos; guided and not;
    eps fp16 and fp32.  The measure pass {s, q, v_lo, v_hi} and the apply pass, given the same fp32 sigma, alpha, g, equal
    tests/unipc_ref.py bit for bit."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(n + videos)
    sigma, alpha, gs = float(np.float32(0.7431)), float(np.float32(0.6692)), 7.5
    for eps_dt in (torch.float16, torch.float32):
        for guided in (True, False):
            x = torch.randn((videos,) + shape, generator=g) * 2
            if videos == 3:
                x[1] *= 0.05                                             # this video's q lies below 1: s = 1
            eps = torch.randn(((2 if guided else 1) * videos,) + shape, generator=g).to(eps_dt)
            if videos == 3:
                eps[1] *= 0.05
                if guided:
                    eps[videos + 1] = eps[1] + (eps[videos + 1] * 0.001).to(eps_dt)
            want, tab = UR.predict(x, eps, sigma, alpha, gs, guided)
            out, table = _both_passes(x, eps, sigma, alpha, gs, guided)
            tag = (shape, videos, eps_dt, guided)
            assert _same(table, tab), (tag, table, tab)
            assert _same(out, want), tag
            assert (tab[:, 0] >= 1).all() and (tab[0, 1] > 1) and (videos == 1 or (tab[1, 1] < 1 and tab[1, 0] == 1)), (tag, tab)
    # designed x0: eps = 0 and alpha = 1, so x0 = (x - sigma * 0) / 1 is x bit for bit (what each design catches: unipc_ref.design)
    for name in UR.DESIGNS:
        x = torch.stack([UR.design(name, n, g) for _ in range(videos)]).view((videos,) + shape)
        for guided in (True, False):
            eps = torch.zeros(((2 if guided else 1) * videos,) + shape)
            want, tab = UR.predict(x, eps, 0.5, 1.0, gs, guided)
            assert torch.equal(_bits(UR.x0_of(x, eps, 0.5, 1.0, gs, guided)), _bits(x))
            out, table = _both_passes(x, eps, 0.5, 1.0, gs, guided)
            assert _same(table, tab), (shape, videos, name, guided, table, tab)
            assert _same(out, want), (shape, videos, name, guided)
        if name == "signed_zeros":
            assert tab[0].tolist() == [1.0, 0.0, 0.0, 0.0] and torch.equal(_bits(out), _bits(x))          # +-0 / 1: the sign is kept
        if name == "below_one":
            assert tab[0, 0] == 1.0 and 0 < tab[0, 1] < 1 and torch.equal(out, x)
        if name in ("ties_straddle", "all_equal"):
            assert tab[0, 2] == tab[0, 3] == tab[0, 1]
        if name == "hi_past_ties":
            assert tab[0, 2] == 1.5 and tab[0, 3] >= 3.0
        if name == "infs":
            assert torch.isfinite(tab).all() and torch.isinf(x).any() and out.abs().max() == 1.0       # clamp(+-inf, -s, s) / s = +-1


def test_a_nan_poisons_its_own_video_only():
    shape = (3, 4, 3, 16, 16)
    g = torch.Generator().manual_seed(53)
    x = torch.randn(shape, generator=g) * 3
    x[1, 2, 1, 5, 7] = float("nan")
    eps = torch.randn((6,) + shape[1:], generator=g)
    want, tab = UR.predict(x, eps, 0.7431, 0.6692, 7.5, True)
    out, table = _both_passes(x, eps, 0.7431, 0.6692, 7.5, True)
    assert torch.isnan(table[1, 0]) and torch.isnan(table[1, 1]) and torch.isnan(out[1]).all() and torch.isnan(want[1]).all()
    for v in (0, 2):
        assert _same(table[v], tab[v]) and _same(out[v], want[v]) and not torch.isnan(out[v]).any(), v
    # ... the same through the eps pair
    x[1, 2, 1, 5, 7] = 0.25
    eps[3 + 2, 0, 0, 0, 0] = float("nan")                                # the unconditional prediction of video 2
    want, tab = UR.predict(x, eps, 0.7431, 0.6692, 7.5, True)
    out, table = _both_passes(x, eps, 0.7431, 0.6692, 7.5, True)
    assert torch.isnan(table[2, 0:2]).all() and torch.isnan(out[2]).all() and _same(out[:2], want[:2]) and _same(table[:2], tab[:2])


def test_mode0_and_mode1_records_give_what_they_gave():
    """The same pointers through the plain records: mode 1 = `_ddim_update`'s documented formula (tests/test_samplers_cpu.py), mode 0 the
    DDIM_Gaussian step (tests/x0_threshold_ref.py, no restriction)."""
    shape = (2, 4, 3, 16, 16)
    g = torch.Generator().manual_seed(59)
    x, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    eps = torch.randn((4,) + shape[1:], generator=g)
    for eps_dt in (torch.float16, torch.float32):
        e = eps.to(eps_dt)
        for sigma in (0.0, 0.25):
            coef = [0.7431, 0.6692, 0.9, 0.3, sigma, 7.5]
            out = S._ddim_update(torch.empty(shape, device=DEV), x.to(DEV), e.to(DEV), noise.to(DEV), coef, 4, mode=1)
            want = _ddim_update_cpu(torch.empty(shape), x, e, noise, coef, 4, 1)
            assert rel_l2(out.cpu(), want) < 1e-6, (eps_dt, sigma, "mode 1")
            coef0 = [1.7130, 1.3908, 0.9, 0.3, sigma, 7.5]
            out = S._ddim_update(torch.empty(shape, device=DEV), x.to(DEV), e.to(DEV), noise.to(DEV), coef0, 2, mode=0)
            want, _ = XR.step(x, e, noise, coef0, 2, kind=0)
            assert rel_l2(out.cpu(), want) < 1e-6, (eps_dt, sigma, "mode 0")


def test_refused_records_launch_nothing():
    shape = (1, 4, 3, 16, 16)
    g = torch.Generator().manual_seed(61)
    x = torch.randn(shape, generator=g).to(DEV)
    eps = torch.randn((2,) + shape[1:], generator=g).to(DEV)
    out = torch.full(shape, 123.0, device=DEV)
    table = torch.full((1, 4), 123.0, device=DEV)
    lib = L.load()
    ok = dict(table=table, f6=Q)

    def refused(needle, *ops):
        return _launch(*ops) == -1 and b"DDIM step" in lib.t2v_last_error() and needle in lib.t2v_last_error()      # -1 = T2V_ERR_BAD_ARG

    assert refused(b"mode 2", _record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=1, **ok))                   # the clamp
    assert refused(b"mode 2", _record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=0, **ok))
    x16, out16 = x.half(), torch.full(shape, 123.0, device=DEV, dtype=torch.float16)
    for i8 in (2, 3):
        assert refused(b"fp32 x", _record(out16, x16, eps, 0.5, 0.8, 9.0, 4, i8=i8, **ok)), i8     # an fp16 x
        assert refused(b"16 777 216", _record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=i8, inner=4194305, **ok)), i8     # n > 2^24 (never launched)
        assert refused(b"p[7]", _record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=i8, f6=Q)), i8
    assert refused(b"all channels", _record(out, x, eps, 0.5, 0.8, 9.0, 2, i8=2, **ok))
    # a refused second record keeps the first from launching too
    assert refused(b"mode 2", _record(None, x, eps, 0.5, 0.8, 9.0, 4, i8=3, **ok), _record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=1, **ok))
    torch.cuda.synchronize()
    assert (out == 123.0).all() and (out16 == 123.0).all() and (table == 123.0).all()
    # the measure pass writes the table and nothing else
    assert _launch(_record(out, x, eps, 0.5, 0.8, 9.0, 4, i8=3, **ok)) == 0
    torch.cuda.synchronize()
    assert (out == 123.0).all() and not (table == 123.0).any()


# ---- the sampler against the reference's golden runs -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, betas


def _sample(model, betas, gold, name):
    steps, guidance, strength, kw = UR.CASES[name]
    smp = S.Txt2VideoSampler(model, torch.device(DEV), betas=betas, sampler_name="UniPC")
    smp.progress = False
    c, uc, noise = (torch.from_numpy(gold[k]).to(DEV) for k in ("c", "uc", "noise"))
    S.state.sampling_step = 0
    x = smp.sample_loop(steps=steps, strength=strength, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=None,
                        shape=tuple(noise.shape), noise=noise, guidance_scale=guidance, eta=0.0, sampler_name="UniPC", unipc=kw)
    th = smp.sampler.last_thresholds
    return x.float().cpu(), None if th is None else th.cpu()


@pytest.mark.parametrize("name", list(UR.CASES))
def test_option_loops_match_the_reference_golden(tiny, gold, name):
    net, betas = tiny
    x, th = _sample(net, betas, gold, name)
    r = rel_l2(x, torch.from_numpy(gold[f"{name}_out"]))
    print(f"UniPC {name}: rel-L2 vs the reference golden = {r:.3e}")
    if name in UR.THRESHOLDED:
        assert tuple(th.shape) == (UR.evaluations(name), 1, 4)
        q_gold = torch.from_numpy(gold[f"{name}_q"])
        print(f"UniPC {name}: q = {th[:, 0, 1].tolist()}, golden {q_gold.tolist()}, max relative error {float(((th[:, 0, 1] - q_gold).abs() / q_gold).max()):.3e}")
    else:
        assert th is None
    assert LOOP_GATES[name] <= LOOP_CAP and r < LOOP_GATES[name], r


class _ReplayOnDevice:
    """The reference UNet's recorded answers, handed back on the device: one [cond | uncond] call per evaluation (one row at guidance 1)."""
    supports_cfg_batch = True
    num_timesteps = 1000

    def __init__(self, eps):
        self.eps, self.calls = torch.from_numpy(eps).to(DEV), 0

    def __call__(self, x, t, cond):
        assert x.shape[0] == self.eps.shape[1]
        self.calls += 1
        return self.eps[self.calls - 1].clone()


@pytest.mark.parametrize("name", UR.REPLAYED)
def test_replayed_runs_reproduce_the_reference_thresholds(gold, name):
    """With the reference UNet's answers replayed, what is left is the solver: the latent and `last_thresholds` (q and s of every
    evaluation) equal the golden's to 2e-5, the gate of the host-side loop (tests/test_unipc_options_cpu.py)."""
    model = _ReplayOnDevice(gold[f"{name}_eps"])
    x, th = _sample(model, tp.beta_schedule_linear_sd(), gold, name)
    assert model.calls == UR.evaluations(name)
    g = gold[f"{name}_out"]
    r = float(np.abs(x.numpy() - g).max() / np.abs(g).max())
    print(f"UniPC {name}, replayed: max-abs error / max-abs vs the reference golden = {r:.3e}")
    if name in UR.THRESHOLDED:
        for col, key in ((1, "q"), (0, "s")):
            want = torch.from_numpy(gold[f"{name}_{key}"])
            e = float(((th[:, 0, col] - want).abs() / want).max())
            print(f"    {key} = {th[:, 0, col].tolist()}: max relative error {e:.3e}")
            assert e < 2e-5, (key, e)
    assert r < 2e-5, r


# ---- several videos per batch ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(tiny):
    from sd_webui_text2video_amd import pipeline
    net, betas = tiny
    p = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=None, betas=betas, device=DEV)
    p.diffusion.progress = False
    return p


@pytest.mark.parametrize("sampler,steps,extra", [
    ("UniPC", 6, {}),
    ("UniPC", 6, dict(unipc=dict(thresholding=True))),
    ("DDIM", 4, {}),
    ("DDIM", 4, dict(vid2vid=True)),
], ids=["unipc", "unipc-thresholding", "ddim", "ddim-vid2vid"])
def test_two_videos_per_batch_match_their_single_runs(pipe, gold, sampler, steps, extra):
    """`infer_conditioned(videos=2)`: video v equals the single run of seed + v within 3e-3 rel-L2, the gate of
    test_gpu_e2e.py::test_several_videos_per_batch_match_single_video_runs (the UNet's GEMM tiling differs with the batch); the
    thresholds to the same gate; the two videos differ."""
    c, uc = torch.from_numpy(gold["c"]), torch.from_numpy(gold["uc"])
    extra = dict(extra)
    kw = {}
    if extra.pop("vid2vid", False):
        z0 = torch.randn((1, 4, 3, 16, 16), generator=torch.Generator().manual_seed(11))
        kw = dict(latents=z0, strength=0.75, is_vid2vid=True)
    kw.update(extra)
    thresholded = "unipc" in kw
    _, xb = pipe.infer_conditioned(c, uc, steps, 3, 77, 9.0, 128, 128, 0.0, decode=False, sampler=sampler, videos=2, **kw)
    thb = pipe.diffusion.sampler.last_thresholds.cpu() if thresholded else None
    assert tuple(xb.shape) == (2, 4, 3, 16, 16)
    for v in range(2):
        _, x1 = pipe.infer_conditioned(c, uc, steps, 3, 77 + v, 9.0, 128, 128, 0.0, decode=False, sampler=sampler, **kw)
        r = rel_l2(xb[v:v + 1].float().cpu(), x1.float().cpu())
        print(f"{sampler} {kw.keys()}: video {v} of a batch of 2 vs its single run: rel-L2 {r:.3e}")
        assert r < 3e-3, (v, r)
        if thresholded:
            th1 = pipe.diffusion.sampler.last_thresholds.cpu()
            rs = float(((thb[:, v, 0] - th1[:, 0, 0]).abs() / th1[:, 0, 0]).max())
            print(f"    thresholds {thb[:, v, 0].tolist()} vs {th1[:, 0, 0].tolist()} ({rs:.3e})")
            assert tuple(thb.shape) == (steps, 2, 4) and rs < 3e-3, (v, rs)
    assert rel_l2(xb[0:1].float().cpu(), xb[1:2].float().cpu()) > 0.1
    if thresholded:
        assert not torch.equal(thb[:, 0, 0], thb[:, 1, 0])
