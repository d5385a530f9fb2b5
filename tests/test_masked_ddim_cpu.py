"""CPU: masked DDIM sampling of the VideoCrafter path (lvdm/samplers/ddim.py:188-195) — the sampler's host logic against golden
outputs of the REAL reference's masked loop (tests/golden/make_golden_masked.py), with the oracle UNet as `apply_model` and torch
restatements of the three device bindings; `LatentDiffusion.q_sample`; the DDIM_STEP blend record's validation."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import masked_ref as MR
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers, videocrafter as VC
from test_samplers_cpu import _ddim_update_cpu, _lincomb_cpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _ddim_update_blend_cpu(out, xt, eps_pair, noise, coef, guided, known, mask, qnoise, qcoef):
    xn = _ddim_update_cpu(torch.empty(xt.shape), xt, eps_pair, noise, coef, guided, 1)
    assert known.shape == mask.shape == qnoise.shape == xt.shape and mask.is_contiguous()
    out.copy_(MR.blend_cpu(xn, known, mask, qnoise, qcoef))
    return out


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "lvdm_masked_tiny.npz"))


@pytest.fixture(scope="module")
def tiny_sd():
    net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    return synth.synth_state_dict(synth.param_spec(net), seed=0)


@pytest.fixture()
def ld(tiny_sd, monkeypatch):
    """LatentDiffusion's schedule and q_sample around the oracle UNet; the device bindings replaced by their restatements, the blend
    binding counted."""
    blends = []

    def blend(*a):
        blends.append(a[-1])
        return _ddim_update_blend_cpu(*a)
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update", _ddim_update_cpu)
    monkeypatch.setattr(samplers, "_ddim_update_blend", blend)
    m = VC.LatentDiffusion.__new__(VC.LatentDiffusion)
    torch.nn.Module.__init__(m)
    VC.LatentDiffusion.register_schedule(m, **configs.LVDM_SCHEDULE)
    m.apply_model = lambda x, t, c, **kw: tp.lvdm_unet_forward(tiny_sd, configs.TINY_LVDM_UNET, x, t, c)
    m.model = types.SimpleNamespace(diffusion_model=types.SimpleNamespace(refresh_weights=lambda d: None, auto_refresh=True))
    m.blends = blends
    return m


def _run(ld, name):
    c = MR.case(name)
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(MR.NOISE_GEN_SEED)
    torch.manual_seed(MR.GLOBAL_SEED)
    return smp.sample(**MR.conditions(c))


@pytest.mark.parametrize("name", MR.CASES)
def test_masked_loop_matches_reference_golden(ld, gold, name):
    c = MR.case(name)
    assert np.array_equal(c["x0"].numpy(), gold[f"{name}_x0"]) and np.array_equal(c["mask"].numpy(), gold[f"{name}_mask"])
    x, inter = _run(ld, name)
    want = gold[f"{name}_out"]
    assert np.abs(x.numpy() - want).max() < 2e-4 * np.abs(want).max()
    # one blend launch per step, with the q_sample coefficients of t' = step - 1 = 750, 500, 250, 0
    assert gold[f"{name}_t"][:, 0].tolist() == [750, 500, 250, 0]
    want_q = [(float(ld.sqrt_alphas_cumprod[t]), float(ld.sqrt_one_minus_alphas_cumprod[t])) for t in (750, 500, 250, 0)]
    assert ld.blends == want_q
    assert torch.equal(inter["x_inter"][-1], x)                  # x_inter receives the blended img


def test_held_frames_keep_the_t0_noise(ld):
    """Frames 0-1 of (a) end as q_sample(x0, 0) with the LAST q-noise draw: the reference leaves sqrt(1 - ac[0]) ~ 0.029 of noise in."""
    c = MR.case("a")
    x, _ = _run(ld, "a")
    torch.manual_seed(MR.GLOBAL_SEED)
    for _ in range(MR.STEPS):
        n_last = torch.randn(tuple(c["x0"].shape))
    want = ld.sqrt_alphas_cumprod[0] * c["x0"] + ld.sqrt_one_minus_alphas_cumprod[0] * n_last
    assert (x[:, :, 0:2] - want[:, :, 0:2]).abs().max() < 1e-6
    assert (x[:, :, 2:] - want[:, :, 2:]).abs().max() > 0.1       # the free frames are generated


def test_mask_rules(ld):
    c = MR.case("a")
    kw = MR.conditions(c)
    smp = VC.DDIMSampler(ld)
    with pytest.raises(NotImplementedError):                      # a 1-D mask would broadcast along the width
        smp.sample(**{**kw, "mask": torch.ones(1)})
    with pytest.raises(NotImplementedError):
        smp.sample(**{**kw, "mask": torch.ones(5, 8, 8)})
    with pytest.raises(ValueError):                               # mask without x0
        smp.sample(**{**kw, "x0": None})
    with pytest.raises(ValueError):                               # not broadcastable to the latent
        smp.sample(**{**kw, "mask": torch.ones(1, 1, 3, 1, 1)})
    with pytest.raises(ValueError):                               # x0 of another shape
        smp.sample(**{**kw, "x0": c["x0"][:, :, :3]})
    for refused in (dict(quantize_x0=True), dict(noise_dropout=0.1), dict(score_corrector=object()), dict(cond_fn=lambda *a: None)):
        with pytest.raises(NotImplementedError):
            smp.sample(**kw, **refused)
    assert ld.blends == []


def test_unmasked_sample_leaves_the_global_rng_and_the_blend_alone(ld):
    kw = MR.conditions(MR.case("a"))
    del kw["mask"], kw["x0"]
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(MR.NOISE_GEN_SEED)
    torch.manual_seed(MR.GLOBAL_SEED)
    before = torch.get_rng_state()
    x, _ = smp.sample(**kw)
    assert torch.equal(torch.get_rng_state(), before) and ld.blends == []
    gold = np.load(os.path.join(GOLD, "lvdm_tiny.npz"))["ddim_x0"]              # the unmasked golden of the same inputs
    assert np.abs(x.numpy() - gold).max() < 2e-4 * np.abs(gold).max()


def test_q_sample_matches_the_formula(ld):
    g = torch.Generator().manual_seed(3)
    x, n = torch.randn(2, 4, 5, 8, 8, generator=g), torch.randn(2, 4, 5, 8, 8, generator=g)
    t = torch.tensor([750, 3])
    got = ld.q_sample(x, t, noise=n)
    for b in range(2):
        ac = ld.alphas_cumprod[t[b]].double()
        want = ac.sqrt() * x[b].double() + (1 - ac).sqrt() * n[b].double()
        assert (got[b].double() - want).abs().max() < 1e-6
    assert got.dtype == torch.float32 and (got[0] - got[1]).abs().max() > 0.1
    # noise=None: one draw of x's shape from the CPU default generator
    torch.manual_seed(5)
    a = ld.q_sample(x, t)
    torch.manual_seed(5)
    assert torch.equal(a, ld.q_sample(x, t, noise=torch.randn(tuple(x.shape))))


def test_first_stage_encoding_helpers(ld):
    from sd_webui_text2video_amd.vae import DiagonalGaussianDistribution
    ld.scale_factor, ld.shift_factor = 0.5, 0.25
    g = torch.Generator().manual_seed(4)
    z = torch.randn(3, 4, 2, 2, generator=g)
    assert torch.equal(ld.get_first_stage_encoding(z), 0.5 * (z + 0.25))
    post = DiagonalGaussianDistribution(torch.randn(3, 8, 2, 2, generator=g))
    n = torch.randn(3, 4, 2, 2, generator=g)
    assert torch.equal(ld.get_first_stage_encoding(post, noise=n), 0.5 * (post.mean + post.std * n + 0.25))
    with pytest.raises(NotImplementedError):
        ld.get_first_stage_encoding([z])
    with pytest.raises(NotImplementedError, match="the reference fails too"):
        ld.encode_first_stage_2DAE(torch.zeros(1, 3, 2, 8, 8), encode_bs=None)
    with pytest.raises(NotImplementedError, match="the reference fails too"):
        ld.encode_first_stage(torch.zeros(1, 3, 2, 8, 8))


def test_blend_record_validation_without_gpu(built_lib):
    """Validation runs before any HIP call: every malformed blend record is refused with a message naming the DDIM step."""
    h = ctypes.c_void_p()
    ptr = 0x1000

    def create(i7=1, mode=1, x_dt=L.F32, p4=ptr, p5=ptr, p6=ptr, f7=0.5):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_DDIM_STEP
        for k, v in enumerate((8, 64, 4, L.F32, x_dt, mode, 4, i7)):
            op[0].i[k] = v
        op[0].f[6], op[0].f[7] = 0.9, f7
        for k, v in enumerate((ptr, ptr, 0, ptr, p4, p5, p6)):
            op[0].p[k] = v
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    assert create()[0] == 0 and create(p6=0, f7=0.0)[0] == 0
    assert create(i7=0, mode=0, x_dt=L.F16, p4=0, p5=0, p6=0)[0] == 0          # i[7] = 0: none of the blend fields is looked at
    for bad in (dict(i7=2), dict(i7=-1), dict(mode=0), dict(x_dt=L.F16), dict(p4=0), dict(p5=0), dict(p6=0)):
        rc, msg = create(**bad)
        assert rc == -1 and b"DDIM step" in msg, (bad, rc, msg)
