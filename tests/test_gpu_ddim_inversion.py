"""GPU (-m gpu): DDIM inversion — T2V_OP_DDIM_STEP mode 3 against its float64 restatement (tests/inversion_ref.py), `DDIMSampler.encode`
and the vid2vid route through it against golden outputs of the REAL reference (tests/golden/make_golden_inversion.py).

Op level: rel-L2 against float64 within max(1e-6, 4 e32), e32 = the error of the fp32 torch restatement of the reference's statements on
the same inputs (the gate of the adversarial elementwise suite).  Inputs as there: magnitudes that differ from one (sample, channel)
segment to the next, every tensor a window of a NaN-filled allocation, outputs pre-filled with NaN; the unguided cases carry NaN in the
unconditional half of the eps pair, which must not be read.  Measured values: profiles/ddim_inversion.txt."""
import numpy as np
import pytest
import torch

import elementwise_inputs as EI
import inversion_ref as IR
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L, samplers, unet as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = EI.PAD_FLAT            # 64 elements: a window that starts there keeps the allocation's 16-byte alignment, one element further it does not


def _coef():
    """Step 1 of a 4-step schedule, as `encode` computes it (float64 tables, fp32 values)."""
    ac = torch.cumprod(1 - tp.beta_schedule_linear_sd(), 0)
    a_next, a = ac[251], ac[1]
    return float((a_next / a).sqrt().float()), float((a_next.sqrt() * ((1 / a_next - 1).sqrt() - (1 / a - 1).sqrt())).float())


def _window(n, dtype, offset, value=None):
    """-> (big, view): `n` elements inside a NaN-filled device allocation, `offset` elements behind the aligned start."""
    big = torch.full((n + 2 * PAD + 1,), EI.NAN, dtype=dtype, device=DEV)
    view = big[PAD + offset: PAD + offset + n]
    if value is not None:
        view.copy_(value.reshape(-1).to(dtype))
    return big, view


def _fence_untouched(big, n, offset):
    return bool(torch.isnan(big[:PAD + offset]).all() and torch.isnan(big[PAD + offset + n:]).all())


def _op_case(S, C, inner, edt, guided, gscale, keep, offset=0, wrap_units=None):
    n = S * C * inner
    g = EI._gen(1000 * S + 10 * C + inner % 997 + (1 if guided else 0))
    s_i, c_i = torch.arange(S).view(S, 1, 1), torch.arange(C).view(1, C, 1)
    scale = EI.seg_scale(c_i, s_i)
    X, Y, Un = (scale * EI.body((S, C, inner), g) for _ in range(3))
    if wrap_units is not None:               # what only the second pass of the grid-stride loop reads is 16 x larger and negative
        m = EI.second_pass((n + wrap_units - 1) // wrap_units, wrap_units)[:n].view(S, C, inner)
        assert m.any() and not m.all()
        X, Y, Un = EI.mark_wrap(X, m), EI.mark_wrap(Y, m), EI.mark_wrap(Un, m)
    te = EI.TD[edt]
    X, Y, Un = X.float(), Y.to(te), Un.to(te)
    pair = torch.cat([Y, Un if guided else torch.full_like(Un, EI.NAN)])          # [cond (S) | uncond (S)]
    cx, ce = _coef()
    ref64 = IR.invert_step(X, pair, cx, ce, gscale, guided, torch.float64)
    e32 = IR.rel_l2(IR.invert_step(X, pair.float(), cx, ce, gscale, guided, torch.float32), ref64)
    _, xv = _window(n, torch.float32, offset, X)
    _, ev = _window(2 * n, te, offset, pair)
    ob, ov = _window(n, torch.float32, offset)
    kb, kv = _window(n, torch.float32, offset) if keep else (None, None)
    shape = (S, C, inner)
    samplers._ddim_invert(ov.view(shape), xv.view(shape), ev.view((2 * S, C, inner)), (cx, ce, gscale), guided,
                          keep=kv.view(shape) if keep else None)
    torch.cuda.synchronize()
    L.async_status()
    got = ov.cpu().view(shape)
    err = IR.rel_l2(got, ref64)
    bound = max(1e-6, 4 * e32)
    print(f"mode 3 S{S} C{C} in{inner} eps={edt} guided={int(guided)} g={gscale:g} keep={int(keep)} offset={offset}"
          f"{' grid-stride' if wrap_units else ''}: out.relL2 {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
    assert torch.isfinite(got).all()                                  # every element written; the NaN half of the pair was not read
    assert _fence_untouched(ob, n, offset)
    if keep:
        assert _fence_untouched(kb, n, offset)
        assert torch.equal(kv.view(torch.int32), ov.view(torch.int32))      # both destinations: the same bits
    assert err <= bound, (err, bound)
    # the first pass by itself: the second pass's elements are 16 x larger and dominate the norm above
    if wrap_units is not None:
        assert IR.rel_l2(got[~m], ref64[~m]) <= bound


SHAPES = [(1, 4, 105), (3, 4, 99), (2, 3, 35)]          # C = 3: the element count is no multiple of 4 (the tail; guided: the scalar path)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("guided,gscale", [(True, 9.0), (True, 1.0), (False, 1.0)])
@pytest.mark.parametrize("edt", ["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_mode3_matches_float64(shape, edt, guided, gscale, keep):
    _op_case(*shape, edt, guided, gscale, keep)


@pytest.mark.parametrize("guided,gscale", [(True, 9.0), (False, 1.0)])
@pytest.mark.parametrize("edt", ["f16", "f32"])
def test_mode3_unaligned_views_take_the_scalar_path(edt, guided, gscale):
    _op_case(1, 4, 105, edt, guided, gscale, True, offset=1)


@pytest.mark.parametrize("name,shape,edt,guided,offset,units", [
    # more than one pass of 8192 x 256 threads x 4 elements, plus a ragged tail of 3 (vector path; unguided: no aligned second half exists)
    ("vector-tail", (1, 1, 8388608 + 4 * 1031 + 3), "f32", False, 0, 4),
    # the same with guidance and the kept copy: fp16 eps, an element count that keeps the unconditional half 16-byte aligned
    ("vector-guided", (1, 1, 8388608 + 4 * 1032), "f16", True, 0, 4),
    # the scalar path's own second pass
    ("scalar", (1, 1, 2097152 + 259), "f32", True, 1, 1)])
def test_mode3_grid_stride(name, shape, edt, guided, offset, units):
    _op_case(*shape, edt, guided, 9.0 if guided else 1.0, guided, offset=offset, wrap_units=units)


# ---- the sampler on the tiny UNet ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    sd = synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, sd, betas


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(IR.GOLD))


UNGUIDED_GATE, GUIDED_GATE = 2.6e-3, 8.1e-3      # rel-L2 against the reference golden, see the test below


def _sampler(net, betas):
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM")
    smp.progress = False
    return smp


def _loop_kw(noise, c, uc, z0, **more):
    return dict(steps=4, strength=0.75, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=z0, shape=tuple(noise.shape),
                noise=noise, is_vid2vid=True, guidance_scale=9.0, eta=0.0, sampler_name="DDIM", **more)


def test_encode_and_the_inverted_vid2vid_match_reference_golden(tiny, gold):
    """Against the reference's own class on the CPU in fp32.  The rel-L2 3e-2 of the tiny DDIM test (tests/test_gpu_e2e.py: the synthetic
    weights make guided trajectories expansive, which amplifies the fp16-operand error of every UNet call) proved uselessly loose
    here — inversion walks towards noise, where the latent grows and the UNet's error does not: measured 5.2e-5 .. 1.7e-3 for the
    unguided runs, 5.1e-3 (enc_guided) and 5.4e-3 (the three guided decode steps behind the inversion).  The gates are the measured
    maxima x 1.5, that file's margin: 2.6e-3 unguided, 8.1e-3 with guidance (profiles/ddim_inversion.txt)."""
    net, _, betas = tiny
    z0, noise, c, uc = (t.to(DEV) for t in IR.inputs())
    s = _sampler(net, betas).sampler
    s.make_schedule(4)
    r = {}
    x, info = s.encode(z0, c, 3)
    assert x.dtype == torch.float32 and x.device == z0.device and info["intermediate_steps"] == []
    r["enc_plain"] = IR.rel_l2(x, gold["enc_plain"])
    r["enc_guided"] = IR.rel_l2(s.encode(z0, c, 3, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)[0], gold["enc_guided"])
    r["enc_orig"] = IR.rel_l2(s.encode(z0, c, 5, use_original_steps=True)[0], gold["enc_orig"])
    s.make_schedule(6)
    x, info = s.encode(z0, c, 5, return_intermediates=2)
    assert info["intermediate_steps"] == [0, 2, 3, 4] and len(info["intermediates"]) == 4
    r["enc_inter"] = IR.rel_l2(x, gold["enc_inter"])
    for k, t in enumerate(info["intermediates"]):
        r[f"enc_inter[{k}]"] = IR.rel_l2(t, gold["enc_inter_intermediates"][k])
    assert torch.equal(info["intermediates"][-1], x) and info["intermediates"][-1].data_ptr() != x.data_ptr()
    x0 = _sampler(net, betas).sample_loop(**_loop_kw(noise, c, uc, z0, inversion=True))
    r["vid2vid_inverted_x0"] = IR.rel_l2(x0, gold["vid2vid_inverted_x0"])
    print("DDIM inversion on the tiny UNet, rel-L2 vs the reference golden: " + " ".join(f"{k} {v:.3e}" for k, v in r.items()))
    assert torch.equal(z0.cpu(), IR.inputs()[0])
    guided = ("enc_guided", "vid2vid_inverted_x0")
    assert max(v for k, v in r.items() if k not in guided) < UNGUIDED_GATE and max(r[k] for k in guided) < GUIDED_GATE, r


@pytest.mark.parametrize("k", range(len(IR.ROUNDTRIPS)))
def test_constant_eps_round_trip_on_the_device(gold, k):
    """decode(encode(x0, n), n) with an eps that depends on nothing is the identity up to fp32 arithmetic: within 4 x the error of the
    reference's own arithmetic on it (roundtrip_ref_rel), floor 1e-6."""
    S, n = IR.ROUNDTRIPS[k]
    z0, _, c, _ = (t.to(DEV) for t in IR.inputs())
    model = IR.ConstEpsModel(IR.const_eps(), DEV)
    s = _sampler(model, tp.beta_schedule_linear_sd()).sampler
    s.make_schedule(S)
    enc, _ = s.encode(z0, c, n, model_timesteps="schedule")
    back = s.decode(enc, c, n)
    assert [cl[1][0] for cl in model.calls[:n]] == [float(t) for t in s.ddim_timesteps[:n]]
    assert [cl[1][0] for cl in model.calls[n:]] == [float(t) for t in s.ddim_timesteps[:n][::-1]]       # the same pairs, walked back
    r, ref = IR.rel_l2(back, z0), float(gold["roundtrip_ref_rel"][k])
    print(f"constant-eps round trip on the device S={S} n={n}: {r:.3e} (the reference's arithmetic: {ref:.3e})")
    assert r <= max(1e-6, 4 * ref)


def test_batches_match_their_single_runs(tiny):
    """Two videos, and a pair of prompts of different lengths, each against its own single run (the GEMM tiling differs with the
    batch: to rounding, the 3e-3 of test_several_videos_per_batch_match_single_video_runs)."""
    net, _, betas = tiny
    z0 = IR.inputs()[0].to(DEV)
    g = torch.Generator().manual_seed(21)
    z1 = torch.randn(IR.SHAPE, generator=g).to(DEV)
    ctx = configs.TINY_UNET["context_dim"]
    ca, cb, uc = (torch.randn(1, n, ctx, generator=g).to(DEV) for n in (77, 154, 77))
    s = _sampler(net, betas).sampler
    s.make_schedule(4)
    kw = dict(unconditional_guidance_scale=9.0, model_timesteps="schedule")
    single = {k: s.encode(z, cc, 3, unconditional_conditioning=uc, **kw)[0] for k, (z, cc) in
              dict(a0=(z0, ca), a1=(z1, ca), b1=(z1, cb)).items()}
    zz = torch.cat([z0, z1])
    two, _ = s.encode(zz, ca, 3, unconditional_conditioning=uc, **kw)
    ragged, _ = s.encode(zz, [ca, cb], 3, unconditional_conditioning=uc, **kw)
    r = {"two[0]": IR.rel_l2(two[0:1], single["a0"]), "two[1]": IR.rel_l2(two[1:2], single["a1"]),
         "ragged[0]": IR.rel_l2(ragged[0:1], single["a0"]), "ragged[1]": IR.rel_l2(ragged[1:2], single["b1"])}
    print("batched DDIM inversion vs single runs, rel-L2: " + " ".join(f"{k} {v:.3e}" for k, v in r.items()))
    assert IR.rel_l2(single["a1"], single["b1"]) > 1e-2              # the prompt matters
    assert max(r.values()) < 3e-3, r


def test_public_route_equals_the_sampler_level_result(tiny):
    from sd_webui_text2video_amd.pipeline import TextToVideoSynthesis
    net, _, betas = tiny
    z0, noise, c, uc = (t.to(DEV) for t in IR.inputs())
    want = _sampler(net, betas).sample_loop(**_loop_kw(noise, c, uc, z0, inversion=True))
    pipe = TextToVideoSynthesis(sd_model=net, betas=betas, device=DEV)
    pipe.diffusion.progress = False
    _, x0 = pipe.infer_conditioned(c, uc, 4, 3, 1234, 9.0, 128, 128, 0.0, latents=z0, strength=0.75, is_vid2vid=True, sampler="DDIM",
                                   inversion=True, decode=False)
    assert x0.dtype == torch.float32 and torch.equal(x0, want)
    _, noised = pipe.infer_conditioned(c, uc, 4, 3, 1234, 9.0, 128, 128, 0.0, latents=z0, strength=0.75, is_vid2vid=True, sampler="DDIM",
                                       decode=False)
    assert not torch.equal(noised.float(), want)                     # without the keyword: the noising route
