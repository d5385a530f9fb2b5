"""CPU: the VideoCrafter driver seam — form 1 of T2V_OP_TO_UINT8 (torch_to_np) in the interpreter and `videocrafter.torch_to_np` against
bytes of the REAL reference's function on designed inputs (tests/golden/make_golden_frames.py), the decoder program with the form-1
tail, the unchanged form-0 record, and the host logic of `process_videocrafter` and of the per-video noise streams."""
import os
import types

import numpy as np
import pytest
import torch

import frames_inputs as FI
from interp_frames import FramesInterp
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers, vae as V, videocrafter as VC
from sd_webui_text2video_amd.program import NULL, Program, Ref
from test_samplers_cpu import _ddim_update_cpu, _lincomb_cpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def designed():
    z = np.load(os.path.join(GOLD, "torch_to_np_designed.npz"))
    d = {k: torch.from_numpy(z[k].copy()) for k in ("f32_in", "f32_out", "f32_half_out", "f16_out")}
    d["f16_in"] = torch.from_numpy(z["f16_in"].copy().view(np.float16))
    return d


# (name, input key, expected key, half)
KINDS = [("f32", "f32_in", "f32_out", False), ("f16", "f16_in", "f16_out", False), ("f32-half", "f32_in", "f32_half_out", True),
         ("f16-half", "f16_in", "f16_out", True)]


def _form1(video, half, tokens):
    """One form-1 record over `video` [NI, C, F, H, W], in the NCFHW layout or as channels-last tokens of ld = 4 -> the interpreter's bytes."""
    NI, C, Fr, H, W = video.shape
    dt = "f16" if video.dtype == torch.float16 else "f32"
    if tokens:
        src = torch.full((NI * Fr * H * W, 4), float("nan"), dtype=video.dtype)          # the padding channel is never read
        src[:, :C] = video.permute(0, 2, 3, 4, 1).reshape(-1, C)
        strides = (Fr * H * W * 4, 1, H * W * 4, W * 4, 4)
    else:
        src, strides = video.contiguous(), (C * Fr * H * W, Fr * H * W, H * W, W, 1)
    P = Program()
    op = P.to_uint8("u8", Ref("ext", L.EXT_X), dt, Ref("ext", L.EXT_OUT), NI=NI, C=C, F=Fr, H=H, W=W, strides=strides, half=half, form=1)
    assert op.i[15] == 1 and op.i[7] == 0 and op.i[6] == int(half)
    out = torch.full((NI, Fr, H, W, C), 77, dtype=torch.uint8)
    FramesInterp(P, {}).run({L.EXT_X: src, L.EXT_OUT: out})
    return out


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("tokens", [True, False], ids=["tokens-ld4", "ncfhw"])
def test_form1_and_torch_to_np_give_the_reference_bytes(designed, kind, tokens):
    _, kin, kout, half = kind
    video, n = FI.as_video(designed[kin], FI.FILL)
    want = FI.want_video(designed[kout], FI.FILL_BYTE, video.shape)
    assert video.shape[2] % 2 == 0 and n == designed[kin].numel()
    got = _form1(video, half, tokens)
    assert torch.equal(got, want)
    # the product's own CPU function: what the device route is contracted against.  `half`: the fp16 model's video is the fp16 tensor
    mine = VC.torch_to_np(video.half() if half else video)
    assert mine.dtype == torch.uint8 and torch.equal(mine, want)


def test_designed_inputs_expose_the_arithmetic(designed):
    x32, b32 = designed["f32_in"], designed["f32_out"]
    for k in ("f32_out", "f16_out"):
        assert sorted(set(designed[k].tolist())) == list(range(256)), k
    assert designed["f16_in"].numel() == 63490 and not torch.isnan(designed["f16_in"]).any()
    assert torch.isinf(designed["f16_in"]).sum() == 2 and torch.isinf(x32).sum() == 2
    # +-inf, -0 and the far values end at the clamp
    for v, b in ((float("inf"), 255), (float("-inf"), 0), (3.0, 255), (-1.5, 0), (1.0, 255), (-1.0, 0), (-0.0, 127), (0.0, 127)):
        assert b32[x32 == v].tolist()[0] == b, v
    # form 0's arithmetic (tensor2vid).  What it does to an fp16 video — every intermediate rounded to fp16, i[6] = 1 — gives other bytes.
    # Its fp32 chain trunc(clamp(x * 0.5 + 0.5, 0, 1) * 255) provably gives the SAME bytes as form 1 for every finite fp32 x:
    # x * 0.5 is exact, fl(x * 0.5 + 0.5) = fl(x + 1) / 2 (a power-of-two scaling commutes with rounding), and then a * 255 and
    # (2 a) * 127.5 are the same real product under the same rounding; the clamps cut at the same places.  So between the two fp32
    # kernels only the layout differs (videos side by side | one block per video), and the designed inputs confirm it rather than
    # tell them apart
    x16h = designed["f16_in"]
    form0_half = ((x16h * 0.5 + 0.5).clamp(0, 1) * 255).float().to(torch.uint8)
    fin16 = torch.isfinite(x16h)
    assert (form0_half[fin16] != designed["f16_out"][fin16]).sum() > 500             # (1002 of the 30 722 values in [-1, 1])
    fin32 = torch.isfinite(x32)
    assert torch.equal(((x32 * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)[fin32], b32[fin32])
    for name, x, want in (("f32", x32, b32), ("f16", designed["f16_in"].float(), designed["f16_out"])):
        fin = torch.isfinite(x)
        # round to nearest in place of truncation
        nearest = torch.round(((x + 1) * 127.5).clamp(0, 255)).to(torch.uint8)
        assert (nearest[fin] != want[fin]).any(), name
    # a contracted fma(x, 127.5, 127.5): one rounding.  Exact in float64 where |x| is in [2^-20, 2^20] (24 + 8 product bits, aligned with
    # 127.5 inside 53 bits), then rounded once to fp32.  fp32 inputs only: for an fp16 input x + 1 is exact and the two agree
    mid = torch.isfinite(x32) & (x32.abs() >= 2.0 ** -20) & (x32.abs() <= 2.0 ** 20)
    fma = (x32[mid].double() * 127.5 + 127.5).float().clamp(0, 255).to(torch.uint8)
    assert (fma != b32[mid]).any()
    x16 = designed["f16_in"].float()
    m16 = torch.isfinite(x16) & (x16.abs() >= 2.0 ** -20)
    assert torch.equal((x16[m16].double() * 127.5 + 127.5).float().clamp(0, 255).to(torch.uint8), designed["f16_out"][m16])


def test_form0_record_is_unchanged_and_form_is_validated():
    """`Program.to_uint8` without the keyword: the parent's record, field by field (i[15] = 0 like every record before the form existed)."""
    P = Program()
    src, dst = Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT)
    si = 5 * 2 ** 31 + 12
    op = P.to_uint8("u8", src, "f16", dst, NI=2, C=3, F=4, H=6, W=10, strides=(si, 1, 240, 40, 4), half=True, bgr=True)
    assert op.kind == L.OP_TO_UINT8 and op.name == "u8"
    assert op.i == [2, 3, 4, 6, 10, L.F16, 1, 1, si & 0xFFFFFFFF, si >> 32, 1, 240, 0, 40, 4] + [0] * (L.OP_NI - 15)
    assert op.f == [0.0] * L.OP_NF and op.p == [src, dst] + [NULL] * (L.OP_NP - 2) and op.out is None and P.ops == [op]
    op0 = P.to_uint8("u8", src, "f32", dst, NI=1, C=3, F=4, H=6, W=10, strides=(720, 1, 240, 40, 4), half=False, form=0)
    assert op0.i == [1, 3, 4, 6, 10, L.F32, 0, 0, 720, 0, 1, 240, 0, 40, 4] + [0] * (L.OP_NI - 15)
    op1 = P.to_uint8("u8", src, "f32", dst, NI=1, C=3, F=4, H=6, W=10, strides=(720, 1, 240, 40, 4), half=False, form=1)
    assert op1.i[:15] == op0.i[:15] and op1.i[15] == 1 and op1.i[16:] == op0.i[16:]
    with pytest.raises(ValueError):
        P.to_uint8("u8", src, "f32", dst, NI=1, C=3, F=4, H=6, W=10, strides=(720, 1, 240, 40, 4), half=False, form=2)
    with pytest.raises(ValueError):
        P.to_uint8("u8", src, "f32", dst, NI=1, C=3, F=4, H=6, W=10, strides=(720, 1, 240, 40, 4), half=False, bgr=True, form=1)


def test_record_validation_without_gpu(built_lib):
    """Validation runs before any HIP call: i[15] outside {0, 1} and form 1 with bgr are T2V_ERR_BAD_ARG."""
    import ctypes
    h = ctypes.c_void_p()

    def create(form, bgr):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_TO_UINT8
        for k, v in enumerate((1, 3, 2, 8, 8, L.F32, 0, bgr, 384, 0, 128, 64, 0, 8, 1, form)):
            op[0].i[k] = v
        op[0].p[0], op[0].p[1] = 0x1000, 0x2000
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    assert create(0, 0)[0] == 0 and create(0, 1)[0] == 0 and create(1, 0)[0] == 0
    for bad in ((2, 0), (-1, 0), (1, 1)):
        rc, msg = create(*bad)
        assert rc == -1 and b"uint8" in msg, (bad, rc, msg)


# ---- the decoder program with the form-1 tail ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_vae():
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4, init_weights=False)
    ae.load_state_dict(synth.synth_state_dict(synth.param_spec(ae), seed=3), strict=True)
    return ae


def _decode_both(ae, z, out_dt):
    """One chunk z [n, 4, 8, 8] through the float program and through the program with the form-1 tail, in the interpreter."""
    n = z.shape[0]
    lo_f, lo_u = V._VaeLowering(ae, n, 8, 8, "f32", out_dt), V._VaeLowering(ae, n, 8, 8, "f32", out_dt)
    pf, pu = lo_f.build(None), lo_u.build((1, False, "np"))
    kinds = [op.kind for op in pu.ops]
    assert kinds.count(L.OP_TO_UINT8) == 1 and kinds[-1] == L.OP_TO_UINT8 and L.OP_CL_TO_NCTHW not in kinds and pu.ops[-1].i[15] == 1
    assert [op.kind for op in pf.ops][:-1] == kinds[:-1] and pf.ops[-1].kind == L.OP_CL_TO_NCTHW
    assert pu.ops[-1].i[6] == int(out_dt == "f16") and pu.ops[-1].i[14] == 4            # tokens of ld 4
    img = torch.empty(n, 3, 64, 64, dtype=torch.float16 if out_dt == "f16" else torch.float32)
    FramesInterp(pf, lo_f.packer.materialise(ae.state_dict(), "cpu")).run({L.EXT_X: z, L.EXT_OUT: img})
    u8 = torch.zeros(1, n, 64, 64, 3, dtype=torch.uint8)
    FramesInterp(pu, lo_u.packer.materialise(ae.state_dict(), "cpu")).run({L.EXT_X: z, L.EXT_OUT: u8})
    return VC.torch_to_np(img), u8[0]


@pytest.mark.parametrize("chunk,out_dt", [(None, "f32"), (1, "f32"), (2, "f32"), (None, "f16"), (2, "f16")])
def test_decoder_program_with_form1_tail(tiny_vae, chunk, out_dt):
    """5 frames of an 8x8 latent, scaled so that the frames reach both clamps; chunks of None, 1 and 2 (ragged: 2, 2, 1)."""
    z = torch.randn(5, 4, 8, 8, generator=torch.Generator().manual_seed(21)) * 3.0
    parts = [z] if chunk is None else list(torch.split(z, chunk))
    assert [p.shape[0] for p in parts] == {None: [5], 1: [1] * 5, 2: [2, 2, 1]}[chunk]
    both = [_decode_both(tiny_vae, p.contiguous(), out_dt) for p in parts]
    want, got = torch.cat([b[0] for b in both]), torch.cat([b[1] for b in both])
    assert got.shape == (5, 64, 64, 3) and torch.equal(got, want)
    assert len(set(got.reshape(-1).tolist())) > 100                   # real frames, not one clamp value


# ---- host logic of process_videocrafter and of the per-video streams ------------------------------------------------------------------------
def _eps_standin(x, t, c, **kw):
    """An elementwise stand-in for the UNet: every output element depends on its own input element and on per-sample scalars."""
    s = c.float().mean(dim=(1, 2)).view(-1, 1, 1, 1, 1)
    return 0.3 * x + 0.1 * torch.sin(x) + 0.05 * s + 1e-4 * t.float().view(-1, 1, 1, 1, 1)


class _Enc:
    def __init__(self):
        self.calls = []

    def encode(self, prompts):
        self.calls.append(list(prompts))
        ctx = FI.driver_inputs()[0]
        return torch.cat([ctx[0:1] if p == "a cat" else ctx[1:2] for p in prompts])


@pytest.fixture()
def driver(monkeypatch):
    """LatentDiffusion's schedule around the elementwise stand-in; the device bindings replaced by their torch restatements; the uint8
    decode replaced by a recorder (the real one is a device program: tests/test_gpu_videocrafter_driver.py)."""
    noises = []

    def update(out, xt, eps, noise, coef, guided, mode):
        noises.append(noise.clone())
        return _ddim_update_cpu(out, xt, eps, noise, coef, guided, mode)
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update", update)
    state = types.SimpleNamespace(interrupted=False, skipped=False, sampling_step=0, sampling_steps=0)
    monkeypatch.setattr(samplers, "state", state)
    m = VC.LatentDiffusion.__new__(VC.LatentDiffusion)
    torch.nn.Module.__init__(m)
    VC.LatentDiffusion.register_schedule(m, **configs.LVDM_SCHEDULE)
    m.apply_model = _eps_standin
    m.model = types.SimpleNamespace(diffusion_model=types.SimpleNamespace(refresh_weights=lambda d: None, auto_refresh=True, in_channels=4,
                                                                          temporal_length=16))
    m.image_size, m.cond_stage_model = [8, 8], _Enc()
    m.latents, m.decode_bs = [], []

    def decode_u8(z, decode_bs=16, to_host=True):
        m.latents.append(z.clone())
        m.decode_bs.append(decode_bs)
        b, _, t, h, w = z.shape
        return VC.torch_to_np(z[:, :3].repeat_interleave(8, 3).repeat_interleave(8, 4) / 3.0)
    m.decode_first_stage_uint8 = decode_u8
    m.decode_first_stage = lambda *a, **k: pytest.fail("the driver's frames leave as uint8")
    m.noises, m.state = noises, state
    return m


def _args(model, **kw):
    return {**dict(model=model, prompt="a cat", n_prompt="", steps=4, frames=5, seed=1234, cfg_scale=7.5, eta=1.0, fps=8, width=999, height=7), **kw}


def _spy_sampler(model):
    smp = VC.DDIMSampler(model)
    smp.seen = []
    real = smp.sample

    def sample(**kw):
        gens = smp.noise_gens
        smp.seen.append(dict(batch=kw["batch_size"], x_T=None if kw.get("x_T") is None else kw["x_T"].clone(),
                             seeds=[smp.noise_gen.initial_seed()] if gens is None else [g.initial_seed() for g in gens],
                             cond=kw["conditioning"], uncond=kw["unconditional_conditioning"], S=kw["S"], eta=kw["eta"],
                             cfg=kw["unconditional_guidance_scale"], shape=list(kw["shape"])))
        return real(**kw)
    smp.sample = sample
    return smp


U64 = (1 << 64) - 1          # Generator.manual_seed(-1)


@pytest.mark.parametrize("seed", [1234, -1])
def test_one_pass_equals_the_loop_on_an_elementwise_model(driver, seed):
    """On the CPU the start latents come from the default generator in both routes, so with an elementwise model the two agree exactly."""
    V_ = 3
    smp = _spy_sampler(driver)
    torch.manual_seed(5)
    loop = VC.process_videocrafter(_args(driver, sampler=smp, batch_count=V_, one_pass=False, seed=seed))
    assert [s["seeds"] for s in smp.seen] == [[seed + v if seed != -1 else U64] for v in range(V_)]
    assert all(s["batch"] == 1 and s["x_T"] is None and s["shape"] == [4, 5, 8, 8] for s in smp.seen)      # width / height ignored, frames = 5
    loop_lat, loop_noise = list(driver.latents), list(driver.noises)
    assert driver.decode_bs == [1] * V_ and len(driver.cond_stage_model.calls) == 2 * V_        # the loop encodes both prompts per video
    driver.latents.clear(), driver.noises.clear(), driver.decode_bs.clear(), driver.cond_stage_model.calls.clear()

    smp2 = _spy_sampler(driver)
    torch.manual_seed(5)
    want_xT = torch.cat([torch.randn(1, 4, 5, 8, 8) for _ in range(V_)])             # V consecutive draws of ONE video's shape
    torch.manual_seed(5)
    one = VC.process_videocrafter(_args(driver, sampler=smp2, batch_count=V_, seed=seed, decode_frame_bs=None))
    (s,) = smp2.seen
    assert s["batch"] == V_ and s["seeds"] == [seed + v if seed != -1 else U64 for v in range(V_)] and torch.equal(s["x_T"], want_xT)
    assert (s["S"], s["eta"], s["cfg"], s["shape"]) == (4, 1.0, 7.5, [4, 5, 8, 8])
    ctx = FI.driver_inputs()[0]
    assert torch.equal(s["cond"]["c_crossattn"][0], ctx[0:1].repeat(V_, 1, 1)) and torch.equal(s["uncond"]["c_crossattn"][0], ctx[1:2].repeat(V_, 1, 1))
    assert driver.cond_stage_model.calls == [["a cat"], [""]]         # the conditions are computed once
    assert smp2.noise_gens is None                                    # the sampler is handed back as it came
    assert driver.decode_bs == [None] and len(driver.latents) == 1 and driver.latents[0].shape == (V_, 4, 5, 8, 8)
    for v in range(V_):
        assert torch.equal(driver.latents[0][v:v + 1], loop_lat[v]), v
        assert np.array_equal(one[v], loop[v]) and one[v].shape == (5, 64, 64, 3) and one[v].dtype == np.uint8
    # the noise: video v's stream is the batch-of-one stream of seed + v, step by step
    for step in range(4):
        for v in range(V_):
            assert torch.equal(driver.noises[step][v:v + 1], loop_noise[v * 4 + step])
    same = torch.equal(driver.noises[0][0], driver.noises[0][1])
    assert same == (seed == -1)                                       # seed -1: every video the same stream (the reference's quirk, kept)
    assert not np.array_equal(one[0], one[1])                         # (the start latents still differ)


def test_state_fields_interrupt_and_skip(driver):
    st = driver.state
    st.skipped = True
    smp = VC.DDIMSampler(driver)
    jobs = []
    real = driver.decode_first_stage_uint8

    def decode(z, **k):
        jobs.append((st.job_count, st.job_no, st.job, st.skipped))
        if len(jobs) == 2:
            st.interrupted = True
        return real(z, **k)
    driver.decode_first_stage_uint8 = decode
    out = VC.process_videocrafter(_args(driver, sampler=smp, batch_count=4, one_pass=False))
    assert jobs == [(4, 1, "Batch 1 out of 4", False), (4, 2, "Batch 2 out of 4", False)]
    assert len(out) == 2 and st.job_no == 3 and st.job == "Batch 2 out of 4"       # the break comes before the third job's name
    # already interrupted: nothing is sampled on either route
    for one_pass in (False, True):
        before = len(jobs)
        assert VC.process_videocrafter(_args(driver, sampler=smp, batch_count=2, one_pass=one_pass)) == [] and len(jobs) == before
        assert VC.process_videocrafter(_args(driver, sampler=smp, batch_count=2, one_pass=one_pass, stitch=lambda f, fps: b"x")) == []
    st.interrupted = False
    VC.process_videocrafter(_args(driver, sampler=smp, batch_count=2))
    assert jobs[-1] == (2, 1, "Batches 1-2 out of 2", False) and st.job_no == 2


@pytest.mark.parametrize("one_pass", [True, False])
def test_return_values_with_and_without_stitch(driver, one_pass):
    import base64
    got = []

    def stitch(frames, fps):
        got.append((frames.copy(), fps))
        return b"mp4:" + bytes([len(got)])
    urls = VC.process_videocrafter(_args(driver, batch_count=3, one_pass=one_pass, stitch=stitch))           # (no sampler given: one is made)
    assert len(got) == 3 and all(f.shape == (5, 64, 64, 3) and f.dtype == np.uint8 and fps == 8 for f, fps in got)
    assert urls == ["data:video/mp4;base64," + base64.b64encode(b"mp4:\x03").decode()]               # the LAST video only
    assert not np.array_equal(got[0][0], got[1][0])
    vids = VC.process_videocrafter(_args(driver, batch_count=1, one_pass=one_pass))
    assert isinstance(vids, list) and len(vids) == 1 and vids[0].shape == (5, 64, 64, 3)
    assert driver.latents[-1].shape == (1, 4, 5, 8, 8)               # one video: the loop route either way
    with pytest.raises(NotImplementedError, match="only the DDIM path"):
        VC.process_videocrafter(_args(driver, batch_count=2, one_pass=one_pass, sample_type="ddpm"))


def test_noise_gens_length_and_default_stream(driver):
    ctx, x_T = FI.driver_inputs()
    kw = dict(S=4, conditioning={"c_crossattn": [ctx[0:1].repeat(2, 1, 1)]}, batch_size=2, shape=list(FI.SHAPE), verbose=False, eta=1.0,
              x_T=x_T[:2], unconditional_guidance_scale=7.5, unconditional_conditioning={"c_crossattn": [ctx[1:2].repeat(2, 1, 1)]})
    smp = VC.DDIMSampler(driver)
    assert smp.noise_gens is None
    for n in (1, 3):
        smp.noise_gens = [torch.Generator().manual_seed(k) for k in range(n)]
        with pytest.raises(ValueError, match="one per video"):
            smp.sample(**kw)
    assert driver.noises == []
    # noise_gens = None: ONE draw of the batch's shape per step from noise_gen, the global generator untouched — as before
    smp.noise_gens = None
    smp.noise_gen.manual_seed(9)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    a, _ = smp.sample(**kw)
    assert torch.equal(torch.get_rng_state(), before)
    g = torch.Generator().manual_seed(9)
    assert len(driver.noises) == 4 and all(torch.equal(n, torch.randn(2, *FI.SHAPE, generator=g)) for n in driver.noises)
    # with the list: per video, batch-of-one draws; the global generator untouched; `sample_noise` still wins
    driver.noises.clear()
    smp.noise_gens = [torch.Generator().manual_seed(40), torch.Generator().manual_seed(41)]
    b, _ = smp.sample(**kw)
    assert torch.equal(torch.get_rng_state(), before) and not torch.equal(a, b)
    g0, g1 = torch.Generator().manual_seed(40), torch.Generator().manual_seed(41)
    for n in driver.noises:
        assert torch.equal(n, torch.cat([torch.randn(1, *FI.SHAPE, generator=g0), torch.randn(1, *FI.SHAPE, generator=g1)]))
    driver.noises.clear()
    fixed = torch.randn(2, *FI.SHAPE, generator=torch.Generator().manual_seed(1))
    smp.sample(**kw, sample_noise=fixed)
    assert all(torch.equal(n, fixed) for n in driver.noises) and smp.noise_gens[0].initial_seed() == 40
    g0 = torch.Generator().manual_seed(40)
    for _ in range(4):
        torch.randn(1, *FI.SHAPE, generator=g0)
    assert torch.equal(torch.randn(3, generator=smp.noise_gens[0]), torch.randn(3, generator=g0))        # no draw was taken for it
