"""GPU (-m gpu): T2V_OP_RESAMPLE — Pillow's 8-bit Lanczos resize of vid2vid / inpainting input on the device, bit for bit.

  * every case of tests/golden/resize_lanczos.npz through the real op: bytes equal tests/resample_ref.py and the recorded Pillow digest,
    guard bytes around the intermediate and the output stay untouched, also at odd byte offsets inside larger buffers;
  * the 24-frame 320x576 -> 576x1024 clip in both output forms (uint8, and the VAE encoder's fp16 / fp32 entry tokens);
  * malformed records are refused by host-side validation (nothing is launched) and leave `t2v_async_status()` clean;
  * end to end on the tiny synthetic pipeline: off-size uint8 frames / inpainting image through `process_modelscope` give the bits of
    the same input resized beforehand by resample_ref; device frames of one pipeline chain into a vid2vid call at twice the size.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as rr
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L, packing as pk, pipeline, unet as U, vae as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5
_Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "resize_lanczos.npz"))
_CASES = json.loads(str(_Z["meta"]))["cases"]


def _run_pass(src_t, src_off, dst_t, dst_off, n, h, w, out, axis, form=0, ld=3, lut=None):
    coef, bounds = pk.resample_table(w if axis == 0 else h, out)
    ct, bt = torch.from_numpy(coef).to(DEV), torch.from_numpy(bounds).to(DEV)
    op = L.T2VOp()
    op.kind = L.OP_RESAMPLE
    for k, v in enumerate((n, h, w, 3, out, axis, coef.shape[1], form, ld)):
        op.i[k] = v
    op.p[0], op.p[1], op.p[2], op.p[3] = src_t.data_ptr() + src_off, dst_t.data_ptr() + dst_off, ct.data_ptr(), bt.data_ptr()
    op.p[4] = lut.data_ptr() if lut is not None else 0
    L.check(L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _guarded(nbytes, off):
    return torch.full((off + nbytes + 64,), GUARD, dtype=torch.uint8, device=DEV)


def _resize_guarded(x, h2, w2, off):
    """Two raw passes with source, intermediate and output at byte offset `off` inside guard-filled buffers."""
    n, h, w, _ = x.shape
    src = _guarded(x.size, off)
    src[off:off + x.size] = torch.from_numpy(x.reshape(-1)).to(DEV)
    cur, cur_hw, bufs = src, (h, w), []
    for axis, a, b in ([(0, w, w2)] if w != w2 else []) + ([(1, h, h2)] if h != h2 else []):
        oh, ow = (cur_hw[0], b) if axis == 0 else (b, cur_hw[1])
        dst = _guarded(n * oh * ow * 3, off)
        _run_pass(cur, off, dst, off, n, cur_hw[0], cur_hw[1], b, axis)
        bufs.append((dst, n * oh * ow * 3))
        cur, cur_hw = dst, (oh, ow)
    for buf, nb in bufs:                                   # the intermediate and the output: nothing outside [off, off + nb) was written
        host = buf.cpu().numpy()
        assert (host[:off] == GUARD).all() and (host[off + nb:] == GUARD).all()
    return bufs[-1][0][off:off + bufs[-1][1]].cpu().numpy().reshape(n, h2, w2, 3)


@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_every_fixture_case_through_the_op(case):
    x = rr.case_input(case)
    h2, w2 = case["dst"]
    want = rr.resample_ref(x, h2, w2)
    assert rr.digest(want) == case["sha256"]
    for off in (64, 77) if case["frames"] == 1 else (64,):          # aligned, and odd byte offsets inside larger buffers
        got = _resize_guarded(x, h2, w2, off)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"offset {off}: {len(bad)} bytes differ, first at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        assert rr.digest(got) == case["sha256"]


def test_clip_both_output_forms_and_resize_frames():
    case = next(c for c in _CASES if c["name"] == "clip24")
    x = rr.case_input(case)
    h2, w2 = case["dst"]
    want = rr.resample_ref(x, h2, w2)
    pipe = pipeline.TextToVideoSynthesis.__new__(pipeline.TextToVideoSynthesis)
    pipe.device = torch.device(DEV)
    got = pipe.resize_frames(x, h2, w2)
    assert got.dtype == torch.uint8 and got.is_cuda and rr.digest(got.cpu().numpy()) == case["sha256"]
    assert torch.equal(pipe.resize_frames(torch.from_numpy(x).to(DEV), h2, w2), got) and len(pipe._resize_programs) == 1
    # token forms: horizontal pass to uint8, vertical pass writing lut[value] as [rows, 8] tokens, padding zeroed
    n, h, w, _ = x.shape
    lut = pk.resample_lut().to(DEV)
    f32 = 2 * torch.from_numpy(want.astype(np.float32) / 255) - 1
    src = torch.from_numpy(x).to(DEV)
    mid = torch.empty((n, h, w2, 3), dtype=torch.uint8, device=DEV)
    _run_pass(src, 0, mid, 0, n, h, w, w2, 0)
    for form, dt in ((1, torch.float32), (2, torch.float16)):
        tok = torch.full((n, h2, w2, 8), 7.0, dtype=dt, device=DEV)
        _run_pass(mid, 0, tok, 0, n, h, w2, h2, 1, form=form, ld=8, lut=lut)
        tok = tok.cpu()
        assert torch.equal(tok[..., :3], f32.to(dt)) and not tok[..., 3:].any()


@pytest.mark.parametrize("form,dt", [(1, torch.float32), (2, torch.float16)])
@pytest.mark.parametrize("ld", [8, 5])
def test_width_only_resize_writes_tokens_in_the_horizontal_pass(form, dt, ld):
    """Frames whose height already matches: the LAST pass is the horizontal one, so it writes the tokens (ld 8 = the encoder's rows,
    one 16-byte store for fp16; ld 5 = the element-wise store path)."""
    x = np.random.RandomState(12).randint(0, 256, (2, 40, 301, 3), dtype=np.uint8)
    w2 = 517                                             # more than 256 pixels: several workgroups per row, a ragged last one
    want = rr.resample_ref(x, 40, w2)
    f32 = 2 * torch.from_numpy(want.astype(np.float32) / 255) - 1
    tok = torch.full((2 * 40 * w2 * ld + 16,), 7.0, dtype=dt, device=DEV)
    _run_pass(torch.from_numpy(x).to(DEV), 0, tok, 0, 2, 40, 301, w2, 0, form=form, ld=ld, lut=pk.resample_lut().to(DEV))
    tok = tok.cpu()
    assert (tok[-16:] == 7.0).all()
    tok = tok[:-16].view(2, 40, w2, ld)
    assert torch.equal(tok[..., :3], f32.to(dt)) and not tok[..., 3:].any()


def test_compute_latents_on_frames_of_matching_height(tiny_pipe):
    pipe, _, _ = tiny_pipe
    clip = np.random.RandomState(6).randint(0, 256, (3, 128, 75, 3), dtype=np.uint8)
    a = pipe.compute_latents(clip, "GPU", torch.device(DEV), height=128, width=128)       # horizontal pass writes the tokens
    b = pipe.compute_latents(pipeline.frames_to_video_tensor(rr.resample_ref(clip, 128, 128)), "GPU", torch.device(DEV))
    c = pipe.compute_latents(rr.resample_ref(clip, 128, 128), "GPU", torch.device(DEV))   # on-size uint8: the one-tap copy pass
    assert torch.equal(a, b) and torch.equal(c, b)


def test_malformed_records_are_refused_before_any_launch():
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    ptr = buf.data_ptr()
    for i, p in (((2, 8, 0, 3, 20, 0, 7, 0, 3), (ptr, ptr, ptr, ptr)), ((2, 8, 12, 4, 20, 0, 7, 0, 3), (ptr, ptr, ptr, ptr)),
                 ((2, 8, 12, 3, 20, 0, 7, 0, 3), (ptr, ptr, 0, ptr)), ((2, 8, 12, 3, 20, 0, 7, 5, 3), (ptr, ptr, ptr, ptr))):
        op = L.T2VOp()
        op.kind = L.OP_RESAMPLE
        for k, v in enumerate(i):
            op.i[k] = v
        for k, v in enumerate(p):
            op.p[k] = v
        assert lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, None) == -1 and b"resample" in lib.t2v_last_error()
    torch.cuda.synchronize()
    assert lib.t2v_async_status() == 0 and not buf.any()


@pytest.fixture(scope="module")
def tiny_pipe():
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4, init_weights=False)
    ae.load_state_dict(synth.synth_state_dict(synth.param_spec(ae), seed=3), strict=True)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=ae, betas=betas, device=DEV)
    pipe.diffusion.progress = False
    g = torch.Generator().manual_seed(5)
    c = torch.randn(1, 7, configs.TINY_UNET["context_dim"], generator=g)
    uc = torch.randn(1, 7, configs.TINY_UNET["context_dim"], generator=g)
    return pipe, c, uc


def _args(pipe, c, uc, **kw):
    d = dict(pipe=pipe, cond=c, uncond=uc, steps=8, frames=3, seed=1234, cfg_scale=9.0, width=128, height=128, eta=0.0,
             sampler="DDIM_Gaussian", cpu_vae="GPU", do_vid2vid=True, strength=0.5)
    d.update(kw)
    return d


def test_off_size_vid2vid_frames_equal_frames_resized_beforehand(tiny_pipe):
    pipe, c, uc = tiny_pipe
    clip = np.random.RandomState(4).randint(0, 256, (3, 90, 161, 3), dtype=np.uint8)
    sized = rr.resample_ref(clip, 128, 128)
    lat_a = pipe.compute_latents(clip, "GPU", torch.device(DEV), height=128, width=128)          # ONE program: resample + encoder
    lat_b = pipe.compute_latents(pipeline.frames_to_video_tensor(sized), "GPU", torch.device(DEV))
    assert torch.equal(lat_a, lat_b)
    fa = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, vid2vid_frames=clip)))
    xa = pipe.last_tensor.clone()
    fb = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, vid2vid_frames=sized)))
    assert torch.equal(xa, pipe.last_tensor) and np.array_equal(fa, fb) and torch.isfinite(xa).all()


def test_off_size_inpainting_image_equals_image_resized_beforehand(tiny_pipe):
    pipe, c, uc = tiny_pipe
    img = np.random.RandomState(8).randint(0, 256, (200, 75, 3), dtype=np.uint8)
    kw = dict(do_vid2vid=False, steps=4, inpainting_frames=2, inpainting_weights=[0.0, 0.5, 1.0])
    np.random.seed(3)
    fa = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, inpainting_image=img, **kw)))
    xa = pipe.last_tensor.clone()
    np.random.seed(3)
    fb = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, inpainting_image=rr.resample_ref(img, 128, 128), **kw)))
    assert torch.equal(xa, pipe.last_tensor) and np.array_equal(fa, fb) and torch.isfinite(xa).all()


def test_device_frames_chain_into_vid2vid_at_twice_the_size(tiny_pipe):
    pipe, c, uc = tiny_pipe
    rgb, _ = pipe.infer_conditioned(c, uc, 4, 3, 77, 9.0, 64, 64, 0.0, to_host=False)
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, 64, 64, 3)
    fa = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, vid2vid_frames=rgb)))               # stays on the device
    xa = pipe.last_tensor.clone()
    fb = np.stack(pipeline.process_modelscope(_args(pipe, c, uc, vid2vid_frames=rr.resample_ref(rgb.cpu().numpy(), 128, 128))))
    assert torch.equal(xa, pipe.last_tensor) and np.array_equal(fa, fb)
