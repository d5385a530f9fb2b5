"""CPU: the Lanczos resize of vid2vid / inpainting input (T2V_OP_RESAMPLE) — host side.

  * `packing.resample_table` + the integer two-pass algorithm (tests/resample_ref.py) reproduce what Pillow's
    `Image.resize(..., Image.LANCZOS)` returned when tests/golden/resize_lanczos.npz was recorded — and a live Pillow, where installed;
  * table properties; the lowering (`Program.resample`, the encoder's uint8 front end) executed by the CPU interpreter;
  * the routing of `process_modelscope`: off-size frames / inpainting image go through `pipe.resize_frames`, on-size ones never do,
    a tensor clip stays a tensor, a pipeline object without `resize_frames` keeps refusing.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import resample_ref as rr
from interp import Interp
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L, packing as pk, pipeline, vae as V
from sd_webui_text2video_amd.program import Program, Ref

GOLD = os.path.join(os.path.dirname(__file__), "golden", "resize_lanczos.npz")


def _fixture():
    z = np.load(GOLD)
    meta = json.loads(str(z["meta"]))
    return meta, z["head"]


_META, _HEAD = _fixture()
_CASES = _META["cases"]
_IDS = [c["name"] for c in _CASES]


class ResampleInterp(Interp):
    """tests/interp.Interp + T2V_OP_RESAMPLE: one integer pass (resample_ref.resample_pass); the token forms store lut[value]."""

    def _op21(self, op, ext):
        I = op.i
        n, h, w, c, out, axis, ksize, form, ld = I[0:9]
        assert c == 3
        src = self.view(op.p[0], (n, h, w, 3), (h * w * 3, w * 3, 3, 1), torch.uint8, ext).numpy()
        coef = self.mat(op.p[2], out, ksize, ksize, torch.int32, ext).numpy()
        bounds = self.mat(op.p[3], out, 2, 2, torch.int32, ext).numpy()
        res = torch.from_numpy(rr.resample_pass(src, coef, bounds, axis))
        rows = res.shape[0] * res.shape[1] * res.shape[2]
        if form == 0:
            self.view(op.p[1], (rows, 3), (3, 1), torch.uint8, ext).copy_(res.reshape(rows, 3))
            return
        lut = self.view(op.p[4], (256,), (1,), torch.float32, ext)
        dt = torch.float32 if form == 1 else torch.float16
        dst = self.mat(op.p[1], rows, ld, ld, dt, ext)
        dst.zero_()
        dst[:, :3] = lut[res.reshape(rows, 3).long()].to(dt)


# ---- the algorithm against the recorded Pillow results ------------------------------------------------------------------------
def test_fixture_is_small_and_marks_saturation():
    assert os.path.getsize(GOLD) < 64 * 1024 and len(_CASES) == 11 and _META["pillow"]
    by = {c["name"]: c for c in _CASES}
    assert not by["down_aspect"]["saturates"] and by["checker3_up"]["saturates"] and by["checker5_down"]["saturates"]
    assert by["clip24"]["frames"] == 24 and tuple(by["clip24"]["dst"]) == (576, 1024)


@pytest.mark.parametrize("case", _CASES, ids=_IDS)
def test_reference_algorithm_reproduces_pillow(case):
    x = rr.case_input(case)
    h2, w2 = case["dst"]
    out = rr.resample_ref(x, h2, w2)
    assert out.shape == (case["frames"], h2, w2, 3)
    assert np.array_equal(out.reshape(-1)[:256], _HEAD[_CASES.index(case)])
    assert rr.digest(out) == case["sha256"]
    assert bool(((out == 0) | (out == 255)).any()) == case["saturates"]


@pytest.mark.parametrize("case", [c for c in _CASES if c["frames"] == 1], ids=[c["name"] for c in _CASES if c["frames"] == 1])
def test_reference_algorithm_equals_live_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    x = rr.case_input(case)[0]
    h2, w2 = case["dst"]
    want = np.asarray(Image.fromarray(x).resize((w2, h2), Image.LANCZOS))
    got = rr.resample_ref(x, h2, w2)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.parametrize("a,b", [(576, 1024), (1024, 256), (333, 256), (1920, 1024), (64, 1024), (7, 3), (3, 7), (1, 5), (5, 1)])
def test_table_properties(a, b):
    coef, bounds = pk.resample_table(a, b)
    ksize = pk.resample_ksize(a, b)
    assert ksize == math.ceil(3.0 * max(a / b, 1.0)) * 2 + 1          # Pillow: ceil(support) * 2 + 1, support = 3 * max(scale, 1)
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (b, ksize) and bounds.shape == (b, 2)
    first, count = bounds[:, 0], bounds[:, 1]
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= a).all() and (first < a).all()
    assert (np.diff(first) >= 0).all()
    for o in range(b):
        assert not coef[o, count[o]:].any()
        assert abs(int(coef[o].sum()) - (1 << 22)) <= ksize          # normalised weights, each rounded to 2^-22
    with pytest.raises(ValueError):
        pk.resample_table(0, 4)


def test_identity_size_gives_no_pass():
    P, packer = Program("t"), pk.WeightPacker()
    with pytest.raises(ValueError, match="equal"):
        P.resample("r", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=1, src_hw=(8, 8), dst_hw=(8, 8))
    ops = P.resample("r", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=2, src_hw=(8, 12), dst_hw=(8, 20))
    assert [(o.kind, o.i[5]) for o in ops] == [(L.OP_RESAMPLE, 0)]
    ops = P.resample("r", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=2, src_hw=(8, 12), dst_hw=(5, 12))
    assert [(o.kind, o.i[5]) for o in ops] == [(L.OP_RESAMPLE, 1)]
    ops = P.resample("r", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=2, src_hw=(8, 12), dst_hw=(5, 20))
    assert [(o.i[5], o.i[1], o.i[2], o.i[4]) for o in ops] == [(0, 8, 12, 20), (1, 8, 20, 5)]     # horizontal first, like Pillow
    assert rr.resample_ref(np.zeros((1, 8, 8, 3), np.uint8), 8, 8).shape == (1, 8, 8, 3)


def test_malformed_records_are_refused_without_gpu(built_lib):
    """Host-side validation (plan creation, nothing is launched): sizes, channel count, pointers, output form."""
    h = ctypes.c_void_p()
    ptr = 0x1000
    good_i, good_p = (2, 8, 12, 3, 20, 0, 7, 0, 3), (ptr, ptr, ptr, ptr, 0)

    def create(i, p):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_RESAMPLE
        for k, v in enumerate(i):
            op[0].i[k] = v
        for k, v in enumerate(p):
            op[0].p[k] = v
        return built_lib.t2v_plan_create(op, 1, ctypes.byref(h)), built_lib.t2v_last_error()

    rc, _ = create(good_i, good_p)
    assert rc == 0
    built_lib.t2v_plan_destroy(h)
    bad = [((0, 8, 12, 3, 20, 0, 7, 0, 3), good_p, b"positive"), ((2, 8, 12, 3, 0, 0, 7, 0, 3), good_p, b"positive"),
           ((2, 8, 12, 3, 20, 0, 0, 0, 3), good_p, b"positive"), ((2, 8, 12, 4, 20, 0, 7, 0, 3), good_p, b"3 channels"),
           ((2, 8, 12, 3, 20, 2, 7, 0, 3), good_p, b"axis"), ((2, 8, 12, 3, 20, 0, 7, 3, 3), good_p, b"output form"),
           ((2, 8, 12, 3, 20, 0, 7, 2, 8), good_p, b"value table"), ((2, 8, 12, 3, 20, 0, 7, 1, 2), (ptr,) * 5, b"ld >= 3"),
           (good_i, (ptr, ptr, 0, ptr, 0), b"null resample pointer"), (good_i, (ptr, ptr, ptr, 0, 0), b"null resample pointer"),
           (good_i, (0, ptr, ptr, ptr, 0), b"null resample pointer"),
           ((1 << 20, 1 << 10, 12, 3, 20, 0, 7, 0, 3), good_p, b"too many rows")]
    for i, p, needle in bad:
        rc, msg = create(i, p)
        assert rc == -1 and needle in msg, (i, p, rc, msg)


# ---- lowering ---------------------------------------------------------------------------------------------------------------------
def _run_resample(x, dst_hw, form, ld=3):
    n, h, w, _ = x.shape
    P, packer = Program("t"), pk.WeightPacker()
    P.begin()
    P.resample("r", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), packer, n=n, src_hw=(h, w), dst_hw=dst_hw, form=form, ld=ld)
    P.finish()
    dt = {"u8": torch.uint8, "f32": torch.float32, "f16": torch.float16}[form]
    out = torch.empty((n, dst_hw[0], dst_hw[1], ld), dtype=dt)
    ResampleInterp(P, packer.materialise({}, "cpu")).run({L.EXT_X: torch.from_numpy(x), L.EXT_OUT: out})
    return out


@pytest.mark.parametrize("src,dst", [((37, 53), (24, 80)), ((24, 40), (24, 16)), ((20, 16), (48, 16)), ((16, 24), (16, 24))])
def test_resample_program_in_interpreter(src, dst):
    x = np.random.RandomState(7).randint(0, 256, (2,) + src + (3,), dtype=np.uint8)
    want = rr.resample_ref(x, *dst)
    if src != dst:
        assert np.array_equal(_run_resample(x, dst, "u8").numpy(), want)
    f32 = 2 * torch.from_numpy(want.astype(np.float32) / 255) - 1          # the reference's float32 arithmetic (process_modelscope.py:129,137)
    t32 = _run_resample(x, dst, "f32", ld=8)
    assert torch.equal(t32[..., :3], f32) and not t32[..., 3:].any()
    t16 = _run_resample(x, dst, "f16", ld=8)
    assert torch.equal(t16[..., :3], f32.half()) and not t16[..., 3:].any()
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1).repeat(3, axis=3)
    assert torch.equal(pk.resample_lut(), pipeline.frames_to_video_tensor(ramp)[0, 0, 0, 0])


def test_encoder_program_from_uint8_frames():
    """compute_latents on uint8 frames: ONE program = resample passes (the last one writing the entry tokens) + the encoder ops of the
    float path; in the interpreter its moments equal the float path's on the frames resized by resample_ref, bit for bit."""
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4, init_weights=False)
    ae.load_state_dict(synth.synth_state_dict(synth.param_spec(ae), seed=3), strict=True)
    x = np.random.RandomState(3).randint(0, 256, (2, 45, 70, 3), dtype=np.uint8)
    h, w = 64, 48
    low_f = V._VaeLowering(ae, 2, h, w, "f32", "f32")
    pf = low_f.build_encoder()
    low_u = V._VaeLowering(ae, 2, h, w, "f16", "f32")
    pu = low_u.build_encoder(u8_src=(45, 70))
    assert [o.kind for o in pu.ops[:2]] == [L.OP_RESAMPLE, L.OP_RESAMPLE] and pu.ops[1].i[7] == 2 and pu.ops[1].i[8] == 8
    assert pf.ops[0].name == "x.to_tokens" and pu.ops[1].p[1] == pf.ops[0].p[1]                    # same entry buffer
    assert [(o.kind, o.name, list(o.i)) for o in pu.ops[2:]] == [(o.kind, o.name, list(o.i)) for o in pf.ops[1:]]
    sized = rr.resample_ref(x, h, w)
    video = pipeline.frames_to_video_tensor(sized)[0].permute(1, 0, 2, 3).contiguous()             # [n, 3, h, w] float32
    mf, mu = torch.empty(2, 8, 8, 6), torch.empty(2, 8, 8, 6)
    Interp(pf, low_f.packer.materialise(ae.state_dict(), "cpu")).run({L.EXT_X: video, L.EXT_OUT: mf})
    ResampleInterp(pu, low_u.packer.materialise(ae.state_dict(), "cpu")).run({L.EXT_X: torch.from_numpy(x), L.EXT_OUT: mu})
    assert torch.isfinite(mu).all() and torch.equal(mf, mu)
    # on-size uint8 frames: one identity pass does the conversion
    pi = V._VaeLowering(ae, 2, h, w, "f16", "f32").build_encoder(u8_src=(h, w))
    assert [o.kind for o in pi.ops[:2]] == [L.OP_RESAMPLE, L.OP_GEMM] and pi.ops[0].i[6] == 1 and pi.ops[0].i[5] == 1


# ---- process_modelscope routing -------------------------------------------------------------------------------------------------
class _Pipe:
    device = "cpu"

    def __init__(self):
        self.resized, self.encoded, self.kw = [], [], None

    def resize_frames(self, frames, height, width):
        self.resized.append((frames, height, width))
        return torch.zeros((frames.shape[0], height, width, 3), dtype=torch.uint8)

    def compute_latents(self, vd, cpu_vae="GPU (half precision)", device=None):
        self.encoded.append(vd)
        F = vd.shape[0] if vd.dtype == torch.uint8 else vd.shape[2]
        return torch.full((1, 4, F, 1, 2), 0.5)

    def infer(self, prompt, n_prompt, steps, frames, seed, scale, width=256, height=256, **kw):
        self.kw = kw
        return [np.zeros((height, width, 3), np.uint8)] * frames, None, ""


def _args(pipe, **kw):
    d = dict(pipe=pipe, prompt="p", n_prompt="n", steps=7, frames=3, seed=40, cfg_scale=9.0, width=16, height=8, eta=0.0, sampler="DDIM_Gaussian")
    d.update(kw)
    return d


def test_process_modelscope_routes_off_size_input_through_resize_frames():
    pipe = _Pipe()
    clip = np.random.RandomState(0).randint(0, 256, (3, 11, 9, 3), dtype=np.uint8)
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=clip, strength=0.7))
    assert len(pipe.resized) == 1 and np.array_equal(pipe.resized[0][0], clip) and pipe.resized[0][1:] == (8, 16)
    assert len(pipe.encoded) == 1 and pipe.encoded[0].dtype == torch.uint8 and tuple(pipe.encoded[0].shape) == (3, 8, 16, 3)
    assert pipe.kw["is_vid2vid"] is True and pipe.kw["latents"].shape == (1, 4, 3, 1, 2)
    # the inpainting image: resized ONCE (not per frame, not per video of the batch), then repeated for every frame
    pipe = _Pipe()
    img = clip[0]
    pipeline.process_modelscope(_args(pipe, inpainting_frames=2, inpainting_image=img, inpainting_weights=[0.0, 0.5, 1.0], batch_count=2,
                                      stitch=lambda fr, info: b"x"))
    assert len(pipe.resized) == 1 and tuple(pipe.resized[0][0].shape) == (1, 11, 9, 3) and pipe.resized[0][1:] == (8, 16)
    assert np.array_equal(pipe.resized[0][0][0], img)
    assert len(pipe.encoded) == 2 and all(tuple(e.shape) == (3, 8, 16, 3) and e.dtype == torch.uint8 for e in pipe.encoded)


def test_process_modelscope_on_size_input_never_reaches_resize_frames():
    pipe = _Pipe()
    clip = np.random.RandomState(1).randint(0, 256, (3, 8, 16, 3), dtype=np.uint8)
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=clip, strength=0.7))
    pipeline.process_modelscope(_args(pipe, inpainting_frames=2, inpainting_image=clip[0], inpainting_weights=[0.0, 0.5, 1.0]))
    assert pipe.resized == [] and len(pipe.encoded) == 2
    for vd in pipe.encoded:                                   # the float video of today's path
        assert vd.dtype == torch.float32 and tuple(vd.shape) == (1, 3, 3, 8, 16)
    assert torch.equal(pipe.encoded[0], pipeline.frames_to_video_tensor(clip))


def test_process_modelscope_keeps_a_tensor_clip_a_tensor():
    pipe = _Pipe()
    clip = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (3, 4, 8, 3), dtype=np.uint8))
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=clip, strength=0.7))
    assert len(pipe.resized) == 1 and pipe.resized[0][0] is clip and pipe.resized[0][1:] == (8, 16)
    on = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (3, 8, 16, 3), dtype=np.uint8))
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=on, strength=0.7))
    assert len(pipe.resized) == 1 and pipe.encoded[-1] is on


def test_pipeline_object_without_resize_frames_keeps_refusing():
    class Old:
        device = "cpu"

        def compute_latents(self, vd, cpu_vae="GPU (half precision)", device=None):
            raise AssertionError("off-size input must be refused before it is encoded")

    pipe = Old()
    clip = np.zeros((3, 4, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="resize"):
        pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=clip, strength=0.5))
    with pytest.raises(ValueError, match="resize"):
        pipeline.process_modelscope(_args(pipe, inpainting_frames=2, inpainting_image=clip[0], inpainting_weights=[0.0, 0.5, 1.0]))
    assert hasattr(pipeline.TextToVideoSynthesis, "resize_frames")
