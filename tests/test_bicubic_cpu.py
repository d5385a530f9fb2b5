"""CPU: the float bicubic mode of T2V_OP_RESAMPLE (i[9] = 1) — tables, arithmetic (tests/interp_bicubic.py), lowering, the library's
validation and the opt-in switch of T2VAdapterDepth, without a GPU.

Semantics.  The reference's call is torch's `F.interpolate(x, size, mode="bicubic", align_corners=False)` (ddpm3d.py:1443-1462).  Per shape,
with exact = the same call on float64 input: err_ref = max |F.interpolate(x) - exact|, err_int = max |interpreter(x) - exact|, and the gate
is err_int <= 2 err_ref — both are float32 evaluations of the same 16-tap sum, a factor 2 covers the order of summation, and a wrong tap,
weight or clamp shows as 1e-2 or more.  Measured: profiles/bicubic.txt (ratios 0.00 .. 1.08)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapter_ref as AR
from interp_bicubic import bicubic_interp, bicubic_record
from oracle import configs
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd import vae as V
from sd_webui_text2video_amd import videocrafter as VC
from sd_webui_text2video_amd.program import BoundProgram, Program, Ref

SHAPES = [((1, 1, 1), (3, 5)), ((2, 2, 3), (7, 5)), ((3, 5, 7), (13, 3)), ((2, 8, 8), (24, 16)), ((2, 24, 16), (8, 8)), ((3, 32, 32), (24, 24)),
          ((1, 24, 24), (32, 32)), ((1, 4, 300), (3, 259)), ((3, 40, 56), (384, 384)), ((2, 384, 384), (40, 56))]
IDS = [f"{p}x{h}x{w}-{ho}x{wo}" for (p, h, w), (ho, wo) in SHAPES]


def shape_input(src):
    return torch.randn(*src, generator=torch.Generator().manual_seed(0))


def errors(src, dst):
    """-> (err_ref, err_int, err64): torch float32, the interpreter, and the interpreter in float64, each against torch in float64."""
    x = shape_input(src)
    kw = dict(size=dst, mode="bicubic", align_corners=False)
    exact = F.interpolate(x[None].double(), **kw)[0].numpy()
    ref = F.interpolate(x[None], **kw)[0].numpy()
    got = bicubic_interp(x.numpy(), *dst)
    assert got.dtype == np.float32 and got.shape == exact.shape
    got64 = bicubic_interp(x.double().numpy(), *dst, dtype=np.float64)
    return float(np.abs(ref - exact).max()), float(np.abs(got - exact).max()), float(np.abs(got64 - exact).max())


# ---- semantics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_interpreter_is_as_close_to_exact_as_torch(src, dst):
    err_ref, err_int, err64 = errors(src, dst)
    print(f"bicubic {src} -> {dst}: err_ref {err_ref:.3e}  err_int {err_int:.3e}  ratio {err_int / max(err_ref, 1e-300):.2f}  float64 {err64:.1e}")
    assert err_int <= 2 * err_ref, (src, dst, err_int, err_ref)
    assert err64 <= 1e-12, (src, dst, err64)           # the tables themselves: float64 weights on float64 input (measured <= 2e-14)


def test_fp16_input_is_converted_exactly():
    x = shape_input((3, 5, 7)).half().numpy()
    assert np.array_equal(bicubic_interp(x, 13, 3), bicubic_interp(x.astype(np.float32), 13, 3))


# ---- impulses -------------------------------------------------------------------------------------------------------------------------
def test_impulse_images_give_the_products_the_tables_predict():
    H, W, Ho, Wo = 5, 7, 13, 3
    (wy, iy), (wx, ix) = pk.bicubic_table(H, Ho), pk.bicubic_table(W, Wo)
    f32 = np.float32
    for r in range(H):
        for c in range(W):
            x = np.zeros((1, H, W), f32)
            x[0, r, c] = 1.0
            got = bicubic_interp(x, Ho, Wo)[0]
            for y in range(Ho):
                for xo in range(Wo):
                    # the record's order on an impulse: the taps that name (r, c) contribute their weight, the others an exact 0
                    acc = None
                    for a in range(4):
                        h = None
                        for b in range(4):
                            t = f32(wx[xo, b]) * f32(1.0 if (iy[y, a] == r and ix[xo, b] == c) else 0.0)
                            h = t if h is None else f32(h + t)
                        t = f32(wy[y, a] * h)
                        acc = t if acc is None else f32(acc + t)
                    assert got[y, xo] == acc, (r, c, y, xo)
                    if not ((iy[y] == r).any() and (ix[xo] == c).any()):
                        assert got[y, xo] == 0.0, (r, c, y, xo)
    # borders collect the clamped taps: output (0, 0) names source row 0 three times and column 0 twice, and the corner impulse shows
    # the sums of the replicated weights
    assert list(iy[0]) == [0, 0, 0, 1] and list(ix[0]) == [0, 0, 1, 2]
    x = np.zeros((1, H, W), f32)
    x[0, 0, 0] = 1.0
    want = float(wy[0, :3].astype(np.float64).sum() * wx[0, :2].astype(np.float64).sum())
    assert abs(float(bicubic_interp(x, Ho, Wo)[0, 0, 0]) - want) < 1e-6 and abs(want - float(wy[0, 2]) * float(wx[0, 1])) > 1e-2
    x = np.zeros((1, H, W), f32)
    x[0, H - 1, W - 1] = 1.0
    assert list(iy[-1]) == [3, 4, 4, 4] and list(ix[-1]) == [4, 5, 6, 6]
    want = float(wy[-1, 1:].astype(np.float64).sum() * wx[-1, 2:].astype(np.float64).sum())
    assert abs(float(bicubic_interp(x, Ho, Wo)[0, -1, -1]) - want) < 1e-6 and abs(want - float(wy[-1, 1]) * float(wx[-1, 2])) > 1e-2


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1, 3), (1, 1), (2, 7), (5, 13), (7, 3), (8, 24), (24, 8), (32, 24), (24, 32), (300, 259), (40, 384), (384, 56),
                                 (256, 384), (384, 256)])
def test_table_properties(a, b):
    w, idx = pk.bicubic_table(a, b)
    assert w.dtype == np.float32 and idx.dtype == np.int32 and w.shape == idx.shape == (b, 4)
    assert (idx >= 0).all() and (idx <= a - 1).all() and (np.diff(idx, axis=1) >= 0).all() and (np.diff(idx, axis=0) >= 0).all()
    # the float64 weights sum to 1 up to their own rounding; each float32 weight is off by at most half an ulp of [0.5, 1): 4 x 2^-25
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= np.finfo(np.float32).eps
    w64, idx64 = pk.bicubic_table(a, b, dtype=np.float64)
    assert w64.dtype == np.float64 and np.array_equal(idx64, idx) and np.array_equal(w64.astype(np.float32), w)
    assert np.abs(w64.sum(axis=1) - 1.0).max() <= 8 * np.finfo(np.float64).eps
    if a == b:
        assert np.array_equal(w, np.tile(np.array([0, 1, 0, 0], np.float32), (b, 1)))
        assert np.array_equal(idx[:, 1], np.arange(a))


def test_equal_sizes_are_the_identity_and_bad_sizes_raise():
    w, idx = pk.bicubic_table(6, 6)
    assert np.array_equal(w, np.tile(np.array([0, 1, 0, 0], np.float32), (6, 1))) and np.array_equal(idx[:, 1], np.arange(6))
    x = shape_input((2, 6, 5)).numpy()
    assert np.array_equal(bicubic_interp(x, 6, 5), x)
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError, match="positive"):
            pk.bicubic_table(*bad)


# ---- lowering -------------------------------------------------------------------------------------------------------------------------
def _bicubic_records(prog):
    return [o for o in prog.ops if o.kind == L.OP_RESAMPLE and o.i[9] != 0]


def test_program_bicubic_emits_one_record_with_the_documented_fields():
    P, packer = Program("t"), pk.WeightPacker()
    P.begin()
    op = P.bicubic("b", Ref("ext", L.EXT_X), "f16", Ref("ext", L.EXT_OUT), packer, planes=6, src_hw=(5, 7), dst_hw=(13, 3))
    op2 = P.bicubic("b2", Ref("ext", L.EXT_X), "f32", Ref("ext", L.EXT_OUT), packer, planes=2, src_hw=(5, 7), dst_hw=(13, 3))
    P.finish()
    assert P.ops == [op, op2] and op.kind == L.OP_RESAMPLE
    assert list(op.i[:12]) == [6, 5, 7, 1, 13, 0, 4, 1, 0, 1, 3, L.F16] and not any(op.i[12:]) and not any(op.f)
    assert list(op2.i[:12]) == [2, 5, 7, 1, 13, 0, 4, 1, 0, 1, 3, L.F32]
    assert op.p[0] == Ref("ext", L.EXT_X) and op.p[1] == Ref("ext", L.EXT_OUT) and all(p.space == "null" for p in op.p[4:])
    # the tables: one fp32 and one int32 image per geometry, shared by the two passes
    assert [(n, d) for n, d, _ in packer.recipes] == [("bicubic:5x7->13x3:w", "f32"), ("bicubic:5x7->13x3:idx", "i32")]
    assert op.p[2] == op2.p[2] == Ref("weight", 0, "bicubic:5x7->13x3:w") and op.p[3] == op2.p[3] == Ref("weight", 0, "bicubic:5x7->13x3:idx")
    packed = packer.materialise({}, "cpu")
    w, idx = packed["bicubic:5x7->13x3:w"], packed["bicubic:5x7->13x3:idx"]
    assert w.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(w.shape) == tuple(idx.shape) == (16, 4)
    assert np.array_equal(w.numpy()[:13], pk.bicubic_table(5, 13)[0]) and np.array_equal(idx.numpy()[13:], pk.bicubic_table(7, 3)[1])
    x = shape_input((6, 5, 7)).half().numpy()
    assert np.array_equal(bicubic_record(op, x, w.numpy(), idx.numpy()), bicubic_interp(x, 13, 3))
    with pytest.raises(ValueError, match="equal"):
        P.bicubic("b3", Ref("ext", L.EXT_X), "f32", Ref("ext", L.EXT_OUT), packer, planes=2, src_hw=(8, 8), dst_hw=(8, 8))
    assert len(P.ops) == 2


def _small_adapter():
    return VC.Adapter(channels=[320], nums_rb=2, cin=64, ksize=1, sk=True, use_conv=False, init_weights=False)


def test_opt_in_depth_program_is_a_bicubic_pass_and_the_front_end():
    net = _small_adapter()
    comp = net._compile(5, 32, 32, "f32", True, front_only=True, src_hw=(24, 24))
    rs, tok = comp.prog.ops
    assert (rs.kind, tok.kind) == (L.OP_RESAMPLE, L.OP_DEPTH_TOKENS)
    assert list(rs.i[:12]) == [5, 24, 24, 1, 32, 0, 4, 1, 0, 1, 32, L.F32]
    assert list(tok.i[:6]) == [5, 32, 32, L.F32, 1, 64]
    # the bicubic destination is an arena buffer of its own, read by the front end; the tokens go to the caller's slot, the tables are weights
    dst = rs.p[1]
    assert rs.p[0] == Ref("ext", L.EXT_X) and dst.space == "arena" and tok.p[0] == dst and tok.p[1] == Ref("ext", L.EXT_ADAPTER)
    assert dst.off >= 0 and dst.off + 5 * 32 * 32 * 4 <= comp.prog.arena.high
    assert rs.p[2].space == rs.p[3].space == "weight" and rs.p[2].name != rs.p[3].name
    assert {n for n, _, _ in comp.packer.recipes} == {rs.p[2].name, rs.p[3].name}
    # fp16 depth maps of a rectangular size
    comp16 = net._compile(2, 16, 24, "f16", True, front_only=True, src_hw=(7, 40))
    assert [o.kind for o in comp16.prog.ops] == [L.OP_RESAMPLE, L.OP_DEPTH_TOKENS] and comp16.prog.ops[0].i[11] == L.F16 and comp16.prog.ops[1].i[3] == L.F32
    # depth maps already at the target size: the front end alone, as before
    same = net._compile(5, 32, 32, "f32", True, front_only=True)
    assert [o.kind for o in same.prog.ops] == [L.OP_DEPTH_TOKENS] and same.prog.ops[0].p[0] == Ref("ext", L.EXT_X) and not same.packer.recipes
    with pytest.raises(AssertionError):
        net._compile(5, 32, 32, "f32", True, front_only=False, src_hw=(24, 24))


def test_opt_in_depth_program_in_the_interpreter_is_resize_then_normalise():
    """The two records evaluated on the CPU: the bicubic interpreter, then the reference's normalisation (tests/adapter_ref.py) in float32,
    rounded to the fp16 values the front end stores."""
    net = _small_adapter()
    comp = net._compile(3, 16, 24, "f32", True, front_only=True, src_hw=(10, 9))
    packed = comp.packer.materialise({}, "cpu")
    rs = comp.prog.ops[0]
    d = shape_input((3, 10, 9)).numpy() * 3 + 5
    big = bicubic_record(rs, d, packed[rs.p[2].name].numpy(), packed[rs.p[3].name].numpy())
    assert big.shape == (3, 16, 24) and np.array_equal(big, bicubic_interp(d, 16, 24))
    ref = F.interpolate(torch.from_numpy(d)[:, None], size=(16, 24), mode="bicubic", align_corners=False)
    assert (AR.normalise_depth(torch.from_numpy(big)[:, None]) - AR.normalise_depth(ref)).abs().max() < 1e-5


def test_existing_lowerings_hold_no_bicubic_record():
    net = _small_adapter()
    progs = [net._compile(5, 32, 32, "f32", True).prog, net._compile(5, 32, 32, "f16", False, front_only=True).prog]
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4, init_weights=False)
    progs.append(V._VaeLowering(ae, 2, 64, 48, "f16", "f32").build_encoder(u8_src=(45, 70)))
    P = Program("resize")
    P.begin()
    P.resample("frames.resample", Ref("ext", L.EXT_X), Ref("ext", L.EXT_OUT), pk.WeightPacker(), n=2, src_hw=(45, 70), dst_hw=(64, 48))
    P.finish()
    progs.append(P)
    assert sum(o.kind == L.OP_RESAMPLE for p in progs for o in p.ops) == 4
    for p in progs:
        assert p.ops and not _bicubic_records(p) and all(not any(o.i[9:]) for o in p.ops if o.kind == L.OP_RESAMPLE)


# ---- validation (plan creation: nothing is launched) --------------------------------------------------------------------------------------
def test_malformed_bicubic_records_are_refused_without_gpu(built_lib):
    h = ctypes.c_void_p()
    ptr = 0x1000
    good_i, good_p = (6, 5, 7, 1, 13, 0, 4, 1, 0, 1, 3, L.F16), (ptr, ptr, ptr, ptr)

    def create(i, p):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_RESAMPLE
        for k, v in enumerate(i):
            op[0].i[k] = v
        for k, v in enumerate(p):
            op[0].p[k] = v
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    def edit(k, v):
        i = list(good_i)
        i[k] = v
        return tuple(i)

    assert create(good_i, good_p)[0] == 0 and create(edit(11, L.F32), good_p)[0] == 0
    assert create((48, 256, 256, 1, 384, 0, 4, 1, 0, 1, 384, L.F32), good_p)[0] == 0          # 16 frames of 256 x 256 into MiDaS
    bad = [(edit(0, 0), good_p), (edit(1, 0), good_p), (edit(2, -3), good_p), (edit(4, 0), good_p), (edit(10, 0), good_p),      # sizes
           (edit(3, 3), good_p), (edit(3, 4), good_p), (edit(6, 7), good_p), (edit(6, 0), good_p),                              # channels, taps
           (edit(7, 0), good_p), (edit(7, 2), good_p), (edit(7, 3), good_p),                                                    # output form
           (edit(11, 2), good_p), (edit(11, -1), good_p),                                                                       # input dtype
           (good_i, (0, ptr, ptr, ptr)), (good_i, (ptr, 0, ptr, ptr)), (good_i, (ptr, ptr, 0, ptr)), (good_i, (ptr, ptr, ptr, 0)),
           ((1 << 14, 5, 7, 1, 1 << 10, 0, 4, 1, 0, 1, 300, L.F32), good_p)]                                                    # 2^14 x 2^10 rows x 2 tiles
    for i, p in bad:
        rc, msg = create(i, p)
        assert rc == -1 and b"bicubic" in msg, (i, p, rc, msg)
    rc, msg = create((1 << 14, 5, 7, 1, 1 << 10, 0, 4, 1, 0, 1, 300, L.F32), good_p)
    assert b"too many rows" in msg
    assert create((1 << 14, 5, 7, 1, 1 << 9, 0, 4, 1, 0, 1, 256, L.F32), good_p)[0] == 0     # one tile per row: 2^23 workgroups
    for mode in (2, -1):
        rc, msg = create(edit(9, mode), good_p)
        assert rc == -1 and b"i[9]" in msg, mode
    # the uint8 passes are validated as before: i[9] = 0 relaxes nothing
    assert create((2, 8, 12, 3, 20, 0, 7, 0, 3), (ptr, ptr, ptr, ptr, 0))[0] == 0
    rc, msg = create((2, 8, 12, 4, 20, 0, 7, 0, 3), (ptr, ptr, ptr, ptr, 0))
    assert rc == -1 and b"3 channels" in msg
    rc, msg = create((2, 8, 12, 1, 20, 0, 4, 1, 3), (ptr, ptr, ptr, ptr, ptr))
    assert rc == -1 and b"3 channels" in msg
    rc, msg = create((2, 8, 12, 3, 20, 0, 7, 3, 3), (ptr, ptr, ptr, ptr, 0))
    assert rc == -1 and b"output form" in msg


def test_bicubic_programs_pass_the_library_validation(built_lib):
    net = _small_adapter()
    comps = [net._compile(5, 32, 32, "f32", True, front_only=True, src_hw=(24, 24)), net._compile(16, 256, 256, "f16", True, front_only=True, src_hw=(384, 384)),
             VC._bicubic_compile(48, (256, 256), (384, 384), "f32"), VC._bicubic_compile(1, (4, 300), (3, 259), "f16")]
    for comp in comps:
        fake = {n: 0x40000000 + 0x1000000 * k for k, (n, _, _) in enumerate(comp.packer.recipes)}
        bound = BoundProgram(comp.prog, 0x10000000, fake, reset_sync=False)
        assert built_lib.t2v_plan_num_ops(bound.handle) == len(comp.prog.ops) and len(_bicubic_records(comp.prog)) == 1


# ---- the opt-in switch ----------------------------------------------------------------------------------------------------------------
def test_depth_resize_is_off_by_default():
    ld = VC.T2VAdapterDepth.__new__(VC.T2VAdapterDepth)
    torch.nn.Module.__init__(ld)
    assert getattr(ld, "depth_resize", None) is None
    ld.adapter = _small_adapter()
    seen = []

    def estimator(frames):
        seen.append(tuple(frames.shape))
        return torch.zeros(frames.shape[0], 1, 48, 48)
    ld.depth_stage_model = estimator
    videos = torch.zeros(1, 3, 2, 64, 48)
    for off in ("absent", None):
        if off is None:
            ld.depth_resize = None
        with pytest.raises(ValueError, match="must arrive at target_size"):
            ld.get_batch_depth(videos, (64, 48))
    assert seen == [(2, 3, 64, 48)] * 2                      # the estimator saw the frames at their own size
    # opted in: the frames go through the resize launch, which has no CPU fallback
    ld.depth_resize = (24, 24)
    with pytest.raises(L.T2VError, match="no CPU fallback"):
        ld.get_batch_depth(videos, (64, 48))
    assert len(seen) == 2


def test_bicubic_resize_argument_checks():
    with pytest.raises(L.T2VError, match="no CPU fallback"):
        VC.bicubic_resize(torch.zeros(1, 1, 4, 4), (8, 8))
    with pytest.raises(L.T2VError):
        VC.bicubic_resize(np.zeros((1, 1, 4, 4), np.float32), (8, 8))
    assert VC.T2VAdapterDepth.prepare_midas_input.__doc__ and "depth_resize" in VC.T2VAdapterDepth.__doc__
