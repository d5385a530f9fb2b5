"""GPU (-m gpu): the halo A staging of the stride-1 3x3 convolutions (csrc/gemm2.hip gemm2_halo_kernel) against the per-tap staging of
gemm2_kernel, record by record.

Every case holds the SAME convolution twice in one program — same input, same weights, separate outputs (and separate split-K slabs): the
first record takes the path the launcher chooses (the halo staging wherever csrc/gemm2.hip conv_halo_eligible admits the record), the
second carries i[31] = 1, a word no validation reads, which forces the per-tap staging.  The two keep the k order, so every accumulator is
the same sum in the same order: the tests assert that EVERY output byte is equal (and every slab byte of a split-K record, every byte of
the normalised image of a fused GroupNorm), no tolerance.  The per-tap path is what tests/test_gpu_ops.py and tests/test_gpu_gemm_adversarial.py
pin against the CPU interpreter and float64.

Inputs are N(0, 1) between two NaN allocations (a halo row taken from outside the input, or a padding tap that is not masked, turns the
output NaN on one side only — and NaN bytes are compared like any others); the weights carry a distinct scale per tap (1, 2, 4 .. 256 — exact
in fp16), so that a wrong tap or a wrong shift cannot cancel.

A record's M must be a whole number of images (executor.hip: "M not a multiple of Hout*Wout"), so "rows past M" are the rows of a partial
last tile: 16x16 x 5 images = 1280 rows on the 192-row tile.

That the halo instantiations are the kernels that ran is shown by the kernel trace in profiles/conv_halo.txt."""
import math
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":      # the child process of the last test: the paths tests/conftest.py sets up
    sys.path[:0] = [os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), os.path.dirname(os.path.abspath(__file__))]

from interp import Interp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd.program import BoundProgram, Program, Ref

pytestmark = pytest.mark.gpu

TAP_SCALE = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0]).view(1, 1, 3, 3)
TILE_BN = {1: 256, 3: 256, 5: 128, 8: 320, 9: 256, 11: 320}


def build(tile, B, H, W, Cin, N, *, split=1, gn=False, seed=0):
    """-> (program, weights, init, [(what, halo-path buffer, forced-per-tap buffer)]).  split > 1: that many splits, each record with slabs
    of its own; gn: a per-frame GroupNorm (+SiLU) that becomes the convolution's epilogue."""
    P = Program()
    P.force_tile = tile
    g = torch.Generator().manual_seed(seed)
    M = B * H * W
    fence_lo, a, fence_hi = P.alloc(96, Cin, "f16"), P.alloc(M, Cin, "f16"), P.alloc(96, Cin, "f16")
    wt = torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin) / 64.0 * TAP_SCALE
    w = {"w": pk.conv3x3(wt).half(), "b": torch.randn(N, generator=g)}
    if gn:
        w["g"], w["be"] = torch.randn(N, generator=g), torch.randn(N, generator=g)
        w["gb"] = torch.cat([w["g"], w["be"]])
    pairs = []
    bufs = []
    for legacy in (0, 1):
        out = P.alloc(M, N, "f32")
        ws = P.alloc(split * M, N, "f32") if split > 1 else None
        nout = P.alloc(M, N, "f16") if gn else None
        op = P.gemm(f"conv{legacy}", a, Ref("weight", 0, "w"), N, 9 * Cin, out, bias=Ref("weight", 0, "b"), gather=L.GATHER_CONV3X3,
                    conv=dict(Hin=H, Win=W, Cin=Cin, stride=1, up=0, Hout=H, Wout=W), allow_splitk=False)
        assert op.i[22] == tile and op.i[19] == 1 and op.i[31] == 0
        if split > 1:
            op.i[19], op.p[6], op.meta["split"] = split, ws.ref, split
        if gn:
            fused = P.groupnorm(f"gn{legacy}", out, Ref("weight", 0, "g"), Ref("weight", 0, "be"), nout, n_inst=B, eps=1e-5, silu=True,
                                gb=Ref("weight", 0, "gb"))
            assert fused is op and op.i[16] == L.EPI_GN, "the norm did not become the convolution's epilogue"
        op.i[31] = legacy
        bufs.append((out, ws, nout))
    pairs.append(("output", bufs[0][0], bufs[1][0]))
    if split > 1:
        pairs.append(("split-K slabs", bufs[0][1], bufs[1][1]))
    if gn:
        pairs.append(("normalised output", bufs[0][2], bufs[1][2]))

    def init(it):
        for f in (fence_lo, fence_hi):
            it.mat(f.ref, f.rows, f.cols, f.ld, torch.float16, {}).fill_(float("nan"))
        it.mat(a.ref, a.rows, a.cols, a.ld, torch.float16, {}).copy_(torch.randn(M, Cin, generator=g).half())
    return P, w, init, pairs


def run_and_compare(P, w, init, pairs, what):
    it = Interp(P, w, poison=False)
    init(it)
    dev = torch.device("cuda:0")
    arena = it.arena.to(dev)
    wd = {k: v.to(dev).contiguous() for k, v in w.items()}
    bp = BoundProgram(P, arena.data_ptr(), {k: v.data_ptr() for k, v in wd.items()})
    bp.run({}, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    L.async_status()
    it.arena = arena.cpu()
    for name, x, y in pairs:
        dt = torch.float16 if x.dtype == "f16" else torch.float32
        bx = it.mat(x.ref, x.rows, x.cols, x.ld, dt, {}).contiguous().view(torch.uint8)
        by = it.mat(y.ref, y.rows, y.cols, y.ld, dt, {}).contiguous().view(torch.uint8)
        diff = int((bx != by).sum())
        assert diff == 0, f"{what}: {name}: {diff} of {bx.numel()} bytes differ between the halo and the per-tap staging"
        if name != "split-K slabs":
            v = it.mat(y.ref, y.rows, y.cols, y.ld, dt, {}).float()
            assert torch.isfinite(v).all() and float(v.abs().max()) > 0.0, f"{what}: {name} of the per-tap path is not a finite, non-zero tensor"


# W, H, images, tile: eight 4x4 images per 128-row tile (top and bottom halos cross images); 32x32 on the 192-row tile (interior tiles whose
# halo is live data, a partial last tile); 32x3 (the widest halo); 5x3 and 1x7 (column masks, a width that is no power of two); 16x16 x 5
# images on the 192-row tile (rows of the last tile past M)
GEOMETRY = [(4, 4, 24, 5), (32, 32, 1, 8), (32, 3, 3, 5), (5, 3, 11, 5), (1, 7, 23, 5), (16, 16, 5, 8)]


@pytest.mark.parametrize("W,H,B,tile", GEOMETRY)
def test_geometry(W, H, B, tile):
    run_and_compare(*build(tile, B, H, W, 128, TILE_BN[tile], seed=1), f"{W}x{H} x {B} tile {tile}")


@pytest.mark.parametrize("Cin", [64, 128, 192, 320])
def test_channel_chunks(Cin):
    """One chunk; the buffer swap; an odd count; the deployed count."""
    run_and_compare(*build(8, 3, 9, 16, Cin, 320, seed=2), f"Cin {Cin}")


@pytest.mark.parametrize("split", [2, 3])
def test_split_k(split):
    """Cin = 128 is 18 k-tiles: two splits of 9 start on a chunk boundary (halo staging); three splits of 6 do not — the launcher must
    take the per-tap staging for them, and the two records are equal either way.  The slabs are compared too."""
    run_and_compare(*build(5, 3, 8, 8, 128, 128, split=split, seed=3), f"split-K {split}")


@pytest.mark.parametrize("tile", sorted(TILE_BN))
def test_every_instantiated_tile(tile):
    run_and_compare(*build(tile, 3, 20, 16, 128, TILE_BN[tile], seed=4), f"tile {tile}")


@pytest.mark.parametrize("tile", [t for t in sorted(TILE_BN) if L.GEMM_TILES[t].has(L.TILE_GN)])
def test_fused_groupnorm(tile):
    """Per-frame GroupNorm in the epilogue, a grid of one round: 4 frames of 16x16 (256 rows per instance)."""
    run_and_compare(*build(tile, 4, 16, 16, 64, TILE_BN[tile], gn=True, seed=5), f"fused GroupNorm tile {tile}")


def test_switch_in_a_child_process():
    """T2V_CONV_HALO=0: the whole process on the per-tap staging; the first geometry case still runs and is equal."""
    env = dict(os.environ, T2V_CONV_HALO="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "CONVHALO-CHILD equal under T2V_CONV_HALO=0" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    W_, H_, B_, tile_ = GEOMETRY[0]
    run_and_compare(*build(tile_, B_, H_, W_, 128, TILE_BN[tile_], seed=1), "child")
    print(f"CONVHALO-CHILD equal under T2V_CONV_HALO={os.environ.get('T2V_CONV_HALO')}")
