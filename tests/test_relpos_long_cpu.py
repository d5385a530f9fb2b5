"""CPU: VideoCrafter clips longer than 32 frames — kernel selection of the relative-position attention (RELPOS_ATTN i[17] = 3
beyond 32 frames), the table packing of the long-clip kernel, the tiny LVDM UNet at 40 frames lowered and run in the CPU
interpreter against the reference (tests/golden/make_golden_long.py), and its T-sharded form over gloo."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from harness import rel_l2
from interp import Interp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd import parallel
from sd_webui_text2video_amd import videocrafter as VC
from sd_webui_text2video_amd.program import Program, Ref, TShardSpec

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HEADER = open(os.path.join(os.path.dirname(__file__), "..", "include", "t2v_hip.h")).read()


def _relpos_op(nk, relpos_mfma, nq=None, q_offset=0, tables_long=True, R=16, D=40):
    nq = nk if nq is None else nq
    P = Program()
    q, kv, o = P.alloc(nq * 4, 2 * D, "f16"), P.alloc(nk * 4, 4 * D, "f16"), P.alloc(nq * 4, 2 * D, "f16")
    extra = dict(rel_k16=Ref("weight", 0, "ek16"), rel_vT16=Ref("weight", 0, "ev16"))
    if tables_long:
        extra.update(rel_k_long=Ref("weight", 0, "ekL"), rel_vT_long=Ref("weight", 0, "evL"))
    return P.attention("a", q.ref, kv.col_slice(0, 2 * D).ref, kv.col_slice(2 * D, 4 * D).ref, o.ref, nq=nq, nk=nk, heads=2,
                       b_outer=1, b_inner=4, q_strides=(8 * D, 0, 2 * D), kv_strides=(16 * D, 0, 4 * D), o_strides=(8 * D, 0, 2 * D),
                       scale=D ** -0.5, head_dim=D, rel_k=Ref("weight", 0, "ek"), rel_v=Ref("weight", 0, "ev"), max_rel=R,
                       q_offset=q_offset, relpos_mfma=relpos_mfma, **extra)


@pytest.mark.parametrize("nk", [33, 48, 250])
@pytest.mark.parametrize("sel", [None, 0, 1, 2])
def test_long_clips_select_the_long_kernel(nk, sel):
    op = _relpos_op(nk, sel)
    assert op.kind == L.OP_RELPOS_ATTN and op.i[17] == 3
    assert op.p[6] == Ref("weight", 0, "ekL") and op.p[7] == Ref("weight", 0, "evL")
    # T-sharded slice of a long clip (temporal_attn_sharded: nk = all frames)
    op = _relpos_op(nk, sel, nq=nk // 3, q_offset=nk // 3)
    assert op.i[17] == 3 and op.i[16] == nk // 3


@pytest.mark.parametrize("sel,nk,want", [(None, 16, 2), (None, 24, 0), (None, 32, 0), (0, 16, 0), (1, 16, 1), (1, 32, 1),
                                         (2, 16, 2), (2, 17, 0), (3, 24, 3), (3, 8, 3)])
def test_up_to_32_frames_keeps_todays_selection(sel, nk, want):
    """<= 32 frames: 0 / 1 / 2 exactly as before; 3 only when asked for (the A/B switch) and the long tables are given."""
    assert _relpos_op(nk, sel).i[17] == want
    assert _relpos_op(nk, 3, tables_long=False).i[17] == 0


def test_beyond_the_kernel_bound_raises():
    bound = L.RELPOS_MAX_FRAMES
    assert _relpos_op(bound, None).i[17] == 3
    with pytest.raises(ValueError, match=str(bound)):
        _relpos_op(bound + 1, None)
    with pytest.raises(ValueError, match="40 frames"):
        _relpos_op(40, None, tables_long=False)


def test_header_bounds_match_binding():
    defs = dict(re.findall(r"#define\s+(T2V_RELPOS_\w+)\s+(\d+)", HEADER))
    assert int(defs["T2V_RELPOS_MAX_FRAMES"]) == L.RELPOS_MAX_FRAMES
    assert int(defs["T2V_RELPOS_LONG_PADL"]) == L.RELPOS_LONG_PADL == pk.RELPOS_LONG_PADL
    m = re.search(r"#define\s+T2V_RELPOS_LONG_COLS\(R\)\s+\(\(2 \* \(R\) \+ (\d+)\) / 8 \* 8\)", HEADER)
    assert m is not None
    for R in range(0, 300, 7):
        assert pk.relpos_long_cols(R) == (2 * R + int(m.group(1))) // 8 * 8


@pytest.mark.parametrize("R,d", [(0, 40), (2, 64), (16, 40), (16, 80), (16, 160), (249, 40)])
def test_relpos_table_long_packing(R, d):
    tab = torch.randn(2 * R + 1, d, generator=torch.Generator().manual_seed(R + d))
    ek = pk.relpos_table_long(tab, False)
    DK, DV = (d + 15) // 16 * 16, (d + 31) // 32 * 32
    assert ek.dtype == torch.float16 and ek.shape == (2 * R + 1, DK)
    assert torch.equal(ek[:, :d], tab.half()) and not ek[:, d:].any()
    evt = pk.relpos_table_long(tab, True)
    nc = pk.relpos_long_cols(R)
    assert evt.dtype == torch.float16 and evt.shape == (DV, nc) and nc % 8 == 0
    # every window the kernel reads: aligned base >= 0, 80 columns, for table-row offsets jb in [-61, 2R - 1]
    assert (-61 + pk.RELPOS_LONG_PADL) // 8 * 8 >= 0 and (2 * R - 1 + pk.RELPOS_LONG_PADL) // 8 * 8 + 80 <= nc
    for c in range(nc):
        j = min(max(c - pk.RELPOS_LONG_PADL, 0), 2 * R)
        assert torch.equal(evt[:d, c], tab[j].half()), c
    assert not evt[d:].any()


def _inputs_tiny40():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 40, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 40, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def test_tiny_unet_40_frames_in_interpreter_matches_reference_golden():
    net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    x, t, ctx, _ = _inputs_tiny40()
    comp = net._compile(2, 40, 8, 8, 9, "f32", "f32", "f32")
    rel = [op for op in comp.prog.ops if op.kind == L.OP_RELPOS_ATTN]
    assert rel and all(op.i[1] == 40 and op.i[17] == 3 for op in rel)
    out = torch.empty(2, 4, 40, 8, 8)
    Interp(comp.prog, comp.packer.materialise(net.state_dict(), "cpu")).run({L.EXT_X: x, L.EXT_T: t.float(), L.EXT_CTX: ctx, L.EXT_OUT: out})
    gold = torch.from_numpy(np.load(os.path.join(GOLD, "lvdm_tiny_40f.npz"))["unet_eps"])
    r = rel_l2(out, gold)
    assert r < 4e-3, r


# ---- T-sharded tiny LVDM at 40 frames over gloo (as test_tshard_cpu.py:_lvdm_worker) --------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Seg:
    def __init__(self, it, ops):
        self.it, self.ops = it, ops

    def run(self, ext, stream):
        self.it.run(ext, ops=self.ops)


def _lvdm_inputs(F):
    g = torch.Generator().manual_seed(31)
    return torch.randn(1, 4, F, 8, 8, generator=g), torch.tensor([431.0]), torch.randn(1, 9, 768, generator=g)


def _lvdm_worker(rank, world, port, F, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
        net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
        x, t, ctx = _lvdm_inputs(F)
        spec = TShardSpec.make(F, world, rank)
        shard = parallel.TShard(dist.group.WORLD, list(range(world)), spec)
        comp = net._compile(1, spec.frames, 8, 8, 9, "f32", "f32", "f32", shard=spec)
        rel = [op for op in comp.prog.ops if op.kind == L.OP_RELPOS_ATTN]
        assert rel and all(op.i[0] == spec.frames and op.i[1] == F and op.i[16] == spec.offset and op.i[17] == 3 for op in rel)
        it = Interp(comp.prog, comp.packer.materialise(net.state_dict(), "cpu"))
        ex = parallel.ShardedExecutor(comp.prog, it.arena, shard, lambda ops: _Seg(it, ops))
        out = torch.empty(1, 4, spec.frames, 8, 8)
        ex.run({L.EXT_X: x[:, :, spec.offset:spec.offset + spec.frames].contiguous(), L.EXT_T: t, L.EXT_CTX: ctx, L.EXT_OUT: out}, None)
        ret[rank] = (spec.frames, spec.offset, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,frames", [(2, [20, 20]), (3, [14, 14, 12])])
def test_tsharded_lvdm_40_frames_matches_unsharded_gloo(world, frames):
    F = 40
    port = _free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_lvdm_worker, args=(world, port, F, ret), nprocs=world, join=True)
    assert [ret[r][0] for r in range(world)] == frames
    assert [ret[r][1] for r in range(world)] == [sum(frames[:r]) for r in range(world)]
    sharded = torch.cat([ret[r][2] for r in range(world)], dim=2)
    net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    sd = synth.synth_state_dict(synth.param_spec(net), seed=0)
    x, t, ctx = _lvdm_inputs(F)
    ref = tp.lvdm_unet_forward(sd, configs.TINY_LVDM_UNET, x, t, ctx)
    assert not torch.isnan(sharded).any()
    assert rel_l2(sharded, ref) < 5e-3
    for f in range(F):
        assert rel_l2(sharded[:, :, f], ref[:, :, f]) < 7e-3, f
