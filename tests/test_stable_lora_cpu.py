"""CPU: Stable LoRA on the ModelScope path (sd-webui-text2video_amd/stable_lora.py, T2V_OP_LORA_MERGE).  `_merge_torch` — the executable
definition of the arithmetic contract, and the path of CPU models — against the digests that the reference's own `process_lora` left on the
reference's fp16 tiny UNet (tests/golden/stable_lora_tiny.npz: merge, undo, two files on one module) and against the numpy statement of the
contract (tests/stable_lora_ref.py); the all-or-nothing resolution; the state machine's call sequence against the reference's recorded one;
the op's host validation, its refusal in a plan, and the header / binding constants."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
from torch import nn

import stable_lora_ref as R
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import stable_lora as SL
from sd_webui_text2video_amd import unet as U

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FLAGS = dict(use_bias=True, use_time=True, use_conv=True, use_emb=True, use_linear=True)


@pytest.fixture(scope="module")
def gold():
    return R.golden()


def torch_file(f):
    return {k: torch.from_numpy(v.copy()) for k, v in f.items()}


@pytest.fixture()
def net16():
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    return net.half()


def digests(net, names):
    mods = dict(net.named_modules())
    return [R.digest(mods[n].weight.detach().numpy()) for n in names]


def merge(proc, net, files, alpha, undo=False, **flags):
    f = {**FLAGS, **flags}
    return proc.process_lora(net, files, f["use_bias"], f["use_time"], f["use_conv"], f["use_emb"], f["use_linear"], alpha, undo_merge=undo)


def test_merge_torch_reproduces_the_references_bytes(gold, net16):
    """Merge, undo, two files in one call: the bytes of every touched weight are the reference's; the Conv1d and the biased module's weight
    (the last two watched names) and that module's bias never move; the Parameters stay the same objects."""
    watched = gold["touched"] + gold["untouched"]
    f1, f2 = torch_file(gold["file1"]), torch_file(gold["file2"])
    mods = dict(net16.named_modules())
    ids = [id(mods[n].weight) for n in watched]
    bias0 = R.digest(mods[gold["untouched"][1]].bias.detach().numpy())
    assert digests(net16, watched) == gold["sha_original"]
    proc = SL.StableLoraProcessor()
    touched = merge(proc, net16, [f1], gold["alpha"])
    assert touched == [n + ".weight" for n in gold["touched"]]
    assert digests(net16, watched) == gold["sha_merged"]
    assert gold["sha_merged"][-2:] == gold["sha_original"][-2:] and all(a != b for a, b in zip(gold["sha_merged"][:-2], gold["sha_original"]))
    merge(proc, net16, [f1], gold["alpha"], undo=True)
    assert digests(net16, watched) == gold["sha_undone"]
    merge(proc, net16, [f1, f2], gold["alpha"])
    assert digests(net16, watched) == gold["sha_two_files"]
    assert [id(mods[n].weight) for n in watched] == ids
    assert R.digest(mods[gold["untouched"][1]].bias.detach().numpy()) == bias0
    assert float(gold["separation_over_gate"]) >= 100          # the file matters: merged and un-merged eps are >= 100 gates apart


def test_class_switches_follow_the_reference(gold, net16):
    """use_linear / use_conv / use_time select the classes: with a class off its weights keep their bytes."""
    f1 = torch_file(gold["file1"])
    mods = dict(net16.named_modules())
    for flags, moved in ((dict(use_linear=False), (nn.Conv2d, nn.Conv3d)), (dict(use_conv=False), (nn.Linear,)), (dict(use_time=False), (nn.Linear, nn.Conv2d))):
        before = digests(net16, gold["touched"])
        touched = merge(SL.StableLoraProcessor(), net16, [f1], 0.5, **flags)
        after = digests(net16, gold["touched"])
        for n, a, b in zip(gold["touched"], before, after):
            assert (a != b) == isinstance(mods[n], moved) == (n + ".weight" in touched), (flags, n)


@pytest.mark.parametrize("shape,r,form", [((6, 10), 3, R.DIRECT), ((1, 1), 1, R.DIRECT), ((8, 33), 64, R.DIRECT), ((4, 3, 3, 3), 2, R.DIRECT),
                                         ((5, 7, 3, 1, 1), 4, R.TEMPORAL), ((16, 16, 3, 1, 1), 1, R.TEMPORAL)])
def test_numpy_contract_equals_merge_torch_bit_for_bit(shape, r, form):
    rng = np.random.default_rng(len(shape) * 100 + r)
    N, J = shape[0], int(np.prod(shape[1:]))
    W = rng.standard_normal(shape).astype(np.float16)
    A = rng.standard_normal((r, J * (3 if form == R.TEMPORAL else 1))).astype(np.float16)
    B = rng.standard_normal((N, r)).astype(np.float16)
    A[:, J // 2] *= 37.0                                      # one large column, one zero row: a shifted index moves the result
    B[N // 2, :] = 0
    for alpha in (0.7, -0.7, 1.0, 0.05):
        w = torch.from_numpy(W.copy())
        SL._merge_torch(w, torch.from_numpy(A), torch.from_numpy(B), alpha, form)
        want = R.merge_f16(W, A, B, alpha, form)
        assert w.numpy().tobytes() == want.tobytes(), alpha
        # and the fp32 path against the float64 evaluation, inside the bound the kernel's test uses
        w32 = torch.from_numpy(W.astype(np.float32))
        SL._merge_torch(w32, torch.from_numpy(A.astype(np.float32)), torch.from_numpy(B.astype(np.float32)), alpha, form)
        w_star, S = R.merge_f64(W.astype(np.float32), A.astype(np.float32), B.astype(np.float32), alpha, form)
        assert np.all(np.abs(w32.numpy().astype(np.float64) - w_star) <= R.f32_bound(w_star, S, alpha, r))


def test_nothing_changes_when_any_key_fails(gold, net16):
    f1 = torch_file(gold["file1"])
    first = gold["touched"][0]
    free = next(n for n, m in net16.named_modules() if isinstance(m, nn.Linear) and m.bias is None)
    bad_files = []
    missing = dict(f1)
    missing["middle_block.0.in_layers.2.lora_A"] = torch.zeros(4, 9)          # a matched module, no lora_B
    bad_files.append((missing, "no partner"))
    misfit = dict(f1)
    last = gold["touched"][-3]
    misfit[last + ".lora_A"] = misfit.pop(last + ".lora_A")[:, :-1].contiguous()   # moved to the end of the file, one column short
    bad_files.append((misfit, "do not fit"))
    bias = dict(f1)
    bias[free + ".bias"] = torch.zeros(1)
    bad_files.append((bias, "no slot"))
    before = {k: R.digest(v.numpy()) for k, v in net16.state_dict().items()}
    for f, needle in bad_files:
        with pytest.raises(L.T2VError, match=needle):
            merge(SL.StableLoraProcessor(), net16, [f1, f], 0.7)
        assert {k: R.digest(v.numpy()) for k, v in net16.state_dict().items()} == before, needle
    # the bias key for a bias-free module is only judged under use_bias, and keys of other models are not ours to judge
    other = dict(f1)
    other["transformer.resblocks.0.mlp.c_fc.lora_A"] = torch.zeros(4, 8)
    assert merge(SL.StableLoraProcessor(), net16, [bias, other], 0.7, use_bias=False)
    assert R.digest(dict(net16.named_modules())[first].weight.detach().numpy()) != before[first + ".weight"]
    # a weight that is not contiguous, and two targets that share memory
    lin = nn.Module()
    lin.a, lin.b = nn.Linear(4, 4, bias=False), nn.Linear(4, 4, bias=False)
    lin.b.weight = lin.a.weight
    fac = {f"{n}.lora_{x}": torch.ones(4, 1) if x == "B" else torch.ones(1, 4) for n in "ab" for x in "AB"}
    with pytest.raises(L.T2VError, match="overlap"):
        merge(SL.StableLoraProcessor(), lin, [fac], 1.0)
    lin.b.weight = nn.Parameter(torch.zeros(4, 8)[:, ::2])
    with pytest.raises(L.T2VError, match="not contiguous"):
        merge(SL.StableLoraProcessor(), lin, [fac], 1.0)
    assert torch.equal(lin.b.weight, torch.zeros(4, 4))


def test_process_emits_the_references_call_sequence(gold, tmp_path):
    """first load, alpha change, second file added, option toggled, selection emptied: the (model, files, flags, alpha, undo) calls and
    the `lora_loaded` state after every step are the ones the reference's own StableLoraScript.process produced."""
    from safetensors.torch import save_file
    for tag in ("f1", "f2"):
        save_file({"tag." + tag: torch.zeros(1)}, str(tmp_path / (tag + ".safetensors")), metadata={"stable_lora_text_to_video": "1"})
    save_file({"tag.f3": torch.zeros(1)}, str(tmp_path / "f3.safetensors"))                       # no metadata: not a Stable LoRA file
    assert SL.get_lora_files(str(tmp_path))[1] == ["f1", "f2"]
    pipe = types.SimpleNamespace(sd_model=nn.Linear(2, 2), clip_encoder=types.SimpleNamespace(model=types.SimpleNamespace(transformer=nn.Linear(3, 3))))
    script = SL.StableLoraScript()
    script.log = lambda *a, **k: None
    calls = []

    def recorder(model, lora_files_list, use_bias, use_time, use_conv, use_emb, use_linear, lora_alpha, undo_merge=False):
        calls.append(dict(step=step, model="sd_model" if model is pipe.sd_model else "transformer",
                          files=[k.split(".")[1] for f in lora_files_list for k in f if k.startswith("tag.")],
                          flags=[bool(use_bias), bool(use_time), bool(use_conv), bool(use_emb), bool(use_linear)],
                          alpha=float(lora_alpha), undo=bool(undo_merge)))
    script.process_lora = recorder
    rec = gold["call_sequence"]
    loaded = []
    for step, args in enumerate(rec["scenario"]):
        script.process(pipe, *args, lora_dir=str(tmp_path))
        loaded.append(script.is_lora_loaded(pipe.sd_model))
    assert loaded == rec["loaded_after"]
    assert calls == rec["calls"]
    assert len(calls) == 15 and {c["step"] for c in calls} == {0, 1, 2, 3, 4}
    with pytest.raises(L.T2VError, match="not found"):
        script.process(pipe, ["nowhere"], 1.0, True, True, True, True, 1, True)


def test_process_modelscope_routes_the_settings(monkeypatch):
    """`stable_lora` in args_dict, or an eight-element extra_args, reaches StableLoraScript.process before sampling; neither: nothing runs."""
    from sd_webui_text2video_amd import pipeline as P
    seen = []
    monkeypatch.setattr(SL.StableLoraScript, "process", lambda self, pipe, *a, **k: seen.append((a, k)))
    pipe = types.SimpleNamespace(device="cpu", infer_conditioned=lambda *a, **k: ("frames", None))
    args = dict(pipe=pipe, cond=torch.zeros(1), uncond=torch.zeros(1), steps=1, frames=1, seed=0, cfg_scale=1.0)
    assert P.process_modelscope(dict(args)) == "frames" and seen == []
    P.process_modelscope(dict(args, stable_lora=dict(lora_files_selection=["x"], lora_alpha=0.5, use_time=False)))
    assert seen[-1][1] == dict(lora_files_selection=["x"], lora_alpha=0.5, use_bias=True, use_linear=True, use_conv=True, use_emb=True,
                               use_multiplier=1, use_time=False, lora_dir=None)
    P.process_modelscope(dict(args), extra_args=[["y"], 0.25, True, False, True, True, 2, True])
    assert seen[-1][1] == dict(lora_files_selection=["y"], lora_alpha=0.25, use_bias=True, use_linear=False, use_conv=True, use_emb=True,
                               use_multiplier=2, use_time=True, lora_dir=None)
    assert len(seen) == 2 and isinstance(pipe._stable_lora_script, SL.StableLoraScript)
    with pytest.raises(L.T2VError, match="unknown"):
        P.process_modelscope(dict(args, stable_lora=dict(alpha=1)))


def test_tile_table_covers_every_tile_once():
    T = L.LORA_TILE
    assert SL.tile_table([1, T - 1, T, T + 1, 3 * T]).tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]]


def test_record_validation_without_gpu(built_lib):
    """The record is checked before any HIP call, and a plan refuses the kind: it is a stand-alone op."""
    ptr = 0x1000

    def rec(i, p):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_LORA_MERGE
        for k, v in enumerate(i):
            op[0].i[k] = v
        for k, v in enumerate(p):
            op[0].p[k] = v
        op[0].f[0] = 1.0
        return op

    for i, p, needle in (((0, 1), (ptr, ptr), b"n segments > 0"), ((4, 3), (ptr, ptr), b"at least one tile per segment"), ((1, 1), (0, ptr), b"null lora merge pointer"),
                         ((1, 1), (ptr, 0), b"null lora merge pointer"), ((1, 1), (ptr, ptr + 4), b"8-byte aligned"), ((1, 1), (ptr + 2, ptr), b"8-byte aligned")):
        assert built_lib.t2v_run_ops(rec(i, p), 1, None, 0, None) == -1, (i, p)
        assert needle in built_lib.t2v_last_error() and b"lora merge" in built_lib.t2v_last_error(), (i, p)
    h = ctypes.c_void_p()
    assert built_lib.t2v_plan_create(rec((1, 1), (ptr, ptr)), 1, ctypes.byref(h)) == -1
    assert b"lora merge: a stand-alone op" in built_lib.t2v_last_error()


def test_header_and_binding_constants_agree():
    header = open(os.path.join(ROOT, "include", "t2v_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(T2V_\w+)\s+\(?(-?\d+)\)?", header)}
    enums = {k: int(v) for k, v in re.findall(r"(T2V_\w+)\s*=\s*(\d+)", header)}
    assert enums["T2V_OP_LORA_MERGE"] == L.OP_LORA_MERGE == 26 and enums["T2V_OP_KIND_MAX"] == L.OP_KIND_MAX == 27
    assert defs["T2V_LORA_TILE"] == L.LORA_TILE and defs["T2V_LORA_DIRECT"] == L.LORA_DIRECT == R.DIRECT
    assert defs["T2V_LORA_TEMPORAL"] == L.LORA_TEMPORAL == R.TEMPORAL
    assert defs["T2V_ABI_VERSION"] == L.ABI_VERSION == 11                   # additive: the version does not move
    assert SL._SEG_DTYPE.itemsize == 48
