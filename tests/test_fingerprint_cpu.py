"""CPU: the byte-level fingerprint of the parameters (T2V_OP_FINGERPRINT, packing.ParamFingerprint) — what the function exposes, on its
torch implementation (the reference of the kernel's tests, tests/test_gpu_fingerprint.py), and `verify_weights` on the tiny LVDM model
with a CPU pack: an edit through `.data`, which moves neither the parameter's identity nor its version, is found by its bytes."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd import videocrafter as VC

M64 = (1 << 64) - 1


def definition(raw: bytes) -> int:
    """The definition, word by word in Python integers (include/t2v_hip.h, FINGERPRINT)."""
    w = np.frombuffer(raw, dtype="<u2")
    total = (len(w) + 1) * pk.FINGERPRINT_LEN
    for j, v in enumerate(w.tolist()):
        total += v * (2 * j + 1) + ((v * v) << 32)
    return total & M64


def fp_bytes(raw: bytes) -> int:
    return pk.fingerprint_torch(torch.frombuffer(bytearray(raw), dtype=torch.uint8)) if raw else pk.fingerprint_torch(torch.zeros(0, dtype=torch.uint8))


def _segment(seed=0, nbytes=64):
    return bytes(np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tolist())


def test_torch_implementation_is_the_definition():
    for nbytes in (0, 2, 4, 14, 16, 18, 64, 1000, 70002):
        raw = _segment(nbytes, nbytes)
        assert fp_bytes(raw) == definition(raw), nbytes
    # all-ones words over more than one piece of the implementation's fold (sums far beyond 2^64): closed form
    n = (1 << 21) + 3
    t = torch.full((n,), -1, dtype=torch.int16)
    assert pk.fingerprint_torch(t) == (65535 * n * n + ((65535 * 65535 * n) << 32) + (n + 1) * pk.FINGERPRINT_LEN) & M64
    assert pk.FINGERPRINT_LEN == L.FINGERPRINT_LEN and pk.FINGERPRINT_CHUNK == L.FINGERPRINT_CHUNK


def test_every_single_bit_flip_changes_its_segment_and_no_other():
    segs = [bytearray(_segment(s)) for s in range(3)]
    base = [fp_bytes(bytes(s)) for s in segs]
    assert len(set(base)) == 3
    for bit in range(64 * 8):
        segs[1][bit // 8] ^= 1 << (bit % 8)
        now = [fp_bytes(bytes(s)) for s in segs]
        segs[1][bit // 8] ^= 1 << (bit % 8)
        assert now[1] != base[1] and now[0] == base[0] and now[2] == base[2], bit


def test_a_swap_of_two_unequal_elements_changes_the_value():
    raw = bytearray(_segment(5))
    base = fp_bytes(bytes(raw))
    w = np.frombuffer(bytes(raw), dtype="<u2")
    for j, k in ((0, 1), (0, 31), (7, 8), (15, 16), (3, 29)):
        assert w[j] != w[k]
        s = w.copy()
        s[j], s[k] = w[k], w[j]
        assert fp_bytes(s.tobytes()) != base, (j, k)
    # fp32 elements (two words each) swapped, and the two halves of one element
    f = np.frombuffer(bytes(raw), dtype="<f4").copy()
    f[[2, 9]] = f[[9, 2]]
    assert fp_bytes(f.tobytes()) != base


def test_equal_bytes_of_different_lengths_differ():
    raw = _segment(6, 32)
    vals = {fp_bytes(raw + b"\0" * pad) for pad in (0, 2, 4, 16, 32)}
    assert len(vals) == 5
    assert len({fp_bytes(b"\0" * n) for n in (0, 2, 4, 64)}) == 4


def test_value_does_not_depend_on_the_start_alignment():
    raw = _segment(7, 70)
    want = definition(raw)
    for off in range(0, 16, 2):
        buf = torch.zeros(16 + 128, dtype=torch.uint8)
        base = (-buf.data_ptr()) % 16 + off                 # `off` bytes past a 16-byte boundary
        buf[base:base + 70] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        view = buf[base:base + 70]
        assert view.data_ptr() % 16 == off
        assert pk.fingerprint_torch(view) == want, off


def test_chunk_table_covers_every_chunk_once_and_keeps_empty_segments():
    C = pk.FINGERPRINT_CHUNK
    sizes = [0, 2, C - 2, C, C + 2, 3 * C + 6]
    tab = pk.ParamFingerprint.chunk_table(sizes)
    assert tab == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (5, 0), (5, 1), (5, 2), (5, 3)]


def test_record_validation_without_gpu(built_lib):
    """The record is checked before any HIP call, and a plan refuses the kind: it is a stand-alone op."""
    ptr = 0x1000

    def rec(i, p):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_FINGERPRINT
        for k, v in enumerate(i):
            op[0].i[k] = v
        for k, v in enumerate(p):
            op[0].p[k] = v
        return op

    for i, p, needle in (((0, 1), (ptr, ptr, ptr), b"fingerprint"), ((4, 3), (ptr, ptr, ptr), b"fingerprint"), ((1, 1), (ptr, 0, ptr), b"fingerprint"),
                         ((1, 1), (ptr, ptr + 4, ptr), b"8-byte")):
        assert built_lib.t2v_run_ops(rec(i, p), 1, None, 0, None) == -1 and needle in built_lib.t2v_last_error(), (i, p)
    h = ctypes.c_void_p()
    assert built_lib.t2v_plan_create(rec((1, 1), (ptr, ptr, ptr)), 1, ctypes.byref(h)) == -1 and b"stand-alone" in built_lib.t2v_last_error()
    assert L.OP_FINGERPRINT == 25


@pytest.fixture()
def tiny():
    net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    return net


def test_verify_weights_finds_a_data_edit_and_repacks_only_its_dependents(tiny):
    net = tiny
    assert net.verify_weights("cpu") == []                      # nothing packed yet: nothing to do
    net.refresh_weights("cpu")
    assert net.last_repack == -1
    n_images = len(net._packed)
    ptrs = {k: v.data_ptr() for k, v in net._packed.items()}
    assert net.verify_weights("cpu") == [] and net.last_repack == -1
    name = "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"
    w = dict(net.named_parameters())[name]
    version = w._version
    g = torch.Generator().manual_seed(1)
    w.data += 0.01 * torch.randn(w.shape, generator=g)          # the reference's way (lora.py:666)
    assert w._version == version
    net.refresh_weights("cpu")
    assert net.last_repack == -1                                # the signature check is blind to it
    for c in net._programs.values():
        c.ctx_token = "cached"
    assert net.verify_weights("cpu") == [name]
    assert 0 < net.last_repack < n_images // 2, (net.last_repack, n_images)
    assert {k: v.data_ptr() for k, v in net._packed.items()} == ptrs
    assert all(c.ctx_token is None for c in net._programs.values())       # the partial path's invalidations apply
    rewritten = [k for k, d in net._packed_deps.items() if name in d]
    assert len(rewritten) == net.last_repack and any(k.startswith("kv_all") for k in rewritten)     # the concatenated K/V image reads it
    full = net._get_compiled_any().packer.materialise(net.state_dict(), "cpu")
    assert full.keys() == net._packed.keys()
    for k in full:
        assert torch.equal(full[k], net._packed[k]), k
    assert net.verify_weights("cpu") == []                      # recorded at the end of the partial pack
    # `.data = other` (the v2 removal of the reference): new storage, same parameter object, same version
    w.data = w.data.clone() * 1.5
    assert net.verify_weights("cpu") == [name] and net.verify_weights("cpu") == []


def test_verify_weights_skips_cpu_parameters_beside_a_gpu_pack(tiny):
    """Parameters on the CPU while the pack is on a GPU are not fingerprinted (INTEGRATION): compute() says so with None."""
    fp = pk.ParamFingerprint()
    assert fp.compute(list(tiny.named_parameters())[:3], torch.device("cuda:0")) is None
    vals = fp.compute(list(tiny.named_parameters())[:3], "cpu")
    assert len(vals) == 3 and all(isinstance(v, int) and 0 <= v <= M64 for v in vals.values())


def test_text_tower_refuses_an_mlp_that_is_not_four_times_the_width():
    """The tower program's MLP GEMMs are built for 4 x width; a holder of another size must be refused when the tower is made, not read
    out of bounds on the device."""
    import transformers
    from sd_webui_text2video_amd import text_encoder as TE
    kw = dict(vocab_size=100, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=77, hidden_act="quick_gelu",
              bos_token_id=1, eos_token_id=2)
    TE.ClipTextTower(transformers.CLIPTextModel(transformers.CLIPTextConfig(intermediate_size=512, **kw)))
    with pytest.raises(L.T2VError, match="4 x width"):
        TE.ClipTextTower(transformers.CLIPTextModel(transformers.CLIPTextConfig(intermediate_size=256, **kw)))
