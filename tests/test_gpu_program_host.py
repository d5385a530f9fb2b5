"""GPU (-m gpu): compiled.ProgramHost under eviction — a program that was dropped is lowered, packed against the live images and bound
again, and gives the bits it gave before; programs that stayed keep running on the pack they were bound to."""
import pytest
import torch

from oracle import configs, synth
from sd_webui_text2video_amd import vae as V
from sd_webui_text2video_amd import videocrafter as VC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_vae_programs_evicted_and_built_again_repeat_bit_for_bit():
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4)
    synth.load_synth(ae, seed=3)
    ae.max_programs = 2
    g = torch.Generator().manual_seed(17)
    z = torch.randn(2, 4, 8, 8, generator=g).to(DEV)
    x = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    calls = [("decode", lambda: ae.decode(z)), ("encode", lambda: ae.encode(x).parameters),
             ("decode_to_uint8", lambda: ae.decode_to_uint8(z)), ("decode", lambda: ae.decode(z))]
    first, seen = {}, []
    for round_ in range(2):
        for name, fn in calls:
            held = set(ae._programs)
            out = fn()
            assert len(ae._programs) <= 2, (round_, name, list(ae._programs))
            seen.append(bool(set(ae._programs) - held))          # did this call compile?
            assert torch.isfinite(out.float()).all()
            if name in first:
                assert out.dtype == first[name].dtype and torch.equal(out, first[name]), (round_, name)
            else:
                first[name] = out.clone()
    # three geometries through two slots: the decoder of call 1 was evicted by call 3 and is compiled and bound again by call 4
    assert seen[:4] == [True, True, True, True] and seen[4] is False and all(seen[5:])
    assert first["decode"].shape == (2, 3, 64, 64) and first["decode_to_uint8"].dtype == torch.uint8


def test_bicubic_program_cache_shares_one_pack():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, 8, 8, generator=g).to(DEV)
    a = VC.bicubic_resize(x, (16, 16))
    other = VC.bicubic_resize(x, (12, 20))
    b = VC.bicubic_resize(x, (16, 16))
    assert a.shape == (1, 1, 16, 16) and other.shape == (1, 1, 12, 20) and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert len(VC._BICUBIC._programs) <= 4 and VC._BICUBIC._packed_device == x.device          # (values: tests/test_gpu_bicubic.py)
