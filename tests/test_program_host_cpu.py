"""CPU: compiled.ProgramHost, the one owner of "programs keyed by geometry + the packed images they are bound to", on a bare host and
on every kind of owner (VAE, adapter, text tower, a parameterless table cache).  Host bookkeeping only: packs are made on "cpu", no
program is bound — a sentinel in `comp.bound` stands for a live binding wherever "stays bound" / "is unbound" is the property."""
import torch

import adapter_ref as AR
from oracle import configs, synth
from sd_webui_text2video_amd import compiled as CP
from sd_webui_text2video_amd import text_encoder as TE
from sd_webui_text2video_amd import unet as U
from sd_webui_text2video_amd import vae as V
from sd_webui_text2video_amd import videocrafter as VC
from test_text_encoder_cpu import TINY, _seed_params

BOUND = object()          # stands for a BoundProgram


def test_unet_module_still_exports_the_moved_names():
    assert U._Compiled is CP._Compiled and U._dt is CP._dt and issubclass(U.UNetSD, CP.ProgramHost)


# ---- (1) programs: get-or-build and eviction ------------------------------------------------------------------------------------------
def test_eviction_keeps_the_newest_and_a_held_program_is_not_built_again():
    host = CP.ProgramHost()
    assert host.max_programs == 4 and host._programs == {} and host._packed is None and host._param_signature() == {}
    host.max_programs = 2
    built = []

    def build(k):
        built.append(k)
        return object()

    comps = {k: host._program(k, lambda k=k: build(k)) for k in "abc"}
    assert list(host._programs) == ["b", "c"] and built == ["a", "b", "c"]
    assert host._program("b", lambda: build("b")) is comps["b"] and built == ["a", "b", "c"]
    assert list(host._programs) == ["b", "c"]
    assert host._program("a", lambda: build("a")) is not comps["a"] and list(host._programs) == ["c", "a"]      # evicted: built again

    host = CP.ProgramHost(max_programs=None)
    for k in range(5):
        host._program(k, object)
    assert list(host._programs) == [0, 1, 2, 3, 4]


# ---- (2), (3) a module with parameters and two programs that declare different images -------------------------------------------------
def _equals_full_pack(host, comps, sd):
    for comp in comps:
        full = comp.packer.materialise(sd, "cpu")
        assert full and full.keys() <= host._packed.keys()
        for k, v in full.items():
            assert host._packed[k].dtype == v.dtype and torch.equal(host._packed[k], v), k


def _second_program_then_parameter_edit(host, build_a, build_b, param):
    names = lambda comp: {n for n, _, _ in comp.packer.recipes}
    a = host._program("a", build_a)
    host._ensure_packed(a, "cpu")
    assert set(host._packed) == names(a) and host._packed_device == torch.device("cpu")
    a.bound = BOUND
    pack, images = host._packed, dict(host._packed)
    ptrs = {k: v.data_ptr() for k, v in images.items()}

    b = host._program("b", build_b)
    assert names(b) - names(a), "the second program must declare images the first one does not"
    host._ensure_packed(b, "cpu")
    assert host._packed is pack and a.bound is BOUND                          # the first program stays bound ...
    assert all(host._packed[k] is t for k, t in images.items())               # ... to the very tensors it was bound to
    assert {k: host._packed[k].data_ptr() for k in ptrs} == ptrs
    assert set(host._packed) == names(a) | names(b)
    _equals_full_pack(host, (a, b), host.state_dict())
    host._ensure_packed(a, "cpu")                                             # nothing moved: nothing happens
    assert host._packed is pack and set(host._packed) == names(a) | names(b) and a.bound is BOUND

    b.bound = BOUND
    before = {k: v.clone() for k, v in host._packed.items()}
    with torch.no_grad():
        param.add_(0.25)                                                      # in place: the version counter moves
    host._ensure_packed(a, "cpu")
    assert host._packed is not pack and a.bound is None and b.bound is None   # a fresh pack, every program unbound
    assert set(host._packed) == names(a)
    _equals_full_pack(host, (a,), host.state_dict())
    assert any(not torch.equal(host._packed[k], before[k]) for k in host._packed), "the edit did not reach the pack"
    host._ensure_packed(b, "cpu")
    _equals_full_pack(host, (a, b), host.state_dict())
    assert host.verify_weights("cpu") == []                                   # no fingerprints kept by this owner


def test_vae_encoder_program_joins_the_decoder_pack_without_touching_it():
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4)
    synth.load_synth(ae, seed=3)
    assert ae.max_programs == 4
    _second_program_then_parameter_edit(
        ae, lambda: ae._lower(2, 8, 8, "f32", "f32", lambda low: low.build()),
        lambda: ae._lower(2, 64, 64, "f32", "f32", lambda low: low.build_encoder()), ae.decoder.conv_in.weight)


def test_adapter_front_only_program_joins_the_full_pack_without_touching_it():
    ad = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS["t2i"])
    assert ad.max_programs == 4
    _second_program_then_parameter_edit(
        ad, lambda: ad._compile(5, 64, 48, "f32", True),
        lambda: ad._compile(5, 64, 48, "f32", True, front_only=True, src_hw=(40, 30)), ad.conv_in.weight)


# ---- (4) the text tower: fingerprints, "drop the pack" ---------------------------------------------------------------------------------
def test_text_tower_data_edit_drops_the_pack_and_programs_pack_their_own_images():
    model = _seed_params(TE.OpenClipTextModel(**TINY), 4)
    tower = TE.ClipTextTower(model, heads=2, act="gelu", skip_last=1)
    assert tower.max_programs is None
    assert tower.verify_weights("cpu") == []                                  # before any pack
    plain = tower._program((2, 77), lambda: tower._compile(2, 77))
    tower._ensure_packed(plain, "cpu")
    plain.bound = BOUND
    assert tower.verify_weights("cpu") == [] and plain.bound is BOUND and tower._packed is not None

    name = tower.names.tok()
    p = dict(model.named_parameters())[name]
    ident = (id(p), p._version)
    old = {k: v.clone() for k, v in tower._packed.items()}
    p.data += 0.5                                                             # neither identity nor version moves
    assert (id(p), p._version) == ident and tower._param_signature() == tower._packed_sig
    assert tower.verify_weights("cpu") == [name] and tower._packed is None
    tower._ensure_packed(plain, "cpu")
    assert plain.bound is None                                                # the images are new tensors
    _equals_full_pack(tower, (plain,), model.state_dict())
    assert any(not torch.equal(tower._packed[k], old[k]) for k in old), "the edited bytes did not reach the pack"
    assert tower.verify_weights("cpu") == [] and tower._packed is not None

    plain.bound = BOUND
    pack, images = tower._packed, dict(tower._packed)
    emph = tower._program((2, 77, True), lambda: tower._compile(2, 77, emphasis=True))
    tower._ensure_packed(emph, "cpu")
    assert tower._packed is pack and plain.bound is BOUND and all(tower._packed[k] is t for k, t in images.items())
    _equals_full_pack(tower, (plain, emph), model.state_dict())
    assert list(tower._programs) == [(2, 77), (2, 77, True)]


# ---- (5) a host without parameters: tables only ----------------------------------------------------------------------------------------
def test_parameterless_host_shares_one_pack_and_a_device_change_drops_it():
    host = CP.ProgramHost(max_programs=4)
    a = host._program("a", lambda: VC._bicubic_compile(1, (8, 8), (16, 16), "f32"))
    b = host._program("b", lambda: VC._bicubic_compile(1, (8, 8), (12, 20), "f32"))
    host._ensure_packed(a, "cpu")
    pack, images = host._packed, dict(host._packed)
    a.bound = BOUND
    host._ensure_packed(b, "cpu")
    b.bound = BOUND
    assert host._packed is pack and a.bound is BOUND and all(host._packed[k] is t for k, t in images.items())
    assert set(pack) == {n for c in (a, b) for n, _, _ in c.packer.recipes} and len(pack) > len(images)
    assert host._packed_sig == {} and host.verify_weights("cpu") == []
    _equals_full_pack(host, (a, b), {})

    host._ensure_packed(a, "meta")
    assert host._packed is not pack and host._packed_device == torch.device("meta")
    assert a.bound is None and b.bound is None
    assert set(host._packed) == {n for n, _, _ in a.packer.recipes} and all(t.device.type == "meta" for t in host._packed.values())
    host.invalidate()
    assert host._packed is None and host._packed_sig is None

