"""GPU (-m gpu): T2V_OP_FINGERPRINT against the torch implementation of the same function (packing.fingerprint_torch, itself pinned to the
definition in tests/test_fingerprint_cpu.py) — bit for bit, every size and start alignment at which the kernel takes another path —
and `verify_weights` end to end: an edit through `.data` (no version counter moves) must reach the next sampling call / encode."""
import pytest
import torch

from oracle import configs, synth
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd import text_encoder as TE
from sd_webui_text2video_amd import videocrafter as VC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = pk.FINGERPRINT_CHUNK
SIZES = [0, 2, 4, 14, 16, 18, C - 2, C, C + 2, 3 * C + 6]


def _layout(pairs):
    """[(nbytes, offset past a 16-byte boundary)] -> (host byte buffer, [(start, nbytes)]): the segments lie in one buffer of random bytes
    (so a read outside a segment would show), filled alternately with the bytes of fp16 and of fp32 normal variates."""
    g = torch.Generator().manual_seed(len(pairs))
    starts, pos = [], 0
    for nb, off in pairs:
        pos = (pos + 15) // 16 * 16 + 16 + off
        starts.append(pos)
        pos += nb
    buf = torch.randint(0, 256, (pos + 64,), dtype=torch.uint8, generator=g)
    for k, ((nb, off), st) in enumerate(zip(pairs, starts)):
        if k % 2 == 0:
            src = torch.randn(nb // 2, generator=g).to(torch.float16).view(torch.uint8)
        else:
            src = torch.cat([torch.randn(nb // 4, generator=g).view(torch.uint8), torch.randint(0, 256, (nb % 4,), dtype=torch.uint8, generator=g)])
        buf[st:st + nb] = src
    return buf, [(st, nb) for (nb, _), st in zip(pairs, starts)]


def _device_values(fp, dbuf, segs):
    assert dbuf.data_ptr() % 16 == 0
    return fp.compute_ranges([(dbuf.data_ptr() + st, nb) for st, nb in segs], DEV)


TABLES = {
    "one": [(3 * C + 6, 6)],
    "forty_a": [(nb, 2 * (2 * (k // 10) + (k % 10) % 2)) for k, nb in enumerate(SIZES * 4)],
    "forty_b": [(nb, 2 * (2 * (k // 10) + 1 - (k % 10) % 2)) for k, nb in enumerate(SIZES * 4)],
}


def test_tables_cover_every_size_at_every_alignment():
    seen = {(nb, off) for name in ("forty_a", "forty_b") for nb, off in TABLES[name]}
    assert seen == {(nb, off) for nb in SIZES for off in range(0, 16, 2)}


@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_torch_implementation(name):
    buf, segs = _layout(TABLES[name])
    want = [pk.fingerprint_torch(buf[st:st + nb]) for st, nb in segs]
    dbuf = buf.to(DEV)
    fp = pk.ParamFingerprint()
    got = _device_values(fp, dbuf, segs)
    assert got == want, [k for k in range(len(segs)) if got[k] != want[k]]
    assert _device_values(fp, dbuf, segs) == want                                   # cached tables, second launch: the same bits
    assert _device_values(pk.ParamFingerprint(), dbuf.clone(), segs) == want        # another address, fresh tables
    assert fp.last_bytes == sum(nb for _, nb in segs)


def test_one_element_edits_change_exactly_their_segment():
    buf, segs = _layout(TABLES["forty_a"])
    big = max(range(len(segs)), key=lambda k: (segs[k][1], k))
    st, nb = segs[big]
    assert nb == 3 * C + 6
    dbuf = buf.to(DEV)
    fp = pk.ParamFingerprint()
    base = _device_values(fp, dbuf, segs)
    words = dbuf[st:st + nb].view(torch.int16)
    for j in (0, nb // 2 - 1, C // 2 - 1, C // 2, 2 * C // 2 - 1):                  # first, last, the two words at a chunk boundary, ...
        old = int(words[j])
        words[j] = old ^ 0x0400
        now = _device_values(fp, dbuf, segs)
        hbuf = dbuf.cpu()
        assert [k for k in range(len(segs)) if now[k] != base[k]] == [big], j
        assert now[big] == pk.fingerprint_torch(hbuf[st:st + nb]), j
        words[j] = old
    assert _device_values(fp, dbuf, segs) == base
    # a four-byte element that straddles the chunk boundary: both of its words at once
    words[C // 2 - 1] ^= 0x0010
    words[C // 2] ^= 0x0010
    now = _device_values(fp, dbuf, segs)
    assert [k for k in range(len(segs)) if now[k] != base[k]] == [big] and now[big] == pk.fingerprint_torch(dbuf.cpu()[st:st + nb])


def _inputs_tiny():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 5, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def _tiny_ld(sd=None):
    ld = VC.LatentDiffusion(configs.TINY_LVDM_UNET, image_size=[8, 8], video_length=5, init_weights=False, **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    net.load_state_dict(sd if sd is not None else synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    return ld.to(DEV), net


def _sample(ld, ctx, x_T):
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(3)
    x0, _ = smp.sample(S=2, conditioning=ctx[0:1].to(DEV), batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                       unconditional_guidance_scale=7.5, unconditional_conditioning=ctx[1:2].to(DEV), eta=0.0, x_T=x_T.to(DEV))
    return x0


def test_a_data_edit_reaches_the_next_sampling_call():
    """The reference's LoRA loaders write `weight.data += ...`: no identity, no version moves, and the signature check sees nothing.  The
    sampler's once-per-call `verify_weights` must: the output equals, bit for bit, a fresh model built on the edited weights."""
    x, t, ctx, x_T = _inputs_tiny()
    ld, net = _tiny_ld()
    net(x.to(DEV), t.to(DEV), context=ctx.to(DEV))                                # packs and binds
    stale = _sample(ld, ctx, x_T)
    name = "input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"
    w = dict(net.named_parameters())[name]
    version, ptrs = w._version, {k: v.data_ptr() for k, v in net._packed.items()}
    g = torch.Generator().manual_seed(2)
    w.data += (0.05 * torch.randn(w.shape, generator=g)).to(DEV)
    assert w._version == version
    got = _sample(ld, ctx, x_T)
    assert 0 < net.last_repack < len(net._packed) // 2 and {k: v.data_ptr() for k, v in net._packed.items()} == ptrs
    fresh_ld, _ = _tiny_ld({k: v.detach().cpu() for k, v in net.state_dict().items()})
    want = _sample(fresh_ld, ctx, x_T)
    assert torch.equal(got, want)
    assert not torch.equal(got, stale)
    assert net.verify_weights(DEV) == []


def test_a_data_edit_reaches_the_next_text_encode():
    import transformers
    cfg = transformers.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                                      max_position_embeddings=77, hidden_act="quick_gelu", bos_token_id=1, eos_token_id=2)
    torch.manual_seed(13)

    def build():
        m = transformers.CLIPTextModel(cfg).eval()
        return m

    m = build().to(DEV)
    tower = TE.ClipTextTower(m)
    tok = torch.randint(0, 1000, (2, 77), generator=torch.Generator().manual_seed(1)).to(DEV)
    z0 = tower(tok)
    w = next(mod for n, mod in m.named_modules() if n.endswith("encoder.layers.0.self_attn.q_proj")).weight     # (with or without a `text_model.` level)
    version = w._version
    w.data += 0.05
    assert w._version == version
    z1 = tower(tok)
    m2 = build().to(DEV)
    m2.load_state_dict(m.state_dict())
    want = TE.ClipTextTower(m2)(tok)
    assert torch.equal(z1, want) and not torch.equal(z1, z0)
    assert tower.verify_weights(DEV) == []
