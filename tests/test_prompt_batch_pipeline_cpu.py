"""CPU: the public interface of a batch of different prompts — `TextToVideoSynthesis.preprocess` / `infer_conditioned` and
`process_modelscope` — with a toy encoder and stand-in samplers: per-prompt encoder calls, the noise of `seeds`, the frame split of
`stitch`, and every refusal.  No GPU, no arithmetic."""
import base64
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sd_webui_text2video_amd import pipeline, samplers


class _ToyEncoder:
    """One 77-token chunk per started 10 words; pads a CALL to its longest prompt, as the reference's embedder does."""

    def __init__(self):
        self.calls = []

    def __call__(self, texts):
        self.calls.append(list(texts))
        chunks = max(1, max(-(-len(t.split()) // 10) for t in texts))
        return torch.stack([torch.full((77 * chunks, 8), float(len(t))) for t in texts])


class _Loop(samplers.Txt2VideoSampler):
    """The real `get_noise`; `sample_loop` hands the noise back as the result and records what it was given."""

    def __init__(self):
        self.device, self.noise_gen = "cpu", torch.Generator(device="cpu")
        self.sampler = SimpleNamespace(cfg_parallel=None)
        self.given = None

    def get_sampler(self, *a, **kw):
        return None

    def sample_loop(self, **kw):
        self.given = kw
        return kw["noise"] if kw["latents"] is None else kw["latents"]


def _pipe(enc=None):
    p = pipeline.TextToVideoSynthesis.__new__(pipeline.TextToVideoSynthesis)
    p.clip_encoder, p.diffusion, p.device = enc, _Loop(), torch.device("cpu")
    p.sd_model = SimpleNamespace(to=lambda dev: None)
    return p


def _x0(p, c, uc, **kw):
    return p.infer_conditioned(c, uc, steps=3, frames=2, seed=kw.pop("seed", 40), scale=9.0, width=16, height=16, decode=False, **kw)[1]


# ---- preprocess ------------------------------------------------------------------------------------------------------------------------
def test_preprocess_encodes_every_prompt_by_a_call_of_its_own():
    enc = _ToyEncoder()
    p = _pipe(enc)
    long, short = " ".join(["w"] * 25), "a cat"
    cs, ucs = p.preprocess([long, short, short], "blurry", 5)
    assert enc.calls == [[long], [short], ["blurry"]]                     # one text per call; a text that repeats is encoded once
    assert [c.shape for c in cs] == [(1, 231, 8), (1, 77, 8), (1, 77, 8)]       # the short prompt keeps ITS chunk count
    assert cs[1] is cs[2] and len(ucs) == 3 and all(u is ucs[0] for u in ucs) and ucs[0].shape == (1, 77, 8)
    together = enc([long, short])
    assert together.shape == (2, 231, 8)                                    # what one call for both would have made of the short one
    enc.calls.clear()
    cs, ucs = p.preprocess("a cat", ["n1", "n2 " + long], 5)               # one prompt against several negative prompts
    assert len(cs) == 2 and cs[0] is cs[1] and [u.shape[1] for u in ucs] == [77, 231] and enc.calls == [["a cat"], ["n1"], ["n2 " + long]]
    with pytest.raises(ValueError, match="3 prompts against 2 negative prompts"):
        p.preprocess(["a", "b", "c"], ["x", "y"], 5)
    enc.calls.clear()
    c, uc = p.preprocess("a cat", "blurry", 5)                             # single texts: what it was
    assert torch.is_tensor(c) and torch.is_tensor(uc) and enc.calls == [["a cat"], ["blurry"]]


# ---- infer_conditioned -------------------------------------------------------------------------------------------------------------------
def test_seeds_give_every_video_the_noise_of_its_own_run():
    p = _pipe()
    cs, ucs = [torch.zeros(1, n, 8) for n in (77, 154, 231)], [torch.zeros(1, 77, 8)] * 3
    seeds = [5, 99, 7]
    batch = _x0(p, cs, ucs, seeds=seeds)
    given = p.diffusion.given
    assert batch.shape == (3, 4, 2, 2, 2) and given["batch_size"] == 3 and given["shape"] == (3, 4, 2, 2, 2)
    assert isinstance(given["conditioning"], list) and [v.shape[1] for v in given["conditioning"]] == [77, 154, 231]
    assert isinstance(given["unconditional_conditioning"], list) and len(given["unconditional_conditioning"]) == 3
    for v, s in enumerate(seeds):
        single = _x0(p, cs[v], ucs[v], seed=s)
        assert torch.is_tensor(p.diffusion.given["conditioning"]) and p.diffusion.given["batch_size"] == 1
        assert torch.equal(batch[v:v + 1], single)                          # bit for bit
    default = _x0(p, cs, ucs[0], seed=40)                                   # no seeds: seed + v, as videos=V
    assert p.diffusion.given["unconditional_conditioning"] is ucs[0] and p.diffusion.given["batch_size"] == 3   # (the samplers repeat a single uncond)
    assert all(torch.equal(default[v:v + 1], _x0(p, cs[v], ucs[v], seed=40 + v)) for v in range(3))
    assert torch.equal(_x0(p, cs[0], ucs[0], videos=3, seeds=seeds), batch)          # `seeds` with one prompt for every video
    assert torch.is_tensor(p.diffusion.given["conditioning"])


def test_lists_of_one_entry_and_single_tensors_take_todays_path():
    p = _pipe()
    c, uc = torch.zeros(1, 154, 8), torch.zeros(1, 77, 8)
    a = _x0(p, [c], [uc], seed=11)
    g = p.diffusion.given
    assert g["conditioning"] is c and g["unconditional_conditioning"] is uc and g["batch_size"] == 1
    assert torch.equal(a, _x0(p, c, uc, seed=11)) and torch.equal(a, _x0(p, c, uc, seed=0, seeds=[11]))
    _x0(p, [c], uc, videos=2, seed=11)
    assert p.diffusion.given["conditioning"] is c and p.diffusion.given["batch_size"] == 2


def test_infer_conditioned_refusals():
    p = _pipe()
    cs, ucs = [torch.zeros(1, 77, 8), torch.zeros(1, 154, 8)], [torch.zeros(1, 77, 8)] * 2
    with pytest.raises(NotImplementedError, match="img2vid"):
        _x0(p, cs, ucs, latents=torch.zeros(1, 4, 2, 2, 2), mask=torch.ones(1, 4, 2, 2, 2))
    with pytest.raises(NotImplementedError, match="img2vid"):
        _x0(p, cs, ucs, latents=torch.zeros(1, 4, 2, 2, 2))                   # latents that are no vid2vid clip
    p.sd_model.t_shard = object()
    with pytest.raises(NotImplementedError, match="T-shard"):
        _x0(p, cs, ucs)
    p.sd_model.t_shard = None
    p.diffusion.sampler.cfg_parallel = SimpleNamespace(size=2, role=0)
    with pytest.raises(NotImplementedError, match="CFG-pair"):
        _x0(p, cs, ucs)
    p.diffusion.sampler.cfg_parallel = None
    with pytest.raises(ValueError, match="videos=3"):
        _x0(p, cs, ucs, videos=3)
    with pytest.raises(ValueError, match="3 seeds for 2 videos"):
        _x0(p, cs, ucs, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="one per video"):
        _x0(p, cs, ucs + ucs[:1])
    out = _x0(p, cs, ucs, latents=torch.zeros(1, 4, 2, 2, 2), is_vid2vid=True, strength=0.5)          # vid2vid is not refused
    assert out is not None and p.diffusion.given["is_vid2vid"] and p.diffusion.given["noise"].shape[0] == 2


# ---- process_modelscope --------------------------------------------------------------------------------------------------------------------
class _FakePipe:
    device = "cpu"

    def __init__(self):
        self.calls, self.encoded = [], []

    def preprocess(self, prompt, n_prompt, steps):
        self.encoded.append((prompt, n_prompt))
        return [f"c:{t}" for t in prompt], [f"u:{t}" for t in n_prompt]

    def infer_conditioned(self, c, uc, steps, frames, seed, scale, width=256, height=256, eta=0.0, sampler="DDIM_Gaussian",
                          videos=1, seeds=None, **kw):
        self.calls.append((c, uc, steps, seed, videos, seeds))
        self.kw = kw
        return [np.concatenate([np.full((height, width, 3), s % 256, dtype=np.uint8) for s in seeds], axis=1) for _ in range(frames)], None


def _args(pipe, **kw):
    d = dict(pipe=pipe, prompt="p", n_prompt="n", steps=7, frames=3, seed=40, cfg_scale=9.0, width=16, height=8, eta=0.0, sampler="DDIM_Gaussian")
    d.update(kw)
    return d


def test_process_modelscope_prompt_lists_make_one_pass():
    pipe = _FakePipe()
    frames = pipeline.process_modelscope(_args(pipe, prompts=["a", "b b", "c"], seeds=[3, 200, 9]))
    assert pipe.encoded == [(["a", "b b", "c"], ["n", "n", "n"])]                    # the single negative prompt is broadcast
    assert pipe.calls == [(["c:a", "c:b b", "c:c"], ["u:n"] * 3, 7, 3, 3, [3, 200, 9])]          # ONE pass
    assert len(frames) == 3 and frames[0].shape == (8, 48, 3)                        # side by side
    assert [int(frames[0][0, 16 * v, 0]) for v in range(3)] == [3, 200, 9]
    pipe.calls.clear()
    seen = []
    urls = pipeline.process_modelscope(_args(pipe, prompts=["a", "b b"], n_prompts=["x", "y"],
                                             stitch=lambda fr, info: seen.append((len(fr), fr[0].shape, info)) or bytes([fr[0][0, 0, 0], fr[-1][-1, -1, 2]])))
    assert len(pipe.calls) == 1 and pipe.calls[0][5] == [40, 41]                      # default seeds: seed + v
    assert len(urls) == 2 and all(u.startswith("data:video/mp4;base64,") for u in urls)          # one data-URL per prompt
    assert [list(base64.b64decode(u.split(",", 1)[1])) for u in urls] == [[40, 40], [41, 41]]    # each from its own columns only
    assert [s[:2] for s in seen] == [(3, (8, 16, 3))] * 2
    assert seen[0][2].startswith("a\nNegative prompt: x\n") and "seed: 40" in seen[0][2] and seen[1][2].startswith("b b\nNegative prompt: y\n")
    assert "seed: 41" in seen[1][2]


def test_process_modelscope_context_lists():
    pipe = _FakePipe()
    frames = pipeline.process_modelscope(_args(pipe, conds=["C0", "C1"], unconds=["U0", "U1"], seeds=[1, 2]))
    assert pipe.calls == [(["C0", "C1"], ["U0", "U1"], 7, 1, 2, [1, 2])] and pipe.encoded == [] and frames[0].shape == (8, 32, 3)
    pipe.calls.clear()
    pipeline.process_modelscope(_args(pipe, conds=["C0", "C1", "C2"], uncond="U"))              # a single uncond beside the list
    assert pipe.calls == [(["C0", "C1", "C2"], "U", 7, 40, 3, [40, 41, 42])]
    pipe.calls.clear()
    urls = pipeline.process_modelscope(_args(pipe, conds=["C0", "C1"], unconds=["U0", "U1"], stitch=lambda fr, info: info.encode() + b"."))
    assert len(urls) == 2 and len(pipe.calls) == 1


def test_process_modelscope_prompt_list_vid2vid_and_refusals():
    pipe = _FakePipe()
    lat = torch.randn(1, 4, 3, 1, 2)
    pipeline.process_modelscope(_args(pipe, conds=["C0", "C1"], unconds=["U0", "U1"], do_vid2vid=True, vid2vid_frames=lat, strength=0.5))
    assert pipe.calls[-1][2] == 7 - 3 and pipe.kw["is_vid2vid"] is True and torch.equal(pipe.kw["latents"], lat) and pipe.kw["strength"] == 0.5
    n = len(pipe.calls)
    with pytest.raises(ValueError, match="batch_count"):
        pipeline.process_modelscope(_args(pipe, prompts=["a", "b"], batch_count=2))
    with pytest.raises(NotImplementedError, match="img2vid"):
        pipeline.process_modelscope(_args(pipe, prompts=["a", "b"], inpainting_frames=2, inpainting_image=np.zeros((8, 16, 3), dtype=np.uint8),
                                          inpainting_weights=[0.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="negative prompts"):
        pipeline.process_modelscope(_args(pipe, prompts=["a", "b", "c"], n_prompts=["x", "y"]))
    assert len(pipe.calls) == n                                                       # refused before anything ran
