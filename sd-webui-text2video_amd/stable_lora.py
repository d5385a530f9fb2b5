"""Stable LoRA for the ModelScope path (reference: scripts/stable_lora/stable_utils/lora_processor.py, scripts/stable_lora/scripts/lora_webui.py):
the selected LoRA files are MERGED into the weights of `pipe.sd_model` and `pipe.clip_encoder.model.transformer` before sampling, and taken
out again (the same merge with -alpha) when the selection, the weight or an option changes.

    StableLoraProcessor.process_lora   one model, a list of loaded files: resolve every key, then merge file by file
    StableLoraScript.process           the webui state machine around it (what changed since the last generation -> undo / merge calls)
    pipeline.process_modelscope        runs `process` when args_dict has a `stable_lora` entry (or an eight-element `extra_args`)

Weights on a GPU are updated by ONE launch per file and model (`T2V_OP_LORA_MERGE`, csrc/elementwise.hip): a device table of segments
{W, A, B, N, J, r, form, dtype} and a tile table, each workgroup one run of `LORA_TILE` elements of one weight.  Weights on the CPU go through
`_merge_torch`, the same arithmetic in torch ops and its executable definition.  The arithmetic, per element, every step rounded once to the
weight's dtype T:

    d = T(sum over ascending k of B[n, k] A[k, j], fp32)          direct form: Linear, Conv2d (`(B @ A).view(weight.shape)` on contiguous memory)
    d = T((d[3j] + d[3j + 1] + d[3j + 2]) / 3)                    temporal form: Conv3d [o, i, 3, 1, 1] — the product viewed [o, i, 3, 3, 1],
                                                                  mean over the second 3 (lora_processor.py:87-94)
    e = T(d * alpha);   W = T(W + e)                              un-merge: alpha -> -alpha

For fp16 weights this is bit for bit what the reference's torch calls give (tests/golden/stable_lora_tiny.npz holds its digests)."""
from __future__ import annotations

import ctypes
import glob
import os

import numpy as np
import torch
from torch import nn

from . import _lib as L

_SEG_DTYPE = np.dtype([("w", "<u8"), ("a", "<u8"), ("b", "<u8"), ("N", "<i4"), ("J", "<i4"), ("r", "<i4"), ("form", "<i4"),
                       ("dtype", "<i4"), ("pad", "<i4")])          # the 48-byte segment record of include/t2v_hip.h
_DTYPES = {torch.float16: L.F16, torch.float32: L.F32}


# ------------------------------------------------------------------------------------------
# the arithmetic
# ------------------------------------------------------------------------------------------
@torch.no_grad()
def _merge_torch(weight: torch.Tensor, lora_A: torch.Tensor, lora_B: torch.Tensor, alpha: float, form: int = L.LORA_DIRECT) -> None:
    """The contract in torch ops, in place on a contiguous `weight` (any device): A [r, Jf], B [N, r] in the weight's dtype T.  The sum runs
    over k in ascending order in fp32 (one rank-1 update per k: no library reduction order enters), every later step is rounded once to T."""
    T = weight.dtype
    N, r = lora_B.shape
    Jf = lora_A.shape[1]
    A32, B32 = lora_A.to(torch.float32), lora_B.to(torch.float32)
    s = torch.zeros(N, Jf, dtype=torch.float32, device=weight.device)
    for k in range(r):
        s.addcmul_(B32[:, k:k + 1], A32[k:k + 1, :])
    d = s.to(T)
    if form == L.LORA_TEMPORAL:
        d3 = d.to(torch.float32).view(N, Jf // 3, 3)
        d = (((d3[..., 0] + d3[..., 1]) + d3[..., 2]) / 3.0).to(T)
    e = (d.to(torch.float32) * float(np.float32(alpha))).to(T)
    w = weight.view(N, -1)
    w.copy_((w.to(torch.float32) + e.to(torch.float32)).to(T))


def tile_table(sizes) -> np.ndarray:
    """uint32 [tiles, 2] = {segment, tile} of element counts: every tile of LORA_TILE elements of every segment exactly once, segment by
    segment (numpy: the full UNet has 3.4e5 tiles)."""
    counts = -(-np.asarray(sizes, dtype=np.int64) // L.LORA_TILE)
    first = np.cumsum(counts) - counts
    seg = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    return np.stack([seg, np.arange(int(counts.sum()), dtype=np.int64) - first[seg]], axis=1).astype(np.uint32)


def merge_device(segments, alpha: float, device, stream=None):
    """ONE launch of T2V_OP_LORA_MERGE.  segments: [(W address, A address, B address, N, J, r, form, dtype tag)] on `device`, element-aligned,
    pairwise disjoint weights.  -> the two device tables: the caller keeps them (and every tensor the addresses point into) alive until the
    stream has been synchronised."""
    if not segments:
        return ()
    seg = np.zeros(len(segments), dtype=_SEG_DTYPE)
    for k, (w, a, b, N, J, r, form, dt) in enumerate(segments):
        seg[k] = (w, a, b, N, J, r, form, dt, 0)
    tiles = tile_table([int(s[3]) * int(s[4]) for s in segments])
    if len(tiles) >= 1 << 31:
        raise L.T2VError("lora merge: too many tiles for one launch")
    seg_d = torch.from_numpy(seg.view(np.int64).reshape(-1, 6)).to(device)
    til_d = torch.from_numpy(tiles.view(np.int32)).to(device)
    op = L.T2VOp()
    op.kind = L.OP_LORA_MERGE
    op.i[0], op.i[1] = len(segments), len(tiles)
    op.f[0] = alpha
    op.p[0], op.p[1] = seg_d.data_ptr(), til_d.data_ptr()
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    L.check(L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(stream)))
    return seg_d, til_d


# ------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------
def load_lora_file(entry):
    """A selection entry -> {key: tensor}: an already-loaded dict as it is, `.safetensors` through safetensors, anything else torch.load."""
    if isinstance(entry, dict):
        return entry
    if str(entry).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(entry)
    return torch.load(entry, map_location="cpu")


def get_lora_files(lora_dir):
    """lora_processor.py:18-34: the `.safetensors` files under `lora_dir` whose metadata has the key `stable_lora_text_to_video`.
    -> ([metadata + {path, lora_name}], [lora_name])"""
    from safetensors import safe_open
    found = []
    for path in sorted(glob.glob(os.path.join(lora_dir, "**/*.safetensors"), recursive=True)):
        with safe_open(path, "pt") as f:
            metadata = f.metadata()
        if metadata is not None and "stable_lora_text_to_video" in metadata.keys():
            metadata = dict(metadata)
            metadata["path"] = path
            metadata["lora_name"] = os.path.splitext(os.path.basename(path))[0]
            found.append(metadata)
    return found, [m["lora_name"] for m in found]


# ------------------------------------------------------------------------------------------
# lora_processor.py
# ------------------------------------------------------------------------------------------
class StableLoraProcessor:
    def __init__(self):
        self.lora_loaded = "lora_loaded"
        self.previous_lora_alpha = 1
        self.previous_lora_file_names = []
        self.previous_advanced_options = []
        self.lora_dir = None
        self.last_touched = []          # parameter names the last process_lora call wrote (in order, once each)

    def log(self, *args):
        print("[Stable LoRA]", *args)

    def key_name_match(self, value, key, name):
        return value in key and name == key.split(f".{value}")[0]

    def is_lora_loaded(self, sd_model):
        return hasattr(sd_model, self.lora_loaded)

    # ---- resolution: every key of every file, before any weight changes ---------------------------
    def _resolve(self, model, lora_files_list, use_bias, use_time, use_conv, use_linear):
        """-> per file [(name, module, A, B, N, J, r, form)] in key order.  A key counts when `key_name_match` pairs it with a module of
        THIS model (one file carries the UNet's and the text encoder's keys: the others are not ours to judge)."""
        modules = dict(model.named_modules())
        plan = []
        for lora_model in lora_files_list:
            todo = []
            for key in lora_model.keys():
                if "bias" in key and use_bias:
                    name = key.split(".bias")[0]
                    m = modules.get(name)
                    if m is not None and self.key_name_match("bias", key, name) and getattr(m, "bias", None) is None:
                        raise L.T2VError(f"LoRA key {key!r}: a bias for the bias-free module {name!r} — the compiled programs have no slot "
                                         "for an added parameter; no weight was changed")
                if "lora_A" not in key:
                    continue
                name = key.split(".lora_A")[0]
                m = modules.get(name)
                if m is None or not self.key_name_match("lora_A", key, name):
                    continue
                partner = f"{name}.lora_B"
                if partner not in lora_model:
                    raise L.T2VError(f"LoRA key {key!r} has no partner {partner!r}; no weight was changed")
                if isinstance(m, nn.Linear) and use_linear:
                    form = L.LORA_DIRECT
                elif isinstance(m, nn.Conv2d) and use_conv:
                    form = L.LORA_DIRECT
                elif isinstance(m, nn.Conv3d) and use_conv and use_time:
                    form = L.LORA_TEMPORAL
                else:
                    continue                # Conv1d, Embedding (the reference computes a table and drops it), a class switched off
                A, B = lora_model[key], lora_model[partner]
                if isinstance(m, nn.Linear) and "proj" in name:
                    A, B = A.squeeze(-1), B.squeeze(-1)
                w = m.weight
                if w.dtype not in _DTYPES:
                    raise L.T2VError(f"LoRA key {key!r}: the weight of {name!r} is {w.dtype}; fp16 and fp32 weights are merged; no weight was changed")
                if not w.is_contiguous():
                    raise L.T2VError(f"LoRA key {key!r}: the weight of {name!r} is not contiguous; no weight was changed")
                fits = A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[1] and A.shape[0] >= 1 and w.numel() > 0
                if fits and form == L.LORA_DIRECT:
                    fits = B.shape[0] * A.shape[1] == w.numel()
                elif fits:
                    fits = (w.dim() == 5 and tuple(w.shape[2:]) == (3, 1, 1) and A.shape[1] % 3 == 0 and B.shape[0] * A.shape[1] == 3 * w.numel())
                if not fits:
                    raise L.T2VError(f"LoRA key {key!r}: factors {tuple(B.shape)} x {tuple(A.shape)} do not fit the weight {tuple(w.shape)} of "
                                     f"{name!r}; no weight was changed")
                J = A.shape[1] // 3 if form == L.LORA_TEMPORAL else A.shape[1]
                if max(B.shape[0], J, A.shape[0]) >= 1 << 31:
                    raise L.T2VError(f"LoRA key {key!r}: a dimension does not fit 32 bits; no weight was changed")
                todo.append((name, m, A, B, int(B.shape[0]), int(J), int(A.shape[0]), form))
            # the targets of ONE file are the segments of one launch: they must not overlap
            spans = sorted((m.weight.data_ptr(), m.weight.data_ptr() + m.weight.numel() * m.weight.element_size(), name) for name, m, *_ in todo)
            for (b0, e0, n0), (b1, e1, n1) in zip(spans, spans[1:]):
                if b1 < e0:
                    raise L.T2VError(f"LoRA targets {n0!r} and {n1!r} overlap in memory; no weight was changed")
            plan.append(todo)
        return plan

    @torch.no_grad()
    def process_lora(self, model, lora_files_list, use_bias, use_time, use_conv, use_emb, use_linear, lora_alpha, undo_merge=False):
        """lora_processor.py:202-246 with the reference's signature and matching rules: `key_name_match` on `.lora_A` / `.bias`; Linear under
        `use_linear` (both factors `squeeze(-1)` when 'proj' is in the module's name), Conv2d under `use_conv`, Conv3d under `use_conv and
        use_time`; the files of the list in list order.  `undo_merge` subtracts: the same merge with -alpha.  Differences from the reference:
          * every key of every file is resolved and shape-checked BEFORE any weight changes; a missing `lora_B`, factors that do not fit,
            a non-contiguous weight or overlapping targets raise T2VError naming the key (the reference dies half-merged);
          * the weights are written in place in the existing Parameter (the reference assigns a new one), on a GPU by one launch per file
            (T2V_OP_LORA_MERGE); a model of this package with a live pack is then re-packed partially (`_refresh_weights(also_changed=...)`:
            the fingerprints follow the new bytes, the cached context K/V are dropped);
          * a `.bias` key for a module that HAS a bias is ignored — the reference's `m.bias.weight = v` sets an attribute and changes
            nothing; for a bias-free module it is refused under `use_bias`, before anything changes: the compiled programs have no slot
            for an added parameter;
          * Embedding targets are ignored (the reference computes a table and drops it), Conv1d never matches there either;
          * the factors are cast to the weight's dtype.  fp32 weights: fp32 throughout, the reference's CPU result (its autocast on a GPU
            would make the product fp16); the deployed model is `.half()`, where both agree bit for bit."""
        plan = self._resolve(model, lora_files_list, use_bias, use_time, use_conv, use_linear)
        alpha = -float(lora_alpha) if undo_merge else float(lora_alpha)
        keep, touched, devices = [], [], set()
        for todo in plan:
            by_device = {}
            for name, m, A, B, N, J, r, form in todo:
                w = m.weight
                A = A.to(w.device, w.dtype).contiguous()
                B = B.to(w.device, w.dtype).contiguous()
                if name + ".weight" not in touched:
                    touched.append(name + ".weight")
                if w.device.type == "cpu":
                    _merge_torch(w, A, B, alpha, form)
                    continue
                keep.append((A, B))
                by_device.setdefault(w.device, []).append((w.data_ptr(), A.data_ptr(), B.data_ptr(), N, J, r, form, _DTYPES[w.dtype]))
            for dev, segments in by_device.items():
                with torch.cuda.device(dev):
                    keep.append(merge_device(segments, alpha, dev))
                devices.add(dev)
        for dev in devices:
            torch.cuda.current_stream(dev).synchronize()       # the tables and the factors may go now
        del keep
        self.last_touched = touched
        if touched and getattr(model, "_packed", None) is not None and hasattr(model, "_refresh_weights"):
            model._refresh_weights(model._packed_device, also_changed=touched)
        return touched

    # ---- the state machine's helpers (lora_processor.py:103-200) ------------------------------------
    def get_loras_to_process(self, lora_files):
        """Selection entries -> what `load_loras_from_list` reads: a dict as it is, a path as it is, a name resolved against `lora_dir`
        (the file itself, with `.safetensors` appended, or by the `lora_name` of `get_lora_files`).  A name that resolves to nothing is
        an error here; the reference drops it silently and generates with the base model."""
        out = []
        for entry in lora_files:
            if isinstance(entry, dict) or os.path.isfile(str(entry)):
                out.append(entry)
                continue
            found = None
            if self.lora_dir is not None:
                for cand in (os.path.join(self.lora_dir, str(entry)), os.path.join(self.lora_dir, str(entry) + ".safetensors")):
                    if os.path.isfile(cand):
                        found = cand
                        break
                if found is None:
                    found = next((m["path"] for m in get_lora_files(self.lora_dir)[0] if m["lora_name"] == entry), None)
            if found is None:
                raise L.T2VError(f"LoRA file {entry!r} not found (lora_dir = {self.lora_dir!r})")
            out.append(found)
        return out

    def load_loras_from_list(self, lora_files):
        return [load_lora_file(f) for f in lora_files]

    def undo_merge_preprocess(self):
        previous = self.load_loras_from_list(self.get_loras_to_process(self.previous_lora_file_names))
        return previous, self.previous_lora_alpha

    def handle_lora_load(self, sd_model, lora_files_list, set_lora_loaded=False, unload_args=None):
        if not hasattr(sd_model, self.lora_loaded) and set_lora_loaded:
            setattr(sd_model, self.lora_loaded, True)
        if self.is_lora_loaded(sd_model) and not set_lora_loaded:
            unload_args[1], unload_args[-1] = self.undo_merge_preprocess()
            self.process_lora(*unload_args, undo_merge=True)
            delattr(sd_model, self.lora_loaded)

    def handle_alpha_change(self, lora_alpha, model):
        return (lora_alpha != self.previous_lora_alpha) and self.is_lora_loaded(model)

    def handle_options_change(self, options, model):
        return (options != self.previous_advanced_options) and self.is_lora_loaded(model)

    def handle_lora_start(self, lora_files, model, unload_args):
        if len(lora_files) == 0 and self.is_lora_loaded(model):
            self.handle_lora_load(model, lora_files, set_lora_loaded=False, unload_args=unload_args)
            self.log("Unloaded previously loaded LoRA files")

    def handle_after_lora_load(self, model, lora_files, lora_file_names, advanced_options, lora_alpha):
        self.handle_lora_load(model, lora_files, set_lora_loaded=True)
        self.previous_lora_file_names = lora_file_names
        self.previous_advanced_options = advanced_options
        self.previous_lora_alpha = lora_alpha


def _same_selection(a, b) -> bool:
    """List equality where loaded dicts compare by identity (a dict of tensors has no usable ==)."""
    return len(a) == len(b) and all((x is y) if isinstance(x, dict) or isinstance(y, dict) else x == y for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------
# lora_webui.py
# ------------------------------------------------------------------------------------------
class StableLoraScript(StableLoraProcessor):
    @staticmethod
    def models_of(pipe) -> list:
        """The reference's two targets in its order (lora_webui.py:187): the UNet, then the text encoder's transformer (None when the pipe
        has no encoder of that shape, e.g. ready conditioning tensors: its calls are skipped, the rest of the sequence is unchanged)."""
        enc = getattr(pipe, "clip_encoder", None)
        return [pipe.sd_model, getattr(getattr(enc, "model", None), "transformer", None)]

    @torch.no_grad()
    def process(self, pipe, lora_files_selection, lora_alpha, use_bias, use_linear, use_conv, use_emb, use_multiplier, use_time, lora_dir=None):
        """lora_webui.py:127-214, the state machine as it stands: `lora_loaded` on `pipe.sd_model`; the previous file names, alpha and
        options; unload (the UNet only, as there) when the selection empties; undo-then-merge when alpha, options or files change; both
        models in the reference's order.  It emits the reference's sequence of `process_lora(model, files, ..., alpha, undo_merge)` calls,
        INCLUDING its two habits: `lora_alpha` is rescaled by `use_multiplier / len(files)` inside the loop over the two
        models, so the text encoder receives the factor twice, and the value recorded for the next undo is the last one computed — which
        is also what the UNet is then un-merged with.  With one file and multiplier 1 every one of these values is the slider's."""
        if lora_dir is not None:
            self.lora_dir = lora_dir
        lora_file_names = [x for x in lora_files_selection if isinstance(x, dict) or x != "None"]
        lora_files = self.get_loras_to_process(lora_file_names)
        advanced_options = [use_bias, use_linear, use_conv, use_emb, use_multiplier, use_time]
        sd_model, transformer = self.models_of(pipe)
        alpha_changed = self.handle_alpha_change(lora_alpha, sd_model)
        options_changed = self.handle_options_change(advanced_options, sd_model)
        lora_changed = not _same_selection(self.previous_lora_file_names, lora_file_names)
        first_lora_init = not self.is_lora_loaded(sd_model)
        unload_args = [sd_model, None, use_bias, use_time, use_conv, use_emb, use_linear, None]
        self.handle_lora_start(lora_files, sd_model, unload_args)
        can_use_lora = not self.is_lora_loaded(sd_model)
        lora_params_changed = any([alpha_changed, lora_changed, options_changed])
        if can_use_lora or lora_params_changed:
            if len(lora_files) == 0:
                return
            for i, model in enumerate([sd_model, transformer]):
                lora_alpha = (lora_alpha * use_multiplier) / len(lora_files)
                if model is None:
                    continue
                lora_files_list = self.load_loras_from_list(lora_files)
                args = [model, lora_files_list, use_bias, use_time, use_conv, use_emb, use_linear, lora_alpha]
                if lora_params_changed and not first_lora_init:
                    if i == 0:
                        self.log("Resetting weights to reflect changed options.")
                    undo_args = args.copy()
                    undo_args[1], undo_args[-1] = self.undo_merge_preprocess()
                    self.process_lora(*undo_args, undo_merge=True)
                self.process_lora(*args, undo_merge=False)
            self.handle_after_lora_load(sd_model, lora_files, lora_file_names, advanced_options, lora_alpha)


STABLE_LORA_ARGS = ("lora_files_selection", "lora_alpha", "use_bias", "use_linear", "use_conv", "use_emb", "use_multiplier", "use_time")


def run_for_pipe(pipe, settings) -> None:
    """`settings`: a dict with the eight values of STABLE_LORA_ARGS (missing ones: weight 1, every class on, multiplier 1; optional
    `lora_dir`), or the eight values as a sequence in that order (the reference's `extra_args`).  The script object — the state between
    generations — lives on the pipe."""
    if not isinstance(settings, dict):
        settings = list(settings)
        if len(settings) != len(STABLE_LORA_ARGS):
            raise L.T2VError(f"stable_lora: expected the {len(STABLE_LORA_ARGS)} values {STABLE_LORA_ARGS}, got {len(settings)}")
        settings = dict(zip(STABLE_LORA_ARGS, settings))
    unknown = set(settings) - set(STABLE_LORA_ARGS) - {"lora_dir"}
    if unknown:
        raise L.T2VError(f"stable_lora: unknown entries {sorted(unknown)}")
    defaults = dict(lora_files_selection=[], lora_alpha=1, use_bias=True, use_linear=True, use_conv=True, use_emb=True, use_multiplier=1,
                    use_time=True, lora_dir=None)
    script = getattr(pipe, "_stable_lora_script", None)
    if script is None:
        script = pipe._stable_lora_script = StableLoraScript()
    script.process(pipe, **{**defaults, **settings})
