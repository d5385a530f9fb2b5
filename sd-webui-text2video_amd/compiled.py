"""The host side of every lowered program: `_Compiled` (one program with its arena and binding) and `ProgramHost`, the one owner of
"compiled programs keyed by geometry + the packed weight images they are bound to".

Every owner of programs — UNetSD / videocrafter.UNetModel, AutoencoderKL, ClipTextTower, videocrafter.Adapter as a mixin, the two
parameterless resize caches as a bare object — hands device arenas and image addresses to the library as raw pointers, so the rules for
"this pack is stale" and "this binding is stale" live here and nowhere else:
  * programs: an insertion-ordered dict, at most `max_programs` kept (`_program`, `_evict_programs`);
  * the pack: dropped — and every program unbound — when the parameter signature or the device moves (`_ensure_packed`); otherwise
    only the images a program declares that are not packed yet are made (`_pack_missing`): image tensors are never replaced while
    the pack lives, so programs already bound stay bound;
  * edits the signature cannot see (through `.data`) are found by byte fingerprints where the owner keeps them (`verify_weights`).
A host serves ONE device at a time and is not thread-safe: a call for another device drops the pack and unbinds every program (calls
that alternate between two GPUs re-pack and re-bind each time), and two threads on one host could free images that the other's bound
program still points to.  Images of evicted programs stay in the pack until it is dropped (the UNet alone prunes them, at a partial
re-pack): for the table-only hosts that is a few KB per geometry ever asked for, accepted.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from . import _lib as L
from . import packing as pk
from .program import COLLECTIVE_KINDS, BoundProgram, Program


def _dt(dtype) -> str:
    return "f16" if dtype == torch.float16 else "f32"


class _Compiled:
    def __init__(self, prog: Program, packer: pk.WeightPacker):
        self.prog = prog
        self.packer = packer
        self.bound: Optional[BoundProgram] = None
        self.arena: Optional[torch.Tensor] = None
        self.ctx_token = None          # context token of the last run (step-invariant prologue reuse)
        self.ctx_bound = None

    def ensure_bound(self, packed: Dict[str, torch.Tensor], device, t_shard=None):
        """Bind the program to a device arena and the packed weights.  A program with collective ops (T-sharded
        forward) is bound together with the T group's communicator: its exchanges then run inside the library (RCCL on
        the launch stream) — or, with T2V_COLLECTIVES=host / a non-GPU group, through parallel.ShardedExecutor."""
        if self.bound is not None and self.arena is not None and self.arena.device == device:
            return
        # zero-filled once at bind time: padding lanes that an op reads before any op wrote them (they only ever meet
        # zero weights) must not hold NaN bit patterns of recycled allocator blocks
        self.arena = torch.zeros(self.prog.arena.high + 256, dtype=torch.uint8, device=device)
        wptr = {k: v.data_ptr() for k, v in packed.items()}
        st = torch.cuda.current_stream(device).cuda_stream       # the bind-time reset of the sync words is ordered with the first run
        if any(op.kind in COLLECTIVE_KINDS for op in self.prog.ops):
            if t_shard is None:
                raise L.T2VError("a T-sharded program needs the T group (UNetSD.t_shard)")
            comm = t_shard.communicator(device)
            if comm is not None:
                self.bound = BoundProgram(self.prog, self.arena.data_ptr(), wptr, comm=comm, stream=st)
            else:
                from .parallel import ShardedExecutor
                self.bound = ShardedExecutor(self.prog, self.arena, t_shard,
                                             lambda ops: BoundProgram(self.prog, self.arena.data_ptr(), wptr, ops=ops))
        else:
            self.bound = BoundProgram(self.prog, self.arena.data_ptr(), wptr, stream=st)


class ProgramHost:
    """See the module docstring.  A mixin beside nn.Module (the owner calls `_init_programs()` in its constructor), or an object of its
    own for programs whose images are tables that read no parameter."""

    def __init__(self, max_programs: Optional[int] = 4):
        self._init_programs(max_programs)

    def _init_programs(self, max_programs: Optional[int] = 4, fingerprint: bool = False):
        self._programs: Dict[tuple, _Compiled] = {}          # key (geometry + lowering options) -> program, oldest first
        self._packed: Optional[Dict[str, torch.Tensor]] = None
        self._packed_sig = None
        self._packed_device = None
        self._packed_deps = None          # image name -> state-dict keys its recipe read
        self.max_programs = max_programs  # programs kept (each owns a device arena); None = unbounded
        # byte-level values of the parameters at the last pack (`verify_weights`); None: this host keeps none
        self._fingerprint = pk.ParamFingerprint() if fingerprint else None

    # ---- programs -------------------------------------------------------------------------
    def _program(self, key, build: Callable[[], _Compiled]) -> _Compiled:
        comp = self._programs.get(key)
        if comp is None:
            comp = self._programs[key] = build()
            self._evict_programs(keep=key)
        return comp

    def _evict_programs(self, keep):
        """Least-recently-compiled eviction: a webui session that varies frames / resolution / batch_count would otherwise
        accumulate one arena per geometry (the reference frees its activations after every call)."""
        while self.max_programs is not None and len(self._programs) > self.max_programs:
            victim = next(k for k in self._programs if k != keep)
            del self._programs[victim]

    # ---- parameters -----------------------------------------------------------------------
    def _param_module(self):
        """The module whose parameters the images are packed from: the owner itself; None for a parameterless host."""
        return self if isinstance(self, torch.nn.Module) else None

    def _named_params(self) -> list:
        m = self._param_module()
        return list(m.named_parameters()) if m is not None else []

    def _state_dict(self) -> dict:
        m = self._param_module()
        return m.state_dict() if m is not None else {}

    def _param_signature(self) -> dict:
        """name -> (identity, version, device, dtype, shape) of every parameter: what a pack is valid for."""
        return {n: (id(p), p._version, p.device.type, p.dtype, p.shape) for n, p in self._named_params()}

    # ---- the pack -------------------------------------------------------------------------
    def invalidate(self):
        """Drop the packed weight images (call after mutating parameters in place)."""
        self._packed = None
        self._packed_sig = None

    def _ensure_packed(self, comp: _Compiled, device):
        """The images of `comp` are packed on `device` from the parameters as they are now.  An owner that keeps fingerprints calls
        `verify_weights` first (ClipTextTower.__call__ does): packing missing images records the fingerprints of ALL parameters
        again, which would hide an earlier edit through `.data` from the images already packed."""
        device = torch.device(device)
        sig = self._param_signature()
        if self._packed is None or sig != self._packed_sig or device != self._packed_device:
            self._packed, self._packed_deps = {}, {}
            self._packed_sig, self._packed_device = sig, device
            for c in self._programs.values():
                c.bound = None
        if self._pack_missing(comp, device):
            self._record_fingerprints(device)

    def _pack_missing(self, comp: _Compiled, device) -> int:
        """Images a program needs that no earlier program declared: packed and merged into the live set (existing device
        tensors — and the programs bound to them — are untouched).  -> the number of images packed."""
        missing = [r for r in comp.packer.recipes if r[0] not in self._packed]
        if missing:
            tmp = pk.WeightPacker()
            for n, d, f in missing:
                tmp.add(n, d, f)
            self._packed.update(tmp.materialise(self._state_dict(), device))
            self._packed_deps.update(tmp.deps)
        return len(missing)

    def _record_fingerprints(self, device, values=None):
        """End of a full or partial pack: the parameters' fingerprints as of now (None when they are not fingerprinted)."""
        fp = self._fingerprint
        if fp is not None:
            fp.recorded = values if values is not None else fp.compute(self._named_params(), device)

    def verify_weights(self, device=None) -> list:
        """Look at the BYTES of the parameters: fingerprint every tensor (one launch, packing.ParamFingerprint), compare with the values
        recorded when the images were last packed -> the changed names; any such edit drops the pack (`_bytes_changed`), and the run
        that follows packs again.  This is what sees an edit through `.data` (`w.data += d`, `w.data = saved.clone()`: the reference's
        VideoCrafter LoRA loaders), which moves neither the parameter's identity nor its version.  Does nothing for a host that keeps
        no fingerprints, nothing before the first pack, and nothing for parameters that live on the CPU while the pack is on a GPU
        (they are not fingerprinted: `invalidate()` is the call for that arrangement)."""
        device = torch.device(device) if device is not None else self._packed_device
        fp = self._fingerprint
        if fp is None or self._packed is None or device is None or device != self._packed_device or fp.recorded is None:
            return []
        fresh = fp.compute(self._named_params(), device)
        if fresh is None:
            return []
        changed = [n for n, v in fresh.items() if fp.recorded.get(n) != v]
        if changed:
            self._bytes_changed(device, changed, fresh)
        return changed

    def _bytes_changed(self, device, changed: list, fingerprints: dict):
        self.invalidate()
        self._fingerprint.recorded = None

    # ---- run ------------------------------------------------------------------------------
    def _prepare(self, comp: _Compiled, device):
        """Pack what `comp` still misses and bind it — before the caller allocates the tensors of this run: pack, arena, outputs
        is the order in which the device memory of a first run is taken."""
        self._ensure_packed(comp, device)
        comp.ensure_bound(self._packed, device)

    def _launch(self, comp: _Compiled, device, ext: Dict[int, int]):
        """Run a prepared program on the current stream."""
        comp.ensure_bound(self._packed, device)
        comp.bound.run(ext, torch.cuda.current_stream(device).cuda_stream)
