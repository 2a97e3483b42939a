"""The per-step operand registry: which low-precision copy of an fp32 tensor a kernel reads.

Pure bookkeeping over storage pointers, offsets and sizes -- no kernel is launched from here and only torch is imported,
so all of it runs on CPU tensors (tests/test_operands_cpu.py).

One `Record` per fp32 storage, found by `untyped_storage().data_ptr()`.  A record holds a reference to an fp32 tensor of
that storage (`owner`), so the storage cannot be recycled while the record lives; a kernel that writes INTO an existing
tensor drops that tensor's record (`touch`, O(1)), `clear()` drops all of them.

* The bf16 twin and the producer-recorded amax pair belong to the WHOLE storage: they are registered only for a tensor
  at offset 0 that covers its storage.  A batch slice of such a tensor reads the same slice of the flat twin; the amax
  pair answers only for the whole tensor (`storage_amax` is the one reader that lets a slice share it).
* The fp8 copy and the two gradient bundles are made per request and are specific to (offset, numel) -- the fp8 copy
  also to `relu`, the bundles and the stand-alone amax pair to the pointer of their per-sample scale (0: no scale).
  Every entry keyed by a scale holds a reference to the scale tensor, so its address names it for as long as the entry
  lives.  The CONTENTS are not part of the key: a per-sample scale tensor must not be rewritten within a step, because the
  copies made with its old factors are keyed by its address and would be found again.
* A ghost mark (one set of storage pointers, `ghosts`): the fp32 tensor is a never-written handle; its consumers must
  read the copies.

Safety cap: a new record past MAX_RECORDS (512) clears ALL records first -- ghost marks and the only copy of an
operand-only result included (a step registers far fewer; the cap bounds a caller that never calls new_step()).

The registry also owns the two other per-step stores of the low-precision and Winograd paths: the per-stream pool of
amax slots and the forward launches' kept Winograd input transforms."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

MAX_RECORDS = 512
MAX_KEPT = 256
AMAX_POOL_FLOATS = 2048


@dataclass(slots=True)
class Amax:
    pair: torch.Tensor                  # {max |t|, max |scale t|}, written by the producing conv's epilogue
    scale_ptr: int                      # the scale element 1 belongs to (0: none)
    scale: Optional[torch.Tensor] = None    # (kept alive: a freed scale's address could be handed to another [B] tensor)


@dataclass(slots=True)
class Fp8Copy:
    data: torch.Tensor                  # e4m3 bytes of relu?(t) * 448 / amax
    amax: torch.Tensor                  # [1]


@dataclass(slots=True)
class GradBf16:
    scale: Optional[torch.Tensor]       # (kept alive: its pointer is part of the key)
    data: torch.Tensor                  # bf16 copy of scale[b] * dy[b]
    colsum: Optional[torch.Tensor]      # fp32 column sums of it


@dataclass(slots=True)
class GradFp8:
    scale: Optional[torch.Tensor]
    data: Optional[torch.Tensor]        # e5m2 bytes of scale[b] * dy[b] * 57344 / amax
    amax: torch.Tensor                  # [1] = amax2[1:2]
    colsum: Optional[torch.Tensor]
    amax2: torch.Tensor                 # {max |dy|, max |scale dy|}


@dataclass(slots=True)
class Record:
    owner: torch.Tensor
    bf16: Optional[torch.Tensor] = None                 # the flat twin of the whole storage
    amax: Optional[Amax] = None
    fp8: Dict[tuple, Fp8Copy] = field(default_factory=dict)             # (relu, offset, numel) ->
    grad_bf16: Dict[tuple, GradBf16] = field(default_factory=dict)      # (scale_ptr, offset, numel) ->
    grad_fp8: Dict[tuple, GradFp8] = field(default_factory=dict)        # (scale_ptr, offset, numel) ->
    amax2: Dict[tuple, torch.Tensor] = field(default_factory=dict)      # (scale_ptr, offset, numel) -> stand-alone amax pair
    amax2_scale: Dict[tuple, torch.Tensor] = field(default_factory=dict)    # (the scales of those keys, kept alive; not counted)

    def count(self) -> int:
        return (self.bf16 is not None) + (self.amax is not None) + len(self.fp8) + len(self.grad_bf16) + len(self.grad_fp8) + len(self.amax2)


@dataclass(slots=True)
class KeptTransform:
    x: torch.Tensor                     # the forward launch's input [B,H,W,K]
    relu_in: bool
    tile: int
    V: torch.Tensor                     # its transform, [(tile + 2)^2 planes][plane_rows][K]
    plane_rows: int
    stream: int                         # raw handle of the stream V was written on


def whole(t: torch.Tensor) -> bool:
    return t.storage_offset() == 0 and t.numel() * 4 == t.untyped_storage().nbytes()


def _by_scale(t: torch.Tensor, scale) -> tuple:
    return (0 if scale is None else scale.data_ptr(), t.storage_offset(), t.numel())


class Registry:
    def __init__(self):
        self._records: Dict[int, Record] = {}
        self.ghosts = set()             # THE ghost mark: storage pointers of the never-written fp32 handles (each has a record, which
                                        # keeps its storage alive); ops._p tests membership per pointer argument, and only while there is one
        self._amax_pool = {}            # raw stream handle -> [buffer, next free float]: a pool is zeroed and handed out on ONE stream
        self._kept: Dict[int, KeptTransform] = {}
        self.keeping = False            # inside a step: forward Winograd launches keep their input transform

    # ---- records
    def find(self, t: torch.Tensor) -> Optional[Record]:
        return self._records.get(t.untyped_storage().data_ptr())

    def record(self, t: torch.Tensor) -> Record:
        k = t.untyped_storage().data_ptr()
        r = self._records.get(k)
        if r is None:
            if len(self._records) > MAX_RECORDS:
                self.clear()
            r = self._records[k] = Record(t)
        return r

    def touch(self, t: Optional[torch.Tensor]) -> None:
        """A kernel is about to write into t: every copy of its storage is stale."""
        if t is not None and (self._records or self._kept):
            k = t.untyped_storage().data_ptr()
            self._kept.pop(k, None)
            self._records.pop(k, None)
            self.ghosts.discard(k)

    def clear(self) -> None:
        self._records.clear()
        self.ghosts.clear()

    def drop_copies(self) -> None:
        """Every copy goes (the conv dtype changed mid-step); the ghost marks stay, each with an empty record that keeps its storage
        alive: a never-written handle remains one, so its consumers fail loudly instead of reading it as fp32."""
        self._records = {k: Record(r.owner) for k, r in self._records.items() if k in self.ghosts}

    def new_step(self, keep_transforms: bool) -> None:
        self.clear()
        self._amax_pool.clear()
        self._kept.clear()
        self.keeping = keep_transforms

    def end_step(self) -> None:
        self._kept.clear()
        self.keeping = False

    def count(self) -> int:
        return len(self.ghosts) + sum(r.count() for r in self._records.values())

    # ---- ghost mark
    def mark_ghost(self, t: torch.Tensor) -> None:
        self.record(t)
        self.ghosts.add(t.untyped_storage().data_ptr())

    def is_ghost(self, t: torch.Tensor) -> bool:
        return t.untyped_storage().data_ptr() in self.ghosts

    # ---- whole-storage copies
    def put_bf16(self, t: torch.Tensor, t16: torch.Tensor) -> None:
        if whole(t):
            self.record(t).bf16 = t16.view(-1)

    def get_bf16(self, t: torch.Tensor) -> Optional[torch.Tensor]:
        r = self._records.get(t.untyped_storage().data_ptr())
        if r is None or r.bf16 is None:
            return None
        off = t.storage_offset()
        return r.bf16[off:off + t.numel()].view(t.shape)

    def put_amax(self, t: torch.Tensor, pair: torch.Tensor, scale) -> None:
        if whole(t):
            self.record(t).amax = Amax(pair, 0 if scale is None else scale.data_ptr(), scale)

    def get_amax(self, t: torch.Tensor, scale=None, need_scaled: bool = False) -> Optional[torch.Tensor]:
        """The producer-recorded amax pair of a WHOLE tensor, or None.  need_scaled: element 1 must belong to `scale`."""
        r = self._records.get(t.untyped_storage().data_ptr())
        if r is None or r.amax is None or not whole(t):
            return None
        if need_scaled and r.amax.scale_ptr != (0 if scale is None else scale.data_ptr()):
            return None
        return r.amax.pair

    def storage_amax(self, t: torch.Tensor) -> Optional[torch.Tensor]:
        """The amax pair recorded for t's storage, whichever part of it t is (a batch slice shares the whole tensor's scale)."""
        r = self._records.get(t.untyped_storage().data_ptr())
        return None if r is None or r.amax is None else r.amax.pair

    # ---- per-slice copies
    def get_fp8(self, t: torch.Tensor, relu: bool) -> Optional[Fp8Copy]:
        r = self._records.get(t.untyped_storage().data_ptr())
        return None if r is None else r.fp8.get((bool(relu), t.storage_offset(), t.numel()))

    def put_fp8(self, t: torch.Tensor, relu: bool, data, amax) -> Fp8Copy:
        e = self.record(t).fp8[(bool(relu), t.storage_offset(), t.numel())] = Fp8Copy(data, amax)
        return e

    def get_grad_bf16(self, t: torch.Tensor, scale) -> Optional[GradBf16]:
        r = self._records.get(t.untyped_storage().data_ptr())
        return None if r is None else r.grad_bf16.get(_by_scale(t, scale))

    def put_grad_bf16(self, t: torch.Tensor, scale, data, colsum) -> GradBf16:
        e = self.record(t).grad_bf16[_by_scale(t, scale)] = GradBf16(scale, data, colsum)
        return e

    def get_grad_fp8(self, t: torch.Tensor, scale) -> Optional[GradFp8]:
        r = self._records.get(t.untyped_storage().data_ptr())
        return None if r is None else r.grad_fp8.get(_by_scale(t, scale))

    def put_grad_fp8(self, t: torch.Tensor, scale, data, amax, colsum, amax2) -> GradFp8:
        e = self.record(t).grad_fp8[_by_scale(t, scale)] = GradFp8(scale, data, amax, colsum, amax2)
        return e

    def get_amax2(self, t: torch.Tensor, scale) -> Optional[torch.Tensor]:
        r = self._records.get(t.untyped_storage().data_ptr())
        return None if r is None else r.amax2.get(_by_scale(t, scale))

    def put_amax2(self, t: torch.Tensor, scale, pair: torch.Tensor) -> torch.Tensor:
        r, k = self.record(t), _by_scale(t, scale)
        r.amax2[k] = pair
        if scale is not None:
            r.amax2_scale[k] = scale
        return pair

    # ---- amax slots
    def amax_slot(self, stream: int, device) -> torch.Tensor:
        """Two zeroed floats (max |t|, max |scale t|) from a per-step, per-stream pool: ONE memset launch per 1024 convolutions.
        (A pool's slots are written by that stream's conv epilogues and read by that stream's conversion kernels, or behind a join.)"""
        pool = self._amax_pool.get(stream)
        if pool is None or pool[1] + 2 > pool[0].numel() or pool[0].device != device:
            pool = self._amax_pool[stream] = [torch.zeros(AMAX_POOL_FLOATS, device=device), 0]
        pool[1] += 2
        return pool[0][pool[1] - 2:pool[1]]

    # ---- kept Winograd input transforms
    def keep(self, x: torch.Tensor, relu_in: bool, tile: int, V: torch.Tensor, plane_rows: int, stream: int) -> None:
        if len(self._kept) > MAX_KEPT:
            self._kept.clear()
        self._kept[x.untyped_storage().data_ptr()] = KeptTransform(x, bool(relu_in), tile, V, plane_rows, stream)

    def kept_count(self) -> int:
        return len(self._kept)

    def kept(self, x: torch.Tensor, relu_in: bool, tile: int) -> Optional[Tuple[KeptTransform, int]]:
        """-> (the kept transform of x or of the batch x is a slice of, the row of x's first tile in every plane) or None"""
        e = self._kept.get(x.untyped_storage().data_ptr())
        if e is None or e.relu_in != relu_in or e.tile != tile or e.x.shape[1:] != x.shape[1:]:
            return None
        per = x.shape[1] * x.shape[2] * x.shape[3]
        off = x.storage_offset() - e.x.storage_offset()
        if off < 0 or off % per or off // per + x.shape[0] > e.x.shape[0]:
            return None
        return e, (off // per) * (x.shape[1] // tile) * (x.shape[2] // tile)
