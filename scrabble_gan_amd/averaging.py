"""The averaged generator: an exponential moving average of G's weights, BatchNorm statistics re-estimated for those
weights, and the per-epoch sample sheet.

BigGAN-family generators are trained with beta_1 = 0 and evaluated from an average of their iterates; the last Adam iterate
that `train()` saves is noisy.  Nothing here feeds back into training: the average is a second flat buffer beside
`model.store.flat`, updated by one sweep after each step (csrc/averaging.hip through ops).

    avg = WeightAverage(G, decay=0.9999)
    ...train_step(...); avg.update()                        # every step
    with avg.applied():                                      # G's parameter views now show the averaged weights
        standing_statistics(avg, batches)                    # BN moving statistics for THOSE weights (kept in avg)
    with avg.applied():
        sheet = sample_sheet(G, style, labels)               # uint8 [rows*(32+pad)-pad, cols*(16L+pad)-pad]

`applied()` exchanges the two buffers in place (no second copy of G) and exchanges them back on exit; the packed / transposed /
Winograd-domain filter copies ops caches per weight tensor are dropped on both sides (ops.weights_changed)."""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import ops
from .legibility import preserved_rng
from .nn import LOCAL


def ema_coefficient(t: int, decay: float, start_step: int = 0, warmup: bool = True) -> float:
    """1 - decay_t of update number `t` (0-based), in double.  Before `start_step` the average IS the live weights (1).  With
    `warmup` the decay is min(decay, (1 + t') / (10 + t')), t' = t - start_step -- tf.train.ExponentialMovingAverage(num_updates):
    early averages are not dominated by the initial weights."""
    if t < start_step:
        return 1.0
    d = float(decay)
    if warmup:
        tp = t - start_step
        d = min(d, (1.0 + tp) / (10.0 + tp))
    return 1.0 - d


class WeightAverage:
    """Exponential moving average of `model.store.flat` in one fp32 buffer of the same size (initialised as a copy)."""

    def __init__(self, model, decay: float = 0.9999, start_step: int = 0, warmup: bool = True):
        if not 0.0 <= decay <= 1.0:
            raise ValueError("decay must be in [0, 1], got %r" % (decay,))
        self.model = model
        self.decay, self.start_step, self.warmup = float(decay), int(start_step), bool(warmup)
        self.flat = model.store.flat.clone()
        self.t = 0
        self.standing: Optional[torch.Tensor] = None       # BN moving statistics for the averaged weights (layout of store.state)
        self._applied = False

    def update(self) -> None:
        """One sweep on the launch stream: flat += (1 - decay_t) (weights - flat)."""
        if self._applied:
            raise RuntimeError("update() inside applied(): the model's buffer holds the average")
        ops.ema_update(self.flat, self.model.store.flat, ema_coefficient(self.t, self.decay, self.start_step, self.warmup))
        self.t += 1

    @contextlib.contextmanager
    def applied(self):
        """The model computes with the averaged weights (and the standing statistics, once computed; the live moving
        statistics until then).  On exit -- also when the body raises -- weights and BN state are bitwise what they were."""
        if self._applied:
            raise RuntimeError("applied() is not re-entrant")
        store = self.model.store
        live_state = store.state.clone()
        ops.swap_buffers(store.flat, self.flat)
        if self.standing is not None:
            store.state.copy_(self.standing)
        ops.weights_changed()
        self._applied = True
        try:
            yield self.model
        finally:
            self._applied = False
            store.state.copy_(live_state)
            ops.swap_buffers(store.flat, self.flat)
            ops.weights_changed()

    def standing_named(self) -> Dict[str, torch.Tensor]:
        """The standing statistics by variable name (views of the kept buffer); {} before standing_statistics ran."""
        if self.standing is None:
            return {}
        store = self.model.store
        out = {}
        for name in store.names:
            if not store.trainable[name]:
                o, shape = store._off[name], store.shapes[name]
                out[name] = self.standing[o:o + store.p[name].numel()].view(shape)
        return out

    def export(self) -> Dict[str, torch.Tensor]:
        """The averaged model in the layout of `store.export()` (what `save_weights` writes): CPU tensors by name."""
        with self.applied():
            return self.model.store.export()

    def save_weights(self, prefix: str) -> None:
        with self.applied():
            self.model.save_weights(prefix)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {"flat": self.flat.detach().cpu().clone(), "t": torch.tensor([self.t], dtype=torch.int64)}
        if self.standing is not None:
            out["standing"] = self.standing.detach().cpu().clone()
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        if sd["flat"].numel() != self.flat.numel():
            raise ValueError("averaged buffer of %d elements, the model has %d" % (sd["flat"].numel(), self.flat.numel()))
        self.flat.copy_(sd["flat"].reshape(-1).to(self.flat.device, torch.float32))
        self.t = int(sd["t"].reshape(-1)[0])
        self.standing = None
        if "standing" in sd:
            self.standing = sd["standing"].reshape(-1).to(self.flat.device, torch.float32).clone()


def standing_statistics(avg: WeightAverage, batches: Iterable, nl: Optional[dict] = None) -> None:
    """Inside `avg.applied()`: moving mean / variance of every BatchNorm of G := the mean over `batches` of the batch mean and
    of the batch variance times count / (count - 1) -- the quantities the training path feeds to the moving-statistics update,
    with momentum i / (i + 1) for batch i instead of 0.99 (momentum 0 on the first batch overwrites the old value).
    `batches`: (style, labels) pairs.  The result is kept in `avg` (installed by later `applied()` blocks); the live model's
    statistics come back on exit.  Statistics are local to this process whatever `model.reducer` is: only rank 0 evaluates, and
    a collective there would wait for ranks that never join.  `nl` = {"G.style": ..., "G.up": ...} gives explicit NonLocalBlock
    kernels; every generator the passes draw from is put back afterwards, so training draws what it would have drawn anyway."""
    if not avg._applied:
        raise RuntimeError("standing_statistics runs inside `with avg.applied():`")
    model = avg.model
    nl = nl or {}
    reducer = model.reducer
    model.reducer = LOCAL
    n = 0
    try:
        with preserved_rng(model):
            for i, (style, labels) in enumerate(batches):
                model.forward(style, labels, nl.get("G.style"), nl.get("G.up"), training=True, momentum=i / (i + 1.0))
                n += 1
    finally:
        model.reducer = reducer
        ops.new_step()              # operand copies (bf16 / fp8 modes) of these passes are released
        ops.end_step()
    if n:
        avg.standing = model.store.state.clone()


def sample_sheet(generator, style, labels, cols: int = 4, pad: int = 2) -> np.ndarray:
    """Inference-mode G([style, labels]) laid out as a uint8 sheet on the device (ops.image_sheet_u8): word i in cell
    (i // cols, i % cols), white gutters.  One device-to-host copy."""
    with preserved_rng(generator):
        img = generator([style, labels], training=False)
    return ops.image_sheet_u8(img, cols, pad).cpu().numpy()
