"""Host side of the averaged generator that needs no GPU: the command line, the coefficient schedule, and the keys of the full
training state with and without an average."""
import random

import numpy as np
import pytest
import torch


def test_main_parses_the_averaging_flags():
    from scrabble_gan_amd.main import build_parser
    ap = build_parser()
    off = ap.parse_args([])
    assert (off.ema_decay, off.ema_start, off.ema_standing_batches, off.samples_every) == (0.0, 0, 0, 0)     # everything off by default
    on = ap.parse_args(["--synthetic", "--ema-decay", "0.9999", "--ema-start", "1000", "--ema-standing-batches", "16",
                        "--samples-every", "5", "--legibility-every", "2"])
    assert on.ema_decay == 0.9999 and on.ema_start == 1000 and on.ema_standing_batches == 16 and on.samples_every == 5
    assert on.legibility_every == 2 and on.synthetic
    with pytest.raises(SystemExit):
        ap.parse_args(["--ema-decay", "much"])


def test_train_takes_the_averaging_arguments_with_everything_off_by_default():
    import inspect
    from scrabble_gan_amd.data_utils import train
    sig = inspect.signature(train).parameters
    assert [sig[k].default for k in ("ema_decay", "ema_start", "ema_standing_batches", "samples_every")] == [0.0, 0, 0, 0]


def test_coefficient_schedule():
    from scrabble_gan_amd.averaging import ema_coefficient
    # before start_step the average is the live weights; then TensorFlow's num_updates rule min(decay, (1 + t') / (10 + t'))
    got = [ema_coefficient(t, 0.999, start_step=2, warmup=True) for t in range(5)]
    assert got[:2] == [1.0, 1.0]
    assert got[2:] == pytest.approx([1 - 1 / 10, 1 - 2 / 11, 1 - 3 / 12], rel=1e-15)
    # the warm-up hands over to the decay itself once (1 + t') / (10 + t') exceeds it: t' = 8990 for 0.999
    assert ema_coefficient(8990, 0.999) == pytest.approx(1 - 8991 / 9000, rel=1e-12)
    assert ema_coefficient(8992, 0.999) == 1 - 0.999
    assert [ema_coefficient(t, 0.9, warmup=False) for t in (0, 7)] == [1 - 0.9] * 2
    assert ema_coefficient(3, 0.9, start_step=4, warmup=False) == 1.0
    # computed in double: 1 - 0.9999 keeps its digits (in fp32 the subtraction keeps only half of them)
    assert ema_coefficient(10 ** 6, 0.9999) == pytest.approx(1e-4, rel=1e-12)
    assert abs(float(np.float32(1) - np.float32(0.9999)) - 1e-4) > 1e-10


class _Store:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.names = ["a.w", "a.b", "bn.mm"]
        self.trainable = {"a.w": True, "a.b": True, "bn.mm": False}
        self.shapes = {"a.w": (3, 4), "a.b": (4,), "bn.mm": (4,)}
        self._off = {"a.w": 0, "a.b": 12, "bn.mm": 0}
        self.flat = torch.randn(16, generator=g)
        self.state = torch.randn(4, generator=g)
        self.p = {"a.w": self.flat[0:12].view(3, 4), "a.b": self.flat[12:16], "bn.mm": self.state[0:4]}

    def export(self):
        return {k: v.clone() for k, v in self.p.items()}

    def load(self, weights):
        for k, v in weights.items():
            self.p[k].copy_(v.reshape(self.p[k].shape))


class _Model:
    def __init__(self, seed):
        self.store = _Store(seed)
        self.nl_gen = torch.Generator().manual_seed(seed)


class _Opt:
    def __init__(self):
        self.iterations = 3

    def flat_state(self, store):
        return {"m": torch.zeros_like(store.flat), "iterations": torch.tensor([self.iterations])}

    def load_flat_state(self, store, d):
        self.iterations = int(d["iterations"][0])


def test_training_state_keys_with_and_without_an_average(tmp_path):
    from safetensors.torch import load_file
    from scrabble_gan_amd import data_utils as DU
    from scrabble_gan_amd.averaging import WeightAverage
    models, opts = [_Model(i) for i in range(4)], [_Opt() for _ in range(4)]
    plain = str(tmp_path / "plain.safetensors")
    DU.save_training_state(plain, *models, *opts, epoch_idx=1, batch_idx=2)
    old_keys = {"position"} | {"%s/%s" % (t, k) for t in "GDRS" for k in ("a.w", "a.b", "bn.mm")} | \
               {"%s.opt/%s" % (t, k) for t in "GDRS" for k in ("m", "iterations")}
    assert set(load_file(plain)) == old_keys                # without `averages` the file has exactly the keys it always had

    avg = WeightAverage(models[0], decay=0.9)
    avg.flat.mul_(0.5)
    avg.t = 7
    with_avg = str(tmp_path / "avg.safetensors")
    DU.save_training_state(with_avg, *models, *opts, epoch_idx=1, batch_idx=2, averages={"G": avg})
    assert set(load_file(with_avg)) == old_keys | {"G.ema/flat", "G.ema/t"}
    avg.standing = torch.arange(4.0)
    full = str(tmp_path / "full.safetensors")
    random.seed(5)
    np.random.seed(6)
    DU.save_training_state(full, *models, *opts, epoch_idx=1, batch_idx=2, averages={"G": avg}, streams=True)
    st = load_file(full)
    assert set(st) == old_keys | {"G.ema/flat", "G.ema/t", "G.ema/standing", "rng/random", "rng/random.gauss", "rng/numpy",
                                  "rng/numpy.gauss"} | {"rng/%s.nl_gen" % t for t in "GDRS"}
    expect = (random.random(), np.random.rand(), torch.rand(2, generator=models[0].nl_gen))     # what the run would draw next

    fresh, fresh_opts = [_Model(10 + i) for i in range(4)], [_Opt() for _ in range(4)]
    avg2 = WeightAverage(fresh[0], decay=0.9)
    random.seed(99)
    np.random.seed(98)
    assert DU.load_training_state(full, *fresh, *fresh_opts, averages={"G": avg2}, streams=True) == (1, 2)
    assert torch.equal(avg2.flat, avg.flat) and avg2.t == 7 and torch.equal(avg2.standing, avg.standing)
    assert torch.equal(fresh[0].store.flat, models[0].store.flat)
    got = (random.random(), np.random.rand(), torch.rand(2, generator=fresh[0].nl_gen))
    assert got[0] == expect[0] and got[1] == expect[1] and torch.equal(got[2], expect[2])
    # a state written without an average: the average restarts from the loaded weights, the streams stay where they are
    avg3 = WeightAverage(fresh[0], decay=0.9)
    avg3.flat.zero_()
    assert DU.load_training_state(plain, *fresh, *fresh_opts, averages={"G": avg3}, streams=True) == (1, 2)
    assert torch.equal(avg3.flat, fresh[0].store.flat) and avg3.t == 0
