"""Time ONE validation epoch of a MultiStage model both ways on the same box, in the same process (developer script; bench.py
is the flagship yardstick and is not involved).

    python tools/valbench.py [--levels 5] [--years 3] [--bands 369] [--batch 128] [--batches 40] [--epochs 7] [--precision bf16]

  leg A: the validation loop of loop.fit_multistage as it stands without metrics -- per level and batch one eval-mode forward
         chain, one loss launch and a host-issued torch.softmax (MultiStageTrainer.validation_step), then the mean of the
         batch losses read back per level;
  leg B: loop.validate_multistage -- per batch ONE chain over all levels with ONE epilogue launch (loss, softmax, top-2,
         metric counts), then one device-to-host copy of the accumulators.
Both legs see the same batches (a few distinct ones, cycled, resident on the device).  Timed with events around the epoch,
after warm-up epochs; prints one JSON line with the medians, min / max and the kernel launches per batch of each leg."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class CycledBatches:
    """A `.loader(batch_size)` over `count` batches that cycles through a few distinct ones."""

    def __init__(self, distinct, count):
        self.distinct, self.count = distinct, count

    def loader(self, batch_size, shuffle=False, seed=0, drop_last=False):
        for i in range(self.count):
            yield self.distinct[i % len(self.distinct)]


def leg_a(trainer, data, batch_size):
    """fit_multistage's validation half (metrics=False), statement for statement."""
    models = [t.model for t in trainer.levels]
    was = [bool(m.training) for m in models]
    for m in models:
        m.eval()
    try:
        vl = []
        for l, d in enumerate(data):
            out = [trainer.validation_step(b, i, l)["val_loss"].reshape(()).float() for i, b in enumerate(d.loader(batch_size))]
            vl.append(float(torch.stack(out).mean()))
    finally:
        for m, w in zip(models, was):
            if w:
                m.train()
    return vl


def leg_b(trainer, data, batch_size):
    from deeptreeattention_amd.loop import validate_multistage
    return [m["val_loss"] for m in validate_multistage(trainer, data, batch_size)]


def timed(fn, epochs, warmup):
    ms, last = [], None
    for e in range(warmup + epochs):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        last = fn()
        b.record()
        torch.cuda.synchronize()
        if e >= warmup:
            ms.append(a.elapsed_time(b))
    return ms, last


def launches(fn):
    """Kernel launches of one call, counted by the profiler; None where it cannot see them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "emcpy" not in ev.name and "emset" not in ev.name)
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--years", type=int, default=3)
    ap.add_argument("--bands", type=int, default=369)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.engine import MultiStageTrainer
    from deeptreeattention_amd.year import learned_ensemble
    dev = torch.device("cuda:0")
    classes = [2, 2, 12, 7, 5, 9, 4, 3][:a.levels]
    torch.manual_seed(0)
    models = []
    for c in classes:
        m = learned_ensemble(a.years, c, {"pretrain_state_dict": None, "bands": a.bands}).to(dev).train()
        for net in m.year_models:
            net.precision = a.precision
        models.append(m)
    trainer = MultiStageTrainer(models, [1e-4] * a.levels)
    data = []
    for c in classes:
        distinct = [(None, {"HSI": [torch.rand(a.batch, a.bands, 11, 11, device=dev) for _ in range(a.years)]},
                     torch.randint(0, c, (a.batch,), device=dev)) for _ in range(a.distinct)]
        data.append(CycledBatches(distinct, a.batches))
    res = {"shape": vars(a), "build": _lib.lib().dta_build_id().decode()}
    for name, fn in (("A_level_by_level", lambda: leg_a(trainer, data, a.batch)), ("B_validate_multistage", lambda: leg_b(trainer, data, a.batch))):
        ms, loss = timed(fn, a.epochs, a.warmup)
        res[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "val_loss": loss}
    one = [CycledBatches(d.distinct, 1) for d in data]
    na, nb = launches(lambda: leg_a(trainer, one, a.batch)), launches(lambda: leg_b(trainer, one, a.batch))
    res["launches_per_batch"] = {"A": na, "B": nb}
    sa, sb = res["A_level_by_level"], res["B_validate_multistage"]
    res["spread_ms"] = max(sa["max_ms"] - sa["min_ms"], sb["max_ms"] - sb["min_ms"])
    res["B_not_slower_than_A_beyond_spread"] = sb["median_ms"] <= sa["median_ms"] + res["spread_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
