"""Developer tool: what feeds the multi-stage train step.  The per-level loaders of loop.SyntheticTreeDataset with
training_step_all(present=None) -- 15 index selects, one host read of the selection per level and the dta_year_flags read of
the whole batch per step -- against treedata.LevelViews.batches with training_step_all(year_flags=): one gather launch per
step that also sets the flags.

    python tools/feedbench.py [--n 2048] [--blocks 20] [--block-steps 50] [--out FILE]

5 levels x 3 years, 369 bands, 11 x 11, B = 128, bf16 models, `n` individuals per level; both routes read the SAME crops
(the pool is built from the synthetic data sets' tensors) and train a model of their own from the same start.  After a
warm-up epoch of each route, blocks of `block-steps` steps ALTERNATE between the routes in the same call.  Every step is
timed with a pair of stream events around "produce the batch, enqueue the step" (read after the block, so the host may run
ahead where the route lets it); a route's figure is the median over all its steps, its spread the lowest and highest block
median.  Then the gather launch alone (dta_pool_batches into fixed outputs; it reads and writes levels x years x B x 178,596
bytes each way) and dta_epoch_order at n = 20,000 x 5 levels and at the largest n it takes.  One JSON line."""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, treedata  # noqa: E402
from deeptreeattention_amd.engine import MultiStageTrainer  # noqa: E402
from deeptreeattention_amd.loop import SyntheticTreeDataset  # noqa: E402
from deeptreeattention_amd.year import learned_ensemble  # noqa: E402

CLASSES, YEARS, BANDS, SIZE, B = [2, 2, 12, 7, 5], 3, 369, 11, 128


def trainer(dev):
    torch.manual_seed(5)
    ms = []
    for c in CLASSES:
        m = learned_ensemble(YEARS, c, {"pretrain_state_dict": None, "bands": BANDS}).to(dev).train()
        for net in m.year_models:
            net.precision = "bf16"
        ms.append(m)
    return MultiStageTrainer(ms, [1e-4] * len(CLASSES))


def parent_steps(tr, data):
    """The parent's route, a step at a time: every level's loader (shuffled, a new seed per epoch) and the step on them."""
    for epoch in itertools.count():
        its = [d.loader(B, True, seed=epoch) for d in data]
        for i in range(len(data[0]) // B):
            yield tr.training_step_all([next(it) for it in its], i)


def new_steps(tr, levels):
    for epoch in itertools.count():
        for i, (batch, flags) in enumerate(levels.batches(B, True, seed=epoch)):
            yield tr.training_step_all(batch, i, year_flags=flags)


def block(gen, steps):
    ev = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        next(gen)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def summary(blocks):
    per_block = [float(np.median(b)) for b in blocks]
    every = [t for b in blocks for t in b]
    return {"ms_per_step_median": round(float(np.median(every)), 4), "block_median_min": round(min(per_block), 4),
            "block_median_max": round(max(per_block), 4), "steps": len(every), "seconds": round(sum(every) * 1e-3, 2)}


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "calls": calls}


def gather_alone(levels, dev, calls):
    """dta_pool_batches itself on the first step of a shuffled epoch, into outputs that stay."""
    L = _lib.lib()
    pool, nl = levels.pool, len(levels)
    per = pool.bands * pool.size * pool.size
    orders = treedata.epoch_order([len(v) for v in levels], 0, 0, None, dev)
    outs = [torch.empty(B, pool.bands, pool.size, pool.size, device=dev) for _ in range(nl * pool.n_years)]
    ints = torch.empty(nl, 2, B, dtype=torch.int64, device=dev)
    banks = torch.zeros(2, nl * pool.n_years, device=dev)
    lv = (_lib.PoolLevel * nl)(*[_lib.PoolLevel(orders[l].data_ptr(), v.rows.data_ptr(), v.labels.data_ptr(), len(v), 0, B, 1,
                                                 ints[l, 0].data_ptr(), ints[l, 1].data_ptr()) for l, v in enumerate(levels)])
    op = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    code = _lib.DTA_F32 if pool.dtype == torch.float32 else _lib.DTA_BF16
    k = [0]

    def call():
        k[0] ^= 1
        _lib.check(L.dta_pool_batches(_lib.ptr(pool.data), code, pool.n, pool.n_years, pool.bands, pool.size, nl, lv, op,
                                      _lib.ptr(banks[k[0]]), _lib.ptr(banks[k[0] ^ 1]), _lib.current_stream_ptr()), "dta_pool_batches")
    t = timed(call, calls, warm=10)
    written = nl * pool.n_years * B * per * 4
    read = nl * pool.n_years * B * per * pool.data.element_size()
    t.update(bytes_read=read, bytes_written=written, tb_per_s=round((read + written) / (t["ms_median"] * 1e-3) / 1e12, 3))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--block-steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "feedbench needs the MI355X"
    assert a.n % B == 0, "n must be a multiple of the batch size: every step is then one launch chain on both routes"
    dev = torch.device("cuda:0")
    data = [SyntheticTreeDataset(a.n, BANDS, c, size=SIZE, years=YEARS, missing=0.1, seed=l, device=dev) for l, c in enumerate(CLASSES)]
    crops = torch.cat([torch.stack(d.hsi, dim=1) for d in data])               # [5 n][Y][C][S][S]: the same crops, once
    res = {"workload": "feed of the multi-stage train step: 5 levels x 3 years, 369 x 11 x 11, B = 128, bf16 models",
           "individuals_per_level": a.n, "build_id": _lib.lib().dta_build_id().decode()}
    for name, dtype in (("pool_float32", torch.float32), ("pool_bfloat16", torch.bfloat16)):
        pool = treedata.CropPool(crops, device=dev, dtype=dtype)
        levels = treedata.LevelViews([pool.view(torch.arange(l * a.n, (l + 1) * a.n), d.labels, train=True) for l, d in enumerate(data)])
        old, new = trainer(dev), trainer(dev)
        routes = {"parent_loaders_present_none": parent_steps(old, data), "level_views_year_flags": new_steps(new, levels)}
        for g in routes.values():
            block(g, a.n // B)                                                  # warm-up: an epoch, every shape
        assert old.batched_last and new.batched_last
        blocks = {k: [] for k in routes}
        for _ in range(a.blocks):
            for k, g in routes.items():
                blocks[k].append(block(g, a.block_steps))
        res[name] = {k: summary(v) for k, v in blocks.items()}
        res[name]["gather_alone"] = gather_alone(levels, dev, 200)
        res[name]["pool_bytes"] = pool.data.numel() * pool.data.element_size()
        del pool, levels, old, new, routes
    del crops, data
    torch.cuda.empty_cache()
    res["epoch_order_20000_x_5"] = timed(lambda: treedata.epoch_order([20000] * 5, 1, 0, None, dev), 20)
    res["epoch_order_max_n_x_1"] = timed(lambda: treedata.epoch_order([treedata.MAX_N], 1, 0, None, dev), 3, warm=1)
    res["epoch_order_max_n_x_5"] = timed(lambda: treedata.epoch_order([treedata.MAX_N] * 5, 1, 0, None, dev), 3, warm=1)
    res["epoch_order_max_n"] = treedata.MAX_N
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
