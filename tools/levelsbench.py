"""Time levels.build on the GPU: the device chain alone (dta_level_build into outputs that stay), the whole call (the host
definition, the launch, a synchronise) and the host definition alone, at two table sizes.

    python tools/levelsbench.py [--out profiles/levelsbench.json]

The chain is timed by a pair of stream events around a block of calls, read after the block; the figure is the median
over the blocks per call, the spread the lowest and highest block.  `enqueue_ms` is the host clock around the same calls
without a synchronise: what the host spends to put a chain on the stream."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import levels_cases as LC  # noqa: E402
from deeptreeattention_amd import _lib, levels as LV  # noqa: E402

SIZES = ((20000, 50000), (3000, 6000))
BLOCKS, PER_BLOCK = 20, 25


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    assert torch.cuda.is_available(), "levelsbench needs a GPU"
    dev = torch.device("cuda:0")
    result = {"build_id": _lib.lib().dta_build_id().decode(), "sizes": []}
    for n, records in SIZES:
        table, rules = LC.synthetic(n, seed=8, records=records)
        config = LC.CONFIG
        first = LV.build(table, rules, config, True, seed=1, epoch=0, device=dev)
        LC.same(first, first.host, True)
        cfg = LV._config(config)
        out = LV._out_struct(*first._buffers)
        need = int(_lib.lib().dta_level_workspace_bytes(table.N, table.R, rules.C, table.Y))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        tab, rul = table.resident(dev), rules.resident(dev)

        def chain(epoch):
            LV._launch(tab, rul, None, cfg, True, 1, epoch, out, ws, table.N, table.R, rules.C, table.Y)
        for e in range(10):
            chain(e)
        torch.cuda.synchronize()
        device_ms, enqueue_ms = [], []
        for b in range(BLOCKS):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record()
            for k in range(PER_BLOCK):
                chain(b * PER_BLOCK + k)
            stop.record()
            enqueue_ms.append((time.perf_counter() - t0) * 1e3 / PER_BLOCK)
            torch.cuda.synchronize()
            device_ms.append(start.elapsed_time(stop) / PER_BLOCK)
        whole_ms, host_ms = [], []
        for e in range(12):
            t0 = time.perf_counter()
            LV.build(table, rules, config, True, seed=1, epoch=e, device=dev, into=None)
            torch.cuda.synchronize()
            whole_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            LV.build_np(table, rules, config, True, seed=1, epoch=e)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        row = {"individuals": table.N, "records": table.R, "species": rules.C, "years": table.Y, "kept": first.n,
               "chain_ms": statistics.median(device_ms), "chain_ms_blocks": [min(device_ms), max(device_ms)],
               "enqueue_ms": statistics.median(enqueue_ms),
               "build_ms": statistics.median(whole_ms[2:]), "build_ms_range": [min(whole_ms[2:]), max(whole_ms[2:])],
               "build_np_ms": statistics.median(host_ms[2:]), "build_np_ms_range": [min(host_ms[2:]), max(host_ms[2:])],
               "blocks": BLOCKS, "calls_per_block": PER_BLOCK}
        print(json.dumps(row), flush=True)
        result["sizes"].append(row)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
