"""Developer tool: canopy.CanopyRaster.crown_height (one launch pair for all crowns of a tile) on a resident CHM raster vs
the host mirror crown_height_np + min_height_np, on the same input; the two results are compared exactly before anything is
timed.

    python tools/canopybench.py [--crowns 100000] [--large 10] [--size 1000] [--calls 20] [--out FILE]

The workload: `crowns` boxes with sides of 3-25 cells anywhere on a size x size raster (some hang over its edges) plus
`large` boxes of 300 x 300, heights of 0-40 m (0-2.4 m in the left three tenths) with NaN, nodata and sub-floor cells;
q = 99, floor 0.5, MinHeight(3).  The
device time is the median of `calls` stream-event timings after a warm-up, boxes resident; the host time one run of the
mirror.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, canopy  # noqa: E402


def workload(crowns, large, size, seed=0):
    rng = np.random.default_rng(seed)
    chm = (rng.random((size, size), dtype=np.float32) * np.float32(40.0)).astype(np.float32)
    chm[:, :size * 3 // 10] *= np.float32(0.06)                # a strip of low vegetation: under 2.4 m, MinHeight(3) drops it
    r = rng.random((size, size))
    chm[r < 0.02] = np.nan
    chm[(r >= 0.02) & (r < 0.04)] = -9999.0
    chm[(r >= 0.04) & (r < 0.10)] = 0.0
    r0 = rng.integers(-5, size - 5, crowns)
    c0 = rng.integers(-5, size - 5, crowns)
    small = np.stack([r0, c0, r0 + rng.integers(3, 26, crowns), c0 + rng.integers(3, 26, crowns)], 1)
    br, bc = rng.integers(0, size - 299, large), rng.integers(0, size - 299, large)
    big = np.stack([br, bc, br + 300, bc + 300], 1)
    boxes = np.concatenate([small, big]).astype(np.int32)
    return chm, boxes[rng.permutation(len(boxes))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crowns", type=int, default=100000)
    ap.add_argument("--large", type=int, default=10)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "canopybench needs the MI355X"
    dev = torch.device("cuda:0")
    chm, boxes = workload(a.crowns, a.large, a.size)
    rule = canopy.MinHeight(3.0)

    t0 = time.perf_counter()
    height, count = canopy.crown_height_np(chm, boxes)
    keep = canopy.min_height_np(height, rule.m)
    host_s = time.perf_counter() - t0

    ras = canopy.CanopyRaster(chm, device=dev)
    dboxes = torch.from_numpy(boxes).to(dev)
    got = ras.crown_height(dboxes, rule=rule)
    nan = torch.isnan(got.height).cpu()
    assert torch.equal(nan, torch.from_numpy(np.isnan(height))), "device and host disagree (NaN heights)"
    assert torch.equal(got.height.cpu()[~nan].view(torch.int32), torch.from_numpy(height)[~nan].view(torch.int32)), "device and host disagree (height)"
    assert torch.equal(got.count.cpu(), torch.from_numpy(count)) and torch.equal(got.keep.cpu(), torch.from_numpy(keep)), "device and host disagree"

    for _ in range(5):
        ras.crown_height(dboxes, rule=rule)
    torch.cuda.synchronize()
    times = []
    for _ in range(max(a.calls, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ras.crown_height(dboxes, rule=rule)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    _, _, rows, cols = canopy.clip_boxes(boxes, a.size, a.size)
    area = rows * cols
    wave = area <= canopy.WAVE_CELLS
    # cells read: a wave's crown once; a workgroup's crown in four histogram passes, five when the hi-th value needs its own
    cells_wave, cells_block = int(area[wave].sum()), int(area[~wave].sum())
    res = {"workload": "canopy.crown_height: CHM q99 per crown box + MinHeight(3), one launch pair",
           "crowns": int(len(boxes)), "large_boxes": a.large, "raster": [a.size, a.size], "kept_share": round(float(keep.mean()), 3),
           "device_ms_median": round(ms, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
           "calls": len(times), "host_mirror_s": round(host_s, 3), "speedup_over_host": round(host_s * 1e3 / ms, 1),
           "crowns_per_s": round(len(boxes) / (ms * 1e-3), 0), "cells_in_wave_crowns": cells_wave,
           "cells_in_block_crowns": cells_block, "cells_read_at_least": cells_wave + 4 * cells_block,
           "exact_match_with_host": True, "build_id": _lib.lib().dta_build_id().decode()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
