"""Developer tool: mosaic.mosaic (shift, exact greedy NMS by cells and parallel rounds, pixel boxes; dta_mosaic) vs the host
definition mosaic.nms_np / pixel_boxes_np on the same boxes; the results are compared exactly before anything is timed.

    python tools/mosaicbench.py [--side 27] [--extent 10000] [--trees 83000] [--dense 4] [--calls 20] [--host-only] [--out FILE]

The workload: a tile of side x side detector windows (27: 10,000 x 10,000 px, 729 windows) over a tree scene
(tests/mosaic_cases.py: scene) -- about 10^5 boxes at 83,000 trees, the overlap strips holding the same tree twice or four
times -- and the same tile at `dense` times the trees.  Per scene: the device time per call (median of `calls` stream-event
timings after a warm-up, inputs resident), its split -- rounds=0 without the tail launch (shift, binning and the winner pass),
the default rounds without the tail launch, the whole call -- the boxes still undecided after r = 0 .. 16 rounds, and one run
of nms_np + pixel_boxes_np on the host.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import mosaic_cases as MC  # noqa: E402
from deeptreeattention_amd import _lib, mosaic as M  # noqa: E402


def timed(fn, calls):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(calls, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}


def measure(side, extent, trees, seed, calls, host_only):
    c = MC.scene(side, trees, seed, extent=extent)
    n = len(c["boxes"])
    t0 = time.perf_counter()
    status, winner, tile = M.nms_np(**MC.nms_args(c))
    pixel = M.pixel_boxes_np(tile, c["height"], c["width"])
    host_s = time.perf_counter() - t0
    cell, gx, gy = M.grid(n, c["height"], c["width"], c["max_side"])
    res = {"tile": [c["height"], c["width"]], "windows": int(len(c["origins"])), "trees": trees, "boxes": n,
           "kept": int((status == 1).sum()), "dropped": int((status == 0).sum()), "cell": cell, "cells": [gx, gy],
           "boxes_per_cell_mean": round(n / (gx * gy), 1), "host_nms_np_s": round(host_s, 3)}
    if host_only:
        return res
    import torch
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("boxes", "scores", "window", "origins")}

    def call(**kw):
        return M.mosaic(d["boxes"], d["scores"], d["window"], d["origins"], height=c["height"], width=c["width"],
                        max_side=c["max_side"], **kw)
    m = call()
    assert np.array_equal(m.status.cpu().numpy(), status) and np.array_equal(m.winner.cpu().numpy(), winner), "device and host disagree"
    assert np.array_equal(m.boxes.cpu().numpy().view(np.uint32), tile.view(np.uint32)), "device and host disagree (boxes)"
    assert np.array_equal(m.pixel_boxes.cpu().numpy(), pixel), "device and host disagree (pixel boxes)"
    left = [int((call(rounds=r, tail=False).status == M.UNDECIDED).sum().item()) for r in range(17)]
    res["undecided_after_rounds"] = left
    res["rounds_needed"] = int(next((r for r, v in enumerate(left) if v == 0), -1))
    res["device_call"] = timed(call, calls)
    res["device_rounds0_no_tail"] = timed(lambda: call(rounds=0, tail=False), calls)
    res["device_one_round_no_tail"] = timed(lambda: call(rounds=1, tail=False), calls)
    res["device_default_rounds_no_tail"] = timed(lambda: call(tail=False), calls)
    full, bins, rounds = (res[k]["ms_median"] for k in ("device_call", "device_rounds0_no_tail", "device_default_rounds_no_tail"))
    res["split_ms"] = {"shift_bin_winner": bins, "rounds": round(rounds - bins, 4), "tail": round(full - rounds, 4)}
    res["speedup_over_host"] = round(host_s * 1e3 / full, 1)
    res["boxes_per_s"] = round(n / (full * 1e-3), 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=27)
    ap.add_argument("--extent", type=int, default=10000)
    ap.add_argument("--trees", type=int, default=83000)
    ap.add_argument("--dense", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.host_only:
        import torch
        assert torch.cuda.is_available(), "mosaicbench needs the MI355X (or --host-only)"
    res = {"workload": "mosaic.mosaic: detector boxes of all windows of a tile -> crown boxes (shift, exact greedy NMS, pixel boxes)",
           "default_rounds": M.ROUNDS, "scene": measure(a.side, a.extent, a.trees, 1, a.calls, a.host_only),
           "scene_dense": measure(a.side, a.extent, a.trees * a.dense, 2, a.calls, a.host_only),
           "calls": max(a.calls, 20), "exact_match_with_host": not a.host_only, "build_id": _lib.lib().dta_build_id().decode()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
