"""Developer tool: boundary.Boundary.clip on crown boxes and Boundary.rasterise (one launch each, the edge table resident)
vs the host mirrors boxes_np / rasterise_np on the same input; the results are compared exactly before anything is timed.

    python tools/boundarybench.py [--crowns 1000000] [--edges 2048] [--size 1000] [--calls 20] [--out FILE]

The workload: a star-shaped boundary of `edges` edges in all (an exterior ring and a hole of an eighth of them) at UTM
magnitudes; `crowns` pixel boxes of 3-25 m on a 0.1 m grid over the square around it, roughly a third of them outside; a
size x size rasterise of 1 m cells over that square.  The raster is timed twice: dta_boundary_raster (the
edges that straddle a row compacted per workgroup) and the plain per-cell loop, which is Boundary.contains on the size x size
cell centres.  The device time is the median of `calls` stream-event timings after a warm-up, queries resident; the host time
one run of the mirror.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, boundary  # noqa: E402

UTM = (4.0e5, 3.3e6)


def star(n, cx, cy, r_in, r_out, rng):
    ang = 2 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
    rad = np.where(np.arange(n) % 2 == 0, r_out, r_in) * rng.uniform(0.9, 1.0, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def workload(crowns, edges, size, seed=0):
    rng = np.random.default_rng(seed)
    half = size / 2.0
    cx, cy = UTM[0] + half, UTM[1] + half
    hole = max(3, edges // 8)
    rings = [star(edges - hole, cx, cy, 0.88 * half, 0.95 * half, rng), star(hole, cx, cy, 0.08 * half, 0.16 * half, rng)[::-1]]
    # crown boxes on a 0.1 m grid, their first corner anywhere on the size x size square around the boundary
    a = 0.1
    t = (UTM[0], a, UTM[1] + size, -a)
    cells = int(size / a)
    r0, c0 = rng.integers(0, cells, crowns), rng.integers(0, cells, crowns)
    side = (rng.uniform(3.0, 25.0, (crowns, 2)) / a).astype(np.int64)
    boxes = np.stack([r0, c0, r0 + side[:, 0], c0 + side[:, 1]], axis=1).astype(np.int32)
    raster_t = (UTM[0], 1.0, UTM[1] + size, -1.0)
    return rings, boxes, t, raster_t


def timed(fn, calls):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crowns", type=int, default=1000000)
    ap.add_argument("--edges", type=int, default=2048)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "boundarybench needs the MI355X"
    dev = torch.device("cuda:0")
    rings, boxes, t, raster_t = workload(a.crowns, a.edges, a.size)
    table = boundary.edge_table(rings)

    t0 = time.perf_counter()
    code = boundary.boxes_np(table, pixel_boxes=boxes, transform=t)
    host_boxes_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    mask = boundary.rasterise_np(table, a.size, a.size, raster_t)
    host_raster_s = time.perf_counter() - t0

    site = boundary.Boundary(rings, device=dev)
    dboxes = torch.from_numpy(boxes).to(dev)
    centres = torch.from_numpy(boundary.cell_centres(a.size, a.size, raster_t)).to(dev)
    assert torch.equal(site.boxes(pixel_boxes=dboxes, transform=t).cpu(), torch.from_numpy(code)), "device and host disagree (boxes)"
    assert torch.equal(site.clip(pixel_boxes=dboxes, transform=t).cpu(), torch.from_numpy((code != 0).astype(np.uint8)))
    assert torch.equal(site.rasterise(a.size, a.size, raster_t).cpu(), torch.from_numpy(mask)), "device and host disagree (raster)"
    assert torch.equal(site.contains(centres).cpu(), torch.from_numpy(mask.reshape(-1))), "device and host disagree (cell centres)"

    clip = timed(lambda: site.clip(pixel_boxes=dboxes, transform=t), a.calls)
    codes = timed(lambda: site.boxes(pixel_boxes=dboxes, transform=t), a.calls)
    raster = timed(lambda: site.rasterise(a.size, a.size, raster_t), a.calls)
    plain = timed(lambda: site.contains(centres), a.calls)
    res = {"workload": "boundary.clip: crown pixel boxes against a site boundary, one launch; boundary.rasterise: cell centres",
           "crowns": int(len(boxes)), "edges": int(site.n_edges), "raster": [a.size, a.size],
           "share_outside": round(float((code == 0).mean()), 3), "share_on_the_line": round(float((code == 1).mean()), 3),
           "share_inside": round(float((code == 2).mean()), 3), "cells_inside": int(mask.sum()),
           "clip_device": clip, "boxes_device": codes, "host_boxes_np_s": round(host_boxes_s, 3),
           "clip_speedup_over_host": round(host_boxes_s * 1e3 / clip["ms_median"], 1),
           "crowns_per_s": round(len(boxes) / (clip["ms_median"] * 1e-3), 0),
           "box_edge_tests_per_s": round(len(boxes) * site.n_edges / (codes["ms_median"] * 1e-3), 0),
           "raster_device_compacted": raster, "raster_device_plain_per_cell": plain, "host_rasterise_np_s": round(host_raster_s, 3),
           "raster_speedup_over_host": round(host_raster_s * 1e3 / raster["ms_median"], 1),
           "calls": max(a.calls, 20), "exact_match_with_host": True, "build_id": _lib.lib().dta_build_id().decode()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
