"""Developer tool: stems.CrownBoxes.assign (field stems to crown boxes: join, nearest box, one stem per box; three launches,
the box table resident) vs the host definition stems.assign_np on the same input; the results are compared exactly before
anything is timed.

    python tools/stemsbench.py [--calls 20] [--out FILE]

Two shapes, one JSON line each:
    plots   2,000 plots of 40 m with 150 boxes of 3-15 m and 30 stems each, a tenth of the stems measured twice
    tile    ONE plot of 1 km with 100,000 boxes and 5,000 stems: what a caller gets who makes a whole tile one plot (every
            stem walks every box of the plot)
`assign` is the whole call with resident inputs (the sort of the stems by plot, the three launches, the way back to the
caller's order); `kernels` is dta_stems_assign alone on tables that are already sorted.  The device time is the median of
`calls` stream-event timings after a warm-up; the host time one run of the definition."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, stems  # noqa: E402

UTM = (4.0e5, 3.3e6)


def workload(plots, boxes, points, cell, seed=0):
    rng = np.random.default_rng(seed)
    org = np.stack([UTM[0] + 2 * cell * (np.arange(plots) % 64), UTM[1] + 2 * cell * (np.arange(plots) // 64)], axis=1)
    low, side = rng.uniform(0.0, cell - 15.0, (plots, boxes, 2)), rng.uniform(3.0, 15.0, (plots, boxes, 2))
    b = np.concatenate([org[:, None] + low, org[:, None] + low + side], axis=2).reshape(-1, 4)
    p = org[:, None] + rng.uniform(0.0, cell, (plots, points, 2))
    twice = rng.random((plots, points)) < 0.1
    p[twice] = p[:, :1].repeat(points, axis=1)[twice]                  # onto the plot's first stem
    n = plots * points
    height = np.where(rng.random(n) < 0.25, np.nan, np.round(rng.uniform(2.0, 40.0, n)))
    chm = np.where(rng.random(n) < 0.2, np.nan, np.round(rng.uniform(2.0, 40.0, n) * 2) / 2)
    return dict(boxes=np.ascontiguousarray(b), box_plot=np.repeat(np.arange(plots), boxes), points=np.ascontiguousarray(p.reshape(-1, 2)),
                point_plot=np.repeat(np.arange(plots), points), height=height, chm=chm, plots=plots)


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


def run(name, w, calls, dev):
    t0 = time.perf_counter()
    want = stems.assign_np(w["boxes"], w["box_plot"], w["points"], w["point_plot"], w["height"], w["chm"], 1.0, w["plots"])
    host_s = time.perf_counter() - t0
    table = stems.CrownBoxes(w["boxes"], w["box_plot"], w["plots"], device=dev)
    d = {k: torch.from_numpy(w[k]).to(dev) for k in ("points", "point_plot", "height", "chm")}
    got = table.assign(d["points"], d["point_plot"], d["height"], d["chm"])
    assert np.array_equal(got.box.cpu().numpy(), want.box) and np.array_equal(got.status.cpu().numpy(), want.status), \
        "device and host disagree"
    assert np.array_equal(got.crowns.cpu().numpy(), want.crowns, equal_nan=True), "device and host disagree (crowns)"
    whole = timed(lambda: table.assign(d["points"], d["point_plot"], d["height"], d["chm"]), calls)
    # the C entry alone: the workload is sorted by plot as it is
    n, m = len(w["points"]), len(w["boxes"])
    codes = d["point_plot"].to(torch.int32)
    start = torch.searchsorted(d["point_plot"], torch.arange(w["plots"] + 1, device=dev)).to(torch.int32)
    choice = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    crowns = torch.empty((n, 4), dtype=torch.float64, device=dev)
    L = _lib.lib()

    def kernels():
        _lib.check(L.dta_stems_assign(_lib.ptr(table.boxes), _lib.ptr(table.box_start), m, _lib.ptr(d["points"]), _lib.ptr(codes),
                                      _lib.ptr(start), _lib.ptr(d["height"]), _lib.ptr(d["chm"]), n, w["plots"], 1.0,
                                      _lib.ptr(choice), _lib.ptr(status), _lib.ptr(crowns), _lib.current_stream_ptr()),
                   "dta_stems_assign")
    alone = timed(kernels, calls)
    assert np.array_equal(status.cpu().numpy(), want.status)
    return {"workload": "stems.CrownBoxes.assign: field stems to crown boxes, " + name, "plots": w["plots"], "boxes": m, "stems": n,
            "status_counts": np.bincount(want.status, minlength=5).tolist(), "assign_device": whole, "kernels_device": alone,
            "host_assign_np_s": round(host_s, 3), "assign_speedup_over_host": round(host_s * 1e3 / whole["ms_median"], 1),
            "stems_per_s": round(n / (whole["ms_median"] * 1e-3), 0), "calls": max(calls, 20), "exact_match_with_host": True,
            "build_id": L.dta_build_id().decode()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stemsbench needs the MI355X"
    dev = torch.device("cuda:0")
    lines = [json.dumps(run("2,000 plots x 150 boxes x 30 stems", workload(2000, 150, 30, 40.0), a.calls, dev)),
             json.dumps(run("one plot of 100,000 boxes x 5,000 stems", workload(1, 100000, 5000, 1000.0), a.calls, dev))]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
