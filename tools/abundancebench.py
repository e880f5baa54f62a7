"""Developer tool: abundance.resample (every iteration in one launch) on a resident prediction vs the host mirror
resample_np, on the same input; the two results are compared exactly before anything is timed.

    python tools/abundancebench.py [--crowns 1000000] [--species 200] [--iterations 100] [--calls 30] [--out FILE]

Scores come from Beta(4, 1) (mean 0.8), so about a fifth of the draws search the table.  The device time is the median of
`calls` stream-event timings after a warm-up; the host time one run of resample_np.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, abundance  # noqa: E402

ITER_GROUP = 8      # AB_G (csrc/abundance.hip): iterations that share one read of a crown


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crowns", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "abundancebench needs the MI355X"
    dev = torch.device("cuda:0")
    N, S, T = a.crowns, a.species, a.iterations
    rng = np.random.default_rng(0)
    conf = rng.integers(0, 30, (S, S)) * (rng.random((S, S)) < 0.1) + np.eye(S, dtype=np.int64) * rng.integers(20, 200, S)
    table = abundance.sampling_table(conf)
    label = rng.integers(0, S, N).astype(np.int64)
    label[rng.random(N) < 0.01] = -1
    score = rng.beta(4.0, 1.0, N).astype(np.float32)
    mask = rng.random(N) < 0.95

    t0 = time.perf_counter()
    want = abundance.resample_np(label, score, table, T, seed=1, mask=mask)
    host_s = time.perf_counter() - t0

    dl, ds, dm = (torch.from_numpy(x).to(dev) for x in (label, score, mask))
    dt = abundance.device_table(table, dev)
    got = abundance.resample(dl, ds, dt, T, seed=1, mask=dm)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), "device and host disagree"
    searched = 1.0 - float(np.mean(np.where(np.isnan(score), 1.0, np.clip(score, 0, 1))))

    for _ in range(5):
        abundance.resample(dl, ds, dt, T, seed=1, mask=dm)
    torch.cuda.synchronize()
    times = []
    for _ in range(max(a.calls, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        abundance.resample(dl, ds, dt, T, seed=1, mask=dm)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    groups = -(-T // ITER_GROUP)
    read_bytes = 13 * N * groups           # label 8 B + score 4 B + mask 1 B per crown per iteration group
    res = {"workload": "abundance.resample: confusion resampling of predicted crowns, all iterations in one launch",
           "crowns": N, "species": S, "iterations": T, "share_of_draws_that_search": round(searched, 3),
           "device_ms_median": round(ms, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
           "calls": len(times), "host_resample_np_s": round(host_s, 3), "speedup_over_host": round(host_s * 1e3 / ms, 1),
           "iteration_groups": groups, "bytes_read_per_call": read_bytes,
           "implied_read_GBps": round(read_bytes / (ms * 1e-3) / 1e9, 1),
           "draws_per_s": round(N * T / (ms * 1e-3), 0), "exact_match_with_host": True,
           "build_id": _lib.lib().dta_build_id().decode()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
