"""Developer tool: split.SplitTable.search (every iteration of the train/test plot split search in one launch) vs the host
definition search_np on the same table; the results are compared exactly before anything is timed.

    python tools/splitbench.py [--calls 20] [--host-iterations 2048] [--out FILE]

Three workloads: 100 000 iterations at (C = 64 candidate plots, S = 200 species), 100 000 at (2048, 256), and the
reference's own setting, 100 iterations at (64, 200).  The tables are seeded: some 40 individuals a plot spread over the
species, so most species are too rare to complete and a walk ends late or not at all (`mean_last_test_position`).
Each workload is timed three ways, to see where the time goes:
    search          the call as it is used: hash, sort, walk with the early exit, the best
    given_orders    the same orders handed in as an array: no hash and no sort (at the large shape on 8192 iterations,
                    beside `search_at_orders_iterations`, the hashed search of as many)
    no_early_exit   min_test so large that no species completes: the walk visits every candidate and takes every plot
The device time is the median of `calls` stream-event timings after a warm-up, the table resident.  search_np is timed on
the first `host-iterations` iterations (it costs minutes at the large shape) and reported per iteration; those iterations
are the ones compared exactly.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeptreeattention_amd import _lib, split  # noqa: E402

WORKLOADS = ((100000, 64, 200), (100000, 2048, 256), (100, 64, 200))


def workload(C, S, seed=0):
    """Columns of a table with C candidate plots of C + C // 8 + 1, about 40 single-row individuals a plot, the species
    drawn from a long-tailed distribution."""
    rng = np.random.default_rng(seed)
    plots = C + C // 8 + 1
    share = rng.gamma(0.5, 1.0, S) + 0.02
    n = 40 * plots
    taxon = np.concatenate([np.arange(S), rng.choice(S, n - S, p=share / share.sum())])      # every species somewhere
    plot = np.concatenate([np.arange(plots), rng.integers(0, plots, n - plots)])             # every plot holds something
    rng.shuffle(plot)
    return {"individual": np.arange(n), "plot": plot, "taxon": taxon, "fixed": rng.uniform(size=n) < 0.1, "candidate": plot < C}


def timed(fn, calls):
    for _ in range(3):
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
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}


def entry(table, iterations, orders, out, min_train=5, min_test=3):
    """dta_split_search itself on a checked `orders`: SplitTable.search copies a device `orders` back for its permutation
    check on every call, which is host time between the two events."""
    floor = np.ascontiguousarray(table.floor(min_test))
    _lib.check(_lib.lib().dta_split_search(
        _lib.ptr(table.rows_dev), _lib.ptr(table.totals_dev), table.n_candidates, table.n_species,
        floor.ctypes.data_as(_lib.c_double_p), min_train, min_test, iterations, 0, 0, _lib.ptr(orders), _lib.ptr(out.species),
        _lib.ptr(out.train_rows), _lib.ptr(out.test_plots), _lib.ptr(out.best), None, None, _lib.current_stream_ptr()),
        "dta_split_search")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-iterations", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "splitbench needs the MI355X"
    dev = torch.device("cuda:0")
    rows = []
    for iterations, C, S in WORKLOADS:
        table = split.SplitTable.from_columns(**workload(C, S), device=dev)
        assert table.n_candidates == C and table.n_species == S
        n_host = min(iterations, a.host_iterations if C <= 64 else a.host_iterations // 8)
        t0 = time.perf_counter()
        want = split.search_np(table, n_host, seed=1)
        host_s = time.perf_counter() - t0
        got = table.search(n_host, seed=1, membership=True, taxa=True)
        for name in ("species", "train_rows", "test_plots", "membership", "taxa"):
            assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), "device and host disagree: " + name
        assert tuple(got.best.cpu().tolist()) == want.best
        n_orders = iterations if C <= 64 else 8192        # (100 000 x 2048 orders would be 800 MB)
        orders = torch.from_numpy(split.order_np(C, np.arange(n_orders), seed=1)).to(dev)
        # position of the last test plot in the order: where the early exit, if any, ends the walk
        last = [int(np.flatnonzero(want.membership[t][split.order_np(C, t, seed=1)])[-1]) + 1 for t in range(min(n_host, 256))]
        out = table.search(iterations, seed=1)
        keep = split.SplitSearch(out.species, out.train_rows, out.test_plots, out.best, None, None)
        res = {"iterations": iterations, "candidates": C, "species": S, "plots": table.n_plots, "rows": int(len(table.individual)),
               "search": timed(lambda: table.search(iterations, seed=1, out=keep), a.calls),
               "no_early_exit": timed(lambda: table.search(iterations, seed=1, min_test=10 ** 6, out=keep), a.calls)}
        if iterations == n_orders:
            res["given_orders"] = timed(lambda: entry(table, iterations, orders, keep), a.calls)
        else:
            small = split.SplitSearch(out.species[:n_orders], out.train_rows[:n_orders], out.test_plots[:n_orders], out.best, None, None)
            res["orders_iterations"] = n_orders
            res["search_at_orders_iterations"] = timed(lambda: table.search(n_orders, seed=1, out=small), a.calls)
            res["given_orders"] = timed(lambda: entry(table, n_orders, orders, small), a.calls)
        best = out.best.cpu().tolist()
        res.update({"host_iterations": n_host, "host_search_np_s": round(host_s, 3),
                    "host_ms_per_iteration": round(host_s * 1e3 / n_host, 4),
                    "device_us_per_iteration": round(res["search"]["ms_median"] * 1e3 / iterations, 4),
                    "speedup_over_host_per_iteration": round(host_s / n_host / (res["search"]["ms_median"] * 1e-3 / iterations), 1),
                    "mean_test_plots": round(float(want.test_plots.mean()), 2), "mean_last_test_position": round(float(np.mean(last)), 2),
                    "best": best, "best_of_first_100": split.search_np(table, min(100, n_host), seed=1).best[1:3]})
        rows.append(res)
    line = json.dumps({"workload": "split.SplitTable.search: train/test plot split search, one wavefront per iteration, one launch",
                       "cases": rows, "calls": a.calls, "exact_match_with_host": True,
                       "build_id": _lib.lib().dta_build_id().decode()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
