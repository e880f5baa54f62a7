"""Developer tool: abundance.resample (every iteration in one launch) on a resident prediction vs the host mirror
resample_np, on the same input; the two results are compared exactly before anything is timed.

    python tools/abundancebench.py [--crowns 1000000] [--species 200] [--iterations 100] [--calls 30] [--out FILE]
                                   [--grouped 80,8000] [--loop-cells 200] [--rounds 5] [--grouped-out FILE]

Scores come from Beta(4, 1) (mean 0.8), so about a fifth of the draws search the table.  The device time is the median of
`calls` stream-event timings after a warm-up; the host time one run of resample_np.  Prints one JSON line.

--grouped G[,G...]: then the same crowns per tile or map cell (abundance.resample(group=, groups=G), every cell equally
likely, 2 % of the crowns outside the grid), one more JSON line per G.  Compared exactly with resample_np(group=) first.
Timed: the call with the ordering (torch.sort) included, and its three stream operations alone (the C entry on crowns
ordered beforehand, buffers allocated beforehand); today's route, the loop of G masked ungrouped calls
`resample(mask=mask & (cell == g))` on the same tensors -- the two alternate in blocks in one process, `rounds` blocks each,
and above `loop-cells` cells the loop runs over the first `loop-cells` cells only and is scaled to G, which the line says;
G = 1 against the ungrouped call; summary_device on the grouped table against the read-back and the host summary."""
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


def timed(fn, calls):
    """Median / min / max of `calls` stream-event timings of fn(), in ms."""
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def grouped(a, G, label, score, mask, table, dl, ds, dm, dt, host_ungrouped_s, ungrouped_ms):
    dev = dl.device
    N, S, T = a.crowns, a.species, a.iterations
    rng = np.random.default_rng(G)
    cell = rng.integers(0, G, N).astype(np.int64)
    cell[rng.random(N) < 0.02] = -1
    dc = torch.from_numpy(cell).to(dev)
    print("grouped G={}: the NumPy definition ...".format(G), file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    want = abundance.resample_np(label, score, table, T, seed=1, mask=mask, group=cell, groups=G)
    host_s = time.perf_counter() - t0
    got = abundance.resample(dl, ds, dt, T, seed=1, mask=dm, group=dc, groups=G)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), "device and host disagree"
    del want

    def call():
        return abundance.resample(dl, ds, dt, T, seed=1, mask=dm, group=dc, groups=G, out=got)

    # the stream operations alone: crowns ordered and buffers allocated beforehand
    L = _lib.lib()
    gs, order = torch.sort(dc, stable=True)
    nbytes = L.dta_abundance_grouped_workspace_bytes(N, S, T, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dm8 = dm.view(torch.uint8)

    def launches():
        _lib.check(L.dta_abundance_resample_grouped(_lib.ptr(dl), _lib.ptr(ds), _lib.ptr(dm8), _lib.ptr(gs), _lib.ptr(order), N, G,
                                                    _lib.ptr(dt), S, T, 1, 0, _lib.ptr(got), _lib.ptr(ws), nbytes,
                                                    _lib.current_stream_ptr()), "dta_abundance_resample_grouped")

    # today's route: one masked ungrouped call per cell, the mask formed on the device
    loop_cells = min(G, a.loop_cells)
    one = torch.empty(T, S + 1, dtype=torch.int64, device=dev)

    def loop():
        for g in range(loop_cells):
            abundance.resample(dl, ds, dt, T, seed=1, mask=dm & (dc == g), out=one)

    for fn in (call, launches, loop):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(one, got[:, loop_cells - 1])
    print("grouped G={}: timing ...".format(G), file=sys.stderr, flush=True)
    blocks = {"call": [], "loop": []}
    for _ in range(a.rounds):                 # the two routes alternate in blocks
        blocks["call"].append(timed(call, 5)[0])
        blocks["loop"].append(timed(loop, 1)[0])
    call_ms, loop_ms = float(np.median(blocks["call"])), float(np.median(blocks["loop"])) * G / loop_cells
    launch_ms = timed(launches, max(a.calls, 20))
    sort_ms = timed(lambda: torch.sort(dc, stable=True), max(a.calls, 20))
    res = {"workload": "abundance.resample(group=, groups=G): the resampled counts per tile or map cell in one call",
           "crowns": N, "species": S, "iterations": T, "cells": G,
           "grouped_call_ms_median_of_blocks": round(call_ms, 4), "grouped_call_ms_blocks": [round(x, 4) for x in blocks["call"]],
           "grouped_launches_alone_ms_median": round(launch_ms[0], 4), "grouped_launches_alone_ms_min": round(launch_ms[1], 4),
           "grouped_launches_alone_ms_max": round(launch_ms[2], 4), "torch_sort_ms_median": round(sort_ms[0], 4),
           "masked_loop_ms": round(loop_ms, 3), "masked_loop_cells_timed": loop_cells, "masked_loop_scaled_by": round(G / loop_cells, 3),
           "masked_loop_ms_blocks_unscaled": [round(x, 3) for x in blocks["loop"]],
           "speedup_over_masked_loop": round(loop_ms / call_ms, 1),
           "host_resample_np_grouped_s": round(host_s, 3), "speedup_over_host": round(host_s * 1e3 / call_ms, 1),
           "ungrouped_call_ms_median": round(ungrouped_ms, 4), "host_resample_np_ungrouped_s": round(host_ungrouped_s, 3)}
    # what the grouping itself costs: one cell that holds every crown, against the ungrouped call (alternating blocks)
    zero = torch.zeros(N, dtype=torch.int64, device=dev)
    o1 = torch.empty(T, 1, S + 1, dtype=torch.int64, device=dev)
    pair = {"g1": [], "plain": []}
    f1 = lambda: abundance.resample(dl, ds, dt, T, seed=1, mask=dm, group=zero, groups=1, out=o1)
    f0 = lambda: abundance.resample(dl, ds, dt, T, seed=1, mask=dm, out=one)
    f1(), f0()
    assert torch.equal(o1[:, 0], one)
    for _ in range(a.rounds):
        pair["g1"].append(timed(f1, 5)[0])
        pair["plain"].append(timed(f0, 5)[0])
    res["one_cell_grouped_call_ms"] = round(float(np.median(pair["g1"])), 4)
    res["ungrouped_call_ms_same_blocks"] = round(float(np.median(pair["plain"])), 4)
    # the summary: on the device, against the read-back and the host summary it replaces
    dsum = abundance.summary_device(got)
    res["summary_device_ms_median"] = round(timed(lambda: abundance.summary_device(got), max(a.calls, 20))[0], 4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    back = got.cpu().numpy()
    t1 = time.perf_counter()
    print("grouped G={}: the host summary of {:.0f} MB ...".format(G, back.nbytes / 1e6), file=sys.stderr, flush=True)
    hsum = abundance.summary(back.reshape(T, -1))
    t2 = time.perf_counter()
    assert np.array_equal(dsum.mean.cpu().numpy().reshape(-1), hsum.mean) and np.array_equal(dsum.quantiles.cpu().numpy().reshape(3, -1), hsum.quantiles)
    res.update({"table_bytes": int(back.nbytes), "read_back_s": round(t1 - t0, 4), "host_summary_s": round(t2 - t1, 3),
                "summary_bytes": int(dsum.mean.numel() * 8 * 4), "summary_equals_host_summary": True,
                "exact_match_with_host": True, "build_id": L.dta_build_id().decode()})
    line = json.dumps(res)
    print(line)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crowns", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grouped", default="")
    ap.add_argument("--loop-cells", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grouped-out", default=None)
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
    lines = [grouped(a, G, label, score, mask, table, dl, ds, dm, dt, host_s, ms) for G in (int(g) for g in a.grouped.split(",") if g)]
    if a.grouped_out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.grouped_out)), exist_ok=True)
        with open(a.grouped_out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))


if __name__ == "__main__":
    main()
