"""Label every pixel of a hyperspectral raster both ways on the same box, in the same process (developer script; bench.py is
the flagship yardstick and is not involved).

    python tools/densebench.py [--side 256] [--bands 369] [--classes 200] [--batch 4096] [--repeats 5] [--warmup 1]
                               [--only B] [--out FILE]

One 11x11 window per pixel (centre-anchored) of a `bands`-band int16 raster of side x side pixels, bf16 Hang2020.
  leg A : the route the parent commit offers, code this change does not touch: the windows sliced on the host from a
          zero-padded copy, preprocess.preprocess_batch (one upload and one launch per batch, float32 batch) and
          engine.Predictor;
  leg A2: the same with preprocess_batch(tiles=True) -- the bf16 tiles straight from the crop kernel.  Predictor taking a
          PatchTiles is new with this change; slicing, upload and crop kernel are the parent's;
  leg B : dense.DenseRaster (one upload, one normalise launch) + dense.predict_windows (tile gather, forward, top-2).
All legs share ONE Predictor, built and run once before anything is timed (`predictor_setup_ms`).  Every leg is timed end
to end -- host work included, the raw raster in host memory at the start, the labels on the device at the end -- with events around it and a host clock around the synchronised call, after warm-up runs, `repeats` times,
legs alternating.  The legs' labels are compared.  The gather launch is also timed alone (events around 20 back-to-back
launches of one batch) and reported as achieved bytes/s: bytes = 32 read + 32 written per (window, chunk, pixel).
--only B runs leg B alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/densebench.py --only B).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--bands", type=int, default=369)
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densebench needs the GPU (no fallback)")
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dense import DenseRaster, predict_windows, window_origins
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    dev = torch.device("cuda:0")
    S, P = 11, a.side * a.side
    rng = np.random.default_rng(7)
    raw = rng.integers(-500, 9000, size=(a.bands, a.side, a.side), dtype=np.int16)
    torch.manual_seed(3)
    model = H.Hang2020(a.bands - 20, a.classes, precision="bf16").to(dev).eval()
    origins, _ = window_origins([(0, 0, a.side, a.side)], anchor="center")
    N = len(origins)

    # one Predictor for every leg and repeat, built and warmed outside the timed region: a caller pays for its weight
    # tables, workspace and first-call packing once, so they are reported apart (`predictor_setup_ms`)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = Predictor(model)
    pred(torch.zeros(min(a.batch, N), a.bands - 20, S, S, device=dev), return_probs=False)
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t0) * 1e3

    def host_route(tiles):
        pad = S
        big = np.zeros((a.bands, a.side + 2 * pad, a.side + 2 * pad), dtype=raw.dtype)
        big[:, pad:pad + a.side, pad:pad + a.side] = raw
        top = torch.empty(N, 2, dtype=torch.int64, device=dev)
        for n0 in range(0, N, a.batch):
            o = origins[n0:n0 + a.batch]
            wins = [big[:, r + pad:r + pad + S, c + pad:c + pad + S] for r, c in o]
            x = preprocess_batch(wins, S, device=dev, tiles=tiles)
            top[n0:n0 + len(o)] = pred(x, return_probs=False)[1]
        return top

    def leg_b():
        return predict_windows(pred, DenseRaster(raw, precision="bf16", device=dev), origins, batch_size=a.batch).top_idx

    legs = {"A": lambda: host_route(False), "A2": lambda: host_route(True), "B": leg_b}
    if a.only:
        legs = {k: legs[k] for k in a.only.split(",")}
    ms = {k: [] for k in legs}
    wall = {k: [] for k in legs}
    last = {}
    for rep in range(a.warmup + a.repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            last[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
                wall[k].append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "densebench", "build": _lib.lib().dta_build_id().decode(), "side": a.side, "bands_raw": a.bands,
           "classes": a.classes, "windows": N, "batch": a.batch, "repeats": a.repeats, "warmup": a.warmup, "predictor_setup_ms": round(setup_ms, 2), "legs": {}}
    for k in legs:
        out["legs"][k] = {"event_ms": [round(v, 2) for v in ms[k]], "median_ms": round(statistics.median(ms[k]), 2),
                          "min_ms": round(min(ms[k]), 2), "max_ms": round(max(ms[k]), 2),
                          "wall_median_ms": round(statistics.median(wall[k]), 2)}
    if "B" in last:
        for k in last:
            if k != "B":
                out["legs"][k]["top1_differs_from_B"] = int((last[k][:, 0] != last["B"][:, 0]).sum())
                out["legs"][k]["top2_identical_to_B"] = bool(torch.equal(last[k], last["B"]))
    if "B" in legs and "A" in legs:
        A, B = out["legs"]["A"], out["legs"]["B"]
        best_a = min(out["legs"][k]["median_ms"] for k in legs if k != "B")
        spread = max(out["legs"][k]["max_ms"] - out["legs"][k]["min_ms"] for k in legs if k != "B")
        out["B_below_A_median_by_more_than_A_spread"] = bool(B["median_ms"] < best_a - spread)
        out["speedup_A_over_B"] = round(A["median_ms"] / B["median_ms"], 2)
    # the gather alone: one batch, 20 back-to-back launches between two events
    ras = DenseRaster(raw, precision="bf16", device=dev)
    n = min(a.batch, N)
    o = torch.from_numpy(origins[:n]).to(dev)
    buf = ras.windows(o, tiles=True).tiles
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ras.windows(o, tiles=True, out=buf)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 20
    nbytes = 2 * n * ((ras.bands + 15) // 16) * S * S * 32
    out["gather_tiles"] = {"windows": n, "bytes_read_plus_written": nbytes, "us_per_launch": round(us, 1),
                           "achieved_TB_per_s": round(nbytes / us / 1e6, 3), "copy_probe_TB_per_s": 5.8}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
