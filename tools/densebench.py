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
  leg C : leg B with predict_windows(share_conv1=True): the first conv once per raster (DenseRaster.conv1_table, built inside
          the timed call), then per batch a gather of its output and the forward without its first conv.  Its top-1 labels
          are compared with B's: they may differ only where B's own top-2 margin is below 1e-2 (both counts are reported);
          `C_below_B_median_by_more_than_B_spread` is the acceptance.  The table build is also timed alone.
All legs share ONE Predictor, built and run once before anything is timed (`predictor_setup_ms`).  Every leg is timed end
to end -- host work included, the raw raster in host memory at the start, the labels on the device at the end -- with events around it and a host clock around the synchronised call, after warm-up runs, `repeats` times,
legs alternating.  The legs' labels are compared.  The gather launch is also timed alone (events around 20 back-to-back
launches of one batch) and reported as achieved bytes/s: bytes = 32 read + 32 written per (window, chunk, pixel).
--only B runs leg B alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/densebench.py --only B);
--only B,C alternates the two resident-raster legs without the slow host-sliced ones.

    python tools/densebench.py --multistage [--levels 2,2,3,3,3] [--years 3] [--missing 1] [--boxes 64] [--box-side 20] ...

A multi-stage model (levels x years bf16 spectral networks, a chain hierarchy) over the windows of `boxes` crown boxes:
  leg A : calls the parent commit has: per-year dta_gather_windows into MultiStagePredictor.ensemble(present=None) (which
          launches dta_year_flags), the same device copies, then per-level dense.crown_reduce + engine.resolve_hierarchy;
  leg B : dense.predict_windows_multistage (dta_gather_windows_years, ensemble(year_flags=...), dta_crown_resolve);
  leg C : leg B with share_conv1=True on bf16-resident rasters: every year's first convs of all levels once per raster
          (dense.Conv1TableYears, built inside the timed call), then per batch ONE gather of their outputs and the grouped
          forward without its first convs.  Its per-window ens_labels are compared with B's, next to B's margin census (the
          windows where some level's top-2 margin is below 1e-2); `C_below_B_median_by_more_than_B_spread` is the
          acceptance.  The table build is also timed alone.
All legs start from resident rasters and share one MultiStagePredictor warmed before the timed region; timed as above.
Window and crown labels of the legs are compared.  One batch is also timed in pieces (20 back-to-back repeats between
events): gather + flags each way, and the forward + epilogue chain with and without its own dta_year_flags launch.
--only B,C alternates the two routes of this package without leg A.

    python tools/densebench.py --crops [--side 256] [--boxes 4096] [--min-side 3] [--max-side 25] [--batch 4096] ...

One crop per crown box, resized to 11x11 with NEAREST (the reference's production path), bf16 Hang2020:
  leg A : what the parent commit offers: every box sliced from the raw host raster, preprocess.preprocess_batch(tiles=True)
          (one upload and one launch per batch), engine.Predictor, dta_softmax_top2;
  leg B : dense.DenseRaster (one upload, one normalise launch, inside the timed call) + dense.predict_crops;
  leg B_resident : dense.predict_crops on a raster that is already resident (reported, not part of the acceptance).
One Predictor for all legs, warmed before the timed region; legs alternate, timed as above; their top-2 labels are compared.
`B_below_A_median_and_ranges_apart` is the acceptance.  The crop gather launch is also timed alone (20 back-to-back launches
of one batch) and reported as bytes written per second next to the measured copy figure.
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


def _timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def multistage(a):
    import ctypes as C
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dense import Conv1TableYears, DenseRaster, crown_reduce, predict_windows_multistage, window_origins
    from deeptreeattention_amd.engine import MultiStagePredictor, resolve_hierarchy
    from deeptreeattention_amd.hierarchy import Hierarchy
    from deeptreeattention_amd.year import learned_ensemble
    dev = torch.device("cuda:0")
    L = _lib.lib()
    S = 11
    classes = [int(c) for c in a.levels.split(",")]
    nl, Y = len(classes), a.years
    # a chain: class 1 of every level but the last passes on to the next level, every other class is a species
    nxt, sp, ns = [], [], 0
    for l, c in enumerate(classes):
        nx = [l + 1 if (k == 1 and l < nl - 1) else -1 for k in range(c)]
        row = []
        for v in nx:
            row.append(ns if v == -1 else -1)
            ns += v == -1
        nxt.append(nx)
        sp.append(row)
    h = Hierarchy(nxt, sp, ns)
    torch.manual_seed(3)
    models = [learned_ensemble(Y, c, {"pretrain_state_dict": None, "bands": a.bands - 20}).to(dev).eval() for c in classes]
    for m in models:
        for net in m.year_models:
            net.precision = "bf16"
    rng = np.random.default_rng(7)
    raws = [None if y == a.missing else rng.integers(-500, 9000, size=(a.bands, a.side, a.side), dtype=np.int16) for y in range(Y)]
    rs = [None if r is None else DenseRaster(r, precision="fp32", device=dev) for r in raws]
    r0 = next(r for r in rs if r is not None)
    bs = a.box_side
    corners = rng.integers(-bs // 2, a.side - bs // 2, size=(a.boxes, 2))
    boxes = [(int(r), int(c), int(r) + int(rng.integers(1, bs + 1)), int(c) + int(rng.integers(1, bs + 1))) for r, c in corners]
    origins, offsets = window_origins(boxes, anchor="corner")
    N = len(origins)
    o = torch.from_numpy(origins).to(dev)
    B = min(a.batch, N)
    pred = MultiStagePredictor(models, frozen=True, hierarchy=h)
    if not pred.supported(Y):
        raise SystemExit("levels x years must fit one chain ({} networks)".format(_lib.MAX_YEARS))
    bufs = [torch.zeros(B, r0.bands, S, S, device=dev) for _ in range(Y)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred.ensemble([b for b in bufs], return_probs=True)
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t0) * 1e3

    def leg_a():
        ens = (torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
               torch.empty(N, dtype=torch.int32, device=dev))
        ti = [torch.empty(N, 2, dtype=torch.int64, device=dev) for _ in range(nl)]
        ts = [torch.empty(N, 2, dtype=torch.float32, device=dev) for _ in range(nl)]
        pr = [torch.empty(N, c, dtype=torch.float32, device=dev) for c in classes]
        for n0 in range(0, N, B):
            n = min(B, N - n0)
            xs = [b[:n] if r is None else r.windows(o[n0:n0 + n], out=b[:n]) for r, b in zip(rs, bufs)]
            e = pred.ensemble(xs, present=None)
            for d, s_ in zip(ens, e):
                d[n0:n0 + n].copy_(s_)
            for l in range(nl):
                ti[l][n0:n0 + n].copy_(pred.top_idx[l])
                ts[l][n0:n0 + n].copy_(pred.top_score[l])
                pr[l][n0:n0 + n].copy_(pred.probs[l])
        per = [crown_reduce(p, offsets) for p in pr]
        crown = resolve_hierarchy(h, [c.top_idx for c in per], [c.top_score for c in per])
        return ens[0], crown[0], crown[1]

    margins = {}

    def leg_b():
        res = predict_windows_multistage(pred, rs, o, crown_offsets=offsets, batch_size=B)
        margins["B"] = [t[:, 0] - t[:, 1] for t in res.top_score]
        return res.ens_label, res.crowns.label, res.crowns.score

    rs16 = None

    def leg_c():
        res = predict_windows_multistage(pred, rs16, o, crown_offsets=offsets, batch_size=B, share_conv1=True)
        return res.ens_label, res.crowns.label, res.crowns.score

    legs = {"A": leg_a, "B": leg_b, "C": leg_c}
    legs = {k: legs[k] for k in (a.only.split(",") if a.only else ("A", "B"))}
    if "C" in legs:      # resident like leg B's, in the form the shared first conv reads
        rs16 = [None if r is None else DenseRaster(r, precision="bf16", device=dev) for r in raws]
    ms, wall, last = {k: [] for k in legs}, {k: [] for k in legs}, {}
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
    out = {"tool": "densebench --multistage", "build": L.dta_build_id().decode(), "side": a.side, "bands_raw": a.bands,
           "levels": classes, "years": Y, "missing_year": a.missing, "boxes": a.boxes, "windows": N, "batch": B,
           "repeats": a.repeats, "warmup": a.warmup, "predictor_setup_ms": round(setup_ms, 2), "legs": {}}
    for k in legs:
        out["legs"][k] = {"event_ms": [round(v, 2) for v in ms[k]], "median_ms": round(statistics.median(ms[k]), 2),
                          "min_ms": round(min(ms[k]), 2), "max_ms": round(max(ms[k]), 2),
                          "wall_median_ms": round(statistics.median(wall[k]), 2)}
    if "A" in last and "B" in last:
        A, Bv = last["A"], last["B"]
        out["window_labels_identical"] = bool(torch.equal(A[0], Bv[0]))
        out["crown_labels_identical"] = bool(torch.equal(A[1], Bv[1]))
        out["crown_score_bits_identical"] = bool(torch.equal(A[2].view(torch.int32), Bv[2].view(torch.int32)))
        la, lb = out["legs"]["A"], out["legs"]["B"]
        out["A_spread_ms"] = round(la["max_ms"] - la["min_ms"], 2)
        out["B_spread_ms"] = round(lb["max_ms"] - lb["min_ms"], 2)
        out["B_below_A_median_by_more_than_both_spreads"] = bool(lb["median_ms"] < la["median_ms"] - max(out["A_spread_ms"], out["B_spread_ms"]))
        out["speedup_A_over_B"] = round(la["median_ms"] / lb["median_ms"], 3)
    if "B" in last and "C" in last:
        Bl, Cl = out["legs"]["B"], out["legs"]["C"]
        out["B_spread_ms"] = round(Bl["max_ms"] - Bl["min_ms"], 2)
        out["C_below_B_median_by_more_than_B_spread"] = bool(Cl["median_ms"] < Bl["median_ms"] - out["B_spread_ms"])
        out["speedup_B_over_C"] = round(Bl["median_ms"] / Cl["median_ms"], 3)
        differ = last["C"][0] != last["B"][0]
        close = torch.stack([m < 1e-2 for m in margins["B"]]).any(dim=0)
        out["C_ens_label_differs_from_B"] = int(differ.sum())
        out["C_ens_label_differs_where_every_B_margin_at_least_1e-2"] = int((differ & ~close).sum())
        out["B_windows_with_a_level_margin_below_1e-2"] = int(close.sum())
        out["C_crown_label_differs_from_B"] = int((last["C"][1] != last["B"][1]).sum())
    if "C" in legs:      # the once-per-call cost: per present year weight image + tap GEMM + class sums + mask
        Conv1TableYears(rs16, pred)
        out["conv1_table_years"] = {"us_per_build": round(_timed(lambda: Conv1TableYears(rs16, pred), reps=5), 1),
                                    "table_MB_per_year": round(((a.side + 2) ** 2 + 1) * 9 * 32 * nl * 2 / 1e6, 1)}
    # one batch in pieces
    ob = o[:B]
    xs = [b[:B] for b in bufs]
    st = _lib.current_stream_ptr()
    banks = [torch.zeros(Y, device=dev) for _ in range(2)]
    ybanks = [torch.zeros(Y, device=dev) for _ in range(2)]
    xptr = (C.c_void_p * Y)(*[x.data_ptr() for x in xs])
    state = {"b": 0, "y": 0}

    def gather_a():
        for r, b in zip(rs, xs):
            if r is not None:
                r.windows(ob, out=b)
        f, nx = ybanks[state["y"]], ybanks[state["y"] ^ 1]
        state["y"] ^= 1
        _lib.check(L.dta_year_flags(xptr, Y, xs[0].numel(), _lib.ptr(f), _lib.ptr(nx), st), "dta_year_flags")

    def gather_b():
        f, nx = banks[state["b"]], banks[state["b"] ^ 1]
        state["b"] ^= 1
        state["flags"] = DenseRaster.windows_years(rs, ob, xs, f, nx)

    out["per_batch_us"] = {"windows": B,
                           "A_gathers_plus_year_flags": round(_timed(gather_a), 1),
                           "B_gather_windows_years": round(_timed(gather_b), 1)}
    flags = state["flags"].clone()
    out["per_batch_us"]["forward_chain_with_own_year_flags"] = round(_timed(lambda: pred.ensemble(xs, present=None)), 1)
    out["per_batch_us"]["forward_chain_given_year_flags"] = round(_timed(lambda: pred.ensemble(xs, year_flags=flags)), 1)
    out["per_batch_us"]["year_flags"] = [float(v) for v in flags.cpu().tolist()]
    if "C" in legs:
        table = Conv1TableYears(rs16, pred)

        def gather_c():
            f, nx = banks[state["b"]], banks[state["b"] ^ 1]
            state["b"] ^= 1
            state["flags_c"] = table.gather(ob, pred, f, nx)

        out["per_batch_us"]["C_gather_conv1_windows_years"] = round(_timed(gather_c), 1)
        flags_c = state["flags_c"].clone()
        out["per_batch_us"]["forward_chain_behind_the_first_convs"] = round(_timed(lambda: pred.ensemble_from_conv1(flags_c)), 1)
        out["per_batch_us"]["year_flags_C"] = [float(v) for v in flags_c.cpu().tolist()]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def crops(a):
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dense import DenseRaster, predict_crops
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    dev = torch.device("cuda:0")
    S = 11
    rng = np.random.default_rng(7)
    raw = rng.integers(-500, 9000, size=(a.bands, a.side, a.side), dtype=np.int16)
    hs, ws = (rng.integers(a.min_side, a.max_side + 1, size=a.boxes) for _ in range(2))
    r0, c0 = rng.integers(0, a.side - hs + 1), rng.integers(0, a.side - ws + 1)
    boxes = np.stack([r0, c0, r0 + hs, c0 + ws], axis=1).astype(np.int32)
    N = len(boxes)
    torch.manual_seed(3)
    model = H.Hang2020(a.bands - 20, a.classes, precision="bf16").to(dev).eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = Predictor(model)
    pred(torch.zeros(min(a.batch, N), a.bands - 20, S, S, device=dev), return_probs=False)
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t0) * 1e3

    def leg_a():
        top = torch.empty(N, 2, dtype=torch.int64, device=dev)
        for n0 in range(0, N, a.batch):
            bb = boxes[n0:n0 + a.batch]
            x = preprocess_batch([raw[:, p:q, u:v] for p, u, q, v in bb], S, device=dev, tiles=True)
            top[n0:n0 + len(bb)] = pred(x, return_probs=False)[1]
        return top

    resident = DenseRaster(raw, precision="bf16", device=dev)
    legs = {"A": leg_a,
            "B": lambda: predict_crops(pred, DenseRaster(raw, precision="bf16", device=dev), boxes, batch_size=a.batch).top_idx,
            "B_resident": lambda: predict_crops(pred, resident, boxes, batch_size=a.batch).top_idx}
    if a.only:
        legs = {k: legs[k] for k in a.only.split(",")}
    ms, wall, last = {k: [] for k in legs}, {k: [] for k in legs}, {}
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
    raw_bytes = int((hs * ws).sum()) * a.bands * raw.itemsize
    out = {"tool": "densebench --crops", "build": _lib.lib().dta_build_id().decode(), "side": a.side, "bands_raw": a.bands,
           "classes": a.classes, "boxes": N, "box_sides": [a.min_side, a.max_side], "batch": a.batch, "repeats": a.repeats,
           "warmup": a.warmup, "predictor_setup_ms": round(setup_ms, 2),
           "host_link_bytes": {"A_raw_crops": raw_bytes, "B_raster_plus_boxes": raw.nbytes + boxes.nbytes,
                               "B_resident_boxes": boxes.nbytes}, "legs": {}}
    for k in legs:
        out["legs"][k] = {"event_ms": [round(v, 2) for v in ms[k]], "median_ms": round(statistics.median(ms[k]), 2),
                          "min_ms": round(min(ms[k]), 2), "max_ms": round(max(ms[k]), 2),
                          "wall_median_ms": round(statistics.median(wall[k]), 2), "wall_min_ms": round(min(wall[k]), 2),
                          "wall_max_ms": round(max(wall[k]), 2)}
    if "A" in last and "B" in last:
        A, B = out["legs"]["A"], out["legs"]["B"]
        out["top2_labels_identical"] = bool(torch.equal(last["A"], last["B"]))
        # host work is most of leg A: the acceptance is on the host clock around the synchronised call
        out["B_below_A_median_and_ranges_apart"] = bool(B["wall_median_ms"] < A["wall_median_ms"] and B["wall_max_ms"] < A["wall_min_ms"])
        out["B_below_A_event_median_and_ranges_apart"] = bool(B["median_ms"] < A["median_ms"] and B["max_ms"] < A["min_ms"])
        out["speedup_A_over_B_wall"] =round(A["wall_median_ms"] / B["wall_median_ms"], 2)
    # the crop gather alone: one batch, 20 back-to-back launches between two events
    n = min(a.batch, N)
    bb = torch.from_numpy(boxes[:n]).to(dev)
    buf = resident.crops(bb, tiles=True).tiles
    us = _timed(lambda: resident.crops(bb, tiles=True, out=buf))
    written = n * ((resident.bands + 15) // 16) * S * S * 32
    out["gather_crops_tiles"] = {"crops": n, "bytes_written": written, "us_per_launch": round(us, 1),
                                 "written_TB_per_s": round(written / us / 1e6, 3), "copy_probe_TB_per_s": 5.8}
    r32 = DenseRaster(raw, precision="fp32", device=dev)
    buf32 = r32.crops(bb)
    us32 = _timed(lambda: r32.crops(bb, out=buf32))
    out["gather_crops_fp32"] = {"crops": n, "bytes_written": buf32.numel() * 4, "us_per_launch": round(us32, 1),
                                "written_TB_per_s": round(buf32.numel() * 4 / us32 / 1e6, 3), "copy_probe_TB_per_s": 5.8}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", action="store_true")
    ap.add_argument("--min-side", type=int, default=3)
    ap.add_argument("--max-side", type=int, default=25)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--bands", type=int, default=369)
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--multistage", action="store_true")
    ap.add_argument("--levels", default="2,2,3,3,3")
    ap.add_argument("--years", type=int, default=3)
    ap.add_argument("--missing", type=int, default=1)
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--box-side", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densebench needs the GPU (no fallback)")
    if a.multistage:
        return multistage(a)
    if a.crops:
        if a.boxes == 64:      # (--boxes' default belongs to --multistage)
            a.boxes = 4096
        return crops(a)
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

    scores = {}

    def leg_b():
        res = predict_windows(pred, DenseRaster(raw, precision="bf16", device=dev), origins, batch_size=a.batch)
        scores["B"] = res.top_score
        return res.top_idx

    def leg_c():
        res = predict_windows(pred, DenseRaster(raw, precision="bf16", device=dev), origins, batch_size=a.batch, share_conv1=True)
        scores["C"] = res.top_score
        return res.top_idx

    legs = {"A": lambda: host_route(False), "A2": lambda: host_route(True), "B": leg_b, "C": leg_c}
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
            if k not in ("B", "C"):
                out["legs"][k]["top1_differs_from_B"] = int((last[k][:, 0] != last["B"][:, 0]).sum())
                out["legs"][k]["top2_identical_to_B"] = bool(torch.equal(last[k], last["B"]))
    if "B" in legs and "A" in legs:
        A, B = out["legs"]["A"], out["legs"]["B"]
        best_a = min(out["legs"][k]["median_ms"] for k in legs if k not in ("B", "C"))
        spread = max(out["legs"][k]["max_ms"] - out["legs"][k]["min_ms"] for k in legs if k not in ("B", "C"))
        out["B_below_A_median_by_more_than_A_spread"] = bool(B["median_ms"] < best_a - spread)
        out["speedup_A_over_B"] = round(A["median_ms"] / B["median_ms"], 2)
    ras = DenseRaster(raw, precision="bf16", device=dev)
    if "B" in last and "C" in last:
        Bl, Cl = out["legs"]["B"], out["legs"]["C"]
        out["B_spread_ms"] = round(Bl["max_ms"] - Bl["min_ms"], 2)
        out["C_below_B_median_by_more_than_B_spread"] = bool(Cl["median_ms"] < Bl["median_ms"] - out["B_spread_ms"])
        out["speedup_B_over_C"] = round(Bl["median_ms"] / Cl["median_ms"], 3)
        differ = last["C"][:, 0] != last["B"][:, 0]
        close = (scores["B"][:, 0] - scores["B"][:, 1]) < 1e-2
        out["C_top1_differs_from_B"] = int(differ.sum())
        out["C_top1_differs_where_B_margin_at_least_1e-2"] = int((differ & ~close).sum())
        out["B_windows_with_margin_below_1e-2"] = int(close.sum())
    if "C" in legs:      # the once-per-raster cost: weight image + tap GEMM + class sums (the scratch comes from torch's cache)
        ras.conv1_table(pred)
        out["conv1_table"] = {"us_per_build": round(_timed(lambda: ras.conv1_table(pred), reps=5), 1),
                              "table_MB": round((ras.height + 2) * (ras.width + 2) * 9 * 64 * 2 / 1e6, 1)}
    # the gather alone: one batch, 20 back-to-back launches between two events
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
