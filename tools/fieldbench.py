"""Time deeptreeattention_amd.field: the filter chain on the GPU (dta_field_filter alone, by stream events), the host
definition filter_np, the string work of FieldTable.from_frame, and the megaplot plot codes by both rules with their host
definition; optionally the reference's own filter_data on the same table written as CSV (a CPU figure).

    python tools/fieldbench.py [--out profiles/fieldbench.json] [--rows 500000] [--individuals 200000]
                               [--reference <path of a checkout of the reference>] [--host-only]

The table is a raw NEON-like frame made here from a seed (strings and all), so that the package and the reference read the
same thing.  The chain is timed by a pair of stream events around a block of calls, read after the block: the figure is the
median over the blocks per call, the spread the lowest and highest block.  Host figures are medians of a host clock.
--host-only (or no GPU with --reference) skips everything that needs the device; without --reference the reference is
"not measured"."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import field_cases as FC  # noqa: E402
from deeptreeattention_amd import field as F  # noqa: E402

BLOCKS, PER_BLOCK = 20, 25
MIN_STEM_DIAMETER = 10.0


def frame(rows, individuals, seed=8):
    """A raw field table as a pandas frame whose strings give the flag bits of FC.table (known errors left out: the
    reference names three individuals)."""
    import pandas as pd
    c = FC.table(rows, individuals, seed)["columns"]
    f, ind = c["flags"], c["individual"]

    def pick(bit, yes, no):
        return np.where(f & bit != 0, yes, no).astype(object)
    name = np.char.add(np.char.mod("NEON.PLA.D01.HARV.%06d", ind), np.where(f & F.MULTIBOLE != 0, "A", ""))
    year = np.where(f & F.EVENT_DROPPED != 0, 2014, 2015 + c["event"] % 7)
    canopy = pick(F.SHADED, "Full shade", "Partially shaded")
    canopy[f & F.SUNNY != 0] = "Full sun"
    return pd.DataFrame({
        "individualID": name, "eventID": np.char.mod("vst_HARV_%d", year), "siteID": pick(F.SITE_EXCLUDED, "ORNL", "HARV"),
        "plotID": pick(F.PLOT_EXCLUDED, "OSBS_026", "HARV_001"), "taxonID": pick(F.TAXON_EXCLUDED, "PINUS", "ACRU"),
        "utmZone": "18N", "itcEasting": np.where(f & F.COORDS != 0, 725000.0 + 0.25 * (ind % 4000), np.nan),
        "itcNorthing": 4700000.0 + 0.25 * (ind % 3000), "growthForm": pick(F.GROWTH, "single bole tree", "liana"),
        "plantStatus": pick(F.LIVE, "Live", "Standing dead"), "canopyPosition": canopy, "height": c["height"],
        "stemDiameter": c["diameter"]})


def host_ms(fn, repeats=5):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(times), "range": [min(times), max(times)], "repeats": repeats}


def event_ms(torch, fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    device_ms, enqueue_ms = [], []
    for _ in range(BLOCKS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        for _ in range(PER_BLOCK):
            fn()
        stop.record()
        enqueue_ms.append((time.perf_counter() - t0) * 1e3 / PER_BLOCK)
        torch.cuda.synchronize()
        device_ms.append(start.elapsed_time(stop) / PER_BLOCK)
    return {"ms": statistics.median(device_ms), "blocks": [min(device_ms), max(device_ms)],
            "enqueue_ms": statistics.median(enqueue_ms), "n_blocks": BLOCKS, "calls_per_block": PER_BLOCK}


def main():
    def arg(name, default=None):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out_path, ref = arg("--out"), arg("--reference")
    rows, individuals = int(arg("--rows", 500000)), int(arg("--individuals", 200000))
    import torch
    gpu = torch.cuda.is_available() and "--host-only" not in sys.argv
    assert gpu or ref or "--host-only" in sys.argv, "fieldbench needs a GPU (or --host-only / --reference for the host figures)"
    result = {"rows": rows, "individuals": individuals, "min_stem_diameter": MIN_STEM_DIAMETER, "device": gpu}
    df = frame(rows, individuals)
    result["from_frame"] = host_ms(lambda: F.FieldTable.from_frame(df), 3)
    table = F.FieldTable.from_frame(df)
    columns = dict(table.columns, individuals=table.individuals)
    want = F.filter_np(columns, MIN_STEM_DIAMETER)
    result["kept"] = int(want.count)
    result["reasons"] = np.bincount(want.reason, minlength=14).tolist()
    result["filter_np"] = host_ms(lambda: F.filter_np(columns, MIN_STEM_DIAMETER))
    stems = {"buffer": FC.lattice(1000, seed=50, span=2400), "grid": FC.lattice(100000, seed=51, span=40000)}
    for rule, points in stems.items():
        result["plots_np_" + rule] = dict(host_ms(lambda: F.plots_np(points, rule)), stems=len(points))
    if gpu:
        from deeptreeattention_amd import _lib
        dev = torch.device("cuda:0")
        result["build_id"] = _lib.lib().dta_build_id().decode()
        resident = F.FieldTable(columns, device=dev)
        got = resident.filter(MIN_STEM_DIAMETER)
        assert np.array_equal(got.rows.cpu().numpy(), want.rows) and np.array_equal(got.reason.cpu().numpy(), want.reason)
        result["filter_chain"] = event_ms(torch, lambda: resident.filter(MIN_STEM_DIAMETER))
        for rule, points in stems.items():
            p = torch.from_numpy(points).to(dev)
            code = F.megaplot_plots(p, rule, device=dev).code
            assert np.array_equal(code.cpu().numpy(), F.plots_np(points, rule).code)
            result["megaplot_" + rule] = dict(event_ms(torch, lambda: F.megaplot_plots(p, rule, device=dev)), stems=len(points))
    result["reference_filter_data"] = "not measured"
    if ref:
        from make_field_golden import import_reference
        D = import_reference(ref)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "field.csv")
            df.assign(row=np.arange(len(df))).to_csv(path, index=False)
            t0 = time.perf_counter()
            out = D.filter_data(path, {"min_stem_diameter": MIN_STEM_DIAMETER})
            seconds = time.perf_counter() - t0
            t0 = time.perf_counter()
            ours = F.filter_data(path, {"min_stem_diameter": MIN_STEM_DIAMETER})
            ours_seconds = time.perf_counter() - t0
        # the same individuals in the same order (equal events within an individual without a height are the reference's
        # unstable sort: the row may differ there, the individual may not)
        assert ours["row"].tolist() == want.index().tolist() and out["individualID"].tolist() == ours["individualID"].tolist()
        result["reference_filter_data"] = {"ms": seconds * 1e3, "repeats": 1, "where": "host CPU, read_csv included"}
        result["filter_data_host"] = {"ms": ours_seconds * 1e3, "repeats": 1, "where": "host CPU, read_csv included, device=None"}
    print(json.dumps(result), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
