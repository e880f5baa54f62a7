"""Time deeptreeattention_amd.evaluate: the counting launch in both forms (dta_eval_count, PLAIN and COMBINE) on a
concentrated and on a spread input, the report launch (dta_eval_report), first_per_individual and novel_scores on the GPU,
by stream events; the host definitions count_np / report_np; optionally the reference's own site_confusion and
genus_confusion loops on the same labels (a CPU figure).

    python tools/evalbench.py [--out profiles/evalbench.json] [--rows 1000000] [--species 200] [--sites 23]
                              [--reference <path of a checkout of the reference>] [--host-only]

Inputs, made here from a seed: `concentrated` has 90 % of its rows on 5 diagonal entries (a validation set a model gets mostly
right, dominated by a few species of one site), `spread` is uniform over species and sites.  The two count forms are timed in
ONE process in alternating blocks (a pair of stream events around a block of calls into a table that stays, read after the
block): the figure is the median per call over the blocks, the spread the lowest and the highest block.  Every device result
is verified equal to the definition before timing.  Host figures are medians of a host clock.  --host-only (or no GPU with
--reference) skips everything that needs the device; without --reference the reference is "not measured"."""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from deeptreeattention_amd import evaluate as E  # noqa: E402

BLOCKS, PER_BLOCK = 20, 25


def inputs(rows, S, G, concentrated, seed=17):
    rs = np.random.RandomState(seed + concentrated)
    t, g = rs.randint(0, S, rows).astype(np.int64), rs.randint(0, G, rows).astype(np.int64)
    p = np.where(rs.rand(rows) < 0.7, t, rs.randint(0, S, rows)).astype(np.int64)
    if concentrated:
        hot = rs.rand(rows) < 0.9
        t[hot] = rs.randint(0, 5, hot.sum()) * 7 % S
        p[hot], g[hot] = t[hot], 3 % G
    return t, p, g


def tables(S, sites, seed=3):
    rs = np.random.RandomState(seed)
    site_lists = {k: sorted(set(rs.randint(0, sites, rs.randint(1, 5)).tolist())) for k in range(S)}
    scientific = {k: ["Genus{} species{}".format(rs.randint(0, max(2, S // 5)), k)] for k in range(S)}
    return site_lists, scientific


def host_ms(fn, repeats=5):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(times), "range": [min(times), max(times)], "repeats": repeats}


def event_ms(torch, fns):
    """fns: name -> callable; blocks alternate between them.  name -> the figures."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    device_ms, enqueue_ms = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(BLOCKS):
        for name, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record()
            for _ in range(PER_BLOCK):
                fn()
            stop.record()
            enqueue_ms[name].append((time.perf_counter() - t0) * 1e3 / PER_BLOCK)
            torch.cuda.synchronize()
            device_ms[name].append(start.elapsed_time(stop) / PER_BLOCK)
    return {k: {"ms": statistics.median(device_ms[k]), "blocks": [min(device_ms[k]), max(device_ms[k])],
                "enqueue_ms": statistics.median(enqueue_ms[k]), "n_blocks": BLOCKS, "calls_per_block": PER_BLOCK} for k in fns}


def main():
    def arg(name, default=None):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out_path, ref = arg("--out"), arg("--reference")
    rows, S, G = int(arg("--rows", 1000000)), int(arg("--species", 200)), int(arg("--sites", 23))
    import torch
    gpu = torch.cuda.is_available() and "--host-only" not in sys.argv
    assert gpu or ref or "--host-only" in sys.argv, "evalbench needs a GPU (or --host-only / --reference for the host figures)"
    result = {"rows": rows, "species": S, "sites": G, "device": gpu, "combine_rounds": 4}
    site_lists, scientific = tables(S, G)
    masks, genus = E.site_masks(site_lists, S), E.genus_ids(scientific, S)
    data = {"concentrated": inputs(rows, S, G, 1), "spread": inputs(rows, S, G, 0)}
    want = {}
    for name, (t, p, g) in data.items():
        want[name] = E.count_np(t, p, g, None, S, G)
        key = (g * S + t) * S + p
        result[name] = {"distinct_entries": int(len(np.unique(key))), "largest_entry": int(want[name][0].max()),
                        "count_np": host_ms(lambda: E.count_np(t, p, g, None, S, G), 3),
                        "report_np": host_ms(lambda: E.report_np(want[name][0], masks, genus), 3)}
    if gpu:
        from deeptreeattention_amd import _lib
        dev = torch.device("cuda:0")
        L = _lib.lib()
        result["build_id"] = L.dta_build_id().decode()
        result["default_form"] = "combine" if E.FORM == E.COMBINE else "plain"
        for name, (t, p, g) in data.items():
            td, pd_, gd = (torch.from_numpy(a).to(dev) for a in (t, p, g))
            for form in (E.PLAIN, E.COMBINE):
                table = E.EvalTable(S, G, device=dev).count(td, pd_, group=gd, form=form)
                assert np.array_equal(table.conf.cpu().numpy(), want[name][0]) and np.array_equal(table.tally.cpu().numpy(), want[name][1])
            rep = table.report(masks, genus).cpu()
            ref_rep = E.report_np(want[name][0], masks, genus)
            assert all(np.array_equal(rep[k].view(np.int64), ref_rep[k].view(np.int64)) for k in ref_rep)
            sink = E.EvalTable(S, G, device=dev)

            def count(form):
                return lambda: _lib.check(L.dta_eval_count(_lib.ptr(td), _lib.ptr(pd_), _lib.ptr(gd), 1, None, rows, S, G, form,
                                                           _lib.ptr(sink.conf), _lib.ptr(sink.tally), _lib.current_stream_ptr()), "count")
            timed = event_ms(torch, {"count_plain": count(E.PLAIN), "count_combine": count(E.COMBINE)})
            # the same pair once more, the other form first: the run-to-run spread of one call
            again = event_ms(torch, {"count_combine": count(E.COMBINE), "count_plain": count(E.PLAIN)})
            result[name].update(timed)
            result[name]["again"] = again
            md, gn = torch.from_numpy(masks.view(np.int64)).to(dev), torch.from_numpy(genus).to(dev)
            result[name].update(event_ms(torch, {"report": lambda: table.report(md, gn)}))
        ids = torch.from_numpy(np.random.RandomState(1).randint(0, rows // 2, rows).astype(np.int64)).to(dev)
        assert np.array_equal(E.first_per_individual(ids, rows // 2).cpu().numpy(), E.first_per_individual_np(ids.cpu().numpy(), rows // 2))
        result.update(event_ms(torch, {"first_per_individual": lambda: E.first_per_individual(ids, rows // 2)}))
        z = torch.randn(100000, S, device=dev)
        result.update(event_ms(torch, {"novel_scores_100000_rows": lambda: E.novel_scores(z)}))
    result["reference_loops"] = "not measured"
    if ref:
        from make_evaluate_golden import import_reference
        M = import_reference(ref)
        result["reference_loops"] = {"where": "host CPU", "repeats": 1}
        for name, (t, p, g) in data.items():
            yt, yp = t.tolist(), p.tolist()
            t0 = time.perf_counter()
            site = M.site_confusion(yt, yp, site_lists)
            t1 = time.perf_counter()
            gen = M.genus_confusion(yt, yp, scientific)
            t2 = time.perf_counter()
            r = E.report_np(want[name][0], masks, genus)
            assert r["scores"][G, 2] == site and r["scores"][G, 3] == gen
            result["reference_loops"][name] = {"site_confusion_ms": (t1 - t0) * 1e3, "genus_confusion_ms": (t2 - t1) * 1e3,
                                               "site_confusion": site, "genus_confusion": gen}
    print(json.dumps(result), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
