"""Per-batch time of prediction with the site-metadata fusion model (369 bands / 200 classes / 23 sites, bf16):
engine.MetadataPredictor (sensor forward + dta_meta_site_table + dta_meta_predict; frozen: without the table launch) next
to the same prediction composed from the train / validation path's calls (FusedTrainer._forward_scores +
dta_meta_head_forward(training = 0) + dta_softmax_top2), and the two heads alone on fixed HSI scores.  One process, the
arms alternate inside every round, HIP-event timed; prints one JSON line per batch size.

    python tools/metapredictbench.py [--batches 64,2048,4096] [--rounds 7] [--iters 40] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BANDS, CLASSES, SITES = 369, 200, 23


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,2048,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.engine import MetadataPredictor, MetadataTrainer
    from deeptreeattention_amd.metadata import metadata_sensor_fusion
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    torch.manual_seed(0)
    m = metadata_sensor_fusion(BANDS, SITES, CLASSES, precision="bf16").to(dev).eval()
    tr = MetadataTrainer(m, lr=1e-3)
    live, frozen = MetadataPredictor(m), MetadataPredictor(m, frozen=True)
    lines = []
    for B in [int(b) for b in args.batches.split(",")]:
        x = torch.rand(B, BANDS, 11, 11, device=dev)
        site = torch.randint(0, SITES, (B,), device=dev)
        probs = torch.empty(B, CLASSES, device=dev)
        top_idx = torch.empty(B, 2, dtype=torch.int64, device=dev)
        top_score = torch.empty(B, 2, device=dev)
        old_ok = L.dta_meta_head_workspace_bytes(B, CLASSES, SITES) != 0
        refusal = None if old_ok else L.dta_last_error().decode()

        def old_head(scores):
            out, _ = tr._native_forward(scores, site, False)
            _lib.check(L.dta_softmax_top2(_lib.ptr(out), B, CLASSES, _lib.ptr(probs), _lib.ptr(top_idx), _lib.ptr(top_score),
                                          _lib.current_stream_ptr()), "dta_softmax_top2")

        def old_route():
            with torch.no_grad():
                old_head(tr.sensor._forward_scores(x))

        scores = live.sensor.logits_of(x).clone()
        out = torch.empty(B, CLASSES, device=dev)

        def new_head(pred):
            pred.head(scores, B, pred.table(), site, out, probs, top_idx, top_score)

        arms = {"new_route": lambda: live(x, site), "new_route_frozen": lambda: frozen(x, site),
                "new_head": lambda: new_head(live), "new_head_frozen": lambda: new_head(frozen)}
        if old_ok:
            arms["old_route"] = old_route
            arms["old_head"] = lambda: old_head(scores)
        for fn in arms.values():                 # warm up every arm at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        if old_ok:
            old_route()
            a = probs.clone()
            live(x, site)
            d = float((live(x, site)[0] - a).abs().max())
        else:
            d = None
        t = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn, args.iters))
        res = {"batch": B, "bands": BANDS, "classes": CLASSES, "sites": SITES, "precision": "bf16", "rounds": args.rounds,
               "iters": args.iters, "old_route_refused": refusal, "max_abs_prob_diff_new_vs_old": d,
               "launches": {"new_head": 2, "new_head_frozen": 1, "old_head": 4},
               "us_per_batch": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in t.items()},
               "build": L.dta_build_id().decode()}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del x
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    tr.close()


if __name__ == "__main__":
    main()
