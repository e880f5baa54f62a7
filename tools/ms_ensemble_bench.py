"""Developer tool: the hierarchical ensemble label (5 levels x 3 years, 64 crops, bf16) -- dta_multistage_predict_ensemble
against dta_multistage_predict on the same models, live and frozen weights, and for context the host route the call
replaces (the five probability tensors to the host + the NumPy walk).  The two device calls are timed in alternating
blocks, the median block of each is reported.  python tools/ms_ensemble_bench.py [B] [steps] [blocks]"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeptreeattention_amd  # noqa: E402
from deeptreeattention_amd import _lib  # noqa: E402
from deeptreeattention_amd.engine import MultiStagePredictor  # noqa: E402
from deeptreeattention_amd.hierarchy import Hierarchy  # noqa: E402
from deeptreeattention_amd.year import learned_ensemble  # noqa: E402
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 9
deeptreeattention_amd.set_default_precision("bf16")
dev = torch.device("cuda:0")
cfg = {"pretrain_state_dict": None, "bands": 369}
classes = [2, 2, 12, 7, 5]
torch.manual_seed(0)
models = [learned_ensemble(3, c, cfg).to(dev).eval() for c in classes]
x = [torch.rand(B, 369, 11, 11, device=dev) for _ in range(3)]
# the reference's shape of hierarchy: level 0 class 0 ends, level 1 class 1 -> level 2 else level 3, level 2 class 1 -> level 4
nxt = [[-1, 1], [3, 2], [-1, 4] + [-1] * 10, [-1] * 7, [-1] * 5]
n, spc = 0, []
for row in nxt:
    spc.append([])
    for v in row:
        spc[-1].append(n if v == -1 else -1)
        n += v == -1
h = Hierarchy(nxt, spc, n)
labels = torch.randint(0, n, (B,), device=dev)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def host_route(pred):
    probs = [o[0].cpu().numpy() for o in pred(x)]
    return h.resolve_np([p.argmax(1) for p in probs], [p.max(1) for p in probs])


out = {"workload": "MultiStage predict + ensemble label: 5 levels x 3 years, 369 bands, 11x11, bf16", "batch": B, "steps": steps,
       "blocks": blocks, "build": _lib.lib().dta_build_id().decode() if hasattr(_lib.lib(), "dta_build_id") else None}
for frozen in (False, True):
    plain = MultiStagePredictor(models, frozen=frozen)
    ens = MultiStagePredictor(models, frozen=frozen, hierarchy=h)
    forms = {"predict": lambda: plain(x), "ensemble": lambda: ens.ensemble(x), "ensemble_confusion": lambda: ens.ensemble(x, None, labels)}
    for fn in forms.values():
        for _ in range(10):
            fn()
    t = {k: [] for k in forms}
    for _ in range(blocks):
        for k, fn in forms.items():
            t[k].append(timed(fn))
    tag = "frozen" if frozen else "live"
    for k in forms:
        out["{}_{}_ms".format(tag, k)] = round(float(np.median(t[k])), 4)
        out["{}_{}_ms_min_max".format(tag, k)] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    out[tag + "_ensemble_over_predict"] = round(float(np.median(t["ensemble"]) / np.median(t["predict"])), 4)
    want = host_route(plain)
    got = ens.ensemble(x)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    out[tag + "_host_route_ms"] = round(timed(lambda: host_route(plain)), 4)
out["levels_decided"] = np.bincount(got[2].cpu().numpy(), minlength=5).tolist()
print(json.dumps(out))
