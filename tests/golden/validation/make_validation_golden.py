"""Generate tests/golden/validation/validation_epoch.npz by running the REFERENCE ITSELF on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/validation/make_validation_golden.py

Imports the reference's src/models/year.py read-only by path (its unused torchmetrics import is stubbed, as in
tests/golden/make_golden.py), loads parameters and BatchNorm running statistics from oracle/prng.py through
load_state_dict, puts the models in eval() and runs one validation epoch (recipe.py): three levels of
learned_ensemble(years=3), three batches of 24, 24 and 10 crops per level.  Stores ONLY arrays: per batch and level the
reference's scores, F.cross_entropy(weight=...) and F.softmax; per level the confusion matrix of argmax, the top-1 / top-2
hit counts taken with NumPy and the top-1 minus top-2 probability gap per row.  No reference source is copied anywhere.
Writes the fixture's own checksum file (SHA256SUMS in this directory)."""
import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
sys.modules.setdefault("torchmetrics", types.ModuleType("torchmetrics"))

from oracle import hang2020_np as O  # noqa: E402
from src.models import year as RY  # noqa: E402  (the reference)
import recipe as R  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def main():
    c = R.VALIDATION
    out = {}
    for l, classes in enumerate(c["classes"]):
        m = RY.learned_ensemble(years=c["years"], classes=classes, config={"pretrain_state_dict": None, "bands": c["bands"]})
        p = R.params(l, O.init_params, O.learned_ensemble_spec)
        sd = m.state_dict()
        m.load_state_dict({k: torch.from_numpy(np.array(p[k])).to(v.dtype) for k, v in sd.items()})
        m.eval()
        w = torch.from_numpy(R.weight(classes))
        conf = np.zeros((classes, classes), np.int64)
        gaps, top1, top2, rows = [], 0, 0, 0
        for b in range(len(c["batches"])):
            imgs, y = R.inputs(b, l)
            with torch.no_grad():
                s = m([torch.from_numpy(a) for a in imgs])
                loss = F.cross_entropy(s, torch.from_numpy(y), weight=w)
                pr = F.softmax(s, dim=1)
            tag = f"batch{b}/level{l}"
            out[f"{tag}/score"] = s.numpy().copy()
            out[f"{tag}/loss"] = np.float64(loss.item())
            out[f"{tag}/softmax"] = pr.numpy().copy()
            prn = pr.numpy().astype(np.float64)
            order = np.argsort(-prn, axis=1, kind="stable")          # ties towards the lower index
            gap = prn[np.arange(len(y)), order[:, 0]] - prn[np.arange(len(y)), order[:, 1]]
            out[f"{tag}/gap"] = gap
            keep = gap >= c["min_gap"]
            np.add.at(conf, (y[keep], order[keep, 0]), 1)            # rows = label, columns = argmax; close calls left out
            top1 += int((order[:, 0] == y).sum())
            top2 += int(((order[:, 0] == y) | (order[:, 1] == y)).sum())
            rows += len(y)
            gaps.append(gap)
        gaps = np.concatenate(gaps)
        excluded = float((gaps < c["min_gap"]).mean())
        # the condition on the fixture: the reference alone must satisfy it (else change the seed / head scale in recipe.py)
        assert excluded <= c["max_excluded"], (l, excluded)
        out[f"level{l}/confusion"] = conf
        out[f"level{l}/counts"] = np.array([rows, top1, top2], np.int64)       # all rows, ties towards the lower index
        print(f"level {l}: {classes} classes, {rows} rows, top-1 {top1}, top-2 {top2}, excluded {excluded:.3f}, min gap {gaps.min():.2e}")
    path = os.path.join(HERE, "validation_epoch.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "SHA256SUMS"), "w") as f:
        f.write("{}  validation_epoch.npz\n".format(hashlib.sha256(open(path, "rb").read()).hexdigest()))
    print("validation_epoch.npz", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
