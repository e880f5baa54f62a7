"""Generate tests/golden/multistage_ensemble.json by running the REFERENCE ITSELF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_ensemble_golden.py <path of a checkout of the reference>

Imports the reference's src/models/multi_stage.py read-only (its GIS / Lightning / torchmetrics imports are stubbed the
way tests/golden/make_golden.py stubs them: only the import has to succeed) and calls `MultiStage.gather_predictions`
(multi_stage.py:368-402) and `MultiStage.ensemble` (:404-434) UNBOUND on a stub object that carries the two attributes
they read, `label_to_taxonIDs` and `species_label_dict`.  Needs pandas besides NumPy and torch.

The file holds only data: the five {taxonID: label} dictionaries, the species dictionary, the per-level probability rows
(float32 bit patterns, so they round-trip exactly), and the reference's `individual`, `ensembleTaxonID`, `ens_label`,
`ens_score` (bit pattern) and per-level top-1 columns.  No reference source is copied anywhere.

Conditions on the inputs, asserted here and again by the tests that load the file:
  * individuals are unique.  With repeats `gather_predictions` takes `argmax` of a FLATTENED stack of the crown's rows
    (an index into rows x classes, not a class) -- a quirk not worth reproducing;
  * the reference returns its rows sorted by `individual` as strings: consumers join on the name, not on position;
  * no two classes of a row tie for first place;
  * each of the four terminal branches (level 0, level 2 non-oak, level 3, level 4) is taken by at least 8 rows,
    counted on the reference's own output.
"""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "multistage_ensemble.json")
sys.dont_write_bytecode = True

ROWS, BATCH, SEED = 256, 64, 20240611
LEVEL_LABEL_DICTS = [
    {"PIPA2": 0, "OTHER": 1},
    {"CONIFER": 0, "BROADLEAF": 1},
    {"ACRU": 0, "OAK": 1, "NYSY": 2},
    {"PICL": 0, "PIEL": 1, "PITA": 2},
    {"QUGE2": 0, "QULA2": 1, "QUNI": 2},
]
SPECIES = ["ACRU", "NYSY", "PICL", "PIEL", "PIPA2", "PITA", "QUGE2", "QULA2", "QUNI"]


def _stub_missing_packages():
    """Every package the reference imports that is absent here becomes an empty stub module (only the import has to
    succeed: gather_predictions and ensemble use pandas and NumPy alone)."""
    import torch
    roots = {"pytorch_lightning", "torchmetrics", "geopandas", "rasterio", "comet_ml", "deepforest", "dask", "distributed",
             "h5py", "shapely", "rasterstats", "skimage", "torchvision", "descartes", "pyproj", "rtree", "cv2", "seaborn",
             "albumentations", "imblearn"}

    class Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return Anything()

        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return Anything()

    class Stub(types.ModuleType):
        __path__ = []

        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            v = Anything()
            setattr(self, k, v)
            return v

    class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        def find_spec(self, name, path, target=None):
            if name.split(".")[0] in roots and name not in sys.modules:
                return importlib.machinery.ModuleSpec(name, self, is_package=True)

        def create_module(self, spec):
            return Stub(spec.name)

        def exec_module(self, module):
            pass

    sys.meta_path.insert(0, Finder())
    import pytorch_lightning as pl
    pl.LightningModule = type("LightningModule", (torch.nn.Module,), {})
    pl.LightningDataModule = type("LightningDataModule", (), {})


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "models", "multi_stage.py")):
        sys.exit("usage: make_ensemble_golden.py <path of a checkout of the reference>")
    _stub_missing_packages()
    sys.path.insert(0, sys.argv[1])
    from src.models.multi_stage import MultiStage

    rng = np.random.default_rng(SEED)
    classes = [len(d) for d in LEVEL_LABEL_DICTS]
    probs = []
    for c in classes:
        z = rng.standard_normal((ROWS, c)) * 1.5
        p = np.exp(z - z.max(1, keepdims=True))
        probs.append((p / p.sum(1, keepdims=True)).astype(np.float32))
    for p in probs:                                   # no two classes of a row tie for first place
        top = np.sort(p, 1)
        assert (top[:, -1] > top[:, -2]).all()
    # names that do NOT sort in row order (the reference sorts by name as strings: "crown_10" < "crown_9")
    individuals = ["crown_{}".format(i) for i in rng.permutation(ROWS)]
    assert len(set(individuals)) == ROWS

    stub = types.SimpleNamespace(label_to_taxonIDs=[{v: k for k, v in d.items()} for d in LEVEL_LABEL_DICTS],
                                 species_label_dict={t: i for i, t in enumerate(SPECIES)})
    predict_df = [(individuals[lo:lo + BATCH], [p[lo:lo + BATCH] for p in probs]) for lo in range(0, ROWS, BATCH)]
    results = MultiStage.gather_predictions(stub, predict_df)
    ens = MultiStage.ensemble(stub, results)
    assert len(ens) == ROWS and list(ens.individual) == sorted(individuals)

    # every terminal branch is taken often enough, on the reference's own columns
    t0, t1, t2 = (ens["pred_taxa_top1_level_{}".format(l)] for l in range(3))
    branch = {"level0": int((t0 == "PIPA2").sum()),
              "level2": int(((t0 != "PIPA2") & (t1 == "BROADLEAF") & (t2 != "OAK")).sum()),
              "level3": int(((t0 != "PIPA2") & (t1 != "BROADLEAF")).sum()),
              "level4": int(((t0 != "PIPA2") & (t1 == "BROADLEAF") & (t2 == "OAK")).sum())}
    assert sum(branch.values()) == ROWS and min(branch.values()) >= 8, branch

    out = {"level_label_dicts": LEVEL_LABEL_DICTS,
           "species_label_dict": stub.species_label_dict,
           "input": {"individual": individuals, "probs_bits": [[bits(r) for r in p] for p in probs]},
           "reference": {"individual": list(ens.individual),
                         "ensembleTaxonID": list(ens.ensembleTaxonID),
                         "ens_label": [int(v) for v in ens.ens_label],
                         "ens_score_bits": bits(ens.ens_score.to_numpy(np.float32)),
                         "pred_label_top1": [[int(v) for v in ens["pred_label_top1_level_{}".format(l)]] for l in range(5)],
                         "top1_score_bits": [bits(ens["top1_score_level_{}".format(l)].to_numpy(np.float32)) for l in range(5)]},
           "branch_counts": branch}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes", branch)


if __name__ == "__main__":
    main()
