"""Generate tests/golden/evaluate/evaluate_reference.npz and evaluate_reference.json by running the REFERENCE ITSELF (build
container only; needs pandas and torch, which the reference's src/metrics.py imports).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_evaluate_golden.py <path of a checkout of the reference>

Imports the reference's src/metrics.py read-only; its one project import (`from src import data`, used by novel_prediction
only) is stubbed, as tools/make_field_golden.py stubs src/data.py's.  Then calls its OWN `site_confusion` and
`genus_confusion` (metrics.py:8-72) on plain Python lists and dicts and records what they return.  Cases:
  ref_site_same, ref_site_disjoint, ref_genus_within, ref_genus_cross
             the four cases of the reference's tests/test_metrics.py, restated as arrays (their scientific names are plain
             strings: "QUMU" and "QUMLA" are one genus only because `value[0]` is the first CHARACTER)
  synthetic  about 600 rows, 40 species, 7 sites, 420 individuals with repeated rows: species on several sites, a species
             pair with disjoint sites (3, 4), names given as lists and as plain strings so that the first-character quirk
             decides pairs both ways (0 ["Quercus alba"] vs 1 "Quercus rubra": "Quercus" != "Q"; 1 vs 2 "Quamoclit
             coccinea": "Q" == "Q").  The reference's figures are taken on the first row of every individual
             (pandas' groupby("individual").head(1), recorded as `synthetic_first`), as evaluation_scores does.
  no_error   every prediction right: both functions return 0

The files hold only data: labels, predictions, site and individual codes as integer arrays (.npz, written with fixed zip
timestamps so that a rerun reproduces the bytes), and per case the two tables and the reference's two numbers (.json).  No
reference source is copied anywhere.  tests/golden/evaluate/SHA256SUMS is written here."""
import hashlib
import importlib
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "evaluate")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.path.insert(0, REPO)

SITES = ("BART", "HARV", "OSBS", "SOAP", "TEAK", "UNDE", "WREF")
SPECIES, ROWS, INDIVIDUALS = 40, 600, 420


def import_reference(ref):
    pkg = types.ModuleType("src")
    pkg.__path__, pkg.__file__ = [os.path.join(ref, "src")], os.path.join(ref, "src", "__init__.py")
    sys.modules["src"] = pkg
    sys.modules["src.data"] = types.ModuleType("src.data")
    pkg.data = sys.modules["src.data"]
    return importlib.import_module("src.metrics")


def synthetic(seed=23):
    rs = np.random.RandomState(seed)
    site_lists = {}
    for k in range(SPECIES):
        site_lists[k] = sorted(SITES[i] for i in rs.permutation(len(SITES))[:rs.randint(1, 4)])
    site_lists[3], site_lists[4] = ["BART"], ["OSBS"]                     # a pair that shares no site
    site_lists[0], site_lists[1], site_lists[2] = ["HARV", "BART"], ["HARV"], ["HARV", "TEAK"]
    genera = ("Acer", "Pinus", "Betula", "Carya", "Fagus", "Tsuga", "Nyssa", "Abies")
    scientific = {}
    for k in range(SPECIES):
        name = "{} species{}".format(genera[k % len(genera)], k)
        scientific[k] = [name] if k % 3 else name                         # a list: the first word; a string: its first letter
    scientific[0], scientific[1], scientific[2] = ["Quercus alba"], "Quercus rubra", "Quamoclit coccinea"
    individual = np.concatenate([np.arange(INDIVIDUALS), rs.randint(0, INDIVIDUALS, ROWS - INDIVIDUALS)])
    individual = individual[rs.permutation(ROWS)].astype(np.int64)
    true_of = rs.randint(0, SPECIES, INDIVIDUALS)
    true_of[:12] = (0, 1, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2)
    site_of = np.array([SITES.index(site_lists[int(t)][rs.randint(len(site_lists[int(t)]))]) for t in true_of])
    y_true = true_of[individual].astype(np.int64)
    y_pred = np.where(rs.rand(ROWS) < 0.62, y_true, rs.randint(0, SPECIES, ROWS)).astype(np.int64)
    forced = {0: 1, 1: 0, 2: 2, 3: 1, 4: 4, 5: 3, 6: 1, 7: 2, 8: 1, 9: 4, 10: 3, 11: 1}     # individual -> prediction, every row
    for who, p in forced.items():
        y_pred[individual == who] = p
    return {"true": y_true, "pred": y_pred, "site": site_of[individual].astype(np.int64), "individual": individual,
            "site_lists": site_lists, "scientific": scientific}


def cases():
    five = np.array([0, 0, 1, 1, 1], np.int64)
    names = {0: "ACRU", 1: "QUMU", 2: "QUMLA"}
    out = {
        "ref_site_same": {"true": five, "pred": np.array([0, 0, 1, 1, 0], np.int64), "site_lists": {0: [0], 1: [0]}},
        "ref_site_disjoint": {"true": five, "pred": np.array([0, 0, 1, 1, 0], np.int64), "site_lists": {0: [1], 1: [0]}},
        "ref_genus_within": {"true": five, "pred": np.array([0, 0, 1, 1, 2], np.int64), "scientific": names},
        "ref_genus_cross": {"true": five, "pred": np.array([0, 0, 1, 1, 0], np.int64), "scientific": names},
        "synthetic": synthetic(),
    }
    rs = np.random.RandomState(5)
    same = rs.randint(0, 6, 50).astype(np.int64)
    out["no_error"] = {"true": same, "pred": same.copy(), "site_lists": {k: [SITES[k % 3]] for k in range(6)},
                       "scientific": {k: ["Genus{} x".format(k % 2)] for k in range(6)}}
    return out


def write_npz(path, arrays):
    """np.load reads it; fixed member timestamps, so the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isfile(os.path.join(args[0], "src", "metrics.py")):
        sys.exit("usage: make_evaluate_golden.py <path of a checkout of the reference>")
    import pandas as pd
    M = import_reference(args[0])
    from deeptreeattention_amd import evaluate
    arrays, tables = {}, {}
    for name, c in cases().items():
        y_true, y_pred = c["true"], c["pred"]
        for k in ("true", "pred", "site", "individual"):
            if k in c:
                arrays["{}_{}".format(name, k)] = c[k]
        if "individual" in c:
            frame = pd.DataFrame({"individual": c["individual"], "row": np.arange(len(y_true))})
            first = np.zeros(len(y_true), bool)
            first[frame.groupby("individual").head(1)["row"].to_numpy()] = True
            arrays[name + "_first"] = first
            y_true, y_pred = y_true[first], y_pred[first]
        rec = {}
        if "site_lists" in c:
            rec["site_lists"] = {str(k): list(v) for k, v in c["site_lists"].items()}
            rec["site_confusion"] = float(M.site_confusion(y_true.tolist(), y_pred.tolist(), c["site_lists"]))
        if "scientific" in c:
            rec["scientific"] = {str(k): v for k, v in c["scientific"].items()}
            rec["genus_confusion"] = float(M.genus_confusion(y_true.tolist(), y_pred.tolist(), c["scientific"]))
        tables[name] = rec
        # the package's definitions agree, or the fixture is not written
        S = int(max(y_true.max(), y_pred.max(), max(c.get("site_lists", {0: 0}).keys()), max(c.get("scientific", {0: 0}).keys()))) + 1
        conf, _ = evaluate.count_np(y_true, y_pred, n_species=S)
        r = evaluate.report_np(conf, evaluate.site_masks(c["site_lists"], S) if "site_lists" in c else None,
                               evaluate.genus_ids(c["scientific"], S) if "scientific" in c else None)
        if "site_lists" in c:
            assert r["scores"][1, 2] == rec["site_confusion"], name
        if "scientific" in c:
            assert r["scores"][1, 3] == rec["genus_confusion"], name
        print(name, len(y_true), "rows,", int(r["counts"][1, 2]), "errors:", {k: v for k, v in rec.items() if k.endswith("confusion")})
    s = cases()["synthetic"]
    first = arrays["synthetic_first"]
    t, p = s["true"][first], s["pred"][first]
    genus = evaluate.genus_ids(s["scientific"], SPECIES)
    assert genus[0] != genus[1] and genus[1] == genus[2]
    assert ((t == 0) & (p == 1)).any() and ((t == 1) & (p == 2)).any() and ((t == 3) & (p == 4)).any() and ((t == 4) & (p == 3)).any()
    assert first.sum() == INDIVIDUALS and 0.0 < tables["synthetic"]["site_confusion"] < 1.0
    assert 0.0 < tables["synthetic"]["genus_confusion"] < 1.0
    os.makedirs(GOLDEN, exist_ok=True)
    out = os.path.join(GOLDEN, "evaluate_reference.npz")
    write_npz(out, arrays)
    tables_out = os.path.join(GOLDEN, "evaluate_reference.json")
    with open(tables_out, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        for path in (out, tables_out):
            f.write("{}  {}\n".format(hashlib.sha256(open(path, "rb").read()).hexdigest(), os.path.basename(path)))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
