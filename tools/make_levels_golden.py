"""Generate tests/golden/levels/levels_reference.npz by running the REFERENCE ITSELF (build container only; needs pandas).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_levels_golden.py <path of a checkout of the reference> [--time]

Imports the reference's src/models/multi_stage.py read-only -- its third-party imports are stubbed (only the import has to
succeed; `LightningModule` is an `nn.Module` with a no-op `save_hyperparameters`), torch and pandas are the real ones -- and
runs its OWN `MultiStage.__init__` (and so `create_datasets`, :82-219, and the loss weights, :62-79) on seeded synthetic
annotation frames.  `pandas.DataFrame.sample` is wrapped to log the index of every frame it returns: the calls level 2
makes (the frames whose taxonID is "OAK" throughout) are its per-species shuffles, recorded as orders of record numbers.

The file holds only data.  Per case k: the input columns of both frames, integer-coded (`c<k>_<train|test>_individual` in
order of first appearance, `_year`, `_label`), the names (`_names`, by individual code; `c<k>_taxa`, by label;
`c<k>_dict_order`, the labels in the key order of the reference's species_label_dict), `c<k>_ceilings` (other, evergreen,
oaks) and `c<k>_min_loss_weight`, the logged level-2 orders (`c<k>_l2_species`, `c<k>_l2_orders` padded with -1), per level
and frame the individuals in data set order (`c<k>_<train|test>_L<l>_individuals`), their labels (`_labels`) and the kept
(individual, year) pairs (`_pairs`, sorted), `c<k>_num_classes` and the `loss_weight_<l>` buffers as registered
(`c<k>_loss_weight_<l>`, float32).  No reference source is copied anywhere.  tests/golden/levels/SHA256SUMS is written here.

What the frames contain is asserted in check_case below.  --time prints the reference's seconds per create_datasets call on a
frame of about 3,000 individuals (pandas, this CPU)."""
import hashlib
import importlib
import os
import sys
import time
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "levels")
OUT = os.path.join(GOLDEN, "levels_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

HEAD, CONIFERS = "PIPA2", ("PICL", "PIEL", "PITA")
YEARS = (2019, 2020, 2021)
# individuals per taxon of the train and the test frame; conifer_mod: the CONIFER record count modulo 11 the frame must have
CASES = (
    dict(train={"PIPA2": 9, "PICL": 5, "PIEL": 4, "PITA": 3, "QUGE2": 7, "QULA2": 5, "QUHE2": 1, "QUNI": 3,
                "ACRU": 6, "LIST2": 7, "NYSY": 4, "MAGR4": 9, "CAGL8": 2},
         test={"PICL": 3, "PITA": 2, "QUGE2": 3, "QULA2": 2, "ACRU": 3, "MAGR4": 2, "NYSY": 1},      # no HEAD
         ceilings=(6, 7, 4), min_loss_weight=0.2, conifer_mod=0),
    dict(train={"PIPA2": 4, "PICL": 6, "PIEL": 2, "PITA": 5, "QUGE2": 6, "QULA2": 2, "QUNI": 4,
                "ACRU": 5, "LIST2": 3, "MAGR4": 8},
         test={"PIPA2": 2, "PICL": 2, "PIEL": 1, "QUGE2": 2, "QUNI": 2, "ACRU": 2, "LIST2": 2},
         ceilings=(4, 5, 3), min_loss_weight=0.35, conifer_mod=1),
    dict(train={"PIPA2": 3, "PICL": 4, "PITA": 4, "QUGE2": 4, "QULA2": 3, "ACRU": 2},                 # k2 = 0
         test={"PIPA2": 1, "PICL": 2, "QUGE2": 2, "ACRU": 1},
         ceilings=(3, 4, 2), min_loss_weight=0.1, conifer_mod=None, plain_records=4),
)
BIG = {"PIPA2": 900, "PICL": 150, "PIEL": 90, "PITA": 120, "QUGE2": 400, "QULA2": 380, "QUHE2": 60, "QUNI": 100,
       "ACRU": 200, "LIST2": 150, "NYSY": 120, "MAGR4": 230, "CAGL8": 100}


def frame(counts, labels, seed, prefix):
    """A synthetic annotation frame: 1..3 years per individual, one duplicated (individual, year) row, rows shuffled."""
    import pandas as pd
    rs = np.random.RandomState(seed)
    rows = []
    serial = rs.permutation(100000)
    at = 0
    for taxon, count in counts.items():
        for _ in range(count):
            name = "NEON.PLA.%s.%d" % (prefix, serial[at])      # not zero-padded: string order is not numeric order
            at += 1
            for y in rs.choice(len(YEARS), size=rs.randint(1, 4), replace=False):
                rows.append((name, YEARS[y], taxon, labels[taxon], "%s_%d.tif" % (name, YEARS[y])))
    rows.append(rows[rs.randint(len(rows))])
    order = rs.permutation(len(rows))
    return pd.DataFrame([rows[k] for k in order], columns=["individual", "tile_year", "taxonID", "label", "image_path"])


def codes(values):
    v = np.asarray(values).astype(str)
    names, first, inverse = np.unique(v, return_index=True, return_inverse=True)
    rank = np.empty(len(names), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(names))
    return rank[inverse.reshape(-1)], names[np.argsort(first, kind="stable")]


def acceptable(case, train):
    """The record counts a case's train frame must have (the frame seed is searched for them)."""
    con = int(train.taxonID.isin(CONIFERS).sum())
    if case["conifer_mod"] is not None and con % 11 != case["conifer_mod"]:
        return False
    plain = int((~train.taxonID.isin(CONIFERS + (HEAD,)) & ~train.taxonID.str.contains("QU")).sum())
    if "plain_records" in case and plain != case["plain_records"]:
        return False
    # level 3: the ceiling must cut an individual between its years
    ec = case["ceilings"][1]
    for _, g in train[train.taxonID.isin(CONIFERS)].groupby("taxonID"):
        kept, cut = g.head(ec), g.iloc[ec:]
        both = set(kept.individual) & set(cut.individual)
        if any(set(cut[cut.individual == i].tile_year) - set(kept[kept.individual == i].tile_year) for i in both):
            return True
    return False


def check_case(k, case, train, test, result, orders):
    ic, _ = codes(train.individual)
    assert not np.array_equal(np.argsort(np.asarray(train.individual.unique()).astype(str), kind="stable"),
                              np.arange(ic.max() + 1)), "names are in string order"
    assert train.duplicated(["individual", "tile_year"]).any()
    per = train.groupby("individual").tile_year.nunique()
    assert {1, 2, 3} <= set(per.values)
    oc, ec, qc = case["ceilings"]
    n = train[train.taxonID != HEAD].groupby("taxonID").individual.nunique()
    if k == 0:
        assert oc in n.values and oc + 1 in n.values and (n < oc).any()
        assert HEAD not in set(test.taxonID)
        w = [result["loss_weight_%d" % l] for l in range(5)]
        assert any((x == np.float32(case["min_loss_weight"])).any() and (x > np.float32(case["min_loss_weight"])).sum() > 1 for x in w)
    plain = int((~train.taxonID.isin(CONIFERS + (HEAD,)) & ~train.taxonID.str.contains("QU")).sum())
    k2 = plain // 5
    if k == 2:
        assert k2 == 0 and not orders_pick_anything(orders, k2)
    else:
        oak = train[train.taxonID.str.contains("QU")]
        assert k2 > 0 and (oak.groupby("taxonID").size() < k2).any(), "no OAK species with fewer than k2 records"
    l3 = result["train"][3]
    first = {n: i for i, n in enumerate(train.individual.unique())}
    at = [first[n] for n in l3["individuals"]]
    assert at != sorted(at), "level 3's regrouping does not show"
    have = {(r.individual, r.tile_year) for r in train.itertuples()}
    assert any((i, y) not in set(l3["pairs"]) for i, y in have if i in set(l3["individuals"])), "level 3 cuts no year"


def orders_pick_anything(orders, k2):
    return k2 > 0 and any(len(o) for o in orders.values())


def twice_among_first(train, orders, k2):
    """An OAK individual two of whose records both fall among the first k2 of its species' shuffle."""
    ind = train.individual.to_numpy()
    for o in orders.values():
        head = ind[np.asarray(o[:k2], np.int64)]
        if len(set(head.tolist())) < len(head):
            return True
    return False


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isfile(os.path.join(args[0], "src", "models", "multi_stage.py")):
        sys.exit("usage: make_levels_golden.py <path of a checkout of the reference> [--time]")
    import pandas as pd
    import torch
    warnings.simplefilter("ignore")
    ref = args[0]

    class Whatever:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return Whatever()

    class Anything(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return type(name, (Whatever,), {})

    for name in ("distributed", "geopandas", "pytorch_lightning", "shapely", "shapely.geometry", "rasterio", "torchmetrics",
                 "torchvision", "sklearn", "yaml", "src.generate", "src.CHM", "src.augmentation", "src.megaplot",
                 "src.neon_paths", "src.models.dead", "src.utils"):
        if name not in sys.modules:
            sys.modules[name] = Anything(name)
            sys.modules[name].__all__ = []

    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass
    sys.modules["pytorch_lightning"].LightningModule = LightningModule
    for pkg_name, sub in (("src", "src"), ("src.models", os.path.join("src", "models"))):
        pkg = types.ModuleType(pkg_name)
        pkg.__path__, pkg.__file__ = [os.path.join(ref, sub)], os.path.join(ref, sub, "__init__.py")
        sys.modules[pkg_name] = pkg
    M = importlib.import_module("src.models.multi_stage")

    log = []
    plain_sample = pd.DataFrame.sample

    def logged_sample(self, *a, **k):
        out = plain_sample(self, *a, **k)
        log.append((self, out.index.to_numpy().copy()))
        return out
    pd.DataFrame.sample = logged_sample

    def run(train, test, case, seed):
        """The reference's MultiStage on copies of the frames; returns its data sets as plain data and level 2's orders."""
        del log[:]
        config = {"other_sampling_ceiling": case["ceilings"][0], "evergreen_ceiling": case["ceilings"][1],
                  "oaks_sampling_ceiling": case["ceilings"][2], "min_loss_weight": case["min_loss_weight"], "image_size": 11,
                  "preload_images": False, "pretrain_state_dict": None, "bands": 4, "crop_dir": ""}
        np.random.seed(seed)
        m = M.MultiStage(train.copy(), test.copy(), crowns=None, config=config)
        # level 2 shuffles frames whose taxonID is "OAK" throughout; their index numbers the rows of the frame without
        # HEAD and CONIFER records, re-indexed from 0 (:150)
        outside = np.flatnonzero(~train.taxonID.isin(CONIFERS + (HEAD,)).to_numpy())
        orders = {}
        for f, index in log:
            if (f.taxonID == "OAK").all():
                label = int(f.label.iloc[0])
                assert label not in orders and (f.label == label).all()
                orders[label] = outside[index]
        result = {"train": [], "test": [], "num_classes": list(m.num_classes), "dict_keys": list(m.species_label_dict)}
        for which, sets in (("train", m.train_datasets), ("test", m.test_datasets)):
            for ds in sets:
                pairs = sorted((i, int(y)) for i in ds.individuals for y in ds.image_paths[i])
                result[which].append({"individuals": list(ds.individuals), "labels": [int(ds.labels[i]) for i in ds.individuals],
                                      "pairs": pairs})
        for l in range(5):
            result["loss_weight_%d" % l] = getattr(m, "loss_weight_%d" % l).numpy().copy()
        return result, orders

    data, found = {"cases": np.int64(len(CASES))}, []
    for k, case in enumerate(CASES):
        taxa = sorted(case["train"])
        labels = {t: i for i, t in enumerate(taxa)}
        train = next(f for f in (frame(case["train"], labels, 1000 * k + s, "A%d" % k) for s in range(2000)) if acceptable(case, f))
        test = frame(case["test"], labels, 50000 + k, "B%d" % k)
        plain = int((~train.taxonID.isin(CONIFERS + (HEAD,)) & ~train.taxonID.str.contains("QU")).sum())
        k2 = plain // 5
        for seed in range(200):      # case 0 wants a shuffle that names an individual twice among the first k2
            result, orders = run(train, test, case, seed)
            if k != 0 or twice_among_first(train, orders, k2):
                break
        else:
            raise AssertionError("no shuffle names an individual twice")
        found.append(twice_among_first(train, orders, k2))
        check_case(k, case, train, test, result, orders)
        assert result["dict_keys"] == list(dict.fromkeys(train.taxonID))
        data["c%d_taxa" % k] = np.array(taxa)
        data["c%d_dict_order" % k] = np.array([labels[t] for t in dict.fromkeys(train.taxonID)], np.int64)
        data["c%d_ceilings" % k] = np.array(case["ceilings"], np.int64)
        data["c%d_min_loss_weight" % k] = np.float64(case["min_loss_weight"])
        data["c%d_num_classes" % k] = np.array(result["num_classes"], np.int64)
        species = sorted(orders)
        width = max([len(orders[s]) for s in species] + [1])
        data["c%d_l2_species" % k] = np.array(species, np.int64)
        data["c%d_l2_orders" % k] = np.array([np.pad(orders[s], (0, width - len(orders[s])), constant_values=-1) for s in species],
                                             np.int64).reshape(len(species), width)
        for l in range(5):
            data["c%d_loss_weight_%d" % (k, l)] = result["loss_weight_%d" % l].astype(np.float32)
        for which, df in (("train", train), ("test", test)):
            ic, names = codes(df.individual)
            code = {n: i for i, n in enumerate(names.tolist())}
            p = "c%d_%s_" % (k, which)
            data[p + "individual"], data[p + "names"] = ic.astype(np.int32), names
            data[p + "year"], data[p + "label"] = df.tile_year.to_numpy().astype(np.int32), df.label.to_numpy().astype(np.int32)
            for l, ds in enumerate(result[which]):
                data[p + "L%d_individuals" % l] = np.array([code[i] for i in ds["individuals"]], np.int32)
                data[p + "L%d_labels" % l] = np.array(ds["labels"], np.int32)
                data[p + "L%d_pairs" % l] = np.array([(code[i], y) for i, y in ds["pairs"]], np.int32).reshape(-1, 2)
    assert found[0], "case 0 must name an OAK individual twice among the first k2 records"
    mods = [int(np.isin(data["c%d_taxa" % k][data["c%d_train_label" % k]], CONIFERS).sum()) % 11 for k in range(2)]
    assert mods == [0, 1], mods      # both sides of level 1's ceil

    if "--time" in sys.argv:
        taxa = sorted(BIG)
        big = frame(BIG, {t: i for i, t in enumerate(taxa)}, 7, "T")
        m = M.MultiStage(big.copy(), big.iloc[:500].copy(), None, {"other_sampling_ceiling": 100, "evergreen_ceiling": 200,
                         "oaks_sampling_ceiling": 150, "min_loss_weight": 0.01, "image_size": 11, "preload_images": False,
                         "pretrain_state_dict": None, "bands": 4})
        t0 = time.perf_counter()
        for _ in range(3):
            m.create_datasets()
        print("reference create_datasets (pandas {}): {:.3f} s per call, {} individuals, {} records".format(
            pd.__version__, (time.perf_counter() - t0) / 3, big.individual.nunique(), len(big)))

    pd.DataFrame.sample = plain_sample
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(OUT, **data)
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes;", len(CASES), "cases")


if __name__ == "__main__":
    main()
