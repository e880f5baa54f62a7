"""Generate tests/golden/field/field_reference.npz and field_rules.json by running the REFERENCE ITSELF (build container
only; needs pandas).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_field_golden.py <path of a checkout of the reference>

Imports the reference's src/data.py read-only, its absent third-party imports stubbed (only the import has to succeed),
except the two things filter_data touches: `geopandas.GeoDataFrame` is a pandas.DataFrame subclass with no-op set_crs /
to_crs, and `shapely.geometry.Point` is a tuple.  Then calls its OWN `filter_data` (data.py:22-106) on two tables, each
written as a CSV into a temporary directory with one extra column `row` (the row's position in the table), which is how
the kept rows are recognised in the output -- the reference resets the index of half of them:
  sample     the reference's tests/data/sample_neon.csv: 86 rows, 15 kept, all chosen by height
  synthetic  a few hundred rows made here that reach every step 1-13 of deeptreeattention_amd/field.py's rule and both
             branches of step 9 (asserted below with the package's own reason codes): an individual whose only measured
             height is <= 3 next to a row without height, a shaded individual with one sunny year, remapped and excluded
             taxa, 2014 events, multibole tags, NaN diameters, and no equal eventIDs within an individual

The files hold only data: the input columns deeptreeattention_amd.field needs (strings as unicode arrays with a `_null` mask,
numbers as float64), the reference's kept rows in ITS output order (`<table>_kept`) and its taxonID column
(`<table>_taxon`), the threshold used, and -- field_rules.json -- the lists of names filter_data carries, read out of the
reference's syntax tree as string constants.  No reference source is copied anywhere.  tests/golden/field/SHA256SUMS is
written here."""
import ast
import hashlib
import importlib
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "field")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STRINGS = ("individualID", "eventID", "growthForm", "plantStatus", "canopyPosition", "taxonID", "plotID", "siteID", "utmZone")
NUMBERS = ("itcEasting", "itcNorthing", "height", "stemDiameter")
MIN_STEM_DIAMETER = 10


def import_reference(ref):
    import pandas as pd
    from make_treedata_golden import torchvision_stand_in

    class Anything(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return type(name, (), {})
    for name in ("distributed", "geopandas", "pytorch_lightning", "shapely", "shapely.geometry", "rasterio", "src.generate",
                 "src.CHM", "src.megaplot", "src.neon_paths", "src.models", "src.models.dead"):
        if name not in sys.modules:
            sys.modules[name] = Anything(name)
            sys.modules[name].__all__ = []

    class GeoDataFrame(pd.DataFrame):
        @property
        def _constructor(self):
            return GeoDataFrame

        def set_crs(self, *a, **k):
            return self

        def to_crs(self, *a, **k):
            return self
    sys.modules["geopandas"].GeoDataFrame = GeoDataFrame
    sys.modules["shapely.geometry"].Point = lambda x, y: (x, y)
    torchvision_stand_in()
    pkg = types.ModuleType("src")
    pkg.__path__, pkg.__file__ = [os.path.join(ref, "src")], os.path.join(ref, "src", "__init__.py")
    sys.modules["src"] = pkg
    return importlib.import_module("src.data")


def synthetic(seed=11):
    """A raw field table of a few hundred rows as a pandas frame (see the module's text)."""
    import pandas as pd
    rs = np.random.RandomState(seed)
    sites = [("HARV", "D01"), ("OSBS", "D03"), ("SOAP", "D17"), ("TEAK", "D17"), ("PUUM", "D20"), ("ORNL", "D07"), ("BART", "D01")]
    taxa = ["ACRU", "PIPA2", "QULA2", "TSCA", "PSMEM", "ACSA3", "NYBI", "BEPAC2", "BEPAP", "PINUS", "QUERC", "2PLANT", "FRAXI"]
    growth = ["single bole tree", "multi-bole tree", "small tree", "liana", "small shrub", None]
    status = ["Live", "Live, insect damaged", "Live, physically damaged", "Standing dead", "Lost, fate unknown", None]
    canopy = ["Full sun", "Open grown", "Partially shaded", "Mostly shaded", "Full shade", None]
    rows = []

    def add(name, site, plot, taxon, years, heights, canopies, **over):
        for k, year in enumerate(years):
            rows.append(dict(individualID=name, eventID="vst_{}_{}".format(site, year), siteID=site, plotID=plot, taxonID=taxon,
                             utmZone="17N", itcEasting=400000.0 + 0.5 * len(rows), itcNorthing=3300000.0 + 0.25 * len(rows),
                             growthForm="single bole tree", plantStatus="Live", canopyPosition=canopies[k], height=heights[k],
                             stemDiameter=25.0, **over))

    # the cases the table must hold, by hand
    add("NEON.PLA.D01.HARV.90001", "HARV", "HARV_001", "ACRU", (2016, 2018), (2.5, np.nan), ("Full sun", "Full sun"))
    add("NEON.PLA.D01.HARV.90002", "HARV", "HARV_001", "TSCA", (2015, 2016, 2017), (12.0, 12.5, 13.0),
        ("Full shade", "Open grown", "Mostly shaded"))
    add("NEON.PLA.D01.HARV.90003", "HARV", "HARV_002", "TSCA", (2015, 2016), (9.0, 9.5), ("Full shade", "Mostly shaded"))
    add("NEON.PLA.D01.HARV.90004", "HARV", "HARV_002", "ACRU", (2019, 2015, 2017), (np.nan, np.nan, np.nan), (None, None, None))
    add("NEON.PLA.D01.HARV.90005", "HARV", "HARV_003", "QULA2", (2015, 2016, 2017), (14.0, 14.0, 11.0), ("Full sun",) * 3)
    add("NEON.PLA.D03.OSBS.03382", "OSBS", "OSBS_001", "PIPA2", (2016,), (17.0,), ("Full sun",))
    add("NEON.PLA.D17.TEAK.01883", "TEAK", "TEAK_004", "ACRU", (2017,), (np.nan,), ("Full sun",))
    add("NEON.PLA.D17.SOAP.90006", "SOAP", "SOAP_054", "ACRU", (2017,), (8.0,), ("Full sun",))
    add("NEON.PLA.D03.OSBS.90007", "OSBS", "OSBS_027", "PIPA2", (2017,), (np.nan,), ("Open grown",))
    for k in range(170):
        site, domain = sites[rs.randint(len(sites))]
        name = "NEON.PLA.{}.{}.{:05d}{}".format(domain, site, 1000 + k, "ABC"[rs.randint(3)] if rs.rand() < 0.12 else "")
        plot = "{}_{:03d}".format(site, rs.choice([26, 27, 29, 36, 39, 54]) if rs.rand() < 0.15 else rs.randint(1, 20))
        years = 2014 + rs.permutation(6)[:rs.randint(1, 6)]
        base = canopy[rs.randint(len(canopy))]
        no_height = rs.rand() < 0.3
        for year in years:
            rows.append(dict(
                individualID=name, eventID="vst_{}_{}".format(site, year), siteID=site, plotID=plot,
                taxonID=taxa[rs.randint(len(taxa))] if rs.rand() < 0.1 else taxa[k % len(taxa)], utmZone="17N",
                itcEasting=np.nan if rs.rand() < 0.06 else 400000.0 + rs.randint(0, 4000) * 0.25,
                itcNorthing=3300000.0 + rs.randint(0, 4000) * 0.25,
                growthForm=growth[rs.randint(len(growth))] if rs.rand() < 0.25 else "single bole tree",
                plantStatus=status[rs.randint(len(status))] if rs.rand() < 0.3 else "Live",
                canopyPosition=canopy[rs.randint(len(canopy))] if rs.rand() < 0.3 else base,
                height=np.nan if no_height or rs.rand() < 0.25 else float(rs.randint(2, 120)) * 0.25,
                stemDiameter=np.nan if rs.rand() < 0.06 else float(rs.randint(2, 200)) * 0.25))
    df = pd.DataFrame(rows)
    df = df.iloc[rs.permutation(len(df))].reset_index(drop=True)            # individuals interleaved
    return df


def record(data, name, df, D, tmp):
    """Run the reference on df (written as CSV with a `row` column) and record the inputs and its answer under `name`."""
    import pandas as pd
    df = df.reset_index(drop=True).copy()
    df["row"] = np.arange(len(df))
    path = os.path.join(tmp, name + ".csv")
    df.to_csv(path, index=False)
    out = D.filter_data(path, {"min_stem_diameter": MIN_STEM_DIAMETER})
    back = pd.read_csv(path)                                                # what the reference saw
    for k in STRINGS:
        col = back[k].to_numpy(dtype=object)
        null = np.array([v is None or v != v for v in col], bool)
        data["{}_{}".format(name, k)] = np.array(["" if n else str(v) for v, n in zip(col, null)])
        data["{}_{}_null".format(name, k)] = null
    for k in NUMBERS:
        data["{}_{}".format(name, k)] = back[k].to_numpy(dtype=np.float64)
    data[name + "_kept"] = out["row"].to_numpy().astype(np.int64)
    data[name + "_taxon"] = out["taxonID"].to_numpy().astype(str)
    data[name + "_individual"] = out["individual"].to_numpy().astype(str)
    assert len(set(data[name + "_kept"].tolist())) == len(out)
    return back, data[name + "_kept"]


def rule_lists(ref):
    """The names filter_data carries, read out of its syntax tree: string constants only."""
    tree = ast.parse(open(os.path.join(ref, "src", "data.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "filter_data")
    text = lambda n: n.value if isinstance(n, ast.Constant) and isinstance(n.value, str) else None      # noqa: E731
    lists, remap, contains, equals = [], [], [], []
    for n in ast.walk(fn):
        if isinstance(n, ast.List) and n.elts and all(text(e) is not None for e in n.elts):
            lists.append([text(e) for e in n.elts])
        if (isinstance(n, ast.Assign) and text(n.value) is not None and isinstance(n.targets[0], ast.Subscript)
                and isinstance(n.targets[0].slice, ast.Tuple) and isinstance(n.targets[0].slice.elts[0], ast.Compare)):
            remap.append([text(n.targets[0].slice.elts[0].comparators[0]), text(n.value)])
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "contains":
            contains.append(text(n.args[0]))
        if isinstance(n, ast.Compare) and isinstance(n.left, ast.Attribute) and n.left.attr == "plotID":
            equals.append(text(n.comparators[0]))
    by_first = {l[0]: l for l in lists}
    return {"growth_excluded": by_first["liana"], "status_contains": contains[0], "shaded": by_first["Full shade"],
            "sunny": by_first["Open grown"], "remap": remap, "taxa_excluded": by_first["BETUL"], "event_excluded": contains[1],
            "multibole": contains[2], "known_errors": by_first["NEON.PLA.D03.OSBS.03422"],
            "plots_excluded": equals + by_first["OSBS_026"], "sites_excluded": by_first["PUUM"]}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isfile(os.path.join(args[0], "src", "data.py")):
        sys.exit("usage: make_field_golden.py <path of a checkout of the reference>")
    import pandas as pd
    warnings.simplefilter("ignore")
    ref = args[0]
    D = import_reference(ref)
    from deeptreeattention_amd import field
    data = {"min_stem_diameter": np.float64(MIN_STEM_DIAMETER)}
    with tempfile.TemporaryDirectory() as tmp:
        tables = {"sample": pd.read_csv(os.path.join(ref, "tests", "data", "sample_neon.csv")), "synthetic": synthetic()}
        for name, df in tables.items():
            back, kept = record(data, name, df, D, tmp)
            table = field.FieldTable.from_frame(back)
            got = table.filter(MIN_STEM_DIAMETER)
            seen = np.bincount(got.reason, minlength=14)
            h = table.columns["height"]
            by_event = int(np.isnan(h[got.reason == 0]).sum()) + int(np.isnan(h[got.reason >= 10]).sum())
            print(name, len(back), "rows,", len(kept), "kept; reasons 0..13:", seen.tolist(), "; records chosen by event:", by_event)
            assert np.array_equal(got.index(), kept), name
            if name == "synthetic":
                assert seen.min() >= 1 and by_event >= 3 and int((~np.isnan(h[got.reason == 0])).sum()) >= 3
                for who, group in back[back.height.isnull()].groupby("individualID"):
                    assert group.eventID.is_unique
    rules = rule_lists(ref)
    assert rules == field.Rules.reference().as_lists(), rules
    os.makedirs(GOLDEN, exist_ok=True)
    out = os.path.join(GOLDEN, "field_reference.npz")
    np.savez_compressed(out, **data)
    rules_out = os.path.join(GOLDEN, "field_rules.json")
    with open(rules_out, "w") as f:
        json.dump(rules, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        for p in (out, rules_out):
            f.write("{}  {}\n".format(hashlib.sha256(open(p, "rb").read()).hexdigest(), os.path.basename(p)))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
