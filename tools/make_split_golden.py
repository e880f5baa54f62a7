"""Generate tests/golden/split/split_reference.npz by running the REFERENCE ITSELF (build container only; needs pandas).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_split_golden.py <path of a checkout of the reference> [--time]

Imports the reference's src/data.py read-only (its GIS / Lightning / dask / torch imports are stubbed: only the import has
to succeed) and runs its OWN `sample_plots` (data.py:108-162) and `train_test_split` (:165-236, client=None) on seeded
synthetic annotation tables.  The only random numbers those functions draw are `np.random.shuffle(plotIDs)`, one per
sample_plots call, on a fresh `plotID.unique()` array of the candidate (siteID == "OSBS") rows; so every shuffle is
recovered here by re-seeding and shuffling the same array, and recorded as an order of the candidates.

The file holds only data: per table the input columns, integer-coded (`t<k>_individual`, `_plot`, `_taxon`, `_fixed`,
`_candidate`, one entry per row, in frame order with a RangeIndex); the sample_plots cases stacked as `sp_table`, `sp_min`
(min_train, min_test), `sp_candidates` (C), `sp_orders` [cases][1][C, padded with -1] and the resulting rows as bit-packed
masks over the row numbers (`sp_train_bits`, `sp_test_bits`: np.unpackbits(..., axis=1)); the train_test_split cases
likewise as `tts_table`, `tts_min`, `tts_seed`, `tts_candidates`, `tts_orders` [cases][iterations][C], the rows the
reference returned (`tts_train_bits`, `tts_test_bits`), `tts_chosen` (the iteration whose split that is) and `tts_figures`
[cases][iterations][2] (test species and train rows of every iteration, as the reference's frames give them).  No reference source is copied anywhere.  tests/golden/split/SHA256SUMS is written here.

The tables (asserted below): non-candidate sites; an individual whose first row is fixed and whose second is not; an
individual that is all fixed; a species that lives only outside the candidate plots; species of 220, 80 and 40 individuals,
whose 0.05 * n is the whole number 11.0 / 4.0 / 2.0 and lies above min_test = 10 / 3 / 1 (tests/test_split_cpu.py checks
that a running count EQUALS such a floor in a recorded scan, where only the strict `>` gives the reference's answer); the
settings (5, 3), (10, 10) and (1, 1); a train_test_split case in which several iterations tie on species and the train rows
decide for a later one, and one with a full tie in which the earliest wins.

--time prints the reference's seconds per sample_plots call on the large table (pandas, this CPU)."""
import hashlib
import importlib
import os
import sys
import time
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "split")
OUT = os.path.join(GOLDEN, "split_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

SETTINGS = ((5, 3), (10, 10), (1, 1))
# individuals per species; the last species lives outside the candidate site only
LARGE = dict(species=(220, 80, 40, 60, 33, 25, 12, 9), candidate_plots=14, other_plots=6)
SMALL = dict(species=(40, 30, 20, 14, 9), candidate_plots=5, other_plots=2)
TTS_ITERATIONS = 8


def table(spec, seed):
    """A synthetic annotation frame: individual x year rows in shuffled order."""
    import pandas as pd
    rs = np.random.RandomState(seed)
    n_cand, n_other = spec["candidate_plots"], spec["other_plots"]
    plots = ["OSBS_%03d" % p for p in range(n_cand)] + ["%s_%03d" % (("JERC", "TALL", "DSNY")[p % 3], p) for p in range(n_other)]
    sites = [p.split("_")[0] for p in plots]
    rows = []
    n_species = len(spec["species"])
    for s, count in enumerate(spec["species"]):
        outside_only = s == n_species - 1
        # a species prefers a few plots: the counts per (plot, species) are uneven, some plots lack the species
        weight = rs.gamma(0.6, 1.0, n_cand + n_other) + 1e-3
        if outside_only:
            weight[:n_cand] = 0
        home = rs.choice(n_cand + n_other, size=count, p=weight / weight.sum())
        for i in range(count):
            name = "NEON.T%d.%04d" % (s, i)
            years = rs.randint(1, 4)
            fixed = rs.uniform(size=years) < 0.2
            if s == 1 and i == 0:
                years, fixed = 2, np.array([True, False])      # fixed row FIRST, a free row after it
            if s == 1 and i == 1:
                years, fixed = 3, np.array([True, True, True])  # all fixed
            for y in range(years):
                rows.append((name, plots[home[i]], sites[home[i]], "T%d" % s,
                             "fixed_%d" % len(rows) if fixed[y] else str(len(rows)), 2019 + y))
    # the two special individuals sit in a candidate plot
    rows = [(r[0], plots[0], sites[0]) + r[3:] if r[0] in ("NEON.T1.0000", "NEON.T1.0001") else r for r in rows]
    order = rs.permutation(len(rows))
    # ... and the fixed-first individual keeps its fixed row first after the shuffle of the rows
    df = pd.DataFrame([rows[k] for k in order], columns=["individual", "plotID", "siteID", "taxonID", "box_id", "year"])
    at = df.index[df.individual == "NEON.T1.0000"]
    df.loc[at, "box_id"] = ["fixed_a", "b"]
    return df


def coded(df):
    def codes(col):
        return np.unique(df[col].to_numpy().astype(str), return_inverse=True)[1].astype(np.int16)
    return dict(individual=codes("individual"), plot=codes("plotID"), taxon=codes("taxonID"),
                fixed=df.box_id.astype(str).str.contains("fixed").to_numpy(), candidate=(df.siteID == "OSBS").to_numpy())


def candidates(shp):
    return shp[shp.siteID == "OSBS"].plotID.unique()


def recover_orders(shp, seed, calls):
    """The shuffles `calls` consecutive sample_plots calls make under np.random.seed(seed), as orders of candidates(shp)."""
    ids = candidates(shp)
    at = {p: j for j, p in enumerate(ids)}
    np.random.seed(seed)
    out = []
    for _ in range(calls):
        arr = candidates(shp)
        np.random.shuffle(arr)
        out.append([at[p] for p in arr])
    return np.array(out, np.int32)


def pack(data, prefix, cases, max_rows):
    """The cases of one kind as a few stacked arrays: orders padded with -1, the row sets as bit-packed masks."""
    width = max(c["orders"].shape[1] for c in cases)
    for name in ("table", "min", "seed", "chosen", "figures"):
        if name in cases[0]:
            data["%s_%s" % (prefix, name)] = np.array([c[name] for c in cases], np.int64)
    data[prefix + "_candidates"] = np.array([c["orders"].shape[1] for c in cases], np.int64)
    data[prefix + "_orders"] = np.stack([np.pad(c["orders"], ((0, 0), (0, width - c["orders"].shape[1])), constant_values=-1)
                                         for c in cases]).astype(np.int16)
    for name in ("train", "test"):
        mask = np.zeros((len(cases), max_rows), bool)
        for i, c in enumerate(cases):
            mask[i, c[name]] = True
        data["%s_%s_bits" % (prefix, name)] = np.packbits(mask, axis=1)


def check_tables(frames):
    for df in frames:
        assert (df.siteID != "OSBS").any()
        a = df[df.individual == "NEON.T1.0000"]
        assert list(a.box_id.str.contains("fixed")) == [True, False] and (a.siteID == "OSBS").all()
        assert df[df.individual == "NEON.T1.0001"].box_id.str.contains("fixed").all()
        last = sorted(df.taxonID.unique())[-1]
        assert (df[df.taxonID == last].siteID != "OSBS").all()
    n = frames[0].groupby("taxonID").individual.nunique()
    assert {220, 80, 40} <= set(n.values) and 220 * 0.05 == 11.0 and 80 * 0.05 == 4.0 and 40 * 0.05 == 2.0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isfile(os.path.join(args[0], "src", "data.py")):
        sys.exit("usage: make_split_golden.py <path of a checkout of the reference> [--time]")
    import pandas as pd
    warnings.simplefilter("ignore")
    ref = args[0]

    class Anything(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return type(name, (), {})
    for name in ("distributed", "geopandas", "pytorch_lightning", "shapely", "shapely.geometry", "torch", "torch.utils",
                 "torch.utils.data", "rasterio", "src.generate", "src.CHM", "src.augmentation", "src.megaplot",
                 "src.neon_paths", "src.models", "src.models.dead", "src.utils"):
        if name not in sys.modules:
            sys.modules[name] = Anything(name)
            sys.modules[name].__all__ = []
    pkg = types.ModuleType("src")
    pkg.__path__, pkg.__file__ = [os.path.join(ref, "src")], os.path.join(ref, "src", "__init__.py")
    sys.modules["src"] = pkg
    D = importlib.import_module("src.data")

    frames = [table(LARGE, 0), table(LARGE, 1), table(LARGE, 2), table(SMALL, 3), table(SMALL, 4)]
    check_tables(frames)
    data = {}
    for k, df in enumerate(frames):
        for name, col in coded(df).items():
            data["t%d_%s" % (k, name)] = col
    data["tables"] = np.int64(len(frames))

    if "--time" in sys.argv:
        t0 = time.perf_counter()
        for _ in range(5):
            D.sample_plots(frames[0], 5, 3)
        print("reference sample_plots (pandas {}): {:.3f} s per call, {} rows, {} candidate plots".format(
            pd.__version__, (time.perf_counter() - t0) / 5, len(frames[0]), len(candidates(frames[0]))))

    # sample_plots on its own: 3 large tables x 3 settings x 3 shuffles
    singles = []
    for k in (0, 1, 2):
        for mins in SETTINGS:
            for shuffle_seed in (11, 12, 13):
                order = recover_orders(frames[k], shuffle_seed, 1)[0]
                np.random.seed(shuffle_seed)
                train, test = D.sample_plots(frames[k].copy(), min_train_samples=mins[0], min_test_samples=mins[1])
                singles.append(dict(table=k, min=mins, orders=order[None], train=train.index.values, test=test.index.values))
    pack(data, "sp", singles, max(len(f) for f in frames))

    # train_test_split: the large tables under every setting, and two small-table cases picked for their ties
    def run_tts(k, mins, seed):
        config = {"min_train_samples": mins[0], "min_test_samples": mins[1], "iterations": TTS_ITERATIONS}
        shp = frames[k]
        keep = shp.taxonID.value_counts() > sum(mins)           # the frame sample_plots sees (data.py:173-176)
        filtered = shp[shp.taxonID.isin(keep[keep].index)]
        orders = recover_orders(filtered, seed, TTS_ITERATIONS)
        np.random.seed(seed)
        each = [D.sample_plots(filtered, min_train_samples=mins[0], min_test_samples=mins[1]) for _ in range(TTS_ITERATIONS)]
        figures = np.array([(te.taxonID.nunique(), tr.shape[0]) for tr, te in each], np.int64)
        np.random.seed(seed)
        train, test = D.train_test_split(shp.copy(), config, client=None)
        same = [t for t, (tr, te) in enumerate(each)
                if np.array_equal(tr.index.values, train.index.values) and np.array_equal(te.index.values, test.index.values)]
        return dict(table=k, min=mins, seed=seed, orders=orders, figures=figures, train=train.index.values,
                    test=test.index.values, chosen=same[0])

    cases = [run_tts(k, mins, 20 + k) for k in (0, 1) for mins in SETTINGS]
    rows_decide = full_tie = None
    for seed in range(400):
        if rows_decide is not None and full_tie is not None:
            break
        for k in (3, 4):
            c = run_tts(k, (5, 3), seed)
            f, top = c["figures"], c["figures"][:, 0].max()
            tied = np.flatnonzero(f[:, 0] == top)
            most = f[tied, 1].max()
            winners = tied[f[tied, 1] == most]
            if rows_decide is None and len(tied) > 1 and winners[0] != tied[0] and len(winners) == 1:
                assert c["chosen"] == winners[0]
                rows_decide = c
            elif full_tie is None and len(winners) > 1 and winners[0] == tied[0] and len(np.unique(c["orders"][winners], axis=0)) > 1:
                assert c["chosen"] == winners[0]
                full_tie = c
    assert rows_decide is not None and full_tie is not None, "no tie cases found"
    cases += [rows_decide, full_tie]
    pack(data, "tts", cases, max(len(f) for f in frames))
    data["tts_rows_decide"], data["tts_full_tie"] = np.int64(len(cases) - 2), np.int64(len(cases) - 1)

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(OUT, **data)
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes;", len(singles), "sample_plots cases,", len(cases), "train_test_split cases")


if __name__ == "__main__":
    main()
