"""The train/test plot split search on the host: the NumPy definition against the reference's own results
(tests/golden/split/split_reference.npz, made by tools/make_split_golden.py from the reference's sample_plots and
train_test_split), the order, the refusals of split.py and of dta_split_search, and the ABI bookkeeping.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return SC.Fixture()


def table_of(columns, **kw):
    from deeptreeattention_amd import split as S
    return S.SplitTable.from_columns(**columns, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the definition equals the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_checksum_and_contents(fx):
    import hashlib
    line = open(os.path.join(os.path.dirname(SC.GOLDEN), "SHA256SUMS")).read().split()
    assert line[1] == "split_reference.npz" and hashlib.sha256(open(SC.GOLDEN, "rb").read()).hexdigest() == line[0]
    assert os.path.getsize(SC.GOLDEN) < 100 * 1024
    assert {c["min"] for c in fx.cases("sp")} == {(5, 3), (10, 10), (1, 1)} <= {c["min"] for c in fx.cases("tts")}
    for cols in fx.columns:
        t = table_of(cols)
        assert 0 < t.n_candidates < t.n_plots                                     # non-candidate sites
        rows = np.bincount(t.individual)
        nonfixed = np.bincount(t.individual, weights=~t.fixed).astype(int)
        assert ((nonfixed == 0) & (rows > 1)).any()                               # an individual that is all fixed
        first = np.array([np.flatnonzero(t.individual == i)[0] for i in np.flatnonzero((nonfixed > 0) & (nonfixed < rows))])
        assert t.fixed[first].any()                                               # part fixed, the fixed row first
        assert ((t.A[t.candidates].sum(0) == 0) & (t.totA > 0)).any()             # a species outside the candidates only


def test_sample_plots_rows_equal_the_reference(fx):
    from deeptreeattention_amd import split as S
    n = 0
    for c in fx.cases("sp"):
        t = table_of(fx.columns[c["table"]])
        r = S.search_np(t, 1, orders=c["orders"], min_train=c["min"][0], min_test=c["min"][1])
        train, test = S.rows_np(t, r.membership[0], r.taxa[0])
        assert np.array_equal(train, c["train"]) and np.array_equal(test, c["test"]), c["min"]
        assert r.species[0] == len(np.unique(t.taxon[c["test"]])) == r.best[1] and r.train_rows[0] == c["train"].sum() == r.best[2]
        assert r.test_plots[0] == r.membership[0].sum() == r.best[3] and r.best[0] == 0
        assert set(np.unique(t.taxon[c["test"]])) == set(np.flatnonzero(r.taxa[0]))
        n += 1
    assert n == 27


def test_a_count_that_equals_its_floor_does_not_complete_the_species(fx):
    """0.05 * n is the whole number 11.0 / 4.0 / 2.0 above min_test for the species of 220 / 80 / 40 individuals; in recorded
    scans the running count EQUALS it after some plot, and with `>=` in place of the strict `>` the split differs from the
    reference's -- which test_sample_plots_rows_equal_the_reference holds the definition to."""
    from deeptreeattention_amd import split as S
    met = differs = 0
    for c in fx.cases("sp"):
        t = table_of(fx.columns[c["table"]])
        floor = t.floor(c["min"][1])
        whole = (floor == np.floor(floor)) & (floor > c["min"][1])
        assert whole.any()
        Ac = t.A[t.candidates]

        def scan(complete):
            cnt, wanted, inc, eq = np.zeros(t.n_species, np.int64), np.ones(t.n_species, bool), [], False
            for p in c["orders"][0]:
                if ((Ac[p] > 0) & wanted).any():
                    inc.append(p)
                    cnt = cnt + Ac[p]
                    eq |= bool(((cnt == floor) & whole).any())
                    wanted = ~complete(cnt.astype(np.float64), floor)
            return inc, eq
        strict, eq = scan(np.greater)
        r = S.search_np(t, 1, orders=c["orders"], min_train=c["min"][0], min_test=c["min"][1])
        assert sorted(strict) == sorted(np.flatnonzero(r.membership[0]))
        met += eq
        differs += scan(np.greater_equal)[0] != strict
    assert met >= 3 and differs >= 1, (met, differs)


def test_train_test_split_equals_the_reference(fx):
    from deeptreeattention_amd import split as S
    z = fx.z
    cases = list(fx.cases("tts"))
    for c in cases:
        cols = fx.columns[c["table"]]
        sp = S.train_test_split_np(cols, c["min"][0], c["min"][1], iterations=len(c["orders"]), orders=c["orders"])
        assert np.array_equal(sp.train, c["train"]) and np.array_equal(sp.test, c["test"]) and sp.iteration == c["chosen"]
        # ... and every iteration's figures, on the prefiltered table the reference's sample_plots saw
        sub, _ = SC.prefiltered(cols, *c["min"])
        r = S.search_np(table_of(sub), len(c["orders"]), orders=c["orders"], min_train=c["min"][0], min_test=c["min"][1])
        assert np.array_equal(r.species, c["figures"][:, 0]) and np.array_equal(r.train_rows, c["figures"][:, 1])
        assert r.best[0] == c["chosen"]
    f = cases[int(z["tts_rows_decide"])]["figures"]        # several iterations tie on species; the train rows decide
    tied = np.flatnonzero(f[:, 0] == f[:, 0].max())
    assert len(tied) > 1 and cases[int(z["tts_rows_decide"])]["chosen"] == tied[np.argmax(f[tied, 1])] != tied[0]
    f = cases[int(z["tts_full_tie"])]["figures"]           # a full tie: the earliest wins
    top = np.flatnonzero((f[:, 0] == f[:, 0].max()))
    top = top[f[top, 1] == f[top, 1].max()]
    assert len(top) > 1 and cases[int(z["tts_full_tie"])]["chosen"] == top[0]


def test_from_frame_reads_the_reference_columns():
    pd = pytest.importorskip("pandas")
    from deeptreeattention_amd import split as S
    df = pd.DataFrame({"individual": ["a", "a", "b", "c"], "plotID": ["OSBS_1", "OSBS_1", "X_2", "OSBS_3"],
                       "taxonID": ["PIPA", "PIPA", "QULA", "QULA"], "box_id": ["fixed_1", "7", None, "9"],
                       "siteID": ["OSBS", "OSBS", "X", "OSBS"]})
    t = S.SplitTable.from_frame(df)
    assert t.fixed.tolist() == [True, False, False, False] and t.candidates.tolist() == [0, 2]
    assert t.A.tolist() == [[1, 0], [0, 1], [0, 1]] and t.B.tolist() == t.A.tolist() and t.R.tolist() == [[2, 0], [0, 1], [0, 1]]
    assert list(t.plots) == ["OSBS_1", "X_2", "OSBS_3"] and list(t.taxa) == ["PIPA", "QULA"]


# ---------------------------------------------------------------------------------------------------------------------
# the order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 4096])
def test_order_is_a_permutation(C):
    from deeptreeattention_amd import split as S
    o = S.order_np(C, [0, 1, 2 ** 32 + 5, 2 ** 64 - 1], seed=3)
    assert o.dtype == np.int32 and o.shape == (4, C)
    assert (np.sort(o, axis=1) == np.arange(C)).all()
    assert np.array_equal(S.order_np(C, 1, seed=3), o[1]) and np.array_equal(S.order_np(C, 2 ** 64 - 1, seed=3), o[3])
    assert np.array_equal(S.order_np(C, np.array([1, 2 ** 32 + 5]), seed=3), o[1:3])
    assert np.array_equal(S.order_np(C, -1, seed=3), o[3]) and np.array_equal(S.order_np(C, 2 ** 64, seed=3), o[0])    # modulo 2^64
    if C >= 63:
        assert not np.array_equal(o[0], o[1]) and not np.array_equal(o[0], S.order_np(C, 0, seed=4))
        assert len({tuple(r) for r in o.tolist()}) == 4
        assert not np.array_equal(o[0], np.arange(C))


def test_order_is_the_documented_hash():
    from deeptreeattention_amd import abundance, split as S
    C, t, seed = 7, 2 ** 63 + 11, 5
    M = (1 << 64) - 1
    keys = []
    for j in range(C):
        z = (((t * C + j) & M) * 0x9E3779B97F4A7C15 + abundance.stream_key(seed, 0)) & M
        keys.append(((abundance._mix_int(z) >> 32), j))
    assert S.order_np(C, t, seed).tolist() == [j for _, j in sorted(keys)]
    with pytest.raises(ValueError):
        S.order_np(0, 0)
    with pytest.raises(ValueError):
        S.order_np(4097, 0)


# ---------------------------------------------------------------------------------------------------------------------
# refusals and small paths of split.py
# ---------------------------------------------------------------------------------------------------------------------
def test_from_columns_refuses_an_individual_with_two_plots_or_two_taxa():
    from deeptreeattention_amd import split as S
    ok = dict(individual=[0, 0, 1, 2], plot=[0, 0, 1, 2], taxon=[0, 0, 1, 1], fixed=[0, 1, 0, 0])
    S.SplitTable.from_columns(**ok)
    with pytest.raises(ValueError, match="more than one plot"):
        S.SplitTable.from_columns(**dict(ok, plot=[0, 1, 1, 2]))
    with pytest.raises(ValueError, match="more than one taxon"):
        S.SplitTable.from_columns(**dict(ok, taxon=[0, 1, 1, 1]))
    with pytest.raises(ValueError, match="same for every row of a plot"):
        S.SplitTable.from_columns(**ok, candidate=[1, 0, 1, 1])
    with pytest.raises(ValueError, match="not both"):
        S.SplitTable.from_columns(**ok, candidate=[1, 1, 1, 1], site=list("aabc"), candidate_site="a")
    with pytest.raises(ValueError, match="one entry per row"):
        S.SplitTable.from_columns(**dict(ok, fixed=[0, 1]))
    with pytest.raises(ValueError, match="species"):
        S.SplitTable.from_columns(np.arange(300), np.arange(300) % 5, np.arange(300), np.zeros(300))
    with pytest.raises(ValueError, match="candidate plots"):
        S.SplitTable.from_columns(np.arange(5000), np.arange(5000), np.zeros(5000, int), np.zeros(5000))
    t = S.SplitTable.from_columns(**ok, site=list("aabc"), candidate_site="a")
    assert t.candidates.tolist() == [0]


def test_search_np_refuses_bad_arguments(fx):
    from deeptreeattention_amd import split as S
    t = table_of(fx.columns[3])
    C = t.n_candidates
    good = S.order_np(C, [0, 1])
    for bad in (good[:1], good[:, :-1], good.astype(np.float64), np.zeros_like(good), good + 1, -good):
        with pytest.raises(ValueError, match="orders"):
            S.search_np(t, 2, orders=bad)
    for kw in ({"min_train": 0}, {"min_test": 0}, {"min_test": -1}, {"iterations": -1}):
        with pytest.raises(ValueError):
            S.search_np(t, **dict({"iterations": 1}, **kw))
    empty = S.search_np(t, 0)
    assert empty.best == (-1, 0, 0, 0) and empty.species.shape == (0,) and empty.membership.shape == (0, C)
    with pytest.raises(ValueError, match="no candidate plots"):
        S.search_np(table_of(dict(fx.columns[3], candidate=np.zeros(len(t.individual), bool))), 1)
    # row k of a longer run is iterations=1, first_iteration=k
    whole = S.search_np(t, 6, seed=2)
    one = S.search_np(t, 1, seed=2, first_iteration=4)
    assert one.species[0] == whole.species[4] and np.array_equal(one.membership[0], whole.membership[4])
    with pytest.raises(ValueError):
        S.rows_np(t, np.zeros(C + 1), np.zeros(t.n_species))


def test_two_plots_or_fewer_give_the_reference_fixed_answer(monkeypatch):
    """data.py:120-124: the first plot is the test set, the second the train set, nothing is filtered and nothing searched;
    the device route takes this path without a launch (the library is never reached)."""
    from deeptreeattention_amd import _lib, split as S

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    cols = {"individual": np.arange(40), "plot": np.array(["b"] * 15 + ["a"] * 25), "taxon": np.arange(40) % 2,
            "fixed": np.arange(40) % 3 == 0}
    for fn in (S.train_test_split_np, S.train_test_split):
        sp = fn(cols, min_train=5, min_test=3, iterations=10)
        assert np.array_equal(sp.test, cols["plot"] == "b") and np.array_equal(sp.train, cols["plot"] == "a")
    # the prefilter comes first: a third plot that holds only a rare species is gone before the plots are counted
    more = {k: np.concatenate([v, v[:1]]) for k, v in cols.items()}
    more["individual"][-1], more["plot"][-1], more["taxon"][-1] = 99, "c", 7
    sp = S.train_test_split_np(more, min_train=5, min_test=3)
    assert not sp.train[-1] and not sp.test[-1] and sp.test.sum() == 15 and sp.train.sum() == 25
    with pytest.raises(ValueError, match="at least two plots"):
        S.train_test_split_np({k: v[:15] for k, v in cols.items()}, min_train=2, min_test=2)
    with pytest.raises(ValueError, match="no species has more than"):
        S.train_test_split_np(cols, min_train=30, min_test=30)
    with pytest.raises(ValueError, match="needs individual"):
        S.train_test_split_np({"individual": [1]})


def test_a_best_split_without_species_is_an_error():
    from deeptreeattention_amd import split as S
    # three plots, every species in one plot only: no species can be in train and in test
    cols = {"individual": np.arange(60), "plot": np.arange(60) // 20, "taxon": np.arange(60) // 20, "fixed": np.zeros(60, bool)}
    r = S.search_np(S.SplitTable.from_columns(**cols), 5)
    assert (r.species == 0).all() and r.best[:2] == (0, 0)
    with pytest.raises(ValueError, match="keeps a species in both"):
        S.train_test_split_np(cols, min_train=5, min_test=3, iterations=5)
    with pytest.raises(ValueError, match="no candidate plots"):
        S.train_test_split_np(dict(cols, candidate=np.zeros(60, bool)), iterations=5)


def test_device_route_checks_its_arguments_on_the_host(monkeypatch, fx):
    """Everything below is refused before _lib.lib() is reached.  The permutation check of `orders` is the WRAPPER's
    (split.check_orders); dta_split_search only keeps a bad entry inside the table."""
    torch = pytest.importorskip("torch")
    from deeptreeattention_amd import _lib, split as S

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    t = table_of(fx.columns[3])
    with pytest.raises(RuntimeError, match="ROCm device only"):
        t.search(1)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        t.to("cpu")
    with pytest.raises(RuntimeError, match="ROCm device only"):
        S.SplitTable.from_columns(**fx.columns[3], device="cpu")
    rows, totals = t.device_rows()
    SP = (t.n_species + 3) & ~3
    assert rows.shape == (t.n_candidates, 3, SP) and rows.dtype == np.int32 and totals.shape == (2, SP)
    assert np.array_equal(rows[:, 0, :t.n_species], t.A[t.candidates]) and not rows[:, :, t.n_species:].any()
    # a table that claims a device: the argument checks run, the library is not reached
    t.device, t.rows_dev, t.totals_dev = torch.device("meta"), torch.from_numpy(rows).to("meta"), torch.from_numpy(totals).to("meta")
    C = t.n_candidates
    good = S.order_np(C, [0, 1])
    for bad in (good[:1], np.zeros_like(good), good + 1):
        with pytest.raises(ValueError, match="orders"):
            t.search(2, orders=bad)
    for kw in ({"min_train": 0}, {"min_test": 0}, {"iterations": -1}):
        with pytest.raises(ValueError):
            t.search(**dict({"iterations": 1}, **kw))
    out = S.SplitSearch(torch.empty(3, dtype=torch.int32, device="meta"), None, None, None, None, None)
    with pytest.raises(ValueError, match="out.species"):
        t.search(2, out=out)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, bound, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from deeptreeattention_amd import _lib, build, split
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    new = {n for n in names if n.startswith("dta_split_")}
    assert new == {"dta_split_search"}
    for n in new:
        assert hasattr(lib, n) and '"%s"' % n in entry
        assert len(getattr(lib, n).argtypes) == 18 and getattr(lib, n).restype is C.c_int
    assert "split.hip" in build.SOURCES and build.SOURCES[-1] != "split.hip"
    assert build.SOURCES.index("split.hip") < build.SOURCES.index("boundary.hip")
    assert int(re.search(r"#define\s+DTA_SPLIT_MAX_SPECIES\s+(\d+)", hdr).group(1)) == _lib.SPLIT_MAX_SPECIES == split.MAX_SPECIES == 256
    cand = int(re.search(r"#define\s+DTA_SPLIT_MAX_CANDIDATES\s+(\d+)", hdr).group(1))
    assert cand == _lib.SPLIT_MAX_CANDIDATES == split.MAX_CANDIDATES == 4096 and cand & (cand - 1) == 0
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the device pointers are host buffers nobody
    dereferences; floor is a host array, which the entry reads.  That `orders` holds permutations is not checked here but
    by split.check_orders (test_device_route_checks_its_arguments_on_the_host)."""
    buf = (C.c_ubyte * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    nan, inf = float("nan"), float("inf")

    def d(*v):
        return (C.c_double * len(v))(*v)

    def call(rows=p, totals=p, candidates=8, species=3, floor=d(3.0, 3.0, 4.0), min_train=5, min_test=3, iterations=2,
             orders=None, species_out=p, train_rows=p, test_plots=p, best=p, membership=None, taxa=None):
        return lib.dta_split_search(rows, totals, candidates, species, floor, min_train, min_test, iterations, 0, 0, orders,
                                    species_out, train_rows, test_plots, best, membership, taxa, None)

    cases = (({"rows": None}, "null"), ({"totals": None}, "null"), ({"floor": None}, "null"), ({"species_out": None}, "null"),
             ({"train_rows": None}, "null"), ({"test_plots": None}, "null"), ({"best": None}, "null"),
             ({"species": 0}, "species=0"), ({"species": 257, "floor": d(*([3.0] * 257))}, "species=257"),
             ({"species": -1}, "species=-1"),
             ({"candidates": 0}, "candidates=0"), ({"candidates": 4097}, "candidates=4097"), ({"candidates": -2}, "candidates=-2"),
             ({"iterations": -1}, "iterations=-1"), ({"min_train": 0}, "min_train=0"), ({"min_test": 0}, "min_test=0"),
             ({"rows": odd}, "16-byte aligned"), ({"totals": odd}, "16-byte aligned"),
             ({"floor": d(3.0, nan, 4.0)}, "floor is not finite"), ({"floor": d(inf, 3.0, 4.0)}, "floor is not finite"),
             ({"floor": d(3.0, 3.0, -inf)}, "floor is not finite"))
    for kw, what in cases:
        assert call(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_split_search: ") and what in err, (kw, err)
    assert call(iterations=0) == 0                     # nothing to do, nothing launched
    # the refusals come first even then
    assert call(iterations=0, floor=d(nan, 3.0, 4.0)) != 0 and call(iterations=0, species=0) != 0


def test_the_split_kernels_have_no_private_segment(tmp_path):
    import glob
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump, readelf = os.path.join(llvm, "llvm-objdump"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    from deeptreeattention_amd import _lib
    so = os.path.join(str(tmp_path), "libdta_hip.so")
    shutil.copy(os.path.join(os.path.dirname(_lib.LIB_PATH), "libdta_hip.so"), so)
    subprocess.run([objdump, "--offloading", so], cwd=str(tmp_path), capture_output=True, check=True)
    found = {}
    for f in sorted(glob.glob(so + ".*gfx950*")):
        notes = subprocess.run([readelf, "--notes", f], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.?name:\s+(\S+)", blk)
            seg = re.search(r"private_segment_fixed_size:\s+(\d+)", blk)
            if name and seg and "k_split_" in name.group(1):
                found[name.group(1)] = int(seg.group(1))
    assert len(found) == 2 and all(v == 0 for v in found.values()), found
