"""Abundance per tile and map cell on the host (deeptreeattention_amd/abundance.py): cells_np / cell_names against what the
REFERENCE's own bounds_to_geoindex recorded (tests/golden/abundance_grid/geoindex_reference.npz, made by
tools/make_geoindex_golden.py); the group= forms of counts_np / resample_np against the masked ungrouped calls they are
defined by; summary_np against np.mean / np.quantile; and the argument checks of the new C entry points.  No GPU needed."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from test_abundance_cpu import random_confusion, random_crowns

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0, 0.025, 0.5, 0.975, 1)


@pytest.fixture(scope="module")
def geoindex(golden):
    g = golden(os.path.join("abundance_grid", "geoindex_reference.npz"))
    return {k: g[k] for k in g.files}


def grouped_case(seed, N, S, G):
    """Random labels (with -1, DEAD and far-out ones), scores (NaN, 0, 1, outside [0, 1]), a mask, and groups of which some
    are -1, some exactly G and some far outside."""
    from deeptreeattention_amd.abundance import sampling_table
    rng = np.random.default_rng(seed)
    table = sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    mask = rng.random(N) < 0.7
    group = rng.integers(0, G, N).astype(np.int64)
    out = rng.random(N) < 0.15
    group[out] = rng.choice(np.array([-1, G, G + 3, -2 ** 40, 2 ** 40], np.int64), int(out.sum()))
    return table, label, score, mask, group


# ---------------------------------------------------------------------------------------------------------------------
# which cell a crown is in
# ---------------------------------------------------------------------------------------------------------------------
def test_geoindex_fixture_is_the_committed_one():
    here = os.path.join(REPO, "tests", "golden", "abundance_grid")
    lines = [ln.split() for ln in open(os.path.join(here, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert [name for _, name in lines] == sorted(f for f in os.listdir(here) if f.endswith(".npz")) == ["geoindex_reference.npz"]
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(here, name), "rb").read()).hexdigest() == digest, name


def test_geoindex_fixture_is_the_documented_one(geoindex):
    b, names, block = geoindex["bounds"], geoindex["geoindex"], geoindex["block"]
    assert b.dtype == np.float64 and b.shape == (len(names), 4) and 300 <= len(b) <= 1000 and names.dtype.kind == "U"
    assert (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    utm = block == 0
    assert (cx[utm] > 4e5).all() and (cy[utm] > 4.1e6).all()                                   # UTM-sized values
    assert int(((cx % 1000 == 0) | (cy % 1000 == 0)).sum()) >= 60                              # centres on a tile line
    assert int(((cx % 1000 == 0.5) | (cx % 1000 == 999.5)).sum()) >= 40                        # ... and half a metre off
    straddle = (np.floor(b[:, 0] / 1000) != np.floor(b[:, 2] / 1000)) | (np.floor(b[:, 1] / 1000) != np.floor(b[:, 3] / 1000))
    assert int(straddle.sum()) >= 100
    assert int(((cx < 0) | (cy < 0)).sum()) >= 60                                              # truncation is not floor there
    assert int(((np.trunc(cx) != np.floor(cx)) | (np.trunc(cy) != np.floor(cy))).sum()) >= 40
    for c in (-0.5, -999.5, -1000.0, -1000.5, 0.0):
        assert (cx == c).any(), c


def test_cells_np_names_every_fixture_row_as_the_reference_does(geoindex):
    from deeptreeattention_amd.abundance import cell_names, cells_np
    b, names, block, grid = geoindex["bounds"], geoindex["geoindex"], geoindex["block"], geoindex["grid"]
    for k in range(len(grid)):
        ox, oy, cols, rows = (int(v) for v in grid[k])
        sel = block == k
        cell = cells_np(b[sel], cols, rows, origin=(ox, oy), size=1000)
        assert cell.dtype == np.int64 and cell.shape == (int(sel.sum()),) and (cell >= 0).all()
        table = np.array(cell_names(cols, rows, origin=(ox, oy), size=1000))
        assert len(table) == cols * rows
        assert (table[cell] == names[sel]).all(), k
        assert len(set(cell.tolist())) > 20
    # the defaults are the reference's: origin 0, size 1000
    pos = (b[:, 0] > 0) & (b[:, 1] > 0)
    cell = cells_np(b[pos], 431, 4131)
    assert all("{}_{}".format(c % 431 * 1000, c // 431 * 1000) == n for c, n in zip(cell.tolist(), names[pos].tolist()))


def test_cells_np_rules_edges_and_refusals():
    from deeptreeattention_amd.abundance import cell_names, cells_np
    f = lambda rows: np.array(rows, np.float64)
    # geoindex truncates toward zero first: a centre of -0.5 is easting 0, tile 0; -1000.5 is -1000, tile -1000
    b = f([(-1.5, 0, 0.5, 2), (-1002, 0, -999, 2), (999, 999, 1000, 1001), (2999, 0, 3001, 1), (0, -2001, 0, -2000)])
    assert cells_np(b, 4, 4, origin=(-1000, -1000)).tolist() == [5, 4, 9, -1, -1]
    # the centre rule floors the float centre: -0.5 lies in the cell left of zero, -1000.5 left of the grid
    assert cells_np(b, 4, 4, origin=(-1000, -1000), rule="centre").tolist() == [4, -1, 9, -1, -1]
    # hectare cells with a float origin; the upper edge is outside, the lower edge inside
    h = f([(0.5, 0.5, 0.5, 0.5), (100.5, 0.5, 100.5, 0.5), (300.5, 0.5, 300.5, 0.5), (0.25, 0.5, 0.5, 0.5), (50, 250.5, 60, 250.5)])
    assert cells_np(h, 3, 3, origin=(0.5, 0.5), size=100.0, rule="centre").tolist() == [0, 1, -1, -1, 6]
    # not finite, or beyond 2^53: outside, under both rules
    bad = f([(np.nan, 0, 1, 1), (0, 0, np.inf, 1), (-np.inf, 0, np.inf, 1), (2.0 ** 60, 0, 2.0 ** 60, 1), (0, 0, 1, 1)])
    for rule in ("geoindex", "centre"):
        assert cells_np(bad, 2, 2, rule=rule).tolist() == [-1, -1, -1, -1, 0], rule
    assert cells_np(np.zeros((0, 4)), 2, 2).shape == (0,)
    assert cell_names(2, 2, origin=(-1000, 4000)) == ["-1000_4000", "0_4000", "-1000_5000", "0_5000"]
    for kw, what in (({"rule": "floor"}, "rule"), ({"size": 0}, "size"), ({"size": 0.5}, "integer"), ({"origin": (0.5, 0)}, "integer"),
                     ({"origin": (np.nan, 0), "rule": "centre"}, "finite"), ({"cols": 0}, "cols")):
        args = dict(cols=2, rows=2)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            cells_np(bad, **args)
    with pytest.raises(ValueError, match="float64"):
        cells_np(bad.astype(np.float32), 2, 2)


# ---------------------------------------------------------------------------------------------------------------------
# grouped counts and resampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,iterations,S,G", [(1, 2, 1, 1), (40, 5, 2, 3), (300, 6, 23, 7), (150, 3, 6, 150)])
def test_grouped_resample_np_is_the_masked_call_per_cell_and_sums_to_the_ungrouped_one(N, iterations, S, G):
    from deeptreeattention_amd.abundance import resample_np
    table, label, score, mask, group = grouped_case(100 * N + G, N, S, G)
    for sc in (score, None):
        for m in (None, mask):
            kw = dict(seed=11, first_iteration=2)
            got = resample_np(label, sc, table, iterations, mask=m, group=group, groups=G, **kw)
            assert got.shape == (iterations, G, S + 1) and got.dtype == np.int64
            live = np.ones(N, bool) if m is None else m
            for g in range(G):
                want = resample_np(label, sc, table, iterations, mask=live & (group == g), **kw)
                assert np.array_equal(got[:, g], want), (sc is None, m is None, g)
            inside = (group >= 0) & (group < G)
            assert np.array_equal(got.sum(1), resample_np(label, sc, table, iterations, mask=live & inside, **kw))
    assert resample_np(label, score, table, 0, group=group, groups=G).shape == (0, G, S + 1)


def test_one_cell_is_the_ungrouped_table_and_bad_groups_are_refused():
    from deeptreeattention_amd.abundance import counts_np, resample_np
    table, label, score, mask, _ = grouped_case(7, 200, 6, 1)
    zero = np.zeros(200, np.int64)
    for m in (None, mask):
        want = resample_np(label, score, table, 9, seed=3, mask=m)
        assert np.array_equal(resample_np(label, score, table, 9, seed=3, mask=m, group=zero, groups=1), want.reshape(9, 1, 7))
        assert np.array_equal(counts_np(label, 6, m, group=zero, groups=1), counts_np(label, 6, m).reshape(1, 7))
    for call in (lambda **kw: resample_np(label, score, table, 2, **kw), lambda **kw: counts_np(label, 6, **kw)):
        with pytest.raises(ValueError, match="groups"):
            call(group=zero)
        with pytest.raises(ValueError, match="groups"):
            call(group=zero, groups=0)
        with pytest.raises(ValueError, match="groups without group"):
            call(groups=3)
        with pytest.raises(ValueError, match="one integer cell index per crown"):
            call(group=zero[:-1], groups=2)
        with pytest.raises(ValueError, match="one integer cell index per crown"):
            call(group=zero.astype(np.float64), groups=2)


def test_grouped_counts_np_is_a_two_dimensional_bincount():
    from deeptreeattention_amd.abundance import counts_np
    for N, S, G in ((1, 1, 1), (300, 6, 5), (500, 37, 64)):
        _, label, _, mask, group = grouped_case(31 + N, N, S, G)
        binned = np.where((label >= 0) & (label < S), label, S)
        for m in (None, mask):
            keep = ((group >= 0) & (group < G)) & (np.ones(N, bool) if m is None else m)
            want = np.zeros((G, S + 1), np.int64)
            np.add.at(want, (group[keep], binned[keep]), 1)
            got = counts_np(label, S, m, group=group, groups=G)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert np.array_equal(want.reshape(-1), np.bincount(group[keep] * (S + 1) + binned[keep], minlength=G * (S + 1)))


# ---------------------------------------------------------------------------------------------------------------------
# the summary
# ---------------------------------------------------------------------------------------------------------------------
def tied_table(rng, T, shape):
    """Counts full of ties and zeros, with a few large entries."""
    c = rng.integers(0, 4, (T,) + shape) * (rng.random((T,) + shape) < 0.6)
    c[rng.random((T,) + shape) < 0.05] = 10 ** 6 + 7
    c[:, ..., 0] = 0                                            # an entry that is zero in every iteration
    return c.astype(np.int64)


@pytest.mark.parametrize("T", [1, 2, 7, 100])
def test_summary_np_is_numpy_mean_and_quantile_entry_for_entry(T):
    from deeptreeattention_amd.abundance import summary, summary_np
    rng = np.random.default_rng(T)
    for shape in ((201,), (5, 37)):
        c = tied_table(rng, T, shape)
        got = summary_np(c, QS)
        assert got.q == QS and got.mean.shape == shape and got.quantiles.shape == (len(QS),) + shape
        assert got.mean.dtype == np.float64 and got.quantiles.dtype == np.float64
        want = summary(c.reshape(T, -1), QS)
        assert np.array_equal(got.mean.reshape(-1), want.mean)
        assert np.array_equal(got.quantiles.reshape(len(QS), -1), want.quantiles)
        assert np.array_equal(got.quantiles[0], c.min(0)) and np.array_equal(got.quantiles[-1], c.max(0))
    one = summary_np(c, (0.3,))
    assert np.array_equal(one.quantiles[0], np.quantile(c.astype(np.float64), 0.3, axis=0))
    assert summary_np(c, ()).quantiles.shape == (0,) + shape
    with pytest.raises(ValueError, match="integer table"):
        summary_np(c.astype(np.float64))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        summary_np(c, (1.5,))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_and_exported(lib):
    from deeptreeattention_amd import _lib, abundance, build
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    for n in ("dta_abundance_cells", "dta_abundance_resample_grouped", "dta_abundance_counts_grouped",
              "dta_abundance_grouped_workspace_bytes", "dta_abundance_summary"):
        assert n in names and hasattr(lib, n), n
    define = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert define("DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS") == _lib.ABUNDANCE_SUMMARY_MAX_ITERATIONS == abundance.SUMMARY_MAX_ITERATIONS >= 256
    assert define("DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS") * 64 * 8 <= 160 * 1024                # a workgroup's tile fits the LDS
    assert define("DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES") == _lib.ABUNDANCE_SUMMARY_MAX_QUANTILES == abundance.SUMMARY_MAX_QUANTILES
    assert (define("DTA_CELLS_GEOINDEX"), define("DTA_CELLS_CENTRE")) == (_lib.CELLS_GEOINDEX, _lib.CELLS_CENTRE)
    assert abundance.RULES == {"geoindex": _lib.CELLS_GEOINDEX, "centre": _lib.CELLS_CENTRE}
    assert lib.dta_abi_version() == 2 and define("DTA_ABI_VERSION") == 2                       # entry points were only added
    assert "abundance_grid.hip" in build.SOURCES and "abundance_dev.h" in build.HEADERS


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (this machine has no GPU): the device pointers are null or host buffers
    nobody dereferences."""
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    big = 1 << 30
    org = (C.c_double * 2)(0.0, 0.0)

    def err():
        return lib.dta_last_error().decode()

    def resample(label=p, score=p, mask=p, gs=p, order=p, n=10, groups=4, table=p, species=6, iterations=3, counts=p, ws=p,
                 ws_bytes=big):
        return lib.dta_abundance_resample_grouped(label, score, mask, gs, order, n, groups, table, species, iterations, 0, 0,
                                                  counts, ws, ws_bytes, None)

    def counts(label=p, mask=p, gs=p, order=p, n=10, groups=4, species=6, out=p, ws=p, ws_bytes=big):
        return lib.dta_abundance_counts_grouped(label, mask, gs, order, n, groups, species, out, ws, ws_bytes, None)

    who = "dta_abundance_resample_grouped"
    for kw in ({"label": None}, {"gs": None}, {"order": None}, {"table": None}, {"counts": None}, {"ws": None}):
        assert resample(**kw) != 0 and who in err() and "null" in err(), kw
    for kw, what in (({"n": 0}, "n="), ({"groups": 0}, "groups"), ({"groups": -3}, "groups"), ({"groups": 2 ** 31 - 1}, "groups"),
                     ({"species": 0}, "species"), ({"species": 257}, "species"), ({"iterations": -1}, "iterations")):
        assert resample(**kw) != 0 and who in err() and what in err(), (kw, err())
    need = lib.dta_abundance_grouped_workspace_bytes(10, 6, 3, 4)
    assert need >= 10 * 12 and need % 8 == 0
    assert resample(ws_bytes=need - 1) != 0 and who in err() and "workspace too small" in err()
    assert resample(ws=odd) != 0 and who in err() and "aligned" in err()
    assert resample(iterations=0) == 0                          # an empty table: nothing to write, nothing launched
    who = "dta_abundance_counts_grouped"
    for kw in ({"label": None}, {"gs": None}, {"order": None}, {"out": None}, {"ws": None}):
        assert counts(**kw) != 0 and who in err() and "null" in err(), kw
    for kw, what in (({"n": 0}, "n="), ({"groups": 0}, "groups"), ({"species": 0}, "species"), ({"species": 257}, "species")):
        assert counts(**kw) != 0 and who in err() and what in err(), (kw, err())
    need1 = lib.dta_abundance_grouped_workspace_bytes(10, 6, 1, 4)
    assert counts(ws_bytes=need1 - 1) != 0 and who in err() and "workspace too small" in err()
    assert counts(ws=odd) != 0 and who in err() and "aligned" in err()
    for args in ((0, 6, 3, 4), (10, 0, 3, 4), (10, 257, 3, 4), (10, 6, -1, 4), (10, 6, 3, 0)):
        assert lib.dta_abundance_grouped_workspace_bytes(*args) == 0 and "dta_abundance_grouped_workspace_bytes" in err(), args
    # the workspace grows with the crowns, not with the cells or the iterations: nothing per cell is kept
    assert lib.dta_abundance_grouped_workspace_bytes(1000, 6, 3, 4) == lib.dta_abundance_grouped_workspace_bytes(1000, 200, 100, 8000)

    who = "dta_abundance_cells"

    def cells(boxes=p, n=10, rule=0, origin=org, size=1000.0, cols=3, rows=3, out=p):
        return lib.dta_abundance_cells(boxes, n, rule, origin, size, cols, rows, out, None)

    for kw in ({"boxes": None}, {"origin": None}, {"out": None}):
        assert cells(**kw) != 0 and who in err() and "null" in err(), kw
    for kw, what in (({"n": 0}, "n="), ({"cols": 0}, "cols"), ({"rows": -1}, "rows"), ({"rule": 2}, "rule"), ({"size": 0.0}, "size"),
                     ({"size": float("nan"), "rule": 1}, "size"), ({"size": 0.5}, "integer"),
                     ({"origin": (C.c_double * 2)(0.5, 0.0)}, "integer"), ({"origin": (C.c_double * 2)(float("inf"), 0.0), "rule": 1}, "finite")):
        assert cells(**kw) != 0 and who in err() and what in err(), (kw, err())

    who = "dta_abundance_summary"
    lower, frac = (C.c_int * 3)(0, 1, 2), (C.c_double * 3)(0.0, 0.5, 0.25)

    def summary(table=p, iterations=3, entries=7, lower=lower, frac=frac, nq=3, mean=p, quant=p):
        return lib.dta_abundance_summary(table, iterations, entries, lower, frac, nq, mean, quant, None)

    for kw in ({"table": None}, {"mean": None}, {"quant": None}, {"lower": None}, {"frac": None}):
        assert summary(**kw) != 0 and who in err() and "null" in err(), kw
    from deeptreeattention_amd import _lib
    cap = _lib.ABUNDANCE_SUMMARY_MAX_ITERATIONS
    for kw, what in (({"iterations": 0}, "iterations"), ({"iterations": cap + 1}, "DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS"),
                     ({"entries": 0}, "entries"), ({"nq": -1}, "quantiles"), ({"nq": 17}, "quantiles"),
                     ({"lower": (C.c_int * 3)(0, 3, 0)}, "lower"), ({"frac": (C.c_double * 3)(0.0, 1.0, 0.0)}, "frac"),
                     ({"frac": (C.c_double * 3)(0.0, float("nan"), 0.0)}, "frac")):
        assert summary(**kw) != 0 and who in err() and what in err(), (kw, err())


def test_python_route_checks_its_arguments_on_the_host():
    import torch
    from deeptreeattention_amd import abundance
    with pytest.raises(ValueError, match="boxes"):
        abundance.cells(torch.zeros(4, 4, dtype=torch.float64), 2, 2)           # not on the device
    with pytest.raises(ValueError, match="rule"):
        abundance.cells(torch.zeros(4, 4, dtype=torch.float64), 2, 2, rule="nearest")
    with pytest.raises(ValueError, match="counts must be"):
        abundance.summary_device(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="label"):
        abundance.resample(torch.zeros(4, dtype=torch.int64), None, np.full((1, 1), 1 << 24, np.uint32),
                           group=torch.zeros(4, dtype=torch.int64), groups=1)
