"""Field records to canopy points, host side (no GPU): the NumPy definitions (field.filter_np, field.plots_np) against the
reference's own recorded answers (tests/golden/field, made by tools/make_field_golden.py from the reference's filter_data)
and against a line-by-line re-statement of create_grid and buffer_plots; a hand-made table with the reasons written out;
the C entries' refusals, none of which reaches a launch; the Python route's host-side argument checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import field_cases as FC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = FC.GOLDEN


# ---------------------------------------------------------------------------------------------------------------------
# filter_data against the reference's recorded answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "field_reference.npz"))


def test_fixture_checksums():
    """tests/golden/field has a checksum file of its own, written by tools/make_field_golden.py."""
    import hashlib
    lines = [ln.split() for ln in open(os.path.join(GOLDEN, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert sorted(name for _, name in lines) == ["field_reference.npz", "field_rules.json"]
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == digest, name


@pytest.mark.parametrize("name", ("sample", "synthetic"))
def test_definition_reproduces_the_reference_on_its_recorded_tables(recorded, name):
    from deeptreeattention_amd import field
    df = FC.frame_of(recorded, name)
    want, taxa = recorded[name + "_kept"], recorded[name + "_taxon"]
    table = field.FieldTable.from_frame(df)
    got = field.filter_np(dict(table.columns, individuals=table.individuals), float(recorded["min_stem_diameter"]))
    assert int(got.count) == len(want) and np.array_equal(got.rows[:len(want)], want) and (got.rows[len(want):] == -1).all()
    assert np.array_equal(np.flatnonzero(got.keep), np.sort(want))
    out = field.filter_data(df, {"min_stem_diameter": float(recorded["min_stem_diameter"])}, device=None)
    assert out.index.tolist() == want.tolist()                     # the reference's order
    assert out.taxonID.astype(str).tolist() == taxa.tolist()       # the remapped taxa
    assert out.individual.tolist() == recorded[name + "_individual"].tolist()
    seen = np.bincount(got.reason, minlength=14)
    if name == "sample":
        assert len(df) == 86 and len(want) == 15 and not np.isnan(table.columns["height"][want]).any()
    else:
        assert seen.min() >= 1, seen                               # the recorded table reaches every step
        assert np.isnan(table.columns["height"][want]).sum() >= 3 and (~np.isnan(table.columns["height"][want])).sum() >= 3


def test_filter_data_reads_a_csv(recorded, tmp_path):
    from deeptreeattention_amd import field
    path = os.path.join(str(tmp_path), "field.csv")
    FC.frame_of(recorded, "synthetic").to_csv(path, index=False)
    out = field.filter_data(path, {"min_stem_diameter": float(recorded["min_stem_diameter"])})
    assert out.index.tolist() == recorded["synthetic_kept"].tolist()


def test_reference_rules_equal_the_recorded_lists():
    from deeptreeattention_amd import field
    want = json.load(open(os.path.join(GOLDEN, "field_rules.json")))
    rules = field.Rules.reference()
    assert rules.as_lists() == want
    assert len(rules.remap) == 15 and len(rules.taxa_excluded) == 8 and rules.event_excluded == "2014"
    assert rules.multibole == "[A-Z]$" and "SOAP_054" in rules.plots_excluded and len(rules.plots_excluded) == 6
    assert set(rules.sites_excluded) == {"PUUM", "ORNL"}


def test_a_table_that_needs_the_reprojection_is_refused(recorded):
    from deeptreeattention_amd import field
    df = FC.frame_of(recorded, "sample")
    df.loc[3, ["siteID", "utmZone"]] = ["BLAN", "18N"]
    with pytest.raises(ValueError, match="reprojection"):
        field.FieldTable.from_frame(df)
    df = FC.frame_of(recorded, "sample")
    df.loc[5, "eventID"] = np.nan
    with pytest.raises(ValueError, match="eventID must not be null"):
        field.FieldTable.from_frame(df)
    with pytest.raises(ValueError, match="lacks the columns plotID"):
        field.FieldTable.from_frame(FC.frame_of(recorded, "sample").drop(columns=["plotID"]))


# ---------------------------------------------------------------------------------------------------------------------
# the reason codes, and the families the device tests run
# ---------------------------------------------------------------------------------------------------------------------
def test_reason_codes_follow_the_hand_made_table():
    from deeptreeattention_amd import field
    case, want = FC.hand()
    got = FC.run_np(case)
    assert got.keep.dtype == np.uint8 and got.reason.dtype == np.uint8 and got.rows.dtype == np.int64
    assert got.reason.tolist() == want.tolist()
    assert got.keep.tolist() == (want == 0).astype(int).tolist()
    assert got.index().tolist() == FC.HAND_ROWS and int(got.count) == len(FC.HAND_ROWS)
    assert (got.rows[len(FC.HAND_ROWS):] == -1).all() and len(got.rows) == len(want)
    # codes out of range take part in nothing
    bad = dict(case["columns"])
    bad["individual"] = bad["individual"].copy()
    bad["individual"][[7, 20]] = (-1, 13)
    bad["event"] = bad["event"].copy()
    bad["event"][26] = -4
    worse = field.filter_np(bad, 10.0)
    assert worse.reason[[7, 20, 26]].tolist() == [255, 255, 255]
    assert worse.reason[19] == 0 and worse.reason[6] == 4            # their individuals go on without them: row 7 was the
    assert worse.index().tolist() == [3, 16, 19, 13]                 # sunny year of individual 2
    assert len(field.REASONS) == 14


def test_the_synthetic_family_reaches_every_step():
    case = FC.synthetic()
    c = case["columns"]
    sizes = np.bincount(c["individual"], minlength=1200)
    assert len(c["individual"]) == 3000 and sizes.min() == 1 and sizes.max() == 6
    seen = FC.census(case, FC.run_np(case))
    print(seen)
    assert min(seen["reason"]) >= 5 and sum(seen["reason"]) == 3000
    assert seen["by_height"] >= 20 and seen["by_event"] >= 20


def test_the_special_table_is_decided_by_step_nine():
    case = FC.special()
    got = FC.run_np(case)
    c = case["columns"]
    assert (c["individual"] == 1).sum() == 700 and c["individual"][0] == c["individual"][-1] == 0
    n = len(got.reason)
    assert got.index().tolist() == [n - 1, 131, 701, 704, 708, 709, 712, 715, 718, 720, 728, 731, 723, 725]
    assert got.reason[722] == 5 and set(np.unique(got.reason).tolist()) == {0, 5, 9}


# ---------------------------------------------------------------------------------------------------------------------
# megaplot: plots_np against the reference's loops, re-stated line by line
# ---------------------------------------------------------------------------------------------------------------------
def create_grid_and_join(points, cell=40.0):
    """create_grid (src/megaplot.py:69-90) and the join of :43 with the head(1) of :48: the cells in the order of its two
    loops, box(x0, y0, x0 - cell, y0 + cell) as its closed rectangle, every point given the first cell that holds it."""
    xmin, ymin = points.min(axis=0)
    xmax, ymax = points.max(axis=0)
    grid_cells = []
    for x0 in np.arange(xmin, xmax + cell, cell):
        for y0 in np.arange(ymin, ymax + cell, cell):
            x1 = x0 - cell
            y1 = y0 + cell
            grid_cells.append((min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1)))
    cells = np.array(grid_cells)
    code = np.full(len(points), -1, np.int64)
    for k, (x, y) in enumerate(points):
        inside = np.flatnonzero((cells[:, 0] <= x) & (x <= cells[:, 2]) & (cells[:, 1] <= y) & (y <= cells[:, 3]))
        if len(inside):
            code[k] = inside[0]
    return code, len(cells)


def buffer_plots(points, cell=40.0):
    """buffer_plots (:56-67) as the sequential loop it is, the disc of radius cell as the buffer."""
    plot = np.full(len(points), -1, np.int64)
    plotID = 0
    for x, y in points:
        dx, dy = points[:, 0] - x, points[:, 1] - y
        touches = dx * dx + dy * dy <= cell * cell
        if touches.any():
            plot[touches] = plotID
            plotID += 1
    return plot


def test_grid_rule_equals_the_reference_loops_on_the_lattice():
    from deeptreeattention_amd import field
    points = FC.lattice()
    shared = FC.cells_holding(points)
    assert (shared >= 2).sum() >= 20 and (shared >= 4).sum() >= 5 and shared.min() >= 1     # lines, corners
    got = field.plots_np(points, "grid")
    want, cells = create_grid_and_join(points)
    assert got.code.dtype == np.int32 and got.plots == cells == 121
    assert np.array_equal(got.code, want)
    # the bounds themselves: the least point lies in cell (0, 0), whose left neighbour does not exist
    assert got.code[0] == 0 and got.code[1] == 10 * 11 + 9            # (the top edge is shared: the lower row of cells)
    for n in (1, 2, 1000, 1001):
        p = FC.auto(n)
        assert np.array_equal(field.plots_np(p, "grid").code, create_grid_and_join(p)[0]), n


def test_buffer_rule_equals_the_reference_loop_on_ring_and_lattice():
    from deeptreeattention_amd import field
    ring = FC.ring()
    assert FC.pairs_exactly_at(ring) >= 5
    got = field.plots_np(ring, "buffer")
    assert np.array_equal(got.code, buffer_plots(ring)) and got.plots == len(ring) and got.code.min() >= 0
    lattice = FC.lattice(700, seed=12, span=900)
    assert FC.pairs_exactly_at(lattice) >= 5
    assert np.array_equal(field.plots_np(lattice, "buffer").code, buffer_plots(lattice))
    for n in (1, 2, 1000):
        p = FC.auto(n)
        assert np.array_equal(field.plots_np(p, "buffer").code, buffer_plots(p)), n


def test_auto_is_the_reference_switch_and_odd_points_get_no_plot():
    from deeptreeattention_amd import field
    for n, rule in ((1, "buffer"), (2, "buffer"), (1000, "buffer"), (1001, "grid")):
        p = FC.auto(n)
        auto, named = field.plots_np(p), field.plots_np(p, rule)
        assert np.array_equal(auto.code, named.code) and auto.plots == named.plots == (n if rule == "buffer" else named.plots)
    p = FC.lattice(40, seed=2)
    p[3, 0], p[7, 1], p[9] = np.nan, np.inf, (-np.inf, np.nan)
    for rule in ("grid", "buffer"):
        got = field.plots_np(p, rule)
        assert (got.code[[3, 7, 9]] == -1).all() and (np.delete(got.code, [3, 7, 9]) >= 0).all()
    clean = np.delete(p, [3, 7, 9], axis=0)
    assert np.array_equal(np.delete(field.plots_np(p, "grid").code, [3, 7, 9]), field.plots_np(clean, "grid").code)
    assert field.plot_names(np.array([3, 12]), "OSBS_2019", "grid") == ["3_contrib", "12_contrib"]
    assert field.plot_names(np.array([3, 12]), "OSBS_2019", "buffer") == ["OSBS_2019_contrib_3", "OSBS_2019_contrib_12"]


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
    import deeptreeattention_amd
    from deeptreeattention_amd import _lib, build, field
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    new = {"dta_field_filter", "dta_field_workspace_bytes", "dta_megaplot_plots"}
    assert {n for n in names if n.startswith(("dta_field_", "dta_megaplot_"))} == new
    for n in new:
        assert hasattr(lib, n) and '"%s"' % n in entry
    assert len(lib.dta_field_filter.argtypes) == 17 and lib.dta_field_filter.restype is C.c_int
    assert len(lib.dta_megaplot_plots.argtypes) == 10 and lib.dta_field_workspace_bytes.restype is C.c_size_t
    assert "field.hip" in build.SOURCES and build.SOURCES[-1] == "boundary.hip"

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    for name in ("COORDS", "GROWTH", "LIVE", "SHADED", "SUNNY", "TAXON_EXCLUDED", "EVENT_DROPPED", "MULTIBOLE", "KNOWN_ERROR",
                 "PLOT_EXCLUDED", "SITE_EXCLUDED"):
        assert macro("DTA_FIELD_" + name) == getattr(_lib, "FIELD_" + name) == getattr(field, name)
    assert macro("DTA_FIELD_REASON_BAD_CODE") == _lib.FIELD_REASON_BAD_CODE == field.BAD_CODE == 255
    assert macro("DTA_MEGAPLOT_GRID") == _lib.MEGAPLOT_GRID == field.GRID and macro("DTA_MEGAPLOT_BUFFER") == field.BUFFER == 1
    assert macro("DTA_MEGAPLOT_BUFFER_MAX") == _lib.MEGAPLOT_BUFFER_MAX == field.BUFFER_MAX == 65536
    assert lib.dta_abi_version() == 2 and macro("DTA_ABI_VERSION") == 2
    assert "deeptreeattention_amd.field" in deeptreeattention_amd.__doc__


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the device pointers are host buffers nobody
    dereferences."""
    buf = (C.c_ubyte * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    nan, inf = float("nan"), float("inf")
    assert lib.dta_field_workspace_bytes(0, 1) == 0 and lib.dta_field_workspace_bytes(1 << 31, 5) == 0
    assert lib.dta_field_workspace_bytes(10, 0) == 0 and lib.dta_field_workspace_bytes(10, 11) == 0
    need = lib.dta_field_workspace_bytes(100, 40)
    assert 40 * 28 <= need <= 2048 and need % 16 == 0
    assert lib.dta_field_workspace_bytes(1000, 1000) > need

    def call(individual=p, event=p, height=p, diameter=p, flags=p, rows=100, individuals=40, min_d=10.0, min_h=3.0, keep=p,
             reason=p, rows_out=p, count=p, errors=None, workspace=p, nbytes=need):
        return lib.dta_field_filter(individual, event, height, diameter, flags, rows, individuals, min_d, min_h, keep, reason,
                                    rows_out, count, errors, workspace, nbytes, None)

    cases = [({k: None}, "null") for k in ("individual", "event", "height", "diameter", "flags", "keep", "reason", "rows_out",
                                            "count", "workspace")]
    cases += [({"rows": 0}, "rows=0"), ({"rows": -1}, "rows=-1"), ({"rows": 1 << 31}, "rows=2147483648"),
              ({"individuals": 0}, "individuals=0"), ({"individuals": 101}, "individuals=101"), ({"min_d": nan}, "min_stem_diameter"),
              ({"min_h": nan}, "min_height"), ({"nbytes": need - 1}, "workspace"),
              ({"workspace": C.c_void_p(p.value + 8)}, "workspace"), ({"individuals": 100}, "workspace")]
    for kw, what in cases:
        assert call(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_field_filter: ") and what in err, (kw, err)

    def plots(points=p, n=50, rule=0, cell=40.0, xs=p, nx=4, ys=p, ny=5, code=p):
        return lib.dta_megaplot_plots(points, n, rule, cell, xs, nx, ys, ny, code, None)

    cases = [({"points": None}, "null"), ({"code": None}, "null"), ({"xs": None}, "null xs or ys"), ({"ys": None}, "null xs or ys"),
             ({"rule": 2}, "rule=2"), ({"rule": -1}, "rule=-1"), ({"cell": 0.0}, "cell=0"), ({"cell": -40.0}, "cell=-40"),
             ({"cell": nan}, "cell=nan"), ({"cell": inf}, "cell=inf"), ({"rule": 1, "cell": 1e200}, "cell * cell"),
             ({"n": 0}, "n=0"), ({"n": 1 << 31}, "n=2147483648"), ({"rule": 1, "n": 0}, "n=0"), ({"rule": 1, "n": 65537}, "n=65537"),
             ({"nx": 0}, "nx=0"), ({"ny": -2}, "ny=-2"), ({"nx": 1 << 16, "ny": 1 << 15}, "nx=65536, ny=32768")]
    for kw, what in cases:
        assert plots(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_megaplot_plots: ") and what in err, (kw, err)


# ---------------------------------------------------------------------------------------------------------------------
# the Python route's own argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_python_route_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached."""
    import torch
    from deeptreeattention_amd import _lib, field

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    case, _ = FC.hand()
    good = case["columns"]
    n = len(good["individual"])
    for key, value, what in (("individual", good["individual"][1:], "one-dimensional"), ("individual", good["height"], "individual"),
                             ("event", good["event"].astype(np.float64), "event"), ("height", good["height"].astype(np.float32), "height"),
                             ("height", good["height"][:, None], "height"), ("diameter", good["event"], "diameter"),
                             ("flags", good["flags"].astype(np.int64) + 2 ** 16, "flags"), ("flags", good["diameter"], "flags"),
                             ("individuals", 0, "individuals"), ("individuals", n + 1, "individuals"), ("individuals", 2.0, "individuals")):
        with pytest.raises(ValueError, match=what):
            field.filter_np(dict(good, **{key: value}), 10.0)
        with pytest.raises(ValueError, match=what):
            field.FieldTable(dict(good, **{key: value}))
    with pytest.raises(ValueError, match="columns must be a dict"):
        field.filter_np({k: v for k, v in good.items() if k != "flags"}, 10.0)
    for bad in (np.nan, "thick", None):
        with pytest.raises(ValueError, match="min_stem_diameter"):
            field.filter_np(good, bad)
        with pytest.raises(ValueError, match="min_stem_diameter"):
            field.FieldTable(good).filter(bad)
    with pytest.raises(ValueError, match="min_height"):
        field.filter_np(good, 10.0, np.nan)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        field.FieldTable(good, device="cpu")
    t = {k: torch.from_numpy(good[k].view(np.int16) if k == "flags" else good[k]) for k in field._COLUMNS}
    for key, value in (("individual", t["individual"].long()), ("height", t["height"].float()), ("event", t["event"][:-1]),
                       ("diameter", t["diameter"][::2]), ("flags", good["flags"]), ("individuals", 0), ("individuals", n + 1)):
        with pytest.raises(ValueError, match="resident|individuals"):
            field.FieldTable.resident(**dict(dict(t, individuals=13), **{key: value}))
    with pytest.raises(RuntimeError, match="ROCm device only"):        # host tensors pass the checks and find no device
        field.FieldTable.resident(individuals=13, **t)
    host = field.FieldTable(good).filter(10.0)                       # a table without a device runs the definition
    assert host.reason.tolist() == FC.run_np(case).reason.tolist()
    pts = FC.lattice(30)
    for kw, what in (({"points": pts.astype(np.float32)}, "points"), ({"points": pts[:0]}, "points"), ({"points": pts[:, :1]}, "points"),
                     ({"points": pts.reshape(-1)}, "points"), ({"points": torch.from_numpy(pts).float()}, "points"),
                     ({"rule": "disc"}, "rule"), ({"cell": 0.0}, "cell"), ({"cell": -1.0}, "cell"), ({"cell": np.nan}, "cell"),
                     ({"cell": np.inf}, "cell"), ({"cell": "wide"}, "cell"), ({"cell": 1e200}, "cell"),
                     ({"points": np.zeros((field.BUFFER_MAX + 1, 2)), "rule": "buffer"}, "at most 65536"),
                     ({"points": np.full((3, 2), np.nan), "rule": "grid"}, "no point has finite"),
                     ({"points": np.array([[0.0, 0.0], [1e12, 1e12]]), "rule": "grid", "cell": 1.0}, "2\\^31")):
        for fn in (field.plots_np, field.megaplot_plots):
            with pytest.raises(ValueError, match=what):
                fn(**dict(dict(points=pts, rule="auto", cell=40.0), **kw))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        field.megaplot_plots(pts, device="cpu")
    assert np.array_equal(field.megaplot_plots(pts, device=None).code, field.plots_np(pts).code)
    with pytest.raises(ValueError, match="rule"):
        field.plot_names(np.arange(3), "x", "auto")
