"""Site boundary clip, host side (no GPU): the NumPy definition (boundary.contains_np / boxes_np / rasterise_np / geo_boxes)
on pinned cases, under re-statements of the same boundary (orientation, closing vertex, ring order), against matplotlib's
Path on a seeded star with a hole and an island at UTM magnitudes; the C entries' refusals, none of which reaches a launch;
the Python route's host-side argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import boundary_cases as BC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = np.array([(0, 0), (4, 0), (4, 4), (0, 4)], np.float64)


def f64(rows):
    return np.array(rows, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# pinned cases
# ---------------------------------------------------------------------------------------------------------------------
def test_points_on_the_line_of_a_square():
    """The rule puts the left and the bottom side in, the right and the top side out; nothing more is promised."""
    from deeptreeattention_amd import boundary as B
    got = B.contains_np([SQUARE], f64([(0, 2), (2, 0), (4, 2), (2, 4)]))
    assert got.dtype == np.uint8 and got.tolist() == [1, 1, 0, 0]
    assert B.contains_np([SQUARE], f64([(2, 2), (5, 2), (-1, 2), (2, 5), (2, -1)])).tolist() == [1, 0, 0, 0, 0]
    # the same square anywhere: org is subtracted once from the table and once from the query
    far = SQUARE + f64(BC.UTM)
    assert B.contains_np([far], f64([(0, 2), (2, 0), (4, 2), (2, 4), (2, 2)]) + f64(BC.UTM)).tolist() == [1, 1, 0, 0, 1]


def test_nan_and_infinite_points_are_outside():
    from deeptreeattention_amd import boundary as B
    nan, inf = np.nan, np.inf
    pts = f64([(nan, 2), (2, nan), (nan, nan), (inf, 2), (-inf, 2), (2, inf), (2, -inf), (inf, inf)])
    assert B.contains_np([SQUARE], pts).tolist() == [0] * 8


def test_the_same_boundary_said_differently():
    """Orientation reversed, a ring closed or not, rings in another order, a vertex repeated: the same masks."""
    from deeptreeattention_amd import boundary as B
    rings = BC.prototype_site()
    pts = BC.points(rings, 3000, 11)
    boxes, t = BC.pixel_boxes(rings, 800, 12)
    ref_p, ref_b = B.contains_np(rings, pts), B.boxes_np(rings, pixel_boxes=boxes, transform=t)
    ref_r = B.rasterise_np(rings, 23, 31, (BC.UTM[0], 150.0, BC.UTM[1] + 4200.0, -190.0))
    assert 0 < ref_p.sum() < len(pts) and set(ref_b.tolist()) == {0, 1, 2} and 0 < ref_r.sum() < ref_r.size
    closed = [np.concatenate([r, r[:1]]) for r in rings]
    doubled = [np.repeat(r, 2, axis=0) for r in rings]                      # zero-length edges are dropped
    for other in ([r[::-1] for r in rings], closed, rings[::-1], [rings[1], rings[2], rings[0]], doubled,
                  [np.roll(r, 5, axis=0) for r in rings]):
        assert np.array_equal(B.contains_np(other, pts), ref_p)
        assert np.array_equal(B.boxes_np(other, pixel_boxes=boxes, transform=t), ref_b)
        assert np.array_equal(B.rasterise_np(other, 23, 31, (BC.UTM[0], 150.0, BC.UTM[1] + 4200.0, -190.0)), ref_r)
    assert len(B.edge_table(doubled).edges) == len(B.edge_table(rings).edges) == 257 + 31 + 17
    assert np.array_equal(B.edge_table(closed).edges, B.edge_table(rings).edges)


def test_hole_and_island_are_even_odd():
    from deeptreeattention_amd import boundary as B
    outer = f64([(0, 0), (20, 0), (20, 20), (0, 20)])
    hole = f64([(5, 5), (15, 5), (15, 15), (5, 15)])
    island = f64([(8, 8), (12, 8), (12, 12), (8, 12)])                     # a part inside the hole
    apart = f64([(30, 0), (34, 0), (34, 4), (30, 4)])                      # a part of its own
    rings = [outer, hole, island, apart]
    pts = f64([(2, 2), (6, 6), (10, 10), (32, 2), (25, 2), (6, 18)])
    assert B.contains_np(rings, pts).tolist() == [1, 0, 1, 1, 0, 1]
    assert B.contains_np([outer, hole[::-1], island, apart[::-1]], pts).tolist() == [1, 0, 1, 1, 0, 1]
    boxes = f64([(1, 1, 3, 3),        # in the ring of land
                 (6, 6, 7, 7),        # in the hole: disjoint
                 (9, 9, 11, 11),      # on the island
                 (4, 4, 6, 6),        # over the hole's corner
                 (6, 6, 14, 14),      # in the hole, around the island: crosses the island's line
                 (31, 1, 33, 3), (22, 1, 28, 3), (-5, -5, 40, 40)])
    assert B.boxes_np(rings, geo_boxes=boxes).tolist() == [2, 0, 2, 1, 1, 2, 0, 1]


def test_a_spike_crosses_a_box_whose_corners_are_all_inside():
    from deeptreeattention_amd import boundary as B
    notched = f64([(0, 0), (10, 0), (10, 10), (5.1, 10), (5, 3), (4.9, 10), (0, 10)])
    box = f64([(4, 2, 6, 4), (4, 1, 6, 2.5), (1, 1, 3, 3)])
    corners = f64([(4, 2), (6, 2), (6, 4), (4, 4)])
    assert B.contains_np([notched], corners).tolist() == [1, 1, 1, 1]
    assert B.boxes_np([notched], geo_boxes=box).tolist() == [1, 2, 2]


def test_touching_degenerate_and_refused_boxes():
    from deeptreeattention_amd import boundary as B
    nan, inf = np.nan, np.inf
    boxes = f64([(4, 1, 5, 2), (4, 4, 5, 5), (-1, -1, 0, 0), (1, -2, 3, 0), (-3, 0, 0, 4),      # share a side or a corner
                 (2, 2, 2, 2), (4, 2, 4, 2), (1, 2, 3, 2), (5, 5, 5, 5), (2, -1, 2, 5),         # points and lines
                 (4.5, 1, 5, 2), (0, 0, 4, 4), (0.5, 0.5, 3.5, 3.5)])
    assert B.boxes_np([SQUARE], geo_boxes=boxes).tolist() == [1, 1, 1, 1, 1, 2, 1, 2, 0, 1, 0, 1, 2]
    bad = f64([(nan, 1, 2, 2), (1, nan, 2, 2), (1, 1, nan, 2), (1, 1, 2, nan), (inf, 1, 2, 2), (1, 1, inf, 2), (-inf, 1, 2, 2),
               (1, -inf, 2, inf), (3, 1, 1, 2), (1, 3, 2, 1), (3, 3, 1, 1)])
    assert B.boxes_np([SQUARE], geo_boxes=bad).tolist() == [0] * len(bad)
    assert B.boxes_np([SQUARE], geo_boxes=f64([(1, 1, 2, 2)])).tolist() == [2]


def test_geo_boxes_negative_e_and_non_square_pixels():
    from deeptreeattention_amd import boundary as B
    t = (405000.0, 0.5, 3305000.0, -0.25)
    boxes = np.array([(0, 0, 4, 8), (10, 20, 10, 21), (7, 3, 2, 1), (-4, -8, 0, 0)], np.int32)
    got = B.geo_boxes(boxes, t)
    assert got.dtype == np.float64 and got.tolist() == [[405000.0, 3304999.0, 405004.0, 3305000.0],
                                                         [405010.0, 3304997.5, 405010.5, 3304997.5],
                                                         [405000.5, 3304998.25, 405001.5, 3304999.5],
                                                         [404996.0, 3305000.0, 405000.0, 3305001.0]]
    # the product and the sum are rounded one by one
    t3 = (0.1, 0.3, 0.7, -0.3)
    b = np.array([(3, 7, 11, 13)], np.int64)
    x = [np.float64(0.1) + np.float64(c) * np.float64(0.3) for c in (7, 13)]
    y = [np.float64(0.7) + np.float64(r) * np.float64(-0.3) for r in (3, 11)]
    assert B.geo_boxes(b, t3).tolist() == [[min(x), min(y), max(x), max(y)]]
    # a positive e (south-up) and a negative a: min / max per axis
    assert B.geo_boxes(np.array([(0, 0, 2, 2)]), (10.0, -1.0, 20.0, 1.0)).tolist() == [[8.0, 20.0, 10.0, 22.0]]
    ring = [f64([(405000.5, 3304990), (405020, 3304990), (405020, 3305010), (405000.5, 3305010)])]
    assert np.array_equal(B.boxes_np(ring, pixel_boxes=boxes, transform=t), B.boxes_np(ring, geo_boxes=got))
    assert B.boxes_np(ring, pixel_boxes=boxes, transform=t).tolist() == [1, 2, 1, 0]
    for bad in ((0, 0, 0, 1), (0, 1, 0, 0), (0, np.nan, 0, 1), (0, 1, np.inf, 1), (0, 1, 0)):
        with pytest.raises(ValueError, match="transform"):
            B.geo_boxes(boxes, bad)
    with pytest.raises(ValueError, match="pixel_boxes"):
        B.geo_boxes(boxes.astype(np.float64), t)


def test_rasterise_is_contains_of_the_cell_centres():
    from deeptreeattention_amd import boundary as B
    got = B.rasterise_np([SQUARE], 3, 3, (-1.0, 2.0, 5.0, -2.0))          # centres at x = 0, 2, 4 and y = 4, 2, 0
    assert got.dtype == np.uint8 and got.tolist() == [[0, 0, 0], [1, 1, 0], [1, 1, 0]]
    rings = BC.prototype_site()
    t = (BC.UTM[0] - 100.0, 37.5, BC.UTM[1] + 4100.0, -41.0)
    mask = B.rasterise_np(rings, 40, 29, t)
    centres = B.cell_centres(40, 29, t)
    assert centres[29 * 3 + 5].tolist() == [t[0] + 5.5 * 37.5, t[2] + 3.5 * -41.0]
    assert np.array_equal(mask.reshape(-1), B.contains_np(rings, centres))


def test_from_geojson():
    from deeptreeattention_amd import boundary as B
    outer = [(0, 0), (20, 0), (20, 20), (0, 20), (0, 0)]
    hole = [(5, 5), (5, 15), (15, 15), (15, 5), (5, 5)]
    part = [(30.0, 0.0, 7.0), (34.0, 0.0, 7.0), (34.0, 4.0, 7.0), (30.0, 4.0, 7.0), (30.0, 0.0, 7.0)]     # with a z
    poly = {"type": "Polygon", "coordinates": [outer, hole]}
    multi = {"type": "MultiPolygon", "coordinates": [[outer, hole], [part]]}
    pts = f64([(2, 2), (10, 10), (32, 2)])
    r = B.geojson_rings(poly)
    assert len(r) == 2 and r[0].shape == (5, 2) and r[0].dtype == np.float64
    assert B.contains_np(r, pts).tolist() == [1, 0, 0]
    assert B.contains_np(B.geojson_rings(multi), pts).tolist() == [1, 0, 1]
    assert len(B.edge_table(B.geojson_rings(multi)).edges) == 12

    class Shape:                                                             # what shapely geometries offer
        __geo_interface__ = multi
    assert B.contains_np(B.geojson_rings(Shape()), pts).tolist() == [1, 0, 1]
    for bad in ({"type": "Point", "coordinates": [1, 2]}, {"type": "Polygon", "coordinates": []}, [outer]):
        with pytest.raises(ValueError, match="Polygon|empty"):
            B.geojson_rings(bad)
    import sys
    assert "geopandas" not in sys.modules and "shapely" not in sys.modules
    # the constructor route reaches the device check with the rings read: no GPU here, so only the refusal is seen
    with pytest.raises(RuntimeError, match="ROCm device only"):
        B.Boundary.from_geojson(multi, device="cpu")


def test_edge_table_refusals():
    from deeptreeattention_amd import boundary as B
    for bad, what in (([], "empty"), ([SQUARE[:2]], "at least 3"), ([np.zeros((4, 3))], r"\[K, 2\]"),
                      ([f64([(0, 0), (1, np.nan), (1, 1)])], "finite"), ([f64([(0, 0), (1, 1), (0, 0)])], "at least 3"),
                      ([f64([(1, 1), (1, 1), (1, 1), (1, 1)])], "edges")):
        with pytest.raises(ValueError, match=what):
            B.edge_table(bad)
    t = B.edge_table([SQUARE + 7.0])
    assert t.org.tolist() == [7.0, 7.0] and t.edges.dtype == np.float64 and t.edges.flags["C_CONTIGUOUS"]
    assert t.edges.tolist() == [[0, 0, 4, 0], [4, 0, 4, 4], [4, 4, 0, 4], [0, 4, 0, 0]]
    assert B.edge_table(SQUARE).edges.shape == (4, 4)                      # a single ring as it is


# ---------------------------------------------------------------------------------------------------------------------
# the definition against matplotlib's Path
# ---------------------------------------------------------------------------------------------------------------------
def nearest_edge(rings, pts):
    """The distance of every point to the nearest edge, in float64 on coordinates moved to the boundary's corner."""
    org = np.concatenate(rings).min(axis=0)
    p = pts - org
    best = np.full(len(p), np.inf)
    for r in rings:
        a = r - org
        b = np.roll(a, -1, axis=0)
        d = b - a
        for k in range(len(a)):
            w = p - a[k]
            s = np.clip((w @ d[k]) / (d[k] @ d[k]), 0.0, 1.0)
            best = np.minimum(best, np.linalg.norm(w - s[:, None] * d[k], axis=1))
    return best


def test_points_agree_with_matplotlib_ring_by_ring():
    """matplotlib ORs the subpaths of a compound path, so the oracle for holes is contains_points per ring, XOR-ed.  Points
    nearer than 1e-6 m to an edge could be left out; with these seeded inputs none is."""
    Path = pytest.importorskip("matplotlib.path").Path
    from deeptreeattention_amd import boundary as B
    rings = BC.prototype_site()
    assert [len(r) for r in rings] == [257, 31, 17] and np.concatenate(rings).min() > 4e5
    rng = np.random.default_rng(20)
    x0, y0, x1, y1 = BC.extent(rings)
    pts = np.stack([rng.uniform(x0 - 100, x1 + 100, 20000), rng.uniform(y0 - 100, y1 + 100, 20000)], axis=1)
    dist = nearest_edge(rings, pts)
    print("nearest point to an edge: %.3e m" % dist.min())
    far = dist >= 1e-6
    assert far.all(), "a seeded point lies within 1e-6 m of the boundary line"
    oracle = np.zeros(len(pts), bool)
    for r in rings:
        oracle ^= Path(np.concatenate([r, r[:1]]), closed=True).contains_points(pts)
    got = B.contains_np(rings, pts)
    assert np.array_equal(got[far].astype(bool), oracle[far])
    assert 0.2 < got.mean() < 0.8                              # both answers are well represented
    hole = Path(np.concatenate([rings[1], rings[1][:1]]), closed=True).contains_points(pts)
    island = Path(np.concatenate([rings[2], rings[2][:1]]), closed=True).contains_points(pts)
    assert hole.sum() > 50 and not got[hole].any() and island.sum() > 50 and got[island].all()


def test_boxes_agree_with_matplotlib_on_one_ring():
    mpath = pytest.importorskip("matplotlib.path")
    from matplotlib.transforms import Bbox
    from deeptreeattention_amd import boundary as B
    ring = BC.prototype_site()[0]
    path = mpath.Path(np.concatenate([ring, ring[:1]]), closed=True)
    rng = np.random.default_rng(21)
    x0, y0, x1, y1 = BC.extent([ring])
    lo = np.stack([rng.uniform(x0 - 100, x1 + 60, 3000), rng.uniform(y0 - 100, y1 + 60, 3000)], axis=1)
    boxes = np.concatenate([lo, lo + rng.uniform(1.0, 40.0, (3000, 2))], axis=1)
    code = B.boxes_np([ring], geo_boxes=boxes)
    oracle = np.array([path.intersects_bbox(Bbox([[b[0], b[1]], [b[2], b[3]]]), filled=True) for b in boxes])
    assert np.array_equal(code != 0, oracle)
    assert min((code == c).sum() for c in (0, 1, 2)) > 100
    # code 2 implies four corners inside; four corners inside do not imply code 2 (a spike crosses some such boxes)
    corners = [B.contains_np([ring], boxes[:, ix]).astype(bool) for ix in ([0, 1], [2, 1], [2, 3], [0, 3])]
    four = corners[0] & corners[1] & corners[2] & corners[3]
    assert four[code == 2].all()
    assert ((code == 1) & four).sum() >= 1
    assert not four[code == 0].any()


def test_code_two_means_four_corners_inside_with_hole_and_island():
    from deeptreeattention_amd import boundary as B
    rings = BC.prototype_site()
    boxes, t = BC.pixel_boxes(rings, 4000, 22)
    code = B.boxes_np(rings, pixel_boxes=boxes, transform=t)
    g = B.geo_boxes(boxes, t)
    four = np.ones(len(g), bool)
    for ix in ([0, 1], [2, 1], [2, 3], [0, 3]):
        four &= B.contains_np(rings, np.ascontiguousarray(g[:, ix])).astype(bool)
    assert four[code == 2].all() and (code == 2).sum() > 300 and (code == 0).sum() > 300 and (code == 1).sum() > 50


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, bound, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ("dta_boundary_points", "dta_boundary_boxes", "dta_boundary_raster")


@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from deeptreeattention_amd import _lib, boundary, build
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    for n, nargs in zip(NAMES, (7, 9, 8)):
        assert n in names and hasattr(lib, n) and '"%s"' % n in entry
        assert len(getattr(lib, n).argtypes) == nargs and getattr(lib, n).restype is C.c_int
        assert not n.startswith(("dta_net_", "dta_ensemble_", "dta_multistage_"))
    assert {n for n in names if n.startswith("dta_boundary_")} == set(NAMES)
    assert build.SOURCES[-1] == "boundary.hip"
    chunk = int(re.search(r"#define\s+DTA_BOUNDARY_EDGE_CHUNK\s+(\d+)", hdr).group(1))
    assert chunk == _lib.BOUNDARY_EDGE_CHUNK == boundary.EDGE_CHUNK == 1024
    assert re.search(r"#define\s+DTA_BOUNDARY_MAX_EDGES\s+\(1 << 20\)", hdr)
    assert _lib.BOUNDARY_MAX_EDGES == boundary.MAX_EDGES == 1 << 20
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the device pointers are host buffers nobody
    dereferences; org and transform are host arrays, which the entry reads."""
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def d(*v):
        return (C.c_double * len(v))(*v)

    def err():
        return lib.dta_last_error().decode()

    ORG, T = d(4e5, 3.3e6), d(4e5, 0.5, 3.3e6, -0.5)

    def points(edges=p, n_edges=8, org=ORG, points=p, n=4, out=p):
        return lib.dta_boundary_points(edges, n_edges, org, points, n, out, None)

    def boxes(edges=p, n_edges=8, org=ORG, geo=None, pix=p, t=T, n=4, out=p):
        return lib.dta_boundary_boxes(edges, n_edges, org, geo, pix, t, n, out, None)

    def raster(edges=p, n_edges=8, org=ORG, height=10, width=10, t=T, out=p):
        return lib.dta_boundary_raster(edges, n_edges, org, height, width, t, out, None)

    table = (({"edges": None}, "null"), ({"org": None}, "null"), ({"out": None}, "null"),
             ({"n_edges": 2}, "n_edges=2"), ({"n_edges": 0}, "n_edges=0"), ({"n_edges": -1}, "n_edges=-1"),
             ({"n_edges": (1 << 20) + 1}, "n_edges=1048577"),
             ({"org": d(nan, 0.0)}, "org is not finite"), ({"org": d(0.0, inf)}, "org is not finite"),
             ({"org": d(-inf, 0.0)}, "org is not finite"))
    counts = (({"n": 0}, "n=0"), ({"n": -3}, "n=-3"), ({"n": 1 << 31}, "n=2147483648"))
    transforms = (({"t": d(nan, 1.0, 0.0, -1.0)}, "transform is not finite"), ({"t": d(0.0, inf, 0.0, -1.0)}, "transform is not finite"),
                  ({"t": d(0.0, 1.0, -inf, -1.0)}, "transform is not finite"), ({"t": d(0.0, 1.0, 0.0, nan)}, "transform is not finite"),
                  ({"t": d(0.0, 0.0, 0.0, -1.0)}, "a=0"), ({"t": d(0.0, 1.0, 0.0, 0.0)}, "e=0"), ({"t": d(0.0, -0.0, 0.0, 1.0)}, "a=-0"))
    cases = [(points, "dta_boundary_points", table + counts + (({"points": None}, "null"),)),
             (boxes, "dta_boundary_boxes", table + counts + transforms + (
                 ({"geo": p}, "exactly one of geo_boxes and pixel_boxes"), ({"pix": None}, "exactly one of geo_boxes and pixel_boxes"),
                 ({"t": None}, "pixel_boxes without a transform"), ({"geo": p, "pix": None}, "geo_boxes with a transform"))),
             (raster, "dta_boundary_raster", table + transforms + (
                 ({"t": None}, "null"), ({"height": 0}, "height=0"), ({"width": 0}, "width=0"), ({"height": -1}, "height=-1"),
                 ({"height": 65536, "width": 32768}, "int32"), ({"height": 2 ** 31 - 1, "width": 2}, "int32")))]
    for call, who, rows in cases:
        for kw, what in rows:
            assert call(**kw) != 0, (who, kw)
            assert err().startswith(who + ": ") and what in err(), (who, kw, err())


def test_python_route_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached.  Boundary.resident on a host tensor stands in for a
    resident table: the checks are the same, and a call that passes them is refused for want of a device."""
    import torch
    from deeptreeattention_amd import _lib, boundary as B

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        B.Boundary([SQUARE], device="cpu")
    table = B.edge_table([SQUARE])
    edges = torch.from_numpy(table.edges)
    for bad in ((table, edges.float()), (table, edges[:3]), (table, edges.t()), (table.edges, edges), (table, table.edges)):
        with pytest.raises(ValueError, match="resident"):
            B.Boundary.resident(*bad)
    site = B.Boundary.resident(table, edges)
    assert site.n_edges == 4 and site.table is table and site.org.tolist() == [0.0, 0.0]
    pts = f64([(1, 1), (2, 2), (5, 5)])
    for bad in (pts.astype(np.float32), pts[:, :1], pts[:0], pts.reshape(-1), torch.from_numpy(pts).float(),
                torch.zeros(3, 2, dtype=torch.float64, device="meta"), [[1, 2]]):
        with pytest.raises(ValueError, match="points"):
            site.contains(bad)
    geo = f64([(1, 1, 2, 2), (3, 3, 5, 5)])
    pix = np.array([(0, 0, 2, 2), (1, 1, 9, 9)], np.int32)
    t = (0.0, 1.0, 4.0, -1.0)
    for method in (site.boxes, site.clip):
        for bad in (geo.astype(np.float32), geo[:, :3], geo[:0], torch.from_numpy(geo).half(), pix):
            with pytest.raises(ValueError, match="geo_boxes"):
                method(geo_boxes=bad)
        for bad in (pix.astype(np.float64), pix[:, :2], pix[:0], torch.from_numpy(pix).double(), torch.from_numpy(pix) > 0,
                    np.array([(0, 0, 2 ** 31, 2)], np.int64), torch.zeros(2, 4, dtype=torch.int32, device="meta")):
            with pytest.raises(ValueError, match="pixel_boxes"):
                method(pixel_boxes=bad, transform=t)
        with pytest.raises(ValueError, match="exactly one"):
            method()
        with pytest.raises(ValueError, match="exactly one"):
            method(geo_boxes=geo, pixel_boxes=pix, transform=t)
        with pytest.raises(ValueError, match="need a transform"):
            method(pixel_boxes=pix)
        with pytest.raises(ValueError, match="no transform"):
            method(geo_boxes=geo, transform=t)
        for bad in ((0, 0, 4, -1), (0, 1, 4, 0), (0, 1, np.nan, -1), (0, 1, 4)):
            with pytest.raises(ValueError, match="transform"):
                method(pixel_boxes=pix, transform=bad)
    for h, w in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
        with pytest.raises(ValueError, match="height and width"):
            site.rasterise(h, w, t)
    with pytest.raises(ValueError, match="transform"):
        site.rasterise(4, 4, (0, 0, 4, -1))
    for call in (lambda: site.contains(pts), lambda: site.boxes(geo_boxes=geo), lambda: site.clip(pixel_boxes=pix, transform=t),
                 lambda: site.rasterise(4, 4, t)):
        with pytest.raises(RuntimeError, match="ROCm device only"):       # no fallback: a host table computes nothing
            call()
