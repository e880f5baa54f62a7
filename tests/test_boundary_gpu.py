"""Site boundary clip on the device (dta_boundary_points / _boxes / _raster, boundary.Boundary) against the host definition
(boundary.contains_np / boxes_np / rasterise_np): every comparison is exact equality of the uint8 results.  Boundaries are an
exterior star with a hole and an island at UTM magnitudes (tests/boundary_cases.py), with edge counts around the LDS chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_cases as BC

pytestmark = pytest.mark.gpu

CHUNK = 1024                     # boundary.EDGE_CHUNK (asserted below)
EDGES = (3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2500)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def same(got, want):
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    assert want.dtype == np.uint8
    return torch.equal(got.cpu(), torch.from_numpy(want))


_cases = {}


def case(n_edges):
    """One boundary per edge count, resident once, with 1000 points and 1000 pixel boxes and the mirror's answers."""
    from deeptreeattention_amd import boundary as B
    if n_edges not in _cases:
        assert B.EDGE_CHUNK == CHUNK
        rings, _, _ = BC.site(n_edges, seed=n_edges)
        site = B.Boundary(rings, device=dev())
        assert site.n_edges == n_edges and site.edges.dtype == torch.float64 and tuple(site.edges.shape) == (n_edges, 4)
        pts = BC.points(rings, 1000, 100 + n_edges)
        boxes, t = BC.pixel_boxes(rings, 1000, 200 + n_edges)
        _cases[n_edges] = dict(rings=rings, site=site, points=pts, inside=B.contains_np(site, pts), boxes=boxes, transform=t,
                               geo=B.geo_boxes(boxes, t), code=B.boxes_np(site, pixel_boxes=boxes, transform=t))
    return _cases[n_edges]


@pytest.mark.parametrize("n_edges", EDGES)
def test_points_equal_the_mirror(n_edges):
    c = case(n_edges)
    inside = c["inside"]
    assert 0 < inside.sum() < len(inside)
    assert inside[:40].any() or inside[40:80].any()            # queries on vertices and on edges, whichever way they fall
    x0, y0, x1, y1 = BC.extent(c["rings"])
    p = c["points"]
    with np.errstate(invalid="ignore"):
        outside_box = (p[:, 0] < x0) | (p[:, 0] > x1) | (p[:, 1] < y0) | (p[:, 1] > y1)
    assert outside_box.sum() > 50 and not inside[outside_box].any() and np.isnan(p).any()
    dp = torch.from_numpy(p).to(dev())
    for n in COUNTS:
        assert same(c["site"].contains(dp[:n]), inside[:n]), n
    assert same(c["site"].contains(p), inside)                 # a host array is uploaded
    assert same(c["site"].contains(dp[:257].cpu()), inside[:257])


@pytest.mark.parametrize("n_edges", EDGES)
def test_boxes_equal_the_mirror_in_both_forms(n_edges):
    from deeptreeattention_amd import boundary as B
    c = case(n_edges)
    code, site = c["code"], c["site"]
    assert set(code.tolist()) == {0, 1, 2}
    assert np.array_equal(B.boxes_np(site, geo_boxes=c["geo"]), code)
    dpix, dgeo = torch.from_numpy(c["boxes"]).to(dev()), torch.from_numpy(c["geo"]).to(dev())
    for n in COUNTS:
        assert same(site.boxes(pixel_boxes=dpix[:n], transform=c["transform"]), code[:n]), n
        assert same(site.boxes(geo_boxes=dgeo[:n]), code[:n]), n
    assert same(site.clip(pixel_boxes=c["boxes"], transform=c["transform"]), (code != 0).astype(np.uint8))
    assert same(site.clip(geo_boxes=c["geo"]), (code != 0).astype(np.uint8))
    assert same(site.boxes(pixel_boxes=dpix.long(), transform=c["transform"]), code)


def test_refused_and_touching_boxes_on_the_device():
    from deeptreeattention_amd import boundary as B
    nan, inf = np.nan, np.inf
    square = np.array([(0, 0), (4, 0), (4, 4), (0, 4)], np.float64) + np.array(BC.UTM)
    boxes = np.array([(4, 1, 5, 2), (4, 4, 5, 5), (-1, -1, 0, 0), (2, 2, 2, 2), (4, 2, 4, 2), (1, 2, 3, 2), (5, 5, 5, 5),
                      (2, -1, 2, 5), (4.5, 1, 5, 2), (0, 0, 4, 4), (0.5, 0.5, 3.5, 3.5), (-9, 1, -8, 2), (1, 8, 2, 9), (1, -9, 2, -8),
                      (nan, 1, 2, 2), (1, nan, 2, 2), (1, 1, nan, 2), (1, 1, 2, nan), (inf, 1, 2, 2), (1, 1, inf, 2),
                      (-inf, 1, 2, 2), (1, -inf, 2, inf), (3, 1, 1, 2), (1, 3, 2, 1)], np.float64) + np.array(BC.UTM * 2)
    want = B.boxes_np([square], geo_boxes=boxes)
    assert want.tolist() == [1, 1, 1, 2, 1, 2, 0, 1, 0, 1, 2, 0, 0, 0] + [0] * 10
    assert same(B.Boundary([square], device=dev()).boxes(geo_boxes=boxes), want)
    pts = np.array([(0, 2), (2, 0), (4, 2), (2, 4), (2, 2), (nan, 2), (2, nan), (inf, 2), (-inf, 2)], np.float64) + np.array(BC.UTM)
    assert B.contains_np([square], pts).tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 0]
    assert same(B.Boundary([square], device=dev()).contains(pts), B.contains_np([square], pts))


@pytest.mark.parametrize("n_edges", (4, CHUNK + 1))
def test_every_output_byte_is_written_and_none_beyond(n_edges):
    """Through the C entries with buffers of this test's own: 0xFF everywhere first, n results after, 0xFF still behind them."""
    from deeptreeattention_amd import _lib
    c = case(n_edges)
    site, L = c["site"], _lib.lib()
    org = (C.c_double * 2)(*site.org)
    t = (C.c_double * 4)(*c["transform"])
    stream = _lib.current_stream_ptr()
    dp = torch.from_numpy(c["points"]).to(dev())
    dpix, dgeo = torch.from_numpy(c["boxes"]).to(dev()), torch.from_numpy(c["geo"]).to(dev())
    for n in (1, 65, 257, 1000):
        out = torch.full((3, n + 300), 0xFF, dtype=torch.uint8, device=dev())
        _lib.check(L.dta_boundary_points(_lib.ptr(site.edges), n_edges, org, _lib.ptr(dp), n, _lib.ptr(out[0]), stream), "points")
        _lib.check(L.dta_boundary_boxes(_lib.ptr(site.edges), n_edges, org, None, _lib.ptr(dpix), t, n, _lib.ptr(out[1]), stream), "boxes")
        _lib.check(L.dta_boundary_boxes(_lib.ptr(site.edges), n_edges, org, _lib.ptr(dgeo), None, None, n, _lib.ptr(out[2]), stream), "boxes")
        got = out.cpu().numpy()
        assert np.array_equal(got[0, :n], c["inside"][:n]) and np.array_equal(got[1, :n], c["code"][:n])
        assert np.array_equal(got[2, :n], c["code"][:n]) and (got[:, n:] == 0xFF).all()
    H, W = 5, 67
    rt = raster_transform(c["rings"], H, W)
    out = torch.full((H * W + 300,), 0xFF, dtype=torch.uint8, device=dev())
    _lib.check(L.dta_boundary_raster(_lib.ptr(site.edges), n_edges, org, H, W, (C.c_double * 4)(*rt), _lib.ptr(out), stream), "raster")
    from deeptreeattention_amd import boundary as B
    got = out.cpu().numpy()
    assert np.array_equal(got[:H * W].reshape(H, W), B.rasterise_np(site, H, W, rt)) and (got[H * W:] == 0xFF).all()


def test_shuffled_queries_give_the_shuffled_result():
    c = case(2500)
    perm = np.random.default_rng(7).permutation(1000)
    assert same(c["site"].contains(np.ascontiguousarray(c["points"][perm])), c["inside"][perm])
    assert same(c["site"].boxes(pixel_boxes=np.ascontiguousarray(c["boxes"][perm]), transform=c["transform"]), c["code"][perm])
    assert same(c["site"].boxes(geo_boxes=np.ascontiguousarray(c["geo"][perm])), c["code"][perm])


# ---------------------------------------------------------------------------------------------------------------------
# the raster
# ---------------------------------------------------------------------------------------------------------------------
def raster_transform(rings, H, W, margin=0.15):
    """A grid of H x W cells over the boundary's bounding box and a margin, north-up."""
    x0, y0, x1, y1 = BC.extent(rings)
    w, h = x1 - x0, y1 - y0
    return (x0 - margin * w, (1 + 2 * margin) * w / W, y1 + margin * h, -(1 + 2 * margin) * h / H)


def through_a_vertex(rings, H, W, row):
    """A grid whose row `row` has its centre line exactly through the exterior's first vertex and whose cells are 2^k
    metres: (row + .5) * e + y0 == the vertex's y without rounding."""
    x0, _, x1, _ = BC.extent(rings)
    vy = float(np.floor(rings[0][0, 1]))
    e = -64.0
    return (float(np.floor(x0)) - 32.0, float(2 ** np.ceil(np.log2((x1 - x0 + 64.0) / W))), vy - (row + 0.5) * e, e), vy


@pytest.mark.parametrize("H", (1, 3, 37))
def test_raster_equals_the_mirror(H):
    from deeptreeattention_amd import boundary as B
    for n_edges in (4, 2500):
        c = case(n_edges)
        site, rings = c["site"], c["rings"]
        _, y0, _, y1 = BC.extent(rings)
        for W in (1, 63, 64, 65, 130):
            t = raster_transform(rings, H, W)
            want = B.rasterise_np(site, H, W, t)
            assert same(site.rasterise(H, W, t), want), (n_edges, W)
            if H * W >= 37 * 63:
                assert 0 < want.sum() < want.size
            # rows that no edge straddles: the grid moved up until its first row lies above the boundary
            above = (t[0], t[1], y1 + 10.0 - 1.5 * t[3], t[3])       # e < 0: row 0's centre line is 10 m + a cell above
            want = B.rasterise_np(site, H, W, above)
            assert not want[0].any() and same(site.rasterise(H, W, above), want), (n_edges, W)


@pytest.mark.parametrize("H", (1, 3, 37))
def test_raster_row_through_a_vertex(H):
    """The boundary's first vertex moved to whole metres; a row's centre line passes through it exactly."""
    from deeptreeattention_amd import boundary as B
    rings, _, _ = BC.site(300, seed=5)
    rings = [r.copy() for r in rings]
    rings[0][0] = np.floor(rings[0][0])
    site = B.Boundary(rings, device=dev())
    for W in (1, 63, 64, 65, 130):
        t, vy = through_a_vertex(rings, H, W, H // 2)
        centres = B.cell_centres(H, W, t).reshape(H, W, 2)
        assert (centres[H // 2, :, 1] == vy).all() and vy == rings[0][0, 1]
        want = B.rasterise_np(site, H, W, t)
        assert same(site.rasterise(H, W, t), want), W
    assert want[H // 2].any()


def test_raster_wider_than_one_workgroup_and_more_edges_than_one_chunk():
    """A workgroup takes 1024 columns of a row and compacts 1024 edges at a time: widths and edge counts on both sides."""
    from deeptreeattention_amd import boundary as B
    for n_edges in (CHUNK - 1, CHUNK, CHUNK + 1, 2500):
        c = case(n_edges)
        for H, W in ((2, 1023), (2, 1024), (3, 1025), (2, 2049)):
            t = raster_transform(c["rings"], H, W, margin=0.02)
            want = B.rasterise_np(c["site"], H, W, t)
            assert 0 < want.sum() < want.size
            assert same(c["site"].rasterise(H, W, t), want), (n_edges, H, W)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_feeds_abundance_counts():
    """pixel boxes -> clip -> abundance.counts(label, S, mask=keep & inside) equals counts_np with the mirror's mask."""
    from deeptreeattention_amd import abundance
    c = case(2500)
    rng = np.random.default_rng(9)
    S, n = 11, 1000
    label = rng.integers(0, S, n)
    keep = rng.random(n) < 0.7
    inside = c["site"].clip(pixel_boxes=torch.from_numpy(c["boxes"]).to(dev()), transform=c["transform"])
    mask = torch.from_numpy(keep).to(dev()) & inside
    assert mask.dtype in (torch.bool, torch.uint8)
    got = abundance.counts(torch.from_numpy(label).to(dev()), S, mask=mask)
    want = abundance.counts_np(label, S, mask=keep & (c["code"] != 0))
    assert np.array_equal(got.cpu().numpy(), want)
    assert 0 < int(np.asarray(want).sum()) < int(keep.sum())   # the boundary took some crowns away


def test_rasterise_blanks_a_label_map():
    """rasterise applied to a predict_map-shaped label array ([H][W] int64, -1 where nothing was predicted)."""
    from deeptreeattention_amd import boundary as B
    c = case(CHUNK)
    H, W = 45, 70
    t = raster_transform(c["rings"], H, W)
    label = np.random.default_rng(10).integers(-1, 9, (H, W))
    site_mask = c["site"].rasterise(H, W, t)
    got = torch.where(site_mask.bool(), torch.from_numpy(label).to(dev()), torch.full((), -1, dtype=torch.int64, device=dev()))
    want = np.where(B.rasterise_np(c["site"], H, W, t) != 0, label, -1)
    assert np.array_equal(got.cpu().numpy(), want) and (want != label).any() and (want >= 0).any()
    assert int(site_mask.sum()) == int(B.rasterise_np(c["site"], H, W, t).sum())      # counting cells
