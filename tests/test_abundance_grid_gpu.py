"""Abundance per tile and map cell on the device (dta_abundance_cells / _resample_grouped / _counts_grouped / _summary;
abundance.cells, the group= forms of abundance.resample / counts, abundance.summary_device) against the host definitions
(cells_np, resample_np / counts_np with group=, summary_np): every comparison is exact -- the counts are integers, a cell is
decided in float64 operation by operation, and the summary's one interpolation follows NumPy's."""
import os

import numpy as np
import pytest
import torch

import boundary_cases as BC
from test_abundance_cpu import random_confusion, random_crowns

pytestmark = pytest.mark.gpu

QS = (0, 0.025, 0.5, 0.975, 1)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def groups_of(rng, kind, N, G):
    """The cell of each crown.  Every kind but "own" and "one" has crowns outside [0, G): -1, G itself and far values, which
    sort in front of and behind the cells."""
    if kind == "own":                                       # every crown its own cell
        return rng.permutation(N).astype(np.int64)
    if kind == "one":
        return np.zeros(N, np.int64)
    if kind == "random":
        group = rng.integers(0, G, N).astype(np.int64)
    elif kind == "half":                                    # half the cells empty
        group = 2 * rng.integers(0, G // 2, N).astype(np.int64)
    elif kind == "skew":                                    # one cell holds all but ten crowns
        group = np.full(N, G // 2, np.int64)
        group[rng.choice(N, 10, replace=False)] = rng.integers(0, G, 10)
        return group
    out = rng.random(N) < 0.1
    group[out] = rng.choice(np.array([-1, G, G + 3, -2 ** 40, 2 ** 40], np.int64), int(out.sum()))
    return group


# (N, iterations, S, G): one crown; under a wave; five slices of 820 sorted positions with cells of about 800 crowns, so every
# slice boundary falls inside a cell and every cell but the last lies in two slices (runs through the LDS histogram); every
# crown its own cell (runs of one: the direct adds); 64 cells of which half are empty, about 30 crowns each (runs either
# side of the 32 at which a run goes through the histogram); one cell with all but ten crowns
CASES = [(1, 1, 1, 1, "one"), (65, 7, 2, 3, "random"), (4099, 33, 200, 5, "random"), (4099, 19, 6, 4099, "own"),
         (1000, 100, 256, 64, "half"), (5000, 9, 200, 4, "skew")]


@pytest.mark.parametrize("N,iterations,S,G,kind", CASES)
def test_grouped_resample_equals_the_definition(N, iterations, S, G, kind):
    from deeptreeattention_amd import abundance
    rng = np.random.default_rng(1000 * N + G)
    table = abundance.sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    mask = rng.random(N) < 0.7
    group = groups_of(rng, kind, N, G)
    if kind == "half":
        assert not (group[(group >= 0) & (group < G)] % 2).any()
    if kind == "skew":
        assert int((group == G // 2).sum()) >= N - 10
    dtable = abundance.device_table(table, dev())
    dl, ds, dm, dg = up(label), up(score), up(mask), up(group)
    zero = torch.zeros(N, dtype=torch.int64, device=dev())
    kw = dict(seed=7, first_iteration=3)
    for sc, dsc in ((score, ds), (None, None)):
        for m, dmm in ((None, None), (mask, dm)):
            want = abundance.resample_np(label, sc, table, iterations, mask=m, group=group, groups=G, **kw)
            got = abundance.resample(dl, dsc, dtable, iterations, mask=dmm, group=dg, groups=G, **kw)
            assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (iterations, G, S + 1)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (sc is None, m is None)
            # one cell that holds every crown is the ungrouped kernel's table, bit for bit
            plain = abundance.resample(dl, dsc, dtable, iterations, mask=dmm, **kw)
            one = abundance.resample(dl, dsc, dtable, iterations, mask=dmm, group=zero, groups=1, **kw)
            assert tuple(one.shape) == (iterations, 1, S + 1) and torch.equal(one[:, 0], plain), (sc is None, m is None)


def test_grouped_counts_are_overwritten_in_full_and_reruns_are_identical():
    from deeptreeattention_amd import abundance
    N, iterations, S, G = 4099, 33, 200, 37
    rng = np.random.default_rng(5)
    table = abundance.sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    mask = rng.random(N) < 0.7
    group = groups_of(rng, "half", N, G + 1)                 # odd cells empty: their planes have to come back as zeros
    dl, ds, dm, dg, dt = up(label), up(score), up(mask), up(group), abundance.device_table(table, dev())
    want = torch.from_numpy(abundance.resample_np(label, score, table, iterations, seed=5, mask=mask, group=group, groups=G))
    assert not want[:, 1::2].any() and want[:, 0::2].any()
    first = abundance.resample(dl, ds, dt, iterations, seed=5, mask=dm, group=dg, groups=G)
    buf = torch.full((iterations, G, S + 1), (1 << 40) + 12345, dtype=torch.int64, device=dev())
    assert abundance.resample(dl, ds, dt, iterations, seed=5, mask=dm, group=dg, groups=G, out=buf) is buf
    again = abundance.resample(dl, ds, dt, iterations, seed=5, mask=dm, group=dg, groups=G, out=buf)     # into its own result
    for got in (first, buf, again):
        assert torch.equal(got.cpu(), want)
    with pytest.raises(ValueError, match="out must be"):
        abundance.resample(dl, ds, dt, iterations, group=dg, groups=G, out=torch.empty(iterations, S + 1, dtype=torch.int64, device=dev()))
    assert tuple(abundance.resample(dl, ds, dt, 0, group=dg, groups=G).shape) == (0, G, S + 1)
    # one iteration per call is a plane of the longer run
    for k in (0, 8, 32):
        assert torch.equal(abundance.resample(dl, ds, dt, 1, seed=5, first_iteration=k, mask=dm, group=dg, groups=G)[0], first[k]), k


def test_grouped_counts_equal_the_definition():
    from deeptreeattention_amd import abundance
    for N, S, G, kind in ((1, 1, 1, "one"), (65, 6, 3, "random"), (4099, 200, 5, "random"), (1000, 256, 64, "half"), (4099, 6, 4099, "own")):
        rng = np.random.default_rng(31 + N + G)
        label, _ = random_crowns(rng, N, S)
        mask = rng.random(N) < 0.7
        group = groups_of(rng, kind, N, G)
        for m in (None, mask):
            got = abundance.counts(up(label), S, mask=up(m), group=up(group), groups=G)
            assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (G, S + 1)
            assert torch.equal(got.cpu(), torch.from_numpy(abundance.counts_np(label, S, m, group=group, groups=G))), (N, G, m is None)
        assert torch.equal(abundance.counts(up(label), S, mask=up(mask), group=up(group), groups=G).sum(0).cpu(),
                           torch.from_numpy(abundance.counts_np(label, S, mask & (group >= 0) & (group < G))))


def test_device_route_refuses_bad_tensors_before_any_launch(monkeypatch):
    from deeptreeattention_amd import _lib, abundance
    rng = np.random.default_rng(41)
    label, score = random_crowns(rng, 65, 6)
    dl, ds, dt = up(label), up(score), abundance.device_table(abundance.sampling_table(random_confusion(rng, 6)), dev())
    dg = torch.zeros(65, dtype=torch.int64, device=dev())
    table = torch.zeros(abundance.SUMMARY_MAX_ITERATIONS + 1, 7, dtype=torch.int64, device=dev())
    boxes = torch.zeros(5, 4, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_launch)
    for call in (lambda **kw: abundance.resample(dl, ds, dt, 3, **kw), lambda **kw: abundance.counts(dl, 6, **kw)):
        with pytest.raises(ValueError, match="group must be"):
            call(group=dg.to(torch.int32), groups=2)
        with pytest.raises(ValueError, match="group must be"):
            call(group=dg[:-1], groups=2)
        with pytest.raises(ValueError, match="group must be"):
            call(group=dg.cpu(), groups=2)
        with pytest.raises(ValueError, match="groups"):
            call(group=dg)
        with pytest.raises(ValueError, match="groups"):
            call(group=dg, groups=0)
        with pytest.raises(ValueError, match="groups without group"):
            call(groups=2)
    with pytest.raises(ValueError, match=r"abundance\.summary"):
        abundance.summary_device(table)                                        # above the cap: the host summary
    with pytest.raises(ValueError, match="counts must be"):
        abundance.summary_device(table[:4].double())
    with pytest.raises(ValueError, match="counts must be"):
        abundance.summary_device(table[:4, ::2])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        abundance.summary_device(table[:4], q=(1.5,))
    with pytest.raises(ValueError, match="boxes"):
        abundance.cells(boxes.float(), 2, 2)
    with pytest.raises(ValueError, match="boxes"):
        abundance.cells(boxes[:, :3], 2, 2)
    with pytest.raises(ValueError, match="integer"):
        abundance.cells(boxes, 2, 2, size=0.5)


# ---------------------------------------------------------------------------------------------------------------------
# which cell a crown is in
# ---------------------------------------------------------------------------------------------------------------------
def test_cells_equal_the_definition_on_the_reference_bounds_and_on_random_boxes(golden):
    from deeptreeattention_amd import abundance
    g = golden(os.path.join("abundance_grid", "geoindex_reference.npz"))
    b, grid = g["bounds"], g["grid"]
    db = up(b)
    seen_outside = False
    for k in range(len(grid)):
        ox, oy, cols, rows = (int(v) for v in grid[k])
        # every row against each block's grid (the other block's rows lie outside it), and against a smaller grid
        for args in ((cols, rows, (ox, oy), 1000), (cols - 7, rows - 3, (ox + 2000, oy + 1000), 1000), (7, 9, (ox + 500, oy - 250), 3000)):
            want = abundance.cells_np(b, *args)
            got = abundance.cells(db, *args)
            assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(want)), (k, args)
            seen_outside |= bool((want < 0).any()) and bool((want >= 0).any())
            want = abundance.cells_np(b, args[0], args[1], (args[2][0] + 0.25, args[2][1] - 0.125), 99.5, rule="centre")
            got = abundance.cells(db, args[0], args[1], (args[2][0] + 0.25, args[2][1] - 0.125), 99.5, rule="centre")
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (k, args)
    assert seen_outside
    # random boxes at UTM magnitudes, hectare cells whose size is no power of two, NaN / inf / far boxes in front
    rng = np.random.default_rng(3)
    n = 4099
    lo = np.stack([rng.uniform(4.0e5 - 300, 4.0e5 + 3300, n), rng.uniform(3.3e6 - 300, 3.3e6 + 3300, n)], axis=1)
    boxes = np.concatenate([lo, lo + rng.uniform(0.0, 25.0, (n, 2))], axis=1)
    boxes[:6] = [(np.nan, 3.3e6, 4.0e5, 3.3e6), (4.0e5, 3.3e6, np.inf, 3.3e6), (-np.inf, 3.3e6, np.inf, 3.3e6),
                 (2.0 ** 60, 3.3e6, 2.0 ** 60, 3.3e6), (4.0e5, -1e300, 4.0e5, 1e300), (1e308, 3.3e6, 1e308, 3.3e6)]
    boxes[6:40, 0] = boxes[6:40, 2] = 4.0e5 + 100.0 * np.arange(34)                          # centres exactly on cell lines
    for rule, origin, size, cols, rows in (("centre", (4.0e5, 3.3e6), 100.0, 30, 30), ("centre", (4.0e5 + 0.3, 3.3e6 - 0.7), 33.3, 97, 97),
                                           ("geoindex", (400000, 3300000), 100, 30, 30), ("geoindex", (399999, 3300001), 7, 450, 411)):
        want = abundance.cells_np(boxes, cols, rows, origin, size, rule=rule)
        assert (want[:6] == -1).all() and (want < 0).sum() > 100 and (want >= 0).sum() > 2000
        assert torch.equal(abundance.cells(up(boxes), cols, rows, origin, size, rule=rule).cpu(), torch.from_numpy(want)), (rule, size)
    assert torch.equal(abundance.cells(up(boxes[:1]), 2, 2).cpu(), torch.from_numpy(abundance.cells_np(boxes[:1], 2, 2)))


# ---------------------------------------------------------------------------------------------------------------------
# the summary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 7, 100, 256])
def test_summary_device_equals_summary_np(T):
    from deeptreeattention_amd import abundance
    from test_abundance_grid_cpu import tied_table
    assert 256 == abundance.SUMMARY_MAX_ITERATIONS
    rng = np.random.default_rng(T)
    # 201 and 5 x 37 = 185 entries: neither a multiple of the 64 entries of a workgroup; ungrouped and grouped
    for shape in ((201,), (5, 37)):
        c = tied_table(rng, T, shape)
        if T >= 7:
            c[:, ..., 1] = np.arange(T, 0, -1).reshape((T,) + (1,) * (len(shape) - 1))       # descending: the sort's longest walk
        want = abundance.summary_np(c, QS)
        got = abundance.summary_device(up(c), QS)
        assert got.q == QS and got.mean.dtype == torch.float64 and got.quantiles.dtype == torch.float64 and got.mean.is_cuda
        assert tuple(got.mean.shape) == shape and tuple(got.quantiles.shape) == (len(QS),) + shape
        assert torch.equal(got.mean.cpu(), torch.from_numpy(want.mean)), shape
        assert torch.equal(got.quantiles.cpu(), torch.from_numpy(want.quantiles)), shape
    other = (0.1, 0.3, 0.7, 0.9)
    assert torch.equal(abundance.summary_device(up(c), other).quantiles.cpu(), torch.from_numpy(abundance.summary_np(c, other).quantiles))
    assert tuple(abundance.summary_device(up(c), ()).quantiles.shape) == (0,) + shape


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_pixel_boxes_to_a_map_of_means_and_intervals():
    """Pixel boxes -> boundary.geo_boxes -> cells (hectare cells) -> resample(group=, mask=keep & inside) -> summary_device,
    against the same chain through the NumPy definitions."""
    from deeptreeattention_amd import abundance
    from deeptreeattention_amd import boundary as B
    rings, _, _ = BC.site(64, seed=64)
    site = B.Boundary(rings, device=dev())
    pix, transform = BC.pixel_boxes(rings, 1000, 264)
    N, S, iterations = len(pix), 23, 40
    rng = np.random.default_rng(9)
    table = abundance.sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    keep = rng.random(N) < 0.8                                       # e.g. the height filter's
    geo = B.geo_boxes(pix, transform)
    cols, rows, origin, size = 22, 21, (BC.UTM[0] + 400.0, BC.UTM[1] + 300.0), 100.0
    # the definitions
    cell = abundance.cells_np(geo, cols, rows, origin, size, rule="centre")
    inside = B.boxes_np(site, geo_boxes=geo) != 0
    assert (cell < 0).any() and len(set(cell[cell >= 0].tolist())) > 100 and 0 < (keep & inside).sum() < N
    want_table = abundance.resample_np(label, score, table, iterations, seed=2, mask=keep & inside, group=cell, groups=cols * rows)
    want = abundance.summary_np(want_table)
    # the device
    dcell = abundance.cells(up(geo), cols, rows, origin, size, rule="centre")
    dmask = site.clip(geo_boxes=up(geo)).bool() & up(keep)
    got_table = abundance.resample(up(label), up(score), abundance.device_table(table, dev()), iterations, seed=2, mask=dmask,
                                   group=dcell, groups=cols * rows)
    got = abundance.summary_device(got_table)
    assert torch.equal(dcell.cpu(), torch.from_numpy(cell))
    assert torch.equal(got_table.cpu(), torch.from_numpy(want_table))
    assert tuple(got.mean.shape) == (cols * rows, S + 1) and tuple(got.quantiles.shape) == (3, cols * rows, S + 1)
    assert torch.equal(got.mean.cpu(), torch.from_numpy(want.mean)) and torch.equal(got.quantiles.cpu(), torch.from_numpy(want.quantiles))
    assert abs(float(got.mean.sum()) - int((keep & inside & (cell >= 0)).sum())) < 1e-6
