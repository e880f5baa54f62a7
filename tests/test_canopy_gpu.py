"""Crown height filter on the device (dta_crown_height, canopy.CanopyRaster.crown_height) against the host definition
(canopy.crown_height_np / min_height_np / height_rules_np) and the reference-made fixture: every comparison is exact -- the
float32 heights bit for bit (viewed as int32; any NaN is the one NaN the route writes), the counts and the keep mask."""
import os

import numpy as np
import pytest
import torch

from test_canopy_cpu import NODATA, random_boxes, special_raster

pytestmark = pytest.mark.gpu

QS = (0, 50, 99, 100)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def canon(height):
    """float32 heights as int32 bit patterns, every NaN as the same pattern."""
    h = torch.as_tensor(height).cpu()
    assert h.dtype == torch.float32
    return torch.where(torch.isnan(h), torch.full_like(h, float("nan")), h).view(torch.int32)


def same(got, chm, boxes, q=99.0, floor=0.5, field=None, rule=None):
    """got: CrownHeights of the device; equals the mirror exactly.  Returns the mirror's (height, count, keep)."""
    from deeptreeattention_amd import canopy
    height, count = canopy.crown_height_np(chm, boxes, q=q, floor=floor)
    assert got.height.dtype == torch.float32 and got.count.dtype == torch.int32 and got.height.is_cuda and got.count.is_cuda
    assert tuple(got.height.shape) == tuple(got.count.shape) == (len(boxes),)
    assert torch.equal(got.count.cpu(), torch.from_numpy(count)), "count"
    assert torch.equal(canon(got.height), canon(torch.from_numpy(height))), "height"
    keep = None
    if rule is None:
        assert got.keep is None
    else:
        keep = (canopy.min_height_np(height, rule.m) if isinstance(rule, canopy.MinHeight)
                else canopy.height_rules_np(height, field, *rule))
        assert got.keep.dtype == torch.bool and got.keep.is_cuda and tuple(got.keep.shape) == (len(boxes),)
        assert torch.equal(got.keep.cpu(), torch.from_numpy(keep)), "keep"
    return height, count, keep


@pytest.fixture(scope="module")
def small():
    """A 37 x 53 raster with NaN / nodata / sub-floor cells and a tie quarter, resident once for the module."""
    from deeptreeattention_amd.canopy import CanopyRaster
    chm = special_raster(np.random.default_rng(1), 37, 53)
    return chm, CanopyRaster(chm, device=dev())


@pytest.fixture(scope="module")
def large():
    """A 300 x 300 raster: NaN / nodata / sub-floor cells everywhere, the top-left quarter heights of 27-30 m rounded to
    0.1 m (31 distinct values: the lo-th and hi-th values of a big box there are equal), the rest 0.5-35 m."""
    from deeptreeattention_amd.canopy import CanopyRaster
    rng = np.random.default_rng(2)
    chm = special_raster(rng, 300, 300, ties=False)
    quarter = chm[:150, :150]
    with np.errstate(invalid="ignore"):
        live = quarter >= 0.5
    quarter[live] = np.round(rng.uniform(27.0, 30.0, int(live.sum())), 1).astype(np.float32)
    return chm, CanopyRaster(chm, device=dev())


def test_fixture_raster_and_boxes(golden):
    from deeptreeattention_amd.canopy import CanopyRaster
    g = golden(os.path.join("canopy", "canopy_reference.npz"))
    chm, boxes = g["chm"], g["boxes"]
    got = CanopyRaster(chm, device=dev()).crown_height(boxes)
    height, count, _ = same(got, chm, boxes)
    assert torch.equal(canon(got.height), canon(torch.from_numpy(g["ref_q99"])))        # the reference's own answer
    assert torch.equal(got.count.cpu(), torch.from_numpy(g["kept"]))
    # the recorded rule rows: the device applies the rule to ITS height, so hand it the recorded heights through a raster of
    # single cells (a one-cell box of a cell >= floor has that cell as its height; the recorded heights go down to 0.26)
    ch, fh = g["chm_height"], g["field_height"]
    cells = np.where(np.isnan(ch), NODATA, ch).astype(np.float32).reshape(1, -1)
    assert (cells[0][~np.isnan(ch)] >= 0.01).all()
    one = np.array([(0, k, 1, k + 1) for k in range(len(ch))], np.int32)
    from deeptreeattention_amd import canopy
    ras = CanopyRaster(cells, device=dev())
    for rule, want in ((canopy.HeightRules(), g["ref_keep_default"]), (canopy.HeightRules(*g["other"]), g["ref_keep_other"])):
        got = ras.crown_height(one, floor=0.01, field_height=fh, rule=rule)
        assert torch.equal(canon(got.height), canon(torch.from_numpy(ch)))
        assert torch.equal(got.keep.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_random_crowns_on_a_small_raster(small, N, q):
    """Boxes of up to 45 x 45 cells around a 37 x 53 raster: inside, over every edge, wholly outside; clipped areas on both
    sides of the wave path's limit (N = 1000)."""
    from deeptreeattention_amd import canopy
    chm, ras = small
    boxes = random_boxes(np.random.default_rng(10 * N + q), N, 37, 53, max_side=45, margin=6)
    height, count, _ = same(ras.crown_height(boxes, q=q), chm, boxes, q=q)
    if N == 1000:
        _, _, rows, cols = canopy.clip_boxes(boxes, 37, 53)
        area = rows * cols
        assert (area == 0).any() and (area > canopy.WAVE_CELLS).any() and ((area > 0) & (area <= canopy.WAVE_CELLS)).any()
        assert (count == 0).any() and (count == 1).any()
        # another floor: other cells are kept
        same(ras.crown_height(boxes, q=q, floor=20.0), chm, boxes, q=q, floor=20.0)
        # a device tensor of boxes is taken as it is
        same(ras.crown_height(torch.from_numpy(boxes).to(dev()), q=q), chm, boxes, q=q)


@pytest.mark.parametrize("N", [2048, 2049, 4173])
def test_more_crowns_than_the_block_kernel_has_workgroups(large, N):
    """Up to canopy.BLOCK_GROUPS crowns the block kernel has a workgroup per crown, above that a workgroup looks at a chunk
    of consecutive crowns (2 from 2049 on, 3 at 4173 with a short last chunk) and works through the large ones among them:
    a quarter of these boxes is over the wave limit, so chunks with none, one and several of them occur."""
    from deeptreeattention_amd import canopy
    assert canopy.BLOCK_GROUPS == 2048
    chm, ras = large
    boxes = random_boxes(np.random.default_rng(N), N, 300, 300, max_side=45, margin=6)
    _, _, rows, cols = canopy.clip_boxes(boxes, 300, 300)
    big = rows * cols > canopy.WAVE_CELLS
    assert 0.1 < big.mean() < 0.5 and (big[:-1] & big[1:]).any() and (~big[:-1] & ~big[1:]).any()
    rule = canopy.MinHeight(33.0)
    _, _, keep = same(ras.crown_height(boxes, rule=rule), chm, boxes, rule=rule)
    assert keep.any() and not keep.all()


def area_boxes():
    """Clipped areas 1, 2, 3, 63, 64, 65, the wave path's limit and one cell either side, in several shapes (narrower and
    wider than a wave's 64 lanes and a workgroup's 256 threads), and the whole 300 x 300 raster."""
    from deeptreeattention_amd.canopy import WAVE_CELLS
    assert WAVE_CELLS == 1024, "the shapes below are written for a limit of 1024 cells"
    shapes = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (7, 9), (9, 7), (1, 63), (8, 8), (1, 64), (64, 1), (5, 13), (13, 5), (1, 65),
              (31, 33), (33, 31), (11, 93), (93, 11), (3, 300),                       # 1023 (three ways), 900 in rows of 300
              (32, 32), (4, 256), (256, 4), (16, 64), (8, 128),                      # 1024
              (25, 41), (41, 25), (5, 205), (205, 5),                                # 1025
              (4, 257), (257, 4), (100, 100), (10, 300), (300, 10), (300, 300)]
    boxes = []
    for k, (h, w) in enumerate(shapes):
        for r0, c0 in ((0, 0), (300 - h, 300 - w), ((37 * k) % (301 - h), (91 * k) % (301 - w))):
            boxes.append((r0, c0, r0 + h, c0 + w))
    return np.array(boxes, np.int32)


@pytest.mark.parametrize("q", QS)
def test_box_areas_around_the_wave_limit(large, q):
    from deeptreeattention_amd import canopy
    chm, ras = large
    boxes = area_boxes()
    _, _, rows, cols = canopy.clip_boxes(boxes, 300, 300)
    assert {1, 2, 3, 63, 64, 65, canopy.WAVE_CELLS - 1, canopy.WAVE_CELLS, canopy.WAVE_CELLS + 1, 90000} <= set((rows * cols).tolist())
    height, count, _ = same(ras.crown_height(boxes, q=q), chm, boxes, q=q)
    assert count.max() > 70000


def tiles_with_kept_counts(side, counts, seed):
    """A raster of side x side tiles, tile k with exactly counts[k] cells >= 0.5 (heights of 5-6 m rounded to 0.1: ties) among
    NaN, nodata and sub-floor cells; one box per tile."""
    rng = np.random.default_rng(seed)
    per_row = 3
    rows = -(-len(counts) // per_row)
    fill = np.array([np.nan, NODATA, 0.25, 0.0, -0.0, 0.49999997, -np.inf], np.float32)
    chm = fill[rng.integers(0, len(fill), (rows * side, per_row * side))]
    boxes = []
    for k, n in enumerate(counts):
        r0, c0 = (k // per_row) * side, (k % per_row) * side
        cells = rng.choice(side * side, n, replace=False)
        chm[r0 + cells // side, c0 + cells % side] = np.round(rng.uniform(5.0, 6.0, n), 1).astype(np.float32)
        boxes.append((r0, c0, r0 + side, c0 + side))
    return chm, np.array(boxes, np.int32)


@pytest.mark.parametrize("side", [12, 40])           # 144 cells: a wave's crown; 1600 cells: a workgroup's
def test_kept_counts(side):
    from deeptreeattention_amd import canopy
    assert side * side <= canopy.WAVE_CELLS or side == 40
    wanted = [0, 1, 2, 3, 100, 101, 102, 144]
    chm, boxes = tiles_with_kept_counts(side, wanted, 3 + side)
    ras = canopy.CanopyRaster(chm, device=dev())
    for q in QS:
        height, count, _ = same(ras.crown_height(boxes, q=q), chm, boxes, q=q)
        assert count.tolist() == wanted
    # +inf is kept and takes part in the arithmetic as it does in NumPy
    chm[0, 0] = chm[side, side] = np.inf
    same(canopy.CanopyRaster(chm, device=dev()).crown_height(boxes, q=100), chm, boxes, q=100)
    same(canopy.CanopyRaster(chm, device=dev()).crown_height(boxes, q=99), chm, boxes, q=99)


def test_tall_boxes_of_one_and_two_columns():
    """A box of more cells than the wave limit that is one or two cells wide: whole rows per step of the workgroup."""
    from deeptreeattention_amd import canopy
    chm = special_raster(np.random.default_rng(4), 1100, 3, ties=False)
    boxes = np.array([(0, 0, 1100, 1), (0, 1, 1100, 3), (0, 0, 1100, 3), (10, 2, 1060, 3), (-5, -5, 2000, 2)], np.int32)
    ras = canopy.CanopyRaster(chm, device=dev())
    for q in QS:
        same(ras.crown_height(boxes, q=q), chm, boxes, q=q)


def test_shuffled_crowns_give_the_shuffled_result(large):
    chm, ras = large
    rng = np.random.default_rng(5)
    boxes = np.concatenate([area_boxes(), random_boxes(rng, 500, 300, 300, max_side=30, margin=5)])
    a = ras.crown_height(boxes)
    perm = rng.permutation(len(boxes))
    b = ras.crown_height(boxes[perm])
    p = torch.from_numpy(perm).to(dev())
    assert torch.equal(canon(b.height), canon(a.height[p])) and torch.equal(b.count, a.count[p])
    # and again: nothing depends on what ran before
    c = ras.crown_height(boxes)
    assert torch.equal(canon(c.height), canon(a.height)) and torch.equal(c.count, a.count)


def rule_case(large):
    from deeptreeattention_amd import canopy
    chm, ras = large
    rng = np.random.default_rng(6)
    boxes = np.concatenate([area_boxes()[::3], random_boxes(rng, 400, 300, 300, max_side=20, margin=8)])
    height, count = canopy.crown_height_np(chm, boxes)
    h64 = height.astype(np.float64)
    field = h64 + rng.uniform(-12.0, 8.0, len(boxes))
    field[::5] = np.nan
    live = np.flatnonzero(count > 0)
    for k, d in enumerate((0.0, 4.0, -4.0, 8.0, -8.0, np.nextafter(4.0, 0.0), np.nextafter(8.0, 9.0))):
        field[live[3 * k]] = h64[live[3 * k]] - d        # equal heights; differences of exactly max_diff and limit; next to them
    assert (count == 0).any() and np.isnan(height).any()
    return chm, ras, boxes, field


def test_rules(large):
    from deeptreeattention_amd import canopy
    chm, ras, boxes, field = rule_case(large)
    _, _, keep = same(ras.crown_height(boxes, rule=canopy.MinHeight(3.0)), chm, boxes, rule=canopy.MinHeight(3.0))
    assert keep.any() and not keep.all()
    _, _, keep = same(ras.crown_height(boxes, rule=canopy.MinHeight(29.5)), chm, boxes, rule=canopy.MinHeight(29.5))
    assert keep.any() and not keep.all()
    rule = canopy.HeightRules()
    for f in (field, torch.from_numpy(field).to(dev()), field.astype(np.float32), torch.from_numpy(field.astype(np.float32)).to(dev()),
              torch.from_numpy(field)):
        f_host = f.cpu().numpy() if isinstance(f, torch.Tensor) else f
        _, _, keep = same(ras.crown_height(boxes, field_height=f, rule=rule), chm, boxes, field=f_host, rule=rule)
        assert keep.any() and not keep.all()
    other = canopy.HeightRules(20.0, 2.5, 5.0)
    same(ras.crown_height(boxes, field_height=field, rule=other), chm, boxes, field=field, rule=other)
    assert ras.crown_height(boxes).keep is None
    assert ras.crown_height(boxes, field_height=field).keep is None        # a field height without a rule decides nothing


def test_outputs_are_overwritten_in_full(large):
    """Through the C entry, so that the buffers are the test's: every element of height, count and keep is written for
    every crown (wholly outside, degenerate, a wave's, a workgroup's), and nothing next to them."""
    from deeptreeattention_amd import _lib, canopy
    chm, ras, boxes, field = rule_case(large)
    n = len(boxes)
    L = _lib.lib()
    dboxes = torch.from_numpy(boxes).to(dev())
    dfield = torch.from_numpy(field).to(dev())
    height, count = canopy.crown_height_np(chm, boxes)
    for mode, rule, want in ((0, None, None), (1, _lib.HeightRule(1, 3.0, 0, 0, 0), canopy.min_height_np(height, 3.0)),
                             (2, _lib.HeightRule(2, 0, 1.0, 4.0, 8.0), canopy.height_rules_np(height, field))):
        oh = torch.full((n + 2,), 12345.0, dtype=torch.float32, device=dev())
        oc = torch.full((n + 2,), -7, dtype=torch.int32, device=dev())
        ok = torch.full((n + 2,), 0xA5, dtype=torch.uint8, device=dev())
        _lib.check(L.dta_crown_height(_lib.ptr(ras.data), 300, 300, _lib.ptr(dboxes), n, 99.0, 0.5,
                                      _lib.ptr(dfield) if mode == 2 else None, _lib.C.byref(rule) if mode else None,
                                      _lib.C.c_void_p(oh.data_ptr() + 4), _lib.C.c_void_p(oc.data_ptr() + 4),
                                      _lib.C.c_void_p(ok.data_ptr() + 1) if mode else None, _lib.current_stream_ptr()),
                   "dta_crown_height")
        assert torch.equal(canon(oh[1:-1]), canon(torch.from_numpy(height))) and oh[0] == 12345.0 and oh[-1] == 12345.0
        assert torch.equal(oc[1:-1].cpu(), torch.from_numpy(count)) and oc[0] == -7 and oc[-1] == -7
        if mode:
            assert torch.equal(ok[1:-1].cpu(), torch.from_numpy(want.astype(np.uint8))) and ok[0] == 0xA5 and ok[-1] == 0xA5
        else:
            assert bool((ok == 0xA5).all())


def test_the_cell_limit_is_decided_on_the_device_for_device_boxes():
    """A clipped box of 2^24 cells is computed (the index arithmetic of the last rows of a 4097-wide raster included), one of
    more is refused: count -1, NaN, keep False.  Host boxes are refused by the Python route before the library."""
    from deeptreeattention_amd import canopy
    rng = np.random.default_rng(7)
    chm = rng.random((4097, 4097), dtype=np.float32) * np.float32(40.0)
    ras = canopy.CanopyRaster(chm, device=dev())
    boxes = np.array([(0, 0, 4097, 4097), (1, 1, 4097, 4097), (-9, -9, 9999, 4096), (4090, 4090, 4097, 4097)], np.int32)
    with pytest.raises(ValueError, match="2\\^24"):
        ras.crown_height(boxes)
    got = ras.crown_height(torch.from_numpy(boxes).to(dev()), rule=canopy.MinHeight(3.0))
    assert got.count.tolist()[0] == -1 and got.count.tolist()[2] == -1
    assert bool(torch.isnan(got.height[0])) and bool(torch.isnan(got.height[2])) and got.keep.tolist() == [False, True, False, True]
    height, count = canopy.crown_height_np(chm, boxes[[1, 3]])
    assert torch.equal(got.count[[1, 3]].cpu(), torch.from_numpy(count)) and count[0] > 16000000
    assert torch.equal(canon(got.height[[1, 3]]), canon(torch.from_numpy(height)))


def test_end_to_end_from_crown_boxes_to_counts_of_the_kept_crowns():
    """CanopyRaster.crown_height(boxes, rule=MinHeight(3)) in front of dense.predict_crops_multistage: predicting boxes[keep]
    and predicting every box and counting with mask=keep give the same trees per species, keep.sum() trees in all."""
    from deeptreeattention_amd import abundance, canopy
    from deeptreeattention_amd.dense import predict_crops_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    from test_dense_crops_gpu import route_boxes
    from test_dense_multistage_cpu import three_level_hierarchy
    from test_dense_multistage_gpu import BANDS, H, W, dense_years, year_rasters
    from test_multistage_ensemble_gpu import _small_levels
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)          # (the predictor holds its models weakly)
    pred = MultiStagePredictor(models, hierarchy=h)
    ras = dense_years(year_rasters())
    boxes = route_boxes()
    n, S = len(boxes), h.n_species
    # a canopy of the hyperspectral rasters' height x width: low on the left (everything under 3 m), tall on the right
    rng = np.random.default_rng(8)
    chm = rng.uniform(0.0, 2.9, (H, W)).astype(np.float32)
    chm[:, W // 2:] = rng.uniform(0.0, 25.0, (H, W - W // 2)).astype(np.float32)
    chm[rng.random((H, W)) < 0.05] = NODATA
    got = canopy.CanopyRaster(chm, device=dev()).crown_height(boxes, rule=canopy.MinHeight(3.0))
    same(got, chm, boxes, rule=canopy.MinHeight(3.0))
    keep = got.keep
    kept = int(keep.sum())
    assert 0 < kept < n
    some = predict_crops_multistage(pred, ras, torch.from_numpy(boxes).to(dev())[keep], batch_size=16)
    every = predict_crops_multistage(pred, ras, boxes, batch_size=16)
    assert some.ens_label.shape == (kept,) and every.ens_label.shape == (n,)
    one = abundance.counts(some.ens_label, S)
    two = abundance.counts(every.ens_label, S, mask=keep)
    assert torch.equal(one, two) and int(one.sum()) == kept
