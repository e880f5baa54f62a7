"""Crops of crown boxes out of a resident raster on the device (dta_gather_crops / _tiles / _years, DenseRaster.crops /
crops_years, dense.predict_crops*): against the reference's own crops (tests/golden/preprocess.npz), against the host
definition (dense.gather_crops_np), and against what the package could already do -- the crop preprocessing kernel
(preprocess.preprocess_batch) on host-sliced raw crops, fed to the predictors in the same batches.
Every float comparison is on bits: both sides select the same float32 values and run the same launches on them."""
import numpy as np
import pytest
import torch

from oracle import preprocess_np as PP
from test_dense_crops_cpu import load_golden, mosaic
from test_dense_gpu import assert_same_bits, make, raw_raster
from test_dense_multistage_cpu import three_level_hierarchy
from test_dense_multistage_gpu import BANDS, H, RAW_BANDS, W, dense_years, year_rasters
from test_multistage_ensemble_gpu import _small_levels

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# One batch on the 17 x 13 raster: 1x1, 3x7, 11x11, the whole raster (downsampling), a box on each edge, and a degenerate
# box in the middle of the batch.  9 x 23 x 121 floats: lanes straddle crops with different boxes, and the last lane is short.
MIXED = np.array([(5, 6, 6, 7), (2, 3, 5, 10), (3, 1, 14, 12), (0, 0, H, W), (7, 7, 7, 9),
                  (0, 4, 4, 9), (13, 2, H, 8), (6, 0, 12, 3), (4, 9, 10, W)], dtype=np.int32)
DEGENERATE = 4


def host_sliced(raw, boxes):
    """What the reference's patches.crop reads for each box: the intersection with the raster; None where there is none."""
    Hh, Ww = raw.shape[1:]
    out = []
    for r0, c0, r1, c1 in np.asarray(boxes):
        r0, c0, r1, c1 = max(int(r0), 0), max(int(c0), 0), min(int(r1), Hh), min(int(c1), Ww)
        out.append(np.ascontiguousarray(raw[:, r0:r1, c0:c1]) if r1 > r0 and c1 > c0 else None)
    return out


def route_boxes(n=36, seed=9):
    """n boxes on the 17 x 13 raster with sides 1..17 / 1..13, the first ones hanging over its edges (clipped by the route)."""
    rng = np.random.default_rng(seed)
    boxes = [(-3, -2, 5, 6), (10, 8, 25, 20), (-4, 3, 30, 9), (6, -5, 9, 40)]
    while len(boxes) < n:
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        r0, c0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        boxes.append((r0, c0, r0 + h, c0 + w))
    return np.array(boxes, dtype=np.int32)


BATCHES = (12, 16)      # 36 boxes: three full batches, and two full ones with a rest of four


# ---------------------------------------------------------------------------------------------------------------------
# the gathers
# ---------------------------------------------------------------------------------------------------------------------
def test_mosaic_crops_equal_the_reference_golden():
    from deeptreeattention_amd.dense import DenseRaster, gather_crops_np
    g = load_golden()
    raw, boxes, names = mosaic(g)
    ras = DenseRaster(raw, precision="fp32", device=dev())
    got = ras.crops(boxes).cpu().numpy()
    assert got.shape == (5, 349, 11, 11) and got.size % 4 != 0          # the tail store is exercised
    want = np.stack([g[f"{n}/resized11"] for n in names])
    assert np.array_equal(bits(got), bits(want))
    whole = PP.preprocess_image(raw)
    assert np.array_equal(bits(got), bits(gather_crops_np(whole, boxes, 11)))
    got24 = ras.crops(boxes[:1], size=24).cpu().numpy()
    assert np.array_equal(bits(got24[0]), bits(g[f"{names[0]}/resized24"]))
    assert np.array_equal(bits(ras.crops(boxes, size=24).cpu().numpy()), bits(gather_crops_np(whole, boxes, 24)))


def test_mixed_boxes_equal_host_definition_and_crop_preprocessing():
    from deeptreeattention_amd.dense import DenseRaster, gather_crops_np
    from deeptreeattention_amd.preprocess import preprocess_batch
    raw = year_rasters()[0]
    assert raw.shape == (RAW_BANDS, H, W) and (len(MIXED) * BANDS * 121) % 4 != 0 and (BANDS * 121) % 4 != 0
    sides = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in MIXED]
    assert sides[:5] == [(1, 1), (3, 7), (11, 11), (17, 13), (0, 2)]
    ras = DenseRaster(raw, precision="fp32", device=dev())
    whole = PP.preprocess_image(raw)
    sliced = host_sliced(raw, MIXED)
    assert sliced[DEGENERATE] is None and sum(s is None for s in sliced) == 1
    for train in (False, True):
        got = ras.crops(MIXED, train=train)
        assert got.shape == (len(MIXED), BANDS, 11, 11) and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()), bits(gather_crops_np(whole, MIXED, 11, flip=train))), train
        assert_same_bits(got, preprocess_batch(sliced, 11, train=train, device=dev()), ("preprocess_batch", train))
        assert not got[DEGENERATE].any() and bool(got[DEGENERATE - 1].any()) and bool(got[DEGENERATE + 1].any())
        again = ras.crops(torch.from_numpy(MIXED).to(dev()), train=train)      # a rerun (boxes already on the device)
        assert_same_bits(again, got, "rerun")
    assert not torch.equal(ras.crops(MIXED, train=True), ras.crops(MIXED))
    # other sides: 4 (every box downsampled or kept), 24 (every box upsampled)
    for size in (4, 24):
        got = ras.crops(MIXED, size=size, train=True)
        assert np.array_equal(bits(got.cpu().numpy()), bits(gather_crops_np(whole, MIXED, size, flip=True))), size
        assert_same_bits(got, preprocess_batch(sliced, size, train=True, device=dev()), size)
    # boxes that were not clipped read zeros outside the raster (nothing is read out of bounds)
    wild = np.array([(-11, -11, 11, 11), (10, 5, 40, 30), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (100, 100, 120, 130),
                     (2 ** 31 - 1, 0, -2 ** 31, 5)], dtype=np.int64).astype(np.int32)
    got = ras.crops(wild, size=22).cpu().numpy()
    assert np.array_equal(bits(got[:2]), bits(gather_crops_np(whole, wild[:2], 22)))
    assert not got[0][:, :11, :].any() and np.array_equal(bits(got[0][:, 11:, 11:]), bits(whole[:, :11, :11]))
    assert not got[3].any()
    # out=: written in place; a wrong shape raises
    buf = torch.empty(len(MIXED), BANDS, 11, 11, device=dev())
    assert ras.crops(MIXED, out=buf) is buf
    assert_same_bits(buf, ras.crops(MIXED), "out")
    with pytest.raises(ValueError, match="out must be"):
        ras.crops(MIXED, out=torch.empty(len(MIXED), BANDS, 11, 12, device=dev()))
    with pytest.raises(ValueError, match="boxes"):
        ras.crops(np.zeros((3, 2), np.int32))
    with pytest.raises(RuntimeError, match="precision='bf16'"):
        ras.crops(MIXED, tiles=True)


def test_tile_crops_equal_crop_preprocessing_tiles():
    from deeptreeattention_amd.dense import DenseRaster
    from deeptreeattention_amd.preprocess import preprocess_batch
    raw = year_rasters()[0]
    ras = DenseRaster(raw, precision="bf16", device=dev())
    sliced = host_sliced(raw, MIXED)
    for train in (False, True):
        for size in (11, 5):
            got = ras.crops(MIXED, tiles=True, size=size, train=train)
            want = preprocess_batch(sliced, size, train=train, device=dev(), tiles=True)
            assert got.shape == want.shape == (len(MIXED), BANDS, size, size)
            assert got.tiles.dtype == want.tiles.dtype == torch.int16
            assert torch.equal(got.tiles.cpu(), want.tiles.cpu()), (train, size)
    again = ras.crops(MIXED, tiles=True)
    assert torch.equal(again.tiles, ras.crops(MIXED, tiles=True).tiles)
    with pytest.raises(ValueError, match="out must be"):
        ras.crops(MIXED, tiles=True, out=torch.empty(7, dtype=torch.int16, device=dev()))
    with pytest.raises(RuntimeError, match="precision='fp32'"):
        ras.crops(MIXED)


def test_crops_years_equals_per_year_crops_with_flags_from_the_values():
    from deeptreeattention_amd.dense import DenseRaster
    ras = dense_years(year_rasters())                # a scene, a missing year, a year that normalises to all zeros
    assert not ras[2].data.any()
    n = len(MIXED)
    boxes = torch.from_numpy(MIXED).to(dev())
    banks = [torch.zeros(3, device=dev()), torch.ones(3, device=dev())]      # stale ones in the incoming bank's partner
    outs = [torch.full((n, BANDS, 11, 11), 7.0, device=dev()) for _ in range(3)]
    flags = DenseRaster.crops_years(ras, boxes, outs, banks[0], banks[1])
    assert flags is banks[0] and flags.cpu().tolist() == [1.0, 0.0, 0.0]
    assert not banks[1].any()                                                # clear_next is zeroed
    assert bool((outs[1] == 7.0).all())                                      # the missing year's buffer is untouched
    for y in (0, 2):
        assert_same_bits(outs[y], ras[y].crops(boxes), ("year", y))
    # the next call takes the bank this one cleared: the stale ones do not leak into its flags
    flags2 = DenseRaster.crops_years([ras[2], None, ras[0]], boxes, outs, banks[1], banks[0])
    assert flags2.cpu().tolist() == [0.0, 0.0, 1.0] and not banks[0].any()
    assert_same_bits(outs[2], ras[0].crops(boxes), "swapped")
    # both training flips, on two years that show them (a flipped all-zero year would show nothing)
    scene, other = ras[0], DenseRaster(raw_raster(33, RAW_BANDS, H, W), precision="fp32", device=dev())
    copy = DenseRaster(year_rasters()[0], precision="fp32", device=dev())
    for pair in ([scene, copy], [scene, other]):
        outs2 = [torch.full((n, BANDS, 11, 11), 7.0, device=dev()) for _ in range(2)]
        b2 = [torch.zeros(2, device=dev()) for _ in range(2)]
        assert DenseRaster.crops_years(pair, boxes, outs2, b2[0], b2[1], train=True).cpu().tolist() == [1.0, 1.0]
        for y in range(2):
            assert_same_bits(outs2[y], pair[y].crops(boxes, train=True), ("train", y))
        assert not torch.equal(outs2[0], scene.crops(boxes))
    # NaN counts as non-zero; a batch of boxes off the raster sets no flag
    ras[2].data[3, 4, 5] = float("nan")
    b3 = [torch.zeros(3, device=dev()) for _ in range(2)]
    assert DenseRaster.crops_years(ras, boxes, outs, b3[0], b3[1]).cpu().tolist() == [1.0, 0.0, 1.0]
    off = torch.tensor([[40, 40, 50, 50]], dtype=torch.int32, device=dev())
    assert DenseRaster.crops_years(ras, off, [t[:1] for t in outs], b3[1], b3[0]).cpu().tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="present"):
        DenseRaster.crops_years([None, None], boxes, outs[:2], b3[0][:2], b3[1][:2])


# ---------------------------------------------------------------------------------------------------------------------
# the routes: the new one against the existing predictors fed with host-sliced crops through preprocess_batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_predict_crops_equals_predictor_on_host_sliced_crops(prec):
    """Predictor.__call__ is Predictor.logits_of followed by dta_softmax_top2: the launches predict_crops makes per batch."""
    from deeptreeattention_amd.dense import DenseRaster, predict_crops, raster_precision
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    classes = 7
    raw = year_rasters()[0]
    boxes = route_boxes()
    n = len(boxes)
    model, _ = make("hang", BANDS, classes, 31, prec)
    assert raster_precision(model) == prec
    ras = DenseRaster(raw, precision=prec, device=dev())
    sliced = host_sliced(raw, boxes)
    assert all(s is not None for s in sliced)
    ref = Predictor(model)
    for B in BATCHES:
        res = predict_crops(model, ras, boxes, batch_size=B, return_probs=True)
        assert res.crowns is None and res.top_idx.shape == (n, 2) and res.probs.shape == (n, classes)
        for n0 in range(0, n, B):
            n1 = min(n0 + B, n)
            p, i, s = ref(preprocess_batch(sliced[n0:n1], 11, device=dev(), tiles=prec == "bf16"), return_probs=True)
            assert_same_bits(res.probs[n0:n1], p, ("probabilities", B, n0))
            assert torch.equal(res.top_idx[n0:n1].cpu(), i.cpu()), (B, n0)
            assert_same_bits(res.top_score[n0:n1], s, ("top-2 scores", B, n0))
        lean = predict_crops(Predictor(model), ras, boxes, batch_size=B)
        assert lean.probs is None and torch.equal(lean.top_idx, res.top_idx)
    with pytest.raises(ValueError, match="box 1 "):
        predict_crops(model, ras, [(0, 0, 3, 3), (20, 0, 25, 4)])


def _ensemble():
    from deeptreeattention_amd.year import learned_ensemble
    torch.manual_seed(5)
    return learned_ensemble(3, 6, {"pretrain_state_dict": None, "bands": BANDS}).to(dev()).eval()


def test_predict_crops_three_year_ensemble_with_a_missing_year():
    from deeptreeattention_amd.dense import DenseRaster, predict_crops
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    ens = _ensemble()
    raw0, raw2 = year_rasters()[0], raw_raster(47, RAW_BANDS, H, W)
    boxes = route_boxes()
    n = len(boxes)
    s0, s2 = host_sliced(raw0, boxes), host_sliced(raw2, boxes)
    rasters = [DenseRaster(raw0, precision="fp32", device=dev()), None, DenseRaster(raw2, precision="fp32", device=dev())]
    ref = Predictor(ens)
    for B in BATCHES:
        res = predict_crops(ens, rasters, boxes, batch_size=B, return_probs=True)
        for n0 in range(0, n, B):
            n1 = min(n0 + B, n)
            x0, x2 = preprocess_batch(s0[n0:n1], 11, device=dev()), preprocess_batch(s2[n0:n1], 11, device=dev())
            p, i, s = ref([x0, torch.zeros_like(x0), x2], return_probs=True)
            assert_same_bits(res.probs[n0:n1], p, ("probabilities", B, n0))
            assert torch.equal(res.top_idx[n0:n1].cpu(), i.cpu()), (B, n0)
            assert_same_bits(res.top_score[n0:n1], s, ("top-2 scores", B, n0))


def test_predict_crops_multistage_equals_the_ensemble_on_host_sliced_crops():
    from deeptreeattention_amd.dense import predict_crops_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)
    raws = year_rasters()
    boxes = route_boxes()
    n = len(boxes)
    sliced = [None if r is None else host_sliced(r, boxes) for r in raws]
    ref = MultiStagePredictor(models, hierarchy=h)
    for B in BATCHES:
        res = predict_crops_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws), boxes, batch_size=B,
                                       return_probs=True)
        assert res.crowns is None and res.ens_label.shape == (n,) and int(res.ens_label.min()) >= 0
        for n0 in range(0, n, B):
            n1 = min(n0 + B, n)
            xs = [torch.zeros(n1 - n0, BANDS, 11, 11, device=dev()) if s is None else preprocess_batch(s[n0:n1], 11, device=dev())
                  for s in sliced]
            e = ref.ensemble(xs, present=None)
            for k, name in enumerate(("ens_label", "ens_score", "ens_level")):
                assert_same_bits(getattr(res, name)[n0:n1], e[k], (name, B, n0))
            for l in range(3):
                assert_same_bits(res.top_idx[l][n0:n1], ref.top_idx[l], ("top_idx", l, B, n0))
                assert_same_bits(res.top_score[l][n0:n1], ref.top_score[l], ("top_score", l, B, n0))
                assert_same_bits(res.probs[l][n0:n1], ref.probs[l], ("probs", l, B, n0))
    assert res.ens_label.dtype == torch.int64 and res.ens_score.dtype == torch.float32 and res.ens_level.dtype == torch.int32


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_predict_crops_metadata_equals_metadata_predictor_on_host_sliced_crops(prec):
    from deeptreeattention_amd.dense import DenseRaster, predict_crops_metadata
    from deeptreeattention_amd.engine import MetadataPredictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    from test_metadata_predict_gpu import small_model
    classes, sites, site = 7, 4, 2
    raw = year_rasters()[0]
    boxes = route_boxes()
    n = len(boxes)
    sliced = host_sliced(raw, boxes)
    m = small_model(BANDS, classes, sites, seed=5, precision=prec)
    pred, ref = MetadataPredictor(m), MetadataPredictor(m)
    ras = DenseRaster(raw, precision=prec, device=dev())
    for B in BATCHES:
        res = predict_crops_metadata(pred, ras, site, boxes, batch_size=B, return_probs=True)
        assert res.crowns is None
        for n0 in range(0, n, B):
            n1 = min(n0 + B, n)
            x = preprocess_batch(sliced[n0:n1], 11, device=dev(), tiles=prec == "bf16")
            p, i, s = ref(x, torch.full((n1 - n0,), site, dtype=torch.int64, device=dev()))
            assert_same_bits(res.probs[n0:n1], p, ("probabilities", B, n0))
            assert torch.equal(res.top_idx[n0:n1].cpu(), i.cpu()), (B, n0)
            assert_same_bits(res.top_score[n0:n1], s, ("top-2 scores", B, n0))


def test_crop_routes_refuse_before_any_launch(monkeypatch):
    from deeptreeattention_amd import _lib, dense
    from deeptreeattention_amd.engine import MetadataPredictor, MultiStagePredictor, Predictor
    from test_metadata_predict_gpu import small_model
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)
    raws = year_rasters()
    ras = dense_years(raws)
    bf16 = dense.DenseRaster(raws[0], precision="bf16", device=dev())
    boxes = MIXED[:3]
    ms = MultiStagePredictor(models, hierarchy=h)
    ens = _ensemble()
    hang, fusion = make("hang", BANDS, 7, 31, "fp32")[0], small_model(BANDS, 7, 4, seed=5, precision="fp32")
    single, ens_pred, meta = Predictor(hang), Predictor(ens), MetadataPredictor(fusion)      # (predictors hold their models weakly)
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_launch)
    monkeypatch.setattr(_lib, "current_stream_ptr", no_launch)
    # a wrong raster precision
    with pytest.raises(RuntimeError, match="precision='fp32'"):
        dense.predict_crops(single, bf16, boxes)
    with pytest.raises(RuntimeError, match="fp32"):
        dense.predict_crops_multistage(ms, [bf16, None, None], boxes)
    with pytest.raises(RuntimeError, match="precision='fp32'"):
        dense.predict_crops_metadata(meta, bf16, 1, boxes)
    # a wrong number of years
    with pytest.raises(ValueError, match="3 rasters"):
        dense.predict_crops(ens_pred, ras[:2], boxes)
    with pytest.raises(ValueError, match="rasters"):
        dense.predict_crops_multistage(ms, ras[:2], boxes)
    # no year present
    with pytest.raises(ValueError, match="present"):
        dense.predict_crops(ens_pred, [None, None, None], boxes)
    with pytest.raises(ValueError, match="present"):
        dense.predict_crops_multistage(ms, [None, None, None], boxes)
    # a box that misses the raster
    with pytest.raises(ValueError, match="box 0 "):
        dense.predict_crops_multistage(ms, ras, [(30, 30, 40, 40)])
