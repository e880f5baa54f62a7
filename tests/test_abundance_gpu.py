"""Species abundance with uncertainty on the device (dta_abundance_resample / dta_abundance_counts, abundance.resample /
abundance.counts) against the host definition (abundance.resample_np / counts_np): every comparison is exact, the counts are
integers and every draw is decided by integer arithmetic and one float32 comparison."""

import numpy as np
import pytest
import torch

from test_abundance_cpu import random_confusion, random_crowns

pytestmark = pytest.mark.gpu

MAXS = 256      # DTA_ABUNDANCE_MAX_SPECIES


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def case(seed, N, S):
    from deeptreeattention_amd.abundance import sampling_table
    rng = np.random.default_rng(seed)
    table = sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    mask = rng.random(N) < 0.7
    return table, label, score, mask


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# N: one crown, either side of a wave, under / over the 1024 crowns a workgroup's slice starts at (4099: five slices, the
# last one short); iterations: under, over and not a multiple of the 8 of an iteration group; S: every listed value
SHAPES = [(1, 1, 1), (63, 7, 2), (64, 33, 6), (65, 100, 200), (1000, 7, MAXS), (4099, 33, 200), (4099, 100, 6), (1000, 1, 2),
          (65, 33, MAXS), (64, 100, 1), (63, 1, 200), (1, 7, 6)]


@pytest.mark.parametrize("N,iterations,S", SHAPES)
def test_resample_equals_the_mirror(N, iterations, S):
    from deeptreeattention_amd import abundance
    assert MAXS == abundance.MAX_SPECIES
    table, label, score, mask = case(1000 * N + S, N, S)
    dtable = abundance.device_table(table, dev())
    assert dtable.dtype == torch.uint32 and dtable.is_cuda
    dl, ds, dm = up(label), up(score), up(mask)
    for sc, dsc in ((score, ds), (None, None)):
        for m, dmm in ((None, None), (mask, dm)):
            want = abundance.resample_np(label, sc, table, iterations, seed=7, first_iteration=3, mask=m)
            got = abundance.resample(dl, dsc, dtable, iterations, seed=7, first_iteration=3, mask=dmm)
            assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (iterations, S + 1)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (sc is None, m is None)
    # a uint8 mask is the bool mask; the host table is taken as it is (checked and uploaded by the call)
    want = abundance.resample_np(label, score, table, iterations, seed=7, first_iteration=3, mask=mask)
    assert torch.equal(abundance.resample(dl, ds, table, iterations, seed=7, first_iteration=3, mask=up(mask.astype(np.uint8))).cpu(),
                       torch.from_numpy(want))


def test_counter_is_formed_in_64_bits():
    from deeptreeattention_amd import abundance
    table, label, score, mask = case(11, 65, 6)
    dtable = abundance.device_table(table, dev())
    rows = {}
    for first in (0, 2 ** 33, 2 ** 33 + 5, 2 ** 64 - 2):
        want = abundance.resample_np(label, score, table, 9, seed=2 ** 63 + 11, first_iteration=first, mask=mask)
        got = abundance.resample(up(label), up(score), dtable, 9, seed=2 ** 63 + 11, first_iteration=first, mask=up(mask))
        assert torch.equal(got.cpu(), torch.from_numpy(want)), first
        rows[first] = got.cpu()
    assert not torch.equal(rows[0], rows[2 ** 33])                      # 2^33 is not 0: the high half takes part
    # one iteration per call is a row of the longer run (the reference's use)
    run = abundance.resample(up(label), up(score), dtable, 12, seed=4)
    for k in (0, 7, 8, 11):
        assert torch.equal(abundance.resample(up(label), up(score), dtable, 1, seed=4, first_iteration=k)[0], run[k]), k


def test_counts_are_overwritten_and_nothing_is_left_behind():
    """The documented behaviour: counts is overwritten in full, never added to; a second call with other shapes into the
    same output and the same workspace sees nothing of the first (the C entry, so that both buffers really are shared)."""
    from deeptreeattention_amd import _lib, abundance
    L = _lib.lib()
    big = case(21, 4099, 200)
    small = case(22, 65, 6)
    nbytes = max(L.dta_abundance_workspace_bytes(4099, 200, 33), L.dta_abundance_workspace_bytes(65, 6, 7))
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((33 * 201,), 7, dtype=torch.int64, device=dev())
    keep = []

    def run(c, n, S, iterations):
        table, label, score, mask = c
        t = [abundance.device_table(table, dev()), up(label), up(score), up(mask.astype(np.uint8))]
        keep.append(t)
        _lib.check(L.dta_abundance_resample(_lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), n, _lib.ptr(t[0]), S, iterations, 5, 0,
                                            _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.current_stream_ptr()), "dta_abundance_resample")
        want = abundance.resample_np(label, score, table, iterations, seed=5, mask=mask)
        return out[:iterations * (S + 1)].view(iterations, S + 1).cpu(), torch.from_numpy(want)

    got, want = run(big, 4099, 200, 33)
    assert torch.equal(got, want)
    first = out.clone()
    got, want = run(small, 65, 6, 7)
    assert torch.equal(got, want)
    assert torch.equal(out[7 * 7:], first[7 * 7:])                       # and not an element past its own [7][7] is written
    got, want = run(big, 4099, 200, 33)                                  # and back: the same result, not twice it
    assert torch.equal(got, want)
    # out= of the Python route: overwritten as well
    table, label, score, mask = small
    buf = torch.full((7, 7), 1 << 40, dtype=torch.int64, device=dev())
    assert abundance.resample(up(label), up(score), table, 7, seed=5, mask=up(mask), out=buf) is buf
    assert torch.equal(buf.cpu(), torch.from_numpy(abundance.resample_np(label, score, table, 7, seed=5, mask=mask)))
    with pytest.raises(ValueError, match="out must be"):
        abundance.resample(up(label), up(score), table, 7, out=torch.empty(7, 8, dtype=torch.int64, device=dev()))
    assert tuple(abundance.resample(up(label), up(score), table, 0).shape) == (0, 7)


def test_counts_equal_bincount():
    from deeptreeattention_amd import abundance
    for N, S in ((1, 1), (65, 6), (4099, 200), (1000, MAXS)):
        _, label, _, mask = case(31 + N, N, S)
        inside = (label >= 0) & (label < S)
        assert N < 5 or (~inside).any()
        binned = np.where(inside, label, S)
        got = abundance.counts(up(label), S)
        assert got.dtype == torch.int64 and tuple(got.shape) == (S + 1,)
        assert torch.equal(got.cpu(), torch.from_numpy(np.bincount(binned, minlength=S + 1)))
        assert torch.equal(abundance.counts(up(label), S, mask=up(mask)).cpu(), torch.from_numpy(np.bincount(binned[mask], minlength=S + 1)))
        assert np.array_equal(abundance.counts_np(label, S, mask), np.bincount(binned[mask], minlength=S + 1))
    with pytest.raises(ValueError, match="species"):
        abundance.counts(up(label), MAXS + 1)


def test_device_route_refuses_bad_tensors_before_any_launch(monkeypatch):
    from deeptreeattention_amd import _lib, abundance
    table, label, score, mask = case(41, 65, 6)
    dl, ds, dt = up(label), up(score), abundance.device_table(table, dev())
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_launch)
    with pytest.raises(ValueError, match="label"):
        abundance.resample(dl.to(torch.int32), ds, dt)
    with pytest.raises(ValueError, match="score"):
        abundance.resample(dl, ds.double(), dt)
    with pytest.raises(ValueError, match="score"):
        abundance.resample(dl, ds[:-1], dt)
    with pytest.raises(ValueError, match="mask"):
        abundance.resample(dl, ds, dt, mask=up(mask.astype(np.int32)))
    with pytest.raises(ValueError, match="table"):
        abundance.resample(dl, ds, dt.cpu())
    with pytest.raises(ValueError, match="table"):
        abundance.resample(dl, ds, dt[:, :5])
    with pytest.raises(ValueError, match="iterations"):
        abundance.resample(dl, ds, dt, iterations=-1)


def test_end_to_end_from_crown_boxes_to_resampled_counts():
    """dense.predict_crops_multistage on a small raster -> MultiStagePredictor.confusion -> sampling_table -> resample on the
    returned ens_label / ens_score, as they are: equals the mirror on the copied-back labels, every row sums to the boxes."""
    from deeptreeattention_amd import abundance
    from deeptreeattention_amd.dense import predict_crops_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    from test_dense_crops_gpu import route_boxes
    from test_dense_multistage_cpu import three_level_hierarchy
    from test_dense_multistage_gpu import BANDS, dense_years, year_rasters
    from test_multistage_ensemble_gpu import _small_levels
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)
    pred = MultiStagePredictor(models, hierarchy=h)
    ras = dense_years(year_rasters())
    boxes = route_boxes()
    n, S = len(boxes), h.n_species
    # a confusion matrix of this predictor: its labels on the same crops against made-up truth
    crops = [torch.zeros(n, BANDS, 11, 11, device=dev()) if r is None else r.crops(boxes) for r in ras]
    truth = torch.from_numpy(np.random.default_rng(8).integers(0, S, n))
    pred.ensemble(crops, labels=truth)
    assert tuple(pred.confusion.shape) == (S, S) and int(pred.confusion.sum()) == n
    res = predict_crops_multistage(pred, ras, boxes, batch_size=16)
    assert res.ens_label.dtype == torch.int64 and res.ens_score.dtype == torch.float32 and res.ens_label.shape == (n,)
    for given in ("label", "prediction"):
        table = abundance.sampling_table(pred.confusion, given=given)
        got = abundance.resample(res.ens_label, res.ens_score, abundance.device_table(table, dev()), iterations=20, seed=1)
        want = abundance.resample_np(res.ens_label.cpu().numpy(), res.ens_score.cpu().numpy(), table, 20, seed=1)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), given
        assert bool((got.sum(1) == n).all())
    plain = abundance.counts(res.ens_label, S)
    assert torch.equal(plain.cpu(), torch.from_numpy(np.bincount(res.ens_label.cpu().numpy(), minlength=S + 1)))
    s = abundance.summary(got)
    assert s.mean.shape == (S + 1,) and abs(s.mean.sum() - n) < 1e-9
