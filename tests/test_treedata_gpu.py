"""The resident training set on the device (csrc/treedata.hip) against the host definitions of treedata.py: the gather
equals batch_np bit for bit, the flags equal dta_year_flags' verdict, the order equals epoch_order_np, from_raw equals the
reference's own items (tests/golden/treedata), and fit_multistage on a LevelViews equals fit_multistage on the same views
taken as plain per-level loaders.  Every comparison of copied data is equality of bits."""
import collections
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import treedata_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES, B_LIST = TC.PLAN_SIZES, (1, 5, 64, 129)
_crops = {}


def dev():
    return torch.device("cuda:0")


def host_crops(n, years, bands, size):
    key = (n, years, bands, size)
    if key not in _crops:
        _crops.clear()                       # one set of host crops at a time (the 369-band one is 107 MB)
        _crops[key] = TC.synthetic_crops(n, years, bands, size, seed=bands * 100 + size + years)
    return _crops[key]


def views_of(pool, sizes, seed):
    """One view per size: rows drawn with repeats out of the whole pool, labels, and train on for every other level."""
    rng = np.random.default_rng(seed)
    return [pool.view(rng.integers(0, pool.n, n), rng.integers(0, 9, n), train=l % 2 == 0) for l, n in enumerate(sizes)]


def flags_np(batches):
    """What dta_year_flags says about batches: !(v == 0) somewhere, so a NaN counts and -0.0 does not."""
    return np.array([float((~(b == 0)).any()) for b in batches], np.float32)


def picked(steps):
    return set(range(steps)) if steps <= 8 else {0, 1, 2, steps - 2, steps - 1}


def check_epoch(T, levels, content, B, shuffle, seed, epoch, train=None, drop_last=False):
    views = list(levels)
    sizes = [len(v) for v in views]
    nb, steps = T.plan(sizes, B, drop_last)
    orders = [T.epoch_order_np(n, epoch, seed, v.level) if shuffle else np.arange(n) for n, v in zip(sizes, views)]
    Y, seen = views[0].pool.n_years, 0
    for s, (batch, flags) in enumerate(levels.batches(B, shuffle, seed, train=train, drop_last=drop_last, epoch=epoch)):
        seen += 1
        if s not in picked(steps):
            continue
        want_flags = []
        for l, (v, (names, inputs, labels)) in enumerate(zip(views, batch)):
            start, count = T.step_positions(sizes[l], nb[l], B, s)
            entries = orders[l][start:start + count]
            want = T.batch_np(content, v.rows_np[entries], v.train if train is None else train)      # (every view here sets its own)
            assert len(inputs["HSI"]) == Y
            for y in range(Y):
                x = inputs["HSI"][y]
                assert x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0
                assert TC.same_bits(x.cpu().numpy(), want[y]), (B, s, l, y)
            want_flags += list(flags_np(want))
            assert np.array_equal(inputs["rows"].cpu().numpy(), v.rows_np[entries])
            assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), v.labels.cpu().numpy()[entries])
            assert names == [v.pool.individuals[i] for i in v.rows_np[entries]]
        assert flags.dtype == torch.float32 and np.array_equal(flags.cpu().numpy(), np.array(want_flags, np.float32)), (B, s)
    assert seen == steps


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("bands,size", [(3, 11), (6, 11), (369, 11), (5, 24)])
def test_gather_equals_batch_np(bands, size, dtype):
    """C * S * S mod 4 is 3, 2, 1 and 0: a lane's four floats straddle planes and crops in every phase.  Five levels x three
    years of sizes (7, 130, 64, 1, 200) -- short last batches at different steps, a level smaller than the batch, cycling --
    and one level x one year through the view's own loader; B = 1, 5, 64, 129; the flips on for every other level."""
    from deeptreeattention_amd import treedata as T
    assert (bands * size * size) % 4 == {3: 3, 6: 2, 369: 1, 5: 0}[bands]
    tdt = getattr(torch, dtype)
    crops, present = host_crops(200, 3, bands, size)
    pool = T.CropPool(crops, present=present, device=dev(), dtype=tdt)
    content = crops if dtype == "float32" else T.bf16_round_np(crops)
    assert TC.same_bits(pool.numpy(), content)
    levels = T.LevelViews(views_of(pool, SIZES, seed=bands))
    for B in B_LIST:
        check_epoch(T, levels, content, B, shuffle=True, seed=3, epoch=2)
    if bands != 369:         # (what these two add does not depend on the crop's size)
        check_epoch(T, levels, content, 64, shuffle=False, seed=0, epoch=0, train=True)
        check_epoch(T, T.LevelViews(list(levels)[1:3] + list(levels)[4:]), content, 64, shuffle=True, seed=1, epoch=0, drop_last=True)
    # L = 1, Y = 1: the view's own loader
    one = T.CropPool(crops[:130, :1], device=dev(), dtype=tdt)
    view = one.view(np.arange(130)[::-1].copy(), np.arange(130) % 7, train=True)
    for B in B_LIST:
        order = T.epoch_order_np(130, 5, 9, 0)
        got = list(view.loader(B, shuffle=True, seed=9, epoch=5))
        assert len(got) == -(-130 // B)
        for k in sorted(picked(len(got))):
            names, inputs, labels = got[k]
            entries = order[k * B:(k + 1) * B]
            want = T.batch_np(content[:130, :1], view.rows_np[entries], True)
            assert len(inputs["HSI"]) == 1 and TC.same_bits(inputs["HSI"][0].cpu().numpy(), want[0]), (B, k)
            assert np.array_equal(labels.cpu().numpy(), (np.arange(130) % 7)[entries]) and names == view.rows_np[entries].tolist()
    assert sum(len(b[0]) for b in view.loader(64, drop_last=True)) == 128


def test_flags_missing_batches_nan_and_negative_zero():
    from deeptreeattention_amd import treedata as T
    crops, _ = TC.synthetic_crops(12, 3, 3, 11, seed=4, missing=0.0)
    crops[0:4, 1] = 0                    # rows 0..3: year 1 missing
    crops[4:8] = 0
    crops[5, 2, 1, 7, 3] = np.nan        # rows 4..7: all zero but one NaN in year 2
    crops[8:12] = 0
    crops[8:12, 0] = -0.0                # rows 8..11: year 0 holds only -0.0
    pool = T.CropPool(crops, device=dev())
    levels = T.LevelViews([pool.view([0, 1, 2, 3], [0] * 4), pool.view([4, 5, 6, 7], [0] * 4, train=True), pool.view([8, 9, 10, 11], [0] * 4)])
    (batch, flags), = list(levels.batches(4))
    assert flags.cpu().tolist() == [1, 0, 1, 0, 0, 1, 0, 0, 0]
    minus = batch[2][1]["HSI"][0].cpu().numpy()
    assert (TC.bits(minus) == 0x80000000).all()                            # the bits are copied
    got = batch[1][1]["HSI"][2].cpu().numpy()
    assert np.isnan(got).sum() == 1 and np.isnan(got[1, 1, 10 - 7, 10 - 3])   # train: the plane reversed
    # two steps: the flags of the step before do not leak into the next one's bank
    again = [f.cpu().tolist() for _, f in T.LevelViews(list(levels)[::-1]).batches(2)]
    assert again == [[0, 0, 0, 0, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0, 1, 0, 1]]


def test_flip_defaults_a_loader_does_not_flip_and_training_batches_do():
    """A view that does not say: `loader` leaves the crops as they are (a validation or prediction set), `batches` flips
    them (training batches); a view's own setting comes first, the call's argument before both."""
    from deeptreeattention_amd import treedata as T
    crops, _ = TC.synthetic_crops(5, 2, 3, 11, seed=2, missing=0.0)
    pool = T.CropPool(crops, device=dev())
    rows = np.array([3, 0, 4])
    plain, flipped = T.batch_np(crops, rows, False), T.batch_np(crops, rows, True)

    def year0(batch):
        return batch[1]["HSI"][0].cpu().numpy()
    unset, on, off = pool.view(rows, [0, 1, 2]), pool.view(rows, [0, 1, 2], train=True), pool.view(rows, [0, 1, 2], train=False)
    assert unset.train is None and TC.same_bits(unset.batch_np([0, 1, 2])[0], plain[0])
    assert TC.same_bits(year0(next(unset.loader(3))), plain[0]) and TC.same_bits(year0(next(on.loader(3))), flipped[0])
    assert TC.same_bits(year0(next(on.loader(3, train=False))), plain[0])
    (batch, _), = list(T.LevelViews([unset, on, off]).batches(3))
    assert [TC.same_bits(year0(b), w[0]) for b, w in zip(batch, (flipped, flipped, plain))] == [True] * 3
    (batch, _), = list(T.LevelViews([unset, on, off]).batches(3, train=False))
    assert all(TC.same_bits(year0(b), plain[0]) for b in batch)


def test_epoch_order_equals_the_definition_several_levels_in_one_launch():
    from deeptreeattention_amd import treedata as T
    # (the third launch: sizes either side of the workgroup and of the LDS tile, so whole workgroups of the shorter levels
    # leave before the first barrier while their neighbours in the grid stay)
    for sizes, ids in (((1, 63, 64, 65, 1000), None), ((4097, 20000, 64), (7, 0, 63)), ((255, 256, 257, 1023, 1024, 1025), None)):
        got = T.epoch_order(sizes, epoch=2 ** 40 + 3, seed=11, levels=ids, device=dev())
        for k, n in enumerate(sizes):
            want = T.epoch_order_np(n, 2 ** 40 + 3, 11, k if ids is None else ids[k])
            assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want), n
    with pytest.raises(ValueError, match="entries"):
        T.epoch_order([T.MAX_N + 1], device=dev())
    with pytest.raises(ValueError, match="tables"):
        T.epoch_order([4] * 9, device=dev())


def test_from_annotations_equals_the_reference_items():
    from deeptreeattention_amd import treedata as T
    fx = TC.Fixture()
    z = fx.z
    pool = T.CropPool.from_annotations(fx.columns, fx.raw_by_path, image_size=fx.image_size, device=dev(), chunk=4)
    assert pool.individuals == fx.individuals and pool.years == fx.years and np.array_equal(pool.labels, z["labels"])
    assert TC.same_bits(pool.numpy(), z["items_eval"])                       # train=False, bits
    assert np.array_equal(pool.present, z["items_eval"].reshape(6, 3, -1).any(2))
    raw = T.CropPool.from_raw(fx.raw(), image_size=fx.image_size, device=dev())
    assert TC.same_bits(raw.numpy(), z["items_eval"])
    for train, items in ((False, z["items_eval"]), (True, z["items_train"])):
        view = pool.view(np.arange(6), pool.labels, train=train)
        (names, inputs, labels), = list(view.loader(8))
        assert names == fx.individuals and np.array_equal(labels.cpu().numpy(), z["labels"])
        for y in range(3):
            assert TC.same_bits(inputs["HSI"][y].cpu().numpy(), items[:, y]), (train, y)
    half = T.CropPool.from_raw(fx.raw(), image_size=fx.image_size, device=dev(), dtype=torch.bfloat16)
    assert TC.same_bits(half.numpy(), T.bf16_round_np(z["items_eval"]))


def test_from_rasters_equals_the_single_raster_crops():
    from deeptreeattention_amd import dense, treedata as T
    rng = np.random.default_rng(3)
    raws = [rng.integers(0, 5000, (26, 40, 37)).astype(np.int16), None, rng.integers(0, 5000, (26, 40, 37)).astype(np.int16)]
    rasters = [None if r is None else dense.DenseRaster(r, precision="fp32", device=dev()) for r in raws]
    r0 = rng.integers(0, 30, 9)
    c0 = rng.integers(0, 28, 9)
    boxes = np.stack([r0, c0, r0 + rng.integers(1, 10, 9), c0 + rng.integers(1, 9, 9)], 1).astype(np.int32)
    pool = T.CropPool.from_rasters(rasters, boxes, image_size=11, chunk=4)
    assert (pool.n, pool.n_years, pool.bands, pool.size) == (9, 3, 6, 11) and pool.present.tolist() == [[1, 0, 1]] * 9
    for y, ras in enumerate(rasters):
        got = pool.data[:, y].cpu().numpy()
        assert TC.same_bits(got, np.zeros_like(got) if ras is None else ras.crops(boxes, size=11).cpu().numpy())


def test_second_stream_and_reruns_are_bit_identical():
    from deeptreeattention_amd import treedata as T
    crops, present = host_crops(200, 3, 6, 11)
    pool = T.CropPool(crops, present=present, device=dev())
    levels = T.LevelViews(views_of(pool, (7, 130, 64), seed=1))

    def run():
        out = []
        for batch, flags in levels.batches(64, shuffle=True, seed=2, epoch=1):
            out.append([x.clone() for b in batch for x in b[1]["HSI"]] + [flags.clone()] + [b[2].clone() for b in batch])
        return out
    first = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    third = run()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        for x, y, z in zip(a, b, c):
            assert TC.same_bits(x.cpu().numpy(), y.cpu().numpy()) and TC.same_bits(x.cpu().numpy(), z.cpu().numpy())


def test_rows_outside_the_pool_write_zeros_at_the_c_entry():
    """The wrapper refuses such rows (tests/test_treedata_cpu.py); here the row and order tables are spoilt by hand and
    handed to dta_pool_batches itself: a bad row or entry gives an all-zero crop, nothing outside the pool is read."""
    from deeptreeattention_amd import _lib, treedata as T
    crops, _ = TC.synthetic_crops(6, 2, 3, 11, seed=8, missing=0.0)
    pool = T.CropPool(crops, device=dev())
    rows = torch.tensor([2, -1, 6, 2 ** 40, 5, -2 ** 62], dtype=torch.int64, device=dev())
    labels = torch.arange(6, dtype=torch.int64, device=dev()) + 10
    order = torch.tensor([4, 1, 0, 6, -3, 3], dtype=torch.int32, device=dev())      # entries 6 and -3 do not exist
    per = 3 * 121
    outs = [torch.full((6, 3, 11, 11), float("nan"), device=dev()) for _ in range(4)]
    ints = torch.full((4, 6), 77, dtype=torch.int64, device=dev())
    flags = torch.zeros(4, device=dev())
    lv = (_lib.PoolLevel * 2)(
        _lib.PoolLevel(None, rows.data_ptr(), labels.data_ptr(), 6, 0, 6, 0, ints[0].data_ptr(), ints[1].data_ptr()),
        _lib.PoolLevel(order.data_ptr(), rows.data_ptr(), labels.data_ptr(), 6, 0, 6, 1, ints[2].data_ptr(), ints[3].data_ptr()))
    L = _lib.lib()
    _lib.check(L.dta_pool_batches(_lib.ptr(pool.data), _lib.DTA_F32, 6, 2, 3, 11, 2, lv, (C.c_void_p * 4)(*[o.data_ptr() for o in outs]),
                                  _lib.ptr(flags), None, _lib.current_stream_ptr()), "dta_pool_batches")
    zero = np.zeros((3, 11, 11), np.float32)
    for y in range(2):
        want = [crops[2, y], zero, zero, zero, crops[5, y], zero]
        assert TC.same_bits(outs[y].cpu().numpy(), np.stack(want)), y
        flip = [crops[5, y][:, ::-1, ::-1], zero, crops[2, y][:, ::-1, ::-1], zero, zero, zero]      # entries 4, 1, 0, (6), (-3), 3
        assert TC.same_bits(outs[2 + y].cpu().numpy(), np.stack(flip)), y
    assert ints[1].cpu().tolist() == rows.cpu().tolist() and ints[0].cpu().tolist() == [10, 11, 12, 13, 14, 15]
    assert ints[3].cpu().tolist() == [5, -1, 2, -1, -1, 2 ** 40] and ints[2].cpu().tolist() == [14, 11, 10, -1, -1, 13]
    assert flags.cpu().tolist() == [1, 1, 1, 1] and per % 4 == 3


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the step takes the flags, the loop takes the views
# ---------------------------------------------------------------------------------------------------------------------
class Counting:
    """The ctypes library with call counters on the entries of interest."""

    def __init__(self, lib, names):
        self._lib, self._names, self.calls = lib, set(names), collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in self._names:
            return f

        def counted(*a):
            self.calls[name] += 1
            return f(*a)
        return counted


def small_trainers(copies):
    from deeptreeattention_amd.engine import MultiStageTrainer
    from deeptreeattention_amd.year import learned_ensemble
    classes, bands, years = [2, 3], 12, 3
    torch.manual_seed(7)
    models = [learned_ensemble(years, c, {"pretrain_state_dict": None, "bands": bands}).to(dev()).train() for c in classes]
    for m in models:
        for net in m.year_models:
            net.precision = "fp32"
    return [MultiStageTrainer(copy.deepcopy(models), [2e-3, 1e-3]) for _ in range(copies)]


def small_levels(sizes=(64, 40)):
    from deeptreeattention_amd import treedata as T
    crops, present = TC.synthetic_crops(80, 3, 12, 11, seed=5, missing=0.3)
    crops[40:, 2] = 0                         # the second level never has its third year: a gated-off network on every step
    pool = T.CropPool(crops, present=present, device=dev())
    rng = np.random.default_rng(6)
    return T.LevelViews([pool.view(np.arange(sizes[0]), rng.integers(0, 2, sizes[0]), train=True),
                         pool.view(40 + np.arange(sizes[1]), rng.integers(0, 3, sizes[1]), train=True)])


def state_of(tr):
    out = []
    for t in tr.levels:
        out += [v.detach().cpu().numpy() for v in t.model.state_dict().values()]
        for yr in t.years:
            for p, g, m, v, cnt in t._year_segments(yr):
                out += [m.detach().reshape(-1)[:cnt].cpu().numpy(), v.detach().reshape(-1)[:cnt].cpu().numpy()]
        out.append(t.dev_steps.cpu().numpy())
    return out


def test_the_gathered_flags_equal_what_the_present_none_step_decides():
    levels = small_levels()
    a, b = small_trainers(2)
    for batch, flags in levels.batches(16, shuffle=True, seed=1):
        want = flags.cpu().tolist()
        a.training_step_all(batch, 0)                                          # present=None: dta_year_flags on the same tensors
        assert a.batched_last == (len({tuple(x[1]["HSI"][0].shape) for x in batch}) == 1)
        local = [f for t in a.levels for f in t.local_flags.cpu().tolist()]
        assert local == want and want[5] == 0
        b.training_step_all(batch, 0, year_flags=flags)
        assert b.batched_last == a.batched_last
    for x, y in zip(state_of(a), state_of(b)):
        assert TC.same_bits(x, y)


def test_fit_multistage_on_level_views_equals_the_per_level_loaders(monkeypatch):
    """float32, the small model sizes of tests/test_multistage_gpu.py, two epochs, shuffled; levels of 64 and 40 crops at
    B = 16: the second level's last batch is short, so one step in four cannot share a chain and falls back."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.loop import fit_multistage
    levels = small_levels()
    new, old = small_trainers(2)
    counting = Counting(_lib.lib(), ("dta_pool_batches", "dta_year_flags", "dta_epoch_order"))
    monkeypatch.setattr(_lib, "_lib", counting)
    shared = []
    step = new.training_step_all

    def watched(*a, **kw):
        before = counting.calls["dta_year_flags"]
        out = step(*a, **kw)
        assert kw.get("year_flags") is not None
        shared.append(new.batched_last)
        assert (counting.calls["dta_year_flags"] == before) == new.batched_last      # never where the levels share a chain
        return out
    new.training_step_all = watched
    h_new = fit_multistage(new, levels, epochs=2, batch_size=16, shuffle=True)
    assert counting.calls["dta_pool_batches"] == 8 == len(shared) and counting.calls["dta_epoch_order"] == 2
    assert shared == [True, True, False, True] * 2
    assert counting.calls["dta_year_flags"] == 2 * len(new.levels)               # the two fallback steps, per level
    counting.calls.clear()
    h_old = fit_multistage(old, list(levels), epochs=2, batch_size=16, shuffle=True)
    assert counting.calls["dta_pool_batches"] == 2 * (4 + 3) and counting.calls["dta_year_flags"] == 2 * (3 + 2)
    assert h_new == h_old and all(np.isfinite(h["train_loss"]).all() for h in h_new)
    for x, y in zip(state_of(new), state_of(old)):
        assert TC.same_bits(x, y)
