"""The resident training set on the host: the definitions of treedata.py against the reference's own TreeDataset
(tests/golden/treedata/treedata_reference.npz, made by tools/make_treedata_golden.py), the epoch order, the batch plan, the
refusals of the wrappers and of the C entry points, and the ABI bookkeeping.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import treedata_cases as TC  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return TC.Fixture()


# ---------------------------------------------------------------------------------------------------------------------
# the fixture against the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_checksum_and_contents(fx):
    import hashlib
    line = open(os.path.join(os.path.dirname(TC.GOLDEN), "SHA256SUMS")).read().split()
    assert line[1] == "treedata_reference.npz" and hashlib.sha256(open(TC.GOLDEN, "rb").read()).hexdigest() == line[0]
    assert os.path.getsize(TC.GOLDEN) < 100 * 1024
    z = fx.z
    N, Y = len(fx.individuals), len(fx.years)
    assert (N, Y) == (6, 3) and z["items_eval"].shape == (N, Y, 6, fx.image_size, fx.image_size)
    assert fx.individuals != sorted(fx.individuals) and fx.years != sorted(fx.years)      # unique() order, not sorted
    assert all(r.shape[0] == 26 and 3 <= min(r.shape[1:]) and max(r.shape[1:]) <= 7 for r in fx.raw_by_path.values())
    for kind in ("train", "eval"):          # preload_images on and off give the same items
        assert TC.same_bits(z["items_" + kind], z["items_%s_lazy" % kind])
    missing = ~z["items_eval"].reshape(N, Y, -1).any(2)
    assert missing.any(0).all() and 0 < missing.sum() < N * Y / 2                          # every year is missing somewhere


def test_annotation_slots_give_the_reference_order_labels_and_missing_years(fx):
    from deeptreeattention_amd import treedata as T
    raw, individuals, years, labels = T.annotation_slots(fx.columns, fx.raw_by_path)
    assert individuals == fx.individuals and years == fx.years
    assert np.array_equal(labels, fx.z["labels"]) and labels.dtype == np.int64
    missing = ~fx.z["items_eval"].reshape(len(individuals), len(years), -1).any(2)
    assert [[c is None for c in r] for r in raw] == missing.tolist()
    want = fx.raw()
    for n in range(len(individuals)):
        for y in range(len(years)):
            assert (raw[n][y] is None) == (want[n][y] is None)
            assert raw[n][y] is None or np.array_equal(raw[n][y], want[n][y])
    # without a label column there are no labels; a path nobody has is a missing year; bad tables are refused
    cols = {k: v for k, v in fx.columns.items() if k != "label"}
    assert T.annotation_slots(cols, fx.raw_by_path)[3] is None
    first = str(fx.columns["image_path"][0])
    fewer = {k: v for k, v in fx.raw_by_path.items() if k != first}
    assert T.annotation_slots(fx.columns, fewer)[0][0][0] is None
    with pytest.raises(ValueError, match="needs individual"):
        T.annotation_slots({"individual": [1]}, {})
    with pytest.raises(ValueError, match="one entry per row"):
        T.annotation_slots(dict(fx.columns, label=fx.columns["label"][:-1]), fx.raw_by_path)


def test_the_last_row_of_an_individual_and_year_wins():
    from deeptreeattention_amd import treedata as T
    cols = {"individual": ["b", "a", "b", "b"], "tile_year": [2020, 2020, 2019, 2020], "image_path": ["p0", "p1", "p2", "p3"],
            "label": [4, 1, 4, 7]}
    raw, individuals, years, labels = T.annotation_slots(cols, {"p%d" % k: np.full((3, 2, 2), k) for k in range(4)})
    assert individuals == ["b", "a"] and years == [2020, 2019] and labels.tolist() == [7, 1]
    assert raw[0][0][0, 0, 0] == 3 and raw[0][1][0, 0, 0] == 2 and raw[1][0][0, 0, 0] == 1 and raw[1][1] is None


def test_batch_np_of_the_unflipped_items_with_train_equals_the_reference_train_items(fx):
    from deeptreeattention_amd import treedata as T
    z = fx.z
    N, Y = z["items_eval"].shape[:2]
    got = T.batch_np(z["items_eval"], np.arange(N), train=True)
    assert len(got) == Y
    for y in range(Y):
        assert TC.same_bits(got[y], z["items_train"][:, y])
    same = T.batch_np(z["items_eval"], [4, 0, 4], train=False)
    assert TC.same_bits(same[1], z["items_eval"][[4, 0, 4], 1])
    # a pool built from the items, on the host: content, zero fill, names, and a view's own batch_np
    present = z["items_eval"].reshape(N, Y, -1).any(2)
    pool = T.CropPool(z["items_eval"], present=present, individuals=fx.individuals, device="cpu")
    assert (pool.n, pool.n_years, pool.bands, pool.size) == (N, Y, 6, fx.image_size) and pool.bytes_per_crop_year == 6 * 25 * 4
    assert TC.same_bits(pool.numpy(), z["items_eval"]) and not pool.numpy()[pool.present == 0].any()
    view = pool.view([5, 2, 0], labels=z["labels"][[5, 2, 0]], train=True)
    assert view.individuals == [fx.individuals[i] for i in (5, 2, 0)] and len(view) == 3
    assert TC.same_bits(view.batch_np([2, 0])[2], z["items_train"][[0, 5], 2])


def test_bf16_storage_is_round_to_nearest_even(fx):
    torch = pytest.importorskip("torch")
    from deeptreeattention_amd import treedata as T
    x = np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.0e38, -1.5e-40, 0.3333333], np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert TC.same_bits(T.bf16_round_np(x), want)
    assert TC.bits(T.bf16_round_np(np.float32([1.00390625])))[0] == 0x3F800000       # a tie goes to the even mantissa
    assert TC.bits(T.bf16_round_np(np.float32([1.01171875])))[0] == 0x3F820000       # ... also upward
    assert np.isnan(T.bf16_round_np(np.float32([np.nan])))[0]
    pool = T.CropPool(fx.z["items_eval"], device="cpu", dtype=torch.bfloat16)
    assert pool.bytes_per_crop_year == 6 * 25 * 2 and TC.same_bits(pool.numpy(), T.bf16_round_np(fx.z["items_eval"]))
    with pytest.raises(ValueError, match="dtype"):
        T.CropPool(fx.z["items_eval"], device="cpu", dtype=torch.float16)


# ---------------------------------------------------------------------------------------------------------------------
# the order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_epoch_order_is_a_permutation(n):
    from deeptreeattention_amd import treedata as T
    o = T.epoch_order_np(n, epoch=3, seed=5, level=2)
    assert o.dtype == np.int32 and o.shape == (n,) and np.array_equal(np.sort(o), np.arange(n))
    assert np.array_equal(o, T.epoch_order_np(n, 3, 5, 2))                                 # a pure function
    assert np.array_equal(T.epoch_order_np(n, 2 ** 64 + 3, 5, 2), o) and np.array_equal(T.epoch_order_np(n, 3, 2 ** 64 + 5, 2), o)
    if n >= 63:
        others = [T.epoch_order_np(n, 4, 5, 2), T.epoch_order_np(n, 3, 6, 2), T.epoch_order_np(n, 3, 5, 3), T.epoch_order_np(n, 3, 5, 0)]
        assert all(not np.array_equal(o, x) for x in others) and not np.array_equal(o, np.arange(n))
        assert len({tuple(x.tolist()) for x in others}) == 4


def test_epoch_order_is_the_documented_hash():
    from deeptreeattention_amd import abundance, treedata as T
    M = (1 << 64) - 1
    for n, epoch, seed, level in ((7, 2 ** 63 + 11, 5, 0), (13, 3, 2 ** 40, 4), (1, 0, 0, 63)):
        keys = []
        for i in range(n):
            z = (((epoch * n + i) & M) * 0x9E3779B97F4A7C15 + abundance.stream_key(seed, 16 + level)) & M
            keys.append((abundance._mix_int(z) >> 32, i))
        assert T.epoch_order_np(n, epoch, seed, level).tolist() == [i for _, i in sorted(keys)]
    # the stream ids are ones abundance (0, 1) and split (0) do not use
    assert T.ORDER_STREAM == 16 and T.MAX_LEVEL_ID == 64 and T.MAX_N == 1 << 20
    for bad in ({"n": 0}, {"n": 5, "level": -1}, {"n": 5, "level": 64}):
        with pytest.raises(ValueError):
            T.epoch_order_np(**bad)


# ---------------------------------------------------------------------------------------------------------------------
# the batch plan
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_plan_against_the_hand_written_table():
    from deeptreeattention_amd import treedata as T
    nb, steps = T.plan(TC.PLAN_SIZES, TC.PLAN_B)
    assert nb == TC.PLAN_NB and steps == TC.PLAN_STEPS
    for s, row in enumerate(TC.PLAN_TABLE):
        assert [T.step_positions(n, k, TC.PLAN_B, s) for n, k in zip(TC.PLAN_SIZES, nb)] == row
    # the cycling is loop.fit_multistage's b[i % len(b)] over lists of batches
    for n, k in zip(TC.PLAN_SIZES, nb):
        chunks = [(lo, min(lo + TC.PLAN_B, n) - lo) for lo in range(0, n, TC.PLAN_B)]
        assert [T.step_positions(n, k, TC.PLAN_B, s) for s in range(steps)] == [chunks[s % len(chunks)] for s in range(steps)]
    nb, steps = T.plan(TC.PLAN_DROP_SIZES, TC.PLAN_B, drop_last=True)
    assert nb == TC.PLAN_DROP_NB and steps == TC.PLAN_DROP_STEPS
    for s, row in enumerate(TC.PLAN_DROP_TABLE):
        assert [T.step_positions(n, k, TC.PLAN_B, s) for n, k in zip(TC.PLAN_DROP_SIZES, nb)] == row
    with pytest.raises(ValueError, match="no batch of 64 with drop_last"):
        T.plan(TC.PLAN_SIZES, TC.PLAN_B, drop_last=True)
    assert T.plan([64], 64, drop_last=True) == ([1], 1) and T.plan([1], 64) == ([1], 1)
    with pytest.raises(ValueError, match="batch_size"):
        T.plan([5], 0)
    with pytest.raises(ValueError, match="empty"):
        T.plan([5, 0], 4)


# ---------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------
def small_pool(n=10, years=3, device="cpu"):
    from deeptreeattention_amd import treedata as T
    crops, present = TC.synthetic_crops(n, years, 2, 3, seed=1)
    return T.CropPool(crops, present=present, device=device)


def test_views_refuse_rows_outside_the_pool_and_bad_tables():
    from deeptreeattention_amd import treedata as T
    pool = small_pool()
    pool.view([0, 9, 3], [1, 2, 3])
    for rows in ([0, 10], [-1, 2], [], [0.5, 1.0]):
        with pytest.raises(ValueError, match="rows"):
            pool.view(rows)
    with pytest.raises(ValueError, match="labels"):
        pool.view([0, 1], [1])
    with pytest.raises(ValueError, match="level"):
        pool.view([0], level=64)
    with pytest.raises(ValueError, match="present"):
        T.CropPool(np.zeros((4, 2, 3, 5, 5), np.float32), present=np.ones((4, 3)), device="cpu")
    with pytest.raises(ValueError, match=r"\[N\]\[Y\]\[C\]\[S\]\[S\]"):
        T.CropPool(np.zeros((4, 2, 3, 5, 6), np.float32), device="cpu")
    with pytest.raises(ValueError, match="one name per individual"):
        T.CropPool(np.zeros((4, 2, 3, 5, 5), np.float32), individuals=["a"], device="cpu")


def test_the_wrappers_check_everything_before_the_library_is_reached(monkeypatch):
    """More levels or networks than the limits, nb_l == 0 under drop_last, an n above the stated bound and a pool that is
    not on a ROCm device: all refused before _lib.lib() is reached."""
    torch = pytest.importorskip("torch")
    from deeptreeattention_amd import _lib, treedata as T

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    pool = small_pool()                                        # 3 years
    v = pool.view(np.arange(10), np.arange(10))
    with pytest.raises(ValueError, match="at most 8 levels"):
        T.LevelViews([v] * 9)
    with pytest.raises(ValueError, match="at most 16 networks"):
        T.LevelViews([v] * 6)                                  # 6 x 3 = 18 networks
    with pytest.raises(ValueError, match="same pool"):
        T.LevelViews([v, small_pool().view([0])])
    with pytest.raises(ValueError, match="at least one level"):
        T.LevelViews([])
    levels = T.LevelViews([v, pool.view([1, 2, 3])])
    assert [x.level for x in levels] == [0, 1] and v.level == 0 and len(levels) == 2 and levels[1].rows_np.tolist() == [1, 2, 3]
    assert levels.steps(4) == 3 and levels.steps(3, drop_last=True) == 3
    with pytest.raises(ValueError, match="no batch of 4 with drop_last"):
        next(levels.batches(4, drop_last=True))                # the second level has 3 entries
    with pytest.raises(ValueError, match="batch_size"):
        next(levels.batches(0))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        next(levels.batches(4))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        next(v.loader(4))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        T.CropPool.from_raw([[np.zeros((3, 2, 2), np.float32)]], device="cpu")
    with pytest.raises(ValueError, match="at least one crop"):
        T.CropPool.from_raw([[None, None]], device="cpu")
    # an n above the bound: a view of 2^20 + 1 entries may exist and be read in order, but not shuffled
    big = pool.view(np.zeros(T.MAX_N + 1, np.int64))
    with pytest.raises(ValueError, match="at most 1048576 entries"):
        next(big.loader(64, shuffle=True))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        next(big.loader(64, shuffle=False))


def test_the_step_refuses_present_together_with_year_flags():
    torch = pytest.importorskip("torch")
    from deeptreeattention_amd import engine

    class Level:
        years = [None, None]
        device = torch.device("cpu")
    tr = object.__new__(engine.MultiStageTrainer)
    tr.levels = [Level(), Level()]
    batch = [None, None]
    with pytest.raises(ValueError, match="not both"):
        tr.training_step_all(batch, 0, present=[[True, True]] * 2, year_flags=torch.ones(4))
    for bad in (torch.ones(3), torch.ones(4, dtype=torch.float64), np.ones(4, np.float32), torch.ones(8)[::2]):
        with pytest.raises(ValueError, match="year_flags must be"):
            tr.training_step_all(batch, 0, year_flags=bad)


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
    import deeptreeattention_amd as pkg
    from deeptreeattention_amd import _lib, build, treedata
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert {"dta_epoch_order", "dta_pool_batches"} <= names
    for n, nargs in (("dta_epoch_order", 7), ("dta_pool_batches", 12)):
        assert hasattr(lib, n) and '"%s"' % n in entry
        assert len(getattr(lib, n).argtypes) == nargs and getattr(lib, n).restype is C.c_int
    assert "treedata.hip" in build.SOURCES
    for name, value in (("DTA_EPOCH_ORDER_MAX_N", _lib.EPOCH_ORDER_MAX_N), ("DTA_EPOCH_ORDER_STREAM", _lib.EPOCH_ORDER_STREAM),
                        ("DTA_EPOCH_ORDER_MAX_LEVEL_ID", _lib.EPOCH_ORDER_MAX_LEVEL_ID), ("DTA_MAX_LEVELS", _lib.MAX_LEVELS),
                        ("DTA_MAX_YEARS", _lib.MAX_YEARS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == value, name
    assert (treedata.MAX_N, treedata.ORDER_STREAM, treedata.MAX_LEVEL_ID) == (1 << 20, 16, 64)
    # dta_pool_level as the header lays it out: 3 pointers, 2 long long, 2 int, 2 pointers
    assert C.sizeof(_lib.PoolLevel) == 64 and _lib.PoolLevel.count.offset == 40 and _lib.PoolLevel.out_rows.offset == 56
    assert pkg.CropPool is treedata.CropPool and pkg.LevelViews is treedata.LevelViews and "CropPool" in pkg.__all__
    assert lib.dta_abi_version() == 2


def test_epoch_order_refuses_bad_arguments_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the tables are host buffers nobody touches."""
    buf = (C.c_ubyte * 4096)()
    p = (C.addressof(buf) + 15) & ~15

    def call(levels=2, n=(5, 9), ids=None, orders=(p, p), null_n=False, null_orders=False):
        n_a = None if null_n else (C.c_longlong * len(n))(*n)
        ids_a = None if ids is None else (C.c_int * len(ids))(*ids)
        o_a = None if null_orders else (C.c_void_p * len(orders))(*orders)
        return lib.dta_epoch_order(levels, n_a, ids_a, 3, 1, o_a, None)

    cases = (({"null_n": True}, "null argument"), ({"null_orders": True}, "null argument"), ({"levels": 0}, "levels=0"),
             ({"levels": 9, "n": (1,) * 9, "orders": (p,) * 9}, "levels=9"), ({"n": (5, 0)}, "n=0 (level 1)"),
             ({"n": (-1, 5)}, "n=-1 (level 0)"), ({"n": (5, (1 << 20) + 1)}, "n=1048577 (level 1)"),
             ({"orders": (p, None)}, "null order table (level 1)"), ({"ids": (0, 64)}, "level id 64"), ({"ids": (-1, 0)}, "level id -1"))
    for kw, what in cases:
        assert call(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_epoch_order: ") and what in err, (kw, err)


def test_pool_batches_refuses_bad_arguments_before_any_launch(lib):
    from deeptreeattention_amd import _lib
    buf = (C.c_ubyte * 4096)()
    p = (C.addressof(buf) + 15) & ~15

    def level(**kw):
        d = dict(order=None, rows=p, labels=p, n=10, start=0, count=4, flip=0, out_labels=p, out_rows=p)
        d.update(kw)
        return _lib.PoolLevel(*[d[k] for k in ("order", "rows", "labels", "n", "start", "count", "flip", "out_labels", "out_rows")])

    def call(pool=p, dtype=0, pool_rows=10, years=3, bands=6, size=11, levels=2, lv=None, outs=None, flags=p, null_lv=False,
             null_outs=False):
        lv = [level(), level()] if lv is None else lv
        outs = [p] * (levels * years) if outs is None else outs
        lv_a = None if null_lv else (_lib.PoolLevel * len(lv))(*lv)
        o_a = None if null_outs else (C.c_void_p * len(outs))(*outs)
        return lib.dta_pool_batches(pool, dtype, pool_rows, years, bands, size, levels, lv_a, o_a, flags, None, None)

    cases = (({"pool": None}, "null argument"), ({"null_lv": True}, "null argument"), ({"null_outs": True}, "null argument"),
             ({"flags": None}, "null argument"), ({"dtype": 2}, "dtype=2"), ({"levels": 0}, "levels=0"),
             ({"levels": 9, "years": 1, "lv": [level()] * 9}, "levels=9"),
             ({"levels": 6, "lv": [level()] * 6}, "levels=6 x years=3: at most 16 networks"), ({"years": 0}, "years=0"),
             ({"pool_rows": 0}, "pool_rows=0"), ({"bands": 0}, "bands=0"), ({"size": 0}, "size=0"), ({"size": 4097}, "size=4097"),
             ({"bands": 65536, "size": 4096}, "more than 2^31 - 1 floats"),
             ({"lv": [level(), level(rows=None)]}, "null rows or out_rows (level 1)"),
             ({"lv": [level(out_rows=None), level()]}, "null rows or out_rows (level 0)"),
             ({"lv": [level(labels=None), level()]}, "labels and out_labels go together (level 0)"),
             ({"lv": [level(), level(out_labels=None)]}, "labels and out_labels go together (level 1)"),
             ({"lv": [level(n=0), level()]}, "n=0 (level 0)"), ({"lv": [level(start=-1), level()]}, "start=-1"),
             ({"lv": [level(count=0), level()]}, "count=0"), ({"lv": [level(), level(start=7)]}, "start=7, count=4, n=10 (level 1)"),
             ({"outs": [p] * 5 + [None]}, "out of level 1, year 2 is null"), ({"outs": [p, p + 4] + [p] * 4}, "out of level 0, year 1"))
    for kw, what in cases:
        assert call(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_pool_batches: ") and what in err, (kw, err)


def test_the_treedata_kernels_have_no_private_segment(tmp_path):
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
            if name and seg and ("k_epoch_order" in name.group(1) or "k_pool_batches" in name.group(1)):
                found[name.group(1)] = int(seg.group(1))
    assert len(found) == 3 and all(v == 0 for v in found.values()), found
