"""Reflectance cube to resident raster, host side (no GPU): the NumPy definitions of deeptreeattention_amd/reflectance.py
against what the reference's own generate_raster / calc_clip_index produced (tests/golden/reflectance, made by
tools/make_reflectance_golden.py) and against oracle.preprocess_np, which tests/golden/preprocess.npz pins to the
reference's preprocess_image; the argument errors; the C entry's refusals, none of which reaches a launch."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from oracle import preprocess_np as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "reflectance")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "reflectance_reference.npz")))


def test_fixture_checksums_match():
    lines = open(os.path.join(GOLDEN, "SHA256SUMS")).read().split("\n")
    lines = [ln for ln in lines if ln.strip()]
    assert len(lines) == 1
    for ln in lines:
        digest, name = ln.split()
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == digest
    assert os.path.getsize(os.path.join(GOLDEN, "reflectance_reference.npz")) < 256 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# the band lists
# ---------------------------------------------------------------------------------------------------------------------
def test_band_index_no_water_is_the_references_mask(gold):
    from deeptreeattention_amd import reflectance as R
    idx = R.band_index("no_water")
    assert idx.dtype == np.int32 and idx.shape == (369,)
    assert np.array_equal(idx, np.concatenate([np.arange(0, 192), np.arange(210, 283), np.arange(315, 419)]))
    assert np.array_equal(idx, gold["bands_no_water"])
    assert np.array_equal(R.band_index(), idx) and np.array_equal(R.band_index("no_water", 426), idx)


def test_band_index_other_forms_and_refusals():
    from deeptreeattention_amd import reflectance as R
    assert np.array_equal(R.band_index("all"), np.arange(426)) and R.band_index("all").dtype == np.int32
    assert np.array_equal(R.band_index("all", 30), np.arange(30))
    assert R.band_index("false_color").tolist() == [16, 54, 112]
    given = [5, 0, 22, 5, 5, 3]
    assert R.band_index(given, 23).tolist() == given and R.band_index(np.array(given), 23).dtype == np.int32
    assert R.band_index((0,), 1).tolist() == [0]
    for bad, src in (([0, 23], 23), ([-1, 2], 23), ("no_water", 400), ("false_color", 100), ([426], 426)):
        with pytest.raises(ValueError, match="outside"):
            R.band_index(bad, src)
    for bad in ("water", [], [[1, 2]], [0.5, 1.0]):
        with pytest.raises(ValueError, match="bands"):
            R.band_index(bad, 23)
    with pytest.raises(ValueError, match="bands_src"):
        R.band_index("all", 0)


def test_selected_bands_applies_the_clip_rule():
    from deeptreeattention_amd import reflectance as R
    from deeptreeattention_amd.preprocess import out_bands
    nw = R.band_index("no_water")
    assert np.array_equal(R.selected_bands("no_water", 426, 10), nw[10:-10]) and len(nw[10:-10]) == out_bands(369, 10) == 349
    assert np.array_equal(R.selected_bands("no_water", 426, 0), nw)
    assert R.selected_bands("false_color", 426, 10).tolist() == [16, 54, 112]               # three bands: no clip
    assert R.selected_bands([4, 4, 1], 23, 10).tolist() == [4, 4, 1]
    assert R.selected_bands("all", 30, 10).tolist() == list(range(10, 20))
    with pytest.raises(ValueError, match="nothing"):
        R.selected_bands("all", 20, 10)
    with pytest.raises(ValueError, match="clip"):
        R.selected_bands("all", 30, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the clip window
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_index_equals_the_reference_including_ties(gold):
    from deeptreeattention_amd import reflectance as R
    ext = tuple(gold["extent"].tolist())
    x_min, x_max, y_min, y_max = ext
    as_dict = {"xMin": x_min, "xMax": x_max, "yMin": y_min, "yMax": y_max}
    full = (x_min, y_min, x_max, y_max)
    for extent in (ext, as_dict):
        assert R.clip_index(full, extent) == tuple(gold["index_full"].tolist()) == (0, 0, 7, 9)
        assert R.clip_index(gold["bounds_a"], extent) == tuple(gold["index_a"].tolist()) == (0, 0, 6, 6)
        assert R.clip_index(gold["bounds_b"], extent) == tuple(gold["index_b"].tolist()) == (2, 2, 4, 8)
    assert all(type(v) is int for v in R.clip_index(gold["bounds_a"], ext))
    # every index of both cases is a .5 tie, resolved to the even integer
    for b in (gold["bounds_a"], gold["bounds_b"]):
        assert all((v - o) % 1 == 0.5 for v, o in zip(b, (x_min, y_min, x_min, y_min)))
    # scales divide the offsets only, as in the reference: the rows are counted down from the extent's height, 7, so
    # row0 = round(7 - 7 / 2) = round(3.5) = 4, row1 = round(7 - 0 / 2) = 7; col1 = round(9 / 2) = round(4.5) = 4
    assert R.clip_index(full, ext, xscale=2, yscale=2) == (4, 0, 7, 4)


# ---------------------------------------------------------------------------------------------------------------------
# the normalised raster
# ---------------------------------------------------------------------------------------------------------------------
CASES = (("full", None), ("a", "index_a"), ("b", "index_b"))


@pytest.mark.parametrize("name,index", CASES)
def test_reflectance_np_equals_generate_raster_then_the_oracle(gold, name, index):
    from deeptreeattention_amd import reflectance as R
    cube = gold["cube"]
    assert cube.shape == (7, 9, 426) and cube.dtype == np.int16
    window = None if index is None else tuple(gold[index].tolist())
    captured = gold["raster_" + name]                                  # [h][w][369], what the reference handed its writer
    band_first = np.ascontiguousarray(np.moveaxis(captured, 2, 0))
    got0 = R.reflectance_np(cube, "no_water", window, clip=0)
    assert got0.dtype == np.float32 and got0.shape == band_first.shape
    assert np.array_equal(got0, O.minmax_over_bands(band_first))
    got10 = R.reflectance_np(cube, "no_water", window, clip=10)
    assert got10.shape == (349,) + band_first.shape[1:]
    assert np.array_equal(got10, O.preprocess_image(band_first))
    assert np.array_equal(R.reflectance_np(cube, window=window), got10)            # the defaults


def test_reflectance_np_on_other_cubes_equals_the_oracle():
    from deeptreeattention_amd import reflectance as R
    rng = np.random.default_rng(5)
    cube = rng.integers(-200, 9000, (4, 21, 23)).astype(np.int16)
    cube[1, 2] = -9999                                                              # nodata takes part in the min-max
    sel = [5, 0, 22, 5, 5, 3, 17, 9]
    want = O.minmax_over_bands(np.moveaxis(cube[1:4, 3:20][:, :, sel], 2, 0))
    assert np.array_equal(R.reflectance_np(cube, sel, (1, 3, 4, 20), clip=0), want)
    assert np.array_equal(R.reflectance_np(cube, sel, (1, 3, 4, 20), clip=2), O.minmax_over_bands(np.moveaxis(cube[1:4, 3:20][:, :, sel[2:-2]], 2, 0)))
    u8 = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    assert np.array_equal(R.reflectance_np(u8, "all"), O.preprocess_image(np.moveaxis(u8, 2, 0)))        # three bands: no clip
    f = rng.standard_normal((3, 17, 40)).astype(np.float32)
    f[0, 1, 3:9] = np.nan
    f[1, 4] = np.nan
    f[2, 5] = 0.25
    got = R.reflectance_np(f, "all")
    assert np.array_equal(got, O.preprocess_image(np.moveaxis(f, 2, 0)), equal_nan=True)
    assert np.isnan(got[:, 1, 4]).all() and not got[:, 2, 5].any() and np.isnan(got[:, 0, 1]).sum() == 0     # its NaN bands, 3-8, are clipped
    assert np.isnan(R.reflectance_np(f, "all", clip=0)[:, 0, 1]).sum() == 6


def test_window_clamps_above_and_refuses_below_and_empty():
    from deeptreeattention_amd import reflectance as R
    cube = np.random.default_rng(6).integers(0, 5000, (4, 21, 23)).astype(np.int16)
    whole = R.reflectance_np(cube, "all", clip=0)
    assert np.array_equal(R.reflectance_np(cube, "all", (0, 0, 99, 99), clip=0), whole)
    assert np.array_equal(R.reflectance_np(cube, "all", (2, 5, 400, 22), clip=0), whole[:, 2:, 5:22])
    assert R.window_of(cube.shape, None) == (0, 0, 4, 21) and R.window_of(cube.shape, (1, 3, 4, 20)) == (1, 3, 4, 20)
    assert R.window_of(cube.shape, np.array([1, 3, 9, 50])) == (1, 3, 4, 21)
    for bad in ((-1, 0, 3, 3), (0, -2, 3, 3), (0, 0, -1, 3), (1, 1, 3, -3)):
        with pytest.raises(ValueError, match="negative"):
            R.reflectance_np(cube, "all", bad)
    for bad in ((2, 0, 2, 5), (3, 0, 1, 5), (0, 7, 3, 7), (4, 0, 9, 5), (0, 21, 3, 30)):
        with pytest.raises(ValueError, match="empty"):
            R.reflectance_np(cube, "all", bad)
    with pytest.raises(ValueError, match="window"):
        R.reflectance_np(cube, "all", (1, 2, 3))
    with pytest.raises(ValueError, match="3-d"):
        R.reflectance_np(cube[0], "all")


def test_from_reflectance_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached."""
    from deeptreeattention_amd import _lib, dense

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    cube = np.zeros((4, 21, 23), np.int16)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dense.DenseRaster.from_reflectance(cube, "all", device="cpu")


def test_launch_plan_keeps_the_lds_stride_odd_and_inside_the_budget():
    from deeptreeattention_amd import reflectance as R
    assert R.launch_plan(426, 2, 1000) == (32, 852)            # 213 dwords: odd as it is
    assert R.launch_plan(426, 4, 1000) == (16, 1708)           # 426 dwords are even: one more
    for bands in (1, 2, 3, 23, 30, 64, 128, 426, 1023, 1024):
        for itemsize in (1, 2, 4):
            for cols in (1, 5, 37, 300, 5000):
                pixels, stride = R.launch_plan(bands, itemsize, cols)
                assert stride % 4 == 0 and (stride // 4) % 2 == 1 and bands * itemsize <= stride <= bands * itemsize + 7
                assert pixels in (8, 16, 32, 64, 128, 256) and (pixels == 8 or pixels * stride <= R.STAGE_BYTES)
                assert pixels * stride + 4 * R.MAX_BANDS + 2048 <= 48 * 1024
                assert pixels == 8 or pixels // 2 < cols


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, bound, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbol_is_declared_exported_and_bound(lib):
    from deeptreeattention_amd import _lib, build, reflectance
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    name = "dta_reflectance_normalise"
    assert name in names and hasattr(lib, name) and '"{}"'.format(name) in entry
    assert len(getattr(lib, name).argtypes) == 6 and getattr(lib, name).restype is C.c_int
    assert "reflectance.hip" in build.SOURCES
    assert int(re.search(r"#define\s+DTA_REFLECTANCE_MAX_BANDS\s+(\d+)", hdr).group(1)) == _lib.REFLECTANCE_MAX_BANDS == reflectance.MAX_BANDS
    struct = re.search(r"typedef struct dta_reflectance_desc \{(.*?)\} dta_reflectance_desc;", hdr, re.S).group(1)
    fields = re.findall(r"\b([a-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", struct))
    assert fields == [f[0] for f in _lib.ReflectanceDesc._fields_] and C.sizeof(_lib.ReflectanceDesc) == 4 * len(fields)
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the pointers are host buffers nobody dereferences."""
    from deeptreeattention_amd import _lib
    buf = (C.c_ubyte * 96)()
    base = C.addressof(buf)
    p = C.c_void_p(base + (-base) % 16)
    odd = C.c_void_p(p.value + 8)
    who = "dta_reflectance_normalise"

    def err():
        return lib.dta_last_error().decode()

    def call(strip=p, index=p, bands=10, out=p, desc=True, **kw):
        f = dict(bands_src=30, width_src=40, rows=3, col0=2, cols=30, dtype=_lib.CROP_I16, tiles=0, out_height=5, out_row0=1)
        f.update(kw)
        d = _lib.ReflectanceDesc(**f) if desc else None
        return lib.dta_reflectance_normalise(d, strip, index, bands, out, None)

    for kw, what in (({"desc": False}, "d"), ({"strip": None}, "strip"), ({"index": None}, "band_index"), ({"out": None}, "out")):
        assert call(**kw) != 0 and who in err() and "null" in err() and err().endswith(": " + what), (kw, err())
    for kw, what in (({"bands_src": 0}, "bands_src=0"), ({"width_src": 0}, "width_src=0"), ({"rows": 0}, "rows=0"), ({"rows": -2}, "rows=-2"),
                     ({"cols": 0}, "cols=0"), ({"out_height": 0}, "out_height=0"), ({"bands": 0}, "bands=0"), ({"bands": -1}, "bands=-1"),
                     ({"col0": -1}, "col0=-1"), ({"col0": 11}, "width_src=40"), ({"cols": 39}, "cols=39"),
                     ({"col0": 2 ** 31 - 1, "cols": 2 ** 31 - 1, "width_src": 2 ** 31 - 1}, "col0="),
                     ({"out_row0": -1}, "out_row0=-1"), ({"out_row0": 3}, "out_height=5"), ({"rows": 5}, "rows=5"),
                     ({"dtype": 3}, "dtype=3"), ({"dtype": -1}, "dtype=-1"),
                     ({"out_height": 2 ** 16, "cols": 2 ** 15, "width_src": 2 ** 15 + 2}, "int32"),
                     ({"bands_src": _lib.REFLECTANCE_MAX_BANDS + 1}, "bands_src=1025"), ({"bands": _lib.REFLECTANCE_MAX_BANDS + 1}, "bands=1025"),
                     ({"strip": odd}, "strip is not 16-byte aligned"), ({"out": odd}, "out is not 16-byte aligned"),
                     ({"out": odd, "tiles": 1}, "out is not 16-byte aligned")):
        assert call(**kw) != 0 and who in err() and what in err(), (kw, err())
    # one below the raster limit passes the size check and is refused for what comes next
    assert call(out_height=2 ** 16, cols=2 ** 15 - 1, width_src=2 ** 15 + 2, bands=1025) != 0 and "bands=1025" in err()
