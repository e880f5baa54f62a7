"""Crown height filter, host side (no GPU): the NumPy definition (canopy.crown_height_np / min_height_np / height_rules_np)
against the reference's own results (tests/golden/canopy/canopy_reference.npz, tools/make_canopy_golden.py), against
np.nanpercentile and against a scalar restatement; clipping; the C entry's refusals, none of which reaches a launch; the
Python route's host-side argument checks."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODATA = np.float32(-9999.0)


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def scalar_height(values, q, floor=0.5):
    """The issue's definition with sorted() and Python control flow; every operation is a np.float32 one."""
    f32 = np.float32
    kept = sorted(float(v) for v in values if f32(v) >= f32(floor))      # NaN >= floor is False
    n = len(kept)
    if n == 0:
        return f32(np.nan), 0
    virt = f32(n - 1) * (f32(q) / f32(100))
    lo = int(math.floor(float(virt)))
    t = virt - f32(lo)
    hi = min(lo + 1, n - 1)
    a, b = f32(kept[lo]), f32(kept[hi])
    d = b - a
    if t >= f32(0.5):
        return f32(b - d * (f32(1) - t)), n
    return f32(a + d * t), n


def special_raster(rng, H, W, ties=True):
    """Heights in 0.5-35 m with NaN, nodata and sub-floor cells sprinkled in, and a quarter rounded to 0.1 m (ties)."""
    chm = rng.uniform(0.5, 35.0, (H, W)).astype(np.float32)
    if ties:
        chm[:H // 2, :W // 2] = np.round(chm[:H // 2, :W // 2], 1)
    r = rng.random((H, W))
    chm[r < 0.03] = np.nan
    chm[(r >= 0.03) & (r < 0.06)] = NODATA
    chm[(r >= 0.06) & (r < 0.12)] = rng.uniform(0.0, 0.49, int(((r >= 0.06) & (r < 0.12)).sum())).astype(np.float32)
    return chm


def random_boxes(rng, N, H, W, max_side=12, margin=0):
    r0 = rng.integers(-margin, H + margin, N)
    c0 = rng.integers(-margin, W + margin, N)
    return np.stack([r0, c0, r0 + rng.integers(1, max_side + 1, N), c0 + rng.integers(1, max_side + 1, N)], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture the reference made
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(golden):
    g = golden(os.path.join("canopy", "canopy_reference.npz"))
    return {k: g[k] for k in g.files}


def test_fixture_is_the_committed_one():
    """tests/golden/canopy has a checksum file of its own (tests/golden/SHA256SUMS lists the fixtures directly in
    tests/golden): the file is the one tools/make_canopy_golden.py wrote from the reference."""
    import hashlib
    here = os.path.join(REPO, "tests", "golden", "canopy")
    lines = [ln.split() for ln in open(os.path.join(here, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert [name for _, name in lines] == sorted(f for f in os.listdir(here) if f.endswith(".npz")) == ["canopy_reference.npz"]
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(here, name), "rb").read()).hexdigest() == digest, name


def test_fixture_is_the_documented_one(fixture):
    chm, boxes, kept = fixture["chm"], fixture["boxes"], fixture["kept"]
    assert chm.dtype == np.float32 and chm.shape == (48, 56) and boxes.dtype == np.int32 and boxes.shape[1] == 4
    assert fixture["ref_q99"].dtype == np.float32 and fixture["ref_q99"].shape == (len(boxes),) == kept.shape
    with np.errstate(invalid="ignore"):
        assert np.isnan(chm).any() and (chm == NODATA).any() and not (chm[30:41, :13] >= 0.5).any()      # nothing kept there
    ties = chm[:19, :23]
    assert same_bits(ties[ties >= 0.5], np.round(ties[ties >= 0.5], 1))
    assert (boxes[:, :2] >= 0).all() and (boxes[:, 2] <= 48).all() and (boxes[:, 3] <= 56).all()
    assert (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()
    assert {0, 1, 2, 3, 100, 101, 102, 201} <= set(kept.tolist()) and len(set(kept.tolist())) >= 12
    # at 101 and 201 kept values the weight t is exactly 0, at 100 and 102 it is not
    for n, zero in ((101, True), (201, True), (100, False), (102, False)):
        virt = np.float32(n - 1) * (np.float32(99) / np.float32(100))
        assert (virt == np.floor(virt)) == zero, n
    # ties fall on the lo / hi ranks: some box of the tie region has equal lo-th and hi-th values away from the ends
    tied = 0
    for b, n in zip(boxes, kept):
        v = chm[b[0]:b[2], b[1]:b[3]]
        with np.errstate(invalid="ignore"):
            s = np.sort(v[v >= 0.5])
        if n >= 50:
            lo = int(np.floor(np.float32(n - 1) * (np.float32(99) / np.float32(100))))
            tied += int(s[lo] == s[min(lo + 1, n - 1)] and lo + 1 <= n - 1)
    assert tied >= 1
    ch, fh = fixture["chm_height"], fixture["field_height"]
    assert ch.dtype == np.float32 and fh.dtype == np.float64 and ch.shape == fh.shape
    assert fixture["ref_keep_default"].dtype == bool and fixture["ref_keep_other"].dtype == bool
    both = np.isnan(ch) & np.isnan(fh)
    assert both.any() and (np.isnan(ch) & ~np.isnan(fh)).any() and (~np.isnan(ch) & np.isnan(fh)).any()
    d = ch.astype(np.float64) - fh
    assert (d == 0).any() and (d == 4).any() and (d == -8).any() and (d == 2.5).any() and (d == -5).any()
    one = np.float32(1)
    assert (ch == one).any() and (ch == np.nextafter(one, np.float32(0))).any() and (ch == np.nextafter(one, np.float32(2))).any()
    assert fixture["other"].tolist() == [2.0, 2.5, 5.0]


def test_crown_height_np_equals_the_reference(fixture):
    from deeptreeattention_amd import canopy
    height, count = canopy.crown_height_np(fixture["chm"], fixture["boxes"])
    assert height.dtype == np.float32 and count.dtype == np.int32
    assert same_bits(height, fixture["ref_q99"])
    assert np.array_equal(count, fixture["kept"])
    assert np.isnan(height[count == 0]).all() and not np.isnan(height[count > 0]).any()


def test_rules_equal_the_reference(fixture):
    from deeptreeattention_amd import canopy
    ch, fh = fixture["chm_height"], fixture["field_height"]
    got = canopy.height_rules_np(ch, fh)
    assert got.dtype == bool and np.array_equal(got, fixture["ref_keep_default"])
    assert np.array_equal(canopy.height_rules_np(ch, fh, *fixture["other"]), fixture["ref_keep_other"])
    assert np.array_equal(canopy.height_rules_np(ch, fh, *canopy.HeightRules()), fixture["ref_keep_default"])
    # the edge rows as the reference decided them: equal heights keep, a difference of exactly 4 or 8 drops, 7.9 keeps
    rows = {(float(c), float(f)): bool(k) for c, f, k in zip(ch, fh, fixture["ref_keep_default"]) if not (np.isnan(c) or np.isnan(f))}
    assert rows[(10.0, 10.0)] and not rows[(14.0, 10.0)] and not rows[(2.0, 10.0)] and rows[(float(np.float32(2.1)), 10.0)]
    # find_crowns' filter: NaN, 3.0 and the next float up
    up = np.nextafter(np.float32(3), np.float32(4))
    got = canopy.min_height_np(np.array([np.nan, 3.0, up, 0.0, np.inf], np.float32), 3.0)
    assert got.dtype == bool and got.tolist() == [False, False, True, False, True]
    assert canopy.min_height_np(np.array([3.0, up], np.float32)).tolist() == [False, True]       # the default is 3
    assert canopy.MinHeight().m == 3.0 and tuple(canopy.HeightRules()) == (1.0, 4.0, 8.0)


# ---------------------------------------------------------------------------------------------------------------------
# the definition against NumPy's percentile and against the scalar rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0, 50, 99, 100])
def test_crown_height_np_equals_nanpercentile_and_the_scalar_rule(q):
    from deeptreeattention_amd import canopy
    rng = np.random.default_rng(100 + q)
    chm = special_raster(rng, 40, 44)
    boxes = random_boxes(rng, 300, 40, 44, max_side=20, margin=3)
    height, count = canopy.crown_height_np(chm, boxes, q=q)
    ref = np.empty(len(boxes), np.float32)
    sca = np.empty(len(boxes), np.float32)
    for i, (r0, c0, r1, c1) in enumerate(boxes):
        v = chm[max(r0, 0):max(min(r1, 40), 0), max(c0, 0):max(min(c1, 44), 0)].reshape(-1)
        with np.errstate(invalid="ignore"):
            x = np.where(v >= np.float32(0.5), v, np.float32(np.nan))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                       # an empty or all-NaN slice
            got = np.nanpercentile(x, q) if x.size else np.float32(np.nan)
        assert np.asarray(got).dtype == np.float32
        ref[i] = got
        sca[i], n = scalar_height(v, q)
        assert n == count[i]
    assert (count == 0).any() and (count == 1).any() and (count > 100).any()
    assert same_bits(height, ref)
    assert same_bits(height, sca)


def test_clipping():
    from deeptreeattention_amd import canopy
    rng = np.random.default_rng(5)
    H, W = 21, 17
    chm = special_raster(rng, H, W, ties=False)
    whole = (0, 0, H, W)
    boxes = np.array([(-3, -2, 5, 6), (15, 10, 30, 40), (-5, 3, 4, 25), (18, -4, 99, 3),      # over each edge and corner
                      (-10, -10, 0, 5), (H, 0, H + 4, 4), (3, W, 9, W + 2), (3, -8, 9, 0),       # wholly outside: touching
                      (-2 ** 31, -2 ** 31, -5, -5), (2 ** 31 - 9, 2, 2 ** 31 - 1, 9),            # wholly outside: far away
                      (5, 5, 5, 9), (7, 3, 2, 9), (4, 9, 8, 9), (4, 9, 8, 1),                    # no rows / no columns
                      whole, (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)], np.int64).astype(np.int32)
    height, count = canopy.crown_height_np(chm, boxes)
    clipped = np.array([(0, 0, 5, 6), (15, 10, H, W), (0, 3, 4, W), (18, 0, H, 3)], np.int32)
    h2, c2 = canopy.crown_height_np(chm, clipped)
    assert same_bits(height[:4], h2) and np.array_equal(count[:4], c2) and (c2 > 0).all()
    assert (count[4:14] == 0).all() and np.isnan(height[4:14]).all()
    with np.errstate(invalid="ignore"):
        everything = chm[chm >= 0.5]
    for k in (14, 15):
        assert count[k] == everything.size and height[k] == canopy.quantile_of_kept(everything)
    r0, c0, rows, cols = canopy.clip_boxes(boxes, H, W)
    assert rows[:4].tolist() == [5, 6, 4, 3] and cols[:4].tolist() == [6, 7, 14, 3] and not (rows[4:14] * cols[4:14]).any()
    with pytest.raises(ValueError, match="boxes"):
        canopy.crown_height_np(chm, np.zeros((0, 4), np.int32))
    with pytest.raises(ValueError, match="boxes"):
        canopy.crown_height_np(chm, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="q must"):
        canopy.crown_height_np(chm, boxes, q=100.5)
    with pytest.raises(ValueError, match="floor"):
        canopy.crown_height_np(chm, boxes, floor=0.0)
    with pytest.raises(ValueError, match="2\\^24"):
        canopy.crown_height_np(np.zeros((4097, 4097), np.float32), np.array([[0, 0, 4097, 4097]], np.int32))


def test_float64_and_integer_rasters_are_converted_once():
    from deeptreeattention_amd import canopy
    rng = np.random.default_rng(6)
    chm = rng.uniform(0, 30, (9, 11))
    boxes = random_boxes(rng, 20, 9, 11, max_side=6)
    h64, c64 = canopy.crown_height_np(chm, boxes)
    h32, c32 = canopy.crown_height_np(chm.astype(np.float32), boxes)
    assert same_bits(h64, h32) and np.array_equal(c64, c32)
    hi, ci = canopy.crown_height_np((chm * 3).astype(np.int16), boxes)
    hf, cf = canopy.crown_height_np((chm * 3).astype(np.int16).astype(np.float32), boxes)
    assert same_bits(hi, hf) and np.array_equal(ci, cf)


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
    from deeptreeattention_amd import _lib, build, canopy
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    assert "dta_crown_height" in names and hasattr(lib, "dta_crown_height")
    assert "canopy.hip" in build.SOURCES
    assert len(lib.dta_crown_height.argtypes) == 13 and lib.dta_crown_height.restype is C.c_int
    assert [n for n, _ in _lib.HeightRule._fields_] == ["mode", "min_height", "min_chm", "max_diff", "limit"]
    assert C.sizeof(_lib.HeightRule) == 40                          # int, padding, four doubles: the C struct
    assert re.search(r"typedef struct \{\s*int mode;[^}]*double min_height;[^}]*double min_chm, max_diff, limit;[^}]*\} dta_height_rule;", hdr)
    cells = int(re.search(r"#define\s+DTA_CROWN_WAVE_CELLS\s+(\d+)", hdr).group(1))
    assert cells == _lib.CROWN_WAVE_CELLS == canopy.WAVE_CELLS and cells % 64 == 0
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert '"dta_crown_height"' in entry


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the pointers are host buffers nobody dereferences."""
    from deeptreeattention_amd import _lib
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)

    def err():
        return lib.dta_last_error().decode()

    def rule(mode):
        return C.byref(_lib.HeightRule(mode, 3.0, 1.0, 4.0, 8.0))

    def call(chm=p, height=10, width=10, boxes=p, n=4, q=99.0, floor=0.5, field=None, rule=None, out_height=p, out_count=p,
             out_keep=None):
        return lib.dta_crown_height(chm, height, width, boxes, n, q, floor, field, rule, out_height, out_count, out_keep, None)

    for kw in ({"chm": None}, {"boxes": None}, {"out_height": None}, {"out_count": None}):
        assert call(**kw) != 0 and "dta_crown_height" in err() and "null" in err(), kw
    for kw, what in (({"n": 0}, "n="), ({"n": -5}, "n="), ({"height": 0}, "height="), ({"width": 0}, "width="),
                     ({"height": -1}, "height="), ({"height": 65536, "width": 32768}, "int32"),
                     ({"height": 2 ** 31 - 1, "width": 2}, "int32"),
                     ({"q": -0.5}, "q="), ({"q": 100.5}, "q="), ({"q": float("nan")}, "q="), ({"q": float("inf")}, "q="),
                     ({"floor": 0.0}, "floor="), ({"floor": -1.0}, "floor="), ({"floor": float("nan")}, "floor="),
                     ({"rule": rule(2), "out_keep": p}, "field_height"),
                     ({"rule": rule(3), "out_keep": p}, "mode"), ({"rule": rule(-1), "out_keep": p}, "mode"),
                     ({"out_keep": p}, "without a rule"), ({"rule": rule(0), "out_keep": p}, "without a rule"),
                     ({"rule": rule(1)}, "without a keep buffer"), ({"rule": rule(2), "field": p}, "without a keep buffer")):
        assert call(**kw) != 0 and "dta_crown_height" in err() and what in err(), (kw, err())


def test_python_route_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached.  CanopyRaster.resident on a host tensor stands in for a
    resident raster: the checks are the same, and a call that passes them is refused for want of a device."""
    import torch
    from deeptreeattention_amd import _lib, canopy

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        canopy.CanopyRaster(np.zeros((4, 4), np.float32), device="cpu")
    with pytest.raises(ValueError, match="resident"):
        canopy.CanopyRaster.resident(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="non-empty"):
        canopy.CanopyRaster.resident(torch.zeros(4, dtype=torch.float32))
    ras = canopy.CanopyRaster.resident(torch.zeros(20, 30, dtype=torch.float32))
    assert ras.shape == (20, 30) and ras.height == 20 and ras.width == 30
    boxes = np.array([[0, 0, 4, 4], [2, 3, 9, 9], [5, 5, 6, 6]], np.int32)
    field = np.array([1.0, np.nan, 3.0])
    for bad in (boxes.astype(np.float32), boxes[:, :3], boxes[:0], torch.from_numpy(boxes).float(), [[0.5, 0, 4, 4]]):   # dtype / shape
        with pytest.raises(ValueError, match="boxes"):
            ras.crown_height(bad)
    with pytest.raises(ValueError, match="field_height"):                            # wrong dtype
        ras.crown_height(boxes, field_height=np.array([1, 2, 3], np.int64), rule=canopy.HeightRules())
    with pytest.raises(ValueError, match="field_height"):
        ras.crown_height(boxes, field_height=torch.from_numpy(field).to(torch.float16), rule=canopy.HeightRules())
    with pytest.raises(ValueError, match="field_height"):                            # wrong length
        ras.crown_height(boxes, field_height=field[:2], rule=canopy.HeightRules())
    with pytest.raises(ValueError, match="field_height"):                            # wrong device
        ras.crown_height(boxes, field_height=torch.empty(3, dtype=torch.float64, device="meta"), rule=canopy.HeightRules())
    with pytest.raises(ValueError, match="HeightRules needs field_height"):
        ras.crown_height(boxes, rule=canopy.HeightRules())
    with pytest.raises(ValueError, match="rule must be"):
        ras.crown_height(boxes, rule=(1, 4, 8))
    for q in (101, -1, float("nan")):
        with pytest.raises(ValueError, match="q must"):
            ras.crown_height(boxes, q=q)
    with pytest.raises(ValueError, match="floor"):
        ras.crown_height(boxes, floor=0)
    big = canopy.CanopyRaster.resident(torch.zeros(1, 1, dtype=torch.float32).expand(4097, 4097).contiguous())
    with pytest.raises(ValueError, match="2\\^24"):                                   # host boxes: refused here, not on the device
        big.crown_height(np.array([[0, 0, 4097, 4097]], np.int32))
    with pytest.raises(RuntimeError, match="ROCm device only"):                      # no fallback: a host raster computes nothing
        ras.crown_height(boxes, field_height=field, rule=canopy.HeightRules())
