"""Reflectance cube to resident raster on the device (dta_reflectance_normalise; dense.DenseRaster.from_reflectance) against
today's route -- select and transpose on the host, then DenseRaster -- and against the host definition
(reflectance.reflectance_np).  Every comparison is bit for bit: the kernel repeats k_raster_normalise's arithmetic, and a
band selection, a window and a transpose round nothing.  (float32 rasters are compared as their int32 bit patterns, so that a
NaN equals the same NaN.)

The cubes are the smallest that reach every path of the kernel: 426 int16 bands (852-byte pixels: 16-byte loads that start
anywhere, 4-byte staging units, 22 chunks with 13 live bands in the last), a row longer than one pixel run, an odd band count
(pixels on 2-byte boundaries only, 2-byte units, the strip's last 16-byte piece cut short), a column window that starts on an
odd pixel and stops before the row does, 3-byte uint8 pixels (1-byte units), and float32 with NaNs, an all-NaN pixel, a
constant pixel and a nodata pixel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ODD_LIST = [5, 0, 22, 5, 5, 3, 17, 9, 1, 22, 0, 11, 13, 2, 7, 19, 21, 4, 4, 16, 8]      # unsorted, repeating; 21 - 2 x 2 = 17 bands


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def cube(name):
    """The test cubes, made once and shared (nobody writes into them)."""
    rng = np.random.default_rng({"neon": 1, "long": 2, "odd": 3, "u8": 4, "f32": 5}[name])
    if name == "neon":
        a = rng.integers(-300, 12000, (5, 37, 426)).astype(np.int16)
        a[2, 11] = -9999
    elif name == "long":
        a = rng.integers(-300, 12000, (3, 300, 30)).astype(np.int16)
    elif name == "odd":
        a = rng.integers(-300, 12000, (4, 21, 23)).astype(np.int16)
    elif name == "u8":
        a = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    else:
        a = (rng.standard_normal((3, 17, 40)) * 1000).astype(np.float32)
        a[0, 1, 12:19] = np.nan                    # NaNs in some of the kept bands (10 .. 29) of some pixels
        a[1, 16, 29] = np.nan
        a[2, 0, 10] = np.nan
        a[1, 4] = np.nan                           # an all-NaN pixel
        a[2, 5] = 0.25                             # a constant pixel: range under `tiny`
        a[0, 9] = 1.0 + np.arange(40) * 1e-8       # ... and one whose range is not zero but under it
        a[2, 16] = -9999.0                         # nodata in every band
    a.setflags(write=False)
    return a


#        cube    bands      window           clip
CASES = {"neon": ("neon", "no_water", None, 10),
         "long": ("long", "all", None, 10),
         "odd": ("odd", ODD_LIST, None, 2),
         "odd_window": ("odd", ODD_LIST, (1, 3, 4, 20), 2),
         "u8": ("u8", "all", None, 10),
         "f32": ("f32", "all", None, 10)}


def bits(raster):
    return raster.data.view(torch.int32) if raster.precision == "fp32" else raster.data


def todays_route(case, precision):
    """Select and transpose on the host, then DenseRaster: what from_reflectance must equal bit for bit."""
    from deeptreeattention_amd import reflectance as R
    from deeptreeattention_amd.dense import DenseRaster
    name, bands, window, clip = CASES[case]
    c = cube(name)
    r0, c0, r1, c1 = R.window_of(c.shape, window)
    sel = R.band_index(bands, c.shape[2])
    band_first = np.ascontiguousarray(np.moveaxis(c[r0:r1, c0:c1][:, :, sel], 2, 0))
    return DenseRaster(band_first, clip=clip, precision=precision, device=dev())


def new_route(case, precision, **kw):
    from deeptreeattention_amd.dense import DenseRaster
    name, bands, window, clip = CASES[case]
    return DenseRaster.from_reflectance(cube(name), bands, window=window, clip=clip, precision=precision, device=dev(), **kw)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
def test_from_reflectance_equals_select_transpose_then_denseraster(case, precision):
    want = todays_route(case, precision)
    got = new_route(case, precision)
    assert got.shape == want.shape and (got.bands, got.height, got.width) == (want.bands, want.height, want.width)
    assert got.precision == want.precision == precision and got.device == want.device
    assert got.data.dtype == want.data.dtype and got.data.shape == want.data.shape
    assert torch.equal(bits(got), bits(want)), case
    expect = {"neon": (349, 5, 37), "long": (10, 3, 300), "odd": (17, 4, 21), "odd_window": (17, 3, 17), "u8": (3, 3, 5),
              "f32": (20, 3, 17)}[case]
    assert got.shape == expect


def test_fp32_raster_equals_the_definition_bit_for_bit():
    from deeptreeattention_amd import reflectance as R
    name, bands, window, clip = CASES["neon"]
    want = R.reflectance_np(cube(name), bands, window, clip)
    got = new_route("neon", "fp32").float().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the float32 cube, NaNs included
    name, bands, window, clip = CASES["f32"]
    want = R.reflectance_np(cube(name), bands, window, clip)
    got = new_route("f32", "fp32").float().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:, 1, 4]).all() and not got[:, 2, 5].any() and np.isnan(got[:, 0, 1]).sum() == 7
    assert got[:, 0, 9].max() < 1e-6 and not got[:, 2, 16].any()                   # range under `tiny`: scale 1; nodata: constant


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_strips_and_a_resident_cube_give_the_same_raster(precision):
    one = new_route("neon", precision)
    for rows in (2, 1, 5, 64):
        assert torch.equal(bits(new_route("neon", precision, strip_rows=rows)), bits(one)), rows
    from deeptreeattention_amd.dense import DenseRaster
    name, bands, window, clip = CASES["odd_window"]
    host = new_route("odd_window", precision, strip_rows=2)
    on_device = torch.from_numpy(np.array(cube(name))).to(dev())
    got = DenseRaster.from_reflectance(on_device, bands, window=window, clip=clip, precision=precision, device=dev())
    assert torch.equal(bits(got), bits(host))
    name, bands, window, clip = CASES["neon"]
    got = DenseRaster.from_reflectance(torch.from_numpy(np.array(cube(name))).to(dev()), bands, clip=clip, precision=precision,
                                       device=dev())
    assert torch.equal(bits(got), bits(one))
    with pytest.raises(ValueError, match="strip_rows"):
        new_route("neon", precision, strip_rows=0)


@pytest.mark.parametrize("tiles", [0, 1])
def test_a_strip_writes_its_rows_and_nothing_else(tiles):
    """The C entry on rows 2-3 of the 5-row cube, into a raster filled with a byte pattern: rows 0, 1 and 4 keep it."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd import reflectance as R
    L = _lib.lib()
    name, bands, window, clip = CASES["neon"]
    c = cube(name)
    H, W, B = c.shape
    sel = R.selected_bands(bands, B, clip)
    Cn, NC = len(sel), (len(sel) + 15) // 16
    whole = new_route("neon", "bf16" if tiles else "fp32")
    if tiles:
        out = torch.full((NC, H, W, 16), 0x5A5A, dtype=torch.int16, device=dev())
        want = whole.data.view(NC, H, W, 16)
        rows_of = lambda t, rows: t[:, rows]
    else:
        out = torch.full((Cn, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
        want = whole.data.view(torch.int32)
        rows_of = lambda t, rows: t[:, rows]
    before = out.clone()
    strip = torch.from_numpy(np.ascontiguousarray(c[2:4])).to(dev())
    index = torch.from_numpy(sel).to(dev())
    d = _lib.ReflectanceDesc(bands_src=B, width_src=W, rows=2, col0=0, cols=W, dtype=_lib.CROP_I16, tiles=tiles, out_height=H,
                             out_row0=2)
    _lib.check(L.dta_reflectance_normalise(d, _lib.ptr(strip), _lib.ptr(index), Cn, _lib.ptr(out), _lib.current_stream_ptr()),
               "dta_reflectance_normalise")
    torch.cuda.synchronize()
    assert torch.equal(rows_of(out, [0, 1, 4]), rows_of(before, [0, 1, 4]))
    assert torch.equal(rows_of(out, [2, 3]), rows_of(want, [2, 3]))


def test_crops_of_a_from_reflectance_raster_equal_the_definition():
    from deeptreeattention_amd import reflectance as R
    from deeptreeattention_amd.dense import gather_crops_np
    name, bands, window, clip = CASES["neon"]
    boxes = np.array([(0, 0, 5, 37), (1, 3, 4, 30), (2, 11, 3, 12), (0, 20, 5, 33), (3, 0, 5, 9)], np.int32)
    want = gather_crops_np(R.reflectance_np(cube(name), bands, window, clip), boxes)
    got = new_route("neon", "fp32").crops(boxes).cpu().numpy()
    assert got.shape == want.shape == (5, 349, 11, 11) and np.array_equal(got, want)
    ras = new_route("neon", "bf16")                                    # the tile route: a selection of the bf16 raster
    tiles = ras.crops(boxes, tiles=True)
    assert tiles.shape == (5, 349, 11, 11)
    assert np.array_equal(tiles.float().cpu().numpy(), gather_crops_np(ras.float().cpu().numpy(), boxes))
