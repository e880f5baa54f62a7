"""Reflectance cube to resident raster: the array work between the file reader and dense.DenseRaster.

A NEON reflectance tile is a pixel-interleaved cube [rows][cols][426] of int16.  The reference turns it into a band-first
GeoTIFF first (src/Hyperspectral.py:152-219 `generate_raster`: drop the water-absorption bands, optionally clip to
geographic bounds, np.moveaxis, write) and normalises what it reads back (src/utils.py:36-57: drop 10 + 10 bands, min-max
every pixel over its bands).  Band selection and a per-pixel min-max are exact and per pixel, so the resident raster can be
made straight from the cube: dense.DenseRaster.from_reflectance (csrc/reflectance.hip, dta_reflectance_normalise).

This module is the host side, pure NumPy, no GPU -- the written-down meaning of the kernel:

    band_index       the source band of every band of the file the reference would have written
    clip_index       geographic bounds -> the half-open pixel window, with the reference's rounding
    selected_bands   band_index with load_image's clip applied: the bands of the RASTER
    reflectance_np   the normalised raster, float32 [C][h][w]

Reading the file (h5py), georeferencing, nodata masking and masks by wavelength stay the caller's.  Nodata (-9999) is not
treated specially, because the reference does not: it takes part in the min-max.
"""
import warnings

import numpy as np

from . import _lib
from .preprocess import out_bands

MAX_BANDS = _lib.REFLECTANCE_MAX_BANDS     # DTA_REFLECTANCE_MAX_BANDS: bands per cube pixel, and bands selected
NEON_BANDS = 426
STAGE_BYTES, MIN_PIXELS = 40 * 1024, 8     # RF_STAGE_BYTES, RF_MIN_PIXELS (csrc/reflectance.hip)
_TINY = np.float32(10.0) * np.finfo(np.float32).eps
_NO_WATER = ((0, 192), (210, 283), (315, 419))     # what is left of 0..424 without 192..209, 283..314 and 419..424


def band_index(bands="no_water", bands_src=NEON_BANDS):
    """The source band of every selected band, int32: "no_water" the reference's mask (369 bands: 0-191, 210-282, 315-418),
    "all" every band, "false_color" (16, 54, 112), or an explicit integer sequence taken as given (any order, repeats
    allowed).  A value outside [0, bands_src) is refused."""
    bands_src = int(bands_src)
    if bands_src < 1:
        raise ValueError("bands_src must be >= 1, got {}".format(bands_src))
    if isinstance(bands, str):
        if bands == "no_water":
            idx = np.concatenate([np.arange(a, b) for a, b in _NO_WATER])
        elif bands == "all":
            idx = np.arange(bands_src)
        elif bands == "false_color":
            idx = np.array([16, 54, 112])
        else:
            raise ValueError("bands must be 'no_water', 'all', 'false_color' or a sequence of band indices, got {!r}".format(bands))
    else:
        idx = np.asarray(bands)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise ValueError("bands must be a non-empty 1-d sequence of integers")
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx.max() >= bands_src:
        raise ValueError("band index {} is outside [0, {})".format(int(idx.min() if idx.min() < 0 else idx.max()), bands_src))
    return idx.astype(np.int32)


def clip_index(bounds, extent, xscale=1, yscale=1):
    """bounds (left, bottom, right, top) and the tile's extent -- the dict with xMin, xMax, yMin, yMax or the tuple
    (xMin, xMax, yMin, yMax) that the reference's reader builds -- to the half-open pixel window (row0, col0, row1, col1).
    Python's round: ties go to the even integer (round(0.5) == 0, round(2.5) == 2)."""
    left, bottom, right, top = (float(v) for v in bounds)
    if isinstance(extent, dict):
        x_min, y_min, y_max = extent["xMin"], extent["yMin"], extent["yMax"]
    else:
        x_min, _, y_min, y_max = extent
    rows = y_max - y_min
    col0 = int(round((left - x_min) / xscale))
    col1 = int(round((right - x_min) / xscale))
    row1 = int(round(rows - (bottom - y_min) / yscale))
    row0 = int(round(rows - (top - y_min) / yscale))
    return row0, col0, row1, col1


def window_of(shape, window):
    """`window` (row0, col0, row1, col1), half-open, against a cube of `shape` [H][W][...]: upper bounds clamp to the cube
    as NumPy slicing does; a negative bound (NumPy would wrap it) and an empty window are refused.  None: the whole cube."""
    H, W = int(shape[0]), int(shape[1])
    if window is None:
        window = (0, 0, H, W)
    try:
        r0, c0, r1, c1 = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError("window must be (row0, col0, row1, col1)")
    if min(r0, c0, r1, c1) < 0:
        raise ValueError("window {} has a negative bound".format((r0, c0, r1, c1)))
    r1, c1 = min(r1, H), min(c1, W)
    if r1 <= r0 or c1 <= c0:
        raise ValueError("window {} is empty on a {} x {} cube".format(tuple(int(v) for v in window), H, W))
    return r0, c0, r1, c1


def selected_bands(bands="no_water", bands_src=NEON_BANDS, clip=10):
    """The source band of every band of the RASTER: band_index, without its first and last `clip` entries when more than 3
    bands are selected (the rule of the reference's preprocess_image and of preprocess.out_bands)."""
    idx = band_index(bands, bands_src)
    clip = int(clip)
    if clip < 0:
        raise ValueError("clip must be >= 0, got {}".format(clip))
    if len(idx) > 3 and clip > 0:
        if out_bands(len(idx), clip) < 1:
            raise ValueError("{} bands leave nothing after dropping 2 x {}".format(len(idx), clip))
        idx = idx[clip:len(idx) - clip]
    return np.ascontiguousarray(idx)


def minmax_np(img):
    """Per-pixel min-max over axis 0 of a [C][h][w] array in float32, rounded as scikit-learn's MinMaxScaler does it:
    nanmin / nanmax, ranges under 10 * eps(float32) count as constant, and X * scale + min_ as two roundings."""
    img = np.asarray(img, dtype=np.float32)
    with np.errstate(all="ignore"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # "All-NaN slice": such a pixel stays NaN
            lo, hi = np.nanmin(img, axis=0), np.nanmax(img, axis=0)
        rng = (hi - lo).astype(np.float32)
        rng = np.where(rng < _TINY, np.float32(1.0), rng).astype(np.float32)
        scale = (np.float32(1.0) / rng).astype(np.float32)
        shift = (np.float32(0.0) - (lo * scale).astype(np.float32)).astype(np.float32)
        out = (img * scale[None]).astype(np.float32)
        return (out + shift[None]).astype(np.float32)


def reflectance_np(cube, bands="no_water", window=None, clip=10):
    """What DenseRaster.from_reflectance computes: cube [H][W][B] -> float32 [C][h][w], the selected bands of the window
    moved first, clipped by `clip` on both ends (more than 3 bands only) and min-max scaled per pixel."""
    cube = np.asarray(cube)
    if cube.ndim != 3:
        raise ValueError("the cube must be a pixel-interleaved 3-d array [rows][cols][bands]")
    r0, c0, r1, c1 = window_of(cube.shape, window)
    sel = selected_bands(bands, cube.shape[2], clip)
    return minmax_np(np.moveaxis(cube[r0:r1, c0:c1][:, :, sel], 2, 0))


def launch_plan(bands_src, itemsize, cols):
    """(pixels per workgroup, LDS bytes from one staged pixel to the next) as dta_reflectance_normalise chooses them: the
    pixel's bytes in whole dwords, an odd number of them; the largest power of two of pixels, 8 to 256, that fits the staging
    budget and is not more than the row needs."""
    stride = (bands_src * itemsize + 3) & ~3
    if (stride >> 2) & 1 == 0:
        stride += 4
    np_ = 256
    while np_ > MIN_PIXELS and (np_ * stride > STAGE_BYTES or np_ // 2 >= cols):
        np_ //= 2
    return np_, stride
