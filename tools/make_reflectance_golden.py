"""Generate tests/golden/reflectance/reflectance_reference.npz by running the REFERENCE ITSELF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_reflectance_golden.py <path of a checkout of the reference>

Imports the reference's src/Hyperspectral.py read-only (`h5py` and `rasterio` are stubbed: only the import has to succeed),
replaces its file reader `h5refl2array` by a function that returns a small synthetic (metadata, cube) and its file writer
`array2raster` by one that keeps what it is handed, and calls the reference's own `generate_raster` (bands="no_water") and
`calc_clip_index`.  The file holds only data: the inputs and what the reference handed to its writer.  No reference source
is copied anywhere.  The fixture has a folder and a checksum file of its own (tests/golden/reflectance/SHA256SUMS, written
here), as tests/golden/canopy has.

`cube` int16 [7][9][426]: band b of pixel q = row * 9 + col holds 70 * b + q, so the source band of any captured value is
value // 70 and its pixel value % 70.  `extent` float64 (xMin, xMax, yMin, yMax) with one-metre pixels.  Three runs:
  no bounds            `raster_full` int16 [7][9][369], `index_full` (yMin, xMin, yMax, xMax as the reference's dict names them:
                       row0, col0, row1, col1)
  `bounds_a`, `bounds_b`   float64 (left, bottom, right, top), every edge HALF a pixel off the grid, so each of the four
                       indices is a .5 tie: a rounds to (0, 0, 6, 6) -- 0.5 -> 0, 5.5 -> 6, 6.5 -> 6 -- and b to (2, 2, 4, 8) --
                       2.5 -> 2, 4.5 -> 4, 7.5 -> 8; `raster_a`, `raster_b`, `index_a`, `index_b`
`bands_no_water` int32 [369]: the source bands recovered from raster_full.
"""
import collections
import hashlib
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "reflectance")
OUT = os.path.join(GOLDEN, "reflectance_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

ROWS, COLS, BANDS, STEP = 7, 9, 426, 70
X_MIN, Y_MIN = 500000.0, 4100000.0
Bounds = collections.namedtuple("Bounds", "left bottom right top")
BOUNDS_A = Bounds(X_MIN + 0.5, Y_MIN + 1.5, X_MIN + 6.5, Y_MIN + 6.5)
BOUNDS_B = Bounds(X_MIN + 2.5, Y_MIN + 2.5, X_MIN + 7.5, Y_MIN + 4.5)


def synthetic():
    q = (np.arange(ROWS)[:, None] * COLS + np.arange(COLS)[None, :])[:, :, None]
    cube = (STEP * np.arange(BANDS)[None, None, :] + q).astype(np.int16)
    assert int(cube.max()) == STEP * (BANDS - 1) + ROWS * COLS - 1 < 32768
    ext = {"xMin": X_MIN, "xMax": X_MIN + COLS, "yMin": Y_MIN, "yMax": Y_MIN + ROWS}
    meta = {"extent": (ext["xMin"], ext["xMax"], ext["yMin"], ext["yMax"]), "ext_dict": ext,
            "res": {"pixelWidth": 1.0, "pixelHeight": 1.0}, "epsg": "32617", "shape": cube.shape}
    return meta, cube


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "Hyperspectral.py")):
        sys.exit("usage: make_reflectance_golden.py <path of a checkout of the reference>")
    for name in ("h5py", "rasterio"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, sys.argv[1])
    from src import Hyperspectral as R

    meta, cube = synthetic()
    captured = []
    R.h5refl2array = lambda path: (meta, cube)
    R.array2raster = lambda name, array, metadata, extent, ras_dir: captured.append(np.array(array))

    def run(bounds):
        del captured[:]
        R.generate_raster("tile.h5", "unused", rgb_filename="tile.tif", bands="no_water", bounds=bounds)
        assert len(captured) == 1 and captured[0].dtype == np.int16, [c.dtype for c in captured]
        clip = {"xMin": meta["extent"][0], "xMax": meta["extent"][1], "yMin": meta["extent"][2], "yMax": meta["extent"][3]}
        if bounds:
            clip = {"xMin": bounds.left, "xMax": bounds.right, "yMin": bounds.bottom, "yMax": bounds.top}
        ind = R.calc_clip_index(clip, meta["ext_dict"])
        index = np.array([int(ind["yMin"]), int(ind["xMin"]), int(ind["yMax"]), int(ind["xMax"])], np.int64)
        assert captured[0].shape[:2] == (index[2] - index[0], index[3] - index[1]), (captured[0].shape, index)
        return captured[0], index

    full, index_full = run(False)
    a, index_a = run(BOUNDS_A)
    b, index_b = run(BOUNDS_B)
    assert index_a.tolist() == [0, 0, 6, 6] and index_b.tolist() == [2, 2, 4, 8], (index_a, index_b)
    bands = (full[0, 0].astype(np.int64) // STEP).astype(np.int32)
    assert np.array_equal(full.astype(np.int64) // STEP, np.broadcast_to(bands, full.shape))

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(OUT, cube=cube, extent=np.array(meta["extent"], np.float64), bands_no_water=bands,
                        bounds_a=np.array(BOUNDS_A, np.float64), bounds_b=np.array(BOUNDS_B, np.float64),
                        raster_full=full, raster_a=a, raster_b=b, index_full=index_full, index_a=index_a, index_b=index_b)
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes;", len(bands), "bands; windows", index_full, index_a, index_b)


if __name__ == "__main__":
    main()
