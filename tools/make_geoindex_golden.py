"""Generate tests/golden/abundance_grid/geoindex_reference.npz by running the REFERENCE ITSELF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_geoindex_golden.py <path of a checkout of the reference>

Imports the reference's src/neon_paths.py read-only (`h5py` and the reference's own `src.Hyperspectral` are stubbed: only
the import has to succeed) and calls its `bounds_to_geoindex` (:9-24) on every row of `bounds`: the rule that says which
1 km tile a crown belongs to, which abundance.cells_np / cell_names restate (rule="geoindex").

The file holds only data: `bounds` float64 [M][4] (xmin, ymin, xmax, ymax), `geoindex` the reference's
"{easting}_{northing}" string of each row, `block` int64 [M] (which of the two grids below a row lies in) and `grid` int64
[2][4] = (origin_x, origin_y, cols, rows) of a 1000 m grid that covers every row of the block.  No reference source is
copied anywhere.  The fixture has a folder and a checksum file of its own (tests/golden/abundance_grid/SHA256SUMS, written
here); tests/golden/abundance stays as it is.

The rows: block 0 is UTM-sized (eastings 400-430 km, northings 4100-4130 km): random crown boxes of 1-20 m; boxes whose
centre is an exact multiple of 1000 on one or both axes; centres at k * 1000 - 0.5 and k * 1000 + 0.5; boxes that straddle a
tile line with unequal parts on either side.  Block 1 lies around the origin, where truncation toward zero and floor
differ: the same four kinds with negative coordinates, and the centres -0.5, -999.5, -1000, -1000.5 and 0.
"""
import hashlib
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "abundance_grid")
OUT = os.path.join(GOLDEN, "geoindex_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

GRID = np.array([[400000, 4100000, 30, 30], [-5000, -5000, 10, 10]], np.int64)


def centred(cx, cy, w, h):
    """Boxes with the given centres: halves that are multiples of 1/4, so that (lo + hi) / 2 is the centre exactly."""
    return np.stack([cx - w, cy - h, cx + w, cy + h], axis=1)


def block(rs, ox, oy, cols, rows, n_random, n_each):
    x0, y0, x1, y1 = ox + 1000, oy + 1000, ox + (cols - 1) * 1000, oy + (rows - 1) * 1000     # a tile's margin all round
    out = []
    # random crown boxes
    xa, ya = rs.uniform(x0, x1, n_random), rs.uniform(y0, y1, n_random)
    out.append(np.stack([xa, ya, xa + rs.uniform(1, 20, n_random), ya + rs.uniform(1, 20, n_random)], axis=1))
    kx = ox + 1000 * rs.randint(1, cols - 1, n_each).astype(np.float64)
    ky = oy + 1000 * rs.randint(1, rows - 1, n_each).astype(np.float64)
    half = rs.randint(1, 40, (2, n_each)) / 4.0
    free_x, free_y = rs.uniform(x0, x1, n_each), rs.uniform(y0, y1, n_each)
    # centres at exact multiples of 1000: on x, on y, on both
    out.append(centred(kx, np.round(free_y * 4) / 4, half[0], half[1]))
    out.append(centred(np.round(free_x * 4) / 4, ky, half[0], half[1]))
    out.append(centred(kx, ky, half[0], half[1]))
    # ... and half a metre either side
    for d in (-0.5, 0.5):
        out.append(centred(kx + d, ky - d, half[0], half[1]))
    # boxes that straddle a tile line, unequal parts on either side
    a, b = rs.uniform(0.1, 15, (2, n_each)), rs.uniform(0.1, 15, (2, n_each))
    out.append(np.stack([kx - a[0], free_y, kx + b[0], free_y + 5], axis=1))
    out.append(np.stack([free_x, ky - a[1], free_x + 5, ky + b[1]], axis=1))
    return np.concatenate(out)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "neon_paths.py")):
        sys.exit("usage: make_geoindex_golden.py <path of a checkout of the reference>")
    for name in ("h5py", "src.Hyperspectral"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, sys.argv[1])
    import src
    src.Hyperspectral = sys.modules["src.Hyperspectral"]
    from src import neon_paths

    rs = np.random.RandomState(11)
    utm = block(rs, *GRID[0], n_random=120, n_each=20)
    zero = block(rs, *GRID[1], n_random=60, n_each=10)
    special = np.array([-0.5, -999.5, -1000.0, -1000.5, 0.0, 0.5, 999.5, -0.25])
    zero = np.concatenate([zero, centred(special, special[::-1].copy(), np.full(8, 1.5), np.full(8, 2.25))])
    bounds = np.ascontiguousarray(np.concatenate([utm, zero]), dtype=np.float64)
    which = np.concatenate([np.zeros(len(utm), np.int64), np.ones(len(zero), np.int64)])
    names = np.array([neon_paths.bounds_to_geoindex([float(v) for v in b]) for b in bounds])
    assert names.dtype.kind == "U"

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(OUT, bounds=bounds, geoindex=names, block=which, grid=GRID)
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes;", len(bounds), "rows;", len(set(names.tolist())), "tiles")


if __name__ == "__main__":
    main()
