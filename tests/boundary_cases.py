"""Seeded boundaries and queries shared by tests/test_boundary_cpu.py and tests/test_boundary_gpu.py: a star-shaped exterior
ring with a hole and an island at UTM magnitudes, with a chosen number of edges."""
import numpy as np

UTM = (4.0e5, 3.3e6)             # easting / northing of the sites' corner: the magnitudes the definition has to survive


def star(n, cx, cy, r_in, r_out, seed, phase=0.0):
    """An n-vertex star: radii alternate between about r_in and about r_out (jittered), counter-clockwise, not closed."""
    rng = np.random.default_rng(seed)
    ang = phase + 2 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
    rad = np.where(np.arange(n) % 2 == 0, r_out, r_in) * rng.uniform(0.9, 1.0, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def prototype_site():
    """The boundary the definition was prototyped on: a 257-vertex star, a 31-vertex hole and a 17-vertex island."""
    cx, cy = UTM[0] + 2000.0, UTM[1] + 2000.0
    return [star(257, cx, cy, 900.0, 1800.0, 1), star(31, cx + 40.0, cy - 30.0, 150.0, 300.0, 2)[::-1],
            star(17, cx + 2600.0, cy + 300.0, 200.0, 420.0, 3)]


def site(n_edges, seed=0):
    """Rings with exactly n_edges edges in all: from 12 edges on an exterior star, a hole and an island (a second part);
    below that the exterior alone.  Returns (rings, centre, r_out)."""
    cx, cy = UTM[0] + 1500.0, UTM[1] + 1500.0
    if n_edges < 12:
        return [star(n_edges, cx, cy, 500.0, 1000.0, seed)], (cx, cy), 1000.0
    hole, island = max(3, n_edges // 8), max(3, n_edges // 16)
    rings = [star(n_edges - hole - island, cx, cy, 500.0, 1000.0, seed),
             star(hole, cx + 20.0, cy - 10.0, 100.0, 200.0, seed + 1)[::-1],
             star(island, cx + 1500.0, cy + 100.0, 150.0, 300.0, seed + 2)]
    return rings, (cx, cy), 1000.0


def extent(rings):
    v = np.concatenate(rings)
    return v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()


def points(rings, n, seed):
    """n float64 points: the first ones by construction on vertices, on edge midpoints, outside the bounding box on each
    side, and NaN / inf; the rest uniform over the bounding box and a margin."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = extent(rings)
    w, h = x1 - x0, y1 - y0
    v = np.concatenate(rings)
    mid = np.concatenate([0.5 * (r + np.roll(r, -1, axis=0)) for r in rings])
    special = np.concatenate([
        v[rng.permutation(len(v))[:40]], mid[rng.permutation(len(mid))[:40]],
        [(x0 - 5.0, y0 + h / 2), (x1 + 5.0, y0 + h / 2), (x0 + w / 2, y0 - 5.0), (x0 + w / 2, y1 + 5.0),
         (x0, y0), (x1, y1), (x0, y1), (x1, y0), (v[0, 0], y1), (x1, v[0, 1]),
         (np.nan, y0 + h / 2), (x0 + w / 2, np.nan), (np.inf, y0 + h / 2), (-np.inf, y0 + h / 2), (x0 + w / 2, np.inf),
         (x0 + w / 2, -np.inf)]])
    rest = np.stack([rng.uniform(x0 - 0.2 * w, x1 + 0.2 * w, n), rng.uniform(y0 - 0.2 * h, y1 + 0.2 * h, n)], axis=1)
    return np.ascontiguousarray(np.concatenate([special, rest])[:n], dtype=np.float64)


def pixel_boxes(rings, n, seed, pixel=(0.5, -0.25)):
    """(boxes int32 [n, 4], transform): crown boxes of 3-25 m over the bounding box and a margin, on a grid with non-square
    pixels and a negative e; a few degenerate ones (no rows, no columns, inverted) first."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = extent(rings)
    a, e = pixel
    t = (float(np.floor(x0 - 300.0)), a, float(np.ceil(y1 + 300.0)), e)
    cols, rows = int((x1 - x0 + 600.0) / a), int((y1 - y0 + 600.0) / -e)
    c0, r0 = rng.integers(0, cols, n), rng.integers(0, rows, n)
    b = np.stack([r0, c0, r0 + (rng.uniform(3, 25, n) / -e).astype(np.int64), c0 + (rng.uniform(3, 25, n) / a).astype(np.int64)], axis=1)
    b[0, 2] = b[0, 0]                                          # no rows: a horizontal line
    b[1, 3] = b[1, 1]                                          # no columns
    b[2, [0, 2]] = b[2, [2, 0]]                                # row1 < row0: min / max put it right
    return b.astype(np.int32), t
