"""Seeded detector outputs shared by tests/test_mosaic_cpu.py, tests/test_mosaic_gpu.py and tools/mosaicbench.py.  Every
case is a dict of the arguments of mosaic.nms_np / mosaic.mosaic: boxes, scores, window, origins, mask (any of the last three
may be None), height, width, max_side."""
import numpy as np

from deeptreeattention_amd import mosaic as M


def case(boxes, scores, height, width, window=None, origins=None, mask=None, max_side=None):
    return {"boxes": np.ascontiguousarray(boxes, np.float32), "scores": np.ascontiguousarray(scores, np.float32), "window": window,
            "origins": origins, "mask": mask, "height": int(height), "width": int(width), "max_side": max_side}


def nms_args(c):
    return {k: c[k] for k in ("boxes", "scores", "window", "origins", "mask", "max_side")}


def scene(side, trees, seed, patch_size=400, patch_overlap=0.05, extent=None):
    """A tree scene seen through side x side detector windows: `trees` crowns of 15 - 45 px scattered over the tile; every
    window reports the crowns whose centre it holds and those that reach at least 6 px into it, clipped to the window and
    jittered by up to 1.5 px, so the overlap strips hold the same tree twice or four times.  Scores are multiples of 1 / 64:
    they tie.  extent: the tile's side in pixels if the last window is not to be a full step from the one before."""
    rng = np.random.default_rng(seed)
    step = patch_size - int(np.floor(patch_size * patch_overlap))
    extent = step * (side - 1) + patch_size if extent is None else int(extent)
    wins = M.windows(extent, extent, patch_size, patch_overlap)
    assert len(wins) == side * side
    cx, cy = rng.uniform(0, extent, trees), rng.uniform(0, extent, trees)
    half = rng.uniform(7.5, 22.5, trees)
    quality = rng.uniform(0.2, 1.0, trees)
    boxes, scores, index = [], [], []
    for k, (x, y, w, h) in enumerate(wins.tolist()):
        seen = np.flatnonzero((cx + half > x + 6) & (cx - half < x + w - 6) & (cy + half > y + 6) & (cy - half < y + h - 6))
        jitter = rng.uniform(-1.5, 1.5, (len(seen), 4))
        b = np.stack([cx[seen] - half[seen] - x, cy[seen] - half[seen] - y, cx[seen] + half[seen] - x, cy[seen] + half[seen] - y],
                     axis=1) + jitter
        b = np.clip(b, 0, [w, h, w, h])
        boxes.append(b)
        scores.append(np.round(np.clip(quality[seen] + rng.uniform(-0.1, 0.1, len(seen)), 0.05, 1.0) * 64) / 64)
        index.append(np.full(len(seen), k, np.int32))
    return case(np.concatenate(boxes), np.concatenate(scores), extent, extent, np.concatenate(index),
                np.ascontiguousarray(wins[:, :2]), max_side=patch_size)


def scene36():
    """The 36-window scene: about 4,400 boxes."""
    return scene(6, 3400, 36)


def scattered(n, seed, max_side=40):
    """n boxes of 8 - 40 px in tile coordinates at a density where most boxes meet a few others; scores tie."""
    rng = np.random.default_rng(seed)
    extent = int(max(64, 18 * np.sqrt(n)))
    x, y = rng.uniform(-5, extent - 5, n), rng.uniform(-5, extent - 5, n)
    w, h = rng.uniform(8, max_side, n), rng.uniform(8, max_side, n)
    return case(np.stack([x, y, x + w, y + h], axis=1), np.round(rng.uniform(0.1, 1, n) * 32) / 32, extent, extent,
                max_side=max_side)


def staircase(n, ties=False):
    """n boxes of 10 x 10 px, each 4 px to the right of the one before: a box overlaps its two neighbours only (IoU 60 / 140
    and 20 / 180), the scores fall along the chain (or all tie, where the index decides): alternate boxes are kept and the
    chain of decisions is n long."""
    x = 4.0 * np.arange(n)
    scores = np.full(n, 0.5) if ties else 1.0 - 1e-4 * np.arange(n)
    return case(np.stack([x, np.full(n, 20.0), x + 10, np.full(n, 30.0)], axis=1), scores, 64, int(x[-1]) + 16, max_side=40)


def cell_edges(seed=5, max_side=40, cells=6):
    """Boxes on a tile of cells x cells cells: centres exactly on cell edges and corners, pairs that overlap across an edge
    and across a corner, and scattered boxes around them."""
    rng = np.random.default_rng(seed)
    n_scatter = 400
    extent = 41 * cells - 1
    cell, gx, gy = M.grid(n_scatter + 200, extent, extent, max_side)
    assert (gx, gy) == (cells, cells)
    boxes = []
    for kx in range(1, cells):
        for ky in range(1, cells):
            ex, ey = kx * cell, ky * cell
            boxes += [(ex - 10, ey - 10, ex + 10, ey + 10),                      # the centre on a corner
                      (ex - 10, ey + 7, ex + 10, ey + 27),                       # ... on a vertical edge
                      (ex - 13, ey - 13, ex + 7, ey + 7), (ex - 7, ey - 7, ex + 13, ey + 13),      # a pair across the corner
                      (ex - 13, ey + 12, ex + 7, ey + 32), (ex - 7, ey + 12, ex + 13, ey + 32)]    # a pair across the edge
    boxes = np.array(boxes)
    x, y = rng.uniform(0, extent - 30, n_scatter), rng.uniform(0, extent - 30, n_scatter)
    w, h = rng.uniform(8, 30, n_scatter), rng.uniform(8, 30, n_scatter)
    boxes = np.concatenate([boxes, np.stack([x, y, x + w, y + h], axis=1)])
    return case(boxes, np.round(rng.uniform(0.1, 1, len(boxes)) * 64) / 64, extent, extent, max_side=max_side)


def one_cell(n, seed):
    """n boxes on a tile that is a single cell (300 x 300 px under max_side 400)."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 280, n), rng.uniform(0, 280, n)
    w, h = rng.uniform(4, 20, n), rng.uniform(4, 20, n)
    return case(np.stack([x, y, x + w, y + h], axis=1), np.round(rng.uniform(0.1, 1, n) * 256) / 256, 300, 300, max_side=400)


def column(n=600, seed=8):
    """A tile one cell wide and many tall."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 12, n), rng.uniform(0, 4960, n)
    w, h = rng.uniform(6, 18, n), rng.uniform(6, 38, n)
    return case(np.stack([x, y, x + w, y + h], axis=1), np.round(rng.uniform(0.1, 1, n) * 64) / 64, 5000, 30, max_side=40)


def all_statuses(seed=9):
    """A small scene in window coordinates with every status: refused for each cause, masked, kept and dropped."""
    c = scene(2, 1000, seed)
    b, s, w = c["boxes"], c["scores"], c["window"].copy()
    b[0, 0] = np.nan
    b[1, 3] = np.inf
    s[2] = np.nan
    s[3] = -np.inf
    b[4, [0, 2]] = b[4, [2, 0]] + [1, 0]                      # xmax < xmin
    b[5, [1, 3]] = b[5, [3, 1]] + [1, 0]                      # ymax < ymin
    b[6] = (0, 10, 400.5, 30)                                  # wider than the window
    b[7] = (10, 0, 30, 401)                                    # taller
    w[8], w[9] = -1, len(c["origins"])                         # no such window
    rng = np.random.default_rng(seed)
    c["mask"] = (rng.uniform(size=len(b)) > 0.2).astype(np.uint8)
    c["mask"][:10] = 1
    c["window"] = w
    return c


REFUSED_ROWS = 10                # of all_statuses
