"""Shared case makers for the stems tests (tests/test_stems_cpu.py, tests/test_stems_gpu.py): stems and crown boxes at UTM
magnitudes, as plain dicts of the arguments of stems.assign_np.

    lattice      40 plots of 40 m, every pairing of 0 / 1 / 7 / 40 / 130 boxes with 1 / 3 / 12 / 33 / 70 stems; corners and
                 stems on a 0.25 m lattice, so that stems on box sides, exact distance ties and coincident stems are common
    continuous   coordinates on a 2^-30 m lattice (as good as continuous: the squares in d2 are inexact), with pairs of
                 boxes mirrored about a stem, whose d2 tie only if every product is rounded on its own
    chunks       plots with 1023 / 1024 / 1025 boxes and 255 / 256 / 257 / 1025 stems: a workgroup spans plots, a plot spans
                 workgroups and LDS chunks
    HAND         small cases with the expected answer written out
"""
import numpy as np

UTM = (4e5, 3.3e6)
BOXES = (0, 1, 7, 40, 130)
STEMS = (1, 3, 12, 33, 70)
LATTICE_SEED = 2                 # every floor of test_the_lattice_family_reaches_every_path is met with room


def _case(boxes, box_plot, points, point_plot, height, chm, plots, size=1.0):
    return dict(boxes=np.ascontiguousarray(boxes, np.float64).reshape(-1, 4), box_plot=np.asarray(box_plot, np.int64),
                points=np.ascontiguousarray(points, np.float64).reshape(-1, 2), point_plot=np.asarray(point_plot, np.int64),
                height=np.asarray(height, np.float64), chm=None if chm is None else np.asarray(chm, np.float64),
                plots=int(plots), size=float(size))


def _plots(counts, seed, step=0.25, nan_x=0.02, copies=0.15):
    """One 40 m cell per (boxes, stems) pair of `counts`, the cells 100 m apart; everything on a lattice of `step` metres."""
    rng = np.random.default_rng(seed)
    cells = int(round(40.0 / step))
    boxes, box_plot, points, point_plot = [], [], [], []
    for plot, (nb, ns) in enumerate(counts):
        org = np.array([UTM[0] + 100.0 * (plot % 8), UTM[1] + 100.0 * (plot // 8)])
        side = rng.integers(int(3 / step), int(15 / step) + 1, (nb, 2))
        low = rng.integers(0, cells - side + 1)
        made = np.concatenate([org + low * step, org + (low + side) * step], axis=1)
        for k in np.flatnonzero(rng.random(nb) < 0.05):                # a crown predicted twice
            made[k] = made[rng.integers(0, nb)]
        boxes.append(made)
        box_plot.append(np.full(nb, plot))
        p = org + rng.integers(0, cells + 1, (ns, 2)) * step
        for k in np.flatnonzero(rng.random(ns) < copies):              # a stem measured twice, or two stems of one tree
            p[k] = p[rng.integers(0, ns)]
        points.append(p)
        point_plot.append(np.full(ns, plot))
    points = np.concatenate(points)
    n = len(points)
    height = np.where(rng.random(n) < 0.25, np.nan, 5.0 * rng.integers(1, 7, n))
    chm = np.where(rng.random(n) < 0.20, np.nan, 0.5 * rng.integers(10, 50, n))
    points[rng.random(n) < nan_x, 0] = np.nan
    return _case(np.concatenate(boxes), np.concatenate(box_plot), points, np.concatenate(point_plot), height, chm, len(counts))


def lattice(seed=LATTICE_SEED):
    return _plots([(BOXES[p % 5], STEMS[(p // 5) % 5]) for p in range(40)], seed)


def chunks(seed=11):
    return _plots([(1023, 255), (1024, 256), (1025, 257), (40, 1025), (0, 1025), (0, 5), (2100, 300), (3, 1)], seed)


def continuous(seed=12, plots=12, per_plot=(60, 40)):
    """Uniform coordinates on a 2^-30 m lattice.  Every third stem gets two more boxes whose centres are the stem plus (a, b)
    and plus (b, a): d2 = a * a + b * b and b * b + a * a tie exactly, a fused multiply-add breaks the tie."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -30

    def grid(lo, hi, shape):
        return np.round(rng.uniform(lo, hi, shape) / q) * q

    boxes, box_plot, points, point_plot = [], [], [], []
    for plot in range(plots):
        org = np.array([UTM[0] + 100.0 * plot, UTM[1]])
        nb, ns = per_plot
        low, side = grid(0.0, 25.0, (nb, 2)), grid(3.0, 15.0, (nb, 2))
        p = org + grid(0.0, 40.0, (ns, 2))
        b = [np.concatenate([org + low, org + low + side], axis=1)]
        for k in range(0, ns, 3):
            a, half = grid(-0.75, 0.75, 2), grid(1.0, 2.0, 1)[0]
            for off in (a, a[::-1]):
                b.append(np.concatenate([p[k] + off - half, p[k] + off + half])[None])
        b = np.concatenate(b)
        boxes.append(b[rng.permutation(len(b))])
        box_plot.append(np.full(len(b), plot))
        points.append(p)
        point_plot.append(np.full(ns, plot))
    points = np.concatenate(points)
    n = len(points)
    height = np.where(rng.random(n) < 0.2, np.nan, rng.uniform(2.0, 40.0, n))
    chm = np.where(rng.random(n) < 0.2, np.nan, rng.uniform(2.0, 40.0, n))
    return _case(np.concatenate(boxes), np.concatenate(box_plot), points, np.concatenate(point_plot), height, chm, plots)


def shuffled(case, seed):
    """The same boxes and stems in another order (another problem: ties go to the lowest index), plot codes interleaved."""
    rng = np.random.default_rng(seed)
    pb, ps = rng.permutation(len(case["boxes"])), rng.permutation(len(case["points"]))
    out = dict(case, boxes=np.ascontiguousarray(case["boxes"][pb]), box_plot=case["box_plot"][pb],
               points=np.ascontiguousarray(case["points"][ps]), point_plot=case["point_plot"][ps], height=case["height"][ps])
    out["chm"] = None if case["chm"] is None else case["chm"][ps]
    return out


def arguments(case, chm=True):
    """The case as the keyword arguments of stems.assign_np (chm=False: without the CHM heights)."""
    kw = {k: case[k] for k in ("boxes", "box_plot", "points", "point_plot", "height", "chm", "size", "plots")}
    if not chm:
        kw["chm"] = None
    return kw


def census(case, result):
    """What a family exercises, counted from the inputs and the definition's answer by plain loops: status counts, stems
    with an exact distance tie for the nearest candidate (predicted or fallback), (stem, box) pairs with the stem on a side of the box, stems that
    chose another stem's fallback box, and boxes whose tallest stems tie."""
    b, bp, p, pp, h = case["boxes"], case["box_plot"], case["points"], case["point_plot"], case["height"]
    M, s = len(b), case["size"]
    ties = sides = 0
    for i in range(len(p)):
        x, y = p[i]
        if result.box[i] >= M:                                          # among the fallback boxes of the plot's missing stems
            mine = np.flatnonzero((pp == pp[i]) & (result.box >= M))
            mine, b = np.arange(len(mine)), np.stack([p[mine, 0] - s, p[mine, 1] - s, p[mine, 0] + s, p[mine, 1] + s], axis=1)
        else:
            mine, b = np.flatnonzero(bp == pp[i]), case["boxes"]
        cand = mine[(b[mine, 0] <= x) & (x <= b[mine, 2]) & (b[mine, 1] <= y) & (y <= b[mine, 3])]
        sides += int(((b[cand, 0] == x) | (b[cand, 2] == x) | (b[cand, 1] == y) | (b[cand, 3] == y)).sum())
        cx, cy = (b[cand, 0] + b[cand, 2]) * 0.5, (b[cand, 1] + b[cand, 3]) * 0.5
        d2 = (cx - x) * (cx - x) + (cy - y) * (cy - y)
        ties += int(len(d2) > 1 and (d2 == d2.min()).sum() > 1)
    height_ties = 0
    for j in np.unique(result.box[result.box >= 0]):
        g = h[result.box == j]
        height_ties += int(len(g) > 1 and not np.isnan(g).all() and (g == np.nanmax(g)).sum() > 1)
    others = int(((result.box >= M) & (result.box != M + np.arange(len(p)))).sum())
    return dict(status=np.bincount(result.status, minlength=5).tolist(), distance_ties=ties, on_side=sides,
                other_fallback=others, height_ties=height_ties)


nan, inf = np.nan, np.inf
# (name, case, box, status): the expected answers are written out; size = 1, so the fallback box of (x, y) is x-1 .. x+1
HAND = (
    ("a stem on the corner two boxes share takes the nearer centre",
     _case([(0, 0, 2, 2), (2, 2, 6, 6)], [0, 0], [(2, 2)], [0], [10.0], [10.0], 1), [0], [1]),
    ("two boxes at the same distance: the lower index; then each stem to its nearer box",
     _case([(2, 0, 6, 4), (0, 0, 4, 4)], [0, 0], [(3, 1), (2.5, 1)], [0, 0], [10.0, 10.0], [10.0, 10.0], 1), [0, 1], [1, 1]),
    ("no boxes at all: coincident missing stems share the first one's fallback box, the taller stays",
     _case([], [], [(10, 10), (10, 10), (30, 30)], [0, 0, 0], [5.0, 8.0, nan], [1.0, 1.0, 1.0], 1), [0, 0, 2], [0, 2, 2]),
    ("a box whose stems all lack a height keeps nobody",
     _case([(0, 0, 10, 10)], [0], [(1, 1), (2, 2), (3, 3)], [0, 0, 0], [nan, nan, nan], [1.0, 2.0, 3.0], 1), [0, 0, 0], [3, 3, 3]),
    ("a height tie broken by CHM; one CHM leaves tied: the lowest index; one with no CHM among the tallest: nobody",
     _case([(0, 0, 10, 10), (100, 100, 110, 110), (200, 200, 210, 210)], [0, 0, 0],
           [(1, 1), (2, 2), (3, 3), (101, 101), (102, 102), (103, 103), (201, 201), (202, 202), (203, 203)], [0] * 9,
           [10.0, 10.0, 8.0, 10.0, 10.0, 10.0, 10.0, 10.0, 4.0], [5.0, 7.0, 9.0, 4.0, 4.0, nan, nan, nan, 30.0], 1),
     [0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 1, 0, 1, 0, 0, 3, 3, 3]),
    ("the same without CHM: the lowest index of the tallest",
     _case([(0, 0, 10, 10), (100, 100, 110, 110), (200, 200, 210, 210)], [0, 0, 0],
           [(1, 1), (2, 2), (3, 3), (101, 101), (102, 102), (103, 103), (201, 201), (202, 202), (203, 203)], [0] * 9,
           [10.0, 10.0, 8.0, 10.0, 10.0, 10.0, 10.0, 10.0, 4.0], None, 1),
     [0, 0, 0, 1, 1, 1, 2, 2, 2], [1, 0, 0, 1, 0, 0, 1, 0, 0]),
    ("boxes of another plot are not met; a plot with boxes and no stems; plot codes outside 0 .. plots-1",
     _case([(0, 0, 10, 10), (0, 0, 10, 10)], [1, 0], [(5, 5), (5, 5), (5, 5), (5, 5)], [0, 2, 7, -1], [1.0] * 4, [1.0] * 4, 3),
     [1, 3, -1, -1], [1, 2, 4, 4]),
    ("an inverted box and a NaN box hold nobody; an infinite box is a candidate at distance +inf",
     _case([(10, 10, 0, 0), (nan, 0, 10, 10), (-inf, -inf, inf, inf), (4, 4, 8, 8)], [0, 0, 1, 1],
           [(5, 5), (5, 5), (0, 0), (nan, 5), (5, inf)], [0, 1, 1, 1, 1], [1.0] * 5, [1.0] * 5, 2),
     [4, 3, 2, -1, -1], [2, 1, 1, 4, 4]),
)


def crowns_of(case, box):
    """The crown boxes the indices `box` stand for, written out from the inputs."""
    M, s = len(case["boxes"]), case["size"]
    out = np.full((len(box), 4), np.nan)
    for i, j in enumerate(box):
        if 0 <= j < M:
            out[i] = case["boxes"][j]
        elif j >= M:
            x, y = case["points"][j - M]
            out[i] = (x - s, y - s, x + s, y + s)
    return out
