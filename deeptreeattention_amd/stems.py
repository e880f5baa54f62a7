"""Field stems to crown boxes: which predicted crown box a field-measured stem gets, and which stem a box keeps -- the
reference's `process_plot` (src/generate.py:92-153) with `create_boxes` (:73-90), `choose_box` (:62-71) and the last line
of `points_to_crowns` (:239).  The reference runs it per plot, one dask future each: `gpd.sjoin(boxes, plot_data)` (:112), a
Python loop over `groupby("individual")` with a shapely distance per group (:122-127) and a second loop over
`groupby("box_id")` (:134-145).  Here all plots of a site are decided in one launch chain (dta_stems_assign,
csrc/stems.hip).  The stage sits between the height rules on stems (canopy.HeightRules) and everything that takes crown
boxes: DenseRaster.crops*, CanopyRaster.crown_height, RgbRaster.crops, Boundary.clip, split.SplitTable.

A stem only ever meets boxes and stems of its own plot (the reference predicts boxes per plot window and joins per plot).
Boxes are float64 (xmin, ymin, xmax, ymax) with a plot code each; stems are float64 (x, y) with a plot code, a height (NaN:
not measured) and optionally a CHM height.  Predicted boxes have the indices 0 .. M-1, the fallback box of stem i has M + i.

Step 1, the join (:112, predicate `intersects`).  Box j is a candidate of stem i iff their plot codes are equal and
    xmin <= px <= xmax  and  ymin <= py <= ymax
closed, on the raw float64 values: no arithmetic, no origin shift; a NaN anywhere makes it false.

Step 2, fallback boxes (:115-119, create_boxes).  A stem without a candidate is MISSING and gets the box
    (px - size, py - size, px + size, py + size)               each bound rounded once
the envelope of Point.buffer(size), whose vertices include 0, 90, 180 and 270 degrees.  The fallback box of i is a candidate
of every MISSING stem k of the same plot that lies in it (closed; k = i included): the reference joins the fixed boxes with
`missing_ids` only (:80).  A stem with a coordinate that is not finite, or with a plot code outside 0 .. plots-1, has no
candidate at all and is in nobody's group.

Step 3, the nearest box (choose_box).  A stem chooses, among its candidates, the one with the smallest
    d2 = (cx - px) * (cx - px) + (cy - py) * (cy - py),   cx = (xmin + xmax) * 0.5,   cy = (ymin + ymax) * 0.5
every product, sum and difference rounded on its own (no fused multiply-add); a d2 that is NaN (a box with an infinite
side) counts as +inf; on equal d2 the lowest box index wins.  The reference orders ties by pandas' unstable sort_values,
and shapely's centroid and distance are not this arithmetic to the last bit: nothing finer than this rule is promised.

Step 4, one stem per box (:134-145 and :239).  G = the stems that chose the same box.  |G| = 1: the stem is kept.
Otherwise hmax = the maximum of the heights of G that are not NaN and S = {k in G: height[k] == hmax} (empty when all are
NaN).  If |S| > 1 and chm is given, cmax = the maximum of the chm of S that are not NaN and S = {k in S: chm[k] == cmax}
(again empty when all are NaN); without chm S stays.  The kept stem is the lowest index of S.  If S is empty the box keeps
nobody, which is what `group[group.height == group.height.max()]` does; every stem of such a box gets status 3.

Assignment(box, status, crowns), in the caller's order:
    box     int64 [N]     the chosen index, or -1
    status  uint8 [N]     0 dropped, another stem of the box is taller;  1 kept with a predicted box;  2 kept with a fallback
                          box;  3 dropped, the box's stems have no height or CHM to compare;  4 no box: a coordinate that is
                          not finite or a plot code outside 0 .. plots-1
    crowns  float64 [N,4] the chosen box, NaN where box == -1
keep = (status == 1) | (status == 2) is a mask in the sense of canopy's `keep`.

assign_np is the definition; CrownBoxes.assign equals it bit for bit.  The device compares a stem with the boxes and the
stems of the plots its workgroup of 256 stems touches: N x (boxes + stems of a plot) in all, linear in practice because
plots are 40 m cells, and quadratic in the stems of one plot if a caller makes a whole tile one plot.
Out of scope: DeepForest itself (what sits between its detector's per-window output and these boxes -- the window layout, the
shift, the non-maximum suppression, the pixel boxes -- is mosaic.py), reading rasters or shapefiles, rasterio.windows.from_bounds (a caller keeps its own pixel
boxes and indexes them with `box`), crown polygons other than boxes.  The `point_plot` codes of a contributed megaplot
(the grid and the buffers of src/megaplot.py) come from field.megaplot_plots.
"""
import collections
import math

import numpy as np

from .boundary import _host, geo_boxes

CHUNK = 1024                     # DTA_STEMS_CHUNK: boxes or stems staged through LDS at a time
_PAIRS = 1 << 22                 # candidate pairs assign_np looks at in one step: bounded temporaries

Assignment = collections.namedtuple("Assignment", "box status crowns")
Assignment.__doc__ = """box int64 [N] (0 .. M-1 a predicted box, M + i the fallback box of stem i, -1 none); status uint8 [N]
(0 dropped for a taller stem, 1 kept with a predicted box, 2 kept with a fallback box, 3 dropped: nothing to compare, 4 no
box); crowns float64 [N, 4] (xmin, ymin, xmax, ymax) of the chosen box or NaN."""

_BOXES = "boxes must be a float64 [M, 4] array of (xmin, ymin, xmax, ymax)"
_BOX_PLOT = "box_plot must be an integer [M] array, one plot code per box"
_POINTS = "points must be a non-empty float64 [N, 2] array of (x, y)"
_POINT_PLOT = "point_plot must be an integer [N] array, one plot code per stem"
_HEIGHT = "height must be a float64 [N] array (NaN: not measured)"
_CHM = "chm must be a float64 [N] array or None"


def _plots(plots):
    if isinstance(plots, (bool, np.bool_)) or not isinstance(plots, (int, np.integer)) or not 1 <= plots < 2 ** 31 - 1:
        raise ValueError("plots must be an integer in 1 .. 2^31 - 2, the number of plot codes, got {!r}".format(plots))
    return int(plots)


def _size(size):
    try:
        size = float(size)
    except (TypeError, ValueError):
        raise ValueError("size must be a finite number above 0, got {!r}".format(size))
    if not math.isfinite(size) or size <= 0:
        raise ValueError("size must be a finite number above 0, got {!r}".format(size))
    return size


def _which(boxes, pixel_boxes, transform):
    if (boxes is None) == (pixel_boxes is None):
        raise ValueError("exactly one of boxes and pixel_boxes must be given")
    if pixel_boxes is not None and transform is None:
        raise ValueError("pixel_boxes need a transform (x0, a, y0, e)")
    if boxes is not None and transform is not None:
        raise ValueError("boxes take no transform")


def _shaped(a, tail, kind, rows, what, empty=False):
    """`a` (a host array or a tensor) if it is [rows] + tail of the dtype kind "f8" or "int"; rows=None: any number."""
    shape, dtype = tuple(a.shape), str(a.dtype).replace("torch.", "")
    ok = dtype == "float64" if kind == "f8" else dtype in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32")
    if not ok or shape[1:] != tail or len(shape) != 1 + len(tail) or (rows is not None and shape[0] != rows):
        raise ValueError(what)
    if shape[0] < 1 and not empty:
        raise ValueError(what)
    return a


def _array(a):
    return a if hasattr(a, "shape") and hasattr(a, "dtype") else np.asarray(a)


def _nearest(boxes, x, y):
    """Steps 1 and 3 for the stems (x, y) against `boxes` [K, 4]: int64 [S], the position of the nearest candidate, -1: none."""
    best = np.full(len(x), -1, np.int64)
    if not len(boxes) or not len(x):
        return best
    x0, y0, x1, y1 = (boxes[:, j][None, :] for j in range(4))
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    block = max(1, _PAIRS // len(boxes))
    for s in range(0, len(x), block):
        px, py = x[s:s + block, None], y[s:s + block, None]
        cand = (x0 <= px) & (px <= x1) & (y0 <= py) & (py <= y1)
        dx, dy = cx - px, cy - py
        d2 = dx * dx + dy * dy
        d2 = np.where(cand & ~np.isnan(d2), d2, np.inf)
        first = np.argmax(cand & (d2 == d2.min(axis=1)[:, None]), axis=1)      # the lowest index among the nearest
        best[s:s + block] = np.where(cand.any(axis=1), first, -1)
    return best


def _segments(codes, plots):
    """The stable order of the codes inside 0 .. plots-1 and start[plots + 1] of every code's run in it."""
    inside = np.flatnonzero((codes >= 0) & (codes < plots))
    order = inside[np.argsort(codes[inside], kind="stable")]
    return order, np.searchsorted(codes[order], np.arange(plots + 1))


def assign_np(boxes, box_plot, points, point_plot, height, chm=None, size=1.0, plots=None):
    """The definition (see the module's text): Assignment of host arrays.  boxes float64 [M, 4] (M may be 0), box_plot
    integer [M], points float64 [N, 2], point_plot integer [N], height float64 [N], chm float64 [N] or None, size: half the
    side of a fallback box, plots: the number of plot codes."""
    b = _shaped(np.asarray(_host(_array(boxes))), (4,), "f8", None, _BOXES, empty=True)
    bp = _shaped(np.asarray(_host(_array(box_plot))), (), "int", len(b), _BOX_PLOT, empty=True).astype(np.int64)
    p = _shaped(np.asarray(_host(_array(points))), (2,), "f8", None, _POINTS)
    pp = _shaped(np.asarray(_host(_array(point_plot))), (), "int", len(p), _POINT_PLOT).astype(np.int64)
    h = _shaped(np.asarray(_host(_array(height))), (), "f8", len(p), _HEIGHT)
    c = None if chm is None else _shaped(np.asarray(_host(_array(chm))), (), "f8", len(p), _CHM)
    size, plots = _size(size), _plots(plots)
    M, N = len(b), len(p)
    x, y = p[:, 0], p[:, 1]
    box = np.full(N, -1, np.int64)
    status = np.full(N, 4, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        fallback = np.stack([x - size, y - size, x + size, y + size], axis=1)
        valid = np.isfinite(x) & np.isfinite(y)
        border, bstart = _segments(bp, plots)
        sorder, sstart = _segments(np.where(valid, pp, -1), plots)
        for plot in np.flatnonzero(np.diff(sstart)):
            bi, si = border[bstart[plot]:bstart[plot + 1]], sorder[sstart[plot]:sstart[plot + 1]]
            near = _nearest(b[bi], x[si], y[si])                            # steps 1 and 3
            box[si[near >= 0]] = bi[near[near >= 0]]
            missing = si[near < 0]                                          # step 2, and step 3 among the fallback boxes
            box[missing] = M + missing[_nearest(fallback[missing], x[missing], y[missing])]
    chosen = np.flatnonzero(box >= 0)
    status[chosen] = np.where(box[chosen] < M, 1, 2)
    order = chosen[np.argsort(box[chosen], kind="stable")]                  # step 4: groups, ascending stem index inside
    first = np.flatnonzero(np.r_[True, box[order][1:] != box[order][:-1]]) if len(order) else np.zeros(0, np.int64)
    last = np.r_[first[1:], len(order)]
    for s, e in zip(first[last - first > 1], last[last - first > 1]):
        G = order[s:e]
        S = G[h[G] == np.max(h[G][~np.isnan(h[G])], initial=-np.inf)]
        if len(S) > 1 and c is not None:
            S = S[c[S] == np.max(c[S][~np.isnan(c[S])], initial=-np.inf)]
        kept = status[G[0]]
        status[G] = 0 if len(S) else 3
        if len(S):
            status[S[0]] = kept
    crowns = np.full((N, 4), np.nan)
    crowns[box >= M] = fallback[box[box >= M] - M]
    crowns[(box >= 0) & (box < M)] = b[box[(box >= 0) & (box < M)]]
    return Assignment(box, status, crowns)


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
_NO_DEVICE = "deeptreeattention_amd.stems runs on a ROCm device only (no CPU fallback)"


class CrownBoxes:
    """The predicted crown boxes of a site, sorted stably by plot and uploaded once: the table float64 [M, 4], box_start
    int32 [plots + 1] and the permutation back to the caller's indices.  Either boxes (float64 [M, 4] (xmin, ymin, xmax,
    ymax), M may be 0) or pixel_boxes (integer [M, 4] (row0, col0, row1, col1)) with transform = (x0, a, y0, e), through
    boundary.geo_boxes; box_plot: integer [M]; plots: the number of plot codes.  Host arrays or tensors."""

    def __init__(self, boxes=None, box_plot=None, plots=None, device="cuda", pixel_boxes=None, transform=None):
        import torch
        _which(boxes, pixel_boxes, transform)
        if pixel_boxes is not None:
            boxes = geo_boxes(pixel_boxes, transform)
        boxes = _shaped(_array(boxes), (4,), "f8", None, _BOXES, empty=True)
        if box_plot is None:
            raise ValueError(_BOX_PLOT)
        box_plot = _shaped(_array(box_plot), (), "int", boxes.shape[0], _BOX_PLOT, empty=True)
        plots = _plots(plots)
        if boxes.shape[0] >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 boxes are supported")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(_NO_DEVICE)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        b = _upload(boxes, torch.float64, dev)
        key, perm = _plot_order(_upload(box_plot, torch.int64, dev), plots)
        self._adopt(b[perm].contiguous(), _starts(key, plots), perm, plots)

    def _adopt(self, boxes, box_start, perm, plots):
        self.boxes, self.box_start, self.perm, self.plots = boxes, box_start, perm, plots
        self.device, self.n_boxes = boxes.device, int(boxes.shape[0])

    @classmethod
    def resident(cls, boxes, box_start, perm, plots):
        """A table that is already sorted by plot and lives on the device, taken as it is: boxes contiguous float64 [M, 4],
        box_start contiguous int32 [plots + 1] (the first box of every plot, M last), perm int64 [M] (the caller's index of
        every row)."""
        import torch
        plots = _plots(plots)
        ok = all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in (boxes, box_start, perm))
        if (not ok or boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 4 or box_start.dtype != torch.int32
                or tuple(box_start.shape) != (plots + 1,) or perm.dtype != torch.int64 or tuple(perm.shape) != (boxes.shape[0],)
                or not boxes.device == box_start.device == perm.device):
            raise ValueError("resident() takes contiguous tensors on one device: float64 [M, 4] boxes, int32 [plots + 1] "
                             "box_start and int64 [M] perm")
        self = cls.__new__(cls)
        self._adopt(boxes, box_start, perm, plots)
        return self

    def _stems(self, a, tail, kind, rows, what):
        import torch
        a = _shaped(_array(a), tail, kind, rows, what)
        if isinstance(a, torch.Tensor) and a.device.type != "cpu" and a.device != self.device:
            raise ValueError(what + " on " + str(self.device))
        return a

    def assign(self, points, point_plot, height, chm=None, size=1.0):
        """assign_np on the device: Assignment of tensors in the caller's order, with the caller's box indices.  points
        float64 [N, 2], point_plot integer [N], height float64 [N], chm float64 [N] or None: host arrays or tensors.  The
        stems are sorted by plot on the device; nothing here waits for it."""
        import torch
        from . import _lib
        size = _size(size)
        points = self._stems(points, (2,), "f8", None, _POINTS)
        n = int(points.shape[0])
        if n >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 stems are supported")
        point_plot = self._stems(point_plot, (), "int", n, _POINT_PLOT)
        height = self._stems(height, (), "f8", n, _HEIGHT)
        if chm is not None:
            chm = self._stems(chm, (), "f8", n, _CHM)
        if not self.boxes.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        dev, M = self.device, self.n_boxes
        key, perm = _plot_order(_upload(point_plot, torch.int64, dev), self.plots)
        p = _upload(points, torch.float64, dev)[perm].contiguous()
        h = _upload(height, torch.float64, dev)[perm].contiguous()
        c = None if chm is None else _upload(chm, torch.float64, dev)[perm].contiguous()
        codes, start = key.to(torch.int32), _starts(key, self.plots)
        choice = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        crowns = torch.empty((n, 4), dtype=torch.float64, device=dev)
        table = self.boxes if M else self.boxes.new_zeros((1, 4))           # the entry refuses a null table; no row is read
        _lib.check(_lib.lib().dta_stems_assign(_lib.ptr(table), _lib.ptr(self.box_start), M, _lib.ptr(p), _lib.ptr(codes),
                                               _lib.ptr(start), _lib.ptr(h), _lib.ptr(c), n, self.plots, size, _lib.ptr(choice),
                                               _lib.ptr(status), _lib.ptr(crowns), _lib.current_stream_ptr()),
                   "dta_stems_assign")
        # the sorted tables' indices -> the caller's, and the rows back into the caller's order
        theirs = M + perm[(choice - M).clamp(0, n - 1)]
        if M:
            theirs = torch.where(choice >= M, theirs, self.perm[choice.clamp(0, M - 1)])
        theirs = torch.where(choice < 0, choice, theirs)
        out = Assignment(torch.empty_like(theirs), torch.empty_like(status), torch.empty_like(crowns))
        out.box[perm], out.status[perm], out.crowns[perm] = theirs, status, crowns
        return out


def _upload(a, dtype, dev):
    import torch
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device=dev, dtype=dtype)


def _plot_order(codes, plots):
    """The codes with every one outside 0 .. plots-1 set to `plots`, sorted stably, and the permutation that sorts them."""
    import torch
    key = torch.where((codes >= 0) & (codes < plots), codes, torch.full_like(codes, plots))
    return torch.sort(key, stable=True)


def _starts(key, plots):
    import torch
    return torch.searchsorted(key, torch.arange(plots + 1, dtype=torch.int64, device=key.device)).to(torch.int32).contiguous()
