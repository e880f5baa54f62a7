"""Crown boxes of a tile from a detector's per-window output: what sits between a stock detector and `boxes` as canopy,
dead, boundary, dense, abundance and stems take them.  The reference gets its crowns from DeepForest's predict_tile
(src/predict.py:112-138 predict_crowns, src/generate.py:17-60 predict_trees): the detector runs over overlapping 400 px
windows of the RGB tile, every window's boxes are shifted by the window origin, and the duplicates of the overlap strips are
removed by greedy non-maximum suppression at IoU 0.15.  The detector is a stock network that torch runs (as the alive/dead
ResNet is for dead.py) and stays out of this package; the window layout, the shift, the suppression and the pixel boxes are
here, and on the device they are one chain of launches on resident tensors (dta_mosaic, csrc/mosaic.hip): no sort, no
N x N table, no read-back.

windows(height, width, patch_size, patch_overlap): DeepForest's sliding windows, (x, y, w, h) rows, x-major.

nms_np, the definition.  boxes are float32 (xmin, ymin, xmax, ymax) in window pixels, window[i] the row of origins (x, y) of
box i.  Every float32 operation is rounded on its own (no fused multiply-add, no float64 intermediate).
    tile    = box + (ox, oy, ox, oy), float32 adds (window None: the boxes are tile coordinates; a window index out of
              range: the box stays as it is)
    status 3, refused: a coordinate of tile or the score is not finite; xmax < xmin or ymax < ymin; xmax - xmin or
              ymax - ymin above max_side (a detector box cannot exceed its window); a window index out of range
    status 2, masked: mask[i] == 0 (the caller's score threshold).  Refused and masked boxes take no part.
    order:    j precedes i iff score[j] > score[i], or the scores are equal and j < i (torchvision's sort is unstable on
              equal scores and detector scores do tie: the lowest index wins here; nothing finer is promised)
    overlap:  area = (x2 - x1) * (y2 - y1);  inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1));
              j suppresses i iff inter / ((area_i + area_j) - inter) > iou_threshold, strictly; 0 / 0 is NaN and false, so
              zero-area boxes are never suppressed, as in torchvision
    greedy:   walk the order; a box not yet suppressed is kept (status 1) and suppresses every later box it overlaps
              (status 0).  winner[i] is the first kept box in the order that overlaps i for status 0, i for status 1, else -1
This restates torchvision.ops.nms with DeepForest's iou_threshold = 0.15.  Neither library is installed where this package
is built and the reference tree holds no copy of them, so there is no recorded fixture: the tests hold nms_np to a second,
differently written definition instead (nms_fixpoint_np: the unique fixpoint of "dropped when a preceding overlapping box is
kept, kept when all of them are dropped", by Jacobi rounds over the explicit pair list) and to hand-worked cases.

pixel_boxes_np: int32 (row0, col0, row1, col1), half-open: floor(ymin), floor(xmin), ceil(ymax), ceil(xmax), each clamped
to the raster -- the smallest pixel box that covers the detection; zeros for a row with a coordinate that is not finite or
xmax < xmin or ymax < ymin.  This is this package's rule, not rasterio.windows.from_bounds followed by the rounding of
`read`: that rounding depends on the rasterio version and rasterio is not installed to record it.

The device route (mosaic) equals the definition bit for bit; how it gets there -- cells, rounds, the tail launch -- is in
include/dta_hip.h and DESIGN.md.  Out of scope: the detector and its weights, class-aware and soft NMS, polygons.
"""
import collections

import numpy as np

PATCH_SIZE = 400                 # DeepForest's window, and the default max_side
CHUNK = 1024                     # DTA_MOSAIC_CHUNK: boxes staged through LDS at a time
ROUNDS = 12                      # DTA_MOSAIC_ROUNDS: parallel rounds in front of the tail launch
MAX_EXTENT = 1 << 20             # the largest height / width / max_side
DROPPED, KEPT, MASKED, REFUSED, UNDECIDED = 0, 1, 2, 3, 4
_NO_DEVICE = "deeptreeattention_amd.mosaic runs on a ROCm device only (no CPU fallback)"


class Mosaic(collections.namedtuple("Mosaic", "status winner boxes pixel_boxes")):
    """status uint8 [N], winner int32 [N], boxes float32 [N][4] (tile coordinates), pixel_boxes int32 [N][4]
    (row0, col0, row1, col1), in the caller's order."""
    __slots__ = ()

    @property
    def keep(self):
        """bool [N]: status == 1."""
        return self.status == KEPT


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _axis(n, patch_size, patch_overlap):
    w = min(patch_size, n)
    s = w - int(np.floor(w * patch_overlap))
    if s < 1:
        raise ValueError("patch_overlap={!r} leaves no step for a window of {}".format(patch_overlap, w))
    last = n - w
    offs = list(range(0, last + 1, s))
    if offs[-1] != last:
        offs.append(last)
    return offs, w


def windows(height, width, patch_size=PATCH_SIZE, patch_overlap=0.05):
    """int32 [K][4] (x, y, w, h): DeepForest's sliding windows.  Per axis of length n: w = min(patch_size, n),
    s = w - floor(w * patch_overlap), offsets 0, s, 2s, ... <= n - w and n - w itself if it is not the last of them; for each
    x offset all y offsets."""
    height, width, patch_size = int(height), int(width), int(patch_size)
    if height < 1 or width < 1:
        raise ValueError("height and width must be >= 1")
    if patch_size < 1:
        raise ValueError("patch_size must be >= 1")
    if not 0 <= patch_overlap < 1:
        raise ValueError("patch_overlap must be in [0, 1), got {!r}".format(patch_overlap))
    xs, w = _axis(width, patch_size, patch_overlap)
    ys, h = _axis(height, patch_size, patch_overlap)
    return np.array([(x, y, w, h) for x in xs for y in ys], np.int32)


def _threshold(iou_threshold):
    t = np.float32(iou_threshold)
    if not 0 <= t <= 1:
        raise ValueError("iou_threshold must be in [0, 1], got {!r}".format(iou_threshold))
    return t


def _max_side(max_side):
    m = np.float32(PATCH_SIZE if max_side is None else max_side)
    if not 0 < m <= MAX_EXTENT:
        raise ValueError("max_side must be in (0, 2^20], got {!r}".format(max_side))
    return m


def _host_inputs(boxes, scores, window, origins, mask):
    b, s = np.asarray(_host(boxes)), np.asarray(_host(scores))
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.dtype != np.float32:
        raise ValueError("boxes must be a non-empty float32 [N, 4] array of (xmin, ymin, xmax, ymax)")
    n = b.shape[0]
    if s.shape != (n,) or s.dtype != np.float32:
        raise ValueError("scores must be a float32 [{}] array".format(n))
    if (window is None) != (origins is None):
        raise ValueError("window and origins go together")
    w = o = None
    if window is not None:
        w, o = np.asarray(_host(window)), np.asarray(_host(origins))
        if w.shape != (n,) or w.dtype.kind not in "iu":
            raise ValueError("window must be an integer [{}] array".format(n))
        if o.ndim != 2 or o.shape[1] != 2 or o.shape[0] < 1 or o.dtype.kind not in "iu":
            raise ValueError("origins must be a non-empty integer [K, 2] array of (x, y)")
        if np.abs(o.astype(np.int64)).max() >= 1 << 24:
            raise ValueError("origins must be below 2^24 (exact in float32)")
    m = None
    if mask is not None:
        m = np.asarray(_host(mask))
        if m.shape != (n,) or m.dtype not in (np.bool_, np.uint8):
            raise ValueError("mask must be a bool / uint8 [{}] array".format(n))
    return b, s, w, o, m


def _prepare_np(boxes, scores, window, origins, mask, max_side):
    """(tile float32 [N][4], status uint8 [N] with 4 for the boxes that take part)."""
    b, s, w, o, m = _host_inputs(boxes, scores, window, origins, mask)
    side = _max_side(max_side)
    tile = b.copy()
    known = np.ones(len(b), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if w is not None:
            w = w.astype(np.int64)
            known = (w >= 0) & (w < len(o))
            shift = o[np.where(known, w, 0)].astype(np.float32)
            tile[known] = (b + np.concatenate([shift, shift], axis=1))[known]
        x1, y1, x2, y2 = tile.T
        refused = (~known | ~np.isfinite(tile).all(axis=1) | ~np.isfinite(s) | (x2 < x1) | (y2 < y1)
                   | (x2 - x1 > side) | (y2 - y1 > side))
    status = np.full(len(b), UNDECIDED, np.uint8)
    if m is not None:
        status[m == 0] = MASKED
    status[refused] = REFUSED
    return tile, s, status


def _iou_over(tile, area, i, c, thr):
    """bool [len(c)]: box i and the boxes c overlap by more than thr."""
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.maximum(np.float32(0), np.minimum(tile[c, 2], tile[i, 2]) - np.maximum(tile[c, 0], tile[i, 0]))
        h = np.maximum(np.float32(0), np.minimum(tile[c, 3], tile[i, 3]) - np.maximum(tile[c, 1], tile[i, 1]))
        inter = w * h
        return inter / ((area[c] + area[i]) - inter) > thr


def nms_np(boxes, scores, window=None, origins=None, mask=None, iou_threshold=0.15, max_side=None):
    """The definition (module docstring): (status uint8 [N], winner int32 [N], tile_boxes float32 [N][4]).
    The walk looks, for every kept box, only at the boxes whose xmin lies where an intersection is possible (an x-sorted
    index, a superset of the boxes it can overlap); the result is that of the plain greedy walk."""
    thr = _threshold(iou_threshold)
    tile, s, status = _prepare_np(boxes, scores, window, origins, mask, max_side)
    n = len(tile)
    winner = np.full(n, -1, np.int32)
    part = np.flatnonzero(status == UNDECIDED)
    if len(part) == 0:
        return status, winner, tile
    area = (tile[:, 2] - tile[:, 0]) * (tile[:, 3] - tile[:, 1])
    order = part[np.lexsort((part, -s[part]))]                   # by falling score, then by rising index
    rank = np.full(n, -1, np.int64)
    rank[order] = np.arange(len(order))
    by_x = part[np.argsort(tile[part, 0], kind="stable")]
    x_sorted = tile[by_x, 0].astype(np.float64)
    widest = float((tile[part, 2].astype(np.float64) - tile[part, 0]).max())
    for i in order:
        if status[i] != UNDECIDED:
            continue
        status[i] = KEPT
        winner[i] = i
        lo = np.searchsorted(x_sorted, float(tile[i, 0]) - widest * 1.000001 - 1e-3, "left")
        hi = np.searchsorted(x_sorted, float(tile[i, 2]), "left")
        c = by_x[lo:hi]
        c = c[(status[c] == UNDECIDED) & (rank[c] > rank[i])]
        c = c[_iou_over(tile, area, i, c, thr)]
        status[c] = DROPPED
        winner[c] = i
    return status, winner, tile


def nms_fixpoint_np(boxes, scores, window=None, origins=None, mask=None, iou_threshold=0.15, max_side=None, block=512):
    """The second definition, for the tests: (status uint8 [N], depth).  All pairs (j precedes i, j overlaps i) are listed
    from the dense N x N tests; then Jacobi rounds -- every box reads the states of the round before -- of: an undecided box
    is dropped when one of its j is kept, kept when all of its j are dropped.  depth is the number of rounds until nothing
    is undecided."""
    thr = _threshold(iou_threshold)
    tile, s, status = _prepare_np(boxes, scores, window, origins, mask, max_side)
    part = np.flatnonzero(status == UNDECIDED)
    area = (tile[:, 2] - tile[:, 0]) * (tile[:, 3] - tile[:, 1])
    later, earlier = [], []
    for k in range(0, len(part), block):
        rows = part[k:k + block]
        for i in rows:
            pre = part[(s[part] > s[i]) | ((s[part] == s[i]) & (part < i))]
            pre = pre[_iou_over(tile, area, i, pre, thr)]
            later.append(np.full(len(pre), i, np.int64))
            earlier.append(pre)
    later = np.concatenate(later) if later else np.zeros(0, np.int64)
    earlier = np.concatenate(earlier) if earlier else np.zeros(0, np.int64)
    n, depth = len(tile), 0
    while (status == UNDECIDED).any():
        depth += 1
        kept_before = np.bincount(later[status[earlier] == KEPT], minlength=n) > 0
        open_before = np.bincount(later[status[earlier] == UNDECIDED], minlength=n) > 0
        undecided = status == UNDECIDED
        new = status.copy()
        new[undecided & kept_before] = DROPPED
        new[undecided & ~kept_before & ~open_before] = KEPT
        if (new == status).all():
            raise AssertionError("the rounds stopped with undecided boxes")
        status = new
    return status, depth


def _extent(height, width):
    height, width = int(height), int(width)
    if not (1 <= height <= MAX_EXTENT and 1 <= width <= MAX_EXTENT):
        raise ValueError("height and width must be 1 .. 2^20")
    return height, width


def pixel_boxes_np(tile_boxes, height, width):
    """The definition: int32 [N][4] (row0, col0, row1, col1), half-open, of float32 tile boxes (module docstring)."""
    t = np.asarray(_host(tile_boxes))
    if t.ndim != 2 or t.shape[1] != 4 or t.dtype != np.float32:
        raise ValueError("tile_boxes must be a float32 [N, 4] array of (xmin, ymin, xmax, ymax)")
    height, width = _extent(height, width)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(t).all(axis=1) & ~(t[:, 2] < t[:, 0]) & ~(t[:, 3] < t[:, 1])
        safe = np.where(ok[:, None], t, np.float32(0))
        h32, w32 = np.float32(height), np.float32(width)
        out = np.stack([np.clip(np.floor(safe[:, 1]), 0, h32), np.clip(np.floor(safe[:, 0]), 0, w32),
                        np.clip(np.ceil(safe[:, 3]), 0, h32), np.clip(np.ceil(safe[:, 2]), 0, w32)], axis=1)
    return np.where(ok[:, None], out, 0).astype(np.int32)


def grid(n, height, width, max_side=None):
    """(cell side float, cells across, cells down) of a call with n boxes: dta_mosaic_grid (host only, no device)."""
    from . import _lib
    L, C = _lib.lib(), _lib.C
    height, width = _extent(height, width)
    cell, gx, gy = C.c_float(), C.c_int(), C.c_int()
    _lib.check(L.dta_mosaic_grid(int(n), height, width, float(_max_side(max_side)), C.byref(cell), C.byref(gx), C.byref(gy)),
               "dta_mosaic_grid")
    return cell.value, gx.value, gy.value


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
_WORKSPACES = collections.OrderedDict()      # (device, bytes) -> uint8 tensor; the few sizes last used
_WORKSPACES_KEPT = 4


def _workspace(dev, need):
    import torch
    key = (str(dev), need)
    ws = _WORKSPACES.pop(key, None)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _WORKSPACES[key] = ws
    while len(_WORKSPACES) > _WORKSPACES_KEPT:
        _WORKSPACES.popitem(last=False)
    return ws


def _device_of(*arrays):
    import torch
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    return torch.device("cuda", torch.cuda.current_device())


def _check(a, shape, kind, what):
    """a: a NumPy array or a tensor; kind: f (float32), i (integer), m (bool / uint8)."""
    import torch
    if isinstance(a, torch.Tensor):
        k = {torch.float32: "f", torch.int32: "i", torch.int64: "i", torch.bool: "m", torch.uint8: "m"}.get(a.dtype)
    else:
        k = "f" if a.dtype == np.float32 else "m" if a.dtype in (np.bool_, np.uint8) else "i" if a.dtype.kind in "iu" else None
    if k != kind or a.ndim != len(shape) or a.shape[0] < 1 or any(e is not None and a.shape[d] != e for d, e in enumerate(shape)):
        raise ValueError(what)


def mosaic(boxes, scores, window=None, origins=None, mask=None, *, height, width, iou_threshold=0.15, max_side=None,
           rounds=None, tail=True):
    """nms_np and pixel_boxes_np on the device (dta_mosaic): Mosaic(status, winner, boxes, pixel_boxes) of device tensors in
    the caller's order, `.keep` the bool mask canopy / abundance take.  boxes float32 [N, 4], scores float32 [N], window
    int32 / int64 [N] with origins integer [K, 2] (windows()[:, :2]) or neither, mask bool / uint8 [N]: device tensors or
    host arrays (uploaded).  Origins on the device are not checked against 2^24.  rounds / tail are for measurements
    (tools/mosaicbench.py): tail=False leaves boxes that the rounds did not decide at status 4.  Nothing here waits for the
    device."""
    import torch
    from . import _lib
    thr, side = _threshold(iou_threshold), _max_side(max_side)
    height, width = _extent(height, width)
    rounds = -1 if rounds is None else int(rounds)
    if rounds > _lib.MOSAIC_MAX_ROUNDS:
        raise ValueError("rounds must be at most {}".format(_lib.MOSAIC_MAX_ROUNDS))
    if (window is None) != (origins is None):
        raise ValueError("window and origins go together")
    b, s, w, o, m = (a if a is None or (isinstance(a, torch.Tensor) and a.is_cuda) else np.asarray(_host(a))
                     for a in (boxes, scores, window, origins, mask))
    _check(b, (None, 4), "f", "boxes must be a non-empty float32 [N, 4] array of (xmin, ymin, xmax, ymax)")
    n = int(b.shape[0])
    _check(s, (n,), "f", "scores must be a float32 [{}] array".format(n))
    k = 0
    if w is not None:
        _check(w, (n,), "i", "window must be an int32 / int64 [{}] array".format(n))
        _check(o, (None, 2), "i", "origins must be a non-empty integer [K, 2] array of (x, y)")
        k = int(o.shape[0])
        if isinstance(o, np.ndarray) and np.abs(o.astype(np.int64)).max() >= 1 << 24:
            raise ValueError("origins must be below 2^24 (exact in float32)")
    if m is not None:
        _check(m, (n,), "m", "mask must be a bool / uint8 [{}] array".format(n))
    dev = _device_of(b, s, w, o, m)

    def up(a, dtype):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) if a.dtype.kind in "iu" and dtype != torch.uint8 else a))
        elif a.device != dev:
            raise ValueError("all tensors must be on {}".format(dev))
        if a.dtype == torch.bool:
            a = a.contiguous().view(torch.uint8)
        return a.to(device=dev, dtype=dtype).contiguous()

    b, s, o, m = up(b, torch.float32), up(s, torch.float32), up(o, torch.int32), up(m, torch.uint8)
    if w is not None:
        w = up(w, torch.int64)
        w = torch.where((w < 0) | (w >= k), torch.full_like(w, -1), w).to(torch.int32)      # an int64 index must not wrap into range
    L = _lib.lib()
    need = int(L.dta_mosaic_workspace_bytes(n, height, width, float(side)))
    if need == 0:
        raise ValueError("dta_mosaic_workspace_bytes: " + L.dta_last_error().decode())
    ws = _workspace(dev, need)
    out = Mosaic(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                 torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev))
    opt = _lib.MosaicOptions(height, width, k, float(side), float(thr), rounds, 0 if tail else 1)
    with torch.cuda.device(dev):
        _lib.check(L.dta_mosaic(_lib.ptr(b), _lib.ptr(s), _lib.ptr(w), _lib.ptr(o), _lib.ptr(m), n, _lib.C.byref(opt),
                                _lib.ptr(out.status), _lib.ptr(out.winner), _lib.ptr(out.boxes), _lib.ptr(out.pixel_boxes),
                                _lib.ptr(ws), need, _lib.current_stream_ptr()), "dta_mosaic")
    return out


def predict_tile(detect, image, patch_size=PATCH_SIZE, patch_overlap=0.05, iou_threshold=0.15, score_threshold=None, batch=8):
    """DeepForest's predict_tile around a detector: Mosaic of the crowns of `image`, a resident uint8 [H][W][3] tensor.
    detect(list of window views [h][w][3]) returns one {"boxes": float32 [n, 4], "scores": float32 [n]} per view, device
    tensors, as torchvision's detection models do.  The windows are views of the image, `batch` of them per detect call;
    boxes, scores and window indices are concatenated on the device and go through mosaic(max_side=patch_size).
    score_threshold: boxes with score <= it are masked (status 2).  A tile without a single box gives empty tensors.
    Nothing here waits for the device."""
    import torch
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
        raise ValueError("image must be a uint8 [H][W][3] tensor")
    if not image.is_cuda:
        raise RuntimeError(_NO_DEVICE)
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    height, width = int(image.shape[0]), int(image.shape[1])
    wins = windows(height, width, patch_size, patch_overlap)
    boxes, scores, index = [], [], []
    for k0 in range(0, len(wins), batch):
        rows = wins[k0:k0 + batch]
        found = detect([image[y:y + h, x:x + w] for x, y, w, h in rows.tolist()])
        if len(found) != len(rows):
            raise ValueError("detect returned {} results for {} windows".format(len(found), len(rows)))
        for k, f in enumerate(found, k0):
            b, s = f["boxes"], f["scores"]
            if b.dim() != 2 or b.shape[1] != 4 or s.shape != (b.shape[0],):
                raise ValueError("detect must return boxes [n, 4] and scores [n] per window")
            boxes.append(b.to(device=image.device, dtype=torch.float32))
            scores.append(s.to(device=image.device, dtype=torch.float32))
            index.append(torch.full((b.shape[0],), k, dtype=torch.int32, device=image.device))
    boxes, scores, index = torch.cat(boxes), torch.cat(scores), torch.cat(index)
    if boxes.shape[0] == 0:
        return Mosaic(torch.empty(0, dtype=torch.uint8, device=image.device), torch.empty(0, dtype=torch.int32, device=image.device),
                      boxes, torch.empty((0, 4), dtype=torch.int32, device=image.device))
    mask = None if score_threshold is None else scores > float(score_threshold)
    return mosaic(boxes, scores, index, wins[:, :2], mask, height=height, width=width, iou_threshold=iou_threshold,
                  max_side=patch_size)
