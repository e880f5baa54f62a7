"""Dense per-pixel window prediction over a hyperspectral raster: the reference's `bounds_to_pixel` (src/patches.py:50-83:
one 11x11 window per pixel of a crown box, read with boundless=True) followed by `TreeModel.predict_dataloader`
(src/main.py:165-205), without ever slicing a window on the host.

The reference's preprocessing is per pixel position (drop 10 + 10 bands, min-max over the bands of that pixel,
src/utils.py:36-57) and an 11x11 window resized to 11x11 with NEAREST is the identity, so the preprocessed window equals
the window of the preprocessed raster, bit for bit (a zero-filled out-of-bounds pixel stays zero: its range is below
scikit-learn's "constant" threshold).  Hence:

    DenseRaster          one host-to-device copy of the raw raster and ONE normalise launch (dta_raster_normalise)
    DenseRaster.from_reflectance   the same raster straight from a pixel-interleaved reflectance cube: band selection, window,
                         min-max and transpose in one pass per strip of rows (reflectance.py; dta_reflectance_normalise)
    window_origins       pixel boxes -> window origins + crown offsets (pure host function)
    DenseRaster.windows  origins -> the float32 batch or the first conv's bf16 tiles (dta_gather_windows[_tiles])
    predict_windows      gather -> eval forward -> softmax / top-2 per batch, no host synchronisation inside the loop;
                         with crown offsets also the per-crown mean, top-2 and count (dta_crown_reduce)
    predict_map          a label map and a score map of a raster region

For a multi-stage model (engine.MultiStagePredictor: levels x years networks on the same windows, then the hierarchy walk):

    DenseRaster.windows_years    one batch of windows out of every year's raster in ONE launch, with the years' 0/1 flags
                                 taken from the values on their way out (dta_gather_windows_years)
    predict_windows_multistage   gather -> MultiStagePredictor.ensemble(year_flags=...) per batch: a species label, its score
                                 and the deciding level per window; with crown offsets also per crown (crown_resolve)
    predict_map_multistage       a species map, a score map and a level map of a raster region
    crown_resolve                every level's per-crown mean and top-2, the walk on them, the crown's window votes
                                 (dta_crown_resolve)

For the site-metadata fusion model (engine.MetadataPredictor; every window of a raster shares the raster's site):

    predict_windows_metadata     gather -> the sensor model's eval forward -> the whole head, softmax and top-2 in ONE launch
                                 per batch (dta_meta_predict with the raster's site); with crown offsets also crown_reduce
    predict_map_metadata         a label map and a score map of a raster region

For the reference's production path -- ONE crop per crown: patches.crop (src/patches.py:5-30) cuts the crown's bounding box out
of the tile, utils.load_image (src/utils.py:59-79) preprocesses it and resizes it to 11x11 with NEAREST -- the same per-pixel
argument goes one step further: a NEAREST resize only selects pixels, so the resized, preprocessed crop of a box is an index
selection from the normalised raster, bit for bit what preprocess.preprocess_batch gives for the host-sliced raw crop:

    crop_boxes                   pixel boxes -> boxes clipped to the raster as rasterio's non-boundless read clips (host)
    DenseRaster.crops            boxes -> the float32 batch or the first conv's bf16 tiles, resized to size x size, with the
                                 training flips on request (dta_gather_crops[_tiles]); crops_years: every year in ONE launch
                                 with the years' flags (dta_gather_crops_years)
    predict_crops, predict_crops_multistage, predict_crops_metadata
                                 the three loops above with that gather in place of the window gather: one row per box; with
                                 one crop per crown the multi-stage result is the reference's gather_predictions + ensemble
    (no share_conv1 here: a resized crop's 3x3 neighbours are not raster neighbours unless the box is exactly 11x11)

The species of a crown with several windows is THIS package's definition: per level the mean over the crown's windows
(crown_reduce_np), then the walk over the levels' top-1 of those means (Hierarchy.resolve_np).  The reference has none: its
`gather_predictions` (multi_stage.py:368-402) takes a flat argmax over one row per individual.  With one window per crown
the definition is the reference's, exactly.

With share_conv1=True (opt-in; single Hang2020 / spectral_network / spatial_network, 11x11) predict_windows / predict_map
compute the first conv ONCE PER RASTER instead of once per window -- it sits in front of every pool, so its output at a
window position depends only on the raster pixel underneath and on which taps fall outside the window (nine cases):

    DenseRaster.conv1_table      raster + the network's first conv -> Conv1Table (dta_raster_conv1_table), once per call
    Conv1Table.gather            origins -> the first conv's output of a batch, written into the Predictor's workspace
                                 (dta_gather_conv1_windows); the forward then starts behind its first conv (dta_conv1_forward)

predict_windows_multistage / predict_map_multistage take share_conv1=True too (opt-in; the rasters in the MODELS'
precision): every level's year-y network reads year y's raster, so a year's first convs of ALL levels are one table --

    Conv1TableYears              per year: raster + the levels' year-y first convs side by side -> one table and the raster's
                                 non-zero mask (dta_conv1_multistage_raster_table), once per call; a missing year: the biases
    Conv1TableYears.gather       origins -> the first convs of a batch for every level x year, written into the
                                 MultiStagePredictor's workspace in ONE launch that also sets the years' flags
                                 (dta_conv1_multistage_gather_windows); the grouped forward then starts behind its first
                                 convs (dta_conv1_multistage_predict_ensemble)

`gather_windows_np`, `gather_crops_np`, `crown_reduce_np` and `crown_resolve_np` are the written-down meaning of the gathers, reduce and
resolve kernels, `conv1_table_np` and `gather_conv1_np` that of the first-conv table and its gather, `conv1_mask_np`,
`gather_conv1_years_np` and `year_flags_np` that of the multi-stage form.
File reading and georeferencing stay with the caller, as in preprocess.py."""
import collections

import numpy as np
import torch

from . import _lib
from .Hang2020 import forward_only_descs
from .preprocess import PatchTiles, out_bands, _DTYPES

WINDOW = 11     # Hang et al. 2020: one 11x11 window per pixel
_TORCH_DTYPES = {torch.float32: _lib.CROP_F32, torch.int16: _lib.CROP_I16, torch.uint8: _lib.CROP_U8}


# ---------------------------------------------------------------------------------------------------------------------
# host definitions
# ---------------------------------------------------------------------------------------------------------------------
def window_origins(boxes, anchor="corner", size=WINDOW):
    """boxes: pixel boxes (row0, col0, row1, col1), half-open.  One window per pixel of each box, row-major within the box.
    Returns (origins int32 [N, 2] = (row, col) of each window's top-left corner, crown_offsets int64 [len(boxes) + 1]).
    anchor="corner": the pixel is the window's top-left (the reference's bounds_to_pixel: Window(col_off=col, row_off=row));
    anchor="center": the pixel is the window's centre (the paper's form): origins shifted by -(size // 2)."""
    if anchor not in ("corner", "center"):
        raise ValueError("anchor must be 'corner' or 'center', got {!r}".format(anchor))
    shift = size // 2 if anchor == "center" else 0
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    parts, offsets = [], np.zeros(len(boxes) + 1, dtype=np.int64)
    for k, (r0, c0, r1, c1) in enumerate(boxes):
        h, w = max(int(r1 - r0), 0), max(int(c1 - c0), 0)
        rr, cc = np.meshgrid(np.arange(r0, r0 + h), np.arange(c0, c0 + w), indexing="ij")
        parts.append(np.stack([rr.reshape(-1), cc.reshape(-1)], axis=1) - shift)
        offsets[k + 1] = offsets[k] + h * w
    origins = np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), dtype=np.int64)
    return origins.astype(np.int32).reshape(-1, 2), offsets


def gather_windows_np(raster_norm, origins, size=WINDOW):
    """What dta_gather_windows computes: raster_norm [C][H][W] -> [N][C][size][size]; window n covers rows
    origins[n, 0] .. + size and columns origins[n, 1] .. + size of the raster, positions outside it are zero."""
    raster_norm = np.asarray(raster_norm)
    origins = np.asarray(origins).reshape(-1, 2)
    Cb, Hh, Ww = raster_norm.shape
    out = np.zeros((len(origins), Cb, size, size), dtype=raster_norm.dtype)
    for n, (r, c) in enumerate(origins):
        r, c = int(r), int(c)
        ra, rb, ca, cb = max(r, 0), min(r + size, Hh), max(c, 0), min(c + size, Ww)
        if ra < rb and ca < cb:
            out[n, :, ra - r:rb - r, ca - c:cb - c] = raster_norm[:, ra:rb, ca:cb]
    return out


def crop_boxes(boxes, height, width, empty="raise"):
    """boxes: pixel boxes (row0, col0, row1, col1), half-open.  Each is clipped to the raster [0, height) x [0, width): what
    rasterio's non-boundless read(window=...) of the reference's patches.crop returns is the intersection.  An empty
    intersection raises ValueError naming the box (reference patches.py:13-14); with empty="zero" it becomes the
    degenerate box (0, 0, 0, 0), which DenseRaster.crops turns into an all-zero crop.  Returns int32 [N, 4].  A pure host
    function."""
    if empty not in ("raise", "zero"):
        raise ValueError("empty must be 'raise' or 'zero', got {!r}".format(empty))
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    out = np.stack([np.clip(b[:, 0], 0, height), np.clip(b[:, 1], 0, width),
                    np.clip(b[:, 2], 0, height), np.clip(b[:, 3], 0, width)], axis=1)
    none = (out[:, 2] <= out[:, 0]) | (out[:, 3] <= out[:, 1])
    if none.any():
        if empty == "raise":
            k = int(np.flatnonzero(none)[0])
            raise ValueError("box {} {} does not intersect the {} x {} raster".format(k, tuple(int(v) for v in b[k]), height, width))
        out[none] = 0
    return out.astype(np.int32)


def nearest_index(out_size, in_size):
    """The source index of a NEAREST resize from in_size to out_size (ATen, what torchvision dispatches to):
    min(floor(dst * float32(in / out)), in - 1), in float32 -- an integer dst * in // out is not the same function."""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def gather_crops_np(raster_norm, boxes, size=WINDOW, flip=False):
    """What dta_gather_crops computes: raster_norm [C][H][W] -> [N][C][size][size]; crop n is box n = (row0, col0, row1,
    col1) of the raster resized to size x size with NEAREST: pixel (i, j) is raster pixel (row0 + nearest_index(size, h)[i],
    col0 + nearest_index(size, w)[j]), a position outside the raster zero.  flip: both axes reversed after the resize (the
    training flips).  A box with h <= 0 or w <= 0: zeros.  A pure selection: the raster's dtype and bits."""
    raster_norm = np.asarray(raster_norm)
    boxes = np.asarray(boxes).reshape(-1, 4)
    Cb, Hh, Ww = raster_norm.shape
    out = np.zeros((len(boxes), Cb, size, size), dtype=raster_norm.dtype)
    for n, (r0, c0, r1, c1) in enumerate(boxes):
        h, w = int(r1) - int(r0), int(c1) - int(c0)
        if h <= 0 or w <= 0:
            continue
        rows, cols = int(r0) + nearest_index(size, h), int(c0) + nearest_index(size, w)
        if flip:
            rows, cols = rows[::-1], cols[::-1]
        inside = ((rows >= 0) & (rows < Hh))[:, None] & ((cols >= 0) & (cols < Ww))[None, :]
        picked = raster_norm[:, np.clip(rows, 0, Hh - 1)][:, :, np.clip(cols, 0, Ww - 1)]
        out[n] = np.where(inside[None], picked, np.zeros((), dtype=raster_norm.dtype))
    return out


Conv1TableNP = collections.namedtuple("Conv1TableNP", "data height width")


def conv1_class(i, size=WINDOW):
    """Which taps of a 3x3 conv fall outside a window of side `size` at row (or column) i of it: 0 = the first row (the
    tap at -1 is outside), 2 = the last row (the tap at +1 is), 1 = neither."""
    return 0 if i == 0 else (2 if i == size - 1 else 1)


def conv1_table_np(raster_norm, weight, bias):
    """What dta_raster_conv1_table computes, in the dtype of its arguments (float64 for the definition).
    raster_norm [C][H][W], weight [cols][C][3][3] (the branches' first-conv weights concatenated along cols), bias [cols].
        T[q][u][v][n]   = sum_k weight[n][k][u][v] * raster_norm[k][q]                (0 for q outside the raster)
        A[p][rc][cc][n] = bias[n] + sum_{u in R(rc)} sum_{v in R(cc)} T[p + (u - 1, v - 1)][u][v][n]
        R(0) = {1, 2} (first row / column of the window), R(1) = {0, 1, 2}, R(2) = {0, 1} (last row / column)
    each element one accumulator: the bias first, then the taps in ascending (u, v).  Positions p: the raster extended by a
    one-pixel ring, (H + 2) x (W + 2) row-major, then one far-outside row (every tap on zero input: the bias).
    Returns Conv1TableNP(data [(H + 2) * (W + 2) + 1][9][cols], H, W); the class index is rc * 3 + cc."""
    x, w, b = np.asarray(raster_norm), np.asarray(weight), np.asarray(bias)
    Cb, Hh, Ww = x.shape
    cols = w.shape[0]
    if w.shape != (cols, Cb, 3, 3) or b.shape != (cols,):
        raise ValueError("weight must be [cols][{}][3][3] and bias [cols]".format(Cb))
    T = np.zeros((Hh + 4, Ww + 4, 3, 3, cols), dtype=x.dtype)         # two pixels of zero around the raster
    T[2:Hh + 2, 2:Ww + 2] = np.einsum("khw,nkuv->hwuvn", x, w.astype(x.dtype))
    R = ((1, 2), (0, 1, 2), (0, 1))
    A = np.empty(((Hh + 2) * (Ww + 2) + 1, 9, cols), dtype=x.dtype)
    for rc in range(3):
        for cc in range(3):
            acc = np.broadcast_to(b.astype(x.dtype), (Hh + 2, Ww + 2, cols)).copy()
            for u in R[rc]:
                for v in R[cc]:
                    acc = acc + T[u:u + Hh + 2, v:v + Ww + 2, u, v]     # position r (from -1) + (u - 1) is padded row r + u + 1
            A[:-1, rc * 3 + cc] = acc.reshape(-1, cols)
    A[-1] = b.astype(x.dtype)
    return Conv1TableNP(A, Hh, Ww)


def gather_conv1_np(table, origins, size=WINDOW):
    """What dta_gather_conv1_windows computes: table = Conv1TableNP (or a Conv1Table read back: Conv1Table.numpy()),
    origins [N][2] -> [N][size * size][cols]: row i * size + j of window n is table[o_n + (i, j)][rc(i)][cc(j)], a position
    beyond the ring reading the far-outside row.  A pure copy: the result has the table's dtype and bits."""
    data, Hh, Ww = table.data, table.height, table.width
    origins = np.asarray(origins).reshape(-1, 2)
    out = np.empty((len(origins), size * size, data.shape[2]), dtype=data.dtype)
    far = (Hh + 2) * (Ww + 2)
    for n, (r, c) in enumerate(origins):
        for i in range(size):
            for j in range(size):
                rr, cc = int(r) + i, int(c) + j
                pos = (rr + 1) * (Ww + 2) + (cc + 1) if -1 <= rr <= Hh and -1 <= cc <= Ww else far
                out[n, i * size + j] = data[pos, conv1_class(i, size) * 3 + conv1_class(j, size)]
    return out


def conv1_mask_np(raster_norm):
    """The non-zero mask dta_conv1_multistage_raster_table writes next to a year's table: uint8 [(H + 2) * (W + 2) + 1], one
    byte per table position -- 1 where the raster pixel under it has a non-zero stored element (NaN counts as non-zero),
    0 on the ring and in the far-outside row.  raster_norm [C][H][W] as stored (a bf16 raster: its bf16 values);
    None (a missing year): the single zero byte."""
    if raster_norm is None:
        return np.zeros(1, dtype=np.uint8)
    x = np.asarray(raster_norm)
    Cb, Hh, Ww = x.shape
    grid = np.zeros((Hh + 2, Ww + 2), dtype=np.uint8)
    grid[1:-1, 1:-1] = (~(x == 0)).any(axis=0)
    return np.concatenate([grid.reshape(-1), np.zeros(1, dtype=np.uint8)])


def gather_conv1_years_np(tables, origins, levels, size=WINDOW):
    """What dta_conv1_multistage_gather_windows writes.  tables: one Conv1TableNP per year with data
    [(H + 2) * (W + 2) + 1][9][levels * cols] (the levels side by side); a missing year's data is the far-outside row alone,
    [1][9][levels * cols], and every position reads it.  Returns [levels][years][N][size * size][cols]: slice (l, y) is
    gather_conv1_np on columns cols * l .. cols * l + cols - 1 of year y's table -- the first conv of level l's year-y network,
    group l * years + y of the multi-stage forward.  A pure copy: the table's dtype and bits."""
    origins = np.asarray(origins).reshape(-1, 2)
    width = tables[0].data.shape[2]
    if width % levels:
        raise ValueError("{} table columns do not divide into {} levels".format(width, levels))
    cols = width // levels
    out = np.empty((levels, len(tables), len(origins), size * size, cols), dtype=tables[0].data.dtype)
    for y, t in enumerate(tables):
        if t.data.shape[0] == 1:        # a missing year: class by class the one row
            cls = [conv1_class(i, size) * 3 + conv1_class(j, size) for i in range(size) for j in range(size)]
            full = np.broadcast_to(t.data[0][cls], (len(origins), size * size, width))
        else:
            full = gather_conv1_np(t, origins, size)
        for l in range(levels):
            out[l, y] = full[:, :, l * cols:(l + 1) * cols]
    return out


def year_flags_np(rasters_norm, origins, size=WINDOW):
    """The years' flags dta_conv1_multistage_gather_windows sets: float32 [years], 1 where any position of any window lies
    on a raster pixel with a non-zero stored element (NaN counts), else 0 -- a missing year (None) and an all-zero raster
    give 0, as do windows that miss the raster.  rasters_norm: per year [C][H][W] as stored, or None.  For float32 rasters
    this is what dta_year_flags says about the gathered float32 batches."""
    origins = np.asarray(origins).reshape(-1, 2)
    flags = np.zeros(len(rasters_norm), dtype=np.float32)
    for y, x in enumerate(rasters_norm):
        if x is None:
            continue
        Hh, Ww = np.asarray(x).shape[1:]
        mask = conv1_mask_np(x)[:-1].reshape(Hh + 2, Ww + 2)[1:-1, 1:-1]
        for r, c in origins:
            r, c = int(r), int(c)
            ra, rb, ca, cb = max(r, 0), min(r + size, Hh), max(c, 0), min(c + size, Ww)
            if ra < rb and ca < cb and mask[ra:rb, ca:cb].any():
                flags[y] = 1.0
                break
    return flags


def crown_reduce_np(probs, offsets):
    """What dta_crown_reduce computes.  probs [rows][classes] float32, crown k = rows offsets[k] .. offsets[k + 1] - 1.
    Each class is summed in row order in float32 (one accumulator) and divided by the count; top-2 of the mean with ties to
    the lower class; an empty crown has count 0, labels -1, scores and mean 0.
    Returns (mean [n][classes] float32, top_idx [n][2] int64, top_score [n][2] float32, count [n] int32)."""
    probs = np.asarray(probs, dtype=np.float32)
    offsets = np.asarray(offsets, dtype=np.int64)
    n, classes = len(offsets) - 1, probs.shape[1]
    mean = np.zeros((n, classes), dtype=np.float32)
    top_idx = np.full((n, 2), -1, dtype=np.int64)
    top_score = np.zeros((n, 2), dtype=np.float32)
    count = np.zeros(n, dtype=np.int32)
    for k in range(n):
        r0, r1 = int(offsets[k]), int(offsets[k + 1])
        if r1 <= r0:
            continue
        acc = np.zeros(classes, dtype=np.float32)
        for r in range(r0, r1):
            acc = acc + probs[r]                      # float32, row order
        m = acc / np.float32(r1 - r0)
        mean[k], count[k] = m, r1 - r0
        valid = np.flatnonzero(m > -1.0)              # (NaNs never win, as in dta_softmax_top2)
        order = valid[np.argsort(-m[valid], kind="stable")][:2]
        top_idx[k, :len(order)] = order
        top_score[k, :len(order)] = m[order]
    return mean, top_idx, top_score, count


CrownSpecies = collections.namedtuple("CrownSpecies", "label score level count top_idx top_score mean votes")


def crown_resolve_np(probs_levels, offsets, hierarchy, window_labels=None):
    """What dta_crown_resolve computes: crown_reduce_np per level, Hierarchy.resolve_np on the levels' top-1 columns, and
    (window_labels: the windows' own species labels [rows]) the number of each crown's windows per species -- labels
    outside [0, n_species) are not counted.  Returns CrownSpecies(label int64 [n], score float32 [n], level int32 [n],
    count int32 [n], top_idx / top_score / mean: one array per level, votes int32 [n][n_species] or None)."""
    if len(probs_levels) != hierarchy.levels:
        raise ValueError("the hierarchy has {} levels: one probability array per level".format(hierarchy.levels))
    offsets = np.asarray(offsets, dtype=np.int64)
    per = [crown_reduce_np(p, offsets) for p in probs_levels]
    label, score, level = hierarchy.resolve_np([r[1][:, 0] for r in per], [r[2][:, 0] for r in per])
    votes = None
    if window_labels is not None:
        w = np.asarray(window_labels).astype(np.int64).reshape(-1)
        n, ns = len(offsets) - 1, hierarchy.n_species
        votes = np.zeros((n, ns), dtype=np.int32)
        for k in range(n):
            mine = w[int(offsets[k]):max(int(offsets[k + 1]), int(offsets[k]))]
            mine = mine[(mine >= 0) & (mine < ns)]
            votes[k] = np.bincount(mine, minlength=ns)
    return CrownSpecies(label, score, level, per[0][3], [r[1] for r in per], [r[2] for r in per], [r[0] for r in per], votes)


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
class DenseRaster:
    """A raw band-first raster [bands][H][W] (what rasterio's read() returns; int16, uint8 or float32, anything else is
    converted to float32 as the reference does) copied to the device once and normalised there once: the clipped
    per-pixel min-max of preprocess.preprocess_batch.  precision="fp32" keeps float32 [C][H][W] (for the float32 gather),
    "bf16" the first conv's channel chunks [ceil(C / 16)][H * W][16] (for the tile gather; bf16-mode Hang2020)."""

    def _place(self, device, precision):
        """The constructors' first step: the device resolved to an index and the precision checked."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("deeptreeattention_amd.dense runs on a ROCm device only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32', got {!r}".format(precision))
        self.precision, self.device = precision, dev

    def _allocate(self, bands, Hh, Ww):
        """The constructors' last step before their launch: the shape and `data` in this raster's form."""
        self.bands, self.height, self.width = bands, Hh, Ww
        self.shape = (bands, Hh, Ww)
        if self.precision == "bf16":
            self.data = torch.empty(((bands + 15) // 16) * Hh * Ww * 16, dtype=torch.int16, device=self.device)
        else:
            self.data = torch.empty(bands, Hh, Ww, dtype=torch.float32, device=self.device)

    def __init__(self, raster, clip=10, precision="bf16", device="cuda"):
        self._place(device, precision)
        a = raster.detach().cpu().numpy() if isinstance(raster, torch.Tensor) else np.asarray(raster)
        if a.ndim != 3:
            raise ValueError("the raster must be a band-first 3-d array")
        if a.dtype not in _DTYPES:
            a = a.astype(np.float32)
        L = _lib.lib()
        bands_raw, Hh, Ww = a.shape
        self._allocate(out_bands(bands_raw, clip), Hh, Ww)
        raw = torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)
        _lib.check(L.dta_raster_normalise(_lib.ptr(raw), bands_raw, Hh, Ww, clip, _DTYPES[a.dtype], int(precision == "bf16"),
                                          _lib.ptr(self.data), _lib.current_stream_ptr()), "dta_raster_normalise")

    @classmethod
    def from_reflectance(cls, cube, bands="no_water", window=None, clip=10, precision="bf16", device="cuda", strip_rows=None):
        """The resident raster straight from a pixel-interleaved reflectance cube [H][W][B] (how a NEON tile is stored: 426
        int16 bands per pixel), bit for bit what DenseRaster(band_first, clip, precision) gives for
        band_first = np.moveaxis(cube[r0:r1, c0:c1][:, :, reflectance.band_index(bands, B)], 2, 0) -- without that select-and-
        transpose on the host (reflectance.reflectance_np is the definition; dta_reflectance_normalise).  bands: "no_water"
        (the reference's mask), "all", "false_color" or a sequence of band indices; window: (row0, col0, row1, col1),
        half-open, e.g. from reflectance.clip_index.  cube: a host array (np.memmap and anything np.asarray takes; int16, uint8
        and float32 are used as they are, anything else is converted to float32 per strip) uploaded in strips of `strip_rows`
        whole rows, one launch per strip (default: as many rows as 64 MiB of raw data hold -- a bound on memory, not a tuned
        value), or a device tensor, normalised in one launch."""
        from . import reflectance as R
        self = cls.__new__(cls)
        self._place(device, precision)
        dev = self.device
        resident = isinstance(cube, torch.Tensor) and cube.is_cuda
        if isinstance(cube, torch.Tensor) and not resident:
            cube = cube.detach().numpy()
        if not resident:
            cube = cube if isinstance(cube, np.ndarray) else np.asarray(cube)
        if cube.ndim != 3:
            raise ValueError("the cube must be a pixel-interleaved 3-d array [rows][cols][bands]")
        Hs, Ws, B = (int(v) for v in cube.shape)
        if B > R.MAX_BANDS:
            raise ValueError("{} bands per pixel: at most {}".format(B, R.MAX_BANDS))
        r0, c0, r1, c1 = R.window_of(cube.shape, window)
        sel = R.selected_bands(bands, B, clip)
        if len(sel) > R.MAX_BANDS:
            raise ValueError("{} bands selected: at most {}".format(len(sel), R.MAX_BANDS))
        Hh, Ww = r1 - r0, c1 - c0
        if Hh * Ww >= 2 ** 31:
            raise ValueError("a raster of {} x {} pixels is over int32".format(Hh, Ww))
        self._allocate(len(sel), Hh, Ww)
        L = _lib.lib()
        index = torch.from_numpy(sel).to(dev, non_blocking=True)

        def launch(strip, code, rows, out_row0):
            d = _lib.ReflectanceDesc(B, Ws, rows, c0, Ww, code, int(precision == "bf16"), Hh, out_row0)
            _lib.check(L.dta_reflectance_normalise(d, _lib.ptr(strip), _lib.ptr(index), self.bands, _lib.ptr(self.data),
                                                   _lib.current_stream_ptr()), "dta_reflectance_normalise")

        if resident:
            t = cube.detach()
            if t.device != dev:
                raise ValueError("the cube is on {}, the raster was asked for on {}".format(t.device, dev))
            if t.dtype not in _TORCH_DTYPES:
                t = t.float()
            t = t[r0:r1].contiguous()                 # whole rows: a view of a contiguous cube
            if t.data_ptr() % 16:
                t = t.clone()
            launch(t, _TORCH_DTYPES[t.dtype], Hh, 0)
            return self
        if strip_rows is None:
            row_bytes = Ws * B * (cube.dtype.itemsize if cube.dtype in _DTYPES else 4)
            strip_rows = max(1, (64 << 20) // row_bytes)
        strip_rows = int(strip_rows)
        if strip_rows < 1:
            raise ValueError("strip_rows must be >= 1, got {}".format(strip_rows))
        for r in range(r0, r1, strip_rows):
            a = cube[r:min(r + strip_rows, r1)]
            if a.dtype not in _DTYPES:
                a = a.astype(np.float32)
            strip = torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
            launch(strip, _DTYPES[a.dtype], a.shape[0], r - r0)
        return self

    def float(self):
        """The normalised raster as a float32 [C][H][W] tensor (bf16 form: the bf16-rounded values)."""
        if self.precision == "fp32":
            return self.data
        t = self.data.view(-1, self.height * self.width, 16).view(torch.bfloat16).float()      # [chunk][pixel][16]
        return t.permute(0, 2, 1).reshape(-1, self.height, self.width)[:self.bands].contiguous()

    def _index(self, items, cols, what):
        """origins [N, 2] / boxes [N, 4]: a host array or a device tensor -> a contiguous int32 device tensor."""
        if isinstance(items, torch.Tensor):
            o = items
            if o.dtype != torch.int32 or o.device != self.device or not o.is_contiguous():
                o = o.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            o = torch.from_numpy(np.ascontiguousarray(np.asarray(items, dtype=np.int32))).to(self.device)
        if o.dim() != 2 or o.shape[1] != cols or o.shape[0] < 1:
            raise ValueError(what)
        return o

    def _origins(self, origins):
        return self._index(origins, 2, "origins must be a non-empty [N, 2] array of (row, col)")

    def _boxes(self, boxes):
        return self._index(boxes, 4, "boxes must be a non-empty [N, 4] array of (row0, col0, row1, col1)")

    def _batch(self, B, size, zero=False):
        """The buffer a gather of B items writes, in this raster's form: float32 (B, bands, size, size), or for a bf16
        raster int16 (B, elements of an item's tiles).  Either way t[:n] is the buffer of the first n items."""
        make = torch.zeros if zero else torch.empty
        if self.precision == "bf16":
            return make(B, ((self.bands + 15) // 16) * size * size * 16, dtype=torch.int16, device=self.device)
        return make(B, self.bands, size, size, dtype=torch.float32, device=self.device)

    def _gather(self, entry, o, extra, tiles, size, out):
        """The body of windows / crops: `entry`[_tiles](raster, bands, H, W, o, N, size, *extra, out, stream)."""
        L = _lib.lib()
        N = o.shape[0]
        if tiles:
            if self.precision != "bf16":
                raise RuntimeError("tiles=True needs DenseRaster(..., precision='bf16')")
            numel = N * ((self.bands + 15) // 16) * size * size * 16
            if out is None:
                out = self._batch(N, size).view(-1)
            elif out.dtype != torch.int16 or out.numel() != numel or not out.is_contiguous():
                raise ValueError("out must be a contiguous int16 tensor of {} elements".format(numel))
            _lib.check(getattr(L, entry + "_tiles")(_lib.ptr(self.data), self.bands, self.height, self.width, _lib.ptr(o), N,
                                                    size, *extra, _lib.ptr(out), _lib.current_stream_ptr()), entry + "_tiles")
            return PatchTiles(out, N, self.bands, size, size)
        if self.precision != "fp32":
            raise RuntimeError("the float32 batch needs DenseRaster(..., precision='fp32')")
        shape = (N, self.bands, size, size)
        if out is None:
            out = self._batch(N, size)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of shape {}".format(shape))
        _lib.check(getattr(L, entry)(_lib.ptr(self.data), self.bands, self.height, self.width, _lib.ptr(o), N, size, *extra,
                                     _lib.ptr(out), _lib.current_stream_ptr()), entry)
        return out

    def windows(self, origins, tiles=False, size=WINDOW, out=None):
        """origins: [N, 2] int32 (row, col) of each window's top-left corner (host array or device tensor); may hang over
        the raster's edges (zero fill).  Returns the float32 (N, bands, size, size) batch (an fp32 raster), or with
        tiles=True a preprocess.PatchTiles (a bf16 raster).  out: the buffer to write (same shape / element count)."""
        return self._gather("dta_gather_windows", self._origins(origins), (), tiles, size, out)

    def crops(self, boxes, tiles=False, size=WINDOW, train=False, out=None):
        """boxes: [N, 4] int32 (row0, col0, row1, col1), half-open (host array or device tensor).  Each box is cut out of
        the raster and resized to size x size with NEAREST -- the reference's patches.crop + utils.load_image, bit for bit
        what preprocess.preprocess_batch gives for the host-sliced raw crop (gather_crops_np; dta_gather_crops[_tiles]).
        train=True: both training flips after the resize.  A box with no rows or columns gives an all-zero crop (a missing
        crop); the boxes are taken as they are -- pixels of a box outside the raster read 0, clip with crop_boxes for the
        reference's intersection.  Returns what windows() returns, in the same forms; out: the buffer to write."""
        return self._gather("dta_gather_crops", self._boxes(boxes), (int(bool(train)),), tiles, size, out)

    def conv1_table(self, predictor, size=WINDOW):
        """The first conv of `predictor`'s network over this raster, once (dta_raster_conv1_table): a Conv1Table in the
        raster's precision, holding the network's weights as they are now.  Raises RuntimeError for what the shared
        first conv does not cover (_share_conv1_refusals) before anything is launched."""
        pred = _predictor(predictor)
        _share_conv1_refusals(pred, self, size)
        return Conv1Table(self, pred)

    @staticmethod
    def _gather_years(entry, rasters, items, cols, outs, flags, clear_next, size, extra):
        """The body of windows_years / crops_years: `entry`(rasters, Y, bands, H, W, o, N, size, *extra, outs, flags,
        clear_next, stream)."""
        rs = list(rasters)
        have = _check_years(rs)
        r0 = have[0]
        if len(outs) != len(rs):
            raise ValueError("one output batch per year")
        o = r0._origins(items) if cols == 2 else r0._boxes(items)
        N, Y = o.shape[0], len(rs)
        shape = (N, r0.bands, size, size)
        for t in outs:
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != r0.device:
                raise ValueError("every year's out must be a contiguous float32 tensor of shape {} on {}".format(shape, r0.device))
        for t in (flags, clear_next):
            if t.dtype != torch.float32 or t.numel() != Y or not t.is_contiguous() or t.device != r0.device:
                raise ValueError("flags and clear_next must be float32 [{}] tensors on {}".format(Y, r0.device))
        L = _lib.lib()
        rp = (_lib.C.c_void_p * Y)(*[None if r is None else r.data.data_ptr() for r in rs])
        op = (_lib.C.c_void_p * Y)(*[t.data_ptr() for t in outs])
        _lib.check(getattr(L, entry)(rp, Y, r0.bands, r0.height, r0.width, _lib.ptr(o), N, size, *extra, op, _lib.ptr(flags),
                                     _lib.ptr(clear_next), _lib.current_stream_ptr()), entry)
        return flags

    @staticmethod
    def windows_years(rasters, origins, outs, flags, clear_next, size=WINDOW):
        """DenseRaster.windows for every year of an ensemble in ONE launch (dta_gather_windows_years).  rasters: one fp32
        DenseRaster per year (same shape), None for a missing year; outs: one contiguous float32 (N, bands, size, size)
        tensor per year -- a missing year's is not written (keep it zero); flags / clear_next: two float32 [years] device
        tensors used alternately by successive calls (dta_year_flags' banks: `flags` zero on entry, `clear_next` zeroed by
        this call).  flags ends as dta_year_flags' verdict on the years' batches.  Returns flags."""
        return DenseRaster._gather_years("dta_gather_windows_years", rasters, origins, 2, outs, flags, clear_next, size, ())

    @staticmethod
    def crops_years(rasters, boxes, outs, flags, clear_next, size=WINDOW, train=False):
        """DenseRaster.crops for every year of an ensemble in ONE launch (dta_gather_crops_years): all years the same
        boxes.  rasters / outs / flags / clear_next as windows_years takes them; train=True: both flips.  Returns flags."""
        return DenseRaster._gather_years("dta_gather_crops_years", rasters, boxes, 4, outs, flags, clear_next, size,
                                         (int(bool(train)),))


def _share_conv1_refusals(pred, raster, size):
    """What the shared first conv does not cover; raises before anything is launched."""
    if pred.ensemble:
        raise RuntimeError("share_conv1: a year ensemble has one input per year, there is no first conv to share")
    m = pred.nets_mod[0]
    if m._net_code not in (_lib.NET_HANG2020, _lib.NET_SPECTRAL, _lib.NET_SPATIAL):
        raise RuntimeError("share_conv1: Hang2020, spectral_network and spatial_network only (not vanilla_CNN)")
    if m.training:
        raise RuntimeError("share_conv1: the model is in training mode; prediction runs eval-mode BatchNorm (model.eval())")
    if size != 11:
        raise RuntimeError("share_conv1: window side {} -- the first-conv table is laid out for 11x11 windows only".format(size))
    if not isinstance(raster, DenseRaster):
        raise TypeError("rasters must be DenseRaster objects")
    if raster.precision != m.precision:
        raise RuntimeError("share_conv1: a {}-mode network needs DenseRaster(..., precision={!r}), not {!r}"
                           .format(m.precision, m.precision, raster.precision))
    w = next(t for t in m.parameters() if t.dim() == 4)
    if w.shape[1] != raster.bands:
        raise ValueError("the network takes {} bands, the normalised raster has {}".format(w.shape[1], raster.bands))


class Conv1Table:
    """The first conv's output for every position a window can put over a raster (module text; csrc/dense_conv1.hip):
    data [(H + 2) * (W + 2) + 1][9][cols] on the device, IEEE half for a bf16 raster / network, float32 for fp32 -- the
    storage the forward keeps its first conv's output in.  cols = 64 (Hang2020: spectral | spatial branch) or 32.
    Built from the network's weights at construction: rebuild it after a weight update."""

    def __init__(self, raster, pred):
        L = _lib.lib()
        m = pred.nets_mod[0]
        self.height, self.width, self.bands, self.precision, self.device = raster.height, raster.width, raster.bands, raster.precision, raster.device
        self.cols = 64 if m._net_code == _lib.NET_HANG2020 else 32
        self.desc = forward_only_descs(1, raster.bands, WINDOW, WINDOW, m._classes, m._net_code, m.precision)[0]
        scratch_b, table_b = _lib.C.c_size_t(), _lib.C.c_size_t()
        _lib.check(L.dta_conv1_table_bytes(_lib.C.byref(self.desc), self.height, self.width, _lib.C.byref(scratch_b),
                                           _lib.C.byref(table_b)), "dta_conv1_table_bytes")
        dt = torch.float16 if self.precision == "bf16" else torch.float32
        self.data = torch.empty((self.height + 2) * (self.width + 2) + 1, 9, self.cols, dtype=dt, device=self.device)
        if self.data.numel() * self.data.element_size() != table_b.value:
            raise RuntimeError("dta_conv1_table_bytes: {} bytes, the binding expects {}".format(table_b.value, self.data.numel() * self.data.element_size()))
        scratch = torch.empty(scratch_b.value, dtype=torch.uint8, device=self.device)      # T and the weight image: this call only
        nets = pred._tables([m])[0]
        _lib.check(L.dta_raster_conv1_table(_lib.C.byref(self.desc), nets, _lib.ptr(raster.data), self.height, self.width,
                                            _lib.ptr(scratch), _lib.ptr(self.data), _lib.current_stream_ptr()), "dta_raster_conv1_table")

    def gather(self, origins, out):
        """origins: device int32 [n][2]; out: the bytes that receive [n * 121][cols] (engine.Predictor.conv1_slot)."""
        n = origins.shape[0]
        if out.numel() * out.element_size() != n * WINDOW * WINDOW * self.cols * self.data.element_size():
            raise ValueError("out must hold {} windows x 121 x {} elements".format(n, self.cols))
        _lib.check(_lib.lib().dta_gather_conv1_windows(_lib.C.byref(self.desc), _lib.ptr(self.data), self.height, self.width,
                                                       _lib.ptr(origins), n, _lib.ptr(out), _lib.current_stream_ptr()),
                   "dta_gather_conv1_windows")
        return out

    def numpy(self):
        """The table read back, in the form gather_conv1_np takes."""
        return Conv1TableNP(self.data.cpu().numpy(), self.height, self.width)


def _share_conv1_multistage_models(predictor, size):
    """The model side of _share_conv1_multistage_refusals.  Returns the networks."""
    mods = [m for p in predictor.preds for m in p.nets_mod]
    if any(m.training for m in mods):
        raise RuntimeError("share_conv1: a network is in training mode; prediction runs eval-mode BatchNorm (model.eval())")
    if any(m.precision != mods[0].precision for m in mods):
        raise RuntimeError("share_conv1: all levels must run in the same precision")
    if size != 11:
        raise RuntimeError("share_conv1: window side {} -- the first-conv table is laid out for 11x11 windows only".format(size))
    return mods


def _share_conv1_multistage_refusals(predictor, rs, size):
    """What the shared first conv of the multi-stage route does not cover, after _multistage_years; raises before anything
    is allocated or launched.  Returns the present years' rasters."""
    mods = _share_conv1_multistage_models(predictor, size)
    want = mods[0].precision
    have = _check_rasters(rs, want, "share_conv1: {}-mode networks need DenseRaster(..., precision={!r}), not {!r}"
                          .format(want, want, "fp32" if want == "bf16" else "bf16"))      # (a raster is in one of the two)
    for m in mods:
        w = next(t for t in m.parameters() if t.dim() == 4)
        if w.shape[1] != have[0].bands:
            raise RuntimeError("share_conv1: the networks take {} bands, the normalised rasters have {}".format(w.shape[1], have[0].bands))
    return have


class Conv1TableYears:
    """The first convs of a multi-stage model's levels x years networks for every position a window can put over the
    years' rasters (module text; csrc/dense_conv1.hip): per year one table [(H + 2) * (W + 2) + 1][9][levels * 32] -- columns
    32 l .. 32 l + 31 level l's year-y network -- in the storage Conv1Table uses, and the raster's non-zero mask, one byte
    per position.  A missing year (None): the far-outside row alone, [1][9][levels * 32], and one zero byte.  The years are
    built one after the other through ONE scratch.  Built from the networks' weights at construction."""

    def __init__(self, rasters, predictor):
        L = _lib.lib()
        rs = list(rasters)
        r0 = next(r for r in rs if r is not None)
        m0 = predictor.preds[0].nets_mod[0]
        self.height, self.width, self.bands, self.precision, self.device = r0.height, r0.width, r0.bands, r0.precision, r0.device
        self.levels, self.years = len(predictor.preds), len(rs)
        self.cols = 32 * self.levels
        self.present = [r is not None for r in rs]
        self.desc = forward_only_descs(1, r0.bands, WINDOW, WINDOW, m0._classes, _lib.NET_SPECTRAL, m0.precision)[0]
        dt = torch.float16 if self.precision == "bf16" else torch.float32
        size_t = _lib.C.c_size_t

        def sizes(h, w):
            sb, tb, mb = size_t(), size_t(), size_t()
            _lib.check(L.dta_conv1_multistage_table_bytes(_lib.C.byref(self.desc), self.levels, h, w, _lib.C.byref(sb), _lib.C.byref(tb),
                                                          _lib.C.byref(mb)), "dta_conv1_multistage_table_bytes")
            return sb.value, tb.value, mb.value
        scratch_b, table_b, mask_b = sizes(self.height, self.width)
        _, far_b, _ = sizes(0, 0)
        positions = (self.height + 2) * (self.width + 2) + 1
        if table_b != positions * 9 * self.cols * dt.itemsize or mask_b != positions or far_b != 9 * self.cols * dt.itemsize:
            raise RuntimeError("dta_conv1_multistage_table_bytes: {} / {} / {} bytes are not what the binding expects".format(table_b, mask_b, far_b))
        scratch = torch.empty(scratch_b, dtype=torch.uint8, device=self.device)      # T and the weight image: shared by the years
        self.data, self.mask = [], []
        st = _lib.current_stream_ptr()
        for y, r in enumerate(rs):
            n = positions if r is not None else 1
            self.data.append(torch.empty(n, 9, self.cols, dtype=dt, device=self.device))
            self.mask.append(torch.empty(n, dtype=torch.uint8, device=self.device))
            nets = (_lib.SubnetParams * self.levels)(*[p._tables([p.nets_mod[y]])[0][0] for p in predictor.preds])
            _lib.check(L.dta_conv1_multistage_raster_table(_lib.C.byref(self.desc), self.levels, nets, _lib.ptr(r.data) if r is not None else None,
                                                           self.height, self.width, _lib.ptr(scratch), _lib.ptr(self.data[y]),
                                                           _lib.ptr(self.mask[y]), st), "dta_conv1_multistage_raster_table")
        self._tp = (_lib.C.c_void_p * self.years)(*[t.data_ptr() for t in self.data])
        self._mp = (_lib.C.c_void_p * self.years)(*[t.data_ptr() for t in self.mask])
        self._pr = (_lib.C.c_int * self.years)(*[int(p) for p in self.present])

    def gather(self, origins, predictor, flags, clear_next):
        """origins: device int32 [n][2].  Fills predictor.conv1_slot(n, bands) -- every (level, year) group's first conv --
        and sets flags (float32 [years]; dta_gather_windows_years' banks: `flags` zero on entry, `clear_next` zeroed by this
        call, or None: flags cleared first).  Returns flags."""
        n = origins.shape[0]
        predictor._prepare_conv1(n, self.bands)
        _lib.check(_lib.lib().dta_conv1_multistage_gather_windows(
            _lib.C.byref(predictor.desc), self.levels, predictor.lv, self.years, self._tp, self._mp, self._pr, self.height, self.width,
            _lib.ptr(origins), n, _lib.ptr(predictor.ws), _lib.ptr(flags), _lib.ptr(clear_next), _lib.current_stream_ptr()),
            "dta_conv1_multistage_gather_windows")
        return flags

    def numpy(self):
        """The years' tables read back, in the form gather_conv1_years_np takes."""
        return [Conv1TableNP(t.cpu().numpy(), self.height, self.width) for t in self.data]


def _check_rasters(rs, want, refusal, one_device=True):
    """The raster set of a prediction route (one per year, None = missing; a single-raster route passes a list of one):
    at least one present, DenseRasters in precision `want` -- anything else raises RuntimeError(refusal), the route's own
    words -- of one shape and, with one_device, one device.  Returns the present ones.  Launches nothing."""
    have = [r for r in rs if r is not None]
    if not have:
        raise ValueError("at least one year's raster must be present")
    for r in have:
        if not isinstance(r, DenseRaster):
            raise TypeError("rasters must be DenseRaster objects")
        if r.precision != want:
            raise RuntimeError(refusal)
        if r.shape != have[0].shape or (one_device and r.device != have[0].device):
            raise ValueError("all years' rasters must share one shape" + (" and device" if one_device else ""))
    return have


def _check_years(rs):
    """The years' rasters of a multi-stage / float32 ensemble route: fp32 DenseRasters."""
    return _check_rasters(rs, "fp32", "the multi-stage route reads DenseRaster(..., precision='fp32') (bf16 tiles are not taken)")


CrownPredictions = collections.namedtuple("CrownPredictions", "mean top_idx top_score count")
WindowPredictions = collections.namedtuple("WindowPredictions", "top_idx top_score probs crowns")


def crown_reduce(probs, crown_offsets):
    """dta_crown_reduce on device probabilities [rows][classes] (float32, contiguous): CrownPredictions(mean
    [n][classes], top_idx [n][2] int64, top_score [n][2], count [n] int32), all on the device."""
    L = _lib.lib()
    dev = probs.device
    if probs.dtype != torch.float32 or probs.dim() != 2 or not probs.is_contiguous():
        raise ValueError("probs must be a contiguous float32 [rows][classes] tensor")
    host = _host_offsets(crown_offsets, probs.shape[0])
    off = torch.from_numpy(host).to(dev)
    n, classes = len(host) - 1, probs.shape[1]
    out = CrownPredictions(torch.empty(n, classes, dtype=torch.float32, device=dev),
                           torch.empty(n, 2, dtype=torch.int64, device=dev),
                           torch.empty(n, 2, dtype=torch.float32, device=dev),
                           torch.empty(n, dtype=torch.int32, device=dev))
    _lib.check(L.dta_crown_reduce(_lib.ptr(probs), _lib.ptr(off), n, classes, _lib.ptr(out.mean), _lib.ptr(out.top_idx),
                                  _lib.ptr(out.top_score), _lib.ptr(out.count), _lib.current_stream_ptr()), "dta_crown_reduce")
    return out


def _host_offsets(crown_offsets, rows):
    host = crown_offsets.detach().cpu().numpy() if isinstance(crown_offsets, torch.Tensor) else np.asarray(crown_offsets)
    host = host.astype(np.int64)
    if host.ndim != 1 or len(host) < 2 or host[0] < 0 or (np.diff(host) < 0).any() or host[-1] > rows:
        raise ValueError("crown_offsets must be non-decreasing, start at >= 0 and end within the {} rows".format(rows))
    return np.ascontiguousarray(host)


def crown_resolve(probs_levels, crown_offsets, hierarchy, window_labels=None, want_mean=True):
    """dta_crown_resolve: probs_levels = the levels' device probabilities [rows][classes_l] (float32, contiguous),
    hierarchy a hierarchy.Hierarchy over those levels, window_labels (int64 [rows] on the device, e.g. the windows'
    ens_label) for the votes.  Returns CrownSpecies as crown_resolve_np does, on the device (top_idx int64; mean is None
    with want_mean=False; votes None without window_labels).  The offsets are checked here, before the launch."""
    probs_levels = list(probs_levels)
    nl = len(probs_levels)
    if nl != hierarchy.levels:
        raise ValueError("the hierarchy has {} levels: one probability tensor per level".format(hierarchy.levels))
    dev, rows = probs_levels[0].device, probs_levels[0].shape[0]
    for l, p in enumerate(probs_levels):
        if (p.dtype != torch.float32 or p.dim() != 2 or not p.is_contiguous() or p.device != dev
                or tuple(p.shape) != (rows, hierarchy.classes[l])):
            raise ValueError("level {}: probs must be a contiguous float32 [{}][{}] tensor on {}".format(l, rows, hierarchy.classes[l], dev))
    if window_labels is not None:
        w = window_labels
        if w.dtype != torch.int64 or tuple(w.shape) != (rows,) or not w.is_contiguous() or w.device != dev:
            raise ValueError("window_labels must be a contiguous int64 [{}] tensor on {}".format(rows, dev))
    host = _host_offsets(crown_offsets, rows)
    off, n = torch.from_numpy(host).to(dev), len(host) - 1
    L = _lib.lib()
    mean = [torch.empty(n, c, dtype=torch.float32, device=dev) for c in hierarchy.classes] if want_mean else None
    top_idx = [torch.empty(n, 2, dtype=torch.int64, device=dev) for _ in range(nl)]
    top_score = [torch.empty(n, 2, dtype=torch.float32, device=dev) for _ in range(nl)]
    count = torch.empty(n, dtype=torch.int32, device=dev)
    label = torch.empty(n, dtype=torch.int64, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    level = torch.empty(n, dtype=torch.int32, device=dev)
    votes = torch.empty(n, hierarchy.n_species, dtype=torch.int32, device=dev) if window_labels is not None else None
    arr = _lib.C.c_void_p * nl
    table = hierarchy.c_table(dev)
    _lib.check(L.dta_crown_resolve(nl, arr(*[p.data_ptr() for p in probs_levels]), _lib.ptr(off), n, _lib.C.byref(table),
                                   arr(*[t.data_ptr() for t in mean]) if want_mean else None,
                                   arr(*[t.data_ptr() for t in top_idx]), arr(*[t.data_ptr() for t in top_score]),
                                   _lib.ptr(count), _lib.ptr(label), _lib.ptr(score), _lib.ptr(level),
                                   _lib.ptr(window_labels), _lib.ptr(votes), _lib.current_stream_ptr()), "dta_crown_resolve")
    return CrownSpecies(label, score, level, count, top_idx, top_score, mean, votes)


def _predictor(model_or_predictor):
    from .engine import Predictor
    return model_or_predictor if isinstance(model_or_predictor, Predictor) else Predictor(model_or_predictor)


def raster_precision(model_or_predictor):
    """The DenseRaster form the network's route reads: "bf16" for a bf16-mode Hang2020 (tile gather +
    dta_net_forward_tiles), "fp32" for every other network kind and precision (float32 gather)."""
    p = _predictor(model_or_predictor)
    m = p.nets_mod[0]
    tiles = (not p.ensemble) and m._net_code == _lib.NET_HANG2020 and m.precision == "bf16"
    return "bf16" if tiles else "fp32"


# What the prediction loops gather per batch: windows at origins [N, 2] or resized crops of boxes [N, 4].  The routes
# (_single_route, _metadata_route, _predict_batches_multistage) are written once and take one of these two.
#   index(raster, items)  the caller's origins / boxes -> the int32 device tensor the gathers take, once, before the loop
#   one(raster, idx, ...) a batch out of one raster (DenseRaster.windows / .crops)
#   years                 a batch out of every year's raster in one launch (DenseRaster.windows_years / .crops_years)
_Gather = collections.namedtuple("_Gather", "index one years")


def _clipped_boxes(raster, boxes):
    """Raw pixel boxes (host array or tensor) -> crop_boxes of them on the device."""
    host = boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes
    return raster._boxes(crop_boxes(host, raster.height, raster.width))


_WINDOWS = _Gather(DenseRaster._origins, DenseRaster.windows, DenseRaster.windows_years)
_CROPS = _Gather(_clipped_boxes, DenseRaster.crops, DenseRaster.crops_years)


def predict_windows(model_or_predictor, rasters, origins, crown_offsets=None, batch_size=4096, return_probs=False,
                    share_conv1=False):
    """Per-window prediction on 11x11 windows (the side every prediction route here is tested at; DenseRaster.windows
    gathers other sides): walks `origins` in batches of `batch_size` -- gather, the existing eval forward
    (engine.Predictor), dta_softmax_top2 -- writing top_idx [N, 2] / top_score [N, 2] into preallocated device tensors;
    nothing inside the loop waits for the device.
    rasters: a DenseRaster in the form raster_precision() names; for a year.learned_ensemble one per year, None for a
    missing year (an all-zero batch, reference data.py:295-296).
    crown_offsets ([n + 1], windows grouped by crown as window_origins returns them): also the per-crown mean probability
    vector, its top-2 and the window count.  Window probabilities are kept when return_probs or crown_offsets ask for them.
    share_conv1=True (a single Hang2020 / spectral_network / spatial_network in eval mode; the raster in the MODEL's
    precision): the first conv is computed once per raster (DenseRaster.conv1_table, built in this call: weight updates
    between calls are followed) and each batch is a gather of its output into the Predictor's workspace followed by the
    forward without its first conv -- no window of the input is ever formed.  Anything it does not cover raises
    RuntimeError before a launch (_share_conv1_refusals).
    Returns WindowPredictions(top_idx, top_score, probs or None, crowns or None)."""
    return _single_route(_WINDOWS, model_or_predictor, rasters, origins, crown_offsets, batch_size, return_probs, share_conv1)


def predict_crops(model_or_predictor, rasters, boxes, batch_size=4096, return_probs=False):
    """One prediction per crown box, as the reference's production path defines it (predict.py -> generate_crops ->
    patches.crop -> utils.load_image): each box is cut out of the resident raster and resized to 11x11 with NEAREST on the
    device (DenseRaster.crops), then predict_windows' loop -- the eval forward, dta_softmax_top2 -- in batches of
    `batch_size`; nothing inside the loop waits for the device, and no crop passes through the host: one raster upload,
    16 bytes per crown.  boxes: pixel boxes (row0, col0, row1, col1), half-open; they go through crop_boxes once, before
    the loop (clipped to the raster; a box that misses it raises ValueError).  rasters: as for predict_windows, including
    one per year (None: a missing year) for a year.learned_ensemble.
    There is no share_conv1 here: a resized crop's 3x3 neighbours are not raster neighbours unless the box is exactly
    11x11, so the first conv's output at a crop position is not a function of the raster pixel underneath.
    Returns WindowPredictions(top_idx [N, 2], top_score [N, 2], probs or None, crowns=None): one row per box."""
    return _single_route(_CROPS, model_or_predictor, rasters, boxes, None, batch_size, return_probs, False)


def _batch_plan(N, batch_size, crown_offsets):
    """The preamble of every route, before anything is allocated or launched: (the batch size for N items, the crown
    offsets checked on the host or None)."""
    B = min(int(batch_size), N)
    if B < 1:
        raise ValueError("batch_size must be positive")
    return B, None if crown_offsets is None else _host_offsets(crown_offsets, N)


def _year_buffers(r0, rs, B, size):
    """One gather buffer of B items per raster of rs, in r0's form."""
    zeros = r0._batch(B, size, zero=True) if any(r is None for r in rs) else None      # ONE persistent zero batch stands in for every missing year
    return [zeros if r is None else r0._batch(B, size) for r in rs]


def _predict_batches(o, B, crown_offsets, classes, return_probs, batch):
    """The walk of the single-output routes over the items o [N, 2 or 4] in batches of B: the outputs, the row slices, the
    crown tail.  batch(n, items, probs or None, top_idx, top_score) launches one batch of n items into the row slices it is
    handed; nothing here waits for the device."""
    dev, N = o.device, o.shape[0]
    keep = return_probs or crown_offsets is not None
    top_idx = torch.empty(N, 2, dtype=torch.int64, device=dev)
    top_score = torch.empty(N, 2, dtype=torch.float32, device=dev)
    probs = torch.empty(N, classes, dtype=torch.float32, device=dev) if keep else None
    for n0 in range(0, N, B):
        n = min(B, N - n0)
        batch(n, o[n0:n0 + n], probs[n0:n0 + n] if keep else None, top_idx[n0:n0 + n], top_score[n0:n0 + n])
    crowns = crown_reduce(probs, crown_offsets) if crown_offsets is not None else None
    return WindowPredictions(top_idx, top_score, probs if return_probs else None, crowns)


def _single_route(gather, model_or_predictor, rasters, items, crown_offsets, batch_size, return_probs, share_conv1):
    """predict_windows / predict_crops: the checks, then _predict_batches with this route's batch."""
    pred = _predictor(model_or_predictor)
    size = WINDOW
    if share_conv1:
        _share_conv1_refusals(pred, rasters, size)
        want = rasters.precision
    else:
        want = raster_precision(pred)
    if pred.ensemble:
        rs = list(rasters)
        if len(rs) != len(pred.nets_mod):
            raise ValueError("a {}-year ensemble needs {} rasters (None for a missing year)".format(len(pred.nets_mod), len(pred.nets_mod)))
    else:
        rs = [rasters]
    r0 = _check_rasters(rs, want, "this network reads a DenseRaster(..., precision={!r}) (dense.raster_precision)".format(want),
                        one_device=False)[0]
    o = gather.index(r0, items)
    B, crown_offsets = _batch_plan(o.shape[0], batch_size, crown_offsets)
    classes = pred.nets_mod[0]._classes
    L, st = _lib.lib(), _lib.current_stream_ptr()

    def top2(logits, n, probs, top_idx, top_score):
        _lib.check(L.dta_softmax_top2(_lib.ptr(logits), n, classes, _lib.ptr(probs), _lib.ptr(top_idx), _lib.ptr(top_score), st),
                   "dta_softmax_top2")

    if share_conv1:
        table = r0.conv1_table(pred, size=size)

        def batch(n, ob, *out):
            table.gather(ob, pred.conv1_slot(n, r0.bands))
            top2(pred.logits_from_conv1(), n, *out)
    else:
        tiles = want == "bf16"
        bufs = _year_buffers(r0, rs, B, size)

        def batch(n, ob, *out):
            xs = [b[:n] if r is None else gather.one(r, ob, tiles=tiles, size=size, out=b[:n]) for r, b in zip(rs, bufs)]
            top2(pred.logits_of(xs if pred.ensemble else xs[0]), n, *out)
    return _predict_batches(o, B, crown_offsets, classes, return_probs, batch)


def predict_map(model_or_predictor, raster, anchor="center", rows=None, cols=None, clip=10, batch_size=4096, share_conv1=False):
    """Label every pixel of a raster region: rows / cols are half-open (start, stop) pixel ranges (default: the whole
    raster).  raster: a raw band-first array or a DenseRaster (a list with one per year, None allowed, for an ensemble).
    share_conv1: as for predict_windows (a raw array is made resident in the model's precision).
    Returns (labels [h][w] int64, scores [h][w] float32): the top-1 class of each pixel's window and its probability."""
    pred = _predictor(model_or_predictor)
    if share_conv1 and pred.ensemble:
        raise RuntimeError("share_conv1: a year ensemble has one input per year, there is no first conv to share")
    want = pred.nets_mod[0].precision if share_conv1 else raster_precision(pred)

    def resident(r):
        return r if r is None or isinstance(r, DenseRaster) else DenseRaster(r, clip=clip, precision=want, device=pred.device)
    rs = [resident(r) for r in raster] if pred.ensemble else resident(raster)
    origins, hw = _region(next(r for r in rs if r is not None) if pred.ensemble else rs, rows, cols, anchor)
    res = predict_windows(pred, rs, origins, batch_size=batch_size, share_conv1=share_conv1)
    return res.top_idx[:, 0].reshape(hw), res.top_score[:, 0].reshape(hw)


def _region(first, rows, cols, anchor):
    """The region of a predict_map*: rows / cols are half-open (start, stop) pixel ranges, by default all of the raster
    `first`.  Returns (one window origin per pixel, row-major, and the region's (h, w))."""
    r0, r1 = rows if rows is not None else (0, first.height)
    c0, c1 = cols if cols is not None else (0, first.width)
    origins, _ = window_origins([(r0, c0, r1, c1)], anchor=anchor, size=WINDOW)
    return origins, (r1 - r0, c1 - c0)


MultiStageWindowPredictions = collections.namedtuple("MultiStageWindowPredictions",
                                                     "ens_label ens_score ens_level top_idx top_score probs crowns")


def _multistage_years(predictor, rasters):
    """The checks of the multi-stage route that need no device: raises before anything is launched.  Returns the years'
    rasters as a list."""
    from .engine import MultiStagePredictor
    if not isinstance(predictor, MultiStagePredictor):
        raise TypeError("the multi-stage route needs an engine.MultiStagePredictor")
    rs = list(rasters)
    years = len(predictor.preds[0].nets_mod)
    if len(rs) != years:
        raise ValueError("the levels have {} years: {} rasters are needed (None for a missing year), not {}".format(years, years, len(rs)))
    if predictor.hierarchy is None:
        raise RuntimeError("the multi-stage route needs a hierarchy (MultiStagePredictor(models, hierarchy=...))")
    if not predictor.supported(years):
        raise RuntimeError("{} levels x {} years are more networks than one chain takes ({}): this route runs one chain only"
                           .format(len(predictor.preds), years, _lib.MAX_YEARS))
    if predictor.hierarchy.levels != len(predictor.preds):
        raise ValueError("the hierarchy has {} levels, the predictor {}".format(predictor.hierarchy.levels, len(predictor.preds)))
    return rs


def predict_windows_multistage(predictor, rasters, origins, crown_offsets=None, batch_size=4096, return_probs=False,
                               share_conv1=False):
    """Per-window species prediction of a multi-stage model on 11x11 windows: walks `origins` in batches of `batch_size` --
    ONE gather launch for all years (dta_gather_windows_years, which also decides the years' flags), then the levels x years
    forward, every level's softmax / top-2 and the hierarchy walk as MultiStagePredictor.ensemble(year_flags=...) runs them
    -- copying each batch's outputs into preallocated [N] device tensors; nothing inside the loop waits for the device.
    predictor: an engine.MultiStagePredictor with a hierarchy whose levels x years fit one chain (predictor.supported).
    rasters: one DenseRaster(..., precision="fp32") per year, None for a missing year (left out of every level's mean, as
    is a present year whose batch is all zero: reference year.py:27-33).
    crown_offsets ([n + 1], windows grouped by crown as window_origins returns them): also one species per crown
    (crown_resolve: per level the mean over the crown's windows, then the walk -- this package's definition, see the
    module text) with the crown's window votes.
    share_conv1=True (networks in eval mode; the rasters in the MODELS' precision -- DenseRaster(..., precision="bf16") for
    bf16-mode networks): every year's raster goes through the first convs of all levels ONCE (Conv1TableYears, built in this
    call: weight updates between calls are followed), each batch is ONE gather launch of their outputs into the predictor's
    workspace -- which also sets the years' flags from the rasters' non-zero masks -- and the grouped forward without its
    first convs; no window of the input is ever formed.  What it does not cover raises RuntimeError before anything is
    allocated (_share_conv1_multistage_refusals).
    Returns MultiStageWindowPredictions(ens_label int64 [N], ens_score float32 [N], ens_level int32 [N], top_idx / top_score:
    one [N, 2] tensor per level, probs: one [N, classes_l] tensor per level or None, crowns: CrownSpecies or None)."""
    return _predict_batches_multistage(_WINDOWS, predictor, rasters, origins, crown_offsets, batch_size, return_probs, share_conv1)


def predict_crops_multistage(predictor, rasters, boxes, batch_size=4096, return_probs=False):
    """One species per crown box from a multi-stage model: predict_crops' crops (ONE gather launch for all years per batch,
    dta_gather_crops_years, which also decides the years' flags) through predict_windows_multistage's loop.  With one crop
    per crown this is exactly the reference's gather_predictions + ensemble (multi_stage.py:368-485) on the crops its
    predict.predict_species generates.  predictor / rasters as for predict_windows_multistage (fp32 rasters, None: a
    missing year); boxes as for predict_crops (crop_boxes once, before the loop).  No share_conv1: see predict_crops.
    Returns MultiStageWindowPredictions, one row per box, crowns=None."""
    return _predict_batches_multistage(_CROPS, predictor, rasters, boxes, None, batch_size, return_probs, False)


def _predict_batches_multistage(gather, predictor, rasters, items, crown_offsets, batch_size, return_probs, share_conv1):
    """The loop of predict_windows_multistage / predict_crops_multistage."""
    rs = _multistage_years(predictor, rasters)
    have = _share_conv1_multistage_refusals(predictor, rs, WINDOW) if share_conv1 else _check_years(rs)
    r0 = have[0]
    dev, size, Y = r0.device, WINDOW, len(rs)
    o = gather.index(r0, items)
    N = o.shape[0]
    B, crown_offsets = _batch_plan(N, batch_size, crown_offsets)
    classes = [p.nets_mod[0]._classes for p in predictor.preds]
    nl = len(classes)
    keep = return_probs or crown_offsets is not None
    ens = (torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
           torch.empty(N, dtype=torch.int32, device=dev))
    top_idx = [torch.empty(N, 2, dtype=torch.int64, device=dev) for _ in range(nl)]
    top_score = [torch.empty(N, 2, dtype=torch.float32, device=dev) for _ in range(nl)]
    probs = [torch.empty(N, c, dtype=torch.float32, device=dev) for c in classes] if keep else None
    if share_conv1:
        table = Conv1TableYears(rs, predictor)
    else:
        bufs = _year_buffers(r0, rs, B, size)
    banks = [torch.zeros(Y, dtype=torch.float32, device=dev) for _ in range(2)]
    bank = 0
    for n0 in range(0, N, B):
        n = min(B, N - n0)
        if share_conv1:
            flags = table.gather(o[n0:n0 + n], predictor, banks[bank], banks[bank ^ 1])
            bank ^= 1
            e = predictor.ensemble_from_conv1(flags, return_probs=keep)
        else:
            xs = [b[:n] for b in bufs]
            flags = gather.years(rs, o[n0:n0 + n], xs, banks[bank], banks[bank ^ 1], size=size)
            bank ^= 1
            e = predictor.ensemble(xs, year_flags=flags, return_probs=keep)
        for dst, src in zip(ens, e):
            dst[n0:n0 + n].copy_(src)
        for l in range(nl):
            top_idx[l][n0:n0 + n].copy_(predictor.top_idx[l])
            top_score[l][n0:n0 + n].copy_(predictor.top_score[l])
            if keep:
                probs[l][n0:n0 + n].copy_(predictor.probs[l])
    crowns = None
    if crown_offsets is not None:
        crowns = crown_resolve(probs, crown_offsets, predictor.hierarchy, window_labels=ens[0])
    return MultiStageWindowPredictions(ens[0], ens[1], ens[2], top_idx, top_score, probs if return_probs else None, crowns)


def predict_map_multistage(predictor, rasters, anchor="center", rows=None, cols=None, clip=10, batch_size=4096, share_conv1=False):
    """A species map of a raster region from a multi-stage model: rows / cols are half-open (start, stop) pixel ranges
    (default: the whole raster).  rasters: per year a raw band-first array or a DenseRaster(..., precision="fp32"), None for
    a missing year.  share_conv1: as for predict_windows_multistage (raw arrays are made resident in the models' precision).
    Returns (species [h][w] int64, score [h][w] float32, level [h][w] int32): each pixel's window's
    ens_label, the top-1 probability of the level that decided, and that level."""
    rs = _multistage_years(predictor, rasters)
    if all(r is None for r in rs):
        raise ValueError("at least one year's raster must be present")
    want = "fp32"
    if share_conv1:      # every refusal before a raw array is made resident
        want = _share_conv1_multistage_models(predictor, WINDOW)[0].precision
        resident = [r for r in rs if isinstance(r, DenseRaster)]
        if resident:
            _share_conv1_multistage_refusals(predictor, resident, WINDOW)
    rs = [r if r is None or isinstance(r, DenseRaster) else DenseRaster(r, clip=clip, precision=want, device=predictor.device)
          for r in rs]
    first = (_share_conv1_multistage_refusals(predictor, rs, WINDOW) if share_conv1 else _check_years(rs))[0]
    origins, hw = _region(first, rows, cols, anchor)
    res = predict_windows_multistage(predictor, rs, origins, batch_size=batch_size, share_conv1=share_conv1)
    return res.ens_label.reshape(hw), res.ens_score.reshape(hw), res.ens_level.reshape(hw)


def predict_windows_metadata(predictor, raster, site, origins, crown_offsets=None, batch_size=4096, return_probs=False):
    """predict_windows for the site-metadata fusion model: walks `origins` in batches of `batch_size` -- gather, the sensor
    model's eval forward, then site branch + fusion layer + softmax + top-2 as ONE launch (dta_meta_predict with the
    raster's site for every row) writing into row slices of the preallocated outputs; nothing inside the loop waits for the
    device.  predictor: an engine.MetadataPredictor (its table is built once, before the loop).  raster: a DenseRaster in
    the form raster_precision(predictor.sensor) names.  site: the raster's site index, one int.
    Returns WindowPredictions(top_idx, top_score, probs or None, crowns or None) as predict_windows does."""
    return _metadata_route(_WINDOWS, predictor, raster, site, origins, crown_offsets, batch_size, return_probs)


def predict_crops_metadata(predictor, raster, site, boxes, batch_size=4096, return_probs=False):
    """predict_crops for the site-metadata fusion model: the crops of predict_crops through predict_windows_metadata's
    loop (the sensor model's eval forward, then dta_meta_predict with the raster's site for every row).  predictor /
    raster / site as for predict_windows_metadata; boxes as for predict_crops.  No share_conv1: see predict_crops.
    Returns WindowPredictions, one row per box, crowns=None."""
    return _metadata_route(_CROPS, predictor, raster, site, boxes, None, batch_size, return_probs)


def _metadata_route(gather, predictor, raster, site, items, crown_offsets, batch_size, return_probs):
    """predict_windows_metadata / predict_crops_metadata: the checks, then _predict_batches with this route's batch."""
    from .engine import MetadataPredictor
    if not isinstance(predictor, MetadataPredictor):
        raise TypeError("the metadata route needs an engine.MetadataPredictor")
    if not isinstance(raster, DenseRaster):
        raise TypeError("raster must be a DenseRaster")
    sens = predictor.sensor
    want = raster_precision(sens)
    if raster.precision != want:
        raise RuntimeError("this network reads a DenseRaster(..., precision={!r}) (dense.raster_precision)".format(want))
    site = int(site)
    if not 0 <= site < predictor.sites:
        raise ValueError("site {} is outside [0, {})".format(site, predictor.sites))
    size = WINDOW
    o = gather.index(raster, items)
    B, crown_offsets = _batch_plan(o.shape[0], batch_size, crown_offsets)
    buf = raster._batch(B, size)
    ws = predictor.table()

    def batch(n, ob, *out):
        x = gather.one(raster, ob, tiles=want == "bf16", size=size, out=buf[:n])
        predictor.head(sens.logits_of(x), n, ws, site, None, *out)
    return _predict_batches(o, B, crown_offsets, predictor.classes, return_probs, batch)


def predict_map_metadata(predictor, raster, site, anchor="center", rows=None, cols=None, clip=10, batch_size=4096):
    """predict_map for the site-metadata fusion model: raster is a raw band-first array or a DenseRaster, site its site
    index.  Returns (labels [h][w] int64, scores [h][w] float32): the top-1 class of each pixel's window and its probability."""
    from .engine import MetadataPredictor
    if not isinstance(predictor, MetadataPredictor):
        raise TypeError("the metadata route needs an engine.MetadataPredictor")
    if not isinstance(raster, DenseRaster):
        raster = DenseRaster(raster, clip=clip, precision=raster_precision(predictor.sensor), device=predictor.device)
    origins, hw = _region(raster, rows, cols, anchor)
    res = predict_windows_metadata(predictor, raster, site, origins, batch_size=batch_size)
    return res.top_idx[:, 0].reshape(hw), res.top_score[:, 0].reshape(hw)
