"""Species abundance with uncertainty: trees per species over the predicted crowns of a site, and the reference's
confusion resampling of that count (src/multinomial.py, driven 100 times by sample_multinomial.py; abundance.py's
`value_counts` is the plain count).

The rule, per crown and per iteration (multinomial.py:28-35, 61-77):
  * the crown keeps its predicted label with probability ens_score (`sample_binomial`; a missing / NaN score keeps);
  * otherwise it is drawn again from the row of the normalised confusion matrix that belongs to its predicted taxon
    (`sample_confusion`; `format_confusion_json` divides each row by its sum);
  * DEAD crowns stay DEAD;
  * then the labels are counted.
The reference draws from NumPy's global generator inside pandas lambdas; a device cannot follow that stream, so the random
numbers are THIS package's: a counter-based hash, the same for the host mirror and the kernel.  Everything that decides a
draw is integer arithmetic or one exact float32 comparison, so `resample` (k_abundance_resample, csrc/abundance.hip) equals
`resample_np` bit for bit; the tie to the reference is statistical (tests/golden/abundance/abundance_reference.npz).

The NumPy functions are the definition (as hierarchy.resolve_np and dense.crown_reduce_np are).
"""
import collections

import numpy as np

# the hash is _hash.py's: oracle/prng.py's construction, restated there because the product never imports the oracle
from ._hash import M64 as _M64, STREAM_ABUNDANCE_DRAW, STREAM_ABUNDANCE_KEEP, draw24, host as _host, shuffle_base
from ._hash import mix_int as _mix_int, stream_key  # noqa: F401  (their names here, which callers and tests use)

SCALE_BITS = 24
SCALE = 1 << SCALE_BITS          # a threshold of 2^24 is above every 24-bit draw
MAX_SPECIES = 256                # DTA_ABUNDANCE_MAX_SPECIES


def sampling_table(confusion, given="label"):
    """The cumulative thresholds a crown is re-drawn with: uint32 [S][S], row p for a crown PREDICTED as p.

    confusion: [S][S] counts, rows = label, columns = prediction (the package's and Comet's orientation; what the
    reference's visualize.confusion_matrix logs), or an already row-stochastic float table.  A device tensor (e.g.
    MultiStagePredictor.confusion) is copied to the host.
    given="label": the reference's behaviour -- each ROW divided by its sum, and the row of the predicted label used.
    given="prediction": each COLUMN divided by its sum, P(true | predicted), and the column of the predicted label used
    (= given="label" on the transposed matrix).

    Row p = floor(cumsum(row / sum(row), float64) * 2^24); every entry from the row's last non-zero column onward is 2^24,
    so the row ends above every draw and a species of probability zero (a zero-width interval) is never drawn.  A row
    whose sum is zero is the identity: 0 before p, 2^24 from p on -- the label is kept (the reference divides by zero).
    The drawn species of a 24-bit draw r is the number of entries of the row that are <= r."""
    if given not in ("label", "prediction"):
        raise ValueError("given must be 'label' or 'prediction', got {!r}".format(given))
    m = np.array(_host(confusion), dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError("confusion must be a square [S][S] matrix, got shape {}".format(m.shape))
    if m.shape[0] > MAX_SPECIES:
        raise ValueError("at most {} species, got {}".format(MAX_SPECIES, m.shape[0]))
    if not np.isfinite(m).all() or (m < 0).any():
        raise ValueError("confusion must be finite and non-negative")
    if given == "prediction":
        m = m.T
    S = m.shape[0]
    table = np.empty((S, S), np.uint32)
    for p in range(S):
        total = m[p].sum()
        if total <= 0:
            table[p, :p] = 0
            table[p, p:] = SCALE
            continue
        t = np.minimum(np.floor(np.cumsum(m[p] / total) * SCALE), SCALE)
        t[np.flatnonzero(m[p])[-1]:] = SCALE
        table[p] = t.astype(np.uint32)
    return table


def _check_table(table):
    t = _host(table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 1 or t.shape[0] > MAX_SPECIES:
        raise ValueError("table must be [S][S] with 1 <= S <= {}, got shape {}".format(MAX_SPECIES, t.shape))
    if t.dtype.kind not in "iu":
        raise ValueError("table must hold the integer thresholds of sampling_table, got dtype {}".format(t.dtype))
    t = t.astype(np.int64)
    if (np.diff(t, axis=1) < 0).any() or (t < 0).any() or (t[:, -1] != SCALE).any():
        raise ValueError("every table row must be non-decreasing and end at 2^24 (sampling_table makes such rows)")
    return t


def _bins(label, S, mask):
    """The bin of each crown's own label (S for a label outside [0, S)) and which crowns count at all."""
    label = np.asarray(_host(label), np.int64).reshape(-1)
    inside = (label >= 0) & (label < S)
    live = np.ones(len(label), bool) if mask is None else np.asarray(_host(mask)).reshape(-1) != 0
    if len(live) != len(label):
        raise ValueError("mask must have one entry per crown")
    return np.where(inside, label, S), inside, live


def _cells_of(group, groups, live):
    """group= / groups= of counts_np and resample_np: (G, the cell of each crown, which crowns count at all).  A crown whose
    group is outside [0, G) counts nowhere, exactly like mask == 0; group None: one cell, every crown in it."""
    if group is None:
        if groups is not None:
            raise ValueError("groups without group")
        return None, None, live
    if groups is None or int(groups) < 1:
        raise ValueError("group needs groups >= 1, the number of cells")
    G = int(groups)
    cell = np.asarray(_host(group)).reshape(-1)
    if cell.dtype.kind not in "iu" or len(cell) != len(live):
        raise ValueError("group must hold one integer cell index per crown")
    cell = cell.astype(np.int64)
    ok = (cell >= 0) & (cell < G)
    return G, np.where(ok, cell, 0), live & ok


def counts_np(label, S, mask=None, group=None, groups=None):
    """Trees per species: int64 [S + 1], bin S for every label outside [0, S) (DEAD, the walk's unresolved -1); a crown
    with mask == 0 is counted nowhere (the reference's clip to a boundary, decided by the caller: boundary.Boundary.clip
    gives that mask on the device).
    group= (int64 [N], e.g. cells_np's) with groups=G: int64 [G][S + 1], row g = counts_np(mask=mask & (group == g)); a
    crown whose group is outside [0, G) is counted nowhere."""
    S = int(S)
    bins, _, live = _bins(label, S, mask)
    G, cell, live = _cells_of(group, groups, live)
    if G is None:
        return np.bincount(bins[live], minlength=S + 1).astype(np.int64)
    return np.bincount(cell[live] * (S + 1) + bins[live], minlength=G * (S + 1)).astype(np.int64).reshape(G, S + 1)


def resample_np(label, score, table, iterations, seed=0, first_iteration=0, mask=None, group=None, groups=None):
    """The definition of the resampled counts: int64 [iterations][S + 1].

    For iteration t and crown i of N the counter is the 64-bit (first_iteration + t) * N + i (modulo 2^64), and
        r_keep = draw24(seed, 0, counter),  r_draw = draw24(seed, 1, counter)          (_hash.py states the hash)
        keep   = not (float32(r_keep) * 2^-24 >= score)        one float32 comparison; a NaN score keeps, score None: all keep
        drawn  = the number of entries of table[label] that are <= r_draw
        final  = label if keep else drawn
    A label outside [0, S) goes to bin S whatever its score; a crown with mask == 0 is counted nowhere.
    first_iteration=k with iterations=1 is row k of a longer run (the reference's one iteration per call).

    group= (int64 [N]: the tile or map cell of each crown, e.g. cells_np's) with groups=G: int64 [iterations][G][S + 1],
    and [:, g] is by construction resample_np(..., mask=mask & (group == g)) on the same N, seed and first_iteration: i
    is the crown's index in the whole input, so a crown draws the same species whichever cell it is counted in (the
    reference resamples tile by tile, src/multinomial.py:run, and adds the tiles up, :79-98).  A crown whose group is
    outside [0, G) is counted nowhere."""
    t = _check_table(table)
    S = t.shape[0]
    bins, inside, live = _bins(label, S, mask)
    G, cell, live = _cells_of(group, groups, live)
    N = len(bins)
    if score is None:
        score = np.full(N, np.nan, np.float32)
    score = np.asarray(_host(score), np.float32).reshape(-1)
    if len(score) != N:
        raise ValueError("score must have one entry per crown")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    shape = (iterations, S + 1) if G is None else (iterations, G, S + 1)
    width = (S + 1) * (1 if G is None else G)
    out = np.zeros((iterations, width), np.int64)
    if N == 0:
        return out.reshape(shape)
    # rows laid end to end with the row number above the thresholds: one sorted array, so a crown's count of entries
    # <= r_draw in its row is a searchsorted away
    flat = (np.arange(S, dtype=np.int64)[:, None] * (2 * SCALE + 2) + t).reshape(-1)
    resample = inside & live
    rows = bins[resample]
    idx = np.flatnonzero(resample).astype(np.uint64)
    sc = score[resample]
    other = live & ~inside
    # the first bin of each crown's cell in a row of `out` (one cell: 0)
    at = np.zeros(N, np.int64) if G is None else cell * (S + 1)
    fixed = np.bincount(at[other] + bins[other], minlength=width).astype(np.int64)
    at = at[resample]
    with np.errstate(over="ignore"):
        for it in range(iterations):
            counter = np.uint64(shuffle_base(int(first_iteration) + it, N)) + idx
            keep = ~((draw24(seed, STREAM_ABUNDANCE_KEEP, counter).astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)) >= sc)
            r = draw24(seed, STREAM_ABUNDANCE_DRAW, counter)
            drawn = np.searchsorted(flat, rows * (2 * SCALE + 2) + r, side="right") - rows * S
            out[it] = fixed + np.bincount(at + np.where(keep, rows, drawn), minlength=width)
    return out.reshape(shape)


AbundanceSummary = collections.namedtuple("AbundanceSummary", "mean quantiles q")


def summary(counts, q=(0.025, 0.5, 0.975)):
    """Per-bin mean [S + 1] and quantiles [len(q)][S + 1] over the iterations of `counts` [iterations][S + 1] (host)."""
    c = np.asarray(_host(counts), np.float64)
    if c.ndim != 2 or c.shape[0] < 1:
        raise ValueError("counts must be [iterations][S + 1] with at least one iteration")
    return AbundanceSummary(c.mean(0), np.quantile(c, list(q), axis=0), tuple(q))


SUMMARY_MAX_ITERATIONS = 256     # DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS
SUMMARY_MAX_QUANTILES = 16       # DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES


def _quantile_plan(q, T):
    """NumPy's linear rule for T sorted values, per quantile: the lower order statistic floor(q * (T - 1)) and the
    remainder g in [0, 1), both from float64 arithmetic (the device is handed these, it forms neither)."""
    q = [float(x) for x in q]
    if not all(0.0 <= x <= 1.0 for x in q):
        raise ValueError("quantiles must lie in [0, 1]")
    virtual = np.asarray(q, np.float64) * np.float64(T - 1)
    lower = np.floor(virtual)
    return lower.astype(np.int64), virtual - lower


def summary_np(counts, q=(0.025, 0.5, 0.975)):
    """The definition of summary_device: mean float64 [...] and quantiles float64 [len(q)][...] over the iterations of an
    integer table `counts` [iterations][...] (the [S + 1] of resample, or its grouped [G][S + 1]).
      mean      the integer sum divided once in float64: exact in any order while the sum is below 2^53
      quantile  NumPy's linear rule spelt out: virtual index v = q * (T - 1), lower = floor(v), g = v - lower; a <= b the
                lower-th and min(lower + 1, T - 1)-th smallest value; a + (b - a) * g, or b - (b - a) * (1 - g) when g >= 0.5
    which is what `summary` (np.mean / np.quantile) returns, entry for entry."""
    c = np.asarray(_host(counts))
    if c.dtype.kind not in "iu" or c.ndim < 1 or c.shape[0] < 1:
        raise ValueError("counts must be an integer table [iterations][...] with at least one iteration")
    T = c.shape[0]
    lower, g = _quantile_plan(q, T)
    s = np.sort(c.astype(np.int64), axis=0).astype(np.float64)
    quantiles = np.empty((len(lower),) + c.shape[1:], np.float64)
    for j in range(len(lower)):
        a, b = s[lower[j]], s[min(lower[j] + 1, T - 1)]
        d = b - a
        quantiles[j] = b - d * (1.0 - g[j]) if g[j] >= 0.5 else a + d * g[j]
    return AbundanceSummary(c.sum(0, dtype=np.int64) / np.float64(T), quantiles, tuple(q))


# ---------------------------------------------------------------------------------------------------------------------
# which tile or map cell a crown is in
# ---------------------------------------------------------------------------------------------------------------------
RULES = {"geoindex": 0, "centre": 1}      # DTA_CELLS_GEOINDEX, DTA_CELLS_CENTRE
_CELL_LIMIT = 2.0 ** 53


def _grid(cols, rows, origin, size, rule):
    if rule not in RULES:
        raise ValueError("rule must be 'geoindex' or 'centre', got {!r}".format(rule))
    cols, rows = int(cols), int(rows)
    if not (1 <= cols < 2 ** 31 and 1 <= rows < 2 ** 31):
        raise ValueError("a grid has cols >= 1 and rows >= 1 (below 2^31)")
    ox, oy = (float(v) for v in origin)
    size = float(size)
    if not (np.isfinite([ox, oy, size]).all() and size > 0):
        raise ValueError("size must be positive, size and origin finite")
    if rule == "geoindex" and not (size == np.floor(size) and ox == np.floor(ox) and oy == np.floor(oy) and size < 2 ** 31
                                   and abs(ox) < _CELL_LIMIT and abs(oy) < _CELL_LIMIT):
        raise ValueError("the geoindex rule takes an integer size (below 2^31) and an integer origin (below 2^53)")
    return cols, rows, ox, oy, size


def cells_np(boxes, cols, rows, origin=(0, 0), size=1000, rule="geoindex"):
    """The definition of `cells`: int64 [N], the cell row * cols + col of each geographic crown box (xmin, ymin, xmax, ymax)
    (float64 [N][4], as boundary.geo_boxes returns them) in a cols x rows grid of `size`-sized cells whose south-west corner
    is `origin`; rows grow with northing; -1 outside the grid.  Float64, every operation rounded on its own.  Per axis:
      rule="geoindex"  the reference's src/neon_paths.py:bounds_to_geoindex: e = int((lo + hi) / 2), truncated toward zero,
                       then floor_div(e - origin, size) in integers (integer size and origin; the reference has origin 0,
                       size 1000).  A centre that is not finite or not below 2^53 gives -1.
      rule="centre"    floor(((lo + hi) * 0.5 - origin) / size): hectare cells, any float size and origin."""
    cols, rows, ox, oy, size = _grid(cols, rows, origin, size, rule)
    b = np.asarray(_host(boxes))
    if b.dtype != np.float64 or b.ndim != 2 or b.shape[1] != 4:
        raise ValueError("boxes must be a float64 [N][4] array of (xmin, ymin, xmax, ymax)")
    axes = []
    with np.errstate(invalid="ignore", over="ignore"):
        for lo, hi, o, count in ((b[:, 0], b[:, 2], ox, cols), (b[:, 1], b[:, 3], oy, rows)):
            if rule == "geoindex":
                c = (lo + hi) / 2.0
                ok = np.abs(c) < _CELL_LIMIT                      # false for NaN
                k = (np.trunc(np.where(ok, c, 0.0)).astype(np.int64) - np.int64(o)) // np.int64(size)
            else:
                kf = np.floor(((lo + hi) * 0.5 - o) / size)
                ok = (kf >= 0) & (kf < count)                     # false for NaN
                k = np.where(ok, kf, 0.0).astype(np.int64)
            axes.append(np.where(ok & (k >= 0) & (k < count), k, -1))
    col, row = axes
    return np.where((col < 0) | (row < 0), -1, row * cols + col).astype(np.int64)


def cell_names(cols, rows, origin=(0, 0), size=1000):
    """The reference's "{easting}_{northing}" name of every cell of a geoindex grid, in cell order (row * cols + col): the
    south-west corner of the cell.  With an origin that is a multiple of size = 1000 these are the strings
    bounds_to_geoindex gives, the names NEON's tile files carry, so device results join to tile files by name."""
    cols, rows, ox, oy, size = _grid(cols, rows, origin, size, "geoindex")
    ox, oy, size = int(ox), int(oy), int(size)
    return ["{}_{}".format(ox + c * size, oy + r * size) for r in range(rows) for c in range(cols)]


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
def device_table(table, device):
    """The thresholds on the device (uint32 [S][S], checked on the host first): upload once, pass to every resample."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(_check_table(table).astype(np.uint32))).to(device)


def _crowns(label, score, mask):
    import torch
    if not isinstance(label, torch.Tensor) or label.dtype != torch.int64 or label.dim() != 1 or not label.is_cuda:
        raise ValueError("label must be an int64 [N] tensor on the device")
    n, dev = label.shape[0], label.device
    if n < 1:
        raise ValueError("no crowns")
    if score is not None:
        if not isinstance(score, torch.Tensor) or score.dtype != torch.float32 or tuple(score.shape) != (n,) or score.device != dev:
            raise ValueError("score must be a float32 [{}] tensor on {} (or None: every crown keeps its label)".format(n, dev))
        score = score.contiguous()
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (n,)
                or mask.device != dev):
            raise ValueError("mask must be a bool / uint8 [{}] tensor on {}".format(n, dev))
        mask = mask.contiguous().view(torch.uint8)
    return label.contiguous(), score, mask, n, dev


def _workspace(L, n, species, iterations, dev):
    import torch
    nbytes = L.dta_abundance_workspace_bytes(n, species, iterations)
    if nbytes == 0:
        raise RuntimeError("dta_abundance_workspace_bytes: " + L.dta_last_error().decode())
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _order(group, groups, n, dev):
    """group= / groups= of the device route: (G, the groups ascending, the crown at each sorted position).  The ordering is
    a stable torch.sort on the current stream; nothing waits for it."""
    import torch
    if groups is None or int(groups) < 1:
        raise ValueError("group needs groups >= 1, the number of cells")
    if (not isinstance(group, torch.Tensor) or group.dtype != torch.int64 or tuple(group.shape) != (n,) or group.device != dev):
        raise ValueError("group must be an int64 [{}] tensor on {}".format(n, dev))
    G = int(groups)
    if G > 2 ** 31 - 2:
        raise ValueError("groups must be below 2^31 - 1")
    group_sorted, order = torch.sort(group, stable=True)
    return G, group_sorted, order


def _grouped_workspace(L, n, species, iterations, G, dev):
    import torch
    nbytes = L.dta_abundance_grouped_workspace_bytes(n, species, iterations, G)
    if nbytes == 0:
        raise RuntimeError("dta_abundance_grouped_workspace_bytes: " + L.dta_last_error().decode())
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def resample(label, score, table, iterations=100, seed=0, first_iteration=0, mask=None, out=None, group=None, groups=None):
    """resample_np on the device (dta_abundance_resample: every iteration in one launch, a second small one sums the
    workgroups' partial histograms): int64 [iterations][S + 1] on the device (out=: that tensor), overwritten in full by
    the call, never added to.

    label int64 [N] / score float32 [N] (None: all keep) / mask bool or uint8 [N] (optional): device tensors, taken as
    dense.MultiStageWindowPredictions and MultiStagePredictor.ensemble leave them.  table: the uint32 (or int32) [S][S]
    device tensor of device_table -- upload it once and keep it -- or whatever sampling_table returns, which is then
    checked and uploaded by this call.  Nothing here waits for the device.

    group= (int64 [N] on the device, e.g. what `cells` returns) with groups=G: the table per cell, int64 [iterations][G]
    [S + 1] (dta_abundance_resample_grouped: the crowns are ordered by cell with a stable torch.sort, gathered once, and
    every iteration of every cell is counted in one launch; a crown is read once per 8 iterations, not once per cell).
    [:, g] equals resample(mask=mask & (group == g)) bit for bit; a crown whose group is outside [0, G) counts nowhere."""
    import torch
    from . import _lib
    label, score, mask, n, dev = _crowns(label, score, mask)
    if not isinstance(table, torch.Tensor):
        table = device_table(table, dev)
    if (table.dtype not in (torch.uint32, torch.int32) or table.dim() != 2 or table.shape[0] != table.shape[1]
            or table.device != dev or not 1 <= table.shape[0] <= MAX_SPECIES):
        raise ValueError("table must be a uint32 [S][S] tensor on {} with S <= {} (abundance.device_table)".format(dev, MAX_SPECIES))
    table = table.contiguous()
    S, iterations = table.shape[0], int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    if group is None and groups is not None:
        raise ValueError("groups without group")
    if group is not None:
        G, group_sorted, order = _order(group, groups, n, dev)
    shape = (iterations, S + 1) if group is None else (iterations, G, S + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != shape
            or out.device != dev or not out.is_contiguous()):
        raise ValueError("out must be a contiguous int64 {} tensor on {}".format("".join("[{}]".format(d) for d in shape), dev))
    if iterations == 0:
        return out
    L = _lib.lib()
    if group is not None:
        ws, nbytes = _grouped_workspace(L, n, S, iterations, G, dev)
        _lib.check(L.dta_abundance_resample_grouped(_lib.ptr(label), _lib.ptr(score), _lib.ptr(mask), _lib.ptr(group_sorted),
                                                    _lib.ptr(order), n, G, _lib.ptr(table), S, iterations, int(seed) & _M64,
                                                    int(first_iteration) & _M64, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                    _lib.current_stream_ptr()), "dta_abundance_resample_grouped")
        return out
    ws, nbytes = _workspace(L, n, S, iterations, dev)
    _lib.check(L.dta_abundance_resample(_lib.ptr(label), _lib.ptr(score), _lib.ptr(mask), n, _lib.ptr(table), S, iterations,
                                        int(seed) & _M64, int(first_iteration) & _M64, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                        _lib.current_stream_ptr()), "dta_abundance_resample")
    return out


def counts(label, species, mask=None, group=None, groups=None):
    """counts_np on the device (dta_abundance_counts): int64 [species + 1], overwritten in full by the call.
    group= (int64 [N] on the device) with groups=G: int64 [G][species + 1] (dta_abundance_counts_grouped)."""
    import torch
    from . import _lib
    label, _, mask, n, dev = _crowns(label, None, mask)
    species = int(species)
    if not 1 <= species <= MAX_SPECIES:
        raise ValueError("species must be 1..{}".format(MAX_SPECIES))
    if group is None and groups is not None:
        raise ValueError("groups without group")
    if group is not None:
        G, group_sorted, order = _order(group, groups, n, dev)
        out = torch.empty(G, species + 1, dtype=torch.int64, device=dev)
        L = _lib.lib()
        ws, nbytes = _grouped_workspace(L, n, species, 1, G, dev)
        _lib.check(L.dta_abundance_counts_grouped(_lib.ptr(label), _lib.ptr(mask), _lib.ptr(group_sorted), _lib.ptr(order), n, G,
                                                  species, _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.current_stream_ptr()),
                   "dta_abundance_counts_grouped")
        return out
    out = torch.empty(species + 1, dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws, nbytes = _workspace(L, n, species, 1, dev)
    _lib.check(L.dta_abundance_counts(_lib.ptr(label), _lib.ptr(mask), n, species, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                      _lib.current_stream_ptr()), "dta_abundance_counts")
    return out


def cells(boxes, cols, rows, origin=(0, 0), size=1000, rule="geoindex"):
    """cells_np on the device (dta_abundance_cells, one launch): int64 [N] on the device, ready to be the group= of counts
    and resample.  boxes: a float64 [N][4] device tensor of geographic boxes (boundary.geo_boxes, uploaded)."""
    import ctypes as C
    import torch
    from . import _lib
    cols, rows, ox, oy, size = _grid(cols, rows, origin, size, rule)
    if (not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 4
            or boxes.shape[0] < 1 or not boxes.is_cuda):
        raise ValueError("boxes must be a non-empty float64 [N][4] tensor on the device")
    boxes = boxes.contiguous()
    out = torch.empty(boxes.shape[0], dtype=torch.int64, device=boxes.device)
    org = (C.c_double * 2)(ox, oy)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.lib().dta_abundance_cells(_lib.ptr(boxes), boxes.shape[0], RULES[rule], org, size, cols, rows,
                                                  _lib.ptr(out), _lib.current_stream_ptr()), "dta_abundance_cells")
    return out


def summary_device(counts, q=(0.025, 0.5, 0.975)):
    """summary_np on the device (dta_abundance_summary, one launch): AbundanceSummary whose mean [...] and quantiles
    [len(q)][...] are float64 device tensors, for an int64 device table [iterations][...], grouped or not -- a map of means
    and intervals instead of the whole table read back.  The lower order statistic and the remainder of each quantile are
    formed here in float64 (_quantile_plan) and handed to the kernel.  At most SUMMARY_MAX_ITERATIONS iterations (a lane
    sorts its column in LDS): a longer run goes through `summary` on the host."""
    import ctypes as C
    import torch
    from . import _lib
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.dim() < 1 or not counts.is_cuda
            or not counts.is_contiguous() or counts.numel() < 1):
        raise ValueError("counts must be a non-empty contiguous int64 [iterations][...] tensor on the device")
    T = counts.shape[0]
    if T > SUMMARY_MAX_ITERATIONS:
        raise ValueError("summary_device takes at most {} iterations, got {}: read the table back and use abundance.summary "
                         "on the host".format(SUMMARY_MAX_ITERATIONS, T))
    q = tuple(q)
    if len(q) > SUMMARY_MAX_QUANTILES:
        raise ValueError("at most {} quantiles per call".format(SUMMARY_MAX_QUANTILES))
    lower, g = _quantile_plan(q, T)
    rest = tuple(counts.shape[1:])
    entries = counts.numel() // T
    mean = torch.empty(rest, dtype=torch.float64, device=counts.device)
    quantiles = torch.empty((len(q),) + rest, dtype=torch.float64, device=counts.device)
    lo = (C.c_int * max(len(q), 1))(*[int(v) for v in lower])
    fr = (C.c_double * max(len(q), 1))(*[float(v) for v in g])
    with torch.cuda.device(counts.device):
        _lib.check(_lib.lib().dta_abundance_summary(_lib.ptr(counts), T, entries, lo, fr, len(q), _lib.ptr(mean),
                                                    _lib.ptr(quantiles), _lib.current_stream_ptr()), "dta_abundance_summary")
    return AbundanceSummary(mean, quantiles, q)
