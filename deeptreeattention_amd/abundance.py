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


def counts_np(label, S, mask=None):
    """Trees per species: int64 [S + 1], bin S for every label outside [0, S) (DEAD, the walk's unresolved -1); a crown
    with mask == 0 is counted nowhere (the reference's clip to a boundary, decided by the caller: boundary.Boundary.clip
    gives that mask on the device)."""
    bins, _, live = _bins(label, int(S), mask)
    return np.bincount(bins[live], minlength=int(S) + 1).astype(np.int64)


def resample_np(label, score, table, iterations, seed=0, first_iteration=0, mask=None):
    """The definition of the resampled counts: int64 [iterations][S + 1].

    For iteration t and crown i of N the counter is the 64-bit (first_iteration + t) * N + i (modulo 2^64), and
        r_keep = draw24(seed, 0, counter),  r_draw = draw24(seed, 1, counter)          (_hash.py states the hash)
        keep   = not (float32(r_keep) * 2^-24 >= score)        one float32 comparison; a NaN score keeps, score None: all keep
        drawn  = the number of entries of table[label] that are <= r_draw
        final  = label if keep else drawn
    A label outside [0, S) goes to bin S whatever its score; a crown with mask == 0 is counted nowhere.
    first_iteration=k with iterations=1 is row k of a longer run (the reference's one iteration per call)."""
    t = _check_table(table)
    S = t.shape[0]
    bins, inside, live = _bins(label, S, mask)
    N = len(bins)
    if score is None:
        score = np.full(N, np.nan, np.float32)
    score = np.asarray(_host(score), np.float32).reshape(-1)
    if len(score) != N:
        raise ValueError("score must have one entry per crown")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    out = np.zeros((iterations, S + 1), np.int64)
    if N == 0:
        return out
    # rows laid end to end with the row number above the thresholds: one sorted array, so a crown's count of entries
    # <= r_draw in its row is a searchsorted away
    flat = (np.arange(S, dtype=np.int64)[:, None] * (2 * SCALE + 2) + t).reshape(-1)
    resample = inside & live
    rows = bins[resample]
    idx = np.flatnonzero(resample).astype(np.uint64)
    sc = score[resample]
    fixed = np.bincount(bins[live & ~inside], minlength=S + 1).astype(np.int64)
    with np.errstate(over="ignore"):
        for it in range(iterations):
            counter = np.uint64(shuffle_base(int(first_iteration) + it, N)) + idx
            keep = ~((draw24(seed, STREAM_ABUNDANCE_KEEP, counter).astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)) >= sc)
            r = draw24(seed, STREAM_ABUNDANCE_DRAW, counter)
            drawn = np.searchsorted(flat, rows * (2 * SCALE + 2) + r, side="right") - rows * S
            out[it] = fixed + np.bincount(np.where(keep, rows, drawn), minlength=S + 1)
    return out


AbundanceSummary = collections.namedtuple("AbundanceSummary", "mean quantiles q")


def summary(counts, q=(0.025, 0.5, 0.975)):
    """Per-bin mean [S + 1] and quantiles [len(q)][S + 1] over the iterations of `counts` [iterations][S + 1] (host)."""
    c = np.asarray(_host(counts), np.float64)
    if c.ndim != 2 or c.shape[0] < 1:
        raise ValueError("counts must be [iterations][S + 1] with at least one iteration")
    return AbundanceSummary(c.mean(0), np.quantile(c, list(q), axis=0), tuple(q))


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


def resample(label, score, table, iterations=100, seed=0, first_iteration=0, mask=None, out=None):
    """resample_np on the device (dta_abundance_resample: every iteration in one launch, a second small one sums the
    workgroups' partial histograms): int64 [iterations][S + 1] on the device (out=: that tensor), overwritten in full by
    the call, never added to.

    label int64 [N] / score float32 [N] (None: all keep) / mask bool or uint8 [N] (optional): device tensors, taken as
    dense.MultiStageWindowPredictions and MultiStagePredictor.ensemble leave them.  table: the uint32 (or int32) [S][S]
    device tensor of device_table -- upload it once and keep it -- or whatever sampling_table returns, which is then
    checked and uploaded by this call.  Nothing here waits for the device."""
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
    if out is None:
        out = torch.empty(iterations, S + 1, dtype=torch.int64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (iterations, S + 1)
            or out.device != dev or not out.is_contiguous()):
        raise ValueError("out must be a contiguous int64 [{}][{}] tensor on {}".format(iterations, S + 1, dev))
    if iterations == 0:
        return out
    L = _lib.lib()
    ws, nbytes = _workspace(L, n, S, iterations, dev)
    _lib.check(L.dta_abundance_resample(_lib.ptr(label), _lib.ptr(score), _lib.ptr(mask), n, _lib.ptr(table), S, iterations,
                                        int(seed) & _M64, int(first_iteration) & _M64, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                        _lib.current_stream_ptr()), "dta_abundance_resample")
    return out


def counts(label, species, mask=None):
    """counts_np on the device (dta_abundance_counts): int64 [species + 1], overwritten in full by the call."""
    import torch
    from . import _lib
    label, _, mask, n, dev = _crowns(label, None, mask)
    species = int(species)
    if not 1 <= species <= MAX_SPECIES:
        raise ValueError("species must be 1..{}".format(MAX_SPECIES))
    out = torch.empty(species + 1, dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws, nbytes = _workspace(L, n, species, 1, dev)
    _lib.check(L.dta_abundance_counts(_lib.ptr(label), _lib.ptr(mask), n, species, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                      _lib.current_stream_ptr()), "dta_abundance_counts")
    return out
