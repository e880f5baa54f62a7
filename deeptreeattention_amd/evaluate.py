"""Crown-level evaluation: the reference's experiment report.  `MultiStage.evaluation_scores` (src/models/multi_stage.py:436-485)
and `TreeModel.evaluate_crowns` (src/main.py:265-333) keep the first row per individual (`groupby("individual").head(1)`), take
per-species accuracy and precision, and build a per-site table with one pandas group and one torchmetrics call per site;
`site_confusion` and `genus_confusion` (src/metrics.py:8-72) are Python loops over every prediction with a list-membership
test per error; `novel_prediction` (:74-107) indexes per-batch argmaxes on the host.  Here every figure is a function of ONE
grouped confusion table

    conf[g][t][p] = the number of counted crowns of group g (the site code) with label t and prediction p

counted on the device from the label tensors the prediction chain leaves there (dta_eval_count), and reduced in one launch
(dta_eval_report); one small buffer comes back, not the table.  The kernels are in csrc/evaluate.hip.

1. count_np / EvalTable.count.  A row with mask == 0 is neither counted nor tallied.  A row whose label or prediction is
outside [0, S) or whose group is outside [0, G) is skipped and adds one to tally[1] (-1 is the top-1 of a row of NaN); every
other row adds one to conf[group][label][pred] and to tally[0].  Sizes: 1 <= S <= 1020 (the softmax kernels' limit), G >= 1 and
G * S * S <= 2^31 - 1: the device indexes an entry with an int.  Two forms of the same count: PLAIN, one 64-bit atomic add per
counted row, and COMBINE, where the lanes of a wave that hold the same entry are added up first (four first-lane / ballot
rounds, the rest singly).  Integer adds commute: the table does not depend on the form or on the order, and reruns are
bit-identical.  FORM is the one count() uses unless told otherwise; profiles/README.md has the measurement behind it.

2. report_np / EvalTable.report.  Row g < G of every output is plane g, row G the sum of all planes (the pooled row):
    counts    int64   [G+1][8]  total, correct, wrong, within_site, cross_site, within_genus, cross_genus, species seen
    scores    float64 [G+1][4]  micro, macro, within-site share, within-genus share
    accuracy, precision float64 [G+1][S], support int64 [G+1][S]   (per_species)
Conventions of hierarchy.scores_from_confusion -- stated convention, not reference parity (torchmetrics is not what these are
held to): accuracy = diagonal / label sum, precision = diagonal / prediction sum, a zero denominator gives 0.0, a species
without samples ("not seen") is left out of macro.  Every quotient is double(int) / double(int), one IEEE division.  macro is
the seen species' accuracies added left to right in class order (np.cumsum(...)[-1], not np.mean, whose pairwise order is an
implementation detail), divided by their number; it agrees with scores_from_confusion's to a relative S * 2^-52, the other
figures exactly.  An error (t != p) is within_site when site_masks[t] & site_masks[p] != 0 (the reference's `any(site in
incorrect_site for site in correct_sites)`) and within_genus when genus[t] == genus[p]; the two shares are over all errors
and 0.0 when there is none, as the reference returns 0.  Without site_masks / genus the two counts are 0 and the share 0.0.

3. site_masks(site_lists, n_species): uint64 [S][W], bit positions follow the sorted unique sites, W = ceil(sites / 64) <= 4.
A species without an entry gets an EMPTY mask: its errors are cross-site.  Deviation: the reference raises KeyError on the
first error that involves such a species.  genus_ids(scientific_dict, n_species): int32 [S] from the reference's expression
taken literally, `value[0].split()[0]`: the first word of the first name when the value is a list, the first CHARACTER when
it is a plain string (the reference's own test relies on that: "QUMU" and "QUMLA" are one genus, "Q").  A species without an
entry gets an id equal to no other (same deviation).

4. first_per_individual_np / first_per_individual: bool [N], the first row of each individual code -- the reference's
`groupby("individual").head(1)`, also create_prediction_shp.py:35; a code outside [0, n_individuals) gives False.  The mask
is what EvalTable.count(mask=) and abundance.counts(mask=) take.

5. novel_scores_np / novel_scores: NovelScores(label, top_score, softmax_score) per row of logits (metrics.py:91-93).  The
device runs dta_softmax_top2's own row body: label and softmax_score are bit for bit that entry's top_idx[:, 0] and
top_score[:, 0] (ties to the lower class; a row with a NaN gives -1 and -1.0), top_score is logits.max(1) (NaN for such a row).
novel_scores_np is the float64 CPU route with the same rules.

6. evaluate_crowns mirrors evaluation_scores: the first-row mask, one count, one report, the host dict.  It is the only
function here that waits for the device.  Given NumPy arrays it runs the definitions, so it works without a GPU.

Out of scope: top-k accuracy per site, comet logging and plots, reading shapefiles."""
import collections

import numpy as np

MAX_SPECIES = 1020               # DTA_EVAL_MAX_SPECIES
MAX_SITE_WORDS = 4               # DTA_EVAL_MAX_SITE_WORDS
PLAIN, COMBINE = 0, 1            # DTA_EVAL_COUNT_*
FORM = COMBINE                   # what EvalTable.count uses by default (profiles/README.md, "Crown-level evaluation")
COUNTS = ("total", "correct", "wrong", "within_site", "cross_site", "within_genus", "cross_genus", "seen")
SCORES = ("micro", "macro", "within_site", "within_genus")
_NO_DEVICE = "deeptreeattention_amd.evaluate runs on a ROCm device (libdta_hip.so, gfx950); the *_np functions are the CPU route"

NovelScores = collections.namedtuple("NovelScores", "label top_score softmax_score")


def _sizes(n_species, groups):
    for name, v in (("n_species", n_species), ("groups", groups)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("{} must be an integer, got {!r}".format(name, v))
    S, G = int(n_species), int(groups)
    if not 1 <= S <= MAX_SPECIES:
        raise ValueError("n_species must be in 1 .. {}, got {}".format(MAX_SPECIES, S))
    if G < 1 or G * S * S > 2 ** 31 - 1:
        raise ValueError("groups must be >= 1 with groups * n_species * n_species <= 2^31 - 1, got {}".format(G))
    return S, G


# ---------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------
def count_np(labels, preds, group=None, mask=None, n_species=None, groups=1):
    """(conf int64 [G][S][S], tally int64 [2]) of the rows given: section 1 of the module's text."""
    S, G = _sizes(n_species, groups)
    t, p = np.asarray(labels).astype(np.int64).reshape(-1), np.asarray(preds).astype(np.int64).reshape(-1)
    g = np.zeros(len(t), np.int64) if group is None else np.asarray(group).astype(np.int64).reshape(-1)
    live = np.ones(len(t), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if not len(t) == len(p) == len(g) == len(live):
        raise ValueError("labels, preds, group and mask must have one entry per row")
    ok = (t >= 0) & (t < S) & (p >= 0) & (p < S) & (g >= 0) & (g < G)
    conf = np.zeros((G, S, S), np.int64)
    take = live & ok
    np.add.at(conf, (g[take], t[take], p[take]), 1)
    return conf, np.array([take.sum(), (live & ~ok).sum()], np.int64)


def _tables(site_masks, genus, S):
    if site_masks is not None:
        site_masks = np.ascontiguousarray(site_masks)
        if site_masks.dtype != np.uint64 or site_masks.ndim != 2 or site_masks.shape[0] != S or \
                not 1 <= site_masks.shape[1] <= MAX_SITE_WORDS:
            raise ValueError("site_masks must be uint64 [{}][W] with 1 <= W <= {}".format(S, MAX_SITE_WORDS))
    if genus is not None:
        genus = np.ascontiguousarray(genus)
        if genus.dtype != np.int32 or genus.shape != (S,):
            raise ValueError("genus must be int32 [{}]".format(S))
    return site_masks, genus


def report_np(conf, site_masks=None, genus=None):
    """dict(counts, scores, accuracy, precision, support) of a table conf [G][S][S] (or [S][S]): section 2 of the module's
    text.  Row G is the pooled row."""
    conf = np.asarray(conf)
    if conf.ndim == 2:
        conf = conf[None]
    if conf.ndim != 3 or conf.shape[1] != conf.shape[2] or conf.dtype.kind not in "iu":
        raise ValueError("a confusion table is an integer [G][S][S] array")
    conf = conf.astype(np.int64)
    G, S = conf.shape[0], conf.shape[1]
    _sizes(S, G)
    site_masks, genus = _tables(site_masks, genus, S)
    off = ~np.eye(S, dtype=bool)
    share = (site_masks[:, None, :] & site_masks[None, :, :]).any(-1) & off if site_masks is not None else None
    same = (genus[:, None] == genus[None, :]) & off if genus is not None else None
    planes = np.concatenate([conf, conf.sum(0, keepdims=True)])
    counts, scores = np.zeros((G + 1, 8), np.int64), np.zeros((G + 1, 4), np.float64)
    accuracy, precision = np.zeros((G + 1, S), np.float64), np.zeros((G + 1, S), np.float64)
    support = np.zeros((G + 1, S), np.int64)

    def quotient(a, b):
        return float(np.float64(int(a)) / np.float64(int(b))) if b > 0 else 0.0

    for r, c in enumerate(planes):
        diag, rows, cols = np.diag(c), c.sum(1), c.sum(0)
        total, correct = int(rows.sum()), int(diag.sum())
        wrong = total - correct
        seen = rows > 0
        ws = int(c[share].sum()) if share is not None else 0
        wg = int(c[same].sum()) if same is not None else 0
        counts[r] = (total, correct, wrong, ws, wrong - ws if share is not None else 0, wg, wrong - wg if same is not None else 0,
                     int(seen.sum()))
        d = diag.astype(np.float64)
        accuracy[r] = np.divide(d, rows.astype(np.float64), out=np.zeros(S), where=rows > 0)
        precision[r] = np.divide(d, cols.astype(np.float64), out=np.zeros(S), where=cols > 0)
        support[r] = rows
        macro = float(np.cumsum(accuracy[r][seen])[-1] / np.float64(int(seen.sum()))) if seen.any() else 0.0
        scores[r] = (quotient(correct, total), macro, quotient(ws, wrong) if share is not None else 0.0,
                     quotient(wg, wrong) if same is not None else 0.0)
    return {"counts": counts, "scores": scores, "accuracy": accuracy, "precision": precision, "support": support}


def first_per_individual_np(ids, n_individuals):
    """bool [N]: the row is the first of its individual code; codes outside [0, n_individuals) give False."""
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    out = np.zeros(len(ids), bool)
    ok = np.flatnonzero((ids >= 0) & (ids < int(n_individuals)))
    _, first = np.unique(ids[ok], return_index=True)
    out[ok[first]] = True
    return out


def novel_scores_np(logits):
    """NovelScores of float [N][C] logits in float64: label = the first class of the largest probability (-1 for a row with
    a NaN), top_score = the largest logit, softmax_score = the largest probability (-1.0 for a row with a NaN)."""
    z = np.asarray(logits, np.float64)
    if z.ndim != 2 or z.shape[1] < 1:
        raise ValueError("logits must be [N][C] with C >= 1")
    bad = np.isnan(z).any(1)
    safe = np.where(bad[:, None], 0.0, z)
    e = np.exp(safe - safe.max(1, keepdims=True))
    pr = e / e.sum(1, keepdims=True)
    label = np.where(bad, -1, pr.argmax(1)).astype(np.int64)
    return NovelScores(label, np.where(bad, np.nan, safe.max(1)), np.where(bad, -1.0, pr.max(1)))


# ---------------------------------------------------------------------------------------------------------------------
# the string work, once, on the host
# ---------------------------------------------------------------------------------------------------------------------
def site_masks(site_lists, n_species):
    """uint64 [S][W] from a mapping label -> iterable of site names or codes (section 3 of the module's text)."""
    S, _ = _sizes(n_species, 1)
    for k in site_lists:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= k < S:
            raise ValueError("site_lists is keyed by the species label 0 .. {}, got {!r}".format(S - 1, k))
    sites = sorted({s for v in site_lists.values() for s in v})
    if len(sites) > 64 * MAX_SITE_WORDS:
        raise ValueError("at most {} sites, got {}".format(64 * MAX_SITE_WORDS, len(sites)))
    bit = {s: b for b, s in enumerate(sites)}
    out = np.zeros((S, max(1, (len(sites) + 63) // 64)), np.uint64)
    for k, v in site_lists.items():
        for s in v:
            out[int(k), bit[s] // 64] |= np.uint64(1) << np.uint64(bit[s] % 64)
    return out


def genus_ids(scientific_dict, n_species):
    """int32 [S] from a mapping label -> scientific name(s), by the reference's `value[0].split()[0]` (section 3)."""
    S, _ = _sizes(n_species, 1)
    for k in scientific_dict:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= k < S:
            raise ValueError("scientific_dict is keyed by the species label 0 .. {}, got {!r}".format(S - 1, k))
    words = {int(k): v[0].split()[0] for k, v in scientific_dict.items()}
    rank = {w: i for i, w in enumerate(sorted(set(words.values())))}
    return np.array([rank[words[k]] if k in words else len(rank) + k for k in range(S)], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
def _device(device):
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(_NO_DEVICE)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _rows(t, name, dtypes, n, dev):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 1 or t.device != dev or (n is not None and t.shape[0] != n):
        raise ValueError("{} must be a {} [{}] tensor on {}".format(
            name, " / ".join(str(d).replace("torch.", "") for d in dtypes), "N" if n is None else n, dev))
    return t.contiguous()


class EvalReport:
    """The outputs of EvalTable.report as device tensors (views of ONE flat buffer): counts, scores and -- per_species --
    accuracy, precision, support.  cpu() waits for the device and returns them as a dict of NumPy arrays, one transfer."""

    def __init__(self, flat, groups, n_species, per_species):
        self.flat, self.groups, self.n_species, self.per_species = flat, groups, n_species, per_species
        for name, view in self._views(flat).items():
            setattr(self, name, view)

    def _layout(self):
        R, S = self.groups + 1, self.n_species
        parts = [("counts", 8, False), ("scores", 4, True)]
        if self.per_species:
            parts += [("accuracy", S, True), ("precision", S, True), ("support", S, False)]
        at = 0
        for name, width, real in parts:
            yield name, at, R, width, real
            at += R * width

    def _views(self, flat):
        import torch
        out = {}
        for name, at, R, width, real in self._layout():
            piece = flat[at:at + R * width]
            if isinstance(flat, np.ndarray):
                out[name] = (piece.view(np.float64) if real else piece).reshape(R, width)
            else:
                out[name] = (piece.view(torch.float64) if real else piece).view(R, width)
        return out

    @staticmethod
    def words(groups, n_species, per_species):
        return (groups + 1) * (12 + (3 * n_species if per_species else 0))

    def cpu(self):
        return self._views(self.flat.cpu().numpy())


class EvalTable:
    """conf int64 [G][S][S] (rows = label, columns = prediction) and tally int64 [2] (rows counted, rows skipped) on the
    device, zero at first; count() accumulates.  1 <= n_species <= 1020, groups >= 1, groups * n_species^2 <= 2^31 - 1 (the
    kernels index an entry with an int)."""

    def __init__(self, n_species, groups=1, device="cuda"):
        import torch
        self.n_species, self.groups = _sizes(n_species, groups)
        self.device = _device(device)
        self.conf = torch.zeros((self.groups, self.n_species, self.n_species), dtype=torch.int64, device=self.device)
        self.tally = torch.zeros(2, dtype=torch.int64, device=self.device)

    def count(self, labels, preds, group=None, mask=None, form=None):
        """Add the rows given (section 1 of the module's text): labels, preds int64 [N], group int32 / int64 [N] (None: group
        0), mask bool / uint8 [N] (None: every row).  One launch on the current stream, nothing waits; returns self."""
        import torch
        from . import _lib
        labels = _rows(labels, "labels", (torch.int64,), None, self.device)
        n = int(labels.shape[0])
        if not 1 <= n < 2 ** 31:
            raise ValueError("1 .. 2^31 - 1 rows, got {}".format(n))
        preds = _rows(preds, "preds", (torch.int64,), n, self.device)
        if group is not None:
            group = _rows(group, "group", (torch.int32, torch.int64), n, self.device)
        if mask is not None:
            mask = _rows(mask, "mask", (torch.bool, torch.uint8), n, self.device).view(torch.uint8)
        form = FORM if form is None else form
        if form not in (PLAIN, COMBINE):
            raise ValueError("form is evaluate.PLAIN or evaluate.COMBINE")
        _lib.check(_lib.lib().dta_eval_count(_lib.ptr(labels), _lib.ptr(preds), _lib.ptr(group),
                                             int(group is not None and group.dtype == torch.int64), _lib.ptr(mask), n,
                                             self.n_species, self.groups, form, _lib.ptr(self.conf), _lib.ptr(self.tally),
                                             _lib.current_stream_ptr()), "dta_eval_count")
        return self

    def report(self, site_masks=None, genus=None, per_species=True):
        """EvalReport of the table as it stands (section 2): one launch, nothing waits.  site_masks uint64 [S][W] (NumPy, or
        an int64 device tensor of the same bits), genus int32 [S]."""
        import torch
        from . import _lib
        S, G = self.n_species, self.groups
        if isinstance(site_masks, torch.Tensor):
            if site_masks.dtype != torch.int64 or site_masks.dim() != 2 or site_masks.shape[0] != S or \
                    not 1 <= site_masks.shape[1] <= MAX_SITE_WORDS or site_masks.device != self.device:
                raise ValueError("site_masks on the device must be int64 [{}][W], 1 <= W <= {}".format(S, MAX_SITE_WORDS))
            site_masks = site_masks.contiguous()
        elif site_masks is not None:
            site_masks = torch.from_numpy(_tables(site_masks, None, S)[0].view(np.int64)).to(self.device)
        if isinstance(genus, torch.Tensor):
            genus = _rows(genus, "genus", (torch.int32,), S, self.device)
        elif genus is not None:
            genus = torch.from_numpy(_tables(None, genus, S)[1]).to(self.device)
        flat = torch.empty(EvalReport.words(G, S, per_species), dtype=torch.int64, device=self.device)
        out = EvalReport(flat, G, S, per_species)
        _lib.check(_lib.lib().dta_eval_report(_lib.ptr(self.conf), S, G, _lib.ptr(site_masks),
                                              int(site_masks.shape[1]) if site_masks is not None else 0, _lib.ptr(genus),
                                              _lib.ptr(out.counts), _lib.ptr(out.scores),
                                              _lib.ptr(out.accuracy) if per_species else None,
                                              _lib.ptr(out.precision) if per_species else None,
                                              _lib.ptr(out.support) if per_species else None, _lib.current_stream_ptr()),
                   "dta_eval_report")
        return out


def first_per_individual(ids, n_individuals):
    """first_per_individual_np on the device: ids int32 / int64 [N] device tensor -> bool [N].  One fill and two launches on
    the current stream, nothing waits."""
    import torch
    from . import _lib
    if not isinstance(ids, torch.Tensor):
        raise ValueError("ids must be a device tensor (first_per_individual_np is the CPU route)")
    dev = _device(ids.device)
    ids = _rows(ids, "ids", (torch.int32, torch.int64), None, dev)
    n = int(ids.shape[0])
    if isinstance(n_individuals, (bool, np.bool_)) or not isinstance(n_individuals, (int, np.integer)) or \
            not 1 <= n_individuals < 2 ** 31:
        raise ValueError("n_individuals must be an integer in 1 .. 2^31 - 1, got {!r}".format(n_individuals))
    if not 1 <= n < 2 ** 31:
        raise ValueError("1 .. 2^31 - 1 rows, got {}".format(n))
    out = torch.empty(n, dtype=torch.bool, device=dev)
    work = torch.empty(int(n_individuals), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dta_first_rows(_lib.ptr(ids), int(ids.dtype == torch.int64), n, int(n_individuals), _lib.ptr(out),
                                             _lib.ptr(work), _lib.current_stream_ptr()), "dta_first_rows")
    return out


def novel_scores(logits):
    """NovelScores(label int64 [N], top_score float32 [N], softmax_score float32 [N]) of float32 [N][C] device logits,
    1 <= C <= 1020 (section 5).  One launch on the current stream, nothing waits."""
    import torch
    from . import _lib
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("logits must be a float32 [N][C] device tensor (novel_scores_np is the CPU route)")
    dev = _device(logits.device)
    n, c = int(logits.shape[0]), int(logits.shape[1])
    if not 1 <= n < 2 ** 31 or not 1 <= c <= MAX_SPECIES:
        raise ValueError("1 .. 2^31 - 1 rows of 1 .. {} classes, got [{}][{}]".format(MAX_SPECIES, n, c))
    logits = logits.contiguous()
    label = torch.empty(n, dtype=torch.int64, device=dev)
    top = torch.empty(n, dtype=torch.float32, device=dev)
    soft = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dta_novel_scores(_lib.ptr(logits), n, c, _lib.ptr(label), _lib.ptr(top), _lib.ptr(soft),
                                               _lib.current_stream_ptr()), "dta_novel_scores")
    return NovelScores(label, top, soft)


def evaluate_crowns(ens_label, labels, site=None, individual=None, n_species=None, n_sites=1, n_individuals=None,
                    site_masks=None, genus=None):
    """The report of evaluation_scores as a host dict.  ens_label, labels: int64 [N]; site: the site code per row (None: one
    site); individual: the individual code per row with n_individuals (None: every row counts) -- only the first row of each
    individual is counted.  Device tensors run one mask, one count and one report on the device and wait for them; NumPy
    arrays run the definitions.  Keys: micro, macro, accuracy [S], precision [S], support [S] (pooled); site_micro [n_sites],
    site_macro [n_sites], site_counts [n_sites][8] (COUNTS); counts [8] (pooled); within_site / within_genus (the shares over
    all errors; present when the table was given)."""
    S, G = _sizes(n_species, n_sites)
    on_host = isinstance(labels, np.ndarray) or not hasattr(labels, "device")
    if individual is not None and n_individuals is None:
        raise ValueError("individual codes need n_individuals")
    if on_host:
        mask = first_per_individual_np(individual, n_individuals) if individual is not None else None
        conf, _ = count_np(labels, ens_label, site, mask, S, G)
        r = report_np(conf, site_masks, genus)
    else:
        mask = first_per_individual(individual, n_individuals) if individual is not None else None
        table = EvalTable(S, G, device=labels.device)
        with __import__("torch").cuda.device(table.device):
            r = table.count(labels, ens_label, group=site, mask=mask).report(site_masks, genus).cpu()
    pooled = r["scores"][G]
    out = {"micro": float(pooled[0]), "macro": float(pooled[1]), "accuracy": r["accuracy"][G].copy(),
           "precision": r["precision"][G].copy(), "support": r["support"][G].copy(), "counts": r["counts"][G].copy(),
           "site_micro": r["scores"][:G, 0].copy(), "site_macro": r["scores"][:G, 1].copy(), "site_counts": r["counts"][:G].copy()}
    if site_masks is not None:
        out["within_site"] = float(pooled[2])
    if genus is not None:
        out["within_genus"] = float(pooled[3])
    return out
