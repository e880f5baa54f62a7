"""The hierarchy of a multi-stage model as data, and what the reference does with it after prediction.

Reference src/models/multi_stage.py:368-402 (`gather_predictions`: per-level top-1 label and score of every crown),
:404-434 (`ensemble`: ONE species label and score per crown, by a hard-coded walk over the five levels) and :436-485
(`evaluation_scores`: per-species accuracy / precision, micro and macro accuracy).  Here the walk is a table: for every
level `l` and class `c` of that level, `next_level[l][c]` is the level to consult next or -1 (terminal), and
`species[l][c]` the final species label when terminal.  The walk starts at level 0 and, since an edge always leads to a
LATER level, ends in at most `levels` steps.

    resolve_np      the host definition (plain NumPy): what CPU-only users get and what the device kernels
                    (dta_hierarchy_resolve, dta_multistage_predict_ensemble) are tested against
    device_table    the table as one int32 tensor for those kernels
    scores_from_confusion   evaluation_scores' figures from a confusion matrix (rows = label, columns = prediction)
"""
import numpy as np

MAX_LEVELS = 8      # DTA_MAX_LEVELS (include/dta_hip.h)


class Hierarchy:
    def __init__(self, next_level, species, n_species):
        nl = len(next_level)
        if not 1 <= nl <= MAX_LEVELS:
            raise ValueError("a hierarchy has 1..{} levels, not {}".format(MAX_LEVELS, nl))
        if len(species) != nl:
            raise ValueError("next_level and species must describe the same levels")
        self.n_species = int(n_species)
        if self.n_species < 1:
            raise ValueError("n_species must be positive")
        self.next_level, self.species = [], []
        for l, (nx, sp) in enumerate(zip(next_level, species)):
            nx = [int(v) for v in nx]
            sp = [int(v) for v in sp]
            if len(nx) != len(sp) or not nx:
                raise ValueError("level {}: next_level and species need one entry per class (at least one)".format(l))
            for c, (n, s) in enumerate(zip(nx, sp)):
                if n == -1:
                    if not 0 <= s < self.n_species:
                        raise ValueError("level {} class {}: a terminal class needs a species label in [0, {}), not {}"
                                         .format(l, c, self.n_species, s))
                elif not l < n < nl:
                    raise ValueError("level {} class {}: the next level must be a later one (in ({}, {})) or -1, not {}"
                                     .format(l, c, l, nl, n))
            self.next_level.append(np.asarray(nx, np.int32))
            self.species.append(np.asarray([s if n == -1 else -1 for n, s in zip(nx, sp)], np.int32))
        self.levels = nl
        self.classes = [len(n) for n in self.next_level]
        self._tables = {}

    @classmethod
    def from_reference(cls, level_label_dicts, species_label_dict):
        """Exactly the rules hard-coded in the reference's `MultiStage.ensemble` (multi_stage.py:404-434), from its own
        dictionaries ({taxonID: label} per level, as `MultiStage.level_label_dicts` keeps them, and `species_label_dict`):
        level 0 PIPA2 -> terminal, anything else -> level 1; level 1 BROADLEAF -> level 2, anything else -> level 3;
        level 2 OAK -> level 4, anything else terminal; levels 3 and 4 terminal.  A terminal class whose taxon is not a
        species of `species_label_dict` is a KeyError here (the reference raises it per row)."""
        if len(level_label_dicts) != 5:
            raise ValueError("the reference's hierarchy has five levels, not {}".format(len(level_label_dicts)))
        rule = [lambda t: -1 if t == "PIPA2" else 1,
                lambda t: 2 if t == "BROADLEAF" else 3,
                lambda t: 4 if t == "OAK" else -1,
                lambda t: -1,
                lambda t: -1]
        next_level, species = [], []
        for l, d in enumerate(level_label_dicts):
            by_label = {int(v): k for k, v in d.items()}
            if sorted(by_label) != list(range(len(d))):
                raise ValueError("level {}: labels must be 0..{} without gaps or repeats".format(l, len(d) - 1))
            nx = [rule[l](by_label[c]) for c in range(len(d))]
            next_level.append(nx)
            species.append([int(species_label_dict[by_label[c]]) if n == -1 else -1 for c, n in enumerate(nx)])
        return cls(next_level, species, len(species_label_dict))

    def resolve_np(self, top1_labels, top1_scores):
        """The walk in plain NumPy.  top1_labels / top1_scores: [levels][B] (each level's top-1 class and its
        probability).  Returns (ens_label int64 [B], ens_score float32 [B], ens_level int32 [B]): the species, the top-1
        probability of the level the walk ended on (a selection: the same bits) and that level.  A class outside its
        level's range (no class at all: the top-1 of a row of NaN is -1) ends the walk there with label -1."""
        lab = [np.asarray(t).astype(np.int64).reshape(-1) for t in top1_labels]
        sc = [np.asarray(t, np.float32).reshape(-1) for t in top1_scores]
        if len(lab) != self.levels or len(sc) != self.levels:
            raise ValueError("resolve_np needs one label and one score array per level ({})".format(self.levels))
        B = lab[0].shape[0]
        cur = np.zeros(B, np.int64)
        ens_label = np.full(B, -1, np.int64)
        ens_score = np.zeros(B, np.float32)
        ens_level = np.full(B, -1, np.int32)
        for l in range(self.levels):
            here = np.nonzero(cur == l)[0]
            if here.size == 0:
                continue
            c = lab[l][here]
            ok = (c >= 0) & (c < self.classes[l])
            cc = np.where(ok, c, 0)
            nx = np.where(ok, self.next_level[l][cc], -1)
            end = nx < 0
            rows = here[end]
            ens_label[rows] = np.where(ok[end], self.species[l][cc[end]], -1)
            ens_score[rows] = sc[l][rows]
            ens_level[rows] = l
            cur[here] = np.where(end, -1, nx)
        return ens_label, ens_score, ens_level

    def table_np(self):
        """int32: the levels' offsets into the two arrays that follow (levels + 1 entries), `next`, `species`."""
        off = np.concatenate([[0], np.cumsum(self.classes)]).astype(np.int32)
        return np.concatenate([off, np.concatenate(self.next_level), np.concatenate(self.species)]).astype(np.int32)

    def device_table(self, device):
        """The table on `device`, uploaded once per device and kept."""
        import torch
        key = str(torch.device(device))
        t = self._tables.get(key)
        if t is None:
            t = torch.from_numpy(self.table_np()).to(device)
            self._tables[key] = t
        return t

    def c_table(self, device):
        """The `dta_hierarchy` argument of dta_multistage_predict_ensemble / dta_hierarchy_resolve for `device`."""
        from . import _lib
        t = self.device_table(device)
        return _lib.HierarchyTable(self.levels, self.n_species, (_lib.C.c_int * _lib.MAX_LEVELS)(*self.classes), t.data_ptr())


def scores_from_confusion(conf):
    """The figures `MultiStage.evaluation_scores` (multi_stage.py:436-485) and `validation_epoch_end` report, from a
    confusion matrix (rows = label, columns = prediction): per-species accuracy (diagonal / row sum) and precision
    (diagonal / column sum), micro accuracy (trace / total) and macro accuracy (mean of the per-species accuracies).
    Stated convention, not reference parity: a zero denominator gives 0.0, and a species without samples is left out of
    the macro mean."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("a confusion matrix is square")
    c = conf.astype(np.float64)
    diag, rows, cols = np.diag(c), c.sum(1), c.sum(0)
    acc = np.divide(diag, rows, out=np.zeros_like(diag), where=rows > 0)
    prec = np.divide(diag, cols, out=np.zeros_like(diag), where=cols > 0)
    total = c.sum()
    seen = rows > 0
    return {"accuracy": acc, "precision": prec,
            "micro": float(diag.sum() / total) if total > 0 else 0.0,
            "macro": float(acc[seen].mean()) if seen.any() else 0.0}
