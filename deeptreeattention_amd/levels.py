"""The five level data sets of the reference's `MultiStage.create_datasets` (src/models/multi_stage.py:82-219) and the
`loss_weight_<level>` buffers of its `__init__` (:62-79), from one integer table that is resident on the device.

  * `RecordTable`   the annotation frame as integers: records r in frame order; ind[r] the individual, coded in order of
                    first appearance (a CropPool's row); year[r] the pool's year slot; per individual sp (the species label),
                    rank (the place of its name among all names sorted as Python strings -- pandas' groupby("individual")
                    sorts its keys so), first (its first record), m (its records) and present[i][y].
  * `Rules`         per species a class -- HEAD ("PIPA2"), CONIFER ("PICL", "PIEL", "PITA"), OAK ("QU" in the name), else
                    PLAIN --, the five label maps lmap[l][species] (the reference's level_label_dicts, built from the keys of
                    species_label_dict in the dictionary's own order, OAK last in level 2) and species_order (the rank of
                    the taxon name: pandas' groupby("taxonID") order, which level 3 is left in).
  * the rule        pos(i) = the individuals of i's species with a smaller rank.  "By first" = ascending first[i].
        train  L0   every HEAD individual, and a non-HEAD one when pos < other_sampling_ceiling; the HEAD individuals by
                    first, then the others by first; labels 0 / 1.
               L1   non-HEAD: every CONIFER individual, any other when pos < k1 = ceil(CONIFER records / 11); by first;
                    labels 0 (CONIFER) / 1.  (The reference's shuffle there only picks the row that stands for an
                    individual: no effect.)
               L2   neither HEAD nor CONIFER: every non-OAK individual; per OAK species the records in shuffled order, the
                    first k2 = (non-OAK records) // 5 of them name the kept individuals (one named twice is kept once, with
                    all its records); by first.  The shuffle: record r draws key_r = draw32 at the counter epoch * R + r
                    of stream 2 (_hash.py: the counter hash and the streams in use) and a species' records sort ascending
                    by (key_r, r) -- or `orders` hands in explicit orders (the fixture: the reference's own
                    `sample(frac=1)` results).
               L3   CONIFER: per species the first evergreen_ceiling RECORDS in frame order; an individual is kept when a
                    record of it is, with year_keep[i][y] = 1 only where a kept record of (i, y) exists; species ascending by
                    species_order, within a species by the first kept record.
               L4   OAK: pos < oaks_sampling_ceiling; by first.
        test        the populations alone (all / non-HEAD / neither HEAD nor CONIFER / CONIFER / OAK), every level by first.
        weights     (train) num_classes[l] = the level labels present among the kept records; cnt[x] = kept RECORDS of label
                    x; w = 1.0 / cnt in float64, w /= max(w), w[w < min_loss_weight] = min_loss_weight, rounded to float32.
                    Labels that are not exactly 0 .. num_classes - 1, or an empty level: ValueError.
  * `build_np`      the definition.  `build` is the same on the device (dta_level_build: at most four launches on the
                    caller's stream, integer work and a float64 division per class) and equals it bit for bit; the host
                    names every individual from build_np and reads nothing back.  A pure function of (seed, epoch): level
                    2's balanced subsample can be drawn again every epoch.
  * `create_datasets`  two frames and their pools in; (train LevelViews, test LevelViews, Hierarchy, num_classes,
                    loss weights) out: what MultiStageTrainer and loop.fit_multistage take.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._hash import M64 as _M64, draw32, host as _host, shuffle_base
from .hierarchy import Hierarchy
from .split import _codes
from .treedata import LevelViews, PoolView

LEVELS = _lib.LEVEL_COUNT
STREAM = _lib.LEVEL_STREAM
HEAD, CONIFER, OAK, PLAIN = _lib.LEVEL_HEAD, _lib.LEVEL_CONIFER, _lib.LEVEL_OAK, _lib.LEVEL_PLAIN
MAX_N = _lib.EPOCH_ORDER_MAX_N
MAX_SPECIES = _lib.LEVEL_MAX_SPECIES
CONFIG_KEYS = ("other_sampling_ceiling", "evergreen_ceiling", "oaks_sampling_ceiling", "min_loss_weight")


def _column(columns, name, required=True):
    if name not in columns:
        if required:
            raise ValueError("the frame needs the column {!r}".format(name))
        return None
    c = columns[name]
    return c.to_numpy() if hasattr(c, "to_numpy") else np.asarray(_host(c))


def _name_rank(names):
    """rank[i]: the place of names[i] among the names sorted as pandas' groupby sorts its keys (strings as Python strings)."""
    v = np.asarray(names)
    if v.dtype.kind not in "iuf":
        v = v.astype(str)
    rank = np.empty(len(v), np.int32)
    rank[np.argsort(v, kind="stable")] = np.arange(len(v), dtype=np.int32)
    return rank


def _place(group, *keys):
    """For every element, how many elements of its group come before it under the keys (most significant first)."""
    order = np.lexsort(tuple(reversed(keys)) + (group,))
    g = np.asarray(group)[order]
    start = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if len(g) else np.zeros(0, np.int64)
    run = np.cumsum(np.r_[True, g[1:] != g[:-1]]) - 1 if len(g) else np.zeros(0, np.int64)
    place = np.empty(len(g), np.int64)
    place[order] = np.arange(len(g)) - start[run]
    return place


def species_label_dict(columns):
    """{taxonID: label} as the reference's __init__ builds it (:42): the taxa in order of first appearance."""
    taxon, label = _column(columns, "taxonID"), _column(columns, "label")
    out = {}
    for t, l in zip(taxon.tolist(), label.tolist()):
        t = t.decode() if isinstance(t, bytes) else str(t)
        if out.setdefault(t, int(l)) != int(l):
            raise ValueError("taxon {!r} has the labels {} and {}".format(t, out[t], int(l)))
    return out


class RecordTable:
    """An annotation frame as the integer tables the rule needs (module docstring); `resident(device)` uploads them once."""

    def __init__(self, ind, year, sp, n_years, individuals=None, years=None, taxa=None):
        self.ind = np.ascontiguousarray(ind, np.int32).reshape(-1)
        self.year = np.ascontiguousarray(year, np.int32).reshape(-1)
        self.sp = np.ascontiguousarray(sp, np.int32).reshape(-1)
        self.R, self.N, self.Y = len(self.ind), len(self.sp), int(n_years)
        if self.R < 1 or len(self.year) != self.R:
            raise ValueError("at least one record, and one year per record")
        if not 1 <= self.Y <= _lib.MAX_YEARS:
            raise ValueError("1..{} years, got {}".format(_lib.MAX_YEARS, self.Y))
        if self.N > MAX_N or self.R > self.N * _lib.MAX_YEARS:
            raise ValueError("at most {} individuals and {} records each, got {} and {} records".format(
                MAX_N, _lib.MAX_YEARS, self.N, self.R))
        if self.year.min() < 0 or self.year.max() >= self.Y or self.sp.min() < 0:
            raise ValueError("year slots must be 0..{} and species labels at least 0".format(self.Y - 1))
        first = np.full(self.N, self.R, np.int64)
        np.minimum.at(first, self.ind, np.arange(self.R))
        if self.ind.min() < 0 or self.ind.max() >= self.N or (first == self.R).any() or (np.diff(first) <= 0).any():
            raise ValueError("individuals must be coded 0..N-1 in order of first appearance")
        self.first = first.astype(np.int32)
        self.m = np.bincount(self.ind, minlength=self.N).astype(np.int32)
        self.individuals = list(range(self.N)) if individuals is None else list(individuals)
        if len(self.individuals) != self.N:
            raise ValueError("one name per individual ({}), got {}".format(self.N, len(self.individuals)))
        self.rank = _name_rank(self.individuals)
        self.present = np.zeros((self.N, self.Y), np.uint8)
        self.present[self.ind, self.year] = 1
        self.years = list(range(self.Y)) if years is None else list(years)
        self.taxa = taxa
        self._resident = {}

    @classmethod
    def from_frame(cls, df, pool=None):
        """df: a pandas frame (or a mapping of columns) with individual, tile_year, taxonID and label, one entry per record.
        With a pool, the individuals must be the pool's, in its order, and the years the pool's."""
        ind, year = _column(df, "individual"), _column(df, "tile_year")
        taxon, label = _column(df, "taxonID"), _column(df, "label")
        if not len(ind) or any(len(c) != len(ind) for c in (year, taxon, label)):
            raise ValueError("individual, tile_year, taxonID and label must have one entry per record, and at least one")
        icode, inames = _codes(ind)
        tcode, tnames = _codes(taxon)
        label = np.asarray(label)
        if label.dtype.kind not in "iu":
            raise ValueError("label must be an integer column, got {}".format(label.dtype))
        first = np.full(len(inames), len(icode), np.int64)
        np.minimum.at(first, icode, np.arange(len(icode)))
        bad = np.flatnonzero((tcode != tcode[first[icode]]) | (label != label[first[icode]]))
        if len(bad):
            raise ValueError("the records of individual {!r} disagree on taxonID or label (record {})".format(
                inames[icode[bad[0]]], int(bad[0])))
        if pool is not None:
            if [str(v) for v in pool.individuals] != [str(v) for v in inames.tolist()]:
                raise ValueError("the frame's individuals are not the pool's, in its order")
            slot = {str(v): k for k, v in enumerate(pool.years)}
            names = np.asarray(year).astype(str) if np.asarray(year).dtype == object else np.asarray(year)
            try:
                ycode = np.array([slot[str(v)] for v in names.tolist()], np.int64)
            except KeyError as e:
                raise ValueError("the pool has no year {}".format(e))
            n_years, years = pool.n_years, list(pool.years)
        else:
            ycode, ynames = _codes(year)
            n_years, years = len(ynames), ynames.tolist()
        return cls(icode, ycode, label[first], n_years, inames.tolist(), years, [str(v) for v in tnames[tcode[first]].tolist()])

    def resident(self, device):
        dev = torch.device(device)
        if dev not in self._resident:
            self._resident[dev] = {k: torch.from_numpy(getattr(self, k)).to(dev)
                                   for k in ("ind", "year", "sp", "rank", "first", "m", "present")}
        return self._resident[dev]


class Rules:
    """The species classes, the five label maps and the taxon order (module docstring)."""

    def __init__(self, cls, lmap, species_order, level_label_dicts=None, species_label_dict=None):
        self.cls = np.ascontiguousarray(cls, np.int32).reshape(-1)
        self.C = len(self.cls)
        self.lmap = np.ascontiguousarray(lmap, np.int32)
        self.species_order = np.ascontiguousarray(species_order, np.int32).reshape(-1)
        if not 1 <= self.C <= MAX_SPECIES:
            raise ValueError("1..{} species, got {}".format(MAX_SPECIES, self.C))
        if self.lmap.shape != (LEVELS, self.C) or len(self.species_order) != self.C:
            raise ValueError("lmap must be [{}][{}] and species_order [{}]".format(LEVELS, self.C, self.C))
        if self.cls.min() < HEAD or self.cls.max() > PLAIN or self.lmap.min() < -1 or self.lmap.max() > self.C:
            raise ValueError("classes must be 0..3 and level labels -1..{}".format(self.C))
        self.level_label_dicts, self.species_label_dict = level_label_dicts, species_label_dict
        self._resident = {}

    @classmethod
    def reference(cls, species_label_dict, head="PIPA2", conifers=("PICL", "PIEL", "PITA"), oak="QU"):
        """The reference's hard-coded rules over its species_label_dict ({taxonID: label}, labels 0..C-1).  The lists of
        levels 2, 3 and 4 enumerate the dictionary's keys in the dictionary's own order, as create_datasets does."""
        names = [str(k) for k in species_label_dict]
        labels = [int(v) for v in species_label_dict.values()]
        n = len(names)
        if sorted(labels) != list(range(n)) or len(set(names)) != n:
            raise ValueError("species labels must be 0..{} without gaps or repeats".format(n - 1))
        conifers = tuple(conifers)
        kinds = []
        for t in names:
            k = [c for c, hit in ((HEAD, t == head), (CONIFER, t in conifers), (OAK, oak in t)) if hit]
            if len(k) > 1:
                raise ValueError("taxon {!r} falls into more than one class: the classes overlap".format(t))
            kinds.append(k[0] if k else PLAIN)
        broadleaf = {t: k for k, t in enumerate(t for t, c in zip(names, kinds) if c == PLAIN)}
        broadleaf["OAK"] = len(broadleaf)
        dicts = [{head: 0, "OTHER": 1}, {"CONIFER": 0, "BROADLEAF": 1}, broadleaf,
                 {t: k for k, t in enumerate(t for t, c in zip(names, kinds) if c == CONIFER)},
                 {t: k for k, t in enumerate(t for t, c in zip(names, kinds) if c == OAK)}]
        kind = np.zeros(n, np.int32)
        lmap = np.full((LEVELS, n), -1, np.int32)
        order = np.zeros(n, np.int32)
        by_name = {t: k for k, t in enumerate(sorted(names))}
        for t, s, c in zip(names, labels, kinds):
            kind[s], order[s] = c, by_name[t]
            lmap[0, s] = 0 if c == HEAD else 1
            if c != HEAD:
                lmap[1, s] = 0 if c == CONIFER else 1
            if c == PLAIN:
                lmap[2, s] = broadleaf[t]
            elif c == OAK:
                lmap[2, s], lmap[4, s] = broadleaf["OAK"], dicts[4][t]
            elif c == CONIFER:
                lmap[3, s] = dicts[3][t]
        return cls(kind, lmap, order, dicts, dict(zip(names, labels)))

    def resident(self, device):
        dev = torch.device(device)
        if dev not in self._resident:
            self._resident[dev] = {"cls": torch.from_numpy(self.cls).to(dev), "lmap": torch.from_numpy(self.lmap).to(dev),
                                   "species_order": torch.from_numpy(self.species_order).to(dev)}
        return self._resident[dev]


class Levels:
    """The five data sets of one frame.  Per level l: rows[l] (int64 pool rows in data set order), labels[l] (int64),
    year_keep[l] (uint8 [n][Y]), n[l]; with train also num_classes[l] and loss_weight[l] (float32 [num_classes[l]]).
    From build_np these are NumPy arrays; from build, resident tensors (n_dev and num_classes_dev: int32 [5] on the device)
    and `host` is build_np's result, which n, num_classes and the names come from."""

    def __init__(self, table, rows, labels, year_keep, n, num_classes=None, loss_weight=None, train=True, host=None):
        self.table, self.rows, self.labels, self.year_keep, self.n = table, rows, labels, year_keep, [int(v) for v in n]
        self.num_classes, self.loss_weight, self.train, self.host = num_classes, loss_weight, bool(train), host
        self.n_dev = self.num_classes_dev = None

    def individuals(self, level):
        rows = (self.host or self).rows[level]
        return [self.table.individuals[i] for i in rows]


def _config(config):
    missing = [k for k in CONFIG_KEYS if k not in config]
    if missing:
        raise ValueError("config lacks {}".format(", ".join(missing)))
    ceil = [int(config[k]) for k in CONFIG_KEYS[:3]]
    floor = float(config["min_loss_weight"])
    if min(ceil) < 0 or not 0.0 <= floor <= 1.0:
        raise ValueError("the ceilings must be at least 0 and min_loss_weight 0..1, got {} and {}".format(ceil, floor))
    return ceil[0], ceil[1], ceil[2], floor


def record_keys_np(table, rules, orders):
    """orders: {species label: the records of that OAK species, in shuffled order}.  Returns int32 [R]: the place of every
    record in its species' order (0 for the records of other species), which stands in for the hashed key."""
    key = np.zeros(table.R, np.int32)
    rsp = table.sp[table.ind]
    given = {int(k): np.asarray(_host(v), np.int64).reshape(-1) for k, v in dict(orders).items()}
    for s in np.unique(rsp[rules.cls[rsp] == OAK]).tolist():
        want = np.flatnonzero(rsp == s)
        o = given.get(s)
        if o is None or len(o) != len(want) or not np.array_equal(np.sort(o), want):
            raise ValueError("orders must hold every record of OAK species {} exactly once".format(s))
        key[o] = np.arange(len(o), dtype=np.int32)
    return key


def hashed_keys_np(n_records, epoch=0, seed=0):
    """key_r, uint64 [R]: _hash.py's draw32 of the R records in stream STREAM, starting at the counter epoch * R."""
    return draw32(seed, STREAM, shuffle_base(epoch, n_records), n_records)


def _check(table, rules):
    if not isinstance(table, RecordTable) or not isinstance(rules, Rules):
        raise ValueError("table must be a RecordTable and rules a Rules")
    if int(table.sp.max()) >= rules.C:
        raise ValueError("species label {} is not one of the rules' {} species".format(int(table.sp.max()), rules.C))


def build_np(table, rules, config, train=True, seed=0, epoch=0, orders=None):
    """The definition (module docstring): a Levels of NumPy arrays."""
    _check(table, rules)
    other_c, evergreen_c, oaks_c, floor = _config(config)
    t, N, R = table, table.N, table.R
    kind = rules.cls[t.sp]
    rsp = t.sp[t.ind]
    rkind = kind[t.ind]
    first = t.first.astype(np.int64)
    zero = np.zeros(N, np.int64)
    keep_years, records = [t.present] * LEVELS, [t.m.astype(np.int64)] * LEVELS
    if not train:
        masks = [np.ones(N, bool), kind != HEAD, (kind == OAK) | (kind == PLAIN), kind == CONIFER, kind == OAK]
        keys = [(first,)] * LEVELS
    else:
        pos = _place(t.sp, t.rank)
        k1 = -(-int(t.m[kind == CONIFER].sum()) // 11)
        k2 = int(t.m[kind == PLAIN].sum()) // 5
        # level 2: the first k2 records of every OAK species' shuffle
        draw = record_keys_np(t, rules, orders).astype(np.int64) if orders is not None else hashed_keys_np(R, epoch, seed).astype(np.int64)
        oak = np.flatnonzero(rkind == OAK)
        keep2 = np.zeros(N, bool)
        keep2[t.ind[oak[_place(rsp[oak], draw[oak], oak) < k2]]] = True
        # level 3: the first evergreen_ceiling records of every CONIFER species, in frame order
        con = np.flatnonzero(rkind == CONIFER)
        kept = con[_place(rsp[con], con) < evergreen_c]
        m3 = np.bincount(t.ind[kept], minlength=N).astype(np.int64)
        yk3 = np.zeros((N, t.Y), np.uint8)
        yk3[t.ind[kept], t.year[kept]] = 1
        first3 = np.full(N, R, np.int64)
        np.minimum.at(first3, t.ind[kept], kept)
        masks = [(kind == HEAD) | (pos < other_c),
                 (kind == CONIFER) | ((kind != HEAD) & (pos < k1)),
                 (kind == PLAIN) | keep2,
                 m3 > 0,
                 (kind == OAK) & (pos < oaks_c)]
        keys = [((kind != HEAD).astype(np.int64), first), (first,), (first,), (rules.species_order[t.sp].astype(np.int64), first3),
                (first,)]
        keep_years = keep_years[:3] + [yk3] + keep_years[4:]
        records = records[:3] + [m3] + records[4:]
    rows, labels, year_keep, n, classes, weights = [], [], [], [], [], []
    for l in range(LEVELS):
        at = np.flatnonzero(masks[l])
        at = at[np.lexsort(tuple(k[at] for k in reversed(keys[l])))] if len(at) else at
        if not len(at):
            raise ValueError("level {} is empty".format(l))
        lab = rules.lmap[l][t.sp[at]].astype(np.int64)
        rows.append(at.astype(np.int64))
        labels.append(lab)
        year_keep.append(np.ascontiguousarray(keep_years[l][at]))
        n.append(len(at))
        if train:
            cnt = np.zeros(rules.C + 1, np.int64)
            np.add.at(cnt, lab, records[l][at])
            nc = int(np.count_nonzero(cnt))
            gone = np.flatnonzero(cnt[:nc] == 0)
            if len(gone):
                raise ValueError("level {}: label {} has no record among the kept ones (the labels present must be 0..{})".format(
                    l, int(gone[0]), nc - 1))
            w = 1.0 / cnt[:nc].astype(np.float64)
            w = w / np.max(w)
            w[w < floor] = floor
            classes.append(nc)
            weights.append(w.astype(np.float32))
    return Levels(table, rows, labels, year_keep, n, classes if train else None, weights if train else None, train)


def _launch(tab, rul, record_key, cfg, train, seed, epoch, out, workspace, N, R, C_, Y):
    """dta_level_build on the current stream: resident tables in, resident outputs written.  No allocation, no read-back."""
    t = _lib.LevelTables(N, R, C_, Y, *[tab[k].data_ptr() for k in ("ind", "year", "sp", "rank", "first", "m", "present")],
                         rul["cls"].data_ptr(), rul["lmap"].data_ptr(), rul["species_order"].data_ptr(),
                         None if record_key is None else record_key.data_ptr())
    c = _lib.LevelConfig(int(bool(train)), cfg[0], cfg[1], cfg[2], cfg[3], int(seed) & _M64, int(epoch) & _M64)
    _lib.check(_lib.lib().dta_level_build(C.byref(t), C.byref(c), C.byref(out), workspace.data_ptr(), workspace.numel(),
                                          _lib.current_stream_ptr()), "dta_level_build")


def _outputs(host, C_, Y, device, train):
    """Fresh resident outputs of the sizes the definition names, and the dta_level_out that points at them."""
    rows = [torch.empty(n, dtype=torch.int64, device=device) for n in host.n]
    labels = [torch.empty(n, dtype=torch.int64, device=device) for n in host.n]
    keep = [torch.empty(n, Y, dtype=torch.uint8, device=device) for n in host.n]
    counts = torch.empty(2, LEVELS, dtype=torch.int32, device=device)
    weight = torch.empty(LEVELS, C_ + 1, dtype=torch.float32, device=device) if train else None
    return rows, labels, keep, counts, weight


def _out_struct(rows, labels, keep, counts, weight):
    o = _lib.LevelOut()
    for l in range(LEVELS):
        o.rows[l], o.labels[l], o.year_keep[l], o.capacity[l] = rows[l].data_ptr(), labels[l].data_ptr(), keep[l].data_ptr(), len(rows[l])
    o.n, o.num_classes = counts[0].data_ptr(), counts[1].data_ptr()
    o.loss_weight = None if weight is None else weight.data_ptr()
    return o


def build(table, rules, config, train=True, seed=0, epoch=0, orders=None, device="cuda", into=None):
    """build_np on the device: a Levels of resident tensors, equal to build_np's bit for bit (which is its `host`).  into: a
    Levels of an earlier build of the same sizes whose tensors are written again (a new epoch without an allocation)."""
    host = build_np(table, rules, config, train, seed, epoch, orders)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("levels.build runs on a ROCm device only (build_np is the host definition), got {}".format(device))
    cfg = _config(config)
    N, R, C_, Y = table.N, table.R, rules.C, table.Y
    need = int(_lib.lib().dta_level_workspace_bytes(N, R, C_, Y))
    if need == 0:
        raise ValueError("sizes out of range: {} individuals, {} records, {} species, {} years".format(N, R, C_, Y))
    record_key = None if orders is None or not train else torch.from_numpy(record_keys_np(table, rules, orders)).to(dev)
    if into is not None:
        if into.host is None or into.n != host.n or into.train != bool(train) or into._buffers[0][0].device != dev:
            raise ValueError("`into` must come from a build of the same sizes, mode and device")
        rows, labels, keep, counts, weight = into._buffers
    else:
        rows, labels, keep, counts, weight = _outputs(host, C_, Y, dev, train)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    _launch(table.resident(dev), rules.resident(dev), record_key, cfg, train, seed, epoch,
            _out_struct(rows, labels, keep, counts, weight), workspace, N, R, C_, Y)
    out = Levels(table, rows, labels, keep, host.n, host.num_classes,
                 [weight[l, :host.num_classes[l]] for l in range(LEVELS)] if train else None, train, host)
    out.n_dev, out.num_classes_dev = counts[0], counts[1]
    out._buffers = (rows, labels, keep, counts, weight)
    return out


def views(levels, pool, train=None):
    """The LevelViews of a device-built Levels over `pool`: the resident rows, labels and year masks as they are."""
    if levels.host is None:
        raise ValueError("views takes the Levels of levels.build")
    if pool.n != levels.table.N or pool.n_years != levels.table.Y:
        raise ValueError("the pool has {} rows and {} years, the table {} and {}".format(pool.n, pool.n_years, levels.table.N,
                                                                                      levels.table.Y))
    if levels.rows[0].device != pool.device:
        raise ValueError("the levels are on {}, the pool on {}".format(levels.rows[0].device, pool.device))
    out = []
    for l in range(LEVELS):
        v = object.__new__(PoolView)
        v.pool, v.rows_np, v.train, v.level = pool, levels.host.rows[l], None if train is None else bool(train), l
        v.rows, v.labels = levels.rows[l], levels.labels[l]
        v.year_keep_np, v.year_keep = levels.host.year_keep[l], levels.year_keep[l]
        out.append(v)
    return LevelViews(out)


def create_datasets(train_df, test_df, train_pool, test_pool, config, seed=0, epoch=0):
    """The reference's MultiStage.create_datasets and the loss weights of its __init__ over two resident pools: returns
    (train LevelViews, test LevelViews, Hierarchy, num_classes, loss_weights) -- num_classes a list of five ints,
    loss_weights five resident float32 tensors.  The train views flip (TreeDataset(train=True)); so do the reference's
    test data sets, which it builds with the same default."""
    names = species_label_dict(train_df)
    rules = Rules.reference(names)
    train_table = RecordTable.from_frame(train_df, train_pool)
    test_table = RecordTable.from_frame(test_df, test_pool)
    train_levels = build(train_table, rules, config, True, seed, epoch, device=train_pool.device)
    test_levels = build(test_table, rules, config, False, seed, epoch, device=test_pool.device)
    hierarchy = Hierarchy.from_reference(rules.level_label_dicts, rules.species_label_dict)
    return (views(train_levels, train_pool, True), views(test_levels, test_pool, True), hierarchy,
            list(train_levels.num_classes), list(train_levels.loss_weight))
