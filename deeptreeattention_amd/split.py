"""Train/test plot split search: the reference's `train_test_split` (src/data.py:165-236), which runs `sample_plots`
(:108-162) config["iterations"] times -- one dask future each -- and keeps the split with the most test species.

One iteration shuffles the candidate plots, moves whole plots into the test set until every species has more than
max(0.05 * n, min_test) test individuals, and then applies the minimum-sample and common-species filters.  All of it
depends on three integer tables over P plots x S species only (a ROW of the annotation table is individual x year; an
individual has one plot and one taxon):
    A[p][s]  individuals                                  (the reference's `single_year`: one row per individual)
    B[p][s]  individuals with at least one row that is not fixed  (they survive "remove fixed boxes from test",
             whichever of their rows comes first)
    R[p][s]  rows
    totA = A.sum(0), totR = R.sum(0) over ALL plots;  floor[s] = max(float64(totA[s]) * 0.05, float64(min_test))
Given an order of the C candidate plots:
    cnt = 0; to_sample[s] = True; inc[p] = False
    for p in order:
        if any(A[p][s] > 0 and to_sample[s]):
            inc[p] = True; cnt += A[p]; to_sample = ~(float64(cnt) > floor)            strict, as the reference
    testcnt = sum of B over inc;  traincnt = totA - sum of A over inc;  trainrows = totR - sum of R over inc
    T = (testcnt >= min_test) & (traincnt >= min_train)        both .filter() calls and both isin() lines
    species = popcount(T);  train_rows = sum(trainrows[T]);  test_plots = popcount(inc)
The best iteration is the lexicographic maximum of (species, train_rows), the earliest on a full tie (the reference's
`>` / `==` / np.argmax over the ties).  Test rows: plot in inc, not fixed, taxon in T; train rows: plot not in inc, taxon
in T.  min_train and min_test are at least 1: with 0 the reference drops a species that has no row on one side through
its isin() lines, which T would keep.

The reference shuffles with NumPy's global generator; a device cannot follow that stream, so the order is this package's
(_hash.py's counter hash and shuffle): candidate j of iteration t draws  draw32  at the counter t * C + j of stream 0 and
the candidates are sorted ascending by (draw, j).  An explicit `orders` array replaces the hash in the definition and on the
device alike; with the reference's own shuffles it reproduces the reference exactly
(tests/golden/split/split_reference.npz).

The NumPy functions are the definition; SplitTable.search (k_split_search, csrc/split.hip: a wavefront per iteration,
every iteration in one launch) equals search_np bit for bit -- integers and one float64 comparison.
"""
import collections

import numpy as np

from ._hash import M64 as _M64, STREAM_SPLIT, draw32, host as _host, order_of, shuffle_base

MAX_SPECIES = 256          # DTA_SPLIT_MAX_SPECIES
MAX_CANDIDATES = 4096      # DTA_SPLIT_MAX_CANDIDATES
_CHUNK = 4096              # iterations search_np scans at a time

SplitSearch = collections.namedtuple("SplitSearch", "species train_rows test_plots best membership taxa")
SplitSearch.__doc__ = """species int32 / train_rows int64 / test_plots int32 [iterations]; best = (iteration, species,
train_rows, test_plots) of the best iteration, `iteration` counted from the call's first (first_iteration + iteration is
its absolute number; -1 when iterations == 0): four ints from search_np, an int64 [4] device tensor from
SplitTable.search; membership uint8 [iterations][C] (candidate j is a test plot) and taxa uint8 [iterations][S] (T), or
None where not asked for."""
Split = collections.namedtuple("Split", "train test iteration species test_plots")


def _codes(values):
    """Integer codes in the order of first appearance (pandas' .unique() order) and the labels in that order."""
    v = np.asarray(_host(values)).reshape(-1)
    if v.dtype == object:
        v = v.astype(str)
    labels, first, inverse = np.unique(v, return_index=True, return_inverse=True)
    rank = np.empty(len(labels), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(labels))
    return rank[inverse.reshape(-1)], labels[np.argsort(first, kind="stable")]


def order_np(candidates, iteration, seed=0):
    """The order of the candidates in the 64-bit iteration number(s) `iteration`: int32 [C] (or [n][C] for an array of n):
    _hash.py's shuffle of C in stream STREAM_SPLIT, iteration t starting at the counter t * C."""
    C = int(candidates)
    if not 1 <= C <= MAX_CANDIDATES:
        raise ValueError("candidates must be 1..{}".format(MAX_CANDIDATES))
    if not isinstance(iteration, (list, tuple, np.ndarray)):
        return order_of(draw32(seed, STREAM_SPLIT, shuffle_base(iteration, C), C))
    # (Python integers all the way: NumPy would turn a list that holds numbers of 2^63 and more into float64)
    its = np.asarray(iteration).reshape(-1).tolist() if isinstance(iteration, np.ndarray) else list(iteration)
    return order_of(draw32(seed, STREAM_SPLIT, [shuffle_base(t, C) for t in its], C))


def check_orders(orders, iterations, candidates):
    """int32 [iterations][C] with every row a permutation of 0..C-1, or ValueError.  This is the wrapper's check:
    dta_split_search itself only keeps an entry outside 0..C-1 from leaving the table."""
    o = np.asarray(_host(orders))
    if o.dtype.kind not in "iu" or o.shape != (int(iterations), int(candidates)):
        raise ValueError("orders must be an integer [{}][{}] array, got {} {}".format(iterations, candidates, o.dtype, o.shape))
    if o.size and not (np.sort(o, axis=1) == np.arange(int(candidates))).all():
        raise ValueError("every row of orders must be a permutation of 0..{}".format(int(candidates) - 1))
    return np.ascontiguousarray(o.astype(np.int32))


def _minimums(min_train, min_test):
    min_train, min_test = int(min_train), int(min_test)
    if min_train < 1 or min_test < 1 or max(min_train, min_test) > 0x7FFFFFFF:
        raise ValueError("min_train and min_test must be at least 1, got {} and {}".format(min_train, min_test))
    return min_train, min_test


class SplitTable:
    """The integer-coded annotation table and its A / B / R tables.  from_columns (or from_frame) builds it on the host;
    device= keeps the candidate rows resident for search()."""

    def __init__(self, individual, plot, taxon, fixed, plots, taxa, candidate_plot, device=None):
        self.individual, self.plot, self.taxon, self.fixed = individual, plot, taxon, fixed     # per row, coded
        self.plots, self.taxa = plots, taxa                                                     # labels, first appearance
        P, S = len(plots), len(taxa)
        if not 1 <= S <= MAX_SPECIES:
            raise ValueError("1..{} species, got {}".format(MAX_SPECIES, S))
        n_ind = int(individual.max()) + 1
        rows = np.bincount(individual, minlength=n_ind)
        nonfixed = np.bincount(individual, weights=~fixed, minlength=n_ind).astype(np.int64)
        first = np.full(n_ind, len(individual), np.int64)
        np.minimum.at(first, individual, np.arange(len(individual)))
        ind_plot, ind_taxon = plot[first], taxon[first]
        if (plot != ind_plot[individual]).any():
            raise ValueError("an individual has rows in more than one plot")
        if (taxon != ind_taxon[individual]).any():
            raise ValueError("an individual has rows of more than one taxon")
        cell = ind_plot * S + ind_taxon
        self.A = np.bincount(cell, minlength=P * S).reshape(P, S).astype(np.int64)
        self.B = np.bincount(cell[nonfixed > 0], minlength=P * S).reshape(P, S).astype(np.int64)
        self.R = np.bincount(cell, weights=rows, minlength=P * S).reshape(P, S).astype(np.int64)
        self.totA, self.totR = self.A.sum(0), self.R.sum(0)
        if len(individual) > 0x7FFFFFFF:
            raise ValueError("too many rows for 32-bit counts")
        self.candidates = np.flatnonzero(candidate_plot).astype(np.int64)      # plot codes, in first-appearance order
        if len(self.candidates) > MAX_CANDIDATES:
            raise ValueError("at most {} candidate plots, got {}".format(MAX_CANDIDATES, len(self.candidates)))
        self.device = self.rows_dev = self.totals_dev = None
        if device is not None:
            self.to(device)

    @property
    def n_plots(self):
        return len(self.plots)

    @property
    def n_species(self):
        return len(self.taxa)

    @property
    def n_candidates(self):
        return len(self.candidates)

    @classmethod
    def from_columns(cls, individual, plot, taxon, fixed, candidate=None, site=None, candidate_site=None, device=None):
        """One entry per row of the annotation table.  fixed: the row's box_id contains "fixed".  The candidate plots
        (the reference's siteID == "OSBS") are given as `candidate`, a per-row mask that is constant within a plot, or as
        the `site` column and the name `candidate_site`; neither: every plot is a candidate.  ValueError for an individual
        with two plots or two taxa."""
        ind, _ = _codes(individual)
        plt, plots = _codes(plot)
        tax, taxa = _codes(taxon)
        n = len(ind)
        if n < 1 or len(plt) != n or len(tax) != n:
            raise ValueError("individual, plot and taxon must have one entry per row, and at least one row")
        fixed = np.asarray(_host(fixed)).reshape(-1).astype(bool)
        if len(fixed) != n:
            raise ValueError("fixed must have one entry per row")
        if candidate is not None and site is not None:
            raise ValueError("give candidate or site, not both")
        if site is not None:
            if candidate_site is None:
                raise ValueError("site needs candidate_site")
            candidate = np.asarray(_host(site)).reshape(-1).astype(str) == str(candidate_site)
        if candidate is None:
            cand_plot = np.ones(len(plots), bool)
        else:
            candidate = np.asarray(_host(candidate)).reshape(-1).astype(bool)
            if len(candidate) != n:
                raise ValueError("candidate must have one entry per row")
            cand_plot = np.bincount(plt, weights=candidate, minlength=len(plots)) > 0
            if (candidate != cand_plot[plt]).any():
                raise ValueError("candidate must be the same for every row of a plot")
        return cls(ind, plt, tax, fixed, plots, taxa, cand_plot, device=device)

    @classmethod
    def from_frame(cls, df, candidate_site="OSBS", device=None):
        """From the reference's annotation frame (pandas): columns individual, plotID, taxonID, box_id, siteID."""
        fixed = df["box_id"].astype(str).str.contains("fixed").fillna(False).to_numpy()
        return cls.from_columns(df["individual"].to_numpy(), df["plotID"].to_numpy(), df["taxonID"].to_numpy(), fixed,
                                site=df["siteID"].to_numpy(), candidate_site=candidate_site, device=device)

    def floor(self, min_test):
        """floor[s] = max(float64(totA[s]) * 0.05, float64(min_test)): one float64 product."""
        return np.maximum(self.totA.astype(np.float64) * np.float64(0.05), np.float64(min_test))

    def device_rows(self):
        """What search() keeps resident: rows int32 [C][3][SP] (A, B and R of each candidate plot, SP = S rounded up to a
        multiple of 4, the padding zero) and totals int32 [2][SP] (totA, totR)."""
        S, C = self.n_species, self.n_candidates
        SP = (S + 3) & ~3
        rows = np.zeros((C, 3, SP), np.int32)
        for t, table in enumerate((self.A, self.B, self.R)):
            rows[:, t, :S] = table[self.candidates]
        totals = np.zeros((2, SP), np.int32)
        totals[0, :S], totals[1, :S] = self.totA, self.totR
        return rows, totals

    def to(self, device):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("SplitTable.search runs on a ROCm device only (search_np is the host definition), got {}".format(device))
        if self.n_candidates < 1:
            raise ValueError("no candidate plots")
        rows, totals = self.device_rows()
        self.rows_dev, self.totals_dev, self.device = torch.from_numpy(rows).to(device), torch.from_numpy(totals).to(device), device
        return self

    def search(self, iterations=100, seed=0, first_iteration=0, orders=None, min_train=5, min_test=3, membership=False,
               taxa=False, out=None):
        """search_np on the device (dta_split_search: every iteration in one launch, a second small one picks the best).
        Returns a SplitSearch of device tensors, each overwritten in full by the call; membership / taxa only when asked
        for -- the usual use is to search without them and then run iterations=1, first_iteration=first + best[0] with
        them.  orders: int32 [iterations][C], a host array or a tensor on the device; each row is checked to be a
        permutation here, on the host.  out=: a SplitSearch of tensors to write into.  Nothing here waits for the device
        (but a device `orders` is copied back for its check)."""
        import torch
        from . import _lib
        if self.device is None:
            raise RuntimeError("SplitTable.search runs on a ROCm device only: SplitTable.to(device) first (search_np is the host definition)")
        min_train, min_test = _minimums(min_train, min_test)
        iterations = int(iterations)
        if iterations < 0:
            raise ValueError("iterations must be >= 0")
        C, S, dev = self.n_candidates, self.n_species, self.device
        floor = np.ascontiguousarray(self.floor(min_test))
        if orders is not None:
            checked = check_orders(orders, iterations, C)
            orders = (orders.contiguous() if isinstance(orders, torch.Tensor) and orders.device == dev and orders.dtype == torch.int32
                      else torch.from_numpy(checked).to(dev))
        want = (("species", (iterations,), torch.int32, True), ("train_rows", (iterations,), torch.int64, True),
                ("test_plots", (iterations,), torch.int32, True), ("best", (4,), torch.int64, True),
                ("membership", (iterations, C), torch.uint8, membership), ("taxa", (iterations, S), torch.uint8, taxa))
        res = {}
        for name, shape, dtype, asked in want:
            t = getattr(out, name) if out is not None else None
            if not asked:
                t = None
            elif t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev
                    or not t.is_contiguous()):
                raise ValueError("out.{} must be a contiguous {} {} tensor on {}".format(name, dtype, list(shape), dev))
            res[name] = t
        if iterations == 0:
            res["best"].copy_(torch.tensor([-1, 0, 0, 0], dtype=torch.int64))
            return SplitSearch(**res)
        L = _lib.lib()
        _lib.check(L.dta_split_search(_lib.ptr(self.rows_dev), _lib.ptr(self.totals_dev), C, S,
                                      floor.ctypes.data_as(_lib.c_double_p), min_train, min_test, iterations,
                                      int(seed) & _M64, int(first_iteration) & _M64, _lib.ptr(orders),
                                      _lib.ptr(res["species"]), _lib.ptr(res["train_rows"]), _lib.ptr(res["test_plots"]),
                                      _lib.ptr(res["best"]), _lib.ptr(res["membership"]), _lib.ptr(res["taxa"]),
                                      _lib.current_stream_ptr()), "dta_split_search")
        return SplitSearch(**res)


def search_np(table, iterations, seed=0, first_iteration=0, orders=None, min_train=5, min_test=3):
    """The definition of the search (the module docstring spells the rule out): a SplitSearch of host arrays, membership
    and taxa included.  orders: int32 [iterations][C], each row a permutation of the candidates, replaces order_np."""
    min_train, min_test = _minimums(min_train, min_test)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0")
    C, S = table.n_candidates, table.n_species
    if C < 1:
        raise ValueError("no candidate plots")
    if orders is not None:
        orders = check_orders(orders, iterations, C)
    Ac, Bc, Rc = table.A[table.candidates], table.B[table.candidates], table.R[table.candidates]
    floor = table.floor(min_test)
    species = np.zeros(iterations, np.int32)
    train_rows = np.zeros(iterations, np.int64)
    test_plots = np.zeros(iterations, np.int32)
    membership = np.zeros((iterations, C), np.uint8)
    taxa = np.zeros((iterations, S), np.uint8)
    for lo in range(0, iterations, _CHUNK):
        n = min(_CHUNK, iterations - lo)
        its = np.arange(n)
        order = orders[lo:lo + n] if orders is not None else order_np(C, [int(first_iteration) + lo + t for t in range(n)], seed)
        cnt = np.zeros((n, S), np.int64)
        to_sample = np.ones((n, S), bool)
        inc = np.zeros((n, C), bool)
        for k in range(C):
            p = order[:, k]
            a = Ac[p]
            hit = ((a > 0) & to_sample).any(1)
            if hit.any():
                cnt[hit] += a[hit]
                to_sample[hit] = ~(cnt[hit].astype(np.float64) > floor)
                inc[its[hit], p[hit]] = True
            if not to_sample.any():
                break
        sel = inc.astype(np.int64)
        T = ((sel @ Bc) >= min_test) & ((table.totA - sel @ Ac) >= min_train)
        species[lo:lo + n] = T.sum(1)
        train_rows[lo:lo + n] = ((table.totR - sel @ Rc) * T).sum(1)
        test_plots[lo:lo + n] = inc.sum(1)
        membership[lo:lo + n], taxa[lo:lo + n] = inc, T
    if iterations:
        # lexicographic maximum of (species, train_rows), the earliest iteration on a full tie
        b = int(np.lexsort((np.arange(iterations), -train_rows, -species.astype(np.int64)))[0])
        best = (b, int(species[b]), int(train_rows[b]), int(test_plots[b]))
    else:
        best = (-1, 0, 0, 0)
    return SplitSearch(species, train_rows, test_plots, best, membership, taxa)


def rows_np(table, inc, T):
    """The row membership of a split: (train, test) boolean masks over the table's rows.  inc: [C] over the candidate
    plots (a row of SplitSearch.membership); T: [S] over the species (a row of SplitSearch.taxa).
    test: plot in inc, not fixed, taxon in T;  train: plot not in inc, taxon in T."""
    inc, T = np.asarray(_host(inc)).reshape(-1) != 0, np.asarray(_host(T)).reshape(-1) != 0
    if len(inc) != table.n_candidates or len(T) != table.n_species:
        raise ValueError("inc must be [{}] and T [{}]".format(table.n_candidates, table.n_species))
    in_test = np.zeros(table.n_plots, bool)
    in_test[table.candidates[inc]] = True
    kept = T[table.taxon]
    return ~in_test[table.plot] & kept, in_test[table.plot] & ~table.fixed & kept


def _column(columns, *names):
    for n in names:
        try:
            if n in columns:
                c = columns[n]
                return c.to_numpy() if hasattr(c, "to_numpy") else np.asarray(_host(c))
        except TypeError:
            break
    return None


def _split(columns, min_train, min_test, iterations, seed, orders, candidate_site, device):
    min_train, min_test = _minimums(min_train, min_test)
    individual, plot, taxon = (_column(columns, *n) for n in (("individual",), ("plot", "plotID"), ("taxon", "taxonID")))
    if individual is None or plot is None or taxon is None:
        raise ValueError("columns needs individual, plot (or plotID) and taxon (or taxonID)")
    fixed = _column(columns, "fixed")
    if fixed is None:
        box = _column(columns, "box_id")
        fixed = np.zeros(len(individual), bool) if box is None else np.array(["fixed" in str(b) for b in box], bool)
    candidate, site = _column(columns, "candidate"), _column(columns, "site", "siteID")
    if candidate is not None:
        site = None
    n = len(individual)
    # the reference's prefilter: species with more than min_train + min_test ROWS
    tax, _ = _codes(taxon)
    keep = (np.bincount(tax) > min_train + min_test)[tax]
    at = np.flatnonzero(keep)
    if len(at) == 0:
        raise ValueError("no species has more than {} rows".format(min_train + min_test))

    def cut(c):
        return None if c is None else np.asarray(c).reshape(-1)[at]

    plots, plot_labels = _codes(cut(plot))
    train, test = np.zeros(n, bool), np.zeros(n, bool)
    if len(plot_labels) <= 2:
        # the reference's fixed answer (data.py:120-124), filters and all skipped: first plot test, second plot train
        if len(plot_labels) < 2:
            raise ValueError("a split needs at least two plots")
        test[at[plots == 0]], train[at[plots == 1]] = True, True
        return Split(train, test, 0, np.unique(np.asarray(cut(taxon)).astype(str)), 1)
    table = SplitTable.from_columns(cut(individual), cut(plot), cut(taxon), cut(fixed), candidate=cut(candidate), site=cut(site),
                                    candidate_site=candidate_site if site is not None else None)
    if table.n_candidates < 1:
        raise ValueError("no candidate plots")
    if device is None:
        best = search_np(table, iterations, seed, 0, orders, min_train, min_test).best
        one = search_np(table, 1, seed, best[0], None if orders is None else np.asarray(_host(orders))[best[0]:best[0] + 1],
                        min_train, min_test) if best[0] >= 0 else None
    else:
        table.to(device)
        best = tuple(int(v) for v in table.search(iterations, seed, 0, orders, min_train, min_test).best.cpu().tolist())
        one = None
        if best[0] >= 0:
            o = None if orders is None else check_orders(orders, iterations, table.n_candidates)[best[0]:best[0] + 1]
            one = table.search(1, seed, best[0], o, min_train, min_test, membership=True, taxa=True)
            one = one._replace(membership=one.membership.cpu().numpy(), taxa=one.taxa.cpu().numpy())
    if best[0] < 0 or best[1] == 0:
        raise ValueError("no split of {} iterations keeps a species in both train and test".format(iterations))
    tr, te = rows_np(table, one.membership[0], one.taxa[0])
    train[at], test[at] = tr, te
    return Split(train, test, best[0], table.taxa[one.taxa[0] != 0], best[3])


def train_test_split_np(columns, min_train=5, min_test=3, iterations=100, seed=0, orders=None, candidate_site="OSBS"):
    """The definition of train_test_split: the same steps with search_np in place of the device."""
    return _split(columns, min_train, min_test, iterations, seed, orders, candidate_site, None)


def train_test_split(columns, min_train=5, min_test=3, iterations=100, seed=0, orders=None, candidate_site="OSBS",
                     device="cuda"):
    """The whole of the reference's train_test_split: Split(train, test, iteration, species, test_plots) with train and
    test boolean masks over the rows of `columns`.

    columns: a mapping (or a pandas frame) with individual, plot / plotID, taxon / taxonID, fixed (or box_id, fixed = it
    contains "fixed") and the candidate plots as `candidate` (per-row mask) or site / siteID with candidate_site; neither:
    every plot is a candidate.  The steps: the species prefilter (more than min_train + min_test rows); with two plots
    or fewer the reference's fixed answer (first plot test, second train) without a launch; else the search on the
    device and one more iteration for the membership of the best.  ValueError when the best split has no species."""
    return _split(columns, min_train, min_test, iterations, seed, orders, candidate_site, device)
