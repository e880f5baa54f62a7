"""The resident training set: the reference's `TreeDataset` (src/data.py:239-310) and the five of them that
`MultiStage.create_datasets` builds over the same individuals (src/models/multi_stage.py:82-219), kept on the device.

  * `CropPool`    the preprocessed, resized, unflipped crops of a whole data set, [N][Y][C][S][S], resident ONCE: one slot per
                  (individual, year), zeros where an individual has no crop of a year (data.py:274 / :298).  float32 (bit for
                  bit the reference's `load_image`), or bf16 storage on request: the stored value is float32(bf16(x)), round
                  to nearest even, widened exactly on the way out.
  * `PoolView`    one TreeDataset: int64 rows into the pool and int64 labels, both resident.  `LevelViews` is the list of
                  them `create_datasets` returns; a level is only rows and labels, never a second copy of the crops.  Which
                  individuals belong to which level, in what order and with which labels is levels.py's work
                  (`levels.create_datasets` returns the `LevelViews`); a view may carry `year_keep`, uint8 [n][Y], where a
                  level keeps only some of an individual's years (level 3's ceiling counts records): a masked (entry,
                  year) is gathered as a missing year.
  * the order     `epoch_order_np(n, epoch, seed, level)`: entry i draws key_i = draw32 at the counter epoch * n + i of
                  stream 16 + level (_hash.py: the counter hash, the shuffle and the streams in use) and the entries
                  are sorted ascending by (key_i, i).  A pure function of (seed, epoch, level): an epoch can be resumed, the
                  ranks of a data-parallel run agree on it without talking, and the host names the individuals of a batch
                  without asking the device.  dta_epoch_order computes every level's order in one launch, by counting the
                  smaller keys (exact: the (key, i) pairs are distinct); at most MAX_N entries per level.
  * the batches   step s of an epoch at batch size B: level l has nb_l = ceil(n_l / B) batches (floor with drop_last; 0 is
                  refused) and brings batch k = s mod nb_l of its order, positions k * B .. min((k + 1) * B, n_l) - 1 -- the
                  cycling loop.fit_multistage does with lists of batches (Lightning's "max_size_cycle"); the epoch has
                  max_l nb_l steps.  dta_pool_batches writes every level x year batch of a step in ONE launch, with the
                  labels, the pool rows and the level-years' 0/1 flags (what dta_year_flags would say after reading the
                  batches back).  train=True reverses the S * S pixels of every plane: both of the reference's p = 1 flips
                  (src/augmentation.py:13-14) together.

The NumPy functions are the definition (`epoch_order_np`, `plan`, `step_positions`, `batch_np`, `bf16_round_np`); the device
equals them bit for bit.  File reading stays with the caller: the constructors start from arrays.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._hash import M64 as _M64, draw32, host as _host, order_of, shuffle_base
from .split import _codes

MAX_N = _lib.EPOCH_ORDER_MAX_N               # entries of one view that dta_epoch_order sorts
ORDER_STREAM = _lib.EPOCH_ORDER_STREAM       # stream ORDER_STREAM + level (_hash.py lists the streams in use)
MAX_LEVEL_ID = _lib.EPOCH_ORDER_MAX_LEVEL_ID


def epoch_order_np(n, epoch=0, seed=0, level=0):
    """The order of a view of n entries in `epoch`: int32 [n], _hash.py's shuffle of n in stream ORDER_STREAM + level,
    starting at the counter epoch * n."""
    n, level = int(n), int(level)
    if n < 1:
        raise ValueError("n must be at least 1, got {}".format(n))
    if not 0 <= level < MAX_LEVEL_ID:
        raise ValueError("level must be 0..{}, got {}".format(MAX_LEVEL_ID - 1, level))
    return order_of(draw32(seed, ORDER_STREAM + level, shuffle_base(epoch, n), n))


def plan(sizes, batch_size, drop_last=False):
    """(nb, steps): the batches each level has at this batch size and the steps of an epoch, max(nb)."""
    B = int(batch_size)
    if B < 1:
        raise ValueError("batch_size must be at least 1, got {}".format(B))
    nb = []
    for l, n in enumerate(sizes):
        n = int(n)
        if n < 1:
            raise ValueError("level {} is empty".format(l))
        k = n // B if drop_last else -(-n // B)
        if k == 0:
            raise ValueError("level {} has {} entries: no batch of {} with drop_last".format(l, n, B))
        nb.append(k)
    return nb, max(nb)


def step_positions(n, nb, batch_size, step):
    """(start, count): the positions of its order a level of n entries and nb batches brings to `step`."""
    k = int(step) % int(nb)
    start = k * int(batch_size)
    return start, min(start + int(batch_size), int(n)) - start


def bf16_round_np(x):
    """float32(bf16(x)), round to nearest even: what a bf16 pool stores.  A NaN stays a NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).astype(np.uint32)
    r = np.where(np.isnan(x), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def batch_np(crops, rows, train=False, year_keep=None):
    """The definition of a batch: crops [N][Y][C][S][S] (the pool's content), rows the pool rows of the batch in order.
    Returns one [len(rows)][C][S][S] array per year; train=True: every plane flipped along both axes.  year_keep: uint8
    [len(rows)][Y] or None; where it is 0 the crop of that (entry, year) is zeros, as for a missing year."""
    crops = np.asarray(crops)
    rows = np.asarray(rows, np.int64).reshape(-1)
    if year_keep is not None:
        year_keep = np.asarray(year_keep).reshape(len(rows), crops.shape[1])
    out = []
    for y in range(crops.shape[1]):
        b = crops[rows, y]
        if year_keep is not None:
            b = np.where((year_keep[:, y] != 0)[:, None, None, None], b, np.zeros((), b.dtype))
        out.append(np.ascontiguousarray(b[:, :, ::-1, ::-1] if train else b))
    return out


def annotation_slots(columns, raw_by_path):
    """The host half of CropPool.from_annotations: (raw[n][y], individuals, years, labels) -- the reference's
    TreeDataset.__init__ ordering (both in first-appearance order) with one slot per (individual, year), None where the
    table has no row for the pair or raw_by_path has no such path; labels int64 [N] or None without a label column."""
    def col(name):
        if name not in columns:
            return None
        c = columns[name]
        return c.to_numpy() if hasattr(c, "to_numpy") else np.asarray(_host(c))
    ind, year, path, label = col("individual"), col("tile_year"), col("image_path"), col("label")
    if ind is None or year is None or path is None:
        raise ValueError("columns needs individual, tile_year and image_path")
    if not len(ind) or len(year) != len(ind) or len(path) != len(ind) or (label is not None and len(label) != len(ind)):
        raise ValueError("individual, tile_year, image_path and label must have one entry per row, and at least one row")
    icode, inames = _codes(ind)
    ycode, ynames = _codes(year)
    raw = [[None] * len(ynames) for _ in inames]
    labels = np.zeros(len(inames), np.int64) if label is not None else None
    for r in range(len(icode)):
        p = path[r]
        p = p.decode() if isinstance(p, bytes) else str(p)
        raw[icode[r]][ycode[r]] = raw_by_path.get(p) if hasattr(raw_by_path, "get") else raw_by_path[p]
        if labels is not None:
            labels[icode[r]] = int(label[r])
    return raw, inames.tolist(), ynames.tolist(), labels


def _is_cuda(device):
    return torch.device(device).type == "cuda"


class CropPool:
    """The crops of a whole data set, resident once.  crops: [N][Y][C][S][S] float32 -- preprocessed, resized, unflipped --
    as a host array or a tensor; present: uint8 [N][Y] (default: all present; a missing slot holds zeros); individuals: N
    names (default 0 .. N - 1).  dtype=torch.bfloat16 stores float32(bf16(x)).  A pool may be built on any device; the
    launches run on a ROCm device only."""

    def __init__(self, crops, present=None, individuals=None, device="cuda", dtype=torch.float32, years=None, labels=None):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16, got {}".format(dtype))
        t = crops if isinstance(crops, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(crops), dtype=np.float32))
        if t.dim() != 5 or t.shape[3] != t.shape[4] or min(t.shape) < 1:
            raise ValueError("crops must be [N][Y][C][S][S], got shape {}".format(tuple(t.shape)))
        if t.dtype not in (torch.float32, dtype):
            raise ValueError("crops must be float32, got {}".format(t.dtype))
        self.data = t.to(device=torch.device(device), dtype=dtype).contiguous()
        self.device, self.dtype = self.data.device, dtype
        self.n, self.n_years, self.bands, self.size = (int(v) for v in self.data.shape[:4])
        p = np.ones((self.n, self.n_years), np.uint8) if present is None else np.asarray(_host(present)).astype(np.uint8)
        if p.shape != (self.n, self.n_years):
            raise ValueError("present must be [{}][{}], got {}".format(self.n, self.n_years, p.shape))
        self.present = p
        self.individuals = list(range(self.n)) if individuals is None else list(individuals)
        if len(self.individuals) != self.n:
            raise ValueError("one name per individual ({}), got {}".format(self.n, len(self.individuals)))
        self.years = list(range(self.n_years)) if years is None else list(years)
        self.labels = None if labels is None else np.asarray(_host(labels), np.int64).reshape(-1)

    def __len__(self):
        return self.n

    @property
    def bytes_per_crop_year(self):
        return self.bands * self.size * self.size * self.data.element_size()

    # ---- constructors -------------------------------------------------------------------------------------------------
    @classmethod
    def from_raw(cls, raw, image_size=11, clip=10, chunk=256, device="cuda", dtype=torch.float32, **kw):
        """raw[n][y]: a raw band-first crop (bands, h, w) as the file reader returned it, or None for a missing year.  Every
        crop goes through preprocess.preprocess_batch(..., train=False, out=<the pool's slab>), `chunk` slots at a time,
        so a float32 pool holds the reference's load_image(path, image_size) bit for bit."""
        from . import preprocess
        raw = [list(r) for r in raw]
        N = len(raw)
        Y = len(raw[0]) if N else 0
        if N < 1 or Y < 1 or any(len(r) != Y for r in raw):
            raise ValueError("raw must be [N][Y] crops (None for a missing year), N and Y at least 1")
        flat = [c for r in raw for c in r]
        first = next((c for c in flat if c is not None), None)
        if first is None:
            raise ValueError("at least one crop must be present")
        bands = preprocess.out_bands(int((first.shape if hasattr(first, "shape") else np.asarray(first).shape)[0]), clip)
        S = int(image_size)
        if not _is_cuda(device):
            raise RuntimeError("CropPool.from_raw preprocesses on a ROCm device only, got {}".format(device))
        slab = torch.zeros(N * Y, bands, S, S, dtype=torch.float32, device=device)
        for lo in range(0, N * Y, int(chunk)):
            part = flat[lo:lo + int(chunk)]
            if all(c is None for c in part):
                continue                      # (the slab is zero already)
            preprocess.preprocess_batch(part, S, train=False, clip=clip, device=device, out=slab[lo:lo + len(part)])
        present = np.array([[c is not None for c in r] for r in raw], np.uint8)
        return cls(slab.view(N, Y, bands, S, S), present=present, device=device, dtype=dtype, **kw)

    @classmethod
    def from_annotations(cls, columns, raw_by_path, image_size=11, **kw):
        """The reference's TreeDataset.__init__ on an annotation table.  columns: a mapping (or a pandas frame) with
        individual, tile_year, image_path and optionally label, one entry per row; raw_by_path: image_path -> raw band-first
        crop (file reading is the caller's).  Years and individuals are taken in the order of first appearance (pandas'
        .unique()); one slot per (individual, year), the last row of a pair wins (as the reference's to_dict does), a year
        without a row -- or a path raw_by_path does not have -- is missing.  The pool's `labels` are the individuals'
        (the last row's, as set_index("individual").label.to_dict() gives)."""
        raw, individuals, years, labels = annotation_slots(columns, raw_by_path)
        return cls.from_raw(raw, image_size, individuals=individuals, years=years, labels=labels, **kw)

    @classmethod
    def from_rasters(cls, rasters_by_year, boxes, image_size=11, chunk=1024, dtype=torch.float32, **kw):
        """For callers whose tiles are resident: one fp32 dense.DenseRaster per year (None: a missing year) and the
        individuals' crown boxes [N][4] (row0, col0, row1, col1), through DenseRaster.crops_years -- all years of `chunk`
        boxes in one launch."""
        from .dense import DenseRaster
        rs = list(rasters_by_year)
        have = [r for r in rs if r is not None]
        if not have:
            raise ValueError("at least one year must have a raster")
        boxes = np.ascontiguousarray(np.asarray(_host(boxes), np.int32))
        if boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.shape[0] < 1:
            raise ValueError("boxes must be a non-empty [N, 4] array of (row0, col0, row1, col1)")
        N, Y, S, dev = boxes.shape[0], len(rs), int(image_size), have[0].device
        data = torch.zeros(N, Y, have[0].bands, S, S, dtype=torch.float32, device=dev)
        banks = torch.zeros(2, Y, dtype=torch.float32, device=dev)
        for k, lo in enumerate(range(0, N, int(chunk))):
            n = min(int(chunk), N - lo)
            outs = [torch.zeros(n, have[0].bands, S, S, dtype=torch.float32, device=dev) for _ in rs]
            DenseRaster.crops_years(rs, boxes[lo:lo + n], outs, banks[k & 1], banks[(k & 1) ^ 1], size=S, train=False)
            for y, o in enumerate(outs):
                if rs[y] is not None:
                    data[lo:lo + n, y] = o
        present = np.repeat(np.array([[r is not None for r in rs]], np.uint8), N, axis=0)
        return cls(data, present=present, device=dev, dtype=dtype, **kw)

    # ---- views ----------------------------------------------------------------------------------------------------------
    def view(self, rows, labels=None, train=None, level=0, year_keep=None):
        """One TreeDataset over this pool: `rows` (int64 rows of the pool, in the data set's order) and their labels; train:
        the data set's own flip setting (PoolView), None to leave it to the caller of loader / batches; year_keep: uint8
        [len(rows)][Y] or None -- 0 masks that year of that entry, which is then gathered as a missing year."""
        return PoolView(self, rows, labels, train, level, year_keep)

    def numpy(self):
        """The pool's content as float32 [N][Y][C][S][S] on the host (a bf16 pool: the stored values, widened)."""
        return self.data.float().cpu().numpy()


class PoolView:
    """One TreeDataset: rows into a CropPool and their labels, both resident.  train: the data set's own setting (the
    reference's TreeDataset(train=True) flips every crop both ways), which `loader` and `LevelViews.batches` take unless
    they are told otherwise; None (unset): `loader` does not flip and `batches` does.  level: which level's shuffle stream
    the view draws.
    `loader` has the interface of loop.SyntheticTreeDataset.loader, so loop.fit, validate, validate_multistage and
    predict_multistage take a view as it is."""

    def __init__(self, pool, rows, labels=None, train=None, level=0, year_keep=None):
        r = np.asarray(_host(rows)).reshape(-1)
        if r.dtype.kind not in "iu" or len(r) < 1:
            raise ValueError("rows must be a non-empty integer array")
        r = r.astype(np.int64)
        if (r < 0).any() or (r >= pool.n).any():
            raise ValueError("rows must lie in the pool, 0..{}".format(pool.n - 1))
        if not 0 <= int(level) < MAX_LEVEL_ID:
            raise ValueError("level must be 0..{}, got {}".format(MAX_LEVEL_ID - 1, level))
        self.pool, self.rows_np, self.train, self.level = pool, r, None if train is None else bool(train), int(level)
        self.rows = torch.from_numpy(r).to(pool.device)
        self.labels = None
        if labels is not None:
            y = np.asarray(_host(labels)).reshape(-1)
            if y.dtype.kind not in "iu" or len(y) != len(r):
                raise ValueError("labels must be one integer per row ({}), got {} {}".format(len(r), y.dtype, y.shape))
            self.labels = labels.to(device=pool.device, dtype=torch.int64).contiguous() if isinstance(labels, torch.Tensor) \
                else torch.from_numpy(y.astype(np.int64)).to(pool.device)
        self.year_keep_np = self.year_keep = None
        if year_keep is not None:
            k = np.asarray(_host(year_keep))
            if k.dtype.kind not in "iub" or k.shape != (len(r), pool.n_years):
                raise ValueError("year_keep must be [{}][{}] of 0 / 1, got {} {}".format(len(r), pool.n_years, k.dtype, k.shape))
            self.year_keep_np = np.ascontiguousarray(k != 0).astype(np.uint8)
            self.year_keep = torch.from_numpy(self.year_keep_np).to(pool.device)

    def __len__(self):
        return len(self.rows_np)

    def at_level(self, level):
        """The same view (the same resident tables) drawing level `level`'s shuffle stream."""
        if not 0 <= int(level) < MAX_LEVEL_ID:
            raise ValueError("level must be 0..{}, got {}".format(MAX_LEVEL_ID - 1, level))
        v = object.__new__(PoolView)
        v.__dict__.update(self.__dict__)
        v.level = int(level)
        return v

    @property
    def individuals(self):
        return [self.pool.individuals[i] for i in self.rows_np]

    def batch_np(self, positions, train=None):
        """The definition of the batch that brings the entries `positions` of this view (module-level batch_np)."""
        at = np.asarray(positions, np.int64)
        return batch_np(self.pool.numpy(), self.rows_np[at], bool(self.train if train is None else train),
                        None if self.year_keep_np is None else self.year_keep_np[at])

    def loader(self, batch_size, shuffle=False, seed=0, drop_last=False, train=None, epoch=0):
        """Yields (individual, {"HSI": [Y tensors], "rows": pool rows}, labels) per batch, one launch each: the view's
        entries in order, or in epoch_order_np(n, epoch, seed, level)'s.  train: None takes the view's own setting, and no
        flips where that is unset."""
        for batch, _ in _steps([self], batch_size, shuffle, seed, train, drop_last, epoch, False):
            yield batch[0]


class LevelViews:
    """The list of data sets MultiStage.create_datasets returns, as views of ONE pool: level l is views[l], drawing shuffle
    stream l.  A sequence of its (level-tagged) views, so anything that takes one data set per level takes it."""

    def __init__(self, views):
        views = list(views)
        if not views:
            raise ValueError("at least one level")
        if any(not isinstance(v, PoolView) or v.pool is not views[0].pool for v in views):
            raise ValueError("every level must be a view of the same pool")
        if len(views) > _lib.MAX_LEVELS:
            raise ValueError("at most {} levels, got {}".format(_lib.MAX_LEVELS, len(views)))
        if len(views) * views[0].pool.n_years > _lib.MAX_YEARS:
            raise ValueError("at most {} networks (levels x years), got {} x {}".format(_lib.MAX_YEARS, len(views),
                                                                                      views[0].pool.n_years))
        self.pool = views[0].pool
        self.views = [v.at_level(l) for l, v in enumerate(views)]

    def __len__(self):
        return len(self.views)

    def __getitem__(self, l):
        return self.views[l]

    def __iter__(self):
        return iter(self.views)

    def steps(self, batch_size, drop_last=False):
        return plan([len(v) for v in self.views], batch_size, drop_last)[1]

    def batches(self, batch_size, shuffle=False, seed=0, train=None, drop_last=False, epoch=0):
        """The steps of an epoch: yields (batch_per_level, year_flags), ONE launch per step.  batch_per_level[l] is level
        l's (individual, {"HSI": [Y tensors], "rows": ...}, labels) -- a level with fewer batches cycles --, year_flags the
        float32 [levels * years] flags MultiStageTrainer.training_step_all(year_flags=) takes (level-major; one of two
        banks used alternately: it holds until the launch after the next).  train: None takes each view's own setting, and
        both flips where that is unset (these are training batches).
        The individuals' names come from the host's own epoch_order_np: nothing is read back."""
        return _steps(self.views, batch_size, shuffle, seed, train, drop_last, epoch, True)


def epoch_order(sizes, epoch=0, seed=0, levels=None, device="cuda"):
    """epoch_order_np(n, epoch, seed, level) for every (n, level) of `sizes` / `levels` (default 0, 1, ...) on the device,
    all of them in ONE launch (dta_epoch_order): a list of resident int32 [n] tables (slices of one tensor).  At most
    _lib.MAX_LEVELS tables of at most MAX_N entries; refused before the launch otherwise."""
    sizes = [int(n) for n in sizes]
    nl = len(sizes)
    levels = list(range(nl)) if levels is None else [int(v) for v in levels]
    if not 1 <= nl <= _lib.MAX_LEVELS or len(levels) != nl:
        raise ValueError("1..{} tables and one level id each, got {} and {}".format(_lib.MAX_LEVELS, nl, len(levels)))
    if min(sizes) < 1 or max(sizes) > MAX_N:
        raise ValueError("a shuffled view has 1..{} entries (dta_epoch_order), got {}".format(MAX_N, sizes))
    if any(not 0 <= v < MAX_LEVEL_ID for v in levels):
        raise ValueError("level ids must be 0..{}, got {}".format(MAX_LEVEL_ID - 1, levels))
    if not _is_cuda(device):
        raise RuntimeError("epoch_order runs on a ROCm device only (epoch_order_np is the host definition), got {}".format(device))
    L = _lib.lib()
    table = torch.empty(sum(sizes), dtype=torch.int32, device=device)
    orders, at = [], 0
    for n in sizes:
        orders.append(table[at:at + n])
        at += n
    _lib.check(L.dta_epoch_order(nl, (C.c_longlong * nl)(*sizes), (C.c_int * nl)(*levels), int(seed) & _M64, int(epoch) & _M64,
                                 (C.c_void_p * nl)(*[o.data_ptr() for o in orders]), _lib.current_stream_ptr()),
               "dta_epoch_order")
    return orders


def _steps(views, batch_size, shuffle, seed, train, drop_last, epoch, unset):
    """The body of PoolView.loader and LevelViews.batches.  Everything is checked before the library is reached."""
    pool = views[0].pool
    sizes = [len(v) for v in views]
    nb, steps = plan(sizes, batch_size, drop_last)
    B, Y, nl = int(batch_size), pool.n_years, len(views)
    if nl > _lib.MAX_LEVELS or nl * Y > _lib.MAX_YEARS:
        raise ValueError("at most {} levels and {} networks (levels x years), got {} x {}".format(_lib.MAX_LEVELS, _lib.MAX_YEARS, nl, Y))
    if shuffle and max(sizes) > MAX_N:
        raise ValueError("a shuffled view has at most {} entries (dta_epoch_order), got {}".format(MAX_N, max(sizes)))
    if not _is_cuda(pool.device):
        raise RuntimeError("the batches of a CropPool are gathered on a ROCm device only (batch_np is the host definition), "
                           "got a pool on {}".format(pool.device))
    flips = [int(bool(train) if train is not None else unset if v.train is None else v.train) for v in views]
    L = _lib.lib()
    dev = pool.device
    orders_np = orders = None
    if shuffle:
        orders_np = [epoch_order_np(n, epoch, seed, v.level) for n, v in zip(sizes, views)]
        orders = epoch_order(sizes, epoch, seed, [v.level for v in views], dev)
    per = pool.bands * pool.size * pool.size
    code = _lib.DTA_F32 if pool.dtype == torch.float32 else _lib.DTA_BF16
    shape = (pool.bands, pool.size, pool.size)
    # two banks of year flags used alternately (dta_year_flags' protocol): a launch sets one and zeroes the other
    banks = torch.zeros(2, nl * Y, dtype=torch.float32, device=dev)
    # the levels' year masks (PoolView.year_keep), or None: the call without them, as it always was
    keeps = None
    if any(v.year_keep is not None for v in views):
        keeps = (C.c_void_p * nl)(*[None if v.year_keep is None else v.year_keep.data_ptr() for v in views])
    for s in range(steps):
        pos = [step_positions(n, k, B, s) for n, k in zip(sizes, nb)]
        # fresh outputs from torch's allocator: one slab for the crops (every batch 16-byte aligned), one for labels and rows
        seg = [(c * per + 3) & ~3 for _, c in pos]
        slab = torch.empty(Y * sum(seg), dtype=torch.float32, device=dev)
        ints = torch.empty(2 * sum(c for _, c in pos), dtype=torch.int64, device=dev)
        flags, clear_next = banks[s & 1], banks[(s & 1) ^ 1]
        lv, outs, batch, at, iat = [], [], [], 0, 0
        for l, (v, (start, count)) in enumerate(zip(views, pos)):
            xs = []
            for y in range(Y):
                xs.append(slab[at:at + count * per].view((count,) + shape))
                at += seg[l]
            out_rows = ints[iat:iat + count]
            out_labels = ints[iat + count:iat + 2 * count] if v.labels is not None else None
            iat += 2 * count
            lv.append(_lib.PoolLevel(None if orders is None else orders[l].data_ptr(), v.rows.data_ptr(),
                                     None if v.labels is None else v.labels.data_ptr(), sizes[l], start, count, flips[l],
                                     None if out_labels is None else out_labels.data_ptr(), out_rows.data_ptr()))
            outs += [x.data_ptr() for x in xs]
            entries = np.arange(start, start + count) if orders_np is None else orders_np[l][start:start + count]
            names = [pool.individuals[i] for i in v.rows_np[entries]]
            batch.append((names, {"HSI": xs, "rows": out_rows}, out_labels))
        if keeps is None:
            _lib.check(L.dta_pool_batches(_lib.ptr(pool.data), code, pool.n, Y, pool.bands, pool.size, nl,
                                          (_lib.PoolLevel * nl)(*lv), (C.c_void_p * len(outs))(*outs), _lib.ptr(flags),
                                          _lib.ptr(clear_next), _lib.current_stream_ptr()), "dta_pool_batches")
        else:
            _lib.check(L.dta_pool_batches_keep(_lib.ptr(pool.data), code, pool.n, Y, pool.bands, pool.size, nl,
                                               (_lib.PoolLevel * nl)(*lv), keeps, (C.c_void_p * len(outs))(*outs),
                                               _lib.ptr(flags), _lib.ptr(clear_next), _lib.current_stream_ptr()),
                       "dta_pool_batches_keep")
        yield batch, flags
