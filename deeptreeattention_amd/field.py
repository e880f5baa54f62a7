"""Field records to canopy points: the first thing the reference's TreeData does with a raw NEON table -- `filter_data`
(src/data.py:22-106) -- and the plot code `megaplot.format` gives every stem of a contributed megaplot (src/megaplot.py:28-90:
`create_grid` + `gpd.sjoin`, `buffer_plots`).  The reference runs a Python loop over `groupby("individual")` with list
comprehensions per group (:35-43), a `groupby.apply(sort_values().head(1))` per individual (:73), an O(n^2) loop of shapely
buffers and a spatial join against a grid of shapely boxes.  Here the strings are looked at once on the host
(FieldTable.from_frame) and everything after is integer and float columns on the device (dta_field_filter,
dta_megaplot_plots, csrc/field.hip).  The stage sits in front of canopy.HeightRules and stems.CrownBoxes.assign, whose
`point_plot` codes megaplot_plots produces.

1. filter_data.  A row of the table becomes
    individual  int32    the rank of its `individualID` among the sorted unique ones (np.unique order)
    event       int32    the rank of its `eventID` among the sorted unique ones
    height      float64  NaN = missing;   diameter  float64  (`stemDiameter`), NaN = missing
    flags       uint16   COORDS `itcEasting` not null; GROWTH `growthForm` not null and not in rules.growth_excluded; LIVE
                         `plantStatus` not null and contains rules.status_contains; SHADED / SUNNY `canopyPosition` in
                         rules.shaded / rules.sunny; TAXON_EXCLUDED the taxon after rules.remap is in rules.taxa_excluded;
                         EVENT_DROPPED `eventID` contains rules.event_excluded; MULTIBOLE `individualID` matches
                         rules.multibole; KNOWN_ERROR `individualID` in rules.known_errors; PLOT_EXCLUDED `plotID` in
                         rules.plots_excluded; SITE_EXCLUDED `siteID` in rules.sites_excluded
The rule, in the reference's order; `reason` is the first step that drops the row, 0 = kept:
    1 no coordinates (:29)    2 growth form (:30-31)    3 plant status (:32-33)
    4 shaded individual (:35-45): over the rows that passed 1-3, an individual with a SHADED row and no SUNNY row loses all
    5 height (:46): a row stays if height > min_height or height is NaN
    6 stem diameter (:47): a row stays if diameter > min_stem_diameter; NaN fails
    7 taxon excluded (:66)    8 event excluded (:67)
    9 not the individual's record (:68-75): among the rows that passed 1-8 an individual with at least one height keeps the
      row of its maximum height (-0.0 == +0.0), the lowest row among equals (idxmax); one with none keeps the row of its
      largest event code, the lowest row among equals (the reference's sort_values is unstable there: nothing finer is
      promised)
    10 multibole (:78)    11 known error (:82)    12 plot excluded (:83, :104)    13 site excluded (:101)
    255 an individual code outside 0 .. individuals-1 or a negative event code (FieldTable never makes one)
Filtered(keep uint8 [N], reason uint8 [N], rows int64 [N], count int64): rows[:count] are the kept rows in the reference's
output order -- the individuals chosen by height, ascending by code, then those chosen by event, ascending by code -- and
rows[count:] is -1.  The reference's BLAN 18N -> 17N reprojection (:89-98) needs pyproj: a table with such rows is refused.

2. megaplot.format's plot code.  rule "auto" is the reference's switch: n > 1000 -> "grid", else "buffer".
"grid" (create_grid + sjoin, :41-43, :69-90): bounds = min / max of the points with finite coordinates, xs =
np.arange(xmin, xmax + cell, cell), ys likewise (np.arange itself, on the host; resident points cost one read-back of these
four numbers).  Cell (i, j) has the code i * len(ys) + j and is the closed rectangle xs[i] - cell <= x <= xs[i],
ys[j] <= y <= ys[j] + cell, each bound rounded once: the reference's box(x0, y0, x0 - 40, y0 + 40) does extend to the LEFT of
x0.  A point takes the lowest code among the cells that hold it (the reference keeps "the first" of an sjoin whose order it
does not define); -1 for a point with a coordinate that is not finite.  plots = len(xs) * len(ys).
"buffer" (buffer_plots, :56-67): the reference gives, for stem i in row order, the number i to every stem within its 40 m
buffer, later ones overwriting earlier ones, so code[j] = max{i : d2(i, j) <= cell * cell} with d2 = (xi - xj) * (xi - xj) +
(yi - yj) * (yi - yj), every product and sum rounded on its own (no fused multiply-add); -1 for a stem with a coordinate that is
not finite.  plots = n; n <= 65,536 (every pair is compared).
Two deviations from the reference: shapely's buffer(40) is a 64-gon, not a disc, so a stem between about 39.95 m and 40 m
from another can fall on the other side (its vertices are not reproducible arithmetic: the disc is the rule); and the
reference joins whole geometries with the grid, where a caller with polygons passes centroids here.
`format`'s last step, CHM.filter_CHM, is canopy.CanopyRaster.crown_height(..., rule=HeightRules(...)).

filter_np and plots_np are the definitions; FieldTable.filter and megaplot_plots equal them bit for bit on the device.
Out of scope: reading anything but pandas.read_csv, the BLAN reprojection, TreeData's samples_from_other_sites cap."""
import collections
import math
import re

import numpy as np

COORDS, GROWTH, LIVE, SHADED, SUNNY, TAXON_EXCLUDED = 1, 2, 4, 8, 16, 32          # DTA_FIELD_*
EVENT_DROPPED, MULTIBOLE, KNOWN_ERROR, PLOT_EXCLUDED, SITE_EXCLUDED = 64, 128, 256, 512, 1024
BAD_CODE = 255                                                                    # DTA_FIELD_REASON_BAD_CODE
REASONS = ("kept", "no coordinates", "growth form", "plant status", "shaded individual", "height", "stem diameter",
           "taxon excluded", "event excluded", "not the individual's record", "multibole", "known error", "plot excluded",
           "site excluded")
GRID, BUFFER = 0, 1                                                               # DTA_MEGAPLOT_*
BUFFER_MAX = 65536                                                                # DTA_MEGAPLOT_BUFFER_MAX
AUTO_GRID_ABOVE = 1000                                                            # megaplot.format: shape[0] > 1000
_PAIRS = 1 << 22                 # pairs plots_np looks at in one step: bounded temporaries
_COLUMNS = ("individual", "event", "height", "diameter", "flags")
_NEEDED = ("individualID", "eventID", "itcEasting", "growthForm", "plantStatus", "canopyPosition", "height", "stemDiameter",
           "taxonID", "plotID", "siteID")


class Rules(collections.namedtuple("Rules", "growth_excluded status_contains shaded sunny remap taxa_excluded event_excluded "
                                            "multibole known_errors plots_excluded sites_excluded")):
    """The lists filter_data carries in its text, as settings: data, not logic.  remap: ((from, to), ...), applied in order."""
    __slots__ = ()

    @classmethod
    def reference(cls):
        return cls(
            growth_excluded=("liana", "small shrub"), status_contains="Live", shaded=("Full shade", "Mostly shaded"),
            sunny=("Open grown", "Full sun"),
            remap=(("PSMEM", "PSME"), ("BEPAP", "BEPA"), ("ACNEN", "ACNE2"), ("ACRUR", "ACRU"), ("PICOL", "PICO"),
                   ("ABLAL", "ABLA"), ("ACSA3", "ACSAS"), ("CECAC", "CECA4"), ("PRSES", "PRSE2"), ("PIPOS", "PIPO"),
                   ("BEPAC2", "BEPA"), ("JUVIV", "JUVI"), ("PRPEP", "PRPE2"), ("COCOC", "COCO6"), ("NYBI", "NYSY")),
            taxa_excluded=("BETUL", "FRAXI", "HALES", "PICEA", "PINUS", "QUERC", "ULMUS", "2PLANT"), event_excluded="2014",
            multibole="[A-Z]$",
            known_errors=("NEON.PLA.D03.OSBS.03422", "NEON.PLA.D03.OSBS.03422", "NEON.PLA.D03.OSBS.03382",
                          "NEON.PLA.D17.TEAK.01883"),
            plots_excluded=("SOAP_054", "OSBS_026", "OSBS_029", "OSBS_039", "OSBS_027", "OSBS_036"),
            sites_excluded=("PUUM", "ORNL"))

    def as_lists(self):
        """The rules as plain lists and strings (what tests/golden/field records)."""
        return {k: [list(p) for p in v] if k == "remap" else (v if isinstance(v, str) else list(v))
                for k, v in self._asdict().items()}

    def remapped(self, taxon):
        """The taxon column (an object array) after the subspecies remaps, in order."""
        out = np.array(taxon, dtype=object)
        for old, new in self.remap:
            out[out == old] = new
        return out


class Filtered:
    """keep uint8 [N], reason uint8 [N], rows int64 [N] (the kept rows in output order, then -1), count int64: host arrays
    from filter_np, tensors on the device from FieldTable.filter."""

    def __init__(self, keep, reason, rows, count, rules=None):
        self.keep, self.reason, self.rows, self.count, self.rules = keep, reason, rows, count, rules

    def __iter__(self):
        return iter((self.keep, self.reason, self.rows, self.count))

    def index(self):
        """rows[:count] on the host (the one read of a device result)."""
        rows = self.rows.cpu().numpy() if hasattr(self.rows, "cpu") else np.asarray(self.rows)
        return rows[:int((rows >= 0).sum())]

    def frame(self, df):
        """df.iloc[rows[:count]] with the remapped `taxonID` and the `individual` column: what filter_data returns."""
        rules = self.rules if self.rules is not None else Rules.reference()
        out = df.iloc[self.index()].copy()
        out["individual"] = out["individualID"]
        out["taxonID"] = rules.remapped(out["taxonID"].to_numpy(dtype=object))
        return out


def _threshold(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("{} must be a number, got {!r}".format(what, v))
    if math.isnan(v):
        raise ValueError("{} must be a number, got NaN".format(what))
    return v


def _columns(columns):
    """The five columns as contiguous host arrays of their types, and the number of individuals."""
    if not isinstance(columns, dict) or any(k not in columns for k in _COLUMNS):
        raise ValueError("columns must be a dict with " + ", ".join(_COLUMNS))
    c = {k: np.asarray(columns[k]) for k in _COLUMNS}
    n = len(c["individual"])
    kinds = {"individual": "iu", "event": "iu", "height": "f", "diameter": "f", "flags": "iu"}
    for k in _COLUMNS:
        if c[k].ndim != 1 or len(c[k]) != n or c[k].dtype.kind not in kinds[k] or (kinds[k] == "f" and c[k].dtype != np.float64):
            raise ValueError("column {!r} must be a one-dimensional {} array of {} rows".format(
                k, "float64" if kinds[k] == "f" else "integer", n))
    if not 1 <= n < 2 ** 31:
        raise ValueError("a field table has 1 .. 2^31 - 1 rows, got {}".format(n))
    for k in ("individual", "event"):
        if c[k].min() < -2 ** 31 or c[k].max() >= 2 ** 31:
            raise ValueError("column {!r} must fit 32 bits".format(k))
    if c["flags"].min() < 0 or c["flags"].max() >= 2 ** 16:
        raise ValueError("column 'flags' must fit 16 bits")
    out = {"individual": np.ascontiguousarray(c["individual"], np.int32), "event": np.ascontiguousarray(c["event"], np.int32),
           "height": np.ascontiguousarray(c["height"]), "diameter": np.ascontiguousarray(c["diameter"]),
           "flags": np.ascontiguousarray(c["flags"], np.uint16)}
    individuals = columns.get("individuals")
    if individuals is None:
        individuals = max(1, int(out["individual"].max()) + 1)
    if isinstance(individuals, (bool, np.bool_)) or not isinstance(individuals, (int, np.integer)) or not 1 <= individuals <= n:
        raise ValueError("individuals must be an integer in 1 .. rows, got {!r}".format(individuals))
    return out, int(individuals)


def filter_np(columns, min_stem_diameter, min_height=3.0):
    """The definition (see the module's text) on the integer and float columns: Filtered of host arrays.  columns: a dict
    with individual, event, height, diameter, flags and optionally `individuals` (default: the largest code + 1)."""
    c, I = _columns(columns)
    min_d, min_h = _threshold(min_stem_diameter, "min_stem_diameter"), _threshold(min_height, "min_height")
    ind, ev, h, d, f = (c[k] for k in _COLUMNS)
    N = len(ind)
    reason = np.zeros(N, np.uint8)
    reason[(ind < 0) | (ind >= I) | (ev < 0)] = BAD_CODE
    who = np.clip(ind, 0, I - 1).astype(np.int64)

    def drop(mask, step):
        reason[(reason == 0) & mask] = step

    def per_individual(rows, value, fill, better):
        """better.at over the rows' individuals, and the lowest of the rows that reach it (N: none)."""
        best = np.full(I, fill, value.dtype)
        better.at(best, who[rows], value[rows])
        at = rows[value[rows] == best[who[rows]]]
        first = np.full(I, N, np.int64)
        np.minimum.at(first, who[at], at)
        return first

    drop(f & COORDS == 0, 1)
    drop(f & GROWTH == 0, 2)
    drop(f & LIVE == 0, 3)
    passed = reason == 0
    shaded, sunny = np.zeros(I, bool), np.zeros(I, bool)
    shaded[who[passed & (f & SHADED != 0)]] = True
    sunny[who[passed & (f & SUNNY != 0)]] = True
    drop((shaded & ~sunny)[who], 4)
    with np.errstate(invalid="ignore"):
        drop(~((h > min_h) | np.isnan(h)), 5)
        drop(~(d > min_d), 6)
    drop(f & TAXON_EXCLUDED != 0, 7)
    drop(f & EVENT_DROPPED != 0, 8)
    alive = np.flatnonzero(reason == 0)
    measured = alive[~np.isnan(h[alive])]
    by_height = per_individual(measured, h, -np.inf, np.maximum)
    has = by_height < N
    rest = alive[np.isnan(h[alive]) & ~has[who[alive]]]
    by_event = per_individual(rest, ev.astype(np.int64), -1, np.maximum)
    record = np.where(has, by_height, by_event)
    reason[alive[record[who[alive]] != alive]] = 9
    drop(f & MULTIBOLE != 0, 10)
    drop(f & KNOWN_ERROR != 0, 11)
    drop(f & PLOT_EXCLUDED != 0, 12)
    drop(f & SITE_EXCLUDED != 0, 13)
    keep = reason == 0
    rows = np.full(N, -1, np.int64)
    kept = [r[(r < N) & keep[np.minimum(r, N - 1)]] for r in (np.where(has, by_height, N), np.where(has, N, by_event))]
    out = np.concatenate(kept)
    rows[:len(out)] = out
    return Filtered(keep.astype(np.uint8), reason, rows, np.int64(len(out)))


_NO_DEVICE = "deeptreeattention_amd.field runs its device route on a ROCm device only (device=None runs the definition)"


def _device(device):
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(_NO_DEVICE)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class FieldTable:
    """The integer and float columns of a field table (see the module's text), on the host and -- with a device -- resident.
    columns: the dict filter_np takes."""

    def __init__(self, columns, rules=None, device=None):
        self.columns, self.individuals = _columns(columns)
        self.rows = len(self.columns["individual"])
        self.rules = rules if rules is not None else Rules.reference()
        self.device, self.tensors, self.errors = None, None, None
        if device is not None:
            import torch
            self.device = _device(device)
            self.tensors = {k: torch.from_numpy(self.columns[k].view(np.int16) if k == "flags" else self.columns[k]).to(self.device)
                             for k in _COLUMNS}

    @classmethod
    def resident(cls, individual, event, height, diameter, flags, individuals, rules=None):
        """Columns that already live on the device, taken as they are (no copy, no look at their values: codes out of
        range are the kernel's to count): contiguous int32 [N] individual and event, float64 [N] height and diameter, int16
        or uint16 [N] flags, on one device."""
        import torch
        t = dict(zip(_COLUMNS, (individual, event, height, diameter, flags)))
        want = {"individual": (torch.int32,), "event": (torch.int32,), "height": (torch.float64,), "diameter": (torch.float64,),
                "flags": (torch.int16, getattr(torch, "uint16", torch.int16))}
        ok = all(isinstance(v, torch.Tensor) and v.is_contiguous() and v.dim() == 1 and v.dtype in want[k] for k, v in t.items())
        if not ok or len({tuple(v.shape) for v in t.values()}) != 1 or len({v.device for v in t.values()}) != 1:
            raise ValueError("resident() takes contiguous one-dimensional tensors of one length on one device: int32 individual "
                             "and event, float64 height and diameter, int16 / uint16 flags")
        n = int(individual.shape[0])
        if not 1 <= n < 2 ** 31:
            raise ValueError("a field table has 1 .. 2^31 - 1 rows, got {}".format(n))
        if isinstance(individuals, (bool, np.bool_)) or not isinstance(individuals, (int, np.integer)) or not 1 <= individuals <= n:
            raise ValueError("individuals must be an integer in 1 .. rows, got {!r}".format(individuals))
        self = cls.__new__(cls)
        self.columns, self.individuals, self.rows = None, int(individuals), n
        self.rules = rules if rules is not None else Rules.reference()
        self.device, self.tensors, self.errors = _device(individual.device), t, None
        return self

    @classmethod
    def from_frame(cls, df, rules=None, device=None):
        """The string work, once: codes and flag bits from a pandas frame of the raw NEON table."""
        rules = rules if rules is not None else Rules.reference()
        missing = [k for k in _NEEDED if k not in df.columns]
        if missing:
            raise ValueError("the field table lacks the columns " + ", ".join(missing))
        if len(df) < 1:
            raise ValueError("the field table is empty")

        def col(name):
            return df[name].to_numpy(dtype=object)

        def null(a):
            return np.array([v is None or v != v for v in a], bool)

        def among(a, names):
            return np.isin(a.astype(str), list(names)) & ~null(a)

        def holds(a, what):
            return np.array([isinstance(v, str) and what in v for v in a], bool)

        who, event = col("individualID"), col("eventID")
        if null(who).any():
            raise ValueError("individualID must not be null (row {})".format(int(np.flatnonzero(null(who))[0])))
        if null(event).any():
            raise ValueError("eventID must not be null (row {})".format(int(np.flatnonzero(null(event))[0])))
        site = col("siteID")
        if "utmZone" in df.columns and (among(site, ("BLAN",)) & among(col("utmZone"), ("18N",))).any():
            raise ValueError("rows of BLAN in UTM zone 18N need the reference's reprojection to 17N (pyproj), which is out of "
                             "scope: reproject or drop them first")
        growth, status, canopy = col("growthForm"), col("plantStatus"), col("canopyPosition")
        multibole = re.compile(rules.multibole)
        flags = np.zeros(len(df), np.uint16)
        for bit, mask in ((COORDS, ~null(col("itcEasting"))), (GROWTH, ~null(growth) & ~among(growth, rules.growth_excluded)),
                          (LIVE, holds(status, rules.status_contains)), (SHADED, among(canopy, rules.shaded)),
                          (SUNNY, among(canopy, rules.sunny)),
                          (TAXON_EXCLUDED, among(rules.remapped(col("taxonID")), rules.taxa_excluded)),
                          (EVENT_DROPPED, holds(event, rules.event_excluded)),
                          (MULTIBOLE, np.array([multibole.search(str(v)) is not None for v in who], bool)),
                          (KNOWN_ERROR, among(who, rules.known_errors)), (PLOT_EXCLUDED, among(col("plotID"), rules.plots_excluded)),
                          (SITE_EXCLUDED, among(site, rules.sites_excluded))):
            flags[mask] |= np.uint16(bit)
        names, codes = np.unique(who.astype(str), return_inverse=True)
        _, events = np.unique(event.astype(str), return_inverse=True)
        columns = {"individual": codes.astype(np.int32), "event": events.astype(np.int32),
                   "height": df["height"].to_numpy(dtype=np.float64, na_value=np.nan),
                   "diameter": df["stemDiameter"].to_numpy(dtype=np.float64, na_value=np.nan), "flags": flags,
                   "individuals": len(names)}
        return cls(columns, rules, device)

    def filter(self, min_stem_diameter, min_height=3.0):
        """filter_np on the resident columns: Filtered of tensors, one launch chain on the current stream, nothing waits for
        it.  A table without a device runs the definition."""
        min_d, min_h = _threshold(min_stem_diameter, "min_stem_diameter"), _threshold(min_height, "min_height")
        if self.tensors is None:
            out = filter_np(dict(self.columns, individuals=self.individuals), min_d, min_h)
            out.rules = self.rules
            return out
        import torch
        from . import _lib
        L, dev, N = _lib.lib(), self.device, self.rows
        need = int(L.dta_field_workspace_bytes(N, self.individuals))
        if need == 0:
            raise ValueError("sizes out of range: {} rows, {} individuals".format(N, self.individuals))
        keep = torch.empty(N, dtype=torch.uint8, device=dev)
        reason = torch.empty(N, dtype=torch.uint8, device=dev)
        rows = torch.empty(N, dtype=torch.int64, device=dev)
        count = torch.empty((), dtype=torch.int64, device=dev)
        self.errors = torch.empty((), dtype=torch.int32, device=dev)
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        t = self.tensors
        _lib.check(L.dta_field_filter(_lib.ptr(t["individual"]), _lib.ptr(t["event"]), _lib.ptr(t["height"]), _lib.ptr(t["diameter"]),
                                      _lib.ptr(t["flags"]), N, self.individuals, min_d, min_h, _lib.ptr(keep), _lib.ptr(reason),
                                      _lib.ptr(rows), _lib.ptr(count), _lib.ptr(self.errors), _lib.ptr(workspace), need,
                                      _lib.current_stream_ptr()), "dta_field_filter")
        return Filtered(keep, reason, rows, count, self.rules)


def filter_data(df_or_path, config, device=None, rules=None):
    """The reference's whole filter_data: a frame (or the path of a CSV) in, the surviving rows out, in its order, with the
    remapped taxonID and the `individual` column.  device=None runs the definition, so it works without a GPU."""
    import pandas as pd
    df = pd.read_csv(df_or_path) if isinstance(df_or_path, (str, bytes)) or hasattr(df_or_path, "__fspath__") else df_or_path
    table = FieldTable.from_frame(df, rules, device)
    return table.filter(config["min_stem_diameter"]).frame(df)


# ---------------------------------------------------------------------------------------------------------------------
# megaplot.format: a plot code per stem
# ---------------------------------------------------------------------------------------------------------------------
Plots = collections.namedtuple("Plots", "code plots")
Plots.__doc__ = """code int32 [n] (-1: a coordinate that is not finite, or no cell holds the point); plots: the number of plot
codes (len(xs) * len(ys) for the grid rule, n for the buffer rule)."""

_POINTS = "points must be a non-empty float64 [n, 2] array of (x, y)"


def _cell(cell):
    try:
        cell = float(cell)
    except (TypeError, ValueError):
        raise ValueError("cell must be a finite number above 0, got {!r}".format(cell))
    if not math.isfinite(cell) or cell <= 0 or not math.isfinite(cell * cell):
        raise ValueError("cell must be a finite number above 0, got {!r}".format(cell))
    return cell


def _rule(rule, n):
    if rule == "auto":
        rule = "grid" if n > AUTO_GRID_ABOVE else "buffer"
    if rule not in ("grid", "buffer"):
        raise ValueError("rule must be 'auto', 'grid' or 'buffer', got {!r}".format(rule))
    if rule == "buffer" and n > BUFFER_MAX:
        raise ValueError("the buffer rule compares every pair: at most {} stems, got {}".format(BUFFER_MAX, n))
    return rule


def _points(points):
    if not (hasattr(points, "shape") and hasattr(points, "dtype")):
        points = np.asarray(points)
    shape, dtype = tuple(points.shape), str(points.dtype).replace("torch.", "")
    if dtype != "float64" or len(shape) != 2 or shape[1] != 2 or not 1 <= shape[0] < 2 ** 31:
        raise ValueError(_POINTS)
    return points


def grid_tables(bounds, cell):
    """xs, ys of create_grid from (xmin, ymin, xmax, ymax): np.arange itself."""
    xmin, ymin, xmax, ymax = (float(v) for v in bounds)
    if not all(math.isfinite(v) for v in (xmin, ymin, xmax, ymax)):
        raise ValueError("no point has finite coordinates: the grid has no bounds")
    if (xmax - xmin) / cell + 2 >= 2 ** 31 or (ymax - ymin) / cell + 2 >= 2 ** 31:
        raise ValueError("the grid has 2^31 cells or more")
    xs, ys = np.arange(xmin, xmax + cell, cell), np.arange(ymin, ymax + cell, cell)
    if len(xs) < 1 or len(ys) < 1 or len(xs) * len(ys) >= 2 ** 31:
        raise ValueError("the grid has {} x {} cells: 1 .. 2^31 - 1 in all".format(len(xs), len(ys)))
    return xs, ys


def _bounds_np(p):
    ok = np.isfinite(p).all(axis=1)
    if not ok.any():
        return (np.nan,) * 4
    return p[ok, 0].min(), p[ok, 1].min(), p[ok, 0].max(), p[ok, 1].max()


def plots_np(points, rule="auto", cell=40.0):
    """The definition of both rules (see the module's text): Plots of a host array."""
    from .boundary import _host
    p = np.asarray(_host(_points(points)))
    n, cell = len(p), _cell(cell)
    rule = _rule(rule, n)
    x, y = p[:, 0], p[:, 1]
    ok = np.isfinite(x) & np.isfinite(y)
    code = np.full(n, -1, np.int32)
    if rule == "grid":
        xs, ys = grid_tables(_bounds_np(p), cell)
        # the lowest i with x <= xs[i], then its lower bound; the lowest j with y <= ys[j] + cell, then its lower bound:
        # both bounds ascend with the index, so a lowest candidate that fails leaves none
        left, top = xs - cell, ys + cell
        i = np.minimum(np.searchsorted(xs, x[ok], "left"), len(xs) - 1)
        j = np.minimum(np.searchsorted(top, y[ok], "left"), len(ys) - 1)
        inside = (left[i] <= x[ok]) & (x[ok] <= xs[i]) & (ys[j] <= y[ok]) & (y[ok] <= top[j])
        code[ok] = np.where(inside, i * len(ys) + j, -1)
        return Plots(code, len(xs) * len(ys))
    r2 = cell * cell
    block = max(1, _PAIRS // n)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, n, block):
            dx, dy = x[None, :] - x[s:s + block, None], y[None, :] - y[s:s + block, None]
            within = dx * dx + dy * dy <= r2
            code[s:s + block] = np.where(within.any(axis=1), n - 1 - np.argmax(within[:, ::-1], axis=1), -1)
    return Plots(code, n)


def megaplot_plots(points, rule="auto", cell=40.0, device="cuda"):
    """plots_np on the device: Plots(code int32 [n] tensor, plots).  points: float64 [n, 2], a host array or a resident
    tensor (then on its device).  The grid rule reads the four bounds of resident points back to build xs and ys with
    np.arange; nothing else waits.  device=None runs the definition."""
    points = _points(points)
    n, cell = int(points.shape[0]), _cell(cell)
    rule = _rule(rule, n)
    if device is None:
        return plots_np(points, rule, cell)
    import torch
    from . import _lib
    tables = None
    if isinstance(points, torch.Tensor) and points.device.type != "cpu":
        dev = _device(points.device)
        p = points.contiguous()
        if rule == "grid":
            ok = torch.isfinite(p).all(dim=1, keepdim=True)
            lo = torch.where(ok, p, torch.full_like(p, math.inf)).amin(dim=0)
            hi = torch.where(ok, p, torch.full_like(p, -math.inf)).amax(dim=0)
            b = torch.cat([lo, hi]).cpu().numpy()                                     # the one read-back
            tables = grid_tables(tuple(b) if np.isfinite(b).all() else (np.nan,) * 4, cell)
    else:
        host = np.ascontiguousarray(points.numpy() if isinstance(points, torch.Tensor) else points)
        if rule == "grid":
            tables = grid_tables(_bounds_np(host), cell)
        dev = _device(device)
        p = torch.from_numpy(host).to(dev)
    which, tx, nx, ty, ny, plots = BUFFER, None, 0, None, 0, n
    if tables is not None:
        xs, ys = tables
        which, tx, nx, ty, ny, plots = GRID, torch.from_numpy(xs).to(dev), len(xs), torch.from_numpy(ys).to(dev), len(ys), len(xs) * len(ys)
    code = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dta_megaplot_plots(_lib.ptr(p), n, which, cell, _lib.ptr(tx), nx, _lib.ptr(ty), ny, _lib.ptr(code),
                                             _lib.current_stream_ptr()), "dta_megaplot_plots")
    return Plots(code, plots)


def plot_names(code, filename, rule):
    """The reference's plotID strings: "{code}_contrib" (create_grid) or "{filename}_contrib_{code}" (buffer_plots)."""
    if rule not in ("grid", "buffer"):
        raise ValueError("rule must be 'grid' or 'buffer', got {!r}".format(rule))
    code = code.cpu().numpy() if hasattr(code, "cpu") else np.asarray(code)
    if rule == "grid":
        return ["{}_contrib".format(int(c)) for c in code]
    return ["{}_contrib_{}".format(filename, int(c)) for c in code]
