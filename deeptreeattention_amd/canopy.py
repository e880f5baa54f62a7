"""Crown height filter: the canopy height of every crown box of a LiDAR canopy-height model (CHM) and the reference's keep
rules on it -- the step in front of the prediction pipeline (src/predict.py:35-42 find_crowns: `postprocess_CHM`, then
`crowns[crowns.CHM_height > 3]`) and of the training data (src/CHM.py:58-106 filter_CHM: the same statistic, then
`height_rules`).

The statistic is src/CHM.py:9-14 `non_zero_99_quantile`: the 99th percentile, linearly interpolated, of the box's CHM cells
that are >= 0.5.  The reference gets it from rasterstats.zonal_stats: one Python call, one raster window read and one
np.nanpercentile per crown.  Here one launch pair (dta_crown_height, csrc/canopy.hip) computes it for all crowns of a tile
from a resident raster and applies the keep rule; the result is the `mask` abundance.counts / abundance.resample accept, and
it indexes the boxes dense.predict_crops* take.

A crown is a pixel box (row0, col0, row1, col1), half-open, as everywhere in dense.py; it is clipped to the raster.
Georeferencing and polygon rasterisation (which cells a polygon owns) stay with the caller, as in dense.py (for the site's
boundary polygon: boundary.Boundary.clip on pixel boxes with the raster's transform, and Boundary.rasterise).

For one crown, with every operation rounded to float32 on its own (np.nanpercentile's arithmetic on float32 input; a fused
multiply-add, a float64 lerp or a float64 `t` do NOT give the reference's bits):
    kept   = the cells v of the clipped box with v >= floor       (drops NaN, a -9999 nodata value, everything under it)
    n      = len(kept);  n == 0: height NaN, count 0
    virt   = float32(n - 1) * (float32(q) / float32(100));  lo = floor(virt);  t = virt - lo;  hi = min(lo + 1, n - 1)
    a, b   = the lo-th and hi-th smallest kept value;  d = b - a
    height = b - d * (1 - t)  if t >= 0.5  else  a + d * t
float32(n - 1) is exact only up to 2^24: a clipped box of more cells is refused.  floor must be > 0: the kernels select on
the bit patterns of the kept values, which order as unsigned integers only for positive floats.

The NumPy functions are the definition (as abundance.resample_np and dense.crown_reduce_np are); the device route equals
them bit for bit.  The tie to the reference is tests/golden/canopy/canopy_reference.npz (tools/make_canopy_golden.py).
"""
import collections

import numpy as np

WAVE_CELLS = 1024                # DTA_CROWN_WAVE_CELLS: up to here a crown is one wave's work, above it a workgroup's
MAX_CELLS = 1 << 24              # float32(n - 1) is exact up to here
BLOCK_GROUPS = 2048              # CH_BLOCK_GRID (csrc/canopy.hip): above this many crowns a workgroup of the block kernel takes a chunk of them

MinHeight = collections.namedtuple("MinHeight", "m", defaults=(3.0,))
MinHeight.__doc__ = "find_crowns' filter: keep iff height > m (a NaN height is dropped)."
HeightRules = collections.namedtuple("HeightRules", "min_chm max_diff limit", defaults=(1.0, 4.0, 8.0))
HeightRules.__doc__ = "src/CHM.py height_rules(min_CHM_height, max_CHM_diff, CHM_height_limit): see height_rules_np."
CrownHeights = collections.namedtuple("CrownHeights", "height count keep")


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _percent(q, floor):
    q32, f32 = np.float32(q), np.float32(floor)
    if not 0 <= q32 <= 100:
        raise ValueError("q must be in [0, 100], got {!r}".format(q))
    if not f32 > 0:
        raise ValueError("floor must be > 0, got {!r}".format(floor))
    return q32, f32


def _host_boxes(boxes):
    b = np.asarray(_host(boxes))
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.dtype.kind not in "iu":
        raise ValueError("boxes must be a non-empty integer [N, 4] array of (row0, col0, row1, col1)")
    return b.astype(np.int64)


def clip_boxes(boxes, height, width):
    """(row0, col0, rows, cols) int64 [N] each: every box's intersection with the raster; rows or cols is 0 for a box that
    misses the raster or has row1 <= row0 / col1 <= col0."""
    b = _host_boxes(boxes)
    r0, c0 = np.maximum(b[:, 0], 0), np.maximum(b[:, 1], 0)
    r1, c1 = np.minimum(b[:, 2], height), np.minimum(b[:, 3], width)
    return r0, c0, np.maximum(r1 - r0, 0), np.maximum(c1 - c0, 0)


def _rank(n, qf):
    virt = np.float32(n - 1) * qf                      # float32 * float32, rounded once
    lo = int(np.floor(virt))
    return lo, min(lo + 1, n - 1), virt - np.float32(lo)


def quantile_of_kept(kept, q=99.0):
    """The height of one crown from its kept values (float32 [n], n >= 1, any order): the module docstring's formula."""
    kept = np.sort(np.asarray(kept, np.float32))
    n = len(kept)
    if n > MAX_CELLS:
        raise ValueError("more than 2^24 values: float32(n - 1) is not exact")
    lo, hi, t = _rank(n, np.float32(q) / np.float32(100))
    a, b = kept[lo], kept[hi]
    with np.errstate(invalid="ignore"):                # +inf cells: inf - inf, inf * 0 are NaN, as in the reference
        d = b - a
        return np.float32(b - d * (np.float32(1) - t)) if t >= np.float32(0.5) else np.float32(a + d * t)


def crown_height_np(chm, boxes, q=99.0, floor=0.5):
    """The definition: (height float32 [N], count int32 [N]) of the crowns `boxes` on the float32 [H][W] raster `chm`."""
    chm = np.asarray(_host(chm))
    if chm.ndim != 2 or chm.size < 1:
        raise ValueError("chm must be a non-empty [H][W] raster")
    chm = chm.astype(np.float32, copy=False)
    q32, f32 = _percent(q, floor)
    r0, c0, rows, cols = clip_boxes(boxes, *chm.shape)
    if (rows * cols > MAX_CELLS).any():
        raise ValueError("a clipped box has more than 2^24 cells")
    height = np.full(len(r0), np.nan, np.float32)
    count = np.zeros(len(r0), np.int32)
    with np.errstate(invalid="ignore"):
        for i in range(len(r0)):
            v = chm[r0[i]:r0[i] + rows[i], c0[i]:c0[i] + cols[i]]
            kept = v[v >= f32]
            count[i] = kept.size
            if kept.size:
                height[i] = quantile_of_kept(kept, q32)
    return height, count


def min_height_np(height, m=3.0):
    """find_crowns' `CHM_height > 3`, in float64 after exact widening: bool [N]; a NaN height is dropped."""
    with np.errstate(invalid="ignore"):
        return np.asarray(_host(height)).astype(np.float64) > float(m)


def height_rules_np(chm_height, field_height, min_chm=1, max_diff=4, limit=8):
    """src/CHM.py:70-90 height_rules, row by row in float64 (pandas hands it float64 rows): bool [N].  In this order:
        CHM is NaN: drop;  the field height h is NaN: keep;  CHM < min_chm: drop;
        CHM > h: drop iff CHM - h >= max_diff;  otherwise: drop iff h - CHM >= limit.
    Equal heights keep; a difference of exactly max_diff / limit drops.  The reference's fillna of a missing field height
    with the CHM height (src/CHM.py:33, for the rows it keeps afterwards) is NOT part of this rule: it is the caller's
    torch.where(field.isnan(), chm_height, field)."""
    c = np.asarray(_host(chm_height)).astype(np.float64).reshape(-1)
    h = np.asarray(_host(field_height)).astype(np.float64).reshape(-1)
    if len(c) != len(h):
        raise ValueError("field_height must have one entry per crown")
    with np.errstate(invalid="ignore"):
        over = ~(c - h >= float(max_diff))
        under = ~(h - c >= float(limit))
        keep = np.where(c > h, over, under)
        keep = np.where(c < float(min_chm), False, keep)
        keep = np.where(np.isnan(h), True, keep)
        return np.where(np.isnan(c), False, keep).astype(bool)


def _rule(rule, field_height):
    """(mode, min_height, min_chm, max_diff, limit) of a MinHeight / HeightRules / None."""
    if rule is None:
        return 0, 0.0, 0.0, 0.0, 0.0
    if isinstance(rule, MinHeight):
        return 1, float(rule.m), 0.0, 0.0, 0.0
    if isinstance(rule, HeightRules):
        if field_height is None:
            raise ValueError("HeightRules needs field_height (one field-measured height per crown, NaN where missing)")
        return 2, 0.0, float(rule.min_chm), float(rule.max_diff), float(rule.limit)
    raise ValueError("rule must be a MinHeight, a HeightRules or None, got {!r}".format(rule))


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
class CanopyRaster:
    """A canopy-height raster [H][W], uploaded once as float32.  Float64 or integer input is converted once on the host.
    The float32 result is the reference's for a float32 CHM, as NEON's CHM GeoTIFFs are; for a float64 raster the
    reference would interpolate in float64 and differ in the last bits."""

    def __init__(self, chm, device="cuda"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("deeptreeattention_amd.canopy runs on a ROCm device only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if isinstance(chm, torch.Tensor) and chm.is_cuda:
            t = chm.to(device=dev, dtype=torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(_host(chm), dtype=np.float32)).to(dev, non_blocking=True)
        self._adopt(t)

    def _adopt(self, t):
        if t.dim() != 2 or t.numel() < 1:
            raise ValueError("chm must be a non-empty [H][W] raster")
        if t.numel() > 0x7FFFFFFF:
            raise ValueError("the raster has more than 2^31 - 1 cells")
        self.data, self.device = t, t.device
        self.height, self.width = int(t.shape[0]), int(t.shape[1])
        self.shape = (self.height, self.width)

    @classmethod
    def resident(cls, chm):
        """A contiguous float32 [H][W] tensor that already lives on the device, taken as it is (no copy)."""
        import torch
        if not isinstance(chm, torch.Tensor) or chm.dtype != torch.float32 or not chm.is_contiguous():
            raise ValueError("resident() takes a contiguous float32 [H][W] tensor")
        self = cls.__new__(cls)
        self._adopt(chm)
        return self

    def _boxes(self, boxes):
        """What DenseRaster.crops accepts -> a contiguous int32 [N, 4] device tensor; host boxes are checked for the 2^24
        limit here, device boxes by the kernel (count -1)."""
        import torch
        what = "boxes must be a non-empty [N, 4] array of (row0, col0, row1, col1)"
        if isinstance(boxes, torch.Tensor):
            o = boxes
            if o.dim() != 2 or o.shape[1] != 4 or o.shape[0] < 1 or o.dtype.is_floating_point:
                raise ValueError(what)
            if not o.is_cuda:
                return self._boxes(o.numpy())
            if o.dtype != torch.int32 or o.device != self.device or not o.is_contiguous():
                o = o.to(device=self.device, dtype=torch.int32).contiguous()
            return o
        host = np.asarray(boxes)
        if host.ndim != 2 or host.shape[1] != 4 or host.shape[0] < 1 or host.dtype.kind not in "iu":
            raise ValueError(what)
        _, _, rows, cols = clip_boxes(host, self.height, self.width)
        if (rows * cols > MAX_CELLS).any():
            raise ValueError("a clipped box has more than 2^24 cells")
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(self.device)

    def _field(self, field_height, n):
        import torch
        what = "field_height must be a float32 / float64 [{}] host array or tensor on {}".format(n, self.device)
        if isinstance(field_height, torch.Tensor):
            f = field_height
            if f.dtype not in (torch.float32, torch.float64) or tuple(f.shape) != (n,):
                raise ValueError(what)
            if f.device.type != "cpu" and f.device != self.device:
                raise ValueError(what)
            return f.to(device=self.device, dtype=torch.float64).contiguous()
        f = np.asarray(field_height)
        if f.dtype not in (np.float32, np.float64) or f.shape != (n,):
            raise ValueError(what)
        return torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(self.device)

    def crown_height(self, boxes, q=99.0, floor=0.5, field_height=None, rule=None):
        """crown_height_np and the rule on the device (dta_crown_height: one launch pair for all crowns):
        CrownHeights(height float32 [N], count int32 [N], keep bool [N] or None), device tensors.

        boxes: [N, 4] (row0, col0, row1, col1), half-open, a host array or a device tensor -- what DenseRaster.crops takes;
        each box is clipped to the raster.  rule: None, MinHeight(m) (find_crowns' filter) or HeightRules(min_chm, max_diff,
        limit) with field_height, a float32 / float64 [N] host array or device tensor (NaN: no field measurement).  keep is
        the mask abundance.counts / abundance.resample take, and boxes[keep] what predict_crops* take.  A clipped box of
        more than 2^24 cells raises ValueError when the boxes are on the host; device boxes are checked by the kernel, which
        gives such a crown count -1, a NaN height and keep False.  Nothing here waits for the device."""
        import torch
        from . import _lib
        q32, f32 = _percent(q, floor)
        o = self._boxes(boxes)
        n = o.shape[0]
        mode, min_height, min_chm, max_diff, limit = _rule(rule, field_height)
        field = self._field(field_height, n) if mode == 2 else None
        height = torch.empty(n, dtype=torch.float32, device=self.device)
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        keep = torch.empty(n, dtype=torch.bool, device=self.device) if mode else None
        if not self.data.is_cuda:
            raise RuntimeError("deeptreeattention_amd.canopy runs on a ROCm device only (no CPU fallback)")
        L = _lib.lib()
        r = _lib.HeightRule(mode, min_height, min_chm, max_diff, limit)
        _lib.check(L.dta_crown_height(_lib.ptr(self.data), self.height, self.width, _lib.ptr(o), n, float(q32), float(f32),
                                      _lib.ptr(field), _lib.C.byref(r) if mode else None, _lib.ptr(height), _lib.ptr(count),
                                      _lib.ptr(keep), _lib.current_stream_ptr()), "dta_crown_height")
        return CrownHeights(height, count, keep)
