"""Site boundary clip: which crowns, points and raster cells lie inside the site's boundary polygon -- the step in front of
every count the reference publishes (abundance.py:24-35, create_prediction_shp.py:33-41, src/multinomial.py:16-19:
`gpd.clip(crowns, boundary)` with the site's boundary shapefile, one geometry object per crown on the host).  Here the
boundary is one resident edge table and one launch decides all crowns of a tile (dta_boundary_boxes, csrc/boundary.hip); the
result is the third factor of `mask = keep & alive & inside` that abundance.counts / abundance.resample accept, next to
canopy's `keep` and dead's `alive`.  `rasterise` gives the same decision per raster cell, to blank a predict_map* result.

The region is the even-odd interior of all rings together (for a valid (Multi)Polygon: the polygon with its holes).  The host
turns the rings into one edge table [E][4] float64 (ax, ay, bx, by) with the origin org = (min x, min y) subtracted once;
queries have org subtracted first.  All arithmetic is float64, every product and every difference rounded on its own (no
fused multiply-add, no division).

A point p against edge k:
    straddle = (ay > py) != (by > py);  dx = bx - ax;  dy = by - ay
    l = (px - ax) * dy;  r = (py - ay) * dx;  left = l < r if dy > 0 else l > r
    inside = the parity of (straddle & left) over all edges;  a NaN coordinate gives 0
Points exactly on the boundary line follow from this rule and nothing more is promised (of a square, the left and the
bottom side are in, the right and the top side out).

A box (x0, y0, x1, y1):
    code 0 if a coordinate (after org is subtracted) is not finite, or x1 < x0, or y1 < y0
    edge k touches the filled rectangle unless both of its ends are on the outer side of one of the four box sides
    (ax < x0 and bx < x0, ...), or the four corner signs s(c) = dx * (cy - ay) - dy * (cx - ax) are all > 0, or all < 0
    (the separating-axis test of a segment and a rectangle)
    code = 1 if any edge touches, else 2 if (x0, y0) is inside, else 0
so 0 is disjoint, 1 touches or crosses the boundary line, 2 lies entirely inside; `clip` is code != 0: the closed box and the
closed region share a point, this package's reading of "gpd.clip keeps the row".  A corner test alone is wrong: a spike of
the boundary can cross a box whose four corners are inside.

A pixel box is (row0, col0, row1, col1), half-open, as everywhere in dense.py; with the north-up transform (x0, a, y0, e)
(rasterio's Affine(a, 0, x0, 0, e, y0), e usually negative) its corners are x = x0 + col * a, y = y0 + row * e, then min / max
per axis (geo_boxes).  A raster cell (r, c) is the point (x0 + (c + .5) * a, y0 + (r + .5) * e).

The NumPy functions are the definition (as canopy.crown_height_np and abundance.resample_np are); the device route equals
them bit for bit.  The reference's share of this stage is the single call gpd.clip, and geopandas is not a dependency of this
package: there is no recorded fixture; tests/test_boundary_cpu.py holds the definition to matplotlib's Path instead.
Out of scope: the clipped geometry or area of a crown, curved or geodesic edges, reprojection, reading shapefiles.
"""
import collections

import numpy as np

EDGE_CHUNK = 1024                # DTA_BOUNDARY_EDGE_CHUNK: edges staged through LDS at a time
MAX_EDGES = 1 << 20              # DTA_BOUNDARY_MAX_EDGES

EdgeTable = collections.namedtuple("EdgeTable", "edges org")
EdgeTable.__doc__ = "edges: float64 [E][4] (ax, ay, bx, by) with org subtracted; org: float64 [2] (min x, min y)."


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def edge_table(rings):
    """The EdgeTable of a list of [K, 2] rings (x, y): exterior rings and holes of all parts, in any orientation, closed
    (last vertex == first) or not.  Zero-length edges are dropped; org is subtracted once, in float64."""
    if isinstance(rings, np.ndarray) and rings.ndim == 2:
        rings = [rings]
    verts = []
    for ring in rings:
        v = np.asarray(_host(ring))
        if v.ndim != 2 or v.shape[1] != 2 or v.dtype.kind not in "fiu":
            raise ValueError("every ring must be a [K, 2] array of (x, y)")
        v = v.astype(np.float64)
        if not np.isfinite(v).all():
            raise ValueError("a ring has a coordinate that is not finite")
        if len(v) > 1 and (v[0] == v[-1]).all():
            v = v[:-1]
        if len(v) < 3:
            raise ValueError("every ring needs at least 3 distinct vertices")
        verts.append(v)
    if not verts:
        raise ValueError("rings is empty")
    org = np.concatenate(verts).min(axis=0)
    parts = []
    for v in verts:
        a = v - org                                            # one rounding per coordinate
        parts.append(np.concatenate([a, np.roll(a, -1, axis=0)], axis=1))
    edges = np.concatenate(parts)
    edges = np.ascontiguousarray(edges[(edges[:, 0] != edges[:, 2]) | (edges[:, 1] != edges[:, 3])])
    if not 3 <= len(edges) <= MAX_EDGES:
        raise ValueError("the boundary has {} edges: 3 .. 2^20 are supported".format(len(edges)))
    return EdgeTable(edges, org)


def geojson_rings(mapping):
    """The rings of a GeoJSON-like `Polygon` / `MultiPolygon` mapping (a `__geo_interface__` dict, or an object that has
    one): every exterior ring and every hole of every part, as a list of float64 [K, 2] arrays (a z coordinate is ignored)."""
    mapping = getattr(mapping, "__geo_interface__", mapping)
    kind = mapping.get("type") if hasattr(mapping, "get") else None
    if kind == "Polygon":
        polygons = [mapping["coordinates"]]
    elif kind == "MultiPolygon":
        polygons = list(mapping["coordinates"])
    else:
        raise ValueError("from_geojson takes a Polygon or MultiPolygon mapping, got type {!r}".format(kind))
    rings = [np.asarray(ring, np.float64)[:, :2] for polygon in polygons for ring in polygon]
    if not rings:
        raise ValueError("the geometry is empty")
    return rings


def _table(boundary):
    if isinstance(boundary, EdgeTable):
        return boundary
    if isinstance(boundary, Boundary):
        return boundary.table
    return edge_table(boundary)


def _transform(transform):
    t = np.asarray(transform, np.float64).reshape(-1)
    if t.shape != (4,) or not np.isfinite(t).all():
        raise ValueError("transform must be four finite numbers (x0, a, y0, e): rasterio's Affine(a, 0, x0, 0, e, y0)")
    if t[1] == 0 or t[3] == 0:
        raise ValueError("transform has a pixel size of 0: a={!r} e={!r}".format(t[1], t[3]))
    return t


def _host_points(points):
    p = np.asarray(_host(points))
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.dtype != np.float64:
        raise ValueError("points must be a non-empty float64 [N, 2] array of (x, y)")
    return p


def _host_geo(boxes):
    b = np.asarray(_host(boxes))
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.dtype != np.float64:
        raise ValueError("geo_boxes must be a non-empty float64 [N, 4] array of (x0, y0, x1, y1)")
    return b


def _host_pixel(boxes):
    b = np.asarray(_host(boxes))
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.dtype.kind not in "iu":
        raise ValueError("pixel_boxes must be a non-empty integer [N, 4] array of (row0, col0, row1, col1)")
    if b.size and (b.min() < -2 ** 31 or b.max() > 2 ** 31 - 1):
        raise ValueError("pixel_boxes must fit int32")
    return b.astype(np.int64)


def _which(geo_boxes, pixel_boxes, transform):
    if (geo_boxes is None) == (pixel_boxes is None):
        raise ValueError("exactly one of geo_boxes and pixel_boxes must be given")
    if pixel_boxes is not None and transform is None:
        raise ValueError("pixel_boxes need a transform (x0, a, y0, e)")
    if geo_boxes is not None and transform is not None:
        raise ValueError("geo_boxes take no transform")


def geo_boxes(pixel_boxes, transform):
    """float64 [N, 4] (x0, y0, x1, y1) of the pixel boxes (row0, col0, row1, col1) under the north-up transform
    (x0, a, y0, e): x = x0 + col * a, y = y0 + row * e, the product and the sum rounded one by one, then min / max per axis.
    This is what the device computes from pixel boxes."""
    b = _host_pixel(pixel_boxes).astype(np.float64)            # exact: |value| < 2^31
    x0, a, y0, e = _transform(transform)
    xa, xb = x0 + b[:, 1] * a, x0 + b[:, 3] * a
    ya, yb = y0 + b[:, 0] * e, y0 + b[:, 2] * e
    return np.stack([np.minimum(xa, xb), np.minimum(ya, yb), np.maximum(xa, xb), np.maximum(ya, yb)], axis=1)


_geo_boxes = geo_boxes           # (boxes_np and Boundary.boxes have an argument of that name)


def _crossings(edges, px, py, step=1 << 22):
    """bool [N]: the parity rule for points (px, py) that already have org subtracted."""
    inside = np.zeros(len(px), bool)
    block = max(1, step // max(len(px), 1))                    # edges per step: bounded temporaries
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, len(edges), block):
            ax, ay, bx, by = (edges[k:k + block, j][:, None] for j in range(4))
            dx, dy = bx - ax, by - ay
            straddle = (ay > py) != (by > py)
            l = (px - ax) * dy
            r = (py - ay) * dx
            left = np.where(dy > 0, l < r, l > r)
            inside ^= np.logical_xor.reduce(straddle & left, axis=0)
    return inside


def contains_np(boundary, points):
    """The definition: uint8 [N], 1 where the point (x, y) is inside.  boundary: a Boundary, an EdgeTable or a list of rings."""
    t = _table(boundary)
    p = _host_points(points)
    return _crossings(t.edges, p[:, 0] - t.org[0], p[:, 1] - t.org[1]).astype(np.uint8)


def boxes_np(boundary, geo_boxes=None, pixel_boxes=None, transform=None, step=1 << 22):
    """The definition: uint8 [N] codes, 0 disjoint, 1 touches or crosses the boundary line, 2 entirely inside."""
    _which(geo_boxes, pixel_boxes, transform)
    t = _table(boundary)
    b = _host_geo(geo_boxes) if geo_boxes is not None else _geo_boxes(pixel_boxes, transform)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, x1 = b[:, 0] - t.org[0], b[:, 2] - t.org[0]
        y0, y1 = b[:, 1] - t.org[1], b[:, 3] - t.org[1]
        valid = np.isfinite(x0) & np.isfinite(y0) & np.isfinite(x1) & np.isfinite(y1) & ~(x1 < x0) & ~(y1 < y0)
        touch = np.zeros(len(b), bool)
        block = max(1, step // len(b))
        for k in range(0, len(t.edges), block):
            ax, ay, bx, by = (t.edges[k:k + block, j][:, None] for j in range(4))
            dx, dy = bx - ax, by - ay
            outer = ((ax < x0) & (bx < x0)) | ((ax > x1) & (bx > x1)) | ((ay < y0) & (by < y0)) | ((ay > y1) & (by > y1))
            p0, p1 = dx * (y0 - ay), dx * (y1 - ay)
            q0, q1 = dy * (x0 - ax), dy * (x1 - ax)
            s00, s10, s11, s01 = p0 - q0, p0 - q1, p1 - q1, p1 - q0      # corners (x0,y0) (x1,y0) (x1,y1) (x0,y1)
            pos = (s00 > 0) & (s10 > 0) & (s11 > 0) & (s01 > 0)
            neg = (s00 < 0) & (s10 < 0) & (s11 < 0) & (s01 < 0)
            touch |= (~(outer | pos | neg)).any(axis=0)
        inside = _crossings(t.edges, x0, y0)
    return np.where(valid, np.where(touch, 1, np.where(inside, 2, 0)), 0).astype(np.uint8)


def cell_centres(height, width, transform):
    """float64 [H * W, 2]: the centre (x0 + (c + .5) * a, y0 + (r + .5) * e) of every cell, row-major."""
    height, width = int(height), int(width)
    if height < 1 or width < 1 or height * width > 0x7FFFFFFF:
        raise ValueError("height and width must be >= 1 and height * width at most 2^31 - 1")
    x0, a, y0, e = _transform(transform)
    x = x0 + (np.arange(width, dtype=np.float64) + 0.5) * a
    y = y0 + (np.arange(height, dtype=np.float64) + 0.5) * e
    return np.stack([np.broadcast_to(x, (height, width)), np.broadcast_to(y[:, None], (height, width))], axis=2).reshape(-1, 2)


def rasterise_np(boundary, height, width, transform):
    """The definition: uint8 [H][W], 1 where the cell's centre is inside."""
    return contains_np(boundary, cell_centres(height, width, transform)).reshape(int(height), int(width))


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
_NO_DEVICE = "deeptreeattention_amd.boundary runs on a ROCm device only (no CPU fallback)"


class Boundary:
    """A site boundary, its edge table uploaded once (float64 [E][4], E * 32 bytes).  rings: see edge_table."""

    def __init__(self, rings, device="cuda"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(_NO_DEVICE)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        table = _table(rings)
        self._adopt(table, torch.from_numpy(table.edges).to(dev))

    def _adopt(self, table, edges):
        self.table, self.edges, self.device = table, edges, edges.device
        self.org = table.org
        self.n_edges = int(table.edges.shape[0])

    @classmethod
    def from_geojson(cls, mapping, device="cuda"):
        """A Boundary from a `Polygon` / `MultiPolygon` mapping: shapely's `geom.__geo_interface__`, a GeoJSON geometry, or
        the object itself.  Nothing of geopandas or shapely is imported."""
        return cls(geojson_rings(mapping), device=device)

    @classmethod
    def resident(cls, table, edges):
        """An EdgeTable and its contiguous float64 [E, 4] tensor that already lives on the device, taken as it is."""
        import torch
        if (not isinstance(table, EdgeTable) or not isinstance(edges, torch.Tensor) or edges.dtype != torch.float64
                or tuple(edges.shape) != table.edges.shape or not edges.is_contiguous()):
            raise ValueError("resident() takes an EdgeTable and its contiguous float64 [E, 4] tensor")
        self = cls.__new__(cls)
        self._adopt(table, edges)
        return self

    # what the C entries take: a contiguous tensor of the right dtype on this device
    def _queries(self, a, cols, dtype, what):
        import torch
        if isinstance(a, torch.Tensor):
            wrong = a.dtype != torch.float64 if dtype == torch.float64 else a.dtype.is_floating_point or a.dtype == torch.bool
            if a.dim() != 2 or a.shape[1] != cols or a.shape[0] < 1 or wrong:
                raise ValueError(what)
            if a.device.type == "cpu":
                return self._queries(a.numpy(), cols, dtype, what)
            if a.device != self.device:
                raise ValueError(what + " on " + str(self.device))
            return a.to(dtype).contiguous()
        host = _host_points(a) if cols == 2 else _host_geo(a) if dtype == torch.float64 else _host_pixel(a)
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.float64 if dtype == torch.float64 else np.int32))).to(self.device)

    def _launch(self, call, name, out):
        from . import _lib
        if not self.edges.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        org = (_lib.C.c_double * 2)(*self.org)
        _lib.check(call(_lib.lib(), _lib.ptr(self.edges), self.n_edges, org), name)
        return out

    def contains(self, points):
        """contains_np on the device: uint8 [N], 1 where the point is inside.  points: float64 [N, 2] (x, y) in the rings'
        CRS, a host array or a device tensor.  Nothing here waits for the device."""
        import torch
        from . import _lib
        p = self._queries(points, 2, torch.float64, "points must be a non-empty float64 [N, 2] array of (x, y)")
        out = torch.empty(p.shape[0], dtype=torch.uint8, device=self.device)
        return self._launch(lambda L, e, n, org: L.dta_boundary_points(e, n, org, _lib.ptr(p), p.shape[0], _lib.ptr(out),
                                                                        _lib.current_stream_ptr()), "dta_boundary_points", out)

    def boxes(self, geo_boxes=None, pixel_boxes=None, transform=None):
        """boxes_np on the device: uint8 [N] codes, 0 disjoint, 1 touches or crosses the boundary line, 2 entirely inside.
        Exactly one of geo_boxes (float64 [N, 4] (x0, y0, x1, y1)) and pixel_boxes (integer [N, 4] (row0, col0, row1, col1)
        with transform = (x0, a, y0, e)), host arrays or device tensors.  The pixel form computes geo_boxes() on the device."""
        import torch
        from . import _lib
        _which(geo_boxes, pixel_boxes, transform)
        if geo_boxes is not None:
            g, p, t = self._queries(geo_boxes, 4, torch.float64, "geo_boxes must be a non-empty float64 [N, 4] array of (x0, y0, x1, y1)"), None, None
        else:
            t = (_lib.C.c_double * 4)(*_transform(transform))
            g, p = None, self._queries(pixel_boxes, 4, torch.int32,
                                       "pixel_boxes must be a non-empty integer [N, 4] array of (row0, col0, row1, col1)")
        n = (g if p is None else p).shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._launch(lambda L, e, ne, org: L.dta_boundary_boxes(e, ne, org, _lib.ptr(g), _lib.ptr(p), t, n, _lib.ptr(out),
                                                                        _lib.current_stream_ptr()), "dta_boundary_boxes", out)

    def clip(self, geo_boxes=None, pixel_boxes=None, transform=None):
        """uint8 [N], 1 where boxes() is not 0: the closed box and the closed region share a point ("gpd.clip keeps the
        row").  The mask abundance.counts / abundance.resample take: mask = keep & alive & site.clip(...)."""
        import torch
        return (self.boxes(geo_boxes, pixel_boxes, transform) != 0).view(torch.uint8)

    def rasterise(self, height, width, transform):
        """rasterise_np on the device: uint8 [H][W], 1 where the cell's centre is inside; multiply a predict_map* label
        map by it, or torch.where on it, to blank the cells outside the site."""
        import torch
        from . import _lib
        height, width = int(height), int(width)
        if height < 1 or width < 1 or height * width > 0x7FFFFFFF:
            raise ValueError("height and width must be >= 1 and height * width at most 2^31 - 1")
        t = (_lib.C.c_double * 4)(*_transform(transform))
        if not self.edges.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        out = torch.empty((height, width), dtype=torch.uint8, device=self.device)
        return self._launch(lambda L, e, n, org: L.dta_boundary_raster(e, n, org, height, width, t, _lib.ptr(out),
                                                                        _lib.current_stream_ptr()), "dta_boundary_raster", out)
