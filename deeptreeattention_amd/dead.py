"""Alive/dead crown filter: the RGB crop of every crown box, prepared on the device for the reference's alive/dead classifier,
the classifier's score, and the rule that blanks the species of dead crowns -- the `filter_dead=True` branch of the
reference's prediction (src/predict.py predict_tile; src/models/dead.py).

The reference does it per crown on a CPU worker: utm_dataset.__getitem__ opens the RGB tile with rasterio, reads the crown's
box plus one metre, and runs ToTensor, Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]) and
Resize([224, 224]); predict_dead feeds the crops to AliveDead (a torchvision ResNet-50 with two outputs) and keeps
label = argmax, score = max of softmax(sigmoid(logits)); predict_tile then sets ens_label / ens_score to None where
(dead_label == 1) & (dead_score > config["dead_threshold"]).  Here one launch (dta_rgb_crops, csrc/dead.hip) writes the
crops of all crowns of a batch from a resident uint8 raster, the classifier runs as torch runs it, one small launch
(dta_dead_head) turns its logits into label and score, and filter_dead gives the `alive` mask that abundance.counts /
abundance.resample accept, combined with canopy's `keep` by `&`.

A crown is a pixel box (row0, col0, row1, col1), half-open, as in dense.py and canopy.py; `pad` pixels are added on every side
(10 for the reference's 1 m at 0.1 m per pixel) and the result is clipped to the raster.  Georeferencing stays with the caller.

The definition of a crop (crops_np), every operation in float32, for the clipped box with origin (r0, c0), h rows, w columns:
    p(c, y, x) = (float32(u8[c][r0+y][c0+x]) / 255 - mean[c]) / std[c]                  ToTensor, then Normalize
    sy = float32(h) / float32(S);  fy = max(sy * (i + 0.5) - 0.5, 0);  y0 = int(fy);  y1 = min(y0 + 1, h - 1);  ly = fy - y0
    (the same for the columns: sx, fx, x0, x1, lx)
    out(c, i, j) = (1 - ly) * ((1 - lx) * p(c,y0,x0) + lx * p(c,y0,x1)) + ly * ((1 - lx) * p(c,y1,x0) + lx * p(c,y1,x1))
The source position sy * (i + 0.5) - 0.5 is ONE fused multiply-add, rounded once, as torch's CPU kernel computes it: with the
product rounded on its own, ly moves by up to an ulp of fy (1.5e-5 at fy = 200) and a crop of a large box by 1.6e-5 against
torch; fused, the two agree to 5e-7.  Every other operation is rounded on its own.  (y0 and x0 are also held to h - 1 /
w - 1, which no rounding reaches.)  This is
torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) applied after the two transforms:
what transforms.Resize does to a tensor in the torchvision of the reference's time (antialiasing of tensors became the default
only with torchvision 0.17).  A box LARGER than S x S is therefore plain bilinear too: no low-pass filter, source pixels are
skipped.  A box with row1 <= row0 or col1 <= col0, or whose padded box misses the raster, has no crop: valid is False and
the crop is zeros (the reference would raise there).

The tie to the reference: torchvision is not a dependency of this project and no fixture was recorded from the reference's
dead.get_transform; the tests hold crops_np to torch's own interpolate on the CPU, fed with the host-sliced, padded and
clipped box after the two transforms, and the device route to crops_np.

The NumPy functions are the definition (as canopy.crown_height_np and abundance.resample_np are).
"""
import collections

import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_CHANNELS = 4
MAX_SIZE = 512                   # DTA_RGB_CROPS_MAX_SIZE: the two tables of a crown live in a workgroup's LDS
MAX_GROUPS = 1024                # DTA_RGB_CROPS_MAX_GROUPS: above this many units of work a workgroup takes several
UNIT_ELEMS = 65536               # RC_UNIT_ELEMS (csrc/dead.hip): a unit is whole output rows of about this many elements ...
MIN_UNIT_ELEMS = 8192            # RC_MIN_UNIT_ELEMS: ... fewer, down to this, where the crowns are too few to fill the launch

DeadPrediction = collections.namedtuple("DeadPrediction", "label score valid")

# training the classifier (dead_train.py: the resident image pool, the loss, train_dead.py's loop, the precision-recall
# curve) is reachable from here by name; that module builds on this one, so it is imported on first use
_TRAIN = ("ImagePool", "DeadAccumulator", "loss", "fit", "validate", "pool_batch_np", "flips_np", "loss_np", "report_np",
          "pr_curve_np", "threshold_for_precision")


def __getattr__(name):
    if name in _TRAIN:
        from . import dead_train
        return getattr(dead_train, name)
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _norm(mean, std, channels):
    m, s = np.asarray(mean, np.float32).reshape(-1), np.asarray(std, np.float32).reshape(-1)
    if len(m) < channels or len(s) < channels:
        raise ValueError("mean and std need one entry per channel ({})".format(channels))
    m, s = np.ascontiguousarray(m[:channels]), np.ascontiguousarray(s[:channels])
    if np.isnan(m).any() or np.isnan(s).any() or (s == 0).any():
        raise ValueError("std must not be 0, and neither mean nor std may be NaN")
    return m, s


def _size_pad(size, pad):
    size, pad = int(size), int(pad)
    if not 1 <= size <= MAX_SIZE:
        raise ValueError("size must be 1..{}, got {}".format(MAX_SIZE, size))
    if pad < 0:
        raise ValueError("pad must be >= 0, got {}".format(pad))
    return size, pad


def _host_boxes(boxes):
    b = np.asarray(_host(boxes))
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.dtype.kind not in "iu":
        raise ValueError("boxes must be a non-empty integer [N, 4] array of (row0, col0, row1, col1)")
    return b.astype(np.int64)


def _planar(tile):
    """A host uint8 raster as [C][H][W]; [H][W][C] (C <= 4 last, more than 4 first) is permuted."""
    t = np.asarray(_host(tile))
    if t.dtype != np.uint8:
        raise ValueError("the RGB raster must be uint8, got {}".format(t.dtype))
    if t.ndim != 3 or t.size < 1:
        raise ValueError("the RGB raster must be a non-empty [C][H][W] (or [H][W][C]) array")
    if t.shape[0] > MAX_CHANNELS and t.shape[2] <= MAX_CHANNELS:
        t = t.transpose(2, 0, 1)
    if t.shape[0] > MAX_CHANNELS:
        raise ValueError("the RGB raster must have 1 to {} channels, got shape {}".format(MAX_CHANNELS, tuple(t.shape)))
    return np.ascontiguousarray(t)


def launch_plan(n, size, channels):
    """(output rows per unit of work, units per crown) of dta_rgb_crops for n crowns: the launch has min(n * units, MAX_GROUPS)
    workgroups, each with a contiguous share of the units."""
    row = size * channels
    rows = min(-(-UNIT_ELEMS // row), size)
    if n * -(-size // rows) < MAX_GROUPS:
        want = -(-MAX_GROUPS // n)
        rows = max(-(-size // want), min(-(-MIN_UNIT_ELEMS // row), rows))
    return rows, -(-size // rows)


def pad_clip_boxes(boxes, height, width, pad=0):
    """(row0, col0, rows, cols, valid) [N] each: every box grown by `pad` and clipped to the raster.  valid is False (and rows,
    cols 0) for a box with row1 <= row0 or col1 <= col0 and for one whose grown box misses the raster."""
    b = _host_boxes(boxes)
    r0, c0 = np.maximum(b[:, 0] - pad, 0), np.maximum(b[:, 1] - pad, 0)
    r1, c1 = np.minimum(b[:, 2] + pad, height), np.minimum(b[:, 3] + pad, width)
    valid = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]) & (r1 > r0) & (c1 > c0)
    return r0, c0, np.where(valid, r1 - r0, 0), np.where(valid, c1 - c0, 0), valid


def _axis(n, S):
    """(i0, i1, l, 1 - l) of the S output positions over n source positions: float32 operation by operation."""
    f32 = np.float32
    scale = f32(n) / f32(S)
    # one fused multiply-add: the product of two float32 values is exact in float64, the result is rounded to float32 once
    f = (np.float64(scale) * (np.arange(S, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)
    f = np.maximum(f, f32(0))
    i0 = np.minimum(f.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    lam = (f - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam, (f32(1) - lam).astype(np.float32)


def crops_np(tile, boxes, size=224, pad=0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The definition: (x float32 [N, C, size, size], valid bool [N]) of the crowns `boxes` on the uint8 raster `tile`
    ([C][H][W], or [H][W][C]); the module docstring's formula.  Bilinear, align_corners=False, no antialiasing."""
    t = _planar(tile)
    size, pad = _size_pad(size, pad)
    C, H, W = t.shape
    m, s = _norm(mean, std, C)
    r0, c0, rows, cols, valid = pad_clip_boxes(boxes, H, W, pad)
    x = np.zeros((len(r0), C, size, size), np.float32)
    table = ((np.arange(256, dtype=np.float32)[None, :] / np.float32(255) - m[:, None]) / s[:, None]).astype(np.float32)
    for n in np.flatnonzero(valid):
        u8 = t[:, r0[n]:r0[n] + rows[n], c0[n]:c0[n] + cols[n]]
        p = np.stack([table[c][u8[c]] for c in range(C)])                       # [C][h][w] float32
        y0, y1, ly, oly = _axis(int(rows[n]), size)
        x0, x1, lx, olx = _axis(int(cols[n]), size)
        top = olx * p[:, y0][:, :, x0] + lx * p[:, y0][:, :, x1]
        bot = olx * p[:, y1][:, :, x0] + lx * p[:, y1][:, :, x1]
        x[n] = oly[None, :, None] * top + ly[None, :, None] * bot
    return x, valid


def head_np(logits):
    """(label int64 [N], score float32 [N]) of [N, 2] logits in any float dtype: the maximum and the argmax of
    softmax(sigmoid(logits), 1) in float32; a tie gives label 0, as np.argmax does."""
    if hasattr(logits, "detach"):
        logits = logits.detach().float().cpu().numpy()
    l = np.asarray(logits).astype(np.float32)
    if l.ndim != 2 or l.shape[1] != 2:
        raise ValueError("logits must be [N, 2]")
    one = np.float32(1)
    s = (one / (one + np.exp(-l))).astype(np.float32)
    e = np.exp(s - s.max(axis=1, keepdims=True)).astype(np.float32)
    p = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    return np.argmax(p, axis=1).astype(np.int64), p.max(axis=1).astype(np.float32)


def filter_dead(label, score, threshold, ens_label=None, ens_score=None):
    """predict_tile's rule: alive = ~((label == 1) & (float64(score) > threshold)), a bool mask [N] -- the `mask` of
    abundance.counts / abundance.resample, combined with canopy's keep by `&`.  A score equal to the threshold stays alive.
    With ens_label / ens_score (both): also copies of them with -1 and NaN at the dead crowns (the reference's None).
    NumPy arrays give NumPy arrays; torch tensors, on any device, give tensors there without waiting for the device."""
    if (ens_label is None) != (ens_score is None):
        raise ValueError("ens_label and ens_score go together")
    threshold = float(threshold)
    if hasattr(label, "detach"):
        import torch
        alive = ~((label == 1) & (score.to(torch.float64) > threshold))
        if ens_label is None:
            return alive
        return (alive, torch.where(alive, ens_label, torch.full_like(ens_label, -1)),
                torch.where(alive, ens_score, torch.full_like(ens_score, float("nan"))))
    label, score = np.asarray(label), np.asarray(score)
    alive = ~((label == 1) & (score.astype(np.float64) > threshold))
    if ens_label is None:
        return alive
    ens_label, ens_score = np.asarray(ens_label), np.asarray(ens_score)
    return alive, np.where(alive, ens_label, -1).astype(ens_label.dtype), np.where(alive, ens_score, np.nan).astype(ens_score.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the device route
# ---------------------------------------------------------------------------------------------------------------------
def _elem(dtype):
    import torch
    from . import _lib
    codes = {torch.float32: _lib.ELEM_F32, torch.bfloat16: _lib.ELEM_BF16, torch.float16: _lib.ELEM_F16}
    if dtype not in codes:
        raise ValueError("dtype must be torch.float32, torch.bfloat16 or torch.float16, got {!r}".format(dtype))
    return codes[dtype]


class RgbRaster:
    """A uint8 raster kept resident as planar [C][H][W] (the layout rasterio reads), C = 1 to 4.  An [H][W][C] array is
    permuted once at upload."""

    def __init__(self, tile, device="cuda"):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("deeptreeattention_amd.dead runs on a ROCm device only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._adopt(torch.from_numpy(_planar(tile)).to(dev, non_blocking=True))

    def _adopt(self, t):
        if t.dim() != 3 or t.numel() < 1:
            raise ValueError("the RGB raster must be a non-empty [C][H][W] raster")
        if t.shape[0] > MAX_CHANNELS:
            raise ValueError("the RGB raster must have 1 to {} channels, got shape {}".format(MAX_CHANNELS, tuple(t.shape)))
        if t.numel() > 0x7FFFFFFF:
            raise ValueError("the raster has more than 2^31 - 1 elements")
        self.data, self.device = t, t.device
        self.channels, self.height, self.width = (int(v) for v in t.shape)
        self.shape = (self.channels, self.height, self.width)

    @classmethod
    def resident(cls, tile):
        """A contiguous uint8 [C][H][W] tensor that already lives on the device, taken as it is (no copy)."""
        import torch
        if not isinstance(tile, torch.Tensor) or tile.dtype != torch.uint8 or not tile.is_contiguous():
            raise ValueError("resident() takes a contiguous uint8 [C][H][W] tensor")
        self = cls.__new__(cls)
        self._adopt(tile)
        return self

    def _boxes(self, boxes):
        """What DenseRaster.crops and CanopyRaster.crown_height accept -> a contiguous int32 [N, 4] device tensor."""
        import torch
        what = "boxes must be a non-empty integer [N, 4] array of (row0, col0, row1, col1)"
        if isinstance(boxes, torch.Tensor):
            o = boxes
            if o.dim() != 2 or o.shape[1] != 4 or o.shape[0] < 1 or o.dtype.is_floating_point or o.dtype == torch.bool:
                raise ValueError(what)
            if not o.is_cuda:
                return self._boxes(o.numpy())
            if o.dtype != torch.int32 or o.device != self.device or not o.is_contiguous():
                o = o.to(device=self.device, dtype=torch.int32).contiguous()
            return o
        host = np.asarray(boxes)
        if host.ndim != 2 or host.shape[1] != 4 or host.shape[0] < 1 or host.dtype.kind not in "iu":
            raise ValueError(what)
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(self.device)

    def _launch(self, o, size, pad, m, s, x, channels_last, valid):
        """dta_rgb_crops for the int32 device boxes `o` into x and valid (uint8 or bool [N])."""
        from . import _lib
        if not self.data.is_cuda:
            raise RuntimeError("deeptreeattention_amd.dead runs on a ROCm device only (no CPU fallback)")
        L = _lib.lib()
        _lib.check(L.dta_rgb_crops(_lib.ptr(self.data), self.channels, self.height, self.width, _lib.ptr(o), o.shape[0], size, pad,
                                   m.ctypes.data_as(_lib.c_float_p), s.ctypes.data_as(_lib.c_float_p), _elem(x.dtype),
                                   1 if channels_last else 0, _lib.ptr(x), _lib.ptr(valid), _lib.current_stream_ptr()),
                   "dta_rgb_crops")

    def _out(self, n, size, dtype, channels_last, out):
        import torch
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        if out is None:
            return torch.empty((n, self.channels, size, size), dtype=dtype, device=self.device, memory_format=fmt)
        if (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != (n, self.channels, size, size)
                or out.device != self.device or not out.is_contiguous(memory_format=fmt)):
            raise ValueError("out must be a {} [{}, {}, {}, {}] tensor on {}, {}".format(
                dtype, n, self.channels, size, size, self.device, "channels_last" if channels_last else "contiguous"))
        return out

    def crops(self, boxes, size=224, pad=0, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=None, channels_last=False, out=None):
        """crops_np on the device (dta_rgb_crops: one launch for all crowns): (x [N, C, size, size] in `dtype`, valid bool [N]),
        device tensors.

        boxes: [N, 4] (row0, col0, row1, col1), half-open, a host array or a device tensor -- what DenseRaster.crops and
        CanopyRaster.crown_height take; each box is grown by `pad` pixels on every side (10: the reference's 1 m at 0.1 m per
        pixel) and clipped to the raster.  dtype: torch.float32 (the default), bfloat16 or float16 -- one rounding of the
        float32 result.  channels_last: x has torch.channels_last memory.  out=: the tensor to write x into.  Bilinear,
        align_corners=False, NO antialiasing, also for a box larger than size x size (the module docstring says why).
        valid is False where the box is empty or inverted or its padded box misses the raster; that crop is all zeros.
        Device boxes are checked by the kernel.  Nothing here waits for the device."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        _elem(dtype)
        size, pad = _size_pad(size, pad)
        m, s = _norm(mean, std, self.channels)
        o = self._boxes(boxes)
        n = o.shape[0]
        x = self._out(n, size, dtype, channels_last, out)
        valid = torch.empty(n, dtype=torch.bool, device=self.device)
        self._launch(o, size, pad, m, s, x, channels_last, valid)
        return x, valid


def _head_into(logits, label, score, offset):
    import torch
    from . import _lib
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != 2 or logits.shape[0] < 1:
        raise ValueError("logits must be a [N, 2] tensor, N >= 1")
    code = _elem(logits.dtype)
    if not logits.is_cuda:
        raise RuntimeError("deeptreeattention_amd.dead runs on a ROCm device only (no CPU fallback)")
    logits = logits.contiguous()
    _lib.check(_lib.lib().dta_dead_head(_lib.ptr(logits), code, logits.shape[0], offset, _lib.ptr(label), _lib.ptr(score),
                                        _lib.current_stream_ptr()), "dta_dead_head")


def head(logits):
    """head_np on the device (dta_dead_head, one launch): (label int64 [N], score float32 [N]) of the [N, 2] logits, a
    float32 / bfloat16 / float16 device tensor.  Nothing here waits for the device."""
    import torch
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != 2 or logits.shape[0] < 1:
        raise ValueError("logits must be a [N, 2] tensor, N >= 1")
    _elem(logits.dtype)
    n = logits.shape[0]
    label = torch.empty(n, dtype=torch.int64, device=logits.device)
    score = torch.empty(n, dtype=torch.float32, device=logits.device)
    _head_into(logits, label, score, 0)
    return label, score


def predict_dead(model, raster, boxes, batch_size=64, pad=10, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=None,
                 channels_last=False):
    """predict_dead of the reference for all crowns of a tile: DeadPrediction(label int64 [N], score float32 [N],
    valid bool [N]), device tensors.

    model: any callable from [B, C, size, size] (in `dtype`, channels_last on request) to [B, 2] logits; for the reference's
    checkpoint that is AliveDead.model, a torchvision ResNet-50, moved to the raster's device.  raster: an RgbRaster.
    Per batch: RgbRaster.crops into one buffer that every batch reuses, model under torch.no_grad(), dta_dead_head
    straight into the [N] results; no host synchronisation per batch.  A crown with valid False was fed a crop of zeros:
    its label and score mean nothing.

    The reference calls dead_model.train() before it predicts (src/models/dead.py predict_dead), so its BatchNorm layers use
    the statistics of each batch and a crown's score depends on which crowns share its batch.  The mode (model.eval() or
    model.train()) and the batch size are the caller's choice here; nothing in this function changes the model's mode."""
    import torch
    if not isinstance(raster, RgbRaster):
        raise ValueError("raster must be an RgbRaster")
    dtype = torch.float32 if dtype is None else dtype
    _elem(dtype)
    size, pad = _size_pad(size, pad)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    m, s = _norm(mean, std, raster.channels)
    o = raster._boxes(boxes)
    n, dev = o.shape[0], raster.device
    label = torch.empty(n, dtype=torch.int64, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.bool, device=dev)
    buf = raster._out(min(batch_size, n), size, dtype, channels_last, None)
    with torch.no_grad():
        for a in range(0, n, batch_size):
            b = min(a + batch_size, n)
            x = buf[:b - a]
            raster._launch(o[a:b], size, pad, m, s, x, channels_last, valid[a:b])
            logits = model(x)
            if not isinstance(logits, torch.Tensor) or tuple(logits.shape) != (b - a, 2):
                raise ValueError("the model must map [B, C, {0}, {0}] to [B, 2] logits".format(size))
            _head_into(logits, label, score, a)
    return DeadPrediction(label, score, valid)
