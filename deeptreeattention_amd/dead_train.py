"""Training the alive/dead classifier from a resident image pool: the reference's train_dead.py and the training half of
src/models/dead.py (AliveDead), next to the prediction half in dead.py.  Every name here is also reachable as dead.<name>.

The reference's loop is bound by the host: an ImageFolder of 5,701 small JPEGs (sides 25 to 164 pixels) is decoded on the main
thread (num_workers 0), 128 per step, then ToTensor, Normalize, Resize([224, 224]) and RandomHorizontalFlip run on them
before the ResNet sees anything.  The whole set is under 100 MB as uint8, so here it is decoded ONCE and kept on the device:
    ImagePool          every image planar [C][h][w], back to back in one uint8 tensor, and an int64 table per image
                       (offset, h, w, label).  ImagePool.batch: ONE launch (dta_image_pool_batch, csrc/dead_train.hip) writes
                       the normalised, resized, flipped crops of a batch and their labels; ImagePool.loader: the batches of
                       an epoch, whose order (treedata.epoch_order, level id 63) and flips are pure functions of
                       (seed, epoch, image) through the counter hash of _hash.py -- the kernel reads its slice of the order
                       on the device and draws the flips itself, so nothing is read back and a resumed epoch repeats itself.
    loss               F.cross_entropy(F.sigmoid(logits), y) -- a cross-entropy over sigmoid outputs, the reference's loss --
                       with its gradient and the confusion counts in ONE launch (dta_dead_loss); DeadAccumulator sums the
                       loss and the counts of an epoch on the device, one read at its end.
    fit, validate      train_dead.py's loop: Adam(lr), ReduceLROnPlateau(min, 0.5, 10) on val_loss, per-epoch loss, accuracy,
                       per-class accuracy and the Dead class's precision.
    pr_curve_np, threshold_for_precision
                       the precision-recall curve train_dead.py draws at its end, from which config.yml's dead_threshold
                       was read off; host only (a validation set is hundreds of images).

The definitions (NumPy, as dead.crops_np is):
    pool_batch_np   x[b] = crops_np(image, [(0, 0, h, w)], size, pad=0, mean, std)[0], its last axis reversed where flip[b]:
                    RandomHorizontalFlip AFTER Resize, a reversal of the finished columns, so no arithmetic changes.
    flips_np        image i of n is flipped in `epoch` where draw24(seed, 3, epoch * n + i) < 2^23: a function of the image,
                    not of its place in a batch.
    loss_np         per row, float32:  s = 1 / (1 + exp(-l));  m = max(s0, s1);  lse = m + log(exp(s0 - m) + exp(s1 - m));
                    loss_row = lse - s[y];  p = exp(s - lse);  d_l[c] = (p[c] - [c == y]) * s[c] * (1 - s[c]) / B_valid;
                    the mean is a float64 sum over the rows with a label in {0, 1}, rounded to float32 once; the other rows
                    contribute nothing; conf[label][argmax l, a tie giving 0].

The tie to the reference: torchvision and torchmetrics are not dependencies; the tests hold pool_batch_np to torch's own CPU
operations (/255, normalise, F.interpolate, flip), loss_np to F.cross_entropy(torch.sigmoid(l), y) with autograd in float64,
pr_curve_np to sklearn.metrics.precision_recall_curve, and the device route to these definitions.

torchmetrics' Precision() of the reference's time, which AliveDead logs as "dead_precision", is micro-averaged and so
equals the accuracy; it is not reproduced.  `precision` here is the Dead class's, conf[1][1] / (conf[0][1] + conf[1][1]).
"""
import os

import numpy as np
import torch

from . import _lib
from ._hash import DEAD_ORDER_LEVEL, M64, STREAM_DEAD_FLIP, draw24, shuffle_base
from .dead import (IMAGENET_MEAN, IMAGENET_STD, MAX_CHANNELS, _elem, _head_into, _host, _norm, _planar, _size_pad, crops_np)

MAX_N = _lib.EPOCH_ORDER_MAX_N
MAX_LOSS_ROWS = _lib.DEAD_LOSS_MAX_ROWS
ORDER_LEVEL = DEAD_ORDER_LEVEL
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")      # ImageFolder's
_NO_DEVICE = "deeptreeattention_amd.dead runs on a ROCm device only (no CPU fallback)"


# ---------------------------------------------------------------------------------------------------------------------
# definitions
# ---------------------------------------------------------------------------------------------------------------------
def pool_batch_np(images, index, flip=None, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The definition of a batch: x float32 [B, C, size, size]; x[b] is crops_np of the whole image images[index[b]], with
    its last axis reversed where flip[b]."""
    index = np.asarray(_host(index)).reshape(-1)
    flip = np.zeros(len(index), bool) if flip is None else np.asarray(_host(flip)).reshape(-1).astype(bool)
    if len(flip) != len(index):
        raise ValueError("flip must have one entry per index")
    out = []
    for b, i in enumerate(index):
        t = _planar(images[int(i)])
        x = crops_np(t, np.array([(0, 0, t.shape[1], t.shape[2])], np.int64), size=size, pad=0, mean=mean, std=std)[0][0]
        out.append(x[:, :, ::-1] if flip[b] else x)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def flips_np(n, seed=0, epoch=0):
    """bool [n]: is image i flipped in `epoch` -- draw24(seed, STREAM_DEAD_FLIP, shuffle_base(epoch, n) + i) < 2^23."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1, got {}".format(n))
    with np.errstate(over="ignore"):
        counter = np.uint64(shuffle_base(epoch, n)) + np.arange(n, dtype=np.uint64)
    return draw24(seed, STREAM_DEAD_FLIP, counter) < (1 << 23)


def _logits_np(logits):
    if hasattr(logits, "detach"):
        logits = logits.detach().float().cpu().numpy()
    l = np.asarray(logits).astype(np.float32)
    if l.ndim != 2 or l.shape[1] != 2 or l.shape[0] < 1:
        raise ValueError("logits must be [B, 2], B >= 1")
    return l


def loss_np(logits, labels):
    """The definition of the loss: (loss_row float32 [B] (0 where the label is outside {0, 1}), mean float32, d_logits float32
    [B, 2], conf int64 [2][2]) -- the module docstring's formula.  The rows outside {0, 1} number B - conf.sum()."""
    l = _logits_np(logits)
    y = np.asarray(_host(labels)).reshape(-1).astype(np.int64)
    if len(y) != len(l):
        raise ValueError("labels must be [B]")
    f32, one = np.float32, np.float32(1)
    ok = (y == 0) | (y == 1)
    bv = int(ok.sum())
    yy = np.where(ok, y, 0)
    with np.errstate(over="ignore"):
        s = (one / (one + np.exp(-l))).astype(f32)
    m = s.max(axis=1)
    lse = (m + np.log((np.exp(s[:, 0] - m) + np.exp(s[:, 1] - m)).astype(f32))).astype(f32)
    rows = np.where(ok, lse - s[np.arange(len(l)), yy], f32(0)).astype(f32)
    mean = f32(rows[ok].astype(np.float64).sum() / bv) if bv else f32(0)
    p = np.exp(s - lse[:, None]).astype(f32)
    hot = np.zeros_like(p)
    hot[np.arange(len(l)), yy] = one
    d = np.zeros_like(p)
    if bv:
        d = ((p - hot) * s * (one - s) / f32(bv)).astype(f32)
        d[~ok] = 0
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (yy[ok], (l[ok, 1] > l[ok, 0]).astype(np.int64)), 1)
    return rows, mean, d, conf


def report_np(loss_sum, rows, conf):
    """The per-epoch figures from the sums: val_loss = loss_sum / rows, accuracy, class_accuracy[2] (the diagonal over the
    row sums) and the Dead class's precision conf[1][1] / (conf[0][1] + conf[1][1]); a zero denominator gives 0.0."""
    conf = np.asarray(conf, np.int64).reshape(2, 2)
    rows = int(rows)

    def ratio(a, b):
        return float(a) / float(b) if b else 0.0
    return {"val_loss": ratio(loss_sum, rows), "accuracy": ratio(conf[0, 0] + conf[1, 1], conf.sum()),
            "class_accuracy": [ratio(conf[0, 0], conf[0].sum()), ratio(conf[1, 1], conf[1].sum())],
            "precision": ratio(conf[1, 1], conf[0, 1] + conf[1, 1]), "rows": rows, "conf": conf}


def pr_curve_np(labels, scores):
    """(precision, recall, thresholds), float64: sklearn.metrics.precision_recall_curve(labels, scores) as scikit-learn 1.7
    defines it, label 1 being the positive class.  Every distinct score is a threshold, ascending; tps and fps are the counts of
    positives and negatives with score >= threshold; precision = tps / (tps + fps), 0 where the sum is 0; recall =
    tps / tps[-1], all ones if there is no positive; a final (1, 0) is appended, so precision and recall have one entry more
    than thresholds.  (The scikit-learn of the reference's time also dropped the thresholds below the first one with full
    recall; 1.7 keeps them.)

    train_dead.py passes the score of the PREDICTED class (the maximum of the softmax), not the probability of Dead; this
    function takes whatever scores it is given."""
    y = np.asarray(_host(labels)).reshape(-1)
    s = np.asarray(_host(scores)).reshape(-1)
    if len(y) != len(s) or len(y) < 1:
        raise ValueError("labels and scores must be non-empty and of one length")
    pos = (y == 1)
    desc = np.argsort(s, kind="mergesort")[::-1]
    s, pos = s[desc], pos[desc]
    last = np.r_[np.flatnonzero(np.diff(s)), len(s) - 1]          # the last row of every distinct score, scores descending
    tps = np.cumsum(pos, dtype=np.float64)[last]
    fps = 1 + last - tps
    total = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, total, out=precision, where=total != 0)
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    return np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], s[last][::-1]


def threshold_for_precision(labels, scores, precision):
    """The lowest threshold of pr_curve_np(labels, scores) whose precision is at least `precision`, or None."""
    p, _, t = pr_curve_np(labels, scores)
    hit = np.flatnonzero(p[:-1] >= float(precision))
    return t[hit[0]].item() if len(hit) else None


# ---------------------------------------------------------------------------------------------------------------------
# the resident pool
# ---------------------------------------------------------------------------------------------------------------------
class ImagePool:
    """Labelled uint8 images of any sizes kept resident: one uint8 tensor with every image planar [C][h][w] back to back, and
    an int64 [n][4] table (offset, h, w, label).  images: a list of uint8 arrays, [h][w][C] or [C][h][w] by dead._planar's
    rule (an array whose first axis is at most 4 long is planar); C is 1 to 4 and the same for all."""

    def __init__(self, images, labels, device="cuda", classes=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(_NO_DEVICE)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        data, table = self._pack(images, labels)
        self._adopt(torch.from_numpy(data).to(dev, non_blocking=True), torch.from_numpy(table).to(dev, non_blocking=True),
                    table, classes)

    @staticmethod
    def _pack(images, labels):
        images = list(images)
        labels = np.asarray(_host(labels)).reshape(-1)
        if len(images) < 1:
            raise ValueError("an ImagePool needs at least one image")
        if len(images) > MAX_N:
            raise ValueError("an ImagePool holds at most {} images (EPOCH_ORDER_MAX_N), got {}".format(MAX_N, len(images)))
        if len(labels) != len(images) or labels.dtype.kind not in "iub":
            raise ValueError("labels must be one integer per image")
        planes = [_planar(im) for im in images]
        C = planes[0].shape[0]
        table = np.zeros((len(planes), 4), np.int64)
        at = 0
        for i, p in enumerate(planes):
            if p.shape[0] != C:
                raise ValueError("every image must have {} channels, image {} has shape {}".format(C, i, tuple(p.shape)))
            if p.shape[1] * p.shape[2] >= 1 << 31:
                raise ValueError("image {}: h * w must be below 2^31, got {} x {}".format(i, p.shape[1], p.shape[2]))
            table[i] = (at, p.shape[1], p.shape[2], int(labels[i]))
            at += p.size
        return np.concatenate([p.reshape(-1) for p in planes]), table

    def _adopt(self, data, table, host_table, classes):
        if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("data must be a contiguous uint8 [bytes] tensor")
        if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous() or table.device != data.device:
            raise ValueError("table must be a contiguous int64 [n, 4] tensor (offset, h, w, label) next to data")
        t = np.ascontiguousarray(host_table, dtype=np.int64)
        n = t.shape[0]
        if t.shape != tuple(table.shape) or not 1 <= n <= MAX_N:
            raise ValueError("the table must have 1..{} rows, got {}".format(MAX_N, t.shape))
        area = t[:, 1] * t[:, 2]
        if (t[:, 1:3] < 1).any() or (area >= 1 << 31).any():
            raise ValueError("every image needs h, w >= 1 and h * w below 2^31")
        c, rem = divmod(int(data.numel()), int(area.sum()))
        if rem or not 1 <= c <= MAX_CHANNELS or not np.array_equal(t[:, 0], np.r_[0, np.cumsum(area * c)[:-1]]):
            raise ValueError("data must hold the table's images back to back, 1 to {} channels each".format(MAX_CHANNELS))
        self.data, self.table, self.device, self.channels = data, table, data.device, c
        self.heights, self.widths, self.labels = t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy()
        self.classes = None if classes is None else list(classes)

    @classmethod
    def resident(cls, data, table, classes=None):
        """A uint8 [bytes] tensor and its int64 [n, 4] table that already live side by side, taken as they are (no copy of
        the images; the table is read once)."""
        if not isinstance(data, torch.Tensor) or not isinstance(table, torch.Tensor):
            raise ValueError("resident() takes a uint8 [bytes] tensor and an int64 [n, 4] table")
        self = cls.__new__(cls)
        self._adopt(data, table, table.cpu().numpy(), classes)
        return self

    @classmethod
    def from_folder(cls, root, device="cuda", extensions=IMG_EXTENSIONS):
        """torchvision.datasets.ImageFolder's rule: the class directories of `root` sorted by name get labels 0, 1, ... (so
        Alive = 0, Dead = 1), the files of a class are sorted (subdirectories are walked in sorted order too), every image is
        decoded ONCE with PIL as RGB.  .classes holds the names, .paths the files."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("ImagePool.from_folder decodes the images with PIL (pillow), which is not installed; decode them "
                              "yourself and call ImagePool(images, labels)") from e
        root = os.fspath(root)
        classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
        if not classes:
            raise FileNotFoundError("no class directories in {}".format(root))
        images, labels, paths = [], [], []
        for k, name in enumerate(classes):
            for d, _, files in sorted(os.walk(os.path.join(root, name), followlinks=True)):
                for f in sorted(files):
                    if f.lower().endswith(tuple(extensions)):
                        paths.append(os.path.join(d, f))
                        with Image.open(paths[-1]) as im:
                            images.append(np.asarray(im.convert("RGB"), dtype=np.uint8).transpose(2, 0, 1))
                        labels.append(k)
        if not images:
            raise FileNotFoundError("no image files ({}) under {}".format(", ".join(extensions), root))
        self = cls(images, np.asarray(labels, np.int64), device=device, classes=classes)
        self.paths = paths
        return self

    def __len__(self):
        return len(self.labels)

    # ---- arguments -> device tensors; every check before the library is reached
    def _index(self, index):
        what = "index must be a non-empty integer [B] array of image numbers"
        n = len(self)
        if isinstance(index, torch.Tensor) and index.is_cuda:
            if index.dim() != 1 or index.shape[0] < 1 or index.dtype not in (torch.int32, torch.int64):
                raise ValueError(what + " (int32 or int64 on the device)")
            return index.to(self.device).contiguous()              # the kernel checks a device index: outside the pool -> label -1
        host = np.asarray(_host(index))
        if host.ndim != 1 or host.shape[0] < 1 or host.dtype.kind not in "iu":
            raise ValueError(what)
        if int(host.min()) < 0 or int(host.max()) >= n:
            raise IndexError("index outside the pool: {}..{} of {} images".format(int(host.min()), int(host.max()), n))
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.int64))).to(self.device)

    def _flip(self, flip, B):
        if flip is None:
            return None
        what = "flip must be a bool or uint8 [{}] array, one entry per index".format(B)
        if isinstance(flip, torch.Tensor) and flip.is_cuda:
            if tuple(flip.shape) != (B,) or flip.dtype not in (torch.bool, torch.uint8):
                raise ValueError(what)
            f = flip.to(self.device).contiguous()
            return f.view(torch.uint8) if f.dtype == torch.bool else f
        host = np.asarray(_host(flip))
        if host.shape != (B,) or host.dtype not in (np.bool_, np.uint8):
            raise ValueError(what)
        return torch.from_numpy(np.ascontiguousarray(host.astype(np.uint8))).to(self.device)

    def _out(self, B, size, dtype, channels_last, out):
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        if out is None:
            return torch.empty((B, self.channels, size, size), dtype=dtype, device=self.device, memory_format=fmt)
        if (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != (B, self.channels, size, size)
                or out.device != self.device or not out.is_contiguous(memory_format=fmt)):
            raise ValueError("out must be a {} [{}, {}, {}, {}] tensor on {}, {}".format(
                dtype, B, self.channels, size, size, self.device, "channels_last" if channels_last else "contiguous"))
        return out

    def _launch(self, index, start, count, flip, hashed, seed, epoch, size, m, s, x, channels_last, y):
        """dta_image_pool_batch: places start .. start + count - 1 of `index` (None: the identity) into x and y."""
        if not self.data.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        _lib.check(_lib.lib().dta_image_pool_batch(
            _lib.ptr(self.data), self.data.numel(), _lib.ptr(self.table), len(self), self.channels, _lib.ptr(index),
            1 if index is not None and index.dtype == torch.int64 else 0, start, count, _lib.ptr(flip), 1 if hashed else 0,
            int(seed) & M64, int(epoch) & M64, size, m.ctypes.data_as(_lib.c_float_p), s.ctypes.data_as(_lib.c_float_p),
            _elem(x.dtype), 1 if channels_last else 0, _lib.ptr(x), _lib.ptr(y), _lib.current_stream_ptr()), "dta_image_pool_batch")

    def batch(self, index, flip=None, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, channels_last=False,
              out=None):
        """pool_batch_np on the device, and the labels, in one launch: (x [B, C, size, size] in `dtype`, y int64 [B]), device
        tensors.

        index: int32 / int64 [B], a host array (checked here: IndexError outside the pool) or a device tensor (checked by the
        kernel: an index outside the pool gives a crop of zeros and label -1).  flip: bool / uint8 [B], host or device, or
        None for no flips.  dtype: torch.float32, bfloat16 or float16 -- one rounding of the float32 result.
        channels_last: x has torch.channels_last memory.  out=: the tensor to write x into.  Nothing here waits for the device."""
        dtype = torch.float32 if dtype is None else dtype
        _elem(dtype)
        size, _ = _size_pad(size, 0)
        m, s = _norm(mean, std, self.channels)
        idx = self._index(index)
        B = idx.shape[0]
        f = self._flip(flip, B)
        x = self._out(B, size, dtype, channels_last, out)
        y = torch.empty(B, dtype=torch.int64, device=self.device)
        self._launch(idx, 0, B, f, False, 0, 0, size, m, s, x, channels_last, y)
        return x, y

    def loader(self, batch_size, shuffle=False, train=False, seed=0, epoch=0, drop_last=False, size=224, mean=IMAGENET_MEAN,
               std=IMAGENET_STD, dtype=torch.float32, channels_last=False):
        """The batches (x, y) of one epoch, one launch each, as `batch` gives them.

        shuffle: the order is treedata.epoch_order([n], epoch, seed, levels=[63])[0], made once and kept on the device; every
        launch reads its slice of it there.  train: image i is flipped where flips_np(n, seed, epoch)[i], drawn inside the
        kernel.  The last batch is short unless drop_last.  The arguments are checked here, before the first batch."""
        B, n = int(batch_size), len(self)
        if B < 1:
            raise ValueError("batch_size must be at least 1, got {}".format(B))
        dtype = torch.float32 if dtype is None else dtype
        _elem(dtype)
        size, _ = _size_pad(size, 0)
        m, s = _norm(mean, std, self.channels)
        nb = n // B if drop_last else -(-n // B)
        if nb == 0:
            raise ValueError("the pool has {} images: no batch of {} with drop_last".format(n, B))
        if not self.data.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        order = None
        if shuffle:
            from . import treedata
            order = treedata.epoch_order([n], epoch, seed, levels=[ORDER_LEVEL], device=self.device)[0]
        return self._epoch(order, nb, B, bool(train), seed, epoch, size, m, s, dtype, channels_last)

    def _epoch(self, order, nb, B, train, seed, epoch, size, m, s, dtype, channels_last):
        n = len(self)
        for k in range(nb):
            start = k * B
            count = min(start + B, n) - start
            x = self._out(count, size, dtype, channels_last, None)
            y = torch.empty(count, dtype=torch.int64, device=self.device)
            self._launch(order, start, count, None, train, seed, epoch, size, m, s, x, channels_last, y)
            yield x, y


# ---------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------
class DeadAccumulator:
    """The sums of an epoch on the device, seven 8-byte words that dta_dead_loss adds to: loss_sum (float64), rows (the rows
    with a label in {0, 1}), conf[2][2] indexed [label][prediction], bad (the other rows).  read() and report() copy them
    to the host: the one read of an epoch."""

    def __init__(self, device="cuda"):
        self.words = torch.zeros(_lib.DEAD_ACC_WORDS, dtype=torch.int64, device=device)

    def reset(self):
        self.words.zero_()

    def read(self):
        """{"loss_sum": float, "rows": int, "conf": int64 [2][2], "bad": int}: one device-to-host copy."""
        w = self.words.cpu().numpy()
        return {"loss_sum": float(w[:1].view(np.float64)[0]), "rows": int(w[1]), "conf": w[2:6].reshape(2, 2).copy(), "bad": int(w[6])}

    def report(self):
        """report_np of the sums, and `bad`: val_loss = loss_sum / rows, accuracy, class_accuracy[2], the Dead class's
        precision (a zero denominator gives 0.0, evaluate's convention).  One device-to-host copy."""
        r = self.read()
        out = report_np(r["loss_sum"], r["rows"], r["conf"])
        out["bad"] = r["bad"]
        return out


def _check_logits(logits, labels):
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != 2 or not 1 <= logits.shape[0] <= MAX_LOSS_ROWS:
        raise ValueError("logits must be a [B, 2] tensor, 1 <= B <= {}".format(MAX_LOSS_ROWS))
    _elem(logits.dtype)
    if (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (logits.shape[0],)
            or labels.device != logits.device):
        raise ValueError("labels must be an int64 [{}] tensor next to the logits".format(logits.shape[0]))


class _DeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, words):
        if not logits.is_cuda:
            raise RuntimeError(_NO_DEVICE)
        l = logits.detach().contiguous()
        out = torch.empty((), dtype=torch.float32, device=l.device)
        d = torch.empty(l.shape, dtype=torch.float32, device=l.device)
        counts = torch.empty(5, dtype=torch.int64, device=l.device)
        _lib.check(_lib.lib().dta_dead_loss(_lib.ptr(l), _elem(l.dtype), _lib.ptr(labels.contiguous()), l.shape[0], _lib.ptr(out),
                                            _lib.ptr(d), _lib.ptr(counts), _lib.ptr(words), _lib.current_stream_ptr()),
                   "dta_dead_loss")
        ctx.save_for_backward(d)
        ctx.dtype = logits.dtype
        return out

    @staticmethod
    def backward(ctx, grad):
        (d,) = ctx.saved_tensors
        return (d * grad).to(ctx.dtype), None, None


def loss(logits, labels, accumulate=None):
    """loss_np on the device (dta_dead_loss, one launch): the float32 mean of the reference's loss
    F.cross_entropy(F.sigmoid(logits), labels) over the rows with a label in {0, 1}, a 0-dim device tensor; its backward
    hands on the gradient the same launch wrote, scaled by the incoming one, in the logits' dtype.

    logits: [B, 2], float32 / bfloat16 / float16 on the device; labels: int64 [B] there.  accumulate: a DeadAccumulator that
    this batch's loss sum, rows, confusion counts and out-of-range labels are added to, on the device.  Reruns are
    bit-identical.  Nothing here waits for the device."""
    _check_logits(logits, labels)
    if accumulate is not None and (not isinstance(accumulate, DeadAccumulator) or accumulate.words.device != logits.device):
        raise ValueError("accumulate must be a DeadAccumulator on the logits' device")
    return _DeadLoss.apply(logits, labels, None if accumulate is None else accumulate.words)


# ---------------------------------------------------------------------------------------------------------------------
# train_dead.py's loop
# ---------------------------------------------------------------------------------------------------------------------
def validate(model, pool, batch_size=128, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=None, channels_last=False,
             scores=False):
    """One pass over `pool` in its own order: model.eval(), torch.no_grad(), every batch's loss and confusion counts summed
    on the device, ONE read at the end.  Returns DeadAccumulator.report()'s dict (val_loss, accuracy, class_accuracy,
    precision, rows, conf, bad).  scores=True: (that dict, label int64 [n], score float32 [n], true int64 [n]), device
    tensors -- dead.head's label and score per image, what train_dead.py hands to precision_recall_curve.  The model's
    mode is put back afterwards."""
    if not isinstance(pool, ImagePool):
        raise ValueError("pool must be an ImagePool")
    acc = DeadAccumulator(pool.device)
    n = len(pool)
    if scores:
        label = torch.empty(n, dtype=torch.int64, device=pool.device)
        score = torch.empty(n, dtype=torch.float32, device=pool.device)
        true = torch.empty(n, dtype=torch.int64, device=pool.device)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            at = 0
            for x, y in pool.loader(batch_size, size=size, mean=mean, std=std, dtype=dtype, channels_last=channels_last):
                logits = model(x)
                loss(logits, y, accumulate=acc)
                if scores:
                    _head_into(logits, label, score, at)
                    true[at:at + y.shape[0]] = y
                at += y.shape[0]
    finally:
        model.train(was)
    rep = acc.report()
    return (rep, label, score, true) if scores else rep


def fit(model, train_pool, val_pool=None, epochs=40, lr=1e-4, batch_size=128, seed=0, size=224, dtype=None,
        channels_last=False, log=None):
    """train_dead.py's loop on resident pools.  model: any nn.Module on the pools' device that maps [B, C, size, size] (in
    `dtype`, channels_last on request) to [B, 2] logits; the reference's network is
        model = torchvision.models.resnet50(pretrained=True)
        model.fc = torch.nn.Linear(2048, 2)
    The optimiser is torch.optim.Adam(model.parameters(), lr) and, with a val_pool, torch's ReduceLROnPlateau(mode="min",
    factor=0.5, patience=10) on val_loss: AliveDead.configure_optimizers' values (config.yml: dead: epochs 40, lr 1e-4,
    batch_size 128).  Per epoch: train_pool.loader(batch_size, shuffle=True, train=True, seed, epoch) -> model -> dead.loss
    -> backward -> step, with no host synchronisation inside the epoch; then validate(model, val_pool).

    Returns one dict per epoch: epoch, lr (the rate the epoch trained with), train_loss (the mean row loss of the epoch), and
    -- None without a val_pool -- val_loss, accuracy, class_accuracy, precision.  log: called with each dict."""
    if not isinstance(train_pool, ImagePool) or (val_pool is not None and not isinstance(val_pool, ImagePool)):
        raise ValueError("train_pool and val_pool must be ImagePools")
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 0 or batch_size < 1:
        raise ValueError("epochs must be >= 0 and batch_size >= 1")
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=10)
    acc = DeadAccumulator(train_pool.device)
    history = []
    for epoch in range(epochs):
        model.train()
        acc.reset()
        rate = float(opt.param_groups[0]["lr"])
        for x, y in train_pool.loader(batch_size, shuffle=True, train=True, seed=seed, epoch=epoch, size=size, dtype=dtype,
                                      channels_last=channels_last):
            opt.zero_grad(set_to_none=True)
            loss(model(x), y, accumulate=acc).backward()
            opt.step()
        row = {"epoch": epoch, "lr": rate, "train_loss": acc.report()["val_loss"], "val_loss": None, "accuracy": None,
               "class_accuracy": None, "precision": None}
        if val_pool is not None:
            rep = validate(model, val_pool, batch_size=batch_size, size=size, dtype=dtype, channels_last=channels_last)
            row.update({k: rep[k] for k in ("val_loss", "accuracy", "class_accuracy", "precision")})
            row["conf"] = rep["conf"]
            sched.step(rep["val_loss"])
        history.append(row)
        if log is not None:
            log(row)
    return history
