"""Training the alive/dead classifier, host side (no GPU): the NumPy definitions of dead_train.py against torch's own CPU
operations and scikit-learn, ImagePool.from_folder on PNGs written here, argument errors, and the two C entries' refusals,
none of which reaches a launch.

Bounds.  Crops: test_dead_cpu.CROP_TOL (1e-5, derived there).  Loss: 1e-6 max abs on the row losses, the mean and
B * d_logits against float64 torch -- the bound test_dead_gpu.py holds head's scores to: the same float32 exp / sigmoid
evaluations on values of order 1, each good to a few ulp of 6e-8.  The precision-recall curve: exact equality (integer counts,
one float64 division each)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dead_cpu import CROP_TOL, MEAN4, STD4

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (224, 30, 7)
LOSS_TOL = 1e-6
SHAPES = ((1, 1), (1, 9), (9, 1), (7, 13), None, (300, 280), (56, 56))        # None: exactly S x S


def pool_images(channels, S, seed=0):
    """The issue's image list, planar uint8 [C][h][w]: 1x1, 1x9, 9x1, 7x13, exactly S x S, 300x280 (larger than S: source
    pixels are skipped) and the reference's median 56x56."""
    rng = np.random.default_rng(100 * channels + seed)
    return [rng.integers(0, 256, (channels,) + (shape or (S, S)), dtype=np.uint8) for shape in SHAPES]


def case_flips(n):
    return (np.arange(n) % 2 == 1)


def torch_batch(images, index, flip, size, mean, std):
    """The reference's pipeline per image from torch CPU operations: /255, normalise, F.interpolate(bilinear,
    align_corners=False), .flip(-1) where flipped."""
    out = []
    for b, i in enumerate(index):
        im = torch.from_numpy(images[i].copy())
        c = im.shape[0]
        m = torch.tensor(mean[:c], dtype=torch.float32).view(c, 1, 1)
        s = torch.tensor(std[:c], dtype=torch.float32).view(c, 1, 1)
        x = F.interpolate(((im.to(torch.float32) / 255 - m) / s)[None], size=(size, size), mode="bilinear", align_corners=False)[0]
        out.append(x.flip(-1) if flip[b] else x)
    return torch.stack(out).numpy()


@functools.lru_cache(maxsize=None)
def reference(channels, size, flipped=True):
    """pool_batch_np of the image list, every image once, odd places flipped: computed once per case, shared, read-only."""
    from deeptreeattention_amd import dead
    images = pool_images(channels, size)
    index = np.arange(len(images))
    flip = case_flips(len(images)) if flipped else None
    x = dead.pool_batch_np(images, index, flip, size=size, mean=MEAN4, std=STD4)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_pool_batch_np_equals_the_torch_pipeline(size, channels):
    from deeptreeattention_amd import dead
    images = pool_images(channels, size)
    assert [im.shape[1:] for im in images] == [(1, 1), (1, 9), (9, 1), (7, 13), (size, size), (300, 280), (56, 56)]
    index = np.arange(len(images))
    flip = case_flips(len(images))
    got = reference(channels, size)
    want = torch_batch(images, index, flip, size, MEAN4, STD4)
    assert got.dtype == np.float32 and got.shape == want.shape == (7, channels, size, size)
    err = float(np.abs(got - want).max())
    print("pool_batch_np vs torch: size", size, "channels", channels, "max abs", err)
    assert err <= CROP_TOL
    # the flip is a reversal of the finished columns: bit-equal to the unflipped crop reversed; an [h][w][C] image is the same
    plain = reference(channels, size, False)
    assert np.array_equal(got[1::2], plain[1::2, :, :, ::-1]) and np.array_equal(got[0::2], plain[0::2])
    if size > 1:
        assert not np.array_equal(got[5], plain[5])
    if channels == 3:
        hwc = [np.ascontiguousarray(im.transpose(1, 2, 0)) if im.shape[1] > 4 else im for im in images]
        assert np.array_equal(dead.pool_batch_np(hwc, [6, 3, 3], [True, False, True], size=size, mean=MEAN4, std=STD4),
                              np.stack([plain[6][:, :, ::-1], plain[3], plain[3][:, :, ::-1]]))


def test_flips_np_is_a_function_of_seed_epoch_and_image():
    from deeptreeattention_amd import _hash, dead
    from deeptreeattention_amd.treedata import epoch_order_np
    n = 4096
    a = dead.flips_np(n, seed=5, epoch=2)
    assert a.dtype == bool and a.shape == (n,)
    # the statement itself, entry by entry, with Python integers
    key = _hash.stream_key(5, 3)
    for i in (0, 1, 77, n - 1):
        z = _hash.mix_int(((2 * n + i) * _hash.GOLDEN + key) & _hash.M64)
        assert bool(a[i]) == ((z >> 40) < (1 << 23))
    assert _hash.STREAM_DEAD_FLIP == 3 and _hash.DEAD_ORDER_LEVEL == 63
    # whatever batch an image lands in, it is flipped or not by its own number: two batch sizes over the same epoch's order
    order = epoch_order_np(n, 2, 5, 63)
    for B in (128, 100):
        seen = np.zeros(n, bool)
        for k in range(0, n, B):
            batch = order[k:k + B]
            seen[batch] = dead.flips_np(n, 5, 2)[batch]
        assert np.array_equal(seen, a)
    assert np.array_equal(a, dead.flips_np(n, seed=5, epoch=2))
    b = dead.flips_np(n, seed=5, epoch=3)
    c = dead.flips_np(n, seed=6, epoch=2)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert 0.4 < float((a != b).mean()) < 0.6
    # a fair coin over 4,096 images: five standard deviations (0.5 / 64 each) are 0.039
    for f in (a, b, c):
        share = float(f.mean())
        print("flipped share", share)
        assert abs(share - 0.5) <= 0.04
    with pytest.raises(ValueError, match="at least 1"):
        dead.flips_np(0)


# ---------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------
def loss_cases():
    """name -> (logits float32 [B, 2], labels int64 [B]): B = 1, 257, 4097; logits at +-40; ties; labels 2 and -1 among
    valid ones; no valid row."""
    rng = np.random.default_rng(11)
    cases = {}
    for B in (1, 257, 4097):
        cases["B{}".format(B)] = (rng.uniform(-8, 8, (B, 2)).astype(np.float32), rng.integers(0, 2, B))
    cases["saturated"] = (np.array([(40, 40), (40, -40), (-40, 40), (-40, -40), (40, 0.5), (-40, -0.5)], np.float32),
                          np.array([0, 1, 1, 0, 1, 0]))
    t = rng.uniform(-3, 3, 64).astype(np.float32)
    cases["ties"] = (np.stack([t, t], 1), rng.integers(0, 2, 64))
    y = rng.integers(0, 2, 300)
    y[::7] = 2
    y[3::11] = -1
    cases["bad_labels"] = (rng.uniform(-8, 8, (300, 2)).astype(np.float32), y)
    cases["no_valid_row"] = (rng.uniform(-8, 8, (5, 2)).astype(np.float32), np.array([2, -1, 7, 2, -5]))
    return {k: (l, np.asarray(y, np.int64)) for k, (l, y) in cases.items()}


def torch_loss(l, y, dtype):
    """(row losses, mean, B_valid * d mean / d logits, conf) from F.cross_entropy(torch.sigmoid(l), y) and autograd on the
    CPU, over the rows with a label in {0, 1}."""
    ok = (y == 0) | (y == 1)
    lt = torch.from_numpy(l).to(dtype).requires_grad_(True)
    rows = np.zeros(len(l))
    grad = np.zeros(l.shape)
    mean = 0.0
    if ok.any():
        idx = torch.from_numpy(np.flatnonzero(ok))
        r = F.cross_entropy(torch.sigmoid(lt[idx]), torch.from_numpy(y[ok]), reduction="none")
        r.mean().backward()
        rows[ok] = r.detach().double().numpy()
        mean = float(r.detach().double().mean())
        grad = lt.grad.double().numpy() * int(ok.sum())
    conf = np.zeros((2, 2), np.int64)
    for t, p in zip(y[ok], np.argmax(l[ok], 1)):
        conf[t, p] += 1
    return rows, mean, grad, conf


@pytest.mark.parametrize("name", list(loss_cases()))
def test_loss_np_equals_torch_in_float64(name):
    from deeptreeattention_amd import dead
    l, y = loss_cases()[name]
    rows, mean, d, conf = dead.loss_np(l, y)
    assert rows.dtype == np.float32 and d.dtype == np.float32 and conf.dtype == np.int64 and isinstance(mean, np.float32)
    assert rows.shape == (len(l),) and d.shape == l.shape and conf.shape == (2, 2)
    wrows, wmean, wgrad, wconf = torch_loss(l, y, torch.float64)
    frows, fmean, fgrad, _ = torch_loss(l, y, torch.float32)
    bv = int(((y == 0) | (y == 1)).sum())
    errs = (float(np.abs(rows - wrows).max()), abs(float(mean) - wmean), float(np.abs(d.astype(np.float64) * bv - wgrad).max()))
    own = (float(np.abs(frows - wrows).max()), abs(fmean - wmean), float(np.abs(fgrad - wgrad).max()))
    print(name, "loss_np vs float64 torch: rows, mean, B * grad", errs, "| float32 torch's own deviation", own)
    assert max(errs) <= LOSS_TOL
    assert np.array_equal(conf, wconf) and int(conf.sum()) == bv
    bad = ~((y == 0) | (y == 1))
    assert not rows[bad].any() and not d[bad].any()
    if name == "saturated":
        # sigmoid(40) is exactly 1.0 in float32, so s * (1 - s) and the gradient are exactly 0; at -40 s is 4e-18 and the
        # gradient is of that size: not a float32 zero, but far below anything an update sees
        assert (d[l == 40] == 0).all() and float(np.abs(d[l == -40]).max()) < 1e-17
    if name == "ties":
        assert conf[:, 1].sum() == 0                              # a tie predicts class 0
    if name == "no_valid_row":
        assert mean == 0 and not d.any() and not conf.any()
    if name == "bad_labels":
        assert bad.sum() == len(y) - conf.sum() > 40
    # any float dtype is widened exactly
    lb = torch.from_numpy(l).to(torch.bfloat16)
    a, b = dead.loss_np(lb, y), dead.loss_np(lb.float().numpy(), torch.from_numpy(y))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_report_np_and_its_zero_denominators():
    from deeptreeattention_amd import dead
    r = dead.report_np(6.0, 12, [[5, 1], [2, 4]])
    assert r["val_loss"] == 0.5 and r["accuracy"] == 9 / 12 and r["class_accuracy"] == [5 / 6, 4 / 6] and r["precision"] == 4 / 5
    r = dead.report_np(0.0, 0, [[0, 0], [0, 0]])
    assert (r["val_loss"], r["accuracy"], r["class_accuracy"], r["precision"]) == (0.0, 0.0, [0.0, 0.0], 0.0)
    assert dead.report_np(1.0, 3, [[3, 0], [0, 0]])["precision"] == 0.0          # nothing predicted Dead: evaluate's convention


# ---------------------------------------------------------------------------------------------------------------------
# the precision-recall curve
# ---------------------------------------------------------------------------------------------------------------------
HAND_Y = np.array([0, 1, 1, 0, 1])
HAND_S = np.array([0.1, 0.4, 0.35, 0.8, 0.8])


def pr_cases():
    rng = np.random.default_rng(2)
    s = np.round(rng.random(200), 1)                             # eleven distinct scores: ties
    return {"ties": (rng.integers(0, 2, 200), s), "no_positive": (np.zeros(30, np.int64), rng.random(30)),
            "all_positive": (np.ones(30, np.int64), rng.random(30)), "one_row": (np.array([1]), np.array([0.3])),
            "one_negative_row": (np.array([0]), np.array([0.3])), "float32_scores": (rng.integers(0, 2, 99), rng.random(99).astype(np.float32)),
            "hand": (HAND_Y, HAND_S)}


@pytest.mark.parametrize("name", list(pr_cases()))
def test_pr_curve_np_equals_sklearn(name):
    import warnings
    metrics = pytest.importorskip("sklearn.metrics")
    from deeptreeattention_amd import dead
    y, s = pr_cases()[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # "No positive class found in y_true"
        want = metrics.precision_recall_curve(y, s)
    got = dead.pr_curve_np(y, s)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    assert got[0].dtype == got[1].dtype == np.float64 and len(got[0]) == len(got[1]) == len(got[2]) + 1


def test_pr_curve_np_and_the_threshold_on_a_hand_made_case():
    """Five rows, written out: thresholds 0.1, 0.35, 0.4, 0.8; at score >= t there are (3, 2), (3, 1), (2, 1), (1, 1)
    (positives, negatives)."""
    from deeptreeattention_amd import dead
    p, r, t = dead.pr_curve_np(HAND_Y, HAND_S)
    assert t.tolist() == [0.1, 0.35, 0.4, 0.8]
    assert p.tolist() == [3 / 5, 3 / 4, 2 / 3, 1 / 2, 1.0]
    assert r.tolist() == [1.0, 1.0, 2 / 3, 1 / 3, 0.0]
    assert dead.threshold_for_precision(HAND_Y, HAND_S, 0.6) == 0.1
    assert dead.threshold_for_precision(HAND_Y, HAND_S, 0.61) == 0.35
    assert dead.threshold_for_precision(HAND_Y, HAND_S, 0.75) == 0.35
    assert dead.threshold_for_precision(HAND_Y, HAND_S, 0.76) is None          # the appended (1, 0) is no threshold
    assert dead.threshold_for_precision(torch.tensor(HAND_Y), torch.tensor(HAND_S), 0.0) == 0.1
    pn, rn, tn = dead.pr_curve_np(np.zeros(3, np.int64), np.array([0.2, 0.1, 0.2]))
    assert pn.tolist() == [0.0, 0.0, 1.0] and rn.tolist() == [1.0, 1.0, 0.0] and tn.tolist() == [0.1, 0.2]
    with pytest.raises(ValueError, match="non-empty"):
        dead.pr_curve_np([], [])


# ---------------------------------------------------------------------------------------------------------------------
# the pool on the host: packing, from_folder, argument errors
# ---------------------------------------------------------------------------------------------------------------------
def host_pool(channels=3, S=8):
    """An ImagePool adopted from host tensors: every check is the device pool's, a call that passes them is refused for
    want of a device."""
    from deeptreeattention_amd.dead import ImagePool
    images = pool_images(channels, S)
    data, table = ImagePool._pack(images, np.arange(len(images)) % 2)
    return ImagePool.resident(torch.from_numpy(data), torch.from_numpy(table)), images, data, table


def test_packing_layout_and_refusals():
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dead import ImagePool
    pool, images, data, table = host_pool()
    assert len(pool) == 7 and pool.channels == 3 and pool.labels.tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert data.dtype == np.uint8 and table.dtype == np.int64 and table.shape == (7, 4)
    at = 0
    for im, (off, h, w, label) in zip(images, table):
        assert (off, h, w) == (at, im.shape[1], im.shape[2]) and np.array_equal(data[off:off + im.size], im.reshape(-1))
        at += im.size
    assert at == len(data)
    # an [h][w][C] image is stored planar
    hwc = np.ascontiguousarray(images[3].transpose(1, 2, 0))
    d2, t2 = ImagePool._pack([hwc], [1])
    assert np.array_equal(d2, images[3].reshape(-1)) and t2.tolist() == [[0, 7, 13, 1]]
    with pytest.raises(ValueError, match="at least one image"):
        ImagePool._pack([], [])
    with pytest.raises(ValueError, match="channels"):
        ImagePool._pack([images[0], np.zeros((1, 5, 5), np.uint8)], [0, 1])
    with pytest.raises(ValueError, match="one integer per image"):
        ImagePool._pack(images, [0, 1])
    with pytest.raises(ValueError, match="one integer per image"):
        ImagePool._pack(images[:2], [0.5, 1.0])
    with pytest.raises(ValueError, match="uint8"):
        ImagePool._pack([images[0].astype(np.float32)], [0])
    with pytest.raises(ValueError, match="at most"):
        ImagePool._pack([images[0]] * (_lib.EPOCH_ORDER_MAX_N + 1), np.zeros(_lib.EPOCH_ORDER_MAX_N + 1, np.int64))
    wide = torch.tensor([[0, 1 << 16, 1 << 15, 0]])             # h * w = 2^31 (refused from the table: no such image is built)
    with pytest.raises(ValueError, match="2\\^31"):
        ImagePool.resident(torch.zeros(16, dtype=torch.uint8), wide)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        ImagePool(images, np.zeros(7, np.int64), device="cpu")
    with pytest.raises(ValueError, match="back to back"):
        ImagePool.resident(torch.from_numpy(data[:-1].copy()), torch.from_numpy(table))
    with pytest.raises(ValueError, match="int64"):
        ImagePool.resident(torch.from_numpy(data), torch.from_numpy(table.astype(np.int32)))


def test_from_folder_follows_image_folder(tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    from deeptreeattention_amd import dead_train
    from deeptreeattention_amd.dead import ImagePool
    rng = np.random.default_rng(8)
    files = {"Dead/b.png": (5, 9), "Alive/z.png": (25, 31), "Alive/a.png": (7, 3), "Alive/sub/k.PNG": (4, 4), "Dead/a.png": (12, 12),
             "Alive/m.png": (1, 6)}
    pixels = {}
    for name, (h, w) in files.items():
        os.makedirs(tmp_path / os.path.dirname(name), exist_ok=True)
        pixels[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(pixels[name]).save(tmp_path / name, format="PNG")
    Image.fromarray(pixels["Dead/b.png"][:, :, 0]).save(tmp_path / "Dead" / "grey.png")      # one channel: decoded as RGB
    (tmp_path / "Alive" / "notes.txt").write_text("not an image")
    (tmp_path / "readme.md").write_text("not a class")
    got = {}

    def capture(self, images, labels, device="cuda", classes=None):
        got.update(images=images, labels=labels, device=device, classes=classes)
        self.classes = classes
    monkeypatch.setattr(ImagePool, "__init__", capture)          # the upload needs a device; what is uploaded is checked here
    pool = ImagePool.from_folder(tmp_path, device="cuda:0")
    order = ["Alive/a.png", "Alive/m.png", "Alive/z.png", "Alive/sub/k.PNG", "Dead/a.png", "Dead/b.png", "Dead/grey.png"]
    assert pool.classes == ["Alive", "Dead"] and got["device"] == "cuda:0"
    assert [os.path.relpath(p, tmp_path) for p in pool.paths] == order
    assert got["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1] and got["labels"].dtype == np.int64
    for name, im in zip(order[:-1], got["images"]):
        assert im.dtype == np.uint8 and np.array_equal(im, pixels[name].transpose(2, 0, 1)), name
    grey = pixels["Dead/b.png"][:, :, 0]
    assert np.array_equal(got["images"][-1], np.stack([grey] * 3))
    with pytest.raises(FileNotFoundError, match="no class directories"):
        ImagePool.from_folder(tmp_path / "Alive" / "sub")
    os.makedirs(tmp_path / "empty" / "Alive")
    with pytest.raises(FileNotFoundError, match="no image files"):
        ImagePool.from_folder(tmp_path / "empty")
    assert dead_train.IMG_EXTENSIONS[:3] == (".jpg", ".jpeg", ".png")


def test_python_route_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached."""
    from deeptreeattention_amd import _lib, dead

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    pool, images, _, _ = host_pool()
    idx = np.array([0, 3, 6])
    for bad in (np.array([0, 7]), np.array([-1, 2]), torch.tensor([7])):                     # outside the pool, host route
        with pytest.raises(IndexError, match="outside the pool"):
            pool.batch(bad, size=8)
    for bad in (idx.astype(np.float32), idx[:0], idx[None], [[0.5]]):
        with pytest.raises(ValueError, match="index"):
            pool.batch(bad, size=8)
    for bad in (np.array([1, 0]), np.array([1.0, 0.0, 1.0]), np.array([1, 0, 1], np.int64)):
        with pytest.raises(ValueError, match="flip"):
            pool.batch(idx, flip=bad, size=8)
    for size in (0, -1, dead.MAX_SIZE + 1):
        with pytest.raises(ValueError, match="size"):
            pool.batch(idx, size=size)
    with pytest.raises(ValueError, match="dtype"):
        pool.batch(idx, size=8, dtype=torch.float64)
    with pytest.raises(ValueError, match="std"):
        pool.batch(idx, size=8, std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="out must be"):
        pool.batch(idx, size=8, out=torch.zeros(3, 3, 8, 9))
    with pytest.raises(ValueError, match="out must be"):                                      # the wrong memory format
        pool.batch(idx, size=8, channels_last=True, out=torch.zeros(3, 3, 8, 8))
    with pytest.raises(ValueError, match="out must be"):
        pool.batch(idx, size=8, out=torch.zeros(3, 3, 8, 8).contiguous(memory_format=torch.channels_last))
    with pytest.raises(ValueError, match="batch_size"):
        pool.loader(0)
    with pytest.raises(ValueError, match="drop_last"):
        pool.loader(8, drop_last=True)
    with pytest.raises(ValueError, match="size"):
        pool.loader(4, size=600)
    with pytest.raises(RuntimeError, match="ROCm device only"):                               # no fallback
        pool.batch(idx, flip=np.array([True, False, True]), size=8)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        pool.loader(4, shuffle=True, train=True)
    y = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="logits"):
        dead.loss(torch.zeros(4, 3), y)
    with pytest.raises(ValueError, match="dtype"):
        dead.loss(torch.zeros(4, 2, dtype=torch.float64), y)
    with pytest.raises(ValueError, match="labels"):
        dead.loss(torch.zeros(4, 2), y.to(torch.int32))
    with pytest.raises(ValueError, match="labels"):
        dead.loss(torch.zeros(4, 2), y[:3])
    with pytest.raises(ValueError, match="DeadAccumulator"):
        dead.loss(torch.zeros(4, 2), y, accumulate=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dead.loss(torch.zeros(4, 2), y, accumulate=dead.DeadAccumulator("cpu"))
    with pytest.raises(ValueError, match="ImagePool"):
        dead.fit(torch.nn.Linear(2, 2), images)
    with pytest.raises(ValueError, match="ImagePool"):
        dead.validate(torch.nn.Linear(2, 2), images)
    acc = dead.DeadAccumulator("cpu")
    r = acc.read()
    assert (r["loss_sum"], r["rows"], r["bad"]) == (0.0, 0, 0) and r["conf"].shape == (2, 2) and not r["conf"].any()


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from deeptreeattention_amd import _hash, _lib, build
    import deeptreeattention_amd as pkg
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    for name, nargs in (("dta_image_pool_batch", 21), ("dta_dead_loss", 9)):
        assert name in names and hasattr(lib, name) and '"{}"'.format(name) in entry
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is C.c_int
    assert "dead_train.hip" in build.SOURCES and "rgb_crops_dev.h" in build.HEADERS
    for macro, value in (("DTA_DEAD_FLIP_STREAM", _lib.DEAD_FLIP_STREAM), ("DTA_DEAD_ORDER_LEVEL", _lib.DEAD_ORDER_LEVEL),
                         ("DTA_DEAD_ACC_WORDS", _lib.DEAD_ACC_WORDS), ("DTA_DEAD_LOSS_MAX_ROWS", _lib.DEAD_LOSS_MAX_ROWS)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value
    assert (_hash.STREAM_DEAD_FLIP, _hash.DEAD_ORDER_LEVEL) == (_lib.DEAD_FLIP_STREAM, _lib.DEAD_ORDER_LEVEL) == (3, 63)
    assert _lib.DEAD_ORDER_LEVEL < _lib.EPOCH_ORDER_MAX_LEVEL_ID
    table = open(os.path.join(REPO, "deeptreeattention_amd", "csrc", "hash_dev.h")).read()
    assert "DTA_DEAD_FLIP_STREAM" in table and "DTA_DEAD_ORDER_LEVEL" in table
    assert pkg.ImagePool is pkg.dead.ImagePool and pkg.DeadAccumulator is pkg.dead_train.DeadAccumulator


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the pointers are host buffers nobody dereferences."""
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 1)
    off4 = C.c_void_p(p.value + 4)
    half = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    zero = (C.c_float * 4)(0.5, 0.0, 0.5, 0.5)
    nan = (C.c_float * 4)(0.5, 0.5, float("nan"), 0.5)

    def err():
        return lib.dta_last_error().decode()

    def batch(data=p, data_bytes=64, table=p, n=4, channels=3, index=p, index64=0, start=0, count=2, flip=None, hash_flips=0,
              size=8, mean=half, std=half, dtype=0, channels_last=0, out=p, labels=p):
        return lib.dta_image_pool_batch(data, data_bytes, table, n, channels, index, index64, start, count, flip, hash_flips, 0, 0,
                                        size, mean, std, dtype, channels_last, out, labels, None)

    for kw in ({"data": None}, {"table": None}, {"mean": None}, {"std": None}, {"out": None}, {"labels": None}):
        assert batch(**kw) != 0 and "dta_image_pool_batch" in err() and "null" in err(), kw
    for kw, what in (({"size": 0}, "size="), ({"size": -4}, "size="), ({"size": 513}, "size="), ({"channels": 0}, "channels="),
                     ({"channels": 5}, "channels="), ({"count": 0}, "count="), ({"count": -3}, "count="), ({"count": 2 ** 31}, "count="),
                     ({"dtype": 3}, "dtype="), ({"dtype": -1}, "dtype="), ({"out": odd}, "aligned"), ({"out": odd, "dtype": 1}, "aligned"),
                     ({"n": 0}, "n="), ({"n": 2 ** 20 + 1}, "n="), ({"data_bytes": 0}, "data_bytes="), ({"start": -1}, "start="),
                     ({"index": None, "start": 3, "count": 2}, "past the pool"), ({"flip": p, "hash_flips": 1}, "exclude"),
                     ({"std": zero}, "std="), ({"std": nan}, "std="), ({"mean": nan}, "mean=")):
        assert batch(**kw) != 0 and "dta_image_pool_batch" in err() and what in err(), (kw, err())

    def loss(logits=p, dtype=0, labels=p, rows=4, out=p, dl=p, counts=p, acc=None):
        return lib.dta_dead_loss(logits, dtype, labels, rows, out, dl, counts, acc, None)

    for kw in ({"logits": None}, {"labels": None}, {"out": None}, {"dl": None}, {"counts": None}):
        assert loss(**kw) != 0 and "dta_dead_loss" in err() and "null" in err(), kw
    for kw, what in (({"rows": 0}, "rows="), ({"rows": -1}, "rows="), ({"rows": 2 ** 24 + 1}, "rows="), ({"dtype": 3}, "dtype="),
                     ({"dtype": -2}, "dtype="), ({"acc": off4}, "aligned")):
        assert loss(**kw) != 0 and "dta_dead_loss" in err() and what in err(), (kw, err())
