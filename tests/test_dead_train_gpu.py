"""Training the alive/dead classifier on the device (dta_image_pool_batch, dta_dead_loss; dead.ImagePool, dead.loss,
dead.DeadAccumulator, dead.fit, dead.validate) against the host definitions (dead.pool_batch_np, flips_np, loss_np), on the
cases of tests/test_dead_train_cpu.py, and bit for bit against the parent's kernel (RgbRaster.crops).

Tolerances: float32 crops within CROP_TOL = 1e-5 of pool_batch_np (test_dead_cpu.py's derivation); bfloat16 / float16 crops
within 1e-5 + 2^-8 |v| / 1e-5 + 2^-11 |v|, one rounding of the float32 result; the loss's mean and B * gradient within 1e-6 of
loss_np (test_dead_train_cpu.py); counts identical.  With 16-bit logits the float32 gradient the launch wrote is held to
1e-6, and the gradient autograd hands on, which is that one rounded to the logits' dtype, to one such rounding: 2^-8 / 2^-11
of its value, and for float16 half a step of its subnormals (2^-25) where a gradient entry lies below 2^-14 -- d_logits carries
the 1 / B of the mean, so entries of a large batch do."""
import functools

import numpy as np
import pytest
import torch

from test_dead_cpu import CROP_TOL, MEAN4, STD4, StandIn
from test_dead_train_cpu import LOSS_TOL, case_flips, loss_cases, pool_images, reference

pytestmark = pytest.mark.gpu
KW = dict(mean=MEAN4, std=STD4)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def resident(channels, size):
    from deeptreeattention_amd.dead import ImagePool
    images = pool_images(channels, size)
    return ImagePool(images, np.arange(len(images)) + 10, device=dev())           # label = image number + 10


def close(x, want, what, rel=0.0):
    assert x.is_cuda and tuple(x.shape) == want.shape, what
    got = x.float().cpu().numpy()
    excess = np.abs(got - want) - rel * np.abs(want)
    print(what, "max abs difference", float(np.abs(got - want).max()), "max over the relative part", float(excess.max()))
    assert float(excess.max()) <= CROP_TOL, what


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("size", (224, 30, 7, 8))
def test_pool_batches_equal_the_definition(size, channels):
    """The seven images in one pool: contiguous and channels_last, with and without flips, host and device index, out=."""
    pool = resident(channels, size)
    flipped, plain = reference(channels, size), reference(channels, size, False)
    n = len(pool)
    index, flip = np.arange(n), case_flips(n)
    labels = torch.arange(10, 10 + n)
    x, y = pool.batch(index, size=size, **KW)
    assert x.dtype == torch.float32 and x.is_contiguous() and y.dtype == torch.int64 and y.is_cuda
    close(x, plain, "host index, no flips")
    assert torch.equal(y.cpu(), labels)
    dindex = torch.from_numpy(index).to(dev())
    x, y = pool.batch(dindex, flip=flip, size=size, channels_last=True, **KW)
    assert x.is_contiguous(memory_format=torch.channels_last) and tuple(x.shape) == (n, channels, size, size)
    close(x, flipped, "device int64 index, host flips, channels_last")
    assert torch.equal(y.cpu(), labels)
    x, y = pool.batch(dindex.to(torch.int32), flip=torch.from_numpy(flip).to(dev()), size=size, **KW)
    close(x, flipped, "device int32 index, device bool flips")
    x, y = pool.batch(index.astype(np.int32), flip=torch.from_numpy(flip.astype(np.uint8)).to(dev()), size=size, channels_last=True, **KW)
    close(x, flipped, "device uint8 flips")
    # a permuted index with repeats, the labels with it
    perm = np.array([6, 0, 0, 5, 3, 1, 2, 4, 6])
    x, y = pool.batch(perm, flip=np.zeros(9, bool), size=size, **KW)
    close(x, plain[perm], "a permuted index")
    assert y.cpu().tolist() == (perm + 10).tolist()
    # out=: written in place, nothing next to it touched
    for cl in (False, True):
        fmt = torch.channels_last if cl else torch.contiguous_format
        big = torch.full((n + 2, channels, size, size), 7.0, device=dev()).contiguous(memory_format=fmt)
        x, y = pool.batch(dindex, flip=flip, size=size, channels_last=cl, out=big[1:n + 1], **KW)
        assert x.data_ptr() == big[1].data_ptr()
        close(x, flipped, "out=, channels_last {}".format(cl))
        assert bool((big[0] == 7.0).all()) and bool((big[n + 1] == 7.0).all())
    if channels > 1:                                             # (with one channel the two memory formats coincide)
        with pytest.raises(ValueError, match="out must be"):
            pool.batch(index, size=size, out=big[1:n + 1], **KW)     # channels_last memory where contiguous is asked for
    # a device index outside the pool: zeros and label -1, the rest as ever
    x, y = pool.batch(torch.tensor([2, n, -1, 3], device=dev()), size=size, **KW)
    assert y.cpu().tolist() == [12, -1, -1, 13] and not bool(x[1:3].any())
    close(x[[0, 3]], plain[[2, 3]], "next to an index outside the pool")


@pytest.mark.parametrize("dtype,rel", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_sixteen_bit_batches_are_one_rounding_of_the_float32_result(dtype, rel):
    for channels, size in ((3, 224), (3, 30), (3, 7), (4, 8), (1, 8)):
        pool = resident(channels, size)
        want = reference(channels, size)
        for cl in (False, True):
            x, _ = pool.batch(np.arange(len(pool)), flip=case_flips(len(pool)), size=size, dtype=dtype, channels_last=cl, **KW)
            assert x.dtype == dtype
            close(x, want, "{} C={} size={} channels_last={}".format(dtype, channels, size, cl), rel=rel)


@pytest.mark.parametrize("channels,size", [(3, 224), (3, 30), (1, 7), (4, 8)])
def test_batches_equal_the_parents_kernel_bit_for_bit(channels, size):
    """No tolerance: every image alone in an RgbRaster, cropped whole by dta_rgb_crops, is the pool's unflipped crop, and the
    flipped crop is its reversal."""
    from deeptreeattention_amd.dead import RgbRaster
    pool = resident(channels, size)
    images = pool_images(channels, size)
    n = len(images)
    for cl in (False, True):
        x, _ = pool.batch(np.arange(n), size=size, channels_last=cl, **KW)
        f, _ = pool.batch(np.arange(n), flip=np.ones(n, bool), size=size, channels_last=cl, **KW)
        assert torch.equal(f, x.flip(-1))
        for i, im in enumerate(images):
            c, valid = RgbRaster(im, device=dev()).crops(np.array([(0, 0, im.shape[1], im.shape[2])]), size=size, pad=0,
                                                         channels_last=cl, **KW)
            assert bool(valid.all()) and torch.equal(c[0], x[i]), (i, cl)


@pytest.mark.parametrize("B,size", [(1025, 8), (120, 224)])
def test_more_units_of_work_than_workgroups(B, size):
    """1025 places at size 8 are one unit each, one above the cap of workgroups; 120 at size 224 are nine units each (1080):
    workgroups go from one image's last rows to the next image's first."""
    from deeptreeattention_amd import dead
    units = B * dead.launch_plan(B, size, 3)[1]
    assert dead.MAX_GROUPS == 1024 and dead.MAX_GROUPS < units < 2 * dead.MAX_GROUPS
    pool = resident(3, size)
    rng = np.random.default_rng(B)
    index, flip = rng.integers(0, len(pool), B), rng.random(B) < 0.5
    plain = reference(3, size, False)
    want = np.where(flip[:, None, None, None], plain[index][:, :, :, ::-1], plain[index])
    x, y = pool.batch(torch.from_numpy(index).to(dev()), flip=flip, size=size, **KW)
    close(x, want, "{} places at size {}".format(B, size))
    assert y.cpu().tolist() == (index + 10).tolist()
    if size == 8:
        x, y = pool.batch(index, flip=flip, size=size, dtype=torch.bfloat16, channels_last=True, **KW)
        close(x, want, "bf16 channels_last", rel=2.0 ** -8)


def test_a_pool_of_one_image_and_a_short_last_batch():
    from deeptreeattention_amd import dead
    im = pool_images(3, 8)[3]
    one = dead.ImagePool([im], [1], device=dev())
    got = list(one.loader(4, size=8, **KW))
    assert len(got) == 1 and got[0][1].cpu().tolist() == [1]
    close(got[0][0], dead.pool_batch_np([im], [0], None, size=8, **KW), "one image")
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (3, int(h), int(w)), dtype=np.uint8) for h, w in rng.integers(2, 40, (10, 2))]
    pool = dead.ImagePool(images, np.arange(10) % 2, device=dev())
    want = dead.pool_batch_np(images, np.arange(10), None, size=8, **KW)
    got = list(pool.loader(4, size=8, **KW))
    assert [tuple(x.shape) for x, _ in got] == [(4, 3, 8, 8), (4, 3, 8, 8), (2, 3, 8, 8)]
    close(torch.cat([x for x, _ in got]), want, "n = 10 in batches of 4")
    assert torch.cat([y for _, y in got]).cpu().tolist() == (np.arange(10) % 2).tolist()
    got = list(pool.loader(4, drop_last=True, size=8, channels_last=True, dtype=torch.float16, **KW))
    assert len(got) == 2 and got[1][0].dtype == torch.float16 and got[1][0].is_contiguous(memory_format=torch.channels_last)
    close(torch.cat([x for x, _ in got]), want[:8], "drop_last, float16", rel=2.0 ** -11)


def test_the_loader_follows_the_epochs_order_and_flips():
    """shuffle and train over two epochs: the labels (the image numbers) come back in epoch_order_np's order, the flipped
    images are flips_np's, every image appears once per epoch."""
    from deeptreeattention_amd import dead
    from deeptreeattention_amd.treedata import epoch_order_np
    n, B, S, seed = 23, 5, 8, 4
    rng = np.random.default_rng(6)
    images = [rng.integers(0, 256, (3, int(h), int(w)), dtype=np.uint8) for h, w in rng.integers(3, 30, (n, 2))]
    pool = dead.ImagePool(images, np.arange(n), device=dev())
    plain = dead.pool_batch_np(images, np.arange(n), None, size=S, **KW)
    orders = []
    for epoch in (0, 1):
        order, flips = epoch_order_np(n, epoch, seed, 63), dead.flips_np(n, seed, epoch)
        orders.append(order)
        got = list(pool.loader(B, shuffle=True, train=True, seed=seed, epoch=epoch, size=S, **KW))
        assert [len(y) for _, y in got] == [5, 5, 5, 5, 3] and all(x.is_cuda and y.is_cuda for x, y in got)
        y = torch.cat([y for _, y in got]).cpu().numpy()
        assert np.array_equal(y, order) and np.array_equal(np.sort(y), np.arange(n))
        x = torch.cat([x for x, _ in got])
        close(x, np.where(flips[order][:, None, None, None], plain[order][:, :, :, ::-1], plain[order]), "epoch {}".format(epoch))
        assert 0 < flips.sum() < n                               # (a wrong flip of these images costs far more than CROP_TOL)
        # train alone flips in the pool's own order; shuffle alone does not flip
        x = torch.cat([x for x, _ in pool.loader(B, train=True, seed=seed, epoch=epoch, size=S, **KW)])
        close(x, np.where(flips[:, None, None, None], plain[:, :, :, ::-1], plain), "train only")
        x = torch.cat([x for x, _ in pool.loader(B, shuffle=True, seed=seed, epoch=epoch, size=S, **KW)])
        close(x, plain[order], "shuffle only")
    assert not np.array_equal(orders[0], orders[1])


# ---------------------------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(loss_cases()))
def test_loss_equals_the_definition(name):
    from deeptreeattention_amd import dead
    l, y = loss_cases()[name]
    yd = torch.from_numpy(y).to(dev())
    for dtype, rel, tiny in ((torch.float32, 0.0, 0.0), (torch.bfloat16, 2.0 ** -8, 0.0), (torch.float16, 2.0 ** -11, 2.0 ** -25)):
        lh = torch.from_numpy(l).to(dtype)                       # the definition gets the same rounded values
        _, mean, d, conf = dead.loss_np(lh, y)
        bv = int(conf.sum())
        ld = lh.to(dev()).requires_grad_(True)
        acc = dead.DeadAccumulator(dev())
        out = dead.loss(ld, yd, accumulate=acc)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 0 and out.requires_grad
        wrote = out.grad_fn.saved_tensors[0]                     # the float32 gradient the forward launch wrote
        out.backward()
        assert ld.grad.dtype == dtype and wrote.dtype == torch.float32
        e_mean = abs(float(out.detach()) - float(mean))
        e_wrote = float(np.abs(wrote.cpu().numpy().astype(np.float64) - d).max()) * bv
        excess = (np.abs(ld.grad.double().cpu().numpy() - d) - rel * np.abs(d) - tiny).max() * bv
        print(name, dtype, "mean", e_mean, "B * written gradient", e_wrote, "B * handed-on gradient over one rounding", float(excess))
        assert e_mean <= LOSS_TOL and e_wrote <= LOSS_TOL and excess <= LOSS_TOL
        r = acc.read()
        assert np.array_equal(r["conf"], conf) and r["bad"] == len(y) - bv and r["rows"] == bv
        # a rerun gives the same bits; an incoming gradient scales what is handed on
        l2 = lh.to(dev()).requires_grad_(True)
        out2 = dead.loss(l2, yd)
        assert torch.equal(out2, out) and torch.equal(out2.grad_fn.saved_tensors[0], wrote)
        (out2 * 3.0).backward()
        assert torch.equal(l2.grad, (wrote * 3.0).to(dtype))
        if name == "saturated":
            assert not bool(ld.grad[torch.from_numpy(l == 40).to(dev())].any())
        if name == "no_valid_row":
            assert float(out.detach()) == 0.0 and not bool(ld.grad.any())


def test_the_accumulator_sums_three_batches():
    from deeptreeattention_amd import dead
    cases = loss_cases()
    acc = dead.DeadAccumulator(dev())
    loss_sum, rows, conf, bad = 0.0, 0, np.zeros((2, 2), np.int64), 0
    for name in ("B257", "bad_labels", "ties"):
        l, y = cases[name]
        with torch.no_grad():
            out = dead.loss(torch.from_numpy(l).to(dev()), torch.from_numpy(y).to(dev()), accumulate=acc)
        assert not out.requires_grad
        r, _, _, c = dead.loss_np(l, y)
        loss_sum, rows, conf, bad = loss_sum + float(r.astype(np.float64).sum()), rows + int(c.sum()), conf + c, bad + len(y) - int(c.sum())
    got, rep = acc.read(), acc.report()
    assert np.array_equal(got["conf"], conf) and got["rows"] == rows and got["bad"] == bad > 0
    print("accumulated val_loss", rep["val_loss"], "definition", loss_sum / rows)
    assert abs(rep["val_loss"] - loss_sum / rows) <= LOSS_TOL
    want = dead.report_np(loss_sum, rows, conf)
    assert rep["accuracy"] == want["accuracy"] and rep["class_accuracy"] == want["class_accuracy"] and rep["precision"] == want["precision"]
    acc.reset()
    assert acc.read()["rows"] == 0 and acc.read()["loss_sum"] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_with_a_stand_in_classifier():
    """Two epochs on a 40-image train pool and a 12-image val pool at size 16, in batches of 20 (few batch shapes: the
    convolution library tunes itself for every new one, which is most of this test's time).  A forward hook keeps every
    input batch and its logits: the training batches are pool_batch_np of that epoch's order and flips, val_loss and the
    confusion are loss_np of the validation logits, lr is torch's scheduler's, and only the epoch ends hold host numbers."""
    from deeptreeattention_amd import dead
    from deeptreeattention_amd.treedata import epoch_order_np
    S, B, seed, epochs = 16, 20, 9, 2
    rng = np.random.default_rng(12)

    def make(n):
        images = [rng.integers(0, 256, (3, int(h), int(w)), dtype=np.uint8) for h, w in rng.integers(4, 40, (n, 2))]
        labels = rng.integers(0, 2, n)
        for im, lab in zip(images, labels):                      # something to learn: Dead images are darker
            im //= int(1 + 2 * lab)
        return images, labels
    train_images, train_labels = make(40)
    val_images, val_labels = make(12)
    train_pool = dead.ImagePool(train_images, train_labels, device=dev())
    val_pool = dead.ImagePool(val_images, val_labels, device=dev())
    torch.manual_seed(3)
    model = StandIn().to(dev())
    seen = []
    model.register_forward_hook(lambda m, inp, out: seen.append((m.training, inp[0].detach().clone(), out.detach().clone())))
    lines = []
    history = dead.fit(model, train_pool, val_pool, epochs=epochs, lr=1e-2, batch_size=B, seed=seed, size=S, log=lines.append)
    assert len(history) == epochs == len(lines) and all(a is b for a, b in zip(lines, history))
    assert [t for t, _, _ in seen] == [True, True, False] * epochs
    assert all(x.is_cuda and out.is_cuda and tuple(out.shape) == (x.shape[0], 2) for _, x, out in seen)
    sched_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(sched_opt, mode="min", factor=0.5, patience=10)
    for epoch, row in enumerate(history):
        order, flips = epoch_order_np(40, epoch, seed, 63), dead.flips_np(40, seed, epoch)
        batches = seen[3 * epoch:3 * epoch + 3]
        for k, (_, x, _) in enumerate(batches[:2]):
            idx = order[k * B:(k + 1) * B]
            assert x.shape[0] == len(idx) == 20
            close(x, dead.pool_batch_np(train_images, idx, flips[idx], size=S), "epoch {} batch {}".format(epoch, k))
        close(batches[2][1], dead.pool_batch_np(val_images, np.arange(12), None, size=S), "validation batch")
        rows, _, _, conf = dead.loss_np(batches[2][2], val_labels)
        want = dead.report_np(float(rows.astype(np.float64).sum()), 12, conf)
        print("epoch", epoch, "val_loss", row["val_loss"], "definition", want["val_loss"], "train_loss", row["train_loss"])
        assert abs(row["val_loss"] - want["val_loss"]) <= LOSS_TOL and np.array_equal(row["conf"], conf)
        assert (row["accuracy"], row["class_accuracy"], row["precision"]) == (want["accuracy"], want["class_accuracy"], want["precision"])
        train_rows = np.concatenate([dead.loss_np(out, train_labels[order[k * B:(k + 1) * B]])[0] for k, (_, _, out) in enumerate(batches[:2])])
        assert abs(row["train_loss"] - float(train_rows.astype(np.float64).mean())) <= LOSS_TOL
        assert row["lr"] == sched_opt.param_groups[0]["lr"] and row["epoch"] == epoch
        sched.step(row["val_loss"])
        assert all(type(row[k]) is float for k in ("train_loss", "val_loss", "accuracy", "precision", "lr"))
        assert all(type(v) is float for v in row["class_accuracy"])
    assert history[1]["train_loss"] < history[0]["train_loss"]          # Adam at 1e-2 on separable images: the loss falls
    assert model.training
    # validate alone, with the scores: dead.head of the logits per image, and the labels
    rep, label, score, true = dead.validate(model, val_pool, batch_size=6, size=S, scores=True)
    assert label.is_cuda and score.is_cuda and true.is_cuda and model.training
    assert torch.equal(true.cpu(), torch.from_numpy(val_labels))
    logits = torch.cat([out for t, _, out in seen[3 * epochs:]])
    assert logits.shape[0] == 12 and [t for t, _, _ in seen[3 * epochs:]] == [False] * 2
    want_label, want_score = dead.head_np(logits)
    assert np.array_equal(label.cpu().numpy(), want_label) and float(np.abs(score.cpu().numpy() - want_score).max()) <= 1e-6
    assert int(rep["conf"].sum()) == 12 and rep["bad"] == 0
    p, r, t = dead.pr_curve_np(true, score)
    assert len(p) == len(t) + 1 and p[-1] == 1.0 and r[-1] == 0.0


def test_a_pool_from_a_folder(tmp_path):
    """ImageFolder's rule end to end: PNGs of different sizes under Alive/ and Dead/, decoded once, batched on the device."""
    Image = pytest.importorskip("PIL.Image")
    from deeptreeattention_amd import dead
    rng = np.random.default_rng(21)
    files = {"Dead/b.png": (5, 9), "Alive/z.png": (25, 31), "Alive/a.png": (7, 3), "Dead/a.png": (12, 12)}
    pixels = {}
    for name, (h, w) in files.items():
        (tmp_path / name).parent.mkdir(exist_ok=True)
        pixels[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(pixels[name]).save(tmp_path / name)
    pool = dead.ImagePool.from_folder(tmp_path, device=dev())
    order = ["Alive/a.png", "Alive/z.png", "Dead/a.png", "Dead/b.png"]
    assert pool.classes == ["Alive", "Dead"] and len(pool) == 4 and pool.labels.tolist() == [0, 0, 1, 1]
    assert list(zip(pool.heights.tolist(), pool.widths.tolist())) == [files[k] for k in order]
    x, y = pool.batch(np.arange(4), flip=[False, True, True, False], size=16)
    close(x, dead.pool_batch_np([pixels[k] for k in order], np.arange(4), [False, True, True, False], size=16), "from_folder")
    assert y.cpu().tolist() == [0, 0, 1, 1]
