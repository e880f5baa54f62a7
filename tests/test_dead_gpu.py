"""Alive/dead crown filter on the device (dta_rgb_crops, dta_dead_head; dead.RgbRaster.crops, dead.head, dead.predict_dead)
against the host definition (dead.crops_np, dead.head_np, dead.filter_dead), on the cases of tests/test_dead_cpu.py.

Tolerances: float32 crops within 1e-5 of crops_np (test_dead_cpu.py's derivation: a few float32 roundings of values in
[-2.12, 2.64] stay under 1e-6, a wrong source index costs 0.017); bfloat16 / float16 crops within 1e-5 + 2^-8 |v| /
1e-5 + 2^-11 |v|, one rounding of the float32 result; scores within 1e-6; labels identical."""
import copy
import functools

import numpy as np
import pytest
import torch

from test_dead_cpu import (CROP_TOL, H, MEAN4, PADS, SIZES, STANDIN_SIZE, STD4, W, case_boxes, head_logits, raster, standin,
                           standin_boxes, standin_cpu_route, standin_tile)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(channels, size, pad):
    """crops_np of the case boxes, computed once per case and shared (nobody writes into it)."""
    from deeptreeattention_amd import dead
    x, valid = dead.crops_np(raster(channels, seed=0 if channels == 3 else channels), case_boxes(size), size=size, pad=pad,
                             mean=MEAN4, std=STD4)
    x.setflags(write=False)
    return x, valid


@functools.lru_cache(maxsize=None)
def resident(channels):
    from deeptreeattention_amd.dead import RgbRaster
    return RgbRaster(raster(channels, seed=0 if channels == 3 else channels), device=dev())


def close(x, valid, want, wvalid, what, rel=0.0):
    assert x.is_cuda and valid.is_cuda and valid.dtype == torch.bool and tuple(x.shape) == want.shape
    assert torch.equal(valid.cpu(), torch.from_numpy(wvalid)), what
    got = x.float().cpu().numpy()
    excess = np.abs(got - want) - rel * np.abs(want)
    print(what, "max abs difference", float(np.abs(got - want).max()), "max over the relative part", float(excess.max()))
    assert float(excess.max()) <= CROP_TOL, what
    assert not got[~wvalid].any(), what


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("size", SIZES)
def test_crops_equal_the_definition(size, pad):
    """The 13 case boxes (N = 13): host boxes, device boxes, out= given, contiguous and channels_last memory."""
    ras = resident(3)
    want, wvalid = reference(3, size, pad)
    boxes = case_boxes(size)
    assert len(boxes) == 13
    kw = dict(size=size, pad=pad, mean=MEAN4, std=STD4)
    x, valid = ras.crops(boxes, **kw)
    assert x.dtype == torch.float32 and x.is_contiguous()
    close(x, valid, want, wvalid, "host boxes")
    dboxes = torch.from_numpy(boxes).to(dev())
    x, valid = ras.crops(dboxes, channels_last=True, **kw)
    assert x.is_contiguous(memory_format=torch.channels_last) and tuple(x.shape) == (13, 3, size, size)
    close(x, valid, want, wvalid, "device boxes, channels_last")
    x, valid = ras.crops(dboxes.to(torch.int64), **kw)
    close(x, valid, want, wvalid, "int64 device boxes")
    # out=: written in place, nothing next to it touched
    big = torch.full((15, 3, size, size), 7.0, device=dev())
    x, valid = ras.crops(boxes, out=big[1:14], **kw)
    assert x.data_ptr() == big[1].data_ptr()
    close(x, valid, want, wvalid, "out=")
    assert bool((big[0] == 7.0).all()) and bool((big[14] == 7.0).all())
    big = torch.full((15, 3, size, size), 7.0, device=dev()).contiguous(memory_format=torch.channels_last)
    x, valid = ras.crops(dboxes, out=big[1:14], channels_last=True, **kw)
    close(x, valid, want, wvalid, "out=, channels_last")
    assert bool((big[0] == 7.0).all()) and bool((big[14] == 7.0).all())
    with pytest.raises(ValueError, match="out must be"):
        ras.crops(boxes, out=big[1:14], **kw)                    # channels_last memory where contiguous is asked for


@pytest.mark.parametrize("channels", [1, 4])
def test_crops_with_one_and_four_channels(channels):
    ras = resident(channels)
    for size in (30, 7, 8):                                      # lines of 30 / 7 / 8 and of 120 / 28 / 32 elements
        want, wvalid = reference(channels, size, 10)
        for cl in (False, True):
            x, valid = ras.crops(case_boxes(size), size=size, pad=10, mean=MEAN4, std=STD4, channels_last=cl)
            close(x, valid, want, wvalid, "C={} size={} channels_last={}".format(channels, size, cl))


@pytest.mark.parametrize("dtype,rel", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_sixteen_bit_crops_are_one_rounding_of_the_float32_result(dtype, rel):
    for channels, size in ((3, 224), (3, 30), (3, 7), (4, 30)):
        ras = resident(channels)
        want, wvalid = reference(channels, size, 10)
        for cl in (False, True):
            x, valid = ras.crops(case_boxes(size), size=size, pad=10, mean=MEAN4, std=STD4, dtype=dtype, channels_last=cl)
            assert x.dtype == dtype
            close(x, valid, want, wvalid, "{} C={} size={} channels_last={}".format(dtype, channels, size, cl), rel=rel)


def test_pixel_interleaved_upload_and_resident_adoption():
    from deeptreeattention_amd.dead import RgbRaster
    tile = raster()
    want, wvalid = reference(3, 30, 10)
    a = RgbRaster(np.ascontiguousarray(tile.transpose(1, 2, 0)), device=dev())
    assert a.shape == (3, H, W)
    close(*a.crops(case_boxes(30), size=30, pad=10, mean=MEAN4, std=STD4), want, wvalid, "[H][W][C] upload")
    t = torch.from_numpy(tile).to(dev())
    b = RgbRaster.resident(t)
    assert b.data.data_ptr() == t.data_ptr()
    close(*b.crops(case_boxes(30), size=30, pad=10, mean=MEAN4, std=STD4), want, wvalid, "resident()")


def many_boxes(n, seed):
    rng = np.random.default_rng(seed)
    r0, c0 = rng.integers(-12, H, n), rng.integers(-12, W, n)
    boxes = np.stack([r0, c0, r0 + rng.integers(-1, 40, n), c0 + rng.integers(-1, 40, n)], 1).astype(np.int32)
    return boxes


@pytest.mark.parametrize("n,size", [(1025, 8), (120, 224)])
def test_more_units_of_work_than_workgroups(n, size):
    """The launch has at most dead.MAX_GROUPS workgroups, each with a contiguous share of the units (whole output rows of
    one crown).  1025 crowns at size 8 are one unit each: one above the cap, some workgroup takes two crowns.  120 crowns at
    size 224 are nine units each (1080): workgroups go from one crown's last rows to the next crown's first."""
    from deeptreeattention_amd import dead
    units = n * dead.launch_plan(n, size, 3)[1]
    assert dead.launch_plan(n, size, 3) == ((8, 1) if size == 8 else (25, 9))
    assert dead.MAX_GROUPS == 1024 and dead.MAX_GROUPS < units < 2 * dead.MAX_GROUPS
    boxes = many_boxes(n, n)
    want, wvalid = dead.crops_np(raster(), boxes, size=size, pad=3)
    assert wvalid.any() and not wvalid.all()
    x, valid = resident(3).crops(torch.from_numpy(boxes).to(dev()), size=size, pad=3)
    close(x, valid, want, wvalid, "{} crowns at size {}".format(n, size))
    if size == 8:
        x, valid = resident(3).crops(boxes, size=size, pad=3, dtype=torch.bfloat16, channels_last=True)
        close(x, valid, want, wvalid, "bf16 channels_last", rel=2.0 ** -8)


def test_head_equals_the_definition():
    from deeptreeattention_amd import dead
    l, nties = head_logits()
    want_label, want_score = dead.head_np(l)
    label, score = dead.head(torch.from_numpy(l).to(dev()))
    assert label.dtype == torch.int64 and score.dtype == torch.float32 and label.is_cuda and score.is_cuda
    assert torch.equal(label.cpu(), torch.from_numpy(want_label))
    err = float((score.cpu() - torch.from_numpy(want_score)).abs().max())
    print("head: max abs score difference", err)
    assert err <= 1e-6
    assert label[-nties:].tolist() == [0] * nties
    # a row offset: a batch is written into the middle of the tile's result arrays, nothing else is touched
    n, off = len(l), 37
    big_label = torch.full((n + 50,), -9, dtype=torch.int64, device=dev())
    big_score = torch.full((n + 50,), -9.0, dtype=torch.float32, device=dev())
    dead._head_into(torch.from_numpy(l).to(dev()), big_label, big_score, off)
    assert torch.equal(big_label[off:off + n], label) and torch.equal(big_score[off:off + n], score)
    assert bool((big_label[:off] == -9).all()) and bool((big_label[off + n:] == -9).all())
    assert bool((big_score[:off] == -9.0).all()) and bool((big_score[off + n:] == -9.0).all())
    # 16-bit logits are widened exactly; the definition gets the same values
    for dtype in (torch.bfloat16, torch.float16):
        lh = torch.from_numpy(l).clamp(-6e4, 6e4).to(dtype)
        want_label, want_score = dead.head_np(lh)
        label, score = dead.head(lh.to(dev()))
        assert torch.equal(label.cpu(), torch.from_numpy(want_label)), dtype
        assert float((score.cpu() - torch.from_numpy(want_score)).abs().max()) <= 1e-6, dtype


class Recorder:
    """The stand-in on the device; keeps the logits of every batch it is called with."""

    def __init__(self, net):
        self.net, self.logits, self.shapes = net, [], []

    def __call__(self, x):
        self.shapes.append((tuple(x.shape), x.dtype, x.is_contiguous(memory_format=torch.channels_last)))
        y = self.net(x)
        self.logits.append(y)
        return y


def test_predict_dead_with_a_stand_in_classifier():
    """50 crowns in batches of 16 (the last one ragged) through conv -> global mean -> linear in eval mode.  The device's
    logits against the same network on the CPU fed by crops_np, within 4 x the CPU's own float32 - float64 difference
    (the two sides run the network through different libraries); labels wherever the CPU's logit gap exceeds that."""
    from deeptreeattention_amd import dead
    cpu_logits, tol = standin_cpu_route()
    gap = np.abs(cpu_logits[:, 0] - cpu_logits[:, 1])
    sure = gap > tol
    assert sure.mean() >= 0.9
    want_label, want_score = dead.head_np(cpu_logits)
    ras = dead.RgbRaster(standin_tile(), device=dev())
    boxes = standin_boxes()
    for cl in (False, True):
        model = Recorder(copy.deepcopy(standin()).to(dev()))
        got = dead.predict_dead(model, ras, boxes, batch_size=16, pad=10, size=STANDIN_SIZE, channels_last=cl)
        assert [s[0][0] for s in model.shapes] == [16, 16, 16, 2] and all(s[1] == torch.float32 for s in model.shapes)
        assert all(s[2] for s in model.shapes) or not cl
        logits = torch.cat(model.logits).cpu().numpy()
        err = float(np.abs(logits - cpu_logits).max())
        print("stand-in logits, device vs CPU: max abs", err, "tolerance", tol, "channels_last", cl)
        assert err <= tol
        assert got.label.dtype == torch.int64 and got.score.dtype == torch.float32 and got.valid.dtype == torch.bool
        assert tuple(got.label.shape) == tuple(got.score.shape) == tuple(got.valid.shape) == (50,)
        assert bool(got.valid.all())
        assert np.array_equal(got.label.cpu().numpy()[sure], want_label[sure])
        assert float(np.abs(got.score.cpu().numpy() - want_score).max()) <= 1e-6 + tol
        assert 0 < int(got.label.sum()) < 50


def test_end_to_end_height_filter_and_dead_filter_in_front_of_the_counts():
    """CanopyRaster.crown_height(...).keep & filter_dead(...) as the mask of abundance.counts: the same counts as the NumPy
    route (crown_height_np / min_height_np, head_np on the classifier's logits, filter_dead, counts_np)."""
    from deeptreeattention_amd import abundance, canopy, dead
    rng = np.random.default_rng(9)
    boxes = standin_boxes(200, seed=4)
    n, species = len(boxes), 12
    chm = rng.uniform(0.0, 2.9, (H, W)).astype(np.float32)
    chm[:, W // 3:] = rng.uniform(0.0, 25.0, (H, W - W // 3)).astype(np.float32)
    ens_label = rng.integers(-1, species, n)
    ens_score = rng.random(n).astype(np.float32)
    # the device route
    heights = canopy.CanopyRaster(chm, device=dev()).crown_height(boxes, rule=canopy.MinHeight(3.0))
    model = Recorder(copy.deepcopy(standin()).to(dev()))
    pred = dead.predict_dead(model, dead.RgbRaster(standin_tile(), device=dev()), boxes, batch_size=64, size=STANDIN_SIZE)
    # the NumPy route, from the logits the classifier gave
    logits = torch.cat(model.logits).cpu().numpy()
    label_np, score_np = dead.head_np(logits)
    order = np.sort(score_np[label_np == 1])
    k = int(np.argmax(np.diff(order)[len(order) // 4:3 * len(order) // 4])) + len(order) // 4
    assert order[k + 1] - order[k] > 1e-5                        # a threshold no score is within 1e-6 of
    threshold = (float(order[k]) + float(order[k + 1])) / 2
    height, _ = canopy.crown_height_np(chm, boxes)
    keep_np = canopy.min_height_np(height, 3.0)
    alive_np, el_np, es_np = dead.filter_dead(label_np, score_np, threshold, ens_label, ens_score)
    want = abundance.counts_np(ens_label, species, mask=keep_np & alive_np)
    dl, ds = torch.from_numpy(ens_label).to(dev()), torch.from_numpy(ens_score).to(dev())
    alive, el, es = dead.filter_dead(pred.label, pred.score, threshold, dl, ds)
    assert alive.dtype == torch.bool and alive.is_cuda
    assert torch.equal(alive.cpu(), torch.from_numpy(alive_np)) and torch.equal(el.cpu(), torch.from_numpy(el_np))
    assert torch.equal(torch.isnan(es).cpu(), torch.from_numpy(np.isnan(es_np)))
    got = abundance.counts(dl, species, mask=heights.keep & alive)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert 0 < int(want.sum()) < int(keep_np.sum()) < n and 0 < int(alive_np.sum()) < n
    # blanking the labels instead of masking them: the dead crowns move to the last bin
    moved = abundance.counts(el, species, mask=heights.keep)
    assert torch.equal(moved[:species].cpu(), torch.from_numpy(want[:species]))
