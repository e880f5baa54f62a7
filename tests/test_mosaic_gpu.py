"""mosaic on the device equals the definition (mosaic.nms_np, mosaic.pixel_boxes_np) exactly: status, winner, boxes and
pixel_boxes, at box counts around a workgroup and an LDS chunk, at a chain of decisions far deeper than the parallel rounds,
on cell edges, for every status, into poisoned buffers, under permutation and on a rerun; predict_tile with a stored
detector; and the chain mosaic -> canopy -> abundance against the same chain over the NumPy definitions."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mosaic_cases as MC
from deeptreeattention_amd import mosaic as M

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def reference(c, iou_threshold=0.15):
    status, winner, tile = M.nms_np(iou_threshold=iou_threshold, **MC.nms_args(c))
    return status, winner, tile, M.pixel_boxes_np(tile, c["height"], c["width"])


def run(c, to_device=False, **kw):
    args = MC.nms_args(c)
    if to_device:
        args = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev()) if isinstance(v, np.ndarray) else v) for k, v in args.items()}
    return M.mosaic(height=c["height"], width=c["width"], **args, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_equal(m, ref):
    status, winner, tile, pixel = ref
    assert m.status.dtype == torch.uint8 and m.winner.dtype == torch.int32 and m.boxes.dtype == torch.float32
    assert m.pixel_boxes.dtype == torch.int32 and m.keep.dtype == torch.bool
    got = [t.cpu().numpy() for t in m]
    assert np.array_equal(got[0], status)
    assert np.array_equal(got[1], winner)
    assert np.array_equal(bits(got[2]), bits(tile))
    assert np.array_equal(got[3], pixel)
    assert np.array_equal(m.keep.cpu().numpy(), status == 1)


@functools.lru_cache(maxsize=None)
def named(name):
    c = {"scene36": MC.scene36, "staircase": lambda: MC.staircase(3000), "staircase_ties": lambda: MC.staircase(3000, ties=True),
         "cell_edges": MC.cell_edges, "column": MC.column, "all_statuses": MC.all_statuses}[name]()
    return c, reference(c)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257, 1000))
def test_box_counts_around_a_wave_and_a_workgroup(n):
    c = MC.scattered(n, 100 + n)
    ref = reference(c)
    if n >= 63:
        assert (ref[0] == 1).any() and (ref[0] == 0).any()
    assert_equal(run(c), ref)


def test_the_36_window_scene():
    c, ref = named("scene36")
    status, winner = ref[0], ref[1]
    dropped = np.flatnonzero(status == 0)
    assert 4000 < len(status) < 4800 and (status == 1).sum() > 1000 and len(dropped) > 300
    assert (c["window"][dropped] != c["window"][winner[dropped]]).sum() > 100       # duplicates of the overlap strips
    assert (c["scores"][dropped] == c["scores"][winner[dropped]]).any()              # ties, decided by the index
    assert M.grid(len(status), c["height"], c["width"], c["max_side"])[1] > 2
    assert_equal(run(c), ref)
    assert_equal(run(c, to_device=True), ref)
    for rounds in (0, 1, 2, 3, 5):                             # the tail alone; rounds by cells; the first rounds by list
        assert_equal(run(c, rounds=rounds), ref)


@pytest.mark.parametrize("name", ("staircase", "staircase_ties"))
def test_a_chain_deeper_than_the_rounds_is_finished_by_the_tail(name):
    c, ref = named(name)
    status, depth = M.nms_fixpoint_np(**MC.nms_args(c))
    assert depth > 4 * M.ROUNDS and np.array_equal(status, ref[0])
    assert (ref[0][0::2] == 1).all() and (ref[0][1::2] == 0).all()
    assert_equal(run(c), ref)
    m = run(c, tail=False)                                     # without the tail launch the rounds alone do not get there
    left = (m.status == M.UNDECIDED).sum().item()
    assert left > 0 and ((m.status.cpu().numpy() == ref[0]) | (m.status.cpu().numpy() == M.UNDECIDED)).all()
    assert_equal(run(c, rounds=0), ref)                        # the tail alone


@pytest.mark.parametrize("name", ("cell_edges", "column"))
def test_cell_edges_corners_and_a_tile_one_cell_wide(name):
    c, ref = named(name)
    cell, gx, gy = M.grid(len(c["boxes"]), c["height"], c["width"], c["max_side"])
    if name == "column":
        assert gx == 1 and gy > 100
    else:
        cx = (c["boxes"][:, 0] + c["boxes"][:, 2]) * np.float32(0.5)
        cy = (c["boxes"][:, 1] + c["boxes"][:, 3]) * np.float32(0.5)
        on_x, on_y = cx % np.float32(cell) == 0, cy % np.float32(cell) == 0
        assert (on_x & on_y).sum() >= 25 and (on_x & ~on_y).sum() >= 25
        s, w = ref[0], ref[1]
        d = np.flatnonzero(s == 0)
        ix, iy = np.floor(cx / cell), np.floor(cy / cell)
        assert ((ix[d] != ix[w[d]]) & (iy[d] != iy[w[d]])).any() and ((ix[d] != ix[w[d]]) & (iy[d] == iy[w[d]])).any()
    assert (ref[0] == 0).any() and (ref[0] == 1).any()
    assert_equal(run(c), ref)


@pytest.mark.parametrize("n", (M.CHUNK - 1, M.CHUNK, M.CHUNK + 1))
def test_a_single_cell_with_more_boxes_than_one_lds_stage(n):
    from deeptreeattention_amd import _lib
    assert M.CHUNK == _lib.MOSAIC_CHUNK
    c = MC.one_cell(n, 6)
    assert M.grid(n, c["height"], c["width"], c["max_side"])[1:] == (1, 1)
    ref = reference(c)
    assert (ref[0] == 0).sum() > 100 and (ref[0] == 1).sum() > 100
    assert_equal(run(c), ref)


@pytest.mark.parametrize("use_mask", (False, True))
@pytest.mark.parametrize("use_window", (False, True))
def test_all_statuses_with_mask_and_window_on_and_off(use_mask, use_window):
    c, _ = named("all_statuses")
    c = dict(c)
    if not use_mask:
        c["mask"] = None
    if not use_window:
        c["window"] = c["origins"] = None
    ref = reference(c)
    want = {0, 1, 3} | ({2} if use_mask else set())
    assert set(np.unique(ref[0]).tolist()) == want
    assert (ref[0][:MC.REFUSED_ROWS - (0 if use_window else 2)] == 3).all()
    assert_equal(run(c), ref)
    assert_equal(run(c, to_device=True), ref)
    if use_window:                                             # int64 indices, one of them a multiple of 2^32 off a valid one
        c64 = dict(c, window=c["window"].astype(np.int64))
        c64["window"][8] = (1 << 32) + 1
        ref64 = reference(c64)
        assert ref64[0][8] == 3
        assert_equal(run(c64), ref64)
        assert_equal(run(c64, to_device=True), ref64)
        if use_mask:
            cb = dict(c, mask=c["mask"].astype(bool))
            assert_equal(run(cb, to_device=True), ref)


def test_every_output_element_is_written_and_none_beyond():
    """Through the C entry with buffers of this test's own: 0xFF everywhere first, n rows after, 0xFF still behind them."""
    from deeptreeattention_amd import _lib
    c, _ = named("all_statuses")
    L = _lib.lib()
    total = len(c["boxes"])
    assert total >= 1000
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev()) for k in ("boxes", "scores", "window", "origins", "mask")}
    for n in (1, 65, 257, 1000):
        sub = dict(c, boxes=c["boxes"][:n], scores=c["scores"][:n], window=c["window"][:n], mask=c["mask"][:n])
        status, winner, tile, pixel = reference(sub)
        pad = 320
        out_s = torch.full((n + pad,), 0xFF, dtype=torch.uint8, device=dev())
        out_w = torch.full((n + pad,), -1, dtype=torch.int32, device=dev())                  # (every byte 0xFF)
        out_b = torch.full(((n + pad) * 16,), 0xFF, dtype=torch.uint8, device=dev())
        out_p = torch.full(((n + pad) * 16,), 0xFF, dtype=torch.uint8, device=dev())
        need = L.dta_mosaic_workspace_bytes(n, c["height"], c["width"], 400.0)
        ws = torch.empty(need, dtype=torch.uint8, device=dev())
        opt = _lib.MosaicOptions(c["height"], c["width"], len(c["origins"]), 400.0, 0.15, -1, 0)
        _lib.check(L.dta_mosaic(_lib.ptr(d["boxes"]), _lib.ptr(d["scores"]), _lib.ptr(d["window"]), _lib.ptr(d["origins"]),
                                _lib.ptr(d["mask"]), n, C.byref(opt), _lib.ptr(out_s), _lib.ptr(out_w), _lib.ptr(out_b),
                                _lib.ptr(out_p), _lib.ptr(ws), need, _lib.current_stream_ptr()), "dta_mosaic")
        s, w = out_s.cpu().numpy(), out_w.cpu().numpy()
        b, p = out_b.cpu().numpy(), out_p.cpu().numpy()
        assert np.array_equal(s[:n], status) and (s[n:] == 0xFF).all()
        assert np.array_equal(w[:n], winner) and (w[n:].view(np.uint8) == 0xFF).all()
        assert np.array_equal(b[:16 * n].view(np.uint32).reshape(n, 4), bits(tile)) and (b[16 * n:] == 0xFF).all()
        assert np.array_equal(p[:16 * n].view(np.int32).reshape(n, 4), pixel) and (p[16 * n:] == 0xFF).all()
        short = L.dta_mosaic(_lib.ptr(d["boxes"]), _lib.ptr(d["scores"]), None, None, None, n, C.byref(opt), _lib.ptr(out_s),
                             _lib.ptr(out_w), _lib.ptr(out_b), _lib.ptr(out_p), _lib.ptr(ws), need - 16, _lib.current_stream_ptr())
        assert short == 1 and b"workspace" in L.dta_last_error()


def test_a_permuted_input_gives_the_permuted_result():
    c, _ = named("scene36")
    rng = np.random.default_rng(11)
    n = len(c["boxes"])
    scores = (rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1)       # distinct
    c = dict(c, scores=scores)
    ref = reference(c)
    perm = rng.permutation(n)
    inverse = np.empty(n, np.int64)
    inverse[perm] = np.arange(n)
    p = dict(c, boxes=np.ascontiguousarray(c["boxes"][perm]), scores=scores[perm], window=c["window"][perm])
    m = run(p)
    got = [t.cpu().numpy() for t in m]
    assert np.array_equal(got[0], ref[0][perm]) and np.array_equal(bits(got[2]), bits(ref[2][perm]))
    assert np.array_equal(got[3], ref[3][perm])
    w = ref[1][perm]
    assert np.array_equal(got[1], np.where(w >= 0, inverse[np.maximum(w, 0)], -1))
    assert_equal(run(c), ref)


def test_two_calls_are_bit_identical():
    c, _ = named("scene36")
    a, b = run(c, to_device=True), run(c, to_device=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.float32 else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype != torch.float32 else y.view(torch.int32))


def test_predict_tile_with_a_stored_detector():
    c, _ = named("scene36")
    wins = M.windows(c["height"], c["width"])
    image = torch.zeros((c["height"], c["width"], 3), dtype=torch.uint8, device=dev())
    for k, (x, y, w, h) in enumerate(wins.tolist()):           # every window's view starts on a pixel that names the window
        image[y, x, 0], image[y, x, 1] = k % 251, k // 251
    boxes, scores = torch.from_numpy(c["boxes"]).to(dev()), torch.from_numpy(c["scores"]).to(dev())
    index = torch.from_numpy(c["window"]).to(dev())
    calls = []

    def detect(views):
        calls.append(len(views))
        out = []
        for v in views:
            assert tuple(v.shape) == (400, 400, 3) and v.dtype == torch.uint8
            k = int(v[0, 0, 0]) + 251 * int(v[0, 0, 1])
            out.append({"boxes": boxes[index == k], "scores": scores[index == k]})
        return out
    m = M.predict_tile(detect, image, batch=8)
    assert calls == [8, 8, 8, 8, 4]
    order = np.argsort(c["window"], kind="stable")             # the driver concatenates window by window
    assert np.array_equal(order, np.arange(len(order)))
    assert_equal(m, reference(c))
    t = 0.4
    masked = M.predict_tile(detect, image, batch=36, score_threshold=t)
    assert_equal(masked, reference(dict(c, mask=(c["scores"] > np.float32(t)).astype(np.uint8))))
    empty = M.predict_tile(lambda views: [{"boxes": boxes[:0], "scores": scores[:0]} for _ in views], image)
    assert empty.status.shape == (0,) and empty.pixel_boxes.shape == (0, 4)


def test_mosaic_feeds_canopy_and_abundance():
    """m.keep and m.pixel_boxes go straight into CanopyRaster.crown_height; keep & height_keep into abundance.counts."""
    from deeptreeattention_amd import abundance, canopy
    c, ref = named("scene36")
    rng = np.random.default_rng(21)
    chm = (rng.uniform(0, 1, (c["height"] // 20 + 1, c["width"] // 20 + 1)) * 9).astype(np.float32).repeat(20, 0).repeat(20, 1)
    chm = np.ascontiguousarray(chm[:c["height"], :c["width"]])
    label = rng.integers(-1, 12, len(c["boxes"])).astype(np.int64)
    m = run(c, to_device=True)
    raster = canopy.CanopyRaster(chm, device=dev())
    heights = raster.crown_height(m.pixel_boxes, rule=canopy.MinHeight(3))
    counts = abundance.counts(torch.from_numpy(label).to(dev()), 10, mask=m.keep & heights.keep)
    h_np, _ = canopy.crown_height_np(chm, ref[3])
    keep_np = (ref[0] == 1) & canopy.min_height_np(h_np, 3.0)
    want = abundance.counts_np(label, 10, mask=keep_np)
    assert 0 < keep_np.sum() < (ref[0] == 1).sum()
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal((m.keep & heights.keep).cpu().numpy(), keep_np)
