"""Dense per-pixel window prediction, host side (no GPU): the pure host functions of deeptreeattention_amd.dense against
literal restatements, the equivalence the design rests on (preprocessing commutes with window slicing, bit for bit), and
the four new C-ABI symbols."""
import os
import re

import numpy as np

from oracle import preprocess_np as PP
from oracle import prng

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dta_raster_normalise", "dta_gather_windows", "dta_gather_windows_tiles", "dta_crown_reduce")


def test_window_origins_against_a_double_loop():
    from deeptreeattention_amd.dense import window_origins
    boxes = [(2, 3, 6, 5), (0, 0, 1, 7), (4, 4, 4, 9), (10, -2, 13, 1)]      # the third box is empty
    corner, off = window_origins(boxes, anchor="corner")
    want = []
    for r0, c0, r1, c1 in boxes:
        for r in range(r0, r1):
            for c in range(c0, c1):
                want.append((r, c))
    assert corner.dtype == np.int32 and corner.shape == (len(want), 2)
    assert off.dtype == np.int64 and off.shape == (len(boxes) + 1,)
    assert corner.tolist() == [list(w) for w in want]
    areas = [(r1 - r0) * (c1 - c0) for r0, c0, r1, c1 in boxes]
    assert np.diff(off).tolist() == areas                    # counts are the box areas
    assert off.tolist() == [0] + np.cumsum(areas).tolist()   # offsets the cumulative areas
    assert off[3] == off[2]                                  # an empty box: an empty group
    center, off_c = window_origins(boxes, anchor="center")
    assert np.array_equal(center, corner - 5) and np.array_equal(off_c, off)
    center7, _ = window_origins(boxes, anchor="center", size=7)
    assert np.array_equal(center7, corner - 3)
    none, off0 = window_origins([], anchor="corner")
    assert none.shape == (0, 2) and off0.tolist() == [0]


def _padded_windows(raster, origins, size, pad):
    """Explicit slicing of a zero-padded copy of the raster."""
    Cb, Hh, Ww = raster.shape
    big = np.zeros((Cb, Hh + 2 * pad, Ww + 2 * pad), dtype=raster.dtype)
    big[:, pad:pad + Hh, pad:pad + Ww] = raster
    return np.stack([big[:, r + pad:r + pad + size, c + pad:c + pad + size] for r, c in origins])


def test_gather_windows_np_against_padded_slicing():
    from deeptreeattention_amd.dense import gather_windows_np
    raster = prng.uniform01(7, 1, (5, 17, 13)).astype(np.float32) + 0.25      # no zeros inside: the fill is visible
    origins = np.array([(-5, -5), (0, 0), (3, 4), (17 - 6, 13 - 6), (16, 12), (-11, 2), (40, 40), (6, -3)], dtype=np.int32)
    got = gather_windows_np(raster, origins, 11)
    want = _padded_windows(raster, origins, 11, 64)
    assert got.dtype == np.float32 and got.shape == (len(origins), 5, 11, 11)
    assert np.array_equal(got, want)
    assert (got[0, :, :5, :] == 0).all() and (got[0, :, :, :5] == 0).all() and (got[0, :, 5:, 5:] != 0).all()
    assert (got[3, :, 6:, :] == 0).all() and (got[3, :, :, 6:] == 0).all() and (got[3, :, :6, :6] != 0).all()   # far corner
    assert (got[5] == 0).all() and (got[6] == 0).all()                        # entirely outside
    assert np.array_equal(gather_windows_np(raster, origins, 7), _padded_windows(raster, origins, 7, 64))


def test_preprocessing_commutes_with_window_slicing_bit_for_bit():
    """40 raw int16 bands at 17x13, one constant pixel: preprocess(window) == window(preprocess(raster)), every window of
    the raster anchored at its centre (so all four edges and corners are overrun), compared as bit patterns."""
    from deeptreeattention_amd.dense import gather_windows_np, window_origins
    raw = (prng.uniform01(11, 1, (40, 17, 13)) * 6000 - 500).astype(np.int16)
    raw[:, 4, 9] = 1234                                                       # a constant pixel (range 0 -> scale 1)
    raw[:, 0, 0] = 0                                                          # and an all-zero one, like the fill
    origins, _ = window_origins([(0, 0, 17, 13)], anchor="center")
    origins = np.concatenate([origins, np.array([(-5, -5), (17 - 6, 13 - 6), (-10, 3), (12, 12)], dtype=np.int32)])
    whole = PP.preprocess_image(raw)
    assert whole.shape == (20, 17, 13) and whole.dtype == np.float32
    assert (whole[:, 4, 9] == 0).all()
    from_raster = gather_windows_np(whole, origins, 11)
    raw_windows = _padded_windows(raw, origins, 11, 32)                       # what a boundless read returns
    for n in range(len(origins)):
        per_window = PP.preprocess_image(raw_windows[n])
        assert per_window.dtype == np.float32
        assert np.array_equal(per_window.view(np.uint32), from_raster[n].view(np.uint32)), origins[n]
    # ... and through the whole of load_image (the NEAREST resize of an 11x11 window to 11x11 is the identity)
    if hasattr(PP, "load_image"):
        assert np.array_equal(PP.load_image(raw_windows[0], 11).view(np.uint32), from_raster[0].view(np.uint32))


def test_crown_reduce_np_against_mean_and_stable_argsort():
    from deeptreeattention_amd.dense import crown_reduce_np
    classes = 9
    p = prng.uniform01(5, 1, (23, classes)).astype(np.float32)
    p /= p.sum(axis=1, keepdims=True)
    p[7:10] = 0
    p[7:10, 6] = 0.5; p[7:10, 2] = 0.5                                        # crown 2: a tie between classes 2 and 6
    p[22] = 0
    p[22, 4] = 0.25; p[22, 1] = 0.25; p[22, 8] = 0.25; p[22, 0] = 0.25          # crown 5 (one window): a four-way tie
    offsets = np.array([0, 4, 7, 10, 10, 22, 23], dtype=np.int64)             # crown 3 is empty
    mean, top_idx, top_score, count = crown_reduce_np(p, offsets)
    assert mean.dtype == np.float32 and top_idx.dtype == np.int64 and top_score.dtype == np.float32 and count.dtype == np.int32
    assert count.tolist() == np.diff(offsets).tolist()
    for k in range(len(offsets) - 1):
        rows = p[offsets[k]:offsets[k + 1]]
        if len(rows) == 0:
            assert (mean[k] == 0).all() and top_idx[k].tolist() == [-1, -1] and top_score[k].tolist() == [0, 0]
            continue
        assert np.allclose(mean[k], rows.astype(np.float64).mean(axis=0), rtol=1e-6, atol=1e-7)
        order = np.argsort(-mean[k], kind="stable")[:2]
        assert top_idx[k].tolist() == order.tolist()
        assert np.array_equal(top_score[k], mean[k][order])
    assert top_idx[2].tolist() == [2, 6] and top_score[2].tolist() == [0.5, 0.5]
    assert top_idx[5].tolist() == [0, 1]
    assert np.array_equal(mean[5], p[22])                                     # one window: the mean is the row itself


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= names
    from deeptreeattention_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for n in NEW_SYMBOLS:
            assert hasattr(L, n), n
        # null and bad arguments are reported, not dereferenced (no launch happens)
        assert L.dta_raster_normalise(None, 40, 4, 4, 10, 0, 0, None, None) != 0
        assert b"null argument" in L.dta_last_error()
        assert L.dta_gather_windows(None, 20, 4, 4, None, 1, 11, None, None) != 0
        assert L.dta_gather_windows_tiles(None, 20, 4, 4, None, 1, 11, None, None) != 0
        assert L.dta_crown_reduce(None, None, 1, 2, None, None, None, None, None) != 0
        assert b"dta_crown_reduce" in L.dta_last_error()


def test_package_exports_and_imports_without_a_gpu():
    import deeptreeattention_amd as pkg
    for n in ("DenseRaster", "window_origins", "predict_windows", "predict_map"):
        assert hasattr(pkg, n), n
