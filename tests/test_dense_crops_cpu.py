"""Crops of crown boxes out of a resident raster, host side (no GPU): `dense.gather_crops_np` -- the written-down meaning
of dta_gather_crops -- against the reference's own crops (tests/golden/preprocess.npz) pasted into one raster, and against
oracle/preprocess_np.py's load_crop of host-sliced raw boxes; the resize index against torch's own NEAREST; `crop_boxes`;
the three new C entry points are declared, exported, bound and refuse bad arguments before anything is launched.
Every float comparison is on bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import preprocess_np as PP
from oracle import prng

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dta_gather_crops", "dta_gather_crops_tiles", "dta_gather_crops_years")
MOSAIC_H, MOSAIC_W = 29, 31
# where the golden's five crops (three 5x7, two 8x7) sit in the mosaic: the four corners and the middle
MOSAIC_AT = ((0, 0), (0, 24), (24, 0), (21, 24), (10, 12))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def load_golden():
    return np.load(os.path.join(REPO, "tests", "golden", "preprocess.npz"))


def mosaic(g):
    """The five real reference crops pasted into one 369 x 29 x 31 int16 raster (the rest: a synthetic spectrum per pixel).
    Returns (raw raster, boxes int32 [5, 4], names)."""
    names = list(g["names"])
    u = prng.uniform01(53, 1, (369, MOSAIC_H, MOSAIC_W))
    raw = (u * 5000 + 40 * np.arange(369)[:, None, None]).astype(np.int16)
    boxes = []
    for name, (r, c) in zip(names, MOSAIC_AT):
        crop = g[f"{name}/raw"]
        h, w = crop.shape[1:]
        raw[:, r:r + h, c:c + w] = crop
        boxes.append((r, c, r + h, c + w))
    assert boxes[1][3] == MOSAIC_W and boxes[2][2] == MOSAIC_H and boxes[3][2:] == (MOSAIC_H, MOSAIC_W)
    return raw, np.array(boxes, dtype=np.int32), names


# the whole raster, 23x17 (downsampling), 1x1, a 12x1 strip, an 11x11 box
OTHER_BOXES = np.array([(0, 0, MOSAIC_H, MOSAIC_W), (3, 9, 26, 26), (14, 30, 15, 31), (8, 5, 20, 6), (9, 10, 20, 21)], dtype=np.int32)


def test_mosaic_of_reference_crops_equals_the_golden_as_bits():
    from deeptreeattention_amd.dense import gather_crops_np
    g = load_golden()
    raw, boxes, names = mosaic(g)
    whole = PP.preprocess_image(raw)
    assert whole.shape == (349, MOSAIC_H, MOSAIC_W) and whole.dtype == np.float32
    got = gather_crops_np(whole, boxes, 11)
    assert got.shape == (5, 349, 11, 11) and got.dtype == np.float32
    for k, name in enumerate(names):
        assert np.array_equal(bits(got[k]), bits(g[f"{name}/resized11"])), name
    got24 = gather_crops_np(whole, boxes[:1], 24)
    assert np.array_equal(bits(got24[0]), bits(g[f"{names[0]}/resized24"]))


def test_other_boxes_equal_load_crop_of_the_sliced_raw_raster():
    from deeptreeattention_amd.dense import gather_crops_np, gather_windows_np
    raw, _, _ = mosaic(load_golden())
    whole = PP.preprocess_image(raw)
    assert [(int(b[2] - b[0]), int(b[3] - b[1])) for b in OTHER_BOXES] == [(29, 31), (23, 17), (1, 1), (12, 1), (11, 11)]
    for flip in (False, True):
        got = gather_crops_np(whole, OTHER_BOXES, 11, flip=flip)
        for k, (r0, c0, r1, c1) in enumerate(OTHER_BOXES):
            want = PP.load_crop(raw[:, r0:r1, c0:c1], 11, train=flip)
            assert np.array_equal(bits(got[k]), bits(want)), (k, flip)
    plain, flipped = gather_crops_np(whole, OTHER_BOXES, 11), gather_crops_np(whole, OTHER_BOXES, 11, flip=True)
    assert np.array_equal(bits(flipped), bits(plain[:, :, ::-1, ::-1])) and not np.array_equal(bits(flipped[0]), bits(plain[0]))
    # an 11x11 box resized to 11x11 is the window at its origin
    assert np.array_equal(bits(plain[4]), bits(gather_windows_np(whole, OTHER_BOXES[4:5, :2], 11)[0]))
    # a box with no rows, no columns, or negative sides: zeros, among boxes that are not
    mixed = np.array([OTHER_BOXES[1], (5, 5, 5, 9), (5, 9, 8, 9), (7, 7, 3, 2), OTHER_BOXES[2]], dtype=np.int32)
    z = gather_crops_np(whole, mixed, 11)
    assert not z[1:4].any() and np.array_equal(bits(z[0]), bits(plain[1])) and np.array_equal(bits(z[4]), bits(plain[2]))
    # a box that was not clipped: the pixels outside the raster are zero
    over = gather_crops_np(whole, np.array([(-11, -11, 11, 11)], dtype=np.int32), 22)[0]
    assert not over[:, :11, :].any() and not over[:, :, :11].any()
    assert np.array_equal(bits(over[:, 11:, 11:]), bits(whole[:, :11, :11]))


@pytest.mark.parametrize("out_size", [11, 24])
def test_resize_index_is_torch_nearest(out_size):
    from deeptreeattention_amd.dense import nearest_index
    for in_size in range(1, 65):
        src = torch.arange(in_size, dtype=torch.float32).reshape(1, 1, in_size, 1)
        want = torch.nn.functional.interpolate(src, size=(out_size, 1), mode="nearest").reshape(-1).numpy().astype(np.int64)
        got = nearest_index(out_size, in_size)
        assert got.dtype == np.int64 and np.array_equal(got, want), in_size
        assert np.array_equal(got, PP.nearest_index(out_size, in_size)), in_size


def test_crop_boxes_clips_raises_and_zero_fills():
    from deeptreeattention_amd.dense import crop_boxes
    H, W = 17, 13
    boxes = [(-3, 2, 4, 6), (12, 2, 20, 6), (5, -4, 9, 3), (5, 10, 9, 19), (-2, -2, 30, 30), (3, 4, 8, 9)]
    got = crop_boxes(boxes, H, W)
    assert got.dtype == np.int32 and got.shape == (6, 4)
    assert got.tolist() == [[0, 2, 4, 6], [12, 2, 17, 6], [5, 0, 9, 3], [5, 10, 9, 13], [0, 0, 17, 13], [3, 4, 8, 9]]
    for k, bad in enumerate([(17, 0, 20, 5), (0, 13, 4, 20), (-5, 0, 0, 4), (2, -6, 4, 0), (4, 4, 4, 8)]):
        with pytest.raises(ValueError, match="box 2 "):
            crop_boxes([boxes[0], boxes[5], bad], H, W)
        z = crop_boxes([boxes[0], boxes[5], bad], H, W, empty="zero")
        assert z.dtype == np.int32 and z.shape == (3, 4)
        assert z[:2].tolist() == [[0, 2, 4, 6], [3, 4, 8, 9]]
        assert z[2, 2] - z[2, 0] <= 0 or z[2, 3] - z[2, 1] <= 0, k          # degenerate: a zero crop
    with pytest.raises(ValueError, match="empty"):
        crop_boxes(boxes, H, W, empty="skip")
    one = crop_boxes((1, 2, 3, 4), H, W)
    assert one.shape == (1, 4) and one.dtype == np.int32


def _aligned(nbytes=256):
    """A host buffer and a 16-byte aligned address inside it: stands in for a device pointer in calls that must be refused
    before anything is dereferenced or launched."""
    buf = np.zeros(nbytes + 16, dtype=np.uint8)
    addr = buf.ctypes.data
    return buf, C.c_void_p(addr + (-addr) % 16)


def test_new_entry_points_are_declared_exported_bound_and_check_their_arguments():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    declared = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None and getattr(L, s).restype is C.c_int, s      # bound in _lib.py
    assert L.dta_abi_version() == 2
    keep, P = _aligned()

    def refused(rc, who):
        assert rc != 0 and who.encode() in L.dta_last_error(), (who, L.dta_last_error())

    for who in ("dta_gather_crops", "dta_gather_crops_tiles"):
        f = getattr(L, who)
        refused(f(None, 20, 4, 4, None, 1, 11, 0, None, None), who)                     # null pointers
        refused(f(None, 20, 4, 4, P, 1, 11, 0, P, None), who)
        refused(f(P, 20, 4, 4, None, 1, 11, 0, P, None), who)
        refused(f(P, 20, 4, 4, P, 1, 11, 0, None, None), who)
        refused(f(P, 20, 4, 4, P, 1, 0, 0, P, None), who)                               # size < 1
        refused(f(P, 20, 4, 4, P, 1, -3, 1, P, None), who)
        refused(f(P, 20, 4, 4, P, 0, 11, 0, P, None), who)                              # n < 1
        refused(f(P, 369, 4, 4, P, 2 ** 31 - 1, 11, 0, P, None), who)                   # too large for one launch
        assert b"too large" in L.dta_last_error()
    who = "dta_gather_crops_years"
    f = L.dta_gather_crops_years
    none = (C.c_void_p * 3)()
    some = (C.c_void_p * 3)(P, None, P)
    flags = (C.c_float * 6)()
    fp, fq = C.cast(flags, C.c_void_p), C.c_void_p(C.addressof(flags) + 12)
    refused(f(None, 3, 20, 4, 4, None, 1, 11, 0, None, None, None, None), who)         # null pointers
    refused(f(some, 3, 20, 4, 4, P, 1, 11, 0, None, fp, fq, None), who)
    refused(f(some, 3, 20, 4, 4, P, 1, 11, 0, some, None, fq, None), who)
    refused(f(some, 3, 20, 4, 4, None, 1, 11, 0, some, fp, fq, None), who)
    refused(f(some, 3, 20, 4, 4, P, 1, 11, 0, none, fp, fq, None), who)                # a present year without an output
    refused(f(some, 3, 20, 4, 4, P, 1, 0, 0, some, fp, fq, None), who)                 # size < 1
    refused(f(some, 3, 20, 4, 4, P, 0, 11, 0, some, fp, fq, None), who)                # n < 1
    refused(f(some, 3, 369, 4, 4, P, 2 ** 31 - 1, 11, 0, some, fp, fq, None), who)     # too large for one launch
    assert b"too large" in L.dta_last_error()
    refused(f(some, 0, 20, 4, 4, P, 1, 11, 0, some, fp, fq, None), who)                # years outside 1..16
    refused(f(some, 17, 20, 4, 4, P, 1, 11, 0, some, fp, fq, None), who)
    assert b"years" in L.dta_last_error()
    refused(f(some, 3, 20, 4, 4, P, 1, 11, 0, some, fp, fp, None), who)                # one bank for both
    refused(f(none, 3, 20, 4, 4, P, 1, 11, 0, some, fp, fq, None), who)                # no year present
    assert b"every year is missing" in L.dta_last_error()
    del keep


def test_package_exports_and_routes_refuse_without_a_device():
    import deeptreeattention_amd as pkg
    from deeptreeattention_amd import dense
    for n in ("crop_boxes", "predict_crops", "predict_crops_multistage", "predict_crops_metadata"):
        assert hasattr(pkg, n) and hasattr(dense, n), n
    for n in ("gather_crops_np", "nearest_index"):
        assert hasattr(dense, n), n
    assert hasattr(dense.DenseRaster, "crops") and hasattr(dense.DenseRaster, "crops_years")
    boxes = np.array([(0, 0, 3, 3)], dtype=np.int32)
    with pytest.raises(TypeError):
        dense.predict_crops_multistage(object(), [None], boxes)
    with pytest.raises(TypeError):
        dense.predict_crops_metadata(object(), None, 0, boxes)
    # share_conv1 is not offered on the crop routes
    import inspect
    for f in (dense.predict_crops, dense.predict_crops_multistage, dense.predict_crops_metadata):
        assert "share_conv1" not in inspect.signature(f).parameters
