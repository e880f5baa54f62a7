"""The two identities the raster kernels keep by having ONE definition each (csrc/common.h minmax_*, csrc/dense.hip Src<P>):
the window gather and the crop gather are one body over two source policies, and the three normalising kernels
(dta_raster_normalise, dta_reflectance_normalise, dta_preprocess_crops[_tiles]) scale a pixel with one arithmetic.
All assertions are bit equalities; the fixtures are synthetic."""
import numpy as np
import pytest
import torch

from oracle import prng

BANDS = 23          # not a multiple of 16 (a partial last chunk), and 23 * S * S is not a multiple of 4 for S = 11 and S = 5
EPS = np.finfo(np.float32).eps
TINY = np.float32(10.0) * EPS          # scikit-learn: ranges below 10 * eps(float32) are "constant"


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def bf16(a):
    """float32 -> the bf16-rounded float32: nearest even on the bits, a NaN keeps its sign and stays quiet.  (Written out:
    torch's CPU conversion turns NaN into 0xFFFF, a different NaN from the one IEEE narrowing gives.)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = np.where(np.isnan(a), (u >> 16) | 0x40, r)
    return (r << 16).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# one normalise, three kernels
# ---------------------------------------------------------------------------------------------------------------------
def pixel_kinds(dtype):
    """A [23][2][9] raw raster whose pixels are the kinds the scaling rule tells apart (the rest: noise).
    float32: a constant pixel; ranges one float below 10 * eps, exactly 10 * eps and one float above it, from 0; the same
    threshold 19, 20 and 21 ulps above 0.5 (10 * eps is 20 ulps of 0.5); a pixel with one NaN band.
    int16: ranges are whole numbers, so the only range below the threshold is 0 -- two constant pixels (one of them
    negative) -- and the smallest range above it is 1."""
    if dtype == np.float32:
        a = (prng.uniform01(71, 1, (BANDS, 2, 9)) * 3 - 1).astype(np.float32)
        ramp = np.linspace(0, 1, BANDS, dtype=np.float32)
        a[:, 0, 0] = np.float32(2.5)
        for col, hi in ((1, np.nextafter(TINY, np.float32(0))), (2, TINY), (3, np.nextafter(TINY, np.float32(1)))):
            a[:, 0, col] = ramp * hi
            a[-1, 0, col] = hi
        ulp = np.float32(2.0 ** -24)
        for col, steps in ((4, 19), (5, 20), (6, 21)):
            a[:, 0, col] = np.float32(0.5) + np.float32(steps // 2) * ulp
            a[0, 0, col], a[-1, 0, col] = np.float32(0.5), np.float32(0.5) + np.float32(steps) * ulp
        a[7, 1, 8] = np.nan
    else:
        a = (prng.uniform01(71, 2, (BANDS, 2, 9)) * 9000 - 800).astype(np.int16)
        a[:, 0, 0] = 1234
        a[:, 0, 1] = -7
        a[:, 0, 2] = 100
        a[5, 0, 2] = 101
    return a


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_host_minmax_handles_the_pixel_kinds_as_sklearn_does(dtype):
    """The package's host definition (reflectance.minmax_np) and the oracle's, against scikit-learn's MinMaxScaler on the
    very raster the device test below uses -- so what that test compares with is the reference's arithmetic."""
    sk = pytest.importorskip("sklearn.preprocessing")
    from deeptreeattention_amd.reflectance import minmax_np
    from oracle import preprocess_np as PP
    raw = pixel_kinds(dtype).astype(np.float32)          # the reference: np.asarray(image, dtype='float32')
    c, h, w = raw.shape
    with np.errstate(all="ignore"):
        want = sk.minmax_scale(raw.reshape(c, h * w).T.copy(), axis=1).T.reshape(raw.shape)
    assert want.dtype == np.float32
    for got in (minmax_np(raw), PP.minmax_over_bands(raw)):
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    # the kinds are what they are meant to be: constant and below-threshold pixels come out as value - min, unscaled
    rng = np.nanmax(raw, axis=0) - np.nanmin(raw, axis=0)
    if dtype == np.float32:
        assert [bool(v < TINY) for v in rng[0, :7]] == [True, True, False, False, True, False, False]
        assert np.array_equal(want[:, 0, 1], raw[:, 0, 1]) and not want[:, 0, 0].any()
        assert np.isnan(want[7, 1, 8]) and np.isfinite(np.delete(want[:, 1, 8], 7)).all()
    else:
        assert [float(v) for v in rng[0, :3]] == [0.0, 0.0, 1.0]
        assert not want[:, 0, :2].any() and sorted(set(want[:, 0, 2].tolist())) == [0.0, 1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_one_normalise_three_kernels(dtype, precision):
    """DenseRaster, DenseRaster.from_reflectance of the pixel-interleaved copy and preprocess_batch of the whole raster as
    one crop give the same bits, and those are the host definition's.  (preprocess_batch writes squares: the 2 x 9 raster
    goes in zero-padded to 9 x 9 at size 9, where NEAREST is the identity, as preprocess.preprocess_image pads; the
    padding's pixels are dropped from the comparison.)"""
    from deeptreeattention_amd.dense import DenseRaster
    from deeptreeattention_amd.preprocess import preprocess_batch
    from deeptreeattention_amd.reflectance import minmax_np
    raw = pixel_kinds(dtype)
    c, h, w = raw.shape
    want = minmax_np(raw)
    if precision == "bf16":
        want = bf16(want)
    a = DenseRaster(raw, clip=0, precision=precision, device=dev())
    b = DenseRaster.from_reflectance(np.ascontiguousarray(np.moveaxis(raw, 0, 2)), bands="all", clip=0, precision=precision,
                                     device=dev())
    assert a.shape == b.shape == (BANDS, h, w)
    assert np.array_equal(bits(a.data), bits(b.data))                  # the stored form, the chunk padding included
    padded = np.zeros((c, w, w), dtype=raw.dtype)
    padded[:, :h] = raw
    crop = preprocess_batch([padded], w, clip=0, device=dev(), tiles=precision == "bf16")
    crop = (crop.float() if precision == "bf16" else crop)[0, :, :h]
    for name, got in (("DenseRaster", a.float()), ("from_reflectance", b.float()), ("preprocess_batch", crop)):
        assert np.array_equal(bits(got), bits(want)), name
    if precision == "bf16":      # bands 23 .. 31 of the last chunk are zero
        assert not a.data.view(-1, h * w, 16)[1, :, BANDS - 16:].any()


# ---------------------------------------------------------------------------------------------------------------------
# one gather body, two policies
# ---------------------------------------------------------------------------------------------------------------------
H, W = 12, 13


def gather_raw(seed):
    return (prng.uniform01(seed, 1, (BANDS, H, W)) * 3 - 1).astype(np.float32)


def gather_items(S):
    """Three windows -- interior, over the top-left corner by 3, over the bottom-right corner by 3 -- and the S x S boxes
    that are the same pixels (the NEAREST index of an S x S box at side S is the identity)."""
    origins = np.array([((H - S) // 2, (W - S) // 2), (-3, -3), (H - S + 3, W - S + 3)], dtype=np.int32)
    boxes = np.concatenate([origins, origins + S], axis=1).astype(np.int32)
    return origins, boxes


@pytest.mark.gpu
@pytest.mark.parametrize("S", [11, 5])
def test_one_gather_body_two_policies(S):
    """windows(origins) == crops(S x S boxes at the origins) as bits, in the float32 form, the tile form and the years form
    with one missing year (there also the flags, and clear_next zeroed); both are gather_windows_np of the raster."""
    from deeptreeattention_amd.dense import DenseRaster, gather_windows_np, year_flags_np
    assert (BANDS * S * S) % 4 and BANDS % 16 and (3 * BANDS * S * S) % 4      # lanes straddle items, the last lane is partial
    origins, boxes = gather_items(S)
    raw = gather_raw(83)
    # float32
    r = DenseRaster(raw, clip=0, precision="fp32", device=dev())
    win, crop = r.windows(origins, size=S), r.crops(boxes, size=S)
    want = gather_windows_np(r.float().cpu().numpy(), origins, S)
    assert win.shape == (3, BANDS, S, S) and not want[1, :, :3].any() and not want[2, :, :, -3:].any() and want[0].any()
    assert np.array_equal(bits(win), bits(want)) and np.array_equal(bits(crop), bits(want))
    # tiles
    rb = DenseRaster(raw, clip=0, precision="bf16", device=dev())
    tw, tc = rb.windows(origins, tiles=True, size=S), rb.crops(boxes, tiles=True, size=S)
    assert tw.shape == tc.shape == (3, BANDS, S, S)
    assert np.array_equal(bits(tw.tiles), bits(tc.tiles))
    assert np.array_equal(bits(tw.float()), bits(gather_windows_np(rb.float().cpu().numpy(), origins, S)))
    # years: a present year, a missing one, a present year whose raster is all zero (a constant raster normalises to 0)
    zero = DenseRaster(np.full((BANDS, H, W), 4.0, dtype=np.float32), clip=0, precision="fp32", device=dev())
    rasters = [r, None, zero]
    got = []
    for gather, items in ((DenseRaster.windows_years, origins), (DenseRaster.crops_years, boxes)):
        outs = [torch.zeros(3, BANDS, S, S, dtype=torch.float32, device=dev()) if x is None
                else torch.full((3, BANDS, S, S), 7.0, dtype=torch.float32, device=dev()) for x in rasters]
        flags = torch.zeros(3, dtype=torch.float32, device=dev())
        clear_next = torch.ones(3, dtype=torch.float32, device=dev())
        assert gather(rasters, items, outs, flags, clear_next, size=S) is flags
        got.append(([o.cpu().numpy() for o in outs], flags.cpu().numpy(), clear_next.cpu().numpy()))
    (wo, wf, wc), (co, cf, cc) = got
    for y in range(3):
        assert np.array_equal(bits(wo[y]), bits(co[y])), y
    assert np.array_equal(bits(wo[0]), bits(want)) and not wo[1].any() and not wo[2].any()
    assert np.array_equal(wf, cf) and wf.tolist() == [1.0, 0.0, 0.0]
    assert np.array_equal(wf, year_flags_np([r.float().cpu().numpy(), None, zero.float().cpu().numpy()], origins, S))
    assert not wc.any() and not cc.any()
