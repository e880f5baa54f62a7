"""The first conv once per raster, host side (no GPU): the float64 definitions dense.conv1_table_np / gather_conv1_np
against the oracle's first conv (oracle/hang2020_np.py: conv2d_same, bias included, pre-BatchNorm) on explicitly gathered
windows, for every window origin around a small raster; the nine-case rule; the new C-ABI symbols and their refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import hang2020_np as O
from oracle import prng

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dta_conv1_table_bytes", "dta_raster_conv1_table", "dta_gather_conv1_windows", "dta_conv1_output_range",
               "dta_conv1_forward")
BANDS, H, W, COLS = 5, 7, 6, 3


def case():
    x = prng.uniform(71, 1, (BANDS, H, W), 0.0, 1.0).astype(np.float64)
    w = prng.uniform(71, 2, (COLS, BANDS, 3, 3), -0.4, 0.4).astype(np.float64)
    b = prng.uniform(71, 3, (COLS,), -0.3, 0.3).astype(np.float64)
    return x, w, b


def test_nine_case_rule():
    from deeptreeattention_amd.dense import conv1_class
    assert [conv1_class(i) for i in (0, 1, 9, 10)] == [0, 1, 1, 2]
    assert [conv1_class(i) for i in range(11)] == [0] + [1] * 9 + [2]
    # the class of a window position is (row class) * 3 + (column class): the four corners, an edge, the interior
    cls = lambda i, j: conv1_class(i) * 3 + conv1_class(j)
    assert [cls(0, 0), cls(0, 10), cls(10, 0), cls(10, 10), cls(0, 1), cls(9, 10), cls(1, 9)] == [0, 2, 6, 8, 1, 5, 4]


def test_table_and_gather_equal_the_oracles_first_conv_for_every_origin():
    from deeptreeattention_amd.dense import conv1_table_np, gather_conv1_np, gather_windows_np
    x, w, b = case()
    table = conv1_table_np(x, w, b)
    assert table.data.shape == ((H + 2) * (W + 2) + 1, 9, COLS) and table.data.dtype == np.float64
    assert (table.height, table.width) == (H, W)
    origins = np.array([(r, c) for r in range(-12, 9) for c in range(-12, 8)], dtype=np.int32)
    got = gather_conv1_np(table, origins)                               # [N][121][cols]
    want = O.conv2d_same(gather_windows_np(x, origins), w, b)           # [N][cols][11][11]
    want = want.reshape(len(origins), COLS, 121).transpose(0, 2, 1)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    # the range holds windows over each edge and corner, the raster strictly inside the window, and windows with no raster
    # pixel at all, whose first conv is the bias
    r, c = origins[:, 0], origins[:, 1]
    outside = (r + 11 <= 0) | (r >= H) | (c + 11 <= 0) | (c >= W)
    inside = (r < 0) & (r + 11 > H) & (c < 0) & (c + 11 > W)
    assert outside.sum() > 50 and inside.sum() >= 4
    for corner in ((-5, -5), (-5, W - 6), (H - 6, -5), (H - 6, W - 6), (-10, 0), (H - 1, 0), (0, -10), (0, W - 1)):
        assert (origins == np.array(corner)).all(axis=1).any(), corner
    assert np.array_equal(got[outside], np.broadcast_to(b, got[outside].shape))
    assert not np.array_equal(got[~outside][0], np.broadcast_to(b, (121, COLS)))


def test_ring_and_far_rows_of_the_table():
    from deeptreeattention_amd.dense import conv1_table_np
    x, w, b = case()
    A = conv1_table_np(x, w, b).data
    far = (H + 2) * (W + 2)
    assert np.array_equal(A[far], np.broadcast_to(b, (9, COLS)))
    # ring position (-1, -1): only the tap (+1, +1) sees the raster, pixel (0, 0); classes whose R leaves +1 out are the bias
    ring = A[0]
    t = np.einsum("k,nk->n", x[:, 0, 0], w[:, :, 2, 2])
    for rc in range(3):
        for cc in range(3):
            want = b + t if rc != 2 and cc != 2 else b
            np.testing.assert_allclose(ring[rc * 3 + cc], want, rtol=1e-12)
    # interior pixel, middle class: the plain 3x3 conv of the raster
    full = O.conv2d_same(x[None], w, b)[0]                              # [cols][H][W]
    np.testing.assert_allclose(A[(3 + 1) * (W + 2) + (2 + 1), 4], full[:, 3, 2], rtol=1e-10)


def test_gather_keeps_dtype_and_bits():
    from deeptreeattention_amd.dense import Conv1TableNP, gather_conv1_np
    data = prng.uniform(5, 1, ((4 + 2) * (3 + 2) + 1, 9, 8), -2, 2).astype(np.float16)
    out = gather_conv1_np(Conv1TableNP(data, 4, 3), np.array([[-3, 2], [40, 40]], dtype=np.int32))
    assert out.dtype == np.float16 and out.shape == (2, 121, 8)
    from deeptreeattention_amd.dense import conv1_class
    for i in range(11):                 # window 1 lies wholly beyond the ring: the far-outside row, class by class
        for j in range(11):
            assert np.array_equal(out[1][i * 11 + j].view(np.uint16), data[-1, conv1_class(i) * 3 + conv1_class(j)].view(np.uint16))
    # window 0, position (4, 0): raster pixel (1, 2), middle row, left column
    assert np.array_equal(out[0][4 * 11 + 0].view(np.uint16), data[(1 + 1) * 5 + (2 + 1), 3].view(np.uint16))


@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name


def test_c_entries_refuse_before_any_launch(lib):
    """Every call here returns before its first launch: the dummy device pointers are never dereferenced."""
    from deeptreeattention_amd import _lib
    P = 0x1000
    FO = _lib.FORWARD_ONLY

    def desc(kind=_lib.NET_HANG2020, dtype=_lib.DTA_BF16, training=0, heads=4 | FO, side=11):
        return C.byref(_lib.NetDesc(8, 20, side, side, 3, kind, dtype, training, heads, 0.1, 1e-5))

    def err():
        return lib.dta_last_error().decode()
    nets = (_lib.SubnetParams * 2)()
    fwd = lambda d: lib.dta_conv1_forward(d, nets, P, P, None, P, None)
    assert fwd(desc(training=1)) != 0 and err() == "dta_conv1_forward: eval mode (training == 0) with DTA_FORWARD_ONLY only"
    assert fwd(desc(heads=4)) != 0 and err() == "dta_conv1_forward: eval mode (training == 0) with DTA_FORWARD_ONLY only"
    assert fwd(desc(kind=_lib.NET_VANILLA)) != 0 and "Hang2020, spectral_network and spatial_network only" in err()
    assert fwd(desc(side=12)) != 0 and err() == "dta_conv1_forward: 11x11 patches only, not 12x12"
    assert lib.dta_conv1_forward(desc(), nets, P, None, None, P, None) != 0 and err() == "dta_conv1_forward: null argument"
    sb, tb = C.c_size_t(), C.c_size_t()
    assert lib.dta_conv1_table_bytes(desc(kind=_lib.NET_VANILLA), 6, 5, C.byref(sb), C.byref(tb)) != 0 and "spatial_network only" in err()
    assert lib.dta_conv1_table_bytes(desc(dtype=7), 6, 5, C.byref(sb), C.byref(tb)) != 0 and err() == "dta_conv1_table_bytes: unknown dtype 7"
    assert lib.dta_conv1_table_bytes(desc(), 0, 5, C.byref(sb), C.byref(tb)) != 0 and "bad shape" in err()
    # sizes: 20 bands -> 2 chunks; Hang2020 64 columns, half storage; spectral fp32 32 columns
    assert lib.dta_conv1_table_bytes(desc(), 6, 5, C.byref(sb), C.byref(tb)) == 0
    assert tb.value == (8 * 7 + 1) * 9 * 64 * 2 and sb.value == 2 * 9 * 64 * 16 * 2 + 30 * 9 * 64 * 4
    assert lib.dta_conv1_table_bytes(desc(kind=_lib.NET_SPECTRAL, dtype=_lib.DTA_F32), 6, 5, C.byref(sb), C.byref(tb)) == 0
    assert tb.value == (8 * 7 + 1) * 9 * 32 * 4 and sb.value == 2 * 9 * 32 * 16 * 4 + 30 * 9 * 32 * 4
    assert lib.dta_raster_conv1_table(desc(), nets, P, 6, 5, P, None, None) != 0 and err() == "dta_raster_conv1_table: null argument"
    assert lib.dta_raster_conv1_table(desc(), nets, P, 6, 5, P, P, None) != 0 and err() == "dta_raster_conv1_table: the first conv's parameters are missing"
    assert lib.dta_raster_conv1_table(desc(), nets, P + 4, 6, 5, P, P, None) != 0 and "16-byte aligned" in err()
    assert lib.dta_gather_conv1_windows(desc(), P, 6, 5, None, 3, P, None) != 0 and err() == "dta_gather_conv1_windows: null argument"
    assert lib.dta_gather_conv1_windows(desc(), P, 6, 5, P, 0, P, None) != 0 and "bad shape" in err()
    off, nb = C.c_size_t(), C.c_size_t()
    assert lib.dta_conv1_output_range(desc(), C.byref(off), C.byref(nb)) == 0
    assert nb.value == 8 * 121 * 64 * 2 and off.value % 256 == 0 and off.value + nb.value <= lib.dta_net_workspace_bytes(desc())
    assert lib.dta_conv1_output_range(desc(kind=_lib.NET_SPATIAL, dtype=_lib.DTA_F32), C.byref(off), C.byref(nb)) == 0
    assert nb.value == 8 * 121 * 32 * 4
