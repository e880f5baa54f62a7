"""The first conv once per year raster for the multi-stage route, host side (no GPU): the new C-ABI symbols and their
host-side refusals, the host definitions dense.gather_conv1_years_np / year_flags_np / conv1_mask_np on a case small enough
to check by hand, and the oracle-alone condition of the route case the GPU tests hold the route to (route_case: built once,
shared with tests/test_dense_multistage_conv1_gpu.py, never modified)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import hang2020_np as O
from oracle import hang2020_torch as OT
from oracle import preprocess_np as PP
from oracle import prng
from test_dense_conv1_gpu import raw_raster, raw_windows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dta_conv1_multistage_table_bytes", "dta_conv1_multistage_raster_table", "dta_conv1_multistage_output_range",
               "dta_conv1_multistage_gather_windows", "dta_conv1_multistage_predict", "dta_conv1_multistage_predict_ensemble")
MARGIN = 2e-4          # the fp32 eval-mode tolerance (tests/test_dense_conv1_gpu.py: FP32_TIGHT)
HEAD_GAIN = 120.0


# ---------------------------------------------------------------------------------------------------------------------
# the route case: 3 levels x 3 years on 20x15 rasters
# ---------------------------------------------------------------------------------------------------------------------
ROUTE_CLASSES = (3, 2, 5)
ROUTE_BANDS = 20


def params(kind, bands, classes, seed):
    """tests/test_dense_conv1_gpu.py's params with the last head scaled by 120 instead of 30 (a local copy)."""
    p = O.init_params(O.subnet_spec(kind, bands, classes), seed=seed)
    for k in p:
        if k.endswith("running_mean"):
            p[k] = (0.2 * (prng.uniform01(seed, 7, p[k].shape) - 0.5)).astype(np.float32)
        elif k.endswith("running_var"):
            p[k] = (0.5 + prng.uniform01(seed + 1, 9, p[k].shape)).astype(np.float32)
        elif k.endswith("classifier3.fc1.weight"):
            p[k] = (p[k] * HEAD_GAIN).astype(np.float32)
    return p


def oracle_scores(p, x):
    with torch.no_grad():
        pt = {k: torch.from_numpy(np.array(v)) for k, v in p.items()}
        pt = {k: (v.double() if v.is_floating_point() else v) for k, v in pt.items()}
        return OT.subnet(pt, "", "spectral", x, False)[-1].numpy()


@functools.lru_cache(maxsize=None)
def route_case():
    """Years raw_raster(310), None, raw_raster(311) (40 raw bands, 20 after clipping), levels with 3, 2 and 5 classes, the
    level-l year-y network params("spectral", 20, classes, 310 + 10 l + y), one centre-anchored window per pixel (300).
    The float64 oracle: per level softmax of the mean of years 0 and 2's scores (reference year.py:27-33: the missing year is
    left out).  Returns (raws, origins, params[l][y], want[l] probabilities, margin[l])."""
    from deeptreeattention_amd.dense import window_origins
    h, w = 20, 15
    raws = [raw_raster(310, 40, h, w), None, raw_raster(311, 40, h, w)]
    origins, _ = window_origins([(0, 0, h, w)], anchor="center")
    ps = [[params("spectral", ROUTE_BANDS, c, 310 + 10 * l + y) for y in range(3)] for l, c in enumerate(ROUTE_CLASSES)]
    xs = {y: torch.from_numpy(np.stack([PP.preprocess_image(win) for win in raw_windows(raws[y], origins)])).double() for y in (0, 2)}
    want, margin = [], []
    for l in range(len(ROUTE_CLASSES)):
        mean = (oracle_scores(ps[l][0], xs[0]) + oracle_scores(ps[l][2], xs[2])) / 2.0
        pr = torch.softmax(torch.from_numpy(mean), dim=1).numpy()
        top = np.sort(pr, axis=1)
        want.append(pr)
        margin.append(top[:, -1] - top[:, -2])
    for a in want + margin:
        a.setflags(write=False)
    return raws, origins, ps, want, margin


def test_route_case_holds_for_the_oracle_alone():
    """No window's top-2 margin is below 2e-4 at any level (so every label of the fp32 route is pinned), and the label check
    is not empty: some level has at least two distinct labels."""
    raws, origins, ps, want, margin = route_case()
    assert len(origins) == 300
    distinct = []
    for l, (pr, mg) in enumerate(zip(want, margin)):
        low = int((mg < MARGIN).sum())
        distinct.append(len(np.unique(pr.argmax(axis=1))))
        print(f"level {l}: {pr.shape[1]} classes, smallest top-2 margin {mg.min():.3e}, {low} windows below {MARGIN}, "
              f"{distinct[-1]} distinct labels")
        assert pr.shape == (300, ROUTE_CLASSES[l]) and low == 0
    assert max(distinct) >= 2


# ---------------------------------------------------------------------------------------------------------------------
# the host definitions on a case one can check by hand
# ---------------------------------------------------------------------------------------------------------------------
BANDS, H, W, COLS, LEVELS = 2, 3, 4, 2, 2


def hand_case():
    """A 3x4 raster of two bands, 2 levels x 3 years of 2-column first convs.  Year 0 a scene, year 1 missing, year 2 all zero."""
    x0 = prng.uniform(91, 1, (BANDS, H, W), 0.1, 1.0).astype(np.float64)
    w = prng.uniform(91, 2, (LEVELS, 3, COLS, BANDS, 3, 3), -0.5, 0.5).astype(np.float64)      # [level][year]
    b = prng.uniform(91, 3, (LEVELS, 3, COLS), -0.3, 0.3).astype(np.float64)
    return [x0, None, np.zeros_like(x0)], w, b


def year_tables(xs, w, b):
    """A year's table: conv1_table_np on the levels' year-y weights and biases concatenated; a missing year: the biases."""
    from deeptreeattention_amd.dense import Conv1TableNP, conv1_table_np
    out = []
    for y, x in enumerate(xs):
        wy, by = np.concatenate([w[l, y] for l in range(LEVELS)]), np.concatenate([b[l, y] for l in range(LEVELS)])
        out.append(conv1_table_np(x, wy, by) if x is not None else Conv1TableNP(np.broadcast_to(by, (1, 9, len(by))).copy(), H, W))
    return out


def test_gather_conv1_years_np_by_hand():
    from deeptreeattention_amd.dense import conv1_class, conv1_table_np, gather_conv1_np, gather_conv1_years_np
    xs, w, b = hand_case()
    tables = year_tables(xs, w, b)
    assert tables[0].data.shape == ((H + 2) * (W + 2) + 1, 9, LEVELS * COLS) and tables[1].data.shape == (1, 9, LEVELS * COLS)
    origins = np.array([(-1, -1), (0, 0), (-13, 0), (-5, -4), (H + 1, W + 1), (-11, 0)], dtype=np.int32)
    got = gather_conv1_years_np(tables, origins, LEVELS)
    assert got.shape == (LEVELS, 3, len(origins), 121, COLS) and got.dtype == np.float64
    # the slice order is (level, year): each slice is the gather of that one network's own table
    for l in range(LEVELS):
        one = conv1_table_np(xs[0], w[l, 0], b[l, 0])
        assert np.array_equal(got[l, 0], gather_conv1_np(one, origins))
        assert not np.array_equal(got[l, 0], got[1 - l, 0])
        # a missing year and an all-zero year: the level's year-y biases at every position of every window
        for y in (1, 2):
            assert np.array_equal(got[l, y], np.broadcast_to(b[l, y], (len(origins), 121, COLS)))
    # the ring: window 0 starts at (-1, -1), so its position (0, 0) -- first row, first column: class 0 -- lies on ring
    # position 0, whose only tap on the raster is (+1, +1) on pixel (0, 0)
    for l in range(LEVELS):
        want = b[l, 0] + np.einsum("k,nk->n", xs[0][:, 0, 0], w[l, 0][:, :, 2, 2])
        np.testing.assert_allclose(got[l, 0, 0, 0], want, rtol=1e-12)
        assert np.array_equal(got[l, 0, 0, 0], tables[0].data[0, 0, l * COLS:(l + 1) * COLS])
        # window 0, position (1, 1) lies on pixel (0, 0): the middle class of table position (1, 1)
        assert np.array_equal(got[l, 0, 0, 12], tables[0].data[(W + 2) + 1, 4, l * COLS:(l + 1) * COLS])
        # windows two or more pixels outside (2: rows -13 .. -3; 4: from (H + 1, W + 1)) read the far-outside row: the biases
        for n in (2, 4):
            assert np.array_equal(got[l, 0, n], np.broadcast_to(b[l, 0], (121, COLS)))
        # window 5 covers rows -11 .. -1: its last row (class 2: no tap below) sits on the ring and sees nothing either
        assert np.array_equal(got[l, 0, 5], np.broadcast_to(b[l, 0], (121, COLS)))
        # window 1 at (0, 0): position (i, j) on pixel (i, j) while inside, the ring at (3, j) / (i, 4), far beyond
        i, j = 2, 3
        cls = conv1_class(i) * 3 + conv1_class(j)
        assert np.array_equal(got[l, 0, 1, i * 11 + j], tables[0].data[(i + 1) * (W + 2) + (j + 1), cls, l * COLS:(l + 1) * COLS])
        assert np.array_equal(got[l, 0, 1, 5 * 11 + 5], b[l, 0])
    with pytest.raises(ValueError):
        gather_conv1_years_np(tables, origins, 3)


def test_year_flags_np_and_the_mask_by_hand():
    from deeptreeattention_amd.dense import conv1_mask_np, year_flags_np
    xs, w, b = hand_case()
    inside = np.array([(0, 0)], dtype=np.int32)
    assert year_flags_np(xs, inside).tolist() == [1.0, 0.0, 0.0] and year_flags_np(xs, inside).dtype == np.float32
    # windows that miss the raster -- far away, or touching only the ring (rows -11 .. -1) -- set nothing
    assert year_flags_np(xs, np.array([(-13, 0), (-11, 0), (H, 0), (0, W)], dtype=np.int32)).tolist() == [0.0, 0.0, 0.0]
    assert year_flags_np(xs, np.array([(-13, 0), (-10, 0)], dtype=np.int32)).tolist() == [1.0, 0.0, 0.0]      # rows -10 .. 0
    # one non-zero element is enough, and a NaN counts as one
    one = [xs[0], None, xs[2].copy()]
    one[2][1, 2, 3] = np.nan
    assert year_flags_np(one, inside).tolist() == [1.0, 0.0, 1.0]
    assert year_flags_np(one, np.array([(-10, -10)], dtype=np.int32)).tolist() == [1.0, 0.0, 0.0]             # pixel (0, 0) only
    assert year_flags_np(one, np.array([(2, 3)], dtype=np.int32)).tolist() == [1.0, 0.0, 1.0]
    # the mask: ones under the raster's non-zero pixels, zeros on the ring and in the far-outside row
    m = conv1_mask_np(one[2])
    assert m.dtype == np.uint8 and m.shape == ((H + 2) * (W + 2) + 1,)
    assert m.sum() == 1 and m[(2 + 1) * (W + 2) + (3 + 1)] == 1
    full = conv1_mask_np(xs[0])
    grid = full[:-1].reshape(H + 2, W + 2)
    assert full[-1] == 0 and grid[1:-1, 1:-1].all() and grid.sum() == H * W
    assert conv1_mask_np(None).tolist() == [0]
    neg = np.zeros((1, 1, 2)); neg[0, 0, 1] = -0.0
    assert conv1_mask_np(neg).sum() == 0


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
    from deeptreeattention_amd import _lib
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dta_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"#define\s+DTA_ABI_VERSION\s+2\b", hdr)


def test_c_entries_refuse_before_any_launch(lib):
    """Every call here returns before its first launch: the dummy device pointers are never dereferenced."""
    from deeptreeattention_amd import _lib
    P = 0x1000
    FO = _lib.FORWARD_ONLY

    def desc(kind=_lib.NET_SPECTRAL, dtype=_lib.DTA_BF16, training=0, heads=4 | FO, side=11):
        return C.byref(_lib.NetDesc(8, 20, side, side, 3, kind, dtype, training, heads, 0.1, 1e-5))

    def levels(spec=((3, 0, 3), (2, 3, 3))):
        return (_lib.Level * len(spec))(*[_lib.Level(c, f, n, None, None, P, None, None, None, None) for c, f, n in spec])

    def ptrs(vals):
        return (C.c_void_p * len(vals))(*vals)

    def err():
        return lib.dta_last_error().decode()
    nets = (_lib.SubnetParams * 6)()
    six = ((2, 0, 3),) * 1 + tuple((2, 3 * k, 3) for k in range(1, 6))       # 18 networks
    sb, tb, mb = C.c_size_t(), C.c_size_t(), C.c_size_t()
    sizes = lambda d, lv, h, w: lib.dta_conv1_multistage_table_bytes(d, lv, h, w, C.byref(sb), C.byref(tb), C.byref(mb))      # noqa: E731

    # ---- sizes
    who = "dta_conv1_multistage_table_bytes"
    assert lib.dta_conv1_multistage_table_bytes(desc(), 2, 6, 5, None, C.byref(tb), C.byref(mb)) != 0 and err() == who + ": null argument"
    assert sizes(desc(kind=_lib.NET_HANG2020), 2, 6, 5) != 0 and err() == who + ": the descriptor's kind must be DTA_NET_SPECTRAL"
    assert sizes(desc(), 0, 6, 5) != 0 and err() == who + ": 1..8 levels"
    assert sizes(desc(), 9, 6, 5) != 0 and err() == who + ": 1..8 levels"
    assert sizes(desc(dtype=7), 2, 6, 5) != 0 and err() == who + ": unknown dtype 7"
    assert sizes(desc(), 2, 0, 5) != 0 and "bad shape" in err()
    # 20 bands -> 2 chunks; 5 levels = 160 columns; half storage, float32 T
    assert sizes(desc(), 5, 6, 5) == 0
    assert tb.value == (8 * 7 + 1) * 9 * 160 * 2 and mb.value == 8 * 7 + 1 and sb.value == 2 * 9 * 160 * 16 * 2 + 30 * 9 * 160 * 4
    assert sizes(desc(dtype=_lib.DTA_F32), 1, 6, 5) == 0
    assert tb.value == (8 * 7 + 1) * 9 * 32 * 4 and mb.value == 57 and sb.value == 2 * 9 * 32 * 16 * 4 + 30 * 9 * 32 * 4
    assert sizes(desc(), 3, 0, 0) == 0 and (sb.value, tb.value, mb.value) == (0, 9 * 96 * 2, 1)       # a missing year
    # the header's figures: 5 levels at 256x256 in half
    assert sizes(C.byref(_lib.NetDesc(8, 349, 11, 11, 3, _lib.NET_SPECTRAL, _lib.DTA_BF16, 0, 4 | FO, 0.1, 1e-5)), 5, 256, 256) == 0
    assert round(tb.value / 1e6) == 192 and round((sb.value - 22 * 9 * 160 * 32) / 1e6) == 377      # 189 MB + the ring; T

    # ---- the build
    who = "dta_conv1_multistage_raster_table"
    build = lambda d=None, lv=2, n=nets, ras=P, scr=P, tab=P, mask=P: lib.dta_conv1_multistage_raster_table(      # noqa: E731
        d or desc(), lv, n, ras, 6, 5, scr, tab, mask, None)
    assert build(n=None) != 0 and err() == who + ": null argument"
    assert build(tab=None) != 0 and err() == who + ": null argument"
    assert build(mask=None) != 0 and err() == who + ": null argument"
    assert build(scr=None) != 0 and err() == who + ": null argument"
    assert build(d=desc(kind=_lib.NET_SPATIAL)) != 0 and err() == who + ": the descriptor's kind must be DTA_NET_SPECTRAL"
    assert build(lv=9) != 0 and err() == who + ": 1..8 levels"
    assert build(ras=P + 4) != 0 and err() == who + ": raster, scratch and table must be 16-byte aligned"
    assert build(tab=P + 8) != 0 and "16-byte aligned" in err()
    assert build() != 0 and err() == who + ": level 0: the first conv's parameters are missing"
    assert build(ras=None, scr=None) != 0 and err() == who + ": level 0: the first conv's parameters are missing"      # NULL raster: no scratch needed

    # ---- the slot
    who = "dta_conv1_multistage_output_range"
    off, gs, nb = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.dta_conv1_multistage_output_range(desc(), 2, levels(), None, C.byref(gs), C.byref(nb)) != 0 and err() == who + ": null argument"
    assert lib.dta_conv1_multistage_output_range(desc(), 6, levels(six), C.byref(off), C.byref(gs), C.byref(nb)) != 0
    assert err() == who + ": at most 16 networks (levels x kept years) per step"
    assert lib.dta_conv1_multistage_output_range(desc(), 2, levels(), C.byref(off), C.byref(gs), C.byref(nb)) == 0
    assert gs.value == 8 * 121 * 32 * 2 and nb.value == 6 * gs.value and off.value % 256 == 0
    assert off.value + nb.value <= lib.dta_multistage_workspace_bytes(desc(), 2, levels())
    assert lib.dta_conv1_multistage_output_range(desc(dtype=_lib.DTA_F32), 2, levels(), C.byref(off), C.byref(gs), C.byref(nb)) == 0
    assert gs.value == 8 * 121 * 32 * 4

    # ---- the gather
    who = "dta_conv1_multistage_gather_windows"
    present = (C.c_int * 3)(1, 0, 1)

    def gather(d=None, nl=2, lv=None, years=3, tables=None, masks=None, pres=present, origins=P, n=8, ws=P, flags=P, nxt=P + 64):
        return lib.dta_conv1_multistage_gather_windows(d or desc(), nl, lv or levels(), years, tables or ptrs([P] * 3), masks or ptrs([P] * 3),
                                                       pres, 6, 5, origins, n, ws, flags, nxt, None)
    assert gather(origins=None) != 0 and err() == who + ": null argument (or flags == clear_next)"
    assert gather(ws=None) != 0 and err() == who + ": null argument (or flags == clear_next)"
    assert gather(flags=None) != 0 and err() == who + ": null argument (or flags == clear_next)"
    assert gather(nxt=P) != 0 and err() == who + ": null argument (or flags == clear_next)"
    assert gather(pres=None) != 0 and err() == who + ": null argument (or flags == clear_next)"
    assert gather(d=desc(training=1)) != 0 and err() == who + ": eval mode (training == 0) with DTA_FORWARD_ONLY only"
    assert gather(d=desc(heads=4)) != 0 and err() == who + ": eval mode (training == 0) with DTA_FORWARD_ONLY only"
    assert gather(d=desc(side=12)) != 0 and err() == who + ": 11x11 patches only, not 12x12"
    assert gather(d=desc(kind=_lib.NET_HANG2020)) != 0 and err() == who + ": the descriptor's kind must be DTA_NET_SPECTRAL"
    assert gather(d=desc(dtype=7)) != 0 and err() == who + ": unknown dtype 7"
    assert gather(nl=6, lv=levels(six)) != 0 and err() == who + ": at most 16 networks (levels x kept years) per step"
    assert gather(years=2) != 0 and err() == who + ": level 0 has 3 networks, the call 2 years"
    assert gather(n=0) != 0 and "bad shape" in err()
    assert gather(n=9) != 0 and "bad shape" in err()                      # more windows than the descriptor's batch
    assert gather(tables=ptrs([P, None, P])) != 0 and "year 1: null table or mask" in err()
    assert gather(masks=ptrs([P, P, None])) != 0 and "year 2: null table or mask" in err()
    assert gather(tables=ptrs([P, P + 8, P])) != 0 and err() == who + ": year 1: the table must be 16-byte aligned"
    assert gather(ws=P + 4) != 0 and err() == who + ": the workspace must be 16-byte aligned"
    assert gather(pres=(C.c_int * 3)(0, 0, 0)) != 0 and err() == who + ": every year is missing: nothing to gather"

    # ---- the forward behind the first convs
    for name, tail in (("dta_conv1_multistage_predict", ()),
                       ("dta_conv1_multistage_predict_ensemble", (None, P, P, P, None, None))):
        fn = getattr(lib, name)

        def call(d=None, nl=2, lv=None, n=nets, ws=P, idx=1):
            three = ptrs([P] * nl)
            return fn(d or desc(), nl, lv or levels(), n, None, ws, None, three if idx else None, three, *tail, None)
        assert call(n=None) != 0 and err() == name + ": null argument"
        assert call(ws=None) != 0 and err() == name + ": null argument"
        assert call(idx=0) != 0 and err() == name + ": null argument"
        assert call(d=desc(training=1)) != 0 and err() == name + ": eval mode (training == 0) with DTA_FORWARD_ONLY only"
        assert call(d=desc(heads=4)) != 0 and err() == name + ": eval mode (training == 0) with DTA_FORWARD_ONLY only"
        assert call(d=desc(side=12)) != 0 and err() == name + ": 11x11 patches only, not 12x12"
        assert call(d=desc(kind=_lib.NET_SPATIAL)) != 0 and err() == name + ": the descriptor's kind must be DTA_NET_SPECTRAL"
        assert call(nl=6, lv=levels(six)) != 0 and err() == name + ": at most 16 networks (levels x kept years) per step"
        if not tail:      # (with the walk the missing hierarchy table is answered first)
            assert call(d=desc(dtype=7)) != 0 and err() == "unknown dtype 7"
        if tail:
            assert call() != 0 and err() == name + ": null hierarchy table"
