"""Field stems to crown boxes on the device (dta_stems_assign, stems.CrownBoxes) against the host definition
(stems.assign_np): every comparison is exact equality of box, status and crowns (NaNs equal).  The families are those of
tests/stems_cases.py: a 0.25 m lattice full of ties, coordinates off any lattice with mirrored boxes, plots around the
workgroup and LDS chunk sizes, and the hand-made cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import stems_cases as SC

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_families = {}


def family(name):
    """The case of a family and the definition's answers with and without CHM, computed once."""
    from deeptreeattention_amd import stems
    if name not in _families:
        assert stems.CHUNK == 1024
        case = getattr(SC, name)()
        _families[name] = (case, {chm: stems.assign_np(**SC.arguments(case, chm)) for chm in (True, False)})
    return _families[name]


def on_device(case, chm=True, tensors=False):
    from deeptreeattention_amd import stems
    up = (lambda a: torch.from_numpy(a).to(dev())) if tensors else (lambda a: a)
    table = stems.CrownBoxes(up(case["boxes"]), up(case["box_plot"]), case["plots"], device=dev())
    return table.assign(up(case["points"]), up(case["point_plot"]), up(case["height"]),
                        up(case["chm"]) if chm and case["chm"] is not None else None, size=case["size"])


def same(got, want):
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
    assert got.box.dtype == torch.int64 and got.status.dtype == torch.uint8 and got.crowns.dtype == torch.float64
    assert tuple(got.crowns.shape) == want.crowns.shape and tuple(got.box.shape) == want.box.shape
    box, status, crowns = (t.cpu().numpy() for t in got)
    return (np.array_equal(box, want.box) and np.array_equal(status, want.status)
            and np.array_equal(crowns, want.crowns, equal_nan=True))


@pytest.mark.parametrize("chm", (True, False))
@pytest.mark.parametrize("name", ("lattice", "continuous", "chunks"))
def test_assign_equals_the_definition(name, chm):
    case, want = family(name)
    assert min(np.bincount(want[chm].status, minlength=5)[:3]) >= 5
    assert same(on_device(case, chm), want[chm])
    assert same(on_device(case, chm, tensors=True), want[chm])           # resident inputs: the same route, no upload


@pytest.mark.parametrize("name", ("lattice", "continuous", "chunks"))
def test_shuffled_input_is_sorted_and_put_back(name):
    """Plot codes interleaved, boxes and stems in another order: the internal sort and the way back to the caller's order
    and indices (another problem than the unshuffled one: ties go to the lowest index)."""
    from deeptreeattention_amd import stems
    case = SC.shuffled(family(name)[0], 7)
    assert (np.diff(case["point_plot"]) < 0).any() and (np.diff(case["box_plot"]) < 0).any()
    for chm in (True, False):
        assert same(on_device(case, chm), stems.assign_np(**SC.arguments(case, chm)))


def test_hand_made_cases_on_the_device():
    for name, case, box, status in SC.HAND:
        got = on_device(case)
        assert got.box.tolist() == box and got.status.tolist() == status, name
        assert np.array_equal(got.crowns.cpu().numpy(), SC.crowns_of(case, box), equal_nan=True), name


def test_pixel_boxes_go_through_geo_boxes():
    from deeptreeattention_amd import boundary, stems
    t = (SC.UTM[0], 0.5, SC.UTM[1] + 40.0, -0.5)
    rng = np.random.default_rng(5)
    low = rng.integers(0, 60, (50, 2))
    pix = np.concatenate([low, low + rng.integers(4, 20, (50, 2))], axis=1).astype(np.int32)
    plot = rng.integers(0, 2, 50)
    pts = np.array(SC.UTM) + rng.integers(0, 160, (64, 2)) * 0.25
    pp, h = rng.integers(0, 2, 64), 5.0 * rng.integers(1, 5, 64)
    want = stems.assign_np(boundary.geo_boxes(pix, t), plot, pts, pp, h, plots=2)
    assert (want.status == 1).sum() >= 3 and (want.status == 2).sum() >= 3
    assert same(stems.CrownBoxes(pixel_boxes=pix, transform=t, box_plot=plot, plots=2, device=dev()).assign(pts, pp, h), want)


def sorted_tables(case):
    """What CrownBoxes hands to the C entry, made on the host: both tables sorted stably by plot, and the start tables."""
    plots = case["plots"]
    bo, so = np.argsort(case["box_plot"], kind="stable"), np.argsort(case["point_plot"], kind="stable")
    codes = np.arange(plots + 1)
    return dict(boxes=case["boxes"][bo], box_plot=case["box_plot"][bo], points=case["points"][so],
                point_plot=case["point_plot"][so].astype(np.int32), height=case["height"][so], chm=case["chm"][so],
                box_start=np.searchsorted(case["box_plot"][bo], codes).astype(np.int32),
                point_start=np.searchsorted(case["point_plot"][so], codes).astype(np.int32))


def c_entry(t, plots, size, stream=None):
    """dta_stems_assign on sorted tables (host arrays), with buffers of this test's own: (choice, status, crowns)."""
    from deeptreeattention_amd import _lib
    d = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(dev()) for k in ("boxes", "box_start", "points", "point_plot",
                                                                             "point_start", "height", "chm")}
    n, m = len(t["points"]), len(t["boxes"])
    choice = torch.full((n + 64,), -7, dtype=torch.int64, device=dev())
    status = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=dev())
    crowns = torch.full((n + 64, 4), -7.0, dtype=torch.float64, device=dev())
    _lib.check(_lib.lib().dta_stems_assign(_lib.ptr(d["boxes"]), _lib.ptr(d["box_start"]), m, _lib.ptr(d["points"]),
                                           _lib.ptr(d["point_plot"]), _lib.ptr(d["point_start"]), _lib.ptr(d["height"]),
                                           _lib.ptr(d["chm"]), n, plots, size, _lib.ptr(choice), _lib.ptr(status),
                                           _lib.ptr(crowns), stream if stream is not None else _lib.current_stream_ptr()),
               "dta_stems_assign")
    choice, status, crowns = choice.cpu().numpy(), status.cpu().numpy(), crowns.cpu().numpy()
    assert (choice[n:] == -7).all() and (status[n:] == 0xFF).all() and (crowns[n:] == -7.0).all()     # nothing behind the end
    return choice[:n], status[:n], crowns[:n]


def test_out_of_range_starts_and_plot_codes_are_clamped():
    """Start entries below 0 and past the table, and plot codes outside 0 .. plots-1, straight to the C entry.  The entries
    are chosen so that clamping them into the table gives back the true tables: the answer is the definition's on those,
    with status 4 for the stems whose code is out of range.  (The kernel clamps; this only confirms the clamped result.)"""
    from deeptreeattention_amd import stems
    case = SC.lattice()
    # three more plot codes that hold no box and no stem, behind the 40 real ones
    plots = case["plots"] + 3
    t = sorted_tables(dict(case, plots=plots))
    M, N = len(t["boxes"]), len(t["points"])
    assert t["box_start"][0] == 0 and (t["box_start"][-4:] == M).all() and (t["point_start"][-4:] == N).all()
    t["box_start"][0], t["point_start"][0] = -5, -(2 ** 31)
    t["box_start"][-3:] = (M + 1, 2 ** 31 - 1, M + 1000)
    t["point_start"][-3:] = (2 ** 31 - 1, N + 1, N + 77)
    bad = np.arange(3, N, 41)
    t["point_plot"][bad] = np.resize(np.array([-1, plots, 2 ** 31 - 1, -(2 ** 31), plots + 5], np.int32), len(bad))
    want = stems.assign_np(t["boxes"], t["box_plot"], t["points"], t["point_plot"], t["height"], t["chm"], case["size"], plots)
    assert (want.status[bad] == 4).all() and (want.status == 4).sum() > len(bad)
    choice, status, crowns = c_entry(t, plots, case["size"])
    assert np.array_equal(choice, want.box) and np.array_equal(status, want.status)
    assert np.array_equal(crowns, want.crowns, equal_nan=True)


def test_a_second_call_on_another_stream_gives_the_same_bits():
    """No state between calls: the same tables again, on a stream of the caller's, after a call on other input."""
    case, want = family("chunks")
    t = sorted_tables(case)
    first = c_entry(t, case["plots"], case["size"])
    other = sorted_tables(SC.lattice())
    c_entry(other, 40, 1.0)
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = c_entry(t, case["plots"], case["size"], stream=C.c_void_p(side.cuda_stream))
    side.synchronize()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, second))
    # sorted input: the C entry's rows are the caller's rows
    assert (np.diff(case["point_plot"]) >= 0).all() and (np.diff(case["box_plot"]) >= 0).all()
    assert np.array_equal(first[0], want[True].box) and np.array_equal(first[1], want[True].status)
