"""Field stems to crown boxes, host side (no GPU): the NumPy definition (stems.assign_np) against a mirror that follows the
reference's lines with pandas, on a lattice family that reaches every path; hand-made cases with the answer written out;
the C entry's refusals, none of which reaches a launch; the Python route's host-side argument checks."""
import ctypes as C
import fractions
import os
import re

import numpy as np
import pytest

import stems_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the definition against the reference's lines
# ---------------------------------------------------------------------------------------------------------------------
def mirror(case, use_chm=True):
    """process_plot (src/generate.py:112-145) per plot and points_to_crowns' last line (:239) with pandas; the spatial join
    is a plain loop over the pairs, the centroid distance is np.hypot.  Returns (box, kept) per stem, -1 / False for a stem
    that is in no joined frame."""
    import pandas as pd
    b, bp, p, pp = case["boxes"], case["box_plot"], case["points"], case["point_plot"]
    M, N, size = len(b), len(p), case["size"]
    results = []
    for plot in range(case["plots"]):
        stems = [i for i in range(N) if pp[i] == plot and np.isfinite(p[i]).all()]       # plot_data
        if not stems:
            continue

        def row(j, i, x0, y0, x1, y1):
            return dict(individual=i, box_id=j, cx=(x0 + x1) / 2, cy=(y0 + y1) / 2, plotID=plot, height=case["height"][i],
                        CHM_height=case["chm"][i] if use_chm else None)

        def sjoin(boxes, among):                                                          # boxes: (id, x0, y0, x1, y1)
            return [row(j, i, x0, y0, x1, y1) for j, x0, y0, x1, y1 in boxes for i in among
                    if x0 <= p[i, 0] <= x1 and y0 <= p[i, 1] <= y1]

        merged = sjoin([(j,) + tuple(b[j]) for j in range(M) if bp[j] == plot], stems)    # :112
        joined = {r["individual"] for r in merged}
        missing = [i for i in stems if i not in joined]                                    # :115
        merged += sjoin([(M + i, p[i, 0] - size, p[i, 1] - size, p[i, 0] + size, p[i, 1] + size) for i in missing], missing)
        merged = pd.DataFrame(merged)
        if not use_chm:
            merged = merged.drop(columns=["CHM_height"])
        cleaned = []
        for individual, group in merged.groupby("individual"):                             # :122-127, choose_box
            if group.shape[0] > 1:
                dist = pd.Series(np.hypot(group.cx - p[individual, 0], group.cy - p[individual, 1]), index=group.index)
                group = group.loc[[dist.sort_values(kind="stable").index[0]]]
            cleaned.append(group)
        merged = pd.concat(cleaned)
        points = []
        for _, group in merged.groupby("box_id"):                                          # :134-145
            if group.shape[0] > 1:
                selected = group[group.height == group.height.max()]
                if selected.shape[0] > 1:
                    try:
                        selected = selected[selected.CHM_height == selected.CHM_height.max()]
                    except AttributeError:
                        selected.head(1)
                points.append(selected)
            else:
                points.append(group)
        results.append((merged, pd.concat(points)))
    box, kept = np.full(N, -1, np.int64), np.zeros(N, bool)
    for merged, _ in results:
        box[merged.individual.to_numpy()] = merged.box_id.to_numpy()
    final = pd.concat([r[1] for r in results]).sort_values("individual", kind="stable")
    final = final.groupby(["plotID", "box_id"]).head(1)                                    # :239
    kept[final.individual.to_numpy()] = True
    return box, kept


def status_of(box, kept, M):
    """The status the mirror's answer stands for: a dropped stem is 0 if its box kept somebody, else 3."""
    has_keeper = set(box[kept].tolist())
    return np.array([4 if j < 0 else (1 if j < M else 2) if k else 0 if j in has_keeper else 3 for j, k in zip(box, kept)], np.uint8)


@pytest.fixture(scope="module")
def lattice():
    from deeptreeattention_amd import stems
    case = SC.lattice()
    return case, stems.assign_np(**SC.arguments(case))


def test_the_lattice_family_reaches_every_path(lattice):
    case, got = lattice
    assert len(case["points"]) == 675 and len(case["boxes"]) == 1424 and case["plots"] == 40
    seen = SC.census(case, got)
    print(seen)
    assert min(seen["status"]) >= 5 and sum(seen["status"]) == 675
    assert seen["distance_ties"] >= 20 and seen["on_side"] >= 20 and seen["other_fallback"] >= 10 and seen["height_ties"] >= 5


@pytest.mark.parametrize("use_chm", (True, False))
def test_definition_agrees_with_the_reference_lines_in_pandas(lattice, use_chm):
    """On the 0.25 m lattice every d2 is an exact multiple of 1/64, so hypot and d2 order alike, ties included: the two
    agree on every stem."""
    pytest.importorskip("pandas")
    from deeptreeattention_amd import stems
    case, got = lattice
    if not use_chm:
        got = stems.assign_np(**SC.arguments(case, chm=False))
    box, kept = mirror(case, use_chm)
    assert np.array_equal(got.box, box)
    assert np.array_equal((got.status == 1) | (got.status == 2), kept)
    assert np.array_equal(got.status, status_of(box, kept, len(case["boxes"])))
    assert np.array_equal(got.crowns, SC.crowns_of(case, box), equal_nan=True)


def test_the_mirror_agrees_on_shuffled_input_too(lattice):
    pytest.importorskip("pandas")
    from deeptreeattention_amd import stems
    case = SC.shuffled(lattice[0], 3)
    got = stems.assign_np(**SC.arguments(case))
    box, kept = mirror(case)
    assert np.array_equal(got.box, box) and np.array_equal(got.status, status_of(box, kept, len(case["boxes"])))


@pytest.mark.parametrize("name, case, box, status", SC.HAND, ids=["hand%d" % k for k in range(len(SC.HAND))])
def test_hand_made_cases(name, case, box, status):
    from deeptreeattention_amd import stems
    got = stems.assign_np(**SC.arguments(case))
    assert got.box.dtype == np.int64 and got.status.dtype == np.uint8 and got.crowns.dtype == np.float64
    assert got.box.tolist() == box and got.status.tolist() == status, name
    assert np.array_equal(got.crowns, SC.crowns_of(case, box), equal_nan=True)
    assert got.crowns.shape == (len(box), 4) and np.isnan(got.crowns[np.array(box) < 0]).all()


def test_results_are_tensors_or_lists_alike():
    """assign_np takes lists, arrays and host tensors; the fallback bounds are px - size and px + size, rounded once."""
    import torch
    from deeptreeattention_amd import stems
    _, case, box, status = SC.HAND[2]
    kw = SC.arguments(case)
    as_tensors = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    assert stems.assign_np(**as_tensors).status.tolist() == status
    got = stems.assign_np(np.zeros((0, 4)), np.zeros(0, np.int32), [[0.1, 0.7]], [0], [1.0], size=0.3, plots=1)
    assert got.box.tolist() == [0] and got.status.tolist() == [2]
    assert got.crowns.tolist() == [[0.1 - 0.3, 0.7 - 0.3, 0.1 + 0.3, 0.7 + 0.3]]


def test_mirrored_boxes_tie_only_without_a_fused_multiply_add():
    """The continuous family: a stem with boxes centred at the stem + (a, b) and + (b, a) has d2 = a*a + b*b twice, products
    rounded one by one, and takes the lower index.  With the second product left exact (what a fused multiply-add does)
    the two differ for many of these stems, and for some the other box would win."""
    from deeptreeattention_amd import stems
    case = SC.continuous()
    got = stems.assign_np(**SC.arguments(case))
    b, p, F = case["boxes"], case["points"], fractions.Fraction
    tied = flipped = 0
    for i in np.flatnonzero((got.box >= 0) & (got.box < len(b))):
        mine = np.flatnonzero(case["box_plot"] == case["point_plot"][i])
        x, y = p[i]
        cand = mine[(b[mine, 0] <= x) & (x <= b[mine, 2]) & (b[mine, 1] <= y) & (y <= b[mine, 3])]
        dx, dy = (b[cand, 0] + b[cand, 2]) * 0.5 - x, (b[cand, 1] + b[cand, 3]) * 0.5 - y
        d2 = dx * dx + dy * dy
        if (d2 == d2.min()).sum() > 1:
            tied += 1
            assert got.box[i] == cand[d2 == d2.min()].min()
            fused = [float(F(float(u * u)) + F(float(v)) * F(float(v))) for u, v in zip(dx, dy)]
            flipped += int(cand[int(np.argmin(fused))] != got.box[i])
    print("stems with an exact tie: %d, decided otherwise by a fused multiply-add: %d" % (tied, flipped))
    assert tied >= 20 and flipped >= 5
    assert min(np.bincount(got.status, minlength=5)[:3]) >= 5


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, bound, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbol_is_declared_exported_and_bound(lib):
    from deeptreeattention_amd import _lib, build, stems
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert {n for n in names if n.startswith("dta_stems_")} == {"dta_stems_assign"}
    assert hasattr(lib, "dta_stems_assign") and '"dta_stems_assign"' in entry
    assert len(lib.dta_stems_assign.argtypes) == 15 and lib.dta_stems_assign.restype is C.c_int
    assert "stems.hip" in build.SOURCES and build.SOURCES[-1] == "boundary.hip"
    assert build.SOURCES.index("stems.hip") < build.SOURCES.index("split.hip") < build.SOURCES.index("boundary.hip")
    chunk = int(re.search(r"#define\s+DTA_STEMS_CHUNK\s+(\d+)", hdr).group(1))
    assert chunk == _lib.STEMS_CHUNK == stems.CHUNK == 1024
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the device pointers are host buffers nobody
    dereferences."""
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(boxes=p, box_start=p, n_boxes=8, points=p, point_plot=p, point_start=p, height=p, chm=None, n_points=4, plots=2,
             size=1.0, choice=p, status=p, crowns=p):
        return lib.dta_stems_assign(boxes, box_start, n_boxes, points, point_plot, point_start, height, chm, n_points, plots,
                                    size, choice, status, crowns, None)

    cases = [({k: None}, "null") for k in ("boxes", "box_start", "points", "point_plot", "point_start", "height", "choice",
                                            "status", "crowns")]
    cases += [({"boxes": None, "n_boxes": 0}, "null"),
              ({"n_points": 0}, "n_points=0"), ({"n_points": -1}, "n_points=-1"), ({"n_points": 1 << 31}, "n_points=2147483648"),
              ({"n_boxes": -1}, "n_boxes=-1"), ({"n_boxes": 1 << 31}, "n_boxes=2147483648"),
              ({"plots": 0}, "plots=0"), ({"plots": -3}, "plots=-3"),
              ({"size": 0.0}, "size=0"), ({"size": -1.0}, "size=-1"), ({"size": nan}, "size=nan"), ({"size": inf}, "size=inf"),
              ({"size": -inf}, "size=-inf"), ({"chm": p, "size": -0.0}, "size=-0")]
    for kw, what in cases:
        assert call(**kw) != 0, kw
        err = lib.dta_last_error().decode()
        assert err.startswith("dta_stems_assign: ") and what in err, (kw, err)


def test_the_stems_kernels_have_no_private_segment(tmp_path):
    import glob
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump, readelf = os.path.join(llvm, "llvm-objdump"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    from deeptreeattention_amd import _lib
    so = os.path.join(str(tmp_path), "libdta_hip.so")
    shutil.copy(os.path.join(os.path.dirname(_lib.LIB_PATH), "libdta_hip.so"), so)
    subprocess.run([objdump, "--offloading", so], cwd=str(tmp_path), capture_output=True, check=True)
    found = {}
    for f in sorted(glob.glob(so + ".*gfx950*")):
        notes = subprocess.run([readelf, "--notes", f], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.?name:\s+(\S+)", blk)
            seg = re.search(r"private_segment_fixed_size:\s+(\d+)", blk)
            if name and seg and "k_stems_" in name.group(1):
                found[name.group(1)] = int(seg.group(1))
    assert len(found) == 3 and all(v == 0 for v in found.values()), found
    assert {n for n in found if "choose" in n} and {n for n in found if "fallback" in n} and {n for n in found if "resolve" in n}


# ---------------------------------------------------------------------------------------------------------------------
# the Python route's own argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_definition_checks_its_arguments():
    from deeptreeattention_amd import stems
    _, case, _, _ = SC.HAND[4]
    good = SC.arguments(case)
    n = len(case["points"])
    bad = (("boxes", case["boxes"].astype(np.float32), "boxes"), ("boxes", case["boxes"][:, :3], "boxes"),
           ("box_plot", case["box_plot"][:2], "box_plot"), ("box_plot", case["box_plot"].astype(np.float64), "box_plot"),
           ("points", case["points"][:0], "points"), ("points", case["points"].astype(np.float32), "points"),
           ("points", case["points"].reshape(-1), "points"), ("point_plot", np.zeros(n, bool), "point_plot"),
           ("point_plot", case["point_plot"][1:], "point_plot"), ("height", case["height"][1:], "height"),
           ("height", case["height"].astype(np.float32), "height"), ("chm", case["chm"][1:], "chm"),
           ("chm", np.zeros(n, np.int64), "chm"), ("size", 0.0, "size"), ("size", -1.0, "size"), ("size", np.nan, "size"),
           ("size", np.inf, "size"), ("size", "wide", "size"), ("plots", 0, "plots"), ("plots", None, "plots"), ("plots", 2.0, "plots"),
           ("plots", 2 ** 31, "plots"))
    for key, value, what in bad:
        with pytest.raises(ValueError, match=what):
            stems.assign_np(**dict(good, **{key: value}))


def test_device_route_checks_its_arguments_on_the_host(monkeypatch):
    """Every refusal below is raised before _lib.lib() is reached.  CrownBoxes.resident on host tensors stands in for a
    resident table: the checks are the same, and a call that passes them is refused for want of a device."""
    import torch
    from deeptreeattention_amd import _lib, stems

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    _, case, _, _ = SC.HAND[4]
    b, bp = case["boxes"], case["box_plot"]
    pix = np.array([(0, 0, 4, 8), (10, 20, 12, 21), (7, 3, 2, 1)], np.int32)
    t = (405000.0, 0.5, 3305000.0, -0.25)
    for kw, what in (({"boxes": b.astype(np.float32)}, "boxes"), ({"boxes": b[:, :2]}, "boxes"), ({"box_plot": bp[:1]}, "box_plot"),
                     ({"box_plot": None}, "box_plot"), ({"box_plot": bp.astype(np.float64)}, "box_plot"), ({"plots": 0}, "plots"),
                     ({"plots": None}, "plots"), ({"boxes": None}, "exactly one"), ({"pixel_boxes": pix, "transform": t}, "exactly one"),
                     ({"boxes": None, "pixel_boxes": pix}, "need a transform"), ({"transform": t}, "no transform"),
                     ({"boxes": None, "pixel_boxes": pix.astype(np.float64), "transform": t}, "pixel_boxes"),
                     ({"boxes": None, "pixel_boxes": pix, "transform": (0, 0, 1, 1)}, "transform")):
        with pytest.raises(ValueError, match=what):
            stems.CrownBoxes(**dict(dict(boxes=b, box_plot=bp, plots=1, device="cpu"), **kw))
    for kw in ({}, {"boxes": None, "pixel_boxes": pix, "transform": t}):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            stems.CrownBoxes(**dict(dict(boxes=b, box_plot=bp, plots=1, device="cpu"), **kw))
    tb, start, perm = torch.from_numpy(b), torch.tensor([0, 3], dtype=torch.int32), torch.arange(3)
    for bad in ((tb.float(), start, perm, 1), (tb, start.long(), perm, 1), (tb, start, perm[:2], 1), (tb, start, perm, 2),
                (tb.t(), start, perm, 1), (b, start, perm, 1), (tb, start, perm.int(), 1)):
        with pytest.raises(ValueError, match="resident|plots"):
            stems.CrownBoxes.resident(*bad)
    table = stems.CrownBoxes.resident(tb, start, perm, 1)
    assert table.n_boxes == 3 and table.plots == 1 and table.boxes is tb
    good = dict(points=case["points"], point_plot=case["point_plot"], height=case["height"], chm=case["chm"])
    for key, value, what in (("points", case["points"].astype(np.float32), "points"), ("points", case["points"][:0], "points"),
                             ("points", torch.from_numpy(case["points"]).float(), "points"),
                             ("points", torch.zeros(9, 2, dtype=torch.float64, device="meta"), "points"),
                             ("point_plot", case["point_plot"][1:], "point_plot"), ("point_plot", case["height"], "point_plot"),
                             ("height", case["height"][1:], "height"), ("height", case["point_plot"], "height"),
                             ("chm", case["chm"][:2], "chm"), ("chm", torch.from_numpy(case["chm"]).half(), "chm"),
                             ("size", 0, "size"), ("size", np.nan, "size"), ("size", -2.0, "size")):
        with pytest.raises(ValueError, match=what):
            table.assign(**dict(good, **{key: value}))
    for kw in (good, dict(good, chm=None)):
        with pytest.raises(RuntimeError, match="ROCm device only"):           # no fallback: a host table computes nothing
            table.assign(**kw)
