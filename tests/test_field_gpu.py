"""Field records to canopy points on the device (dta_field_filter, dta_megaplot_plots; field.FieldTable, field.megaplot_plots)
against the host definitions (field.filter_np, field.plots_np): every comparison is exact equality.  The families are those
of tests/field_cases.py; tests/test_field_cpu.py checks on the host that each of them reaches what it is meant to reach."""
import numpy as np
import pytest
import torch

import field_cases as FC

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_tables = {}


def family(name, *args):
    """The case of a family and the definition's answer, computed once."""
    key = (name,) + args
    if key not in _tables:
        case = getattr(FC, name)(*args)
        _tables[key] = (case, FC.run_np(case))
    return _tables[key]


def on_device(case, table=None, **thresholds):
    from deeptreeattention_amd import field
    table = table if table is not None else field.FieldTable(case["columns"], device=dev())
    t = dict(min_stem_diameter=case["min_stem_diameter"], min_height=case["min_height"])
    t.update(thresholds)
    return table, table.filter(t["min_stem_diameter"], t["min_height"])


def same(got, want, table=None):
    keep, reason, rows, count = got
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (keep, reason, rows, count))
    assert keep.dtype == torch.uint8 and reason.dtype == torch.uint8 and rows.dtype == torch.int64 and count.dtype == torch.int64
    assert tuple(rows.shape) == want.rows.shape and tuple(count.shape) == ()
    if table is not None:
        assert int(table.errors.item()) == int((want.reason == 255).sum())
    return (np.array_equal(keep.cpu().numpy(), want.keep) and np.array_equal(reason.cpu().numpy(), want.reason)
            and np.array_equal(rows.cpu().numpy(), want.rows) and int(count.item()) == int(want.count))


@pytest.mark.parametrize("name, args", (("synthetic", ()), ("special", ()), ("large", ()), ("sized", (1,)), ("sized", (255,)),
                                        ("sized", (256,)), ("sized", (257,))),
                         ids=("synthetic", "special", "large", "n1", "n255", "n256", "n257"))
def test_filter_equals_the_definition(name, args):
    case, want = family(name, *args)
    if name in ("synthetic", "large"):
        seen = FC.census(case, want)
        assert min(seen["reason"]) >= 5 and seen["by_height"] >= 20 and seen["by_event"] >= 20
    if name == "large":
        assert len(want.reason) == 70000 and case["columns"]["individuals"] == 20000
    table, got = on_device(case)
    assert same(got, want, table)
    again = table.filter(case["min_stem_diameter"], case["min_height"])           # twice: identical bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_resident_columns_are_taken_as_they_are():
    """Columns that already live on the device: the same chain without an upload, and what resident() refuses."""
    from deeptreeattention_amd import field
    case, want = family("synthetic")
    c = case["columns"]
    up = {k: torch.from_numpy(c[k].view(np.int16) if k == "flags" else c[k]).to(dev()) for k in field._COLUMNS}
    table = field.FieldTable.resident(up["individual"], up["event"], up["height"], up["diameter"], up["flags"], c["individuals"])
    assert table.tensors["height"] is up["height"] and table.rows == 3000
    assert same(table.filter(case["min_stem_diameter"], case["min_height"]), want, table)
    for key, value in (("individual", up["individual"].long()), ("height", up["height"].float()), ("event", up["event"][:-1]),
                       ("flags", up["flags"].cpu()), ("diameter", up["diameter"][::2]), ("individuals", 0), ("individuals", 3001)):
        args = dict(up, individuals=c["individuals"])
        args[key] = value
        with pytest.raises(ValueError, match="resident|individuals"):
            field.FieldTable.resident(**args)


def test_hand_made_table_on_the_device():
    case, reasons = FC.hand()
    table, got = on_device(case)
    assert got.reason.cpu().tolist() == reasons.tolist() and got.index().tolist() == FC.HAND_ROWS
    assert int(got.count.item()) == len(FC.HAND_ROWS) and int(table.errors.item()) == 0


def test_other_thresholds_on_the_same_table():
    """The resident table is not changed by a run: other thresholds, then the first ones again."""
    from deeptreeattention_amd import field
    case, want = family("synthetic")
    table, first = on_device(case)
    for min_d, min_h in ((25.0, 3.0), (10.0, 12.0), (-np.inf, -np.inf), (np.inf, 3.0), (30.0, np.inf)):
        other = field.filter_np(case["columns"], min_d, min_h)
        assert same(table.filter(min_d, min_h), other, table)
    assert int(field.filter_np(case["columns"], np.inf, 3.0).count) == 0           # nothing kept: rows is all -1
    assert same(table.filter(case["min_stem_diameter"], case["min_height"]), want, table)


def test_filter_on_a_stream_of_the_callers():
    case, want = family("synthetic")
    other, other_want = family("sized", 257)
    table, _ = on_device(case)
    on_device(other)
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = table.filter(case["min_stem_diameter"], case["min_height"])
    side.synchronize()
    assert same(got, want, table)


def test_codes_out_of_range_are_counted_and_take_part_in_nothing():
    """Codes FieldTable never makes, handed to the C entry through a table whose columns were changed after its checks: the
    rows get reason 255, the error word counts them, nothing outside the workspace is touched (the rule is the
    definition's; the kernel guards every table read)."""
    from deeptreeattention_amd import field
    case, _ = family("synthetic")
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case["columns"].items()}
    table = field.FieldTable(c, device=dev())
    c["individual"][5::97] = np.resize(np.array([-1, 1200, 2 ** 31 - 1, -(2 ** 31)], np.int32), len(c["individual"][5::97]))
    c["event"][11::131] = -3
    want = field.filter_np(c, 10.0)
    assert (want.reason == 255).sum() >= 40
    table.tensors["individual"] = torch.from_numpy(c["individual"]).to(dev())
    table.tensors["event"] = torch.from_numpy(c["event"]).to(dev())
    assert same(table.filter(10.0), want, table)


def test_filter_data_on_the_device_is_the_reference_order():
    """The recorded tables of the reference (tests/golden/field) through the whole route: strings on the host, the rule on
    the device, the frame back."""
    import os
    pytest.importorskip("pandas")
    from deeptreeattention_amd import field
    recorded = np.load(os.path.join(FC.GOLDEN, "field_reference.npz"))
    for name in ("sample", "synthetic"):
        out = field.filter_data(FC.frame_of(recorded, name), {"min_stem_diameter": float(recorded["min_stem_diameter"])},
                                device=dev())
        assert out.index.tolist() == recorded[name + "_kept"].tolist()
        assert out.taxonID.astype(str).tolist() == recorded[name + "_taxon"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# megaplot
# ---------------------------------------------------------------------------------------------------------------------
def plots_same(points, rule, cell=FC.CELL):
    from deeptreeattention_amd import field
    want = field.plots_np(points, rule, cell)
    for p in (points, torch.from_numpy(points).to(dev())):                          # host arrays, resident tensors
        got = field.megaplot_plots(p, rule, cell, device=dev())
        assert got.code.is_cuda and got.code.dtype == torch.int32 and got.plots == want.plots
        if not np.array_equal(got.code.cpu().numpy(), want.code):
            return False
        again = field.megaplot_plots(p, rule, cell, device=dev())
        assert torch.equal(got.code, again.code)
    return True


@pytest.mark.parametrize("rule", ("grid", "buffer"))
def test_plots_equal_the_definition_on_lattice_and_ring(rule):
    lattice, ring = FC.lattice(), FC.ring()
    assert (FC.cells_holding(lattice) >= 2).sum() >= 20 and FC.pairs_exactly_at(ring) >= 5
    assert plots_same(lattice, rule) and plots_same(ring, rule)
    assert plots_same(lattice * 0.5 + 0.1, rule, 13.7)            # off the lattice, a cell that is no binary fraction
    odd = FC.lattice(300, seed=2)
    odd[3, 0], odd[7, 1], odd[9] = np.nan, np.inf, (-np.inf, np.nan)
    assert plots_same(odd, rule)


@pytest.mark.parametrize("n", (1, 2, 1000, 1001))
def test_auto_switches_where_the_reference_does(n):
    from deeptreeattention_amd import field
    points = FC.auto(n)
    assert plots_same(points, "auto")
    got = field.megaplot_plots(points, device=dev())
    assert got.plots == (n if n <= 1000 else field.plots_np(points, "grid").plots)
    assert plots_same(points, "grid") and plots_same(points[:1000], "buffer")


def test_buffer_rule_at_4096_stems_and_grid_rule_at_70000():
    big = FC.lattice(4096, seed=31, span=4000)
    assert plots_same(big, "buffer")
    assert plots_same(FC.lattice(70000, seed=32, span=40000), "grid")


def test_plots_on_a_stream_of_the_callers():
    from deeptreeattention_amd import field
    ring = FC.ring()
    want = field.plots_np(ring, "buffer")
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = field.megaplot_plots(ring, "buffer", device=dev())
        grid = field.megaplot_plots(ring, "grid", device=dev())
    side.synchronize()
    assert np.array_equal(got.code.cpu().numpy(), want.code)
    assert np.array_equal(grid.code.cpu().numpy(), field.plots_np(ring, "grid").code)


def test_the_chain_into_the_crown_boxes():
    """filter -> megaplot_plots -> stems.CrownBoxes.assign: the plot codes are what `point_plot` takes."""
    from deeptreeattention_amd import field, stems
    points = FC.lattice(1200, seed=40)
    plots = field.megaplot_plots(points, "grid", device=dev())
    rs = np.random.RandomState(1)
    boxes = np.concatenate([points - rs.rand(len(points), 2), points + rs.rand(len(points), 2)], axis=1)
    height = rs.randint(12, 100, len(points)) * 0.25
    table = stems.CrownBoxes(torch.from_numpy(boxes).to(dev()), plots.code, plots.plots, device=dev())
    got = table.assign(torch.from_numpy(points).to(dev()), plots.code, torch.from_numpy(height).to(dev()))
    want = stems.assign_np(boxes, plots.code.cpu().numpy(), points, plots.code.cpu().numpy(), height, plots=plots.plots)
    assert np.array_equal(got.status.cpu().numpy(), want.status) and (want.status == 1).sum() >= 600
