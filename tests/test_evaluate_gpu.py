"""Crown-level evaluation on the device (dta_eval_count, dta_eval_report, dta_first_rows, dta_novel_scores; evaluate.EvalTable,
first_per_individual, novel_scores, evaluate_crowns) against the host definitions (evaluate.count_np, report_np,
first_per_individual_np): every comparison is exact equality of every bit.  The families are those of
tests/evaluate_cases.py; tests/test_evaluate_cpu.py checks on the host that each of them reaches what it is meant to."""
import numpy as np
import pytest
import torch

import evaluate_cases as EC

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def count_on_device(case, form, table=None):
    from deeptreeattention_amd import evaluate
    table = table if table is not None else evaluate.EvalTable(case["n_species"], case["groups"], device=dev())
    out = table.count(up(case["labels"]), up(case["preds"]), group=up(case["group"]), mask=up(case["mask"]), form=form)
    assert out is table
    return table


def bits(a):
    """float64 as its bit pattern: equal bits, not merely equal values (-0.0, NaN)."""
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.COUNT_CASES))
def test_count_equals_the_definition_in_both_forms(name):
    from deeptreeattention_amd import evaluate
    case = EC.COUNT_CASES[name]()
    conf, tally = evaluate.count_np(**case)
    if name.startswith("bad_rows") or name in ("mask", "many_blocks"):
        assert tally[1] >= 6
    got = {}
    for form in (evaluate.PLAIN, evaluate.COMBINE):
        table = count_on_device(case, form)
        assert table.conf.dtype == torch.int64 and tuple(table.conf.shape) == conf.shape and table.tally.dtype == torch.int64
        got[form] = (table.conf.cpu().numpy(), table.tally.cpu().numpy())
        assert np.array_equal(got[form][0], conf) and np.array_equal(got[form][1], tally), (name, form)
    assert np.array_equal(got[evaluate.PLAIN][0], got[evaluate.COMBINE][0])
    default = count_on_device(case, None)                                         # the form the module keeps
    assert torch.equal(default.conf.cpu(), torch.from_numpy(conf))


@pytest.mark.parametrize("form", (0, 1), ids=("plain", "combine"))
def test_two_calls_accumulate_to_the_one_call_result(form):
    from deeptreeattention_amd import evaluate
    a, b = EC.rows(257, 9, 3, 41, hot=0.6, bad=True, with_mask=True), EC.rows(130, 9, 3, 42, hot=0.3, with_mask=True)
    both = {k: (np.concatenate([a[k], b[k]]) if isinstance(a[k], np.ndarray) else a[k]) for k in a}
    conf, tally = evaluate.count_np(**both)
    table = count_on_device(b, form, count_on_device(a, form))
    assert np.array_equal(table.conf.cpu().numpy(), conf) and np.array_equal(table.tally.cpu().numpy(), tally)
    once = count_on_device(both, form)
    assert torch.equal(once.conf, table.conf) and torch.equal(once.tally, table.tally)


# ---------------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------------
def report_on_device(case, per_species=True):
    from deeptreeattention_amd import evaluate
    conf = case["conf"]
    table = evaluate.EvalTable(conf.shape[1], conf.shape[0], device=dev())
    table.conf.copy_(torch.from_numpy(conf))
    return table.report(case["site_masks"], case["genus"], per_species=per_species)


def same_report(got, want, per_species=True):
    keys = ("counts", "scores") + (("accuracy", "precision", "support") if per_species else ())
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("name", sorted(EC.REPORT_CASES))
def test_report_equals_the_definition_bit_for_bit(name):
    from deeptreeattention_amd import evaluate
    case = EC.REPORT_CASES[name]()
    want = evaluate.report_np(**case)
    rep = report_on_device(case)
    assert rep.counts.is_cuda and rep.counts.dtype == torch.int64 and rep.scores.dtype == torch.float64
    assert rep.accuracy.dtype == torch.float64 and rep.support.dtype == torch.int64
    assert rep.counts.data_ptr() == rep.flat.data_ptr()                           # views of one buffer
    same_report(rep.cpu(), want)
    same_report(report_on_device(case, per_species=False).cpu(), want, per_species=False)
    if name == "special":
        assert want["counts"][0, 0] == 0 and want["counts"][1, 2] == 0 and want["support"][3, 6] == 0


def test_tables_resident_on_the_device_are_taken_as_they_are():
    from deeptreeattention_amd import evaluate
    case = EC.REPORT_CASES["w2_bit64"]()
    want = evaluate.report_np(**case)
    table = evaluate.EvalTable(case["conf"].shape[1], case["conf"].shape[0], device=dev())
    table.conf.copy_(torch.from_numpy(case["conf"]))
    rep = table.report(torch.from_numpy(case["site_masks"].view(np.int64)).to(dev()), None)
    same_report(rep.cpu(), want)


def test_pooled_row_equals_a_one_group_table_counted_without_group():
    from deeptreeattention_amd import evaluate
    case = EC.rows(3000, 65, 5, 51, hot=0.6, bad=True)
    sites, genus = EC.random_sites(65, 23, 1), EC.random_genus(65, 2)
    grouped = count_on_device(case, None).report(sites, genus).cpu()
    inside = (case["group"] >= 0) & (case["group"] < 5)                             # a row of a group out of range counts nowhere
    one = dict(case, group=None, groups=1, mask=inside)
    single = count_on_device(one, None).report(sites, genus).cpu()
    for k in grouped:
        assert np.array_equal(bits(grouped[k][5]), bits(single[k][0])) and np.array_equal(bits(single[k][0]), bits(single[k][1])), k


# ---------------------------------------------------------------------------------------------------------------------
# first rows, novel scores
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.IDS_CASES)
def test_first_rows_equal_the_definition(name):
    from deeptreeattention_amd import evaluate
    ids, n = EC.ids_case(name)
    want = evaluate.first_per_individual_np(ids, n)
    got = evaluate.first_per_individual(up(ids), n)
    assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    if name == "out_of_range":
        assert not want[ids == 40].any() and not want[ids == -1].any() and (ids == 40).any()


def test_first_row_mask_feeds_count_and_abundance():
    from deeptreeattention_amd import abundance, evaluate
    c = EC.recorded("synthetic")
    mask = evaluate.first_per_individual(up(c["individual"]), 420)
    assert np.array_equal(mask.cpu().numpy(), c["first"])
    table = evaluate.EvalTable(40, device=dev()).count(up(c["true"]), up(c["pred"]), mask=mask)
    assert np.array_equal(table.conf.cpu().numpy(), evaluate.count_np(c["true"], c["pred"], mask=c["first"], n_species=40)[0])
    got = abundance.counts(up(c["pred"]), 40, mask=mask)
    assert np.array_equal(got.cpu().numpy().reshape(-1), abundance.counts_np(c["pred"], 40, mask=c["first"]).reshape(-1))


@pytest.mark.parametrize("classes", EC.NOVEL_CLASSES)
def test_novel_scores_equal_softmax_top2_and_the_row_maximum(classes):
    from deeptreeattention_amd import _lib, evaluate
    z = EC.logits(classes)
    zd = up(z)
    got = evaluate.novel_scores(zd)
    assert got.label.dtype == torch.int64 and got.top_score.dtype == torch.float32 and got.softmax_score.dtype == torch.float32
    label, top, soft = (t.cpu().numpy() for t in got)
    nan_row = np.isnan(z).any(1)
    assert nan_row.sum() == (1 if classes == 1 else 2)
    # top_score == logits.max(1).values, bit for bit (a row with a NaN: NaN, as torch gives)
    want_top = zd.max(1).values.cpu().numpy()
    assert np.array_equal(top[~nan_row].view(np.int32), want_top[~nan_row].view(np.int32))
    assert np.isnan(top[nan_row]).all() and np.isnan(want_top[nan_row]).all()
    assert (label[nan_row] == -1).all() and (soft[nan_row] == -1.0).all()
    if classes > 2:
        assert label[3] == classes // 3 and z[3, classes - 1] == z[3, classes // 3]      # tied maxima: the lower class wins
    assert label[4] == 0
    if classes >= 2:                                                               # dta_softmax_top2 takes classes >= 2
        n = z.shape[0]
        ti = torch.empty((n, 2), dtype=torch.int64, device=dev())
        ts = torch.empty((n, 2), dtype=torch.float32, device=dev())
        _lib.check(_lib.lib().dta_softmax_top2(_lib.ptr(zd), n, classes, None, _lib.ptr(ti), _lib.ptr(ts), _lib.current_stream_ptr()),
                   "dta_softmax_top2")
        assert torch.equal(got.label, ti[:, 0])
        assert np.array_equal(soft.view(np.int32), ts[:, 0].cpu().numpy().view(np.int32))
    else:
        assert (label[~nan_row] == 0).all() and (soft[~nan_row] == 1.0).all()
    ref = evaluate.novel_scores_np(z)                                              # the float64 route agrees on the labels
    clear = ~nan_row
    clear[4] = False                                                               # (all classes equal: float32 exp decides nothing)
    assert np.array_equal(label[clear], ref.label[clear])


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_crowns_equals_the_recorded_reference_figures():
    from deeptreeattention_amd import evaluate
    c = EC.recorded("synthetic")
    sites, genus = evaluate.site_masks(c["site_lists"], 40), evaluate.genus_ids(c["scientific"], 40)
    kw = dict(n_species=40, n_sites=EC.SITES, n_individuals=420, site_masks=sites, genus=genus)
    got = evaluate.evaluate_crowns(up(c["pred"]), up(c["true"]), up(c["site"]), up(c["individual"]), **kw)
    assert got["within_site"] == c["site_confusion"] and got["within_genus"] == c["genus_confusion"]
    want = evaluate.evaluate_crowns(c["pred"], c["true"], c["site"], c["individual"], **kw)         # the definitions
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(bits(a.astype(b.dtype)), bits(b)), k
    first = c["first"]
    for s in range(EC.SITES):                                                       # multi_stage.py:469, restated
        rows = first & (c["site"] == s)
        assert got["site_micro"][s] == np.sum(c["pred"][rows] == c["true"][rows]) / rows.sum()
    no_err = EC.recorded("no_error")
    got = evaluate.evaluate_crowns(up(no_err["pred"]), up(no_err["true"]), n_species=6,
                                   site_masks=evaluate.site_masks(no_err["site_lists"], 6),
                                   genus=evaluate.genus_ids(no_err["scientific"], 6))
    assert got["within_site"] == 0.0 and got["within_genus"] == 0.0 and got["micro"] == 1.0
