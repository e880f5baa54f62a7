"""Crown-level evaluation, host side (no GPU): the NumPy definitions (evaluate.count_np, report_np, first_per_individual_np,
novel_scores_np) and the string helpers against the reference's own recorded answers (tests/golden/evaluate, made by
tools/make_evaluate_golden.py from the reference's site_confusion and genus_confusion), against hierarchy's
scores_from_confusion, against a re-statement of the reference's per-site line and its two novel-score expressions; the C
entries' refusals, none of which reaches a launch; the Python route's host-side argument checks."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import evaluate_cases as EC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_checksums():
    lines = [ln.split() for ln in open(os.path.join(EC.GOLDEN, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert sorted(name for _, name in lines) == ["evaluate_reference.json", "evaluate_reference.npz"]
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(EC.GOLDEN, name), "rb").read()).hexdigest() == digest, name


# ---------------------------------------------------------------------------------------------------------------------
# the reference's recorded answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.RECORDED)
def test_definitions_reproduce_the_recorded_reference_figures(name):
    from deeptreeattention_amd import evaluate
    c = EC.recorded(name)
    S = c["n_species"]
    mask = c.get("first")
    conf, tally = evaluate.count_np(c["true"], c["pred"], mask=mask, n_species=S)
    kept = len(c["true"]) if mask is None else int(mask.sum())
    assert conf.shape == (1, S, S) and tally.tolist() == [kept, 0] and conf.sum() == kept
    r = evaluate.report_np(conf, evaluate.site_masks(c["site_lists"], S) if "site_lists" in c else None,
                           evaluate.genus_ids(c["scientific"], S) if "scientific" in c else None)
    assert np.array_equal(r["counts"][0], r["counts"][1]) and np.array_equal(r["scores"][0], r["scores"][1])    # G = 1
    assert "site_confusion" in c or "genus_confusion" in c
    if "site_confusion" in c:
        assert r["scores"][1, 2] == c["site_confusion"]                   # the same division of the same two integers
        assert r["counts"][1, 3] + r["counts"][1, 4] == r["counts"][1, 2]
    else:
        assert r["scores"][1, 2] == 0.0 and r["counts"][1, 3] == r["counts"][1, 4] == 0
    if "genus_confusion" in c:
        assert r["scores"][1, 3] == c["genus_confusion"]
        assert r["counts"][1, 5] + r["counts"][1, 6] == r["counts"][1, 2]
    else:
        assert r["scores"][1, 3] == 0.0 and r["counts"][1, 5] == r["counts"][1, 6] == 0
    if name == "no_error":
        assert r["counts"][1, 2] == 0 and c["site_confusion"] == 0.0 and c["genus_confusion"] == 0.0 and r["scores"][1, 0] == 1.0
    if name == "synthetic":
        assert len(c["true"]) == 600 and S == 40 and kept == 420 and r["counts"][1, 2] > 100
        assert 0 < r["counts"][1, 3] < r["counts"][1, 2] and 0 < r["counts"][1, 5] < r["counts"][1, 2]


def test_the_recorded_tables_hold_what_they_are_meant_to():
    from deeptreeattention_amd import evaluate
    c = EC.recorded("synthetic")
    m, g = evaluate.site_masks(c["site_lists"], 40), evaluate.genus_ids(c["scientific"], 40)
    assert m.shape == (40, 1) and m.dtype == np.uint64 and g.dtype == np.int32
    assert max(bin(int(v)).count("1") for v in m[:, 0]) >= 2             # species on several sites
    assert not m[3, 0] & m[4, 0] and m[0, 0] & m[1, 0]                    # a pair with disjoint sites, one that shares
    # lists give the first word, plain strings the first character: Quercus alba (list) and Quercus rubra (string) differ,
    # Quercus rubra and Quamoclit coccinea (both strings) are one genus
    assert isinstance(c["scientific"][0], list) and isinstance(c["scientific"][1], str)
    assert g[0] != g[1] and g[1] == g[2]
    first = c["first"]
    t, p = c["true"][first], c["pred"][first]
    for a, b in ((0, 1), (1, 2), (3, 4), (4, 3)):
        assert ((t == a) & (p == b)).any(), (a, b)
    # the reference's own test: "QUMU" and "QUMLA" are one genus, "ACRU" another
    g = evaluate.genus_ids(EC.recorded("ref_genus_within")["scientific"], 3)
    assert g[1] == g[2] != g[0]


def test_helpers_state_their_deviations():
    from deeptreeattention_amd import evaluate
    m = evaluate.site_masks({0: ["b", "a"], 2: ["a"]}, 4)                  # bits follow the sorted unique sites: a = 0, b = 1
    assert m.tolist() == [[3], [0], [1], [0]]                             # a species without an entry: an empty mask
    m = evaluate.site_masks({0: range(65), 1: [64]}, 2)
    assert m.shape == (2, 2) and int(m[1, 0]) == 0 and int(m[1, 1]) == 1 and int(m[0, 0]) == 2 ** 64 - 1
    with pytest.raises(ValueError, match="at most 256 sites"):
        evaluate.site_masks({0: range(257)}, 1)
    with pytest.raises(ValueError, match="keyed by the species label"):
        evaluate.site_masks({5: [1]}, 5)
    g = evaluate.genus_ids({0: ["Acer rubrum", "x"], 1: ["Acer saccharum"], 3: "Acer"}, 5)
    assert g[0] == g[1] and len({g[0], g[2], g[3], g[4]}) == 4           # no entry: an id equal to no other
    conf = np.zeros((1, 4, 4), np.int64)
    conf[0, 0, 1] = 3                                                     # species 1 has no sites: the error is cross-site
    r = evaluate.report_np(conf, evaluate.site_masks({0: ["a"]}, 4))
    assert r["counts"][1].tolist() == [3, 0, 3, 0, 3, 0, 0, 1] and r["scores"][1].tolist() == [0.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# the stated convention: hierarchy.scores_from_confusion; the reference's per-site line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.REPORT_CASES))
def test_report_equals_scores_from_confusion(name):
    from deeptreeattention_amd import evaluate
    from deeptreeattention_amd.hierarchy import scores_from_confusion
    case = EC.REPORT_CASES[name]()
    conf = case["conf"]
    G, S = conf.shape[:2]
    r = evaluate.report_np(**case)
    for row, plane in enumerate(list(conf) + [conf.sum(0)]):
        want = scores_from_confusion(plane)
        assert r["scores"][row, 0] == want["micro"]
        assert np.array_equal(r["accuracy"][row], want["accuracy"]) and np.array_equal(r["precision"][row], want["precision"])
        assert np.array_equal(r["support"][row], plane.sum(1))
        # two summation orders of at most S terms in [0, 1]
        assert abs(r["scores"][row, 1] - want["macro"]) <= S * 2.0 ** -52 * want["macro"]
        assert r["counts"][row, 0] == plane.sum() and r["counts"][row, 1] == np.trace(plane) and r["counts"][row, 7] == (plane.sum(1) > 0).sum()
    if case["site_masks"] is None:
        assert not r["counts"][:, 3:5].any() and not r["scores"][:, 2].any()
    if case["genus"] is None:
        assert not r["counts"][:, 5:7].any() and not r["scores"][:, 3].any()


def test_report_cases_reach_what_they_are_meant_to():
    from deeptreeattention_amd import evaluate
    for sites, word, bit in ((64, 0, 63), (65, 1, 0)):
        case = EC.last_bit(sites)
        m = case["site_masks"]
        assert m.shape[1] == word + 1 and (m[0] & m[1]).tolist() == [0] * word + [1 << bit]
        r = evaluate.report_np(**case)
        cut = m.copy()
        cut[1, word] &= ~(np.uint64(1) << np.uint64(bit))                 # without that one bit the pair is cross-site
        r2 = evaluate.report_np(case["conf"], cut)
        moved = case["conf"][:, 0, 1] + case["conf"][:, 1, 0]
        assert (moved > 0).all() and np.array_equal(r["counts"][:2, 3] - r2["counts"][:2, 3], moved)
    r = evaluate.report_np(**EC.special())
    assert r["counts"][0].tolist() == [0] * 8 and r["scores"][0].tolist() == [0.0] * 4          # an empty group
    assert r["counts"][1, 2] == 0 and r["scores"][1, 0] == 1.0 and r["scores"][1, 2] == r["scores"][1, 3] == 0.0
    # species 4 is predicted but never a label: not in macro
    assert r["support"][3, 4] == 0 and EC.special()["conf"][:, :, 4].sum() > 0 and r["accuracy"][3, 4] == r["precision"][3, 4] == 0.0
    assert r["counts"][3, 7] == 7 and r["precision"][3, 6] == 0.0


def test_per_site_micro_is_the_reference_line():
    """multi_stage.py:469: np.sum(group.ens_label.values == group.label.values) / len(group.ens_label.values), per siteID."""
    import pandas as pd
    from deeptreeattention_amd import evaluate
    c = EC.recorded("synthetic")
    df = pd.DataFrame({"individual": c["individual"], "label": c["true"], "ens_label": c["pred"], "siteID": c["site"]})
    df = df.groupby("individual").head(1)
    out = evaluate.evaluate_crowns(c["pred"], c["true"], c["site"], c["individual"], n_species=40, n_sites=EC.SITES,
                                   n_individuals=420, site_masks=evaluate.site_masks(c["site_lists"], 40),
                                   genus=evaluate.genus_ids(c["scientific"], 40))
    seen = 0
    for site, group in df.groupby("siteID"):
        site_micro = np.sum(group.ens_label.values == group.label.values) / len(group.ens_label.values)
        assert out["site_micro"][site] == site_micro and out["site_counts"][site, 0] == len(group)
        seen += 1
    assert seen == EC.SITES
    assert out["within_site"] == c["site_confusion"] and out["within_genus"] == c["genus_confusion"]
    assert out["counts"][0] == 420 and out["micro"] == np.sum(df.ens_label.values == df.label.values) / len(df)


# ---------------------------------------------------------------------------------------------------------------------
# first rows, counting, novel scores
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.IDS_CASES)
def test_first_rows_equal_pandas_head_1(name):
    import pandas as pd
    from deeptreeattention_amd import evaluate
    ids, n = EC.ids_case(name)
    got = evaluate.first_per_individual_np(ids, n)
    df = pd.DataFrame({"individual": ids, "row": np.arange(len(ids))})
    df = df[(df.individual >= 0) & (df.individual < n)]
    want = np.zeros(len(ids), bool)
    want[df.groupby("individual").head(1)["row"].to_numpy()] = True
    assert got.dtype == bool and np.array_equal(got, want)
    c = EC.recorded("synthetic")
    assert np.array_equal(evaluate.first_per_individual_np(c["individual"], 420), c["first"])


@pytest.mark.parametrize("name", sorted(EC.COUNT_CASES))
def test_count_definition_against_a_plain_loop(name):
    from deeptreeattention_amd import evaluate
    case = EC.COUNT_CASES[name]()
    if len(case["labels"]) > 5000:
        case = {k: (v[:5000] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    S, G = case["n_species"], case["groups"]
    conf, tally = evaluate.count_np(**case)
    want, counted, skipped = np.zeros((G, S, S), np.int64), 0, 0
    for i, (t, p) in enumerate(zip(case["labels"], case["preds"])):
        g = 0 if case["group"] is None else int(case["group"][i])
        if case["mask"] is not None and not case["mask"][i]:
            continue
        if 0 <= t < S and 0 <= p < S and 0 <= g < G:
            want[g, t, p] += 1
            counted += 1
        else:
            skipped += 1
    assert np.array_equal(conf, want) and tally.tolist() == [counted, skipped]
    if name.startswith("bad_rows") or name == "mask":
        assert skipped >= 6


def test_novel_scores_equal_the_reference_expressions():
    """metrics.py:91-93 on torch CPU, in float64: pred[arange, argmax(pred, 1)] and the same of softmax(pred, 1)."""
    import torch
    from torch.nn import functional as F
    from deeptreeattention_amd import evaluate
    for C_ in EC.NOVEL_CLASSES:
        z = EC.logits(C_)
        ok = ~np.isnan(z).any(1)
        pred = torch.from_numpy(z[ok].astype(np.float64))
        top_score = pred[np.arange(len(pred)), np.argmax(pred, 1)]
        softmax_layer = F.softmax(pred, dim=1)
        softmax_score = softmax_layer[np.arange(len(softmax_layer)), np.argmax(softmax_layer, 1)]
        got = evaluate.novel_scores_np(z)
        assert np.array_equal(got.top_score[ok], top_score.numpy())
        # one exp, a sum of at most C terms and one division, each a few ulp in either implementation
        assert np.abs(got.softmax_score[ok] - softmax_score.numpy()).max() <= (C_ + 8) * 2.0 ** -52
        assert np.array_equal(got.label[ok], np.argmax(z[ok].astype(np.float64), 1))
        assert (got.label[~ok] == -1).all() and np.isnan(got.top_score[~ok]).all() and (got.softmax_score[~ok] == -1.0).all()
        assert (~ok).sum() == (1 if C_ == 1 else 2)
        if C_ > 2:
            assert got.label[3] == C_ // 3                                 # tied maxima: the lower class


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, bound, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    import deeptreeattention_amd
    from deeptreeattention_amd import build, evaluate
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    new = {"dta_eval_count": 12, "dta_eval_report": 12, "dta_first_rows": 7, "dta_novel_scores": 7}
    assert set(new) <= names
    for n, args in new.items():
        assert hasattr(lib, n) and '"%s"' % n in entry
        assert len(getattr(lib, n).argtypes) == args and getattr(lib, n).restype is C.c_int

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert macro("DTA_EVAL_MAX_SPECIES") == evaluate.MAX_SPECIES == 1020
    assert macro("DTA_EVAL_MAX_SITE_WORDS") == evaluate.MAX_SITE_WORDS == 4
    assert macro("DTA_EVAL_COUNT_PLAIN") == evaluate.PLAIN and macro("DTA_EVAL_COUNT_COMBINE") == evaluate.COMBINE
    assert evaluate.FORM in (evaluate.PLAIN, evaluate.COMBINE)
    assert "evaluate.hip" in build.SOURCES and lib.dta_abi_version() == 2 and macro("DTA_ABI_VERSION") == 2
    assert "deeptreeattention_amd.evaluate" in deeptreeattention_amd.__doc__
    src = open(os.path.join(build.CSRC, "evaluate.hip")).read()
    assert '#include "top2_dev.h"' in src and "softmax_top2_row_body(" in src and "__expf" not in src   # the shared row body, not a copy
    assert "fast-math" not in " ".join(build.FLAGS) and "-ffp-contract=fast" not in build.FLAGS


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (the test runs without a GPU): the device pointers are host buffers nobody
    dereferences."""
    buf = (C.c_ubyte * 4096)()
    p = C.c_void_p(C.addressof(buf))

    def count(labels=p, preds=p, group=p, g64=1, mask=p, rows=100, S=40, G=7, form=0, conf=p, tally=p):
        return lib.dta_eval_count(labels, preds, group, g64, mask, rows, S, G, form, conf, tally, None)

    def report(conf=p, S=40, G=7, sites=p, W=1, genus=p, counts=p, scores=p, acc=p, pre=p, sup=p):
        return lib.dta_eval_report(conf, S, G, sites, W, genus, counts, scores, acc, pre, sup, None)

    def first(ids=p, i64=1, rows=100, n=40, out=p, work=p):
        return lib.dta_first_rows(ids, i64, rows, n, out, work, None)

    def novel(logits=p, rows=100, classes=40, label=p, top=p, soft=p):
        return lib.dta_novel_scores(logits, rows, classes, label, top, soft, None)

    table = [
        (count, [({k: None}, "null") for k in ("labels", "preds", "conf", "tally")] +
         [({"S": 0}, "n_species=0"), ({"S": 1021}, "n_species=1021"), ({"G": 0}, "groups=0"), ({"rows": 0}, "rows=0"),
          ({"rows": 1 << 31}, "rows=2147483648"), ({"S": 1020, "G": 2065}, "groups=2065"), ({"form": 2}, "form=2")]),
        (report, [({k: None}, "null") for k in ("conf", "counts", "scores")] +
         [({"S": 0}, "n_species=0"), ({"S": 1021}, "n_species=1021"), ({"W": 5}, "site_words=5"), ({"W": 0}, "site_words=0"),
          ({"G": 0}, "groups=0"), ({"acc": None}, "all three or none"), ({"sup": None}, "all three or none")]),
        (first, [({k: None}, "null") for k in ("ids", "out", "work")] +
         [({"rows": 0}, "rows=0"), ({"n": 0}, "n_ids=0"), ({"n": 1 << 31}, "n_ids=2147483648")]),
        (novel, [({k: None}, "null") for k in ("logits", "label", "top", "soft")] +
         [({"classes": 0}, "classes=0"), ({"classes": 1021}, "classes=1021"), ({"rows": 0}, "rows=0")]),
    ]
    for fn, cases in table:
        for kw, what in cases:
            assert fn(**kw) != 0, (fn.__name__, kw)
            err = lib.dta_last_error().decode()
            assert err.startswith("dta_") and what in err, (fn.__name__, kw, err)
    assert 2064 * 1020 * 1020 <= 2 ** 31 - 1 < 2065 * 1020 * 1020          # the size rule's edge, as the docstring states it


def test_python_route_checks_its_arguments_on_the_host():
    """Every refusal below is raised before the library is reached; mismatched lengths among them."""
    import torch
    from deeptreeattention_amd import evaluate
    with pytest.raises(ValueError, match="n_species must be in 1 .. 1020"):
        evaluate.count_np([0], [0], n_species=0)
    with pytest.raises(ValueError, match="n_species must be in 1 .. 1020"):
        evaluate.count_np([0], [0], n_species=1021)
    with pytest.raises(ValueError, match=r"2\^31 - 1"):
        evaluate.count_np([0], [0], n_species=1020, groups=2065)
    with pytest.raises(ValueError, match="one entry per row"):
        evaluate.count_np([0, 1], [0], n_species=3)
    with pytest.raises(ValueError, match="one entry per row"):
        evaluate.count_np([0, 1], [0, 1], mask=[True], n_species=3)
    conf = np.zeros((2, 3, 3), np.int64)
    with pytest.raises(ValueError, match="site_masks must be uint64"):
        evaluate.report_np(conf, np.zeros((3, 5), np.uint64))
    with pytest.raises(ValueError, match="site_masks must be uint64"):
        evaluate.report_np(conf, np.zeros((3, 1), np.int64))
    with pytest.raises(ValueError, match="genus must be int32"):
        evaluate.report_np(conf, None, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="integer"):
        evaluate.report_np(conf.astype(np.float64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        evaluate.EvalTable(3, device="cpu")
    with pytest.raises(ValueError, match="device tensor"):
        evaluate.novel_scores(np.zeros((2, 2), np.float32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        evaluate.novel_scores(torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        evaluate.first_per_individual(torch.zeros(2, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="need n_individuals"):
        evaluate.evaluate_crowns(np.zeros(2, np.int64), np.zeros(2, np.int64), individual=np.zeros(2, np.int64), n_species=2)
    assert evaluate.EvalReport.words(23, 200, True) == 24 * (12 + 600) and evaluate.EvalReport.words(1, 5, False) == 24
