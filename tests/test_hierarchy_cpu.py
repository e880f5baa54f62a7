"""The hierarchy walk and the evaluation figures on the host (no GPU): `hierarchy.Hierarchy` against the reference's own
`gather_predictions` + `ensemble` output (tests/golden/multistage_ensemble.json, made by tools/make_ensemble_golden.py),
the constructor's refusals, `scores_from_confusion`, and the argument checks of the two new C entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_ensemble_fixture():
    """The fixture as arrays, with the conditions its generator asserts checked again: unique individuals, the
    reference's rows joined on the name (it sorts them as strings), no tie for first place, every terminal branch taken
    by at least 8 rows of the reference's own output."""
    with open(os.path.join(REPO, "tests", "golden", "multistage_ensemble.json")) as f:
        g = json.load(f)
    names = g["input"]["individual"]
    assert len(set(names)) == len(names)
    probs = [np.array(p, np.uint32).view(np.float32) for p in g["input"]["probs_bits"]]
    for p in probs:
        assert p.shape[0] == len(names)
        top = np.sort(p, 1)
        assert (top[:, -1] > top[:, -2]).all()
    ref = g["reference"]
    assert sorted(ref["individual"]) == sorted(names) and ref["individual"] != names
    at = {n: i for i, n in enumerate(ref["individual"])}
    order = np.array([at[n] for n in names])                 # the reference's row of each input row
    out = {"level_label_dicts": g["level_label_dicts"], "species_label_dict": g["species_label_dict"], "probs": probs,
           "names": names,
           "taxon": [ref["ensembleTaxonID"][i] for i in order],
           "ens_label": np.array(ref["ens_label"], np.int64)[order],
           "ens_score": np.array(ref["ens_score_bits"], np.uint32).view(np.float32)[order],
           "top1": [np.array(t, np.int64)[order] for t in ref["pred_label_top1"]],
           "top1_score": [np.array(t, np.uint32).view(np.float32)[order] for t in ref["top1_score_bits"]]}
    # the four terminal branches, counted on the reference's own columns
    taxa = [{v: k for k, v in d.items()} for d in g["level_label_dicts"]]
    t = [[taxa[l][int(c)] for c in out["top1"][l]] for l in range(3)]
    n0 = sum(a == "PIPA2" for a in t[0])
    n3 = sum(a != "PIPA2" and b != "BROADLEAF" for a, b in zip(t[0], t[1]))
    n4 = sum(a != "PIPA2" and b == "BROADLEAF" and c == "OAK" for a, b, c in zip(*t))
    n2 = len(names) - n0 - n3 - n4
    assert min(n0, n2, n3, n4) >= 8, (n0, n2, n3, n4)
    out["branch_level"] = np.array([0 if a == "PIPA2" else 3 if b != "BROADLEAF" else 4 if c == "OAK" else 2 for a, b, c in zip(*t)],
                                   np.int32)
    return out


def test_resolve_np_reproduces_the_reference_ensemble():
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    assert h.levels == 5 and h.classes == [2, 2, 3, 3, 3] and h.n_species == 9
    top1 = [p.argmax(1) for p in fx["probs"]]
    score = [p.max(1) for p in fx["probs"]]
    for l in range(5):       # the per-level columns of gather_predictions
        assert np.array_equal(top1[l], fx["top1"][l])
        assert np.array_equal(score[l].view(np.uint32), fx["top1_score"][l].view(np.uint32))
    label, sc, level = h.resolve_np(top1, score)
    assert label.dtype == np.int64 and sc.dtype == np.float32 and level.dtype == np.int32
    assert np.array_equal(label, fx["ens_label"])
    assert np.array_equal(sc.view(np.uint32), fx["ens_score"].view(np.uint32))        # a selection: bit for bit
    assert np.array_equal(level, fx["branch_level"])
    species = {v: k for k, v in fx["species_label_dict"].items()}
    assert [species[int(v)] for v in label] == fx["taxon"]


def test_table_layout_and_out_of_range_classes():
    from deeptreeattention_amd.hierarchy import Hierarchy
    h = Hierarchy([[-1, 1], [-1, -1, -1]], [[4, -1], [0, 1, 2]], 5)
    assert h.table_np().dtype == np.int32
    assert h.table_np().tolist() == [0, 2, 5, -1, 1, -1, -1, -1, 4, -1, 0, 1, 2]
    label, sc, level = h.resolve_np([[0, 1, 1, -1, 1], [0, 2, 3, 0, -1]], [[.9, .8, .7, .6, .5], [.1, .2, .3, .4, .45]])
    assert label.tolist() == [4, 2, -1, -1, -1]
    assert level.tolist() == [0, 1, 1, 0, 1]
    assert np.array_equal(sc, np.array([.9, .2, .3, .6, .45], np.float32))


def test_constructor_refusals():
    from deeptreeattention_amd.hierarchy import Hierarchy, MAX_LEVELS
    Hierarchy([[-1, 1], [-1]], [[0, -1], [1]], 2)                                   # fine
    with pytest.raises(ValueError, match="later"):
        Hierarchy([[-1, 1], [0]], [[0, -1], [-1]], 2)                               # a backward edge
    with pytest.raises(ValueError, match="later"):
        Hierarchy([[0, -1]], [[-1, 0]], 1)                                          # a self edge
    with pytest.raises(ValueError, match="later"):
        Hierarchy([[-1, 2], [-1]], [[0, -1], [1]], 2)                               # an edge past the last level
    with pytest.raises(ValueError, match="species"):
        Hierarchy([[-1, -1]], [[0, -1]], 2)                                         # a terminal without species
    with pytest.raises(ValueError, match="species"):
        Hierarchy([[-1, -1]], [[0, 2]], 2)                                          # ... or with one out of range
    with pytest.raises(ValueError, match="levels"):
        Hierarchy([[-1]] * (MAX_LEVELS + 1), [[0]] * (MAX_LEVELS + 1), 1)
    with pytest.raises(ValueError, match="levels"):
        Hierarchy([], [], 1)
    dicts = [{"PIPA2": 0, "OTHER": 1}, {"CONIFER": 0, "BROADLEAF": 1}, {"ACRU": 0, "OAK": 1}, {"PICL": 0}, {"QUGE2": 0}]
    species = {"PIPA2": 0, "ACRU": 1, "PICL": 2, "QUGE2": 3}
    Hierarchy.from_reference(dicts, species)
    with pytest.raises(KeyError):
        Hierarchy.from_reference(dicts, {k: v for k, v in species.items() if k != "PICL"})      # a missing taxon
    with pytest.raises(ValueError):
        Hierarchy.from_reference(dicts[:4], species)


def test_scores_from_confusion_against_a_direct_count():
    from deeptreeattention_amd.hierarchy import scores_from_confusion
    rng = np.random.default_rng(5)
    n = 7
    y = rng.integers(0, n - 1, 500)           # species n - 1 never occurs as a label ...
    p = rng.integers(0, n, 500)
    p[p == 2] = 3                             # ... and species 2 is never predicted
    conf = np.zeros((n, n), np.int64)
    np.add.at(conf, (y, p), 1)
    s = scores_from_confusion(conf)
    acc, prec = np.zeros(n), np.zeros(n)
    for k in range(n):
        if (y == k).any():
            acc[k] = ((p == k) & (y == k)).sum() / (y == k).sum()
        if (p == k).any():
            prec[k] = ((p == k) & (y == k)).sum() / (p == k).sum()
    assert np.array_equal(s["accuracy"], acc) and np.array_equal(s["precision"], prec)
    assert s["accuracy"][n - 1] == 0.0 and s["precision"][2] == 0.0
    assert s["micro"] == (y == p).mean()
    assert np.isclose(s["macro"], acc[:n - 1].mean(), rtol=1e-15, atol=0)       # the empty species is left out
    z = scores_from_confusion(np.zeros((3, 3), np.int64))
    assert z["micro"] == 0.0 and z["macro"] == 0.0 and not z["accuracy"].any()
    with pytest.raises(ValueError):
        scores_from_confusion(np.zeros((2, 3)))


def test_ensemble_entry_points_refuse_bad_arguments_on_cpu():
    """dta_hierarchy_resolve and dta_multistage_predict_ensemble check their arguments on the host, before anything is
    launched: null table or outputs, labels without confusion or the reverse, a level count or class count that does
    not match the table.  (The device pointers here are never dereferenced.)"""
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    fake = C.c_void_p(4096)

    def table(classes, n_species=9, ptr=4096):
        return _lib.HierarchyTable(len(classes), n_species, (C.c_int * _lib.MAX_LEVELS)(*classes), ptr)

    def arr(n):
        return (C.c_void_p * n)(*([4096] * n))

    def err():
        return L.dta_last_error().decode()
    t5 = table([2, 2, 3, 3, 3])
    r = L.dta_hierarchy_resolve
    assert r(5, arr(5), arr(5), 64, None, fake, fake, fake, None, None, None) == 1 and "null hierarchy table" in err()
    assert r(5, arr(5), arr(5), 64, C.byref(table([2, 2, 3, 3, 3], ptr=None)), fake, fake, fake, None, None, None) == 1
    assert "null hierarchy table" in err()
    for outs in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert r(5, arr(5), arr(5), 64, C.byref(t5), *outs, None, None, None) == 1 and "null ensemble output" in err()
    assert r(5, arr(5), arr(5), 64, C.byref(t5), fake, fake, fake, fake, None, None) == 1 and "together" in err()
    assert r(5, arr(5), arr(5), 64, C.byref(t5), fake, fake, fake, None, fake, None) == 1 and "together" in err()
    assert r(4, arr(4), arr(4), 64, C.byref(t5), fake, fake, fake, None, None, None) == 1 and "5 levels, the call 4" in err()
    assert r(9, arr(9), arr(9), 64, C.byref(t5), fake, fake, fake, None, None, None) == 1 and "levels" in err()
    assert r(5, None, arr(5), 64, C.byref(t5), fake, fake, fake, None, None, None) == 1 and "null argument" in err()
    assert r(5, arr(5), arr(5), 0, C.byref(t5), fake, fake, fake, None, None, None) == 1 and "empty batch" in err()
    holes = arr(5)
    holes[3] = None
    assert r(5, holes, arr(5), 64, C.byref(t5), fake, fake, fake, None, None, None) == 1 and "level 3" in err()
    assert r(5, arr(5), arr(5), 64, C.byref(table([2, 2, 0, 3, 3])), fake, fake, fake, None, None, None) == 1 and "level 2" in err()
    assert r(5, arr(5), arr(5), 64, C.byref(table([2, 2, 3, 3, 3], n_species=0)), fake, fake, fake, None, None, None) == 1
    assert "species" in err()

    desc = _lib.NetDesc(64, 369, 11, 11, 2, _lib.NET_SPECTRAL, _lib.DTA_BF16, 0, 4 | _lib.FORWARD_ONLY, 0.1, 1e-5)
    spec = [(2, 0, 3), (2, 3, 3), (3, 6, 3), (3, 9, 3), (3, 12, 3)]
    lv = (_lib.Level * 5)(*[_lib.Level(c, f, n, None, None, None, None, None, None, None) for c, f, n in spec])
    nets = (_lib.SubnetParams * 15)()
    x = arr(15)
    p = L.dta_multistage_predict_ensemble

    def call(levels=5, lv=lv, nets=nets, x=x, ws=fake, tbl=C.byref(t5), outs=(fake, fake, fake), labels=None, conf=None):
        return p(C.byref(desc), levels, lv, nets, x, None, ws, None, arr(5), arr(5), tbl, *outs, labels, conf, None)
    assert call(nets=None) == 1 and "null argument" in err()
    assert call(ws=None) == 1 and "null argument" in err()
    assert call(tbl=None) == 1 and "null hierarchy table" in err()
    assert call(outs=(fake, None, fake)) == 1 and "null ensemble output" in err()
    assert call(labels=fake) == 1 and "together" in err()
    assert call(conf=fake) == 1 and "together" in err()
    assert call(tbl=C.byref(table([2, 2, 3, 3]))) == 1 and "4 levels, the call 5" in err()
    assert call(tbl=C.byref(table([2, 2, 3, 4, 3]))) == 1 and "level 3 has 3 classes, the hierarchy table 4" in err()
    bad = (_lib.Level * 5)(*[_lib.Level(c, f + (1 if f else 0), n, None, None, None, None, None, None, None) for c, f, n in spec])
    assert call(lv=bad) == 1 and "adjacent" in err()
    xh = arr(15)
    xh[7] = None
    assert call(x=xh) == 1 and "null input for network 7" in err()
