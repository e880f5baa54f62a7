"""levels.build_np -- the definition of the five level data sets -- against the reference's own MultiStage, as recorded in
tests/golden/levels/levels_reference.npz (tools/make_levels_golden.py), and its refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import levels_cases as LC  # noqa: E402

from deeptreeattention_amd import levels as LV  # noqa: E402


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("which", ["train", "test"])
def test_build_np_is_the_references_create_datasets(case, which):
    """Every level: the individuals in data set order, the labels, the kept years; train: num_classes and the loss weights
    bit for bit as float32 -- under the level-2 shuffles the reference drew."""
    c = LC.fixture()[case]
    train = which == "train"
    got = LV.build_np(c[which]["table"], c["rules"], c["config"], train=train, orders=c["orders"] if train else None)
    for l, want in enumerate(c[which]["sets"]):
        assert np.array_equal(got.rows[l], want["rows"]), ("individuals", l)
        assert np.array_equal(got.labels[l], want["labels"]), ("labels", l)
        assert np.array_equal(got.year_keep[l], want["year_keep"]), ("year_keep", l)
        assert got.n[l] == len(want["rows"])
    if train:
        assert got.num_classes == c["num_classes"]
        for l in range(5):
            assert got.loss_weight[l].dtype == np.float32
            assert np.array_equal(got.loss_weight[l].view(np.uint32), c["loss_weight"][l].view(np.uint32)), l
    else:
        assert got.num_classes is None and got.loss_weight is None


def test_the_fixture_holds_what_it_is_meant_to():
    """The properties the tool asserted when it made the file, read back from the file."""
    cases = LC.fixture()
    c = cases[0]
    t, rules = c["train"]["table"], c["rules"]
    kind = rules.cls[t.sp]
    assert (np.diff(t.rank) < 0).any()                                     # string order is not first appearance
    assert t.m.max() > t.present.sum(1).max() or (t.m > t.present.sum(1)).any()      # a duplicated (individual, year) row
    assert {1, 2, 3} <= set(t.present.sum(1).tolist())
    per = np.bincount(t.sp[kind != LV.HEAD], minlength=rules.C)
    oc = c["config"]["other_sampling_ceiling"]
    assert oc in per and oc + 1 in per and ((per > 0) & (per < oc)).any()
    mods = [int(x["train"]["table"].m[x["rules"].cls[x["train"]["table"].sp] == LV.CONIFER].sum()) % 11 for x in cases]
    assert mods[0] == 0 and mods[1] == 1
    t2, r2 = cases[2]["train"]["table"], cases[2]["rules"]
    assert int(t2.m[r2.cls[t2.sp] == LV.PLAIN].sum()) // 5 == 0            # k2 = 0
    k2 = int(t.m[kind == LV.PLAIN].sum()) // 5
    rsp = t.sp[t.ind]
    assert any(0 < (rsp == s).sum() < k2 for s in c["orders"])            # an OAK species with fewer than k2 records
    assert any(len(set(t.ind[o[:k2]].tolist())) < len(o[:k2]) for o in c["orders"].values())      # named twice
    l3 = c["train"]["sets"][3]
    assert not np.array_equal(l3["year_keep"], t.present[l3["rows"]])      # the ceiling cuts an individual's year
    assert (np.diff(t.first[l3["rows"]]) < 0).any()                        # level 3 is regrouped by species
    assert not (rules.cls[c["test"]["table"].sp] == LV.HEAD).any()         # a frame without HEAD
    floor = np.float32(c["config"]["min_loss_weight"])
    assert any((w == floor).any() and (w > floor).sum() > 1 for w in c["loss_weight"])


def test_level_three_can_lose_a_year_and_the_weights_count_kept_records():
    c = LC.fixture()[0]
    t = c["train"]["table"]
    got = LV.build_np(t, c["rules"], c["config"], orders=c["orders"])
    lab, keep = got.labels[3], got.year_keep[3]
    # the ceiling counts records: every CONIFER species keeps at most evergreen_ceiling of them
    assert keep.sum() <= c["config"]["evergreen_ceiling"] * 3
    assert keep.sum() < t.present[got.rows[3]].sum()
    assert len(lab) == got.n[3]


def _frame(rows):
    cols = ("individual", "tile_year", "taxonID", "label")
    return {k: np.array([r[i] for r in rows]) for i, k in enumerate(cols)}


def test_refusals():
    with pytest.raises(ValueError, match="disagree on taxonID or label"):
        LV.RecordTable.from_frame(_frame([("a", 2019, "ACRU", 0), ("b", 2019, "PIPA2", 1), ("a", 2020, "PIPA2", 1)]))
    with pytest.raises(ValueError, match="disagree on taxonID or label"):
        LV.RecordTable.from_frame(_frame([("a", 2019, "ACRU", 0), ("a", 2020, "ACRU", 1)]))
    with pytest.raises(ValueError, match="overlap"):
        LV.Rules.reference({"PIPA2": 0, "QUPI": 1, "ACRU": 2}, conifers=("QUPI",))
    with pytest.raises(ValueError, match="without gaps"):
        LV.Rules.reference({"PIPA2": 0, "ACRU": 2})
    config = {"other_sampling_ceiling": 5, "evergreen_ceiling": 5, "oaks_sampling_ceiling": 5, "min_loss_weight": 0.1}
    names = {"PIPA2": 0, "PICL": 1, "QUGE2": 2, "ACRU": 3}
    rules = LV.Rules.reference(names)
    full = [("a", 2019, "PIPA2", 0), ("b", 2019, "PICL", 1), ("c", 2019, "QUGE2", 2), ("d", 2019, "ACRU", 3),
            ("e", 2019, "ACRU", 3), ("f", 2019, "ACRU", 3), ("g", 2019, "ACRU", 3), ("h", 2019, "ACRU", 3)]
    LV.build_np(LV.RecordTable.from_frame(_frame(full)), rules, config)          # (this one is fine)
    # no HEAD: level 0 has label 1 only, and the reference would divide by zero
    with pytest.raises(ValueError, match="level 0: label 0"):
        LV.build_np(LV.RecordTable.from_frame(_frame(full[1:])), rules, config)
    # no OAK: level 4 is empty
    with pytest.raises(ValueError, match="level 4 is empty"):
        LV.build_np(LV.RecordTable.from_frame(_frame(full[:2] + full[3:])), rules, config)
    with pytest.raises(ValueError, match="level 3 is empty"):
        LV.build_np(LV.RecordTable.from_frame(_frame(full[:1] + full[2:])), rules, config, train=False)
    with pytest.raises(ValueError, match="config lacks"):
        LV.build_np(LV.RecordTable.from_frame(_frame(full)), rules, {"evergreen_ceiling": 1})
    with pytest.raises(ValueError, match="every record of OAK species"):
        LV.build_np(LV.RecordTable.from_frame(_frame(full)), rules, config, orders={2: [0]})
    # a single individual cannot fill five levels
    with pytest.raises(ValueError, match="is empty"):
        LV.build_np(*LC.synthetic(1, 0), LC.CONFIG)


def test_epoch_changes_level_two_and_nothing_else():
    table, rules = LC.synthetic(1025, 3)
    config = dict(LC.CONFIG, other_sampling_ceiling=30)
    a = LV.build_np(table, rules, config, seed=5, epoch=0)
    b = LV.build_np(table, rules, config, seed=5, epoch=1)
    LC.same(a, LV.build_np(table, rules, config, seed=5, epoch=0), True)
    for l in (0, 1, 3, 4):
        assert np.array_equal(a.rows[l], b.rows[l]) and np.array_equal(a.labels[l], b.labels[l])
        assert np.array_equal(a.year_keep[l], b.year_keep[l])
        assert np.array_equal(a.loss_weight[l], b.loss_weight[l])
    assert not np.array_equal(a.rows[2], b.rows[2])
    assert not np.array_equal(a.rows[2], LV.build_np(table, rules, config, seed=6, epoch=0).rows[2])
    # test levels draw nothing
    LC.same(LV.build_np(table, rules, config, train=False, seed=1, epoch=2),
            LV.build_np(table, rules, config, train=False, seed=9, epoch=7), False)


def test_hashed_shuffle_is_the_stated_formula():
    from deeptreeattention_amd.abundance import _mix_int, stream_key
    R, epoch, seed = 37, 3, 11
    want = [_mix_int((((epoch * R + r) & (2 ** 64 - 1)) * 0x9E3779B97F4A7C15 + stream_key(seed, 2)) & (2 ** 64 - 1)) >> 32
            for r in range(R)]
    assert LV.hashed_keys_np(R, epoch, seed).tolist() == want


def test_batch_np_year_keep_masks_a_year_as_a_missing_one():
    from deeptreeattention_amd import treedata as T
    crops = np.arange(1, 1 + 3 * 2 * 2 * 3 * 3, dtype=np.float32).reshape(3, 2, 2, 3, 3)
    rows = np.array([2, 0])
    plain = T.batch_np(crops, rows, True)
    keep = np.array([[1, 0], [1, 1]], np.uint8)
    got = T.batch_np(crops, rows, True, year_keep=keep)
    assert np.array_equal(got[0], plain[0])
    assert not got[1][0].any() and np.array_equal(got[1][1], plain[1][1])
    for a, b in zip(T.batch_np(crops, rows, False, year_keep=None), T.batch_np(crops, rows, False)):
        assert np.array_equal(a, b)
