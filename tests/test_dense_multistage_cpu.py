"""Dense multi-stage prediction on the host (no GPU): `dense.crown_resolve_np`, the written-down meaning of
dta_crown_resolve, against the explicit composition of `crown_reduce_np` and `Hierarchy.resolve_np`, and against the
reference's own `gather_predictions` + `ensemble` output with every crop as its own one-window crown; the new C entry
points are declared, exported and refuse bad arguments before anything is launched."""
import os
import re

import numpy as np

from test_hierarchy_cpu import load_ensemble_fixture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dta_gather_windows_years", "dta_crown_resolve")
CROWN_ROWS = (0, 1, 4, 5, 7)      # an empty crown, one window, the four-loads-in-flight step of the kernel exactly, that + 1, + 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def three_level_hierarchy():
    """Classes 3, 2, 5; every branch reachable: level 0 class 0 ends (species 0), class 1 -> level 1, class 2 -> level 2;
    level 1 class 0 ends (species 1), class 1 -> level 2; level 2's five classes are species 2..6."""
    from deeptreeattention_amd.hierarchy import Hierarchy
    return Hierarchy([[-1, 1, 2], [-1, 2], [-1] * 5], [[0, -1, -1], [1, -1], [2, 3, 4, 5, 6]], 7)


def random_probs(rng, rows, classes):
    z = rng.standard_normal((rows, classes)).astype(np.float32) * 2
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def test_crown_resolve_np_is_reduce_per_level_then_the_walk_then_a_bincount():
    from deeptreeattention_amd.dense import crown_reduce_np, crown_resolve_np
    h = three_level_hierarchy()
    assert h.classes == [3, 2, 5]
    rng = np.random.default_rng(21)
    offsets = np.concatenate([[0], np.cumsum(CROWN_ROWS)]).astype(np.int64)
    rows = int(offsets[-1])
    probs = [random_probs(rng, rows, c) for c in h.classes]
    win = rng.integers(-1, h.n_species, rows)          # the windows' own labels, some of them -1
    assert (win == -1).any()
    got = crown_resolve_np(probs, offsets, h, window_labels=win)
    per = [crown_reduce_np(p, offsets) for p in probs]
    label, score, level = h.resolve_np([r[1][:, 0] for r in per], [r[2][:, 0] for r in per])
    assert got.label.dtype == np.int64 and got.level.dtype == np.int32 and got.count.dtype == np.int32
    assert np.array_equal(got.label, label) and np.array_equal(got.level, level)
    assert np.array_equal(bits(got.score), bits(score))
    assert got.count.tolist() == list(CROWN_ROWS)
    for l, (mean, ti, ts, cnt) in enumerate(per):
        assert np.array_equal(bits(got.mean[l]), bits(mean)) and np.array_equal(got.top_idx[l], ti), l
        assert np.array_equal(bits(got.top_score[l]), bits(ts)) and np.array_equal(cnt, got.count), l
    # the empty crown: no label at any level, the walk ends at level 0 with score 0
    assert got.label[0] == -1 and got.level[0] == 0 and got.score[0] == 0.0
    assert all(int(got.top_idx[l][0, 0]) == -1 for l in range(3))
    assert set(got.level.tolist()) == {0, 1, 2}
    # votes: a bincount of each crown's window labels, -1 skipped
    assert got.votes.dtype == np.int32 and got.votes.shape == (len(CROWN_ROWS), h.n_species)
    for k in range(len(CROWN_ROWS)):
        mine = win[offsets[k]:offsets[k + 1]]
        assert np.array_equal(got.votes[k], np.bincount(mine[mine >= 0], minlength=h.n_species)), k
    assert int(got.votes.sum()) == int((win >= 0).sum()) < rows
    assert crown_resolve_np(probs, offsets, h).votes is None


def test_one_window_per_crown_is_the_reference_ensemble():
    """tests/golden/multistage_ensemble.json (the reference's own gather_predictions + ensemble): every crop its own
    crown -- a mean over one row is that row, so the crown label, score bits and level are the reference's."""
    from deeptreeattention_amd.dense import crown_resolve_np
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    n = len(fx["names"])
    got = crown_resolve_np(fx["probs"], np.arange(n + 1), h, window_labels=fx["ens_label"])
    assert np.array_equal(got.label, fx["ens_label"])
    assert np.array_equal(bits(got.score), bits(fx["ens_score"]))
    assert np.array_equal(got.level, fx["branch_level"])
    assert sorted(set(got.level.tolist())) == [0, 2, 3, 4]
    assert got.count.tolist() == [1] * n
    for l in range(5):
        assert np.array_equal(bits(got.mean[l]), bits(fx["probs"][l]))
        assert np.array_equal(got.top_idx[l][:, 0], fx["top1"][l])
    assert np.array_equal(got.votes.argmax(1), fx["ens_label"]) and (got.votes.sum(1) == 1).all()


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    import ctypes as C
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    declared = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    assert L.dta_abi_version() == 2
    # null arguments, no year present, too many years: refused on the host
    assert L.dta_gather_windows_years(None, 3, 20, 4, 4, None, 1, 11, None, None, None, None) != 0
    assert b"dta_gather_windows_years" in L.dta_last_error()
    none = (C.c_void_p * 3)()
    flags = (C.c_float * 6)()
    fp = C.cast(flags, C.c_void_p)
    assert L.dta_gather_windows_years(none, 3, 20, 4, 4, None, 1, 11, none, fp, None, None) != 0
    assert b"every year is missing" in L.dta_last_error()
    assert L.dta_gather_windows_years(none, 17, 20, 4, 4, None, 1, 11, none, fp, None, None) != 0
    assert b"years" in L.dta_last_error()
    assert L.dta_gather_windows_years(none, 3, 20, 4, 4, None, 1, 11, none, fp, fp, None) != 0        # one bank for both
    assert L.dta_crown_resolve(3, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"dta_crown_resolve" in L.dta_last_error()


def test_the_route_refuses_what_it_cannot_run_without_a_device():
    """The checks that come before anything touches the device need none: a predictor that is no MultiStagePredictor."""
    import pytest
    from deeptreeattention_amd.dense import crown_resolve_np, predict_windows_multistage
    with pytest.raises(TypeError):
        predict_windows_multistage(object(), [None], np.zeros((1, 2), np.int32))
    with pytest.raises(ValueError):
        crown_resolve_np([np.zeros((1, 3), np.float32)], [0, 1], three_level_hierarchy())
