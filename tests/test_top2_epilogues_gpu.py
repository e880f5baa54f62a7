"""The softmax / top-2 rule of the two entry points that take raw scores, dta_softmax_top2 and dta_eval_metrics (both run
softmax_top2_row_body, csrc/top2_dev.h): the stored top-2 of a row is the two largest entries of that entry's OWN returned
probabilities under (value descending, class ascending), an empty slot is (-1, -1.0), a NaN row gives (-1, -1) and is
counted nowhere, and the two entries agree with each other bit for bit.  B = 5 (a partial last workgroup); class counts 1,
2, 64, 65, 256, 257 and 321: one lane, a wave boundary, the end of the register-held part of a row and the re-formed tail.

Nothing here rests on the last bit of __expf: the rows have either no near ties (steps of 0.05 in the scores) or exact ones
(equal scores give equal probabilities, whatever __expf returns for them)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 5
CLASSES = [1, 2, 64, 65, 256, 257, 321]
NAN_ROW = 4
# the maximum planted twice: the same lane in two register slots (3, 67), different lanes (5, 70), register-held against
# re-formed tail (2, 258), each at one class count that has both positions; narrower rows take their first and last class
# (65: classes 0 and 64, one lane's first two slots)
PLANTED = {256: (3, 67), 257: (5, 70), 321: (2, 258)}


def dev():
    return torch.device("cuda:0")


def _scores(classes):
    """[5][classes] float32: two permutations of 0.05 * arange, an all-equal row, a row with its maximum twice, a row
    with one NaN.  Labels: the first row's largest score, the second row's second largest, the second of the equal ones, the
    second planted maximum (the last three are rank 1 where the row has two classes: a top-2 hit, no top-1 hit), class 0."""
    rng = np.random.default_rng(20 + classes)
    ramp = (0.05 * np.arange(classes)).astype(np.float32)
    s = np.stack([rng.permutation(ramp) for _ in range(B)])
    y = np.array([np.argsort(s[0])[-1], np.argsort(s[1])[-min(2, classes)], min(1, classes - 1), 0, 0], np.int64)
    s[2] = 0.25
    lo, hi = PLANTED.get(classes, (0, classes - 1))
    s[3, lo] = s[3, hi] = np.float32(0.05 * classes + 1.0)
    y[3] = hi
    s[NAN_ROW, classes // 2] = np.nan
    return s, y


def _two_largest(p):
    """(classes, values) of the two largest entries of p under (value descending, class ascending); (-1, -1.0) where p has
    no such entry, and twice for a row with a NaN."""
    idx, val = np.full(2, -1, np.int64), np.full(2, -1.0, np.float32)
    if not np.isnan(p).any():
        order = np.lexsort((np.arange(len(p)), -p.astype(np.float64)))[:2]
        idx[:len(order)], val[:len(order)] = order, p[order]
    return idx, val


def _check_rows(who, probs, top_idx, top_score, classes):
    for r in range(B):
        idx, val = _two_largest(probs[r])
        print(who, "classes", classes, "row", r, "top_idx", top_idx[r], "expected", idx, "top_score", top_score[r], "expected", val)
        assert np.array_equal(top_idx[r], idx), (who, classes, r)
        assert np.array_equal(top_score[r], val), (who, classes, r)
    assert (top_idx[NAN_ROW] == -1).all() and np.isnan(probs[NAN_ROW]).all()
    if classes == 1:
        assert (top_idx[:, 1] == -1).all() and (top_score[:, 1] == -1.0).all()
    lo, hi = PLANTED.get(classes, (0, classes - 1))
    assert list(top_idx[3]) == ([lo, hi] if classes > 1 else [0, -1])
    assert list(top_idx[2]) == ([0, 1] if classes > 1 else [0, -1])


def _softmax_top2(s, classes):
    from deeptreeattention_amd import _lib
    sd = torch.from_numpy(s).to(dev())
    probs = torch.empty(B, classes, device=dev())
    ti = torch.empty(B, 2, dtype=torch.int64, device=dev())
    ts = torch.empty(B, 2, device=dev())
    rc = _lib.lib().dta_softmax_top2(_lib.ptr(sd), B, classes, _lib.ptr(probs), _lib.ptr(ti), _lib.ptr(ts), _lib.current_stream_ptr())
    if classes < 2:                                    # this entry point takes two classes or more, and says so
        assert rc != 0
        return None
    _lib.check(rc, "dta_softmax_top2")
    torch.cuda.synchronize()
    return probs.cpu().numpy(), ti.cpu().numpy(), ts.cpu().numpy()


def _eval_metrics(s, y, classes, top_k):
    """As tests/test_validation_gpu.py calls it.  Returns probs, top_idx, top_score, confusion, counts."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.engine import EvalAccumulators
    acc = EvalAccumulators([classes], dev())
    sd, yd = torch.from_numpy(s).to(dev()), torch.from_numpy(y).to(dev())
    probs = torch.empty(B, classes, device=dev())
    ti = torch.empty(B, 2, dtype=torch.int64, device=dev())
    ts = torch.empty(B, 2, device=dev())
    loss = torch.empty((), device=dev())
    scratch = torch.zeros(B + 2, device=dev())
    ev = acc.level(0, probs, ti, ts, top_k)
    _lib.check(_lib.lib().dta_eval_metrics(_lib.ptr(sd), _lib.ptr(yd), None, B, classes, _lib.ptr(loss), _lib.ptr(scratch),
                                           C.byref(ev), _lib.current_stream_ptr()), "dta_eval_metrics")
    torch.cuda.synchronize()
    host = acc.flat.cpu().numpy()
    return (probs.cpu().numpy(), ti.cpu().numpy(), ts.cpu().numpy(), host[:classes * classes].reshape(classes, classes),
            host[classes * classes:classes * classes + 4])


@pytest.mark.parametrize("classes", CLASSES)
def test_top2_rule_on_the_raw_score_entry_points(classes):
    s, y = _scores(classes)
    top_k = min(2, classes)
    probs_e, ti_e, ts_e, confusion, counts = _eval_metrics(s, y, classes, top_k)
    _check_rows("dta_eval_metrics", probs_e, ti_e, ts_e, classes)
    # the NaN row is left out of the counts; the others count with the rule above applied to the returned probabilities
    rows = [r for r in range(B) if r != NAN_ROW]
    exp_conf = np.zeros((classes, classes), np.int64)
    hits_k = 0
    for r in rows:
        exp_conf[y[r], ti_e[r, 0]] += 1
        p = probs_e[r]
        rank = int(((p > p[y[r]]) | ((p == p[y[r]]) & (np.arange(classes) < y[r]))).sum())
        hits_k += rank < top_k
    print("classes", classes, "counts", counts, "expected", [len(rows), int(np.trace(exp_conf)), hits_k, 1])
    assert np.array_equal(confusion, exp_conf)
    assert list(counts) == [len(rows), int(np.trace(exp_conf)), hits_k, 1]
    got = _softmax_top2(s, classes)
    if got is None:
        return
    probs_s, ti_s, ts_s = got
    _check_rows("dta_softmax_top2", probs_s, ti_s, ts_s, classes)
    # the two entries against each other
    assert np.array_equal(ti_s, ti_e)
    assert np.array_equal(probs_s[rows].view(np.uint32), probs_e[rows].view(np.uint32))
    assert np.isnan(probs_s[NAN_ROW]).all() and np.isnan(probs_e[NAN_ROW]).all()
