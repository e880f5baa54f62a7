"""Device-side validation (reference multi_stage.py:290-304 validation_step, :20-28 the metric collection, :323-366
validation_epoch_end; main.py:53-61, :82-133): every level's eval-mode forward, loss, softmax and metric counts in one launch
chain (dta_multistage_validate), against a validation epoch of the reference itself (tests/golden/validation), against
today's level-by-level validation_step, and against NumPy / torch counts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O

pytestmark = pytest.mark.gpu

VAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validation")
sys.path.insert(0, VAL)
import recipe as R  # noqa: E402
sys.path.remove(VAL)


def dev():
    return torch.device("cuda:0")


def _fixture():
    return np.load(os.path.join(VAL, "validation_epoch.npz"), allow_pickle=False)


def _fixture_levels(prec="fp32", training=False):
    from deeptreeattention_amd.year import learned_ensemble
    c = R.VALIDATION
    models, ws = [], []
    for l, classes in enumerate(c["classes"]):
        m = learned_ensemble(years=c["years"], classes=classes, config={"pretrain_state_dict": None, "bands": c["bands"]})
        p = R.params(l, O.init_params, O.learned_ensemble_spec)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
        m = m.to(dev())
        for net in m.year_models:
            net.precision = prec
        m.train(training)
        models.append(m)
        ws.append(torch.from_numpy(R.weight(classes)))
    return models, ws


def _fixture_batch(b, l):
    imgs, y = R.inputs(b, l)
    return (["id"] * len(y), {"HSI": [torch.from_numpy(a).to(dev()) for a in imgs]}, torch.from_numpy(y).to(dev()))


def _rank_hits(probs, y, k):
    """Rows whose label is among the k largest probabilities, ties towards the lower index (NumPy)."""
    py = probs[np.arange(len(y)), y][:, None]
    idx = np.arange(probs.shape[1])[None, :]
    rank = ((probs > py) | ((probs == py) & (idx < y[:, None]))).sum(1)
    return rank < k


def test_validation_epoch_against_the_reference_fixture():
    """The fixture's epoch (three levels of 2 / 5 / 7 classes x three years, batches of 24, 24 and 10 crops, one all-zero year)
    through validation_step_all, with the modules left in train() mode: eval-mode BatchNorm is the call's own.  Per batch and
    level val_loss within 1e-4 relative and yhat rel-L2 < 1e-5 of the reference's F.cross_entropy / F.softmax, top-1 equal on
    every row whose reference top-1 / top-2 gap is at least 1e-4 (at most 5 % of a level's rows may be excluded); per epoch
    the size-weighted val_loss within 1e-4 and the confusion matrix equal on the non-excluded rows.  Every batch is ONE
    chain for all three levels."""
    from deeptreeattention_amd.engine import MultiStageTrainer
    g = _fixture()
    c = R.VALIDATION
    models, ws = _fixture_levels("fp32", training=True)
    tr = MultiStageTrainer(models, [1e-3] * 3, ws)
    nl, nb = len(c["classes"]), len(c["batches"])
    excl_conf = [np.zeros((k, k), np.int64) for k in c["classes"]]
    excluded = np.zeros(nl)
    for b in range(nb):
        batches = [_fixture_batch(b, l) for l in range(nl)]
        out = tr.validation_step_all(batches, b)
        assert tr.val_chains_last == 1 and tr.val_batched_last, (b, tr.val_chains_last)
        for l in range(nl):
            tag = f"batch{b}/level{l}"
            loss, ref = float(out[l]["val_loss"]), float(g[f"{tag}/loss"])
            yhat = out[l]["yhat"].cpu().numpy()
            err = rel_l2(yhat, g[f"{tag}/softmax"])
            print(f"{tag}: val_loss {loss:.7f} reference {ref:.7f} rel {abs(loss - ref) / abs(ref):.2e}; yhat rel-L2 {err:.2e}")
            assert abs(loss - ref) <= 1e-4 * abs(ref), tag
            assert err < 1e-5, tag
            assert set(out[l]) == {"individual", "yhat", "label", "val_loss"}
            keep = g[f"{tag}/gap"] >= c["min_gap"]
            top1 = tr.val_top_idx[l][:, 0].cpu().numpy()
            assert np.array_equal(top1[keep], np.argmax(g[f"{tag}/softmax"], axis=1)[keep]), tag
            y = batches[l][2].cpu().numpy()
            np.add.at(excl_conf[l], (y[~keep], top1[~keep]), 1)
            excluded[l] += (~keep).sum()
    res = tr.validation_epoch_end()
    sizes = np.array(c["batches"], np.float64)
    for l in range(nl):
        assert excluded[l] <= c["max_excluded"] * sizes.sum()
        ref = float((np.array([float(g[f"batch{b}/level{l}/loss"]) for b in range(nb)]) * sizes).sum() / sizes.sum())
        print(f"level {l}: epoch val_loss {res[l]['val_loss']:.7f} reference {ref:.7f}")
        assert abs(res[l]["val_loss"] - ref) <= 1e-4 * abs(ref)
        assert res[l]["rows"] == int(sizes.sum())
        assert np.array_equal(res[l]["confusion"] - excl_conf[l], g[f"level{l}/confusion"]), l
        if excluded[l] == 0:
            assert int(np.trace(res[l]["confusion"])) == int(g[f"level{l}/counts"][1])
    for m in models:
        assert m.training and all(net.training for net in m.year_models)       # the flags were left alone


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_validation_step_all_equals_level_by_level(prec):
    """The same epoch through today's validation_step, level by level with the models in eval(): val_loss and yhat agree
    within 1e-5 relative (fp32) / 2e-3 (bf16); parameters and BatchNorm buffers are bit-identical before and after the call."""
    from deeptreeattention_amd.engine import MultiStageTrainer
    c = R.VALIDATION
    models, ws = _fixture_levels(prec, training=False)
    tr = MultiStageTrainer(models, [1e-3] * 3, ws)
    tol = 1e-5 if prec == "fp32" else 2e-3
    nl = len(c["classes"])
    for b in range(len(c["batches"])):
        batches = [_fixture_batch(b, l) for l in range(nl)]
        before = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models]
        new = tr.validation_step_all(batches, b)
        torch.cuda.synchronize()
        for m, sd in zip(models, before):
            for k, v in m.state_dict().items():
                assert torch.equal(v, sd[k]), k
        for l in range(nl):
            old = tr.validation_step(batches[l], b, l)
            a, r = float(new[l]["val_loss"]), float(old["val_loss"])
            err = rel_l2(new[l]["yhat"].cpu().numpy(), old["yhat"].cpu().numpy())
            print(f"{prec} batch {b} level {l}: val_loss {a:.7f} level-by-level {r:.7f}; yhat rel-L2 {err:.2e}")
            assert abs(a - r) <= tol * abs(r), (b, l)
            assert err < tol, (b, l)


def _random_levels(classes, years, bands, prec, seed=5):
    from deeptreeattention_amd.year import learned_ensemble
    torch.manual_seed(seed)
    ms = []
    for k in classes:
        m = learned_ensemble(years, k, {"pretrain_state_dict": None, "bands": bands}).to(dev()).eval()
        for net in m.year_models:
            net.precision = prec
        ms.append(m)
    return ms


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_counts_are_self_consistent_and_reproducible_at_bench_size(prec):
    """369 bands, 5 levels x 3 years, B = 128, two batches, top_k = 2: the device confusion matrix, top-1 and top-k counts equal
    NumPy counts taken from the call's OWN top_idx / yhat exactly, rows = rows fed, and a second identical run gives
    bit-identical accumulators and losses."""
    from deeptreeattention_amd.engine import MultiStageTrainer
    classes = [2, 2, 12, 7, 5]
    tr = MultiStageTrainer(_random_levels(classes, 3, 369, prec), [1e-4] * 5)
    torch.manual_seed(6)
    epoch = [[(None, {"HSI": [torch.rand(128, 369, 11, 11, device=dev()) for _ in range(3)]}, torch.randint(0, k, (128,), device=dev()))
              for k in classes] for _ in range(2)]
    runs = []
    for run in range(2):
        conf = [np.zeros((k, k), np.int64) for k in classes]
        top1, topk, losses = np.zeros(5, np.int64), np.zeros(5, np.int64), []
        for b, batches in enumerate(epoch):
            out = tr.validation_step_all(batches, b, None, 2)
            assert tr.val_chains_last == 1
            for l in range(5):
                y = batches[l][2].cpu().numpy()
                ti = tr.val_top_idx[l].cpu().numpy()
                pr = out[l]["yhat"].cpu().numpy()
                assert np.isfinite(pr).all()
                assert np.array_equal(ti[:, 0], np.argmax(pr, axis=1))         # top_idx is the argmax of the call's own yhat
                np.add.at(conf[l], (y, ti[:, 0]), 1)
                top1[l] += (ti[:, 0] == y).sum()
                topk[l] += _rank_hits(pr, y, 2).sum()
                losses.append(float(out[l]["val_loss"]))
        raw = tr._val_acc.flat.clone()
        res = tr.validation_epoch_end()
        for l in range(5):
            assert res[l]["rows"] == 256
            assert np.array_equal(res[l]["confusion"], conf[l]), l
            assert round(res[l]["micro"] * 256) == top1[l] and int(np.trace(res[l]["confusion"])) == top1[l]
            assert round(res[l]["top_k"] * 256) == topk[l], (l, res[l]["top_k"] * 256, topk[l])
            assert np.isfinite(res[l]["val_loss"])
        runs.append((raw, losses))
        assert int(tr._val_acc.flat.abs().sum()) == 0           # reset: the next epoch starts from zero
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]


def test_twenty_networks_run_as_two_chains_and_wrong_year_counts_are_refused():
    """5 levels x 4 years = 20 networks: more than one grouped launch takes (DTA_MAX_YEARS = 16), cut on a level boundary into
    two chains, not five; results equal the level-by-level validation_step.  Levels whose batch sizes differ run as chains of
    their own and an exhausted level (None) is skipped.  A wrong year count raises ValueError before anything is launched."""
    from deeptreeattention_amd.engine import MultiStageTrainer
    classes = [2, 3, 12, 7, 5]
    tr = MultiStageTrainer(_random_levels(classes, 4, 16, "fp32", seed=8), [1e-4] * 5)
    torch.manual_seed(9)

    def batch(k, B, years=4):
        return (None, {"HSI": [torch.rand(B, 16, 11, 11, device=dev()) for _ in range(years)]}, torch.randint(0, k, (B,), device=dev()))
    batches = [batch(k, 16) for k in classes]
    new = tr.validation_step_all(batches, 0)
    assert tr.val_chains_last == 2 and not tr.val_batched_last
    for l in range(5):
        old = tr.validation_step(batches[l], 0, l)
        a, r = float(new[l]["val_loss"]), float(old["val_loss"])
        assert abs(a - r) <= 1e-5 * abs(r), l
        assert rel_l2(new[l]["yhat"].cpu().numpy(), old["yhat"].cpu().numpy()) < 1e-5, l
    res = tr.validation_epoch_end()
    assert [r["rows"] for r in res] == [16] * 5
    # a short batch in two levels, one level exhausted: two chains (16 rows: levels 0 and 3; 6 rows: levels 1 and 4)
    mixed = [batch(2, 16), batch(3, 6), None, batch(7, 16), batch(5, 6)]
    out = tr.validation_step_all(mixed, 1)
    assert tr.val_chains_last == 2 and out[2] is None
    for l in (0, 1, 3, 4):
        old = tr.validation_step(mixed[l], 1, l)
        assert abs(float(out[l]["val_loss"]) - float(old["val_loss"])) <= 1e-5 * abs(float(old["val_loss"])), l
    res = tr.validation_epoch_end()
    assert [r["rows"] for r in res] == [16, 6, 0, 16, 6] and np.isnan(res[2]["val_loss"])
    bad = list(batches)
    bad[3] = batch(7, 16, years=3)
    with pytest.raises(ValueError, match="one image tensor per year"):
        tr.validation_step_all(bad, 2)
    torch.cuda.synchronize()
    assert int(tr._val_acc.flat.abs().sum()) == 0               # nothing was launched: no level of the call counted
    with pytest.raises(ValueError, match="top_k"):
        tr.validation_step_all(batches, 2, None, 9)
    assert int(tr._val_acc.flat.abs().sum()) == 0


@pytest.mark.parametrize("classes", [2, 7, 200, 201])
@pytest.mark.parametrize("top_k", [1, 2, 5])
def test_eval_metrics_against_torch_on_the_cpu(classes, top_k):
    """dta_eval_metrics on random scores (67 rows; one label outside the class range -- torch's ignore_index, -100 --; in a
    second call one row of NaN scores as well) against F.cross_entropy, torch.softmax and torch.topk on the CPU: loss within
    1e-5 relative (NaN where torch's is NaN), softmax rel-L2 < 1e-5, confusion and counts exact, accumulated over both calls."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.engine import EvalAccumulators
    L = _lib.lib()
    B = 67
    g = torch.Generator().manual_seed(1000 * classes + top_k)
    acc = EvalAccumulators([classes], dev())
    w = (0.25 + torch.rand(classes, generator=g)) if classes != 7 else None
    conf = np.zeros((classes, classes), np.int64)
    exp = np.zeros(4, np.int64)
    loss_acc = np.zeros(2)
    for call in range(2):
        s = 3.0 * torch.randn(B, classes, generator=g)
        y = torch.randint(0, classes, (B,), generator=g)
        y[5] = -100
        if call == 1:
            s[11] = float("nan")
        ref_loss = torch.nn.functional.cross_entropy(s, y, weight=w)
        ref_p = torch.softmax(s, dim=1)
        k = min(top_k, classes)
        ref_top = torch.topk(ref_p, k, dim=1).indices.numpy()
        sd, yd = s.to(dev()), y.to(dev())
        wd = w.to(dev()) if w is not None else None
        probs = torch.empty(B, classes, device=dev())
        ti = torch.empty(B, 2, dtype=torch.int64, device=dev())
        ts = torch.empty(B, 2, device=dev())
        loss = torch.empty((), device=dev())
        scratch = torch.zeros(B + 2, device=dev())
        ev = acc.level(0, probs, ti, ts, top_k)
        _lib.check(L.dta_eval_metrics(_lib.ptr(sd), _lib.ptr(yd), _lib.ptr(wd), B, classes, _lib.ptr(loss), _lib.ptr(scratch),
                                      C.byref(ev), _lib.current_stream_ptr()), "dta_eval_metrics")
        torch.cuda.synchronize()
        assert float(scratch[B + 1]) == 0.0                      # the block counter is left zero
        valid = (y.numpy() >= 0) & ~np.isnan(s.numpy()).any(1)
        if call == 0:
            assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)), (float(loss), float(ref_loss))
        else:
            assert np.isnan(float(loss)) and np.isnan(float(ref_loss))
        rows = np.where(~np.isnan(s.numpy()).any(1))[0]
        assert rel_l2(probs.cpu().numpy()[rows], ref_p.numpy()[rows]) < 1e-5
        tin = ti.cpu().numpy()
        assert np.array_equal(tin[rows, 0], ref_top[rows, 0])
        assert (tin[11] == -1).all() if call == 1 else True
        yn = y.numpy()
        np.add.at(conf, (yn[valid], ref_top[valid, 0]), 1)
        exp += (valid.sum(), (ref_top[valid, 0] == yn[valid]).sum(), (ref_top[valid] == yn[valid, None]).any(1).sum(), 1)
        loss_acc += (float(loss) * B, B)
    host = acc.flat.cpu().numpy()
    assert np.array_equal(host[:classes * classes].reshape(classes, classes), conf)
    assert np.array_equal(host[classes * classes:classes * classes + 4], exp), (host[classes * classes:classes * classes + 4], exp)
    got = host[classes * classes + 4:].view(np.float64)
    assert got[1] == 2 * B and np.isnan(got[0]) and np.isnan(loss_acc[0])
    res = acc.read()[0]
    assert res["rows"] == exp[0] and res["top_k"] == pytest.approx(exp[2] / exp[0])


def test_fit_and_fit_multistage_with_metrics():
    """fit(..., metrics=True) on Hang2020 and fit_multistage(..., metrics=True): the records carry val_metrics, micro equals
    trace / rows of the returned confusion matrix, val_loss is the size-weighted one; with metrics=False the record keys are
    exactly today's."""
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd.engine import FusedTrainer, MultiStageTrainer
    from deeptreeattention_amd.loop import SyntheticTreeDataset, fit, fit_multistage, validate
    from deeptreeattention_amd.year import learned_ensemble
    torch.manual_seed(2)
    m = H.Hang2020(bands=12, classes=4).to(dev()).train()
    tr = FusedTrainer(m, lr=1e-3)
    train = SyntheticTreeDataset(32, bands=12, classes=4, seed=3)
    val = SyntheticTreeDataset(22, bands=12, classes=4, seed=4)          # batches of 8, 8 and 6
    plain = fit(tr, train, val, epochs=1, batch_size=8)
    assert set(plain[0]) == {"epoch", "train_loss", "val_loss", "lr"}
    hist = fit(tr, train, val, epochs=2, batch_size=8, metrics=True)
    for rec in hist:
        assert set(rec) == {"epoch", "train_loss", "val_loss", "lr", "val_metrics"}
        vm = rec["val_metrics"]
        assert vm["rows"] == 22 and int(vm["confusion"].sum()) == 22
        assert vm["micro"] == pytest.approx(np.trace(vm["confusion"]) / vm["rows"])
        assert rec["val_loss"] == vm["val_loss"] and np.isfinite(rec["val_loss"])
    assert m.training
    # the size-weighted loss against the batch losses of today's validation_step
    m.eval()
    ls = [(float(tr.validation_step(b, i)), b[2].shape[0]) for i, b in enumerate(val.loader(8))]
    m.train()
    vm = validate(tr, val, 8, top_k=2)
    assert vm["val_loss"] == pytest.approx(sum(a * n for a, n in ls) / 22, rel=1e-5)
    assert vm["top_k"] >= vm["micro"]

    classes, years, bands = [3, 5], 2, 8
    torch.manual_seed(7)
    models = [learned_ensemble(years, c, {"pretrain_state_dict": None, "bands": bands}).to(dev()).train() for c in classes]
    for mm in models:
        for net in mm.year_models:
            net.precision = "fp32"
    mtr = MultiStageTrainer(models, [2e-3, 2e-3])
    mtrain = [SyntheticTreeDataset(32, bands, c, years=years, seed=1 + i, device=dev()) for i, c in enumerate(classes)]
    mval = [SyntheticTreeDataset(22, bands, classes[0], years=years, seed=5, device=dev()),
            SyntheticTreeDataset(16, bands, classes[1], years=years, missing=0.3, seed=6, device=dev())]
    plain = fit_multistage(mtr, mtrain, mval, epochs=1, batch_size=8, shuffle=False)
    assert set(plain[0]) == {"epoch", "train_loss", "val_loss", "lr"}
    hist = fit_multistage(mtr, mtrain, mval, epochs=1, batch_size=8, shuffle=False, metrics=True)
    rec = hist[0]
    assert set(rec) == {"epoch", "train_loss", "val_loss", "lr", "val_metrics"}
    assert [v["rows"] for v in rec["val_metrics"]] == [22, 16]
    for l, vm in enumerate(rec["val_metrics"]):
        assert vm["micro"] == pytest.approx(np.trace(vm["confusion"]) / vm["rows"])
        assert rec["val_loss"][l] == vm["val_loss"] and np.isfinite(vm["val_loss"])
    assert all(mm.training for mm in models)
