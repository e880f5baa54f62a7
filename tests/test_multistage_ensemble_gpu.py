"""The hierarchical ensemble label on the device (reference multi_stage.py:368-434, `gather_predictions` + `ensemble`):
the walk alone (dta_hierarchy_resolve) against the reference's own output, the walk inside the one-chain epilogue
(dta_multistage_predict_ensemble) against `Hierarchy.resolve_np` on the same call's per-level outputs -- which stay, bit for
bit, those of dta_multistage_predict --, the per-level route for more networks than one chain takes, the confusion count,
and the prediction loop."""
import numpy as np
import pytest
import torch

from test_hierarchy_cpu import load_ensemble_fixture
from test_multistage_gpu import _batch, _levels

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _np_walk(h, top_idx, top_score):
    return h.resolve_np([t[:, 0].cpu().numpy() for t in top_idx], [t[:, 0].cpu().numpy() for t in top_score])


def _same(got, want):
    """(ens_label, ens_score, ens_level) on the device against resolve_np's: labels and levels exactly, scores bit for bit."""
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2].cpu().numpy(), want[2])


def _small_levels(classes, years, bands=12, prec=None, seed=5):
    from deeptreeattention_amd.year import learned_ensemble
    torch.manual_seed(seed)
    models = [learned_ensemble(years, c, {"pretrain_state_dict": None, "bands": bands}).to(dev()).eval() for c in classes]
    if prec:
        for m in models:
            for net in m.year_models:
                net.precision = prec
    return models


def _count(labels, preds, n):
    conf = np.zeros((n, n), np.int64)
    ok = (labels >= 0) & (labels < n) & (preds >= 0) & (preds < n)
    np.add.at(conf, (labels[ok], preds[ok]), 1)
    return conf


def test_hierarchy_resolve_equals_the_reference_ensemble():
    """dta_hierarchy_resolve on the fixture's per-level top-2 (torch.topk of the fixture's probabilities): the reference's
    labels exactly, its scores bit for bit, every terminal branch taken; and the confusion count of the same launch."""
    from deeptreeattention_amd.engine import resolve_hierarchy
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    top = [torch.topk(torch.from_numpy(p).to(dev()), 2, dim=1) for p in fx["probs"]]
    ti, ts = [t.indices.contiguous() for t in top], [t.values.contiguous() for t in top]
    got = resolve_hierarchy(h, ti, ts)
    _same(got, (fx["ens_label"], fx["ens_score"], fx["branch_level"]))
    assert sorted(set(fx["branch_level"].tolist())) == [0, 2, 3, 4]
    rng = np.random.default_rng(3)
    y = rng.integers(-2, h.n_species + 2, len(fx["names"]))
    conf = torch.zeros(h.n_species, h.n_species, dtype=torch.int64, device=dev())
    again = resolve_hierarchy(h, ti, ts, torch.from_numpy(y), conf, out=got)
    assert again[0] is got[0]
    _same(again, (fx["ens_label"], fx["ens_score"], fx["branch_level"]))
    assert np.array_equal(conf.cpu().numpy(), _count(y, fx["ens_label"], h.n_species))
    assert int(conf.sum()) == int(((y >= 0) & (y < h.n_species)).sum()) < len(y)


@pytest.mark.parametrize("use_present", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_chain_ensemble_equals_the_walk_on_its_own_levels(prec, use_present):
    """On the two trained levels of test_multistage_gpu (one year of the batch all-zero): predictor.ensemble(images) is
    resolve_np of the same call's top_idx / top_score, and those per-level outputs are bit-identical to a predictor
    without a hierarchy; live and frozen weights; two hierarchies that between them send every crop down both branches."""
    from deeptreeattention_amd.engine import MultiStagePredictor, MultiStageTrainer
    from deeptreeattention_amd.hierarchy import Hierarchy
    from oracle.recipes import MULTISTAGE
    models, ws = _levels(prec)
    driver = MultiStageTrainer(models, list(MULTISTAGE["lrs"]), ws)
    for step in range(2):
        b, pr = _batch(step)
        driver.training_step_all(b, step, pr)
    batch, present = _batch(1)                     # level 1's inputs of step 1 have year 2 zeroed
    images = batch[1][1]["HSI"]
    pres = present[1] if use_present else None
    for m in models:
        m.eval()
    c0, c1 = MULTISTAGE["classes"]
    n_species = c0 + c1
    first_ends = Hierarchy([[-1] + [1] * (c0 - 1), [-1] * c1], [[0] + [-1] * (c0 - 1), list(range(c0, c0 + c1))], n_species)
    first_goes_on = Hierarchy([[1] + [-1] * (c0 - 1), [-1] * c1], [[-1] + list(range(1, c0)), list(range(c0, c0 + c1))], n_species)
    plain = [tuple(t.clone() for t in o) for o in MultiStagePredictor(models)(images, True, pres)]
    levels_seen = set()
    for h in (first_ends, first_goes_on):
        for frozen in (False, True):
            pred = MultiStagePredictor(models, frozen=frozen, hierarchy=h)
            for call in range(2 if frozen else 1):          # frozen: the second call reuses the packed weights
                ens = pred.ensemble(images, pres)
                _same(ens, _np_walk(h, pred.top_idx, pred.top_score))
                for l, want in enumerate(plain):
                    got = pred.per_level()[l]
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (l, frozen, call)
            assert pred._packed
            levels_seen |= set(ens[2].cpu().tolist())
            # __call__ is what it was, on the same object
            for got, want in zip(pred(images, True, pres), plain):
                assert all(torch.equal(u, v) for u, v in zip(got, want))
    assert levels_seen == {0, 1}
    assert int(ens[0].min()) >= 0 and int(ens[0].max()) < n_species


def test_a_level_wider_than_256_classes_as_terminal_level():
    """The re-formed tail of the epilogue (classes beyond the 256 a row keeps in registers) in the ensemble kernel: a
    300-class terminal level behind a 2-class level that always passes on; one empty year."""
    from deeptreeattention_amd.engine import MultiStagePredictor, Predictor
    from deeptreeattention_amd.hierarchy import Hierarchy
    models = _small_levels((2, 300), 2)
    xs = [torch.rand(9, 12, 11, 11, device=dev()) for _ in range(2)]
    xs[1][:] = 0
    h = Hierarchy([[1, 1], [-1] * 300], [[-1, -1], list(range(300))], 300)
    pred = MultiStagePredictor(models, hierarchy=h)
    ens = pred.ensemble(xs)
    _same(ens, _np_walk(h, pred.top_idx, pred.top_score))
    assert ens[2].cpu().tolist() == [1] * 9
    assert torch.equal(ens[0], pred.top_idx[1][:, 0]) and torch.equal(ens[1], pred.top_score[1][:, 0])
    for l, m in enumerate(models):
        probs, ti, ts = Predictor(m)(xs, True, None)
        assert torch.equal(pred.probs[l], probs) and torch.equal(pred.top_idx[l], ti) and torch.equal(pred.top_score[l], ts), l


def test_more_networks_than_one_chain_takes_the_per_level_route():
    """The reference's 5 levels x 4 years are 20 networks, more than one chain's 16: predict_ensemble runs the per-level
    predictors and then the walk alone, and gives what resolve_np gives on those predictors' outputs."""
    from deeptreeattention_amd.engine import MultiStageTrainer, Predictor
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    models = _small_levels(h.classes, 4)
    tr = MultiStageTrainer(models, [1e-3] * 5, hierarchy=h)
    xs = [torch.rand(24, 12, 11, 11, device=dev()) for _ in range(4)]
    xs[2][:] = 0
    names = ["crown_{}".format(i) for i in range(24)]
    y = torch.arange(24, device=dev()) % (h.n_species + 1)            # label 9 is out of range: skipped
    ids, label, score, level = tr.predict_ensemble((names, {"HSI": xs}), 0, None, y)
    assert not tr._ms_predictor.supported(4) and ids == names
    outs = [Predictor(m)(xs, False, None) for m in models]
    want = _np_walk(h, [o[1] for o in outs], [o[2] for o in outs])
    _same((label, score, level), want)
    assert np.array_equal(tr.confusion.cpu().numpy(), _count(y.cpu().numpy(), want[0], h.n_species))
    # three years fit one chain: the same trainer method then runs it
    models3 = _small_levels(h.classes, 3)
    tr3 = MultiStageTrainer(models3, [1e-3] * 5, hierarchy=h)
    out3 = tr3.predict_ensemble((names, {"HSI": xs[:3]}))
    assert tr3._ms_predictor.supported(3) and tr3._ms_predictor._ens is not None
    _same(out3[1:], _np_walk(h, tr3._ms_predictor.top_idx, tr3._ms_predictor.top_score))
    with pytest.raises(RuntimeError, match="hierarchy"):
        MultiStageTrainer(models3, [1e-3] * 5).predict_ensemble((names, {"HSI": xs[:3]}))


def test_confusion_accumulates_on_the_device():
    """Two batches counted by the ensemble launch itself equal the NumPy count over both, exactly; labels outside
    [0, n_species) are skipped; a second run from a zeroed matrix gives identical bits."""
    from deeptreeattention_amd.engine import MultiStagePredictor
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    models = _small_levels(h.classes, 3, prec="bf16")
    pred = MultiStagePredictor(models, frozen=True, hierarchy=h)
    g = torch.Generator(device=dev())
    g.manual_seed(9)
    batches = [[torch.rand(40, 12, 11, 11, device=dev(), generator=g) for _ in range(3)] for _ in range(2)]
    rng = np.random.default_rng(11)
    ys = [rng.integers(-1, h.n_species + 1, 40) for _ in range(2)]
    runs = []
    for run in range(2):
        if pred.confusion is not None:
            pred.confusion.zero_()
        labels, preds = [], []
        for xs, y in zip(batches, ys):
            ens = pred.ensemble(xs, None, torch.from_numpy(y))
            labels.append(y)
            preds.append(ens[0].cpu().numpy())
        want = _count(np.concatenate(labels), np.concatenate(preds), h.n_species)
        got = pred.confusion.cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, want)
        skipped = sum(int(((y < 0) | (y >= h.n_species)).sum()) for y in ys)
        assert skipped > 0 and got.sum() == 80 - skipped
        runs.append((got, np.concatenate(preds)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # without labels nothing is counted
    before = pred.confusion.clone()
    pred.ensemble(batches[0])
    assert torch.equal(pred.confusion, before)


def test_predict_multistage_loop_returns_one_row_per_crop_in_order():
    """loop.predict_multistage over a SyntheticTreeDataset whose last batch is ragged (40 crops in batches of 16): one row
    per crop, in the dataset's order, equal to the predictor run on the same slices; the run's confusion matrix and the
    evaluation figures from it."""
    from deeptreeattention_amd.engine import MultiStagePredictor, MultiStageTrainer
    from deeptreeattention_amd.hierarchy import Hierarchy, scores_from_confusion
    from deeptreeattention_amd.loop import SyntheticTreeDataset, predict_multistage
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    models = _small_levels(h.classes, 3)
    tr = MultiStageTrainer(models, [1e-3] * 5, hierarchy=h)
    data = SyntheticTreeDataset(40, 12, h.n_species, years=3, missing=0.3, seed=4, device=dev())
    res = predict_multistage(tr, data, batch_size=16, labels=True)
    assert res["individual"].tolist() == data.individuals
    assert res["ens_label"].shape == res["ens_score"].shape == res["ens_level"].shape == (40,)
    assert res["ens_label"].dtype == np.int64 and res["ens_score"].dtype == np.float32 and res["ens_level"].dtype == np.int32
    pred = MultiStagePredictor(models, hierarchy=h)
    for lo in range(0, 40, 16):
        ens = pred.ensemble([t[lo:lo + 16] for t in data.hsi])
        _same(ens, (res["ens_label"][lo:lo + 16], res["ens_score"][lo:lo + 16], res["ens_level"][lo:lo + 16]))
    y = data.labels.cpu().numpy()
    assert np.array_equal(res["confusion"], _count(y, res["ens_label"], h.n_species)) and res["confusion"].sum() == 40
    s = scores_from_confusion(res["confusion"])
    assert s["micro"] == (y == res["ens_label"]).mean()
    plain = predict_multistage(tr, data, batch_size=16)
    assert "confusion" not in plain and np.array_equal(plain["ens_label"], res["ens_label"])
    assert tr.confusion is None
