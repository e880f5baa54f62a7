"""Dense multi-stage prediction on the device: dta_crown_resolve against its host definition (dense.crown_resolve_np),
dta_gather_windows_years against per-year dta_gather_windows + dta_year_flags, and the route
(dense.predict_windows_multistage / predict_map_multistage) against explicitly sliced, preprocessed windows fed to
MultiStagePredictor.ensemble in the same batches.  Every comparison is exact: labels, levels and counts equal, floats
compared as bits (both sides do the same float32 operations in the same order)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_dense_gpu import assert_same_bits, edge_origins, raw_raster, raw_windows
from test_dense_multistage_cpu import CROWN_ROWS, random_probs, three_level_hierarchy
from test_hierarchy_cpu import load_ensemble_fixture
from test_multistage_ensemble_gpu import _small_levels

pytestmark = pytest.mark.gpu

RAW_BANDS, BANDS, H, W = 43, 23, 17, 13       # 23 * 121 floats per window: not a multiple of the 4 a lane writes


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def year_rasters():
    """Three years of raw int16 rasters: year 0 a scene, year 1 missing, year 2 present but constant over the bands of every
    pixel -- it normalises to all zeros, so its flag is 0 although it is there."""
    y0 = raw_raster(31, RAW_BANDS, H, W)
    flat = (np.arange(H * W, dtype=np.int16).reshape(1, H, W) * 7 + 100).repeat(RAW_BANDS, axis=0)
    return [y0, None, np.ascontiguousarray(flat)]


def dense_years(raws):
    from deeptreeattention_amd.dense import DenseRaster
    return [None if r is None else DenseRaster(r, precision="fp32", device=dev()) for r in raws]


def same_np(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype == np.float32:
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
    else:
        assert np.array_equal(got, want), what


def same_crowns(got, want, mean=True, votes=True):
    assert got.label.dtype == torch.int64 and got.level.dtype == torch.int32 and got.count.dtype == torch.int32
    same_np(got.label, want.label, "label"); same_np(got.score, want.score, "score"); same_np(got.level, want.level, "level")
    same_np(got.count, want.count, "count")
    for l in range(len(want.top_idx)):
        same_np(got.top_idx[l], want.top_idx[l], ("top_idx", l)); same_np(got.top_score[l], want.top_score[l], ("top_score", l))
        if mean:
            same_np(got.mean[l], want.mean[l], ("mean", l))
    if not mean:
        assert got.mean is None
    if votes:
        assert got.votes.dtype == torch.int32
        same_np(got.votes, want.votes, "votes")
    else:
        assert got.votes is None


# ---------------------------------------------------------------------------------------------------------------------
# dta_crown_resolve
# ---------------------------------------------------------------------------------------------------------------------
def chain_hierarchy(classes):
    """Class 1 of every level but the last passes on to the next level, every other class ends with a species of its own."""
    from deeptreeattention_amd.hierarchy import Hierarchy
    nxt, sp, s = [], [], 0
    for l, c in enumerate(classes):
        last = l == len(classes) - 1
        nx = [-1 if (last or k != 1) else l + 1 for k in range(c)]
        row = []
        for v in nx:
            row.append(s if v == -1 else -1)
            s += v == -1
        nxt.append(nx); sp.append(row)
    return Hierarchy(nxt, sp, s)


def hierarchies():
    return {"1": chain_hierarchy([4]), "3": three_level_hierarchy(), "8": chain_hierarchy([2, 3, 2, 4, 2, 2, 3, 5]),
            "wide": chain_hierarchy([2, 300])}


@pytest.mark.parametrize("which", ["1", "3", "8", "wide"])
def test_crown_resolve_equals_host_definition_and_reruns_identically(which):
    from deeptreeattention_amd.dense import crown_resolve, crown_resolve_np
    h = hierarchies()[which]
    assert h.levels == {"1": 1, "3": 3, "8": 8, "wide": 2}[which]
    rng = np.random.default_rng(40 + h.levels)
    # the row counts twice over, the first crown starting at row 2: ten crowns, two of them empty
    offsets = 2 + np.concatenate([[0], np.cumsum(CROWN_ROWS + CROWN_ROWS)]).astype(np.int64)
    rows = int(offsets[-1]) + 3
    probs = [random_probs(rng, rows, c) for c in h.classes]
    if which == "wide":
        probs[0][:, 0] = 0.25; probs[0][:, 1] = 0.75         # the 2-class level always passes on to the 300-class one
        probs[1][int(offsets[1]):int(offsets[2]), 280] = 0.9  # the crown of one window: a winner beyond class 256
    if which == "3":
        probs[2][:, 3] = probs[2][:, 1]                       # a tie in every crown's mean: the lower class wins
    win = rng.integers(-2, h.n_species + 1, rows)             # window labels, some outside [0, n_species)
    want = crown_resolve_np(probs, offsets, h, window_labels=win)
    dprobs = [torch.from_numpy(p).to(dev()) for p in probs]
    dwin = torch.from_numpy(win).to(dev())
    got = crown_resolve(dprobs, offsets, h, window_labels=dwin)
    same_crowns(got, want)
    again = crown_resolve(dprobs, offsets, h, window_labels=dwin)
    for a, b in zip([got.label, got.score, got.level, got.count, got.votes] + got.top_idx + got.top_score + got.mean,
                    [again.label, again.score, again.level, again.count, again.votes] + again.top_idx + again.top_score + again.mean):
        assert_same_bits(a, b, "rerun")
    same_crowns(crown_resolve(dprobs, offsets, h), want, votes=False)
    same_crowns(crown_resolve(dprobs, offsets, h, window_labels=dwin, want_mean=False), want, mean=False)
    same_crowns(crown_resolve(dprobs, offsets, h, want_mean=False), want, mean=False, votes=False)
    # the empty crowns, and every level's own outputs are dta_crown_reduce's
    assert want.label[0] == -1 and want.level[0] == 0 and want.score[0] == 0.0 and want.count[0] == 0
    if which == "wide":
        assert int(got.top_idx[1][1, 0]) == 280 and got.level.cpu().tolist() == [0, 1, 1, 1, 1] * 2
    if which == "3":
        assert not (got.top_idx[2][:, 0] == 3).any()
    if which == "8":
        from deeptreeattention_amd.dense import crown_reduce
        for l, p in enumerate(dprobs):
            one = crown_reduce(p, offsets)
            assert_same_bits(one.mean, got.mean[l], l); assert_same_bits(one.top_idx, got.top_idx[l], l)
            assert_same_bits(one.top_score, got.top_score[l], l); assert_same_bits(one.count, got.count, l)
    with pytest.raises(ValueError):
        crown_resolve(dprobs, [0, rows + 1], h)


def test_crown_resolve_one_window_per_crown_is_the_reference_ensemble():
    from deeptreeattention_amd.dense import crown_resolve
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    n = len(fx["names"])
    got = crown_resolve([torch.from_numpy(p).to(dev()) for p in fx["probs"]], np.arange(n + 1), h)
    same_np(got.label, fx["ens_label"], "label"); same_np(got.score, fx["ens_score"], "score")
    same_np(got.level, fx["branch_level"], "level")
    assert sorted(set(got.level.cpu().tolist())) == [0, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------------------------
# dta_gather_windows_years
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [29, 64])
def test_gather_windows_years_equals_per_year_gathers_and_year_flags(n):
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dense import DenseRaster
    L = _lib.lib()
    ras = dense_years(year_rasters())
    assert not ras[2].data.any() and ras[0].bands == BANDS and (BANDS * 121) % 4 != 0
    origins = edge_origins(H, W, seed=5, extra=n - 12)
    assert len(origins) == n
    assert (origins[:, 0] < 0).any() and (origins[:, 1] < 0).any() and (origins[:, 0] + 11 > H).any() and (origins[:, 1] + 11 > W).any()
    o = torch.from_numpy(origins).to(dev())
    banks = [torch.zeros(3, device=dev()) for _ in range(2)]
    st = _lib.current_stream_ptr()

    def separate(rs):
        xs = [torch.zeros(n, BANDS, 11, 11, device=dev()) if r is None else r.windows(o) for r in rs]
        flags = torch.full((3,), 5.0, device=dev())
        ptrs = (C.c_void_p * 3)(*[x.data_ptr() for x in xs])
        _lib.check(L.dta_year_flags(ptrs, 3, xs[0].numel(), _lib.ptr(flags), None, st), "dta_year_flags")
        return xs, flags

    # three calls, the banks alternating: the third finds the first call's flags cleared by the second
    for call, rs in enumerate(([ras[0], None, ras[2]], [ras[2], None, ras[0]], [ras[2], None, ras[0]])):
        want_x, want_f = separate(rs)
        outs = [torch.full((n, BANDS, 11, 11), 7.0, device=dev()) for _ in range(3)]
        flags, nxt = banks[call & 1], banks[(call & 1) ^ 1]
        got_f = DenseRaster.windows_years(rs, o, outs, flags, nxt)
        assert got_f is flags
        assert_same_bits(flags, want_f, ("flags", call))
        assert flags.cpu().tolist() == ([1.0, 0.0, 0.0] if call == 0 else [0.0, 0.0, 1.0])
        assert not nxt.any()
        for y in (0, 2):
            assert_same_bits(outs[y], want_x[y], ("year", y, call))
        assert bool((outs[1] == 7.0).all())                    # a missing year writes nothing
    # clear_next = NULL: the call clears its own flags first
    stale = torch.full((3,), 1.0, device=dev())
    ptr = lambda ts: (C.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in ts])      # noqa: E731
    outs = [torch.empty(n, BANDS, 11, 11, device=dev()) for _ in range(3)]
    _lib.check(L.dta_gather_windows_years(ptr([ras[2].data, None, ras[0].data]), 3, BANDS, H, W, _lib.ptr(o), n, 11, ptr(outs),
                                          _lib.ptr(stale), None, st), "dta_gather_windows_years")
    assert stale.cpu().tolist() == [0.0, 0.0, 1.0]


def test_gather_windows_years_counts_nan_as_non_zero():
    from deeptreeattention_amd.dense import DenseRaster
    ras = dense_years(year_rasters())
    ras[2].data[3, 4, 5] = float("nan")
    o = torch.tensor([[0, 0], [30, 30]], dtype=torch.int32, device=dev())        # the second window lies outside the raster
    outs = [torch.empty(2, BANDS, 11, 11, device=dev()) for _ in range(3)]
    banks = [torch.zeros(3, device=dev()) for _ in range(2)]
    assert DenseRaster.windows_years(ras, o, outs, banks[0], banks[1]).cpu().tolist() == [1.0, 0.0, 1.0]
    assert DenseRaster.windows_years(ras, o[1:], [t[:1] for t in outs], banks[1], banks[0]).cpu().tolist() == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------------------------------------
BOXES = [(0, 0, 8, 7),        # 56 windows
         (2, 1, 6, 6),        # 20 windows: rows 56 .. 75, across the first batch boundary (64)
         (3, 3, 3, 7),        # empty
         (5, 5, 6, 6),        # a single pixel
         (14, 9, 19, 15)]     # hangs over the raster's lower right corner
BATCH = 64


def host_sliced(pred, raws, origins, keep):
    """The definition: every window sliced from the raw rasters on the host, preprocessed by the crop kernel, the same
    batches through MultiStagePredictor.ensemble with the years' flags taken from the batch (present=None)."""
    from deeptreeattention_amd.preprocess import preprocess_batch
    N, nl = len(origins), len(pred.preds)
    out = {"ens": [[], [], []], "top_idx": [[] for _ in range(nl)], "top_score": [[] for _ in range(nl)], "probs": [[] for _ in range(nl)]}
    for n0 in range(0, N, BATCH):
        ob = origins[n0:n0 + BATCH]
        xs = [torch.zeros(len(ob), BANDS, 11, 11, device=dev()) if r is None else preprocess_batch(raw_windows(r, ob), 11, device=dev())
              for r in raws]
        e = pred.ensemble(xs, present=keep)
        for k in range(3):
            out["ens"][k].append(e[k].clone())
        for l in range(nl):
            out["top_idx"][l].append(pred.top_idx[l].clone()); out["top_score"][l].append(pred.top_score[l].clone())
            out["probs"][l].append(pred.probs[l].clone())
    cat = lambda ts: torch.cat(ts, 0)      # noqa: E731
    return {"ens": [cat(t) for t in out["ens"]], "top_idx": [cat(t) for t in out["top_idx"]],
            "top_score": [cat(t) for t in out["top_score"]], "probs": [cat(t) for t in out["probs"]]}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_route_equals_host_sliced_windows_through_the_ensemble(prec):
    from deeptreeattention_amd.dense import crown_resolve_np, predict_windows_multistage, window_origins
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS, prec=prec)
    raws = year_rasters()
    origins, offsets = window_origins(BOXES, anchor="center")
    N = len(origins)
    assert N == 107 and N % BATCH != 0 and offsets.tolist() == [0, 56, 76, 76, 77, 107]
    res = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws), origins, crown_offsets=offsets,
                                     batch_size=BATCH, return_probs=True)
    ref_pred = MultiStagePredictor(models, hierarchy=h)
    want = host_sliced(ref_pred, raws, origins, None)
    for k, name in enumerate(("ens_label", "ens_score", "ens_level")):
        assert_same_bits(getattr(res, name), want["ens"][k], name)
    assert res.ens_label.dtype == torch.int64 and res.ens_score.dtype == torch.float32 and res.ens_level.dtype == torch.int32
    for l in range(3):
        assert_same_bits(res.top_idx[l], want["top_idx"][l], l); assert_same_bits(res.top_score[l], want["top_score"][l], l)
        assert_same_bits(res.probs[l], want["probs"][l], l)
    crowns = crown_resolve_np([p.cpu().numpy() for p in want["probs"]], offsets, h, window_labels=want["ens"][0].cpu().numpy())
    same_crowns(res.crowns, crowns)
    assert res.crowns.count.cpu().tolist() == [56, 20, 0, 1, 30] and int(res.crowns.label[2]) == -1
    assert int(res.crowns.votes.sum()) == N and int(res.ens_label.min()) >= 0
    # year 2 is there but all zero after normalising: both legs leave it (and the missing year 1) out of every level's mean
    # (had they taken part, as zeros through a network, the probabilities would be other ones ...
    all3 = host_sliced(MultiStagePredictor(models, hierarchy=h), raws, origins, [True, True, True])
    assert not torch.equal(all3["probs"][2], res.probs[2])
    # ... and nothing of their networks reaches the result: other weights in years 1 and 2, the same bits)
    with torch.no_grad():
        for m in models:
            for y in (1, 2):
                for p in m.year_models[y].parameters():
                    p.mul_(-1.5)
    for leg in (predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws), origins, batch_size=BATCH,
                                           return_probs=True).probs,
                host_sliced(MultiStagePredictor(models, hierarchy=h), raws, origins, None)["probs"]):
        for l in range(3):
            assert_same_bits(leg[l], res.probs[l], ("years 1 and 2 left out", l))
    assert not torch.equal(host_sliced(MultiStagePredictor(models, hierarchy=h), raws, origins, [True, True, True])["probs"][2], all3["probs"][2])
    # without probabilities and crowns: the same per-window outputs
    lean = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws), origins, batch_size=BATCH)
    assert lean.probs is None and lean.crowns is None
    assert_same_bits(lean.ens_label, res.ens_label, "lean"); assert_same_bits(lean.ens_score, res.ens_score, "lean")
    assert_same_bits(lean.top_idx[2], res.top_idx[2], "lean")


def test_predict_map_multistage_is_predict_windows_over_all_pixels():
    from deeptreeattention_amd.dense import predict_map_multistage, predict_windows_multistage, window_origins
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)          # (the predictor holds its models weakly)
    pred = MultiStagePredictor(models, hierarchy=h)
    raws = year_rasters()
    for rows, cols in ((None, None), ((3, 12), (2, 9))):
        r0, r1 = rows or (0, H)
        c0, c1 = cols or (0, W)
        origins, _ = window_origins([(r0, c0, r1, c1)], anchor="center")
        want = predict_windows_multistage(pred, dense_years(raws), origins, batch_size=BATCH)
        want = [t.clone() for t in (want.ens_label, want.ens_score, want.ens_level)]
        species, score, level = predict_map_multistage(pred, raws, rows=rows, cols=cols, batch_size=BATCH)
        assert tuple(species.shape) == tuple(score.shape) == tuple(level.shape) == (r1 - r0, c1 - c0)
        assert species.dtype == torch.int64 and score.dtype == torch.float32 and level.dtype == torch.int32
        assert_same_bits(species.reshape(-1), want[0], rows); assert_same_bits(score.reshape(-1), want[1], rows)
        assert_same_bits(level.reshape(-1), want[2], rows)


def test_route_refuses_before_any_launch(monkeypatch):
    from deeptreeattention_amd import _lib, dense
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)
    raws = year_rasters()
    ras = dense_years(raws)
    bf16 = dense.DenseRaster(raws[0], precision="bf16", device=dev())
    origins = np.zeros((4, 2), np.int32)
    pred = MultiStagePredictor(models, hierarchy=h)
    bare = MultiStagePredictor(models)
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_launch)
    monkeypatch.setattr(_lib, "current_stream_ptr", no_launch)
    with pytest.raises(ValueError, match="rasters"):
        dense.predict_windows_multistage(pred, ras[:2], origins)
    with pytest.raises(RuntimeError, match="hierarchy"):
        dense.predict_windows_multistage(bare, ras, origins)
    with pytest.raises(RuntimeError, match="fp32"):
        dense.predict_windows_multistage(pred, [bf16, None, None], origins)
    with pytest.raises(ValueError, match="present"):
        dense.predict_windows_multistage(pred, [None, None, None], origins)
    with pytest.raises(ValueError, match="present"):
        dense.predict_map_multistage(pred, [None, None, None])
    with pytest.raises(ValueError, match="crown_offsets"):
        dense.predict_windows_multistage(pred, ras, origins, crown_offsets=[0, 9])


def test_more_networks_than_one_chain_are_refused():
    from deeptreeattention_amd import dense
    from deeptreeattention_amd.engine import MultiStagePredictor
    from deeptreeattention_amd.hierarchy import Hierarchy
    fx = load_ensemble_fixture()
    h = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    models = _small_levels(h.classes, 4, bands=BANDS)          # 5 levels x 4 years = 20 networks
    pred = MultiStagePredictor(models, hierarchy=h)
    with pytest.raises(RuntimeError, match="one chain"):
        dense.predict_windows_multistage(pred, [None] * 4, np.zeros((1, 2), np.int32))


def test_year_flags_keyword_equals_flags_decided_by_the_call():
    """On explicit crops: ensemble(year_flags=dta_year_flags' own output) gives the bits of ensemble(present=None)."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3)
    g = torch.Generator(device=dev())
    g.manual_seed(2)
    xs = [torch.rand(9, 12, 11, 11, device=dev(), generator=g) for _ in range(3)]
    xs[1][:] = 0
    a = MultiStagePredictor(models, hierarchy=h)
    want = [t.clone() for t in a.ensemble(xs)]
    want_levels = [[t.clone() for t in lv] for lv in a.per_level()]
    flags = torch.zeros(3, device=dev())
    ptrs = (C.c_void_p * 3)(*[x.data_ptr() for x in xs])
    _lib.check(_lib.lib().dta_year_flags(ptrs, 3, xs[0].numel(), _lib.ptr(flags), None, _lib.current_stream_ptr()), "dta_year_flags")
    assert flags.cpu().tolist() == [1.0, 0.0, 1.0]
    b = MultiStagePredictor(models, hierarchy=h)
    got = b.ensemble(xs, year_flags=flags)
    for u, v in zip(got, want):
        assert_same_bits(u, v, "ens")
    for lv_got, lv_want in zip(b.per_level(), want_levels):
        for u, v in zip(lv_got, lv_want):
            assert_same_bits(u, v, "level")
    for u, v in zip(b(xs, year_flags=flags), want_levels):
        assert_same_bits(u[0], v[0], "call")
    with pytest.raises(ValueError):
        b.ensemble(xs, present=[True, False, True], year_flags=flags)
    with pytest.raises(ValueError):
        b.ensemble(xs, year_flags=flags[:2])
