"""The first conv once per year raster for the multi-stage route, on the device
(dense.predict_windows_multistage(share_conv1=True); csrc/dense_conv1.hip): the years' tables against the host definition
and against the single-network table bit for bit, the levels x years gather as a bit-exact copy with the years' flags, the
fp32 and bf16 routes end to end against the float64 oracle (route_case of tests/test_dense_multistage_conv1_cpu.py, built
once), skipped years, reruns, frozen weights, maps, crowns, weight updates and refusals.  All fixtures are synthetic."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O
from test_dense_conv1_gpu import FP32_TIGHT, HALF_TABLE, raw_raster
from test_dense_gpu import assert_same_bits, edge_origins
from test_dense_multistage_conv1_cpu import ROUTE_BANDS, ROUTE_CLASSES, route_case
from test_dense_multistage_cpu import three_level_hierarchy
from test_dense_multistage_gpu import BANDS, H, W, same_crowns, year_rasters
from test_multistage_ensemble_gpu import _small_levels

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def dense_years(raws, precision):
    from deeptreeattention_amd.dense import DenseRaster
    return [None if r is None else DenseRaster(r, precision=precision, device=dev()) for r in raws]


def first_conv(net):
    c = net.conv1.conv_layer
    return c.weight.detach().cpu().numpy(), c.bias.detach().cpu().numpy()


def bits_of(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("h,w,bands", [(6, 5, 20), (17, 13, 20), (6, 5, 349)])
def test_years_table_equals_the_host_definition_and_the_single_network_table(h, w, bands, levels, precision):
    """Two years, the second missing.  fp32: rel-L2 <= 2e-4 against conv1_table_np (float64) on the levels' concatenated
    first convs; bf16: the definition on DenseRaster.float() and bf16-rounded weights, <= 1e-3 -- whole table, interior and
    ring, the bounds of tests/test_dense_conv1_gpu.py.  Every 32-column slice has the bits of DenseRaster.conv1_table of that
    level's network alone (the same kernels on independent columns); the mask equals conv1_mask_np; the missing year's table
    is the bias row and its mask one zero byte."""
    from deeptreeattention_amd.dense import Conv1TableYears, DenseRaster, conv1_mask_np, conv1_table_np
    from deeptreeattention_amd.engine import MultiStagePredictor, Predictor
    models = _small_levels([2 + l for l in range(levels)], 2, bands=bands, prec=precision, seed=11)
    with torch.no_grad():
        for m in models:      # biases that differ between the levels and years
            for net in m.year_models:
                net.conv1.conv_layer.bias.add_((torch.rand(32) - 0.5).to(dev()))
    raw = raw_raster(79, bands + 20, h, w)
    raw[:, 2, 3] = 7          # a constant pixel normalises to zero: a zero inside the mask
    ras = DenseRaster(raw, precision=precision, device=dev())
    table = Conv1TableYears([ras, None], MultiStagePredictor(models))
    cols = 32 * levels
    dt = torch.float16 if precision == "bf16" else torch.float32
    assert table.cols == cols and tuple(table.data[0].shape) == ((h + 2) * (w + 2) + 1, 9, cols) and table.data[0].dtype == dt
    assert tuple(table.data[1].shape) == (1, 9, cols) and table.data[1].dtype == dt
    wb = [[first_conv(m.year_models[y]) for m in models] for y in range(2)]
    wgt = np.concatenate([t[0] for t in wb[0]], axis=0)
    bias = np.concatenate([t[1] for t in wb[0]], axis=0)
    x = ras.float().cpu().numpy().astype(np.float64)
    want = conv1_table_np(x, (O.bf16_round(wgt) if precision == "bf16" else wgt).astype(np.float64), bias.astype(np.float64)).data
    got = table.data[0].cpu().numpy()
    bound = HALF_TABLE if precision == "bf16" else FP32_TIGHT
    grid = np.zeros((h + 2, w + 2), dtype=bool)
    grid[1:-1, 1:-1] = True
    inner = np.concatenate([grid.reshape(-1), [False]])
    ring = np.concatenate([~grid.reshape(-1), [False]])
    e_all, e_in, e_ring = rel_l2(got, want), rel_l2(got[inner], want[inner]), rel_l2(got[ring], want[ring])
    print(f"years table {h}x{w}, {bands} bands, {levels} levels, {precision}: rel-L2 {e_all:.3e} (interior {e_in:.3e}, ring {e_ring:.3e})")
    assert e_all <= bound and e_in <= bound and e_ring <= bound
    assert np.array_equal(got[-1], np.broadcast_to(bias.astype(got.dtype), (9, cols)))
    for l, m in enumerate(models):
        alone = ras.conv1_table(Predictor(m.year_models[0])).data.cpu().numpy()
        assert np.array_equal(bits_of(np.ascontiguousarray(got[:, :, 32 * l:32 * (l + 1)])), bits_of(alone)), l
    # the mask: the raster as stored
    stored = ras.float().cpu().numpy()
    mask = table.mask[0].cpu().numpy()
    assert mask.dtype == np.uint8 and np.array_equal(mask, conv1_mask_np(stored))
    assert mask[(2 + 1) * (w + 2) + (3 + 1)] == 0 and 0 < mask.sum() < h * w
    # the missing year: year 1's biases, rounded once to the table's storage, and the single zero byte
    far = np.concatenate([t[1] for t in wb[1]], axis=0).astype(got.dtype)
    assert np.array_equal(table.data[1].cpu().numpy(), np.broadcast_to(far, (1, 9, cols)))
    assert table.mask[1].cpu().tolist() == [0]
    assert not np.array_equal(far, bias.astype(got.dtype))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the gather
# ---------------------------------------------------------------------------------------------------------------------
def nan_into(ras, pixel):
    """One NaN into a stored raster, band 5 of `pixel`."""
    r, c = pixel
    if ras.precision == "fp32":
        ras.data[5, r, c] = float("nan")
    else:
        ras.data[((0 * ras.height * ras.width) + r * ras.width + c) * 16 + 5] = 0x7FC0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [29, 64])
def test_years_gather_is_a_bit_exact_copy_and_sets_the_flags(n, precision):
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd.dense import Conv1TableYears, DenseRaster, gather_conv1_years_np, year_flags_np
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS, prec=precision)
    pred = MultiStagePredictor(models, hierarchy=h)
    ras = dense_years(year_rasters(), precision)
    assert not ras[2].data.any()
    origins = edge_origins(H, W, seed=5, extra=n - 12)
    assert len(origins) == n
    assert (origins[:, 0] < 0).any() and (origins[:, 1] < 0).any() and (origins[:, 0] + 11 > H).any() and (origins[:, 1] + 11 > W).any()
    assert (origins == np.array([-11, 0])).all(axis=1).any()      # rows -11 .. -2 far outside, row -1 on the ring
    o = torch.from_numpy(origins).to(dev())
    banks = [torch.zeros(3, device=dev()) for _ in range(2)]
    esz = 2 if precision == "bf16" else 4
    # three calls, the banks alternating: the third finds the first call's flags cleared by the second
    for call, rs in enumerate(([ras[0], None, ras[2]], [ras[2], None, ras[0]], [ras[2], None, ras[0]])):
        table = Conv1TableYears(rs, pred)
        host = table.numpy()
        flags, nxt = banks[call & 1], banks[(call & 1) ^ 1]
        assert table.gather(o, pred, flags, nxt) is flags
        slot = pred.conv1_slot(n, BANDS)
        assert tuple(slot.shape) == (9, n * 121 * 32 * esz) and slot.dtype == torch.uint8
        want = gather_conv1_years_np(host, origins, 3)
        got = slot.cpu().numpy()
        for l in range(3):
            for y in range(3):
                g = got[l * 3 + y].view(np.uint16 if esz == 2 else np.uint32).reshape(n, 121, 32)
                assert np.array_equal(g, bits_of(np.ascontiguousarray(want[l, y]))), (call, l, y)
        assert flags.cpu().tolist() == ([1.0, 0.0, 0.0] if call == 0 else [0.0, 0.0, 1.0])
        assert flags.cpu().tolist() == year_flags_np([None if r is None else r.float().cpu().numpy() for r in rs], origins).tolist()
        assert not nxt.any()
        if precision == "fp32":      # what the float32 gather of the existing route says about the same origins
            outs = [torch.empty(n, BANDS, 11, 11, device=dev()) for _ in range(3)]
            theirs = DenseRaster.windows_years(rs, o, outs, torch.zeros(3, device=dev()), torch.zeros(3, device=dev()))
            assert_same_bits(flags, theirs, ("flags", call))
    # clear_next = NULL: the call clears its own flags first
    stale = torch.full((3,), 1.0, device=dev())
    table.gather(o, pred, stale, None)
    assert stale.cpu().tolist() == [0.0, 0.0, 1.0]
    # the forward behind it runs on that workspace
    e = pred.ensemble_from_conv1(stale)
    assert tuple(e[0].shape) == (n,) and bool(torch.isfinite(e[1]).all())
    with pytest.raises(RuntimeError, match="every year is missing"):
        bad = Conv1TableYears([ras[0], None, ras[2]], pred)
        bad._pr = (C.c_int * 3)(0, 0, 0)
        bad.gather(o, pred, banks[0], banks[1])
    assert _lib.lib().dta_abi_version() == 2


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_years_gather_counts_nan_as_non_zero(precision):
    from deeptreeattention_amd.dense import Conv1TableYears
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS, prec=precision)
    pred = MultiStagePredictor(models, hierarchy=h)
    ras = dense_years(year_rasters(), precision)
    nan_into(ras[2], (4, 5))
    table = Conv1TableYears(ras, pred)
    assert int(table.mask[2].sum()) == 1 and int(table.mask[2][(4 + 1) * (W + 2) + (5 + 1)]) == 1
    o = torch.tensor([[0, 0], [30, 30]], dtype=torch.int32, device=dev())        # the second window lies outside the raster
    banks = [torch.zeros(3, device=dev()) for _ in range(2)]
    assert table.gather(o, pred, banks[0], banks[1]).cpu().tolist() == [1.0, 0.0, 1.0]
    assert table.gather(o[1:], pred, banks[1], banks[0]).cpu().tolist() == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# 6. / 7. the route against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def route_models(ps, precision):
    from deeptreeattention_amd.year import learned_ensemble
    models = []
    for l, c in enumerate(ROUTE_CLASSES):
        m = learned_ensemble(3, c, {"pretrain_state_dict": None, "bands": ROUTE_BANDS})
        for y, net in enumerate(m.year_models):
            net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ps[l][y].items()})
            net.precision = precision
        models.append(m.to(dev()).eval())
    return models


def test_fp32_route_against_the_oracle():
    """Batch 64 over 300 windows (the last batch is partial).  Per level: probabilities against the float64 oracle rel-L2
    <= 2e-4; top-1 differing only where that level's oracle margin is below 2e-4, in at most 1 % of the windows.  ens_label
    equals Hierarchy.resolve_np on the route's own per-level top-1."""
    from deeptreeattention_amd.dense import predict_windows_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    raws, origins, ps, want, margin = route_case()
    h = three_level_hierarchy()
    models = route_models(ps, "fp32")
    res = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws, "fp32"), origins, batch_size=64,
                                     return_probs=True, share_conv1=True)
    n = len(origins)
    for l in range(3):
        e = rel_l2(res.probs[l].cpu().numpy(), want[l])
        differ = res.top_idx[l][:, 0].cpu().numpy() != want[l].argmax(axis=1)
        low = margin[l] < FP32_TIGHT
        print(f"fp32 level {l}, shared first conv: rel-L2 {e:.3e}; labels differing {int(differ.sum())}, oracle margins below "
              f"{FP32_TIGHT}: {int(low.sum())} of {n}")
        assert e <= FP32_TIGHT
        assert not (differ & ~low).any()
        assert differ.sum() <= 0.01 * n
    label, score, level = h.resolve_np([t[:, 0].cpu().numpy() for t in res.top_idx], [t[:, 0].cpu().numpy() for t in res.top_score])
    assert np.array_equal(res.ens_label.cpu().numpy(), label) and np.array_equal(res.ens_level.cpu().numpy(), level)
    assert np.array_equal(res.ens_score.cpu().numpy().view(np.uint32), score.view(np.uint32))
    assert len(np.unique(label)) >= 2


def test_bf16_route_against_the_oracle_with_the_existing_route_as_yardstick():
    """Per level: the new route's rel-L2 to the float64 oracle <= max(1e-2, 1.5 x the existing bf16 multi-stage route's
    rel-L2 to the same oracle), both measured here (the project's Bf16Yardstick rule)."""
    from deeptreeattention_amd.dense import predict_windows_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    raws, origins, ps, want, margin = route_case()
    h = three_level_hierarchy()
    models = route_models(ps, "bf16")
    old = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws, "fp32"), origins, batch_size=64,
                                     return_probs=True)
    new = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), dense_years(raws, "bf16"), origins, batch_size=64,
                                     return_probs=True, share_conv1=True)
    errs = []
    for l in range(3):
        e_old, e_new = rel_l2(old.probs[l].cpu().numpy(), want[l]), rel_l2(new.probs[l].cpu().numpy(), want[l])
        differ = int((new.top_idx[l][:, 0] != old.top_idx[l][:, 0]).sum())
        print(f"bf16 level {l} vs the float64 oracle: existing route rel-L2 {e_old:.3e}, shared first conv {e_new:.3e}; "
              f"labels differing between the routes: {differ} of {len(origins)}")
        errs.append((e_new, e_old))
    for e_new, e_old in errs:
        assert e_new <= max(1e-2, 1.5 * e_old)


# ---------------------------------------------------------------------------------------------------------------------
# 8. skipped years, reruns, frozen weights
# ---------------------------------------------------------------------------------------------------------------------
BOXES = [(0, 0, 8, 7), (2, 1, 6, 6), (3, 3, 3, 7), (5, 5, 6, 6), (14, 9, 19, 15)]      # tests/test_dense_multistage_gpu.py
BATCH = 64


def outputs(res):
    return [res.ens_label, res.ens_score, res.ens_level] + list(res.top_idx) + list(res.top_score) + list(res.probs)


def same_outputs(a, b, what):
    for k, (x, y) in enumerate(zip(outputs(a), outputs(b))):
        assert_same_bits(x, y, (what, k))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_skipped_years_reruns_and_frozen_weights(precision):
    from deeptreeattention_amd.dense import Conv1TableYears, predict_windows_multistage, window_origins
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS, prec=precision)
    ras = dense_years(year_rasters(), precision)       # year 1 missing, year 2 all zero after normalising
    origins, _ = window_origins(BOXES, anchor="center")
    N = len(origins)
    assert N == 107 and N % BATCH != 0
    run = lambda pred: predict_windows_multistage(pred, ras, origins, batch_size=BATCH, return_probs=True, share_conv1=True)      # noqa: E731
    pred = MultiStagePredictor(models, hierarchy=h)
    a = run(pred)
    same_outputs(run(pred), a, "rerun on the same predictor")
    same_outputs(run(MultiStagePredictor(models, hierarchy=h)), a, "rerun on a new predictor")
    assert int(a.ens_label.min()) >= 0 and bool(torch.isfinite(a.ens_score).all())
    # a full forward in between (same predictor, same workspace) leaves the route's results as they were
    if precision == "fp32":
        predict_windows_multistage(pred, ras, origins[:50], batch_size=BATCH)
        same_outputs(run(pred), a, "after a full forward on the same workspace")
    # frozen weights: the bits of frozen=False, on a first and on a second call
    frozen = MultiStagePredictor(models, frozen=True, hierarchy=h)
    same_outputs(run(frozen), a, "frozen, first call")
    same_outputs(run(frozen), a, "frozen, second call")
    assert frozen._packed_conv1 and not frozen._packed
    # had years 1 and 2 taken part (their flags forced to 1: the biases resp. zeros through their networks), the
    # probabilities would be other ones ...
    o = ras[0]._origins(origins[:BATCH])
    table = Conv1TableYears(ras, pred)
    flags = table.gather(o, pred, torch.zeros(3, device=dev()), None)
    assert flags.cpu().tolist() == [1.0, 0.0, 0.0]
    pred.ensemble_from_conv1(flags)
    for l in range(3):
        assert_same_bits(pred.probs[l], a.probs[l][:BATCH], ("the route's first batch", l))
    table.gather(o, pred, torch.zeros(3, device=dev()), None)
    pred.ensemble_from_conv1(torch.ones(3, device=dev()))
    all3 = [p.clone() for p in pred.probs]
    assert not torch.equal(all3[2], a.probs[2][:BATCH])
    # ... and nothing of their networks reaches the result: other weights in years 1 and 2, the same bits
    with torch.no_grad():
        for m in models:
            for y in (1, 2):
                for p in m.year_models[y].parameters():
                    p.mul_(-1.5)
    same_outputs(run(MultiStagePredictor(models, hierarchy=h)), a, "years 1 and 2 left out")
    table = Conv1TableYears(ras, pred)
    table.gather(o, pred, torch.zeros(3, device=dev()), None)
    pred.ensemble_from_conv1(torch.ones(3, device=dev()))
    assert not torch.equal(pred.probs[2], all3[2])


# ---------------------------------------------------------------------------------------------------------------------
# 9. maps, crowns, weight updates, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_maps_crowns_and_a_weight_update():
    from deeptreeattention_amd.dense import crown_resolve_np, predict_map_multistage, predict_windows_multistage, window_origins
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS)
    pred = MultiStagePredictor(models, hierarchy=h)
    raws = year_rasters()
    ras = dense_years(raws, "fp32")
    # crowns: crown_resolve_np on this route's own window probabilities
    origins, offsets = window_origins(BOXES, anchor="center")
    res = predict_windows_multistage(pred, ras, origins, crown_offsets=offsets, batch_size=BATCH, return_probs=True, share_conv1=True)
    crowns = crown_resolve_np([p.cpu().numpy() for p in res.probs], offsets, h, window_labels=res.ens_label.cpu().numpy())
    same_crowns(res.crowns, crowns)
    assert res.crowns.count.cpu().tolist() == [56, 20, 0, 1, 30] and int(res.crowns.label[2]) == -1
    lean = predict_windows_multistage(pred, ras, origins, batch_size=BATCH, share_conv1=True)
    assert lean.probs is None and lean.crowns is None
    assert_same_bits(lean.ens_label, res.ens_label, "lean"); assert_same_bits(lean.top_score[2], res.top_score[2], "lean")
    # the map from raw arrays equals the windows over all pixels, whole and in part
    for rows, cols in ((None, None), ((3, 12), (2, 9))):
        r0, r1 = rows or (0, H)
        c0, c1 = cols or (0, W)
        o, _ = window_origins([(r0, c0, r1, c1)], anchor="center")
        want = predict_windows_multistage(pred, ras, o, batch_size=BATCH, share_conv1=True)
        want = [t.clone() for t in (want.ens_label, want.ens_score, want.ens_level)]
        species, score, level = predict_map_multistage(pred, raws, rows=rows, cols=cols, batch_size=BATCH, share_conv1=True)
        assert tuple(species.shape) == tuple(score.shape) == tuple(level.shape) == (r1 - r0, c1 - c0)
        assert species.dtype == torch.int64 and score.dtype == torch.float32 and level.dtype == torch.int32
        assert_same_bits(species.reshape(-1), want[0], rows); assert_same_bits(score.reshape(-1), want[1], rows)
        assert_same_bits(level.reshape(-1), want[2], rows)
    # a weight update between two calls is followed: the tables are built inside each call
    before = [p.clone() for p in res.probs]
    with torch.no_grad():
        models[2].year_models[0].conv1.conv_layer.weight.mul_(1.5)
        models[0].year_models[0].conv1.conv_layer.bias.add_(0.25)
    new = predict_windows_multistage(pred, ras, origins, batch_size=BATCH, return_probs=True, share_conv1=True).probs
    old_route = predict_windows_multistage(MultiStagePredictor(models, hierarchy=h), ras, origins, batch_size=BATCH, return_probs=True).probs
    for l in (0, 2):
        assert not torch.equal(before[l].cpu(), new[l].cpu())
    for l in range(3):
        assert rel_l2(new[l].cpu().numpy(), old_route[l].cpu().numpy()) <= FP32_TIGHT


def test_refusals_allocate_nothing(monkeypatch):
    from deeptreeattention_amd import dense
    from deeptreeattention_amd.engine import MultiStagePredictor
    from deeptreeattention_amd.hierarchy import Hierarchy
    from test_hierarchy_cpu import load_ensemble_fixture
    h = three_level_hierarchy()
    m32 = _small_levels(h.classes, 3, bands=BANDS)
    m16 = _small_levels(h.classes, 3, bands=BANDS, prec="bf16")
    raws = year_rasters()
    r32, r16 = dense_years(raws, "fp32"), dense_years(raws, "bf16")
    other = dense.DenseRaster(raw_raster(3, BANDS + 10, H, W), precision="fp32", device=dev())      # 13 bands after clipping
    p32, p16 = MultiStagePredictor(m32, hierarchy=h), MultiStagePredictor(m16, hierarchy=h)
    fx = load_ensemble_fixture()
    h5 = Hierarchy.from_reference(fx["level_label_dicts"], fx["species_label_dict"])
    m20 = _small_levels(h5.classes, 4, bands=BANDS)          # 5 levels x 4 years = 20 networks
    p20 = MultiStagePredictor(m20, hierarchy=h5)
    origins = np.zeros((4, 2), np.int32)
    torch.cuda.synchronize()
    launched = torch.cuda.memory_allocated()

    def refused(match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
        assert torch.cuda.memory_allocated() == launched

    m32[1].year_models[2].train()
    refused("training mode", lambda: dense.predict_windows_multistage(p32, r32, origins, share_conv1=True))
    refused("training mode", lambda: dense.predict_map_multistage(p32, raws, share_conv1=True))
    m32[1].year_models[2].eval()
    refused("precision='fp32'", lambda: dense.predict_windows_multistage(p32, r16, origins, share_conv1=True))
    refused("precision='bf16'", lambda: dense.predict_windows_multistage(p16, r32, origins, share_conv1=True))
    refused("precision='bf16'", lambda: dense.predict_map_multistage(p16, r32, share_conv1=True))
    refused("13", lambda: dense.predict_windows_multistage(p32, [other, None, None], origins, share_conv1=True))
    refused("one chain", lambda: dense.predict_windows_multistage(p20, [r32[0], None, None, None], origins, share_conv1=True))
    monkeypatch.setattr(dense, "WINDOW", 7)
    refused("window side 7", lambda: dense.predict_windows_multistage(p32, r32, origins, share_conv1=True))
    refused("window side 7", lambda: dense.predict_map_multistage(p32, raws, share_conv1=True))
    monkeypatch.undo()
    # the default route keeps its own checks and messages
    with pytest.raises(RuntimeError, match="fp32"):
        dense.predict_windows_multistage(p32, r16, origins)
    # the single-network route still refuses a year ensemble (tests/test_dense_conv1_gpu.py pins the message)
    refused("year ensemble", lambda: dense.predict_windows(m32[0], r32, origins, share_conv1=True))
