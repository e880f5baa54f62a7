"""Dense per-pixel window prediction on the device (deeptreeattention_amd.dense): the gather against explicitly sliced
windows through the existing crop preprocessing (bit for bit), per-window prediction against the existing Predictor on
the materialised windows, the fp32 route against the torch oracle, the crown reduce against its host definition.
All fixtures are synthetic (oracle.prng)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O
from oracle import hang2020_torch as OT
from oracle import preprocess_np as PP
from oracle import prng

pytestmark = pytest.mark.gpu

FP32_TIGHT = 2e-4      # tests/test_hip_parity.py: the eval-mode golden check of the fp32 Hang2020 (test_hang2020_vs_reference_golden)
HEAD_GAIN = 30.0
ORACLE_SEED = 61       # the fp32-vs-oracle case below


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def raw_raster(seed, bands, h, w, dtype=np.int16):
    u = prng.uniform01(seed, 1, (bands, h, w))
    # a scene, not noise: each quadrant has its own spectral shape (a step at its own band), under 30 % noise
    kind = (np.arange(h)[:, None] >= h // 2) + 2 * (np.arange(w)[None, :] >= w // 2)
    edge = (bands * (1 + kind)) // 5
    shape = (np.arange(bands)[:, None, None] >= edge[None]).astype(np.float64)
    u = 0.3 * u + 0.7 * shape
    if dtype == np.int16:
        a = (u * 9000 - 800).astype(np.int16)
    elif dtype == np.uint8:
        a = (u * 255).astype(np.uint8)
    else:
        a = (u * 3 - 1).astype(np.float32)
    a[:, h // 2, w // 3] = a[0, h // 2, w // 3]       # one constant pixel
    return a


def raw_windows(raw, origins, size=11):
    """What a boundless read of each window returns: slices of a zero-padded copy."""
    pad = 64
    Cb, Hh, Ww = raw.shape
    big = np.zeros((Cb, Hh + 2 * pad, Ww + 2 * pad), dtype=raw.dtype)
    big[:, pad:pad + Hh, pad:pad + Ww] = raw
    return [np.ascontiguousarray(big[:, r + pad:r + pad + size, c + pad:c + pad + size]) for r, c in np.asarray(origins)]


def edge_origins(h, w, seed=3, extra=24):
    """Windows hanging over all four edges and corners, some entirely inside (when the raster allows), one entirely outside."""
    fixed = [(-5, -5), (-5, w - 6), (h - 6, -5), (h - 6, w - 6), (-10, w // 2), (h - 1, w // 2 - 5), (h // 2 - 5, -10),
             (h // 2 - 5, w - 1), (0, 0), (max(h - 11, 0), max(w - 11, 0)), (-11, 0), (h // 2 - 5, w // 2 - 5)]
    rr = prng.randint(seed, 1, (extra,), h + 10) - 10
    cc = prng.randint(seed, 2, (extra,), w + 10) - 10
    return np.array(fixed + list(zip(rr.tolist(), cc.tolist())), dtype=np.int32)


def make(kind, bands, classes, seed, precision):
    from deeptreeattention_amd import Hang2020 as H
    p = oracle_params(kind, bands, classes, seed)
    m = {"hang": H.Hang2020, "vanilla": H.vanilla_CNN}[kind](bands, classes, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
    return m.to(dev()).eval(), p


def predictor_on_windows(model, windows_of_batch, n, batch_size, classes):
    """The existing route: engine.Predictor on explicitly materialised, preprocessed windows, same batch partition."""
    from deeptreeattention_amd.engine import Predictor
    pred = Predictor(model)
    probs = torch.empty(n, classes, dtype=torch.float32, device=dev())
    idx = torch.empty(n, 2, dtype=torch.int64, device=dev())
    score = torch.empty(n, 2, dtype=torch.float32, device=dev())
    for n0 in range(0, n, batch_size):
        n1 = min(n0 + batch_size, n)
        p, i, s = pred(windows_of_batch(n0, n1), return_probs=True)
        probs[n0:n1], idx[n0:n1], score[n0:n1] = p, i, s
    return probs, idx, score


def assert_same_bits(a, b, what):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.float32])
@pytest.mark.parametrize("bands,h,w", [(369, 40, 37), (23, 12, 12), (3, 12, 12)])
def test_fp32_windows_equal_preprocessed_explicit_windows(bands, h, w, dtype):
    from deeptreeattention_amd.dense import DenseRaster, gather_windows_np
    from deeptreeattention_amd.preprocess import preprocess_batch, out_bands
    raw = raw_raster(17, bands, h, w, dtype)
    origins = edge_origins(h, w)
    got = DenseRaster(raw, precision="fp32", device=dev()).windows(origins)
    want = preprocess_batch(raw_windows(raw, origins), 11, device=dev())
    assert got.shape == (len(origins), out_bands(bands), 11, 11)
    assert_same_bits(got, want, "float32 windows")
    # the resident raster is the oracle's preprocessing of the whole raster, and the kernel is gather_windows_np of it
    whole = PP.preprocess_image(raw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), gather_windows_np(whole, origins, 11).view(np.uint32))


@pytest.mark.parametrize("bands,h,w,dtype", [(369, 40, 37, np.int16), (23, 12, 12, np.uint8), (40, 17, 13, np.float32)])
def test_tile_windows_equal_preprocessed_explicit_tiles(bands, h, w, dtype):
    from deeptreeattention_amd.dense import DenseRaster
    from deeptreeattention_amd.preprocess import preprocess_batch
    raw = raw_raster(19, bands, h, w, dtype)
    origins = edge_origins(h, w)
    ras = DenseRaster(raw, precision="bf16", device=dev())
    got = ras.windows(origins, tiles=True)
    want = preprocess_batch(raw_windows(raw, origins), 11, device=dev(), tiles=True)
    assert got.shape == want.shape
    assert got.tiles.dtype == want.tiles.dtype and torch.equal(got.tiles.cpu(), want.tiles.cpu())
    # the resident chunks hold the fp32 raster rounded to bf16
    f32 = DenseRaster(raw, precision="fp32", device=dev()).data
    assert torch.equal(ras.float().cpu(), f32.to(torch.bfloat16).float().cpu())


def test_other_window_sides_and_refused_arguments():
    from deeptreeattention_amd.dense import DenseRaster, gather_windows_np
    raw = raw_raster(23, 30, 14, 16)
    ras = DenseRaster(raw, precision="fp32", device=dev())
    origins = edge_origins(14, 16)
    whole = PP.preprocess_image(raw)
    for size in (4, 7, 24):
        got = ras.windows(origins, size=size)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), gather_windows_np(whole, origins, size).view(np.uint32)), size
    with pytest.raises(RuntimeError, match="window side"):
        ras.windows(origins, size=3)
    with pytest.raises(RuntimeError, match="precision='bf16'"):
        ras.windows(origins, tiles=True)


# ---------------------------------------------------------------------------------------------------------------------
# prediction
# ---------------------------------------------------------------------------------------------------------------------
def all_pixel_case(seed, bands, h, w, anchor="center"):
    from deeptreeattention_amd.dense import window_origins
    raw = raw_raster(seed, bands, h, w)
    boxes = [(0, 0, h // 2, w), (h // 2, 0, h // 2, w), (h // 2, 0, h, w // 2), (h // 2, w // 2, h, w)]    # the second is empty
    origins, offsets = window_origins(boxes, anchor=anchor)
    return raw, origins, offsets


def test_hang2020_bf16_tiles_route_equals_predictor():
    """bf16 Hang2020: tile gather + dta_net_forward_tiles.  Identical bits to the Predictor on preprocess_batch's tiles of
    the explicit windows AND to the Predictor on the float batch of the same windows (the first conv converting to bf16
    while staging: same rounding, same order of the sums -- measured rel-L2 0, profiles/README.md)."""
    from deeptreeattention_amd.dense import DenseRaster, predict_windows, raster_precision
    from deeptreeattention_amd.preprocess import preprocess_batch
    bands_raw, classes, B = 389, 200, 128
    raw, origins, offsets = all_pixel_case(29, bands_raw, 20, 15)
    model, _ = make("hang", 369, classes, 31, "bf16")
    assert raster_precision(model) == "bf16"
    wins = raw_windows(raw, origins)
    n = len(origins)
    res = predict_windows(model, DenseRaster(raw, precision="bf16", device=dev()), origins, batch_size=B, return_probs=True)
    for tiles in (True, False):
        probs, idx, score = predictor_on_windows(model, lambda a, b: preprocess_batch(wins[a:b], 11, device=dev(), tiles=tiles), n, B, classes)
        d = rel_l2(res.probs.cpu().numpy(), probs.cpu().numpy())
        print(f"predict_windows vs Predictor on explicit windows (tiles={tiles}): rel-L2 of the probabilities {d:.3e}, "
              f"labels differing: {int((res.top_idx[:, 0] != idx[:, 0]).sum())} of {n}")
        assert_same_bits(res.probs, probs, "probabilities")
        assert torch.equal(res.top_idx.cpu(), idx.cpu())
        assert_same_bits(res.top_score, score, "top-2 scores")


def test_hang2020_fp32_route_equals_predictor_and_oracle():
    """fp32 Hang2020: float32 gather + the existing Predictor path; identical bits to the Predictor on the explicit windows.
    The probabilities against oracle/hang2020_torch.py (eval forward + softmax) on oracle/preprocess_np.py windows within the
    eval-mode golden tolerance of tests/test_hip_parity.py (2e-4, norm-wise).  Labels may differ from the oracle's only where
    the oracle's own top-2 margin is below that tolerance, in at most 1 % of the windows.  Seed 61: the oracle alone has
    0 of 300 windows with a margin below 2e-4 (smallest margin 1.9e-2; checked on the CPU)."""
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    from deeptreeattention_amd.preprocess import preprocess_batch
    raw, origins, offsets, model, p, classes = oracle_case(True)
    B, n = 128, len(origins)
    wins = raw_windows(raw, origins)
    res = predict_windows(model, DenseRaster(raw, precision="fp32", device=dev()), origins, batch_size=B, return_probs=True)
    probs, idx, score = predictor_on_windows(model, lambda a, b: preprocess_batch(wins[a:b], 11, device=dev()), n, B, classes)
    assert_same_bits(res.probs, probs, "probabilities")
    assert torch.equal(res.top_idx.cpu(), idx.cpu())
    assert_same_bits(res.top_score, score, "top-2 scores")
    want, margin = oracle_probs(p, wins)
    got = res.probs.cpu().numpy()
    e = rel_l2(got, want)
    differ = res.top_idx[:, 0].cpu().numpy() != want.argmax(axis=1)
    low = margin < FP32_TIGHT
    print(f"fp32 probabilities vs the oracle: rel-L2 {e:.3e}; labels differing {int(differ.sum())}, oracle margins below "
          f"{FP32_TIGHT}: {int(low.sum())} of {n}")
    assert e < FP32_TIGHT
    assert not (differ & ~low).any()
    assert differ.sum() <= 0.01 * n and low.sum() <= 0.01 * n


def oracle_case(with_model):
    bands_raw, classes = 40, 7
    raw, origins, offsets = all_pixel_case(ORACLE_SEED, bands_raw, 20, 15)
    if with_model:
        model, p = make("hang", 20, classes, ORACLE_SEED, "fp32")
    else:
        model, p = None, oracle_params("hang", 20, classes, ORACLE_SEED)
    return raw, origins, offsets, model, p, classes


def oracle_params(kind, bands, classes, seed):
    spec = {"hang": O.hang2020_spec, "vanilla": O.vanilla_spec}[kind](bands, classes)
    p = O.init_params(spec, seed=seed)
    # eval-mode BatchNorm reads the running statistics: give them values a trained network would have
    for k in p:
        if k.endswith("running_mean"):
            p[k] = (0.2 * (prng.uniform01(seed, 7, p[k].shape) - 0.5)).astype(np.float32)
        elif k.endswith("running_var"):
            p[k] = (0.5 + prng.uniform01(seed + 1, 9, p[k].shape)).astype(np.float32)
        elif k.endswith("classifier3.fc1.weight") or k == "classifier.weight" or k.endswith("fc1.weight") and kind == "vanilla":
            p[k] = (p[k] * HEAD_GAIN).astype(np.float32)       # heads that tell the classes apart (an untrained head is near-uniform)
    return p


def oracle_probs(p, wins):
    x = torch.from_numpy(np.stack([PP.preprocess_image(w) for w in wins]))
    with torch.no_grad():
        pt = {k: torch.from_numpy(np.array(v)) for k, v in p.items()}
        pr = torch.softmax(OT.hang2020(pt, x, training=False), dim=1).numpy()
    top = np.sort(pr, axis=1)
    return pr, top[:, -1] - top[:, -2]


def test_vanilla_cnn_route_equals_predictor():
    from deeptreeattention_amd.dense import DenseRaster, predict_windows, raster_precision
    from deeptreeattention_amd.preprocess import preprocess_batch
    classes, B = 5, 96
    raw, origins, offsets = all_pixel_case(37, 30, 16, 13, anchor="corner")
    wins, n = raw_windows(raw, origins), len(origins)
    for precision in ("fp32", "bf16"):            # every network but the bf16 Hang2020 takes the float32 gather
        model, _ = make("vanilla", 10, classes, 41, precision)
        assert raster_precision(model) == "fp32"
        res = predict_windows(model, DenseRaster(raw, precision="fp32", device=dev()), origins, batch_size=B, return_probs=True)
        probs, idx, score = predictor_on_windows(model, lambda a, b: preprocess_batch(wins[a:b], 11, device=dev()), n, B, classes)
        assert_same_bits(res.probs, probs, "probabilities")
        assert torch.equal(res.top_idx.cpu(), idx.cpu())
        assert_same_bits(res.top_score, score, "top-2 scores")
    with pytest.raises(RuntimeError, match="precision='fp32'"):
        predict_windows(model, DenseRaster(raw, precision="bf16", device=dev()), origins)
    # the Predictor refuses tiles for anything but a bf16 Hang2020 before the C call does (model: the bf16 vanilla_CNN)
    from deeptreeattention_amd.engine import Predictor
    with pytest.raises(RuntimeError, match="bf16-mode Hang2020"):
        Predictor(model)(preprocess_batch(wins[:4], 11, device=dev(), tiles=True))


def test_three_year_ensemble_with_a_missing_year_equals_predictor():
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.preprocess import preprocess_batch
    from deeptreeattention_amd.year import learned_ensemble
    classes, B, bands_raw = 6, 100, 36
    torch.manual_seed(5)
    ens = learned_ensemble(3, classes, {"pretrain_state_dict": None, "bands": bands_raw - 20}).to(dev()).eval()
    raw0, origins, offsets = all_pixel_case(43, bands_raw, 16, 14)
    raw2 = raw_raster(47, bands_raw, 16, 14)
    n = len(origins)
    w0, w2 = raw_windows(raw0, origins), raw_windows(raw2, origins)
    rasters = [DenseRaster(raw0, precision="fp32", device=dev()), None, DenseRaster(raw2, precision="fp32", device=dev())]
    res = predict_windows(ens, rasters, origins, batch_size=B, return_probs=True)
    pred = Predictor(ens)
    for n0 in range(0, n, B):
        n1 = min(n0 + B, n)
        x0, x2 = preprocess_batch(w0[n0:n1], 11, device=dev()), preprocess_batch(w2[n0:n1], 11, device=dev())
        p, i, s = pred([x0, torch.zeros_like(x0), x2], return_probs=True)
        assert_same_bits(res.probs[n0:n1], p, "probabilities")
        assert torch.equal(res.top_idx[n0:n1].cpu(), i.cpu())
        assert_same_bits(res.top_score[n0:n1], s, "top-2 scores")
    with pytest.raises(ValueError, match="3 rasters"):
        predict_windows(ens, rasters[:2], origins)


# ---------------------------------------------------------------------------------------------------------------------
# crown reduce, map
# ---------------------------------------------------------------------------------------------------------------------
def test_crown_reduce_equals_host_definition_and_reruns_identically():
    from deeptreeattention_amd.dense import DenseRaster, crown_reduce, crown_reduce_np, predict_windows
    raw, origins, offsets, model, p, classes = oracle_case(True)
    # two more crowns: a single window, and a repeat of the first crown
    origins = np.concatenate([origins, origins[5:6], origins[:offsets[1]]])
    offsets = np.concatenate([offsets, [offsets[-1] + 1, offsets[-1] + 1 + offsets[1]]])
    ras = DenseRaster(raw, precision="fp32", device=dev())
    res = predict_windows(model, ras, origins, crown_offsets=offsets, batch_size=128, return_probs=True)
    cr = res.crowns
    mean, top_idx, top_score, count = crown_reduce_np(res.probs.cpu().numpy(), offsets)
    assert np.array_equal(cr.mean.cpu().numpy().view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(cr.top_idx.cpu().numpy(), top_idx)
    assert np.array_equal(cr.top_score.cpu().numpy().view(np.uint32), top_score.view(np.uint32))
    assert np.array_equal(cr.count.cpu().numpy(), count) and count.tolist() == np.diff(offsets).tolist()
    assert count[1] == 0 and top_idx[1].tolist() == [-1, -1] and (mean[1] == 0).all()      # the empty crown
    single = len(offsets) - 3                                                               # a crown of one window: that window's top-2
    assert count[single] == 1
    assert torch.equal(cr.top_idx[single].cpu(), res.top_idx[offsets[single]].cpu())
    assert_same_bits(cr.top_score[single], res.top_score[offsets[single]], "single-window crown")
    assert_same_bits(cr.mean[single], res.probs[offsets[single]], "single-window crown mean")
    again = predict_windows(model, ras, origins, crown_offsets=offsets, batch_size=128).crowns
    for a, b in zip(cr, again):
        assert torch.equal(a.cpu(), b.cpu())
    # ties go to the lower class; a crown longer than the unrolled loop's multiple of four
    pr = torch.zeros(7, 300, device=dev())
    pr[:, 280] = 0.5; pr[:, 17] = 0.5; pr[:, 100] = 0.25
    t = crown_reduce(pr, [0, 7])
    assert t.top_idx.cpu().tolist() == [[17, 280]] and t.count.cpu().tolist() == [7]
    with pytest.raises(ValueError):
        crown_reduce(pr, [0, 9])


def test_predict_map_equals_predict_windows_over_all_pixels():
    from deeptreeattention_amd.dense import DenseRaster, predict_map, predict_windows, window_origins
    raw, _, _, model, p, classes = oracle_case(True)
    h, w = raw.shape[1:]
    assert (h, w) == (20, 15)
    labels, scores = predict_map(model, raw, anchor="center", batch_size=77)
    assert labels.shape == (h, w) and labels.dtype == torch.int64 and scores.dtype == torch.float32
    origins, _ = window_origins([(0, 0, h, w)], anchor="center")
    res = predict_windows(model, DenseRaster(raw, precision="fp32", device=dev()), origins, batch_size=77)
    assert torch.equal(labels.cpu(), res.top_idx[:, 0].reshape(h, w).cpu())
    assert_same_bits(scores, res.top_score[:, 0].reshape(h, w), "score map")
    sub_l, sub_s = predict_map(model, raw, anchor="center", rows=(3, 9), cols=(2, 15))
    assert torch.equal(sub_l.cpu(), labels[3:9, 2:15].cpu())
    # the bf16 Hang2020 through the tile route gives a map as well (a resident raster passed in)
    m16, _ = make("hang", 20, classes, ORACLE_SEED, "bf16")
    l16, s16 = predict_map(m16, DenseRaster(raw, precision="bf16", device=dev()), anchor="corner")
    assert l16.shape == (h, w) and bool((s16 > 0).all())
