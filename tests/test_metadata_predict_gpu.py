"""Prediction with the site-metadata fusion model on the device: engine.MetadataPredictor (dta_meta_site_table +
dta_meta_predict), MetadataTrainer.predict_step and the dense route, against the reference's golden, against the host
statement (metadata.site_table_np / fuse_predict_np) and against themselves (row independence, modes, frozen tables)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O
from oracle import prng

pytestmark = pytest.mark.gpu

BANDS, CLASSES, SITES, B = 369, 200, 23, 64


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def full_model(g, precision):
    """tests/test_config4_gpu.py::_model: the sensor weights from the portable PRNG, the head from the golden."""
    from deeptreeattention_amd.metadata import metadata_sensor_fusion
    m = metadata_sensor_fusion(bands=BANDS, sites=SITES, classes=CLASSES, precision=precision)
    sd = {"sensor_model." + k: torch.from_numpy(np.array(v)) for k, v in
          O.init_params(O.hang2020_spec(BANDS, CLASSES), seed=21).items()}
    for k in g.files:
        if k.startswith("init/"):
            a = g[k]
            sd[k[len("init/"):]] = torch.from_numpy(a.astype(np.float32) if a.dtype == np.float16 else a)
    m.load_state_dict(sd)
    return m.to(dev())


def full_batch():
    x = torch.from_numpy(prng.uniform01(30, 1, (B, BANDS, 11, 11))).to(dev())
    site = torch.from_numpy(prng.randint(30, 2, (B,), SITES)).to(dev())
    return x, site


def small_model(bands, classes, sites, seed, precision="fp32"):
    """A small fusion model with every head tensor, the running statistics included, away from its initial value."""
    from deeptreeattention_amd.metadata import metadata_sensor_fusion
    torch.manual_seed(seed)
    m = metadata_sensor_fusion(bands=bands, sites=sites, classes=classes, precision=precision)
    with torch.no_grad():
        bn = m.metadata_model.batch_norm
        bn.running_mean.copy_(torch.randn(16) * 0.3)
        bn.running_var.copy_(torch.rand(16) + 0.5)
        bn.weight.copy_(torch.rand(16) + 0.5)
        bn.bias.copy_(torch.randn(16) * 0.2)
        m.fc1.weight.mul_(3.0)
        m.fc1.bias.copy_(torch.randn(classes) * 0.1)
    return m.to(dev()).eval()


def head_params(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if not k.startswith("sensor_model.")}


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def clones(res):
    return tuple(None if t is None else t.clone() for t in res)


def check_self_consistent(probs, top_idx, top_score, invalid=()):
    """Item 5: top_idx / top_score are the lowest-index top-2 of the kernel's own probability rows, bit for bit, and the rows
    sum to 1 within 1e-6; rows listed in `invalid` follow the invalid-site convention instead."""
    p, ti, ts = probs.cpu().numpy(), top_idx.cpu().numpy(), top_score.cpu().numpy()
    worst = 0.0
    for b in range(p.shape[0]):
        if b in invalid:
            assert not p[b].any() and np.array_equal(ti[b], [-1, -1]) and not ts[b].any(), b
            continue
        order = np.argsort(-p[b], kind="stable")[:2]
        assert np.array_equal(ti[b], order), (b, ti[b], order)
        assert np.array_equal(ts[b].view(np.int32), p[b][order].view(np.int32)), b
        worst = max(worst, abs(float(p[b].astype(np.float64).sum()) - 1.0))
    print(f"  self-consistency: {p.shape[0] - len(invalid)} rows, largest |sum(probs) - 1| = {worst:.2e}")
    assert worst < 1e-6


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.fixture(scope="module")
def full_fp32(golden):
    from deeptreeattention_amd.engine import MetadataPredictor
    g = golden("metadata_full.npz")
    m = full_model(g, "fp32").eval()
    x, site = full_batch()
    pred = MetadataPredictor(m)
    probs, top_idx, top_score = clones(pred(x, site))
    return g, m, x, site, probs, top_idx, top_score, pred.fused_scores.clone()


def test_golden_real_size_fp32(full_fp32):
    """369 / 200 / 23, B = 64 against the reference's eval output: fused scores rel-L2 < 1e-3 (the project's fp32 bound),
    the probabilities against softmax(eval/out) under the same bound, top-1 equal on all 64 rows, top-2 equal on every row
    whose reference 2nd - 3rd gap exceeds twice this run's largest probability deviation (at most 2 rows left out)."""
    g, m, x, site, probs, top_idx, top_score, fused = full_fp32
    ref = g["eval/out"]
    e = rel_l2(fused.cpu().numpy(), ref)
    want = softmax64(ref)
    got = probs.cpu().numpy().astype(np.float64)
    dev_p = float(np.abs(got - want).max())
    e_p = rel_l2(got, want)
    srt = np.sort(want, axis=1)
    gap12, gap23 = srt[:, -1] - srt[:, -2], srt[:, -2] - srt[:, -3]
    print(f"fp32: fused scores rel-L2 {e:.2e}, probabilities rel-L2 {e_p:.2e}, max-abs {dev_p:.2e}; reference gaps: "
          f"1st - 2nd >= {gap12.min():.2e}, 2nd - 3rd >= {gap23.min():.2e}")
    assert e < 1e-3
    assert e_p < 1e-3
    order = np.argsort(-want, axis=1, kind="stable")
    ti = top_idx.cpu().numpy()
    assert np.array_equal(ti[:, 0], order[:, 0])
    judged = gap23 > 2 * dev_p
    print(f"  top-2 judged on {int(judged.sum())} of {B} rows")
    assert (~judged).sum() <= 2
    assert np.array_equal(ti[judged, 1], order[judged, 1])
    check_self_consistent(probs, top_idx, top_score)


def test_golden_real_size_bf16(golden, bf16_yardstick):
    """The bf16-mode model: fused scores under the reference's own bf16 yardstick (as tests/test_config4_gpu.py holds the
    model's scores); labels only to self-consistency: the 1st - 2nd gaps are the size of the bf16 deviation."""
    from deeptreeattention_amd.engine import MetadataPredictor
    g = golden("metadata_full.npz")
    m = full_model(g, "bf16").eval()
    x, site = full_batch()
    pred = MetadataPredictor(m)
    probs, top_idx, top_score = pred(x, site)
    e = rel_l2(pred.fused_scores.cpu().numpy(), g["eval/out"])
    print(f"bf16: fused scores rel-L2 {e:.2e} (bound {bf16_yardstick.bound('meta64/scores_dev'):.2e})")
    assert e < bf16_yardstick.bound("meta64/scores_dev")
    check_self_consistent(probs, top_idx, top_score)


@pytest.mark.parametrize("classes,batch,sites,mode", [
    (5, 1, 1, "scalar"), (7, 9, 4, "tensor"), (5, 70, 23, "tensor"), (200, 70, 23, "scalar"), (200, 9, 4, "invalid"),
    (301, 70, 4, "tensor"), (301, 9, 23, "invalid"), (7, 70, 1, "invalid")])
def test_small_shapes_vs_host_statement(classes, batch, sites, mode):
    """bands 12; fused scores and probabilities within rel-L2 1e-5 of fuse_predict_np(site_table_np(...)) on the HSI scores the
    sensor Predictor returned; rows with sites -1 and `sites` follow the convention and raise no HIP error."""
    from deeptreeattention_amd.engine import MetadataPredictor
    from deeptreeattention_amd.metadata import fuse_predict_np, site_table_np
    m = small_model(12, classes, sites, seed=classes + batch)
    x = torch.from_numpy(prng.uniform01(50 + classes, 1, (batch, 12, 11, 11))).to(dev())
    site_np = prng.randint(50 + classes, 2, (batch,), sites).astype(np.int64)
    invalid = ()
    if mode == "scalar":
        site_np[:] = sites - 1
        site = sites - 1
    else:
        if mode == "invalid":
            invalid = (0, batch // 2, batch - 1)
            site_np[0], site_np[batch // 2], site_np[batch - 1] = -1, sites, sites + 5
        site = torch.from_numpy(site_np).to(dev())
    pred = MetadataPredictor(m)
    probs, top_idx, top_score = pred(x, site)
    torch.cuda.synchronize()
    hsi = pred.sensor.logits.cpu().numpy()
    p = head_params(m)
    out, want, _, _ = fuse_predict_np(site_table_np(p, m.metadata_model.batch_norm.eps), p["fc1.weight"], site_np, hsi)
    e_out, e_p = rel_l2(pred.fused_scores.cpu().numpy(), out), rel_l2(probs.cpu().numpy(), want)
    print(f"classes {classes} B {batch} sites {sites} {mode}: fused rel-L2 {e_out:.2e}, probabilities rel-L2 {e_p:.2e}")
    assert e_out < 1e-5 and e_p < 1e-5
    for b in invalid:
        assert not pred.fused_scores[b].any()
    check_self_consistent(probs, top_idx, top_score, invalid)
    # return_probs=False: the same labels and scores
    none, ti, ts = pred(x, site, return_probs=False)
    assert none is None and torch.equal(ti, top_idx) and same_bits(ts, top_score)


@pytest.mark.parametrize("classes", [7, 200, 301])
def test_rows_do_not_depend_on_batch_size_or_position(classes):
    """dta_meta_predict on the same 70 HSI score rows: one call equals calls on rows 0..63 and 64..69, and the scalar-site call
    equals the per-row call with a constant tensor, bit for bit."""
    from deeptreeattention_amd.engine import MetadataPredictor
    sites, n = 4, 70
    m = small_model(12, classes, sites, seed=3)
    pred = MetadataPredictor(m)
    x = torch.from_numpy(prng.uniform01(61, 1, (n, 12, 11, 11))).to(dev())
    site = torch.from_numpy(prng.randint(61, 2, (n,), sites).astype(np.int64)).to(dev())
    scores = pred.sensor.logits_of(x).clone()
    ws = pred.table()

    def run(rows, s):
        k = rows.stop - rows.start
        f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=dev())
        out, probs, ti, ts = f(k, classes), f(k, classes), torch.full((k, 2), 9, dtype=torch.int64, device=dev()), f(k, 2)
        pred.head(scores[rows], k, ws, s[rows] if isinstance(s, torch.Tensor) else s, out, probs, ti, ts)
        return out, probs, ti, ts
    whole = run(slice(0, n), site)
    parts = [run(slice(0, 64), site), run(slice(64, n), site)]
    for a, b0, b1 in zip(whole, *parts):
        assert same_bits(a, torch.cat([b0, b1]))
    const = torch.full((n,), 2, dtype=torch.int64, device=dev())
    for a, b in zip(run(slice(0, n), 2), run(slice(0, n), const)):
        assert same_bits(a, b)
    check_self_consistent(*whole[1:])


def test_modes_state_and_trainer_updates():
    """Eval-mode whatever the module's flag says; no buffer of the model is written; a live predictor follows
    MetadataTrainer's in-place updates; a frozen one keeps the table and the sensor's re-layouts until refresh()."""
    from deeptreeattention_amd.engine import MetadataPredictor, MetadataTrainer
    classes, sites, n = 7, 4, 9
    m = small_model(12, classes, sites, seed=8)
    x = torch.from_numpy(prng.uniform01(71, 1, (n, 12, 11, 11))).to(dev())
    site = torch.from_numpy(prng.randint(71, 2, (n,), sites).astype(np.int64)).to(dev())
    y = torch.from_numpy(prng.randint(71, 3, (n,), classes).astype(np.int64)).to(dev())
    pred = MetadataPredictor(m)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ev = clones(pred(x, site))
    m.train()
    tr_mode = clones(pred(x, site))
    for a, b in zip(ev, tr_mode):
        assert same_bits(a, b)
    after = m.state_dict()
    for k, v in before.items():
        assert same_bits(v, after[k]), k
    assert int(after["metadata_model.batch_norm.num_batches_tracked"]) == int(before["metadata_model.batch_norm.num_batches_tracked"])

    tr = MetadataTrainer(m, lr=1e-2)
    live, frozen = MetadataPredictor(m), MetadataPredictor(m, frozen=True)
    live0, frozen0 = clones(live(x, site)), clones(frozen(x, site))
    for a, b, c in zip(ev, live0, frozen0):           # (the trainer moved the parameters: same values, new addresses)
        assert same_bits(a, b) and same_bits(a, c)
    # tensors written behind torch's back, as the fused trainers write them (raw pointers, no version counter moves): what a
    # frozen predictor KEEPS -- the table (embedding, site linear, both halves of fc1) and a conv weight's re-layout
    def poke(t, f):
        alias = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), t.storage_offset(), t.shape, t.stride())
        alias.mul_(f)
    with torch.no_grad():
        for t, f in ((m.fc1.weight, 1.5), (m.metadata_model.embedding.weight, -0.5), (m.metadata_model.mlp.weight, 2.0),
                     (m.sensor_model.spectral_network.conv2.conv_layer.weight, 0.5)):
            poke(t, f)
    kept = clones(frozen(x, site))
    for a, b in zip(frozen0, kept):
        assert same_bits(a, b)
    assert not same_bits(live(x, site)[0], live0[0])
    frozen.refresh()
    for a, b in zip(live(x, site), frozen(x, site)):
        assert same_bits(a, b)
    # one train step: the live predictor equals a freshly constructed one and differs from before; the frozen one (stale table
    # and re-layouts) does not equal them until refresh()
    live1 = clones(live(x, site))
    tr.train_step(x, site, y)
    live2 = clones(live(x, site))
    fresh = clones(MetadataPredictor(m)(x, site))
    for a, b in zip(live2, fresh):
        assert same_bits(a, b)
    assert not same_bits(live2[0], live1[0])
    assert not same_bits(frozen(x, site)[0], fresh[0])
    frozen.refresh()
    for a, b in zip(frozen(x, site), fresh):
        assert same_bits(a, b)
    # predict_step follows the trainer's updates too, and hands the ids through
    ids, p = tr.predict_step((["a"] * n, {"HSI": x, "site": site}))
    assert ids == ["a"] * n and same_bits(p, fresh[0])
    tr.close()


def test_refusals():
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd.engine import MetadataPredictor, Predictor
    m = small_model(12, 5, 4, seed=1)
    with pytest.raises(TypeError):
        MetadataPredictor(m.sensor_model)
    with pytest.raises(TypeError):
        Predictor(m)                                   # unchanged: the plain Predictor still refuses the fusion model
    pred = MetadataPredictor(m)
    x = torch.zeros(3, 12, 11, 11, device=dev())
    with pytest.raises(ValueError):
        pred(x, 4)
    with pytest.raises(ValueError):
        pred(x, -1)
    with pytest.raises(ValueError):
        pred(x, torch.zeros(2, dtype=torch.int64))


def dense_case():
    h, w, bands_raw = 17, 13, 40
    u = prng.uniform01(81, 1, (bands_raw, h, w))
    raw = (u * 9000 - 800).astype(np.int16)
    raw[:, h // 2, w // 3] = raw[0, h // 2, w // 3]              # one constant pixel
    from deeptreeattention_amd.dense import window_origins
    # one window per pixel of three boxes, the second one empty; the windows hang over every edge of the raster
    origins, offsets = window_origins([(-6, -6, 8, w), (3, 3, 3, 9), (8, -6, h, w)], anchor="corner")
    return raw, origins, offsets


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dense_route_equals_predictor_on_gathered_windows(precision):
    """predict_windows_metadata on a 40-raw-band 17 x 13 int16 raster equals MetadataPredictor on the explicitly gathered
    windows (same batch partition) with a constant site tensor, bit for bit: the float32 batch for the fp32 model, its own
    PatchTiles route for the bf16 model.  Crowns: crown_reduce on the same probabilities, one crown empty."""
    from deeptreeattention_amd.dense import (DenseRaster, crown_reduce, predict_map_metadata, predict_windows_metadata,
                                             raster_precision, window_origins)
    from deeptreeattention_amd.engine import MetadataPredictor
    classes, sites, site, batch = 7, 4, 2, 150
    raw, origins, offsets = dense_case()
    n = len(origins)
    m = small_model(20, classes, sites, seed=5, precision=precision)
    pred = MetadataPredictor(m)
    assert raster_precision(pred.sensor) == precision
    ras = DenseRaster(raw, precision=precision, device=dev())
    res = predict_windows_metadata(pred, ras, site, origins, crown_offsets=offsets, batch_size=batch, return_probs=True)
    ref = MetadataPredictor(m)
    probs = torch.empty(n, classes, dtype=torch.float32, device=dev())
    idx = torch.empty(n, 2, dtype=torch.int64, device=dev())
    score = torch.empty(n, 2, dtype=torch.float32, device=dev())
    for n0 in range(0, n, batch):
        n1 = min(n0 + batch, n)
        wins = ras.windows(origins[n0:n1], tiles=precision == "bf16")
        probs[n0:n1], idx[n0:n1], score[n0:n1] = ref(wins, torch.full((n1 - n0,), site, dtype=torch.int64, device=dev()))
    assert same_bits(res.probs, probs) and torch.equal(res.top_idx, idx) and same_bits(res.top_score, score)
    check_self_consistent(res.probs, res.top_idx, res.top_score)
    crowns = crown_reduce(probs, offsets)
    for a, b in zip(res.crowns, crowns):
        assert same_bits(a, b)
    assert res.crowns.count.cpu().tolist() == np.diff(offsets).tolist() and int(res.crowns.count[1]) == 0
    assert res.crowns.top_idx[1].cpu().tolist() == [-1, -1]
    lean = predict_windows_metadata(pred, ras, site, origins, batch_size=batch)
    assert lean.probs is None and lean.crowns is None and torch.equal(lean.top_idx, idx) and same_bits(lean.top_score, score)
    # the map: the reshaped top-1 of one window per pixel
    labels, scores = predict_map_metadata(pred, raw, site, anchor="center", batch_size=batch)
    o, _ = window_origins([(0, 0, 17, 13)], anchor="center")
    want = predict_windows_metadata(pred, ras, site, o, batch_size=batch)
    assert labels.shape == (17, 13) and torch.equal(labels, want.top_idx[:, 0].reshape(17, 13))
    assert same_bits(scores, want.top_score[:, 0].reshape(17, 13))
    with pytest.raises(ValueError):
        predict_windows_metadata(pred, ras, sites, origins)
    with pytest.raises(TypeError):
        predict_windows_metadata(m, ras, site, origins)


def test_trainer_predict_step_returns_the_golden_probabilities(full_fp32):
    from deeptreeattention_amd.engine import MetadataTrainer
    g, m, x, site, probs, top_idx, top_score, fused = full_fp32
    tr = MetadataTrainer(m, lr=1e-3)
    try:
        ids = ["id%d" % i for i in range(B)]
        got_ids, p = tr.predict_step((ids, {"HSI": x, "site": site}))
        assert got_ids is ids
        assert same_bits(p, probs)
        assert rel_l2(p.cpu().numpy(), softmax64(g["eval/out"])) < 1e-3
    finally:
        tr.close()
