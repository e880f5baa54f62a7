"""The first conv once per raster on the device (dense.predict_windows(share_conv1=True); csrc/dense_conv1.hip): the table
against its float64 host definition, the gather as a bit-exact copy, the fp32 and bf16 routes end to end against the torch
oracle (float64) on explicitly sliced and preprocessed windows, single branches, repeatability, crowns, maps, refusals.
All fixtures are synthetic (oracle.prng); the oracle's probabilities of the shared case are computed once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O
from oracle import hang2020_torch as OT
from oracle import preprocess_np as PP
from oracle import prng

pytestmark = pytest.mark.gpu

FP32_TIGHT = 2e-4      # tests/test_hip_parity.py: the eval-mode tolerance of the fp32 networks
HALF_TABLE = 1e-3      # bf16 mode: half storage rounds each element by <= 2^-11 = 4.9e-4 relative, the fp32 accumulation stays < 2e-4
HEAD_GAIN = 30.0
SEED = 61              # 20 bands, 300 windows: the oracle alone has no top-2 margin below 2e-4 (checked below, on the CPU)
CLASSES = 7


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def raw_raster(seed, bands, h, w):
    u = prng.uniform01(seed, 1, (bands, h, w))
    # a scene, not noise: each quadrant has its own spectral shape (a step at its own band), under 30 % noise
    kind = (np.arange(h)[:, None] >= h // 2) + 2 * (np.arange(w)[None, :] >= w // 2)
    edge = (bands * (1 + kind)) // 5
    shape = (np.arange(bands)[:, None, None] >= edge[None]).astype(np.float64)
    a = ((0.3 * u + 0.7 * shape) * 9000 - 800).astype(np.int16)
    a[:, h // 2, w // 3] = a[0, h // 2, w // 3]       # one constant pixel
    return a


def raw_windows(raw, origins, size=11):
    """What a boundless read of each window returns: slices of a zero-padded copy."""
    pad = 64
    Cb, Hh, Ww = raw.shape
    big = np.zeros((Cb, Hh + 2 * pad, Ww + 2 * pad), dtype=raw.dtype)
    big[:, pad:pad + Hh, pad:pad + Ww] = raw
    return [np.ascontiguousarray(big[:, r + pad:r + pad + size, c + pad:c + pad + size]) for r, c in np.asarray(origins)]


def params(kind, bands, classes, seed):
    spec = O.hang2020_spec(bands, classes) if kind == "hang" else O.subnet_spec(kind, bands, classes)
    p = O.init_params(spec, seed=seed)
    for k in p:      # running statistics a trained network would have; last heads that tell the classes apart
        if k.endswith("running_mean"):
            p[k] = (0.2 * (prng.uniform01(seed, 7, p[k].shape) - 0.5)).astype(np.float32)
        elif k.endswith("running_var"):
            p[k] = (0.5 + prng.uniform01(seed + 1, 9, p[k].shape)).astype(np.float32)
        elif k.endswith("classifier3.fc1.weight"):
            p[k] = (p[k] * HEAD_GAIN).astype(np.float32)
    return p


def model_of(kind, bands, classes, p, precision):
    from deeptreeattention_amd import Hang2020 as H
    m = {"hang": H.Hang2020, "spectral": H.spectral_network, "spatial": H.spatial_network}[kind](bands, classes, precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
    return m.to(dev()).eval()


def conv1_of(kind, p):
    """The first conv's weights and bias as the forward concatenates them: [spectral | spatial] for Hang2020."""
    pres = ("spectral_network.", "spatial_network.") if kind == "hang" else ("",)
    w = np.concatenate([p[pre + "conv1.conv_layer.weight"] for pre in pres], axis=0)
    b = np.concatenate([p[pre + "conv1.conv_layer.bias"] for pre in pres], axis=0)
    return w, b


def oracle_probs(kind, p, wins):
    """float64 torch oracle, eval mode, on oracle/preprocess_np.py windows: probabilities and the top-2 margin."""
    x = torch.from_numpy(np.stack([PP.preprocess_image(w) for w in wins])).double()
    with torch.no_grad():
        pt = {k: torch.from_numpy(np.array(v)) for k, v in p.items()}
        pt = {k: (v.double() if v.is_floating_point() else v) for k, v in pt.items()}
        scores = OT.hang2020(pt, x, training=False) if kind == "hang" else OT.subnet(pt, "", kind, x, False)[-1]
        pr = torch.softmax(scores, dim=1).numpy()
    top = np.sort(pr, axis=1)
    return pr, top[:, -1] - top[:, -2]


@functools.lru_cache(maxsize=None)
def shared_case(kind="hang"):
    """20 bands, seed 61, a 20x15 raster, one window per pixel (300) grouped into four crowns, the second empty; with the
    oracle's probabilities.  Built once per network kind and never modified."""
    from deeptreeattention_amd.dense import window_origins
    h, w = 20, 15
    raw = raw_raster(SEED, 40, h, w)
    boxes = [(0, 0, h // 2, w), (h // 2, 0, h // 2, w), (h // 2, 0, h, w // 2), (h // 2, w // 2, h, w)]
    origins, offsets = window_origins(boxes, anchor="center")
    p = params(kind, 20, CLASSES, SEED)
    want, margin = oracle_probs(kind, p, raw_windows(raw, origins))
    low = margin < FP32_TIGHT
    print(f"oracle ({kind}, seed {SEED}): {int(low.sum())} of {len(origins)} windows with a top-2 margin below {FP32_TIGHT}, "
          f"smallest margin {margin.min():.3e}")
    assert low.sum() <= 0.01 * len(origins)      # the cap holds for the oracle alone
    for a in (want, margin):
        a.setflags(write=False)
    return raw, origins, offsets, p, want, margin


def assert_same_bits(a, b, what):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


def held_to_the_oracle(res, want, margin, what):
    n = len(want)
    e = rel_l2(res.probs.cpu().numpy(), want)
    differ = res.top_idx[:, 0].cpu().numpy() != want.argmax(axis=1)
    low = margin < FP32_TIGHT
    print(f"{what}: probabilities vs the float64 oracle rel-L2 {e:.3e}; labels differing {int(differ.sum())}, oracle margins "
          f"below {FP32_TIGHT}: {int(low.sum())} of {n}")
    assert e <= FP32_TIGHT
    assert not (differ & ~low).any()
    assert differ.sum() <= 0.01 * n


# ---------------------------------------------------------------------------------------------------------------------
# 1. the table against the host definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["hang", "spectral"])
@pytest.mark.parametrize("h,w,bands", [(6, 5, 20), (17, 13, 20), (6, 5, 349)])
def test_table_equals_the_host_definition(h, w, bands, kind, precision):
    """fp32: rel-L2 <= 2e-4 against the float64 definition.  bf16: the definition on DenseRaster.float() and bf16-rounded
    weights, rel-L2 <= 1e-3 (half storage <= 4.9e-4 per element + fp32 accumulation < 2e-4).  The ring, the far-outside row
    and the interior are held separately."""
    from deeptreeattention_amd.dense import DenseRaster, conv1_table_np
    from deeptreeattention_amd.engine import Predictor
    p = params(kind, bands, 4, 73)
    model = model_of(kind, bands, 4, p, precision)
    ras = DenseRaster(raw_raster(79, bands + 20, h, w), precision=precision, device=dev())
    table = ras.conv1_table(Predictor(model))
    cols = 64 if kind == "hang" else 32
    assert table.cols == cols and tuple(table.data.shape) == ((h + 2) * (w + 2) + 1, 9, cols)
    assert table.data.dtype == (torch.float16 if precision == "bf16" else torch.float32)
    wgt, bias = conv1_of(kind, p)
    x = ras.float().cpu().numpy().astype(np.float64)
    if precision == "bf16":
        wgt = O.bf16_round(wgt)
    want = conv1_table_np(x, wgt.astype(np.float64), bias.astype(np.float64)).data
    got = table.data.cpu().numpy()
    bound = HALF_TABLE if precision == "bf16" else FP32_TIGHT
    grid = np.zeros((h + 2, w + 2), dtype=bool)
    grid[1:-1, 1:-1] = True
    inner = np.concatenate([grid.reshape(-1), [False]])
    ring = np.concatenate([~grid.reshape(-1), [False]])
    e_all, e_in, e_ring = rel_l2(got, want), rel_l2(got[inner], want[inner]), rel_l2(got[ring], want[ring])
    print(f"conv1 table {h}x{w}, {bands} bands, {kind}, {precision}: rel-L2 {e_all:.3e} (interior {e_in:.3e}, ring {e_ring:.3e})")
    assert e_all <= bound and e_in <= bound and e_ring <= bound
    # the ring is not the far row: its inward-looking classes see the raster
    assert not np.array_equal(got[0, 0], got[-1, 0])
    # the far-outside row is the bias alone, rounded once to the table's storage: exact
    far = bias.astype(got.dtype)
    assert np.array_equal(got[-1], np.broadcast_to(far, (9, cols)))
    # ring position (-1, -1), classes whose taps all stay on zero input (bottom row or right column of a window): the bias too
    for cls in (2, 5, 6, 7, 8):
        assert np.array_equal(got[0, cls], far), cls


# ---------------------------------------------------------------------------------------------------------------------
# 2. the gather is a copy
# ---------------------------------------------------------------------------------------------------------------------
def nineteen_origins(h, w):
    o = [(-5, -5), (-5, w - 6), (h - 6, -5), (h - 6, w - 6),                      # the four corners
         (-10, 1), (h - 1, 1), (1, -10), (1, w - 1), (-1, 0), (0, -1),            # each edge (by ten, and by one)
         (-13, 0), (0, -13), (h + 2, 0), (0, w + 2),                              # fully outside by two
         (-51, -51), (h + 40, w + 40), (-51, w + 40),                             # ... and by forty
         (0, 0), (max(h - 11, 0), max(w - 11, 0))]                                # the interior
    assert len(o) == 19
    return np.array(o, dtype=np.int32)


@pytest.mark.parametrize("kind,precision", [("hang", "bf16"), ("hang", "fp32"), ("spectral", "bf16"), ("spatial", "fp32")])
def test_gather_is_a_bit_exact_copy_of_the_table(kind, precision):
    from deeptreeattention_amd.dense import DenseRaster, gather_conv1_np
    from deeptreeattention_amd.engine import Predictor
    h, w, bands = 17, 13, 20
    p = params(kind, bands, 4, 83)
    model = model_of(kind, bands, 4, p, precision)      # (the Predictor holds its model weakly)
    pred = Predictor(model)
    ras = DenseRaster(raw_raster(89, bands + 20, h, w), precision=precision, device=dev())
    table = ras.conv1_table(pred)
    host = table.numpy()
    origins = nineteen_origins(h, w)
    out = torch.empty(len(origins), 121, table.cols, dtype=table.data.dtype, device=dev())
    table.gather(ras._origins(origins), out)
    want = gather_conv1_np(host, origins)
    bits = np.uint16 if precision == "bf16" else np.uint32
    assert np.array_equal(out.cpu().numpy().view(bits), want.view(bits))
    # a batch whose size is no multiple of the wave size, through the Predictor's workspace: y[0] after the whole batch
    n = 37
    o37 = np.stack([prng.randint(5, 1, (n,), h + 14) - 12, prng.randint(5, 2, (n,), w + 14) - 12], axis=1).astype(np.int32)
    slot = pred.conv1_slot(n, bands)
    assert slot.numel() == n * 121 * table.cols * table.data.element_size()
    table.gather(ras._origins(o37), slot)
    logits = pred.logits_from_conv1()
    assert tuple(logits.shape) == (n, 4) and bool(torch.isfinite(logits).all())
    y0 = slot.cpu().numpy().view(bits).reshape(n, 121, table.cols)
    assert np.array_equal(y0, gather_conv1_np(host, o37).view(bits))


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. the routes end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_route_against_the_oracle():
    """Probabilities of predict_windows(share_conv1=True) against oracle/hang2020_torch.py (float64) on
    oracle/preprocess_np.py windows within 2e-4 norm-wise; labels may differ only where the oracle's own top-2 margin is
    below that, in at most 1 % of the windows."""
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    raw, origins, offsets, p, want, margin = shared_case("hang")
    model = model_of("hang", 20, CLASSES, p, "fp32")
    ras = DenseRaster(raw, precision="fp32", device=dev())
    res = predict_windows(model, ras, origins, batch_size=128, return_probs=True, share_conv1=True)
    held_to_the_oracle(res, want, margin, "fp32 Hang2020, shared first conv")
    # and the existing route (gather + full forward) lands in the same place
    old = predict_windows(model, ras, origins, batch_size=128, return_probs=True)
    print(f"shared first conv vs the existing fp32 route: rel-L2 {rel_l2(res.probs.cpu().numpy(), old.probs.cpu().numpy()):.3e}")
    assert torch.equal(res.top_idx[:, 0].cpu(), old.top_idx[:, 0].cpu())


def test_bf16_route_against_the_oracle_with_the_tile_route_as_yardstick():
    """bf16 Hang2020: the new route's rel-L2 to the float64 oracle <= max(1e-2, 1.5 x the existing tile route's rel-L2 to
    the same oracle) -- the project's bf16 rule with the existing route as the yardstick."""
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    raw, origins, offsets, p, want, margin = shared_case("hang")
    model = model_of("hang", 20, CLASSES, p, "bf16")
    ras = DenseRaster(raw, precision="bf16", device=dev())
    old = predict_windows(model, ras, origins, batch_size=128, return_probs=True)
    new = predict_windows(model, ras, origins, batch_size=128, return_probs=True, share_conv1=True)
    e_old, e_new = rel_l2(old.probs.cpu().numpy(), want), rel_l2(new.probs.cpu().numpy(), want)
    differ = int((new.top_idx[:, 0] != old.top_idx[:, 0]).sum())
    print(f"bf16 Hang2020 vs the float64 oracle: tile route rel-L2 {e_old:.3e}, shared first conv {e_new:.3e}; "
          f"labels differing between the routes: {differ} of {len(origins)}")
    assert e_new <= max(1e-2, 1.5 * e_old)


@pytest.mark.parametrize("kind", ["spectral", "spatial"])
def test_single_branch_fp32_route_against_the_oracle(kind):
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    raw, origins, offsets, p, want, margin = shared_case(kind)
    model = model_of(kind, 20, CLASSES, p, "fp32")
    res = predict_windows(model, DenseRaster(raw, precision="fp32", device=dev()), origins, batch_size=128, return_probs=True,
                          share_conv1=True)
    held_to_the_oracle(res, want, margin, f"fp32 {kind}_network, shared first conv")


# ---------------------------------------------------------------------------------------------------------------------
# 6. repeatability and flow
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reruns_crowns_and_maps(precision):
    from deeptreeattention_amd.dense import DenseRaster, crown_reduce_np, predict_map, predict_windows, window_origins
    from deeptreeattention_amd.engine import Predictor
    raw, origins, offsets, p, want, margin = shared_case("hang")
    h, w = raw.shape[1:]
    model = model_of("hang", 20, CLASSES, p, precision)
    pred = Predictor(model)
    ras = DenseRaster(raw, precision=precision, device=dev())
    a = predict_windows(pred, ras, origins, crown_offsets=offsets, batch_size=128, return_probs=True, share_conv1=True)
    b = predict_windows(pred, ras, origins, crown_offsets=offsets, batch_size=128, return_probs=True, share_conv1=True)
    assert_same_bits(a.probs, b.probs, "probabilities of two runs")
    assert torch.equal(a.top_idx.cpu(), b.top_idx.cpu())
    assert_same_bits(a.top_score, b.top_score, "top-2 scores of two runs")
    for x, y in zip(a.crowns, b.crowns):
        assert torch.equal(x.cpu(), y.cpu())
    # crown offsets flow through unchanged: the crowns are crown_reduce_np of this route's own window probabilities
    mean, top_idx, top_score, count = crown_reduce_np(a.probs.cpu().numpy(), offsets)
    assert np.array_equal(a.crowns.mean.cpu().numpy().view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(a.crowns.top_idx.cpu().numpy(), top_idx)
    assert np.array_equal(a.crowns.top_score.cpu().numpy().view(np.uint32), top_score.view(np.uint32))
    assert a.crowns.count.cpu().tolist() == np.diff(offsets).tolist()
    assert count[1] == 0 and a.crowns.top_idx[1].cpu().tolist() == [-1, -1] and bool((a.crowns.mean[1] == 0).all())
    assert bool((a.crowns.top_score[1] == 0).all())
    # a full forward in between (same Predictor, same workspace) leaves the route's results as they were
    predict_windows(pred, ras, origins[:50], batch_size=128)
    c = predict_windows(pred, ras, origins, batch_size=128, return_probs=True, share_conv1=True)
    assert_same_bits(a.probs, c.probs, "probabilities after a full forward on the same workspace")
    # the map over all pixels, from the raw array and in other batch sizes: a window's bits do not depend on its batch
    labels, scores = predict_map(pred, raw, anchor="center", batch_size=77, share_conv1=True)
    all_o, _ = window_origins([(0, 0, h, w)], anchor="center")
    res = predict_windows(pred, ras, all_o, batch_size=77, share_conv1=True)
    assert labels.shape == (h, w) and labels.dtype == torch.int64 and scores.dtype == torch.float32
    assert torch.equal(labels.cpu(), res.top_idx[:, 0].reshape(h, w).cpu())
    assert_same_bits(scores, res.top_score[:, 0].reshape(h, w), "score map")
    sub_l, _ = predict_map(pred, ras, anchor="center", rows=(3, 9), cols=(2, 15), share_conv1=True)
    assert torch.equal(sub_l.cpu(), labels[3:9, 2:15].cpu())


def test_a_weight_update_between_calls_is_followed():
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    raw, origins, offsets, p, want, margin = shared_case("hang")
    model = model_of("hang", 20, CLASSES, p, "fp32")
    ras = DenseRaster(raw, precision="fp32", device=dev())
    before = predict_windows(model, ras, origins[:64], return_probs=True, share_conv1=True).probs.clone()
    with torch.no_grad():
        model.spectral_network.conv1.conv_layer.weight.mul_(1.5)
        model.spatial_network.conv1.conv_layer.bias.add_(0.25)
    new = predict_windows(model, ras, origins[:64], return_probs=True, share_conv1=True).probs
    old_route = predict_windows(model, ras, origins[:64], return_probs=True).probs
    assert not torch.equal(before.cpu(), new.cpu())
    assert rel_l2(new.cpu().numpy(), old_route.cpu().numpy()) <= FP32_TIGHT


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd import _lib, dense
    from deeptreeattention_amd.engine import Predictor
    from deeptreeattention_amd.year import learned_ensemble
    raw, origins, offsets, p, want, margin = shared_case("hang")
    r32 = dense.DenseRaster(raw, precision="fp32", device=dev())
    r16 = dense.DenseRaster(raw, precision="bf16", device=dev())
    m32 = model_of("hang", 20, CLASSES, p, "fp32")
    m16 = model_of("hang", 20, CLASSES, p, "bf16")
    torch.cuda.synchronize()
    launched = torch.cuda.memory_allocated()       # every refusal comes before the table (its first allocation) is built

    def refused(match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
        assert torch.cuda.memory_allocated() == launched

    torch.manual_seed(5)
    ens = learned_ensemble(3, CLASSES, {"pretrain_state_dict": None, "bands": 20}).to(dev()).eval()
    van = H.vanilla_CNN(20, CLASSES, precision="fp32").to(dev()).eval()
    launched = torch.cuda.memory_allocated()
    refused("year ensemble", lambda: dense.predict_windows(ens, [r32, None, r32], origins, share_conv1=True))
    refused("year ensemble", lambda: dense.predict_map(ens, [r32, None, r32], share_conv1=True))
    refused("vanilla_CNN", lambda: dense.predict_windows(van, r32, origins, share_conv1=True))
    m32.train()
    refused("training mode", lambda: dense.predict_windows(m32, r32, origins, share_conv1=True))
    m32.eval()
    refused("precision='fp32'", lambda: dense.predict_windows(m32, r16, origins, share_conv1=True))
    refused("precision='bf16'", lambda: dense.predict_windows(m16, r32, origins, share_conv1=True))
    refused("window side 7", lambda: r32.conv1_table(Predictor(m32), size=7))
    monkeypatch.setattr(dense, "WINDOW", 7)
    refused("window side 7", lambda: dense.predict_windows(m32, r32, origins, share_conv1=True))
    monkeypatch.undo()
    # the C entry: a training-mode or a non-FORWARD_ONLY descriptor is answered with a message, nothing is launched
    L = _lib.lib()
    nets = (_lib.SubnetParams * 2)()
    ws = torch.zeros(64, dtype=torch.uint8, device=dev())
    for training, heads in ((1, 4 | _lib.FORWARD_ONLY), (0, 4)):
        d = _lib.NetDesc(8, 20, 11, 11, CLASSES, _lib.NET_HANG2020, _lib.DTA_F32, training, heads, 0.1, 1e-5)
        assert L.dta_conv1_forward(C.byref(d), nets, None, _lib.ptr(ws), None, _lib.ptr(ws), None) != 0
        assert L.dta_last_error().decode() == "dta_conv1_forward: eval mode (training == 0) with DTA_FORWARD_ONLY only"
