"""Cases, inputs, cached float64 oracle runs and probe definitions of the fp32 train step at bench-scale batches, shared by
tests/test_fp32_large_batch_cpu.py (which checks, from the oracle alone, that the probes are attainable and row-specific)
and tests/test_fp32_large_batch_gpu.py (which holds the kernels to them).  Plain NumPy on oracle/: test infrastructure,
never imported by the product path.  Everything cached here is shared between tests -- read-only.

Which launch-plan decision each case reaches (fp32, 11x11; read from deeptreeattention_amd/csrc):

  stage.hip, launch_stage_fwd / launch_stage_bwd: `pipe` = two patches per workgroup from B >= 512, grid (B + 1) / 2, second
      patch guarded by b1 < B.  `below_pipe` (511) is the last batch with one patch per workgroup, `pipe_odd` / `pipe_aligned`
      / `ensemble` (513) the first odd batch with pairs: 256 full pairs and a lone last patch.
  conv.hip, conv_geometry (MWG from conv_mwg: 512 rows for 32 / 64 columns, 256 for 128): 512 / 121 = 4 patches per
      workgroup in the first two convs, 256 / 25 = 10 in the third.  511 = 127 * 4 + 3 = 51 * 10 + 1, 513 = 128 * 4 + 1 =
      51 * 10 + 3: the last workgroup of every conv launch is ragged in every case.
  capi.hip, build_plan (weight-gradient slabs): S = 512 / (channel groups * launch groups), rounded down to a multiple of 8,
      at most B.  Hang2020: 512 / 256 / 128 slabs -- B = 511 is under the first conv's 512 (one patch per slab, 511 slabs),
      B = 513 over it (512 slabs, patches dealt unevenly).  Ensemble of 3: 168 / 168 / 80 on the device gate (three launch
      groups), 256 / 256 / 128 under host flags (two).  The other thresholds (128, 168, 256) lie below every case; batches
      under them are what the small-batch files run (B = 4 .. 64).
  heads.hip, gemm_auto_ksplit (K = B for the head and attention weight gradients, capi.hip backward driver): at most
      ceil(B / 128) K slices -- 4 at 511, 5 at 513; gemm_planned_ksplit: wave-tile GEMMs (16-byte loadable rows) do not
      split across workgroups up to K = 8192.  7-class score rows (28 bytes) take the element-wise loads, 12-class rows
      (48 bytes) the vector / wave-tile forms; 5-class rows (ensemble) the element-wise ones again.
  capi.hip, forward driver: eval mode derives the BatchNorm coefficients inside the stage workgroups while a conv launch
      has at most BN_INKERNEL_MAX_NWG = 512 workgroups -- B <= 2048 at 4 per workgroup, beyond the suite's largest fp32
      batch; fused_input (>= 100 first-conv workgroups) is bf16 only; the fan-in switches (read_switches: DTA_FANIN, DTA_LEAD)
      default to 0, so BatchNorm sums take the finalize launches at every batch.
  capi.hip, build_plan: 17 bands = two 16-channel chunks, the second with 15 padded channels (`pipe_aligned`).
  conv.hip / stage.hip grouped launches: gridDim.y = 3 for the ensemble on the device gate (year 1 all-zero, gated off).

So 511 and 513 straddle every batch threshold of the fp32 plan at or under B = 1031 that the small-batch files do not already
sit under; no further batch is needed."""
import functools

import numpy as np

from oracle import hang2020_np as O
from oracle import prng

HW = 11
CASES = {
    "below_pipe": dict(net="hang", bands=20, classes=7, B=511, seed=5200),
    "pipe_odd": dict(net="hang", bands=20, classes=7, B=513, seed=5290),
    "pipe_aligned": dict(net="hang", bands=17, classes=12, B=513, seed=5421),
    "ensemble": dict(net="ensemble", years=3, missing=1, bands=12, classes=5, B=513, seed=5162),
}
# SEEDS.  Chosen from the oracle alone, never from a device run: counting up in tens from 5110 / 5130 / 5131 / 5132, the first
# seed at which (a) the oracle accumulating in float32 sits within an eighth of the 1e-3 bound of its float64 run on every
# tensor of the whole-batch gradient and within a fifth on every judged tensor of every probe (the CPU file asserts a quarter),
# (b) no judged tensor of a probe is all-zero (the spatial attention of the third stage is ReLU-dead in about one patch of
# ten, and a probe of such a row says nothing about its parameters) and (c) every judged tensor is row-specific.  Most seeds
# miss (a): the gradients of the attention blocks' biases are sums over the batch that nearly cancel, and one ReLU decision
# that float32 takes the other way moves them by 1e-3 and more.  A class-weight probe takes the first class c* from 1 up
# that meets (a) - (c) (CW_CLASS).
HANG_CASES = tuple(k for k, c in CASES.items() if c["net"] == "hang")

# What the restated plan arithmetic below must give per case (pinned by tests/test_fp32_large_batch_cpu.py):
# patches per stage workgroup, stage grid, conv workgroups per layer, patches in the last conv workgroup per layer,
# first-conv weight-gradient slabs, K slices of the head weight-gradient GEMMs.
PLAN = {
    "below_pipe": dict(stage_ppw=1, stage_grid=511, conv_wg=(128, 128, 52), conv_tail=(3, 3, 1), slabs0=511, ksplit=4),
    "pipe_odd": dict(stage_ppw=2, stage_grid=257, conv_wg=(129, 129, 52), conv_tail=(1, 1, 3), slabs0=512, ksplit=5),
    "pipe_aligned": dict(stage_ppw=2, stage_grid=257, conv_wg=(129, 129, 52), conv_tail=(1, 1, 3), slabs0=512, ksplit=5),
    "ensemble": dict(stage_ppw=2, stage_grid=257, conv_wg=(129, 129, 52), conv_tail=(1, 1, 3), slabs0=168, ksplit=5),
}


# ---- plan arithmetic restated (stage.hip: pipe; conv.hip: conv_geometry, conv_mwg; capi.hip: build_plan) ----
CONV_PPW = (512 // (HW * HW), 512 // (HW * HW), 256 // ((HW // 2) ** 2))      # 4, 4, 10


def stage_ppw(B):
    return 2 if B >= 512 else 1


def stage_grid(B):
    return (B + 1) // 2 if B >= 512 else B


def conv_wg(B):
    return tuple((B + p - 1) // p for p in CONV_PPW)


def conv_tail(B):
    """Patches in the last workgroup of each conv launch."""
    return tuple(B - (B - 1) // p * p for p in CONV_PPW)


def slabs0(case):
    """First conv's weight-gradient slabs: Hang2020's two branches are one launch of 64 columns (one channel group, one
    launch group); an ensemble year has 32 columns, one channel group per 128 padded input channels, a launch group per year."""
    c = CASES[case]
    S = 512 if c["net"] == "hang" else 512 // c["years"]
    if S >= 8:
        S &= ~7
    return min(S, c["B"])


def ksplit(B):
    return (B + 127) // 128      # gemm_auto_ksplit: 128 / tiles >= this for every head and attention GEMM of these shapes


def interior_row(B):
    """A row that is neither first nor last in its 4-patch and its 10-patch conv workgroup, and the second patch of a pair."""
    r = B // 2 + 1
    while not (r % 4 in (1, 2) and 1 <= r % 10 <= 8 and r % 2 == 1):
        r += 1
    return r


def last_conv1_rows(B):
    """The rows of the last first-conv workgroup: B - B % 4 .. B - 1."""
    return tuple(range(B - B % 4, B))


# ---- inputs ----
def class_weights(classes):
    return (0.1 + (np.arange(classes) % 7)).astype(np.float32)      # tests/test_hip_parity.py


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(parameters, x -- a list of year tensors for the ensemble --, labels, class weights)."""
    c = CASES[case]
    B, seed = c["B"], c["seed"]
    y = prng.randint(seed, 2, (B,), c["classes"])
    w = class_weights(c["classes"])
    if c["net"] == "hang":
        p = O.init_params(O.hang2020_spec(c["bands"], c["classes"]), seed=seed + 1)
        return p, prng.uniform01(seed, 1, (B, c["bands"], HW, HW)), y, w
    p = O.init_params(O.learned_ensemble_spec(c["years"], c["bands"], c["classes"]), seed=seed + 1)
    imgs = [prng.uniform01(seed, 10 + yy, (B, c["bands"], HW, HW)) for yy in range(c["years"])]
    imgs[c["missing"]] = np.zeros_like(imgs[c["missing"]])
    return p, imgs, y, w


def _fwd(case, dt):
    p, x, _, _ = inputs(case)
    fwd = O.hang2020_fwd if CASES[case]["net"] == "hang" else O.learned_ensemble_fwd
    return fwd(p, x, True, dt)


def _bwd(case, cache, d, dt):
    p = inputs(case)[0]
    bwd = O.hang2020_bwd if CASES[case]["net"] == "hang" else O.learned_ensemble_bwd
    return bwd(p, cache, d.astype(dt), dt)


@functools.lru_cache(maxsize=None)
def _forward(case, dt):
    scores, cache, upd = _fwd(case, dt)
    return dict(scores=scores, cache=cache, upd=upd)


def forward(case, dt=np.float64):
    """The oracle's training-mode forward of the case: dict(scores, cache, upd) -- one per (case, precision)."""
    return _forward(case, dt)


def whole_batch(case, dt=np.float64):
    """Weighted cross-entropy and backward of the whole batch on forward(case): dict(loss, dl, grads)."""
    return _whole_batch(case, dt)


@functools.lru_cache(maxsize=None)
def _whole_batch(case, dt):
    f = forward(case, dt)
    _, _, y, w = inputs(case)
    loss, dl = O.weighted_cross_entropy(f["scores"], y, w)
    return dict(loss=float(loss), dl=dl, grads=_bwd(case, f["cache"], dl, dt))


@functools.lru_cache(maxsize=None)
def eval_scores(case):
    """Eval-mode scores on the same batch after the training-mode forward's BatchNorm update (Hang2020 cases)."""
    p, x, _, _ = inputs(case)
    p2 = dict(p)
    p2.update(forward(case)["upd"])
    return O.hang2020_fwd(p2, x, False, np.float64)[0]


# ---- row probes: a score gradient that is zero except in chosen rows ----
def probe_rows(case):
    """{probe name: rows}.  At B = 513 the last first-conv workgroup holds the last row alone: `conv1_tail` is then a second,
    independent draw on that row."""
    B = CASES[case]["B"]
    return {"row0": (0,), "last": (B - 1,), "pair_second": (B - 2,), "interior": (interior_row(B),),
            "conv1_tail": last_conv1_rows(B)}


PROBES = ("row0", "last", "pair_second", "interior", "conv1_tail")


def neighbour(rows):
    """The same rows one patch earlier (one later when that would leave the batch)."""
    s = 1 if min(rows) == 0 else -1
    return tuple(r + s for r in rows)


def probe_d(case, probe, rows=None):
    """(B, classes) float64, uniform in +-1 / B (the size of a cross-entropy gradient row) in the probe's rows -- or in `rows`,
    with the same values."""
    c = CASES[case]
    own = probe_rows(case)[probe]
    v = prng.uniform(c["seed"] + 7, 100 + PROBES.index(probe), (len(own), c["classes"]), -1.0, 1.0).astype(np.float64) / c["B"]
    d = np.zeros((c["B"], c["classes"]))
    d[list(rows or own)] = v
    return d


def probe_grads(case, probe, dt=np.float64, shifted=False):
    """Oracle gradient of the probe on the cached forward (shifted: the values in the neighbouring rows)."""
    return _probe_grads(case, probe, dt, shifted)


@functools.lru_cache(maxsize=None)
def _probe_grads(case, probe, dt, shifted):
    rows = probe_rows(case)[probe]
    d = probe_d(case, probe, neighbour(rows) if shifted else rows)
    return _bwd(case, forward(case, dt)["cache"], d, dt)


# ---- class-weight probes: the weighted cross-entropy itself is nonzero in the probed rows alone ----
def cw_probe_rows(case):
    B = CASES[case]["B"]
    return {"cw_last": (B - 1,)} if CASES[case]["net"] == "ensemble" else {"cw_last": (B - 1,), "cw_pair_second": (B - 2,)}


# The class c* of a class-weight probe (see SEEDS above).
CW_CLASS = {("below_pipe", "cw_last"): 2, ("below_pipe", "cw_pair_second"): 1, ("pipe_odd", "cw_last"): 1,
            ("pipe_odd", "cw_pair_second"): 1, ("pipe_aligned", "cw_last"): 2, ("pipe_aligned", "cw_pair_second"): 1,
            ("ensemble", "cw_last"): 1}


def cw_inputs(case, probe, shifted=False):
    """(class weights, labels): the weight vector is zero except at class c*, and only the probed rows carry label c*."""
    c = CASES[case]
    rows = cw_probe_rows(case)[probe]
    if shifted:
        rows = neighbour(rows)
    star = CW_CLASS[(case, probe)]
    y = inputs(case)[2].copy()
    y[y == star] = (star + 1) % c["classes"]
    y[list(rows)] = star
    w = np.zeros(c["classes"], np.float32)
    w[star] = class_weights(c["classes"])[star]
    return w, y


def cw_oracle(case, probe, dt=np.float64, shifted=False):
    """dict(loss, dl, grads) of the class-weight probe on the cached forward (the forward does not see labels or weights)."""
    return _cw_oracle(case, probe, dt, shifted)


@functools.lru_cache(maxsize=None)
def _cw_oracle(case, probe, dt, shifted):
    f = forward(case, dt)
    w, y = cw_inputs(case, probe, shifted)
    loss, dl = O.weighted_cross_entropy(f["scores"], y, w)
    return dict(loss=float(loss), dl=dl, grads=_bwd(case, f["cache"], dl, dt))


# ---- near decisions of the whole-batch gradient (tests/multistage_oracle.py) ----
def networks(case):
    """[(parameter prefix, kind, the network's cache in forward(case)["cache"], its share of the score gradient)]."""
    c, cache = CASES[case], forward(case)["cache"]
    if c["net"] == "hang":
        return [("spectral_network.", "spectral", cache["spec"], cache["w"]), ("spatial_network.", "spatial", cache["spat"], 1 - cache["w"])]
    return [(f"year_models.{yy}.", "spectral", yc, 1.0 / cache["n"]) for yy, yc in enumerate(cache["years"]) if yc is not None]


def _reaches_gradient(yc, dec):
    """False for a conv-module ReLU decision whose element the following 2x2 max-pool does not pass on (not its window's
    maximum, or in the row / column the floor pool drops): no gradient arrives there, so taking it the other way changes
    nothing -- three near decisions of four in the pooled layers, each a backward saved."""
    L, kind, idx = dec[0], dec[1], dec[2]
    cc = yc["layers"][L][0]
    if kind != "relu" or not cc["pool"]:
        return True
    b, c, h, w = idx
    ho, wo = cc["arg"].shape[2:]
    return h < 2 * ho and w < 2 * wo and cc["arg"][b, c, h // 2, w // 2] == (h % 2) * 2 + (w % 2)


@functools.lru_cache(maxsize=None)
def near_alternatives(case, pre):
    """[{name: gradient change}] of network `pre`: what each ReLU / max-pool decision of the float64 forward that float32
    rounding can take the other way (multistage_oracle._near_decisions, the attention blocks' ReLUs included) adds to the
    whole-batch gradient when it is.  One backward of the network per decision; computed only when a comparison asks."""
    from multistage_oracle import _near_decisions, _toggled
    p, wb = inputs(case)[0], whole_batch(case)
    _, _, yc, share = next(n for n in networks(case) if n[0] == pre)
    out = []
    for dec in _near_decisions(yc, attention=True):
        if not _reaches_gradient(yc, dec):
            continue
        with _toggled(yc, dec):
            other = O.subnet_bwd(p, pre, yc, [None, None, wb["dl"].astype(np.float64) * share], np.float64)
        out.append({k: other[k] - wb["grads"][k] for k in other})
    return out


# ---- judging ----
def analytically_zero(name):
    return name.endswith("conv_layer.bias")      # under batch-statistics BatchNorm


# Tensors a probe does not judge because the oracle's gradient of the neighbouring row is closer than ten bounds to the
# probe's (an off-by-one in the row index would pass on them): at most two per probe, each under 1000 elements, pinned by
# tests/test_fp32_large_batch_cpu.py against the oracle.
#
# The two last-head biases are such tensors for every score-gradient probe: their gradient is the column sum of d, which does
# not know the row.  (A class-weight probe's d is the softmax of its row: there they are judged.)
_HEAD_BIASES = ("spectral_network.classifier3.fc1.bias", "spatial_network.classifier3.fc1.bias")
NOT_ROW_SPECIFIC = {(case, probe): _HEAD_BIASES for case in HANG_CASES for probe in PROBES}


def judged(case, probe, grads):
    """The tensor names of `grads` a probe is judged on."""
    out = NOT_ROW_SPECIFIC.get((case, probe), ())
    return [k for k in grads if not analytically_zero(k) and k not in out]

