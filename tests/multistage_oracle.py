"""Per-level float64 oracle of the multi-stage train step (reference multi_stage.py:277-288 per level: learned_ensemble ->
weighted F.cross_entropy -> backward; :258-262 one Adam per level), shared by tests/test_multistage_oracle_cpu.py (which
ties it to the reference's golden) and tests/test_multistage_oracle_gpu.py (which holds the one-chain step to it).
Plain NumPy on oracle/: test infrastructure, never imported by the product path."""
import contextlib
import functools

import numpy as np

from oracle import hang2020_np as O
from oracle import prng
from oracle.recipes import multistage_weight

# The smallest shapes that still reach the chain's other launch plans (capi.hip): `wide` -- 15 networks on 11x11 at B = 29
# take the fp32-input first conv (8 workgroups x 15 >= 100; 14 networks still do), more deferred parameter-gradient GEMMs
# than one grouped launch holds, two optimizer launches, head GEMMs of 2..201 columns; `crops24` -- 576-row workgroups, the
# wide-window weight-gradient pair, the lean 24x24 stage kernels, 4 x 27 = 108 workgroups fused, 3 x 27 = 81 packed;
# `sixteen` -- the most networks one chain takes, 17 bands (a chunk with 15 padded channels).  B = 29 / 27 / 7: ragged last
# conv workgroup.  missing[step] = (level, year) whose batch tensor is all-zero in that step.
CASES = {
    "wide": dict(seed=9100, hw=11, bands=24, years=3, classes=(2, 3, 12, 37, 201), B=29, steps=2,
                 missing={0: (1, 2), 1: (3, 0)}, lrs=(1e-3, 2e-3, 5e-4, 1e-3, 1e-3)),
    "crops24": dict(seed=9200, hw=24, bands=20, years=2, classes=(5, 130), B=27, steps=2,
                    missing={0: (0, 1)}, lrs=(1e-3, 2e-3)),
    "sixteen": dict(seed=9300, hw=11, bands=17, years=4, classes=(3, 5, 7, 9), B=7, steps=1,
                    missing={}, lrs=(1e-3, 1e-3, 1e-3, 1e-3)),
}


# A ReLU input or the two largest entries of a max-pool window closer than this (BatchNorm outputs: unit scale) are decided by
# float32 rounding, not by the operation: a 3x3 conv over up to 64 channels sums 576 products, whose float32 random-walk
# error is sqrt(576) * 2^-24 = 1.4e-6.
TAU = 2e-6


def _near_decisions(year_cache, attention=False):
    """The ReLU / max-pool decisions of one network's forward that float32 rounding can take the other way:
    [(layer, "relu", index)] and [(layer, "pool", window index, runner-up slot)]; attention=True: also the ReLUs inside the
    attention blocks, [(layer, "att:<cache key>", index)] (spectral: h0; spatial: m0, t1p -- sums of 32..128 products of
    unit-scale factors, the same rounding scale)."""
    out = []
    for L, (cc, _, _) in enumerate(year_cache["layers"]):
        v = cc["v"]
        out += [(L, "relu", idx) for idx in zip(*np.nonzero(np.abs(v) < TAU))]
        if cc["pool"]:
            r = np.maximum(v, 0)
            B, C, H, W = r.shape
            ho, wo = H // 2, W // 2
            xc = r[:, :, :ho * 2, :wo * 2].reshape(B, C, ho, 2, wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, ho, wo, 4)
            order = np.argsort(xc, axis=-1, kind="stable")
            top = np.take_along_axis(xc, order[..., 3:], -1)[..., 0]
            second = np.take_along_axis(xc, order[..., 2:3], -1)[..., 0]
            for idx in zip(*np.nonzero((top - second < TAU) & (second > 0))):
                out.append((L, "pool", idx, int(order[idx][2])))
    if attention:
        for L, (_, ac, _) in enumerate(year_cache["layers"]):
            for key in ("h0", "m0", "t1p"):
                if key in ac:
                    out += [(L, "att:" + key, idx) for idx in zip(*np.nonzero(np.abs(ac[key]) < TAU))]
    return out


def _toggled(year_cache, dec):
    """Context: the cache with one decision taken the other way (restored on exit)."""
    @contextlib.contextmanager
    def ctx():
        att = dec[1].startswith("att:")      # (the backward reads only the sign of a ReLU input)
        cc = year_cache["layers"][dec[0]][1 if att else 0]
        key, idx = (dec[1][4:], dec[2]) if att else ("v", dec[2]) if dec[1] == "relu" else ("arg", dec[2])
        old = cc[key][idx]
        cc[key][idx] = dec[3] if dec[1] == "pool" else (-1.0 if old > 0 else 1.0)
        try:
            yield
        finally:
            cc[key][idx] = old
    return ctx()


def level_oracle(p, imgs, y, w, bf16=False):
    """One level's forward, weighted cross-entropy and backward in float64 (bf16=True: with the kernels' bf16 roundings,
    O.bf16_mode).  -> (scores, loss, {name: gradient} of the kept years, {name: BatchNorm buffer after the step})."""
    if bf16:
        O.bf16_mode(True)
    try:
        scores, cache, upd = O.learned_ensemble_fwd(p, imgs, True, np.float64)
        loss, dl = O.weighted_cross_entropy(scores, y, w)
        g = O.learned_ensemble_bwd(p, cache, dl.astype(np.float64), np.float64)
    finally:
        if bf16:
            O.bf16_mode(False)
    return scores, float(loss), g, upd


@functools.lru_cache(maxsize=None)
def near_alternatives(case, step, level, yy):
    """[{name: gradient change}]: what each near decision (_near_decisions) of network (level, yy) of the float64 trajectory
    would add to the network's gradient when taken the other way.  The backward pass is linear in the incoming gradient,
    so any float32 evaluation of the same network computes trajectory grads + the sum of a SUBSET of these changes, up to
    rounding: one element of ~10^5..10^6 moves the first conv's gradient tensors by ~1 / sqrt(elements) = 1.4e-3..3e-3, more
    than the 1e-3 every tensor is held to, and at 24x24 some network of a step has such an element more often than not (in
    the oracle's own float32 evaluation too).  Computed only for a network that needs it (a forward and one backward per
    near decision of that network)."""
    o = trajectory(case, False)[step][level]
    imgs, y = case_inputs(case, step, level)
    kept = sum(bool(a.any()) for a in imgs)
    _, dl = O.weighted_cross_entropy(o["scores"], y, multistage_weight(CASES[case]["classes"][level]))
    pre = f"year_models.{yy}."
    _, yc, _ = O.subnet_fwd(o["before"], pre, "spectral", imgs[yy], True, np.float64)
    out = []
    for dec in _near_decisions(yc):
        with _toggled(yc, dec):
            other = O.subnet_bwd(o["before"], pre, yc, [None, None, dl.astype(np.float64) / kept], np.float64)
        out.append({k: other[k] - o["grads"][k] for k in other})
    return out


def resolve_near_decisions(got, grads, alts):
    """grads + the subset of `alts` (one network's near decisions, near_alternatives) that the float32 run `got` took the other
    way: least squares over all tensors but the conv biases, rounded to 0 / 1.  -> ({name: gradient}, the 0 / 1 vector)."""
    names = [k for k in alts[0] if not k.endswith("conv_layer.bias") and np.any(grads[k])]
    J = np.stack([np.concatenate([a[k].ravel() for k in names]) for a in alts], axis=1)
    r = np.concatenate([(np.asarray(got[k], np.float64) - grads[k]).ravel() for k in names])
    s = np.clip(np.rint(np.linalg.lstsq(J, r, rcond=None)[0]), 0, 1)
    out = dict(grads)
    for a, on in zip(alts, s):
        if on:
            for k, v in a.items():
                out[k] = out[k] + v
    return out, s


def case_params(case, level):
    c = CASES[case]
    return O.init_params(O.learned_ensemble_spec(c["years"], c["bands"], c["classes"][level]), seed=700 + level)


def case_inputs(case, step, level, B=None):
    """(year tensors, labels) of one level's batch (B: another batch size than the case's); the case's missing year is an
    all-zero tensor (reference year.py:27)."""
    c = CASES[case]
    B = B or c["B"]
    seed = c["seed"] + 10 * level + step
    imgs = [prng.uniform01(seed, yy, (B, c["bands"], c["hw"], c["hw"])) for yy in range(c["years"])]
    if c["missing"].get(step, (None, None))[0] == level:
        yy = c["missing"][step][1]
        imgs[yy] = np.zeros_like(imgs[yy])
    return imgs, prng.randint(seed, 7, (B,), c["classes"][level])


def year_of(name):
    return int(name.split(".")[1])      # "year_models.<y>. ..."


def oracle_adam(p, g, states, lr, betas=(0.9, 0.999), eps=1e-8):
    """One Adam state per year (a year without a gradient is passed over: no moment decay, no step, as torch's Adam passes
    over grad-None parameters).  Conv biases under batch-statistics BatchNorm have a zero gradient analytically; the
    oracle's 1e-17 noise there would become +-lr steps, so it is zeroed."""
    for yy, st in enumerate(states):
        gy = {k: (np.zeros_like(v) if k.endswith("conv_layer.bias") else v) for k, v in g.items() if year_of(k) == yy}
        if gy:
            p = O.adam_step(p, gy, st, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps)
    return p


@functools.lru_cache(maxsize=None)
def trajectory(case, bf16):
    """The oracle's own run of the case: out[step][level] = dict(before = the level's state dict the step starts from,
    scores, loss, grads, upd).  Computed once per (case, precision) and shared by the tests -- read-only.  The tests load
    `before` into the device models ahead of every step, so that each step is compared from identical parameters (Adam's
    first steps are lr * sign(g): after one of them two float trajectories sit 1e-3 apart, which is what this file must
    not depend on)."""
    c = CASES[case]
    ps = [case_params(case, l) for l in range(len(c["classes"]))]
    states = [[dict() for _ in range(c["years"])] for _ in c["classes"]]
    out = []
    for step in range(c["steps"]):
        row = []
        for l, classes in enumerate(c["classes"]):
            imgs, y = case_inputs(case, step, l)
            scores, loss, g, upd = level_oracle(ps[l], imgs, y, multistage_weight(classes), bf16)
            row.append(dict(before=ps[l], scores=scores, loss=loss, grads=g, upd=upd))
            nxt = oracle_adam(ps[l], g, states[l], c["lrs"][l])
            nxt.update(upd)
            ps[l] = nxt
        out.append(row)
    return out


def scale_deviation(got, want):
    """| ||got|| / ||want|| - 1 | over all tensors of `want` but the conv biases: what a wrong 1 / kept, class-weight
    normaliser or dscore routing moves, and what Adam (m / sqrt(v): invariant under g -> c g) hides."""
    a = b = 0.0
    for k, v in want.items():
        if k.endswith("conv_layer.bias"):
            continue
        a += float((np.asarray(got[k], np.float64) ** 2).sum())
        b += float((np.asarray(v, np.float64) ** 2).sum())
    return abs(np.sqrt(a) / np.sqrt(b) - 1.0)
