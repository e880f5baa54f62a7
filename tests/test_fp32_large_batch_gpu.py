"""The float32 train step against the float64 oracle at the batches where its launch plan changes (tests/large_batch_cases.py:
B = 511 and 513 -- one and two patches per stage workgroup, ragged last conv workgroups, the first conv's weight-gradient
slab count on either side of the batch, 4 and 5 K slices in the batch GEMMs, element-wise and vector head GEMM forms, three
grouped years), through the nn.Module / autograd path, FusedTrainer and EnsembleTrainer.

A whole-batch rel-L2 at 1e-3 cannot see one lost patch of 513 (it moves the gradient tensors by about 1e-3 or less).  The
row probes can: a score gradient that is zero except in chosen rows -- the first, the last (the lone patch of the last pair
and of the ragged conv workgroups), the second patch of the last full pair, an interior one, the rows of the last first-conv
workgroup -- gives a gradient whose magnitude is carried by those rows, compared tensor by tensor with the oracle's backward
of the same score gradient.  The trainers compute their loss gradient themselves; there a class-weight vector that is zero
except at one class, with that class as the label of the probed rows only, makes the weighted cross-entropy's own gradient
nonzero in those rows alone.  tests/test_fp32_large_batch_cpu.py shows from the oracle alone that every probe is attainable
in float32 and would not pass with the row index off by one.

Measured on an MI355X (worst per check; below_pipe / pipe_odd / pipe_aligned):
  1 forward            logits 5.8e-7 / 9.4e-7 / 6.3e-7, loss 1.4e-7 / 1.8e-7 / 9.9e-9, BatchNorm statistics 4.3e-8 / 3.4e-8 /
                       2.8e-8, eval logits 1.5e-7 / 1.9e-7 / 1.2e-7
  2 whole batch        gradient tensor 7.0e-6 / 2.0e-5 / 1.0e-4, branch scale 1.6e-7 / 1.8e-7 / 5.0e-8; near decisions taken the
                       other way: none / 1 of 2 (spatial) / 2 of 8 (spectral) + 1 of 3 (spatial) -- what one costs: at seed
                       5190 of pipe_odd's shape the gate bias of the first spectral attention sat 9.84e-4 from the float64
                       decisions' gradient, and one alternative of that network moves exactly that tensor by 9.8e-4
  3 row probes         row0 2.0e-5 / 6.8e-5 / 4.2e-5, last 2.0e-4 / 2.0e-5 / 2.0e-4, pair_second 1.6e-4 / 5.2e-6 / 1.7e-4,
                       interior 2.8e-4 / 2.6e-5 / 8.8e-5, conv1_tail 5.1e-5 / 8.4e-5 / 9.2e-5 -- the worst tensor of a probe is
                       nearly always a one-element bias of a spatial-attention stencil; the large tensors sit at 1e-6
  4 FusedTrainer step  loss 2.0e-8 / 7.6e-8 / 1.1e-7, logits as in 1, gradient tensor 1.0e-5 / 3.6e-6 / 8.7e-5, scale 1.2e-7 /
                       8.3e-8 / 8.6e-8, Adam 0.21 / 0.22 / 0.21 of its bound
  5 class-weight       cw_last 6.3e-4 / 9.7e-5 / 3.5e-5, cw_pair_second 1.2e-4 / 2.1e-5 / 3.0e-4, loss <= 1.7e-7
  6 ensemble           scores 1.1e-6, loss 4.7e-8, gradient tensor 1.6e-6 (device gate and host flags; year 0: 1 of 6 near
                       decisions taken the other way), year scale 4.9e-8, cw_last probe 1.2e-6 (loss 2.0e-7)
No test takes more than 4 s; the file 30 s, nearly all of it the NumPy oracle."""
import functools

import numpy as np
import pytest
import torch

import large_batch_cases as LB
from conftest import rel_l2
from multistage_oracle import resolve_near_decisions, scale_deviation
from oracle import hang2020_np as O
from test_hip_parity import compare_grads, grads_of

pytestmark = pytest.mark.gpu
FP32_TIGHT, FP32_TOL = 2e-4, 1e-3      # tests/test_hip_parity.py
LR = 1e-3
# float32 kernels sit 1e-6..1e-5 from the float64 oracle on most gradient tensors; when one is further off than this the
# network's near decisions are looked at (large_batch_cases.near_alternatives), as tests/test_multistage_oracle_gpu.py does
NEAR_TRIGGER = 1e-4

def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _hang(case):
    from deeptreeattention_amd import Hang2020 as H
    c = LB.CASES[case]
    m = H.Hang2020(c["bands"], c["classes"], precision="fp32")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in LB.inputs(case)[0].items()})
    return m.to(dev()).train()


def _ensemble(case):
    from deeptreeattention_amd.year import learned_ensemble
    c = LB.CASES[case]
    m = learned_ensemble(years=c["years"], classes=c["classes"], config={"pretrain_state_dict": None, "bands": c["bands"]})
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in LB.inputs(case)[0].items()})
    return m.to(dev()).train()


def _snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _branches(grads):
    """{network prefix: its tensors}: the networks whose gradient scale is judged one by one."""
    out = {}
    for k, v in grads.items():
        if k == "alpha":
            continue
        pre = k.split(".")[0] if not k.startswith("year_models.") else ".".join(k.split(".")[:2])
        out.setdefault(pre, {})[k] = v
    return out


def _resolved(case, got, ref):
    """The whole-batch oracle gradient with the ReLU / max-pool decisions that float32 rounding took the other way than float64
    (within multistage_oracle.TAU of the threshold) taken the device's way: at B = 513 a network has a dozen such elements,
    and one of them moves single small tensors -- sums over the batch that nearly cancel -- by 1e-3.  Same bounds after."""
    out, note = dict(ref), []
    for pre, *_ in LB.networks(case):
        names = [k for k in ref if k.startswith(pre) and not LB.analytically_zero(k) and np.any(ref[k])]
        if all(rel_l2(got[k], ref[k]) < NEAR_TRIGGER for k in names):
            continue
        alts = LB.near_alternatives(case, pre)
        if alts:
            fixed, taken = resolve_near_decisions(got, {k: np.asarray(ref[k], np.float64) for k in ref if k.startswith(pre)}, alts)
            out.update(fixed)
            note.append(f"{pre} {len(alts)} near decisions, {int(taken.sum())} taken the other way")
    return out, "; ".join(note)


def _check_scales(got, want, tag):
    worst = 0.0
    for pre, ref in _branches(want).items():
        sd = scale_deviation(got, ref)
        worst = max(worst, sd)
        assert sd < FP32_TOL, (tag, pre, sd)
    return worst


def _check_probe(got, ref, names, tag):
    """Every judged tensor of a probe at FP32_TOL; the analytically zero ones stay rounding-sized against the rest."""
    worst = (0.0, None)
    gmax = max(float(np.abs(np.asarray(ref[k])).max()) for k in names)
    for k in ref:
        assert got[k] is not None, (tag, k)
        if LB.analytically_zero(k):
            assert float(np.abs(got[k]).max()) <= 1e-4 * max(gmax, 1.0), (tag, k)
            continue
        if k not in names:
            continue
        e = rel_l2(got[k], ref[k])
        worst = max(worst, (e, k))
        assert e < FP32_TOL, (tag, k, e)
    return worst


# ---- the module path: m(x), F.cross_entropy(weight=w), backward -- one forward graph per case, kept for the probes ----
@functools.lru_cache(maxsize=None)
def _module_run(case):
    p, x, y, w = LB.inputs(case)
    m = _hang(case)
    logits = m(_t(x))
    loss = torch.nn.functional.cross_entropy(logits, _t(y), weight=_t(w))
    return dict(m=m, logits=logits, loss=loss, after_train=_snapshot(m))


def _module_backward(case, seed_grad=None):
    r = _module_run(case)
    r["m"].zero_grad(set_to_none=True)
    if seed_grad is None:
        r["loss"].backward(retain_graph=True)
    else:
        r["logits"].backward(_t(seed_grad.astype(np.float32)), retain_graph=True)
    return grads_of(r["m"])


@pytest.mark.parametrize("case", LB.HANG_CASES)
def test_module_forward_vs_oracle(case):
    """Check 1: train-mode logits, loss, every BatchNorm running statistic and step count, then eval-mode logits on the same
    batch, at FP32_TIGHT."""
    r = _module_run(case)
    o, wb = LB.forward(case), LB.whole_batch(case)
    e_s = rel_l2(r["logits"].detach().cpu().numpy(), o["scores"])
    e_l = abs(r["loss"].item() - wb["loss"]) / wb["loss"]
    assert e_s < FP32_TIGHT and e_l < FP32_TIGHT, (case, e_s, e_l)
    e_b = 0.0
    assert len(o["upd"]) == 18
    for k, v in o["upd"].items():
        if k.endswith("num_batches_tracked"):
            assert int(r["after_train"][k]) == int(v) == 1, k
            continue
        e = rel_l2(r["after_train"][k], v)
        e_b = max(e_b, e)
        assert e < FP32_TIGHT, (case, k, e)
    m = r["m"]
    m.eval()
    try:
        with torch.no_grad():
            ev = m(_t(LB.inputs(case)[1])).cpu().numpy()
    finally:
        m.train()
    e_e = rel_l2(ev, LB.eval_scores(case))
    assert e_e < FP32_TIGHT, (case, e_e)
    print(f"{case} module forward: logits {e_s:.2e} loss {e_l:.2e} BatchNorm statistics {e_b:.2e} eval logits {e_e:.2e}")


@pytest.mark.parametrize("case", LB.HANG_CASES)
def test_module_whole_batch_gradients_vs_oracle(case):
    """Check 2: every gradient tensor at FP32_TOL by the rules of test_hip_parity.compare_grads (conv biases analytically
    zero, the unused heads without a gradient), and each branch's gradient scale."""
    got = _module_backward(case)
    ref, note = _resolved(case, got, LB.whole_batch(case)["grads"])
    for k in ("classifier1", "classifier2"):
        for br in ("spectral_network", "spatial_network"):
            assert got[f"{br}.{k}.fc1.weight"] is None and got[f"{br}.{k}.fc1.bias"] is None
    worst = compare_grads(got, ref, FP32_TOL)
    sc = _check_scales(got, ref, case)
    print(f"{case} module whole-batch gradients: worst {worst[0]:.2e} {worst[1]}  scale {sc:.2e}  [{note}]")


@pytest.mark.parametrize("probe", LB.PROBES)
@pytest.mark.parametrize("case", LB.HANG_CASES)
def test_module_row_probe_vs_oracle(case, probe):
    """Check 3: a further backward through the kept forward graph from a score gradient that is zero except in the probe's
    rows, against O.hang2020_bwd of the same score gradient on the cached oracle forward."""
    got = _module_backward(case, LB.probe_d(case, probe))
    ref = LB.probe_grads(case, probe)
    worst = _check_probe(got, ref, LB.judged(case, probe, ref), (case, probe))
    print(f"{case} module probe {probe} rows {LB.probe_rows(case)[probe]}: worst {worst[0]:.2e} {worst[1]}")


# ---- FusedTrainer: the one-chain step with the fused forward tail and the in-kernel cross-entropy ----
def _trainer_grads(tr, m):
    got = {k: tr.grad_of(prm).detach().cpu().numpy().copy() for k, prm in m.named_parameters() if prm.dtype == torch.float32}
    if getattr(tr, "hang", False):
        got["alpha"] = np.float64(tr.alpha_g.item())
    return got


def _fused_step(case, w, y):
    from deeptreeattention_amd.engine import FusedTrainer
    m = _hang(case)
    tr = FusedTrainer(m, lr=LR, loss_weight=torch.from_numpy(w), keep_grads=True)
    before = _snapshot(m)
    loss = tr.train_step(_t(LB.inputs(case)[1]), _t(y)).item()
    return m, tr, before, loss


@pytest.mark.parametrize("case", LB.HANG_CASES)
def test_fused_trainer_step_vs_oracle(case):
    """Check 4: one FusedTrainer step -- loss, logits, every gradient and alpha's, each branch's scale, BatchNorm buffers --
    against the whole-batch oracle; then the parameters after the step against Adam in float64 on the device's own gradient
    (the C ABI's float betas and rate), at the bound tests/test_multistage_oracle_gpu.py uses for that comparison."""
    _, _, y, w = LB.inputs(case)
    m, tr, before, loss = _fused_step(case, w, y)
    o, wb = LB.forward(case), LB.whole_batch(case)
    e_l = abs(loss - wb["loss"]) / wb["loss"]
    e_s = rel_l2(tr.logits.cpu().numpy(), o["scores"])
    assert e_l < FP32_TIGHT and e_s < FP32_TIGHT, (case, e_l, e_s)
    got = _trainer_grads(tr, m)
    ref, note = _resolved(case, got, wb["grads"])
    for k in got:
        if "classifier1" in k or "classifier2" in k:
            assert not np.any(got[k]), k      # heads unused by Hang2020.forward
    worst = compare_grads(got, ref, FP32_TOL)
    sc = _check_scales(got, ref, case)
    after = _snapshot(m)
    for k, v in o["upd"].items():
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == 1, k
        else:
            assert rel_l2(after[k], v) < FP32_TIGHT, (case, k)
    # Adam, isolated from the gradient
    names = [k for k in got]
    p0 = {k: before[k].astype(np.float64) for k in names}
    p1 = O.adam_step(p0, {k: np.asarray(got[k], np.float64) for k in names}, {}, lr=float(np.float32(LR)),
                     beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)))
    err = dref = pn = 0.0
    for k in names:
        d_dev, d_ref = after[k].astype(np.float64) - p0[k], p1[k] - p0[k]
        err += float(((d_dev - d_ref) ** 2).sum()); dref += float((d_ref ** 2).sum()); pn += float((p0[k] ** 2).sum())
    # the update is rounded into p once (<= 2^-24 |p| per element) and takes about 8 float32 roundings itself (5e-7)
    bound = 2.0 ** -23 * np.sqrt(pn) + 1e-6 * np.sqrt(dref)
    assert dref > 0 and np.sqrt(err) <= bound, (case, np.sqrt(err), bound)
    print(f"{case} FusedTrainer step: loss {e_l:.2e} logits {e_s:.2e} worst gradient {worst[0]:.2e} {worst[1]}  scale {sc:.2e}  "
          f"Adam error / bound {np.sqrt(err) / bound:.2f}  [{note}]")


@pytest.mark.parametrize("probe", ["cw_last", "cw_pair_second"])
@pytest.mark.parametrize("case", LB.HANG_CASES)
def test_fused_trainer_class_weight_probe_vs_oracle(case, probe):
    """Check 5: a fresh trainer whose class weights and labels leave the cross-entropy gradient nonzero in the probed rows
    alone: loss and every judged gradient at FP32_TOL."""
    w, y = LB.cw_inputs(case, probe)
    m, tr, _, loss = _fused_step(case, w, y)
    o = LB.cw_oracle(case, probe)
    e_l = abs(loss - o["loss"]) / o["loss"]
    assert e_l < FP32_TOL, (case, probe, e_l)
    worst = _check_probe(_trainer_grads(tr, m), o["grads"], LB.judged(case, probe, o["grads"]), (case, probe))
    print(f"{case} FusedTrainer probe {probe} rows {LB.cw_probe_rows(case)[probe]}: loss {e_l:.2e} worst {worst[0]:.2e} {worst[1]}")


# ---- EnsembleTrainer: three grouped years, year 1 all-zero ----
def _ensemble_step(w, y, use_present):
    from deeptreeattention_amd.engine import EnsembleTrainer
    c = LB.CASES["ensemble"]
    imgs = LB.inputs("ensemble")[1]
    present = [yy != c["missing"] for yy in range(c["years"])]
    m = _ensemble("ensemble")
    tr = EnsembleTrainer(m, lr=LR, loss_weight=torch.from_numpy(w), keep_grads=True)
    before = _snapshot(m)
    loss = float(tr.train_step([_t(a) for a in imgs], _t(y), present if use_present else None))
    return m, tr, before, loss, present


@pytest.mark.parametrize("use_present", [False, True])
def test_ensemble_trainer_step_vs_oracle(use_present):
    """Check 6: one EnsembleTrainer step against O.learned_ensemble_fwd / _bwd in float64, with the missing year decided on
    the device (present=None: all three years launched, gridDim.y = 3) and by host flags (two years launched): scores, loss,
    every kept year's gradient tensors and scale, BatchNorm buffers, and the skipped year's untouched parameters and
    statistics."""
    _, _, y, w = LB.inputs("ensemble")
    m, tr, before, loss, present = _ensemble_step(w, y, use_present)
    o, wb = LB.forward("ensemble"), LB.whole_batch("ensemble")
    e_s = rel_l2(tr.scores.cpu().numpy(), o["scores"])
    e_l = abs(loss - wb["loss"]) / wb["loss"]
    assert e_s < FP32_TIGHT and e_l < FP32_TIGHT, (use_present, e_s, e_l)
    got, after = _trainer_grads(tr, m), _snapshot(m)
    ref, note = _resolved("ensemble", got, wb["grads"])
    worst, live = (0.0, None), 0
    for k in got:
        yy = int(k.split(".")[1])
        if not present[yy] or "classifier1" in k or "classifier2" in k:
            assert not np.any(got[k]), k      # a skipped year, the heads year.py:30 does not use: no gradient
            assert k not in ref, k
            continue
        if LB.analytically_zero(k):
            assert np.abs(got[k]).max() < 1e-4, k
            continue
        e = rel_l2(got[k], ref[k])
        worst = max(worst, (e, k))
        live += 1
        assert e < FP32_TOL, (use_present, k, e)
    assert live == 2 * 23 and set(ref) <= set(got)      # per kept year: 9 conv / BatchNorm, 12 attention, 2 head tensors
    sc = _check_scales(got, ref, use_present)
    skipped = f"year_models.{LB.CASES['ensemble']['missing']}."
    for k in after:
        if k.startswith(skipped):
            assert np.array_equal(after[k], before[k]), k      # not stepped, BatchNorm untouched (reference year.py:27-28)
    assert len(o["upd"]) == 9 * sum(present)
    for k, v in o["upd"].items():
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(v) == 1, k
        else:
            assert rel_l2(after[k], v) < FP32_TIGHT, k
    assert tr.step_counts() == [int(f) for f in present]
    print(f"ensemble {'host flags' if use_present else 'device gate'}: scores {e_s:.2e} loss {e_l:.2e} worst gradient "
          f"{worst[0]:.2e} {worst[1]}  scale {sc:.2e}  [{note}]")


def test_ensemble_trainer_class_weight_probe_vs_oracle():
    """The class-weight probe of the last row through the grouped launches (device gate)."""
    w, y = LB.cw_inputs("ensemble", "cw_last")
    m, tr, _, loss, present = _ensemble_step(w, y, False)
    o = LB.cw_oracle("ensemble", "cw_last")
    e_l = abs(loss - o["loss"]) / o["loss"]
    assert e_l < FP32_TOL, e_l
    got = _trainer_grads(tr, m)
    worst = _check_probe(got, o["grads"], LB.judged("ensemble", "cw_last", o["grads"]), "ensemble cw_last")
    for k in got:
        if k not in o["grads"]:
            assert not np.any(got[k]), k
    print(f"ensemble probe cw_last: loss {e_l:.2e} worst {worst[0]:.2e} {worst[1]}")
