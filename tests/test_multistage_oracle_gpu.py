"""The one-chain multi-stage train step (MultiStageTrainer.training_step_all: dta_multistage_forward_loss,
dta_multistage_backward, dta_adam_step_multi -- the step the reference's train.py runs) held to the per-level float64 oracle
of tests/multistage_oracle.py: scores, loss, EVERY GRADIENT (element-wise and by its scale, which Adam's m / sqrt(v) hides
from every comparison of parameters), BatchNorm buffers, step counts, and the optimizer isolated from the gradient -- at the
smallest shapes that reach the chain's other launch plans (multistage_oracle.CASES).  Then dta_adam_step_multi alone
against its float64 statement."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from multistage_oracle import (CASES, case_inputs, case_params, near_alternatives, resolve_near_decisions, scale_deviation,
                               trajectory, year_of)
from oracle import hang2020_np as O
from oracle import prng
from oracle.recipes import multistage_weight

pytestmark = pytest.mark.gpu
FP32_TIGHT, FP32_TOL = 2e-4, 1e-3      # tests/test_hip_parity.py
# float32 kernels sit 1e-6..1e-5 from the float64 oracle on every gradient tensor; one that is further off than this has the
# network's near decisions looked at (multistage_oracle.near_alternatives)
NEAR_TRIGGER = 1e-4


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _load(m, sd):
    """In place: the trainers' flat buffers and pointer tables stay valid."""
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})


def _build(case, prec, lrs=None):
    from deeptreeattention_amd.engine import MultiStageTrainer
    from deeptreeattention_amd.year import learned_ensemble
    c = CASES[case]
    models, ws = [], []
    for l, classes in enumerate(c["classes"]):
        m = learned_ensemble(years=c["years"], classes=classes, config={"pretrain_state_dict": None, "bands": c["bands"]})
        _load(m, case_params(case, l))
        for net in m.year_models:
            net.precision = prec
        models.append(m.to(dev()).train())
        ws.append(torch.from_numpy(multistage_weight(classes)))
    return models, MultiStageTrainer(models, list(lrs or c["lrs"]), ws, keep_grads=True)


def _batch(case, step, B=None):
    batch, present = [], []
    for l in range(len(CASES[case]["classes"])):
        imgs, y = case_inputs(case, step, l, B)
        present.append([bool(a.any()) for a in imgs])
        batch.append((None, {"HSI": [torch.from_numpy(a).to(dev()) for a in imgs]}, torch.from_numpy(y).to(dev())))
    return batch, present


def _snapshot(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _grads(tr, m):
    return {k: tr.grad_of(prm).double().cpu().numpy() for k, prm in m.named_parameters()}


def _whole(got, want):
    """rel-L2 of the whole gradient vector of one network (all tensors of `want` but the conv biases)."""
    num = den = 0.0
    for k, v in want.items():
        if k.endswith("conv_layer.bias"):
            continue
        num += float(((got[k] - v) ** 2).sum()); den += float((v ** 2).sum())
    return np.sqrt(num / den)


def _norm_dev(a, b):
    return abs(np.linalg.norm(a) - np.linalg.norm(b)) / np.linalg.norm(b)


def _yardstick(chain, serial, floor=1e-2):
    """The project's bf16 rule with the existing route as the yardstick: within max(floor, 1.5 x what the level-by-level
    route sits from the same bf16-mode oracle)."""
    return chain <= max(floor, 1.5 * serial)


def _run(case, prec, use_present):
    c = CASES[case]
    bf16 = prec == "bf16"
    traj = trajectory(case, bf16)
    nl, years = len(c["classes"]), c["years"]
    models, driver = _build(case, prec)
    twin_models, twin = _build(case, prec) if bf16 else (None, None)
    adam = [[dict() for _ in range(years)] for _ in range(nl)]      # float64 Adam fed the device's own gradients
    counts = [[0] * years for _ in range(nl)]
    worst_g, worst_scale, worst_adam = (0.0, None), (0.0, None), 0.0
    for step in range(c["steps"]):
        batch, present = _batch(case, step)
        for l in range(nl):
            _load(models[l], traj[step][l]["before"])
            if twin:
                _load(twin_models[l], traj[step][l]["before"])
        before = [_snapshot(m) for m in models]
        losses = driver.training_step_all(batch, step, present if use_present else None)
        assert driver.batched_last
        if twin:
            t_losses = [twin.training_step(batch, step, l, present[l] if use_present else None) for l in range(nl)]
        for l in range(nl):
            o, m, tr, tag = traj[step][l], models[l], driver.levels[l], (case, prec, use_present, step, l)
            scores, loss = tr.scores.cpu().numpy(), float(losses[l])
            got, after = _grads(tr, m), _snapshot(m)
            # ---- 1. scores and loss ----
            e_s, e_l = rel_l2(scores, o["scores"]), abs(loss - o["loss"]) / abs(o["loss"])
            if bf16:
                t_got = _grads(twin.levels[l], twin_models[l])
                s_s = rel_l2(twin.levels[l].scores.cpu().numpy(), o["scores"])
                s_l = abs(float(t_losses[l]) - o["loss"]) / abs(o["loss"])
                print(f"{tag} scores {e_s:.2e} (level by level {s_s:.2e})  loss {e_l:.2e} ({s_l:.2e})")
                assert _yardstick(e_s, s_s, 1e-3) and _yardstick(e_l, s_l, 1e-3), tag
            else:
                print(f"{tag} scores {e_s:.2e}  loss {e_l:.2e}")
                assert e_s < FP32_TIGHT and e_l < FP32_TIGHT, tag
            for yy in range(years):
                names = [k for k in got if year_of(k) == yy]
                state = [k for k in after if year_of(k) == yy]
                ytag = tag + (yy,)
                if not present[l][yy]:
                    # a skipped year (reference year.py:27-28): no gradient, nothing stepped, BatchNorm untouched
                    for k in names:
                        assert not np.any(got[k]), (ytag, k)
                    for k in state:
                        assert np.array_equal(after[k], before[l][k]), (ytag, k)
                    continue
                counts[l][yy] += 1
                # ---- 2. gradients ----
                ref_g = o["grads"]
                if not bf16 and any(rel_l2(got[k], ref_g[k]) >= NEAR_TRIGGER for k in names
                                    if np.any(ref_g.get(k, 0)) and not k.endswith("conv_layer.bias")):
                    # a ReLU / max-pool decision of this network that float32 rounding took the other way than float64
                    # (multistage_oracle.near_alternatives): the oracle with THAT decision is the yardstick -- same bounds
                    alts = near_alternatives(case, step, l, yy)
                    if alts:
                        ref_g, taken = resolve_near_decisions(got, ref_g, alts)
                        print(f"{ytag}: {len(alts)} near decisions, taken the other way: {int(taken.sum())}")
                live = {}
                for k in names:
                    ref = ref_g.get(k)
                    if ref is None or not np.any(ref):
                        assert not np.any(got[k]), (ytag, k)       # the heads year.py:30 does not use
                        continue
                    ref = np.asarray(ref, np.float64)
                    if k.endswith("conv_layer.bias"):
                        assert np.abs(got[k]).max() < 1e-4, (ytag, k)   # analytically zero under batch-statistics BatchNorm
                        continue
                    live[k] = ref
                    if not bf16:
                        e = rel_l2(got[k], ref)
                        if e > worst_g[0]:
                            worst_g = (e, ytag + (k,))
                        assert e < FP32_TOL, (ytag, k, e)
                assert len(live) > 20, ytag
                # ---- 3. the scale of the network's gradient ----
                dev_scale = scale_deviation(got, live)
                if dev_scale > worst_scale[0]:
                    worst_scale = (dev_scale, ytag)
                if bf16:
                    # ---- 4. the level-by-level route as the yardstick ----
                    w_c, w_s = _whole(got, live), _whole(t_got, live)
                    sc_s = scale_deviation(t_got, live)
                    print(f"{ytag} whole gradient vs bf16-mode oracle {w_c:.2e} (level by level {w_s:.2e})  scale {dev_scale:.2e} ({sc_s:.2e})")
                    if w_c > worst_g[0]:
                        worst_g = (w_c, ytag, w_s)
                    assert _yardstick(w_c, w_s), (ytag, w_c, w_s)
                    assert _yardstick(dev_scale, sc_s), (ytag, dev_scale, sc_s)
                    for k, ref in live.items():
                        if ref.size >= 1000:
                            assert _yardstick(_norm_dev(got[k], ref), _norm_dev(t_got[k], ref)), (ytag, k)
                else:
                    assert dev_scale < 1e-3, (ytag, dev_scale)
                # ---- 6. Adam, isolated from the gradient: the float64 statement fed the device's own gradient ----
                p0 = {k: before[l][k].astype(np.float64) for k in names}
                p1 = O.adam_step(p0, {k: got[k] for k in names}, adam[l][yy], lr=c["lrs"][l])
                err = dref = pn = 0.0
                for k in names:
                    d_dev, d_ref = after[k].astype(np.float64) - p0[k], p1[k] - p0[k]
                    err += float(((d_dev - d_ref) ** 2).sum()); dref += float((d_ref ** 2).sum()); pn += float((p0[k] ** 2).sum())
                # the update is rounded into p once (<= 2^-24 |p| per element) and takes about 8 float32 roundings itself (5e-7)
                bound = 2.0 ** -23 * np.sqrt(pn) + 1e-6 * np.sqrt(dref)
                worst_adam = max(worst_adam, np.sqrt(err) / bound)
                assert dref > 0 and np.sqrt(err) <= bound, (ytag, np.sqrt(err), bound)
            # ---- 5. BatchNorm buffers of the kept years ----
            for k, v in o["upd"].items():
                if k.endswith("num_batches_tracked"):
                    assert int(after[k]) == int(v), (tag, k)
                else:
                    assert rel_l2(after[k], v) < (1e-3 if bf16 else FP32_TIGHT), (tag, k)
            assert len(o["upd"]) == 9 * sum(present[l]), tag
            assert tr.step_counts() == counts[l], tag
    print(f"{case} {prec} present={'host' if use_present else 'device'}: worst gradient {worst_g}, worst scale deviation "
          f"{worst_scale}, Adam error / bound {worst_adam:.2f}")


@pytest.mark.parametrize("use_present", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_wide_chain_vs_oracle(prec, use_present):
    """5 levels x 3 years, classes 2 / 3 / 12 / 37 / 201, 24 bands, 11x11, B = 29, two steps (step 0: level 1 lacks year 2,
    step 1: level 3 lacks year 0), learning rates 1e-3 / 2e-3 / 5e-4 / 1e-3 / 1e-3: 15 (14 with host flags) networks in one
    chain -- the fp32-input first conv, a flush of the deferred parameter-gradient GEMMs inside the backward, two optimizer
    launches.  Measured on an MI355X (worst over levels, years and steps; the same with the device gate and with host flags):
    fp32: scores 6.4e-7, loss 8.2e-8, gradient tensor 1.9e-6 (one network -- step 1, level 1, year 0 -- has ONE near decision
    and took it the other way: its conv1.bn1.weight sits 9.1e-4 from the float64 decision's gradient), network scale
    1.3e-7, Adam 0.21 of its bound.  bf16, chain / level by level: whole gradient of a network vs the bf16-mode oracle
    9.54e-3 / 9.54e-3 (worst), scale 1.9e-4 / 1.9e-4, scores 1.4e-4 / 1.4e-4 -- the same kernels: equal to all printed digits."""
    _run("wide", prec, use_present)


@pytest.mark.parametrize("use_present", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_crops24_chain_vs_oracle(prec, use_present):
    """2 levels x 2 years, classes 5 / 130, 20 bands, 24x24 crops, B = 27, two steps (step 0: level 0 lacks year 1): 576-row
    workgroups, the wide-window weight-gradient pair and the lean 24x24 stage kernels in the chain; 4 x 27 = 108 first-conv
    workgroups take the fp32 input, the 3 x 27 = 81 of step 0 under host flags the pack route.  Measured on an MI355X
    (device gate = host flags): fp32: scores 2.2e-7, loss 4.9e-8, gradient tensor 3.6e-6, network scale 5.4e-8, Adam 0.20 of
    its bound; two networks (step 0 level 1 year 0: 5 near decisions, step 1 level 0 year 0: 3) took one first-conv ReLU
    decision the other way -- the ones the oracle's own float32 evaluation takes the other way, 2.4e-3 on conv1's weight
    gradient (tests/test_multistage_oracle_cpu.py).  bf16, chain / level by level: whole gradient 6.71e-3 / 6.71e-3, scale
    4.8e-5 / 4.8e-5, scores 3.4e-5 / 3.4e-5."""
    _run("crops24", prec, use_present)


def test_sixteen_networks_chain_vs_oracle():
    """4 levels x 4 years = the 16 networks one chain takes at most, classes 3 / 5 / 7 / 9, 17 bands (a chunk with 15 padded
    channels), B = 7, fp32, one step.  Measured on an MI355X: scores 6.1e-7, loss 1.1e-7, gradient tensor 1.5e-6, network
    scale 1.3e-7, Adam 0.21 of its bound."""
    _run("sixteen", "fp32", False)


# ---- behaviour: a frozen level, levels whose Adam settings differ (the `wide` models at B = 6, fp32) ----
def _same(ma, mb, tag):
    """Two runs of the same kernels on the same data in another grouping: float32 rounding of the reductions whose split
    depends on the group count (tests/test_multistage_gpu.py: 1e-5); conv biases -- gradient noise under BatchNorm -- apart."""
    for (k, p1), (_, p2) in zip(ma.state_dict().items(), mb.state_dict().items()):
        if k.endswith("conv_layer.bias"):
            continue
        if k.endswith("num_batches_tracked"):
            assert int(p1) == int(p2), (tag, k)
            continue
        assert rel_l2(p1.cpu().numpy(), p2.cpu().numpy()) < 1e-5, (tag, k)


@pytest.mark.parametrize("use_present", [False, True])
def test_a_level_with_learning_rate_zero_is_not_stepped_with_another_levels_rate(use_present):
    """lrs = (1e-3, 0, ...): after two chain steps level 1's parameters are bit-identical to the start (a segment rate of 0
    means the call's rate in dta_adam_step_multi, and the call's rate was level 0's), its moments and step counts are those
    of the level-by-level route (torch's Adam with lr = 0 still advances both), and the other levels are where a run
    without the freeze leaves them."""
    lrs = (1e-3, 0.0, 5e-4, 1e-3, 1e-3)
    ma, a = _build("wide", "fp32", lrs)
    mb, b = _build("wide", "fp32", lrs)
    mc, free = _build("wide", "fp32")
    start = _snapshot(ma[1])
    for step in range(2):
        batch, present = _batch("wide", step, B=6)
        pr = present if use_present else None
        a.training_step_all(batch, step, pr)
        assert a.batched_last
        for l in range(len(mb)):
            b.training_step(batch, step, l, None if pr is None else pr[l])
        free.training_step_all(batch, step, pr)
    after = _snapshot(ma[1])
    for k, _ in ma[1].named_parameters():
        assert np.array_equal(after[k], start[k]), k
    assert any(not np.array_equal(after[k], start[k]) for k in after if k.endswith("running_mean"))   # it did run
    assert a.levels[1].step_counts() == b.levels[1].step_counts() == [2, 2, 1]      # (step 0: level 1 lacks year 2)
    for ya, yb, net_a, net_b in zip(a.levels[1].years, b.levels[1].years, ma[1].year_models, mb[1].year_models):
        for (k, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
            if k.endswith("conv_layer.bias") or "classifier1" in k or "classifier2" in k:
                continue
            (m1, v1), (m2, v2) = ya._moment_views(pa), yb._moment_views(pb)
            assert float(m2.abs().max()) > 0, k
            # m is linear in the gradient, v quadratic: twice the relative rounding difference of the two groupings
            assert rel_l2(m1.cpu().numpy(), m2.cpu().numpy()) < 1e-5, k
            assert rel_l2(v1.cpu().numpy(), v2.cpu().numpy()) < 2e-5, k
    for l in (0, 2, 3, 4):
        _same(ma[l], mc[l], l)
        assert a.levels[l].step_counts() == free.levels[l].step_counts(), l


def test_levels_with_other_adam_settings_are_stepped_level_by_level():
    """One level with other betas: one optimizer launch has one set of Adam settings, so the step must take the
    level-by-level path BEFORE any launch or counter change -- no exception with the state half advanced -- and leave what
    training_step per level leaves."""
    ma, a = _build("wide", "fp32")
    mb, b = _build("wide", "fp32")
    for d in (a, b):
        d.levels[2].betas = (0.8, 0.99)
        for yr in d.levels[2].years:
            yr.betas = (0.8, 0.99)
    for step in range(2):
        batch, present = _batch("wide", step, B=6)
        la = a.training_step_all(batch, step, None)
        assert not a.batched_last
        lb = [b.training_step(batch, step, l, None) for l in range(len(mb))]
        for x, y in zip(la, lb):
            assert torch.isfinite(x) and abs(float(x) - float(y)) <= 1e-5 * abs(float(y))
    for l in range(len(ma)):
        _same(ma[l], mb[l], l)
        assert a.levels[l].step_counts() == b.levels[l].step_counts() == ([2, 2, 1] if l == 1 else [1, 2, 2] if l == 3 else [2, 2, 2]), l


# ---- dta_adam_step_multi against its float64 statement ----
def test_adam_step_multi_vs_float64():
    """Three consecutive launches of five segments: n = 4096 and 12 (16-byte route), 4099 and 1 (scalar route), 4096 with p
    4 bytes off a 16-byte boundary (scalar route); two ungated with a host step count (4099, the misaligned one), two gated
    and active with a device step counter that starts at 4 (4096, 1), one gated and inactive (12); segment rates 1e-3, 2e-3 and 0 = the call's, which is 3e-3 in launches 0 and 2 (inherited) and 0 in launch 1 (frozen: p must not move, the moments do); grad_scale 0.5; zero_grad in
    launch 1 only.  Gradients uniform in +-1e-2 with one block of |g| <= 1e-9 (eps decides the update) and one of exact zeros."""
    from deeptreeattention_amd import _lib
    L = _lib.lib()
    d = dev()
    # the C ABI takes the betas as float: the statement is made for the values the call receives (0.999 as float32 is
    # 0.99900001, whose 1 - beta2 is 1.3e-5 below 0.001: v would sit that far from a statement made for the decimal value)
    b1, b2, eps, gs = float(np.float32(0.9)), float(np.float32(0.999)), 1e-8, 0.5
    #       n     segment lr  gated   active  p offset (floats)
    spec = [(4096, 1e-3, True, 1.0, 0), (12, 1e-3, True, 0.0, 0), (4099, 2e-3, False, None, 0), (1, 0.0, True, 1.0, 0),
            (4096, 0.0, False, None, 1)]
    segs = []
    for i, (n, lr, gated, active, off) in enumerate(spec):
        p0 = prng.uniform(40, i, (n,), -1.0, 1.0)
        buf = torch.zeros(n + 4, dtype=torch.float32, device=d)
        p = buf[off:off + n]
        p.copy_(torch.from_numpy(p0))
        assert p.data_ptr() % 16 == 4 * off
        s = dict(n=n, lr=lr, gated=gated, p=p, buf=buf, g=torch.zeros(n, dtype=torch.float32, device=d),
                 m=torch.zeros(n, dtype=torch.float32, device=d), v=torch.zeros(n, dtype=torch.float32, device=d),
                 m64=np.zeros(n), v64=np.zeros(n), t=2 if not gated else 4)
        if gated:
            s["active"] = torch.tensor([active], dtype=torch.float32, device=d)
            s["steps"] = torch.tensor([4, -7], dtype=torch.int32, device=d)      # two words used alternately
        segs.append(s)
    for launch, (call_lr, zero_grad) in enumerate([(3e-3, 0), (0.0, 1), (3e-3, 0)]):
        arr = (_lib.AdamSegment * len(segs))()
        for i, s in enumerate(segs):
            g = prng.uniform(41 + launch, i, (s["n"],), -1e-2, 1e-2)
            if s["n"] >= 4096:
                g[256:512] *= 1e-7            # |g| <= 1e-9
                g[512:768] = 0.0
            s["g0"] = g
            s["g"].copy_(torch.from_numpy(g))
            cur, nxt = launch & 1, (launch & 1) ^ 1
            a = arr[i]
            a.p, a.g, a.m, a.v, a.n, a.lr = s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["n"], s["lr"]
            if s["gated"]:
                a.active, a.dev_step, a.dev_step_next = s["active"].data_ptr(), s["steps"].data_ptr() + 4 * cur, s["steps"].data_ptr() + 4 * nxt
                a.step = 0
            else:
                a.step = s["t"] + 1
        before = [(s["p"].cpu().numpy().copy(), s["m"].cpu().numpy().copy(), s["v"].cpu().numpy().copy()) for s in segs]
        _lib.check(L.dta_adam_step_multi(len(segs), arr, call_lr, b1, b2, eps, gs, zero_grad, _lib.current_stream_ptr()),
                   "dta_adam_step_multi")
        for i, s in enumerate(segs):
            tag = (launch, i)
            p, m, v, g = (s[k].cpu().numpy() for k in "pmvg")
            guard = s["buf"].cpu().numpy()
            off = (s["p"].data_ptr() - s["buf"].data_ptr()) // 4
            assert not np.any(guard[:off]) and not np.any(guard[off + s["n"]:]), tag      # nothing written beside p
            if s["gated"]:
                cnt = s["steps"].cpu().numpy()
            if s["gated"] and float(s["active"]) == 0.0:
                # not stepped: p, m, v untouched, the gradient cleared whatever zero_grad says, the count stays
                assert all(np.array_equal(x, y) for x, y in zip((p, m, v), before[i])), tag
                assert not np.any(g) and int(cnt[nxt]) == int(cnt[cur]) == 4, tag
                continue
            if s["gated"]:
                assert int(cnt[nxt]) == int(cnt[cur]) + 1 == s["t"] + 1, tag
            s["t"] += 1
            assert np.array_equal(g, np.zeros_like(g) if zero_grad else s["g0"]), tag
            lr = s["lr"] if s["lr"] > 0 else call_lr
            g64 = s["g0"].astype(np.float64) * gs
            s["m64"] = b1 * s["m64"] + (1 - b1) * g64
            s["v64"] = b2 * s["v64"] + (1 - b2) * g64 * g64
            d_ref = -(lr / (1 - b1 ** s["t"])) * s["m64"] / (np.sqrt(s["v64"]) / np.sqrt(1 - b2 ** s["t"]) + eps)
            # m, v: three float32 roundings per step, three steps
            assert rel_l2(m, s["m64"]) <= 1e-6 and rel_l2(v, s["v64"]) <= 1e-6, (tag, rel_l2(m, s["m64"]), rel_l2(v, s["v64"]))
            if lr == 0.0:
                assert np.array_equal(p, before[i][0]), tag                      # frozen: exactly
            d_dev = p.astype(np.float64) - before[i][0].astype(np.float64)
            err = np.linalg.norm(d_dev - d_ref)
            bound = 2.0 ** -23 * np.linalg.norm(before[i][0].astype(np.float64)) + 1e-6 * np.linalg.norm(d_ref)
            assert err <= bound, (tag, err, bound)
            assert lr == 0.0 or np.linalg.norm(d_ref) > 0, tag
