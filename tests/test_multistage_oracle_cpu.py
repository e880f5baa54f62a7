"""The per-level oracle of tests/multistage_oracle.py against the reference's own golden multi-stage step, and the premise
of the gradient-scale check of tests/test_multistage_oracle_gpu.py: Adam hides a gradient's magnitude."""
import numpy as np

from conftest import rel_l2
from multistage_oracle import level_oracle, oracle_adam, scale_deviation
from oracle import hang2020_np as O
from oracle.recipes import MULTISTAGE, multistage_inputs, multistage_weight


def _level(l):
    c = MULTISTAGE
    classes = c["classes"][l]
    p = O.init_params(O.learned_ensemble_spec(c["years"], c["bands"], classes), seed=301 + l)
    imgs, y = multistage_inputs(0, l, c["years"], c["B"], c["bands"], classes)
    return p, imgs, y, multistage_weight(classes)


def test_level_oracle_reproduces_the_reference_golden_step(golden):
    """step 0 of tests/golden/multistage_steps.npz (the reference's learned_ensemble + F.cross_entropy per level, in fp32):
    scores and loss of both levels within 2e-4."""
    g = golden("multistage_steps.npz")
    for l in range(len(MULTISTAGE["classes"])):
        p, imgs, y, w = _level(l)
        scores, loss, grads, upd = level_oracle(p, imgs, y, w)
        ref = float(g[f"step0/level{l}/loss"])
        assert rel_l2(scores, g[f"step0/level{l}/score"]) < 2e-4, l
        assert abs(loss - ref) < 2e-4 * abs(ref), l
        assert len(grads) and all(k in p for k in grads) and all(k in p for k in upd)


def test_adam_hides_a_gradient_scale_that_the_scale_check_sees():
    """A level's gradient multiplied by 2 (a wrong 1 / kept years, a wrong class-weight normaliser): the float64 Adam
    parameters after the step move by far less than the 2e-3 the parameter comparisons of tests/test_multistage_gpu.py
    allow -- m / (sqrt(v) + eps) is invariant under g -> 2 g while |g| >> eps -- and the scale check sees a deviation of 1."""
    p, imgs, y, w = _level(1)
    _, _, grads, _ = level_oracle(p, imgs, y, w)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    doubled = {k: 2.0 * v for k, v in grads.items()}
    years = MULTISTAGE["years"]
    a = oracle_adam(p64, grads, [dict() for _ in range(years)], MULTISTAGE["lrs"][1])
    b = oracle_adam(p64, doubled, [dict() for _ in range(years)], MULTISTAGE["lrs"][1])
    moved = 0
    for k in grads:
        if k.endswith("conv_layer.bias"):
            continue
        moved += int(np.any(a[k] != p64[k]))
        # the bound of the parameter comparisons cannot see the factor (only elements with |g| ~ eps = 1e-8 move at all:
        # 2.7e-4 on the worst tensor, the third attention's 7-tap stencil)
        assert rel_l2(b[k], a[k]) < 2e-3, k
    assert moved > 20
    for yy in range(years):
        want = {k: v for k, v in grads.items() if k.startswith(f"year_models.{yy}.")}
        assert scale_deviation(want, want) == 0.0
        assert scale_deviation(doubled, want) > 0.99   # fails the check's 1e-3 by three orders of magnitude


def test_near_decisions_explain_what_float32_does_to_the_oracle_itself():
    """The premise of multistage_oracle.near_alternatives, on the oracle alone: evaluated in float32, the `crops24` network
    (step 0, level 1, year 0) takes ONE of its 497,664 first-conv ReLU decisions the other way than in float64 (|v| =
    3.6e-7 at unit scale) and its first conv's gradient tensors land 2.4e-3 .. 4.6e-3 from the float64 ones -- past the
    1e-3 every tensor is held to, with nothing wrong.  With that decision taken the same way, every tensor agrees to 1e-5."""
    from multistage_oracle import case_inputs, near_alternatives, resolve_near_decisions, trajectory
    case, step, l, yy = "crops24", 0, 1, 0
    o = trajectory(case, False)[step][l]
    imgs, y = case_inputs(case, step, l)
    kept = [a if i == yy else np.zeros_like(a) for i, a in enumerate(imgs)]      # (the other year: skipped, not computed)
    scores, cache, _ = O.learned_ensemble_fwd(o["before"], kept, True, np.float32)
    _, dl = O.weighted_cross_entropy(o["scores"], y, multistage_weight(130))
    g32 = O.learned_ensemble_bwd(o["before"], cache, (dl / 2).astype(np.float32) * cache["n"], np.float32)
    mine = [k for k in g32 if not k.endswith("conv_layer.bias")]
    assert max(rel_l2(g32[k], o["grads"][k]) for k in mine) > 2e-3
    alts = near_alternatives(case, step, l, yy)
    ref, taken = resolve_near_decisions(g32, o["grads"], alts)
    assert 1 <= len(alts) <= 8 and taken.sum() == 1
    assert max(rel_l2(g32[k], ref[k]) for k in mine) < 1e-5
