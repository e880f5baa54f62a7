"""What tests/test_fp32_large_batch_gpu.py relies on, shown from the oracle alone (tests/large_batch_cases.py):

  attainable   -- the oracle accumulating in float32 stays within a quarter of FP32_TOL of its float64 run on every judged
                  tensor of every probe (and of the whole-batch gradient): the bound asks nothing float32 cannot give;
  row-specific -- the same probe values placed one row off give a gradient at least ten bounds away on every judged tensor:
                  an off-by-one in the row index cannot pass.  A tensor that misses this is not judged by that probe
                  (large_batch_cases.NOT_ROW_SPECIFIC, pinned here; at most two per probe, each under 1000 elements);
  class-weight probes -- O.weighted_cross_entropy with the probe's weights and labels is exactly zero outside the probed rows;
  plan restatement -- the launch-plan arithmetic the cases are chosen by, against the case table.

Run with -s for the table: per case and probe, the float32-oracle distance, the neighbouring-row distance and the count of
tensors left out."""
import numpy as np
import pytest

import large_batch_cases as LB
from conftest import rel_l2

FP32_TOL = 1e-3      # tests/test_hip_parity.py

ALL_PROBES = ([(c, p) for c in LB.HANG_CASES for p in LB.PROBES]
              + [(c, p) for c in LB.CASES for p in LB.cw_probe_rows(c)])


def test_plan_restatement_matches_case_table():
    for case, c in LB.CASES.items():
        B = c["B"]
        got = dict(stage_ppw=LB.stage_ppw(B), stage_grid=LB.stage_grid(B), conv_wg=LB.conv_wg(B), conv_tail=LB.conv_tail(B),
                   slabs0=LB.slabs0(case), ksplit=LB.ksplit(B))
        assert got == LB.PLAN[case], (case, got)
        rows = LB.probe_rows(case)
        assert rows["last"] == (B - 1,) and rows["pair_second"] == (B - 2,) and rows["row0"] == (0,)
        r = rows["interior"][0]
        assert 0 < r < B - 4 and r % 4 in (1, 2) and 1 <= r % 10 <= 8
        assert rows["conv1_tail"] == tuple(range((LB.conv_wg(B)[0] - 1) * 4, B)) and len(rows["conv1_tail"]) == LB.conv_tail(B)[0]
        if LB.stage_ppw(B) == 2:
            # B - 2 is the second patch of the last full pair, B - 1 the lone patch of the last workgroup
            assert (B - 2) % 2 == 1 and (B - 2) // 2 == LB.stage_grid(B) - 2 and (B - 1) // 2 == LB.stage_grid(B) - 1 and B % 2 == 1
    # 511 / 513 straddle: the stage kernels' pairing, the first conv's slab count, a K-slice step
    assert LB.stage_ppw(511) != LB.stage_ppw(513) and LB.ksplit(511) != LB.ksplit(513)
    assert LB.slabs0("below_pipe") == 511 and LB.slabs0("pipe_odd") == 512 < 513


@pytest.mark.parametrize("case,probe", [(c, p) for c in LB.CASES for p in LB.cw_probe_rows(c)])
def test_class_weight_probe_gradient_is_zero_outside_its_rows(case, probe):
    rows = list(LB.cw_probe_rows(case)[probe])
    w, y = LB.cw_inputs(case, probe)
    assert np.count_nonzero(w) == 1 and sorted(np.nonzero(y == int(np.nonzero(w)[0][0]))[0]) == rows
    from oracle import hang2020_np as O
    loss, dl = O.weighted_cross_entropy(LB.forward(case)["scores"], y, w)
    rest = np.delete(dl, rows, axis=0)
    assert rest.shape[0] == LB.CASES[case]["B"] - len(rows) and not np.any(rest)
    assert np.all(np.any(dl[rows] != 0, axis=1)) and loss > 0


def _grads(case, probe, dt=np.float64, shifted=False):
    if probe.startswith("cw_"):
        return LB.cw_oracle(case, probe, dt, shifted)["grads"]
    return LB.probe_grads(case, probe, dt, shifted)


@pytest.mark.parametrize("case,probe", ALL_PROBES)
def test_probe_is_attainable_and_row_specific(case, probe):
    ref, f32, off = _grads(case, probe), _grads(case, probe, np.float32), _grads(case, probe, np.float64, True)
    zero = [k for k in ref if LB.analytically_zero(k)]
    unspecific = tuple(sorted(k for k in ref if k not in zero and rel_l2(off[k], ref[k]) < 10 * FP32_TOL))
    names = LB.judged(case, probe, ref)
    att = max((rel_l2(f32[k], ref[k]), k) for k in names)
    spec = min((rel_l2(off[k], ref[k]), k) for k in names)
    print(f"\n{case:13s} {probe:15s} float32 oracle {att[0]:.2e} ({att[1]})  neighbouring row {spec[0]:.2e} ({spec[1]})  "
          f"left out: {len(unspecific)} not row-specific {unspecific}, {len(zero)} analytically zero")
    assert unspecific == tuple(sorted(LB.NOT_ROW_SPECIFIC.get((case, probe), ()))), unspecific
    assert len(unspecific) <= 2 and all(np.size(ref[k]) < 1000 for k in unspecific)
    assert len(names) == len(ref) - len(zero) - len(unspecific)
    assert att[0] <= FP32_TOL / 4, att
    assert spec[0] >= 10 * FP32_TOL, spec


@pytest.mark.parametrize("case", list(LB.CASES))
def test_whole_batch_gradient_is_attainable(case):
    ref, f32 = LB.whole_batch(case)["grads"], LB.whole_batch(case, np.float32)["grads"]
    att = max((rel_l2(f32[k], ref[k]), k) for k in ref if not LB.analytically_zero(k))
    print(f"\n{case:13s} whole batch     float32 oracle {att[0]:.2e} ({att[1]})")
    assert att[0] <= FP32_TOL / 4, att
