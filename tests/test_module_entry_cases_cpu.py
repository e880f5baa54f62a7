"""CPU companion of tests/test_module_entry_points_gpu.py: the references and case lists of that file, checked alone, so
that the GPU tests cannot pass or fail for the reference's reasons.

* integer GEMM cases: every partial sum stays below 2^24 (exact in fp32 in any order), and every case takes the GEMM
  program it was chosen for (the host restatement of gemm_load_mode / gemm_auto_ksplit against the table of the cases);
* conv_module / attention cases: the oracle run in float32 stays within ONE THIRD of each fp32 bound of the oracle run in
  float64, per quantity -- a case that does not is badly conditioned, not a kernel test;
* no exact ties inside a pool window of the oracle's pre-pool maps, so the argmax convention decides nothing."""
import numpy as np
import pytest

from conftest import rel_l2
from oracle import hang2020_np as O
import test_module_entry_points_gpu as G


def test_integer_cases_stay_exact_in_fp32():
    for case in G.LINEAR_CASES + [G.MISALIGNED_CASE]:
        batch, fin, fout = case
        x, w, b, dout = G.linear_int_inputs(*case)
        for a in (x, w, b, dout):
            assert a.dtype == np.int64 and np.abs(a).max() <= G.INT_RANGE
            assert set(np.unique(a)) == set(range(-G.INT_RANGE, G.INT_RANGE + 1)) or a.size < 40
        # worst-case magnitude of any partial sum, whatever the order
        assert G.INT_RANGE * G.INT_RANGE * fin + G.INT_RANGE < 2 ** 24          # out = x W^T + b
        assert G.INT_RANGE * G.INT_RANGE * fout < 2 ** 24                       # dx = dout W
        assert G.INT_RANGE * G.INT_RANGE * batch < 2 ** 24                      # gw = dout^T x
        assert G.INT_RANGE * batch < 2 ** 24                                    # gb = row sums
        for ref in (x @ w.T + b, dout @ w, dout.T @ x, dout.sum(0)):
            assert np.array_equal(ref.astype(np.float32).astype(np.int64), ref)
    assert 9 * 8198 < 2 ** 24


# (form, ksplit, empty trailing K slices) of the forward, input-gradient and weight-gradient GEMM of every case
WT, BLK = "wt:", "64x64"
EXPECTED_PATHS = {
    (1, 4, 4): {"fwd": ("wt:VEC_K/VEC_K", 1, 0), "dx": ("wt:VEC_K/VEC_ROW", 1, 0), "gw": ("wt:VEC_ROW/VEC_ROW", 1, 0)},
    (3, 5, 7): {"fwd": (BLK, 1, 0), "dx": (BLK, 1, 0), "gw": (BLK, 1, 0)},
    (33, 36, 34): {"fwd": ("wt:VEC_K/VEC_K", 1, 0), "dx": ("wt:SC_K/VEC_ROW", 1, 0), "gw": ("wt:SC_ROW/VEC_ROW", 1, 0)},
    (65, 130, 66): {"fwd": (BLK, 2, 0), "dx": (BLK, 1, 0), "gw": (BLK, 1, 0)},
    (20, 128, 200): {"fwd": ("wt:VEC_K/VEC_K", 1, 0), "dx": ("wt:VEC_K/VEC_ROW", 1, 0), "gw": ("wt:VEC_ROW/VEC_ROW", 1, 0)},
    (20, 128, 201): {"fwd": ("wt:VEC_K/VEC_K", 1, 0), "dx": ("wt:SC_K/VEC_ROW", 1, 0), "gw": ("wt:SC_ROW/VEC_ROW", 1, 0)},
    (3, 1001, 5): {"fwd": (BLK, 8, 0), "dx": (BLK, 1, 0), "gw": (BLK, 1, 0)},
    (5, 8196, 8): {"fwd": ("wt:VEC_K/VEC_K", 65, 0), "dx": ("wt:VEC_K/VEC_ROW", 1, 0), "gw": ("wt:VEC_ROW/VEC_ROW", 1, 0)},
    (65, 8196, 8): {"fwd": ("wt:VEC_K/VEC_K", 64, 12), "dx": ("wt:VEC_K/VEC_ROW", 1, 0), "gw": ("wt:VEC_ROW/VEC_ROW", 1, 0)},
    (65, 8198, 8): {"fwd": (BLK, 64, 12), "dx": (BLK, 1, 0), "gw": (BLK, 1, 0)},
    (2051, 128, 7): {"fwd": ("wt:VEC_K/VEC_K", 1, 0), "dx": ("wt:SC_K/VEC_ROW", 1, 0), "gw": ("wt:SC_ROW/VEC_ROW", 1, 0)},
}


def test_every_linear_case_takes_the_program_it_was_chosen_for():
    assert set(EXPECTED_PATHS) == set(G.LINEAR_CASES)
    for case in G.LINEAR_CASES:
        assert G.linear_paths(*case) == EXPECTED_PATHS[case], case
    # (5, 8196, 8): slice 64 of 65 holds the last 4 of K; (65, 819x, 8): slices 52..63 start past K
    assert (8196 + 64) // 65 == 127 and 64 * 128 == 8192
    # (2051, 128, 7): gw sums K = batch = 2051 = 64 * 32 + 3 (a row-fast K tail); dx covers 65 row tiles of 32
    assert 2051 % 32 == 3 and (2051 + 31) // 32 == 65
    # the aligned call of the misaligned case is all wave tiles; each misaligned operand sends its two GEMMs elsewhere
    al = G.linear_paths(*G.MISALIGNED_CASE)
    assert all(v[0].startswith(WT) for v in al.values())
    mis = {w: G.linear_paths(*G.MISALIGNED_CASE, misaligned=w) for w in ("x", "w", "dout")}
    assert mis["x"]["fwd"][0] == BLK and mis["x"]["gw"][0] == BLK and mis["x"]["dx"] == al["dx"]
    assert mis["w"]["fwd"][0] == BLK and mis["w"]["dx"][0] == BLK and mis["w"]["gw"] == al["gw"]
    assert mis["dout"]["dx"][0] == "wt:SC_K/VEC_ROW" and mis["dout"]["gw"][0] == "wt:SC_ROW/VEC_ROW" and mis["dout"]["fwd"] == al["fwd"]
    # every program of the GEMM is reached by some case: the six wave-tile pairs but the unused (VEC_ROW, VEC_K), and 64x64
    forms = {v[0] for c in G.LINEAR_CASES for v in G.linear_paths(*c).values()}
    assert forms == {"wt:VEC_K/VEC_K", "wt:VEC_K/VEC_ROW", "wt:VEC_ROW/VEC_ROW", "wt:SC_K/VEC_ROW", "wt:SC_ROW/VEC_ROW", BLK}


def test_case_lists_are_the_issue_s():
    assert len(G.CONV_CASES) == 8 and len(G.CONV_RUNS) == 10 and all(c in G.CONV_CASES for c in G.CONV_EVAL_CASES)
    assert sum(G.conv_wants_dx(c) for c in G.CONV_CASES) == 4
    assert len(G.SPATIAL_CASES) == 9 and len(G.SPECTRAL_CASES) == 6
    assert G.SPATIAL_BWD_REFUSED <= set(G.SPATIAL_CASES)
    for Cc, B, Hh, Ww in G.SPATIAL_CASES:
        assert Hh >= O.SPATIAL_POOL[Cc] and Ww >= O.SPATIAL_POOL[Cc]


@pytest.mark.parametrize("run", G.CONV_RUNS, ids=[G._conv_id(r) for r in G.CONV_RUNS])
def test_conv_cases_are_well_conditioned(run):
    case, training = run
    lo, _ = G.conv_oracle(case, training, "f32")
    hi, _ = G.conv_oracle(case, training, "f64")
    bound = G.conv_bounds("fp32")
    assert set(lo) == set(hi)
    for k in sorted(hi):
        if k == "nbt":
            continue
        if k == "g/" + G.CB_KEY and training:
            # The GPU test holds this gradient to |.| < 1e-4 and compares it with no reference: under batch statistics it is
            # analytically zero, which the exact oracle confirms here.  (The float32 oracle adds B*H*W terms of dy naively and
            # lands at up to 1.1e-4 for the 37-patch case: the rounding of that sum, not the conditioning of the case.)
            assert np.abs(hi[k]).max() <= 1e-4 / 3, k
            print(f"  {G._conv_id(run)} conv bias gradient: float64 oracle {np.abs(hi[k]).max():.1e}, float32 oracle {np.abs(lo[k]).max():.1e}")
            continue
        fig = rel_l2(lo[k], hi[k])
        assert fig <= bound(k) / 3, (k, fig, bound(k) / 3)


@pytest.mark.parametrize("run", G.ATT_RUNS, ids=[G._att_id(r) for r in G.ATT_RUNS])
def test_attention_cases_are_well_conditioned(run):
    kind, case = run
    lo, _ = G.att_oracle(kind, case, "f32")
    hi, _ = G.att_oracle(kind, case, "f64")
    for k in sorted(hi):
        fig = rel_l2(lo[k], hi[k])
        assert fig <= G.att_bound(k) / 3, (k, fig)


def test_no_reference_gradient_is_identically_zero():
    """A dead ReLU in front of a stencil would make its gradients exact zeros, which equal any other zeros."""
    for kind, case in G.ATT_RUNS:
        out, _ = G.att_oracle(kind, case)
        assert all(np.any(v) for v in out.values()), (kind, case, [k for k, v in out.items() if not np.any(v)])
    for kind in ("spectral", "spatial"):
        for use_da, use_df in ((True, False), (False, True)):
            out, _ = G.att_oracle(kind, G.NULL_GRAD_CASE, "f64", use_da, use_df)
            assert all(np.any(v) for v in out.values()), (kind, use_da, use_df)
    for case, training in G.CONV_RUNS:
        out, _ = G.conv_oracle(case, training, "f64")
        assert all(np.any(v) for v in out.values()), (case, training)


def test_null_gradient_references_are_well_conditioned():
    for kind in ("spectral", "spatial"):
        for use_da, use_df in ((True, False), (False, True)):
            lo, _ = G.att_oracle(kind, G.NULL_GRAD_CASE, "f32", use_da, use_df)
            hi, _ = G.att_oracle(kind, G.NULL_GRAD_CASE, "f64", use_da, use_df)
            for k in sorted(hi):
                assert rel_l2(lo[k], hi[k]) <= G.att_bound(k) / 3, (kind, use_da, use_df, k)


def _window_ties(r, k):
    """Pool windows of r (B, C, H, W; k x k, stride k, floor) whose maximum is attained more than once."""
    B, Cc, Hh, Ww = r.shape
    ho, wo = Hh // k, Ww // k
    win = r[:, :, :ho * k, :wo * k].reshape(B, Cc, ho, k, wo, k).transpose(0, 1, 2, 4, 3, 5).reshape(B, Cc, ho, wo, k * k)
    mx = win.max(axis=-1, keepdims=True)
    return (win == mx).sum(axis=-1) > 1, mx[..., 0]


def test_no_pool_window_of_the_oracle_has_a_tie_that_matters():
    # conv_module: 2x2 pool of relu(v).  A window whose maximum is the ReLU's zero has ties by construction, and no gradient
    # whichever element is picked (dv = dr * (v > 0)); every other window has ONE maximum.
    # (The oracle's bf16 mode also rounds the conv output to half, as the NETWORK path stores it, and that rounding makes 16
    #  of the 46080 windows of the 24x24 case tie; the stand-alone entry point keeps its conv output in fp32, so it picks
    #  the exact oracle's element there.  Those windows are part of the oracle's own bf16-vs-exact deviation, the yardstick
    #  the bf16 GPU test scales its bound with.)
    for case, training in G.CONV_RUNS:
        if not case[5]:
            continue
        for mode in ("f64", "f32"):
            _, cache = G.conv_oracle(case, training, mode)
            tie, mx = _window_ties(np.maximum(cache["v"], 0), 2)
            assert not (tie & (mx > 0)).any(), (case, training, mode)
    # spatial attention: class pool of the gated map
    for case in G.SPATIAL_CASES:
        for mode in ("f64", "f32"):
            out, cache = G.att_oracle("spatial", case, mode)
            if cache["ps"] == 1:
                continue
            tie, _ = _window_ties(out["a"], cache["ps"])
            assert not tie.any(), (case, mode)
