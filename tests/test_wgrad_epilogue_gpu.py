"""The bf16 weight-gradient kernels' slab epilogue (csrc/conv_bf16.hip, wgrad_bf16_body): every wave writes its partial
tap tiles to an fp32 LDS image and all 512 threads sum the k-slices and store the slab in 16-byte vectors.

1. Every program the stand-alone conv_module reaches, at the shapes where that epilogue can go wrong, against the oracle
   with the bounds and the oracle-relative yardstick of tests/test_module_entry_points_gpu.py (its _check_conv).
2. The network path -- the pair kernel of the second and third conv, the stacked 5x5 windows and the first conv's
   two-windows-in-flight program, none of which conv_module reaches: one bf16 FusedTrainer step through the new epilogue
   and through the first one (developer switch DTA_WGRAD_OLD_EPILOGUE) from the same state.  The k-slices are added in
   the same order, so every gradient and every parameter after the step must be equal bit for bit.  Only the developer
   library reads the switch: the comparison runs in a fresh child pytest of this file with DTA_DEV_LIB=1."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_module_entry_points_gpu import _check_conv

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, Cin, filters, H, W, pool)
EPILOGUE_CASES = [(1, 8, 64, 2, 2, False),       # <1,2>, one k-step: three of the four k-slices contribute zeros; B below the split count: empty slabs
                  (2, 70, 64, 4, 4, False),      # <2,2>, two channel groups, the second partial: the c < Cpad guard
                  (3, 40, 64, 3, 3, False),      # <2,2>, one partial channel group
                  (3, 40, 32, 3, 3, False),      # <4,1>
                  (2, 64, 128, 5, 5, True)]      # <1,2> with two column groups: the ng offset
SWITCH = "DTA_WGRAD_OLD_EPILOGUE"
NETWORK_BATCHES = [3, 37]      # 3: empty slabs; 37: a ragged last stacked window and ragged batch splits


def _case_id(c):
    return "B%d-%dto%d-%dx%d" % c[:5] + ("-pool" if c[5] else "")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=_case_id)
def test_conv_module_backward_at_the_epilogue_edges(case, precision):
    _check_conv(case, True, precision)


def _in_developer_library():
    from deeptreeattention_amd import _lib
    return bool(_lib.lib().dta_dev_switches_enabled())


def test_old_and_new_epilogue_bit_identical_on_the_network_path():
    """Runs test_network_step_bit_identical_child below in a fresh process that loads the developer library."""
    if _in_developer_library():
        pytest.skip("already running in the developer library")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-p", "no:cacheprovider", "-k", "bit_identical_child",
                        os.path.abspath(__file__)], cwd=REPO, env=dict(os.environ, DTA_DEV_LIB="1"), capture_output=True, text=True)
    tail = r.stdout[-3000:] + r.stderr[-1000:]
    assert r.returncode == 0, tail
    passed = [line for line in r.stdout.splitlines() if line.startswith("PASSED") and "bit_identical_child" in line]
    assert len(passed) == len(NETWORK_BATCHES), tail
    print(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("B", NETWORK_BATCHES)
def test_network_step_bit_identical_child(B, monkeypatch):
    if not _in_developer_library():
        pytest.skip("the product library has no switches: runs in the child of test_old_and_new_epilogue_bit_identical_on_the_network_path")
    from deeptreeattention_amd import Hang2020 as H
    from deeptreeattention_amd.engine import FusedTrainer
    torch.manual_seed(100 + B)
    bands, classes = 40, 7
    m0 = H.Hang2020(bands, classes, precision="bf16").cuda().train()
    x = torch.rand(B, bands, 11, 11, device="cuda")
    y = torch.randint(0, classes, (B,), device="cuda")

    def run():
        m = copy.deepcopy(m0)
        tr = FusedTrainer(m, lr=1e-3, keep_grads=True)
        loss = float(tr.train_step(x, y))
        torch.cuda.synchronize()
        grads = {k: tr.grad_of(p).cpu().numpy().copy() for k, p in m.named_parameters() if p.dtype == torch.float32}
        state = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items()}
        return loss, grads, state

    monkeypatch.delenv(SWITCH, raising=False)
    new = run()
    monkeypatch.setenv(SWITCH, "1")
    try:
        old = run()
    finally:
        monkeypatch.delenv(SWITCH, raising=False)
    assert new[0] == old[0]
    assert new[1].keys() == old[1].keys() and new[2].keys() == old[2].keys()
    conv_w = [k for k in new[1] if k.endswith("conv_layer.weight")]
    assert len(conv_w) == 6 and all(np.any(new[1][k]) for k in conv_w)      # the six weight gradients exist and are not all zero
    for k in new[1]:
        assert np.array_equal(new[1][k], old[1][k]), ("gradient", k)
    for k in new[2]:
        assert np.array_equal(new[2][k], old[2][k]), ("parameter / buffer", k)
