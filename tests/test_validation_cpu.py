"""Device-side validation, the parts that need no GPU: the two new C-ABI calls are declared, exported and refuse bad
arguments with a message; the validation fixture is the committed one; validate_multistage zips the levels' loaders without
cycling; the epoch loss is weighted by batch size; the new kernel has no private segment."""
import ctypes as C
import glob
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAL = os.path.join(REPO, "tests", "golden", "validation")


@pytest.fixture(scope="module")
def L():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_header_declares_and_library_exports_the_validation_calls(L):
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    assert {"dta_multistage_validate", "dta_eval_metrics"} <= names
    assert "typedef struct dta_eval_level" in hdr and "#define DTA_ABI_VERSION 2 " in hdr
    for n in ("dta_multistage_validate", "dta_eval_metrics"):
        assert hasattr(L, n), n
    assert L.dta_abi_version() == 2


def _levels(spec):
    from deeptreeattention_amd import _lib
    return (_lib.Level * len(spec))(*[_lib.Level(c, f, n, None, None, None, None, None, None, None) for c, f, n in spec])


def _evs(n, top_k=1, fake=0x1000):
    from deeptreeattention_amd import _lib
    return (_lib.EvalLevel * n)(*[_lib.EvalLevel(None, fake, fake, None, None, None, top_k) for _ in range(n)])


def test_multistage_validate_refuses_bad_arguments_before_any_launch(L):
    """Every refusal below happens in the host-side checks: nothing is launched (there is no GPU here), and the message names
    the cause."""
    from deeptreeattention_amd import _lib
    fo = 4 | _lib.FORWARD_ONLY

    def desc(training=0, mask=fo):
        return _lib.NetDesc(24, 16, 11, 11, 2, _lib.NET_SPECTRAL, _lib.DTA_F32, training, mask, 0.1, 1e-5)
    ok = _levels([(2, 0, 3), (5, 3, 3)])

    def call(d, nl, lv, ev):
        rc = L.dta_multistage_validate(C.byref(d) if d is not None else None, nl, lv, ev, None, None, None, None, None)
        return rc, L.dta_last_error().decode()
    rc, msg = call(None, 2, ok, _evs(2))
    assert rc != 0 and "null argument" in msg
    rc, msg = call(desc(training=1), 2, ok, _evs(2))
    assert rc != 0 and "training must be 0" in msg
    rc, msg = call(desc(mask=4), 2, ok, _evs(2))
    assert rc != 0 and "DTA_FORWARD_ONLY" in msg
    rc, msg = call(desc(mask=fo | _lib.REUSE_PACKED), 2, ok, _evs(2))
    assert rc != 0 and "DTA_REUSE_PACKED" in msg
    rc, msg = call(desc(), 2, _levels([(2, 0, 3), (5, 4, 3)]), _evs(2))
    assert rc != 0 and "adjacent" in msg
    rc, msg = call(desc(), 2, _levels([(2, 0, 9), (5, 9, 9)]), _evs(2))
    assert rc != 0 and "at most" in msg
    for k in (0, -1, _lib.EVAL_TOP_K_MAX + 1):
        rc, msg = call(desc(), 2, ok, _evs(2, top_k=k))
        assert rc != 0 and "top_k" in msg, (k, msg)
    rc, msg = call(desc(), 2, ok, _evs(2, fake=None))
    assert rc != 0 and "top_idx" in msg
    rc, msg = call(desc(), 2, ok, None)
    assert rc != 0 and "null argument" in msg
    rc, msg = call(desc(), 2, ok, _evs(2))          # everything about the levels is fine: nets / x / workspace are null
    assert rc != 0 and "null argument" in msg


def test_eval_metrics_refuses_bad_arguments_before_any_launch(L):
    fake = C.c_void_p(0x1000)
    ev = _evs(1)
    assert L.dta_eval_metrics(None, None, None, 8, 3, None, None, ev, None) != 0
    assert "null argument" in L.dta_last_error().decode()
    assert L.dta_eval_metrics(fake, fake, None, 8, 3, fake, fake, None, None) != 0
    assert "null argument" in L.dta_last_error().decode()
    assert L.dta_eval_metrics(fake, fake, None, 0, 3, fake, fake, ev, None) != 0
    assert "positive" in L.dta_last_error().decode()
    for k in (0, 9):
        assert L.dta_eval_metrics(fake, fake, None, 8, 3, fake, fake, _evs(1, top_k=k), None) != 0
        assert "top_k" in L.dta_last_error().decode()


def test_validation_fixture_is_the_committed_one():
    """tests/golden/validation has a checksum file of its own (tests/golden/SHA256SUMS lists the fixtures directly in
    tests/golden only); the fixture stays small and respects the cap on excluded rows its generator asserts."""
    lines = [ln.split() for ln in open(os.path.join(VAL, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert sorted(n for _, n in lines) == sorted(os.path.basename(f) for f in glob.glob(os.path.join(VAL, "*.npz")))
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(VAL, name), "rb").read()).hexdigest() == digest, name
    path = os.path.join(VAL, "validation_epoch.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(REPO, "tests", "golden", "multistage_steps.npz")) // 4
    import sys
    sys.path.insert(0, VAL)
    try:
        import recipe as R
    finally:
        sys.path.remove(VAL)
    g = np.load(path, allow_pickle=False)
    c = R.VALIDATION
    for l, classes in enumerate(c["classes"]):
        gaps = np.concatenate([g[f"batch{b}/level{l}/gap"] for b in range(len(c["batches"]))])
        assert gaps.shape == (sum(c["batches"]),)
        assert (gaps < c["min_gap"]).mean() <= c["max_excluded"]
        assert g[f"level{l}/confusion"].shape == (classes, classes)
        assert g[f"batch0/level{l}/softmax"].shape == (c["batches"][0], classes)


class _Loader:
    def __init__(self, sizes):
        self.sizes = sizes

    def loader(self, batch_size, shuffle=False, seed=0, drop_last=False):
        for i, n in enumerate(self.sizes):
            yield (["id"] * n, {"HSI": []}, np.zeros(n, np.int64) + i)


class _StubTrainer:
    """Counts what validate_multistage hands it; its epoch figures come from the package's own host-side arithmetic."""

    def __init__(self, nl):
        self.levels = [object()] * nl
        self.calls = []
        self.loss_acc = np.zeros((nl, 2))
        self.counts = np.zeros((nl, 4), np.int64)

    def validation_step_all(self, batches, batch_idx=0, present=None, top_k=1):
        self.calls.append((batch_idx, [None if b is None else len(b[0]) for b in batches], top_k))
        for l, b in enumerate(batches):
            if b is not None:
                n = len(b[0])
                loss = 1.0 + l + 0.5 * batch_idx            # this batch's loss
                self.loss_acc[l] += (loss * n, n)
                self.counts[l] += (n, 0, 0, 1)

    def validation_epoch_end(self, reset=True):
        from deeptreeattention_amd.engine import metrics_from_accumulators
        return [metrics_from_accumulators(np.zeros((2, 2), np.int64), self.counts[l], self.loss_acc[l]) for l in range(len(self.levels))]


def test_validate_multistage_zips_without_cycling_and_weights_the_loss_by_batch_size():
    from deeptreeattention_amd.loop import validate_multistage
    tr = _StubTrainer(3)
    res = validate_multistage(tr, [_Loader([24, 24, 10]), _Loader([24]), _Loader([24, 10])], batch_size=24, top_k=2)
    # every batch once, in order; an exhausted loader brings None (no cycling)
    assert tr.calls == [(0, [24, 24, 24], 2), (1, [24, None, 10], 2), (2, [10, None, None], 2)]
    assert [r["rows"] for r in res] == [58, 24, 34]
    # level 0: losses 1.0, 1.5, 2.0 on 24, 24, 10 rows -- the size-weighted mean, not the plain mean 1.5
    assert res[0]["val_loss"] == pytest.approx((24 * 1.0 + 24 * 1.5 + 10 * 2.0) / 58)
    assert res[0]["val_loss"] != pytest.approx(1.5)
    assert res[2]["val_loss"] == pytest.approx((24 * 3.0 + 10 * 3.5) / 34)
    with pytest.raises(ValueError):
        validate_multistage(tr, [_Loader([4])], batch_size=4)
    with pytest.raises(ValueError):
        validate_multistage(_StubTrainer(1), [_Loader([])], batch_size=4)


def test_metrics_from_accumulators_convention():
    from deeptreeattention_amd.engine import metrics_from_accumulators
    conf = np.array([[3, 1, 0], [0, 0, 0], [2, 0, 4]], np.int64)
    m = metrics_from_accumulators(conf, [10, 7, 9, 2], [5.0, 10.0])
    assert m["rows"] == 10 and m["micro"] == pytest.approx(0.7) and m["top_k"] == pytest.approx(0.9)
    assert m["macro"] == pytest.approx((0.75 + 4 / 6) / 2)        # the class without samples is left out
    assert m["accuracy"][1] == 0.0 and m["precision"][1] == 0.0   # zero denominators give 0.0
    assert m["val_loss"] == pytest.approx(0.5)
    assert np.isnan(metrics_from_accumulators(conf * 0, [0, 0, 0, 0], [0.0, 0.0])["val_loss"])


def test_fit_keywords_keep_the_default_records():
    """metrics=False is the default of both loops (the records then carry today's keys; the GPU tests check the values)."""
    import inspect
    from deeptreeattention_amd import loop
    for f in (loop.fit, loop.fit_multistage):
        assert inspect.signature(f).parameters["metrics"].default is False
    import deeptreeattention_amd as pkg
    assert pkg.validate is loop.validate and pkg.validate_multistage is loop.validate_multistage


def test_the_validation_kernel_has_no_private_segment(tmp_path):
    """tests/test_abi.py's code-object scan, for the new kernel by name: it is in the library and runs out of registers and LDS
    alone (no private segment, hence no scratch)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump, readelf = os.path.join(llvm, "llvm-objdump"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM tools not installed")
    from deeptreeattention_amd import _lib
    lib = os.path.join(str(tmp_path), "libdta_hip.so")
    shutil.copy(os.path.join(os.path.dirname(_lib.LIB_PATH), "libdta_hip.so"), lib)
    subprocess.run([objdump, "--offloading", lib], cwd=str(tmp_path), capture_output=True, check=True)
    found = []
    for f in sorted(glob.glob(lib + ".*gfx950*")):
        notes = subprocess.run([readelf, "--notes", f], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.", notes):
            name = re.search(r"\.?name:\s+(\S+)", blk)
            seg = re.search(r"private_segment_fixed_size:\s+(\d+)", blk)
            if name and seg and "k_eval_metrics_multi" in name.group(1):
                found.append((name.group(1), int(seg.group(1))))
    assert found, "k_eval_metrics_multi is not in the library"
    assert all(s == 0 for _, s in found), found
