"""The argument contract of the network entry points of csrc/capi.hip, pinned on the CPU: a table of refused calls,
each with the exact text dta_last_error() holds afterwards.  Every call here returns before its first launch, so no GPU
is needed and the dummy device pointers are never dereferenced (pointer ARRAYS such as `x` are read on the host: they
are real ctypes arrays of dummy values).  The texts were recorded from the library before the option structs and the
grouped-call helpers went in; a refactor of capi.hip keeps every one of them byte for byte.

Plus one check of build.py: every project header a source includes is one the build watches and hashes."""
import ctypes as C
import glob
import os
import re

import pytest

from deeptreeattention_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000          # a dummy non-null device pointer
SPEC, HANG, VAN = _lib.NET_SPECTRAL, _lib.NET_HANG2020, _lib.NET_VANILLA
BF16, F32 = _lib.DTA_BF16, _lib.DTA_F32
FWD_ONLY, REUSE = _lib.FORWARD_ONLY, _lib.REUSE_PACKED
LEVELS = [(2, 0, 2), (5, 2, 3)]        # (classes, first, count): two levels, five networks


@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def desc(kind=SPEC, dtype=BF16, training=1, heads=4, classes=2):
    return C.byref(_lib.NetDesc(8, 16, 11, 11, classes, kind, dtype, training, heads, 0.1, 1e-5))


def nets(n=5):
    return (_lib.SubnetParams * n)()


def grads(n=5):
    return (_lib.SubnetGrads * n)()


def ptrs(n=5, missing=None):
    a = (C.c_void_p * n)(*([P] * n))
    if missing is not None:
        a[missing] = None
    return a


def levels(spec=LEVELS, **null):
    """dta_level table with every pointer a dummy; `name=l` leaves that field of level l null."""
    out = []
    for l, (c, f, n) in enumerate(spec):
        lv = _lib.Level(c, f, n, P, P, P, P, P, P, P)
        for name, which in null.items():
            if which == l:
                setattr(lv, name, None)
        out.append(lv)
    return (_lib.Level * len(spec))(*out)


def evals(n=2, top_k=1, **null):
    out = [_lib.EvalLevel(P, P, P, P, P, P, top_k) for _ in range(n)]
    for name, which in null.items():
        setattr(out[which], name, None)
    return (_lib.EvalLevel * n)(*out)


def hierarchy(classes=(2, 5), n_levels=None, table=P):
    h = _lib.HierarchyTable(len(classes) if n_levels is None else n_levels, 3, (C.c_int * _lib.MAX_LEVELS)(*classes), table)
    return C.byref(h)


VAL = dict(training=0, heads=4 | FWD_ONLY)      # the descriptor dta_multistage_validate takes


def net_forward(d=None, nets_=1, x=P, ws=P):
    return (d or desc(HANG), nets(2) if nets_ else None, P, x, ws, None, P, None)


def net_forward_loss(d=None, x=P, x_tiles=None, labels=P, joint=P):
    return (d or desc(HANG), nets(2), P, x, x_tiles, P, labels, P, joint, P, P, P, None)


def net_backward_tiles(d=None, x_tiles=P, phases=3):
    return (d or desc(HANG), nets(2), P, x_tiles, P, None, P, grads(2), P, phases, None)


def net_backward(d=None, g=1, phases=3):
    return (d or desc(HANG), nets(2), P, P, None, P, grads(2) if g else None, P, phases, None)


def net_backward_dp(d=None, x_tiles=None, g=1, phases=3):
    return (d or desc(HANG), nets(2), P, x_tiles, P, None, P, grads(2) if g else None, P, P, phases, None)


def net_backward_xchg(d=None, x_tiles=None, xchg=P):
    return (d or desc(HANG), nets(2), P, x_tiles, P, None, P, grads(2), P, xchg, 0, None)


def ens_forward(d=None, years=3, x=None, mean=P):
    return (d or desc(), years, nets(3), x or ptrs(3), P, mean, None)


def ens_forward_gated(d=None, years=3, nets_=1, x=None, gate=P):
    return (d or desc(), years, nets(3) if nets_ else None, x or ptrs(3), gate, P, P, P, None)


def ens_forward_loss(d=None, years=3, x=None, labels=P):
    return (d or desc(), years, nets(3), x or ptrs(3), P, P, labels, P, P, P, P, P, P, None)


def ens_backward(d=None, years=3, dscore=P):
    return (d or desc(), years, nets(3), P, dscore, grads(3), None)


def ens_backward_phased(d=None, years=3, dscore=P, phases=3):
    return (d or desc(), years, nets(3), P, dscore, grads(3), phases, None)


def ens_backward_gated(d=None, years=3, dscore=P, phases=3):
    return (d or desc(), years, nets(3), P, dscore, grads(3), P, phases, None)


def ens_backward_xchg(d=None, years=3, xchg=P):
    return (d or desc(), years, nets(3), P, P, grads(3), P, xchg, None)


def ms_forward(d=None, n=2, lv=None, nets_=1, x=None):      # dta_multistage_forward and _forward_loss
    return (d or desc(), n, lv or levels(), nets() if nets_ else None, x or ptrs(), P, P, None)


def ms_predict(d=None, n=2, lv=None, x=None, top_idx=1):
    return (d or desc(), n, lv or levels(), nets(), x or ptrs(), P, P, ptrs(2), ptrs(2) if top_idx else None, ptrs(2), None)


def ms_validate(d=None, n=2, lv=1, ev=1, nets_=1, x=None):
    return (d or desc(**VAL), n, (levels() if lv == 1 else lv), (evals() if ev == 1 else ev), nets() if nets_ else None,
            x or ptrs(), P, P, None)


def ms_predict_ensemble(d=None, n=2, lv=None, x=None, top_score=1, table=None, ens_label=P, labels=P):
    return (d or desc(), n, lv or levels(), nets(), x or ptrs(), P, P, ptrs(2), ptrs(2), ptrs(2) if top_score else None,
            table or hierarchy(), ens_label, P, P, labels, P, None)


def ms_backward(d=None, n=2, lv=None, g=1):
    return (d or desc(), n, lv or levels(), nets(), P, grads() if g else None, P, None)


D7 = "unknown dtype 7"
SPECTRAL_ONLY = "%s: the descriptor's kind must be DTA_NET_SPECTRAL"

# (entry point, arguments, dta_last_error() after the refused call)
TABLE = [
    # ---- single networks -------------------------------------------------------------------------------------------
    ("dta_net_forward", lambda: net_forward(x=None), "dta_net_forward: null argument"),
    ("dta_net_forward", lambda: net_forward(nets_=0), "dta_net_forward: null argument"),
    ("dta_net_forward", lambda: net_forward(desc(HANG, 7)), D7),
    ("dta_net_forward", lambda: net_forward(desc(9)), "unknown network kind 9"),
    ("dta_net_forward_tiles", lambda: net_forward(x=None), "dta_net_forward_tiles: null argument"),
    ("dta_net_forward_tiles", lambda: net_forward(desc(HANG, 7)), "dta_net_forward_tiles: bf16 mode only"),
    ("dta_net_forward_tiles", lambda: net_forward(desc(HANG, F32)), "dta_net_forward_tiles: bf16 mode only"),
    ("dta_net_forward_tiles", lambda: net_forward(desc(9)), "unknown network kind 9"),
    ("dta_net_forward_loss", lambda: net_forward_loss(labels=None), "dta_net_forward_loss: null argument"),
    ("dta_net_forward_loss", lambda: net_forward_loss(x=None), "dta_net_forward_loss: null argument"),
    ("dta_net_forward_loss", lambda: net_forward_loss(desc(HANG, 7)), D7),
    ("dta_net_forward_loss", lambda: net_forward_loss(desc(SPEC)), "dta_net_forward_loss: single-score networks only (Hang2020, vanilla_CNN)"),
    ("dta_net_forward_loss", lambda: net_forward_loss(desc(VAN), joint=None), "dta_net_forward_loss: vanilla_CNN's scores are written to `joint`"),
    ("dta_net_forward_loss", lambda: net_forward_loss(desc(HANG, F32), x_tiles=P), "dta_net_forward_loss: tile input is bf16 mode only"),
    ("dta_net_forward_loss", lambda: net_forward_loss(desc(HANG, 7), x_tiles=P), "dta_net_forward_loss: tile input is bf16 mode only"),
    ("dta_net_backward_tiles", lambda: net_backward_tiles(x_tiles=None), "dta_net_backward_tiles: null argument"),
    ("dta_net_backward_tiles", lambda: net_backward_tiles(phases=0), "dta_net_backward_tiles: null argument"),
    ("dta_net_backward_tiles", lambda: net_backward_tiles(desc(HANG, 7)), "dta_net_backward_tiles: bf16 mode only"),
    ("dta_net_backward_tiles", lambda: net_backward_tiles(desc(9)), "unknown network kind 9"),
    ("dta_net_backward", lambda: net_backward(g=0), "dta_net_backward: null argument"),
    ("dta_net_backward", lambda: net_backward(phases=0), "dta_net_backward: null argument"),
    ("dta_net_backward", lambda: net_backward(phases=4), "dta_net_backward: null argument"),
    ("dta_net_backward", lambda: net_backward(desc(HANG, 7)), D7),
    ("dta_net_backward", lambda: net_backward(desc(9)), "unknown network kind 9"),
    ("dta_net_backward_dp", lambda: net_backward_dp(g=0), "dta_net_backward_dp: null argument"),
    ("dta_net_backward_dp", lambda: net_backward_dp(phases=0), "dta_net_backward_dp: null argument"),
    ("dta_net_backward_dp", lambda: net_backward_dp(desc(HANG, 7)), D7),
    ("dta_net_backward_dp", lambda: net_backward_dp(desc(HANG, F32), x_tiles=P), "dta_net_backward_dp: tile input is bf16 mode only"),
    ("dta_net_backward_dp", lambda: net_backward_dp(desc(9)), "unknown network kind 9"),
    ("dta_net_backward_xchg", lambda: net_backward_xchg(xchg=None), "dta_net_backward_xchg: null argument"),
    ("dta_net_backward_xchg", lambda: net_backward_xchg(desc(HANG, 7)), D7),
    ("dta_net_backward_xchg", lambda: net_backward_xchg(desc(HANG, F32), x_tiles=P), "dta_net_backward_xchg: tile input is bf16 mode only"),
    ("dta_net_backward_xchg", lambda: net_backward_xchg(desc(9)), "unknown network kind 9"),
    # ---- year ensembles --------------------------------------------------------------------------------------------
    ("dta_ensemble_forward", lambda: ens_forward(mean=None), "dta_ensemble_forward: null argument"),
    ("dta_ensemble_forward", lambda: ens_forward(desc(dtype=7)), D7),
    ("dta_ensemble_forward", lambda: ens_forward(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_forward"),
    ("dta_ensemble_forward", lambda: ens_forward(x=ptrs(3, missing=1)), "dta_ensemble_forward: null input for year 1"),
    ("dta_ensemble_forward", lambda: ens_forward(years=0), "dta_ensemble_forward: 1..16 years"),
    ("dta_ensemble_forward", lambda: ens_forward(years=17), "dta_ensemble_forward: 1..16 years"),
    ("dta_ensemble_forward_gated", lambda: ens_forward_gated(gate=None), "dta_ensemble_forward_gated: null gate"),
    ("dta_ensemble_forward_gated", lambda: ens_forward_gated(nets_=0), "dta_ensemble_forward: null argument"),
    ("dta_ensemble_forward_gated", lambda: ens_forward_gated(desc(dtype=7)), D7),
    ("dta_ensemble_forward_gated", lambda: ens_forward_gated(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_forward"),
    ("dta_ensemble_forward_gated", lambda: ens_forward_gated(x=ptrs(3, missing=2)), "dta_ensemble_forward: null input for year 2"),
    ("dta_ensemble_forward_loss", lambda: ens_forward_loss(labels=None), "dta_ensemble_forward_loss: null argument"),
    ("dta_ensemble_forward_loss", lambda: ens_forward_loss(desc(dtype=7)), D7),
    ("dta_ensemble_forward_loss", lambda: ens_forward_loss(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_forward_loss"),
    ("dta_ensemble_forward_loss", lambda: ens_forward_loss(x=ptrs(3, missing=0)), "dta_ensemble_forward_loss: null input for year 0"),
    ("dta_ensemble_forward_loss", lambda: ens_forward_loss(years=17), "dta_ensemble_forward_loss: 1..16 years"),
    ("dta_ensemble_backward", lambda: ens_backward(dscore=None), "dta_ensemble_backward: null argument"),
    ("dta_ensemble_backward", lambda: ens_backward(desc(dtype=7)), D7),
    ("dta_ensemble_backward", lambda: ens_backward(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_backward"),
    ("dta_ensemble_backward_phased", lambda: ens_backward_phased(dscore=None), "dta_ensemble_backward: null argument"),
    ("dta_ensemble_backward_phased", lambda: ens_backward_phased(phases=0), "dta_ensemble_backward: null argument"),
    ("dta_ensemble_backward_phased", lambda: ens_backward_phased(desc(dtype=7)), D7),
    ("dta_ensemble_backward_phased", lambda: ens_backward_phased(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_backward"),
    ("dta_ensemble_backward_gated", lambda: ens_backward_gated(dscore=None), "dta_ensemble_backward: null argument"),
    ("dta_ensemble_backward_gated", lambda: ens_backward_gated(phases=0), "dta_ensemble_backward: null argument"),
    ("dta_ensemble_backward_gated", lambda: ens_backward_gated(desc(dtype=7)), D7),
    ("dta_ensemble_backward_gated", lambda: ens_backward_gated(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_backward"),
    ("dta_ensemble_backward_gated", lambda: ens_backward_gated(years=0), "dta_ensemble_backward: 1..16 years"),
    ("dta_ensemble_backward_xchg", lambda: ens_backward_xchg(xchg=None), "dta_ensemble_backward_xchg: null argument"),
    ("dta_ensemble_backward_xchg", lambda: ens_backward_xchg(desc(dtype=7)), D7),
    ("dta_ensemble_backward_xchg", lambda: ens_backward_xchg(desc(HANG)), SPECTRAL_ONLY % "dta_ensemble_backward_xchg"),
    # ---- multi-stage steps -----------------------------------------------------------------------------------------
    ("dta_multistage_forward_loss", lambda: ms_forward(nets_=0), "dta_multistage_forward_loss: null argument"),
    ("dta_multistage_forward_loss", lambda: ms_forward(desc(dtype=7)), D7),
    ("dta_multistage_forward_loss", lambda: ms_forward(desc(HANG)), SPECTRAL_ONLY % "dta_multistage_forward_loss"),
    ("dta_multistage_forward_loss", lambda: ms_forward(x=ptrs(5, missing=4)), "dta_multistage_forward_loss: null input for network 4"),
    ("dta_multistage_forward_loss", lambda: ms_forward(lv=levels(labels=1)), "dta_multistage_forward_loss: level 1: labels, loss and scratch are required"),
    ("dta_multistage_forward_loss", lambda: ms_forward(lv=levels(scratch=0)), "dta_multistage_forward_loss: level 0: labels, loss and scratch are required"),
    ("dta_multistage_forward_loss", lambda: ms_forward(n=9), "dta_multistage_forward_loss: 1..8 levels"),
    ("dta_multistage_forward_loss", lambda: ms_forward(lv=levels([(2, 0, 2), (5, 3, 2)])),
     "dta_multistage_forward_loss: level 1: its groups must be [first, first + count) with count >= 1, levels in order and adjacent"),
    ("dta_multistage_forward", lambda: ms_forward(nets_=0), "dta_multistage_forward: null argument"),
    ("dta_multistage_forward", lambda: ms_forward(desc(dtype=7)), D7),
    ("dta_multistage_forward", lambda: ms_forward(desc(HANG)), SPECTRAL_ONLY % "dta_multistage_forward"),
    ("dta_multistage_forward", lambda: ms_forward(x=ptrs(5, missing=0)), "dta_multistage_forward: null input for network 0"),
    ("dta_multistage_forward", lambda: ms_forward(lv=levels(mean_scores=1)), "dta_multistage_forward: level 1 has no score output"),
    ("dta_multistage_forward", lambda: ms_forward(lv=levels([(2, 0, 9), (5, 9, 9)])), "dta_multistage_forward: at most 16 networks (levels x kept years) per step"),
    ("dta_multistage_predict", lambda: ms_predict(top_idx=0), "dta_multistage_predict: null argument"),
    ("dta_multistage_predict", lambda: ms_predict(desc(dtype=7)), D7),
    ("dta_multistage_predict", lambda: ms_predict(desc(HANG)), SPECTRAL_ONLY % "dta_multistage_predict"),
    ("dta_multistage_predict", lambda: ms_predict(x=ptrs(5, missing=3)), "dta_multistage_predict: null input for network 3"),
    ("dta_multistage_predict", lambda: ms_predict(lv=levels([(2, 0, 2), (0, 2, 3)])), "dta_multistage_predict: level 1 has 0 classes"),
    ("dta_multistage_validate", lambda: ms_validate(ev=None), "dta_multistage_validate: null argument"),
    ("dta_multistage_validate", lambda: ms_validate(lv=None), "dta_multistage_validate: null argument"),
    ("dta_multistage_validate", lambda: ms_validate(nets_=0), "dta_multistage_validate: null argument"),
    ("dta_multistage_validate", lambda: ms_validate(desc(training=1, heads=4 | FWD_ONLY)),
     "dta_multistage_validate: validation runs eval-mode BatchNorm: the descriptor's training must be 0"),
    ("dta_multistage_validate", lambda: ms_validate(desc(training=0, heads=4)),
     "dta_multistage_validate: the descriptor's heads_mask must carry DTA_FORWARD_ONLY"),
    ("dta_multistage_validate", lambda: ms_validate(desc(training=0, heads=4 | FWD_ONLY | REUSE)),
     "dta_multistage_validate: DTA_REUSE_PACKED is refused: validation follows weight updates"),
    ("dta_multistage_validate", lambda: ms_validate(ev=evals(top_k=0)), "dta_multistage_validate: level 0: top_k must be 1..8, got 0"),
    ("dta_multistage_validate", lambda: ms_validate(ev=evals(top_k=9)), "dta_multistage_validate: level 0: top_k must be 1..8, got 9"),
    ("dta_multistage_validate", lambda: ms_validate(ev=evals(top_idx=1)), "dta_multistage_validate: level 1: top_idx and top_score are required"),
    ("dta_multistage_validate", lambda: ms_validate(desc(dtype=7, **VAL)), D7),
    ("dta_multistage_validate", lambda: ms_validate(desc(HANG, **VAL)), SPECTRAL_ONLY % "dta_multistage_validate"),
    ("dta_multistage_validate", lambda: ms_validate(x=ptrs(5, missing=2)), "dta_multistage_validate: null input for network 2"),
    ("dta_multistage_validate", lambda: ms_validate(lv=levels(loss=1)), "dta_multistage_validate: level 1: labels, loss and scratch are required"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(top_score=0), "dta_multistage_predict_ensemble: null argument"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(desc(dtype=7)), D7),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(desc(HANG)), SPECTRAL_ONLY % "dta_multistage_predict_ensemble"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(x=ptrs(5, missing=1)), "dta_multistage_predict_ensemble: null input for network 1"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(table=hierarchy(table=None)), "dta_multistage_predict_ensemble: null hierarchy table"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(ens_label=None), "dta_multistage_predict_ensemble: null ensemble output"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(labels=None),
     "dta_multistage_predict_ensemble: labels and confusion come together or not at all"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(table=hierarchy((2, 5, 3))),
     "dta_multistage_predict_ensemble: the hierarchy table has 3 levels, the call 2"),
    ("dta_multistage_predict_ensemble", lambda: ms_predict_ensemble(table=hierarchy((2, 4))),
     "dta_multistage_predict_ensemble: level 1 has 5 classes, the hierarchy table 4"),
    ("dta_multistage_backward", lambda: ms_backward(g=0), "dta_multistage_backward: null argument"),
    ("dta_multistage_backward", lambda: ms_backward(desc(dtype=7)), D7),
    ("dta_multistage_backward", lambda: ms_backward(desc(HANG)), SPECTRAL_ONLY % "dta_multistage_backward"),
    ("dta_multistage_backward", lambda: ms_backward(lv=levels(dscore=1)), "dta_multistage_backward: level 1 has no score gradient"),
    ("dta_multistage_backward", lambda: ms_backward(n=0), "dta_multistage_backward: 1..8 levels"),
]

# the entry points that reach the network forward / backward; the 15 that hold (or share) a dtype dispatch answer dtype = 7
# with its text, the two tile-only ones with their own
ENTRY_POINTS = ["dta_net_forward", "dta_net_forward_tiles", "dta_net_forward_loss", "dta_net_backward_tiles", "dta_net_backward",
                "dta_net_backward_dp", "dta_net_backward_xchg", "dta_ensemble_forward", "dta_ensemble_forward_gated",
                "dta_ensemble_forward_loss", "dta_ensemble_backward", "dta_ensemble_backward_phased", "dta_ensemble_backward_gated",
                "dta_ensemble_backward_xchg", "dta_multistage_forward_loss", "dta_multistage_forward", "dta_multistage_predict",
                "dta_multistage_validate", "dta_multistage_predict_ensemble", "dta_multistage_backward"]


def test_the_table_covers_every_entry_point():
    for name in ENTRY_POINTS:
        texts = [t for n, _, t in TABLE if n == name]
        assert any("null" in t for t in texts), name
        if name not in ("dta_net_forward_tiles", "dta_net_backward_tiles"):
            assert D7 in texts, name
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    declared = set(re.findall(r"\b(dta_(?:net|ensemble|multistage)_[a-z_0-9]+)\s*\(", hdr))
    no_network_pass = {"dta_net_workspace_bytes", "dta_ensemble_workspace_bytes", "dta_multistage_workspace_bytes", "dta_net_loss"}
    assert declared - no_network_pass == set(ENTRY_POINTS)


@pytest.mark.parametrize("name,args,text", TABLE, ids=["%s-%d" % (t[0], i) for i, t in enumerate(TABLE)])
def test_refused_call_and_its_text(lib, name, args, text):
    assert getattr(lib, name)(*args()) != 0
    assert lib.dta_last_error().decode() == text


def test_every_included_project_header_is_a_build_dependency():
    """A header missing from build.HEADERS triggers no rebuild when edited and does not enter dta_build_id."""
    from deeptreeattention_amd import build
    listed = {os.path.normpath(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    missing = []
    for src in sorted(glob.glob(os.path.join(build.CSRC, "*.hip")) + glob.glob(os.path.join(build.CSRC, "*.h"))):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(src).read(), re.M):
            if os.path.normpath(os.path.join(build.CSRC, inc)) not in listed:
                missing.append((os.path.basename(src), inc))
    assert not missing, missing
