"""The stand-alone module entry points of include/dta_hip.h (dta_linear_*, dta_conv_module_*, dta_attention_*) at the
shapes the network path never produces, against plain references of the same operations.

Linear / GEMM (csrc/heads.hip): integer-valued inputs, so that every fp32 sum is exact in any order (MFMA, LDS partial
tiles, atomicAdd) and the result must EQUAL the int64 NumPy product.  The cases are the smallest that reach each program
of the GEMM; `linear_paths` restates gemm_load_mode / gemm_wave_tiles / gemm_auto_ksplit / gemm_planned_ksplit on the host
and names the program each of the three GEMMs of a case takes (the CPU companion pins that table).

conv_module and the two attention modules: the fp64 NumPy oracle (oracle/hang2020_np.py), fp32 at the bounds of
test_hip_modules.py, bf16 against the oracle's bf16 mode at max(test_patch_sizes_gpu.py's bound, 1.5 x what the oracle
itself moves between its exact and its bf16 mode on the same case).  Non-square maps, the pools' minimum sizes, padded
channel chunks, filters = 128, B = 1, eval-mode backward and the null gradients of dta_attention_backward run here and
nowhere else.

The case lists and the references live here; tests/test_module_entry_cases_cpu.py checks, without a GPU, that the
references alone stay inside the bounds (conditioning, pool ties, exactness of the integer sums)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import hang2020_np as O
from oracle import prng

pytestmark = pytest.mark.gpu
TOL = 1e-3          # gradients, fp32 (test_hip_modules.py)
TIGHT = 2e-4        # outputs and buffers, fp32
BF16_OUT = 1e-3     # outputs and buffers, bf16 mode against the oracle with the same rounding (test_patch_sizes_gpu.py)
BF16_GRAD = 1e-2    # gradient tensors, bf16 mode
GEMM_REAL = 1e-5    # fp32 GEMM pieces (test_metadata_predict_gpu.py); sqrt(K) 2^-24 = 8.5e-7 at K = 201


# ------------------------------------------------------------------------------------------------------------------
# 1. linear: cases and the host restatement of the GEMM's program choice
# ------------------------------------------------------------------------------------------------------------------
# (batch, in_features, out_features)
LINEAR_CASES = [(1, 4, 4), (3, 5, 7), (33, 36, 34), (65, 130, 66), (20, 128, 200), (20, 128, 201), (3, 1001, 5),
                (5, 8196, 8), (65, 8196, 8), (65, 8198, 8), (2051, 128, 7)]
MISALIGNED_CASE = (33, 36, 36)          # run with x, w and dout each in turn one float past a 16-byte boundary
LINEAR_REAL_CASES = [(3, 5, 7), (33, 36, 34), (20, 128, 201)]
INT_RANGE = 3                           # integer inputs in [-3, 3]


def _load_mode(aligned, rows, K, s_row, s_k):
    """gemm_load_mode (heads.hip)."""
    if s_k == 1 and aligned and s_row % 4 == 0 and K % 4 == 0:
        return "VEC_K"
    if s_row == 1 and aligned and s_k % 4 == 0 and rows % 4 == 0:
        return "VEC_ROW"
    return "SCALAR"


def _wt_mode(aligned, rows, K, s_row, s_k):
    """gemm_wt_mode."""
    m = _load_mode(aligned, rows, K, s_row, s_k)
    if m != "SCALAR":
        return m
    return "SC_K" if s_k == 1 else ("SC_ROW" if s_row == 1 else "SCALAR")


def gemm_path(M, N, K, a_strides, b_strides, a_aligned=True, b_aligned=True):
    """The program launch_gemm runs for C[M][N] = A[M][K] B[K][N] with a_strides = (sa_m, sa_k), b_strides = (sb_n, sb_k)
    and the caller's ksplit = gemm_auto_ksplit(M, N, K): (form, ksplit, empty trailing K slices)."""
    am = _wt_mode(a_aligned, M, K, *a_strides)
    bm = _load_mode(b_aligned, N, K, *b_strides)
    wave_tiles = am != "SCALAR" and bm != "SCALAR" and (am in ("VEC_K", "VEC_ROW") or bm == "VEC_ROW")
    tiles = ((M + 63) // 64) * ((N + 63) // 64)                 # gemm_auto_ksplit
    ks = max(1, min((128 + tiles - 1) // tiles, (K + 127) // 128))
    if wave_tiles and K <= 8192:                                # gemm_planned_ksplit
        ks = 1
    kper = ((K + ks - 1) // ks + 31) // 32 * 32                 # K slice of one workgroup, whole 32-chunks
    empty = sum(1 for bz in range(ks) if bz * kper >= K)
    return (f"wt:{am}/{bm}" if wave_tiles else "64x64"), ks, empty


def linear_paths(batch, fin, fout, misaligned=None):
    """Programs of the three GEMMs behind dta_linear_forward / dta_linear_backward (capi_modules.hip)."""
    xa, wa, da = misaligned != "x", misaligned != "w", misaligned != "dout"
    return {"fwd": gemm_path(batch, fout, fin, (fin, 1), (fin, 1), xa, wa),       # x W^T
            "dx": gemm_path(batch, fin, fout, (fout, 1), (1, fin), da, wa),       # dout W
            "gw": gemm_path(fout, fin, batch, (1, fout), (1, fin), da, xa)}       # dout^T x


def _path_id(case, misaligned=None):
    p = linear_paths(*case, misaligned=misaligned)
    s = "-".join(f"{k}={v[0]},ks{v[1]}" + (f",empty{v[2]}" if v[2] else "") for k, v in p.items())
    return "x".join(map(str, case)) + (f"-{misaligned}+4B" if misaligned else "") + "-" + s


def linear_int_inputs(batch, fin, fout):
    seed = 700 + batch + 3 * fin + 7 * fout
    draw = lambda stream, shape: (prng.randint(seed, stream, shape, 2 * INT_RANGE + 1) - INT_RANGE)
    return draw(1, (batch, fin)), draw(2, (fout, fin)), draw(3, (fout,)), draw(4, (batch, fout))


def _dev():
    return torch.device("cuda:0")


def _f32(a, misalign=False):
    """A float32 device copy of `a`; misalign: a [1:] view of a flat buffer, one float past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
    if not misalign:
        return t
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=_dev())
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


SENTINEL = 12345.0


def _linear_forward(x, w, b, batch, fin, fout):
    from deeptreeattention_amd import _lib
    out = torch.full((batch, fout), SENTINEL, dtype=torch.float32, device=_dev())
    _lib.check(_lib.lib().dta_linear_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), batch, fin, fout, _lib.ptr(out),
                                             _lib.current_stream_ptr()), "dta_linear_forward")
    return out.cpu().numpy()


def _linear_backward(x, w, dout, batch, fin, fout, want_dx=True, want_gw=True):
    from deeptreeattention_amd import _lib
    dx = torch.full((batch, fin), SENTINEL, dtype=torch.float32, device=_dev()) if want_dx else None
    gw = torch.zeros(fout, fin, dtype=torch.float32, device=_dev()) if want_gw else None      # "arrive zero-filled"
    gb = torch.zeros(fout, dtype=torch.float32, device=_dev()) if want_gw else None
    _lib.check(_lib.lib().dta_linear_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(dout), batch, fin, fout, _lib.ptr(dx),
                                              _lib.ptr(gw), _lib.ptr(gb), _lib.current_stream_ptr()), "dta_linear_backward")
    return tuple(None if t is None else t.cpu().numpy() for t in (dx, gw, gb))


def _assert_exact(got, want, what):
    want = np.asarray(want)
    assert np.abs(want).max() < 2 ** 24
    bad = np.argwhere(got.astype(np.int64) != want)
    assert got.dtype == np.float32 and bad.size == 0 and np.array_equal(got, want.astype(np.float32)), \
        (what, len(bad), bad[:5].tolist(), [(float(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:5]])


def _check_linear_int(case, misaligned=None):
    batch, fin, fout = case
    x, w, b, dout = linear_int_inputs(*case)
    xd, wd, bd, dd = _f32(x, misaligned == "x"), _f32(w, misaligned == "w"), _f32(b), _f32(dout, misaligned == "dout")
    _assert_exact(_linear_forward(xd, wd, bd, *case), x @ w.T + b, "out")
    dx, gw, gb = _linear_backward(xd, wd, dd, *case)
    _assert_exact(dx, dout @ w, "dx")
    _assert_exact(gw, dout.T @ x, "gw")
    _assert_exact(gb, dout.sum(0), "gb")
    return xd, wd, dd, (x, w, dout), (dx, gw, gb)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=[_path_id(c) for c in LINEAR_CASES])
def test_linear_integer_inputs_are_exact(case):
    """out, dx, gw and gb equal the int64 products bit for bit: no tolerance.  The id names the program of each GEMM."""
    _check_linear_int(case)


@pytest.mark.parametrize("which", ["x", "w", "dout"])
def test_linear_operand_off_16_byte_alignment(which):
    """One operand one float past a 16-byte boundary: its vector load modes fall back, the values stay exact."""
    assert linear_paths(*MISALIGNED_CASE) != linear_paths(*MISALIGNED_CASE, misaligned=which)
    _check_linear_int(MISALIGNED_CASE, misaligned=which)


@pytest.mark.parametrize("case", [(3, 5, 7), (33, 36, 34), (65, 130, 66)], ids=lambda c: "x".join(map(str, c)))
def test_linear_optional_arguments(case):
    """b = NULL: no bias.  dx = NULL / gw = gb = NULL: that GEMM is skipped, the other outputs are what the full call gives."""
    xd, wd, dd, (x, w, dout), (dx, gw, gb) = _check_linear_int(case)
    _assert_exact(_linear_forward(xd, wd, None, *case), x @ w.T, "out without bias")
    dx2, gw2, gb2 = _linear_backward(xd, wd, dd, *case, want_dx=False)
    assert dx2 is None and np.array_equal(gw2, gw) and np.array_equal(gb2, gb)
    dx3, gw3, gb3 = _linear_backward(xd, wd, dd, *case, want_gw=False)
    assert gw3 is None and gb3 is None and np.array_equal(dx3, dx)


@pytest.mark.parametrize("case", LINEAR_REAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_classifier_real_values_vs_fp64_oracle(case):
    from deeptreeattention_amd import Hang2020 as H
    batch, fin, fout = case
    p = O.init_params(O.classifier_spec("", fin, fout), seed=31)
    m = H.Classifier(in_features=fin, classes=fout)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
    m = m.to(_dev())
    f = prng.uniform(32, fin, (batch, fin), -1, 1)
    ds = prng.uniform(32, 1000 + fout, (batch, fout), -1, 1)
    ft = torch.from_numpy(f).to(_dev()).requires_grad_(True)
    s = m(ft)
    (s * torch.from_numpy(ds).to(_dev())).sum().backward()
    ref = O.classifier_fwd(p, "", f, np.float64)
    rdf, rg = O.classifier_bwd(p, "", f.astype(np.float64), ds.astype(np.float64), np.float64)
    figs = {"out": rel_l2(s.detach().cpu().numpy(), ref), "dx": rel_l2(ft.grad.cpu().numpy(), rdf),
            "gw": rel_l2(m.fc1.weight.grad.cpu().numpy(), rg["fc1.weight"]), "gb": rel_l2(m.fc1.bias.grad.cpu().numpy(), rg["fc1.bias"])}
    print(f"  classifier {case}: " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert all(v < GEMM_REAL for v in figs.values()), figs


# ------------------------------------------------------------------------------------------------------------------
# 2. conv_module
# ------------------------------------------------------------------------------------------------------------------
# (B, Cin, filters, H, W, pool)
CONV_CASES = [(1, 1, 32, 2, 2, True),        # smallest everything; pooled map 1x1
              (2, 17, 64, 5, 8, True),       # padded second channel chunk; non-square; odd height under the pool
              (2, 16, 128, 8, 5, False),     # filters = 128; non-square the other way
              (37, 33, 32, 8, 8, False),     # several patches per workgroup, ragged last workgroup, three chunks
              (5, 32, 64, 24, 24, True),     # dx; a 576-row map (one workgroup in bf16, two in fp32)
              (3, 64, 128, 5, 5, True),      # dx; the network's stage 2 -> 3 geometry
              (3, 128, 32, 3, 7, False),     # dx through 8 chunks; non-square
              (9, 128, 128, 2, 2, True)]     # dx; the smallest pooled map
CONV_EVAL_CASES = [(2, 17, 64, 5, 8, True), (3, 64, 128, 5, 5, True)]
CONV_RUNS = [(c, True) for c in CONV_CASES] + [(c, False) for c in CONV_EVAL_CASES]
W_KEY, CB_KEY, G_KEY, B_KEY = "conv_layer.weight", "conv_layer.bias", "bn1.weight", "bn1.bias"


def _conv_id(run):
    (B, cin, f, Hh, Ww, pool), training = run
    return f"B{B}-{cin}to{f}-{Hh}x{Ww}" + ("-pool" if pool else "") + ("" if training else "-eval")


def conv_wants_dx(case):
    return case[1] in (32, 64, 128)


def conv_inputs(case):
    B, cin, f, Hh, Ww, pool = case
    seed = 1000 + 131 * B + 17 * cin + f + 3 * Hh + Ww
    p = O.init_params(O.conv_module_spec("", cin, f), seed=seed)       # BatchNorm statistics away from 0 / 1
    x = prng.uniform(seed, 1, (B, cin, Hh, Ww), -1, 1)
    zs = (B, f, Hh // 2, Ww // 2) if pool else (B, f, Hh, Ww)
    return p, x, prng.uniform(seed, 3, zs, -1, 1)


@functools.lru_cache(maxsize=None)
def conv_oracle(case, training, mode):
    """mode: 'f64' (exact), 'f32' (the oracle's own fp32 run) or 'bf16' (fp64 with the bf16 mode's roundings).
    Returns ({quantity: array}, forward cache)."""
    pool = case[5]
    p, x, dz = conv_inputs(case)
    dt = np.float32 if mode == "f32" else np.float64
    O.bf16_mode(mode == "bf16")
    try:
        z, cache, upd = O.conv_module_fwd(p, "", x, pool, training, dt)
        dx, g = O.conv_module_bwd(cache, "", dz.astype(dt), need_dx=conv_wants_dx(case))
        out = {"z": z, "g/" + W_KEY: g[W_KEY], "g/" + CB_KEY: g[CB_KEY], "g/" + G_KEY: g[G_KEY], "g/" + B_KEY: g[B_KEY]}
        if dx is not None:
            out["dx"] = dx
        if training:
            out["buf/bn1.running_mean"], out["buf/bn1.running_var"] = upd["bn1.running_mean"], upd["bn1.running_var"]
            out["nbt"] = upd["bn1.num_batches_tracked"]
            p2 = dict(p); p2.update(upd)
            out["z_eval"] = O.conv_module_fwd(p2, "", x, pool, False, dt)[0]
    finally:
        O.bf16_mode(False)
    return out, cache


def conv_bounds(precision):
    out, grad = (TIGHT, TOL) if precision == "fp32" else (BF16_OUT, BF16_GRAD)
    return lambda k: grad if (k == "dx" or k.startswith("g/")) else out


def _conv_device(case, training, precision):
    from deeptreeattention_amd import Hang2020 as H
    B, cin, f, Hh, Ww, pool = case
    p, x, dz = conv_inputs(case)
    m = H.conv_module(cin, f, maxpool_kernel=(2, 2) if pool else None)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
    m = m.to(_dev())
    m.precision = precision
    m.train(training)
    xt = torch.from_numpy(x).to(_dev()).requires_grad_(conv_wants_dx(case))
    z = m(xt, pool=pool)
    (z * torch.from_numpy(dz).to(_dev())).sum().backward()
    got = {"z": z.detach().cpu().numpy()}
    if xt.grad is not None:
        got["dx"] = xt.grad.cpu().numpy()
    for k, prm in m.named_parameters():
        got["g/" + k] = prm.grad.cpu().numpy()
    for k, b in m.named_buffers():
        got["nbt" if k.endswith("num_batches_tracked") else "buf/" + k] = b.cpu().numpy()
    if training:
        m.eval()
        with torch.no_grad():
            got["z_eval"] = m(xt.detach(), pool=pool).cpu().numpy()
    return got, p


def _check_conv(case, training, precision):
    got, p = _conv_device(case, training, precision)
    exact, _ = conv_oracle(case, training, "f64")
    ref, _ = conv_oracle(case, training, "bf16") if precision == "bf16" else (exact, None)
    base = conv_bounds(precision)
    fails = []
    for k in sorted(ref):
        if k == "nbt":
            assert int(got["nbt"]) == int(ref["nbt"]) == 1
            continue
        if k == "g/" + CB_KEY and training:
            # the conv bias feeds batch-statistics BatchNorm: its gradient is zero up to rounding (absolute bound)
            fig = float(np.abs(got[k]).max())
            print(f"  {_conv_id((case, training))} {precision} {k:24s} max |.| {fig:.2e} (bound 1e-4)")
            if not fig < 1e-4:
                fails.append((k, fig, 1e-4))
            continue
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        fig, bound, own = rel_l2(got[k], ref[k]), base(k), None
        if precision == "bf16":
            # the oracle's own bf16-mode deviation from its exact mode on this case is the yardstick where 1e-2 / 1e-3
            # is not reachable by a correct bf16 kernel (tiny B * H * W)
            own = rel_l2(ref[k], exact[k])
            bound = max(bound, 1.5 * own)
        print(f"  {_conv_id((case, training))} {precision} {k:24s} dev {fig:.2e} bound {bound:.2e}"
              + ("" if own is None else f" (oracle bf16 vs exact {own:.2e})"))
        if not fig < bound:
            fails.append((k, fig, bound))
    if not training:       # eval mode leaves the running statistics alone
        assert int(got["nbt"]) == 0
        assert np.array_equal(got["buf/bn1.running_mean"], p["bn1.running_mean"])
        assert np.array_equal(got["buf/bn1.running_var"], p["bn1.running_var"])
    assert not fails, fails


@pytest.mark.parametrize("run", CONV_RUNS, ids=[_conv_id(r) for r in CONV_RUNS])
def test_conv_module_fp32_vs_fp64_oracle(run):
    _check_conv(run[0], run[1], "fp32")


@pytest.mark.parametrize("run", CONV_RUNS, ids=[_conv_id(r) for r in CONV_RUNS])
def test_conv_module_bf16_vs_bf16_oracle(run):
    _check_conv(run[0], run[1], "bf16")


def test_conv_module_input_gradient_refused_for_padded_channels():
    """dx for in_channels outside {32, 64, 128}: the documented error, not a wrong launch."""
    from deeptreeattention_amd import Hang2020 as H
    B, cin, f, Hh, Ww, pool = CONV_CASES[1]
    m = H.conv_module(cin, f, maxpool_kernel=(2, 2)).to(_dev()).train()
    x = torch.from_numpy(prng.uniform(5, 1, (B, cin, Hh, Ww), -1, 1)).to(_dev()).requires_grad_(True)
    z = m(x, pool=pool)
    with pytest.raises(RuntimeError, match=r"input gradient needs in_channels in \{32,64,128\} \(got 17\)"):
        z.sum().backward()


def test_conv_module_bf16_refuses_what_its_staging_plan_cannot_hold():
    """A bf16 workgroup stages at most 2048 16-byte input vectors: 128 patches of 2x2 (32 filters: 512 rows per workgroup)
    are 4096.  B = 1 runs (CONV_CASES[0]); B = 128 is refused with a message before the conv is launched."""
    from deeptreeattention_amd import Hang2020 as H
    m = H.conv_module(1, 32, maxpool_kernel=(2, 2)).to(_dev()).train()
    m.precision = "bf16"
    with pytest.raises(RuntimeError, match="exceeds the staging plan"):
        m(torch.zeros(128, 1, 2, 2, device=_dev()), pool=True)


# ------------------------------------------------------------------------------------------------------------------
# 3. attention
# ------------------------------------------------------------------------------------------------------------------
# (C, B, H, W)
SPATIAL_CASES = [(32, 1, 4, 4), (32, 2, 6, 9), (32, 3, 24, 24), (64, 1, 2, 2), (64, 2, 5, 8), (128, 1, 1, 1), (128, 2, 3, 2),
                 (32, 130, 5, 5),
                 (32, 3, 23, 23)]    # the largest square 32-channel map whose BACKWARD fits a CU's LDS (see SPATIAL_BWD_REFUSED)
SPECTRAL_CASES = [(32, 1, 1, 1), (32, 2, 6, 9), (32, 3, 24, 24), (64, 2, 5, 8), (128, 2, 3, 2), (64, 130, 2, 2)]
ATT_RUNS = [("spatial", c) for c in SPATIAL_CASES] + [("spectral", c) for c in SPECTRAL_CASES]
# spatial backward keeps the map, its gradient ([H*W][C+1] floats each) and five padded single-channel maps in LDS:
# 2*576*33 + 5*30*30 + 576 + 32 + 512 floats = 174,544 B at 24x24x32, over the 160 KiB of a CU.  launch_stage_bwd refuses
# it (nothing is launched); the forward runs and is compared.
SPATIAL_BWD_REFUSED = {(32, 3, 24, 24)}
NULL_GRAD_CASE = (64, 2, 5, 8)


def _att_id(run):
    kind, (Cc, B, Hh, Ww) = run
    return f"{kind}-C{Cc}-B{B}-{Hh}x{Ww}"


def att_fns(kind):
    if kind == "spectral":
        return O.spectral_attention_spec, O.spectral_attention_fwd, O.spectral_attention_bwd
    return O.spatial_attention_spec, O.spatial_attention_fwd, O.spatial_attention_bwd


def att_feat_shape(kind, case):
    Cc, B, Hh, Ww = case
    ps = O.SPATIAL_POOL[Cc]
    return (B, Cc) if kind == "spectral" else (B, Cc * (Hh // ps) * (Ww // ps))


def _att_draw(kind, case, seed):
    Cc, B, Hh, Ww = case
    p = O.init_params(att_fns(kind)[0]("", Cc), seed=seed)
    x = prng.uniform01(seed, 1, (B, Cc, Hh, Ww))
    da = prng.uniform(seed, 3, (B, Cc, Hh, Ww), -1, 1)
    df = prng.uniform(seed, 4, att_feat_shape(kind, case), -1, 1)
    return p, x, da, df


@functools.lru_cache(maxsize=None)
def att_seed(kind, case):
    """First seed of the case's sequence at which no reference gradient is identically zero.  With U(-1/sqrt(fan_in), ..)
    weights a spatial module's stencil convs often sit behind a dead ReLU (a negative bias over a small map): every
    parameter gradient upstream of it is then exactly 0 and compares equal to anything that is also 0.  Decided by the
    fp64 oracle alone."""
    Cc, B, Hh, Ww = case
    base = 2000 + Cc + 7 * B + 31 * Hh + Ww + (0 if kind == "spectral" else 500)
    _, fwd, bwd = att_fns(kind)
    for seed in range(base, base + 64 * 1000, 1000):
        p, x, da, df = _att_draw(kind, case, seed)
        _, _, cache = fwd(p, "", x, np.float64)
        dx, g = bwd(cache, "", da.astype(np.float64), df.astype(np.float64))
        if all(np.any(v) for v in g.values()) and np.any(dx):
            return seed
    raise AssertionError((kind, case))


def att_inputs(kind, case):
    return _att_draw(kind, case, att_seed(kind, case))


@functools.lru_cache(maxsize=None)
def att_oracle(kind, case, mode="f64", use_da=True, use_df=True):
    """{a, f, dx, g/<name>} and the forward cache; use_da=False: da = None; use_df=False: df = 0."""
    p, x, da, df = att_inputs(kind, case)
    dt = np.float32 if mode == "f32" else np.float64
    _, fwd, bwd = att_fns(kind)
    a, f, cache = fwd(p, "", x, dt)
    dx, g = bwd(cache, "", da.astype(dt) if use_da else None, df.astype(dt) if use_df else np.zeros(df.shape, dt))
    out = {"a": a, "f": f, "dx": dx}
    out.update({"g/" + k: v for k, v in g.items()})
    return out, cache


def att_bound(k):
    return TIGHT if k in ("a", "f") else TOL


@pytest.mark.parametrize("run", ATT_RUNS, ids=[_att_id(r) for r in ATT_RUNS])
def test_attention_vs_fp64_oracle(run):
    from deeptreeattention_amd import Hang2020 as H
    kind, case = run
    p, x, da, df = att_inputs(kind, case)
    m = (H.spectral_attention if kind == "spectral" else H.spatial_attention)(filters=case[0])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in p.items()})
    m = m.to(_dev())
    xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    a, f = m(xt)
    ref, _ = att_oracle(kind, case)
    got = {"a": a.detach().cpu().numpy(), "f": f.detach().cpu().numpy()}
    loss = (a * torch.from_numpy(da).to(_dev())).sum() + (f * torch.from_numpy(df).to(_dev())).sum()
    if kind == "spatial" and case in SPATIAL_BWD_REFUSED:
        with pytest.raises(RuntimeError, match=r"stage_bwd: 24x24x32 patch needs \d+ B of LDS"):
            loss.backward()
    else:
        loss.backward()
        got["dx"] = xt.grad.cpu().numpy()
        for k, prm in m.named_parameters():
            got["g/" + k] = prm.grad.cpu().numpy()
        assert set(got) == set(ref)
    fails = []
    for k in sorted(got):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        fig = rel_l2(got[k], ref[k])
        print(f"  {_att_id(run)} {k:26s} dev {fig:.2e} bound {att_bound(k):.0e}")
        if not fig < att_bound(k):
            fails.append((k, fig))
    assert not fails, fails


def _attention_direct(kind, case, use_da, use_df, null_grad=None):
    """dta_attention_forward / _backward through ctypes: dout_nchw / dfeat / one grads entry may be NULL."""
    from deeptreeattention_amd import _lib
    from deeptreeattention_amd import Hang2020 as H
    L = _lib.lib()
    Cc, B, Hh, Ww = case
    p, x, da, df = att_inputs(kind, case)
    names = H._ATT_NAMES[kind]
    params = [_f32(p[n]) for n in names]
    desc = _lib.AttentionDesc(B, Cc, Hh, Ww, 0 if kind == "spectral" else 1)
    nbytes = L.dta_attention_workspace_bytes(C.byref(desc))
    assert nbytes > 0, L.dta_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
    x_nhwc = _f32(x.transpose(0, 2, 3, 1))
    arr, garr = _lib.PtrArray6(), _lib.PtrArray6()
    grads = [torch.zeros_like(t) for t in params]
    for i, t in enumerate(params):
        arr[i] = t.data_ptr()
        garr[i] = None if i == null_grad else grads[i].data_ptr()
    out = torch.empty(B, Cc, Hh, Ww, dtype=torch.float32, device=_dev())
    feat = torch.empty(att_feat_shape(kind, case), dtype=torch.float32, device=_dev())
    st = _lib.current_stream_ptr()
    _lib.check(L.dta_attention_forward(C.byref(desc), C.byref(arr), _lib.ptr(x_nhwc), _lib.ptr(ws), _lib.ptr(out), _lib.ptr(feat), st),
               "dta_attention_forward")
    dx_nhwc = torch.full((B, Hh * Ww, Cc), SENTINEL, dtype=torch.float32, device=_dev())
    _lib.check(L.dta_attention_backward(C.byref(desc), C.byref(arr), _lib.ptr(x_nhwc), _lib.ptr(ws), _lib.ptr(_f32(da) if use_da else None),
                                        _lib.ptr(_f32(df) if use_df else None), _lib.ptr(dx_nhwc), C.byref(garr), st), "dta_attention_backward")
    got = {"dx": dx_nhwc.view(B, Hh, Ww, Cc).permute(0, 3, 1, 2).cpu().numpy()}
    got.update({"g/" + n: g.cpu().numpy() for n, g in zip(names, grads)})
    return got


@pytest.mark.parametrize("null", ["dfeat", "dout_nchw"])
@pytest.mark.parametrize("kind", ["spectral", "spatial"])
def test_attention_backward_null_gradients(kind, null):
    """Header: "dout_nchw / dfeat ... (either may be null)", "grads[6] ... (null entries are skipped)".  A null dfeat is
    df = 0 in the oracle, a null dout_nchw is da = None; one null grads entry leaves every other gradient as it was."""
    from deeptreeattention_amd import Hang2020 as H
    use_da, use_df = null != "dout_nchw", null != "dfeat"
    ref, _ = att_oracle(kind, NULL_GRAD_CASE, "f64", use_da, use_df)
    got = _attention_direct(kind, NULL_GRAD_CASE, use_da, use_df)
    for k in sorted(ref):
        if k in ("a", "f"):
            continue
        fig = rel_l2(got[k], ref[k])
        print(f"  {kind} {null}=NULL {k:26s} dev {fig:.2e}")
        assert fig < TOL, (k, fig)
    # a weight entry (spectral: conv1's weight, whose GEMM also carries conv1's bias gradient; spatial: the first stencil)
    skip = 0 if kind == "spectral" else 2
    skipped = "g/" + H._ATT_NAMES[kind][skip]
    part = _attention_direct(kind, NULL_GRAD_CASE, use_da, use_df, null_grad=skip)
    assert not part[skipped].any()                       # (the test's own zero-filled buffer: never written)
    for k in sorted(got):
        if k == skipped:
            continue
        assert rel_l2(part[k], got[k]) < 1e-5, k         # (another summation order at most)
        assert rel_l2(part[k], ref[k]) < TOL, k


def test_spatial_attention_below_its_pool_is_refused():
    """32 channels pool 4x4: a 3x3 map has no pooled element.  The workspace query says so and nothing is launched."""
    from deeptreeattention_amd import _lib
    L = _lib.lib()
    desc = _lib.AttentionDesc(1, 32, 3, 3, 1)
    assert L.dta_attention_workspace_bytes(C.byref(desc)) == 0
    assert "spatial_attention: 3x3 map smaller than its 4-pool" in L.dta_last_error().decode()
