"""Species abundance with uncertainty on the host (deeptreeattention_amd/abundance.py): the sampling table, the mirror
`resample_np` against the analytic expectation and against what the REFERENCE's own sample_binomial / sample_confusion
recorded (tests/golden/abundance/abundance_reference.npz, made by tools/make_abundance_golden.py), the edge rules one by one against
a scalar restatement of the rule in Python integers, and the argument checks of the new C entry points.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 1 << 24
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# a scalar restatement of the rule (Python integers, one crown at a time): what the vectorised mirror is held to
# ---------------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _draw(seed, stream, counter):
    key = _mix((seed * 0x9E3779B97F4A7C15 + stream + 1) & M64)
    return _mix((counter * 0x9E3779B97F4A7C15 + key) & M64) >> 40


def scalar_resample(label, score, table, iterations, seed=0, first_iteration=0, mask=None):
    S, N = len(table), len(label)
    out = np.zeros((iterations, S + 1), np.int64)
    for t in range(iterations):
        for i in range(N):
            if mask is not None and not mask[i]:
                continue
            l = int(label[i])
            if not 0 <= l < S:
                out[t, S] += 1
                continue
            counter = ((first_iteration + t) * N + i) & M64
            u = np.float32(_draw(seed, 0, counter)) * np.float32(2.0 ** -24)
            keep = True if score is None else not (u >= np.float32(score[i]))
            drawn = sum(1 for v in table[l] if int(v) <= _draw(seed, 1, counter))
            out[t, l if keep else drawn] += 1
    return out


def random_confusion(rng, S, zero=True):
    """Counts with many zeros, and (S >= 3) a zero row and a zero column."""
    m = rng.integers(0, 6, (S, S)) * (rng.random((S, S)) < 0.6)
    m = m + np.eye(S, dtype=np.int64) * rng.integers(1, 9, S)
    if zero and S >= 3:
        m[S // 2, :] = 0
        m[:, S - 1] = 0
    return m.astype(np.int64)


def random_crowns(rng, N, S):
    """Labels in [-1, S] with a few far outside; scores with NaN, 0, 1, and values outside [0, 1]."""
    label = rng.integers(-1, S + 1, N).astype(np.int64)
    if N > 4:
        label[rng.integers(0, N)] = 2 ** 40 + 1
        label[rng.integers(0, N)] = -2 ** 33
    score = rng.uniform(0.0, 1.0, N).astype(np.float32)
    special = np.array([np.nan, 0.0, 1.0, 1.5, -0.25], np.float32)
    pick = rng.random(N) < 0.3
    score[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return label, score


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def test_table_rows_are_monotone_and_end_at_two_to_the_24():
    from deeptreeattention_amd.abundance import sampling_table
    rng = np.random.default_rng(1)
    for S in (1, 2, 6, 37):
        t = sampling_table(random_confusion(rng, S))
        assert t.dtype == np.uint32 and t.shape == (S, S)
        assert (t[:, -1] == SCALE).all()
        assert (np.diff(t.astype(np.int64), axis=1) >= 0).all()


def test_table_zero_probability_species_has_a_zero_width_interval():
    from deeptreeattention_amd.abundance import sampling_table
    m = np.array([[3, 0, 1, 0, 0],      # a zero inside and trailing zeros
                  [0, 0, 5, 0, 0],      # leading zeros, one species
                  [0, 0, 0, 0, 0],      # a zero row
                  [1, 1, 1, 1, 1],
                  [0, 0, 0, 0, 2]])
    t = sampling_table(m).astype(np.int64)
    lo = np.concatenate([np.zeros((5, 1), np.int64), t[:, :-1]], axis=1)      # species c is drawn for lo[c] <= r < t[c]
    width = t - lo
    for p in (0, 1, 3, 4):
        assert ((width[p] == 0) == (m[p] == 0)).all(), p
    assert t[0].tolist() == [3 * SCALE // 4, 3 * SCALE // 4, SCALE, SCALE, SCALE]       # from the last non-zero column on: 2^24
    assert t[1].tolist() == [0, 0, SCALE, SCALE, SCALE]
    assert t[4].tolist() == [0, 0, 0, 0, SCALE]
    # a zero row is the identity: the label is kept
    assert t[2].tolist() == [0, 0, SCALE, SCALE, SCALE]
    ident = sampling_table(np.zeros((4, 4)))
    for p in range(4):
        assert ident[p].tolist() == [0] * p + [SCALE] * (4 - p)
        for r in (0, 1, SCALE - 1):
            assert int((ident[p] <= r).sum()) == p


def test_table_given_prediction_is_given_label_on_the_transpose_and_floats_are_accepted():
    from deeptreeattention_amd.abundance import sampling_table
    rng = np.random.default_rng(2)
    m = random_confusion(rng, 9)
    assert np.array_equal(sampling_table(m, given="prediction"), sampling_table(m.T, given="label"))
    assert not np.array_equal(sampling_table(m, given="prediction"), sampling_table(m))
    # an already row-stochastic float table gives the same thresholds as its counts (powers of two: the division is exact)
    counts = np.array([[4, 2, 2], [0, 8, 0], [1, 1, 6]])
    stochastic = counts / 8.0
    assert stochastic.dtype == np.float64 and np.allclose(stochastic.sum(1), 1)
    assert np.array_equal(sampling_table(stochastic), sampling_table(counts))
    assert np.array_equal(sampling_table(stochastic.astype(np.float32)), sampling_table(counts))
    with pytest.raises(ValueError, match="given"):
        sampling_table(m, given="truth")
    with pytest.raises(ValueError, match="square"):
        sampling_table(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="non-negative"):
        sampling_table(np.array([[1, -1], [0, 1]]))
    with pytest.raises(ValueError, match="at most"):
        sampling_table(np.eye(257))


# ---------------------------------------------------------------------------------------------------------------------
# the mirror against the analytic expectation and against the reference's recorded results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(golden):
    g = golden(os.path.join("abundance", "abundance_reference.npz"))
    return {k: g[k] for k in g.files}


def expectation(confusion, label, score):
    """Per bin: the expected count sum_i p_ic and its variance sum_i p_ic (1 - p_ic), with
    p_ic = s_i 1(l_i = c) + (1 - s_i) P[l_i][c] for a crown inside [0, S) (a NaN score is 1), bin S otherwise."""
    S = len(confusion)
    P = confusion / np.maximum(confusion.sum(1, keepdims=True), 1)
    p = np.zeros((len(label), S + 1))
    for i, (l, s) in enumerate(zip(label, score)):
        if not 0 <= l < S:
            p[i, S] = 1
            continue
        s = 1.0 if np.isnan(s) else float(s)
        p[i, :S] = (1 - s) * P[l]
        p[i, l] += s
    assert np.allclose(p.sum(1), 1)
    return p.sum(0), (p * (1 - p)).sum(0)


def test_fixture_is_the_committed_one():
    """tests/golden/abundance has a checksum file of its own (tests/golden/SHA256SUMS lists the fixtures directly in
    tests/golden): the file is the one tools/make_abundance_golden.py wrote from the reference."""
    import hashlib
    here = os.path.join(REPO, "tests", "golden", "abundance")
    lines = [ln.split() for ln in open(os.path.join(here, "SHA256SUMS")).read().splitlines() if ln.strip()]
    assert [name for _, name in lines] == sorted(f for f in os.listdir(here) if f.endswith(".npz")) == ["abundance_reference.npz"]
    for digest, name in lines:
        assert hashlib.sha256(open(os.path.join(here, name), "rb").read()).hexdigest() == digest, name


def test_fixture_is_the_documented_one(fixture):
    conf, label, score = fixture["confusion"], fixture["label"], fixture["score"]
    S = 6
    assert conf.shape == (S, S) and label.shape == (96,) and score.shape == (96,) and score.dtype == np.float32
    assert not conf[4].any() and not conf[:, 4].any() and conf[1, 3] == 0
    assert (label[::17] == -1).all() and int((label == S).sum()) == 1 and int(((label < 0) | (label >= S)).sum()) == 7
    assert np.isnan(score[::11]).all() and int((score == 0).sum()) == 1 and int((score == 1).sum()) == 1
    assert int(fixture["ref_iterations"]) == 4000


def test_mirror_and_reference_agree_with_the_analytic_expectation(fixture):
    from deeptreeattention_amd.abundance import resample_np, sampling_table
    conf, label, score = fixture["confusion"], fixture["label"], fixture["score"]
    S, iterations = 6, 400
    mean, var = expectation(conf, label, score)
    got = resample_np(label, score, sampling_table(conf), iterations, seed=0)
    assert got.shape == (iterations, S + 1) and got.dtype == np.int64
    assert (got.sum(1) == len(label)).all()                      # every iteration counts every crown once
    ref_n = int(fixture["ref_iterations"])
    for c in range(S + 1):
        if var[c] == 0:                                          # the absent species: 0; the "other" bin: 7
            assert (got[:, c] == mean[c]).all() and fixture["ref_mean"][c] == mean[c] and fixture["ref_var"][c] == 0, c
            continue
        assert abs(got[:, c].mean() - mean[c]) <= 5 * np.sqrt(var[c] / iterations), (c, got[:, c].mean(), mean[c])
        assert abs(fixture["ref_mean"][c] - mean[c]) <= 5 * np.sqrt(var[c] / ref_n), (c, fixture["ref_mean"][c], mean[c])
    assert var[4] == 0 and mean[4] == 0 and var[S] == 0 and mean[S] == 7
    # the spread, not only the centre: a bin's count is a sum of independent draws, close to normal, so the sample variance
    # of 400 iterations has a relative standard deviation of sqrt(2 / 399) = 7 %: +-30 % is a little over 4 sigma
    live = var > 0
    ratio = got[:, live].var(0, ddof=1) / var[live]
    assert (ratio > 0.7).all() and (ratio < 1.3).all(), ratio


def test_mirror_equals_the_scalar_rule():
    from deeptreeattention_amd.abundance import resample_np, sampling_table
    rng = np.random.default_rng(3)
    for S, N, iterations in ((1, 9, 3), (2, 40, 5), (6, 70, 4), (23, 150, 3)):
        table = sampling_table(random_confusion(rng, S))
        label, score = random_crowns(rng, N, S)
        mask = rng.random(N) < 0.7
        for m in (None, mask):
            for sc in (score, None):
                want = scalar_resample(label, sc, table, iterations, seed=11, first_iteration=2, mask=m)
                got = resample_np(label, sc, table, iterations, seed=11, first_iteration=2, mask=m)
                assert np.array_equal(got, want), (S, N, m is None, sc is None)
    # the counter is formed modulo 2^64, in 64 bits
    table = sampling_table(random_confusion(rng, 6))
    label, score = random_crowns(rng, 65, 6)
    for first in (2 ** 33, 2 ** 64 - 1):
        assert np.array_equal(resample_np(label, score, table, 3, seed=5, first_iteration=first),
                              scalar_resample(label, score, table, 3, seed=5, first_iteration=first))
    # another seed is another sample
    assert not np.array_equal(resample_np(label, score, table, 3, seed=5), resample_np(label, score, table, 3, seed=6))


# ---------------------------------------------------------------------------------------------------------------------
# edge rules, each exact
# ---------------------------------------------------------------------------------------------------------------------
def test_score_one_and_nan_always_keep_and_score_zero_never_keeps():
    from deeptreeattention_amd.abundance import counts_np, resample_np, sampling_table
    rng = np.random.default_rng(4)
    S, N = 5, 200
    conf = np.array([[0, 3, 1, 0, 0],       # the diagonal is zero: a re-drawn crown never lands on its own label
                     [2, 0, 2, 0, 1],
                     [1, 1, 0, 1, 1],
                     [0, 0, 4, 0, 0],
                     [5, 0, 0, 1, 0]])
    table = sampling_table(conf)
    label = rng.integers(0, S, N).astype(np.int64)
    plain = counts_np(label, S)
    for s in (1.0, np.nan, 7.0):
        got = resample_np(label, np.full(N, s, np.float32), table, 6, seed=1)
        assert (got == plain).all(), s
    assert (resample_np(label, None, table, 6, seed=1) == plain).all()
    # score 0 (and below): never kept -- with a zero diagonal every crown moves, so all of species 3 (row: species 2 only)
    # arrives in bin 2, and no crown of species 0 stays in bin 0 unless another row sends one there
    only3 = np.full(N, 3, np.int64)
    for s in (0.0, -1.0):
        got = resample_np(only3, np.full(N, s, np.float32), table, 4, seed=2)
        assert (got[:, 2] == N).all() and got.sum() == 4 * N
    only0 = np.zeros(N, np.int64)
    got = resample_np(only0, np.zeros(N, np.float32), table, 4, seed=2)
    assert (got[:, 0] == 0).all() and (got[:, 1] + got[:, 2] == N).all() and (got[:, 1] > got[:, 2]).all()
    # ... unless the draw lands on the same label: a zero row is the identity
    ident = sampling_table(np.zeros((S, S)))
    assert (resample_np(label, np.zeros(N, np.float32), ident, 3, seed=3) == plain).all()


def test_masked_crowns_are_counted_nowhere_and_other_labels_go_to_the_last_bin():
    from deeptreeattention_amd.abundance import counts_np, resample_np, sampling_table
    rng = np.random.default_rng(5)
    S, N = 4, 120
    table = sampling_table(random_confusion(rng, S, zero=False))
    label, score = random_crowns(rng, N, S)
    mask = (rng.random(N) < 0.5).astype(np.uint8)
    got = resample_np(label, score, table, 5, seed=9, mask=mask)
    assert (got.sum(1) == int(mask.sum())).all()
    other = ((label < 0) | (label >= S)) & (mask != 0)
    assert other.any() and (got[:, S] == int(other.sum())).all()         # whatever their scores
    assert np.array_equal(got, resample_np(label, score, table, 5, seed=9, mask=mask.astype(bool)))
    assert not resample_np(label, score, table, 5, seed=9, mask=np.zeros(N, bool)).any()
    # masking a crown changes nobody else's draw: the counter is the crown's index
    one = np.ones(N, bool)
    inside = np.flatnonzero((label >= 0) & (label < S))
    one[inside[0]] = False
    full, less = resample_np(label, score, table, 5, seed=9), resample_np(label, score, table, 5, seed=9, mask=one)
    assert ((full - less).sum(1) == 1).all() and ((full - less) >= 0).all()
    # counts_np: np.bincount with the same last bin and mask
    assert np.array_equal(counts_np(label, S), np.bincount(np.where((label >= 0) & (label < S), label, S), minlength=S + 1))
    keep = mask != 0
    assert np.array_equal(counts_np(label, S, mask), np.bincount(np.where((label >= 0) & (label < S), label, S)[keep], minlength=S + 1))
    assert counts_np(np.zeros(0, np.int64), S).tolist() == [0] * (S + 1)


def test_first_iteration_is_a_row_of_a_longer_run():
    from deeptreeattention_amd.abundance import resample_np, sampling_table
    rng = np.random.default_rng(6)
    S, N = 6, 300
    table = sampling_table(random_confusion(rng, S))
    label, score = random_crowns(rng, N, S)
    run = resample_np(label, score, table, 12, seed=4)
    assert len({tuple(r) for r in run}) > 1
    for k in (0, 5, 11):
        assert np.array_equal(resample_np(label, score, table, 1, seed=4, first_iteration=k)[0], run[k])
    assert np.array_equal(resample_np(label, score, table, 4, seed=4, first_iteration=8), run[8:])
    assert resample_np(label, score, table, 0).shape == (0, S + 1)


def test_summary_is_mean_and_quantiles_over_the_iterations():
    from deeptreeattention_amd.abundance import summary
    counts = np.arange(40, dtype=np.int64).reshape(10, 4) % 7
    s = summary(counts)
    assert s.q == (0.025, 0.5, 0.975) and s.mean.shape == (4,) and s.quantiles.shape == (3, 4)
    assert np.allclose(s.mean, counts.mean(0)) and np.allclose(s.quantiles[1], np.median(counts, axis=0))
    assert np.allclose(summary(counts, q=(0.0, 1.0)).quantiles, [counts.min(0), counts.max(0)])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: declared, exported, and every bad argument refused on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deeptreeattention_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_and_exported(lib):
    from deeptreeattention_amd import _lib, abundance
    hdr = open(os.path.join(REPO, "include", "dta_hip.h")).read()
    names = set(re.findall(r"\b(dta_[a-z_0-9]+)\s*\(", hdr))
    for n in ("dta_abundance_resample", "dta_abundance_counts", "dta_abundance_workspace_bytes"):
        assert n in names and hasattr(lib, n), n
    max_species = int(re.search(r"#define\s+DTA_ABUNDANCE_MAX_SPECIES\s+(\d+)", hdr).group(1))
    assert max_species >= 256 and max_species == _lib.ABUNDANCE_MAX_SPECIES == abundance.MAX_SPECIES
    assert lib.dta_abi_version() == 2 and int(re.search(r"#define\s+DTA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2


def test_bad_arguments_are_refused_before_any_launch(lib):
    """None of these reaches a kernel launch (this machine has no GPU): the pointers are host buffers nobody dereferences."""
    from deeptreeattention_amd import _lib
    MAXS = _lib.ABUNDANCE_MAX_SPECIES
    buf = (C.c_ubyte * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30

    def err():
        return lib.dta_last_error().decode()

    def resample(label=p, score=p, mask=p, n=10, table=p, species=6, iterations=3, counts=p, ws=p, ws_bytes=big):
        return lib.dta_abundance_resample(label, score, mask, n, table, species, iterations, 0, 0, counts, ws, ws_bytes, None)

    def counts(label=p, mask=p, n=10, species=6, out=p, ws=p, ws_bytes=big):
        return lib.dta_abundance_counts(label, mask, n, species, out, ws, ws_bytes, None)

    for kw in ({"label": None}, {"table": None}, {"counts": None}, {"ws": None}):
        assert resample(**kw) != 0 and "dta_abundance_resample" in err() and "null" in err(), kw
    for kw in ({"label": None}, {"out": None}, {"ws": None}):
        assert counts(**kw) != 0 and "dta_abundance_counts" in err() and "null" in err(), kw
    for kw, what in (({"n": 0}, "n="), ({"n": -5}, "n="), ({"species": 0}, "species"), ({"species": MAXS + 1}, "species"),
                     ({"iterations": -1}, "iterations")):
        assert resample(**kw) != 0 and "dta_abundance_resample" in err() and what in err(), (kw, err())
    for kw, what in (({"n": 0}, "n="), ({"species": 0}, "species"), ({"species": MAXS + 1}, "species")):
        assert counts(**kw) != 0 and "dta_abundance_counts" in err() and what in err(), (kw, err())
    # the workspace: sized by the shape alone, refused when short
    need = lib.dta_abundance_workspace_bytes(10, 6, 3)
    assert need >= 8 * 3 * 7
    assert lib.dta_abundance_workspace_bytes(1000000, 200, 100) > lib.dta_abundance_workspace_bytes(1000, 200, 100) > 0
    assert resample(ws_bytes=need - 1) != 0 and "dta_abundance_resample" in err() and "workspace" in err()
    need1 = lib.dta_abundance_workspace_bytes(10, 6, 1)
    assert counts(ws_bytes=need1 - 1) != 0 and "dta_abundance_counts" in err() and "workspace" in err()
    for args in ((0, 6, 3), (10, 0, 3), (10, MAXS + 1, 3), (10, 6, -1)):
        assert lib.dta_abundance_workspace_bytes(*args) == 0 and "dta_abundance_workspace_bytes" in err(), args
    assert lib.dta_abundance_workspace_bytes(10, MAXS, 0) > 0
    # no iterations: nothing to do, and nothing launched
    assert resample(iterations=0) == 0


def test_python_route_checks_its_arguments_on_the_host():
    import torch
    from deeptreeattention_amd import abundance
    with pytest.raises(ValueError, match="label"):
        abundance.resample(torch.zeros(4, dtype=torch.int64), None, np.full((1, 1), SCALE, np.uint32))
    with pytest.raises(ValueError, match="label"):
        abundance.counts(np.zeros(4, np.int64), 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        abundance.resample_np(np.zeros(4, np.int64), None, np.array([[5, 3], [0, SCALE]], np.uint32), 1)
    with pytest.raises(ValueError, match="non-decreasing"):
        abundance.device_table(np.array([[0, 7], [0, SCALE]], np.uint32), "cpu")
    assert abundance.device_table(abundance.sampling_table(np.eye(3)), "cpu").dtype == torch.uint32
