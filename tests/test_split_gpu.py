"""The train/test plot split search on the device: SplitTable.search (dta_split_search) against split.search_np, and
through the recorded orders against the reference's own results.  Everything is integer arithmetic and one float64
comparison per species, so equality is the bar: there is no tolerance."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_C = 4096


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    return SC.Fixture()


@functools.lru_cache(maxsize=None)
def table(S, C, seed=0):
    """A seeded table of S species with C candidate plots out of C + 3, some 40 000 individuals at the most."""
    from deeptreeattention_amd import split
    plots = C + 3
    cols = SC.synthetic(plots, S, C, seed, individuals_per_cell=min(1.5, 4e4 / (plots * S)))
    t = split.SplitTable.from_columns(**cols)
    assert t.n_species == S and t.n_candidates == C
    return t


def equal(got, want, membership=True):
    """Every output of a device search against the definition's."""
    assert str(got.species.dtype) == "torch.int32" and str(got.best.dtype) == "torch.int64"
    assert str(got.train_rows.dtype) == "torch.int64" and str(got.test_plots.dtype) == "torch.int32"
    assert np.array_equal(got.species.cpu().numpy(), want.species)
    assert np.array_equal(got.train_rows.cpu().numpy(), want.train_rows)
    assert np.array_equal(got.test_plots.cpu().numpy(), want.test_plots)
    assert tuple(got.best.cpu().tolist()) == want.best
    if membership:
        assert np.array_equal(got.membership.cpu().numpy(), want.membership)
        assert np.array_equal(got.taxa.cpu().numpy(), want.taxa)
    else:
        assert got.membership is None and got.taxa is None


def both(t, dev, iterations, **kw):
    from deeptreeattention_amd import split
    if t.device is None:
        t.to(dev)
    want = split.search_np(t, iterations, **kw)
    got = t.search(iterations, membership=True, taxa=True, **kw)
    equal(got, want)
    return got, want


@pytest.mark.parametrize("S", [1, 3, 64, 65, 200, 256])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 257, MAX_C])
def test_search_equals_the_definition(dev, S, C):
    got, want = both(table(S, C), dev, 5, seed=S + C)
    if C >= 63 and S >= 3:
        assert want.test_plots.min() >= 1 and len({tuple(m) for m in want.membership}) > 1      # the iterations differ


@pytest.mark.parametrize("iterations", [1, 5, 1003])
def test_iteration_counts_and_the_best(dev, iterations):
    t = table(65, 65)
    got, want = both(t, dev, iterations, seed=9, min_train=3, min_test=2)
    b = want.best[0]
    assert want.species[b] == want.species.max() and want.train_rows[b] == want.train_rows[want.species == want.species.max()].max()
    if iterations == 1003:
        top = np.flatnonzero((want.species == want.best[1]) & (want.train_rows == want.best[2]))
        assert b == top[0]
        assert len(np.unique(want.species)) > 1 or len(np.unique(want.train_rows)) > 1
    # the usual use: search without the tables, then the best iteration alone with them
    plain = t.search(iterations, seed=9, min_train=3, min_test=2)
    equal(plain, want, membership=False)
    one = t.search(1, seed=9, first_iteration=b, min_train=3, min_test=2, membership=True, taxa=True)
    assert np.array_equal(one.membership.cpu().numpy()[0], want.membership[b]) and np.array_equal(one.taxa.cpu().numpy()[0], want.taxa[b])
    assert one.best.cpu().tolist() == [0, want.best[1], want.best[2], want.best[3]]


def test_no_iterations_launch_nothing(dev):
    t = table(3, 2).to(dev)
    r = t.search(0, membership=True)
    assert r.species.shape == (0,) and r.membership.shape == (0, 2) and r.taxa is None and r.best.cpu().tolist() == [-1, 0, 0, 0]


@pytest.mark.parametrize("first", [2 ** 32 // 65 - 2, 2 ** 64 // 65 - 2, 2 ** 64 - 3, 2 ** 63 + 12345])
def test_counter_crosses_the_32_and_64_bit_limits(dev, first):
    """counter = iteration * C + j modulo 2^64: iteration * 65 passes 2^32 / 2^64 inside the call, and first_iteration + t
    itself wraps."""
    from deeptreeattention_amd import split
    got, want = both(table(65, 65), dev, 5, seed=1, first_iteration=first)
    o = split.order_np(65, [(first + t) % 2 ** 64 for t in range(5)], seed=1)
    assert len({tuple(r) for r in o.tolist()}) == 5


def columns_of(A):
    """One single-row individual per count of the [plots][species] array A."""
    p, s = np.nonzero(A)
    plot, taxon = np.repeat(p, A[p, s]), np.repeat(s, A[p, s])
    return {"individual": np.arange(len(plot)), "plot": plot, "taxon": taxon, "fixed": np.zeros(len(plot), bool)}


def test_every_species_complete_after_the_first_plot(dev):
    from deeptreeattention_amd import split
    A = np.full((9, 70), 4)             # 36 individuals a species: floor = max(1.8, 3) = 3 < 4
    t = split.SplitTable.from_columns(**columns_of(A))
    got, want = both(t, dev, 7, seed=2)
    assert (want.test_plots == 1).all() and (want.species == 70).all()


def test_no_species_ever_completes(dev):
    from deeptreeattention_amd import split
    cols = SC.synthetic(70, 65, 67, 5)
    t = split.SplitTable.from_columns(**cols)
    got, want = both(t, dev, 4, seed=2, min_train=1, min_test=10 ** 6)
    assert (want.test_plots == 67).all() and (want.species == 0).all()      # every candidate taken, nothing left to train on


def test_a_count_equal_to_the_floor_keeps_the_species_wanted(dev):
    """40 individuals, two a plot: floor = max(40 * 0.05, 1) = 2.0.  After the first plot the count EQUALS the floor, which
    does not complete the species (strict >): every iteration takes exactly two plots; with >= it would take one."""
    from deeptreeattention_amd import split
    for S in (1, 5):
        A = np.full((20, S), 2)
        t = split.SplitTable.from_columns(**columns_of(A))
        assert (t.floor(1) == 2.0).all()
        got, want = both(t, dev, 9, seed=4, min_train=1, min_test=1)
        assert (want.test_plots == 2).all() and (got.test_plots.cpu().numpy() == 2).all()
        assert (want.train_rows == 36 * S).all()


def test_recorded_orders_through_the_device_give_the_reference_rows(dev):
    from deeptreeattention_amd import split
    fx = fixture()
    tables = {}
    for c in fx.cases("sp"):
        t = tables.setdefault(c["table"], split.SplitTable.from_columns(**fx.columns[c["table"]], device=dev))
        r = t.search(1, orders=c["orders"], min_train=c["min"][0], min_test=c["min"][1], membership=True, taxa=True)
        train, test = split.rows_np(t, r.membership[0], r.taxa[0])
        assert np.array_equal(train, c["train"]) and np.array_equal(test, c["test"]), c["min"]
        assert r.best.cpu().tolist() == [0, len(np.unique(t.taxon[c["test"]])), int(c["train"].sum()), int(r.membership[0].sum())]
    for c in fx.cases("tts"):
        cols = fx.columns[c["table"]]
        sp = split.train_test_split(cols, c["min"][0], c["min"][1], iterations=len(c["orders"]), orders=c["orders"], device=dev)
        assert np.array_equal(sp.train, c["train"]) and np.array_equal(sp.test, c["test"]) and sp.iteration == c["chosen"]
        sub, _ = SC.prefiltered(cols, *c["min"])
        import torch
        r = split.SplitTable.from_columns(**sub, device=dev).search(
            len(c["orders"]), orders=torch.from_numpy(c["orders"]).to(dev), min_train=c["min"][0], min_test=c["min"][1])
        assert np.array_equal(r.species.cpu().numpy(), c["figures"][:, 0]) and np.array_equal(r.train_rows.cpu().numpy(), c["figures"][:, 1])
        assert int(r.best[0]) == c["chosen"]


def test_train_test_split_with_the_hash_equals_its_definition(dev):
    from deeptreeattention_amd import split
    cols = fixture().columns[0]
    want = split.train_test_split_np(cols, 5, 3, iterations=50, seed=6)
    got = split.train_test_split(cols, 5, 3, iterations=50, seed=6, device=dev)
    assert got.iteration == want.iteration and np.array_equal(got.train, want.train) and np.array_equal(got.test, want.test)
    assert list(got.species) == list(want.species) and got.test_plots == want.test_plots
    assert not (got.train & got.test).any() and got.train.sum() > 0 and got.test.sum() > 0


def test_rerun_stream_and_prefilled_outputs(dev):
    import torch
    from deeptreeattention_amd import split
    t = table(200, 257)
    got, want = both(t, dev, 64, seed=3)
    again = t.search(64, seed=3, membership=True, taxa=True)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # outputs full of garbage are overwritten in full, on a stream that is not the default one
    out = split.SplitSearch(*(torch.full(tuple(x.shape), 0xAB if x.dtype == torch.uint8 else -0x5A5A5A5A, dtype=x.dtype, device=dev)
                              for x in got))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        r = t.search(64, seed=3, membership=True, taxa=True, out=out)
    stream.synchronize()
    assert all(a is b for a, b in zip(r, out))
    equal(r, want)
