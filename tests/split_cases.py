"""Shared by tests/test_split_cpu.py and tests/test_split_gpu.py: the reference fixture (tools/make_split_golden.py) and
seeded synthetic annotation tables.  Host only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split", "split_reference.npz")


class Fixture:
    def __init__(self):
        self.z = np.load(GOLDEN)
        self.columns = [{n: self.z["t%d_%s" % (k, n)] for n in ("individual", "plot", "taxon", "fixed", "candidate")}
                        for k in range(int(self.z["tables"]))]

    def cases(self, kind):
        """Dicts of one kind ("sp": sample_plots alone, "tts": train_test_split): table, min, orders [iterations][C], the
        reference's train / test row masks, and for "tts" seed, chosen, figures."""
        z = self.z
        for i in range(len(z[kind + "_table"])):
            k, C = int(z[kind + "_table"][i]), int(z[kind + "_candidates"][i])
            n = len(self.columns[k]["individual"])
            c = {"table": k, "min": tuple(int(v) for v in z[kind + "_min"][i]), "orders": z[kind + "_orders"][i][:, :C].astype(np.int32),
                 "train": np.unpackbits(z[kind + "_train_bits"][i])[:n].astype(bool),
                 "test": np.unpackbits(z[kind + "_test_bits"][i])[:n].astype(bool)}
            if kind == "tts":
                c.update(seed=int(z["tts_seed"][i]), chosen=int(z["tts_chosen"][i]), figures=z["tts_figures"][i])
            yield c


def prefiltered(columns, min_train, min_test):
    """The columns the reference's sample_plots sees inside train_test_split (species with more than min_train + min_test
    rows) and the row numbers they came from."""
    keep = (np.bincount(columns["taxon"]) > min_train + min_test)[columns["taxon"]]
    return {n: v[keep] for n, v in columns.items()}, np.flatnonzero(keep)


def synthetic(plots, species, candidates, seed, individuals_per_cell=1.5, fixed_share=0.2):
    """Columns of a random table: `plots` plots of which the first `candidates` are candidates, every species somewhere."""
    rng = np.random.default_rng(seed)
    n_cells = rng.poisson(individuals_per_cell, (plots, species))
    n_cells[rng.integers(0, plots, species), np.arange(species)] += 1          # every species somewhere
    n_cells[np.arange(plots), rng.integers(0, species, plots)] += 1            # every plot holds something
    p, s = np.nonzero(n_cells)
    ind_plot, ind_taxon = np.repeat(p, n_cells[p, s]), np.repeat(s, n_cells[p, s])
    years = rng.integers(1, 4, len(ind_plot))
    individual = np.repeat(np.arange(len(ind_plot)), years)
    order = rng.permutation(len(individual))
    individual = individual[order]
    plot = ind_plot[individual]
    return {"individual": individual, "plot": plot, "taxon": ind_taxon[individual],
            "fixed": rng.uniform(size=len(individual)) < fixed_share, "candidate": plot < candidates}
