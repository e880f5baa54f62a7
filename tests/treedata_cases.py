"""Shared by tests/test_treedata_cpu.py and tests/test_treedata_gpu.py: the reference fixture
(tools/make_treedata_golden.py: the reference's own TreeDataset on a handful of tiny crops), seeded synthetic pools and the
hand-written batch plan.  Host only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "treedata", "treedata_reference.npz")


class Fixture:
    def __init__(self):
        z = self.z = np.load(GOLDEN, allow_pickle=False)
        self.columns = {n: z[n] for n in ("individual", "tile_year", "image_path", "label")}
        self.image_size = int(z["image_size"])
        self.raw_by_path = {str(p): z["raw_%d" % k] for k, p in enumerate(z["paths"])}
        self.individuals = [str(v) for v in z["individuals"]]
        self.years = [int(v) for v in z["years"]]

    def raw(self):
        """raw[n][y] in the reference's individual and year order, None where the table has no row."""
        at = {}
        for ind, yr, p in zip(self.columns["individual"], self.columns["tile_year"], self.columns["image_path"]):
            at[(str(ind), int(yr))] = self.raw_by_path[str(p)]
        return [[at.get((i, y)) for y in self.years] for i in self.individuals]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def synthetic_crops(n, years, bands, size, seed, missing=0.25):
    """float32 [n][years][bands][size][size] in [0, 1) with whole (individual, year) slots zeroed, and the present mask.
    Every value is distinct enough that a wrong row, plane or pixel shows."""
    rng = np.random.default_rng(seed)
    crops = rng.random((n, years, bands, size, size), dtype=np.float32)
    crops[crops == 0] = 0.5
    present = rng.random((n, years)) >= missing
    present[:, 0] |= ~present.any(1)            # every individual has a year
    crops[~present] = 0
    return crops, present.astype(np.uint8)


# The batch plan, by hand: level sizes (7, 130, 64, 1, 200) at B = 64.
#   nb = ceil(n / 64) = (1, 3, 1, 1, 4); the epoch has 4 steps; level l brings batch s mod nb_l
PLAN_SIZES, PLAN_B = (7, 130, 64, 1, 200), 64
PLAN_NB, PLAN_STEPS = [1, 3, 1, 1, 4], 4
PLAN_TABLE = [  # per step: (start, count) per level
    [(0, 7), (0, 64), (0, 64), (0, 1), (0, 64)],
    [(0, 7), (64, 64), (0, 64), (0, 1), (64, 64)],
    [(0, 7), (128, 2), (0, 64), (0, 1), (128, 64)],
    [(0, 7), (0, 64), (0, 64), (0, 1), (192, 8)],
]
# with drop_last: nb = floor(n / 64); the levels of 7 and 1 entries have no batch at all (refused); without them
PLAN_DROP_SIZES = (130, 64, 200)
PLAN_DROP_NB, PLAN_DROP_STEPS = [2, 1, 3], 3
PLAN_DROP_TABLE = [
    [(0, 64), (0, 64), (0, 64)],
    [(64, 64), (0, 64), (64, 64)],
    [(0, 64), (0, 64), (128, 64)],
]
