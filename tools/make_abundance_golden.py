"""Generate tests/golden/abundance/abundance_reference.npz by running the REFERENCE ITSELF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_abundance_golden.py <path of a checkout of the reference>

Imports the reference's src/multinomial.py read-only (`geopandas` and `distributed` are stubbed: only the import has to
succeed) and calls its `sample_binomial` (multinomial.py:61-67) and `sample_confusion` (:69-77) crown by crown, in the order
`run` (:28-35) applies them -- every crown's binomial first, then every crown's draw from the row of its predicted taxon --
for ITERATIONS iterations under np.random.seed(0).  The rows are normalised the way `format_confusion_json` (:41-50)
normalises them (`[y / sum(x) for y in x]`).

The file holds only data: the inputs (`confusion` int64 [S][S], rows = label; `label` int64 [N]; `score` float32 [N]) and
the reference's per-bin mean and variance of the counts over the iterations (`ref_mean`, `ref_var` float64 [S + 1], bin S =
DEAD and unresolved crowns; `ref_iterations`).  No reference source is copied anywhere.  The fixture has a folder and a
checksum file of its own (tests/golden/abundance/SHA256SUMS, written here), as tests/golden/validation has:
tests/golden/SHA256SUMS lists the fixtures directly in tests/golden and stays as it is.

The fixture: S = 6 species, N = 96 crowns; species 4 is absent from the confusion matrix (zero row and zero column); one
off-diagonal entry is zero; every 17th crown is unresolved (-1) and one is DEAD (label S): 7 crowns in the last bin; scores
uniform in 0.05-1 with every 11th NaN, one exactly 0 and one exactly 1.  The reference knows no unresolved label: such a
crown goes through it as "DEAD", which it hands back unchanged.
"""
import hashlib
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "abundance")
OUT = os.path.join(GOLDEN, "abundance_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

S, N, ABSENT, ITERATIONS = 6, 96, 4, 4000
DEAD_AT, ZERO_AT, ONE_AT = 50, 5, 7


def fixture():
    rs = np.random.RandomState(7)
    confusion = rs.randint(1, 7, (S, S)).astype(np.int64) + 20 * np.eye(S, dtype=np.int64)
    confusion[ABSENT, :] = 0
    confusion[:, ABSENT] = 0
    confusion[1, 3] = 0
    present = np.array([s for s in range(S) if s != ABSENT])
    label = present[rs.randint(0, len(present), N)].astype(np.int64)
    label[::17] = -1
    label[DEAD_AT] = S
    score = rs.uniform(0.05, 1.0, N).astype(np.float32)
    score[::11] = np.nan
    score[ZERO_AT], score[ONE_AT] = 0.0, 1.0
    assert all(0 <= label[i] < S for i in (ZERO_AT, ONE_AT)) and int(((label < 0) | (label >= S)).sum()) == 7
    return confusion, label, score


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "multinomial.py")):
        sys.exit("usage: make_abundance_golden.py <path of a checkout of the reference>")
    for name in ("geopandas", "distributed"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["distributed"].wait = lambda *a, **k: None
    sys.path.insert(0, sys.argv[1])
    from src import multinomial as M

    confusion, label, score = fixture()
    taxa = ["T{}".format(s) for s in range(S)]
    rows = {taxa[p]: [y / sum(confusion[p]) for y in confusion[p]] for p in range(S) if confusion[p].sum() > 0}
    names = [taxa[l] if 0 <= l < S else "DEAD" for l in label]
    bin_of = {t: s for s, t in enumerate(taxa)}
    bin_of["DEAD"] = S
    scores = [float(x) for x in score]

    np.random.seed(0)
    counts = np.zeros((ITERATIONS, S + 1), np.int64)
    for it in range(ITERATIONS):
        keep = [M.sample_binomial(x) for x in scores]
        drawn = [M.sample_confusion(t, rows) for t in names]
        for k, t, d in zip(keep, names, drawn):
            counts[it, bin_of[t] if k == 1 else (S if isinstance(d, str) else int(d))] += 1
    assert (counts.sum(1) == N).all()

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(OUT, confusion=confusion, label=label, score=score, ref_mean=counts.mean(0), ref_var=counts.var(0, ddof=1),
             ref_iterations=np.int64(ITERATIONS))
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes; mean", np.round(counts.mean(0), 3))


if __name__ == "__main__":
    main()
