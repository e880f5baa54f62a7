"""Generate tests/golden/canopy/canopy_reference.npz by running the REFERENCE ITSELF (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_canopy_golden.py <path of a checkout of the reference>

Imports the reference's src/CHM.py read-only (`rasterstats`, `geopandas` and `src.neon_paths` are stubbed: only the import
has to succeed) and calls
  * its `non_zero_99_quantile` (CHM.py:9-14) on every box's slice of a small CHM raster, handed over as rasterstats hands a
    zone to an `add_stats` function: a masked array with the NaN and nodata cells masked;
  * its `height_rules` (CHM.py:58-95) on a small table of CHM / field heights, with its default parameters and with one
    other parameter set.
The file holds only data: the inputs and what the reference returned.  No reference source is copied anywhere.  The fixture
has a folder and a checksum file of its own (tests/golden/canopy/SHA256SUMS, written here), as tests/golden/abundance has:
tests/golden/SHA256SUMS lists the fixtures directly in tests/golden and stays as it is.

The statistic: `chm` float32 [48][56] of heights in 0.5-30 m with four kinds of special cells -- NaN and -9999 (nodata)
cells sprinkled over the left half, rows 30-40 x columns 0-12 below the 0.5 m floor, rows 0-18 x columns 0-22 heights of
27-30 m rounded to 0.1 m so that ties fall on the lo / hi ranks -- and `boxes` int32 [M][4], all inside the raster, found by a seeded search so
that their kept counts are exactly KEPT (in the tie region: KEPT_TIES): 0, 1, 2, 3, then 100, 101, 102 and 201 (at 101 and
201 the weight t is exactly 0), and a few in between.  `ref_q99` float32 [M] is the reference's answer, `kept` int32 [M]
the number of cells >= 0.5 in each box.

The rules: `chm_height` float32 [K], `field_height` float64 [K], `ref_keep_default` bool [K] (min 1, diff 4, limit 8) and
`ref_keep_other` (OTHER): NaN on either side and on both, equal heights, differences of exactly max_diff and limit and one
float next to them, CHM at, just under and just over min_chm, then random rows.
"""
import hashlib
import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "canopy")
OUT = os.path.join(GOLDEN, "canopy_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

H, W, NODATA = 48, 56, -9999.0
KEPT = (0, 1, 2, 3, 7, 50, 100, 101, 102, 150, 201, 333)
KEPT_TIES = (2, 3, 50, 100, 101, 102, 201)
OTHER = (2.0, 2.5, 5.0)          # min_CHM_height, max_CHM_diff, CHM_height_limit of ref_keep_other


def raster():
    rs = np.random.RandomState(11)
    chm = rs.uniform(0.5, 30.0, (H, W)).astype(np.float32)
    chm[:19, :23] = np.round(rs.uniform(27.0, 30.0, (19, 23)), 1).astype(np.float32)   # 31 distinct heights: ties
    chm[30:41, :13] = rs.uniform(0.0, 0.49, (11, 13)).astype(np.float32)
    left = chm[:, :28]
    left[rs.random_sample(left.shape) < 0.04] = np.nan
    left[rs.random_sample(left.shape) < 0.04] = NODATA
    return chm


def kept_count(chm, b):
    with np.errstate(invalid="ignore"):
        return int((chm[b[0]:b[2], b[1]:b[3]] >= np.float32(0.5)).sum())


def find_boxes(chm):
    """For every wanted kept count the first box of a seeded random sequence that has it."""
    rs = np.random.RandomState(12)
    boxes = []
    for region, wanted in (((0, 0, H, W), KEPT), ((0, 0, 19, 23), KEPT_TIES)):
        todo = list(wanted)
        for _ in range(400000):
            if not todo:
                break
            r0, c0 = rs.randint(region[0], region[2]), rs.randint(region[1], region[3])
            r1, c1 = rs.randint(r0 + 1, region[2] + 1), rs.randint(c0 + 1, region[3] + 1)
            k = kept_count(chm, (r0, c0, r1, c1))
            if k in todo:
                todo.remove(k)
                boxes.append((r0, c0, r1, c1))
        assert not todo, todo
    boxes.append((0, 0, H, W))
    return np.array(boxes, np.int32)


def rule_rows():
    rs = np.random.RandomState(13)
    nan = np.nan
    one = np.float32(1)
    rows = [(nan, 5.0), (5.0, nan), (nan, nan), (0.9, 3.0), (1.0, 3.0), (np.nextafter(one, np.float32(0)), 3.0),
            (np.nextafter(one, np.float32(2)), 3.0), (10.0, 10.0), (14.0, 10.0), (np.nextafter(np.float32(14), one), 10.0),
            (2.0, 10.0), (2.1, 10.0), (2.0, np.nextafter(10.0, 0.0)), (20.0, 10.0), (3.0, 30.0), (0.5, 0.5), (1.5, 1.0),
            (12.5, 10.0), (12.0, 10.0), (5.0, 10.0), (5.5, 10.0), (2.0, 2.0), (1.99, 2.0), (9.0, 17.0), (9.0, 13.0)]
    for _ in range(40):
        rows.append((rs.uniform(0.0, 30.0), rs.uniform(0.0, 30.0) if rs.random_sample() > 0.15 else nan))
    chm_height = np.array([r[0] for r in rows], np.float32)
    field = np.array([r[1] for r in rows], np.float64)
    return chm_height, field


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "src", "CHM.py")):
        sys.exit("usage: make_canopy_golden.py <path of a checkout of the reference>")
    for name in ("rasterstats", "geopandas", "src.neon_paths"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, sys.argv[1])
    import src
    src.neon_paths = sys.modules["src.neon_paths"]
    from src import CHM as R
    import pandas as pd

    chm = raster()
    boxes = find_boxes(chm)
    ref, kept = [], []
    for b in boxes:
        zone = chm[b[0]:b[2], b[1]:b[3]]
        masked = np.ma.masked_array(zone, mask=np.isnan(zone) | (zone == np.float32(NODATA)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                          # "All-NaN slice" for a box without a kept cell
            got = R.non_zero_99_quantile(masked)
        assert np.asarray(got).dtype == np.float32, np.asarray(got).dtype
        ref.append(got)
        kept.append(kept_count(chm, b))
    ref = np.array(ref, np.float32)
    assert sorted(kept[:len(KEPT)]) == list(KEPT) and sorted(kept[len(KEPT):-1]) == list(KEPT_TIES), kept

    chm_height, field = rule_rows()

    def rules(*params):
        df = pd.DataFrame({"CHM_height": chm_height.astype(np.float64), "height": field})
        names = ("min_CHM_height", "max_CHM_diff", "CHM_height_limit")
        out = R.height_rules(df, **dict(zip(names, params)))
        keep = np.zeros(len(chm_height), bool)
        keep[out.index.values] = True
        return keep

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(OUT, chm=chm, boxes=boxes, ref_q99=ref, kept=np.array(kept, np.int32), chm_height=chm_height,
             field_height=field, ref_keep_default=rules(), ref_keep_other=rules(*OTHER), other=np.array(OTHER, np.float64))
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes; kept", kept, "q99", np.round(ref, 3))


if __name__ == "__main__":
    main()
