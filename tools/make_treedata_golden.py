"""Generate tests/golden/treedata/treedata_reference.npz by running the REFERENCE ITSELF (build container only; needs pandas
and scikit-learn).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_treedata_golden.py <path of a checkout of the reference>

Imports the reference's src/data.py read-only (its GIS / Lightning / dask imports are stubbed: only the import has to
succeed; src/utils.py and src/augmentation.py are the reference's own) and runs its OWN `TreeDataset` (data.py:239-310) on a
handful of tiny .npy crops written to a temporary crop_dir: 6 individuals, 3 years, some (individual, year) pairs without a
row, 26 raw bands (6 after the clip of 10 + 10), 3..7 pixels a side, image_size 5 (so the NEAREST resize both enlarges and
shrinks), the rows of the annotation table interleaved so that `individual.unique()` and `tile_year.unique()` differ from the
sorted order (asserted below).

torchvision is absent here, so the three things the reference takes from it are stand-ins written in this file:
`transforms.functional.resize(..., NEAREST)` is torch.nn.functional.interpolate(mode="nearest") -- the routine torchvision's
tensor resize dispatches to, as tests/golden/make_golden.py already does -- and RandomHorizontalFlip(p=1) /
RandomVerticalFlip(p=1) are torch.flip along the last / the second-last axis, which is what they do to a (C, H, W) tensor when
p = 1.

The file holds only data: the annotation columns (`individual`, `tile_year`, `image_path`, `label`, one entry per row, in
frame order), the raw crops (`raw_<k>` for the k-th entry of `paths`), the data set's own `individuals` and `years`, and
the items `__getitem__` returned, stacked [N][Y][6][5][5] float32: `items_train` / `items_eval` with preload_images on,
`items_train_lazy` / `items_eval_lazy` with it off, and the train items' `labels`.  No reference source is copied anywhere.
tests/golden/treedata/SHA256SUMS is written here."""
import hashlib
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "treedata")
OUT = os.path.join(GOLDEN, "treedata_reference.npz")
sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

IMAGE_SIZE, RAW_BANDS = 5, 26
INDIVIDUALS = ["NEON.T5", "NEON.T2", "NEON.T9", "NEON.T0", "NEON.T7", "NEON.T3"]      # first-appearance order, not sorted
YEARS = [2021, 2019, 2020]                                                            # likewise
# which years each individual has a crop of (in YEARS' order); every year is missing somewhere, one individual has one year
HAVE = [(1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 1), (1, 1, 1)]
LABELS = [3, 0, 2, 2, 1, 0]


def torchvision_stand_in():
    import torch
    import torch.nn.functional as F
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")

    class InterpolationMode:
        NEAREST = "nearest"

    def resize(image, size, interpolation=None):
        assert interpolation == InterpolationMode.NEAREST
        return F.interpolate(image[None], size=tuple(size), mode="nearest")[0]

    class RandomHorizontalFlip:
        def __init__(self, p=0.5):
            assert p == 1

        def __call__(self, image):
            return torch.flip(image, dims=[-1])

    class RandomVerticalFlip:
        def __init__(self, p=0.5):
            assert p == 1

        def __call__(self, image):
            return torch.flip(image, dims=[-2])

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, image):
            for t in self.transforms:
                image = t(image)
            return image

    fn.resize = resize
    tr.functional, tr.InterpolationMode = fn, InterpolationMode
    tr.RandomHorizontalFlip, tr.RandomVerticalFlip, tr.Compose = RandomHorizontalFlip, RandomVerticalFlip, Compose
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    sys.modules["torchvision.transforms.functional"] = fn


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isfile(os.path.join(args[0], "src", "data.py")):
        sys.exit("usage: make_treedata_golden.py <path of a checkout of the reference>")
    import pandas as pd
    warnings.simplefilter("ignore")
    ref = args[0]

    class Anything(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return type(name, (), {})
    for name in ("distributed", "geopandas", "pytorch_lightning", "shapely", "shapely.geometry", "rasterio", "src.generate",
                 "src.CHM", "src.megaplot", "src.neon_paths", "src.models", "src.models.dead"):
        if name not in sys.modules:
            sys.modules[name] = Anything(name)
            sys.modules[name].__all__ = []
    torchvision_stand_in()
    pkg = types.ModuleType("src")
    pkg.__path__, pkg.__file__ = [os.path.join(ref, "src")], os.path.join(ref, "src", "__init__.py")
    sys.modules["src"] = pkg
    D = importlib.import_module("src.data")

    rs = np.random.RandomState(7)
    pairs = [(i, y) for y in range(len(YEARS)) for i in range(len(INDIVIDUALS)) if HAVE[i][y]]
    # frame order: the first rows fix the first-appearance orders above, the rest is shuffled
    head = [(0, 0), (1, 0), (2, 1), (3, 0), (4, 2), (5, 0)]
    assert all(p in pairs for p in head)
    rest = [p for p in pairs if p not in head]
    rest = [rest[k] for k in rs.permutation(len(rest))]
    rows = head + rest
    paths, raws = [], []
    for k, (i, y) in enumerate(rows):
        h, w = rs.randint(3, 8, size=2)
        a = rs.randint(-50, 6000, size=(RAW_BANDS, h, w)).astype(np.int16)      # reflectance crops are int16 on disk
        if k == 2:
            a[:, 0, 0] = 17                # a pixel with no range over its bands
        paths.append("{}_{}.npy".format(INDIVIDUALS[i], YEARS[y]))
        raws.append(a)
    df = pd.DataFrame({"individual": [INDIVIDUALS[i] for i, _ in rows], "tile_year": [YEARS[y] for _, y in rows],
                       "image_path": paths, "label": [LABELS[i] for i, _ in rows]})
    assert list(df.individual.unique()) == INDIVIDUALS != sorted(INDIVIDUALS)
    assert list(df.tile_year.unique()) == YEARS != sorted(YEARS)
    sizes = {r.shape[1] for r in raws} | {r.shape[2] for r in raws}
    assert min(sizes) < IMAGE_SIZE < max(sizes)

    data = {"individual": df.individual.to_numpy().astype(str), "tile_year": df.tile_year.to_numpy().astype(np.int64),
            "image_path": df.image_path.to_numpy().astype(str), "label": df.label.to_numpy().astype(np.int64),
            "paths": np.array(paths), "image_size": np.int64(IMAGE_SIZE)}
    for k, a in enumerate(raws):
        data["raw_%d" % k] = a
    with tempfile.TemporaryDirectory() as crop_dir:
        for p, a in zip(paths, raws):
            np.save(os.path.join(crop_dir, p), a)
        for train in (True, False):
            for preload in (True, False):
                config = {"image_size": IMAGE_SIZE, "preload_images": preload, "crop_dir": crop_dir, "bands": RAW_BANDS - 20}
                ds = D.TreeDataset(df=df.copy(), config=config, train=train)
                assert len(ds) == len(INDIVIDUALS)
                items = [ds[k] for k in range(len(ds))]
                assert [it[0] for it in items] == INDIVIDUALS and len(items[0]) == (3 if train else 2)
                stack = np.stack([np.stack([t.numpy() for t in it[1]["HSI"]]) for it in items]).astype(np.float32)
                assert stack.shape == (len(INDIVIDUALS), len(YEARS), RAW_BANDS - 20, IMAGE_SIZE, IMAGE_SIZE)
                data["items_%s%s" % ("train" if train else "eval", "" if preload else "_lazy")] = stack
                if train and preload:
                    data["labels"] = np.array([int(it[2]) for it in items], np.int64)
                    data["individuals"] = np.array([str(v) for v in ds.individuals])
                    data["years"] = np.array([int(v) for v in ds.years], np.int64)
    for kind in ("train", "eval"):
        assert np.array_equal(data["items_" + kind].view(np.uint32), data["items_%s_lazy" % kind].view(np.uint32))
    for i, have in enumerate(HAVE):
        for y, h in enumerate(have):
            assert bool(data["items_eval"][i, y].any()) == bool(h)
    assert np.array_equal(data["items_train"], data["items_eval"][:, :, :, ::-1, ::-1])

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(OUT, **data)
    digest = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    with open(os.path.join(GOLDEN, "SHA256SUMS"), "w") as f:
        f.write("{}  {}\n".format(digest, os.path.basename(OUT)))
    print(OUT, os.path.getsize(OUT), "bytes;", len(rows), "rows,", len(INDIVIDUALS), "individuals,", len(YEARS), "years")


if __name__ == "__main__":
    main()
