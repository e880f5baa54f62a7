"""The validation-epoch fixture's recipe: shapes, seeds and inputs (NumPy + oracle/prng.py only), shared by the generator
(make_validation_golden.py, which runs the reference on them) and by the tests (which run this package on them)."""
import numpy as np

from oracle import prng

VALIDATION = dict(years=3, bands=16, size=11, classes=(2, 5, 7), batches=(24, 24, 10), param_seed=701, input_seed=740,
                  head_scale=64.0, min_gap=1e-4, max_excluded=0.05)
# the second batch of level 1 lacks year 2 (an all-zero tensor: reference year.py:27 skips it)
ZERO_YEAR = dict(batch=1, level=1, year=2)


def weight(classes):
    """Class weights of a level: uneven, all positive."""
    return (0.5 + 0.25 * (np.arange(classes) % 5)).astype(np.float32)


def inputs(batch, level):
    """([year arrays (B, bands, 11, 11) float32 in [0, 1)], labels int64 (B,)) of one validation batch of one level."""
    c = VALIDATION
    B, seed = c["batches"][batch], c["input_seed"] + 10 * level + batch
    imgs = [prng.uniform01(seed, yy, (B, c["bands"], c["size"], c["size"])) for yy in range(c["years"])]
    if batch == ZERO_YEAR["batch"] and level == ZERO_YEAR["level"]:
        imgs[ZERO_YEAR["year"]] = np.zeros_like(imgs[ZERO_YEAR["year"]])
    return imgs, prng.randint(seed, 7, (B,), c["classes"][level])


def params(level, init_params, spec):
    """The level's state dict (oracle.hang2020_np.init_params: randomised BatchNorm affine AND running statistics), with the
    last classifier head's WEIGHT scaled up (the bias is left alone): with the default initialisation the bias decides every
    row alike; scaled, the features do, the softmax is not flat and few rows have a top-1 / top-2 gap under min_gap."""
    c = VALIDATION
    p = init_params(spec(c["years"], c["bands"], c["classes"][level]), seed=c["param_seed"] + level)
    for k in p:
        if k.endswith("classifier3.fc1.weight"):
            p[k] = (np.asarray(p[k]) * np.float32(c["head_scale"])).astype(np.float32)
    return p
