"""The inputs tests/test_evaluate_cpu.py and tests/test_evaluate_gpu.py share (NumPy only): the recorded reference cases of
tests/golden/evaluate, the rows the counting kernel is run on and the tables the report kernel is run on."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate")
RECORDED = ("ref_site_same", "ref_site_disjoint", "ref_genus_within", "ref_genus_cross", "synthetic", "no_error")
SITES = 7                       # of the synthetic case, whose `site` column holds their codes
_cache = {}


def recorded(name):
    """One recorded case: arrays true / pred (/ site / individual / first), the two tables with integer keys, the
    reference's numbers, and n_species."""
    if "npz" not in _cache:
        _cache["npz"] = np.load(os.path.join(GOLDEN, "evaluate_reference.npz"))
        _cache["json"] = json.load(open(os.path.join(GOLDEN, "evaluate_reference.json")))
    z, rec = _cache["npz"], _cache["json"][name]
    c = {k: z["{}_{}".format(name, k)] for k in ("true", "pred", "site", "individual", "first") if "{}_{}".format(name, k) in z.files}
    for k in ("site_lists", "scientific"):
        if k in rec:
            c[k] = {int(a): b for a, b in rec[k].items()}
    for k in ("site_confusion", "genus_confusion"):
        if k in rec:
            c[k] = rec[k]
    keys = [a for k in ("site_lists", "scientific") if k in c for a in c[k]]
    c["n_species"] = int(max([c["true"].max(), c["pred"].max()] + keys)) + 1
    return c


# ---- rows for the count --------------------------------------------------------------------------------------------------
def rows(n, S, G, seed, group_dtype=np.int64, with_group=True, with_mask=False, bad=False, hot=0.0):
    """n rows over S species and G groups; hot: that share of the rows sits on three diagonal entries; bad: some rows carry
    a label, prediction or group one step outside its range on either side."""
    rs = np.random.RandomState(seed)
    t, p = rs.randint(0, S, n).astype(np.int64), rs.randint(0, S, n).astype(np.int64)
    g = rs.randint(0, G, n)
    if hot:
        pick = rs.rand(n) < hot
        t[pick] = rs.randint(0, min(3, S), pick.sum())
        p[pick] = t[pick]
        g[pick] = 0
    if bad:
        for k, (arr, v) in enumerate(((t, -1), (p, -1), (p, S), (g, G), (t, S), (g, -1))):
            arr[k::11] = v
    return {"labels": t, "preds": p, "group": g.astype(group_dtype) if with_group else None,
            "mask": rs.rand(n) < 0.6 if with_mask else None, "n_species": S, "groups": G if with_group else 1}


def one_key(n=64, S=5, G=2):
    """Every row on one entry: 64 equal lanes, the combining path's extreme."""
    return {"labels": np.full(n, 3, np.int64), "preds": np.full(n, 1, np.int64), "group": np.full(n, 1, np.int32), "mask": None,
            "n_species": S, "groups": G}


def distinct_keys(n=64, S=67):
    """Every row on an entry of its own: nothing to combine, everything goes out singly after the rounds."""
    i = np.arange(n, dtype=np.int64)
    return {"labels": i % S, "preds": (i * 7 + 3) % S, "group": None, "mask": None, "n_species": S, "groups": 1}


COUNT_CASES = {
    "n1": lambda: rows(1, 67, 3, 1), "n63": lambda: rows(63, 67, 3, 2), "n64": lambda: rows(64, 67, 3, 3),
    "n65": lambda: rows(65, 67, 3, 4), "n257": lambda: rows(257, 67, 3, 5, hot=0.5),
    "one_key": one_key, "one_key_257": lambda: one_key(257), "distinct": distinct_keys,
    "s1": lambda: rows(65, 1, 1, 6, with_group=False), "s2": lambda: rows(257, 2, 3, 7, group_dtype=np.int32),
    "s67_g1": lambda: rows(300, 67, 1, 8), "s200_g3": lambda: rows(1000, 200, 3, 9, hot=0.7),
    "s200_no_group": lambda: rows(1000, 200, 1, 10, with_group=False, hot=0.9),
    "bad_rows": lambda: rows(257, 5, 3, 11, bad=True), "bad_rows_i32": lambda: rows(257, 5, 3, 12, group_dtype=np.int32, bad=True),
    "mask": lambda: rows(300, 9, 2, 13, with_mask=True, bad=True, hot=0.5),
    "many_blocks": lambda: rows(700000, 40, 7, 14, hot=0.8, bad=True),          # past 2048 workgroups: the grid-stride loop
}


# ---- tables for the report -----------------------------------------------------------------------------------------------
def table(S, G, seed, fill=0.2, top=50):
    """A confusion table [G][S][S]: a share `fill` of the entries non-zero, a heavy diagonal."""
    rs = np.random.RandomState(seed)
    conf = rs.randint(1, top, (G, S, S)) * (rs.rand(G, S, S) < fill)
    idx = np.arange(S)
    conf[:, idx, idx] += rs.randint(0, 20 * top, (G, S))
    return conf.astype(np.int64)


def random_sites(S, sites, seed, per=3):
    rs = np.random.RandomState(seed)
    m = np.zeros((S, (sites + 63) // 64), np.uint64)
    for s in range(S):
        for b in rs.randint(0, sites, rs.randint(1, per + 1)):
            m[s, b // 64] |= np.uint64(1) << np.uint64(b % 64)
    return m


def random_genus(S, seed):
    return np.random.RandomState(seed).randint(0, max(2, S // 4), S).astype(np.int32)


def sized(S):
    G = 1 if S == 1020 else 3
    return {"conf": table(S, G, 100 + S, fill=0.05 if S > 300 else 0.3), "site_masks": random_sites(S, 23, S), "genus": random_genus(S, S + 1)}


def last_bit(sites):
    """sites = 64: W = 1 and bit 63 decides; sites = 65: W = 2 and bit 64 decides.  Species 0 and 1 share only the last
    site, 2 shares only site 0 with 3, nobody else shares anything; every pair among 0..4 has errors."""
    S = 6
    m = np.zeros((S, (sites + 63) // 64), np.uint64)

    def put(s, b):
        m[s, b // 64] |= np.uint64(1) << np.uint64(b % 64)
    put(0, sites - 1); put(0, 5); put(1, sites - 1); put(1, 9); put(2, 0); put(3, 0); put(3, 62); put(4, 61)
    conf = table(S, 2, sites, fill=1.0)
    return {"conf": conf, "site_masks": m, "genus": None}


def special():
    """Group 0 empty, group 1 without an error, group 2 ordinary; species 4 never a label, species 6 never seen at all."""
    S = 9
    conf = table(S, 3, 77, fill=0.5)
    conf[0] = 0
    conf[1] *= np.eye(S, dtype=np.int64)
    conf[:, 4, :] = 0
    conf[:, 6, :] = 0
    conf[:, :, 6] = 0
    return {"conf": conf, "site_masks": random_sites(S, 5, 3), "genus": random_genus(S, 4)}


def absent():
    return {"conf": table(65, 2, 88), "site_masks": None, "genus": None}


REPORT_CASES = {
    "s1": lambda: sized(1), "s2": lambda: sized(2), "s65": lambda: sized(65), "s200": lambda: sized(200),
    "s257": lambda: sized(257), "s1020": lambda: sized(1020), "w1_bit63": lambda: last_bit(64), "w2_bit64": lambda: last_bit(65),
    "special": special, "absent": absent,
    "sites_only": lambda: dict(sized(65), genus=None), "genus_only": lambda: dict(sized(65), site_masks=None),
    "w4": lambda: {"conf": table(30, 2, 5), "site_masks": random_sites(30, 256, 6, per=2), "genus": random_genus(30, 7)},
}


# ---- ids for first_per_individual ---------------------------------------------------------------------------------------
def ids_case(name):
    rs = np.random.RandomState(31)
    if name == "n1":
        return np.array([0], np.int64), 1
    if name == "boundaries":          # repeats across wave (64) and workgroup (256) boundaries, and far apart
        ids = np.arange(600, dtype=np.int64) % 97
        ids[63], ids[64], ids[255], ids[256], ids[599] = 500, 500, 501, 501, 500
        return ids, 502
    if name == "out_of_range":
        ids = rs.randint(0, 40, 300).astype(np.int64)
        ids[::17] = 40
        ids[5::23] = -1
        return ids, 40
    if name == "int32":
        return rs.randint(0, 1000, 5000).astype(np.int32), 1000
    raise KeyError(name)


IDS_CASES = ("n1", "boundaries", "out_of_range", "int32")


# ---- logits for novel_scores -----------------------------------------------------------------------------------------------
def logits(C, n=37, seed=0):
    """float32 [n][C]: random rows, row 1 all NaN, row 2 one NaN (C > 1), row 3 with its maximum at two classes (C > 2: the
    lower one wins), row 4 all equal."""
    rs = np.random.RandomState(seed + C)
    z = (rs.randn(n, C) * 3).astype(np.float32)
    z[1] = np.nan
    if C > 1:
        z[2, C // 2] = np.nan
    if C > 2:
        z[3, C - 1] = z[3, C // 3] = np.float32(z[3].max() + 1.5)
    z[4] = np.float32(0.25)
    return z


NOVEL_CLASSES = (1, 2, 64, 65, 200, 257)
