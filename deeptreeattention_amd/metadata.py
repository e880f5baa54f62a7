"""Site-metadata late fusion around the HIP-backed Hang2020 (drop-in for the model classes of the reference's
`src/models/metadata.py`; parameter names and shapes are the reference's, so state_dicts interoperate).

Only the sensor branch carries real work (>99.9 % of the FLOPs) and it is the HIP path.  The site branch - a 16-wide
embedding, BatchNorm1d, Dropout(0.7) and one Linear - and the 2*classes -> classes fusion layer are <0.2 MFLOP per
sample.  At MODULE level (this file: `model(images, site)` under autograd) they are stock torch modules
that hold the parameters under the reference's names; inside the fused step -- `engine.MetadataTrainer`, the reference's
MetadataModel.training_step (metadata.py:52-63: unweighted cross-entropy of `model(images, site)`) -- the same layers
run natively by default (`native_head=True`: csrc/meta.hip, dta_meta_head_forward / _loss / _backward, 9 launches, checked
against these torch modules' autograd and the reference's golden), and `native_head=False` keeps the torch graph.  The
reference's MetadataModel LightningModule shell itself is out of scope."""
import torch
from torch import nn

from .Hang2020 import Hang2020

_SITE_WIDTH = 16          # reference metadata.py:12
_SITE_DROPOUT = 0.7       # reference metadata.py:15


class metadata(nn.Module):
    """Site index -> (B, classes) scores: embedding -> BN -> dropout -> linear -> ReLU (reference metadata.py:9-24)."""

    def __init__(self, sites, classes):
        super().__init__()
        self.embedding = nn.Embedding(sites, _SITE_WIDTH)
        self.batch_norm = nn.BatchNorm1d(_SITE_WIDTH)
        self.mlp = nn.Linear(_SITE_WIDTH, classes)
        self.dropout = nn.Dropout(_SITE_DROPOUT)

    def forward(self, x):
        # embedding(x) written as one_hot(x) @ weight: the same values (one weight row plus zeros), but the backward is a
        # small deterministic GEMM instead of torch's dense embedding backward (49 us per 1024 x 16 step on MI355X, and
        # float atomics): the metadata train step is run-to-run reproducible like the rest
        onehot = nn.functional.one_hot(x, self.embedding.num_embeddings).to(self.embedding.weight.dtype)
        return torch.relu(self.mlp(self.dropout(self.batch_norm(onehot @ self.embedding.weight))))


class metadata_sensor_fusion(nn.Module):
    """ReLU(Linear(cat[site scores, Hang2020 scores])) (reference metadata.py:26-44)."""

    def __init__(self, bands, sites, classes, precision=None):
        super().__init__()
        self.metadata_model = metadata(sites, classes)
        self.sensor_model = Hang2020(bands, classes, precision)      # the HIP path
        self.fc1 = nn.Linear(2 * classes, classes)

    def forward(self, images, metadata):
        joined = torch.cat((self.metadata_model(metadata), self.sensor_model(images)), dim=1)
        return torch.relu(self.fc1(joined))


# ---------------------------------------------------------------------------------------------------------------------
# Prediction: the written-down meaning of csrc/meta.hip's k_meta_site_table / k_meta_fuse_top2 (engine.MetadataPredictor,
# dense.predict_windows_metadata).  NumPy, float64; for the tests and for readers -- no product path calls them.
# ---------------------------------------------------------------------------------------------------------------------
def site_table_np(params, eps=1e-5):
    """In eval mode (running statistics, no dropout) the site branch depends on the site alone, so the first `classes`
    columns of fc1 contribute one bias row per site:
        T[s][c] = fc1.bias[c] + sum_j fc1.weight[c][j] * ReLU(mlp.bias[j] + sum_f mlp.weight[j][f] * bn(E[s][f]))
    params: a mapping with the model's state_dict names (metadata_model.embedding.weight, metadata_model.batch_norm.weight /
    .bias / .running_mean / .running_var, metadata_model.mlp.weight / .bias, fc1.weight / .bias) as arrays.
    Returns T [sites][classes] float64."""
    import numpy as np
    g = lambda k: np.asarray(params[k], dtype=np.float64)
    emb = g("metadata_model.embedding.weight")
    bn = "metadata_model.batch_norm."
    x = (emb - g(bn + "running_mean")) / np.sqrt(g(bn + "running_var") + float(eps)) * g(bn + "weight") + g(bn + "bias")
    h = np.maximum(x @ g("metadata_model.mlp.weight").T + g("metadata_model.mlp.bias"), 0.0)       # [sites][classes]
    fc_w, fc_b = g("fc1.weight"), g("fc1.bias")
    classes = fc_w.shape[0]
    return h @ fc_w[:, :classes].T + fc_b


def fuse_predict_np(table, fc_w, site, hsi_scores):
    """out[b][c] = ReLU(T[site_b][c] + sum_k fc1.weight[c][classes + k] * hsi[b][k]), its softmax over the classes
    (max-subtracted) and the top-2 of the probabilities: value descending, ties to the lower class (dta_softmax_top2's
    rule -- the ReLU makes about half of the fused scores exactly 0, so ties are the common case).
    site: one int for every row, or an integer array [B].  A row whose site is outside [0, sites) gets labels -1, scores 0
    and zero out / probs rows (dense.crown_reduce_np's empty-crown convention).
    Returns (out [B][classes] float64, probs [B][classes] float64, top_idx [B][2] int64, top_score [B][2] float64)."""
    import numpy as np
    table = np.asarray(table, dtype=np.float64)
    hsi = np.asarray(hsi_scores, dtype=np.float64)
    B, classes = hsi.shape
    sites = table.shape[0]
    wh = np.asarray(fc_w, dtype=np.float64)[:, classes:2 * classes]
    site = np.broadcast_to(np.asarray(site, dtype=np.int64).reshape(-1), (B,))
    out = np.zeros((B, classes))
    probs = np.zeros((B, classes))
    top_idx = np.full((B, 2), -1, dtype=np.int64)
    top_score = np.zeros((B, 2))
    for b in range(B):
        s = int(site[b])
        if s < 0 or s >= sites:
            continue
        z = np.maximum(table[s] + wh @ hsi[b], 0.0)
        e = np.exp(z - z.max())
        p = e / e.sum()
        order = np.argsort(-p, kind="stable")[:2]
        out[b], probs[b] = z, p
        top_idx[b, :len(order)] = order
        top_score[b, :len(order)] = p[order]
    return out, probs, top_idx, top_score
