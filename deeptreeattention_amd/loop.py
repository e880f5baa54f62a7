"""Minimal Trainer-shaped loop around the fused step drivers (BASELINE.json configs[0] plumbing).

The reference trains through PyTorch-Lightning: `TreeModel.training_step / validation_step` (src/main.py:71-94) driven by
`Trainer.fit`, an Adam optimizer and `ReduceLROnPlateau(mode="min", factor=0.75, patience=8, threshold=1e-4 rel,
min_lr=1e-7, eps=1e-8)` monitoring `val_loss` (src/main.py:135-149; per level in src/models/multi_stage.py:258-275).
Lightning itself is out of scope; what a user of the hot path needs from it is small and lives here:

  * `PlateauScheduler`      - the same plateau rule, driving the `lr` of a fused trainer (which is not a
                              torch.optim.Optimizer, so torch's scheduler cannot attach to it);
  * `SyntheticTreeDataset`  - the batch structure of the reference's TreeDataset (src/data.py:284-310:
                              `(individual, {"HSI": ...}, label)`), synthetic, resident on the device;
  * `fit`                   - epochs of `training_step` / `validation_step` + the scheduler, as Trainer.fit runs them;
  * `fit_multistage`        - the same for the reference's MultiStage module (train.py:75-100): every level of a batch in one
                              launch chain, per-level validation loaders and plateau schedulers.
  * `validate` / `validate_multistage` - the validation half of an epoch as one function, with the metric collection the
                              reference logs there (main.py:53-61, :96-133; multi_stage.py:20-28, :323-366) counted on the device;
  * `predict_multistage`    - the prediction loop of src/predict.py:140-151 for a MultiStage module, ending in ONE species label
                              per crop (multi_stage.py:368-434) and, with labels, the confusion matrix of the run.
No arithmetic happens here; every step is the HIP path behind `engine.FusedTrainer` and friends.
"""
import torch


class PlateauScheduler:
    """torch.optim.lr_scheduler.ReduceLROnPlateau with the reference's settings, for objects exposing a float `lr`
    attribute (FusedTrainer, EnsembleTrainer, MetadataTrainer).  `step(metric)` once per validation epoch."""

    def __init__(self, trainer, mode="min", factor=0.75, patience=8, threshold=1e-4, threshold_mode="rel", cooldown=0,
                 min_lr=1e-7, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ("min", "max") or threshold_mode not in ("rel", "abs"):
            raise ValueError("unknown mode")
        self.trainer = trainer
        self.mode, self.factor, self.patience = mode, float(factor), int(patience)
        self.threshold, self.threshold_mode = float(threshold), threshold_mode
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.best = float("inf") if mode == "min" else -float("inf")
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def _is_better(self, a):
        if self.mode == "min":
            ref = self.best * (1.0 - self.threshold) if self.threshold_mode == "rel" else self.best - self.threshold
            return a < ref
        ref = self.best * (1.0 + self.threshold) if self.threshold_mode == "rel" else self.best + self.threshold
        return a > ref

    def step(self, metric):
        current = float(metric)          # a 0-d device tensor is read here: one host sync per EPOCH, as in Lightning
        self.last_epoch += 1
        if self._is_better(current):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = float(self.trainer.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.trainer.lr = new
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return float(self.trainer.lr)


class SyntheticTreeDataset:
    """Synthetic stand-in for the reference's TreeDataset (src/data.py:284-310): item = (individual, inputs, label) with
    `inputs["HSI"]` a (bands, H, W) float32 patch in [0, 1) (real crops are min-max scaled per pixel, src/utils.py:49) or,
    with `years > 0`, a list of per-year patches as TreeDataset yields them for learned_ensemble (`missing` = fraction of
    year crops zero-filled the way TreeDataset fills years without imagery).  Patches are generated once on the device
    from a seeded generator; `loader(batch_size)` yields collated batches the way the default collate would:
    (list of individual ids, {"HSI": (B, bands, H, W) tensor or list of them [, "site": (B,) int64]}, (B,) int64)."""

    def __init__(self, n, bands, classes, size=11, years=0, sites=0, missing=0.0, seed=0, device="cuda"):
        g = torch.Generator(device=device)
        g.manual_seed(int(seed))
        self.n, self.years, self.sites = int(n), int(years), int(sites)
        shape = (self.n, bands, size, size)
        if years:
            self.hsi = [torch.rand(shape, device=device, generator=g) for _ in range(years)]
            if missing > 0:
                # whole batches share the years they have in practice (one flight campaign per site and year); here
                # individuals are dropped independently, which only makes all-zero year BATCHES rarer
                for t in self.hsi[1:]:
                    gone = torch.rand(self.n, device=device, generator=g) < missing
                    t[gone] = 0
        else:
            self.hsi = torch.rand(shape, device=device, generator=g)
        self.labels = torch.randint(0, classes, (self.n,), device=device, generator=g)
        self.site = torch.randint(0, sites, (self.n,), device=device, generator=g) if sites else None
        self.individuals = ["tree_{}".format(i) for i in range(self.n)]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        inputs = {"HSI": [t[i] for t in self.hsi] if self.years else self.hsi[i]}
        if self.site is not None:
            inputs["site"] = self.site[i]
        return self.individuals[i], inputs, self.labels[i]

    def loader(self, batch_size, shuffle=False, seed=0, drop_last=False):
        idx = torch.arange(self.n, device=self.labels.device)
        if shuffle:
            g = torch.Generator(device=self.labels.device)
            g.manual_seed(int(seed))
            idx = torch.randperm(self.n, device=self.labels.device, generator=g)
        for lo in range(0, self.n, batch_size):
            sel = idx[lo:lo + batch_size]
            if drop_last and sel.numel() < batch_size:
                break
            hsi = [t[sel] for t in self.hsi] if self.years else self.hsi[sel]
            inputs = {"HSI": hsi}
            if self.site is not None:
                inputs["site"] = self.site[sel]
            yield [self.individuals[int(i)] for i in sel.tolist()], inputs, self.labels[sel]


def validate(trainer, data, batch_size=64, top_k=1):
    """The validation half of an epoch for a single-model trainer (FusedTrainer / EnsembleTrainer / MetadataTrainer): eval-mode
    `validation_step(batch, i, metrics=True)` on every batch of `data.loader(batch_size)` -- loss, softmax, top-2 and the
    reference's metric collection (main.py:53-61) in one launch behind the forward, accumulated on the device -- then ONE
    device-to-host copy: returns `trainer.validation_epoch_end()`'s dict ({"val_loss" weighted by batch size, "micro",
    "macro", "top_k", "accuracy", "precision", "confusion", "rows"})."""
    model = getattr(trainer, "model", None)
    was_training = bool(model.training) if model is not None else False
    if model is not None:
        model.eval()                 # Lightning's validation loop: running BatchNorm statistics, no updates
    try:
        n = 0
        for i, b in enumerate(data.loader(batch_size)):
            trainer.validation_step(b, i, metrics=True, top_k=top_k)
            n += 1
    finally:
        if model is not None and was_training:
            model.train()
    if n == 0:
        raise ValueError("validate: the dataset yields no batch")
    return trainer.validation_epoch_end()


def validate_multistage(trainer, data, batch_size=128, top_k=1):
    """The validation half of an epoch for an engine.MultiStageTrainer: the levels' own validation loaders
    (multi_stage.py:231-246) zipped WITHOUT cycling -- every validation batch is seen once; a level whose loader ran out
    brings None -- and `validation_step_all` on each list of batches (one launch chain for the levels whose batches agree in
    shape), then ONE device-to-host copy: returns `trainer.validation_epoch_end()`'s list of per-level dicts.  The modules'
    train / eval flags are not touched (the chain always runs eval-mode BatchNorm)."""
    nl = len(trainer.levels)
    if len(data) != nl:
        raise ValueError("one dataset per level ({})".format(nl))
    its = [iter(d.loader(batch_size)) for d in data]
    i = 0
    while True:
        batches = [next(it, None) for it in its]
        if all(b is None for b in batches):
            break
        trainer.validation_step_all(batches, i, None, top_k)
        i += 1
    if i == 0:
        raise ValueError("validate_multistage: the datasets yield no batch")
    return trainer.validation_epoch_end()


def fit(trainer, train_data, val_data=None, epochs=1, batch_size=64, scheduler=None, shuffle=True, log=None, metrics=False):
    """Epoch loop as Lightning's Trainer.fit runs the reference's LightningModules: `training_step(batch, i)` on every
    training batch, then `validation_step(batch, i)` on every validation batch, `val_loss` = mean of the batch losses
    (what `self.log("val_loss", loss)` aggregates, src/main.py:90), then the plateau scheduler.  `trainer` is a
    FusedTrainer / MetadataTrainer (or anything with the two step methods).  Losses stay on the device inside an epoch
    (one host read per epoch).  Returns a list of {"epoch", "train_loss", "val_loss", "lr"} records.
    metrics=True: the validation half is `validate` -- `val_loss` is then weighted by batch size (a short last batch counts
    for its rows, as in Lightning), the scheduler monitors that, and the record gains "val_metrics"."""
    history = []
    for epoch in range(int(epochs)):
        tl = [trainer.training_step(b, i) for i, b in enumerate(train_data.loader(batch_size, shuffle, seed=epoch))]
        rec = {"epoch": epoch, "train_loss": float(torch.stack([t.reshape(()) for t in tl]).mean()), "val_loss": None}
        if val_data is not None and metrics:
            rec["val_metrics"] = validate(trainer, val_data, batch_size)
            rec["val_loss"] = rec["val_metrics"]["val_loss"]
            if scheduler is not None:
                scheduler.step(rec["val_loss"])
        elif val_data is not None:
            model = getattr(trainer, "model", None)
            was_training = bool(model.training) if model is not None else False
            if model is not None:
                model.eval()                 # Lightning's validation loop: running BatchNorm statistics, no updates
            try:
                vl = [trainer.validation_step(b, i) for i, b in enumerate(val_data.loader(batch_size))]
            finally:
                if model is not None and was_training:
                    model.train()
            rec["val_loss"] = float(torch.stack([t.reshape(()).float() for t in vl]).mean())
            if scheduler is not None:
                scheduler.step(rec["val_loss"])
        rec["lr"] = float(trainer.lr)
        history.append(rec)
        if log:
            log(rec)
    return history


def fit_multistage(trainer, train_data, val_data=None, epochs=1, batch_size=128, schedulers=None, shuffle=True, log=None,
                   metrics=False):
    """The epoch loop `train.py:75-100` runs for the reference's MultiStage module: `train_dataloader()` returns one loader
    per level (multi_stage.py:212-229), Lightning zips them into a list-of-batches and calls `training_step` once per
    optimizer -- here ALL levels of a batch are one launch chain (`MultiStageTrainer.training_step_all`; a level whose
    loader ran out is cycled, as Lightning's "max_size_cycle" mode does) --, then `validation_step(batch, i, level)` over every
    level's own validation loader (multi_stage.py:231-246, :290-304), `val_loss/dataloader_idx_{level}` = mean of its batch
    losses, and one plateau scheduler per level monitoring it (multi_stage.py:258-275).
    trainer: engine.MultiStageTrainer; train_data / val_data: one SyntheticTreeDataset(years=...) (or anything with
    `.loader(batch_size, shuffle, seed)`) per level, or a treedata.LevelViews -- the levels as views of one resident crop
    pool: an epoch is then `train_data.batches(...)`, one gather launch per step, whose year flags go to
    `training_step_all(year_flags=)` so that no batch is read back; schedulers: one PlateauScheduler per level (on `trainer.levels[l]`) or
    None.  Returns a list of {"epoch", "train_loss": [...], "val_loss": [...], "lr": [...]} records.
    metrics=True: the validation half is `validate_multistage` (all levels of a validation batch in one launch chain);
    `val_loss` is then weighted by batch size, the schedulers monitor that, and the record gains "val_metrics" (per level)."""
    import itertools
    nl = len(trainer.levels)
    if len(train_data) != nl or (val_data is not None and len(val_data) != nl):
        raise ValueError("one dataset per level ({})".format(nl))
    history = []
    from .treedata import LevelViews
    for epoch in range(int(epochs)):
        sums = [[] for _ in range(nl)]
        if isinstance(train_data, LevelViews):
            # views of one resident pool: every level x year batch of a step is one launch, which also sets the year flags
            # (the same batches, in the same order, as the views' own loaders give below)
            for i, (batch, flags) in enumerate(train_data.batches(batch_size, shuffle, seed=epoch)):
                for l, loss in enumerate(trainer.training_step_all(batch, i, year_flags=flags)):
                    sums[l].append(loss.reshape(()))
        else:
            loaders = [list(d.loader(batch_size, shuffle, seed=epoch)) for d in train_data]
            steps = max(len(b) for b in loaders)
            for i in range(steps):
                batch = [b[i % len(b)] for b in loaders]               # shorter loaders cycle ("max_size_cycle")
                for l, loss in enumerate(trainer.training_step_all(batch, i)):
                    sums[l].append(loss.reshape(()))
        rec = {"epoch": epoch, "train_loss": [float(torch.stack(s).mean()) for s in sums], "val_loss": None}
        if val_data is not None and metrics:
            rec["val_metrics"] = validate_multistage(trainer, val_data, batch_size)
            rec["val_loss"] = [m["val_loss"] for m in rec["val_metrics"]]
            if schedulers is not None:
                for l, sch in enumerate(schedulers):
                    if sch is not None:
                        sch.step(rec["val_loss"][l])
        elif val_data is not None:
            models = [t.model for t in trainer.levels]
            was = [bool(m.training) for m in models]
            for m in models:
                m.eval()                     # Lightning's validation loop: running BatchNorm statistics, no updates
            try:
                vl = []
                for l, d in enumerate(val_data):
                    out = [trainer.validation_step(b, i, l)["val_loss"].reshape(()).float() for i, b in enumerate(d.loader(batch_size))]
                    vl.append(float(torch.stack(out).mean()))
            finally:
                for m, w in zip(models, was):
                    if w:
                        m.train()
            rec["val_loss"] = vl
            if schedulers is not None:
                for l, sch in enumerate(schedulers):
                    if sch is not None:
                        sch.step(vl[l])
        rec["lr"] = [float(t.lr) for t in trainer.levels]
        history.append(rec)
        if log:
            log(rec)
    return history


def predict_multistage(trainer, data, batch_size=64, labels=False):
    """The `predict_species` loop of the reference (src/predict.py:140-151: `trainer.predict(m, dataloaders=...)`, then
    `gather_predictions` and `ensemble`, multi_stage.py:368-434) for an engine.MultiStageTrainer with a hierarchy: batches
    of `data` (a SyntheticTreeDataset(years=...) or anything with `.loader(batch_size)`) through `predict_ensemble`, results
    kept on the device, ONE device-to-host copy at the end.  labels=True: the batches' labels are species labels, and the
    run's confusion matrix (rows = label, columns = prediction; `hierarchy.scores_from_confusion` turns it into
    evaluation_scores' figures) is counted on the device along the way.
    Returns a dict of NumPy arrays: individual, ens_label (int64), ens_score (float32), ens_level (int32) -- one row per
    crop, in the loader's order -- and confusion (int64) when labels are given."""
    import numpy as np
    if labels:
        had = trainer.confusion
        trainer.confusion = None         # this run's own count
    names, parts = [], []
    try:
        for i, batch in enumerate(data.loader(batch_size)):
            out = trainer.predict_ensemble(batch, i, None, batch[2] if labels else None)
            names += list(out[0])
            parts.append(out[1:])
        conf = trainer.confusion if labels else None
    finally:
        if labels:
            trainer.confusion = had
    if not parts:
        raise ValueError("predict_multistage: the dataset yields no batch")
    lab, sc, lev = (torch.cat([p[k] for p in parts]) for k in range(3))
    res = {"individual": np.array(names), "ens_label": lab.cpu().numpy(), "ens_score": sc.cpu().numpy(),
           "ens_level": lev.cpu().numpy()}
    if labels:
        res["confusion"] = conf.cpu().numpy()
    return res
