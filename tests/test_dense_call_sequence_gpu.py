"""The C-ABI call sequence of every dense prediction route (deeptreeattention_amd.dense), entry by entry and in order: what
"nothing inside the loop waits for the device", "ONE gather launch for all years" and "no clearing launch" mean in calls.
Each route runs N = 10 items in batches of 4 -- two full batches and a short last one, for which the predictors prepare
again -- behind a proxy that writes down the name of every dta_* entry it is asked to call.  The expected lists are
literals, recorded on the code before the routes' loops were folded into one walk; they are not derived from the code under
test.  Also: every window route refuses a non-positive batch size and bad crown offsets before it reaches the library."""
import numpy as np
import pytest
import torch

from test_dense_crops_gpu import _ensemble, route_boxes
from test_dense_gpu import ORACLE_SEED, make, oracle_case
from test_dense_multistage_cpu import three_level_hierarchy
from test_dense_multistage_gpu import BANDS, year_rasters
from test_metadata_predict_gpu import small_model
from test_multistage_ensemble_gpu import _small_levels

pytestmark = pytest.mark.gpu

N, BATCH = 10, 4
OFFSETS = [0, 4, 4, 10]      # three crowns, the second one empty


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Recording:
    """The ctypes library; every dta_* entry called through it is appended to `calls`, in order."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("dta_"):
            return f

        def recorded(*a):
            self.calls.append(name)
            return f(*a)
        return recorded


def origins_of(h, w):
    """Ten windows, centre-anchored on the raster's diagonal: the first and last hang over its corners."""
    rows = np.linspace(0, h - 1, N).round().astype(np.int32)
    cols = np.linspace(0, w - 1, N).round().astype(np.int32)
    return np.stack([rows - 5, cols - 5], axis=1).astype(np.int32)


def single_case(precision, **kw):
    from deeptreeattention_amd.dense import DenseRaster, predict_windows
    raw, _, _, _, _, classes = oracle_case(False)
    model, _ = make("hang", 20, classes, ORACLE_SEED, precision)
    ras = DenseRaster(raw, precision=precision, device=dev())
    origins = origins_of(*raw.shape[1:])
    return model, lambda: predict_windows(model, ras, origins, batch_size=BATCH, **kw)


def crops_ensemble_case():
    from deeptreeattention_amd.dense import DenseRaster, predict_crops
    ens = _ensemble()
    raws = year_rasters()
    ras = [DenseRaster(raws[0], precision="fp32", device=dev()), None, DenseRaster(raws[2], precision="fp32", device=dev())]
    return ens, lambda: predict_crops(ens, ras, route_boxes(N), batch_size=BATCH)


def metadata_case(**kw):
    from deeptreeattention_amd.dense import DenseRaster, predict_windows_metadata
    from deeptreeattention_amd.engine import MetadataPredictor
    raw = oracle_case(False)[0]
    m = small_model(20, 7, 4, seed=5, precision="fp32")
    pred = MetadataPredictor(m)
    ras = DenseRaster(raw, precision="fp32", device=dev())
    origins = origins_of(*raw.shape[1:])
    return m, lambda: predict_windows_metadata(pred, ras, 2, origins, batch_size=BATCH, **kw)


def multistage_case(crops=False, **kw):
    from deeptreeattention_amd.dense import DenseRaster, predict_crops_multistage, predict_windows_multistage
    from deeptreeattention_amd.engine import MultiStagePredictor
    h = three_level_hierarchy()
    models = _small_levels(h.classes, 3, bands=BANDS, prec="fp32")
    pred = MultiStagePredictor(models, hierarchy=h)
    raws = year_rasters()      # year 1 missing
    ras = [None if r is None else DenseRaster(r, precision="fp32", device=dev()) for r in raws]
    if crops:
        return models, lambda: predict_crops_multistage(pred, ras, route_boxes(N), batch_size=BATCH)
    origins = origins_of(*raws[0].shape[1:])
    return models, lambda: predict_windows_multistage(pred, ras, origins, batch_size=BATCH, **kw)


CASES = {
    "windows_fp32_crowns": lambda: single_case("fp32", crown_offsets=OFFSETS),
    "windows_bf16_tiles": lambda: single_case("bf16"),
    "windows_share_conv1": lambda: single_case("fp32", share_conv1=True),
    "crops_year_ensemble": crops_ensemble_case,
    "windows_metadata_crowns": lambda: metadata_case(crown_offsets=OFFSETS),
    "windows_multistage_crowns": lambda: multistage_case(crown_offsets=OFFSETS),
    "windows_multistage_share_conv1": lambda: multistage_case(share_conv1=True),
    "crops_multistage": lambda: multistage_case(crops=True),
}

# One line per batch (4, 4 and 2 items); a *_workspace_bytes query wherever a batch shape is first seen.
EXPECTED = {
    "windows_fp32_crowns": [
        "dta_gather_windows", "dta_net_workspace_bytes", "dta_net_forward", "dta_softmax_top2",
        "dta_gather_windows", "dta_net_forward", "dta_softmax_top2",
        "dta_gather_windows", "dta_net_workspace_bytes", "dta_net_forward", "dta_softmax_top2",
        "dta_crown_reduce"],
    "windows_bf16_tiles": [
        "dta_gather_windows_tiles", "dta_net_workspace_bytes", "dta_net_forward_tiles", "dta_softmax_top2",
        "dta_gather_windows_tiles", "dta_net_forward_tiles", "dta_softmax_top2",
        "dta_gather_windows_tiles", "dta_net_workspace_bytes", "dta_net_forward_tiles", "dta_softmax_top2"],
    "windows_share_conv1": [
        "dta_conv1_table_bytes", "dta_raster_conv1_table",
        "dta_net_workspace_bytes", "dta_conv1_output_range", "dta_gather_conv1_windows", "dta_conv1_forward", "dta_softmax_top2",
        "dta_conv1_output_range", "dta_gather_conv1_windows", "dta_conv1_forward", "dta_softmax_top2",
        "dta_net_workspace_bytes", "dta_conv1_output_range", "dta_gather_conv1_windows", "dta_conv1_forward", "dta_softmax_top2"],
    # a single-network year ensemble gathers year by year (the two present ones) and lets dta_year_flags decide
    "crops_year_ensemble": [
        "dta_gather_crops", "dta_gather_crops", "dta_ensemble_workspace_bytes", "dta_year_flags", "dta_ensemble_forward_gated", "dta_softmax_top2",
        "dta_gather_crops", "dta_gather_crops", "dta_year_flags", "dta_ensemble_forward_gated", "dta_softmax_top2",
        "dta_gather_crops", "dta_gather_crops", "dta_ensemble_workspace_bytes", "dta_year_flags", "dta_ensemble_forward_gated", "dta_softmax_top2"],
    "windows_metadata_crowns": [
        "dta_meta_predict_workspace_bytes", "dta_meta_site_table",
        "dta_gather_windows", "dta_net_workspace_bytes", "dta_net_forward", "dta_meta_predict",
        "dta_gather_windows", "dta_net_forward", "dta_meta_predict",
        "dta_gather_windows", "dta_net_workspace_bytes", "dta_net_forward", "dta_meta_predict",
        "dta_crown_reduce"],
    "windows_multistage_crowns": [
        "dta_gather_windows_years", "dta_multistage_workspace_bytes", "dta_multistage_predict_ensemble",
        "dta_gather_windows_years", "dta_multistage_predict_ensemble",
        "dta_gather_windows_years", "dta_multistage_workspace_bytes", "dta_multistage_predict_ensemble",
        "dta_crown_resolve"],
    # one table launch per year, the missing one included (its table is the biases)
    "windows_multistage_share_conv1": [
        "dta_conv1_multistage_table_bytes", "dta_conv1_multistage_table_bytes",
        "dta_conv1_multistage_raster_table", "dta_conv1_multistage_raster_table", "dta_conv1_multistage_raster_table",
        "dta_multistage_workspace_bytes", "dta_conv1_multistage_gather_windows", "dta_conv1_multistage_predict_ensemble",
        "dta_conv1_multistage_gather_windows", "dta_conv1_multistage_predict_ensemble",
        "dta_multistage_workspace_bytes", "dta_conv1_multistage_gather_windows", "dta_conv1_multistage_predict_ensemble"],
    "crops_multistage": [
        "dta_gather_crops_years", "dta_multistage_workspace_bytes", "dta_multistage_predict_ensemble",
        "dta_gather_crops_years", "dta_multistage_predict_ensemble",
        "dta_gather_crops_years", "dta_multistage_workspace_bytes", "dta_multistage_predict_ensemble"],
}


@pytest.mark.parametrize("case", list(CASES))
def test_route_makes_the_recorded_calls_in_order(case, monkeypatch):
    from deeptreeattention_amd import _lib
    keep, route = CASES[case]()      # (the predictors hold their models weakly)
    recording = Recording(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", recording)
    route()
    monkeypatch.undo()
    torch.cuda.synchronize()
    print("CALLS", case, recording.calls)
    assert recording.calls == EXPECTED[case]


@pytest.mark.parametrize("bad", [{"batch_size": 0}, {"crown_offsets": [0, 99]}], ids=["batch_size_0", "offsets_past_the_rows"])
@pytest.mark.parametrize("route", ["windows", "metadata", "multistage"])
def test_window_routes_refuse_batch_size_and_offsets_before_any_launch(route, bad, monkeypatch):
    from deeptreeattention_amd import _lib, dense
    from deeptreeattention_amd.engine import MetadataPredictor, MultiStagePredictor, Predictor
    raw = oracle_case(False)[0]
    origins = origins_of(*raw.shape[1:])
    if route == "multistage":
        h = three_level_hierarchy()
        models = _small_levels(h.classes, 3, bands=BANDS, prec="fp32")
        pred = MultiStagePredictor(models, hierarchy=h)
        ras = [None if r is None else dense.DenseRaster(r, precision="fp32", device=dev()) for r in year_rasters()]
        call = lambda: dense.predict_windows_multistage(pred, ras, origins, **bad)      # noqa: E731
    else:
        ras = dense.DenseRaster(raw, precision="fp32", device=dev())
        if route == "metadata":
            models = small_model(20, 7, 4, seed=5, precision="fp32")
            pred = MetadataPredictor(models)
            call = lambda: dense.predict_windows_metadata(pred, ras, 2, origins, **bad)      # noqa: E731
        else:
            models = make("hang", 20, 7, ORACLE_SEED, "fp32")[0]
            pred = Predictor(models)
            call = lambda: dense.predict_windows(pred, ras, origins, **bad)      # noqa: E731
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_launch)
    monkeypatch.setattr(_lib, "current_stream_ptr", no_launch)
    with pytest.raises(ValueError, match="batch_size" if "batch_size" in bad else "crown_offsets"):
        call()
