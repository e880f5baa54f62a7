"""deeptreeattention_amd: MI355X-native (gfx950) implementation of DeepTreeAttention's Hang2020 hot path.

The package mirrors the reference's module names for this path only:
    deeptreeattention_amd.Hang2020   <->  src/models/Hang2020.py
    deeptreeattention_amd.year       <->  src/models/year.py        (learned_ensemble)
    deeptreeattention_amd.engine     fused train step (forward + weighted CE + backward + Adam, optional RCCL DDP)
    deeptreeattention_amd.hierarchy  <->  src/models/multi_stage.py:368-485 (the levels' predictions -> one species label)
    deeptreeattention_amd.dense      <->  src/patches.py:50-83 + src/main.py:165-205: per-pixel windows of a resident raster,
                                     gathered and predicted on the device, reduced per crown; with a multi-stage model
                                     one species label per pixel and per crown; and src/patches.py:5-30 +
                                     src/utils.py:59-79: one resized crop per crown box, cut out of that raster
    deeptreeattention_amd.abundance  <->  abundance.py + src/multinomial.py: trees per species over the predicted crowns, and
                                     the confusion resampling of that count (every iteration in one launch)
    deeptreeattention_amd.canopy     <->  src/CHM.py + src/predict.py find_crowns: the 99th-percentile canopy height of every
                                     crown box of a resident CHM raster and the height rules on it (one launch pair)
    deeptreeattention_amd.dead       <->  src/models/dead.py + src/predict.py predict_tile(filter_dead=True): the normalised,
                                     resized RGB crop of every crown box from a resident uint8 raster (one launch), the
                                     alive/dead score of the classifier's logits, and the rule that blanks dead crowns
    deeptreeattention_amd.dead_train <->  train_dead.py + src/models/dead.py AliveDead: the labelled images resident once, a
                                     batch (normalise, resize, flip, labels) in one launch, the sigmoid cross-entropy with
                                     its gradient and confusion counts in one launch, the epoch loop, the precision-recall
                                     curve behind dead_threshold (also reachable as dead.<name>)
    deeptreeattention_amd.reflectance  <->  src/Hyperspectral.py:138-219 generate_raster / calc_clip_index: the band mask, the
                                     clip window and the band-first transpose between a pixel-interleaved reflectance cube
                                     and the resident raster (DenseRaster.from_reflectance: one launch per strip of rows)
    deeptreeattention_amd.boundary   <->  gpd.clip(crowns, boundary) in abundance.py, create_prediction_shp.py and
                                     src/multinomial.py: which crown boxes, points and raster cells lie inside the site's
                                     boundary polygon, from a resident edge table (one launch each)
    deeptreeattention_amd.split      <->  src/data.py sample_plots + train_test_split: the search for the plot-level
                                     train/test split with the most test species, every iteration in one launch
    deeptreeattention_amd.stems      <->  src/generate.py process_plot + create_boxes + choose_box: which crown box a
                                     field-measured stem gets (join, fallback box, nearest centre) and which stem a box
                                     keeps (the tallest), all plots of a site in one chain of three launches
    deeptreeattention_amd.treedata   <->  src/data.py TreeDataset + multi_stage.py create_datasets' five of them: the crops
                                     of a whole data set resident once, a level as rows and labels, a shuffled order per
                                     level and epoch, and every level x year batch of a train step in one launch
    deeptreeattention_amd.levels     <->  src/models/multi_stage.py MultiStage.__init__ + create_datasets: which individuals
                                     each of the five levels trains on and in what order, the level labels, num_classes and
                                     the loss weights, from one resident integer table in a chain of at most four launches
    deeptreeattention_amd.field      <->  src/data.py filter_data + src/megaplot.py format (create_grid, buffer_plots): which rows
                                     of a raw NEON field table survive (per-row rules, the shaded individuals, one record
                                     per individual) in a chain of five launches, and the 40 m plot code of every stem of a
                                     contributed megaplot, by grid or by buffer, in one
    deeptreeattention_amd.evaluate   <->  src/models/multi_stage.py evaluation_scores + src/main.py evaluate_crowns +
                                     src/metrics.py: the experiment report from one grouped confusion table counted on the
                                     device (one launch per batch) and reduced in one launch -- per-site micro / macro,
                                     per-species accuracy / precision, the within-site and within-genus shares of the
                                     errors -- plus the first row per individual and the novel-species scores
    deeptreeattention_amd.mosaic     <->  src/predict.py predict_crowns + src/generate.py predict_trees (DeepForest's predict_tile
                                     around a stock detector): the window layout, the shift of every window's boxes to
                                     tile coordinates, the exact greedy non-maximum suppression over the whole tile (binned
                                     by cells, decided in parallel rounds, no sort) and the pixel boxes every module above
                                     takes
    deeptreeattention_amd.loop       epoch loops: fit / fit_multistage, validate / validate_multistage (validation with the
                                     metric counts taken on the device), predict_multistage
All arithmetic runs in libdta_hip.so (HIP, C ABI in include/dta_hip.h); there is no CPU fallback.
"""
from . import Hang2020  # noqa: F401
from .Hang2020 import set_default_precision, get_default_precision  # noqa: F401
from .hierarchy import Hierarchy, scores_from_confusion  # noqa: F401
from .loop import validate, validate_multistage  # noqa: F401
from .dense import DenseRaster, window_origins, predict_windows, predict_map  # noqa: F401
from .dense import predict_windows_multistage, predict_map_multistage, crown_resolve  # noqa: F401
from .dense import predict_windows_metadata, predict_map_metadata  # noqa: F401
from .dense import crop_boxes, predict_crops, predict_crops_multistage, predict_crops_metadata  # noqa: F401
from .treedata import CropPool, PoolView, LevelViews, epoch_order_np  # noqa: F401
from .dead_train import ImagePool, DeadAccumulator  # noqa: F401

__all__ = ["ImagePool", "DeadAccumulator", "CropPool", "PoolView", "LevelViews", "epoch_order_np","Hang2020", "set_default_precision", "get_default_precision", "Hierarchy", "scores_from_confusion",
           "validate", "validate_multistage", "DenseRaster", "window_origins", "predict_windows", "predict_map",
           "predict_windows_multistage", "predict_map_multistage", "crown_resolve",
           "crop_boxes", "predict_crops", "predict_crops_multistage", "predict_crops_metadata"]
