"""ctypes binding of libdta_hip.so (C ABI declared in include/dta_hip.h).

The HIP library is the product; there is no CPU or PyTorch fallback.  If the library is missing or a call
fails, a RuntimeError is raised with dta_last_error().
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DTA_DEV_LIB=1 (a choice of FILE made here, in Python): load the developer library -- the same sources built with
# -DDTA_DEV_SWITCHES, whose launch plans can be switched through DTA_* environment variables for same-box A/B runs
# (tools/, tests/test_kernel_variants_gpu.py).  The product library reads nothing from the environment.
LIB_PATH = os.path.join(_HERE, "libdta_hip_dev.so" if os.environ.get("DTA_DEV_LIB") == "1" else "libdta_hip.so")

DTA_F32, DTA_BF16 = 0, 1
ABI_VERSION = 2    # DTA_ABI_VERSION
MAX_YEARS = 16   # DTA_MAX_YEARS
FORWARD_ONLY = 8   # DTA_FORWARD_ONLY (heads_mask flag)
REUSE_PACKED = 32  # DTA_REUSE_PACKED (heads_mask flag: frozen-weight inference keeps the re-laid-out weights in the workspace)
XCHG_HANDLE_BYTES = 128   # DTA_XCHG_HANDLE_BYTES
SKIP_BLEND = 16    # DTA_SKIP_BLEND (heads_mask flag): the blend is left to dta_net_loss
NET_HANG2020, NET_SPECTRAL, NET_SPATIAL, NET_VANILLA = 0, 1, 2, 3
SITE_CONV_FWD, SITE_CONV_WGRAD, SITE_CONV_DGRAD, SITE_STAGE_FWD, SITE_STAGE_BWD, SITE_GEMM = 0, 3, 6, 9, 12, 15
_DTYPES = {"fp32": DTA_F32, "f32": DTA_F32, "float32": DTA_F32, "bf16": DTA_BF16, "bfloat16": DTA_BF16}

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_ll_p = C.POINTER(C.c_longlong)


class NetDesc(C.Structure):
    _fields_ = [("batch", C.c_int), ("bands", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("classes", C.c_int), ("kind", C.c_int), ("dtype", C.c_int), ("training", C.c_int),
                ("heads_mask", C.c_int), ("bn_momentum", C.c_float), ("bn_eps", C.c_float)]


class CropDesc(C.Structure):      # mirrors dta_crop_desc
    _fields_ = [(n, C.c_int) for n in ("batch", "bands_raw", "clip", "size", "flip", "layout", "dtype")]


CROP_F32, CROP_I16, CROP_U8 = 0, 1, 2
CROP_CHW, CROP_HWC = 0, 1


class SubnetParams(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 3), ("conv_b", C.c_void_p * 3), ("bn_w", C.c_void_p * 3),
                ("bn_b", C.c_void_p * 3), ("bn_rm", C.c_void_p * 3), ("bn_rv", C.c_void_p * 3),
                ("bn_nbt", C.c_void_p * 3), ("att", (C.c_void_p * 6) * 3), ("fc_w", C.c_void_p * 3),
                ("fc_b", C.c_void_p * 3)]


class SubnetGrads(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 3), ("conv_b", C.c_void_p * 3), ("bn_w", C.c_void_p * 3),
                ("bn_b", C.c_void_p * 3), ("att", (C.c_void_p * 6) * 3), ("fc_w", C.c_void_p * 3),
                ("fc_b", C.c_void_p * 3)]


class ConvModuleDesc(C.Structure):
    _fields_ = [("batch", C.c_int), ("in_channels", C.c_int), ("filters", C.c_int), ("height", C.c_int),
                ("width", C.c_int), ("pool", C.c_int), ("training", C.c_int), ("dtype", C.c_int),
                ("bn_momentum", C.c_float), ("bn_eps", C.c_float)]


class AttentionDesc(C.Structure):
    _fields_ = [("batch", C.c_int), ("filters", C.c_int), ("height", C.c_int), ("width", C.c_int), ("kind", C.c_int)]


class AdamSegment(C.Structure):     # dta_adam_segment
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_size_t),
                ("active", C.c_void_p), ("dev_step", C.c_void_p), ("dev_step_next", C.c_void_p), ("step", C.c_int),
                ("lr", C.c_float)]


class Level(C.Structure):           # dta_level
    _fields_ = [("classes", C.c_int), ("first", C.c_int), ("count", C.c_int), ("labels", C.c_void_p), ("weight", C.c_void_p),
                ("mean_scores", C.c_void_p), ("kept", C.c_void_p), ("loss", C.c_void_p), ("dscore", C.c_void_p),
                ("scratch", C.c_void_p)]


MAX_LEVELS = 8   # DTA_MAX_LEVELS
EVAL_TOP_K_MAX = 8   # DTA_EVAL_TOP_K_MAX


class EvalLevel(C.Structure):       # dta_eval_level
    _fields_ = [("probs", C.c_void_p), ("top_idx", C.c_void_p), ("top_score", C.c_void_p), ("confusion", C.c_void_p),
                ("counts", C.c_void_p), ("loss_acc", C.c_void_p), ("top_k", C.c_int)]


class HierarchyTable(C.Structure):  # dta_hierarchy
    _fields_ = [("levels", C.c_int), ("n_species", C.c_int), ("classes", C.c_int * MAX_LEVELS), ("table", C.c_void_p)]


ADAM_MAX_SEGMENTS = 16   # DTA_ADAM_MAX_SEGMENTS
ABUNDANCE_MAX_SPECIES = 256   # DTA_ABUNDANCE_MAX_SPECIES
ABUNDANCE_SUMMARY_MAX_ITERATIONS = 256   # DTA_ABUNDANCE_SUMMARY_MAX_ITERATIONS
ABUNDANCE_SUMMARY_MAX_QUANTILES = 16   # DTA_ABUNDANCE_SUMMARY_MAX_QUANTILES
CELLS_GEOINDEX, CELLS_CENTRE = 0, 1   # DTA_CELLS_*
CROWN_WAVE_CELLS = 1024   # DTA_CROWN_WAVE_CELLS
ELEM_F32, ELEM_BF16, ELEM_F16 = 0, 1, 2   # DTA_ELEM_*
RGB_CROPS_MAX_GROUPS = 1024   # DTA_RGB_CROPS_MAX_GROUPS
RGB_CROPS_MAX_SIZE = 512   # DTA_RGB_CROPS_MAX_SIZE
DEAD_FLIP_STREAM = 3   # DTA_DEAD_FLIP_STREAM
DEAD_ORDER_LEVEL = 63   # DTA_DEAD_ORDER_LEVEL
DEAD_ACC_WORDS = 7   # DTA_DEAD_ACC_WORDS
DEAD_LOSS_MAX_ROWS = 1 << 24   # DTA_DEAD_LOSS_MAX_ROWS
REFLECTANCE_MAX_BANDS = 1024   # DTA_REFLECTANCE_MAX_BANDS
BOUNDARY_EDGE_CHUNK = 1024   # DTA_BOUNDARY_EDGE_CHUNK
BOUNDARY_MAX_EDGES = 1 << 20   # DTA_BOUNDARY_MAX_EDGES
SPLIT_MAX_SPECIES = 256   # DTA_SPLIT_MAX_SPECIES
SPLIT_MAX_CANDIDATES = 4096   # DTA_SPLIT_MAX_CANDIDATES
STEMS_CHUNK = 1024   # DTA_STEMS_CHUNK
EPOCH_ORDER_MAX_N = 1 << 20   # DTA_EPOCH_ORDER_MAX_N
EPOCH_ORDER_STREAM = 16   # DTA_EPOCH_ORDER_STREAM
EPOCH_ORDER_MAX_LEVEL_ID = 64   # DTA_EPOCH_ORDER_MAX_LEVEL_ID


class PoolLevel(C.Structure):       # dta_pool_level
    _fields_ = [("order", C.c_void_p), ("rows", C.c_void_p), ("labels", C.c_void_p), ("n", C.c_longlong),
                ("start", C.c_longlong), ("count", C.c_int), ("flip", C.c_int), ("out_labels", C.c_void_p),
                ("out_rows", C.c_void_p)]


LEVEL_COUNT = 5   # DTA_LEVEL_COUNT
LEVEL_STREAM = 2   # DTA_LEVEL_STREAM
LEVEL_MAX_SPECIES = 4096   # DTA_LEVEL_MAX_SPECIES
LEVEL_HEAD, LEVEL_CONIFER, LEVEL_OAK, LEVEL_PLAIN = 0, 1, 2, 3   # DTA_LEVEL_HEAD ..


# DTA_FIELD_* flag bits, DTA_FIELD_REASON_BAD_CODE, DTA_MEGAPLOT_*
FIELD_COORDS, FIELD_GROWTH, FIELD_LIVE, FIELD_SHADED, FIELD_SUNNY, FIELD_TAXON_EXCLUDED = 1, 2, 4, 8, 16, 32
FIELD_EVENT_DROPPED, FIELD_MULTIBOLE, FIELD_KNOWN_ERROR, FIELD_PLOT_EXCLUDED, FIELD_SITE_EXCLUDED = 64, 128, 256, 512, 1024
FIELD_REASON_BAD_CODE = 255
MEGAPLOT_GRID, MEGAPLOT_BUFFER = 0, 1
MEGAPLOT_BUFFER_MAX = 65536   # DTA_MEGAPLOT_BUFFER_MAX
MEGAPLOT_CHUNK = 1024   # DTA_MEGAPLOT_CHUNK
# DTA_MOSAIC_* status codes and constants
MOSAIC_DROPPED, MOSAIC_KEPT, MOSAIC_MASKED, MOSAIC_REFUSED, MOSAIC_UNDECIDED = 0, 1, 2, 3, 4
MOSAIC_CHUNK = 1024   # DTA_MOSAIC_CHUNK
MOSAIC_ROUNDS = 12  # DTA_MOSAIC_ROUNDS
MOSAIC_MAX_ROUNDS = 64   # DTA_MOSAIC_MAX_ROUNDS


class MosaicOptions(C.Structure):   # dta_mosaic_options
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("n_windows", C.c_int), ("max_side", C.c_float),
                ("iou_threshold", C.c_float), ("rounds", C.c_int), ("no_tail", C.c_int)]


class LevelTables(C.Structure):     # dta_level_tables
    _fields_ = [("individuals", C.c_longlong), ("records", C.c_longlong), ("species", C.c_int), ("years", C.c_int)] + \
               [(n, C.c_void_p) for n in ("ind", "year", "sp", "rank", "first", "m", "present", "cls", "lmap", "species_order",
                                          "record_key")]


class LevelConfig(C.Structure):     # dta_level_config
    _fields_ = [("train", C.c_int), ("other_sampling_ceiling", C.c_longlong), ("evergreen_ceiling", C.c_longlong),
                ("oaks_sampling_ceiling", C.c_longlong), ("min_loss_weight", C.c_double), ("seed", C.c_ulonglong),
                ("epoch", C.c_ulonglong)]


class LevelOut(C.Structure):        # dta_level_out
    _fields_ = [("rows", C.c_void_p * LEVEL_COUNT), ("labels", C.c_void_p * LEVEL_COUNT),
                ("year_keep", C.c_void_p * LEVEL_COUNT), ("capacity", C.c_longlong * LEVEL_COUNT), ("n", C.c_void_p),
                ("num_classes", C.c_void_p), ("loss_weight", C.c_void_p)]


class ReflectanceDesc(C.Structure):     # dta_reflectance_desc
    _fields_ = [(n, C.c_int) for n in ("bands_src", "width_src", "rows", "col0", "cols", "dtype", "tiles", "out_height",
                                       "out_row0")]


class HeightRule(C.Structure):      # dta_height_rule
    _fields_ = [("mode", C.c_int), ("min_height", C.c_double), ("min_chm", C.c_double), ("max_diff", C.c_double),
                ("limit", C.c_double)]


class MetaParams(C.Structure):      # dta_meta_params
    _fields_ = [("emb", C.c_void_p), ("bn_w", C.c_void_p), ("bn_b", C.c_void_p), ("bn_rm", C.c_void_p), ("bn_rv", C.c_void_p),
                ("bn_nbt", C.c_void_p), ("mlp_w", C.c_void_p), ("mlp_b", C.c_void_p), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


class MetaGrads(C.Structure):       # dta_meta_grads
    _fields_ = [("emb", C.c_void_p), ("bn_w", C.c_void_p), ("bn_b", C.c_void_p), ("mlp_w", C.c_void_p), ("mlp_b", C.c_void_p),
                ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


PtrArray6 = C.c_void_p * 6
ScoreTable = (C.c_void_p * 3) * 2

_lib = None


def lib():
    """Load the shared library once; fail loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m deeptreeattention_amd.build` "
                "(hipcc, gfx950).  deeptreeattention_amd has no CPU/PyTorch fallback.")
        L = C.CDLL(LIB_PATH)
        L.dta_abi_version.restype = C.c_int
        L.dta_last_error.restype = C.c_char_p
        L.dta_build_id.restype = C.c_char_p
        L.dta_net_workspace_bytes.restype = C.c_size_t
        L.dta_net_workspace_bytes.argtypes = [C.POINTER(NetDesc)]
        L.dta_net_forward.restype = C.c_int
        L.dta_net_forward.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(ScoreTable), C.c_void_p, C.c_void_p]
        L.dta_net_backward.restype = C.c_int
        L.dta_net_backward.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p,
                                       C.POINTER(ScoreTable), C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p,
                                       C.c_int, C.c_void_p]
        L.dta_net_forward_tiles.restype = C.c_int
        L.dta_net_forward_tiles.argtypes = L.dta_net_forward.argtypes
        L.dta_net_backward_tiles.restype = C.c_int
        L.dta_net_backward_tiles.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(ScoreTable), C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p,
                                             C.c_int, C.c_void_p]
        L.dta_net_backward_dp.restype = C.c_int
        L.dta_net_backward_dp.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(ScoreTable), C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p]
        L.dta_adam_step_dp.restype = C.c_int
        L.dta_adam_step_dp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.dta_preprocess_crops_tiles.restype = C.c_int
        L.dta_preprocess_crops_tiles.argtypes = [C.POINTER(CropDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        L.dta_ensemble_workspace_bytes.restype = C.c_size_t
        L.dta_ensemble_workspace_bytes.argtypes = [C.POINTER(NetDesc), C.c_int]
        L.dta_ensemble_forward.restype = C.c_int
        L.dta_ensemble_forward.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams),
                                           C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_ensemble_backward.restype = C.c_int
        L.dta_ensemble_backward.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.c_void_p,
                                            C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p]
        L.dta_preprocess_out_bands.restype = C.c_int
        L.dta_preprocess_out_bands.argtypes = [C.c_int, C.c_int]
        L.dta_preprocess_crops.restype = C.c_int
        L.dta_preprocess_crops.argtypes = [C.POINTER(CropDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.dta_meta_head_workspace_bytes.restype = C.c_size_t
        L.dta_meta_head_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.dta_meta_head_forward.restype = C.c_int
        L.dta_meta_head_forward.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(MetaParams),
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_meta_head_loss.restype = C.c_int
        L.dta_meta_head_loss.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_meta_head_backward.restype = C.c_int
        L.dta_meta_head_backward.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MetaParams), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MetaGrads), C.c_void_p, C.c_void_p]
        L.dta_meta_predict_workspace_bytes.restype = C.c_size_t
        L.dta_meta_predict_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.dta_meta_site_table.restype = C.c_int
        L.dta_meta_site_table.argtypes = [C.c_int, C.c_int, C.c_float, C.POINTER(MetaParams), C.c_void_p, C.c_void_p]
        L.dta_meta_predict.restype = C.c_int
        L.dta_meta_predict.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_net_loss.restype = C.c_int
        L.dta_net_loss.argtypes = [C.POINTER(NetDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_ensemble_forward_loss.restype = C.c_int
        L.dta_ensemble_forward_loss.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.POINTER(C.c_void_p), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        L.dta_adam_step_multi.restype = C.c_int
        L.dta_adam_step_multi.argtypes = [C.c_int, C.POINTER(AdamSegment), C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_int, C.c_void_p]
        L.dta_multistage_workspace_bytes.restype = C.c_size_t
        L.dta_multistage_workspace_bytes.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level)]
        L.dta_multistage_forward_loss.restype = C.c_int
        L.dta_multistage_forward_loss.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams),
                                                  C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_multistage_forward.restype = C.c_int
        L.dta_multistage_forward.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams),
                                             C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_multistage_predict.restype = C.c_int
        L.dta_multistage_predict.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams),
                                             C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
        L.dta_multistage_predict_ensemble.restype = C.c_int
        L.dta_multistage_predict_ensemble.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams),
                                                      C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(HierarchyTable),
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_hierarchy_resolve.restype = C.c_int
        L.dta_hierarchy_resolve.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(HierarchyTable),
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_multistage_validate.restype = C.c_int
        L.dta_multistage_validate.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(EvalLevel),
                                              C.POINTER(SubnetParams), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_eval_metrics.restype = C.c_int
        L.dta_eval_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(EvalLevel), C.c_void_p]
        L.dta_multistage_backward.restype = C.c_int
        L.dta_multistage_backward.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams), C.c_void_p,
                                              C.POINTER(SubnetGrads), C.c_void_p, C.c_void_p]
        L.dta_net_forward_loss.restype = C.c_int
        L.dta_net_forward_loss.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        L.dta_weighted_ce.restype = C.c_int
        L.dta_weighted_ce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_weighted_ce_scaled.restype = C.c_int
        L.dta_weighted_ce_scaled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_weighted_ce_scaled_dev.restype = C.c_int
        L.dta_weighted_ce_scaled_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_year_flags.restype = C.c_int
        L.dta_year_flags.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_ensemble_forward_gated.restype = C.c_int
        L.dta_ensemble_forward_gated.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.POINTER(C.c_void_p),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dta_adam_step.restype = C.c_int
        L.dta_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.c_void_p]
        L.dta_adam_step_zero_grad.restype = C.c_int
        L.dta_adam_step_zero_grad.argtypes = L.dta_adam_step.argtypes
        L.dta_adam_step_gated.restype = C.c_int
        L.dta_adam_step_gated.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                          C.c_void_p]
        L.dta_ensemble_backward_phased.restype = C.c_int
        L.dta_ensemble_backward_phased.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.c_void_p,
                                                   C.c_void_p, C.POINTER(SubnetGrads), C.c_int, C.c_void_p]
        L.dta_ensemble_backward_gated.restype = C.c_int
        L.dta_ensemble_backward_gated.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.c_void_p,
                                                  C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p, C.c_int, C.c_void_p]
        L.dta_ensemble_backward_xchg.restype = C.c_int
        L.dta_ensemble_backward_xchg.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), C.c_void_p,
                                                 C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p, C.c_void_p, C.c_void_p]
        vp = C.c_void_p
        L.dta_conv_module_workspace_bytes.restype = C.c_size_t
        L.dta_conv_module_workspace_bytes.argtypes = [C.POINTER(ConvModuleDesc)]
        L.dta_conv_module_forward.restype = C.c_int
        L.dta_conv_module_forward.argtypes = [C.POINTER(ConvModuleDesc)] + [vp] * 11
        L.dta_conv_module_backward.restype = C.c_int
        L.dta_conv_module_backward.argtypes = [C.POINTER(ConvModuleDesc)] + [vp] * 10
        L.dta_attention_workspace_bytes.restype = C.c_size_t
        L.dta_attention_workspace_bytes.argtypes = [C.POINTER(AttentionDesc)]
        L.dta_attention_forward.restype = C.c_int
        L.dta_attention_forward.argtypes = [C.POINTER(AttentionDesc), C.POINTER(PtrArray6), vp, vp, vp, vp, vp]
        L.dta_attention_backward.restype = C.c_int
        L.dta_attention_backward.argtypes = [C.POINTER(AttentionDesc), C.POINTER(PtrArray6), vp, vp, vp, vp, vp,
                                             C.POINTER(PtrArray6), vp]
        L.dta_linear_forward.restype = C.c_int
        L.dta_linear_forward.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
        L.dta_linear_backward.restype = C.c_int
        L.dta_linear_backward.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.dta_softmax_top2.restype = C.c_int
        L.dta_softmax_top2.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
        L.dta_raster_normalise.restype = C.c_int
        L.dta_raster_normalise.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        L.dta_gather_windows.restype = C.c_int
        L.dta_gather_windows.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]
        L.dta_gather_windows_tiles.restype = C.c_int
        L.dta_gather_windows_tiles.argtypes = L.dta_gather_windows.argtypes
        L.dta_crown_reduce.restype = C.c_int
        L.dta_crown_reduce.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
        L.dta_gather_windows_years.restype = C.c_int
        L.dta_gather_windows_years.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                               C.POINTER(C.c_void_p), vp, vp, vp]
        L.dta_gather_crops.restype = C.c_int
        L.dta_gather_crops.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp]
        L.dta_gather_crops_tiles.restype = C.c_int
        L.dta_gather_crops_tiles.argtypes = L.dta_gather_crops.argtypes
        L.dta_gather_crops_years.restype = C.c_int
        L.dta_gather_crops_years.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_void_p), vp, vp, vp]
        L.dta_crown_resolve.restype = C.c_int
        L.dta_crown_resolve.argtypes = [C.c_int, C.POINTER(C.c_void_p), vp, C.c_int, C.POINTER(HierarchyTable), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp, vp, vp, vp, vp, vp, vp]
        # the first conv once per raster (dense_conv1.hip)
        L.dta_conv1_table_bytes.restype = C.c_int
        L.dta_conv1_table_bytes.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.dta_raster_conv1_table.restype = C.c_int
        L.dta_raster_conv1_table.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), vp, C.c_int, C.c_int, vp, vp, vp]
        L.dta_gather_conv1_windows.restype = C.c_int
        L.dta_gather_conv1_windows.argtypes = [C.POINTER(NetDesc), vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
        L.dta_conv1_output_range.restype = C.c_int
        L.dta_conv1_output_range.argtypes = [C.POINTER(NetDesc), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.dta_conv1_forward.restype = C.c_int
        L.dta_conv1_forward.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p,
                                            C.POINTER(ScoreTable), C.c_void_p, C.c_void_p]
        # ... for the levels x years of a multi-stage model
        L.dta_conv1_multistage_table_bytes.restype = C.c_int
        L.dta_conv1_multistage_table_bytes.argtypes = [C.POINTER(NetDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                                       C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.dta_conv1_multistage_raster_table.restype = C.c_int
        L.dta_conv1_multistage_raster_table.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(SubnetParams), vp, C.c_int, C.c_int,
                                                        vp, vp, vp, vp]
        L.dta_conv1_multistage_output_range.restype = C.c_int
        L.dta_conv1_multistage_output_range.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(C.c_size_t),
                                                        C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.dta_conv1_multistage_gather_windows.restype = C.c_int
        L.dta_conv1_multistage_gather_windows.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.c_int, C.POINTER(C.c_void_p),
                                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, vp, C.c_int,
                                                          vp, vp, vp, vp]
        L.dta_conv1_multistage_predict.restype = C.c_int
        L.dta_conv1_multistage_predict.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams), vp, vp,
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp]
        L.dta_conv1_multistage_predict_ensemble.restype = C.c_int
        L.dta_conv1_multistage_predict_ensemble.argtypes = [C.POINTER(NetDesc), C.c_int, C.POINTER(Level), C.POINTER(SubnetParams),
                                                            vp, vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                            C.POINTER(C.c_void_p), C.POINTER(HierarchyTable), vp, vp, vp, vp, vp, vp]
        # species abundance: counts and confusion resampling (abundance.hip)
        L.dta_abundance_workspace_bytes.restype = C.c_size_t
        L.dta_abundance_workspace_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
        L.dta_abundance_resample.restype = C.c_int
        L.dta_abundance_resample.argtypes = [vp, vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, vp,
                                             vp, C.c_size_t, vp]
        L.dta_abundance_counts.restype = C.c_int
        L.dta_abundance_counts.argtypes = [vp, vp, C.c_longlong, C.c_int, vp, vp, C.c_size_t, vp]
        # abundance per tile and map cell: the cell of a crown, grouped counts and resampling, the summary (abundance_grid.hip)
        L.dta_abundance_cells.restype = C.c_int
        L.dta_abundance_cells.argtypes = [vp, C.c_longlong, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, vp, vp]
        L.dta_abundance_grouped_workspace_bytes.restype = C.c_size_t
        L.dta_abundance_grouped_workspace_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_longlong]
        L.dta_abundance_resample_grouped.restype = C.c_int
        L.dta_abundance_resample_grouped.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_longlong, vp, C.c_int, C.c_int,
                                                     C.c_ulonglong, C.c_ulonglong, vp, vp, C.c_size_t, vp]
        L.dta_abundance_counts_grouped.restype = C.c_int
        L.dta_abundance_counts_grouped.argtypes = [vp, vp, vp, vp, C.c_longlong, C.c_longlong, C.c_int, vp, vp, C.c_size_t, vp]
        L.dta_abundance_summary.restype = C.c_int
        L.dta_abundance_summary.argtypes = [vp, C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, vp, vp, vp]
        # crown height filter: CHM quantile per box and the keep rules (canopy.hip)
        L.dta_crown_height.restype = C.c_int
        L.dta_crown_height.argtypes = [vp, C.c_int, C.c_int, vp, C.c_longlong, C.c_float, C.c_float, vp, C.POINTER(HeightRule),
                                       vp, vp, vp, vp]
        # alive/dead crown filter: RGB crops resized on the device, and the score (dead.hip)
        L.dta_rgb_crops.restype = C.c_int
        L.dta_rgb_crops.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_longlong, C.c_int, C.c_int, c_float_p, c_float_p,
                                    C.c_int, C.c_int, vp, vp, vp]
        L.dta_dead_head.restype = C.c_int
        L.dta_dead_head.argtypes = [vp, C.c_int, C.c_longlong, C.c_longlong, vp, vp, vp]
        # training the alive/dead classifier: a batch of a resident image pool, and the loss with its gradient (dead_train.hip)
        L.dta_image_pool_batch.restype = C.c_int
        L.dta_image_pool_batch.argtypes = [vp, C.c_longlong, vp, C.c_longlong, C.c_int, vp, C.c_int, C.c_longlong, C.c_longlong,
                                           vp, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_int, c_float_p, c_float_p, C.c_int,
                                           C.c_int, vp, vp, vp]
        L.dta_dead_loss.restype = C.c_int
        L.dta_dead_loss.argtypes = [vp, C.c_int, vp, C.c_longlong, vp, vp, vp, vp, vp]
        # reflectance cube -> resident raster: band selection, window, min-max and transpose in one pass (reflectance.hip)
        L.dta_reflectance_normalise.restype = C.c_int
        L.dta_reflectance_normalise.argtypes = [C.POINTER(ReflectanceDesc), vp, vp, C.c_int, vp, vp]
        # site boundary clip: points, crown boxes and raster cells inside a polygon (boundary.hip); org and transform are
        # HOST arrays
        L.dta_boundary_points.restype = C.c_int
        L.dta_boundary_points.argtypes = [vp, C.c_int, c_double_p, vp, C.c_longlong, vp, vp]
        L.dta_boundary_boxes.restype = C.c_int
        L.dta_boundary_boxes.argtypes = [vp, C.c_int, c_double_p, vp, vp, c_double_p, C.c_longlong, vp, vp]
        L.dta_boundary_raster.restype = C.c_int
        L.dta_boundary_raster.argtypes = [vp, C.c_int, c_double_p, C.c_int, C.c_int, c_double_p, vp, vp]
        # train/test plot split search: every iteration in one launch (split.hip); floor is a HOST array
        L.dta_split_search.restype = C.c_int
        L.dta_split_search.argtypes = [vp, vp, C.c_int, C.c_int, c_double_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong,
                                       C.c_ulonglong, vp, vp, vp, vp, vp, vp, vp, vp]
        # field stems to crown boxes: join, nearest box, one stem per box (stems.hip); tables sorted by plot
        L.dta_stems_assign.restype = C.c_int
        L.dta_stems_assign.argtypes = [vp, vp, C.c_longlong, vp, vp, vp, vp, vp, C.c_longlong, C.c_int, C.c_double, vp, vp, vp,
                                       vp]
        # the resident training set: every level's epoch order, and every level x year batch of a step, one launch each
        # (treedata.hip); n, level_ids, orders, lv and outs are HOST arrays
        L.dta_epoch_order.restype = C.c_int
        L.dta_epoch_order.argtypes = [C.c_int, c_ll_p, C.POINTER(C.c_int), C.c_ulonglong, C.c_ulonglong,
                                      C.POINTER(C.c_void_p), vp]
        L.dta_pool_batches.restype = C.c_int
        L.dta_pool_batches.argtypes = [vp, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PoolLevel),
                                       C.POINTER(C.c_void_p), vp, vp, vp]
        L.dta_pool_batches_keep.restype = C.c_int
        L.dta_pool_batches_keep.argtypes = [vp, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PoolLevel),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp, vp, vp]
        # the five level data sets and their loss weights from one resident table (levels.hip)
        L.dta_level_workspace_bytes.restype = C.c_size_t
        L.dta_level_workspace_bytes.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int]
        L.dta_level_build.restype = C.c_int
        L.dta_level_build.argtypes = [C.POINTER(LevelTables), C.POINTER(LevelConfig), C.POINTER(LevelOut), vp, C.c_size_t, vp]
        # field records to canopy points: the NEON row filter and the megaplot plot codes (field.hip)
        L.dta_field_workspace_bytes.restype = C.c_size_t
        L.dta_field_workspace_bytes.argtypes = [C.c_longlong, C.c_longlong]
        L.dta_field_filter.restype = C.c_int
        L.dta_field_filter.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_longlong, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                       vp, C.c_size_t, vp]
        L.dta_megaplot_plots.restype = C.c_int
        L.dta_megaplot_plots.argtypes = [vp, C.c_longlong, C.c_int, C.c_double, vp, C.c_int, vp, C.c_int, vp, vp]
        # crown-level evaluation: the grouped confusion table, its report, first rows per individual, novel scores (evaluate.hip)
        L.dta_eval_count.restype = C.c_int
        L.dta_eval_count.argtypes = [vp, vp, vp, C.c_int, vp, C.c_longlong, C.c_int, C.c_longlong, C.c_int, vp, vp, vp]
        L.dta_eval_report.restype = C.c_int
        L.dta_eval_report.argtypes = [vp, C.c_int, C.c_longlong, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.dta_first_rows.restype = C.c_int
        L.dta_first_rows.argtypes = [vp, C.c_int, C.c_longlong, C.c_longlong, vp, vp, vp]
        L.dta_novel_scores.restype = C.c_int
        L.dta_novel_scores.argtypes = [vp, C.c_longlong, C.c_int, vp, vp, vp, vp]
        # crown boxes from detector windows: shift, exact greedy NMS by cells and rounds, pixel boxes (mosaic.hip)
        L.dta_mosaic_workspace_bytes.restype = C.c_size_t
        L.dta_mosaic_workspace_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_float]
        L.dta_mosaic_grid.restype = C.c_int
        L.dta_mosaic_grid.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]
        L.dta_mosaic.restype = C.c_int
        L.dta_mosaic.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.POINTER(MosaicOptions), vp, vp, vp, vp, vp, C.c_size_t, vp]
        L.dta_profile_enable.restype = C.c_int
        L.dta_profile_enable.argtypes = [C.c_int]
        L.dta_profile_set_stride.restype = C.c_int
        L.dta_profile_set_stride.argtypes = [C.c_int]
        L.dta_profile_collect.restype = C.c_int
        L.dta_profile_collect.argtypes = [C.POINTER(C.c_float), C.c_int]
        L.dta_profile_collect_site.restype = C.c_int
        L.dta_profile_collect_site.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_int]
        L.dta_dev_reload_switches.restype = C.c_int
        L.dta_dev_switches_enabled.restype = C.c_int
        # peer gradient exchange (opaque handle = void*)
        L.dta_xchg_create.restype = C.c_int
        L.dta_xchg_create.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.dta_xchg_grad_buffer.restype = C.c_void_p
        L.dta_xchg_grad_buffer.argtypes = [C.c_void_p]
        L.dta_xchg_grad_capacity.restype = C.c_size_t
        L.dta_xchg_grad_capacity.argtypes = [C.c_void_p]
        L.dta_xchg_export.restype = C.c_int
        L.dta_xchg_export.argtypes = [C.c_void_p, C.c_void_p]
        L.dta_xchg_connect.restype = C.c_int
        L.dta_xchg_connect.argtypes = [C.c_void_p, C.c_void_p]
        L.dta_xchg_set_timeout.restype = None
        L.dta_xchg_set_timeout.argtypes = [C.c_void_p, C.c_double]
        L.dta_xchg_set_max_workgroups.restype = None
        L.dta_xchg_set_max_workgroups.argtypes = [C.c_void_p, C.c_int]
        L.dta_xchg_allreduce.restype = C.c_int
        L.dta_xchg_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.dta_xchg_reduce_head.restype = C.c_int
        L.dta_xchg_reduce_head.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.dta_xchg_adam_step.restype = C.c_int
        L.dta_xchg_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.dta_xchg_set_split.restype = C.c_int
        L.dta_xchg_set_split.argtypes = [C.c_void_p, C.c_size_t]
        L.dta_net_backward_xchg.restype = C.c_int
        L.dta_net_backward_xchg.argtypes = [C.POINTER(NetDesc), C.POINTER(SubnetParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(ScoreTable), C.c_void_p, C.POINTER(SubnetGrads), C.c_void_p, C.c_void_p,
                                            C.c_longlong, C.c_void_p]
        L.dta_xchg_disconnect.restype = C.c_int
        L.dta_xchg_disconnect.argtypes = [C.c_void_p]
        L.dta_xchg_selftest_fill.restype = C.c_int
        L.dta_xchg_selftest_fill.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dta_xchg_selftest_verify.restype = C.c_int
        L.dta_xchg_selftest_verify.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dta_xchg_selftest_mismatches.restype = C.c_int
        L.dta_xchg_selftest_mismatches.argtypes = [C.c_void_p]
        L.dta_xchg_status.restype = C.c_int
        L.dta_xchg_status.argtypes = [C.c_void_p]
        L.dta_xchg_last_timing.restype = C.c_int
        L.dta_xchg_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.dta_xchg_destroy.restype = C.c_int
        L.dta_xchg_destroy.argtypes = [C.c_void_p]
        if L.dta_abi_version() != ABI_VERSION:
            raise RuntimeError("libdta_hip.so ABI version mismatch: the library says {}, this binding is written for {} "
                               "(rebuild: python -m deeptreeattention_amd.build --force)".format(L.dta_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().dta_last_error().decode()}")


def dtype_code(name):
    try:
        return _DTYPES[str(name).lower()]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(_DTYPES)}, got {name!r}")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
