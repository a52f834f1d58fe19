"""ctypes binding of include/microscopes_hip.h (the C-ABI of the HIP library).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C
common_amd/csrc``) as ``common_amd/lib/libmicroscopes_hip.so``.  There is no
Python / numpy / torch fallback for any of its entry points: if the shared
object is missing or no gfx950 device is usable, calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MSC_LIB_PATH: an experiment build of the same library, common_amd/csrc/Makefile VARIANT=...; the product is the default)
LIB_PATH = os.environ.get("MSC_LIB_PATH") or os.path.join(_HERE, "lib", "libmicroscopes_hip.so")

# families / primitive types / flags, mirrored from the header
BB, GP, DD, NICH, NIW, NOOP, BBNC, BNB, DM = range(9)
(TYPE_B, TYPE_I8, TYPE_U8, TYPE_I16, TYPE_U16, TYPE_I32, TYPE_U32, TYPE_I64, TYPE_U64, TYPE_F32,
 TYPE_F64) = range(11)
SCORE_CRP_PRIOR = 0x1
SCORE_NIW_F32 = 0x2
ACC_RESET, ACC_SUBTRACT, ACC_NO_COMMIT = 0x1, 0x2, 0x4
OP_ADD, OP_REMOVE, OP_SCORE_VALUE, OP_SCORE_DATA = range(4)
ABI_VERSION = 1
HP_CLUSTER = 0xFFFFFFFF          # msc_hp_grid_create's feature index of the CRP concentration
PRED_MASKED_ONLY = 0x1
PRED_GROUP_KEY = 0xD1B54A32D192ED03   # msc_sample_predictive's group draw uses key = seed ^ this
PRIOR_FLAT, PRIOR_EXPONENTIAL, PRIOR_NORMAL, PRIOR_NONINF_BETA = range(4)   # msc_slice_coord.prior
SLICE_KEY = 0x2545F4914F6CDD1D        # msc_hp_slice / msc_theta_slice use key = seed ^ this
SPLIT_MERGE_KEY = 0xA0761D6478BD642F  # msc_split_merge's streams: key = (seed ^ this) + stream * SPLIT_MERGE_STREAM_STRIDE
SPLIT_MERGE_STREAM_STRIDE = 0x9E3779B97F4A7C15
SLICE_STEP_OUT = 64                   # m: the stepping-out limit of a slice update
SLICE_SHRINK = 256                    # rejected proposals before an update keeps its value
ZMATRIX_MAX_ROWS = 1 << 18            # msc_zmatrix_create: m at most
ZMATRIX_MAX_LABELS = 1 << 16          # ... and nlabels at most
ZMATRIX_REFINE_MAX_ROWS = 1 << 15     # msc_zmatrix_partition_refine: m at most
ZMATRIX_REFINE_MAX_CLUSTERS = 1 << 10 # ... and max_clusters at most
LINKAGE_MAX_N = 1 << 16               # msc_linkage_single: n at most
DISTANCES_MAX_ROWS = 1 << 15          # msc_partition_distances: m at most
DISTANCES_MAX_CLUSTERS = 1 << 10      # ... and clusters a partition at most
DISTANCES_LDS_CELLS = 15 * 1024       # ... and the cells K_a x K_b of a pair whose table stays in LDS
REFINE_VI_MAX_ROWS = 1 << 15          # msc_partition_refine_vi: m at most
REFINE_VI_MAX_SAMPLES = 1 << 16       # ... samples at most
REFINE_VI_MAX_CLUSTERS = 1 << 10      # ... and max_clusters, and the clusters of a sample, at most
VI_TABLE_SCALE = 1 << 24              # msc_vi_table: F(n) = rint(n log2 n VI_TABLE_SCALE)


class MicroscopesHipError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "microscopes_hip error %d: %s" % (code, message))
        self.code = code


class RuntimeType(C.Structure):
    _fields_ = [("type", C.c_int32), ("count", C.c_uint32)]


class FeatureSpec(C.Structure):
    _fields_ = [("family", C.c_int32), ("dim", C.c_uint32)]


class SliceCoord(C.Structure):
    """msc_slice_coord"""
    _fields_ = [("feature", C.c_uint32), ("coord", C.c_uint32), ("width", C.c_float), ("prior", C.c_uint32),
                ("prior_a", C.c_float), ("prior_b", C.c_float), ("partner", C.c_uint32)]


_SIGS = {
    "msc_abi_version": (C.c_int, []),
    "msc_last_error": (C.c_char_p, []),
    "msc_build_info": (C.c_char_p, []),
    "msc_last_kernel": (C.c_char_p, [C.c_int]),
    "msc_context_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "msc_context_destroy": (C.c_int, [C.c_void_p]),
    "msc_context_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "msc_context_synchronize": (C.c_int, [C.c_void_p]),
    "msc_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "msc_device_alloc_probed": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "msc_device_alloc_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    "msc_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "msc_pinned_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "msc_pinned_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "msc_device_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "msc_device_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "msc_dataview_from_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.POINTER(RuntimeType), C.c_uint32, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_void_p)]),
    "msc_dataview_from_device_columns": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(RuntimeType),
                                                   C.c_uint32, C.POINTER(C.c_void_p),
                                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "msc_dataview_destroy": (C.c_int, [C.c_void_p]),
    "msc_dataview_invalidate": (C.c_int, [C.c_void_p]),
    "msc_dataview_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "msc_dataview_column": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p),
                                      C.POINTER(RuntimeType)]),
    "msc_state_create": (C.c_int, [C.c_void_p, C.POINTER(FeatureSpec), C.c_uint32, C.c_uint32,
                                   C.POINTER(C.c_void_p)]),
    "msc_state_destroy": (C.c_int, [C.c_void_p]),
    "msc_state_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "msc_hp_floats": (C.c_size_t, [C.c_int, C.c_uint32]),
    "msc_state_set_hp": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "msc_state_get_hp": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "msc_ss_bytes": (C.c_size_t, [C.c_int, C.c_uint32]),
    "msc_state_set_ss": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "msc_state_get_ss": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "msc_state_set_alpha": (C.c_int, [C.c_void_p, C.c_float]),
    "msc_state_get_alpha": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "msc_state_set_group_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "msc_state_get_group_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "msc_score_value": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                  C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "msc_score_tune": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                 C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "msc_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                 C.c_void_p, C.c_uint32]),
    "msc_entity_op": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]),
    "msc_score_data": (C.c_int, [C.c_void_p, C.c_void_p]),
    "msc_sweep_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                   C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "msc_sweep_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                 C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "msc_sweep_step_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                       C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "msc_sweep_step_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "msc_sweep_sequential": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "msc_blocked_draw": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "msc_blocked_tables": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    "msc_blocked_niw_params": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_uint32)]),
    "msc_blocked_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                     C.c_uint64, C.c_uint64]),
    "msc_sweep_blocked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    # (st, view, cols, row0, nrows, row_id0, z_dev, nproposals, launch_iters, seed, sweep, log_dev, trace_dev,
    #  proposed_dev, counters_dev)
    "msc_split_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                  C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "msc_split_merge_tables": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    "msc_chains_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]),
    "msc_chains_destroy": (C.c_int, [C.c_void_p]),
    "msc_chains_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    # (ch, view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, nsweeps, host_seeds, sweep, trace_every,
    #  trace_dev, occupied_dev)
    "msc_chains_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                   C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint64,
                                   C.c_uint32, C.c_void_p, C.c_void_p]),
    # (ch, view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, nsweeps, host_seeds, sweep, beta_dev,
    #  trace_every, trace_dev, occupied_dev)
    "msc_chains_sweep_tempered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                            C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_void_p]),
    # (ch, joint_dev, ld_joint, nrungs, beta_dev, rung_dev, parity, seed, sweep, proposed_dev, accepted_dev)
    "msc_chains_exchange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    # (ch, joint_dev, ld_joint, beta_from_dev, beta_to_dev, logw_dev)
    "msc_chains_anneal_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (ch, view, cols, row0, nrows, row_id0, z_dev, ld_z, order_dev, ld_order, pos0, npos, host_seeds, sweep, logw_dev,
    #  visit_logp_dev, ld_logp)
    "msc_chains_visit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                   C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                   C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    # (ch, host_ancestors, z_dev, ld_z, nrows)
    "msc_chains_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.c_uint64]),
    # (ch, view, cols, row0, nrows, features, nfeatures, logw_dev, flags, mix_dev, chain_logp_dev, ld_logp)
    "msc_chains_score_marginal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32),
                                            C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    # (ch, view, cols, row0, nrows, row_id0, logw_dev, flags, seed, sweep, chain_out_dev, z_out_dev, out_dev)
    "msc_chains_sample_predictive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                               C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    # (ch, view, cols, nrows, row_id0, z_dev, ld_z, nproposals, launch_iters, host_seeds, sweep, log_dev, trace_dev,
    #  proposed_dev, counters_dev)
    "msc_chains_split_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    # (ch, coords, n, slots_dev, ld_slots, host_seeds, sweep, values_host, evals_host)
    "msc_chains_hp_slice": (C.c_int, [C.c_void_p, C.POINTER(SliceCoord), C.c_uint32, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p, C.c_void_p]),
    # (st, coords, n, slots_dev, out_dev)
    "msc_score_joint": (C.c_int, [C.c_void_p, C.POINTER(SliceCoord), C.c_uint32, C.c_void_p, C.c_void_p]),
    # (ch, coords, n, slots_dev, ld_slots, out_dev, ld_out)
    "msc_chains_score_joint": (C.c_int, [C.c_void_p, C.POINTER(SliceCoord), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_uint64]),
    # (ch, joint_dev, ld_joint, z_dev, ld_z, nrows, iter, best_dev, best_z_dev, ld_best, best_iter_dev)
    "msc_chains_keep_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "msc_state_reduce_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "msc_state_commit_reduce": (C.c_int, [C.c_void_p]),
    "msc_state_reduce_pack": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "msc_state_reduce_unpack": (C.c_int, [C.c_void_p]),
    "msc_state_set_sweep_rows": (C.c_int, [C.c_void_p, C.c_uint64]),
    "msc_state_col_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "msc_state_set_col_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "msc_comm_unique_id_bytes": (C.c_size_t, []),
    "msc_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "msc_comm_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "msc_comm_adopt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "msc_comm_destroy": (C.c_int, [C.c_void_p]),
    "msc_comm_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "msc_state_allreduce": (C.c_int, [C.c_void_p, C.c_void_p]),
    "msc_sweep_step_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                         C.c_uint64, C.c_uint64, C.c_void_p]),
    "msc_accumulate_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "msc_hp_grid_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                     C.POINTER(C.c_void_p)]),
    "msc_hp_grid_destroy": (C.c_int, [C.c_void_p]),
    "msc_hp_grid_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "msc_hp_grid_gibbs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_void_p]),
    "msc_hp_slice": (C.c_int, [C.c_void_p, C.POINTER(SliceCoord), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                               C.c_void_p, C.c_void_p]),
    "msc_theta_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                  C.c_void_p]),
    "msc_sample_predictive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                        C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "msc_score_marginal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "msc_value_op_single": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "msc_relation_slice_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64]),
    "msc_relation_blocks": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p]),
    "msc_zmatrix_create": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "msc_zmatrix_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64]),
    "msc_zmatrix_nsamples": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "msc_zmatrix_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "msc_zmatrix_result": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "msc_zmatrix_partition_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "msc_zmatrix_partition_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "msc_zmatrix_partition_refine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "msc_zmatrix_reset": (C.c_int, [C.c_void_p]),
    "msc_zmatrix_destroy": (C.c_int, [C.c_void_p]),
    "msc_linkage_single": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "msc_partition_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_uint32, C.c_uint32] + [C.c_void_p] * 8),
    "msc_vi_table": (C.c_int, [C.c_uint32, C.c_void_p]),
    "msc_partition_refine_vi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32] +
                                [C.c_void_p] * 4),
}

EXPORTS = tuple(sorted(_SIGS))
_lib = None


def load():
    """dlopen the HIP library (torch first, so both share one libamdhip64)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C common_amd/csrc).  common_amd has no CPU fallback." % LIB_PATH)
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.msc_abi_version() != ABI_VERSION:
        raise ImportError("libmicroscopes_hip.so ABI %d != binding ABI %d" %
                          (lib.msc_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise MicroscopesHipError(rc, load().msc_last_error().decode("utf-8", "replace"))
