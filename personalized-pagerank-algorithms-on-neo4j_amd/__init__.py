"""pprhip — MI355X-native Personalized PageRank (FORA + All-Pair-Backward-Search).

Thin ctypes binding of the C ABI in include/pprhip.h.  The compute path lives entirely in
libpprhip.so (hand-written HIP kernels for gfx950); there is no Python or CPU fallback: importing
this package without the built library raises, and every compute call fails loudly when no GPU is
usable.  Build with `make -C personalized-pagerank-algorithms-on-neo4j_amd` or
`__graft_entry__.build()`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PPRHIP_LIB_PATH: another build of the SAME sources (the Makefile's sanitizer build, `make asan-test`); never a fallback
LIB_PATH = os.environ.get("PPRHIP_LIB_PATH") or os.path.join(_HERE, "libpprhip.so")

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_IO, ERR_STATE = -1, -2, -3, -4, -5, -6

KERNEL_NAMES = {0: "none", 1: "dense_pull", 2: "sparse_push", 3: "walk", 4: "backward_batch", 5: "dense_pull_batch",
                6: "query_setup"}
BATCH = 16  # PPRHIP_BATCH: queries in flight in fora_batch_single_source


class PprhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pprhip error %d: %s" % (code, msg))
        self.code = code


class Stats(C.Structure):
    _fields_ = [("pops", C.c_uint64), ("edge_pushes", C.c_uint64), ("enqueues", C.c_uint64),
                ("dead_end_pops", C.c_uint64), ("dense_nodes", C.c_uint64), ("levels", C.c_uint32),
                ("dense_levels", C.c_uint32), ("rounds", C.c_uint32), ("xl_targets", C.c_uint32),
                ("mc_sources", C.c_uint64), ("walks", C.c_uint64), ("walk_steps", C.c_uint64),
                ("select_passes", C.c_uint64), ("rsum", C.c_double), ("rmax_final", C.c_double),
                ("omega", C.c_double), ("kth_value", C.c_double), ("push_ms", C.c_double), ("mc_ms", C.c_double),
                ("select_ms", C.c_double), ("total_ms", C.c_double), ("push_bytes", C.c_uint64),
                ("mc_bytes", C.c_uint64), ("select_bytes", C.c_uint64), ("dominant_kernel_ms", C.c_double),
                ("dominant_kernel_bytes", C.c_uint64), ("dominant_kernel_launches", C.c_uint32),
                ("dominant_kernel_id", C.c_uint32), ("class_ms", C.c_double * 8), ("class_bytes", C.c_uint64 * 8),
                ("class_launches", C.c_uint32 * 8), ("dense_edges", C.c_uint64), ("sweep_min_bytes", C.c_uint64),
                ("walk_loads", C.c_uint64), ("walk_load_lanes", C.c_uint64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved") and not k.startswith("class_")}
        for k in ("class_ms", "class_bytes", "class_launches"):
            d[k] = list(getattr(self, k))
        return d


class Sweep(C.Structure):
    """pprhip_sweep_t: what a sweep cut found (support, the best prefix, the volume scanned, HIP-event times)."""
    _fields_ = [("support", C.c_uint64), ("profiled", C.c_uint64), ("best_size", C.c_uint64), ("best_cut", C.c_uint64),
                ("best_vol", C.c_uint64), ("best_conductance", C.c_double), ("total_vol", C.c_uint64),
                ("edge_slots", C.c_uint64), ("sort_ms", C.c_double), ("scan_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WeightedSweep(C.Structure):
    """pprhip_wsweep_t: what a weighted sweep cut found; cut and volume in quanta, one weight unit being 2**shift quanta."""
    _fields_ = [("support", C.c_uint64), ("profiled", C.c_uint64), ("best_size", C.c_uint64),
                ("best_cut_q", C.c_uint64), ("best_vol_q", C.c_uint64), ("best_conductance", C.c_double),
                ("total_vol_q", C.c_uint64), ("shift", C.c_int32), ("reserved", C.c_int32), ("edge_slots", C.c_uint64),
                ("sort_ms", C.c_double), ("scan_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class Tuning(C.Structure):
    _fields_ = [("c_walk_ns", C.c_double), ("c_edge_ns", C.c_double), ("c_pop_ns", C.c_double),
                ("c_level_ns", C.c_double), ("c_dense_edge_ns", C.c_double), ("c_dense_node_ns", C.c_double),
                ("dense_frac", C.c_double), ("max_rounds", C.c_int32), ("max_halvings", C.c_int32),
                ("halving_ratio", C.c_double), ("prior_levels", C.c_int32), ("gs_blocks", C.c_int32),
                ("gs_frac", C.c_double)]


class ForaConf(C.Structure):
    _fields_ = [("alpha", C.c_double), ("delta", C.c_double), ("pfail", C.c_double), ("rsum", C.c_double),
                ("min_delta", C.c_double), ("k", C.c_int32), ("n", C.c_uint32), ("m", C.c_uint64)]


# every symbol include/pprhip.h declares (tests check the library exports all of them)
EXPORTS = [
    "pprhip_last_error", "pprhip_version", "pprhip_device_count", "pprhip_tuning_default",
    "pprhip_conf_fora_whole_graph", "pprhip_conf_fora_topk", "pprhip_fora_whole_params", "pprhip_fora_topk_params",
    "pprhip_rmat_edges", "pprhip_edgelist_from_neo4j_csv", "pprhip_edgelist_info", "pprhip_edgelist_edges",
    "pprhip_edgelist_node_name", "pprhip_edgelist_destroy", "pprhip_csr_build", "pprhip_graph_create",
    "pprhip_graph_destroy", "pprhip_graph_release", "pprhip_graph_info", "pprhip_graph_set_tuning", "pprhip_graph_get_tuning",
    "pprhip_get_reserve", "pprhip_get_residue", "pprhip_forward_push", "pprhip_fwdpush_topk_reset",
    "pprhip_fwdpush_topk_round", "pprhip_random_walk_batch", "pprhip_fora_single_source", "pprhip_fora_topk",
    "pprhip_topk_select", "pprhip_monte_carlo", "pprhip_fora_batch_topk", "pprhip_backward_push",
    "pprhip_all_pair_backward", "pprhip_index_merge", "pprhip_index_info", "pprhip_index_arrays",
    "pprhip_index_write_dir", "pprhip_index_destroy", "pprhip_power_method", "pprhip_index_from_arrays",
    "pprhip_format_double", "pprhip_edgelist_from_neo4j_store", "pprhip_edgelist_build_csr",
    "pprhip_fora_batch_single_source", "pprhip_tuning_batch", "pprhip_tuning_batch_for", "pprhip_results_create", "pprhip_results_destroy",
    "pprhip_results_info", "pprhip_results_fetch", "pprhip_results_sum", "pprhip_fora_batch_single_source_resident",
    "pprhip_fora_batch", "pprhip_all_pair_backward_multi", "pprhip_comm_unique_id", "pprhip_comm_create",
    "pprhip_comm_destroy", "pprhip_comm_info", "pprhip_shard_target_range", "pprhip_all_pair_backward_sharded",
    "pprhip_topk_gather", "pprhip_comm_abort", "pprhip_owner_partition", "pprhip_index_from_entries",
    "pprhip_device_memory", "pprhip_graph_lift_host", "pprhip_lift_array", "pprhip_lift_destroy",
    "pprhip_fora_stream_open", "pprhip_fora_stream_submit", "pprhip_fora_stream_wait", "pprhip_fora_stream_close",
    "pprhip_set_kernel_timing", "pprhip_shard_target_cuts", "pprhip_forward_push_seeds", "pprhip_fora_seeds",
    "pprhip_fora_topk_seeds", "pprhip_fora_batch_seeds", "pprhip_fora_batch_topk_seeds",
    "pprhip_pair_params", "pprhip_walk_survival", "pprhip_ppr_pairs", "pprhip_ppr_targets",
    "pprhip_walk_index_density", "pprhip_walk_index_build", "pprhip_walk_index_drop", "pprhip_walk_index_info",
    "pprhip_walk_index_fetch", "pprhip_walk_index_usage", "pprhip_tuning_indexed", "pprhip_tuning_indexed_batch",
    "pprhip_sweep_cut", "pprhip_results_sweep_cut", "pprhip_local_cluster_seeds",
    "pprhip_get_reserve_sparse", "pprhip_get_residue_sparse", "pprhip_results_fetch_sparse",
    "pprhip_results_fetch_sparse_all",
    "pprhip_graph_set_weights", "pprhip_weights_info", "pprhip_weight_table_host", "pprhip_weighted_power_method",
    "pprhip_weighted_forward_push", "pprhip_weighted_random_walk_batch", "pprhip_weighted_fora",
    "pprhip_weighted_backward_push", "pprhip_weighted_walk_survival", "pprhip_weighted_ppr_targets",
    "pprhip_weighted_ppr_pairs", "pprhip_weighted_all_pair_backward",
    "pprhip_weighted_forward_push_seeds", "pprhip_weighted_fora_seeds", "pprhip_weighted_fora_topk",
    "pprhip_weighted_fora_topk_seeds",
    "pprhip_weighted_walk_index_build", "pprhip_weighted_walk_index_drop", "pprhip_weighted_walk_index_info",
    "pprhip_weighted_walk_index_fetch", "pprhip_weighted_walk_index_usage",
    "pprhip_weighted_fora_batch", "pprhip_weighted_fora_batch_seeds",
    "pprhip_weighted_fora_batch_topk", "pprhip_weighted_fora_batch_topk_seeds", "pprhip_walk_multi_shares",
    "pprhip_weight_quantum", "pprhip_weighted_sweep_cut", "pprhip_results_weighted_sweep_cut",
    "pprhip_weighted_local_cluster_seeds",
]
SPARSE_BY_ID, SPARSE_BY_VALUE = 0, 1  # PPRHIP_SPARSE_BY_*: the orders of the sparse getters
RELEASE_SPARSE = 16  # PPRHIP_RELEASE_SPARSE
RELEASE_WEIGHTS = 128  # PPRHIP_RELEASE_WEIGHTS
RELEASE_WEIGHTED_WALK_INDEX = 256  # PPRHIP_RELEASE_WEIGHTED_WALK_INDEX
PAIR_WALK_STREAM = 0xFFFF  # PPRHIP_PAIR_WALK_STREAM: the walk stream of every single-pair walk
COMM_ID_BYTES = 128

_lib = None
_LIVE = {}


def lib():
    """Loads libpprhip.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libpprhip.so is not built (%s); run `make -C %s`" % (LIB_PATH, _HERE))
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64, dbl, ci = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_int
    P = C.POINTER
    L.pprhip_last_error.restype = C.c_char_p
    L.pprhip_version.restype = ci
    L.pprhip_device_count.argtypes = [P(ci)]
    L.pprhip_tuning_default.argtypes = [P(Tuning)]
    L.pprhip_tuning_default.restype = None
    L.pprhip_tuning_batch.argtypes = [P(Tuning)]
    L.pprhip_tuning_batch.restype = None
    L.pprhip_tuning_batch_for.argtypes = [ci, P(Tuning)]
    L.pprhip_tuning_batch_for.restype = None
    L.pprhip_conf_fora_whole_graph.argtypes = [u32, u64, dbl, P(ForaConf)]
    L.pprhip_conf_fora_topk.argtypes = [u32, u64, ci, dbl, P(ForaConf)]
    L.pprhip_fora_whole_params.argtypes = [P(ForaConf), dbl, P(dbl), P(dbl)]
    L.pprhip_fora_topk_params.argtypes = [P(ForaConf), dbl, dbl, P(dbl), P(dbl), P(dbl)]
    L.pprhip_rmat_edges.argtypes = [ci, ci, u64, vp, vp]
    L.pprhip_edgelist_from_neo4j_csv.argtypes = [C.c_char_p, C.c_char_p, P(vp)]
    L.pprhip_edgelist_from_neo4j_store.argtypes = [C.c_char_p, P(vp)]
    L.pprhip_edgelist_build_csr.argtypes = [vp, ci, vp, vp]
    L.pprhip_edgelist_info.argtypes = [vp, P(u32), P(u64)]
    L.pprhip_edgelist_edges.argtypes = [vp, P(vp), P(vp)]
    L.pprhip_edgelist_node_name.argtypes = [vp, u32]
    L.pprhip_edgelist_node_name.restype = C.c_char_p
    L.pprhip_edgelist_destroy.argtypes = [vp]
    L.pprhip_edgelist_destroy.restype = None
    L.pprhip_csr_build.argtypes = [u32, u64, vp, vp, ci, vp, vp]
    L.pprhip_graph_create.argtypes = [u32, u64, vp, vp, vp, vp, ci, P(vp)]
    L.pprhip_graph_destroy.argtypes = [vp]
    L.pprhip_graph_destroy.restype = None
    L.pprhip_graph_release.argtypes = [vp, C.c_uint]
    L.pprhip_graph_info.argtypes = [vp, P(u32), P(u64), P(ci)]
    L.pprhip_device_memory.argtypes = [vp, P(u64), P(u64)]
    L.pprhip_graph_set_tuning.argtypes = [vp, P(Tuning)]
    L.pprhip_graph_get_tuning.argtypes = [vp, P(Tuning)]
    L.pprhip_get_reserve.argtypes = [vp, vp]
    L.pprhip_get_residue.argtypes = [vp, vp]
    L.pprhip_forward_push.argtypes = [vp, i32, dbl, dbl, vp, vp, P(dbl), P(Stats)]
    L.pprhip_fwdpush_topk_reset.argtypes = [vp, i32, dbl]
    L.pprhip_fwdpush_topk_round.argtypes = [vp, dbl, dbl, P(dbl), P(Stats)]
    L.pprhip_random_walk_batch.argtypes = [vp, vp, vp, u64, dbl, u64, u32, ci, vp, vp]
    L.pprhip_fora_single_source.argtypes = [vp, i32, dbl, P(ForaConf), u64, ci, vp, P(Stats)]
    L.pprhip_forward_push_seeds.argtypes = [vp, vp, vp, ci, dbl, dbl, vp, vp, P(dbl), P(Stats)]
    L.pprhip_fora_seeds.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), u64, ci, vp, P(Stats)]
    L.pprhip_fora_topk_seeds.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), u64, vp, vp, ci, P(ci), vp, P(Stats)]
    L.pprhip_fora_batch_seeds.argtypes = [vp, vp, vp, vp, ci, dbl, P(ForaConf), u64, ci, vp, vp, ci, vp, vp, vp, vp,
                                          P(Stats)]
    L.pprhip_fora_batch_topk_seeds.argtypes = [vp, vp, vp, vp, ci, ci, dbl, dbl, u64, vp, vp, P(Stats)]
    L.pprhip_fora_topk.argtypes = [vp, i32, dbl, P(ForaConf), u64, vp, vp, ci, P(ci), vp, P(Stats)]
    L.pprhip_topk_select.argtypes = [vp, ci, vp, vp, ci, P(ci), P(dbl), P(Stats)]
    L.pprhip_monte_carlo.argtypes = [vp, i32, dbl, P(ForaConf), u64, vp, P(Stats)]
    L.pprhip_fora_batch_single_source.argtypes = [vp, vp, ci, dbl, P(ForaConf), u64, ci, vp, ci, vp, vp, vp, vp, P(Stats)]
    L.pprhip_fora_batch_single_source_resident.argtypes = [vp, vp, ci, dbl, P(ForaConf), u64, ci, vp, vp, ci, vp, vp, vp,
                                                           vp, P(Stats)]
    L.pprhip_results_create.argtypes = [vp, ci, P(vp)]
    L.pprhip_results_destroy.argtypes = [vp]
    L.pprhip_results_destroy.restype = None
    L.pprhip_results_info.argtypes = [vp, P(ci), P(ci), P(u32)]
    L.pprhip_results_fetch.argtypes = [vp, ci, vp]
    L.pprhip_results_sum.argtypes = [vp, ci, P(dbl)]
    L.pprhip_fora_batch_topk.argtypes = [vp, vp, ci, ci, dbl, dbl, u64, vp, vp, P(Stats)]
    L.pprhip_fora_batch.argtypes = [P(vp), ci, vp, ci, ci, dbl, P(ForaConf), u64, ci, vp, vp, vp, vp]
    L.pprhip_all_pair_backward_multi.argtypes = [P(vp), ci, dbl, dbl, ci, P(vp), vp]
    L.pprhip_comm_unique_id.argtypes = [vp]
    L.pprhip_comm_create.argtypes = [vp, vp, ci, ci, P(vp)]
    L.pprhip_comm_destroy.argtypes = [vp]
    L.pprhip_comm_destroy.restype = None
    L.pprhip_comm_info.argtypes = [vp, P(ci), P(ci)]
    L.pprhip_shard_target_range.argtypes = [ci, ci, u32, P(u32), P(u32)]
    L.pprhip_shard_target_cuts.argtypes = [vp, ci, dbl, dbl, ci, vp, P(dbl)]
    L.pprhip_all_pair_backward_sharded.argtypes = [vp, dbl, dbl, ci, P(vp), P(Stats)]
    L.pprhip_topk_gather.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
    L.pprhip_comm_abort.argtypes = [vp]
    L.pprhip_owner_partition.argtypes = [u32, ci, vp, u64, vp, vp]
    L.pprhip_index_from_entries.argtypes = [u32, vp, vp, vp, u64, ci, P(vp)]
    L.pprhip_backward_push.argtypes = [vp, i32, dbl, dbl, vp, vp, P(Stats)]
    L.pprhip_all_pair_backward.argtypes = [vp, dbl, dbl, ci, u32, u32, P(vp), P(Stats)]
    L.pprhip_weighted_all_pair_backward.argtypes = [vp, dbl, dbl, ci, u32, u32, P(vp), P(Stats)]
    L.pprhip_index_merge.argtypes = [P(vp), ci, ci, P(vp)]
    L.pprhip_index_from_arrays.argtypes = [u32, vp, vp, vp, P(vp)]
    L.pprhip_format_double.argtypes = [dbl, C.c_char_p, C.c_size_t]
    L.pprhip_index_info.argtypes = [vp, P(u32), P(u64)]
    L.pprhip_index_arrays.argtypes = [vp, P(vp), P(vp), P(vp)]
    L.pprhip_index_write_dir.argtypes = [vp, C.c_char_p]
    L.pprhip_index_destroy.argtypes = [vp]
    L.pprhip_index_destroy.restype = None
    L.pprhip_power_method.argtypes = [vp, i32, dbl, ci, vp, P(Stats)]
    L.pprhip_graph_lift_host.argtypes = [u32, u64, vp, vp, vp, vp, ci, P(vp)]
    L.pprhip_lift_array.argtypes = [vp, ci, P(vp), P(u64)]
    L.pprhip_lift_destroy.argtypes = [vp]
    L.pprhip_lift_destroy.restype = None
    L.pprhip_fora_stream_open.argtypes = [vp, dbl, P(ForaConf), ci, P(vp)]
    L.pprhip_fora_stream_submit.argtypes = [vp, vp, ci, u64, vp, ci, vp, vp, vp, P(u64)]
    L.pprhip_fora_stream_wait.argtypes = [vp, u64, P(Stats)]
    L.pprhip_fora_stream_close.argtypes = [vp]
    L.pprhip_set_kernel_timing.argtypes = [ci]
    L.pprhip_pair_params.argtypes = [P(ForaConf), dbl, dbl, P(dbl), P(u64)]
    L.pprhip_walk_survival.argtypes = [vp, dbl, vp]
    L.pprhip_ppr_pairs.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), dbl, u64, vp, P(Stats)]
    L.pprhip_ppr_targets.argtypes = [vp, vp, vp, vp, ci, dbl, dbl, vp, vp, ci, vp, vp, vp, vp, P(Stats)]
    L.pprhip_walk_index_density.argtypes = [P(ForaConf), dbl, dbl, P(dbl)]
    L.pprhip_walk_index_build.argtypes = [vp, dbl, u64, dbl, P(Stats)]
    L.pprhip_walk_index_drop.argtypes = [vp]
    L.pprhip_walk_index_info.argtypes = [vp, P(ci), P(dbl), P(u64), P(dbl), P(u64), P(u64)]
    L.pprhip_walk_index_fetch.argtypes = [vp, i32, vp, u64, P(u64)]
    L.pprhip_walk_index_usage.argtypes = [vp, P(u64), P(u64), ci]
    L.pprhip_weighted_walk_index_build.argtypes = [vp, dbl, u64, dbl, P(Stats)]
    L.pprhip_weighted_walk_index_drop.argtypes = [vp]
    L.pprhip_weighted_walk_index_info.argtypes = [vp, P(ci), P(dbl), P(u64), P(dbl), P(u64), P(u64)]
    L.pprhip_weighted_walk_index_fetch.argtypes = [vp, i32, vp, u64, P(u64)]
    L.pprhip_weighted_walk_index_usage.argtypes = [vp, P(u64), P(u64), ci]
    L.pprhip_tuning_indexed.argtypes = [P(Tuning)]
    L.pprhip_tuning_indexed.restype = None
    L.pprhip_tuning_indexed_batch.argtypes = [P(Tuning)]
    L.pprhip_tuning_indexed_batch.restype = None
    L.pprhip_sweep_cut.argtypes = [vp, ci, u64, u64, vp, vp, vp, u64, P(Sweep)]
    L.pprhip_results_sweep_cut.argtypes = [vp, ci, ci, u64, u64, vp, vp, vp, u64, P(Sweep)]
    L.pprhip_local_cluster_seeds.argtypes = [vp, vp, vp, ci, dbl, dbl, ci, u64, u64, vp, u64, P(Sweep), P(Stats)]
    L.pprhip_get_reserve_sparse.argtypes = [vp, dbl, ci, vp, vp, u64, P(u64)]
    L.pprhip_get_residue_sparse.argtypes = [vp, dbl, ci, vp, vp, u64, P(u64)]
    L.pprhip_results_fetch_sparse.argtypes = [vp, ci, dbl, ci, vp, vp, u64, P(u64)]
    L.pprhip_results_fetch_sparse_all.argtypes = [vp, dbl, ci, vp, vp, vp, u64, P(u64)]
    L.pprhip_graph_set_weights.argtypes = [vp, vp]
    L.pprhip_weights_info.argtypes = [vp, P(ci), P(u64)]
    L.pprhip_weight_table_host.argtypes = [u32, u64, vp, vp, vp, vp]
    L.pprhip_weighted_power_method.argtypes = [vp, i32, dbl, ci, vp, P(Stats)]
    L.pprhip_weighted_forward_push.argtypes = [vp, i32, dbl, dbl, vp, vp, P(dbl), P(Stats)]
    L.pprhip_weighted_random_walk_batch.argtypes = [vp, vp, vp, u64, dbl, u64, u32, ci, vp, vp]
    L.pprhip_weighted_fora.argtypes = [vp, i32, dbl, P(ForaConf), u64, dbl, vp, P(Stats)]
    L.pprhip_weighted_forward_push_seeds.argtypes = [vp, vp, vp, ci, dbl, dbl, vp, vp, P(dbl), P(Stats)]
    L.pprhip_weighted_fora_seeds.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), u64, dbl, vp, P(Stats)]
    L.pprhip_weighted_fora_topk.argtypes = [vp, i32, dbl, P(ForaConf), u64, vp, vp, ci, P(ci), vp, P(Stats)]
    L.pprhip_weighted_fora_topk_seeds.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), u64, vp, vp, ci, P(ci), vp,
                                                  P(Stats)]
    L.pprhip_weighted_fora_batch.argtypes = [vp, vp, ci, dbl, P(ForaConf), u64, dbl, vp, vp, ci, vp, vp, vp, vp, P(Stats)]
    L.pprhip_weighted_fora_batch_seeds.argtypes = [vp, vp, vp, vp, ci, dbl, P(ForaConf), u64, dbl, vp, vp, ci, vp, vp, vp,
                                                   vp, P(Stats)]
    L.pprhip_weighted_fora_batch_topk.argtypes = [vp, vp, ci, dbl, P(ForaConf), u64, vp, vp, vp, vp, vp, P(Stats)]
    L.pprhip_weighted_fora_batch_topk_seeds.argtypes = [vp, vp, vp, vp, ci, dbl, P(ForaConf), u64, vp, vp, vp, vp, vp,
                                                        P(Stats)]
    L.pprhip_walk_multi_shares.argtypes = [vp, u32, P(u64), vp]
    L.pprhip_weighted_backward_push.argtypes = [vp, i32, dbl, dbl, vp, vp, P(Stats)]
    L.pprhip_weighted_walk_survival.argtypes = [vp, dbl, vp]
    L.pprhip_weighted_ppr_targets.argtypes = [vp, vp, vp, vp, ci, dbl, dbl, vp, vp, ci, vp, vp, vp, vp, P(Stats)]
    L.pprhip_weighted_ppr_pairs.argtypes = [vp, vp, vp, ci, dbl, P(ForaConf), dbl, u64, vp, P(Stats)]
    L.pprhip_weight_quantum.argtypes = [u64, vp, P(ci)]
    L.pprhip_weighted_sweep_cut.argtypes = [vp, ci, u64, dbl, vp, vp, vp, u64, P(WeightedSweep)]
    L.pprhip_results_weighted_sweep_cut.argtypes = [vp, ci, ci, u64, dbl, vp, vp, vp, u64, P(WeightedSweep)]
    L.pprhip_weighted_local_cluster_seeds.argtypes = [vp, vp, vp, ci, dbl, dbl, ci, u64, dbl, vp, u64, P(WeightedSweep),
                                                      P(Stats)]
    _lib = L
    # the destroy entry points, reachable from destructors that run while the interpreter shuts down (the name `lib`
    # may already be None then: "TypeError: 'NoneType' object is not callable" out of Index.__del__, round 3)
    _LIVE.update(graph_destroy=L.pprhip_graph_destroy, results_destroy=L.pprhip_results_destroy,
                 comm_destroy=L.pprhip_comm_destroy)
    return L


def _check(rc):
    if rc != OK:
        raise PprhipError(rc, lib().pprhip_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _seed_arrays(seeds, weights):
    """A seed set as the C ABI takes it: int32 ids and float64 weights of the same length (None: uniform)."""
    s = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(np.atleast_1d(weights), dtype=np.float64)
    if w is not None and w.size != s.size:
        raise ValueError("weights: %d entries for %d seeds" % (w.size, s.size))
    return s, w


def _seed_start(seeds, weights):
    """The leading arguments of a seed-set call (Graph._push_call and its like): ids, weights | None, count."""
    s, w = _seed_arrays(seeds, weights)
    return s, w, s.size


def _batch_outputs(q, n, k, fetch, out, per_query):
    """The output arrays of a batched call of q queries: (vectors[q, n] | None, ids[q, k] | None, vals[q, k] | None,
    n_sel[q] | None, Stats array | None).  out: the caller's array for the vectors (with fetch), checked here."""
    if fetch and out is not None:
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.shape == (q, n)
    elif fetch:
        out = np.empty((q, n))
    else:
        out = None
    ids = np.empty((q, k), dtype=np.int32) if k > 0 else None
    vals = np.empty((q, k)) if k > 0 else None
    nsel = np.zeros(q, dtype=np.int32) if k > 0 else None
    return out, ids, vals, nsel, ((Stats * q)() if per_query and q else None)


def _seed_set_arrays(sets, weights):
    """q seed sets as the batched C calls take them: (seeds int32, weights float64 | None, offsets uint64 [q + 1]).
    weights: None (every set uniform) or one entry per set, each None (that set uniform: ones) or as long as its set."""
    sets = [np.ascontiguousarray(np.atleast_1d(s), dtype=np.int32).ravel() for s in sets]
    if weights is not None:
        weights = list(weights)
        if len(weights) != len(sets):
            raise ValueError("weights: %d entries for %d seed sets" % (len(weights), len(sets)))
    offsets = np.zeros(len(sets) + 1, dtype=np.uint64)
    if sets:
        offsets[1:] = np.cumsum([s.size for s in sets], dtype=np.uint64)
    seeds = np.concatenate(sets).astype(np.int32, copy=False) if sets else np.zeros(0, dtype=np.int32)
    if weights is None:
        return np.ascontiguousarray(seeds), None, offsets
    ws = []
    for i, (s, w) in enumerate(zip(sets, weights)):
        w = np.ones(s.size) if w is None else np.ascontiguousarray(np.atleast_1d(w), dtype=np.float64).ravel()
        if w.size != s.size:
            raise ValueError("weights of set %d: %d entries for %d seeds" % (i, w.size, s.size))
        ws.append(w)
    wv = np.concatenate(ws).astype(np.float64, copy=False) if ws else np.zeros(0)
    return np.ascontiguousarray(seeds), np.ascontiguousarray(wv), offsets


def _sweep_call(n, max_size, cap, call, info_type=None):
    """The output arrays of a sweep cut for `cap` positions (None: everything profiled), the call, the filled parts."""
    room = n if not max_size else min(n, int(max_size))
    cap = room if cap is None else min(int(cap), room)
    order = np.empty(cap, dtype=np.int32) if cap else None
    vol = np.empty(cap, dtype=np.uint64) if cap else None
    cut = np.empty(cap, dtype=np.uint64) if cap else None
    info = (info_type or Sweep)()
    _check(call(_ptr(order), _ptr(vol), _ptr(cut), cap, C.byref(info)))
    k = min(cap, info.profiled)
    if not cap:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), info
    return order[:k].copy(), vol[:k].copy(), cut[:k].copy(), info


def set_kernel_timing(on):
    """Kernel-class times in Stats.class_ms (HIP events around every group of launches): off by default - they cost the
    latency-bound paths 2-8 %; on == 2 ("sweeps"): only the dense sweeps are timed, every other class counted.  Returns
    the previous state (False, True or 2), which can be passed back."""
    was = lib().pprhip_set_kernel_timing(2 if (on == 2 and on is not True) else (1 if on else 0))
    return 2 if was == 2 else bool(was)


def device_count():
    c = C.c_int(0)
    _check(lib().pprhip_device_count(C.byref(c)))
    return c.value


# ------------------------------------------------------------------ ingest helpers (host side)
def rmat_edges(scale, edge_factor=16, seed=1):
    m = edge_factor << scale
    src = np.empty(m, dtype=np.int32)
    dst = np.empty(m, dtype=np.int32)
    _check(lib().pprhip_rmat_edges(scale, edge_factor, seed, _ptr(src), _ptr(dst)))
    return src, dst


def csr_build(n, key, val, newest_first=False):
    key = np.ascontiguousarray(key, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.int32)
    rp = np.empty(n + 1, dtype=np.uint32)
    ci = np.empty(max(key.size, 1), dtype=np.int32)
    _check(lib().pprhip_csr_build(n, key.size, _ptr(key), _ptr(val), int(newest_first), _ptr(rp), _ptr(ci)))
    return rp, ci[:key.size]


def load_neo4j_csv(nodes_csv, rels_csv):
    """Returns (n, src, dst, names) with node id = row index of the nodes file."""
    h = C.c_void_p()
    _check(lib().pprhip_edgelist_from_neo4j_csv(nodes_csv.encode(), rels_csv.encode(), C.byref(h)))
    try:
        n, m = C.c_uint32(), C.c_uint64()
        _check(lib().pprhip_edgelist_info(h, C.byref(n), C.byref(m)))
        ps, pd = C.c_void_p(), C.c_void_p()
        _check(lib().pprhip_edgelist_edges(h, C.byref(ps), C.byref(pd)))
        if m.value:
            src = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_int32)), shape=(m.value,)).copy()
            dst = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_int32)), shape=(m.value,)).copy()
        else:
            src = np.zeros(0, dtype=np.int32)
            dst = np.zeros(0, dtype=np.int32)
        names = [lib().pprhip_edgelist_node_name(h, i).decode() for i in range(n.value)]
    finally:
        lib().pprhip_edgelist_destroy(h)
    return n.value, src, dst, names


def out_edge_order(src, newest_first=False):
    """The permutation from an edge list's order to the order of HostCsr(n, src, dst, newest_first).out_ci (csr_build:
    stable by source; inside a row descending edge index with newest_first): out_ci == dst[perm].  A caller holding
    (src, dst, w) aligns its relationship weights with it: Graph.set_weights(w[perm])."""
    src = np.asarray(src)
    idx = np.arange(src.size, dtype=np.int64)
    if newest_first:
        idx = idx[::-1]
    return idx[np.argsort(src[idx], kind="stable")]


def weight_table_host(out_rp, weights):
    """The prefix rule of the relationship weights without a device (pprhip_weight_table_host): (cum[m], wsum[n]) -
    cum of a row is the left-to-right sequential fp64 sum in row order, wsum its last element.  The validation of
    Graph.set_weights: PprhipError(ERR_INVALID) names the edge or the node."""
    rp = np.ascontiguousarray(out_rp, dtype=np.uint32)
    w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    n, m = rp.size - 1, w.size
    cum, ws = np.empty(m), np.empty(max(n, 1))
    _check(lib().pprhip_weight_table_host(n, m, _ptr(rp), _ptr(w), _ptr(cum), _ptr(ws)))
    return cum, ws[:n]


def walk_multi_shares(counts, base_waves):
    """The dealing rule of the batched weighted top-k's merged walk launch without a device
    (pprhip_walk_multi_shares).  counts: the walks of the BATCH columns' plans (0: idle); base_waves: the waves of a
    single walk launch.  Returns (per, first[BATCH + 1]): column c owns the waves [first[c], first[c + 1]), wave b of
    them the column's walks [(b - first[c]) * per, min(.. + per, counts[c]))."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).ravel()
    if c.size != BATCH:
        raise ValueError("counts: %d entries for %d columns" % (c.size, BATCH))
    per, first = C.c_uint64(), np.zeros(BATCH + 1, dtype=np.uint32)
    _check(lib().pprhip_walk_multi_shares(_ptr(c), int(base_waves), C.byref(per), _ptr(first)))
    return per.value, first


def weight_quantum(weights):
    """The shift s of the weighted sweep cut's quantum rule for a weight array, without a device
    (pprhip_weight_quantum): relationship e counts q(e) = max(1, rint(w(e) * 2**s)) quanta.  The validation of
    Graph.set_weights: PprhipError(ERR_INVALID) names the edge."""
    w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    s = C.c_int()
    _check(lib().pprhip_weight_quantum(w.size, _ptr(w), C.byref(s)))
    return s.value


class HostCsr:
    """Host out-/in-CSR pair built by the product's ingest code (input data for engine and oracle)."""

    def __init__(self, n, src, dst, newest_first=False):
        self.n = int(n)
        self.m = int(len(src))
        self.out_rp, self.out_ci = csr_build(n, src, dst, newest_first)
        self.in_rp, self.in_ci = csr_build(n, dst, src, newest_first)

    @classmethod
    def rmat(cls, scale, edge_factor=16, seed=1):
        src, dst = rmat_edges(scale, edge_factor, seed)
        return cls(1 << scale, src, dst)

    @classmethod
    def from_neo4j_store(cls, store_dir):
        """A Neo4j 3.x store directory (e.g. target/got.db) read without a JVM; adjacency in chain order."""
        h = C.c_void_p()
        _check(lib().pprhip_edgelist_from_neo4j_store(store_dir.encode(), C.byref(h)))
        try:
            n, m = C.c_uint32(), C.c_uint64()
            _check(lib().pprhip_edgelist_info(h, C.byref(n), C.byref(m)))
            self = cls.__new__(cls)
            self.n, self.m = n.value, m.value
            self.out_rp = np.empty(self.n + 1, dtype=np.uint32)
            self.in_rp = np.empty(self.n + 1, dtype=np.uint32)
            self.out_ci = np.empty(max(self.m, 1), dtype=np.int32)
            self.in_ci = np.empty(max(self.m, 1), dtype=np.int32)
            _check(lib().pprhip_edgelist_build_csr(h, 0, _ptr(self.out_rp), _ptr(self.out_ci)))
            _check(lib().pprhip_edgelist_build_csr(h, 1, _ptr(self.in_rp), _ptr(self.in_ci)))
            self.out_ci, self.in_ci = self.out_ci[:self.m], self.in_ci[:self.m]
            self.names = [lib().pprhip_edgelist_node_name(h, i).decode() for i in range(self.n)]
        finally:
            lib().pprhip_edgelist_destroy(h)
        return self

    @classmethod
    def from_neo4j_csv(cls, nodes_csv, rels_csv):
        n, src, dst, names = load_neo4j_csv(nodes_csv, rels_csv)
        h = cls(n, src, dst, newest_first=True)  # HeavyGraph lists newest relationships first
        h.names = names
        return h


LIFT_ARRAYS = {  # pprhip_lift_array: name -> (id, dtype)
    "new2old": (0, np.int32), "old2new": (1, np.int32), "out_rp": (2, np.uint32), "out_ci": (3, np.int32),
    "in_rp": (4, np.uint32), "in_ci": (5, np.int32), "nz_rows": (6, np.int32), "zin_rows": (7, np.int32),
    "flags": (8, np.uint8), "chunk_starts": (9, np.uint32), "cross": (10, np.uint64), "edge_base": (11, np.uint64),
    "seg_base": (12, np.uint64), "sl_ci": (13, np.int32), "sl_flags": (14, np.uint8), "sl_chunk_starts": (15, np.uint32),
    "seg_row": (16, np.uint32), "seg_off": (17, np.uint32),
    # the row-panel copy the single-query sweep walks (empty when the graph has none)
    "panel_sizes": (18, np.uint64), "panel_src": (19, np.int32), "panel_row": (20, np.uint16),
    "panel_items": (21, np.uint32), "panel_desc": (22, np.uint32), "panel_item0": (23, np.uint32),
}


def lift_host(host, threads=0, with_in=True):
    """The host half of the graph lift (pprhip_graph_lift_host; needs no device): dict of the internal layout's arrays."""
    h = C.c_void_p()
    _check(lib().pprhip_graph_lift_host(C.c_uint32(host.n), C.c_uint64(host.m), _ptr(host.out_rp), _ptr(host.out_ci),
                                        _ptr(host.in_rp) if with_in else None, _ptr(host.in_ci) if with_in else None,
                                        int(threads), C.byref(h)))
    try:
        out = {}
        for name, (which, dt) in LIFT_ARRAYS.items():
            p, nb = C.c_void_p(), C.c_uint64()
            _check(lib().pprhip_lift_array(h, which, C.byref(p), C.byref(nb)))
            if nb.value:
                buf = (C.c_uint8 * nb.value).from_address(p.value)
                out[name] = np.frombuffer(buf, dtype=dt).copy()
            else:
                out[name] = np.empty(0, dtype=dt)
        return out
    finally:
        lib().pprhip_lift_destroy(h)


# ------------------------------------------------------------------ device graph
def conf_whole_graph(n, m, alpha):
    c = ForaConf()
    _check(lib().pprhip_conf_fora_whole_graph(n, m, alpha, C.byref(c)))
    return c


def conf_topk(n, m, k, alpha):
    c = ForaConf()
    _check(lib().pprhip_conf_fora_topk(n, m, k, alpha, C.byref(c)))
    return c


def fora_whole_params(conf, eps):
    a, b = C.c_double(), C.c_double()
    _check(lib().pprhip_fora_whole_params(C.byref(conf), eps, C.byref(a), C.byref(b)))
    return a.value, b.value


def pair_params(conf, eps, rmax=0.0):
    """Single pairs (pprhip_pair_params): (r_max, walks per pair); rmax 0 picks the balanced default."""
    r, w = C.c_double(), C.c_uint64()
    _check(lib().pprhip_pair_params(C.byref(conf), eps, rmax, C.byref(r), C.byref(w)))
    return r.value, w.value


def fora_topk_params(conf, eps, delta):
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _check(lib().pprhip_fora_topk_params(C.byref(conf), eps, delta, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def tuning_default():
    t = Tuning()
    lib().pprhip_tuning_default(C.byref(t))
    return t


def tuning_batch():
    t = Tuning()
    lib().pprhip_tuning_batch(C.byref(t))
    return t


def tuning_indexed():
    """The single-query profile for a handle with a walk index (pprhip_tuning_indexed); set it with Graph.set_tuning."""
    t = Tuning()
    lib().pprhip_tuning_indexed(C.byref(t))
    return t


def tuning_indexed_batch():
    """The batch profile for a handle with a walk index (pprhip_tuning_indexed_batch)."""
    t = Tuning()
    lib().pprhip_tuning_indexed_batch(C.byref(t))
    return t


def walk_index_density(conf, eps, rmax=0.0):
    """Terminals per out-edge of a walk index that covers every whole-graph FORA query whose last push threshold is
    <= rmax (0: rmax0 of conf and eps): (1 - alpha) * rmax * omega * (1 + 2^-20)  (pprhip_walk_index_density)."""
    d = C.c_double()
    _check(lib().pprhip_walk_index_density(C.byref(conf), eps, rmax, C.byref(d)))
    return d.value


def tuning_batch_for(q):
    """The batch profile for a call of q queries (pprhip_tuning_batch_for)."""
    t = Tuning()
    lib().pprhip_tuning_batch_for(int(q), C.byref(t))
    return t


class Index:
    """All-pair inverted index (CSR by source)."""

    def __init__(self, handle):
        self.h = handle
        self._destroy = lib().pprhip_index_destroy  # kept: at interpreter shutdown the module's globals may be gone

    def arrays(self):
        n, e = C.c_uint32(), C.c_uint64()
        _check(lib().pprhip_index_info(self.h, C.byref(n), C.byref(e)))
        po, pt, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().pprhip_index_arrays(self.h, C.byref(po), C.byref(pt), C.byref(pv)))
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n.value + 1,)).copy()
        if e.value:
            tg = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_int32)), shape=(e.value,)).copy()
            vl = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_double)), shape=(e.value,)).copy()
        else:
            tg, vl = np.zeros(0, dtype=np.int32), np.zeros(0)
        return off, tg, vl

    def write_dir(self, path):
        _check(lib().pprhip_index_write_dir(self.h, path.encode()))

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (a destructor at interpreter shutdown must not raise)
            pass


def index_from_arrays(n, offsets, targets, values):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float64)
    out = C.c_void_p()
    _check(lib().pprhip_index_from_arrays(n, _ptr(offsets), _ptr(targets), _ptr(values), C.byref(out)))
    return Index(out)


def format_double(d):
    """java.lang.Double.toString(d), the number format of the reference's result files."""
    buf = C.create_string_buffer(64)
    n = lib().pprhip_format_double(d, buf, 64)
    if n < 0:
        raise PprhipError(n, "pprhip_format_double failed")
    return buf.value.decode()


def merge_indexes(shards, k):
    arr = (C.c_void_p * len(shards))(*[s.h for s in shards])
    out = C.c_void_p()
    _check(lib().pprhip_index_merge(arr, len(shards), k, C.byref(out)))
    return Index(out)


def owner_partition(n, world, sources):
    """The sharded All-Pair's partition rule on the host: (counts[world], order[count]) - entries owner by owner."""
    sources = np.ascontiguousarray(sources, dtype=np.int32)
    counts = np.zeros(world, dtype=np.uint64)
    order = np.zeros(max(sources.size, 1), dtype=np.uint64)
    _check(lib().pprhip_owner_partition(n, world, _ptr(sources), sources.size, _ptr(counts), _ptr(order)))
    return counts, order[:sources.size]


def index_from_entries(n, sources, targets, values, k):
    """The finished index from (source, target, value) entries in any order (k rule applied per source)."""
    sources = np.ascontiguousarray(sources, dtype=np.int32)
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float64)
    out = C.c_void_p()
    _check(lib().pprhip_index_from_entries(n, _ptr(sources), _ptr(targets), _ptr(values), sources.size, k, C.byref(out)))
    return Index(out)


def shard_target_range(rank, world, n):
    b, e = C.c_uint32(), C.c_uint32()
    _check(lib().pprhip_shard_target_range(rank, world, n, C.byref(b), C.byref(e)))
    return b.value, e.value


CUT_EQUAL, CUT_BY_WORK, CUT_AUTO = 0, 1, 2


def shard_target_cuts(graph, world, alpha, threshold, mode=CUT_AUTO):
    """pprhip_shard_target_cuts: (cuts[world + 1], skew) - the target ranges a sharded All-Pair run searches and the
    largest share of the modelled work equal counts would give one rank (x the mean)."""
    cuts = np.zeros(world + 1, dtype=np.uint32)
    skew = C.c_double()
    _check(lib().pprhip_shard_target_cuts(graph.h, world, alpha, threshold, mode, _ptr(cuts), C.byref(skew)))
    return cuts, skew.value


def comm_unique_id():
    """The bytes rank 0 hands to every rank before Comm() (an RCCL unique id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().pprhip_comm_unique_id(buf))
    return buf.raw


class Comm:
    """One rank of a multi-GPU group: an RCCL communicator bound to this rank's graph replica (collective create)."""

    def __init__(self, graph, uid, rank, world):
        self.graph = graph
        self.rank, self.world = rank, world
        self.h = C.c_void_p()
        buf = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _check(lib().pprhip_comm_create(graph.h, buf, rank, world, C.byref(self.h)))

    def all_pair_backward_sharded(self, alpha, threshold, k):
        """Collective: returns (Index of the sources this rank owns, Stats)."""
        out, st = C.c_void_p(), Stats()
        _check(lib().pprhip_all_pair_backward_sharded(self.h, alpha, threshold, k, C.byref(out), C.byref(st)))
        return Index(out), st

    def topk_gather(self, ids, vals, rows_max):
        """Collective: rank 0 gets (ids[world, rows_max, k], vals[...]), the others None."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        rows, k = ids.shape
        ri = np.empty((self.world, rows_max, k), dtype=np.int32) if self.rank == 0 else None
        rv = np.empty((self.world, rows_max, k)) if self.rank == 0 else None
        _check(lib().pprhip_topk_gather(self.h, _ptr(ids), _ptr(vals), rows, rows_max, k, _ptr(ri), _ptr(rv)))
        return (ri, rv) if self.rank == 0 else None

    def abort(self):
        """Leaves the group at once (peers' pending operations end with an error instead of waiting)."""
        if getattr(self, "h", None):
            _check(lib().pprhip_comm_abort(self.h))

    def close(self):
        if getattr(self, "h", None):
            _LIVE["comm_destroy"](self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def fora_batch_multi(graphs, srcs, k, eps, alpha, seed, n_rounds=0, conf=None):
    """pprhip_fora_batch: q queries over len(graphs) GPUs of this process; returns (ids[q, k], vals[q, k], n_sel[q], [Stats])."""
    srcs = np.ascontiguousarray(srcs, dtype=np.int32)
    q = int(srcs.size)
    g0 = graphs[0]
    conf = conf or conf_whole_graph(g0.n, g0.m, alpha)
    hs = (C.c_void_p * len(graphs))(*[g.h for g in graphs])
    ids = np.empty((q, k), dtype=np.int32)
    vals = np.empty((q, k))
    nsel = np.zeros(q, dtype=np.int32)
    sts = (Stats * len(graphs))()
    _check(lib().pprhip_fora_batch(hs, len(graphs), _ptr(srcs), q, k, eps, C.byref(conf), seed, n_rounds, _ptr(ids),
                                   _ptr(vals), _ptr(nsel), C.cast(sts, C.c_void_p)))
    return ids, vals, nsel, list(sts)


def all_pair_backward_multi(graphs, alpha, threshold, k):
    """pprhip_all_pair_backward_multi: the whole index over len(graphs) GPUs of this process; returns (Index, [Stats])."""
    hs = (C.c_void_p * len(graphs))(*[g.h for g in graphs])
    out = C.c_void_p()
    sts = (Stats * len(graphs))()
    _check(lib().pprhip_all_pair_backward_multi(hs, len(graphs), alpha, threshold, k, C.byref(out),
                                                C.cast(sts, C.c_void_p)))
    return Index(out), list(sts)


def _sparse_order(order):
    """"id" / "value" or the constants SPARSE_BY_ID / SPARSE_BY_VALUE; anything else goes to the library as it is."""
    return {"id": SPARSE_BY_ID, "value": SPARSE_BY_VALUE}.get(order, order)


def _sparse_call(threshold, order, cap, call):
    """One sparse getter: call(threshold, order, ids, vals, cap, count*) is the C entry point.  cap None: count first,
    then fetch everything.  Returns (ids int32, vals float64, count): min(cap, count) entries, count whatever cap is."""
    order = _sparse_order(order)
    cnt = C.c_uint64()
    counted = cap is None
    if counted:
        _check(call(threshold, order, None, None, 0, C.byref(cnt)))
        cap = cnt.value
    cap = int(cap)
    ids = np.empty(cap, dtype=np.int32)
    vals = np.empty(cap)
    if cap > 0:
        _check(call(threshold, order, _ptr(ids), _ptr(vals), cap, C.byref(cnt)))
    elif not counted:
        _check(call(threshold, order, None, None, 0, C.byref(cnt)))
    k = min(cap, cnt.value)
    return ids[:k], vals[:k], cnt.value


class Results:
    """Device-resident result vectors of a batched call (slot i = query i)."""

    def __init__(self, graph, capacity):
        self.n = graph.n
        self.graph = graph  # the store lives on the graph's device: keep the handle alive
        self.h = C.c_void_p()
        _check(lib().pprhip_results_create(graph.h, capacity, C.byref(self.h)))

    def info(self):
        cap, cnt, n = C.c_int(), C.c_int(), C.c_uint32()
        _check(lib().pprhip_results_info(self.h, C.byref(cap), C.byref(cnt), C.byref(n)))
        return cap.value, cnt.value, n.value

    def fetch(self, i):
        out = np.empty(self.n)
        _check(lib().pprhip_results_fetch(self.h, i, _ptr(out)))
        return out

    def fetch_sparse(self, i, threshold=0.0, order="id", cap=None):
        """Graph.reserve_sparse over vector i of the store (pprhip_results_fetch_sparse)."""
        return _sparse_call(threshold, order, cap, lambda t, o, ids, vals, k, cnt: lib().pprhip_results_fetch_sparse(
            self.h, int(i), t, o, ids, vals, k, cnt))

    def fetch_sparse_all(self, threshold=0.0, order="id", cap=None):
        """Every vector of the store in sparse form, as one CSR (pprhip_results_fetch_sparse_all).  Returns (offsets
        uint64[count + 1], ids, vals, total): row i is the entries [offsets[i], offsets[i + 1]) of vector i in the chosen
        order; the first min(cap, total) entries of the concatenated rows are returned (cap None: all of them)."""
        order = _sparse_order(order)
        offs = np.zeros(self.info()[1] + 1, dtype=np.uint64)
        tot = C.c_uint64()
        if cap is None:
            _check(lib().pprhip_results_fetch_sparse_all(self.h, threshold, order, _ptr(offs), None, None, 0, C.byref(tot)))
            cap = tot.value
        cap = int(cap)
        ids = np.empty(cap, dtype=np.int32)
        vals = np.empty(cap)
        _check(lib().pprhip_results_fetch_sparse_all(self.h, threshold, order, _ptr(offs), _ptr(ids) if cap else None,
                                                     _ptr(vals) if cap else None, cap, C.byref(tot)))
        k = min(cap, tot.value)
        return offs, ids[:k], vals[:k], tot.value

    def sweep_cut(self, i, normalize=True, max_size=0, max_vol=0, cap=None):
        """Graph.sweep_cut over vector i of the store (pprhip_results_sweep_cut)."""
        return _sweep_call(self.n, max_size, cap, lambda o, v, c, k, info: lib().pprhip_results_sweep_cut(
            self.h, int(i), int(bool(normalize)), int(max_size), int(max_vol), o, v, c, k, info))

    def weighted_sweep_cut(self, i, normalize=True, max_size=0, max_vol=0.0, cap=None):
        """Graph.weighted_sweep_cut over vector i of the store (pprhip_results_weighted_sweep_cut)."""
        return _sweep_call(self.n, max_size, cap, lambda o, v, c, k, info: lib().pprhip_results_weighted_sweep_cut(
            self.h, int(i), int(bool(normalize)), int(max_size), float(max_vol), o, v, c, k, info), WeightedSweep)

    def sum(self, i):
        s = C.c_double()
        _check(lib().pprhip_results_sum(self.h, i, C.byref(s)))
        return s.value

    def close(self):
        if getattr(self, "h", None):
            _LIVE["results_destroy"](self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class QueryStream:
    """pprhip_fora_stream_*: single-source FORA queries submitted in blocks and run by the batched driver without a
    drain between the blocks.  submit() returns a ticket; wait(ticket) returns (ids[q, k], vals[q, k], n_sel[q], Stats)."""

    def __init__(self, graph, eps, alpha, k=0, conf=None):
        self.graph = graph
        self.k = int(k)
        self.conf = conf or conf_whole_graph(graph.n, graph.m, alpha)
        self.h = C.c_void_p()
        self._out = {}
        _check(lib().pprhip_fora_stream_open(graph.h, eps, C.byref(self.conf), self.k, C.byref(self.h)))

    def submit(self, srcs, seed, keep=None, keep_first=0):
        srcs = np.ascontiguousarray(srcs, dtype=np.int32)
        q = int(srcs.size)
        ids = np.empty((q, self.k), dtype=np.int32) if self.k > 0 else None
        vals = np.empty((q, self.k)) if self.k > 0 else None
        nsel = np.zeros(q, dtype=np.int32) if self.k > 0 else None
        t = C.c_uint64()
        _check(lib().pprhip_fora_stream_submit(self.h, _ptr(srcs), q, seed, keep.h if keep is not None else None,
                                               int(keep_first), _ptr(ids), _ptr(vals), _ptr(nsel), C.byref(t)))
        self._out[t.value] = (ids, vals, nsel)  # (the library writes into these until the wait returns)
        return t.value

    def wait(self, ticket):
        st = Stats()
        _check(lib().pprhip_fora_stream_wait(self.h, ticket, C.byref(st)))
        ids, vals, nsel = self._out.pop(ticket)
        return ids, vals, nsel, st

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            # The close runs every submission that nobody waited for, and the driver writes their top-k blocks
            # into the arrays of _out: those must outlive the call (pprhip_jni.cpp: close_stream has the same order).
            try:
                _check(lib().pprhip_fora_stream_close(h))
            finally:
                self._out.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Graph:
    """Device-resident CSR pair + per-query workspace (one per GPU, one thread at a time)."""

    def __init__(self, host, device=0):
        self.n, self.m = host.n, host.m
        self.h = C.c_void_p()
        _check(lib().pprhip_graph_create(host.n, host.m, _ptr(host.out_rp), _ptr(host.out_ci), _ptr(host.in_rp),
                                         _ptr(host.in_ci), device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            _LIVE["graph_destroy"](self.h)
            self.h = None

    RELEASE_ALL_PAIR, RELEASE_BATCH, RELEASE_WALK_INDEX, RELEASE_SWEEP, RELEASE_SPARSE = 1, 2, 4, 8, 16
    RELEASE_WEIGHTS = 128
    RELEASE_WEIGHTED_WALK_INDEX = 256

    def release(self, what):
        """Hands the workspaces of the named entry points back (pprhip_graph_release); they come back on next use."""
        _check(lib().pprhip_graph_release(self.h, what))

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_memory(self):
        """(free, total) bytes of HBM on the handle's device."""
        f, t = C.c_uint64(), C.c_uint64()
        _check(lib().pprhip_device_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def set_tuning(self, t):
        _check(lib().pprhip_graph_set_tuning(self.h, C.byref(t)))

    def get_tuning(self):
        t = Tuning()
        _check(lib().pprhip_graph_get_tuning(self.h, C.byref(t)))
        return t

    def reserve(self):
        out = np.empty(self.n)
        _check(lib().pprhip_get_reserve(self.h, _ptr(out)))
        return out

    def residue(self):
        out = np.empty(self.n)
        _check(lib().pprhip_get_residue(self.h, _ptr(out)))
        return out

    def reserve_sparse(self, threshold=0.0, order="id", cap=None):
        """The entries of reserve() with value > threshold, compacted on the device (pprhip_get_reserve_sparse).  order
        "id": id ascending; "value": value descending, ties by id ascending.  Returns (ids int32, vals float64, count):
        the first min(cap, count) entries of that order (cap None: all of them; 0: the count alone); the values are the
        bits reserve() returns."""
        return _sparse_call(threshold, order, cap, lambda t, o, ids, vals, k, cnt: lib().pprhip_get_reserve_sparse(
            self.h, t, o, ids, vals, k, cnt))

    def residue_sparse(self, threshold=0.0, order="id", cap=None):
        """reserve_sparse over the vector residue() returns (pprhip_get_residue_sparse)."""
        return _sparse_call(threshold, order, cap, lambda t, o, ids, vals, k, cnt: lib().pprhip_get_residue_sparse(
            self.h, t, o, ids, vals, k, cnt))

    def sweep_cut(self, normalize=True, max_size=0, max_vol=0, cap=None):
        """The sweep cut over the result vector in HBM (what reserve() returns; pprhip_sweep_cut): the support ordered by
        x(v) / deg(v) (normalize False: by x(v)), ties by id, and the prefix of least conductance.  Returns (order, vol,
        cut, Sweep): the first `cap` positions of the order (node ids) with the volume and the cut of every prefix
        (cap None: everything profiled; 0: the Sweep alone).  max_size / max_vol > 0 bound the prefixes considered."""
        return _sweep_call(self.n, max_size, cap, lambda o, v, c, k, info: lib().pprhip_sweep_cut(
            self.h, int(bool(normalize)), int(max_size), int(max_vol), o, v, c, k, info))

    def local_cluster(self, seeds, alpha, rmax, weights=None, normalize=True, max_size=0, max_vol=0, cap=None):
        """PageRank-Nibble (pprhip_local_cluster_seeds): forward_push_seeds(seeds, alpha, rmax, weights) left in HBM,
        then sweep_cut.  Returns (members, Sweep, Stats): the nodes of the best prefix, at most `cap` of them."""
        s, w = _seed_arrays(seeds, weights)
        room = self.n if not max_size else min(self.n, int(max_size))
        cap = room if cap is None else min(int(cap), room)
        members = np.empty(cap, dtype=np.int32) if cap else None
        info, st = Sweep(), Stats()
        _check(lib().pprhip_local_cluster_seeds(self.h, _ptr(s), _ptr(w), s.size, alpha, rmax, int(bool(normalize)),
                                                int(max_size), int(max_vol), _ptr(members), cap, C.byref(info),
                                                C.byref(st)))
        k = min(cap, info.best_size)
        return (members[:k].copy() if cap else np.zeros(0, dtype=np.int32)), info, st

    # ---- the forward single-query calls, weighted and unweighted: one helper per return shape.  call: the C function;
    # start: the arguments that name where the query starts - (src,) or _seed_start(seeds, weights)
    def _push_call(self, call, start, alpha, rmax, fetch):
        """(reserve | None, residue | None, rsum, Stats)"""
        reserve = np.empty(self.n) if fetch else None
        residue = np.empty(self.n) if fetch else None
        rsum, st = C.c_double(), Stats()
        _check(call(self.h, *self._start(start), alpha, rmax, _ptr(reserve), _ptr(residue), C.byref(rsum), C.byref(st)))
        return reserve, residue, rsum.value, st

    def _fora_call(self, call, start, eps, alpha, seed, knob, conf, fetch):
        """(estimate | None, Stats); knob: n_rounds of the unweighted calls, rmax of the weighted ones"""
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out = np.empty(self.n) if fetch else None
        st = Stats()
        _check(call(self.h, *self._start(start), eps, C.byref(conf), seed, knob, _ptr(out), C.byref(st)))
        return out, st

    def _topk_call(self, call, start, eps, alpha, k, seed, cap, conf, fetch):
        """(nsel, ids, vals, estimate | None, Stats)"""
        conf = conf or conf_topk(self.n, self.m, k, alpha)
        cap = cap if cap is not None else k
        ids = np.empty(max(cap, 1), dtype=np.int32)
        vals = np.empty(max(cap, 1))
        nsel, st = C.c_int(0), Stats()
        out = np.empty(self.n) if fetch else None
        _check(call(self.h, *self._start(start), eps, C.byref(conf), seed, _ptr(ids), _ptr(vals), cap, C.byref(nsel),
                    _ptr(out), C.byref(st)))
        w = min(nsel.value, cap)
        return nsel.value, ids[:w].copy(), vals[:w].copy(), out, st

    def _walk_call(self, call, starts, idx, alpha, seed, stream, no_zero_hop):
        """(terminals, steps)"""
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        term = np.empty(starts.size, dtype=np.int32)
        steps = np.empty(starts.size, dtype=np.uint32)
        _check(call(self.h, _ptr(starts), _ptr(idx), starts.size, alpha, seed, stream, int(no_zero_hop), _ptr(term),
                    _ptr(steps)))
        return term, steps

    @staticmethod
    def _start(start):
        return [_ptr(a) if a is None or isinstance(a, np.ndarray) else a for a in start]

    def forward_push(self, src, alpha, rmax, fetch=True):
        return self._push_call(lib().pprhip_forward_push, (src,), alpha, rmax, fetch)

    def topk_push_reset(self, src, alpha):
        _check(lib().pprhip_fwdpush_topk_reset(self.h, src, alpha))

    def topk_push_round(self, min_rmax, rmax):
        rsum, st = C.c_double(), Stats()
        _check(lib().pprhip_fwdpush_topk_round(self.h, min_rmax, rmax, C.byref(rsum), C.byref(st)))
        return rsum.value, st

    def random_walks(self, starts, idx, alpha, seed, stream=0, no_zero_hop=False):
        return self._walk_call(lib().pprhip_random_walk_batch, starts, idx, alpha, seed, stream, no_zero_hop)

    def build_walk_index(self, alpha, seed, density=None, eps=0.5, conf=None, _weighted=False):
        """Builds the FORA+ walk index of (alpha, seed) on the handle (pprhip_walk_index_build): ceil(d_out(v) * density)
        stored walk terminals per node, which every whole-graph FORA call at that alpha and seed then reads instead of
        walking.  density None: the density at rmax0 of eps and conf (walk_index_density).  Returns the build's Stats."""
        if density is None:
            density = walk_index_density(conf or conf_whole_graph(self.n, self.m, alpha), eps)
        st = Stats()
        build = lib().pprhip_weighted_walk_index_build if _weighted else lib().pprhip_walk_index_build
        _check(build(self.h, alpha, seed, density, C.byref(st)))
        return st

    def drop_walk_index(self):
        _check(lib().pprhip_walk_index_drop(self.h))

    def walk_index_info(self, _weighted=False):
        """None without an index, else dict(alpha, seed, density, terminals, bytes)."""
        present, a, s, d = C.c_int(), C.c_double(), C.c_uint64(), C.c_double()
        t, b = C.c_uint64(), C.c_uint64()
        info = lib().pprhip_weighted_walk_index_info if _weighted else lib().pprhip_walk_index_info
        _check(info(self.h, C.byref(present), C.byref(a), C.byref(s), C.byref(d), C.byref(t), C.byref(b)))
        if not present.value:
            return None
        return dict(alpha=a.value, seed=s.value, density=d.value, terminals=t.value, bytes=b.value)

    def walk_index_terminals(self, node, _weighted=False):
        """The stored terminals of one node (original ids), in walk-index order."""
        cnt = C.c_uint64()
        fetch = lib().pprhip_weighted_walk_index_fetch if _weighted else lib().pprhip_walk_index_fetch
        _check(fetch(self.h, node, None, 0, C.byref(cnt)))
        out = np.empty(cnt.value, dtype=np.int32)
        if cnt.value:
            _check(fetch(self.h, node, _ptr(out), cnt.value, C.byref(cnt)))
        return out

    def walk_index_usage(self, reset=False, _weighted=False):
        """(served, walked): walks of whole-graph FORA phases read from the index / walked live in those phases, since
        the build or the last reset."""
        s, w = C.c_uint64(), C.c_uint64()
        usage = lib().pprhip_weighted_walk_index_usage if _weighted else lib().pprhip_walk_index_usage
        _check(usage(self.h, C.byref(s), C.byref(w), int(bool(reset))))
        return s.value, w.value

    def fora_single_source(self, src, eps, alpha, seed, n_rounds=0, conf=None, fetch=True):
        return self._fora_call(lib().pprhip_fora_single_source, (src,), eps, alpha, seed, n_rounds, conf, fetch)

    def forward_push_seeds(self, seeds, alpha, rmax, weights=None, fetch=True):
        """forward_push personalized to a seed set (weights None: uniform); the same return shape."""
        return self._push_call(lib().pprhip_forward_push_seeds, _seed_start(seeds, weights), alpha, rmax, fetch)

    def fora_seeds(self, seeds, eps, alpha, seed, weights=None, n_rounds=0, conf=None, fetch=True):
        """fora_single_source personalized to a seed set (weights None: uniform); the same return shape."""
        return self._fora_call(lib().pprhip_fora_seeds, _seed_start(seeds, weights), eps, alpha, seed, n_rounds, conf,
                               fetch)

    def fora_topk_seeds(self, seeds, eps, alpha, k, seed, weights=None, cap=None, conf=None, fetch=False):
        """fora_topk personalized to a seed set (weights None: uniform); the same return shape."""
        return self._topk_call(lib().pprhip_fora_topk_seeds, _seed_start(seeds, weights), eps, alpha, k, seed, cap, conf,
                               fetch)

    def fora_topk(self, src, eps, alpha, k, seed, cap=None, conf=None, fetch=False):
        return self._topk_call(lib().pprhip_fora_topk, (src,), eps, alpha, k, seed, cap, conf, fetch)

    def topk_select(self, k, cap=None):
        cap = cap if cap is not None else k
        ids = np.empty(max(cap, 1), dtype=np.int32)
        vals = np.empty(max(cap, 1))
        nsel, kth, st = C.c_int(0), C.c_double(0.0), Stats()
        _check(lib().pprhip_topk_select(self.h, k, _ptr(ids), _ptr(vals), cap, C.byref(nsel), C.byref(kth),
                                        C.byref(st)))
        w = min(nsel.value, cap)
        return nsel.value, ids[:w].copy(), vals[:w].copy(), kth.value, st

    def monte_carlo(self, src, eps, alpha, seed, conf=None):
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out = np.empty(self.n)
        st = Stats()
        _check(lib().pprhip_monte_carlo(self.h, src, eps, C.byref(conf), seed, _ptr(out), C.byref(st)))
        return out, st

    def fora_batch_single_source(self, srcs, eps, alpha, seed, n_rounds=0, k=0, conf=None, fetch=False, per_query=False,
                                 keep=None, out=None):
        """q single-source FORA queries, BATCH of them in flight; returns (reserve[q, n] | None, ids[q, k] | None,
        vals[q, k] | None, n_sel[q] | None, per-query Stats list | None, summed Stats).  keep: a Results store that
        receives every query's vector (device-resident); out: caller's [q, n] float64 array for fetch=True."""
        srcs = np.ascontiguousarray(srcs, dtype=np.int32)
        q = int(srcs.size)
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out, ids, vals, nsel, pq = _batch_outputs(q, self.n, k, fetch, out, per_query)
        st = Stats()
        _check(lib().pprhip_fora_batch_single_source_resident(
            self.h, _ptr(srcs), q, eps, C.byref(conf), seed, n_rounds, keep.h if keep is not None else None, _ptr(out),
            k, _ptr(ids), _ptr(vals), _ptr(nsel), C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return out, ids, vals, nsel, (list(pq) if pq is not None else None), st

    def fora_batch_seeds(self, sets, eps, alpha, seed, weights=None, n_rounds=0, k=0, conf=None, fetch=False,
                         per_query=False, keep=None, out=None):
        """fora_batch_single_source over seed sets: query i is fora_seeds(sets[i], ..., weights[i]); the same return
        tuple.  sets: a sequence of array-likes of node ids; weights: None or one entry per set (None: uniform)."""
        s, w, offsets = _seed_set_arrays(sets, weights)
        q = int(offsets.size - 1)
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out, ids, vals, nsel, pq = _batch_outputs(q, self.n, k, fetch, out, per_query)
        st = Stats()
        _check(lib().pprhip_fora_batch_seeds(
            self.h, _ptr(s), _ptr(w), _ptr(offsets), q, eps, C.byref(conf), seed, n_rounds,
            keep.h if keep is not None else None, _ptr(out), k, _ptr(ids), _ptr(vals), _ptr(nsel),
            C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return out, ids, vals, nsel, (list(pq) if pq is not None else None), st

    def fora_batch_topk_seeds(self, sets, k, eps, alpha, seed, weights=None):
        """fora_batch_topk over seed sets: query i is fora_topk_seeds(sets[i], ..., seed + i); returns (ids, vals,
        summed Stats)."""
        s, w, offsets = _seed_set_arrays(sets, weights)
        q = int(offsets.size - 1)
        ids = np.empty((q, k), dtype=np.int32)
        vals = np.empty((q, k))
        st = Stats()
        _check(lib().pprhip_fora_batch_topk_seeds(self.h, _ptr(s), _ptr(w), _ptr(offsets), q, k, eps, alpha, seed,
                                                  _ptr(ids), _ptr(vals), C.byref(st)))
        return ids, vals, st

    def fora_batch_topk(self, srcs, k, eps, alpha, seed):
        srcs = np.ascontiguousarray(srcs, dtype=np.int32)
        ids = np.empty((srcs.size, k), dtype=np.int32)
        vals = np.empty((srcs.size, k))
        st = Stats()
        _check(lib().pprhip_fora_batch_topk(self.h, _ptr(srcs), srcs.size, k, eps, alpha, seed, _ptr(ids), _ptr(vals),
                                            C.byref(st)))
        return ids, vals, st

    def walk_survival(self, alpha):
        """S of the leaking walk at alpha (pprhip_walk_survival), n doubles by node id."""
        out = np.empty(self.n)
        _check(lib().pprhip_walk_survival(self.h, alpha, _ptr(out)))
        return out

    def ppr_pairs(self, sources, targets, eps, alpha, seed, rmax=0.0, conf=None, _weighted=False):
        """pi(sources[i], targets[i]) for every i by the bidirectional estimator (pprhip_ppr_pairs); conf defaults to
        conf_whole_graph(n, m, alpha) (its alpha is the one used).  Returns (values, summed Stats)."""
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        s = np.ascontiguousarray(np.atleast_1d(sources), dtype=np.int32).ravel()
        t = np.ascontiguousarray(np.atleast_1d(targets), dtype=np.int32).ravel()
        if s.size != t.size:
            raise ValueError("%d sources for %d targets" % (s.size, t.size))
        out = np.empty(s.size)
        st = Stats()
        fn = lib().pprhip_weighted_ppr_pairs if _weighted else lib().pprhip_ppr_pairs
        _check(fn(self.h, _ptr(s), _ptr(t), s.size, eps, C.byref(conf), rmax, seed, _ptr(out), C.byref(st)))
        return out, st

    def _ppr_targets(self, t, w, offsets, q, alpha, rmax, k, keep, fetch, weighted=False):
        values, ids, vals, nsel, pq = _batch_outputs(q, self.n, k, fetch, None, True)  # (always per-query stats)
        st = Stats()
        fn = lib().pprhip_weighted_ppr_targets if weighted else lib().pprhip_ppr_targets
        _check(fn(
            self.h, _ptr(t), _ptr(w), _ptr(offsets), q, alpha, rmax, keep.h if keep is not None else None, _ptr(values),
            k, _ptr(ids), _ptr(vals), _ptr(nsel), C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return values, ((ids, vals, nsel) if k > 0 else None), st, (list(pq) if pq is not None else [])

    def ppr_targets(self, targets, alpha, rmax, k=0, keep=None, fetch=True):
        """Single-target PPR (pprhip_ppr_targets): for every target t the vector value(s) <= pi(s, t) <= value(s) + rmax
        over all sources s.  Returns (values[q, n] | None, (ids[q, k], vals[q, k], n_sel[q]) | None, summed Stats,
        per-query Stats list).  keep: a Results store that receives every target's vector (device-resident)."""
        t = np.ascontiguousarray(np.atleast_1d(targets), dtype=np.int32).ravel()
        return self._ppr_targets(t, None, None, int(t.size), alpha, rmax, k, keep, fetch)

    def ppr_target_sets(self, sets, alpha, rmax, weights=None, k=0, keep=None, fetch=True):
        """ppr_targets over weighted target sets: query i is pi(s, sets[i]) = sum_t w_t pi(s, t), the weights NOT
        normalized (None: 1 each, the probability that the walk from s ends in the set).  sets: a sequence of array-likes
        of node ids; weights: None or one entry per set (None: ones).  The same return tuple."""
        t, w, offsets = _seed_set_arrays(sets, weights)
        return self._ppr_targets(t, w, offsets, int(offsets.size - 1), alpha, rmax, k, keep, fetch)

    def backward_push(self, target, alpha, rmax):
        reserve = np.empty(self.n)
        residue = np.empty(self.n)
        st = Stats()
        _check(lib().pprhip_backward_push(self.h, target, alpha, rmax, _ptr(reserve), _ptr(residue), C.byref(st)))
        return reserve, residue, st

    def all_pair_backward(self, alpha, threshold, k, t_begin=0, t_end=None):
        t_end = self.n if t_end is None else t_end
        out, st = C.c_void_p(), Stats()
        _check(lib().pprhip_all_pair_backward(self.h, alpha, threshold, k, t_begin, t_end, C.byref(out), C.byref(st)))
        return Index(out), st

    def power_method(self, src, alpha, iters=100):
        out = np.empty(self.n)
        st = Stats()
        _check(lib().pprhip_power_method(self.h, src, alpha, iters, _ptr(out), C.byref(st)))
        return out, st

    # ---- weighted relationships (include/pprhip.h "weighted relationships"): P(u, v) = w(u -> v) / W(u)
    def set_weights(self, weights):
        """Relationship weights on the handle (pprhip_graph_set_weights): m doubles aligned with the host's out_ci
        (out_edge_order aligns an edge list's), every one finite and > 0; None drops them.  Only the weighted_* calls
        read them."""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if w.size != self.m:
                raise ValueError("weights: %d entries for %d relationships" % (w.size, self.m))
        _check(lib().pprhip_graph_set_weights(self.h, _ptr(w)))

    def weights_info(self):
        """(present, bytes of HBM the weights hold)."""
        p, b = C.c_int(), C.c_uint64()
        _check(lib().pprhip_weights_info(self.h, C.byref(p), C.byref(b)))
        return bool(p.value), b.value

    def weighted_power_method(self, src, alpha, iters=100):
        out = np.empty(self.n)
        st = Stats()
        _check(lib().pprhip_weighted_power_method(self.h, src, alpha, iters, _ptr(out), C.byref(st)))
        return out, st

    def weighted_forward_push(self, src, alpha, rmax, fetch=True):
        """forward_push over the weighted transition matrix; the same return shape."""
        return self._push_call(lib().pprhip_weighted_forward_push, (src,), alpha, rmax, fetch)

    def weighted_random_walks(self, starts, idx, alpha, seed, stream=0, no_zero_hop=False):
        """random_walks with the weighted neighbour pick; the same return shape."""
        return self._walk_call(lib().pprhip_weighted_random_walk_batch, starts, idx, alpha, seed, stream, no_zero_hop)

    def weighted_fora(self, src, eps, alpha, seed, rmax=0.0, conf=None, fetch=True):
        """One weighted push at rmax (0: rmax0 of conf and eps), then the whole-graph FORA walk phase with weighted
        walks (pprhip_weighted_fora).  Returns (estimate | None, Stats)."""
        return self._fora_call(lib().pprhip_weighted_fora, (src,), eps, alpha, seed, rmax, conf, fetch)

    # ---- weighted seed sets and top-k: the return shapes of the unweighted / weighted namesakes
    def build_weighted_walk_index(self, alpha, seed, density=None, eps=0.5, conf=None):
        """build_walk_index over the weighted walks (pprhip_weighted_walk_index_build): weighted_fora and
        weighted_fora_seeds at that alpha and seed then read the stored terminals instead of walking.  It lives beside
        the unweighted index and goes with the weights (set_weights, RELEASE_WEIGHTS)."""
        return self.build_walk_index(alpha, seed, density, eps, conf, _weighted=True)

    def drop_weighted_walk_index(self):
        _check(lib().pprhip_weighted_walk_index_drop(self.h))

    def weighted_walk_index_info(self):
        """walk_index_info of the weighted walk index."""
        return self.walk_index_info(_weighted=True)

    def weighted_walk_index_terminals(self, node):
        """walk_index_terminals of the weighted walk index."""
        return self.walk_index_terminals(node, _weighted=True)

    def weighted_walk_index_usage(self, reset=False):
        """(served, walked) of the weighted whole-graph FORA phases that used the weighted walk index."""
        return self.walk_index_usage(reset, _weighted=True)

    def weighted_forward_push_seeds(self, seeds, alpha, rmax, weights=None, fetch=True):
        """forward_push_seeds over the weighted transition matrix (`weights`: the seeds' weights, None: uniform)."""
        return self._push_call(lib().pprhip_weighted_forward_push_seeds, _seed_start(seeds, weights), alpha, rmax, fetch)

    def weighted_fora_seeds(self, seeds, eps, alpha, seed, weights=None, rmax=0.0, conf=None, fetch=True):
        """weighted_fora personalized to a seed set (`weights`: the seeds' weights, None: uniform)."""
        return self._fora_call(lib().pprhip_weighted_fora_seeds, _seed_start(seeds, weights), eps, alpha, seed, rmax, conf,
                               fetch)

    def weighted_fora_topk(self, src, eps, alpha, k, seed, cap=None, conf=None, fetch=False):
        """fora_topk over the weighted transition matrix, in plain rounds; the same return shape."""
        return self._topk_call(lib().pprhip_weighted_fora_topk, (src,), eps, alpha, k, seed, cap, conf, fetch)

    def weighted_fora_topk_seeds(self, seeds, eps, alpha, k, seed, weights=None, cap=None, conf=None, fetch=False):
        """weighted_fora_topk personalized to a seed set; the return shape of fora_topk_seeds."""
        return self._topk_call(lib().pprhip_weighted_fora_topk_seeds, _seed_start(seeds, weights), eps, alpha, k, seed,
                               cap, conf, fetch)

    # ---- batched weighted FORA: the return tuple of fora_batch_single_source
    def weighted_fora_batch(self, srcs, eps, alpha, seed, rmax=0.0, k=0, conf=None, fetch=False, per_query=False,
                            keep=None, out=None):
        """q weighted_fora queries in one call, BATCH of them in flight, their dense levels in one shared sweep
        (pprhip_weighted_fora_batch): query i is weighted_fora(srcs[i], eps, alpha, seed, rmax).  Returns what
        fora_batch_single_source returns."""
        srcs = np.ascontiguousarray(srcs, dtype=np.int32)
        q = int(srcs.size)
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out, ids, vals, nsel, pq = _batch_outputs(q, self.n, k, fetch, out, per_query)
        st = Stats()
        _check(lib().pprhip_weighted_fora_batch(
            self.h, _ptr(srcs), q, eps, C.byref(conf), seed, rmax, keep.h if keep is not None else None, _ptr(out), k,
            _ptr(ids), _ptr(vals), _ptr(nsel), C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return out, ids, vals, nsel, (list(pq) if pq is not None else None), st

    def weighted_fora_batch_seeds(self, sets, eps, alpha, seed, weights=None, rmax=0.0, k=0, conf=None, fetch=False,
                                  per_query=False, keep=None, out=None):
        """weighted_fora_batch over seed sets: query i is weighted_fora_seeds(sets[i], ..., weights[i]); sets and weights
        as fora_batch_seeds takes them; the same return tuple."""
        s, w, offsets = _seed_set_arrays(sets, weights)
        q = int(offsets.size - 1)
        conf = conf or conf_whole_graph(self.n, self.m, alpha)
        out, ids, vals, nsel, pq = _batch_outputs(q, self.n, k, fetch, out, per_query)
        st = Stats()
        _check(lib().pprhip_weighted_fora_batch_seeds(
            self.h, _ptr(s), _ptr(w), _ptr(offsets), q, eps, C.byref(conf), seed, rmax,
            keep.h if keep is not None else None, _ptr(out), k, _ptr(ids), _ptr(vals), _ptr(nsel),
            C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return out, ids, vals, nsel, (list(pq) if pq is not None else None), st

    # ---- batched weighted top-k: query i is weighted_fora_topk(srcs[i], ..., seed + i)
    def _weighted_batch_topk(self, call, head, q, k, eps, alpha, seed, conf, per_query, keep):
        conf = conf or conf_topk(self.n, self.m, k, alpha)
        if conf.k != k:
            raise ValueError("conf.k = %d, k = %d" % (conf.k, k))
        ids = np.empty((q, k), dtype=np.int32)
        vals = np.empty((q, k))
        nsel = np.zeros(q, dtype=np.int32)
        pq = (Stats * q)() if per_query and q else None
        st = Stats()
        _check(call(self.h, *head, q, eps, C.byref(conf), seed, keep.h if keep is not None else None, _ptr(ids),
                    _ptr(vals), _ptr(nsel), C.cast(pq, C.c_void_p) if pq is not None else None, C.byref(st)))
        return (ids, vals, nsel, st) + ((list(pq) if pq is not None else [],) if per_query else ())

    def weighted_fora_batch_topk(self, srcs, k, eps, alpha, seed, conf=None, per_query=False, keep=None):
        """q weighted_fora_topk queries in one call, BATCH of them in flight: their dense levels in one shared sweep,
        the walk phases that are ready in one launch (pprhip_weighted_fora_batch_topk).  Query i is
        weighted_fora_topk(srcs[i], eps, alpha, k, seed + i); conf defaults to conf_topk(n, m, k, alpha); keep: a Results
        store that receives the estimate vectors.  Returns (ids[q, k], vals[q, k], n_out[q], summed Stats[, per-query
        Stats])."""
        srcs = np.ascontiguousarray(srcs, dtype=np.int32).ravel()
        return self._weighted_batch_topk(lib().pprhip_weighted_fora_batch_topk, (_ptr(srcs),), int(srcs.size), k, eps,
                                         alpha, seed, conf, per_query, keep)

    def weighted_fora_batch_topk_seeds(self, sets, k, eps, alpha, seed, weights=None, conf=None, per_query=False,
                                       keep=None):
        """weighted_fora_batch_topk over seed sets: query i is weighted_fora_topk_seeds(sets[i], ..., seed + i,
        weights[i]); sets and weights as fora_batch_seeds takes them; the same return tuple."""
        s, w, offsets = _seed_set_arrays(sets, weights)
        return self._weighted_batch_topk(lib().pprhip_weighted_fora_batch_topk_seeds, (_ptr(s), _ptr(w), _ptr(offsets)),
                                         int(offsets.size - 1), k, eps, alpha, seed, conf, per_query, keep)

    # ---- weighted local clustering: the sweep cut by relationship weight, in quanta (include/pprhip.h)
    def weighted_sweep_cut(self, normalize=True, max_size=0, max_vol=0.0, cap=None):
        """sweep_cut by relationship weight (pprhip_weighted_sweep_cut): the support ordered by x(v) / qdeg(v)
        (normalize False: by x(v)), ties by id, and the prefix of least weighted conductance.  Returns (order, vol_q,
        cut_q, WeightedSweep): volume and cut of every prefix in quanta (uint64), one weight unit being 2**shift quanta.
        max_vol: a bound in weight units (0: none); max_size and cap as in sweep_cut."""
        return _sweep_call(self.n, max_size, cap, lambda o, v, c, k, info: lib().pprhip_weighted_sweep_cut(
            self.h, int(bool(normalize)), int(max_size), float(max_vol), o, v, c, k, info), WeightedSweep)

    def weighted_local_cluster(self, seeds, alpha, rmax, weights=None, normalize=True, max_size=0, max_vol=0.0,
                               cap=None):
        """PageRank-Nibble on the weighted graph (pprhip_weighted_local_cluster_seeds): weighted_forward_push_seeds(seeds,
        alpha, rmax, weights) left in HBM, then weighted_sweep_cut.  Returns (members, WeightedSweep, Stats)."""
        s, w = _seed_arrays(seeds, weights)
        room = self.n if not max_size else min(self.n, int(max_size))
        cap = room if cap is None else min(int(cap), room)
        members = np.empty(cap, dtype=np.int32) if cap else None
        info, st = WeightedSweep(), Stats()
        _check(lib().pprhip_weighted_local_cluster_seeds(self.h, _ptr(s), _ptr(w), s.size, alpha, rmax,
                                                         int(bool(normalize)), int(max_size), float(max_vol),
                                                         _ptr(members), cap, C.byref(info), C.byref(st)))
        k = min(cap, info.best_size)
        return (members[:k].copy() if cap else np.zeros(0, dtype=np.int32)), info, st

    # ---- the backward direction over the weights: the unweighted namesakes' arguments and return shapes
    def weighted_backward_push(self, target, alpha, rmax):
        """backward_push over the weighted transition matrix (pprhip_weighted_backward_push)."""
        reserve = np.empty(self.n)
        residue = np.empty(self.n)
        st = Stats()
        _check(lib().pprhip_weighted_backward_push(self.h, target, alpha, rmax, _ptr(reserve), _ptr(residue),
                                                   C.byref(st)))
        return reserve, residue, st

    def weighted_all_pair_backward(self, alpha, threshold, k, t_begin=0, t_end=None):
        """all_pair_backward over the weighted transition matrix (pprhip_weighted_all_pair_backward): (Index, Stats)."""
        t_end = self.n if t_end is None else t_end
        out, st = C.c_void_p(), Stats()
        _check(lib().pprhip_weighted_all_pair_backward(self.h, alpha, threshold, k, t_begin, t_end, C.byref(out),
                                                       C.byref(st)))
        return Index(out), st

    def weighted_walk_survival(self, alpha):
        """S_w of the leaking walk over the weighted P at alpha (pprhip_weighted_walk_survival), n doubles by node id."""
        out = np.empty(self.n)
        _check(lib().pprhip_weighted_walk_survival(self.h, alpha, _ptr(out)))
        return out

    def weighted_ppr_targets(self, targets, alpha, rmax, k=0, keep=None, fetch=True):
        """ppr_targets over the weighted P (pprhip_weighted_ppr_targets); the same return tuple."""
        t = np.ascontiguousarray(np.atleast_1d(targets), dtype=np.int32).ravel()
        return self._ppr_targets(t, None, None, int(t.size), alpha, rmax, k, keep, fetch, weighted=True)

    def weighted_ppr_target_sets(self, sets, alpha, rmax, weights=None, k=0, keep=None, fetch=True):
        """ppr_target_sets over the weighted P; the same return tuple."""
        t, w, offsets = _seed_set_arrays(sets, weights)
        return self._ppr_targets(t, w, offsets, int(offsets.size - 1), alpha, rmax, k, keep, fetch, weighted=True)

    def weighted_ppr_pairs(self, sources, targets, eps, alpha, seed, rmax=0.0, conf=None):
        """ppr_pairs over the weighted P with weighted walks (pprhip_weighted_ppr_pairs); (values, summed Stats)."""
        return self.ppr_pairs(sources, targets, eps, alpha, seed, rmax, conf, _weighted=True)
