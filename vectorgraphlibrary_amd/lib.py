"""ctypes binding of libvgl_hip.so (the C ABI declared in include/vgl_hip.h).

There is no CPU fallback: if the shared object is missing or no HIP device is visible the
package raises.  Build the library with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C vectorgraphlibrary_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvgl_hip.so")


class VglHipError(RuntimeError):
    pass


class BfsStats(C.Structure):
    _fields_ = [("levels", C.c_int32), ("td_steps", C.c_int32), ("bu_steps", C.c_int32),
                ("edges_examined", C.c_int64), ("frontier_total", C.c_int64), ("discovered", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("td_edges", C.c_int64), ("td_frontier", C.c_int64),
                ("bu_edges", C.c_int64), ("bu_found", C.c_int64)]


class SsspStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("edges_relaxed", C.c_int64), ("algorithmic_bytes", C.c_int64),
                ("push_steps", C.c_int32), ("pull_steps", C.c_int32)]


class PrStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("ranks_sum", C.c_double), ("algorithmic_bytes", C.c_int64)]


class SccStats(C.Structure):
    _fields_ = [("trim_rounds", C.c_int32), ("forward_backward_steps", C.c_int32), ("colour_rounds", C.c_int32), ("edge_passes", C.c_int32)]


class CcStats(C.Structure):
    _fields_ = [("hook_passes", C.c_int32), ("algorithmic_bytes", C.c_int64)]


class LpStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("frontier_steps", C.c_int32), ("changed_last", C.c_int64),
                ("rows_processed", C.c_int64), ("edges_examined", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class TriStats(C.Structure):
    _fields_ = [("triangles", C.c_int64), ("undirected_edges", C.c_int64), ("intersections", C.c_int64), ("elements_examined", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("max_oriented_degree", C.c_int32), ("prepared_now", C.c_int32), ("rows_light", C.c_int64),
                ("rows_table", C.c_int64), ("rows_huge", C.c_int64)]


class MsbfsStats(C.Structure):
    _fields_ = [("sources", C.c_int32), ("batches", C.c_int32), ("max_depth", C.c_int32), ("prepared_now", C.c_int32),
                ("levels_push", C.c_int32), ("levels_pull", C.c_int32), ("levels_total", C.c_int64), ("reached_total", C.c_int64),
                ("edges_push", C.c_int64), ("edges_pull", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class BcStats(C.Structure):
    _fields_ = [("sources", C.c_int32), ("max_depth", C.c_int32), ("sigma_inexact", C.c_int32), ("prepared_now", C.c_int32),
                ("levels_total", C.c_int64), ("reached_total", C.c_int64), ("edges_forward", C.c_int64), ("edges_backward", C.c_int64),
                ("algorithmic_bytes", C.c_int64)]


class KcoreStats(C.Structure):
    _fields_ = [("degeneracy", C.c_int32), ("rounds", C.c_int32), ("max_degree", C.c_int32), ("prepared_now", C.c_int32),
                ("sub_rounds", C.c_int64), ("undirected_edges", C.c_int64), ("edges_examined", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class KtrussStats(C.Structure):
    _fields_ = [("max_truss", C.c_int32), ("rounds", C.c_int32), ("max_support", C.c_int32), ("prepared_now", C.c_int32),
                ("sub_rounds", C.c_int64), ("undirected_edges", C.c_int64), ("triangles", C.c_int64), ("support_elements", C.c_int64),
                ("peel_elements", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class MsfStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("prepared_now", C.c_int32), ("forest_edges", C.c_int64), ("components", C.c_int64),
                ("undirected_edges", C.c_int64), ("entries_walked", C.c_int64), ("algorithmic_bytes", C.c_int64), ("total_weight", C.c_double)]


class BiccStats(C.Structure):
    _fields_ = [("depth", C.c_int32), ("prepared_now", C.c_int32), ("undirected_edges", C.c_int64), ("components", C.c_int64),
                ("bridges", C.c_int64), ("articulation_points", C.c_int64), ("biconnected_components", C.c_int64),
                ("two_edge_components", C.c_int64), ("largest_component_edges", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class MisStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("prepared_now", C.c_int32), ("set_size", C.c_int64), ("live_total", C.c_int64),
                ("entries_walked", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class MatchingStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("prepared_now", C.c_int32), ("matched_edges", C.c_int64), ("matched_vertices", C.c_int64),
                ("undirected_edges", C.c_int64), ("live_total", C.c_int64), ("entries_walked", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class SimPairsStats(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("pairs_short", C.c_int64), ("pairs_wave", C.c_int64), ("pairs_wg", C.c_int64),
                ("elements_examined", C.c_int64), ("common_total", C.c_int64), ("algorithmic_bytes", C.c_int64), ("prepared_now", C.c_int32)]


class SimTopkStats(C.Structure):
    _fields_ = [("queries", C.c_int64), ("rows_small", C.c_int64), ("rows_table", C.c_int64), ("rows_global", C.c_int64),
                ("two_paths_walked", C.c_int64), ("candidates_total", C.c_int64), ("filled", C.c_int64), ("scratch_slots", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("prepared_now", C.c_int32)]


class SubgraphStats(C.Structure):
    _fields_ = [("vertices_kept", C.c_int64), ("rows_short_out", C.c_int64), ("rows_wave_out", C.c_int64), ("rows_wg_out", C.c_int64),
                ("rows_short_in", C.c_int64), ("rows_wave_in", C.c_int64), ("rows_wg_in", C.c_int64), ("entries_read_out", C.c_int64),
                ("entries_read_in", C.c_int64), ("entries_kept_out", C.c_int64), ("entries_kept_in", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class QuotientStats(C.Structure):
    _fields_ = [("vertices", C.c_int64), ("rows_short_out", C.c_int64), ("rows_wave_out", C.c_int64), ("rows_table_out", C.c_int64),
                ("rows_sorted_out", C.c_int64), ("rows_short_in", C.c_int64), ("rows_wave_in", C.c_int64), ("rows_table_in", C.c_int64),
                ("rows_sorted_in", C.c_int64), ("entries_read_out", C.c_int64), ("entries_read_in", C.c_int64), ("entries_out", C.c_int64),
                ("entries_in", C.c_int64), ("sorted_keys_out", C.c_int64), ("sorted_keys_in", C.c_int64), ("sort_pieces_out", C.c_int64),
                ("sort_pieces_in", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class LouvainStats(C.Structure):
    _fields_ = [("levels", C.c_int32), ("prepared_now", C.c_int32), ("total_weight", C.c_int64), ("modularity_num", C.c_int64),
                ("entries_walked", C.c_int64), ("algorithmic_bytes", C.c_int64), ("rows_short", C.c_int64), ("rows_wave", C.c_int64),
                ("rows_wg", C.c_int64), ("rows_sorted", C.c_int64), ("sorted_keys", C.c_int64), ("sort_pieces", C.c_int64),
                ("vertices", C.c_int64 * 32), ("entries", C.c_int64 * 32), ("communities", C.c_int64 * 32),
                ("level_modularity_num", C.c_int64 * 32), ("rounds", C.c_int32 * 32), ("outcome", C.c_int32 * 32)]


class PprStats(C.Structure):
    _fields_ = [("sources", C.c_int32), ("batches", C.c_int32), ("iterations_max", C.c_int32), ("batches_converged", C.c_int32),
                ("prepared_now", C.c_int32), ("iterations_total", C.c_int64), ("entries_walked", C.c_int64), ("algorithmic_bytes", C.c_int64),
                ("max_err", C.c_double)]


class AggStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("entries", C.c_int64), ("rows_short", C.c_int64), ("rows_wave", C.c_int64), ("rows_wg", C.c_int64),
                ("chunks", C.c_int64), ("hub_rows", C.c_int64), ("algorithmic_bytes", C.c_int64), ("column_tiles", C.c_int32 * 3), ("vec", C.c_int32),
                ("transposed", C.c_int32), ("heads", C.c_int32)]


class KhopStats(C.Structure):
    _fields_ = [("reached", C.c_int64), ("frontier_total", C.c_int64), ("edges_examined", C.c_int64), ("levels_run", C.c_int32)]


class SampleStats(C.Structure):
    _fields_ = [("seeds", C.c_int64), ("rows_short", C.c_int64), ("rows_wave", C.c_int64), ("rows_wg", C.c_int64),
                ("entries_examined", C.c_int64), ("sampled_total", C.c_int64), ("algorithmic_bytes", C.c_int64)]


class ExchangeStats(C.Structure):
    _fields_ = [("collectives", C.c_int64), ("bytes_received", C.c_int64), ("list_steps", C.c_int32), ("dense_steps", C.c_int32),
                ("sparse_levels", C.c_int32), ("exchanges", C.c_int32)]


_lib = None

_p, _i32, _i64, _u64, _int, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_int, C.c_double
_pp = C.POINTER(C.c_void_p)

# name -> (argtypes)  ; every entry returns int status unless listed in _SPECIAL
_SIGNATURES = {
    "vgl_hip_ctx_create": [_int, _p, _pp],
    "vgl_hip_ctx_destroy": [_p],
    "vgl_hip_ctx_sync": [_p],
    "vgl_hip_ctx_trim": [_p],
    "vgl_hip_malloc": [_p, C.c_size_t, _pp],
    "vgl_hip_free": [_p, _p],
    "vgl_hip_memcpy_h2d": [_p, _p, _p, C.c_size_t],
    "vgl_hip_memcpy_d2h": [_p, _p, _p, C.c_size_t],
    "vgl_hip_memset": [_p, _p, _int, C.c_size_t],
    "vgl_hip_gen_rmat": [_p, _int, _i64, _i64, _u64, _int, _int, _int, _int, _int, _p, _p],
    "vgl_hip_gen_uniform": [_p, _int, _i64, _i64, _u64, _p, _p],
    "vgl_hip_gen_weights": [_p, _i64, _i64, _u64, _p],
    "vgl_hip_coo_to_csr": [_p, _i32, _i64, _p, _p, _i32, _i32, _p, _p, _p, C.POINTER(_i64)],
    "vgl_hip_gather_u32": [_p, _i64, _p, _p, _p],
    "vgl_hip_degree_order": [_p, _i32, _i64, _p, _p, _int, _p, _p],
    "vgl_hip_degree_hist_add": [_p, _i64, _p, _p, _int, _p],
    "vgl_hip_degree_order_from_degrees": [_p, _i32, _p, _p, _p],
    "vgl_hip_relabel_i32": [_p, _i64, _p, _p, _p],
    "vgl_hip_permute_u32": [_p, _i64, _p, _p, _p],
    "vgl_hip_cc_labels_to_original": [_p, _i32, _p, _p, _p, _p, _p],
    "vgl_hip_partition_rows": [_p, _i32, _p, _int, C.POINTER(_i32)],
    "vgl_hip_graph_create": [_p, _i32, _i32, _i32, _p, _p, _i64, _p, _p, _i64, _pp],
    "vgl_hip_graph_destroy": [_p, _p],
    "vgl_hip_graph_info": [_p, C.POINTER(_i32), C.POINTER(_int), C.POINTER(_i32)],
    "vgl_hip_frontier_create": [_p, _p, _pp],
    "vgl_hip_frontier_destroy": [_p, _p],
    "vgl_hip_frontier_create_on": [_p, _p, _p, _p, _pp],
    "vgl_hip_frontier_set_state": [_p, _p, _p, _i32, _i64, _int],
    "vgl_hip_frontier_set_all_active": [_p, _p],
    "vgl_hip_frontier_clear": [_p, _p],
    "vgl_hip_frontier_add_vertex": [_p, _p, _i32],
    "vgl_hip_frontier_info": [_p, _p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_int)],
    "vgl_hip_gnf_from_flags": [_p, _p, _p, _dbl, _p],
    "vgl_hip_gnf_equal_i32": [_p, _p, _p, _i32, _dbl, _p],
    "vgl_hip_graph_tile_rows": [_p, _int, _pp, C.POINTER(_i64)],
    "vgl_hip_frontier_advance_plan": [_p, _p, _p, _int, _pp, _pp, C.POINTER(_i64)],
    "vgl_hip_reduce_sum_f64_buffer": [_p, _i64, _p, C.POINTER(_dbl)],
    "vgl_hip_gnf_begin": [_p, _p, _p, _int, _p],
    "vgl_hip_gnf_complete": [_p, _p, _p, _dbl, _int, _i64],
    "vgl_hip_reduce_sum_i32": [_p, _p, _p, C.POINTER(_i64)],
    "vgl_hip_reduce_sum_f32": [_p, _p, _p, C.POINTER(_dbl)],
    "vgl_hip_count_not_equal_u32": [_p, _i32, _p, _p, C.POINTER(_i64)],
    "vgl_hip_bfs_run": [_p, _p, _i32, _int, _p, C.POINTER(BfsStats)],
    "vgl_hip_bfs_run_batch": [_p, _p, C.POINTER(_i32), _i32, _int, _p, C.POINTER(BfsStats)],
    "vgl_hip_bfs_prepare_blocked": [_p, _p],
    "vgl_hip_sssp_run": [_p, _p, _p, _i32, _int, _p, C.POINTER(SsspStats)],
    "vgl_hip_sswp_run": [_p, _p, _p, _i32, _int, _p, C.POINTER(SsspStats)],
    "vgl_hip_sssp_run_delta": [_p, _p, _p, _i32, C.c_float, _p, C.POINTER(SsspStats)],
    "vgl_hip_sssp_pull_plan_create": [_p, _p, _p, _pp],
    "vgl_hip_sssp_pull_plan_destroy": [_p, _p],
    "vgl_hip_sssp_pull_pass": [_p, _p, _p, _p, C.POINTER(_int)],
    "vgl_hip_sssp_pull_plan_info": [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_sssp_run_pull": [_p, _p, _p, _p, _i32, _int, _p, C.POINTER(SsspStats)],
    "vgl_hip_sswp_run_pull": [_p, _p, _p, _p, _i32, _int, _p, C.POINTER(SsspStats)],
    "vgl_hip_sssp_plan_create": [_p, _p, _p, C.c_float, _pp],
    "vgl_hip_sssp_plan_destroy": [_p, _p],
    "vgl_hip_sssp_run_plan": [_p, _p, _p, _i32, _p, C.POINTER(SsspStats)],
    "vgl_hip_pr_run": [_p, _p, _p, _int, _p, C.POINTER(PrStats)],
    "vgl_hip_pr_run_mode": [_p, _p, _p, _int, _int, _p, C.POINTER(PrStats)],
    "vgl_hip_pr_prepare": [_p, _p, _int, C.POINTER(_int)],
    "vgl_hip_cc_prepare": [_p, _p],
    "vgl_hip_hits_run": [_p, _p, _int, _p, _p],
    "vgl_hip_scc_run": [_p, _p, _p, C.POINTER(SccStats)],
    "vgl_hip_cc_run": [_p, _p, _p, C.POINTER(CcStats)],
    "vgl_hip_cc_run_symmetric": [_p, _p, _p, C.POINTER(CcStats)],
    "vgl_hip_lp_prepare": [_p, _p, _int],
    "vgl_hip_lp_run": [_p, _p, _int, _int, _int, _int, _p, _p, C.POINTER(_i64), C.POINTER(LpStats)],
    "vgl_hip_tri_prepare": [_p, _p],
    "vgl_hip_tri_run": [_p, _p, C.POINTER(_i64), _p, _p, C.POINTER(TriStats)],
    "vgl_hip_bc_prepare": [_p, _p, _int],
    "vgl_hip_bc_run": [_p, _p, C.POINTER(_i32), _i32, _int, _int, _p, _p, _p, _p, C.POINTER(BcStats)],
    "vgl_hip_msbfs_prepare": [_p, _p, _int, _int],
    "vgl_hip_msbfs_run": [_p, _p, C.POINTER(_i32), _i32, _int, _int, _p, _p, _p, _p, _p, C.POINTER(MsbfsStats)],
    "vgl_hip_kcore_prepare": [_p, _p],
    "vgl_hip_kcore_run": [_p, _p, _i32, _p, _p, C.POINTER(KcoreStats)],
    "vgl_hip_ktruss_prepare": [_p, _p, C.POINTER(_i64)],
    "vgl_hip_ktruss_run": [_p, _p, _i32, _p, _p, _p, _p, C.POINTER(KtrussStats)],
    "vgl_hip_msf_prepare": [_p, _p, C.POINTER(_i64)],
    "vgl_hip_msf_run": [_p, _p, _p, _p, _p, _p, _p, _p, C.POINTER(MsfStats)],
    "vgl_hip_bicc_prepare": [_p, _p, C.POINTER(_i64)],
    "vgl_hip_bicc_run": [_p, _p, _p, _p, _p, _p, _p, _p, C.POINTER(BiccStats)],
    "vgl_hip_mis_prepare": [_p, _p],
    "vgl_hip_mis_run": [_p, _p, _p, C.c_uint32, _p, _p, C.POINTER(MisStats)],
    "vgl_hip_matching_prepare": [_p, _p, C.POINTER(_i64)],
    "vgl_hip_matching_run": [_p, _p, _p, C.c_uint32, _p, _p, _p, _p, _p, C.POINTER(MatchingStats)],
    "vgl_hip_sim_prepare": [_p, _p],
    "vgl_hip_sim_pairs": [_p, _p, _p, _p, _i64, _p, _p, _p, _p, C.POINTER(SimPairsStats)],
    "vgl_hip_sim_topk": [_p, _p, _p, _i32, _int, _i32, _int, _p, _p, _p, C.POINTER(SimTopkStats)],
    "vgl_hip_subgraph_plan_create": [_p, _p, _p, _p, _pp],
    "vgl_hip_subgraph_plan_info": [_p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(SubgraphStats)],
    "vgl_hip_subgraph_plan_vertex_maps": [_p, _p, _p, _p],
    "vgl_hip_subgraph_plan_fill": [_p, _p, _int, _p, _p, _p],
    "vgl_hip_subgraph_plan_destroy": [_p, _p],
    "vgl_hip_khop_run": [_p, _p, _p, _i64, _i32, _int, _int, _p, C.POINTER(KhopStats)],
    "vgl_hip_sample_neighbors": [_p, _p, _p, _i64, _i32, _int, C.c_uint32, _p, _p, _p, C.POINTER(SampleStats)],
    "vgl_hip_quotient_plan_create": [_p, _p, _p, _int, _pp],
    "vgl_hip_quotient_plan_info": [_p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(QuotientStats)],
    "vgl_hip_quotient_plan_vertex_maps": [_p, _p, _p, _p, _p],
    "vgl_hip_quotient_plan_members": [_p, _p, _p, _p],
    "vgl_hip_quotient_plan_fill": [_p, _p, _int, _p, _p, _p, _p],
    "vgl_hip_quotient_plan_destroy": [_p, _p],
    "vgl_hip_louvain_move": [_p, _p, _p, _i32, _i64, C.c_uint32, _p, C.POINTER(LouvainStats)],
    "vgl_hip_ppr_prepare": [_p, _p, _int],
    "vgl_hip_ppr_run": [_p, _p, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_dbl), _i32, _dbl, _i32, _dbl, _int, _p, _p, _p, C.POINTER(PprStats)],
    "vgl_hip_agg_plan_create": [_p, _p, _p, _i32, _i32, _pp],
    "vgl_hip_agg_plan_info": [_p, C.POINTER(AggStats)],
    "vgl_hip_agg_plan_destroy": [_p, _p],
    "vgl_hip_agg_run": [_p, _p, _int, _p, _p, _i64, _i32, _p, _i64, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_run_transposed": [_p, _p, _int, _p, _p, _p, _i64, _i32, _p, _i64, C.POINTER(AggStats)],
    "vgl_hip_agg_sddmm": [_p, _p, _p, _i64, _p, _i64, _i32, _int, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_softmax": [_p, _p, _p, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_softmax_backward": [_p, _p, _p, _p, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_sddmm_heads": [_p, _p, _p, _i64, _p, _i64, _i32, _i32, _int, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_softmax_heads": [_p, _p, _p, _i32, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_softmax_backward_heads": [_p, _p, _p, _p, _i32, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_run_heads": [_p, _p, _int, _p, _i32, _p, _i64, _i32, _p, _i64, C.POINTER(AggStats)],
    "vgl_hip_agg_run_transposed_heads": [_p, _p, _int, _p, _i32, _p, _i64, _i32, _p, _i64, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_add_heads": [_p, _p, _p, _i64, _p, _i64, _i32, C.c_float, _p, C.POINTER(AggStats)],
    "vgl_hip_agg_edge_sum_heads": [_p, _p, _p, _p, C.c_float, _i32, _int, _p, _i64, C.POINTER(AggStats)],
    "vgl_hip_bfs_init": [_p, _i32, _i32, _p],
    "vgl_hip_bfs_step_top_down": [_p, _p, _p, _i32, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_bfs_step_top_down_bits": [_p, _p, _p, _i32, _p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_bitmap_or_parts": [_p, _i64, _int, _p, _p],
    "vgl_hip_bfs_step_bottom_up": [_p, _p, _p, _i32, _p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_bfs_front_fold": [_p, _i64, _p, _p],
    "vgl_hip_levels_to_bitmap": [_p, _i32, _p, _i32, _p],
    "vgl_hip_bfs_apply_bitmaps": [_p, _i32, _int, _p, _p, _i32, _p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_bfs_apply_bitmaps_owned": [_p, _i32, _int, _p, _p, _i32, _p, _p, _p, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_bitmap_to_ids": [_p, _i64, _p, _i32, _p],
    "vgl_hip_bfs_apply_ids": [_p, _i32, _int, _i32, _p, _p, _i32, _p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "vgl_hip_sssp_init": [_p, _i32, _i32, _p],
    "vgl_hip_sssp_relax_owned": [_p, _p, _p, _p, C.POINTER(_int)],
    "vgl_hip_sswp_init": [_p, _i32, _i32, _p],
    "vgl_hip_sswp_relax_owned": [_p, _p, _p, _p, C.POINTER(_int)],
    "vgl_hip_cc_init": [_p, _i32, _p],
    "vgl_hip_cc_hook_owned": [_p, _p, _p, C.POINTER(_int)],
    "vgl_hip_cc_jump": [_p, _i32, _p],
    "vgl_hip_pr_setup": [_p, _i32, _p, _p, _p],
    "vgl_hip_sum_over_edges_f32": [_p, _p, _p, C.c_float, _p],
    "vgl_hip_sum_over_edges_check": [_p, C.POINTER(C.c_uint)],
    "vgl_hip_sssp_prepare": [_p, _p],
    "vgl_hip_comm_set_timeout_ms": [_p, C.c_double],
    "vgl_hip_pr_iteration_owned": [_p, _p, _p, _p, _p, _p],
    "vgl_hip_indegree_noloops_add": [_p, _p, _p],
    "vgl_hip_diff_to_pairs_u32": [_p, _i32, _p, _p, _i32, _p],
    "vgl_hip_apply_pairs_u32": [_p, _int, _i64, _int, _p, _int, _i32, _p, C.POINTER(_int)],
    "vgl_hip_comm_unique_id": [_p],
    "vgl_hip_comm_create": [_p, _int, _int, _p, _pp],
    "vgl_hip_comm_create_hosted": [_p, _int, _int, C.c_char_p, C.c_size_t, _pp],
    "vgl_hip_comm_create_peer": [_p, _int, _int, C.c_char_p, C.c_size_t, _pp],
    "vgl_hip_comm_abort": [_p],
    "vgl_hip_comm_destroy": [_p],
    "vgl_hip_comm_info": [_p, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)],
    "vgl_hip_comm_barrier": [_p],
    "vgl_hip_comm_stats": [_p, C.POINTER(ExchangeStats)],
    "vgl_hip_exchange_allreduce_min_i32": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_min_f32": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_max_f32": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_sum_i32": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_sum_i64": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_sum_f32": [_p, _p, _i64],
    "vgl_hip_exchange_allreduce_sum_f64": [_p, _p, _i64],
    "vgl_hip_exchange_allgather": [_p, _p, _p, _i64],
    "vgl_hip_exchange_allgather_slices": [_p, _p, C.POINTER(_i64), _int],
    "vgl_hip_exchange_bitmap_or": [_p, _p, _i64],
    "vgl_hip_exchange_changed_u32": [_p, _i32, _p, _p, _int, C.POINTER(_int)],
    "vgl_hip_bfs_run_sharded": [_p, _p, _p, _i32, _int, _i64, _int, _p, C.POINTER(BfsStats)],
    "vgl_hip_sssp_run_sharded": [_p, _p, _p, _p, _i32, _p, C.POINTER(SsspStats)],
    "vgl_hip_sswp_run_sharded": [_p, _p, _p, _p, _i32, _p, C.POINTER(SsspStats)],
    "vgl_hip_cc_run_sharded": [_p, _p, _p, _p, C.POINTER(CcStats)],
    "vgl_hip_pr_run_sharded": [_p, _p, _p, _int, _int, _p, C.POINTER(PrStats)],
    "vgl_hip_hits_run_sharded": [_p, _p, _p, _int, _p, _p],
    "vgl_hip_timing_enable": [_p, _int],
    "vgl_hip_timing_only": [_p, C.c_char_p],
    "vgl_hip_timing_reset": [_p],
    "vgl_hip_timing_stride": [_p, _int],
    "vgl_hip_timing_get": [_p, C.c_char_p, C.POINTER(_i64), C.POINTER(_dbl)],
}
_SPECIAL = {
    "vgl_hip_abi_version": (_int, []),
    "vgl_hip_last_error": (C.c_char_p, []),
    "vgl_hip_ctx_stream": (_p, [_p]),
    "vgl_hip_frontier_ids": (_p, [_p]),
    "vgl_hip_frontier_flags": (_p, [_p]),
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + list(_SPECIAL))


def load():
    """dlopen libvgl_hip.so and declare every entry point; raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VglHipError(
            f"{LIB_PATH} is missing: the MI355X backend has no CPU fallback. "
            "Build it with `make -C vectorgraphlibrary_amd/csrc` (hipcc, gfx950).")
    L = C.CDLL(LIB_PATH)
    for name, args in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = _int
        fn.argtypes = args
    for name, (res, args) in _SPECIAL.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status):
    if status != 0:
        raise VglHipError(load().vgl_hip_last_error().decode("utf-8", "replace"))
