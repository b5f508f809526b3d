"""ctypes binding of libmmf_hg.so (include/mmf_hg.h).  Fails loudly when the library is missing:
there is no CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MMF_HG_LIBRARY") or os.path.join(_HERE, "libmmf_hg.so")   # override: a library built elsewhere

MMF_OK, MMF_E_INVALID, MMF_E_UNSUPPORTED, MMF_E_HIP, MMF_E_NOMEM, MMF_E_INTERNAL = 0, -1, -2, -3, -4, -5
DOT, COSINE, NEG_SQ_L2, RBF, RBF_DIRECT = 0, 1, 2, 3, 4
METRICS = {"dot": DOT, "cosine": COSINE, "neg_sq_l2": NEG_SQ_L2, "rbf": RBF, "rbf_direct": RBF_DIRECT}
F32, BF16, F16 = 0, 1, 2
PRECISIONS = {"auto": 0, "exact": 1, "fast": 2, "fast_bf16": 3}
QUERY_ORDERS = {"auto": 0, "off": 1, "on": 2}
ABI_VERSION = 3          # MMF_ABI_VERSION of the include/mmf_hg.h this binding was written against


class SimtopkOpts(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int), ("profile", ctypes.c_int), ("col_splits", ctypes.c_int),
                ("query_order", ctypes.c_int), ("select_wait_event", ctypes.c_void_p)]


class PreparedSide(ctypes.Structure):
    _fields_ = [("Z", ctypes.c_void_p), ("scal", ctypes.c_void_p), ("zn", ctypes.c_void_p), ("rn", ctypes.c_void_p),
                ("un", ctypes.c_void_p), ("cb", ctypes.c_void_p)]


class Panel(ctypes.Structure):
    _fields_ = [("Z", ctypes.c_void_p), ("cb", ctypes.c_void_p), ("m", ctypes.c_int64), ("m_pad", ctypes.c_int64),
                ("seg_len", ctypes.c_int64), ("seg_stride", ctypes.c_int64), ("id_base", ctypes.c_int64),
                ("ready_event", ctypes.c_void_p)]


class SimtopkStats(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_float), ("prep_ms", ctypes.c_float), ("rerank_ms", ctypes.c_float),
                ("fallback_ms", ctypes.c_float), ("candidates", ctypes.c_int64), ("fallback_rows", ctypes.c_int64),
                ("precision_used", ctypes.c_int), ("col_splits", ctypes.c_int), ("scan_grid", ctypes.c_int),
                ("scan_wait_ms", ctypes.c_float), ("overflow_rows", ctypes.c_int64), ("short_rows", ctypes.c_int64),
                ("near_rows", ctypes.c_int64), ("order_ms", ctypes.c_float), ("query_order", ctypes.c_int)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if not f.startswith("reserved")}


_lib = None

EXPORTS = ["mmf_version", "mmf_last_error", "mmf_simtopk", "mmf_simtopk_ex", "mmf_row_scalars", "mmf_prep_rows",
           "mmf_simtopk_prepared", "mmf_simtopk_panels", "mmf_simtopk_segmented", "mmf_padded_dim", "mmf_fast_scan_supported", "mmf_topk_merge", "mmf_edge_cosine",
           "mmf_sim_dense", "mmf_sim_dense_stats", "mmf_sim_dense_combined", "mmf_offdiag_lower_median", "mmf_threshold_edges", "mmf_threshold_edges_count", "mmf_threshold_edges_fill", "mmf_lower_median", "mmf_array_stats",
           "mmf_segment_sort", "mmf_segment_mean", "mmf_segment_offdiag_mean", "mmf_clique_pairs", "mmf_knn_pairs", "mmf_kmeans_fit", "mmf_kmeans_fit_segmented", "mmf_combined_offdiag_median", "mmf_combined_threshold_edges",
           "mmf_sim_dense_combined_segmented", "mmf_offdiag_lower_median_segmented", "mmf_threshold_edges_segmented_count",
           "mmf_threshold_edges_segmented_fill", "mmf_knn_clique_edges_count", "mmf_knn_clique_edges_fill", "mmf_release_workspaces", "mmf_debug_query_order",
           "mmf_debug_symmetric_schedule"]

# The cohort entries (include/mmf_hg.h): additions to ABI version 3, bound like EXPORTS.  Their synchronisation
# behaviour is INTEGRATION.md's table "Cohort entries", pinned by tests/test_wsi_tma_segmented_cpu.py.
EXPORTS_COHORT = ["mmf_sim_dense_stats_segmented", "mmf_lower_median_segmented"]

# The pooling entries (include/mmf_hg_pool.h): additions to ABI version 3 declared in a header of their own, so
# that the two lists above stay exactly what include/mmf_hg.h declares.  Their synchronisation behaviour is INTEGRATION.md's table
# "Pooling entries", pinned by tests/test_super_patches_segmented_cpu.py.
EXPORTS_POOL = ["mmf_segment_sort_segmented", "mmf_super_patches_segmented"]

# The streaming entries (include/mmf_hg_stream.h): additions to ABI version 3 in a header of their own, like the
# pooling entries.  Their synchronisation behaviour is INTEGRATION.md's table "Streaming entries", pinned by
# tests/test_super_patch_stats_streamed_cpu.py.
EXPORTS_STREAM = ["mmf_super_patch_stats_streamed", "mmf_super_patch_stats_streamed_bytes"]

# The top-k entries (include/mmf_hg_topk.h): an addition to ABI version 3 in a header of its own, like the pooling
# entries.  Its synchronisation behaviour is INTEGRATION.md's table "Top-k entries", pinned by tests/test_simtopk_combined_cpu.py.
EXPORTS_TOPK = ["mmf_simtopk_combined"]

# The wide-scan queries (include/mmf_hg_wide.h): an addition to ABI version 3 in a header of its own.  Host-only:
# they take neither a device nor a stream.
EXPORTS_WIDE = ["mmf_wide_scan_supported", "mmf_wide_scan_list_capacity"]

# The segmented wide scan (include/mmf_hg_wide_seg.h): an addition to ABI version 3 in a header of its own.  Its
# synchronisation behaviour is INTEGRATION.md's table "Wide segmented entries", pinned by tests/test_wide_segmented_cpu.py.
EXPORTS_WIDE_SEG = ["mmf_simtopk_segmented_wide"]

# The 16-bit top-k of the combined similarity (include/mmf_hg_topk16.h): an addition to ABI version 3 in a header
# of its own.  Its synchronisation behaviour is INTEGRATION.md's table "16-bit top-k entries", pinned by
# tests/test_simtopk_combined_fast_cpu.py.
EXPORTS_TOPK16 = ["mmf_simtopk_combined_fast"]

# The segmented 16-bit top-k of the combined similarity (include/ext/mmf_hg_topk16_seg.h): an addition to ABI
# version 3 in a header of its own.  Its synchronisation behaviour is INTEGRATION.md's table "Segmented 16-bit top-k entries",
# pinned by tests/test_simtopk_combined_fast_segmented_cpu.py.
EXPORTS_TOPK16_SEG = ["mmf_simtopk_combined_fast_segmented"]

# The two-set top-k of the combined similarity (include/ext/mmf_hg_topk_xy.h): an addition to ABI version 3 in a
# header of its own.  Its synchronisation behaviour is INTEGRATION.md's table "Two-set top-k entries", pinned by
# tests/test_simtopk_combined_xy_cpu.py.
EXPORTS_TOPK_XY = ["mmf_simtopk_combined_xy"]

# The segmented exact scan (include/ext/mmf_hg_seg_exact.h): an addition to ABI version 3 in a header of its own.
# Both entries synchronise once per call (the re-rank's fail counts; once more when a segment is short of k admissible columns);
# mmf_segmented_exact_table is host-only.  Pinned by tests/test_segmented_exact_cpu.py.
EXPORTS_SEG_EXACT = ["mmf_simtopk_segmented_exact", "mmf_simtopk_combined_segmented_exact", "mmf_segmented_exact_table"]

# The ragged-width segmented KMeans (include/ext/mmf_hg_kmeans_ragged.h): an addition to ABI version 3 in a header
# of its own.  mmf_kmeans_fit_ragged synchronises once per Lloyd iteration, like mmf_kmeans_fit_segmented (INTEGRATION.md's table
# "Ragged KMeans entries"); mmf_kmeans_ragged_groups is host-only.  Pinned by tests/test_kmeans_ragged_cpu.py.
EXPORTS_KMEANS_RAGGED = ["mmf_kmeans_fit_ragged", "mmf_kmeans_ragged_groups"]

# The combined top-k for any k (include/ext/mmf_hg_topk_anyk.h): an addition to ABI version 3 in a header of its
# own.  Its synchronisation behaviour is INTEGRATION.md's table "Any-k top-k entries", pinned by
# tests/test_simtopk_combined_anyk_cpu.py.
EXPORTS_TOPK_ANYK = ["mmf_simtopk_combined_anyk", "mmf_simtopk_combined_xy_anyk"]

# The cross-segment top-k (include/ext/mmf_hg_cross_seg.h): an addition to ABI version 3 in a header of its own.
# mmf_simtopk_cross_segments synchronises once per call (the re-rank's fail counts); mmf_cross_segments_table is host-only.  Pinned
# by tests/test_cross_segments_cpu.py.  (The name does not begin with EXPORTS: tests/test_simtopk_combined_anyk_cpu.py pins the
# set of names that do.)
CROSS_SEG_EXPORTS = ["mmf_simtopk_cross_segments", "mmf_cross_segments_table"]

# The cross-segment top-k on the 16-bit scan (include/ext/mmf_hg_cross_seg16.h): an addition to ABI version 3 in a
# header of its own.  mmf_simtopk_cross_segments_fast synchronises once per call (the re-rank's fail counts; once more when rows
# were flagged for the exact rescan); mmf_cross_segments_fast_table is host-only.  Pinned by tests/test_cross_segments_fast_cpu.py.
CROSS_SEG16_EXPORTS = ["mmf_simtopk_cross_segments_fast", "mmf_cross_segments_fast_table"]

# The cross-segment top-k on the wide 16-bit scan (include/ext/mmf_hg_cross_segw.h): an addition to ABI version 3 in
# a header of its own.  mmf_simtopk_cross_segments_wide synchronises as its narrow twin does (once per call; once more when rows
# were flagged); mmf_cross_segments_wide_table is host-only.  Pinned by tests/test_cross_segments_wide_cpu.py.
CROSS_SEGW_EXPORTS = ["mmf_simtopk_cross_segments_wide", "mmf_cross_segments_wide_table"]

# The 16-bit top-k for any k (include/ext/mmf_hg_fast_anyk.h): an addition to ABI version 3 in a header of its own.
# mmf_simtopk_fast_anyk synchronises once per pass (fail counts and yield histogram together; once more in a pass that sends rows to
# the exact rescan); mmf_fast_anyk_plan is host-only.  Pinned by tests/test_fast_anyk_cpu.py.
FAST_ANYK_EXPORTS = ["mmf_simtopk_fast_anyk", "mmf_fast_anyk_plan"]
FAST_ANYK_MAX_PASSES = 16

# The wide 16-bit top-k for any k (include/ext/mmf_hg_wide_anyk.h): an addition to ABI version 3 in a header of its
# own; the twin of the two entries above for 1024 < d <= 4096 (same info struct, same synchronisation: once per pass, once more in a
# pass that sends rows to the exact rescan; mmf_wide_anyk_plan is host-only).  Pinned by tests/test_wide_anyk_cpu.py.
WIDE_ANYK_EXPORTS = ["mmf_simtopk_wide_anyk", "mmf_wide_anyk_plan"]

# The segmented 16-bit top-k for any k (include/ext/mmf_hg_seg_anyk.h): an addition to ABI version 3 in a header of
# its own; the cohort form of mmf_simtopk_fast_anyk for d <= 1024 (same info struct).  mmf_simtopk_segmented_fast_anyk synchronises
# once per pass (fail counts and yield histogram together) and once more in a pass that sends rows to the exact rescan (the rows are
# read and grouped per segment on the host); mmf_segmented_anyk_plan is host-only.  Pinned by tests/test_segmented_anyk_cpu.py.
SEG_ANYK_EXPORTS = ["mmf_simtopk_segmented_fast_anyk", "mmf_segmented_anyk_plan"]

# The 16-bit cross-segment top-k for any k (include/ext/mmf_hg_cross_seg_anyk.h): an addition to ABI version 3 in a
# header of its own; the cross-segment form of mmf_simtopk_fast_anyk for d <= 1024 (same info struct).
# mmf_simtopk_cross_segments_fast_anyk synchronises once per pass (fail counts and yield histogram together) and once more in a pass
# that sends rows to the exact rescan (the rows are read to the host, which builds the exact table over them);
# mmf_cross_segments_anyk_plan is host-only.  Pinned by tests/test_cross_segments_anyk_cpu.py.
CROSS_ANYK_EXPORTS = ["mmf_simtopk_cross_segments_fast_anyk", "mmf_cross_segments_anyk_plan"]

# The wide 16-bit cross-segment top-k for any k (include/ext/mmf_hg_cross_segw_anyk.h): an addition to ABI version 3
# in a header of its own; the twin of the two entries above for 1024 < d <= 4096 (same info struct, same synchronisation: once per
# pass, once more in a pass that sends rows to the exact rescan; mmf_cross_segments_wide_anyk_plan is host-only).  Pinned by
# tests/test_cross_segments_wide_anyk_cpu.py.
CROSS_WIDE_ANYK_EXPORTS = ["mmf_simtopk_cross_segments_wide_anyk", "mmf_cross_segments_wide_anyk_plan"]

# The segmented wide 16-bit top-k for any k (include/ext/mmf_hg_segw_anyk.h): an addition to ABI version 3 in a header
# of its own; the twin of SEG_ANYK_EXPORTS for 1024 < d <= 4096 (same arguments, same info struct, same synchronisation: once per pass,
# once more in a pass that sends rows to the exact rescan; mmf_segmented_wide_anyk_plan is host-only).  Pinned by
# tests/test_segmented_wide_anyk_cpu.py.
SEGW_ANYK_EXPORTS = ["mmf_simtopk_segmented_wide_anyk", "mmf_segmented_wide_anyk_plan"]

# The 16-bit combined top-k for any k (include/ext/mmf_hg_topk16_anyk.h): an addition to ABI version 3 in a header of
# its own; the arguments of mmf_simtopk_combined plus the info struct of FAST_ANYK_EXPORTS.  mmf_simtopk_combined_fast_anyk
# synchronises once per pass (fail counts and yield histogram together) and, in a pass that sends rows to the exact rescan, once
# more for the rows (read and grouped per segment on the host) and once for the rescan's fail count; mmf_combined_fast_anyk_plan is
# host-only.  Pinned by tests/test_simtopk_combined_fast_anyk_cpu.py.
TOPK16_ANYK_EXPORTS = ["mmf_simtopk_combined_fast_anyk", "mmf_combined_fast_anyk_plan"]

# The 16-bit combined top-k for two node sets and any k (include/ext/mmf_hg_topk16_xy_anyk.h): an addition to ABI
# version 3 in a header of its own; the arguments of mmf_simtopk_combined_xy plus the info struct of FAST_ANYK_EXPORTS.  It
# synchronises once per pass (fail counts and yield histogram together) and, in a pass that sends queries to the exact rescan, once
# more for their list and once for the rescan's fail count; mmf_combined_fast_anyk_plan answers for it too.  Pinned by
# tests/test_simtopk_combined_xy_fast_anyk_cpu.py.
TOPK16_XY_ANYK_EXPORTS = ["mmf_simtopk_combined_xy_fast_anyk"]

# Hypergraph propagation on the incidence (include/ext/mmf_hg_hgconv.h): an addition to ABI version 3 in a header of
# its own.  mmf_incidence_plan_bytes is host-only; the other three enqueue on the caller's stream and never synchronise (the plan's
# verdict on out-of-range ids is a device status word that the Python layer reads).  Pinned by tests/test_hgconv_cpu.py.
HGCONV_EXPORTS = ["mmf_incidence_plan_bytes", "mmf_incidence_plan", "mmf_csr_gather_sum", "mmf_hypergraph_propagate"]

# The attention readout over a ragged batch (include/ext/mmf_hg_readout.h): an addition to ABI version 3 in a header
# of its own.  mmf_attention_readout_table is host-only; the other two enqueue on the caller's stream and never synchronise.  Pinned
# by tests/test_readout_cpu.py.
READOUT_EXPORTS = ["mmf_attention_readout_table", "mmf_attention_readout", "mmf_attention_readout_backward"]

# Pair-weighted hypergraph propagation and the softmax over the pairs of a row (include/ext/mmf_hg_hgpair.h): an
# addition to ABI version 3 in a header of its own.  All six enqueue on the caller's stream and never synchronise.  Pinned by
# tests/test_hgpair_cpu.py.
HGPAIR_EXPORTS = ["mmf_incidence_pair_plan", "mmf_pair_scales", "mmf_hypergraph_propagate_pairs", "mmf_pair_weight_grad", "mmf_pair_softmax",
                  "mmf_pair_softmax_backward"]

# 16-bit activations for the hypergraph branch (include/ext/mmf_hg_hg16.h): f16 / bf16 x, f32 chains, one rounding
# per stored tensor.  An addition to ABI version 3 in a header of its own.  All five enqueue on the caller's stream and never
# synchronise.  Pinned by tests/test_hg16_cpu.py.
HG16_EXPORTS = ["mmf_csr_gather_sum_16", "mmf_hypergraph_propagate_16", "mmf_pair_weight_grad_16", "mmf_attention_readout_16",
                "mmf_attention_readout_backward_16"]


class FastAnykInfo(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int32), ("yield_", ctypes.c_int32 * FAST_ANYK_MAX_PASSES),
                ("ghost_max", ctypes.c_int32 * FAST_ANYK_MAX_PASSES), ("exact_rows", ctypes.c_int64 * FAST_ANYK_MAX_PASSES)]

    def as_dict(self):
        p = min(int(self.passes), FAST_ANYK_MAX_PASSES)
        return {"passes": int(self.passes), "yield": list(self.yield_[:p]), "ghost_max": list(self.ghost_max[:p]),
                "exact_rows": list(self.exact_rows[:p])}


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            "or python multimodal-fusion_amd/csrc/build.py).  This package has no CPU fallback.")
    L = ctypes.CDLL(SO_PATH)
    vp, i64, ci, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    L.mmf_version.restype = ci
    L.mmf_last_error.restype = ctypes.c_char_p
    L.mmf_simtopk.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, ci, i64, i64, vp, vp, ci, vp]
    L.mmf_simtopk_ex.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, ci, i64, i64, vp, vp,
                                 ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_padded_dim.argtypes = [i64]
    L.mmf_fast_scan_supported.argtypes = [i64, ci, ci]
    L.mmf_row_scalars.argtypes = [vp, i64, i64, ci, ci, vp, vp, ci, vp]
    L.mmf_prep_rows.argtypes = [vp, i64, i64, ci, ci, ci, vp, vp, vp, i64, vp, vp, vp, vp, vp, ci, vp]
    L.mmf_simtopk_prepared.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, ci, i64, i64,
                                       ctypes.POINTER(PreparedSide), ctypes.POINTER(PreparedSide), i64, vp, ci, vp, vp,
                                       ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_simtopk_panels.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, ci, i64, i64,
                                     ctypes.POINTER(PreparedSide), vp, ctypes.POINTER(Panel), ci, vp, ci, vp, vp,
                                     ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_simtopk_segmented.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, ci, vp, vp, i64, vp, vp,
                                        ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_topk_merge.argtypes = [vp, vp, vp, vp, i64, ci, vp, vp, ci, vp]
    L.mmf_edge_cosine.argtypes = [vp, i64, i64, ci, vp, i64, vp, ci, vp]
    L.mmf_sim_dense.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, vp, ci, vp]
    L.mmf_sim_dense_stats.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, vp, vp, i64, ci, vp]
    L.mmf_sim_dense_combined.argtypes = [vp, vp, i64, i64, i64, f32, f32, vp, ci, vp]
    L.mmf_offdiag_lower_median.argtypes = [vp, i64, vp, ci, vp]
    L.mmf_segment_sort.argtypes = [vp, i64, i64, vp, vp, vp, ci, vp]
    L.mmf_segment_mean.argtypes = [vp, i64, i64, vp, vp, i64, vp, ci, vp]
    L.mmf_segment_offdiag_mean.argtypes = [vp, i64, vp, vp, i64, vp, ci, vp]
    L.mmf_clique_pairs.argtypes = [vp, vp, i64, i64, vp, vp, i64, vp, ci, vp]
    L.mmf_knn_pairs.argtypes = [vp, i64, ci, vp, vp, vp, vp, ci, vp]
    L.mmf_kmeans_fit.argtypes = [vp, i64, i64, i64, i64, ci, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, ci, vp]
    L.mmf_kmeans_fit_segmented.argtypes = [vp, i64, i64, vp, i64, i64, i64, ci, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, ci, vp]
    L.mmf_lower_median.argtypes = [vp, i64, vp, ci, vp]
    L.mmf_array_stats.argtypes = [vp, i64, vp, ci, vp]
    L.mmf_threshold_edges.argtypes = [vp, i64, f32, vp, vp, i64, vp, ci, vp]
    L.mmf_threshold_edges_count.argtypes = [vp, i64, f32, vp, vp, ci, vp]
    L.mmf_threshold_edges_fill.argtypes = [vp, i64, f32, vp, vp, vp, i64, ci, vp]
    L.mmf_combined_offdiag_median.argtypes = [vp, vp, i64, i64, i64, f32, f32, i64, vp, ci, vp]
    L.mmf_combined_threshold_edges.argtypes = [vp, vp, i64, i64, i64, f32, f32, f32, i64, vp, vp, i64, vp, ci, vp]
    L.mmf_sim_dense_combined_segmented.argtypes = [vp, vp, i64, i64, i64, vp, i64, f32, f32, vp, ci, vp]
    L.mmf_offdiag_lower_median_segmented.argtypes = [vp, vp, i64, vp, ci, vp]
    L.mmf_threshold_edges_segmented_count.argtypes = [vp, vp, i64, vp, vp, vp, ci, vp]
    L.mmf_threshold_edges_segmented_fill.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, ci, vp]
    L.mmf_knn_clique_edges_count.argtypes = [vp, i64, ci, vp, i64, vp, i64, vp, vp, vp, ci, vp]
    L.mmf_knn_clique_edges_fill.argtypes = [vp, i64, ci, vp, i64, vp, i64, vp, vp, i64, ci, vp]
    L.mmf_sim_dense_stats_segmented.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, vp, vp, i64, vp, vp, ci, vp]
    L.mmf_lower_median_segmented.argtypes = [vp, vp, i64, vp, ci, vp]
    L.mmf_segment_sort_segmented.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, ci, vp]
    L.mmf_super_patches_segmented.argtypes = [vp, vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.mmf_super_patch_stats_streamed.argtypes = [vp, vp, i64, i64, i64, f32, f32, vp, vp, i64, i64, vp, vp, ci, vp]
    L.mmf_super_patch_stats_streamed_bytes.argtypes = [i64, i64, i64, i64, i64]
    L.mmf_simtopk_combined.argtypes = [vp, vp, i64, i64, i64, f32, f32, ci, ci, vp, i64, vp, vp,
                                       ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_wide_scan_supported.argtypes = [i64, ci, ci]
    L.mmf_wide_scan_list_capacity.argtypes = [ci, ci]
    L.mmf_simtopk_segmented_wide.argtypes = list(L.mmf_simtopk_segmented.argtypes)
    L.mmf_simtopk_combined_fast.argtypes = list(L.mmf_simtopk_combined.argtypes)
    L.mmf_simtopk_combined_fast_segmented.argtypes = list(L.mmf_simtopk_combined.argtypes)
    L.mmf_simtopk_combined_xy.argtypes = [vp, vp, i64, vp, vp, i64, i64, i64, f32, f32, ci, ci, i64, i64, vp, vp,
                                          ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_simtopk_segmented_exact.argtypes = list(L.mmf_simtopk_segmented.argtypes)
    L.mmf_simtopk_combined_segmented_exact.argtypes = list(L.mmf_simtopk_combined.argtypes)
    L.mmf_simtopk_segmented_exact.restype = L.mmf_simtopk_combined_segmented_exact.restype = ci
    L.mmf_segmented_exact_table.argtypes = [vp, vp, i64, ci, ci, ci, vp, i64, ctypes.POINTER(ci)]
    L.mmf_segmented_exact_table.restype = i64
    L.mmf_kmeans_fit_ragged.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, ci, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, ci, vp]
    L.mmf_kmeans_fit_ragged.restype = ci
    L.mmf_kmeans_ragged_groups.argtypes = [vp, vp, i64, i64, i64, ci, vp, vp]
    L.mmf_kmeans_ragged_groups.restype = i64
    L.mmf_simtopk_combined_anyk.argtypes = list(L.mmf_simtopk_combined.argtypes)
    L.mmf_simtopk_combined_xy_anyk.argtypes = list(L.mmf_simtopk_combined_xy.argtypes)
    L.mmf_simtopk_combined_anyk.restype = L.mmf_simtopk_combined_xy_anyk.restype = ci
    L.mmf_simtopk_cross_segments.argtypes = [vp, i64, vp, i64, i64, ci, ci, f32, ci, vp, vp, i64, vp, vp,
                                             ctypes.POINTER(SimtopkOpts), ctypes.POINTER(SimtopkStats), ci, vp]
    L.mmf_simtopk_cross_segments.restype = ci
    L.mmf_cross_segments_table.argtypes = [vp, vp, i64, ci, ci, vp, i64, ctypes.POINTER(ci)]
    L.mmf_cross_segments_table.restype = i64
    L.mmf_simtopk_cross_segments_fast.argtypes = list(L.mmf_simtopk_cross_segments.argtypes)
    L.mmf_simtopk_cross_segments_fast.restype = ci
    L.mmf_cross_segments_fast_table.argtypes = [vp, vp, i64, i64, ci, ci, vp, i64, ctypes.POINTER(ci)]
    L.mmf_cross_segments_fast_table.restype = i64
    L.mmf_simtopk_cross_segments_wide.argtypes = list(L.mmf_simtopk_cross_segments_fast.argtypes)
    L.mmf_simtopk_cross_segments_wide.restype = ci
    L.mmf_cross_segments_wide_table.argtypes = list(L.mmf_cross_segments_fast_table.argtypes)
    L.mmf_cross_segments_wide_table.restype = i64
    L.mmf_simtopk_fast_anyk.argtypes = list(L.mmf_simtopk_ex.argtypes) + [ctypes.POINTER(FastAnykInfo)]
    L.mmf_simtopk_fast_anyk.restype = ci
    L.mmf_fast_anyk_plan.argtypes = [i64, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.mmf_fast_anyk_plan.restype = ci
    L.mmf_simtopk_wide_anyk.argtypes = list(L.mmf_simtopk_fast_anyk.argtypes)
    L.mmf_simtopk_wide_anyk.restype = ci
    L.mmf_wide_anyk_plan.argtypes = list(L.mmf_fast_anyk_plan.argtypes)
    L.mmf_wide_anyk_plan.restype = ci
    L.mmf_simtopk_segmented_fast_anyk.argtypes = list(L.mmf_simtopk_segmented.argtypes) + [ctypes.POINTER(FastAnykInfo)]
    L.mmf_simtopk_segmented_fast_anyk.restype = ci
    L.mmf_segmented_anyk_plan.argtypes = list(L.mmf_fast_anyk_plan.argtypes)
    L.mmf_segmented_anyk_plan.restype = ci
    L.mmf_simtopk_cross_segments_fast_anyk.argtypes = list(L.mmf_simtopk_cross_segments_fast.argtypes) + [ctypes.POINTER(FastAnykInfo)]
    L.mmf_simtopk_cross_segments_fast_anyk.restype = ci
    L.mmf_cross_segments_anyk_plan.argtypes = [i64, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.mmf_cross_segments_anyk_plan.restype = ci
    L.mmf_simtopk_cross_segments_wide_anyk.argtypes = list(L.mmf_simtopk_cross_segments_fast_anyk.argtypes)
    L.mmf_simtopk_cross_segments_wide_anyk.restype = ci
    L.mmf_cross_segments_wide_anyk_plan.argtypes = list(L.mmf_cross_segments_anyk_plan.argtypes)
    L.mmf_cross_segments_wide_anyk_plan.restype = ci
    L.mmf_simtopk_segmented_wide_anyk.argtypes = list(L.mmf_simtopk_segmented_fast_anyk.argtypes)
    L.mmf_simtopk_segmented_wide_anyk.restype = ci
    L.mmf_segmented_wide_anyk_plan.argtypes = list(L.mmf_segmented_anyk_plan.argtypes)
    L.mmf_segmented_wide_anyk_plan.restype = ci
    L.mmf_simtopk_combined_fast_anyk.argtypes = list(L.mmf_simtopk_combined.argtypes) + [ctypes.POINTER(FastAnykInfo)]
    L.mmf_simtopk_combined_fast_anyk.restype = ci
    L.mmf_combined_fast_anyk_plan.argtypes = list(L.mmf_fast_anyk_plan.argtypes)
    L.mmf_combined_fast_anyk_plan.restype = ci
    L.mmf_simtopk_combined_xy_fast_anyk.argtypes = list(L.mmf_simtopk_combined_xy.argtypes) + [ctypes.POINTER(FastAnykInfo)]
    L.mmf_simtopk_combined_xy_fast_anyk.restype = ci
    L.mmf_incidence_plan_bytes.argtypes = [i64, i64, i64, vp]
    L.mmf_incidence_plan.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.mmf_csr_gather_sum.argtypes = [vp, vp, i64, vp, i64, i64, vp, vp, vp, i64, ci, vp]
    L.mmf_hypergraph_propagate.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, ci, ci, vp]
    for name in HGCONV_EXPORTS:
        getattr(L, name).restype = ci
    L.mmf_attention_readout_table.argtypes = [vp, i64, vp, i64]
    L.mmf_attention_readout_table.restype = i64
    L.mmf_attention_readout.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, ci, vp]
    L.mmf_attention_readout.restype = ci
    L.mmf_attention_readout_backward.argtypes = [vp, i64, vp, vp, vp, i64, vp, vp, i64, i64, i64, vp, vp, ci, vp]
    L.mmf_attention_readout_backward.restype = ci
    L.mmf_incidence_pair_plan.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.mmf_pair_scales.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, ci, vp]
    L.mmf_hypergraph_propagate_pairs.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i64, vp, vp, ci, ci, vp]
    L.mmf_pair_weight_grad.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, i64, i64, i64, i64, vp, ci, vp]
    L.mmf_pair_softmax.argtypes = [vp, vp, i64, i64, vp, vp, ci, vp]
    L.mmf_pair_softmax_backward.argtypes = [vp, vp, i64, i64, vp, vp, vp, ci, vp]
    for name in HGPAIR_EXPORTS:
        getattr(L, name).restype = ci
    L.mmf_csr_gather_sum_16.argtypes = [vp, vp, vp, vp, i64, vp, i64, i64, ci, vp, vp, vp, vp, vp, i64, ci, vp]
    L.mmf_hypergraph_propagate_16.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i64, ci, vp, vp, vp, ci, ci, vp]
    L.mmf_pair_weight_grad_16.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, i64, i64, i64, ci, vp, ci, vp]
    L.mmf_attention_readout_16.argtypes = [vp, i64, ci, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, ci, vp]
    L.mmf_attention_readout_backward_16.argtypes = [vp, i64, ci, vp, vp, vp, i64, vp, vp, i64, i64, i64, vp, vp, ci, vp]
    for name in HG16_EXPORTS:
        getattr(L, name).restype = ci
    for name in (EXPORTS + EXPORTS_COHORT + EXPORTS_POOL + EXPORTS_STREAM + EXPORTS_TOPK + EXPORTS_WIDE + EXPORTS_WIDE_SEG + EXPORTS_TOPK16 +
                 EXPORTS_TOPK16_SEG + EXPORTS_TOPK_XY):
        fn = getattr(L, name)
        if name not in ("mmf_last_error", "mmf_padded_dim", "mmf_super_patch_stats_streamed_bytes"):
            fn.restype = ci
    L.mmf_padded_dim.restype = i64
    L.mmf_super_patch_stats_streamed_bytes.restype = i64
    L.mmf_debug_symmetric_schedule.argtypes = [i64, ci, ci, vp, i64]
    L.mmf_debug_symmetric_schedule.restype = i64
    L.mmf_last_error.restype = ctypes.c_char_p
    if L.mmf_version() != ABI_VERSION:
        raise RuntimeError(f"{SO_PATH}: ABI version {L.mmf_version()}, this package binds version {ABI_VERSION} "
                           "(include/mmf_hg.h MMF_ABI_VERSION): rebuild the library")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc == MMF_OK:
        return
    msg = lib().mmf_last_error().decode("utf-8", "replace")
    if rc == MMF_E_INVALID:
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg} (code {rc})")
