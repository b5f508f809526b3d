"""multimodal-fusion_amd — MI355X-native hypergraph construction (similarity + per-row top-k).

The directory name carries a hyphen (it mirrors the reference repo's name), so import it through the
shim at the repo root:  ``import multimodal_fusion_amd as mmf``.

    mmf.ops.simtopk(...)                          fused similarity + top-k on gfx950
    mmf.ops.simtopk_segmented(..., ptr=/batch=)   the same per segment of a ragged batch (one graph per slide)
    mmf.ragged.*                                  host-side offsets, plans and size checks of a ragged batch, shared by every module below
    mmf.weighted_hypergraph.*                     the median-threshold weighted hypergraph of every graph of a batch
    mmf.knn_kmeans_hypergraph.*                   the k-NN + KMeans hypergraph of every slide of a cohort (ordered edges, one host read)
    mmf.wsi_tma_similarity.*                      WSI x TMA similarity + statistics, grouping and the median edge filter of every slide of a cohort
    mmf.super_patches.*                           super-patch aggregation of every slide of a cohort (sort, pooling, statistics; one host read per group)
    mmf.super_patch_stats.*                       the statistics of that step for a slide whose similarity matrix does not fit: K recomputed in row panels
    mmf.combined_topk.*                           the k best columns per row of K_h * K_g (features x positions) of one graph or a batch, K never stored
    mmf.combined_topk16.*                         the same top-k of K_h * K_g of one graph from the 16-bit matrix cores, bit for bit (f16 / bf16 scan, exact re-rank)
    mmf.combined_topk16_segmented.*               that 16-bit top-k for every graph of a ragged batch from one launch of the scan, bit for bit
    mmf.combined_topk_xy.*                        the top-k of K_h * K_g for two node sets (queries x candidates, id offsets), or rows [lo, hi) of one graph against all of it
    mmf.segmented_exact.*                         the exact f32 top-k of every segment of a batch from one table-driven scan launch (any k), and the router
    mmf.combined_topk_anyk.*                      the top-k of K_h * K_g for any k (one graph, a batch, two node sets, row panels): exact passes behind per-row floors
    mmf.cross_segments.*                          the exact top-k of every row among the rows of all OTHER segments (leave-one-slide-out k-NN, inter-slide edges)
    mmf.cross_segments16.*                        that top-k from the 16-bit matrix cores, bit for bit, and the router between the two
    mmf.cross_segments_wide.*                     that top-k from the wide 16-bit scan (feature dims 1025..4096), bit for bit, and the three-way router
    mmf.fast_anyk.*                               the 16-bit top-k for any k at feature dims <= 1024 (later passes scan under per-row ceilings), bit for bit, and the router
    mmf.segmented_anyk.*                          that any-k 16-bit top-k for every segment of a ragged batch (the cohort form), bit for bit, and the router
    mmf.cross_segments_anyk.*                     that any-k 16-bit top-k across segments (every row against all OTHER segments), bit for bit, and the router
    mmf.cross_segments_wide_anyk.*                that any-k top-k across segments from the wide 16-bit scan (feature dims 1025..4096), bit for bit, and the router
    mmf.segmented_wide_anyk.*                     that any-k top-k for every segment of a ragged batch from the wide 16-bit scan (feature dims 1025..4096), bit for bit, and the router
    mmf.combined_topk16_anyk.*                    the any-k top-k of K_h * K_g from the 16-bit scan of the combined key (one graph or a batch), bit for bit, and the router
    mmf.combined_topk16_xy_anyk.*                 that any-k 16-bit top-k of K_h * K_g for two node sets or rows [lo, hi) of one graph, bit for bit, and the routers
    mmf.hgconv.*                                  hypergraph propagation D^-1 H W B^-1 H^T x on an incidence (the reference model's HypergraphConv), bit-stable gather-sums over a reusable plan
    mmf.readout.*                                 the attention readout over a ragged batch (the reference model's GlobalAttention), bit-stable chains, and HypergraphNetwork on top
    mmf.hgpair.*                                  that propagation with one weight per (node, hyperedge) pair (the builders' edge_weights), the softmax over the pairs of a hyperedge or node, and the attention convolution on top
    mmf.hg16.*                                    those three for float16 / bfloat16 x (what torch.autocast hands a layer): 16-bit storage, float32 chains, one rounding per stored tensor
    mmf.kmeans_ragged.*                           scikit-learn's KMeans fit for every block of a flat buffer in one call, each block with a width of its own
    mmf.wide_scan.*                               what the wide 16-bit scan (feature dims 1025..4096) covers: host-only queries
    mmf.cohort.build_cohort_hypergraphs(...)      the four steps of process_single_file for every slide of a cohort, in memory
    mmf.build_hypergraph.*                        the reference's function names and signatures
    mmf.distributed.sharded_simtopk(...)          row-sharded multi-GPU driver (RCCL all-gather)
    mmf.distributed.sharded_simtopk_combined(...) the same driver for the top-k of K_h * K_g
    mmf.distributed.sharded_simtopk_combined_any_k(...) that driver for any k
    mmf.distributed.sharded_simtopk_combined_fast_any_k(...) that driver for any k on the 16-bit scan of the combined key
"""
from . import _lib, ops  # noqa: F401
from .ops import (edge_cosine, offdiag_lower_median, sim_dense, sim_dense_combined, sim_dense_combined_segmented,  # noqa: F401
                  simtopk, simtopk_segmented, threshold_edges, topk_merge)
from .knn_kmeans_hypergraph import build_hypergraph_knn_kmeans_segmented, knn_kmeans_edges_segmented  # noqa: F401
from .wsi_tma_similarity import (compute_wsi_tma_similarity_segmented, filter_edges_by_median_segmented,  # noqa: F401
                                 group_by_similarity_segmented, lower_median_segmented, sim_dense_stats_segmented, similarity_block)
from . import cohort, super_patch_stats, super_patches  # noqa: F401,E402
from .cohort import build_cohort_hypergraphs  # noqa: F401,E402
from .super_patches import (aggregate_wsi_super_patches_segmented, pool_super_patches_segmented,  # noqa: F401,E402
                            segment_sort_segmented)

from . import combined_topk  # noqa: F401,E402
from .combined_topk import build_topk_hypergraph_data, build_topk_weighted_hypergraph, simtopk_combined  # noqa: F401,E402

from . import combined_topk16  # noqa: F401,E402
from .combined_topk16 import build_topk_weighted_hypergraph_fast, simtopk_combined_fast  # noqa: F401,E402

from . import combined_topk16_segmented  # noqa: F401,E402
from .combined_topk16_segmented import (build_topk_hypergraph_data_fast, build_topk_weighted_hypergraph_fast_segmented,  # noqa: F401,E402
                                        simtopk_combined_fast_segmented)

from . import combined_topk_xy  # noqa: F401,E402
from .combined_topk_xy import simtopk_combined_rows, simtopk_combined_xy  # noqa: F401,E402

from . import segmented_exact  # noqa: F401,E402
from .segmented_exact import segmented_exact_table, simtopk_combined_exact, simtopk_segmented_exact  # noqa: F401,E402

from . import kmeans_ragged  # noqa: F401,E402
from .kmeans_ragged import kmeans_fit_predict_ragged, kmeans_fit_ragged, ragged_groups  # noqa: F401,E402

from . import combined_topk_anyk  # noqa: F401,E402
from .combined_topk_anyk import (anyk_route, build_topk_hypergraph_data_any_k, build_topk_weighted_hypergraph_any_k,  # noqa: F401,E402
                                 simtopk_combined_any_k, simtopk_combined_rows_any_k, simtopk_combined_xy_any_k)

from . import cross_segments  # noqa: F401,E402
from .cross_segments import cross_segment_knn_edges, cross_segments_table, simtopk_cross_segments  # noqa: F401,E402

from . import cross_segments16  # noqa: F401,E402
from .cross_segments16 import cross_segments_fast_table, simtopk_cross_segments_fast  # noqa: F401,E402

from . import cross_segments_wide  # noqa: F401,E402
from .cross_segments_wide import cross_segments_route, cross_segments_wide_table, simtopk_cross_segments_wide  # noqa: F401,E402

from . import fast_anyk  # noqa: F401,E402
from .fast_anyk import fast_anyk_plan, simtopk_fast_any_k  # noqa: F401,E402

from . import wide_anyk  # noqa: F401,E402
from .wide_anyk import simtopk_wide_any_k, wide_anyk_plan  # noqa: F401,E402

from . import segmented_anyk  # noqa: F401,E402
from .segmented_anyk import segmented_anyk_plan, simtopk_segmented_fast_any_k  # noqa: F401,E402

from . import cross_segments_anyk  # noqa: F401,E402
from .cross_segments_anyk import cross_segments_anyk_plan, simtopk_cross_segments_fast_any_k  # noqa: F401,E402

from . import cross_segments_wide_anyk  # noqa: F401,E402
from .cross_segments_wide_anyk import cross_segments_wide_anyk_plan, simtopk_cross_segments_wide_any_k  # noqa: F401,E402

from . import segmented_wide_anyk  # noqa: F401,E402
from .segmented_wide_anyk import segmented_wide_anyk_plan, simtopk_segmented_wide_any_k  # noqa: F401,E402

# (the module's router carries the name of combined_topk_anyk's call, which keeps the package-level name: reach it through the module)
from . import combined_topk16_anyk  # noqa: F401,E402
from .combined_topk16_anyk import (build_topk_hypergraph_data_fast_any_k, build_topk_weighted_hypergraph_fast_any_k,  # noqa: F401,E402
                                   combined_fast_anyk_plan, simtopk_combined_fast_any_k)

# (the module's routers carry the names of combined_topk_anyk's calls, which keep the package-level names: reach them through the module)
from . import combined_topk16_xy_anyk  # noqa: F401,E402
from .combined_topk16_xy_anyk import simtopk_combined_rows_fast_any_k, simtopk_combined_xy_fast_any_k  # noqa: F401,E402

from . import hgconv  # noqa: F401,E402
from .hgconv import HypergraphConv, hypergraph_propagate, incidence_plan, knn_incidence  # noqa: F401,E402

from . import readout  # noqa: F401,E402
from .readout import GlobalAttention, attention_readout, readout_plan  # noqa: F401,E402

from . import hypergraph_network  # noqa: F401,E402
from .hypergraph_network import HypergraphNetwork  # noqa: F401,E402

from . import hgpair  # noqa: F401,E402
from .hgpair import (HypergraphAttentionConv, IncidencePairPlan, PairWeightedHypergraphConv, hypergraph_propagate_pairs,  # noqa: F401,E402
                     incidence_pair_plan, pair_scales, pair_softmax)

from . import hg16  # noqa: F401,E402
from .hg16 import attention_readout_16, hypergraph_propagate_16, hypergraph_propagate_pairs_16  # noqa: F401,E402

from . import wide_scan  # noqa: F401,E402
from .wide_scan import list_capacity, wide_scan_supported  # noqa: F401,E402

__all__ = ["ops", "simtopk", "simtopk_segmented", "sim_dense", "sim_dense_combined", "sim_dense_combined_segmented", "edge_cosine",
           "topk_merge", "offdiag_lower_median", "threshold_edges", "knn_kmeans_edges_segmented", "build_hypergraph_knn_kmeans_segmented",
           "sim_dense_stats_segmented", "lower_median_segmented", "compute_wsi_tma_similarity_segmented", "similarity_block",
           "group_by_similarity_segmented", "filter_edges_by_median_segmented", "super_patches", "super_patch_stats", "cohort", "segment_sort_segmented",
           "pool_super_patches_segmented", "aggregate_wsi_super_patches_segmented", "build_cohort_hypergraphs", "combined_topk",
           "simtopk_combined", "build_topk_weighted_hypergraph", "build_topk_hypergraph_data", "wide_scan", "wide_scan_supported",
           "list_capacity", "combined_topk16", "simtopk_combined_fast", "build_topk_weighted_hypergraph_fast",
           "combined_topk16_segmented", "simtopk_combined_fast_segmented", "build_topk_weighted_hypergraph_fast_segmented",
           "build_topk_hypergraph_data_fast", "combined_topk_xy", "simtopk_combined_xy", "simtopk_combined_rows",
           "segmented_exact", "simtopk_segmented_exact", "simtopk_combined_exact", "segmented_exact_table",
           "kmeans_ragged", "kmeans_fit_ragged", "kmeans_fit_predict_ragged", "ragged_groups",
           "combined_topk_anyk", "anyk_route", "simtopk_combined_any_k", "simtopk_combined_xy_any_k", "simtopk_combined_rows_any_k",
           "build_topk_weighted_hypergraph_any_k", "build_topk_hypergraph_data_any_k",
           "cross_segments", "simtopk_cross_segments", "cross_segments_table", "cross_segment_knn_edges",
           "cross_segments16", "simtopk_cross_segments_fast", "cross_segments_fast_table",
           "cross_segments_wide", "simtopk_cross_segments_wide", "cross_segments_wide_table", "cross_segments_route",
           "fast_anyk", "simtopk_fast_any_k", "fast_anyk_plan",
           "wide_anyk", "simtopk_wide_any_k", "wide_anyk_plan",
           "segmented_anyk", "simtopk_segmented_fast_any_k", "segmented_anyk_plan",
           "cross_segments_anyk", "simtopk_cross_segments_fast_any_k", "cross_segments_anyk_plan",
           "cross_segments_wide_anyk", "simtopk_cross_segments_wide_any_k", "cross_segments_wide_anyk_plan",
           "segmented_wide_anyk", "simtopk_segmented_wide_any_k", "segmented_wide_anyk_plan",
           "combined_topk16_anyk", "simtopk_combined_fast_any_k", "combined_fast_anyk_plan",
           "build_topk_weighted_hypergraph_fast_any_k", "build_topk_hypergraph_data_fast_any_k",
           "combined_topk16_xy_anyk", "simtopk_combined_xy_fast_any_k", "simtopk_combined_rows_fast_any_k",
           "hgconv", "incidence_plan", "hypergraph_propagate", "knn_incidence", "HypergraphConv",
           "readout", "attention_readout", "readout_plan", "GlobalAttention", "hypergraph_network", "HypergraphNetwork",
           "hgpair", "incidence_pair_plan", "IncidencePairPlan", "pair_scales", "hypergraph_propagate_pairs", "pair_softmax",
           "PairWeightedHypergraphConv", "HypergraphAttentionConv",
           "hg16", "hypergraph_propagate_16", "hypergraph_propagate_pairs_16", "attention_readout_16"]
