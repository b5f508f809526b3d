"""process_single_file's four arithmetic steps (build_hypergraph/preprocess_hypergraph.py:554-603) for every slide of a cohort, in
memory and without HDF5: super patches -> WSI x TMA similarity -> grouping -> k-NN + KMeans hypergraph, one cohort call per step
(DESIGN.md §4.12, §4.11, §4.10).  The HDF5 pipelines (process_dataset, batch_rebuild_hypergraph) keep their per-file loop.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ragged
from .cross_segments import link_slides  # noqa: F401  (cohort.link_slides: the inter-slide edges of this module's result)
from .knn_kmeans_hypergraph import build_hypergraph_knn_kmeans_segmented
from .super_patches import aggregate_wsi_super_patches_segmented
from .wsi_tma_similarity import compute_wsi_tma_similarity_segmented, group_by_similarity_segmented


def build_cohort_hypergraphs(wsi_features: torch.Tensor, wsi_positions: torch.Tensor, tma_features: torch.Tensor, *, wsi_ptr=None,
                             wsi_batch=None, tma_ptr=None, tma_batch=None, num_wsi_super_patches: int = 100, num_groups: int = 10,
                             hypergraph_k: int = 5, num_hyperedges: int = 10, lambda_h: float = 1.0, lambda_g: float = 1.0,
                             device: Optional[torch.device] = None, keep_similarity: bool = False,
                             budget_bytes: Optional[int] = None) -> Dict:
    """The hypergraph of every slide of a cohort.  Slide s is wsi rows wsi_ptr[s]:wsi_ptr[s+1] (patches) with tma rows
    tma_ptr[s]:tma_ptr[s+1]; each side's slides come as ptr or batch.  Every slide needs TMA rows (process_single_file skips a
    file without them; here that is a ValueError naming the slide).  Returns a dict:

        super_features [S*C, D], super_positions [S*C, dp]     slide s's super patches are rows s*C .. (s+1)*C - 1
        S_flat, s_ptr                                          WSI x TMA similarity blocks [C, m_s] at s_ptr[s]
        group_labels int32 [S*C], group_ptr [S + 1]            slide s's labels are group_ptr[s]:group_ptr[s+1]
        edge_index [2, E], edge_weights [E], edge_ptr, node_ptr   slide s's nodes are numbered from node_ptr[s]
        K_flat, k_ptr                                          the WSI similarity blocks, K_flat None unless keep_similarity
        stats                                                  per slide {"wsi_aggregation", "similarity", "grouping",
                                                               "hypergraph"}: process_single_file's dict, JSON-serialisable

    Per slide everything equals the chain of the four plain mirrors on that slide.  budget_bytes: the memory the similarity
    blocks of one group of slides may take in the first step (aggregate_wsi_super_patches_segmented; None: its default); with
    keep_similarity=False a slide whose block alone is larger has its statistics streamed and its block never stored."""
    what = "build_cohort_hypergraphs"
    if wsi_features.dim() != 2 or wsi_positions.dim() != 2 or tma_features.dim() != 2:
        raise ValueError(f"{what}: slide 0: wsi_features, wsi_positions and tma_features must be 2-D")
    if wsi_features.shape[1] != tma_features.shape[1]:
        raise ValueError(f"{what}: slide 0: wsi_features have D={wsi_features.shape[1]}, tma_features D={tma_features.shape[1]}")
    wp, tp = ragged.two_sided(wsi_features.shape[0], tma_features.shape[0], wsi_ptr, wsi_batch, tma_ptr, tma_batch, xs="wsi_",
                              ys="tma_", what=what, unit="slide", min_rows=(1, 0))
    S = wp.numel() - 1
    empty = torch.nonzero(tp[1:] == tp[:-1]).reshape(-1)
    if empty.numel():
        raise ValueError(f"{what}: slide {int(empty[0])} has no TMA rows (the per-file pipeline skips such a file)")
    C, G = int(num_wsi_super_patches), int(num_groups)
    # what the four steps' KMeans and k-NN calls would object to, before the first step touches the device (the first step's
    # own limits on C are its to report: it checks them on the host too)
    ragged.check_kmeans_sizes((wp[1:] - wp[:-1]).tolist(), C, what, "slide")
    ragged.check_kmeans_sizes([C], G, what, "slide")
    k, H = int(hypergraph_k), int(num_hyperedges)
    ragged.check_knn_sizes((C + (tp[1:] - tp[:-1])).tolist(), k, what, "slide", n_clusters=H)
    sf, sp, agg_stats, K_flat, k_ptr = aggregate_wsi_super_patches_segmented(
        wsi_features, wsi_positions, C, lambda_h, lambda_g, device, ptr=wp, keep_similarity=keep_similarity,
        budget_bytes=budget_bytes)
    sw = torch.arange(S + 1, dtype=torch.int64) * C
    S_flat, s_ptr, sim_stats = compute_wsi_tma_similarity_segmented(sf, sp, tma_features, lambda_h, lambda_g, device, wsi_ptr=sw,
                                                                    tma_ptr=tp)
    labels, group_stats, _ = group_by_similarity_segmented(S_flat, G, wsi_ptr=sw, tma_ptr=tp)
    edge_index, edge_weights, edge_ptr, hg = build_hypergraph_knn_kmeans_segmented(sf, tma_features, labels, k, H,
                                                                                  device, wsi_ptr=sw, tma_ptr=tp)
    stats = [{"wsi_aggregation": agg_stats[s], "similarity": sim_stats[s], "grouping": group_stats[s], "hypergraph": hg["segments"][s]}
             for s in range(S)]
    return {"super_features": sf, "super_positions": sp, "S_flat": S_flat, "s_ptr": s_ptr, "group_labels": labels, "group_ptr": sw,
            "edge_index": edge_index, "edge_weights": edge_weights, "edge_ptr": edge_ptr,
            "node_ptr": torch.tensor(hg["node_ptr"], dtype=torch.int64), "K_flat": K_flat, "k_ptr": k_ptr, "stats": stats}

