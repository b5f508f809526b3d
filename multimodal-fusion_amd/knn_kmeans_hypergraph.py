"""The k-NN + KMeans hypergraph (build_hypergraph/preprocess_hypergraph.py:373-433, what process_single_file writes for every
slide) of every graph of a ragged batch in one call: Euclidean k-NN pairs, the cliques of a KMeans over the same nodes, the
undirected dedup, max(0, cosine) weights.

Segment s's edges are bit for bit those of ``build_hypergraph_knn_kmeans`` on that slide with both ids shifted by the
segment's first node.  The three batched steps run once for the whole batch: ``simtopk_segmented`` for the
neighbours (``wide_scan.simtopk_segmented`` where the feature dim is above 1024 and the wide 16-bit scan applies,
``segmented_exact.simtopk_segmented_exact`` where no 16-bit scan applies), ``kmeans_fit_predict_segmented`` for the labels, ``ops.knn_clique_edges`` for the edge list, which comes out in
its documented order without a sort and costs one host read (the edge count).  The labels are scikit-learn's unless a seeding
decision came within float32 noise of going the other way: ``ambiguous_draws`` / ``ambiguous_trials`` say for which segments.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops, ragged, wide_scan
from .kmeans import segmented_labels
from .build_hypergraph import preprocess_hypergraph
from .build_hypergraph._common import compute_device, result_device_like_preprocess, to_gpu


def knn_kmeans_edges_segmented(X: torch.Tensor, k: int = 5, num_hyperedges: int = 10, *, ptr=None, batch=None,
                               return_info: bool = False):
    """The hypergraph of every segment of X ([N, D] nodes, already concatenated per segment; exactly one of ptr / batch):
    (edge_index [2, E] int64 global row ids, lexicographic in (lo, hi); edge_weights [E] f32; edge_ptr [S + 1] int64) on X's
    device, which must be a ROCm device.  return_info adds a dict with the KMeans backend and, for the device backend, every
    segment's ambiguous_draws / ambiguous_trials (None for 'sklearn')."""
    what = "knn_kmeans_edges_segmented"
    X = ops._feat(X, what + " X")
    p = ragged.offsets(ptr, batch, X.shape[0], what=what)
    k, num_hyperedges = int(k), int(num_hyperedges)
    ragged.check_knn_sizes((p[1:] - p[:-1]).tolist(), k, what, n_clusters=num_hyperedges)
    ops._need_gpu(X, what)
    X = X.detach().float().contiguous()
    # feature dims above 1024: the entry with the wide 16-bit scan behind it (one launch, not the exact pass per segment; the same
    # bits — DESIGN.md §4.16)
    if wide_scan.wide_scan_supported(X.shape[1], k, True):
        nbr, _ = wide_scan.simtopk_segmented(X, ptr=p, metric="neg_sq_l2", k=k, exclude_self=True)
    elif not ops.fast_scan_supported(X.shape[1], k, True):
        # no 16-bit scan applies (k + self > 20 above d = 512, d > 4096): one table-driven launch of the exact scan instead of the
        # exact pass per segment; the same bits — DESIGN.md §4.20
        from . import segmented_exact
        nbr, _ = segmented_exact.simtopk_segmented_exact(X, ptr=p, metric="neg_sq_l2", k=k, exclude_self=True)
    else:
        nbr, _ = ops.simtopk_segmented(X, ptr=p, metric="neg_sq_l2", k=k, exclude_self=True)
    labels, draws, trials = segmented_labels(X, p, num_hyperedges)
    edge_index, edge_ptr = ops.knn_clique_edges(nbr, labels, num_hyperedges, ptr=p)
    if edge_index.shape[1] == 0:
        edge_weights = torch.empty((0,), dtype=torch.float32, device=X.device)
    else:
        edge_weights = ops.edge_cosine(X, edge_index)
    if return_info:
        return edge_index, edge_weights, edge_ptr, {"kmeans_backend": preprocess_hypergraph.KMEANS_BACKEND,
                                                    "ambiguous_draws": draws, "ambiguous_trials": trials}
    return edge_index, edge_weights, edge_ptr


def node_offsets(n_wsi: int, n_tma: int, *, wsi_ptr=None, wsi_batch=None, tma_ptr=None, tma_batch=None,
                 what: str = "build_hypergraph_knn_kmeans_segmented") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Host offsets (wsi_ptr, tma_ptr, node_ptr = wsi_ptr + tma_ptr) of the two-sided segment description: segment s has the
    nodes wsi[wsi_ptr[s]:wsi_ptr[s+1]] then tma[tma_ptr[s]:tma_ptr[s+1]], numbered from node_ptr[s].  Both sides must describe the same
    number of segments (a batch vector ends at its last id: trailing segments without rows need ptr)."""
    wp, tp = ragged.two_sided(n_wsi, n_tma, wsi_ptr, wsi_batch, tma_ptr, tma_batch, xs="wsi_", ys="tma_", what=what)
    return wp, tp, wp + tp


def build_hypergraph_knn_kmeans_segmented(wsi_features: torch.Tensor, tma_features: torch.Tensor, group_labels=None, k: int = 5,
                                          num_hyperedges: int = 10, device: Optional[torch.device] = None, *, wsi_ptr=None,
                                          wsi_batch=None, tma_ptr=None,
                                          tma_batch=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Dict]:
    """build_hypergraph_knn_kmeans of every slide of a cohort: (edge_index [2, E] int64, edge_weights [E] f32, edge_ptr [S + 1]
    int64, stats) on `device` (None: the features' device if it is a GPU, else the CPU, as the plain mirror).  Slide s has the
    nodes wsi[wsi_ptr[s]:wsi_ptr[s+1]] then tma[tma_ptr[s]:tma_ptr[s+1]] (the mirror's torch.cat; a slide may have no TMA rows),
    numbered from stats['node_ptr'][s]; each side's segments come as ptr or batch.  `group_labels` is accepted and ignored, as
    in the mirror.  stats is JSON-serialisable: the totals, node_ptr, 'segments' (per slide the plain mirror's stats) and
    'ambiguous_draws' / 'ambiguous_trials' per slide (None with the 'sklearn' KMeans backend).  Every argument error is raised
    on the host, before any device work, and names the first bad segment."""
    what = "build_hypergraph_knn_kmeans_segmented"
    if wsi_features.dim() != 2 or tma_features.dim() != 2:
        raise ValueError(f"{what}: wsi_features and tma_features must be 2-D [N, D]")
    if wsi_features.shape[1] != tma_features.shape[1]:
        raise ValueError(f"{what}: wsi_features have D={wsi_features.shape[1]}, tma_features D={tma_features.shape[1]}")
    n_wsi, n_tma = wsi_features.shape[0], tma_features.shape[0]
    wp, tp, node_ptr = node_offsets(n_wsi, n_tma, wsi_ptr=wsi_ptr, wsi_batch=wsi_batch, tma_ptr=tma_ptr, tma_batch=tma_batch,
                                    what=what)
    k, num_hyperedges = int(k), int(num_hyperedges)
    sizes = (node_ptr[1:] - node_ptr[:-1]).tolist()
    ragged.check_knn_sizes(sizes, k, what, n_clusters=num_hyperedges)
    out_dev = result_device_like_preprocess(wsi_features, device)
    dev = out_dev if out_dev.type == "cuda" else compute_device(wsi_features, tma_features)
    # the mirror's torch.cat per slide, as two scatters: wsi row r of slide s -> r + tma_ptr[s], tma row r -> r + wsi_ptr[s+1]
    w_sizes, t_sizes = wp[1:] - wp[:-1], tp[1:] - tp[:-1]
    X = torch.empty((n_wsi + n_tma, wsi_features.shape[1]), dtype=torch.float32, device=dev)
    X[(torch.arange(n_wsi) + torch.repeat_interleave(tp[:-1], w_sizes)).to(dev)] = to_gpu(wsi_features, dev)
    if n_tma:
        X[(torch.arange(n_tma) + torch.repeat_interleave(wp[1:], t_sizes)).to(dev)] = to_gpu(tma_features, dev)
    edge_index, edge_weights, edge_ptr, info = knn_kmeans_edges_segmented(X, k, num_hyperedges, ptr=node_ptr, return_info=True)
    counts = (edge_ptr[1:] - edge_ptr[:-1]).tolist()
    segments = [{"num_nodes": int(n_s), "num_wsi_super_patches": int(nw), "num_tma_patches": int(nt), "num_edges": int(e),
                 "num_hyperedges": num_hyperedges, "k": k}
                for n_s, nw, nt, e in zip(sizes, w_sizes.tolist(), t_sizes.tolist(), counts)]
    stats = {"num_segments": len(sizes), "num_nodes": int(node_ptr[-1]), "num_wsi_super_patches": int(n_wsi),
             "num_tma_patches": int(n_tma), "num_edges": int(edge_index.shape[1]), "num_hyperedges": num_hyperedges, "k": k,
             "node_ptr": node_ptr.tolist(), "kmeans_backend": info["kmeans_backend"], "ambiguous_draws": info["ambiguous_draws"],
             "ambiguous_trials": info["ambiguous_trials"], "segments": segments}
    return edge_index.to(out_dev), edge_weights.to(out_dev), edge_ptr.to(out_dev), stats
