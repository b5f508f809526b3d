"""Segmented k-NN + KMeans hypergraph: one build_hypergraph_knn_kmeans_segmented call (A) against the Python loop of the plain
build_hypergraph_knn_kmeans per slide (B) and, where the old pair ops can hold the clusters (segments x H <= 16384), against
the composition of the existing batched pieces (C: simtopk_segmented + kmeans_fit_predict_segmented + segment_sort /
clique_pairs / knn_pairs over global labels + torch.sort + edge_cosine).  d = 512, k = 5, H = 10.

    python scripts/knn_kmeans_segmented_timing.py [out.txt] [--shapes 1,2,3,4] [--reps N] [--a-only]

Shapes: (1) 1000 slides of 100 + 64 rows; (2) 2048 x 128 rows; (3) a ragged cohort of 300 slides of 40 .. 2000 rows
(log-uniform, fixed seed, about 60 % wsi rows); (4) 16 x 4096 rows.  Rows are Gaussian.  Same process, one warm-up call of
each variant per shape, then `reps` rounds that time A, B, C in turn with a device synchronisation around every timed call;
median and min .. max are reported; the edge stage is also timed alone, neighbours and labels given.  The outputs of all variants are compared in the same run before anything is timed (edge
ids equal, weights the same bits, edge_ptr equal to the loop's counts).  --a-only times A alone (for a kernel trace)."""
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_fusion_amd as mmf  # noqa: E402

kk = import_module("multimodal_fusion_amd.knn_kmeans_hypergraph")
bh = import_module("multimodal_fusion_amd.build_hypergraph")
kmeans = import_module("multimodal_fusion_amd.kmeans")
ops = mmf.ops
dev = torch.device("cuda", 0)
lines = []
D, K, H = 512, 5, 10
SEG_MAX = 16384          # clusters mmf_segment_sort / mmf_clique_pairs hold


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def shapes():
    rng = np.random.RandomState(7)
    ragged = np.exp(rng.uniform(np.log(40), np.log(2000), 300)).astype(np.int64).tolist()
    ragged[0], ragged[-1] = 40, 2000
    split = lambda sizes: ([(3 * n) // 5 for n in sizes], [n - (3 * n) // 5 for n in sizes])
    return {1: ("1000 x (100 + 64)", [100] * 1000, [64] * 1000), 2: ("2048 x 128", *split([128] * 2048)),
            3: ("ragged 300 x 40..2000", *split(ragged)), 4: ("16 x 4096", *split([4096] * 16))}


def variant_b(W, Tm, wp, tp):
    eis, ews, cnt = [], [], []
    for s in range(len(wp) - 1):
        ei, ew, _ = bh.build_hypergraph_knn_kmeans(W[wp[s]:wp[s + 1]], Tm[tp[s]:tp[s + 1]], None, K, H)
        eis.append(ei + (wp[s] + tp[s])); ews.append(ew); cnt.append(ew.numel())
    return torch.cat(eis, 1), torch.cat(ews), cnt


def variant_c(X, node_ptr, seg_of_row):
    n = X.shape[0]
    nbr, _ = ops.simtopk_segmented(X, ptr=node_ptr, metric="neg_sq_l2", k=K, exclude_self=True)
    labels, _, _ = kmeans.kmeans_fit_predict_segmented(X, H, ptr=node_ptr, n_init=10, seed=42)
    gl = seg_of_row * H + labels
    seg = ops.segment_sort(gl, (len(node_ptr) - 1) * H)
    c_lo, c_hi = ops.clique_pairs(seg)
    k_lo, k_hi = ops.knn_pairs(nbr, gl)
    code = torch.sort(torch.cat([c_lo, k_lo]) * n + torch.cat([c_hi, k_hi])).values
    ei = torch.stack([code // n, code % n], dim=0).contiguous()
    return ei, ops.edge_cosine(X, ei)


def edges_new(X, nbr, labels, node_ptr):
    ei, _ = ops.knn_clique_edges(nbr, labels, H, ptr=node_ptr)
    return ei, ops.edge_cosine(X, ei)


def edges_old(X, nbr, gl, n_ids):
    n = X.shape[0]
    seg = ops.segment_sort(gl, n_ids)
    c_lo, c_hi = ops.clique_pairs(seg)
    k_lo, k_hi = ops.knn_pairs(nbr, gl)
    code = torch.sort(torch.cat([c_lo, k_lo]) * n + torch.cat([c_hi, k_hi])).values
    ei = torch.stack([code // n, code % n], dim=0).contiguous()
    return ei, ops.edge_cosine(X, ei)


def stat(ts):
    return f"{np.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    args = sys.argv[1:]
    out_path = next((a for a in args if a.endswith(".txt")), None)
    sel = [int(v) for v in args[args.index("--shapes") + 1].split(",")] if "--shapes" in args else [1, 2, 3, 4]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    a_only = "--a-only" in args
    for key in sel:
        name, nw, nt = shapes()[key]
        wp, tp = offsets(nw), offsets(nt)
        sizes = [a + b for a, b in zip(nw, nt)]
        node_ptr = offsets(sizes)
        g = torch.Generator().manual_seed(key)
        W, Tm = torch.randn(wp[-1], D, generator=g).to(dev), torch.randn(tp[-1], D, generator=g).to(dev)
        run_a = lambda: kk.build_hypergraph_knn_kmeans_segmented(W, Tm, None, K, H, wsi_ptr=wp, tma_ptr=tp)
        _, (ei, ew, eptr, st) = once(run_a)
        head = (f"{name}: slides {len(sizes)}  nodes {node_ptr[-1]}  nodes/slide {min(sizes)}..{max(sizes)}  d {D}  k {K}  H {H}  "
                f"edges {ew.numel()}  ambiguous slides {sum(1 for v in st['ambiguous_draws'] if v)}")
        if a_only:
            ta = [once(run_a)[0] for _ in range(reps)]
            say(head)
            say(f"  A segmented builder {stat(ta)}")
            continue
        with_c = len(sizes) * H <= SEG_MAX
        X = torch.cat([torch.cat([W[wp[s]:wp[s + 1]], Tm[tp[s]:tp[s + 1]]]) for s in range(len(sizes))])
        seg_of_row = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
        run_b = lambda: variant_b(W, Tm, wp, tp)
        run_c = lambda: variant_c(X, node_ptr, seg_of_row)
        _, (bei, bew, cnt) = once(run_b)
        assert torch.equal(ei, bei) and torch.equal(ew.view(torch.int32), bew.view(torch.int32)), "A and B differ"
        assert (eptr[1:] - eptr[:-1]).tolist() == cnt, "edge_ptr differs from the loop's counts"
        if with_c:
            _, (cei, cew) = once(run_c)
            assert torch.equal(ei, cei) and torch.equal(ew.view(torch.int32), cew.view(torch.int32)), "A and C differ"
            del cei, cew
        del bei, bew
        ta, tb, tc = [], [], []
        for _ in range(reps):
            ta.append(once(run_a)[0])
            tb.append(once(run_b)[0])
            if with_c:
                tc.append(once(run_c)[0])
        say(head)
        say(f"  A segmented builder          {stat(ta)}")
        say(f"  B loop of the plain mirror   {stat(tb)}   B / A {np.median(tb) / np.median(ta):7.2f}x")
        if with_c:
            say(f"  C composition of the pieces  {stat(tc)}   C / A {np.median(tc) / np.median(ta):7.2f}x")
        else:
            say(f"  C not possible: {len(sizes)} x {H} clusters > {SEG_MAX}")
        say("  same edges and weight bits in all variants: True")
        # the edge stage alone (neighbours and labels given): the new entry + edge_cosine against the pieces + sort + edge_cosine
        nbr, _ = ops.simtopk_segmented(X, ptr=node_ptr, metric="neg_sq_l2", k=K, exclude_self=True)
        labels, _, _ = kmeans.kmeans_fit_predict_segmented(X, H, ptr=node_ptr, n_init=10, seed=42)
        gl = seg_of_row * H + labels
        once(lambda: edges_new(X, nbr, labels, node_ptr))
        tn, to = [], []
        if with_c:
            once(lambda: edges_old(X, nbr, gl, len(sizes) * H))
        for _ in range(reps):
            tn.append(once(lambda: edges_new(X, nbr, labels, node_ptr))[0])
            if with_c:
                to.append(once(lambda: edges_old(X, nbr, gl, len(sizes) * H))[0])
        say(f"  edge stage alone: new entry  {stat(tn)}" + (f"   pieces + sort {stat(to)}   {np.median(to) / np.median(tn):5.2f}x" if with_c else ""))
        tn = [once(lambda: ops.knn_clique_edges(nbr, labels, H, ptr=node_ptr))[0] for _ in range(reps)]
        say(f"  of which the edge list (count + fill, without weights) {stat(tn)}")
        del ei, ew, X
        torch.cuda.empty_cache()
    say(f"device: {torch.cuda.get_device_name(0)}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
