"""Pair-weighted hypergraph propagation and the softmax over pairs against their compositions in torch, whole-call
times on one device.

    python scripts/hgpair_timing.py [out.txt] [--reps N] [--only CLASS]

    A    mmf.hypergraph_propagate_pairs(x, a, plan=plan, normalization="weight", scales=ready): the two weighted gather-sums
    A'   mmf.incidence_pair_plan(edge_index, N, M, check=False): the pair-plan build (two SortPairs)
    B    the same operator in torch with index_add_ on gathered, weighted rows, the scales ready (as A has them):
         Y = zeros.index_add_(0, e, a[:, None] * x[v]) * es; out = zeros.index_add_(0, v, a[:, None] * Y[e]) * ns.  Float atomics: its
         bits change from run to run.  It is the only baseline there is.
    C    mmf.hypergraph_propagate(x, plan=plan): the unweighted operator on the same incidence — what the extra operand costs
    FB   forward + backward of A under normalization="count" with gradients in x and in a (A-fb), against autograd through B (B-fb)
    S    mmf.pair_softmax(score, plan=plan, group="edge") against torch (scatter_reduce amax, exp, index_add_, divide)
    L    one HypergraphAttentionConv layer (C -> 64, heads 1), forward

The four shape classes of scripts/hgconv_timing.py; the weights are the builders' own edge_weights (class 1: the cosines of simtopk,
1 for a node in its own hyperedge).  Protocol: same process; A against B to a tolerance and A against A bit for bit before anything is
timed; one warm-up of every arm; then `reps` rounds (default 7) that time the arms in turn, each measurement a window of calls of at
least 20 ms between two device synchronisations; median and min .. max per call.  For A the minimal traffic is that of §4.35 plus
the weights read twice and the two position lists.  A machine without a GPU fails."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
WINDOW_MS = 20.0


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def knn_class(mmf, n, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, 64, generator=g).cuda()
    idx, val = mmf.simtopk(f, k=5)
    ei = mmf.knn_incidence(idx)
    rows = torch.arange(n, device=idx.device).unsqueeze(1)
    keep = torch.cat([torch.ones((n, 1), dtype=torch.bool, device=idx.device), (idx >= 0) & (idx != rows)], dim=1)
    a = torch.cat([torch.ones((n, 1), device=idx.device), val.float()], dim=1)[keep]
    return ei, a.contiguous(), n, n


def cohort_class(mmf, seed):
    from multimodal_fusion_amd import knn_kmeans_hypergraph as kk
    g = torch.Generator().manual_seed(seed)
    S, nw, nt = 2048, 77, 51
    W, T = torch.randn(S * nw, 64, generator=g).cuda(), torch.randn(S * nt, 64, generator=g).cuda()
    wp, tp = torch.arange(S + 1) * nw, torch.arange(S + 1) * nt
    ei, ew, _, _ = kk.build_hypergraph_knn_kmeans_segmented(W, T, None, 5, 10, wsi_ptr=wp, tma_ptr=tp)
    return ei.contiguous(), ew.float().contiguous(), S * (nw + nt), S * (nw + nt)


def threshold_class(mmf, seed):
    g = torch.Generator().manual_seed(seed)
    f = (torch.randn(4096, 64, generator=g) * 0.1).cuda()
    K = mmf.sim_dense(f, metric="rbf", lam=1.0)
    thr = float(mmf.offdiag_lower_median(K))
    ei, ew = mmf.threshold_edges(K, thr)
    return ei.contiguous(), ew.float().contiguous(), 4096, 4096


def scatter_arm(x, a, ei, N, M, es, ns):
    v, e = ei[0], ei[1]
    Y = torch.zeros((M, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, e, a.unsqueeze(1) * x[v]) * es
    return torch.zeros((N, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, v, a.unsqueeze(1) * Y[e]) * ns


def softmax_arm(score, e, M):
    m = torch.full((M,), float("-inf"), device=score.device).scatter_reduce_(0, e, score, "amax")
    w = torch.exp(score - m[e])
    return w / torch.zeros((M,), device=score.device).index_add_(0, e, w)[e]


def main():
    import multimodal_fusion_amd as mmf
    if not torch.cuda.is_available():
        raise SystemExit("hgpair_timing: no GPU: nothing is measured on a CPU")
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    only = args[args.index("--only") + 1] if "--only" in args else None
    out_path = args[0] if args and not args[0].startswith("--") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                    "profiles", "hgpair_timing.txt")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"# scripts/hgpair_timing.py --reps {reps} ({torch.cuda.get_device_name(0)}; same process, one warm-up of every arm, then {reps} rounds "
        f"timing the arms in turn; windows of >= {WINDOW_MS:.0f} ms between device synchronisations; per call: median (min .. max))")
    classes = [("1", "k-NN incidence, N = 262144, k = 5 with self, cosine weights", lambda: knn_class(mmf, 262144, 1), 256),
               ("2", "cohort of 2048 graphs x 128 nodes, k-NN + KMeans edges and weights", lambda: cohort_class(mmf, 2), 256),
               ("3", "median-threshold graph, N = 4096, RBF weights", lambda: threshold_class(mmf, 3), 256),
               ("4", "k-NN incidence, N = 262144, k = 5 with self, cosine weights", lambda: knn_class(mmf, 262144, 1), 16)]
    for tag, name, make, C in classes:
        if only is not None and only != tag:
            continue
        ei, a, N, M = make()
        E = ei.shape[1]
        gen = torch.Generator().manual_seed(10 + int(tag))
        x = torch.randn(N, C, generator=gen).cuda()
        G = torch.randn(N, C, generator=gen).cuda()
        score = (3 * torch.randn(E, generator=gen)).cuda()
        plan = mmf.incidence_pair_plan(ei, N, M)
        es, ns = mmf.pair_scales(a, plan=plan)
        esu, nsu = es.unsqueeze(1), ns.unsqueeze(1)
        binv, dinv = plan.edge_scale.unsqueeze(1), plan.node_scale.unsqueeze(1)
        torch.manual_seed(0)
        layer = mmf.HypergraphAttentionConv(C, 64).cuda()
        attr = torch.randn(M, C, generator=gen).cuda()

        def fb_a():
            xd, ad = x.detach().requires_grad_(), a.detach().requires_grad_()
            mmf.hypergraph_propagate_pairs(xd, ad, plan=plan).backward(G)
            return xd.grad, ad.grad

        def fb_b():
            xd, ad = x.detach().requires_grad_(), a.detach().requires_grad_()
            scatter_arm(xd, ad, ei, N, M, binv, dinv).backward(G)
            return xd.grad, ad.grad

        def layer_fwd():
            with torch.no_grad():
                return layer(x, ei, hyperedge_attr=attr, plan=plan)

        arms = [("A", lambda: mmf.hypergraph_propagate_pairs(x, a, plan=plan, normalization="weight", scales=(es, ns))),
                ("A'", lambda: mmf.incidence_pair_plan(ei, N, M, check=False)),
                ("B", lambda: scatter_arm(x, a, ei, N, M, esu, nsu)),
                ("C", lambda: mmf.hypergraph_propagate(x, plan=plan)),
                ("A-fb", fb_a), ("B-fb", fb_b),
                ("S", lambda: mmf.pair_softmax(score, plan=plan, group="edge")), ("S-torch", lambda: softmax_arm(score, ei[1], M)),
                ("L", layer_fwd)]
        fns = dict(arms)
        a0, a1, b0 = fns["A"](), fns["A"](), fns["B"]()
        (gxa, gaa), (gxb, gab) = fb_a(), fb_b()
        s0, s1 = fns["S"](), fns["S-torch"]()
        torch.cuda.synchronize()
        deg_e, deg_n = (plan.eptr[1:] - plan.eptr[:-1]), (plan.nptr[1:] - plan.nptr[:-1])
        say(f"class {tag}: {name}, C = {C}: N {N}  M {M}  pairs {E}  hyperedge size median {int(deg_e.median())} max {int(deg_e.max())}  "
            f"node degree median {int(deg_n.median())} max {int(deg_n.max())}  weights {float(a.min()):.3f} .. {float(a.max()):.3f}")
        say(f"   A against A bit for bit: {bool(torch.equal(a0, a1))};  max |A - B| = {float((a0 - b0).abs().max()):.3e} at max |B| = {float(b0.abs().max()):.3e};  "
            f"grad_x {float((gxa - gxb).abs().max()):.3e} at {float(gxb.abs().max()):.3e};  grad_a {float((gaa - gab).abs().max()):.3e} at {float(gab.abs().max()):.3e};  "
            f"softmax {float((s0 - s1).abs().max()):.3e}")
        inner = {}
        for key, fn in arms:
            window(fn, 1)
            inner[key] = max(1, int(np.ceil(WINDOW_MS / max(window(fn, 2), 1e-3))))
        t = {key: [] for key, _ in arms}
        for _ in range(reps):
            for key, fn in arms:
                t[key].append(window(fn, inner[key]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        AP = "A'"
        minimal = 2 * (N + M) * C * 4 + 2 * E * 4 + 2 * E * 4 + 2 * E * 4 + (N + M + 2) * 8 + (N + M) * 4
        asked = 2 * E * C * 4 + (N + M) * C * 4
        rate = minimal / (med["A"] * 1e-3)

        def row(key, label, extra=""):
            say(f"   {key:<8}{label:<44}{med[key]:9.3f} ms ({min(t[key]):.3f} .. {max(t[key]):.3f})   calls per window {inner[key]}{extra}")

        row("A", "propagate_pairs, ready plan and scales", f";  minimal traffic {minimal / 1e6:.1f} MB -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the "
            f"8 TB/s HBM peak;  the gathers ask for {asked / 1e6:.1f} MB -> {asked / (med['A'] * 1e-3) / 1e12:.3f} TB/s")
        row("A'", "pair-plan build", f";  = {med[AP] / med['A']:.1f} propagations")
        row("B", "index_add_ on weighted rows in torch", f";  B / A = {med['B'] / med['A']:.2f}")
        row("C", "unweighted hypergraph_propagate", f";  A / C = {med['A'] / med['C']:.2f}")
        row("A-fb", "forward + backward, grad_x and grad_a")
        row("B-fb", "autograd through B", f";  B-fb / A-fb = {med['B-fb'] / med['A-fb']:.2f}")
        row("S", "pair_softmax, group = edge")
        row("S-torch", "amax, exp, index_add_, divide in torch", f";  S-torch / S = {med['S-torch'] / med['S']:.2f}")
        row("L", f"HypergraphAttentionConv({C}, 64), forward")
        del plan, x, G, ei, a, a0, a1, b0, gxa, gaa, gxb, gab, layer, attr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
