"""Hypergraph propagation against the scatter formulation in torch, whole-call times on one device.

    python scripts/hgconv_timing.py [out.txt] [--reps N] [--only CLASS]

    A    mmf.hypergraph_propagate(x, plan=plan): the two gather-sums over a ready plan (mmf_hypergraph_propagate)
    A'   mmf.incidence_plan(edge_index, N, M, check=False): the plan build (mmf_incidence_plan; two radix sorts)
    B    the same operator as torch_geometric's HypergraphConv computes it, written with index_add_ in torch on the same device, with
         1 / B_e and 1 / D_v ready (as A's plan has them): Y = zeros.index_add_(0, e, x[v]) * Binv; out = zeros.index_add_(0, v, Y[e]) * Dinv.
         Float atomics: its bits change from run to run.  It is the only baseline there is (torch_geometric itself is not installable
         next to this library).

Shape classes, C = 256 unless said otherwise:
    1  the k-NN incidence (knn_incidence, with self) of N = 262144, k = 5: hyperedges of 6 nodes, node degrees around 6
    2  a cohort of 2048 graphs of 128 nodes, the edges of build_hypergraph_knn_kmeans_segmented read as the model reads them
    3  the median-threshold graph of N = 4096: about 8.4 M pairs, rows of about 2048 members
    4  class 1 at C = 16

Protocol: same process; A against B to a tolerance and A against A bit for bit before anything is timed; one warm-up call of every arm;
then `reps` rounds (default 7) that time A, A', B in turn, each measurement a window of calls of at least 20 ms between two device
synchronisations; median and min .. max per call.  For A also: the bytes of the minimal traffic (x and Y read once, Y and out written
once, both id lists, offsets and scales) over the median time, and that rate as a share of the 8 TB/s HBM peak; the bytes the
gathers ask for (every member row once per pair) are listed beside it.  A machine without a GPU fails."""
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
    idx, _ = mmf.simtopk(f, k=5)
    return mmf.knn_incidence(idx), n, n


def cohort_class(mmf, seed):
    from multimodal_fusion_amd import knn_kmeans_hypergraph as kk
    g = torch.Generator().manual_seed(seed)
    S, nw, nt = 2048, 77, 51
    W, T = torch.randn(S * nw, 64, generator=g).cuda(), torch.randn(S * nt, 64, generator=g).cuda()
    wp, tp = torch.arange(S + 1) * nw, torch.arange(S + 1) * nt
    ei, _, _, _ = kk.build_hypergraph_knn_kmeans_segmented(W, T, None, 5, 10, wsi_ptr=wp, tma_ptr=tp)
    return ei.contiguous(), S * (nw + nt), S * (nw + nt)


def threshold_class(mmf, seed):
    g = torch.Generator().manual_seed(seed)
    f = (torch.randn(4096, 64, generator=g) * 0.1).cuda()
    K = mmf.sim_dense(f, metric="rbf", lam=1.0)
    thr = float(mmf.offdiag_lower_median(K))
    ei, _ = mmf.threshold_edges(K, thr)
    return ei.contiguous(), 4096, 4096


def scatter_arm(x, ei, N, M, binv, dinv):
    v, e = ei[0], ei[1]
    Y = torch.zeros((M, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, e, x[v]) * binv
    return torch.zeros((N, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, v, Y[e]) * dinv


def main():
    import multimodal_fusion_amd as mmf
    if not torch.cuda.is_available():
        raise SystemExit("hgconv_timing: no GPU: nothing is measured on a CPU")
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    only = args[args.index("--only") + 1] if "--only" in args else None
    out_path = args[0] if args and not args[0].startswith("--") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                    "profiles", "hgconv_timing.txt")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"# scripts/hgconv_timing.py --reps {reps} ({torch.cuda.get_device_name(0)}; same process, one warm-up of every arm, then {reps} rounds "
        f"timing A, A', B in turn; windows of >= {WINDOW_MS:.0f} ms between device synchronisations; per call: median (min .. max))")
    classes = [("1", "k-NN incidence, N = 262144, k = 5 with self", lambda: knn_class(mmf, 262144, 1), 256),
               ("2", "cohort of 2048 graphs x 128 nodes, k-NN + KMeans edges", lambda: cohort_class(mmf, 2), 256),
               ("3", "median-threshold graph, N = 4096", lambda: threshold_class(mmf, 3), 256),
               ("4", "k-NN incidence, N = 262144, k = 5 with self", lambda: knn_class(mmf, 262144, 1), 16)]
    for tag, name, make, C in classes:
        if only is not None and only != tag:
            continue
        ei, N, M = make()
        E = ei.shape[1]
        x = torch.randn(N, C, generator=torch.Generator().manual_seed(10 + int(tag))).cuda()
        plan = mmf.incidence_plan(ei, N, M)
        deg_e, deg_n = (plan.eptr[1:] - plan.eptr[:-1]), (plan.nptr[1:] - plan.nptr[:-1])
        binv, dinv = plan.edge_scale.unsqueeze(1), plan.node_scale.unsqueeze(1)
        run_a = lambda: mmf.hypergraph_propagate(x, plan=plan)
        run_p = lambda: mmf.incidence_plan(ei, N, M, check=False)
        run_b = lambda: scatter_arm(x, ei, N, M, binv, dinv)
        a0, a1, b0 = run_a(), run_a(), run_b()
        torch.cuda.synchronize()
        scale = float(b0.abs().max())
        dev_ab = float((a0 - b0).abs().max())
        say(f"class {tag}: {name}, C = {C}: N {N}  M {M}  pairs {E}  hyperedge size median {int(deg_e.median())} max {int(deg_e.max())}  "
            f"node degree median {int(deg_n.median())} max {int(deg_n.max())}")
        say(f"   A against A bit for bit: {bool(torch.equal(a0, a1))};  max |A - B| = {dev_ab:.3e} at max |B| = {scale:.3e}"
            f" (B against B bit for bit: {bool(torch.equal(b0, run_b()))})")
        inner = {}
        for key, fn in (("A", run_a), ("A'", run_p), ("B", run_b)):
            window(fn, 1)
            inner[key] = max(1, int(np.ceil(WINDOW_MS / max(window(fn, 2), 1e-3))))
        AP = "A'"
        t = {"A": [], AP: [], "B": []}
        for _ in range(reps):
            for key, fn in (("A", run_a), ("A'", run_p), ("B", run_b)):
                t[key].append(window(fn, inner[key]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        minimal = 2 * (N + M) * C * 4 + 2 * E * 4 + (N + M + 2) * 8 + (N + M) * 4
        asked = 2 * E * C * 4 + (N + M) * C * 4
        rate = minimal / (med["A"] * 1e-3)
        say(f"   A   propagate, ready plan   {med['A']:9.3f} ms ({min(t['A']):.3f} .. {max(t['A']):.3f})   calls per window {inner['A']};  minimal traffic "
            f"{minimal / 1e6:.1f} MB -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak;  the gathers ask for {asked / 1e6:.1f} MB"
            f" -> {asked / (med['A'] * 1e-3) / 1e12:.3f} TB/s")
        say(f"   A'  plan build              {med[AP]:9.3f} ms ({min(t[AP]):.3f} .. {max(t[AP]):.3f})   calls per window {inner[AP]};  = {med[AP] / med['A']:.1f} propagations")
        spread_b = max(t["B"]) - min(t["B"])
        say(f"   B   index_add_ in torch     {med['B']:9.3f} ms ({min(t['B']):.3f} .. {max(t['B']):.3f})   calls per window {inner['B']};  B / A = {med['B'] / med['A']:.2f}, "
            f"B - A = {(med['B'] - med['A']) / max(spread_b, 1e-9):+.1f} spreads of B")
        del plan, x, ei, a0, a1, b0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
