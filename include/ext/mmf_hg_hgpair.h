/* mmf_hg_hgpair.h — hypergraph propagation with one weight per (node, hyperedge) pair, and the softmax over the pairs of a
 * hyperedge or of a node.  Every builder of this library returns edge_index [2, E] and edge_weights [E], one weight
 * per column; mmf_hg_hgconv.h can use the first alone (as torch_geometric's HypergraphConv without attention does).  This header is
 * the operator underneath torch_geometric's attention mode — a value per pair multiplies the message in both gather steps, a
 * softmax over the pairs of a hyperedge (or of a node) produces that value — with gradients.  An addition to ABI version 3 of
 * mmf_hg.h, whose conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list
 * HGPAIR_EXPORTS of multimodal-fusion_amd/_lib.py.
 *
 * The pair plan.  Everything mmf_incidence_plan builds, with the same bits (eptr, emem, nptr, nmem, edge_scale, node_scale, status
 * int64 [2]; out-of-range pairs checked before they are keyed, left out of both CSRs, reported by lowest column), and two arrays
 * more: epos int32 [E] and npos int32 [E] hold, for every CSR slot, the column of edge_index that the slot came from.  The sort is
 * hipcub::DeviceRadixSort::SortPairs with the column as the value; it is stable, so the copies of a pair that occurs several times
 * sit in ascending column order — that order is part of the rule.  The slots past eptr[M] = nptr[N] hold 0 and are never visited.
 *
 * Propagation.  a = pair_weight f32 [E], indexed by column of edge_index; x f32 [N, C], rows `x_stride` >= C floats apart.
 *     Y_e   = (chain over the slots j of hyperedge e, in plan order, of (a[epos[j]] * x[emem[j], :])) * edge_scale_e
 *             with hyperedge weights, Y_e is then multiplied by w_e
 *     out_v = (chain over the slots j of node v of (a[npos[j]] * Y[nmem[j], :])) * node_scale_v
 * Bits.  Every product is a rounded f32 multiply, every sum a sequential f32 chain acc = 0; acc = acc + term — no fma, no tree, no
 * atomics on floats.  With a all ones the result is that of mmf_hypergraph_propagate, bit for bit, on finite normal inputs.
 * The scales are the caller's: the plan's own (Binv_e = 1 / B_e from the pair count, Dinv_v = 1 / D_v from w: torch_geometric's
 * attention-mode norm, "count"), or those of mmf_pair_scales (the real-valued incidence normalised by its own degrees, "weight"):
 *     B_e = chain of a[epos[j]] over the hyperedge's slots;   D_v = chain of (a[npos[j]] * w[nmem[j]]) over the node's slots (without
 *     w: of a[npos[j]]);   each scale 1.0f / that, 0 when the degree is 0.
 *
 * Gradients ("count" scales, which do not depend on a).  G = dL/dout [N, C], g' = node_scale . G (the caller's multiply):
 *     Z_e = chain of (a[epos[j]] * g'[emem[j], :]);  T_e = Z_e * edge_scale_e (* w_e);  grad_x_u = chain of (a[npos[j]] * T[nmem[j], :])
 *     — mmf_hypergraph_propagate_pairs with transpose != 0 on x = g' — and, for a valid column p = (v, e),
 *     grad_a[p] = dot64(g'_v, Y_e) + dot64(x_v, T_e)         (dot64: mmf_hg_readout.h; the sum one rounded add; other columns 0).
 *
 * Softmax over pairs.  ptr / pos are eptr / epos (group by hyperedge: normalise over the nodes of a hyperedge) or nptr / npos
 * (group by node).  For row r with its slots in plan order: m_r the exact maximum of score[pos[j]] (-0 < +0);
 * e_j = cexp(score[pos[j]] - m_r) with the cexp of mmf_hg_readout.h;  Z_r the sequential chain of e_j in slot order;
 * alpha[pos[j]] = e_j / Z_r;  columns in no CSR get 0.  cexp(0) == 1 gives Z_r >= 1: no "+ 1e-16".
 * Backward: c_r = chain of (alpha[pos[j]] * g[pos[j]]) in slot order;  grad_score[pos[j]] = alpha[pos[j]] * (g[pos[j]] - c_r).
 *
 * Limits: N, M, E and C < 2^31.  Every device entry enqueues on the caller's stream only, never synchronises with the host,
 * allocates nothing beyond the cached (device, stream) workspace, answers MMF_E_INVALID for NULL pointers, negative sizes and row
 * pitches below C and MMF_E_UNSUPPORTED for sizes of 2^31 or more, and starts its error message with the entry's name.
 */
#ifndef MMF_HG_HGPAIR_H
#define MMF_HG_HGPAIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The pair plan into the caller's arrays (sizes of the first six and status: mmf_incidence_plan_bytes; epos, npos int32 [E]).
 * Work: the keys of mmf_incidence_plan, one SortPairs per CSR over the bits in use with the column numbers 0 .. E - 1 as values,
 * the offsets by a bounds search, one pass that zeroes the positions of the pairs left out, one thread per row for the scales.
 * Workspace: 24 bytes per pair for the keys, 4 bytes per pair for the column numbers, plus the sort's temporary storage. */
int mmf_incidence_pair_plan(const int64_t* edge_index, int64_t num_pairs, int64_t num_nodes, int64_t num_edges, const float* hyperedge_weight,
                            int64_t* eptr, int32_t* emem, int32_t* epos, int64_t* nptr, int32_t* nmem, int32_t* npos, float* edge_scale,
                            float* node_scale, int64_t* status, int device_id, void* hip_stream);

/* The scales of the "weight" normalisation: edge_scale [M] = 1 / B_e, node_scale [N] = 1 / D_v as defined above, one thread per row.
 * pair_weight f32 [num_pairs]; hyperedge_weight f32 [M] or NULL.  No workspace. */
int mmf_pair_scales(const int64_t* eptr, const int32_t* epos, const int64_t* nptr, const int32_t* nmem, const int32_t* npos,
                    const float* pair_weight, const float* hyperedge_weight, int64_t num_nodes, int64_t num_edges, int64_t num_pairs,
                    float* edge_scale, float* node_scale, int device_id, void* hip_stream);

/* The two weighted gather-sums: Y [M, channels] (caller-provided, dense), out [N, channels] (dense).  edge_scale / node_scale: the
 * plan's or mmf_pair_scales'.  transpose != 0: the node step takes no scale (the caller passes x = node_scale . G), node_scale may
 * then be NULL; Y then holds T.  Pitches and bases that are multiples of four floats with channels % 4 == 0 take the float4
 * kernel, everything else the scalar one; the bits are the same.  No workspace. */
int mmf_hypergraph_propagate_pairs(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const int64_t* nptr, const int32_t* nmem,
                                   const int32_t* npos, const float* edge_scale, const float* node_scale, const float* hyperedge_weight,
                                   const float* pair_weight, int64_t num_pairs, const float* x, int64_t x_stride, int64_t num_nodes,
                                   int64_t num_edges, int64_t channels, float* Y, float* out, int transpose, int device_id, void* hip_stream);

/* grad_a [num_pairs] from g' [N, channels] (dense), x (rows x_stride apart), Y and T [M, channels] (dense): one wave per hyperedge
 * walks the row's slots and scatters through epos; grad_a is zeroed first (one memset).  No workspace. */
int mmf_pair_weight_grad(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const float* gprime, const float* x, int64_t x_stride,
                         const float* Y, const float* T, int64_t num_nodes, int64_t num_edges, int64_t channels, int64_t num_pairs,
                         float* grad_a, int device_id, void* hip_stream);

/* alpha [num_pairs] from score [num_pairs] over the rows of (ptr, pos) = (eptr, epos) or (nptr, npos): one memset, one launch, one
 * wave per row.  No workspace. */
int mmf_pair_softmax(const int64_t* ptr, const int32_t* pos, int64_t rows, int64_t num_pairs, const float* score, float* alpha,
                     int device_id, void* hip_stream);

/* grad_score [num_pairs] from the forward's alpha and grad_alpha [num_pairs]: one memset, one launch.  No workspace. */
int mmf_pair_softmax_backward(const int64_t* ptr, const int32_t* pos, int64_t rows, int64_t num_pairs, const float* alpha,
                              const float* grad_alpha, float* grad_score, int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_HGPAIR_H */
