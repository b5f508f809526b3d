/* mmf_hg_hg16.h — 16-bit activations for the hypergraph branch: the propagation of mmf_hg_hgconv.h, the
 * pair-weighted propagation and its weight gradient of mmf_hg_hgpair.h and the attention readout of mmf_hg_readout.h for x in f16 or
 * bf16 — what torch.autocast hands a layer.  Storage is 16-bit, arithmetic is f32: every operation here is the f32 rule of those
 * headers applied to the exactly widened operands, followed by ONE round-to-nearest-even per stored 16-bit tensor.  So every result
 * equals the f32 entry on widened operands with r16 at each store, bit for bit.  An addition to ABI version 3 of mmf_hg.h, whose
 * conventions hold (status codes, device pointers, `device_id`, `hip_stream`, mmf_last_error); bound from the list HG16_EXPORTS of
 * multimodal-fusion_amd/_lib.py.
 *
 * T is f16 or bf16: `dtype` = MMF_F16 / MMF_BF16 of mmf_hg.h.  MMF_F32 is refused (MMF_E_UNSUPPORTED) with a message that names the
 * f32 entry; any other value is MMF_E_INVALID.
 *   Widening.   f32(t) is exact.  For bf16 it is the bits shifted left by 16.
 *   Narrowing.  r16(f) is round-to-nearest-even of a finite f32.
 *       bf16, on the bits u of f, so that it does not move with the toolchain:   (u + 0x7fff + ((u >> 16) & 1)) >> 16
 *             (ties go to the even 16-bit pattern; the carry runs into the exponent and into infinity correctly).
 *       f16:  IEEE binary16, subnormals kept, overflow to infinity — numpy's astype(float16), torch's .to(float16).
 *   bf16 data that is 0 or has |x| >= 2^-100 keeps every f32 intermediate normal; f32 subnormals are outside the contract
 *   (DESIGN.md §3), as are non-finite values.
 *
 * Gather step.  mmf_csr_gather_sum with src and out of type T, an optional per-source-row scale, an optional pair operand and an
 * optional bias.  For row r with its slots j in [ptr[r], ptr[r + 1]) in order:
 *     t_j = f32(src[col[j], c]);   with src_scale: t_j = t_j * src_scale[col[j]];   with the pair operand: t_j = a[pos[j]] * t_j
 *           (each one rounded f32 multiply, in that order)
 *     acc = +0;  acc = acc + t_j  (the sequential f32 chain of mmf_hg_hgconv.h: no fma, no tree, no atomics)
 *     acc = acc * scale[r], then acc * scale2[r] (either may be NULL);  with bias f32 [C]: acc = acc + bias[c] (one rounded f32 add)
 *     out[r, c] = r16(acc)
 * A row without members writes r16 of (+0 times its scales, plus the bias if given).
 *
 * Propagation.  Y [M, C] is stored as T, rounded once; the node step reads the rounded Y; out [N, C] is stored as T, rounded once,
 * after the optional bias.  Chains, scales and their order are those of mmf_hg_hgconv.h (pair arrays NULL) and mmf_hg_hgpair.h.
 * transpose != 0: the node scale is not a pre-multiplied tensor — it is the src_scale of the hyperedge step, so the caller passes
 * G as it is; the node step takes no scale and no bias; Y then holds T_e rounded to T.
 *
 * Gradient in the pair weights ("count" scales).  grad_a[p] = dot64(g'_v, Y_e) + dot64(x_v, T_e) as in mmf_hg_hgpair.h with
 * g'_v[c] = f32(G[v, c]) * node_scale_v formed on the fly (one rounded multiply), G, Y_e, T_e and x_v widened from T, grad_a in f32.
 *
 * Readout.  x has type T; gate, out [S, C], alpha, seg_max, seg_sum, grad_gate and G = dL/dout stay f32.  The rule of
 * mmf_hg_readout.h runs on f32(x): out and alpha are bit for bit those of the f32 entry on the widened x.  grad_x has type T:
 * grad_x[i, c] = r16(alpha_i * G[s, c]).
 *
 * Limits: N, M, E, S, C and the chunk count < 2^31.  Every entry enqueues on the caller's stream only, never synchronises with the
 * host, allocates nothing beyond the cached (device, stream) workspace, answers MMF_E_INVALID for NULL pointers, negative sizes, row
 * pitches below C and an unknown dtype and MMF_E_UNSUPPORTED for sizes of 2^31 or more and for MMF_F32, and starts its error message
 * with the entry's name.
 */
#ifndef MMF_HG_HG16_H
#define MMF_HG_HG16_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The gather step.  src / out: rows of `channels` values of type T, `src_stride` / `out_stride` ELEMENTS apart.  pos / a: the pair
 * operand (both or neither); src_scale f32 by source row, scale / scale2 f32 by row, bias f32 [channels]: each may be NULL.  The ids
 * of col and pos are trusted: a plan's are in range by construction.  channels % 8 == 0 with both pitches multiples of 8 elements
 * and both bases 16-byte aligned takes the form where a lane owns 8 columns through one 16-byte access, everything else the one
 * where it owns 1 column; the bits are the same.  No workspace. */
int mmf_csr_gather_sum_16(const int64_t* ptr, const int32_t* col, const int32_t* pos, const float* a, int64_t rows, const void* src,
                          int64_t src_stride, int64_t channels, int dtype, const float* src_scale, const float* scale, const float* scale2,
                          const float* bias, void* out, int64_t out_stride, int device_id, void* hip_stream);

/* The two steps over a plan: Y [M, channels] and out [N, channels] of type T (caller-provided, dense).  pair_weight NULL: the plain
 * propagation of mmf_hypergraph_propagate (epos / npos are not read); otherwise that of mmf_hypergraph_propagate_pairs over
 * pair_weight f32 [num_pairs].  bias f32 [channels] or NULL enters `out` of the forward form only.  transpose != 0: x is G and
 * node_scale its src_scale (see above).  No workspace. */
int mmf_hypergraph_propagate_16(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const int64_t* nptr, const int32_t* nmem,
                                const int32_t* npos, const float* edge_scale, const float* node_scale, const float* hyperedge_weight,
                                const float* pair_weight, int64_t num_pairs, const void* x, int64_t x_stride, int64_t num_nodes,
                                int64_t num_edges, int64_t channels, int dtype, const float* bias, void* Y, void* out, int transpose,
                                int device_id, void* hip_stream);

/* grad_a f32 [num_pairs] from G [N, channels] (dense, type T), node_scale f32 [N], x (type T, rows x_stride elements apart), Y and T
 * [M, channels] (dense, type T): one wave per hyperedge, as mmf_pair_weight_grad; grad_a is zeroed first (one memset).  No workspace. */
int mmf_pair_weight_grad_16(const int64_t* eptr, const int32_t* emem, const int32_t* epos, const void* G, const float* node_scale, const void* x,
                            int64_t x_stride, const void* Y, const void* T, int64_t num_nodes, int64_t num_edges, int64_t channels,
                            int64_t num_pairs, int dtype, float* grad_a, int device_id, void* hip_stream);

/* mmf_attention_readout for x of type T (rows x_stride elements apart); everything else as there, workspace included. */
int mmf_attention_readout_16(const void* x, int64_t x_stride, int dtype, const float* gate, const int64_t* ptr_dev, const int32_t* table_dev,
                             int64_t num_chunks, int64_t N, int64_t S, int64_t C, float* out, float* alpha, float* seg_max, float* seg_sum,
                             int device_id, void* hip_stream);

/* mmf_attention_readout_backward for x of type T: grad_x [N, C] (dense) has type T, grad_gate f32 [N] or NULL (x is then not read). */
int mmf_attention_readout_backward_16(const void* x, int64_t x_stride, int dtype, const float* alpha, const int64_t* ptr_dev,
                                      const int32_t* table_dev, int64_t num_chunks, const float* out, const float* grad_out, int64_t N, int64_t S,
                                      int64_t C, void* grad_x, float* grad_gate, int device_id, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_HG_HG16_H */
