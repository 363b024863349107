/*
 * pdivgnn.h — C ABI of libpdivgnn_hip.so, the MI355X (gfx950) implementation of
 * the P-DivGNN hot path: EncodeProcessDecode forward/backward
 * (gnn_local_stress/models.py:98-326) and the divergence-regularised loss
 * (scripts/gnn_train.py:41-92).
 *
 * The reference is pure Python over PyTorch ATen + torch_geometric; it has no
 * FFI of its own.  Each entry point below replaces the group of ATen/PyG ops
 * named in its comment (file:line of the reference call site).  The Python
 * mirror (p-div-gnn_amd/gnn_local_stress) binds them with ctypes; INTEGRATION.md
 * shows the binding a maintainer would add to the reference.
 *
 * Conventions (all entry points):
 *   - device pointers to fp32 / int32 arrays; latent tensors are row-major
 *     (rows x 128) fp32, natural feature order, 16-byte aligned;
 *   - `stream` is a hipStream_t passed as void* (0 = null stream);
 *   - kernels never allocate; partial-sum buffers are caller-provided, sized
 *     by pdg_max_blocks();
 *   - return 0 on success, otherwise a nonzero code; pdg_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - edges are in dst-sorted order (CSR over edge_index[1]); `src`/`dst` are
 *     the endpoints of each dst-sorted edge, `rowptr` the dst-CSR offsets.
 */
#ifndef PDIVGNN_H
#define PDIVGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDG_LATENT 128
#define PDG_OK 0
#define PDG_ERR_ARG 1
#define PDG_ERR_HIP 2

/* Graph-LayerNorm statistics of one call (torch_geometric LayerNorm, mode="graph", batch=None). */
typedef struct pdg_ln_stat {
  float mean;   /* mean over all rows x channels of the call */
  float den;    /* std_pop + eps (the forward divides by it) */
  float rstd;   /* 1 / den */
  float std_;   /* population std */
  double mean_d, std_d, count; /* fp64 copies and the element count M */
} pdg_ln_stat;

/* Backward scalars of one graph-LayerNorm call. */
typedef struct pdg_ln_bwd {
  float c1, c2;
  double S1, S2;
} pdg_ln_bwd;

/* ---------------------------------------------------------------- library */
const char* pdg_last_error(void);
int pdg_version(void);
/* Hash of the sources the library was built from (16 hex digits; build.py). */
const char* pdg_source_hash(void);
/* Upper bound on the number of per-block partials any launcher writes. */
int pdg_max_blocks(void);
/* Layout of the node pre-pass outputs P, Q (pdg_node_pq_rw[_fin] writes it, pdg_edge_fwd_coop reads it):
 * 0 = two N x 128 row-major arrays; 1 = one N x 256 array whose rows hold, per 16-feature block b,
 * P[16b..16b+15] then Q[16b..16b+15], passed as P = base, Q = base + 16 floats. */
int pdg_pq_layout(void);

/* ---------------------------------------------------------------- forward */

/* models.py:140-152 (format_node_features) + :154-162, :303-307 (format_edge_features):
 * x_in[n] = [(mean_stress-mu)/s (3), (pos-mu)/s (2), node_type (1)]; e_in[k] = (edge_attr[perm[k]]-mu)/s.
 * stats8 = {mean_pos, std_pos, mean_mean_stress, std_mean_stress, mean_local_stress,
 *           std_local_stress, mean_edge_weight, std_edge_weight} (device, fp32). */
int pdg_format_inputs(int n_nodes, int n_edges, const float* pos, const float* mean_stress,
                      const int64_t* node_types, const float* edge_attr, const int* perm,
                      const float* stats8, int scale_input, float* x_in, float* e_in, void* stream);

/* The node encoder (models.py:260-274, 6 inputs) in the cooperative layout: a1 = relu(W0 x + b0) bitwise
 * pdg_encoder_fwd's (stored when a1 != NULL), a2 = relu(W2 a1 + b2) as an unbiased bf16x6 product from
 * registers, nblocks blocks of 512 threads (partials: nblocks (sum, sumsq) pairs).  x_in 8-byte aligned. */
int pdg_node_enc_fwd(int n_nodes, const float* x_in, const float* w0, const float* b0, const float* W2,
                     const float* b2, float* a1, float* a2, double* partials, int nblocks, void* stream);
/* Encoder MLP (models.py:260-274): a1 = relu(W0 x + b0) (K = in_features in {1..8}),
 * a2 = relu(W2 a1 + b2); writes a1, a2 and per-block LayerNorm partials (sum, sumsq). */
int pdg_encoder_fwd(int rows, int in_features, const float* x_in, const float* W0, const float* b0,
                    const float* W2, const float* b2, float* a1, float* a2,
                    double* partials, int* nparts, void* stream);
/* (a1 == NULL: the layer-1 output is not stored; pdg_edge_enc_bwd recomputes it.) */

/* Reduce LayerNorm partials -> statistics (mean, std_pop + eps). */
int pdg_ln_finalize(const double* partials, int nparts, double count, pdg_ln_stat* out, void* stream);
/* Two pdg_ln_finalize calls with the same nparts and count in one launch (the message and
 * edge-update LayerNorms after pdg_edge_fwd); bit-identical to the two calls.  New in this
 * build: the reference has no separate statistics step (models.py:42-55 computes them inline). */
int pdg_ln_finalize2(const double* part_a, const double* part_b, int nparts, double count,
                     pdg_ln_stat* out_a, pdg_ln_stat* out_b, void* stream);
/* Exact data-parallel LayerNorm (optional "sync" DP mode): reduce the
 * per-block partials to out2 = {sum, sumsq} (device, 2 doubles) for an all-reduce over
 * ranks, then pdg_ln_finalize(out2, 1, global_count, ...).  New in this build: the
 * reference LayerNorm (models.py:42-55) runs on one device and needs no exchange. */
int pdg_ln_partials_sum(const double* partials, int nparts, double* out2, void* stream);

/* Processor node pre-pass (models.py:221/236 re-associated): x_t = LN(a2_prev) [+ x_res];
 * P = W1[:, 0:128] x_t, Q = W1[:, 128:256] x_t  (W1 = processor.edge_net.0.weight, 128 x 384). */
int pdg_node_pq(int n_nodes, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                const float* ln_b, const float* x_res, float* x_out, const float* W1,
                float* P, float* Q, void* stream);
/* Same result as pdg_node_pq (bitwise), with Wa/Wb held in registers by 8 compute waves and
 * the LN + residual rows staged by 4 loader waves (better for node-sized row counts). */
int pdg_node_pq_rw(int n_nodes, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                   const float* ln_b, const float* x_res, float* x_out, const float* W1, float* P,
                   float* Q, void* stream);
/* pdg_node_pq_rw with the node LayerNorm statistics of a2_prev folded in: every block reduces the
 * (sum, sumsq) partials of pdg_node_net itself in the pdg_ln_finalize order (bit-identical) and
 * block 0 stores them to st_out for the backward, replacing a separate pdg_ln_finalize launch.
 * New in this build (the reference computes the statistics inline, models.py:42-55). */
int pdg_node_pq_rw_fin(int n_nodes, const float* a2_prev, const double* partials, int nparts, double count,
                       pdg_ln_stat* st_out, const float* ln_g, const float* ln_b, const float* x_res,
                       float* x_out, const float* W1, float* P, float* Q, void* stream);

/* Fused edge pass of one message-passing step (models.py:215-222, :233-238).
 * with_edge_update == 0 skips the edge-update branch (the last step's e_S is never consumed,
 * models.py:316): a1e/a2e/part_e unused and may be NULL.
 * e_t = LN(a2_prev) [+ e_res]; C = W1[:, 256:384] e_t + b1;
 * message:  a1m = relu(C + P[dst] + Q[src]), a2m = relu(W2 a1m + b2)
 * edge upd: a1e = relu(C + P[src] + Q[dst]), a2e = relu(W2 a1e + b2)
 * writes e_t, a1m, a2m, a1e, a2e and LayerNorm partials of a2m and a2e.  a1m and a1e are only
 * needed by the backward: NULL skips storing them (inference). */
int pdg_edge_fwd(int n_edges, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                 const float* ln_b, const float* e_res, float* e_out, const int* src, const int* dst,
                 const float* P, const float* Q, const float* W1, const float* b1,
                 const float* W2, const float* b2, float* a1m, float* a2m, float* a1e, float* a2e,
                 double* part_m, double* part_e, int with_edge_update, int* nparts, void* stream);

/* PyG "add" aggregation (scatter_add_ at edge_index[1]) of LN-normalised rows:
 * out[v] = sum_{k in rowptr[v]..rowptr[v+1]} LN(rows[k]); st == NULL -> raw rows.
 * xhat_sum (nullable): sum_k (rows[k] - mean)/(std + eps), kept for the LayerNorm backward. */
int pdg_segment_sum(int n_nodes, const int* rowptr, const float* rows, const pdg_ln_stat* st,
                    const float* ln_g, const float* ln_b, float* out, float* xhat_sum, void* stream);
/* pdg_segment_sum with the message LayerNorm's statistics reduced in the kernel from the edge
 * forward's per-block (sum, sumsq) partials part_a (nparts pairs, count = rows x 128 elements), bitwise
 * pdg_ln_finalize's, stored to st_a; with part_b also the edge-update LayerNorm's, stored to st_b.
 * Replaces pdg_ln_finalize2 + pdg_segment_sum (one launch fewer per message-passing step). */
int pdg_segment_sum_fin(int n_nodes, const int* rowptr, const float* rows, const double* part_a,
                        const double* part_b, int nparts, double count, pdg_ln_stat* st_a, pdg_ln_stat* st_b,
                        const float* ln_g, const float* ln_b, float* out, float* xhat_sum, void* stream);

/* Processor.update first layer (models.py:240-243, :202-204):
 * a1n = relu(Wn1[:, 0:128] aggr + Wn1[:, 128:256] x + bn1). */
int pdg_node_mlp1(int n_nodes, const float* aggr, const float* x, const float* Wn1,
                  const float* bn1, float* a1n, void* stream);

/* Second MLP layer with LN partials: a2 = relu(W2 a1 + b2). */
int pdg_mlp2_fwd(int rows, const float* a1, const float* W2, const float* b2, float* a2,
                 double* partials, int* nparts, void* stream);

/* Fused node_net of one step (models.py:240-243): a1n = relu(Wn1 [aggr | x] + bn1),
 * a2n = relu(Wn2 a1n + bn2) and LayerNorm partials of a2n, in one pass with the weights held
 * in registers.  Bitwise the same a1n / a2n as pdg_node_mlp1 + pdg_mlp2_fwd.  a1n is only
 * needed by the backward and may be NULL. */
int pdg_node_net(int n_nodes, const float* aggr, const float* x, const float* Wn1, const float* bn1,
                 const float* Wn2, const float* bn2, float* a1n, float* a2n, double* partials,
                 int* nparts, void* stream);
/* Decoder (models.py:282-286, :316-321): x_S = LN(a2_prev) + x_res; a1d = relu(Wd1 x_S + bd1);
 * y = Wd2 a1d + bd2 (3 outputs); if scale_output: y = y * std_local_stress + mean_local_stress. */
int pdg_decoder_fwd(int n_nodes, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                    const float* ln_b, const float* x_res, float* x_out, const float* Wd1,
                    const float* bd1, float* a1d, const float* Wd2, const float* bd2,
                    const float* stats8, int scale_output, float* y, void* stream);
/* pdg_decoder_fwd with the last node LayerNorm's statistics folded in: every block reduces the
 * (sum, sumsq) partials of pdg_node_net in pdg_ln_finalize's order (bit-identical) and block 0
 * stores them to st_out for the backward, replacing a separate pdg_ln_finalize launch (as
 * pdg_node_pq_rw_fin does for the earlier steps). */
int pdg_decoder_fwd_fin(int n_nodes, const float* a2_prev, const double* partials, int nparts, double count,
                        pdg_ln_stat* st_out, const float* ln_g, const float* ln_b, const float* x_res,
                        float* x_out, const float* Wd1, const float* bd1, float* a1d, const float* Wd2,
                        const float* bd2, const float* stats8, int scale_output, float* y, void* stream);
/* The decoder in the cooperative layout (pdg_efwd.hip): x_out bitwise pdg_decoder_fwd's, Wd1 x_S as an
 * unbiased bf16x6 product from registers, a1d and y to fp32 rounding; partials != NULL: the statistics
 * reduced in-kernel as pdg_decoder_fwd_fin does (st unused), else st.  nblocks blocks of 512 threads. */
int pdg_decoder_fwd_coop(int n_nodes, const float* a2_prev, const pdg_ln_stat* st, const double* partials,
                         int nparts, double count, pdg_ln_stat* st_out, const float* ln_g, const float* ln_b,
                         const float* x_res, float* x_out, const float* Wd1, const float* bd1, float* a1d,
                         const float* Wd2, const float* bd2, const float* stats8, int scale_output, float* y,
                         int nblocks, void* stream);

/* torch.any(x != 0) into *flag (int, device). models.py:294 */
int pdg_any_nonzero(const float* x, int64_t n, int* flag, void* stream);

/* y[i] = 0 for every i < n unless *flag (device int) is set: the zero-stress guard of models.py:294-299
 * ("return zeros_like(mean_stress)") decided on the device, for a forward replayed from a HIP graph
 * (pdg/serve.py) where the reference's host-side torch.any would cost a synchronisation per call. */
int pdg_zero_unless(const int* flag, float* y, int64_t n, void* stream);

/* ---------------------------------------------------------------- backward */

/* Decoder backward: gz1d = (Wd2^T gy) * [a1d > 0]; gx = Wd1^T gz1d. */
int pdg_decoder_bwd(int n_nodes, const float* gy, const float* a1d, const float* Wd2,
                    const float* Wd1T, float* gz1d, float* gx, void* stream);

/* LayerNorm backward without finalize launches (every column-sum producer below): block b of a
 * producer emits its row of per-channel partials, partials[b] = [sum gy (128) | sum gy*xhat (128)]
 * (accumulate != 0: added to the row, so one buffer spans all message-passing steps and
 * pdg_ln_param_grads turns it into the LayerNorm weight / bias gradients once), and, when
 * pairs != NULL, pairs[2b..2b+1] = (sum_c g_c row_c, sum_c g_c row_{128+c}) with g = ln_g.  The
 * consumer kernels (pdg_node_bwd, pdg_edge_bwd(_w2), pdg_mlp2_bwd) take these pairs in place of
 * a finalized pdg_ln_bwd and reduce them themselves (S1, S2, c1 = S1/M, c2 = S2/(M std)).
 * With accumulate == 0 every one of the producer's blocks writes its row and its pair, zeros for a
 * block without rows, so neither buffer needs a fill and a consumer may reduce all nblocks pairs; with
 * accumulate != 0 the caller zeroes the accumulator once (the pairs are still written, never added).
 * New in this build: the reference's autograd computes these sums inside the LayerNorm backward
 * (models.py:199,207,265,273). */
/* Per-channel LayerNorm backward sums over rows: sum gy, sum gy*xhat (xhat from a2 and st);
 * gy row k = gy_rows[gidx ? gidx[k] : k]. Writes per-block partials (2 x 128 doubles each). */
int pdg_ln_colsum(int rows, const float* gy_rows, const int* gidx, const float* a2,
                  const pdg_ln_stat* st, double* partials, int* nparts, const float* ln_g,
                  double* pairs, int accumulate, void* stream);

/* Node-level form of pdg_ln_colsum for the message LayerNorm, whose upstream gradient is the
 * gathered gaggr[dst]: sum_k gy = sum_v deg_v gaggr[v], sum_k gy*xhat = sum_v gaggr[v]*xhat_sum[v]
 * (deg from rowptr, xhat_sum from pdg_segment_sum).  Same partial layout as pdg_ln_colsum. */
int pdg_ln_colsum_nodes(int n_nodes, const float* gaggr, const int* rowptr, const float* xhat_sum,
                        double* partials, int* nparts, const float* ln_g, double* pairs, int accumulate,
                        void* stream);

/* Reduce colsum partials: grad_b += sum gy, grad_g += sum gy*xhat, and the call's
 * backward scalars (S1 = sum g*gy, S2 = sum g*gy*xhat): the column sums of the LayerNorm
 * backward (PyG LayerNorm graph mode, models.py:199,207,265,273; autograd of its weight/bias).
 * One launch (a single 1024-thread block, fixed-order fp64 sums). */
int pdg_ln_colsum_finalize(const double* partials, int nparts, const float* ln_g,
                           const pdg_ln_stat* st, float* grad_g, float* grad_b, pdg_ln_bwd* out,
                           void* stream);
/* LayerNorm weight / bias gradients from producer accumulators (accumulate mode above): for
 * group i, grad_b[i][c] += sum over rows r < rows[i] of acc[i][r][c], grad_g[i][c] += ... [128 + c];
 * fixed order; ngroups <= 4 (node_net, edge_net, node encoder, edge encoder LayerNorms).
 * acc/rows/grad_g/grad_b are HOST arrays of device pointers. */
int pdg_ln_param_grads(int ngroups, const double* const* acc, const int* rows, float* const* grad_g,
                       float* const* grad_b, void* stream);

/* MLP tail backward (LN -> relu -> Linear2 -> relu): ga2 = LNbwd(gy); gz2 = ga2 * [a2 > 0];
 * gz1 = (W2^T gz2) * [a1 > 0].  gy row k = gy_rows[gidx ? gidx[k] : k]. */
int pdg_mlp2_bwd(int rows, const float* gy_rows, const int* gidx, const float* a2, const float* a1,
                 const pdg_ln_stat* st, const pdg_ln_bwd* lb, const float* ln_g, const float* W2T,
                 float* gz2, float* gz1, const double* lb_pairs, int lb_npairs, void* stream);

/* pdg_decoder_bwd in the block-cooperative layout (the Wd1^T product in bf16x6). With partials != NULL
 * it also forms pdg_ln_colsum's column partials / (S1, S2) pairs of gx for the LayerNorm with output
 * statistics ln_st over ln_a2 (one partial per block: *nparts = nblocks), as pdg_gemm_sum2_coop.
 * narrow_partials != NULL: also node_decoder.2's weight / bias gradient (models.py:316-321 backward,
 * pdg_wgrad_narrow(rows, a1d, gy, 3, ...)'s block partials, nblocks of them) for
 * pdg_wgrad_narrow_finalize(narrow_partials, nblocks, 3, 1, ...): one pass over a1d / gy fewer. */
int pdg_decoder_bwd_coop(int rows, const float* gy, const float* a1d, const float* Wd2, const float* Wd1T,
                         float* gz1d, float* gx, const float* ln_a2, const pdg_ln_stat* ln_st, double* partials,
                         const float* ln_g, double* pairs, int accumulate, double* narrow_partials, int nblocks,
                         void* stream);

/* pdg_mlp2_bwd (gidx = NULL) in the block-cooperative layout: the W2^T product in bf16x6 with W2^T
 * stationary in registers, whole-row access (the node encoder's backward).  x_narrow != NULL (rows x 6,
 * the encoder input): also the first layer's weight / bias gradient from gz1, as the block partials of
 * pdg_wgrad_narrow(rows, gz1, x_narrow, 6, ...) in narrow_partials (nblocks of them, for
 * pdg_wgrad_narrow_finalize(narrow_partials, nblocks, 6, 0, ...)); gz1 may then be NULL (not stored). */
int pdg_mlp2_bwd_coop(int rows, const float* gy, const float* a2, const float* a1, const pdg_ln_stat* st,
                      const pdg_ln_bwd* lb, const float* ln_g, const float* W2T, float* gz2, float* gz1,
                      const double* lb_pairs, int lb_npairs, const float* x_narrow, double* narrow_partials,
                      int nblocks, void* stream);

/* Fused node_net backward of one step (the work of pdg_mlp2_bwd + pdg_gemm_dual with
 * res0 = NULL, res1 = gy): gz2 = LN_bwd(gy) * [a2n > 0]; gz1 = (Wn2^T gz2) * [a1n > 0];
 * gaggr = Wn1a^T gz1; gx_part = Wn1b^T gz1 + gy.  Weights held in registers; bitwise the
 * results of the separate kernels. */
int pdg_node_bwd(int n_nodes, const float* gy, const float* a2n, const float* a1n, const pdg_ln_stat* st,
                 const pdg_ln_bwd* lb, const float* ln_g, const float* Wn2T, const float* Wn1aT,
                 const float* Wn1bT, float* gz2, float* gz1, float* gaggr, float* gx_part,
                 const double* lb_pairs, int lb_npairs, void* stream);
/* lb_pairs != NULL: the LayerNorm backward scalars come from a producer's pairs (see
 * pdg_ln_colsum) and lb is ignored. */

/* out0 = W0T in [+ res0]; out1 = W1T in [+ res1]  (two 128x128 products of one input). */
int pdg_gemm_dual(int rows, const float* in, const float* W0T, const float* W1T,
                  const float* res0, const float* res1, float* out0, float* out1, void* stream);

/* out = res + W0T in0 + W1T in1. */
int pdg_gemm_sum2(int rows, const float* in0, const float* in1, const float* W0T, const float* W1T,
                  const float* res, float* out, void* stream);
/* Same result as pdg_gemm_sum2 (bitwise), weights held in registers.  partials != NULL: also
 * the pdg_ln_colsum partials of the LayerNorm backward with upstream gradient `out` and input
 * ln_a2 / statistics ln_st (the node LayerNorm of the previous message-passing step, whose
 * output x_t = LN(a2n) + x_{t-1} receives this gradient), *nparts rows of 256 doubles. */
int pdg_gemm_sum2_rw(int rows, const float* in0, const float* in1, const float* W0T, const float* W1T,
                     const float* res, float* out, const float* ln_a2, const pdg_ln_stat* ln_st,
                     double* partials, int* nparts, const float* ln_g, double* pairs, int accumulate,
                     void* stream);

/* Fused edge backward of one step: both edge_net evaluations' LN/relu/Linear2 backward
 * (message: gy = gaggr[dst]; edge update: gy = ge_next), gC = gz1m + gz1e,
 * ge_out = ge_next + WcT gC.  Writes gz2m, gz1m, gz2e, gz1e, gC, ge_out.
 * ge_next == NULL: the edge-update branch had no consumer (last step): gz2e/gz1e are not
 * written, gC = gz1m, ge_out = WcT gC. */
/* Edge encoder forward (models.py:264-275, 1 -> 128 -> 128) in the block-cooperative layout: a2 =
 * relu(W2 relu(w0 e_in + b0) + b2) with the W2 product in bf16x6 (as pdg_edge_fwd's), and the
 * LayerNorm partials of a2 (nblocks pairs).  a1 is not stored (pdg_edge_enc_bwd recomputes it). */
int pdg_edge_enc_fwd(int n_edges, const float* e_in, const float* w0, const float* b0, const float* W2,
                     const float* b2, float* a2, double* partials, int nblocks, void* stream);
/* pdg_gemm_sum2_rw in the block-cooperative layout (nblocks blocks of 512 threads, contiguous row
 * ranges): out = W0T in0 + W1T in1 [+ res], both products in bf16x6 with the weights stationary in
 * registers; partials != NULL: the LayerNorm column partials and pairs as pdg_gemm_sum2_rw (nblocks
 * rows of 256 doubles). */
int pdg_gemm_sum2_coop(int rows, const float* in0, const float* in1, const float* W0T, const float* W1T,
                       const float* res, float* out, const float* ln_a2, const pdg_ln_stat* ln_st,
                       double* partials, const float* ln_g, double* pairs, int accumulate, int nblocks,
                       void* stream);
/* pdg_node_bwd in the block-cooperative layout (nblocks blocks of 512 threads): the same outputs with
 * the three W^T products in bf16x6, weights stationary in registers. */
int pdg_node_bwd_coop(int n_nodes, const float* gy, const float* a2n, const float* a1n, const pdg_ln_stat* st,
                      const pdg_ln_bwd* lb, const float* ln_g, const float* Wn2T, const float* Wn1aT,
                      const float* Wn1bT, float* gz2, float* gz1, float* gaggr, float* gx_part,
                      const double* lb_pairs, int lb_npairs, int nblocks, void* stream);
/* pdg_edge_fwd in the block-cooperative layout (pdg_efwd.hip): nblocks blocks of 512 threads, one
 * contiguous row range each, Wc and W2 stationary in registers as bf16 terms, whole-row HBM access.
 * Same outputs to fp32 rounding (e_t bitwise; C = Wc e and the W2 products as unbiased bf16x6
 * products); part_m / part_e get nblocks partials.  P and Q in the pdg_pq_layout() layout (what
 * pdg_node_pq_rw[_fin] writes; pdg_edge_fwd takes two N x 128 arrays). */
int pdg_edge_fwd_coop(int n_edges, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                      const float* ln_b, const float* e_res, float* e_out, const int* src, const int* dst,
                      const float* P, const float* Q, const float* W1, const float* b1, const float* W2,
                      const float* b2, float* a1m, float* a2m, float* a1e, float* a2e, double* part_m,
                      double* part_e, int with_edge_update, int nblocks, void* stream);
/* Inference edge forward (no layer-1 outputs: nothing reads them without a backward): pdg_edge_fwd_coop's
 * e_out, a2m, a2e (bitwise) and LayerNorm partials (the rows added in another order) from 16-row rounds with
 * one barrier per round -- the C product of round k beside the two W2 products of round k - 1, the gathers
 * one round ahead, two register sets of row loads (pdg_efwd.hip).  Arguments as pdg_edge_fwd_coop's without
 * a1m / a1e. */
int pdg_edge_fwd_infer(int n_edges, const float* a2_prev, const pdg_ln_stat* st, const float* ln_g,
                       const float* ln_b, const float* e_res, float* e_out, const int* src, const int* dst,
                       const float* P, const float* Q, const float* W1, const float* b1, const float* W2,
                       const float* b2, float* a2m, float* a2e, double* part_m, double* part_e,
                       int with_edge_update, int nblocks, void* stream);
int pdg_edge_bwd(int n_edges, const int* dst, const float* gaggr, const float* ge_next,
                 const float* a2m, const float* a1m, const float* a2e, const float* a1e,
                 const pdg_ln_stat* st_m, const pdg_ln_stat* st_e, const pdg_ln_bwd* lb_m,
                 const pdg_ln_bwd* lb_e, const float* ln_g, const float* W2T, const float* WcT,
                 float* gz2m, float* gz1m, float* gz2e, float* gz1e, float* gC, float* ge_out,
                 const double* pairs_m, int npairs_m, const double* pairs_e, int npairs_e, void* stream);

/* Edge backward with the shared-weight gradients fused (pdg_ebw.hip), replacing
 * pdg_edge_bwd + the W2 / Wc passes of pdg_wgrad_segments (gnn_local_stress/models.py:194-208,
 * backward).  Weights stationary in registers, 32-row operand images in LDS; one block per
 * slab, `nslabs` blocks (the same value for every call of a backward pass: the block ->
 * slab map is fixed and the slabs accumulate, reduced once by pdg_wgrad_reduce).
 *   pdg_edge_bwd_w2:  gz1m/gz1e/gC as pdg_edge_bwd; slabs += gz2m^T a1m + gz2e^T a1e and the
 *                     b2 column sums (slab_init != 0: slabs = ..., the first call of a backward,
 *                     so the slabs need no zero fill; the same for pdg_edge_gout_wc and
 *                     pdg_edge_enc_bwd); gz2m/gz2e are not
 *                     materialised.  ge_next == NULL: message branch only, gC = gz1m (gC may
 *                     then be the gz1m pointer itself: written once).  gz1e may be NULL with
 *                     the edge update: it is then not stored (pdg_pq_scatter_bwd with
 *                     e_is_sum forms it from gC - gz1m).
 *   pdg_edge_gout_wc: ge_out = [ge_next +] WcT gC; slabs += gC^T e and the b1 column sums.
 *                     a2ln != NULL: also the column sums of the backward of the LayerNorm that
 *                     produced e (input a2ln, statistics st_ln, upstream gradient ge_out), as
 *                     pdg_ln_colsum partials: nslabs rows of 256 doubles in ln_partials (one
 *                     spare row after them for pdg_ln_colsum_finalize). */
int pdg_edge_bwd_w2(int n_edges, const int* dst, const float* gaggr, const float* ge_next,
                    const float* a2m, const float* a1m, const float* a2e, const float* a1e,
                    const pdg_ln_stat* st_m, const pdg_ln_stat* st_e, const pdg_ln_bwd* lb_m,
                    const pdg_ln_bwd* lb_e, const float* ln_g, const float* W2T, float* gz1m,
                    float* gz1e, float* gC, float* slabs, int nslabs, const double* pairs_m, int npairs_m,
                    const double* pairs_e, int npairs_e, int slab_init, void* stream);
/* Edge encoder backward (models.py:268-274), fused: gz2 = LN_bwd(gy) [a2 > 0], slabs (zeroed
 * before, pdg_wgrad_reduce layout) += gz2^T a1 and the b2 sums, gz1 = (W2T gz2) [a1 > 0], and per
 * block narrow_sums[b] = (sum gz1 e_in, sum gz1) as 2 x 128 doubles; a1 = relu(w0 e_in + b0) is
 * recomputed (pdg_encoder_fwd may skip storing it).  Replaces pdg_mlp2_bwd + the edge encoder's
 * pdg_wgrad_segments and pdg_wgrad_narrow passes.  lb / lb_pairs as pdg_mlp2_bwd.  Computed (default)
 * as M = (gz2 e)^T mask and N = gz2^T mask with mask = [a1 > 0]: slab += w0 M + b0 N,
 * narrow_sums = (sum_j W2[j][k] M[j][k], sum_j W2[j][k] N[j][k]) -- the same sums regrouped. */
int pdg_edge_enc_bwd(int n_edges, const float* gy, const float* a2, const float* e_in, const float* w0,
                     const float* b0, const pdg_ln_stat* st, const pdg_ln_bwd* lb, const double* lb_pairs,
                     int lb_npairs, const float* ln_g, const float* W2T, float* slabs, double* narrow_sums,
                     int nslabs, int slab_init, void* stream);
/* Input gradients of the encoders (pdg_ingrad.hip): the vector-Jacobian product of the forward with respect
 * to the mesh inputs, one product past where pdg_edge_enc_bwd / pdg_mlp2_bwd_coop stop.  Both take the
 * operands of those calls (gy = d loss / d e_0 or x_0, a2, st, lb / lb_pairs, ln_g, W2T) and form, per row,
 *   gz2 = LN_bwd(gy) [a2 > 0],  u = W2T gz2,  g_in[c] = sum_j W0[j][c] [a1[j] > 0] u[j]
 * (models.py:260-274 backwards, the W2T product in bf16x6), then undo the input formatting of
 * pdg_format_inputs (models.py:140-162; stats8 and scale_input as there: / std when scale_input).
 * nblocks blocks of 512 threads, contiguous row ranges; deterministic, no scratch.
 *   pdg_edge_enc_gin: a1 = w0 e_in + b0 recomputed from the scalar input (plan order);
 *                     g_edge_attr[perm[k]] = g_in of plan row k (the caller's edge order, n_edges floats).
 *   pdg_node_enc_gin: a1 as stored by the forward, W0 = node_encoder.0.weight (128 x 6); columns 0-2 go to
 *                     g_mean_stress (n_nodes x 3), 3-4 to g_pos (n_nodes x 2); column 5 (the integer
 *                     node type) gets no gradient. */
int pdg_edge_enc_gin(int n_edges, const float* gy, const float* a2, const float* e_in, const float* w0,
                     const float* b0, const pdg_ln_stat* st, const pdg_ln_bwd* lb, const double* lb_pairs,
                     int lb_npairs, const float* ln_g, const float* W2T, const int* perm, const float* stats8,
                     int scale_input, float* g_edge_attr, int nblocks, void* stream);
int pdg_node_enc_gin(int n_nodes, const float* gy, const float* a2, const float* a1, const float* W0,
                     const pdg_ln_stat* st, const pdg_ln_bwd* lb, const double* lb_pairs, int lb_npairs,
                     const float* ln_g, const float* W2T, const float* stats8, int scale_input,
                     float* g_mean_stress, float* g_pos, int nblocks, void* stream);
/* out[g][c] = sum of rows[ptr[g] .. ptr[g + 1])[c], c < 3: the gradient with respect to a graph's imposed
 * mean stress when it is broadcast to every node (benchmark_gnn_fem.py:404-407) from the per-node
 * g_mean_stress.  One block per graph, fp64 in a fixed order, rounded once; an empty graph gets zeros. */
int pdg_graph_colsum3(int n_graphs, const int* ptr, const float* rows, float* out, void* stream);
/* ---------------------------------------------------------------- tangent pass (pdg_tangent.hip)
 * The Jacobian-vector product of the forward with respect to the formatted inputs, (dx_in (N x 6), de_in (E))
 * -> d local_stress (N x 3), linearised at the activations a need_grad forward keeps: biases drop out, a relu
 * is a multiplication by the stored mask [a > 0], residuals add the previous tangent, and a graph LayerNorm
 * y = g (a - mu) / (sigma + eps) + b over n = rows x 128 elements becomes
 *   dLN = g ((da - T1 / n) / (sigma + eps) - (a - mu) T2 / (n sigma (sigma + eps)^2)),
 *   T1 = sum da, T2 = sum (a - mu) da over all n elements.
 * Every kernel that produces a pre-LayerNorm tangent da writes nblocks fp64 pairs (T1, T2) (`partials`, one per
 * block, every entry written); its consumer takes them as `pairs` / `npairs` (16-byte aligned) with the
 * LayerNorm's forward statistics `st` and reduces them itself in a fixed order: no atomics, no launch in
 * between, bitwise reproducible.  All 128 x 128 products are unbiased bf16x6 MFMA products.  nblocks blocks of
 * 512 threads over contiguous row ranges, 1 .. pdg_max_blocks(); rows per call below 2^22; launches only
 * (no allocation, no synchronisation, capturable).  Weights are the nn.Linear (out x in) arrays of the forward.
 *
 *   pdg_node_enc_tan   da2 = [a2 > 0] W2 [a1 > 0] W0 dx_in          (W0 128 x 6; a1, a2 as stored)
 *   pdg_edge_enc_tan   da2 = [a2 > 0] W2 [w0 e_in + b0 > 0] w0 de_in (the first layer's sign recomputed as
 *                      fma(w0, e_in, 0) + b0 > 0, pdg_edge_enc_bwd's form); plan order
 *   pdg_node_pre_tan   dx_out = dLN(da2_prev) [+ dx_res], dP = Wa dx_out, dQ = Wb dx_out (W1 = edge_net.0's
 *                      128 x 384 weight; dP, dQ plain N x 128 arrays)
 *   pdg_edge_tan       de_out = dLN(da2_prev) [+ de_res], C = Wc de_out;
 *                      da2m = [a2m > 0] W2 [a1m > 0] (C + dP[dst] + dQ[src]), part_m;
 *                      with_edge_update: da2e = [a2e > 0] W2 [a1e > 0] (C + dP[src] + dQ[dst]), part_e
 *                      (st_m / st_e: the forward statistics of a2m / a2e; endpoints clamped to n_nodes)
 *   pdg_segment_sum_tan daggr[n] = g sum_{k in rowptr[n] .. rowptr[n + 1])} dLN(da2m[k]) without the weight,
 *                      in edge order
 *   pdg_node_net_tan   da2n = [a2n > 0] W2 [a1n > 0] (W1[:, :128] daggr + W1[:, 128:] dx)   (W1 128 x 256)
 *   pdg_decoder_tan    dy = Wd2 [a1d > 0] Wd1 (dLN(da2_prev) [+ dx_res]) [* std_out[0], the output's
 *                      standard deviation (one float), with scale_output]
 *   pdg_edge_len_tan   dlen[k] = (pos[s] - pos[d]) . (dpos[s] - dpos[d]) / edge_attr[k] where edge_attr[k] > 0
 *                      and both endpoints lie in 0 .. n_nodes - 1, else 0 (periodic pairs, coincident nodes:
 *                      a constant length 0); s, d = src[k], dst[k] in the caller's edge order; fp64, rounded once. */
int pdg_node_enc_tan(int n_nodes, const float* dx_in, const float* a1, const float* W0, const float* W2,
                     const float* a2, const pdg_ln_stat* st, float* da2, double* partials, int nblocks,
                     void* stream);
int pdg_edge_enc_tan(int n_edges, const float* de_in, const float* e_in, const float* w0, const float* b0,
                     const float* W2, const float* a2, const pdg_ln_stat* st, float* da2, double* partials,
                     int nblocks, void* stream);
int pdg_node_pre_tan(int n_nodes, const float* da2_prev, const float* a2_prev, const pdg_ln_stat* st,
                     const double* pairs, int npairs, const float* ln_g, const float* dx_res, float* dx_out,
                     const float* W1, float* dP, float* dQ, int nblocks, void* stream);
int pdg_edge_tan(int n_edges, int n_nodes, const float* da2_prev, const float* a2_prev, const pdg_ln_stat* st,
                 const double* pairs, int npairs, const float* ln_g, const float* de_res, float* de_out,
                 const int* src, const int* dst, const float* dP, const float* dQ, const float* W1, const float* W2,
                 const float* a1m, const float* a2m, const pdg_ln_stat* st_m, const float* a1e, const float* a2e,
                 const pdg_ln_stat* st_e, float* da2m, float* da2e, double* part_m, double* part_e,
                 int with_edge_update, int nblocks, void* stream);
int pdg_segment_sum_tan(int n_nodes, int n_edges, const int* rowptr, const float* da2m, const float* a2m,
                        const pdg_ln_stat* st, const double* pairs, int npairs, const float* ln_g, float* daggr,
                        int nblocks, void* stream);
int pdg_node_net_tan(int n_nodes, const float* daggr, const float* dx, const float* W1, const float* W2,
                     const float* a1n, const float* a2n, const pdg_ln_stat* st, float* da2n, double* partials,
                     int nblocks, void* stream);
int pdg_decoder_tan(int n_nodes, const float* da2_prev, const float* a2_prev, const pdg_ln_stat* st,
                    const double* pairs, int npairs, const float* ln_g, const float* dx_res, const float* Wd1,
                    const float* a1d, const float* Wd2, const float* std_out, int scale_output, float* dy,
                    int nblocks, void* stream);
int pdg_edge_len_tan(int n_edges, int n_nodes, const int64_t* src, const int64_t* dst, const float* pos,
                     const float* dpos, const float* edge_attr, float* dlen, void* stream);
/* grad_w0 += sum_b narrow_sums[b][0:128], grad_b0 += sum_b narrow_sums[b][128:256] (block order). */
int pdg_enc_narrow_reduce(const double* narrow_sums, int nslabs, float* grad_w0, float* grad_b0, void* stream);
int pdg_edge_gout_wc(int n_edges, const float* gC, const float* e, const float* ge_next,
                     const float* WcT, float* ge_out, float* slabs, int nslabs, const float* a2ln,
                     const pdg_ln_stat* st_ln, double* ln_partials, const float* ln_g, double* pairs,
                     int accumulate, int slab_init, void* stream);

/* Mesh graph on the device (pdg_graph.hip): FaceToEdge of a triangle
 * mesh (convert_utils.py:47-60), edge lengths (datasets.py:182-188) and, when `periodic`,
 * compute_periodic_graph (datasets.py:39-119), coalesced (rows ascending, columns ascending
 * within a row; attribute = the length for a mesh edge, 0 for a periodic-only pair).
 * points: (n_nodes, dim) fp32, dim 2 or 3 (sides from the first two coordinates); faces:
 * (n_faces, 3) int64.  Outputs edge_rows / edge_cols (int64) / edge_attr (fp32) of
 * `capacity` >= 6 n_faces (+ 4 PDG_SIDE_MAX + 4 when periodic) entries; *n_edges (device
 * int) receives the edge count, or -1 for invalid periodic geometry (opposite sides of
 * different lengths, a corner that is not exactly one node, a side longer than
 * PDG_SIDE_MAX = 4096).  scratch: pdg_mesh_graph_scratch_bytes(n_nodes, n_faces) bytes. */
long pdg_mesh_graph_scratch_bytes(int n_nodes, int n_faces);
int pdg_mesh_graph(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                   int periodic, int64_t* edge_rows, int64_t* edge_cols, float* edge_attr,
                   long capacity, int* n_edges, void* scratch, long scratch_bytes, void* stream);
/* The same for faces of nv vertices, (n_faces, nv) int64: nv == 3 is pdg_mesh_graph, bitwise, with its
 * scratch size; nv == 4 is a quad mesh, whose edges are the four sides (f0,f1) (f1,f2) (f2,f3) (f0,f3)
 * of every quad and never a diagonal (convert_utils.py:63-81, _quad_face_to_edge).  `capacity` >=
 * 2 nv n_faces (+ 4 PDG_SIDE_MAX + 4 when periodic).  Any other nv is refused on the host (the size
 * function returns < 0).  Both calls: a face with an index outside [0, n_nodes) is never dereferenced;
 * its edges are dropped and *n_edges = -2 reports it. */
long pdg_mesh_graph_cells_scratch_bytes(int n_nodes, int n_faces, int nv);
int pdg_mesh_graph_cells(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                         int periodic, int64_t* edge_rows, int64_t* edge_cols, float* edge_attr,
                         long capacity, int* n_edges, void* scratch, long scratch_bytes, void* stream);

/* Backward of the P/Q gathers: gP[v] = sum_{dst-seg(v)} gz1m + sum_{src-seg(v)} gz1e,
 * gQ[v] = sum_{src-seg(v)} gz1m + sum_{dst-seg(v)} gz1e.  src-seg uses rowptr_src and
 * perm_src (positions of the dst-sorted edges grouped by src).  gz1e may be NULL (no
 * edge-update branch).  e_is_sum != 0: the gz1e argument holds gC = gz1m + gz1e instead and
 * each row's gz1e is formed as gC - gz1m in fp32 (the edge backward then stores no gz1e). */
int pdg_pq_scatter_bwd(int n_nodes, const int* rowptr_dst, const int* rowptr_src,
                       const int* perm_src, const float* gz1m, const float* gz1e, int e_is_sum,
                       float* gP, float* gQ, void* stream);

/* Weight gradient of a 128x128 Linear: per-block partial of sum_k G[k]^T X[k] (+ a second
 * pair G2/X2) and of sum_k G[k] (+G2); accumulated (+=) into slab[block] (128*128 + 128 floats),
 * so repeated calls over message-passing steps sum in a fixed order. */
int pdg_wgrad_accum(int rows, const float* G, const float* X, const float* G2, const float* X2,
                    float* slabs, int nslabs, void* stream);
/* grad_W[o*ld + col0 + i] += sum over slabs; grad_b[o] += (if grad_b) sum over slabs.
 * Two fixed-order passes; the slabs are scratch and are overwritten. */
int pdg_wgrad_reduce(float* slabs, int nslabs, float* grad_W, int ld, int col0,
                     float* grad_b, void* stream);
/* Weight gradient of a 128x128 Linear over a list of row segments (all message-passing steps
 * and both edge_net evaluations in one pass): slab[b] = per-block partial of
 * sum_seg sum_k G_seg[k]^T X_seg[k] and of sum G_seg[k] (written, not accumulated);
 * reduce with pdg_wgrad_reduce.  g_ptrs/x_ptrs/rows are HOST arrays of nseg <= PDG_MAX_SEGS entries. */
#define PDG_MAX_SEGS 32
/* Blocks per CU that pdg_wgrad_segments is built for (its nslabs should be this x the CU count). */
int pdg_wgrad_slabs_per_cu(void);
int pdg_wgrad_segments(int nseg, const float* const* g_ptrs, const float* const* x_ptrs, const int* rows,
                       float* slabs, int nslabs, void* stream);
/* Two weight gradients sharing an operand in one pass over nseg row segments (the shared array is
 * read once): shared_x != 0: slabs0 = A0^T A2, slabs1 = A1^T A2 (bias rows: column sums of A0 /
 * A1); shared_x == 0: slabs0 = A0^T A1, slabs1 = A0^T A2 (bias rows: column sums of A0 in both).
 * Block b writes slab b of both sets with its partial (written, not accumulated; a block without rows
 * writes zeros), nslabs each, reduced with pdg_wgrad_reduce.  Pointer and row arrays are HOST arrays
 * of nseg <= PDG_MAX_SEGS entries; a segment of 0 rows may carry NULL pointers. */
int pdg_wgrad_pairs(int nseg, const float* const* a0_ptrs, const float* const* a1_ptrs, const float* const* a2_ptrs,
                    const int* rows, int shared_x, float* slabs0, float* slabs1, int nslabs, void* stream);
/* Narrow weight gradient: T[c][i] = sum_k Wide[k][c] Narrow[k][i] (c < 128, i < k_narrow <= 8),
 * sums sum_k Wide[k][c] and sum_k Narrow[k][i]; added into grad arrays:
 * transpose == 0: grad_W[c*k_narrow + i] (shape 128 x k), else grad_W[i*128 + c] (k x 128);
 * grad_b_wide[c] += ..., grad_b_narrow[i] += ... (each nullable). */
int pdg_wgrad_narrow(int rows, const float* wide, const float* narrow, int k_narrow, int transpose,
                     double* partials, float* grad_W, float* grad_b_wide, float* grad_b_narrow,
                     void* stream);
/* The finalize step of pdg_wgrad_narrow alone (grad_W / grad_b_* += the reduced block partials, in
 * pdg_wgrad_narrow's order), for partials formed inside pdg_mlp2_bwd_coop / pdg_decoder_bwd_coop. */
int pdg_wgrad_narrow_finalize(const double* partials, int nparts, int k_narrow, int transpose, float* grad_W,
                              float* grad_b_wide, float* grad_b_narrow, void* stream);
/* Every end-of-backward reduction in one launch: n_reduce slab reductions as pdg_wgrad_reduce_batch
 * (<= 16), n_ln LayerNorm groups as pdg_ln_param_grads (<= 4), n_narrow (<= 2) narrow finalizes as
 * pdg_wgrad_narrow_finalize, and (enc_sums != NULL) the edge encoder's first-layer sums as
 * pdg_enc_narrow_reduce.  Bitwise the separate launches' gradients except the encoder sums, which add
 * their rows in another fixed order.  New in this build (the reference's autograd accumulates the
 * parameter gradients in place, gnn_train.py:160-161). */
int pdg_bwd_epilogue(int n_reduce, const float* const* slabs, const int* nslabs, float* const* grad_W,
                     const int* ld, const int* col0, float* const* grad_b, int n_ln, const double* const* ln_acc,
                     const int* ln_rows, float* const* ln_grad_g, float* const* ln_grad_b, int n_narrow,
                     const double* const* narrow_partials, const int* narrow_nparts, const int* narrow_k,
                     const int* narrow_transpose, float* const* narrow_gW, float* const* narrow_gb_wide,
                     float* const* narrow_gb_narrow, const double* enc_sums, int enc_nslabs, float* enc_grad_w0,
                     float* enc_grad_b0, void* stream);

/* ---------------------------------------------------------------- losses */

/* Per-graph normalised MSE (gnn_train.py:41-57) over node segments ptr[0..B]:
 * loss_g = mean_c sum_n (gt-pred)^2 / sum_n (gt - mean gt)^2.  Writes loss[g] and den[g*3+c]. */
int pdg_nmse_fwd(int n_graphs, const int* ptr, const float* gt, const float* pred,
                 float* loss, float* den, void* stream);
/* g_pred[n][c] (+)= scale * (-2/3) (gt-pred)/den_c. */
int pdg_nmse_bwd(int n_graphs, const int* ptr, int n_nodes, const float* gt, const float* pred,
                 const float* den, const float* scale, int accumulate, float* g_pred, void* stream);
/* pdg_nmse_fwd + pdg_nmse_bwd in one launch (bitwise the two): each graph's block also writes its
 * gradient rows from the denominators it just formed. */
int pdg_nmse_fwd_bwd(int n_graphs, const int* ptr, const float* gt, const float* pred, float* loss, float* den,
                     const float* scale, int accumulate, float* g_pred, void* stream);

/* Divergence penalty (gnn_train.py:60-92) with the operator in CSR over global rows and
 * graph-local columns (col < n_i: x-derivative, else y-derivative), ptr = node offsets:
 * div[v] = A_v . [[sxx;sxy],[sxy;syy]], rows with node_type +-1 zeroed, loss_g = mean_v |div|^2
 * (reduce_abs: mean_v |div|), summed over the two components.  The A arrays may hold entries with
 * col >= 2 n_g: they are ignored (gnn_train.py:74 slices them off); columns are never negative.  A graph
 * without nodes (ptr[g] == ptr[g+1]) gets loss[g] = NaN, as torch.mean of an empty tensor, and no row of
 * div is touched for it; nothing past row ptr[n_graphs] of div is written. */
int pdg_div_fwd(int n_graphs, const int* ptr, const int* a_rowptr, const int* a_col,
                const float* a_val, const int64_t* node_types, const float* sigma, int reduce_abs,
                float* div, float* loss, void* stream);
/* g_sigma (+)= A^T-weighted grads: uses A^T in CSR (at_rowptr over global nodes, at_row = source
 * row v, at_comp = 0/1 (x/y column block), at_val).  d loss_g / d div = 2 div / n_g ("square")
 * or sign(div) / n_g ("abs", sign(0) = 0), times *scale.  Unlike the A arrays, the A^T arrays must not
 * hold an entry with col >= 2 n_g (pdg_div_plan drops them): at_comp is all the kernel knows of the column.
 * Every row m < n_nodes is written (a node without A^T entries gets 0, or keeps its value when
 * accumulating); a graph without nodes owns no row and changes nothing. */
int pdg_div_bwd(int n_graphs, const int* ptr, int n_nodes, const int* at_rowptr, const int* at_row,
                const int* at_comp, const float* at_val, const float* div, const float* scale,
                int reduce_abs, int accumulate, float* g_sigma, void* stream);

/* ---------------------------------------------------------------- evaluation metrics */
/* The numbers of scripts/compare_results.py (main, lines 1098-1245), one workgroup per graph over
 * the node segments ptr[0..B], fp64 sums in a fixed order, kernel launches only (no memset, nothing
 * allocated: both calls can be captured).  A graph's values depend on its own rows and their position
 * inside the graph only, so it scores bitwise the same alone and inside any batch.  A graph without
 * nodes (ptr[g] == ptr[g+1]) gets NaN in its table row and no field row; nothing past row N of a
 * field is written.  n_graphs <= 0, a NULL ptr, table or required input (and std == 0) are refused on
 * the host before any launch.
 *
 * pdg_eval_nmse replaces normalized_mse_loss_single(reduce=False / True) (compare_results.py:333-348),
 * normalized_mse_loss_element_wise (:351-364), von_mises_stress (:713-726) and sklearn's r2_score as
 * main calls it (:1166-1204).  gt, pred: (N, 3) fp32 in xx, yy, xy order; every mean, difference and
 * square is formed in fp64 from them.  table: (B, 6) fp64 =
 *   nmse_xx, nmse_yy, nmse_xy   sum (gt - pred)^2 / sum (gt - mean gt)^2 per component,
 *   nmse                        the mean of the three,
 *   nmse_vm                     the same ratio on vm = sqrt(0.5 ((x-y)^2 + x^2 + y^2 + 6 xy^2)),
 *   r2                          1 - nmse: sklearn's r2_score(gt, pred) with uniform averaging whenever
 *                               the denominators are non-zero.  sklearn's special case for a zero
 *                               denominator (a constant gt column scores 0 or 1) is NOT reproduced:
 *                               a zero denominator gives the IEEE quotient (inf or NaN), as numpy does.
 * Optional outputs (each may be NULL), fp32 rounded once from fp64: err_field (N, 4; 16-byte aligned) =
 * (gt - pred)^2 / den_c for the three components and for von Mises; vm_gt, vm_pred (N). */
int pdg_eval_nmse(int n_graphs, const int* ptr, const float* gt, const float* pred, double* table,
                  float* err_field, float* vm_gt, float* vm_pred, void* stream);
/* pdg_eval_div replaces compute_divergence (compare_results.py:647-673) on a field and on its
 * standardised image (data_utils.standardize, compare_results.py:1081-1084, :1152-1155) and
 * compute_divergence_norm_field (:122-141) on both.  The operator is pdg_div_fwd's: CSR over global
 * rows with graph-local columns (col < n_g: x block; entries at or beyond 2 n_g are ignored).  One
 * walk over a row's entries forms div[v] = A_v . [[sxx;sxy],[sxy;syy]] on sigma and on
 * (sigma - mean) / std, each entry standardised, multiplied and summed in fp64 (the second is not the
 * first over std: the operator's row sums are not zero on boundary rows).  table: (B, 2) fp64 = the
 * divergence scalar of the raw and of the standardised field: rows with node_type +-1 zeroed,
 * |.| (reduce_abs) or the square, the mean over all n_g rows, summed over the two components.
 * norm, norm_std (N, each may be NULL): sqrt(dx^2 + dy^2) of the raw / standardised field with only
 * the node_type == +1 rows zeroed, fp32 rounded once. */
int pdg_eval_div(int n_graphs, const int* ptr, const int* a_rowptr, const int* a_col, const float* a_val,
                 const int64_t* node_types, const float* sigma, float mean, float std, int reduce_abs,
                 double* table, float* norm, float* norm_std, void* stream);

/* ---------------------------------------------------------------- stress criteria */
/* Failure criteria of a plane-stress field, their per-graph aggregates and the aggregates' gradients, built
 * like the evaluation metrics above: one workgroup per graph over the node segments ptr[0..B], fp64 arithmetic
 * from the fp32 inputs in a fixed order, kernel launches only (no float atomics, no memset, nothing allocated:
 * both calls can be captured), a graph's values bitwise the same alone and inside any batch.  sigma: (N, 3)
 * fp32 in xx, yy, xy order, unstandardised.  Per node, with m = (sx + sy) / 2, d = (sx - sy) / 2,
 * r = sqrt(d^2 + sxy^2), s1 = m + r, s2 = m - r:
 *   criterion 0  von Mises  sqrt(0.5 ((sx - sy)^2 + sx^2 + sy^2 + 6 sxy^2)) (datasets.py:82 of the reference);
 *                           gradient (2 sx - sy, 2 sy - sx, 6 sxy) / (2 vm), 0 where vm == 0;
 *   criterion 1  Tresca     max(2 r, |s1|, |s2|) (the out-of-plane principal stress is 0), the branch chosen in
 *                           that order, the first winning an exact tie; gradient of the chosen branch with
 *                           dr = (d / (2 r), -d / (2 r), sxy / r) (0 where r == 0), ds1,2 = (1/2, 1/2, 0) +- dr
 *                           and sign(0) = 0;
 *   criterion 2  Rankine    max(s1, 0); gradient ds1 where s1 > 0, else 0.
 * weights: (N) fp32 or NULL (1 everywhere).  A node takes part in its graph's aggregates if and only if its
 * weight is > 0 (0, negative and NaN weights exclude it: the weights are also the mask); W is the sum of the
 * participating weights.
 *
 * pdg_stress_criteria.  table: (B, 4) fp64 =
 *   max     M, the largest criterion value c over the participating nodes,
 *   mean    sum w c / W,
 *   pnorm   M (sum w (c / M)^p / W)^(1/p), 0 where M == 0 (scaled by M: no overflow for any finite c),
 *   ks      M + log(sum w exp(rho (c - M)) / W) / rho.
 * argmax: (B) int32, the graph-local index of the first participating node with c == M.  fields: NULL or (N, 6)
 * fp32, rounded once from fp64 = von Mises, s1, s2, r, the principal angle atan2(sxy, d) / 2, the chosen
 * criterion; written for every node of a non-empty graph, participating or not (scalar stores: no alignment
 * requirement).  A graph without nodes or without a participating node gets a NaN row and argmax -1 (no field
 * row is touched for an empty graph); so does a graph with a NaN criterion at a participating node.
 * n_graphs <= 0, a NULL ptr, sigma, table or argmax, a criterion outside 0..2, p < 1 or not finite and
 * rho <= 0 or not finite are refused on the host before any launch. */
int pdg_stress_criteria(int n_graphs, const int* ptr, const float* sigma, const float* weights, int criterion,
                        double p, double rho, double* table, int* argmax, float* fields, void* stream);
/* g_sigma (N, 3) fp32 = g_value[g] d J_g / d sigma(n), J the aggregate 0 max, 1 mean, 2 pnorm, 3 ks of the same
 * criterion, weights, p and rho; table and argmax as pdg_stress_criteria wrote them; g_value (B) fp32 or NULL
 * (ones).  d J / d c_n times the criterion's gradient above, with d J / d c_n =
 *   max     1 at argmax, 0 elsewhere (a subgradient where the maximum is attained more than once),
 *   mean    w / W,
 *   pnorm   (w / W) (c / J)^(p - 1), 0 where J == 0,
 *   ks      w exp(rho (c - M)) / sum w exp(rho (c - M)).
 * W and the ks sum are formed again here with one block sum (the table keeps its four columns).  A node that
 * takes no part gets an exact zero row, a graph whose argmax is -1 NaN rows at its participating nodes, an empty
 * graph nothing.  The host checks of pdg_stress_criteria, and a NULL g_sigma and an aggregate outside 0..3. */
int pdg_stress_criteria_bwd(int n_graphs, const int* ptr, const float* sigma, const float* weights, int criterion,
                            int aggregate, double p, double rho, const double* table, const int* argmax,
                            const float* g_value, float* g_sigma, void* stream);

/* ---------------------------------------------------------------- homogenisation */
/* Per-graph weighted integrals of a nodal field and the shift that makes its average equal a target
 * (pdg_homog.hip), built like the stress criteria above: segmented by ptr[0..B], fp64 arithmetic from the fp32
 * inputs in a fixed order, kernel launches only (no float atomics, no memset, nothing allocated: both calls can
 * be captured).  With the nodal areas of pdg_nodal_areas as weights, S / (cell area) is the reference's
 * mean_stress (integrate_field(sigma) / bounding_box.volume, scripts/generate_dataset.py:278-289) and S / W its
 * mean_stress_material (integrate_field(sigma) / integrate_field(1)).
 *
 * pdg_graph_wmean.  rows: (N, n_cols) fp32, 1 <= n_cols <= 9; weights: (N) fp32 or NULL (ones).  A row takes
 * part if and only if its weight is > 0 (the criteria's rule: 0, negative and NaN weights exclude it).  table:
 * (B, n_cols + 1) fp64 = W_g = sum w, then S_g,c = sum w rows[., c] over the participating rows.  One 1024-thread
 * workgroup per graph, thread t owning rows t, t + 1024, ... in that order and the block folded in a fixed
 * order: a graph gets bitwise the same row alone and inside any batch, and from call to call.  A graph without
 * rows or without a participating row gets zeros (its averages are then 0 / 0).  n_graphs <= 0, n_cols outside
 * 1..9 and a NULL ptr, rows or table are refused on the host before any launch. */
int pdg_graph_wmean(int n_graphs, const int* ptr, const float* rows, int n_cols, const float* weights,
                    double* table, void* stream);
/* out (N, 3) fp32 = sigma + shift_g with shift_g,c = (target[g, c] D_g - S_g,c) / W_g formed in fp64 and the sum
 * rounded once; table as pdg_graph_wmean wrote it for sigma with n_cols = 3; target: (B, 3) fp32; denom: (B)
 * fp64 = D_g, or NULL for D_g = W_g.  A constant shift c moves S / D by c W / D, so denom = the cell's area
 * makes the average over the cell (the mean_stress convention) equal the target and denom = NULL the average
 * over the material (mean_stress_material).  Every row of the graph is shifted, participating or not.  A graph
 * whose W is not > 0 gets a NaN shift, hence NaN rows: a plain result would hide that it has no average.  out
 * may alias sigma: an output element depends on its own input and its graph's table row only.  n_graphs <= 0
 * (or >= 2^27) and a NULL ptr, sigma, table, target or out are refused on the host before any launch. */
int pdg_mean_correct(int n_graphs, const int* ptr, const float* sigma, const double* table, const float* target,
                     const double* denom, float* out, void* stream);

/* ---------------------------------------------------------------- equilibration */
/* The hard correction for div sigma = 0 (pdg_equil.hip): the field closest to a given one among those whose
 * divergence vanishes at the interior nodes, and the transpose of that projection.  Per graph of n nodes, with
 * A = [Dx | Dy] exactly as pdg_div_fwd reads it (a_rowptr / a_col / a_val: CSR over global rows, graph-local
 * columns, entries with col >= 2 n ignored; at_rowptr / at_row / at_comp / at_val: the same entries by global node,
 * as pdg_div_plan writes both) and m_v = 1 where node_types[v] == 0, else 0:
 *   (C s)_x[v] = m_v sum_c (Dx[v,c] sxx[c] + Dy[v,c] sxy[c]),  (C s)_y[v] = m_v sum_c (Dx[v,c] sxy[c] + Dy[v,c] syy[c]).
 * The metric is |t|^2_W = sum_v w_v (txx^2 + tyy^2 + 2 txy^2), W = diag(w, w, 2 w) on (xx, yy, xy), w = weights
 * (N, fp32, e.g. the nodal areas of pdg_nodal_areas) or 1 when weights is NULL.  With S = C W^-1 C^T:
 *   transpose == 0:  S lam = C in,       out = in - W^-1 C^T lam    (P in: C out = 0, |out - in|_W least)
 *   transpose != 0:  S lam = C W^-1 in,  out = in - C^T lam         (P^T in, the vector-Jacobian product of P)
 * with (W^-1 C^T lam)_xx[c] = sum_v m_v Dx[v,c] lam_x[v] / w_c, _yy[c] = sum_v m_v Dy[v,c] lam_y[v] / w_c and
 * _xy[c] = sum_v m_v (Dy[v,c] lam_x[v] + Dx[v,c] lam_y[v]) / (2 w_c).  The system is solved by conjugate gradients
 * on S from lam = 0: vectors fp32, each row of a product accumulated in fp64 and rounded once, every inner product
 * an fp64 sum in a fixed order; it stops when the recurrence residual |r|_2 <= rtol |b|_2 (b the right-hand side),
 * after max_iter iterations, or when p^T S p is not > 0.  in, out: (N, 3) fp32 in xx, yy, xy order, unstandardised;
 * out is rounded once from fp64.  table: (B, 4) fp64 =
 *   0  |C in|_2 (transpose: |C W^-1 in|_2), formed in fp64;
 *   1  the true final residual |C out|_2 (transpose: |C W^-1 out|_2), recomputed in fp64 from the stored fp32 out
 *      by one more operator application after the loop;
 *   2  the iterations run;
 *   3  status bits: 1 the loop ended (max_iter, or p^T S p not > 0) before the recurrence residual fell to
 *      rtol table[g][0]; 2 the true residual exceeds 2 rtol table[g][0]; 4 a weight of the graph is <= 0 or not
 *      finite: out is then a bitwise copy of in, columns 0 and 1 are NaN and column 2 is 0.
 * A graph whose right-hand side is exactly zero (no interior node, no operator entry, in == 0) runs no iteration:
 * out is a bitwise copy of in and its row is (0, 0, 0, 0).  So is out whenever no iteration ran (max_iter == 0).
 * A graph without nodes gets NaN in its table row and no field row.  Built like the metrics and homogenisation
 * kernels: one persistent 1024-thread workgroup per graph, thread t owning rows t, t + 1024, ... in that order,
 * one kernel launch (no memset or copy node, nothing allocated, no host synchronisation: it can be captured), no
 * float atomics; a graph gets bitwise the same rows and table row alone and inside any batch, and from call to
 * call.  scratch holds pdg_equilibrate_scratch_bytes(n_nodes, n_graphs) bytes (11 floats a node; host arithmetic,
 * < 0 for n_nodes <= 0, n_graphs <= 0 or n_nodes >= 2^29); n_nodes = ptr[n_graphs].  Bad sizes, a NULL pointer
 * other than weights, rtol not finite and > 0, max_iter < 0, a short scratch and an out that overlaps in are
 * refused on the host before the launch. */
long pdg_equilibrate_scratch_bytes(int n_nodes, int n_graphs);
int pdg_equilibrate(int n_graphs, const int* ptr, int n_nodes, const int* a_rowptr, const int* a_col,
                    const float* a_val, const int* at_rowptr, const int* at_row, const int* at_comp,
                    const float* at_val, const int64_t* node_types, const float* weights, const float* in,
                    int transpose, float rtol, int max_iter, float* out, double* table, void* scratch,
                    long scratch_bytes, void* stream);

/* ---------------------------------------------------------------- utilities */
/* out (cols x rows, contiguous) = in^T for a (rows x cols) row-major matrix with row stride ld. */
int pdg_transpose(int rows, int cols, int ld, const float* in, float* out, void* stream);
/* n <= 16 transposes of 128 x 128 blocks in one launch: out_ptrs[i] (128 x 128, row-major) =
 * in_ptrs[i]^T, in_ptrs[i] with row stride lds[i]; host arrays. */
/* Up to 3 pdg_wgrad_segments passes in one launch: job j has nseg[j] segments (its entries of g_ptrs /
 * x_ptrs / rows follow job j-1's) and its own slab set slabs[j] (nslabs slabs each). */
int pdg_wgrad_segments_batch(int njobs, const int* nseg, const float* const* g_ptrs, const float* const* x_ptrs,
                             const int* rows, float* const* slabs, int nslabs, void* stream);
/* Several pdg_wgrad_reduce calls in one launch (njobs <= 16): job i adds the sum of its nslabs[i]
 * slabs into grad_W[i] (row stride ld[i], column offset col0[i]) and, when grad_b[i] != NULL,
 * the bias sums into grad_b[i].  Slab sets must be distinct buffers. */
int pdg_wgrad_reduce_batch(int njobs, const float* const* slabs, const int* nslabs, float* const* grad_W,
                           const int* ld, const int* col0, float* const* grad_b, void* stream);
int pdg_transpose128_batch(int n, const float* const* in_ptrs, const int* lds, float* const* out_ptrs, void* stream);
/* pdg_nonfinite + the zero-mean-stress skip in one launch, no memset: flags[2] double-buffered by call
 * parity; flags[parity] = any non-finite x[i] || (zero_flag && *zero_flag == 0), and flags[parity ^ 1] is
 * cleared for the next call (replaces GradScaler's inf check, gnn_train.py:205-207, and the guard of
 * models.py:294-299; pdg_adam then reads flags + parity as its skip flag). */
int pdg_nonfinite2(const float* x, int64_t n, const float* zero_flag, int* flags, int parity, void* stream);
/* The step's loss scalars (gnn_train.py:189-197) in one launch: out[0] = *zero_flag (1 when NULL),
 * out[1] = scale_nmse * sum_g loss_nmse[g], out[2] = scale_div * sum_g loss_div[g] (0 when loss_div is
 * NULL), out[3] = out[1] + out[2].  Each sum is formed in fp64 in a fixed order and rounded to fp32, then
 * multiplied by its scale in fp32 (a second rounding), and out[3] is the fp32 sum of the two products:
 * out[1] and out[2] are within 2 roundings of the exact scaled sums. */
int pdg_loss_reduce(int n_graphs, const float* loss_nmse, const float* loss_div, float scale_nmse,
                    float scale_div, const float* zero_flag, float* out, void* stream);
/* Adam as torch.optim.Adam (amsgrad=False, weight_decay=0) stepped by GradScaler.step
 * (gnn_train.py:111,118,204-207) on a flat parameter buffer.  Adam's step count lives on the
 * device: step_count[parity] = optimizer steps taken so far (c); the update uses
 * table[2c] = (float) lr / (1 - beta1^(c+1)) and table[2c+1] = (float) sqrt(1 - beta2^(c+1)), both
 * computed in double on the host as torch does, and writes step_count[parity ^ 1] = c + !skip.
 * When *skip_flag (nullable, device) is set nothing else changes: parameters, moments and the
 * step count stay as they were (GradScaler skips optimizer.step()).  w1 = (float)(1 - beta1),
 * w2 = (float)(1 - beta2) rounded from double.  Requires table_len > c. */
int pdg_adam(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
             const float* table, int table_len, float w1, float beta2, float w2, float eps,
             const int* skip_flag, int* step_count, int parity, void* stream);

/* ---------------------------------------------------------------- device-side collate (§8f row 1) */
/* One copy job: dst[i] = src[i] (+ add for the integer kinds), i < count.  `src`/`dst` are
 * device pointers; the job table itself lives in device memory (40 bytes per job). */
enum { PDG_COPY_F32 = 0, PDG_COPY_B32 = 1, PDG_COPY_B64 = 2 };
typedef struct pdg_copy_job {
  const void* src;
  void* dst;
  int64_t count;
  int64_t add;
  int32_t kind;
  int32_t pad_;
} pdg_copy_job;
/* Assemble a minibatch from HBM-resident graphs (PyG collate, gnn_train.py:387-394): runs all
 * jobs (njobs <= 65535, the largest count max_count) in one launch. */
int pdg_collate(const pdg_copy_job* jobs, int njobs, long max_count, void* stream);

/* Graph plan on the device (pdg_plan.hip): what pdg/plan.py builds with torch.sort / bincount /
 * searchsorted, without a host read.  Every array is device memory; scratch holds
 * pdg_graph_plan_scratch_bytes(n_nodes, n_edges, nnz) bytes (one allocation serves both calls;
 * < 0 for n_nodes <= 0, a negative count, n_edges or nnz >= 2^31, or n_nodes + 1024 >= 2^31).
 *
 * pdg_graph_plan: edge_src / edge_dst are the two int64 rows of edge_index, in any order, with
 * duplicates, self-loops and isolated nodes.  perm / src / dst (n_edges): the edges in stable
 * (dst, src) order, perm the original edge id; rowptr_dst (n_nodes + 1) over that order;
 * perm_src (n_edges): the stable (src, dst) order of those sorted edges; rowptr_src (n_nodes + 1).
 * *status (device int) is cleared, then set to 1 when an endpoint lies outside [0, n_nodes); such
 * an endpoint counts as node 0, so the outputs are a valid in-range plan either way.  The edge
 * arrays may be NULL when n_edges == 0.
 *
 * pdg_div_plan: the COO divergence operator (rows / cols int64, vals fp32, nnz entries in any
 * order) of a batch whose graph g owns the nodes ptr[g] .. ptr[g + 1] (ptr: n_graphs + 1 int32).
 * An entry of row r belongs to the graph g with ptr[g] <= r < ptr[g + 1] and is kept when
 * col < 2 N_g (gnn_train.py:74).  a_rowptr (n_nodes + 1) / a_col / a_val: the kept entries by row,
 * in entry order, graph-local columns; at_rowptr (n_nodes + 1) / at_row / at_comp / at_val: the
 * same entries by global node ptr[g] + (col mod N_g), at_comp = col >= N_g.  The entry arrays hold
 * nnz elements, of which the first a_rowptr[n_nodes] (= at_rowptr[n_nodes], the kept count) are
 * written; values are copied bit for bit.  An entry with a row outside [0, n_nodes), a negative
 * column or a node outside [0, n_nodes) sets *status and is dropped.  clear_status != 0 clears
 * *status first; 0 keeps what pdg_graph_plan left there. */
long pdg_graph_plan_scratch_bytes(int n_nodes, long n_edges, long nnz);
int pdg_graph_plan(int n_nodes, long n_edges, const int64_t* edge_src, const int64_t* edge_dst, int* perm,
                   int* src, int* dst, int* rowptr_dst, int* perm_src, int* rowptr_src, int* status,
                   void* scratch, long scratch_bytes, void* stream);
int pdg_div_plan(int n_nodes, int n_graphs, const int* ptr, long nnz, const int64_t* rows, const int64_t* cols,
                 const float* vals, int* a_rowptr, int* a_col, float* a_val, int* at_rowptr, int* at_row,
                 int* at_comp, float* at_val, int* status, int clear_status, void* scratch, long scratch_bytes,
                 void* stream);

/* Per-node fields of a bare triangle mesh on the device (pdg_meshfields.hip): the last host step of
 * the reference's convert_mesh_to_graph (benchmark_gnn_fem.py:388-415) and the operator of the
 * divergence check, with no host-side topology work.  points: (n_nodes, dim) fp32, dim 2 or 3 (only
 * x and y are used); faces: (n_faces, 3) int64 (may be NULL when n_faces == 0).  scratch holds
 * pdg_mesh_fields_scratch_bytes(n_nodes, n_faces) bytes (host arithmetic; one size serves both calls;
 * < 0 for n_nodes <= 0, n_faces < 0, n_nodes + 1024 >= 2^31 or 9 n_faces + 1024 >= 2^31).  Sizes, null
 * pointers, the scratch size and the capacity are checked on the host before any HIP call.  Kernel
 * launches only (no memset or copy node, no cooperative launch); the results do not depend on the
 * order in which the kernels' atomics land.
 *
 * pdg_node_labels: compute_node_labels (datasets.py:122-179).  A boundary edge is an undirected edge
 * of exactly one face (extract_feature_edges(boundary_edges=True)); a boundary node an endpoint of
 * one; the boundary nodes are grouped into connected components over the boundary edges.  A component
 * is external (labels +1) when one of its nodes lies on the bounding box: x equal to the smallest or
 * largest x, or y equal to the smallest or largest y, compared exactly in fp32 against the min / max
 * of the same array.  (The reference tests `coord in bounds_2d` over all four bounds, so it would
 * also accept x == ymin; comparing each coordinate with its own bounds only is deliberate.)  Every
 * other component is an internal boundary (-1); interior nodes and nodes of no face get 0.
 * info (3 device ints): info[0] = boundary components, info[1] = external ones, info[2] = status bits:
 *   1  a face holds an index outside [0, n_nodes): the face is ignored, the index never dereferenced;
 *   2  a boundary node has other than two boundary edges (non-manifold boundary; labels still written);
 *   4  the component search stopped at its iteration cap (boundary edges + 2 passes; never on a search
 *      that works as designed, since a pass moves a component's smallest id one edge further).
 *
 * pdg_p1_div_operator: the area-averaged P1 nodal divergence operator A = [Dx | Dy] (n_nodes x
 * 2 n_nodes) of pdg/meshgen.py p1_divergence_operator (the role of op_div_matrix, datasets.py:191-213):
 * per face det = (xb-xa)(yc-ya) - (xc-xa)(yb-ya), area = |det| / 2 and the P1 gradients gx, gy; row i
 * (a vertex of the face) receives area gx[vn] at column vn and area gy[vn] at column vn + n_nodes for
 * each vertex vn, divided by the node's summed incident area.  Output: COO sorted by (row, col),
 * duplicates summed, structural zeros kept (every key the host keeps); *nnz (device int) entries of
 * the `capacity` >= 18 n_faces provided.  Sums are fp64 in face-index order, rounded once to fp32.
 * *status (device int) bits: 1 a face has det == 0 (its contributions are skipped; the host function
 * divides by zero there), 2 a face index is out of range (the face is ignored).
 *
 * pdg_nodal_areas: the lumped nodal areas area[n] = sum over the faces f that hold n of area_f / 3, with
 * area_f = |det| / 2 and the det above, of pdg/meshgen.py nodal_areas.  For P1 triangles these are the
 * reference's quadrature weights gathered to the nodes, so area / cell area is its op_mean_stress
 * (scripts/generate_dataset.py:73-82).  The 3 n_faces (node, face) items are grouped by node and ordered by
 * face; a node's thread sums its terms in that order in fp64 and rounds once to fp32 (no float atomics: the
 * result does not depend on the order of the slot atomics).  A face that names a node twice gives it two
 * terms, a face of zero area contributes 0 and is no error, a node of no face gets exactly 0.  bbox: 4 fp32 =
 * (xmin, xmax, ymin, ymax) of all points, whether a face uses them or not.  *status (device int) bit 1: a
 * face index is out of range (the face is ignored, the index never dereferenced).  Scratch and host checks
 * as pdg_node_labels. */
long pdg_mesh_fields_scratch_bytes(int n_nodes, int n_faces);
int pdg_nodal_areas(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, float* area,
                    float* bbox, int* status, void* scratch, long scratch_bytes, void* stream);
int pdg_node_labels(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                    int64_t* labels, int* info, void* scratch, long scratch_bytes, void* stream);
int pdg_p1_div_operator(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces,
                        int64_t* rows, int64_t* cols, float* vals, long capacity, int* nnz, int* status,
                        void* scratch, long scratch_bytes, void* stream);
/* pdg_boundary_vectors: the lumped outward boundary vectors of pdg/meshgen.py boundary_vectors.  A boundary edge
 * is pdg_node_labels' (an undirected edge of exactly one face; the same device code finds them).  For the boundary
 * edge (a, b) of face (a, b, c), in the face's own vertex order, r = (yb - ya, -(xb - xa)) is formed in fp64 from
 * the fp32 coordinates and negated if r . (pc - pa) > 0: it then points out of the material, away from the third
 * vertex, whatever the face's orientation, and r = length * n_outward.  bvec (n_nodes, 2) fp32: bvec[n] = 1/2 sum
 * r_e, and blen (n_nodes) fp32: blen[n] = 1/2 sum |r_e|, over the boundary edges that hold n, each summed in fp64
 * in ascending order of the edge's other endpoint and rounded once (a manifold boundary node has two edges; no
 * float atomics: the result does not depend on the order of the slot atomics).  A node that is not on a boundary
 * edge gets exact zeros.  sigma(n) . bvec[n], that is fx = sxx mx + sxy my and fy = sxy mx + syy my, is the
 * nodal boundary force, the lumped traction integral.  *status (device int) bits:
 *   1  a face index is out of range: the face is ignored, the index never dereferenced;
 *   2  a boundary node has other than two boundary edges (outputs still written);
 *   4  a boundary edge belongs to a face of zero area (det == 0 with the det above): it adds its length to blen
 *      and nothing to bvec.
 * scratch holds pdg_boundary_vectors_scratch_bytes(n_nodes, n_faces) bytes, a size of its own (the endpoints of
 * up to 3 n_faces boundary edges are grouped a second time; pdg_mesh_fields_scratch_bytes is unchanged; < 0 under
 * the same conditions).  Sizes, null pointers and the scratch size are checked on the host before any HIP call;
 * kernel launches only, so the call can be captured. */
long pdg_boundary_vectors_scratch_bytes(int n_nodes, int n_faces);
int pdg_boundary_vectors(int n_nodes, const float* points, int dim, int n_faces, const int64_t* faces, float* bvec,
                         float* blen, int* status, void* scratch, long scratch_bytes, void* stream);

/* The mesh fields for faces of nv vertices, (n_faces, nv) int64 in the face's own vertex order (either
 * orientation): the same kernels as templates on nv.  nv == 3 gives bitwise what the calls above give, with
 * their scratch sizes; nv == 4 is a quad mesh (a, b, c, d), the restatements being pdg/meshgen.py's quad
 * branches.  Any other nv is refused on the host (the size functions return < 0), as are sizes with
 * nv^2 n_faces + 1024 >= 2^31.  Outputs, status bits, host checks and capture as for the calls above.  For a quad:
 *   edges     the four sides (a,b) (b,c) (c,d) (d,a), never a diagonal: a boundary edge is a side of one face;
 *   det       (xc-xa)(yd-yb) - (xd-xb)(yc-ya), the diagonals' cross product = 2 x the signed area; area = |det| / 2;
 *   operator  pdg_div_operator_cells, the Q1 counterpart of pdg_p1_div_operator with the face's mean Q1 gradients
 *             gx = (yb-yd, yc-ya, yd-yb, ya-yc) / det, gy = (xd-xb, xa-xc, xb-xd, xc-xa) / det: area g[vn] is the
 *             integral of grad N_vn over the face for the bilinear shape functions of any quad.  nv^2 (row, column
 *             node) pairs per face, so `capacity` >= 2 nv^2 n_faces (32 per quad); det == 0 is status bit 1;
 *   areas     area[n] = sum over the faces of the integral of N_n = (|det| + sgn(det) t_k) / 12 at the face's corner
 *             k, t_k = (x[k+1]-x[k])(y[k-1]-y[k]) - (y[k+1]-y[k])(x[k-1]-x[k]) (twice the signed corner triangle):
 *             area / 4 on a parallelogram, and what a 2 x 2 Gauss rule gathers to the nodes; det == 0 adds 0;
 *   vectors   the side (v_j, v_j+1) is oriented away from v_j+2; det == 0 is status bit 4. */
long pdg_mesh_fields_cells_scratch_bytes(int n_nodes, int n_faces, int nv);
int pdg_node_labels_cells(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                          int64_t* labels, int* info, void* scratch, long scratch_bytes, void* stream);
int pdg_div_operator_cells(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                           int64_t* rows, int64_t* cols, float* vals, long capacity, int* nnz, int* status,
                           void* scratch, long scratch_bytes, void* stream);
int pdg_nodal_areas_cells(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                          float* area, float* bbox, int* status, void* scratch, long scratch_bytes, void* stream);
long pdg_boundary_vectors_cells_scratch_bytes(int n_nodes, int n_faces, int nv);
int pdg_boundary_vectors_cells(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces,
                               float* bvec, float* blen, int* status, void* scratch, long scratch_bytes,
                               void* stream);

/* ---------------------------------------------------------------- boundary residuals */
/* What a plane-stress field does on the boundary of the periodic cell (pdg_boundary.hip), built like the
 * homogenisation above: segmented by ptr[0..B], fp64 arithmetic from the fp32 inputs in a fixed order, kernel
 * launches only (no atomics, no memset, nothing allocated: both calls can be captured).
 *
 * pdg_boundary_residuals.  sigma: (N, 3) fp32 in xx, yy, xy order; bvec (N, 2) and blen (N) as
 * pdg_boundary_vectors wrote them; labels: (N) int64, the +1 / -1 / 0 of nodes_types; rowptr_dst (N + 1 int32),
 * src (int32, dst-sorted) and perm (int32) of the graph plan (pdg_graph_plan) and edge_attr (fp32, original edge
 * order): the four edge arguments may all be NULL, the periodic columns are then 0.  With f(n) = sigma(n) .
 * bvec[n], a node takes part in the traction sums if and only if its label is +1 or -1 and blen[n] > 0 (the
 * criteria's rule: a zero, negative or NaN blen excludes it).  A periodic connection is an incoming edge of n (the
 * plan's dst-sorted lists) whose edge_attr is exactly 0; one whose source lies outside n's graph is not read.
 * table: (B, 9) fp64 =
 *   0     L_int = sum blen over the participating nodes labelled -1,
 *   1     L_ext = sum blen over the participating nodes labelled +1,
 *   2     T2 = sum over -1 of |f|^2 / blen, the integral of the squared traction over the hole's edge,
 *   3, 4  F_int = sum over -1 of f, the net force on the hole (0 for a traction-free hole),
 *   5, 6  F_ext = sum over +1 of f, the net force on the cell (0 for any periodic field in equilibrium),
 *   7     P2 = 1/2 sum_n sum over the periodic edges into n of |sigma(n) - sigma(src)|^2 (the plain sum of the
 *         three components),
 *   8     n_pairs = 1/2 the number of those edges.
 * argmax: (B) int32, the graph-local index of the first participating -1 node that attains the largest
 * |f| / blen; -1 when there is none, and -1 when a participating node of the graph has a NaN traction (a plain
 * maximum would hide the NaN, as in pdg_stress_criteria).  One 1024-thread workgroup per graph, thread t owning
 * rows t, t + 1024, ... in that order and the block folded in a fixed order: a graph gets bitwise the same row and
 * argmax alone and inside any batch, and from call to call.  A graph without rows gets zeros and argmax -1.
 * n_graphs <= 0, a NULL ptr, sigma, bvec, blen, labels, table or argmax, and partial edge arguments are refused
 * on the host before any launch.
 *
 * pdg_boundary_residuals_bwd.  out (N, 3) fp32 = the gradient with respect to sigma of
 *   sum_g g_traction[g] T2_g / L_int,g + g_periodic[g] P2_g / n_pairs,g,
 * the mean-square hole traction and the mean-square periodic jump; table as the forward wrote it; g_traction,
 * g_periodic: (B) fp64, either may be NULL (taken as 0).  Per row: at a participating -1 node
 * (2 / blen) (fx [mx, 0, my] + fy [0, my, mx]) times g_traction / L_int; at any node 2 sum over the periodic
 * edges into n of (sigma(n) - sigma(src)) times g_periodic / n_pairs.  Precondition: the periodic term is the
 * full gradient when the periodic connections appear in both directions, as compute_periodic_graph and
 * pdg_mesh_graph build them and coalesce keeps them.  Node-parallel and without atomics: a row depends on its own
 * inputs, its neighbours' sigma and its graph's table row.  Rows that take no part get exact zeros (a zero weight
 * switches its term off); a graph whose denominator is not > 0 under a non-zero weight gets NaN in that term's
 * participating rows (the NaN rule of the criteria and of pdg_mean_correct).  Each output is formed in fp64 and
 * rounded once.  n_graphs <= 0 (or >= 2^27), a NULL ptr, sigma, bvec, blen, labels, table or out, and partial
 * edge arguments are refused on the host before any launch. */
int pdg_boundary_residuals(int n_graphs, const int* ptr, const float* sigma, const float* bvec, const float* blen,
                           const int64_t* labels, const int* rowptr_dst, const int* src, const int* perm,
                           const float* edge_attr, double* table, int* argmax, void* stream);
int pdg_boundary_residuals_bwd(int n_graphs, const int* ptr, const float* sigma, const float* bvec,
                               const float* blen, const int64_t* labels, const int* rowptr_dst, const int* src,
                               const int* perm, const float* edge_attr, const double* table,
                               const double* g_traction, const double* g_periodic, float* out, void* stream);

/* ---------------------------------------------------------------- fused physics loss (training) */
/* The hole traction, the periodic jump and the mean-consistency defect as training penalties on the trainer's
 * STANDARDISED prediction (pdg_physloss.hip), built like the diagnostics above: segmented by ptr[0..B], fp64
 * arithmetic from the fp32 inputs in a fixed order, kernel launches only (no atomics, no memset, nothing
 * allocated: every call can be captured).
 *
 * y: (N, 3) fp32, the standardised prediction; affine: two fp32 values on the device, (std, mean) of the local
 * stress.  Every term is evaluated on z = y + mean / std formed in fp64 (= sigma / std: units of the dataset's
 * standard deviation, dz / dy = 1).  Three argument groups, each given together or all NULL (a NULL group makes
 * its term absent for every graph, a partial group is refused):
 *   bvec (N, 2), blen (N), labels (N int64)          as pdg_boundary_residuals takes them,
 *   rowptr_dst, src, perm, edge_attr                 as pdg_boundary_residuals takes them,
 *   area (N fp32), target (B, 3 fp32)                the nodal areas of pdg_nodal_areas and each graph's imposed
 *                                                    mean stress, unstandardised (the kernel forms target / std);
 *   denom (B fp64) goes with the last group and may be NULL.
 *
 * pdg_phys_loss_fwd.  table: (B, 12) fp64 =
 *   0      L_int, 1 T2, 2 P2, 3 n_pairs   as pdg_boundary_residuals defines them, on z,
 *   4      W, 5..7 S_xx, S_yy, S_xy       as pdg_graph_wmean defines them, on z with area as weights,
 *   8      D = denom[g], or W when denom is NULL (the "material" convention); 0 without the mean group,
 *   9      traction loss T2 / L_int,
 *   10     periodic loss P2 / n_pairs,
 *   11     mean loss sum_c (S_c / D - target[g, c] / std)^2.
 * loss: (B, 3) fp32 = columns 9..11 rounded once.  The training rule, which differs from the diagnostics' NaN
 * rule on purpose: a term whose denominator is not > 0 is absent for that graph -- its loss is exactly 0 and its
 * gradient rows are exactly 0 (a plate without a hole, a graph without periodic connections, a graph whose W or D
 * is not > 0).  A NaN in a participating input still gives a NaN loss, which the step's non-finite test sees.
 * One 1024-thread workgroup per graph, thread t owning rows t, t + 1024, ... in that order and the block folded
 * in a fixed order: a graph gets bitwise the same row alone and inside any batch, and from call to call.
 * n_graphs <= 0, a NULL ptr, y, affine, table or loss, and a partial group are refused on the host before any
 * launch.
 *
 * pdg_phys_loss_bwd.  g_y (N, 3) fp32 receives the gradient with respect to y of
 *   sum_g scale[0] traction_g + scale[1] periodic_g + scale[2] mean_g,
 * scale: three fp32 weights on the device (the trainer passes mu / B, as pdg_div_bwd takes penalty / B); table as
 * the forward wrote it (D is read from it: denom is taken for the group check only).  Per row: the traction and
 * periodic rows of pdg_boundary_residuals_bwd with g_traction = scale[0], g_periodic = scale[1]; the mean row
 * 2 area[n] / D (S_c / D - target[g, c] / std) times scale[2] at the rows whose area is > 0.  Each output
 * element is (float)((double)g_y_old + term) when accumulate is set, else (float)term: one rounding.  A weight
 * that is exactly 0 switches its term off with exact zeros, whatever the table holds (NaN included); so does a
 * denominator that is not > 0.  Node-parallel and without atomics.  n_graphs <= 0, n_nodes <= 0, a NULL ptr, y,
 * affine, table, scale or g_y, and a partial group are refused on the host before any launch.
 *
 * pdg_loss_reduce_phys.  pdg_loss_reduce with the three physics sums: out[0..2] as pdg_loss_reduce writes them,
 * out[4 + k] = scale_phys[k] * sum_g loss_phys[g, k] (fp64 sum in a fixed order, rounded to fp32, scaled in fp32;
 * exactly 0 when scale_phys[k] is 0 or loss_phys is NULL), out[3] = pdg_loss_reduce's out[3] (bitwise: as its
 * compiled code forms it, fma(sum_nmse, scale_nmse, out[2])) + out[4] + out[5] + out[6], added in that order in
 * fp32, so with all three weights 0 the seven values repeat pdg_loss_reduce's four.  loss_phys: (B, 3) fp32 as the forward wrote it; scale_phys: three fp32 values on
 * the device; both NULL or both given.  out holds 7 values. */
int pdg_phys_loss_fwd(int n_graphs, const int* ptr, const float* y, const float* affine, const float* bvec,
                      const float* blen, const int64_t* labels, const int* rowptr_dst, const int* src,
                      const int* perm, const float* edge_attr, const float* area, const double* denom,
                      const float* target, double* table, float* loss, void* stream);
int pdg_phys_loss_bwd(int n_graphs, const int* ptr, int n_nodes, const float* y, const float* affine,
                      const float* bvec, const float* blen, const int64_t* labels, const int* rowptr_dst,
                      const int* src, const int* perm, const float* edge_attr, const float* area,
                      const double* denom, const float* target, const double* table, const float* scale,
                      int accumulate, float* g_y, void* stream);
int pdg_loss_reduce_phys(int n_graphs, const float* loss_nmse, const float* loss_div, const float* loss_phys,
                         float scale_nmse, float scale_div, const float* scale_phys, const float* zero_flag,
                         float* out, void* stream);

/* ---------------------------------------------------------------- sampling at arbitrary points */
/* The operator S that maps a nodal field to its values at query points, and its transpose (pdg_sample.hip).  The
 * mesh is given as everywhere above: points (n_nodes, dim) fp32 with dim 2 or 3 (x and y are read), faces
 * (n_faces, nv) int64 with nv 3 or 4 in the face's own vertex order, either orientation.  fp64 arithmetic from the
 * fp32 inputs, every result rounded to fp32 once; kernel launches only (no host read, no memset node), so every call
 * can be captured.  Sizes, null pointers (all but the stream) and scratch sizes are refused on the host before any
 * HIP call; every index read on the device is checked against its array before use.
 *
 * pdg_cell_bins.  A uniform gx x gy grid over the mesh's bounding box (bbox: min x, min y, max x, max y, written
 * here); bin by * gx + bx lists in bin_cells[bin_ptr[bin] .. bin_ptr[bin + 1]) the cells whose own bounding box,
 * inflated by 8 * 2^-40 of its extents, overlaps the bin (count, exclusive scan, fill; the order inside a bin is
 * unspecified and nothing depends on it).  bin_ptr: gx gy + 1 ints; bin_cells: `capacity` ints.  info (4 ints):
 *   0  the total number of entries (saturated at 2^31 - 1),
 *   1  1 when the total exceeds capacity: no slot at or past capacity was written, bin_cells is incomplete and
 *      the call is to be repeated with capacity >= info[0],
 *   2  the number of cells of zero area (det == 0, the det of the mesh fields above): they enter no bin,
 *   3  the number of cells with a vertex index outside [0, n_nodes): they enter no bin, the index is never used.
 * scratch holds pdg_cell_bins_scratch_bytes(gx, gy) bytes (< 0 unless gx, gy >= 1 and gx gy + 1024 < 2^31).
 *
 * pdg_locate_points.  queries: (n_q, 2) fp32.  With periodic != 0 a query is first wrapped into the box in fp64,
 * x' = x - floor((x - xmin) / Lx) Lx and the same for y; otherwise a query outside the box is outside.  The
 * candidates are the cells of the query's bin.  Triangles: barycentric weights, signed sub-area over signed area.
 * Quads: the closed-form inverse of the bilinear map (the root of the quadratic on which the map's Jacobian has
 * the sign of the quad's area), weights (1-s)(1-t), s(1-t), st, (1-s)t for (a, b, c, d).  A cell contains the query
 * iff every weight >= -2^-40; among the containing cells the one whose smallest weight is largest wins, the lowest
 * cell id among equals.  cell: (n_q) int32, -1 when no cell contains the query (a hole, outside, a NaN query);
 * weights: (n_q, nv) fp32 with negative weights set to 0, all 0 for -1; *n_outside: the number of -1 (cleared
 * here).  gx, gy, bin_ptr, bin_cells, capacity, bbox as pdg_cell_bins took and wrote them.
 *
 * pdg_sample_field.  out[q, c] = sum_k weights[q, k] field[node_offset + faces[cell[q], k], c], an fp64 sum of
 * exact products in the order of k; `fill` where cell[q] is -1 (and where an index cannot be used).  field:
 * (n_rows, n_cols) fp32; node_offset addresses one mesh's rows inside a batched field.
 *
 * pdg_sample_csr.  The node-major CSR of S: rowptr (n_nodes + 1) and entries (n_q nv ints, rowptr[n_nodes] of
 * them used), the entry q nv + k standing for weights[q, k] of a located query whose cell has node n as vertex k;
 * a row's entries ascend, whatever the atomics' order (the grouping of pdg_graph_plan, rows of any length).
 * *status: 1 when a cell or a vertex index is out of range (the item is dropped).  scratch holds
 * pdg_sample_csr_scratch_bytes(n_nodes, n_q, nv) bytes (< 0 for bad sizes).
 *
 * pdg_sample_field_bwd.  gfield[n, c] = sum over row n's entries of weights[entry] gout[entry / nv, c], in the
 * row's order in fp64, rounded once; no atomics, so two calls agree bitwise; a row without entries gets 0.
 * gout: (n_q, n_cols), gfield: (n_nodes, n_cols). */
long pdg_cell_bins_scratch_bytes(int gx, int gy);
int pdg_cell_bins(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces, int gx,
                  int gy, int* bin_ptr, int* bin_cells, long capacity, float* bbox, int* info, void* scratch,
                  long scratch_bytes, void* stream);
int pdg_locate_points(int n_nodes, const float* points, int dim, int n_faces, int nv, const int64_t* faces, int gx,
                      int gy, const int* bin_ptr, const int* bin_cells, long capacity, const float* bbox,
                      int periodic, long n_q, const float* queries, int* cell, float* weights, int* n_outside,
                      void* stream);
int pdg_sample_field(long n_q, int n_faces, int nv, const int64_t* faces, const int* cell, const float* weights,
                     const float* field, long n_rows, int n_cols, long node_offset, float fill, float* out,
                     void* stream);
long pdg_sample_csr_scratch_bytes(int n_nodes, long n_q, int nv);
int pdg_sample_csr(int n_nodes, int n_faces, int nv, const int64_t* faces, long n_q, const int* cell, int* rowptr,
                   int* entries, int* status, void* scratch, long scratch_bytes, void* stream);
int pdg_sample_field_bwd(int n_nodes, long n_q, int nv, const int* rowptr, const int* entries, const float* weights,
                         const float* gout, int n_cols, float* gfield, void* stream);

/* ---------------------------------------------------------------- FEM targets */
/* The periodic elastic cell problem on P1 triangles (pdg_fem.hip): plane stress, one isotropic material,
 * C = E / (1 - nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, (1 - nu) / 2]] on (xx, yy, xy) with the engineering shear
 * gamma_xy, u(x) = eps x + ut(x), eps = [[exx, gxy / 2], [gxy / 2, eyy]], ut periodic.  A batch is the concatenation
 * of its meshes: points (n_nodes, dim) fp32 with dim 2 or 3 (x and y are read), ptr (n_graphs + 1) the node segments,
 * fptr (n_graphs + 1) the face segments, and, all int32 with batch-wide indices,
 *   verts (3 n_faces)       the node of every corner, in the face's own vertex order (either orientation),
 *   rep (n_nodes)           the periodic representative of every node (rep[rep[v]] == rep[v], inside v's graph),
 *   rverts (3 n_faces)      rep[verts],
 *   item_rowptr, item       a CSR keyed by representative: row v lists 3 face + corner of every corner that is v or an
 *                           image of v, ascending; the rows of image nodes are empty.
 * Every index read on the device is checked against its array before it addresses anything; an item that fails is
 * skipped.  Sizes, null pointers (all but the stream), the material (young finite and > 0, poisson in (-1, 0.5)) and
 * the scratch size are refused on the host before any HIP call.
 *
 * pdg_fem_elements.  elem (n_faces, 8) fp64 = det, area = |det| / 2, gx[3], gy[3], in fp64 from the fp32
 * coordinates with the expressions of the P1 divergence operator above, each as written there, contraction off.
 * *status (cleared here): 1 a face with det == 0 (its gradients are not finite: launch no solve), 2 a vertex outside
 * [0, n_nodes) (the face's row is NaN).
 *
 * pdg_fem_solve.  A = P^T K P, b = -P^T K (eps x) over the representatives, solved by Jacobi-preconditioned
 * conjugate gradients from x0 = 0; after the preconditioner the mean over the representatives is taken off z, per
 * component, which keeps the two translations out, and the returned ut has zero mean over the representatives.  One
 * persistent workgroup of 1024 threads per (graph, load case), grid n_graphs x n_cases: thread t owns the
 * representatives t, t + 1024, ... of its graph, every product row is gathered by its owner (no scatter), every
 * inner product is an fp64 block sum folded in a fixed order, no float atomics, nothing allocated, no memset: a graph
 * gets bitwise the same rows alone and inside any batch, and it can be captured.  strains (n_graphs, n_cases, 3) fp64
 * = exx, eyy, gxy.  ut (n_cases, n_nodes, 2) fp64: the periodic part at every node (an image holds its
 * representative's row).  All vectors are fp64 in scratch, pdg_fem_solve_scratch_bytes(n_nodes, n_cases) bytes (x, r,
 * p, A p, 1 / diag A: 80 bytes per node and case; < 0 unless 0 < n_nodes < 2^29 and 0 < n_cases <= 64).
 * Termination, all of it decided inside the kernel so that no input makes the workgroup spin:
 *   noise rule   alongside b the kernel sums b_abs, the same sums with every element term's absolute value; when
 *                |b|_2 <= 1e-12 |b_abs|_2 the right-hand side is rounding noise (a plate without a hole: the exact
 *                b is 0): ut = 0, 0 iterations, status TRIVIAL;
 *   convergence  |r|_2 <= rtol |b|_2 (the recurrence residual; rtol in (0, 1)): status CONVERGED;
 *   cap          max_iter is clamped to [0, 100000] on the host; reaching it returns the current iterate, MAX_ITER;
 *   breakdown    p^T A p <= 0 or not finite, or a residual (or b) that is not finite: BREAKDOWN.
 * table (n_graphs, n_cases, 4) fp64 = iterations, |b|_2, the true final relative residual |b - A x|_2 / |b|_2
 * recomputed after the loop (0 for TRIVIAL), status (0 CONVERGED, 1 TRIVIAL, 2 MAX_ITER, 3 BREAKDOWN).  An empty
 * graph (ptr[g + 1] == ptr[g]) gets a NaN table row and nothing else is written for it.
 *
 * pdg_fem_stress.  From u = eps x + ut in fp64: the element strains and stresses, and
 *   stress, strain (n_cases, n_nodes, 3) fp32: the average over the node's own corners (not its images') of the
 *     incident elements' values, weighted by the element's area (nodal == 0) or unweighted (nodal == 1), the terms
 *     added in ascending item order and rounded once; 0 for a node of no face;
 *   sums (n_graphs, n_cases, 8) fp64 = sum area sigma (3), sum area eps (3), the material area, the bounding box's
 *     area ((xmax - xmin)(ymax - ymin) in fp64 from the fp32 extremes), each a block sum in a fixed order; NaN for an
 *     empty graph.
 * Two kernel launches, nothing else: it can be captured. */
int pdg_fem_elements(int n_nodes, const float* points, int dim, int n_faces, const int* verts, double* elem,
                     int* status, void* stream);
long pdg_fem_solve_scratch_bytes(int n_nodes, int n_cases);
int pdg_fem_solve(int n_graphs, int n_cases, const int* ptr, int n_nodes, const float* points, int dim, int n_faces,
                  const int* verts, const int* rverts, const int* rep, const int* item_rowptr, const int* item,
                  const double* elem, const double* strains, double young, double poisson, double rtol, int max_iter,
                  double* ut, double* table, void* scratch, long scratch_bytes, void* stream);
int pdg_fem_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, const float* points,
                   int dim, int n_faces, const int* verts, const int* rep, const int* item_rowptr, const int* item,
                   const double* elem, const double* strains, const double* ut, double young, double poisson,
                   int nodal, float* stress, float* strain, double* sums, void* stream);

/* ---------------------------------------------------------------- Hyperelastic FEM targets */
/* The periodic cell problem of a compressible neo-Hookean material in plane strain under a finite mean deformation
 * (pdg_hyper.hip), on the meshes, the plan arrays and the element table of "FEM targets" above (pdg_fem_elements):
 *   u(X) = (Fbar - I) X + ut(X), ut periodic; per element F = Fbar + grad ut, F3 = diag(F, 1), I1 = tr(F^T F) + 1,
 *   J = det F,  W = mu / 2 (J^(-2/3) I1 - 3) + U(J),
 *   volumetric 0 ("log"):       U = kappa (J ln J - J + 1),  U' = kappa ln J,
 *   volumetric 1 ("quadratic"): U = kappa / 2 (J - 1)^2,
 *   P = mu J^(-2/3) (F - I1 / 3 F^-T) + U'(J) J F^-T (first Piola-Kirchhoff, 2 x 2), A = dP/dF (4 x 4, symmetric, on
 *   (F00, F01, F10, F11)), sigma = P F^T / J (Cauchy).
 * fbar (n_graphs, n_cases, 4) fp64 = F00, F01, F10, F11 of every problem.  Sizes, null pointers (all but the stream),
 * the material (mu, kappa finite and > 0, volumetric 0 or 1), rtol and eta in (0, 1), n_steps in [1, 10000] and the
 * scratch size are refused on the host before any HIP call.  Every index read on the device is checked against its
 * array before it addresses anything; an item that fails is skipped.  Every expression is evaluated as written,
 * contraction off.
 *
 * pdg_hyper_solve.  The balance r_v = -sum area P_e g_c = 0 at every periodic representative, with ut of zero mean
 * over the representatives.  One persistent workgroup of 1024 threads per (graph, load case), grid n_graphs x n_cases:
 * thread t owns the representatives t, t + 1024, ... and the faces fptr[g] + t, fptr[g] + t + 1024, ... of its
 * graph; every row is gathered by its owner in ascending item order (no scatter), every sum is an fp64 block sum
 * folded in a fixed order, no float atomics, nothing allocated, no memset: a graph gets bitwise the same rows alone
 * and inside any batch, and it can be captured.  For each of n_steps equal increments Fbar(t) = I + t (Fbar - I),
 * t = step / n_steps, Newton iterations, each of
 *   element pass   F_e, P_e, A_e of the graph's faces into scratch (14 doubles a face), and Phi = sum area W(F_e); an
 *                  element with J_e <= 0 or a value that is not finite is counted through the same block sum;
 *   row pass       r_v, f_abs (the same sums of the terms' absolute values) and the diagonal of the tangent;
 *   convergence    |r|_2 <= rtol |f_abs|_2: scale-free; a plate without a hole converges with no iteration, ut = 0;
 *   inner solve    A d = r by the Jacobi-preconditioned conjugate gradients of pdg_fem_solve (the mean over the
 *                  representatives taken off z) from d = 0, the tangent applied from the stored A_e, until
 *                  |r_k|_2 <= eta |r_0|_2 or max_pcg iterations (clamped to [1, 100000]); on p^T A p <= 0 it stops
 *                  with the iterate so far, or with the preconditioned residual when there is none yet: a descent
 *                  direction, a truncation and not a failure;
 *   backtracking   alpha = 1, 1/2, .. 2^-10: the step is accepted when no element has J_e <= 0 and
 *                  Phi(x + alpha d) <= Phi(x) - 1e-4 alpha r.d, the two rounded sums compared with an allowance of
 *                  32 ulp of the sum of area |terms of W| (what cancels inside W is rounding, not an increase).
 * Every decision is taken from block sums every thread holds alike, and every loop is capped, so no input makes the
 * workgroup spin.  Status (pdg_fem_solve's codes; 1 is not used): 0 CONVERGED; 2 MAX_ITER, a load step's Newton
 * iteration reached max_newton (per step, clamped to [0, 1000]); 3 BREAKDOWN, an exhausted line search, a sum that
 * is not finite, or a load step that starts with an inverted element.  MAX_ITER and BREAKDOWN return the current
 * iterate; when a sum was not finite ut is NaN.
 * ut (n_cases, n_nodes, 2) fp64: the periodic part at every node (an image holds its representative's row).
 * table (n_graphs, n_cases, 6) fp64 = load steps completed, Newton iterations (all steps), conjugate-gradient
 * iterations (all steps), the last row pass's |f_abs|_2, the true final relative residual |r|_2 / |f_abs|_2
 * recomputed from the returned ut under the whole load (NaN when it holds an inverted element), status.  An empty
 * graph (ptr[g + 1] == ptr[g]) gets a NaN table row and nothing else is written for it.
 * scratch: seven 2 n_nodes fp64 vectors and 14 doubles per face, per load case;
 * pdg_hyper_solve_scratch_bytes(n_nodes, n_faces, n_cases) bytes (< 0 unless 0 < n_nodes, n_faces < 2^29 and
 * 0 < n_cases <= 64).
 *
 * pdg_hyper_stress.  From F_e = Fbar + grad ut in fp64:
 *   stress (n_cases, n_nodes, 3) fp32: the Cauchy stress xx, yy, xy; strain, the same shape: the logarithmic strain
 *     1/2 ln(F F^T) as xx, yy, 2 xy; each the average over the node's own corners (not its images') of the incident
 *     elements' values, weighted by the deformed area area J_e (nodal == 0) or unweighted (nodal == 1), the terms
 *     added in ascending item order and rounded once; 0 for a node of no face;
 *   sums (n_graphs, n_cases, 10) fp64 = sum area J sigma (xx, yy, xy), sum area P (00, 01, 10, 11), sum area J (the
 *     deformed material area), the material area, the bounding box's area of the undeformed points, each a block sum
 *     in a fixed order; NaN for an empty graph.
 * Two kernel launches, nothing else: it can be captured. */
long pdg_hyper_solve_scratch_bytes(int n_nodes, int n_faces, int n_cases);
int pdg_hyper_solve(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, int n_faces,
                    const int* rverts, const int* rep, const int* item_rowptr, const int* item, const double* elem,
                    const double* fbar, double mu, double kappa, int volumetric, double rtol, int n_steps,
                    int max_newton, double eta, int max_pcg, double* ut, double* table, void* scratch,
                    long scratch_bytes, void* stream);
int pdg_hyper_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, const float* points,
                     int dim, int n_faces, const int* verts, const int* rep, const int* item_rowptr, const int* item,
                     const double* elem, const double* fbar, const double* ut, double mu, double kappa,
                     int volumetric, int nodal, float* stress, float* strain, double* sums, void* stream);

/* ---------------------------------------------------------------- Q1 FEM targets */
/* The linear cell problem of "FEM targets" above on bilinear (Q1) quads (pdg_femq1.hip): the same material, load
 * cases, arrays and checks, argument for argument, with four corners a face: verts, rverts and item hold 4 n_faces
 * entries, an item is 4 face + corner, and a face's vertices run around it in either orientation.  The integrals are
 * the 2 x 2 Gauss rule's, xi, eta = +-1 / sqrt(3), which is exact for the stiffness of a parallelogram; Gauss point g
 * is the one nearest corner g of the face's own vertex order (reference corners (-1, -1), (1, -1), (1, 1), (-1, 1)).
 * Host-side refusals, their order and their messages are those of the triangle calls.
 *
 * pdg_femq1_elements.  elem (n_faces, 36) fp64: for each Gauss point g, at 9 g, det J, dN/dx[4], dN/dy[4], in fp64
 * from the fp32 coordinates, every expression as written, contraction off; the gradients use the signed inverse of J
 * and every weight is |det J|, so a clockwise quad (all four det J < 0) is accepted.  *status (cleared here): 1 a
 * face whose four det J are not all strictly of one sign (a zero, a non-convex quad, a bow-tie: launch no solve),
 * 2 a vertex outside [0, n_nodes) (the face's row is NaN).
 *
 * pdg_femq1_solve.  pdg_fem_solve's contract with K = sum_f sum_g |det J_g| B(g)^T C B(g): one persistent workgroup
 * of 1024 threads per (graph, load case), thread t owning the representatives t, t + 1024, ...; row v is gathered by
 * its owner over the items of v in ascending order, each item's corner force the sum over g = 0..3, in that order, of
 * |det J_g| B_c(g)^T C B(g) u (no scatter); Jacobi preconditioner, zero mean over the representatives; b_abs sums the
 * items' absolute corner forces; the noise rule, the clamp of max_iter to [0, 100000], the breakdown rule, the true
 * final relative residual, the table row, the NaN row of an empty graph and the status codes are pdg_fem_solve's.
 * scratch: pdg_femq1_solve_scratch_bytes(n_nodes, n_cases) bytes, x, r, p, A p, 1 / diag A: 80 bytes per node and
 * case (< 0 unless 0 < n_nodes < 2^29 and 0 < n_cases <= 64).  No float atomics, nothing allocated, no memset: a
 * graph gets bitwise the same rows alone and inside any batch, and it can be captured.
 *
 * pdg_femq1_stress.  From u = eps x + ut in fp64:
 *   stress, strain (n_cases, n_nodes, 3) fp32: the average over the node's own corners (not its images') of the
 *     incident faces' values at the Gauss point nearest that corner, weighted by that point's |det J| (nodal == 0) or
 *     unweighted (nodal == 1), the terms added in ascending item order and rounded once; 0 for a node of no face;
 *   sums (n_graphs, n_cases, 8) fp64, pdg_fem_stress's layout: sum_f sum_g |det J_g| sigma_g (3), the same of eps
 *     (3), the material area sum |det J_g|, the bounding box's area; NaN for an empty graph.
 * Two kernel launches, nothing else: it can be captured. */
int pdg_femq1_elements(int n_nodes, const float* points, int dim, int n_faces, const int* verts, double* elem,
                       int* status, void* stream);
long pdg_femq1_solve_scratch_bytes(int n_nodes, int n_cases);
int pdg_femq1_solve(int n_graphs, int n_cases, const int* ptr, int n_nodes, const float* points, int dim, int n_faces,
                    const int* verts, const int* rverts, const int* rep, const int* item_rowptr, const int* item,
                    const double* elem, const double* strains, double young, double poisson, double rtol,
                    int max_iter, double* ut, double* table, void* scratch, long scratch_bytes, void* stream);
int pdg_femq1_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, const float* points,
                     int dim, int n_faces, const int* verts, const int* rep, const int* item_rowptr, const int* item,
                     const double* elem, const double* strains, const double* ut, double young, double poisson,
                     int nodal, float* stress, float* strain, double* sums, void* stream);

/* ---------------------------------------------------------------- Q1 hyperelastic FEM targets */
/* The neo-Hookean cell problem of "Hyperelastic FEM targets" above on the bilinear quads of "Q1 FEM targets"
 * (pdg_hyperq1.hip): the same law, load cases, solver, outputs and checks, argument for argument, on the plan arrays
 * of a quad mesh (verts, rverts and item hold 4 n_faces entries, an item is 4 face + corner) and the element table of
 * pdg_femq1_elements, elem (n_faces, 36) fp64.  The law is evaluated at the four Gauss points of every face:
 *   F_g = Fbar + sum_k ut_k (x) grad N_k(g),  w_g = |det J_g|,  P_g, A_g as above,  Phi = sum_f sum_g w_g W(F_g).
 * Host-side refusals, their order and their messages are those of pdg_hyper_solve and pdg_hyper_stress.  Every index
 * read on the device is checked against its array before it addresses anything; an item that fails is skipped.  Every
 * expression is evaluated as written, contraction off; the constitutive code is pdg_hyper.hip's (pdg_neohooke.hpp).
 *
 * pdg_hyperq1_solve.  The balance r_v = -sum_items sum_g w_g P_g grad N_c(g) = 0 at every periodic representative,
 * ut of zero mean over the representatives.  One persistent workgroup of 512 threads per (graph, load case), grid
 * n_graphs x n_cases (512, not the triangle solver's 1024: four Gauss points a face want more than the 128 registers
 * a thread of 1024 has, and nothing may spill inside the solver's loops): thread t owns the representatives t,
 * t + 512, ... and the faces fptr[g] + t, fptr[g] + t + 512, ... of its graph; every row is gathered by its owner in
 * ascending item order, g = 0..3 inside an item (no scatter), every sum is an fp64 block sum folded in a fixed order,
 * no float atomics, nothing allocated, no memset: a graph gets bitwise the same rows alone and inside any batch, and
 * it can be captured.  The solver is pdg_hyper_solve's, word for word: n_steps equal increments of Fbar - I, Newton
 * with the backtracking line search (alpha = 1, 1/2, .. 2^-10, the Armijo constant 1e-4, the allowance of 32 ulp of
 * the sum of w_g |terms of W|), the inner Jacobi-preconditioned conjugate gradients with the mean taken off z, the
 * truncation at eta and a direction of no positive curvature treated as a truncation; convergence at
 * |r|_2 <= rtol |f_abs|_2, f_abs the same sums as r of the terms' absolute values, one term a (item, Gauss point);
 * the same caps (n_steps <= 10000, max_newton clamped to [0, 1000] per step, max_pcg to [1, 100000], 11 trial
 * steps), so no input makes the workgroup spin; the same status codes and the same table (n_graphs, n_cases, 6), its
 * true final relative residual recomputed from the returned ut under the whole load; an empty graph gets a NaN table
 * row and nothing else is written for it.  What differs from triangles:
 *   element pass   P_g (4) and A_g (10) of every Gauss point into scratch, 56 doubles a face; a face counts as
 *                  inverted when any of its four J_g is <= 0 or not finite, counted through the same block sum, and
 *                  then stores zeros at all four points: it adds no force and no stiffness;
 *   row passes     the diagonal and the tangent-times-vector row use dF_g = sum_k q_k (x) grad N_k(g) from the
 *                  face's four representatives (rverts);
 *   a plate without a hole converges with no iteration and ut = 0 on any mesh of convex quads: the 2 x 2 rule
 *                  integrates grad N det J exactly, so the exact residual of a uniform P is 0.
 * scratch: seven 2 n_nodes fp64 vectors and 56 doubles per face, per load case;
 * pdg_hyperq1_solve_scratch_bytes(n_nodes, n_faces, n_cases) bytes (< 0 unless 0 < n_nodes, n_faces < 2^29 and
 * 0 < n_cases <= 64: pdg_hyper_solve_scratch_bytes' ranges).
 *
 * pdg_hyperq1_stress.  pdg_femq1_stress's nodal rule with pdg_hyper_stress's quantities, from F_g in fp64:
 *   stress (n_cases, n_nodes, 3) fp32: the Cauchy stress xx, yy, xy; strain, the same shape: the logarithmic strain
 *     1/2 ln(F F^T) as xx, yy, 2 xy; each the average over the node's own corners (not its images') of the incident
 *     faces' values at the Gauss point nearest that corner, weighted by that point's deformed weight w_g J_g
 *     (nodal == 0) or unweighted (nodal == 1), the terms added in ascending item order and rounded once; 0 for a
 *     node of no face;
 *   sums (n_graphs, n_cases, 10) fp64, pdg_hyper_stress's layout with sum_f sum_g w_g .. in place of area ..:
 *     sum w_g J_g sigma_g (xx, yy, xy), sum w_g P_g (00, 01, 10, 11), sum w_g J_g (the deformed material area), the
 *     material area sum w_g, the bounding box's area of the undeformed points; NaN for an empty graph.
 * Two kernel launches, nothing else: it can be captured. */
long pdg_hyperq1_solve_scratch_bytes(int n_nodes, int n_faces, int n_cases);
int pdg_hyperq1_solve(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, int n_faces,
                      const int* rverts, const int* rep, const int* item_rowptr, const int* item, const double* elem,
                      const double* fbar, double mu, double kappa, int volumetric, double rtol, int n_steps,
                      int max_newton, double eta, int max_pcg, double* ut, double* table, void* scratch,
                      long scratch_bytes, void* stream);
int pdg_hyperq1_stress(int n_graphs, int n_cases, const int* ptr, const int* fptr, int n_nodes, const float* points,
                       int dim, int n_faces, const int* verts, const int* rep, const int* item_rowptr,
                       const int* item, const double* elem, const double* fbar, const double* ut, double mu,
                       double kappa, int volumetric, int nodal, float* stress, float* strain, double* sums,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDIVGNN_H */
