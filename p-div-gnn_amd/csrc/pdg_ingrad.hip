// Input gradients of the two encoders (the vector-Jacobian product of EncodeProcessDecode.forward with
// respect to mean_stress, pos and edge_attr; models.py:260-274 backwards, then format_node_features /
// format_edge_features, models.py:140-162).  The training backward (pdg_mlp2_bwd_coop, pdg_edge_enc_bwd)
// forms the first layer's gz1 = (W2^T gz2) [a1 > 0] per row, reduces it into weight gradients and drops it;
// here the same row is multiplied by the first layer's weight instead:
//
//   gz2 = LN_bwd(gy) [a2 > 0],  u = W2^T gz2,  g_in[c] = sum_j W0[j][c] [a1[j] > 0] u[j]
//
// with c < 5 for the node encoder (mean_stress 3, pos 2; the node-type column gets no gradient) and the one
// scalar column for the edge encoder, whose a1 = w0 e_in + b0 is recomputed from the scalar input as
// pdg_edge_enc_bwd does.  Then the unformat step: / std (scale_input), edges back to the caller's order
// through the plan's permutation.
//
// Layout: pdg_mlp2_bwd_coop's (one block of 8 waves per contiguous row range, W2^T stationary in registers as
// bf16 terms, 32-row bf16x6 images of gz2 in LDS, the product's rows through an fp32 row tile so that thread
// (rg, cg) meets columns 4cg .. 4cg + 3 of the rows rg and rg + 16 it staged, their relu bits still in its
// registers).  The 128-wide dot with W0 is the thread's four products in order, then an xor butterfly over
// the 32 lanes of the row (float addition commutes, so every lane holds the same sum: a fixed order, no
// atomics).  No memory operation in the loop is conditional: loads are clamped to the block's last row and
// the narrow stores go through buffer resources with an out-of-range offset for the lanes and rows that
// write nothing, so the next round's loads, issued before these stores, are waited for by count.
#include "pdg_coop.hpp"

using namespace pdg;

namespace {

constexpr unsigned DROP = 0x7ffffff0u;   // a buffer offset past every range: the store is dropped

__device__ __forceinline__ __amdgpu_buffer_rsrc_t floats_rsrc(float* base, long n) {
  return __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)(n * 4), 0x00020000);
}
__device__ __forceinline__ void store1(__amdgpu_buffer_rsrc_t rs, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, off, 0, 0);
}
// Sum over the 32 lanes that share a row (cg = lane & 31), the same value in each of them.
__device__ __forceinline__ float row_sum32(float x) {
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o);
  return x;
}

struct GinLds {   // the gz2 image and the row tile of u; no post-loop area
  static constexpr size_t tile = EBW_IMG, total = tile + EFC_TILE * sizeof(float);
};

// EDGE: x1 = e_in (M), w0 (128), b0 (128), perm (M); out_a = g_edge_attr (M).
// node: x1 = a1 (M x 128), w0 = W0 (128 x 6); out_a = g_mean_stress (M x 3), out_b = g_pos (M x 2).
template <bool EDGE>
__global__ __launch_bounds__(EBW_THREADS, 1) void enc_gin_kernel(
    int M, const float* __restrict__ gy, const float* __restrict__ a2, const float* __restrict__ x1,
    const float* __restrict__ w0, const float* __restrict__ b0, const pdg_ln_stat* __restrict__ stp,
    const pdg_ln_bwd* __restrict__ lbp, const double* __restrict__ lb_pairs, int lb_npairs,
    const float* __restrict__ lg, const float* __restrict__ W2T, const int* __restrict__ perm,
    const float* __restrict__ st8, int scale, float* __restrict__ out_a, float* __restrict__ out_b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img2 = sm;                                    // gz2
  float* t_u = reinterpret_cast<float*>(sm + GinLds::tile);    // u = W2^T gz2 rows
  constexpr int K = EDGE ? 1 : 5, LD0 = EDGE ? 1 : 6;
  const int l = lane_id(), w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int oc = 16 * w + 4 * (l >> 4);
  int r0, r1;
  block_rows(M, r0, r1);
  f32x4 pg[2], pa2[2], pa1[2];
  float pe[2];
  int pp[2];
  auto issue = [&](int base) {   // clamped: M > 0 (an empty block reads row M - 1)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int rr = clamp_row(base + rg + 16 * u, r1);
      const size_t rc = (size_t)rr * L + 4 * cg;
      pg[u] = *reinterpret_cast<const f32x4*>(gy + rc);
      pa2[u] = *reinterpret_cast<const f32x4*>(a2 + rc);
      if constexpr (EDGE) {
        pe[u] = x1[rr];
        pp[u] = perm[rr];
      } else {
        pa1[u] = *reinterpret_cast<const f32x4*>(x1 + rc);
      }
    }
  };
  issue(r0);
  WSlice w2;
  load_wslice(w2, W2T, w);
  const LNStat st = *reinterpret_cast<const LNStat*>(stp);
  const pdg_ln_bwd lb = lnb_resolve(lbp, lb_pairs, lb_npairs, stp);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + 4 * cg);
  // the first layer's weight rows 4cg .. 4cg + 3 (and, for the recomputed a1, its bias)
  float w0r[4][K], b0r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < K; ++c) w0r[j][c] = w0[(4 * cg + j) * LD0 + c];
    b0r[j] = EDGE ? b0[4 * cg + j] : 0.f;
  }
  // models.py:140-162 backwards: x = (v - mean) / std
  float std_a = 1.f, std_b = 1.f;   // edge: std_edge_weight; node: std_mean_stress, std_pos
  if (scale) {
    std_a = EDGE ? st8[7] : st8[3];
    std_b = st8[1];
  }
  // the loop-invariant loads complete here: a first use inside the loop would put their wait (vmcnt(0), which
  // also waits for the previous round's stores) into every round
  pin_vgpr(g4);
  pin_vgpr(std_a);
  pin_vgpr(std_b);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pin_vgpr(b0r[j]);
#pragma unroll
    for (int c = 0; c < K; ++c) pin_vgpr(w0r[j][c]);
  }
  const __amdgpu_buffer_rsrc_t rs_a = floats_rsrc(out_a, (long)M * (EDGE ? 1 : 3));
  const __amdgpu_buffer_rsrc_t rs_b = floats_rsrc(EDGE ? out_a : out_b, EDGE ? 0 : (long)M * 2);
  for (int base = r0; base < r1; base += X6_ROWS) {
    unsigned mk[2];   // [a1 > 0] of the thread's four columns, rows rg and rg + 16
    int prow[2];      // edge: the caller's edge id of those rows
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      gz2_stage4<false>(img2, nullptr, base + r, r1, r, cg, pg[u], pa2[u], st, lb, g4);
      if constexpr (EDGE) {
        f32x4 a;   // encoder_kernel's a1 sign: fma(w0, e, 0) + b0 > 0 (pdg_edge_enc_bwd's)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = fmaf(w0r[j][0], pe[u], 0.f) + b0r[j];
        mk[u] = relu_mask4(a);
        prow[u] = pp[u];
      } else {
        mk[u] = relu_mask4(pa1[u]);
        prow[u] = 0;
      }
    }
    __syncthreads();   // the gz2 image is complete (and the previous round's tile reads are done)
    issue(base + X6_ROWS);
    f32x4 d[1][2];
    const unsigned char* imgs[1] = {img2};
    gemm_round<1>(d, w2, imgs);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      *reinterpret_cast<f32x4*>(t_u + (16 * nb + (l & 15)) * OT_STRIDE + oc) = d[0][nb];
    __syncthreads();   // the tile is complete; the image is free for the next round
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, row = base + r;
      const bool ok = row < r1;
      const f32x4 uv = *reinterpret_cast<const f32x4*>(t_u + r * OT_STRIDE + 4 * cg);
      float g[K];
#pragma unroll
      for (int c = 0; c < K; ++c) g[c] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float z1 = (mk[u] >> (8 * j)) & 1u ? uv[j] : 0.f;   // gz1
#pragma unroll
        for (int c = 0; c < K; ++c) g[c] = fmaf(w0r[j][c], z1, g[c]);
      }
#pragma unroll
      for (int c = 0; c < K; ++c) g[c] = row_sum32(g[c]);
      if constexpr (EDGE) {
        const float v = scale ? g[0] / std_a : g[0];
        store1(rs_a, ok && cg == 0 ? (unsigned)prow[u] * 4u : DROP, v);
      } else {
        // lane cg writes column cg: 0-2 -> g_mean_stress, 3-4 -> g_pos
        float v = g[0];
#pragma unroll
        for (int c = 1; c < K; ++c) v = cg == c ? g[c] : v;
        if (scale) v = v / (cg < 3 ? std_a : std_b);
        store1(rs_a, ok && cg < 3 ? (unsigned)(row * 3 + cg) * 4u : DROP, v);
        store1(rs_b, ok && cg >= 3 && cg < 5 ? (unsigned)(row * 2 + cg - 3) * 4u : DROP, v);
      }
    }
  }
}

// (N, 3) rows summed per graph: one block per graph, fp64 over the block's threads (each its strided
// rows in order), then the xor butterfly of a wave and the waves in order through LDS; rounded once.
__global__ __launch_bounds__(1024) void graph_colsum3_kernel(const int* __restrict__ ptr, const float* __restrict__ x,
                                                             float* __restrict__ out) {
  __shared__ double red[3 * 16];
  const int g = blockIdx.x;
  const int n0 = ptr[g], n1 = ptr[g + 1];
  double s[3] = {0, 0, 0};
  for (int i = n0 + (int)threadIdx.x; i < n1; i += (int)blockDim.x)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (double)x[(size_t)i * 3 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
  const int w = wave_id(), nw = blockDim.x >> 6;
  if (lane_id() == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c * 16 + w] = s[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0;
    for (int i = 0; i < nw; ++i) v += red[threadIdx.x * 16 + i];
    out[g * 3 + threadIdx.x] = (float)v;
  }
}

// the narrow outputs are addressed with 32-bit byte offsets below DROP
constexpr int GIN_MAX_ROWS = 1 << 26;

}  // namespace

extern "C" int pdg_edge_enc_gin(int n_edges, const float* gy, const float* a2, const float* e_in, const float* w0,
                                const float* b0, const pdg_ln_stat* st, const pdg_ln_bwd* lb, const double* lb_pairs,
                                int lb_npairs, const float* ln_g, const float* W2T, const int* perm,
                                const float* stats8, int scale_input, float* g_edge_attr, int nblocks,
                                void* stream) {
  PDG_CHECK_ARG(n_edges > 0 && n_edges <= GIN_MAX_ROWS, "pdg_edge_enc_gin: n_edges must be in 1 .. 2^26");
  PDG_CHECK_ARG(nblocks > 0 && nblocks <= MAX_BLOCKS, "pdg_edge_enc_gin: bad sizes");
  PDG_CHECK_ARG(gy && a2 && e_in && w0 && b0 && st && (lb || lb_pairs) && ln_g && W2T && perm && g_edge_attr &&
                    (stats8 || !scale_input),
                "pdg_edge_enc_gin: null argument");
  PDG_CHECK_ARG(!lb_pairs || lb_npairs > 0, "pdg_edge_enc_gin: lb_pairs without a count");
  PDG_CHECK_ARG(PDG_ALIGNED(gy) && PDG_ALIGNED(a2) && PDG_ALIGNED(ln_g) && PDG_ALIGNED(W2T),
                "pdg_edge_enc_gin: misaligned pointer");
  hipLaunchKernelGGL(enc_gin_kernel<true>, dim3(nblocks), dim3(EBW_THREADS), GinLds::total, (hipStream_t)stream, n_edges,
                     gy, a2, e_in, w0, b0, st, lb, lb_pairs, lb_npairs, ln_g, W2T, perm, stats8, scale_input,
                     g_edge_attr, (float*)nullptr);
  PDG_CHECK_LAUNCH("pdg_edge_enc_gin");
  return PDG_OK;
}

extern "C" int pdg_node_enc_gin(int n_nodes, const float* gy, const float* a2, const float* a1, const float* W0,
                                const pdg_ln_stat* st, const pdg_ln_bwd* lb, const double* lb_pairs, int lb_npairs,
                                const float* ln_g, const float* W2T, const float* stats8, int scale_input,
                                float* g_mean_stress, float* g_pos, int nblocks, void* stream) {
  PDG_CHECK_ARG(n_nodes > 0 && n_nodes <= GIN_MAX_ROWS, "pdg_node_enc_gin: n_nodes must be in 1 .. 2^26");
  PDG_CHECK_ARG(nblocks > 0 && nblocks <= MAX_BLOCKS, "pdg_node_enc_gin: bad sizes");
  PDG_CHECK_ARG(gy && a2 && a1 && W0 && st && (lb || lb_pairs) && ln_g && W2T && g_mean_stress && g_pos &&
                    (stats8 || !scale_input),
                "pdg_node_enc_gin: null argument");
  PDG_CHECK_ARG(!lb_pairs || lb_npairs > 0, "pdg_node_enc_gin: lb_pairs without a count");
  PDG_CHECK_ARG(PDG_ALIGNED(gy) && PDG_ALIGNED(a2) && PDG_ALIGNED(a1) && PDG_ALIGNED(ln_g) && PDG_ALIGNED(W2T),
                "pdg_node_enc_gin: misaligned pointer");
  hipLaunchKernelGGL(enc_gin_kernel<false>, dim3(nblocks), dim3(EBW_THREADS), GinLds::total, (hipStream_t)stream, n_nodes,
                     gy, a2, a1, W0, (const float*)nullptr, st, lb, lb_pairs, lb_npairs, ln_g, W2T,
                     (const int*)nullptr, stats8, scale_input, g_mean_stress, g_pos);
  PDG_CHECK_LAUNCH("pdg_node_enc_gin");
  return PDG_OK;
}

extern "C" int pdg_graph_colsum3(int n_graphs, const int* ptr, const float* rows, float* out, void* stream) {
  PDG_CHECK_ARG(n_graphs > 0, "pdg_graph_colsum3: n_graphs must be > 0");
  PDG_CHECK_ARG(ptr && rows && out, "pdg_graph_colsum3: null argument");
  hipLaunchKernelGGL(graph_colsum3_kernel, dim3(n_graphs), dim3(1024), 0, (hipStream_t)stream, ptr, rows, out);
  PDG_CHECK_LAUNCH("pdg_graph_colsum3");
  return PDG_OK;
}
