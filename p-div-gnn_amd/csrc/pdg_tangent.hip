// The tangent pass: the Jacobian-vector product of EncodeProcessDecode.forward (models.py:288-326) with
// respect to the formatted inputs, (dx_in (N x 6), de_in (E)) -> d local_stress (N x 3), through the forward
// linearised at the activations a need_grad forward keeps:
//
//   biases drop out; every relu is a multiplication by the stored mask [a > 0] (the edge encoder's first layer,
//   which the forward does not store, recomputed as fma(w0, e_in, 0) + b0 > 0, pdg_edge_enc_bwd's form);
//   every graph LayerNorm y = g (a - mu) / (sigma + eps) + b over n = rows x 128 elements becomes
//     dLN = g ((da - T1 / n) / (sigma + eps) - (a - mu) T2 / (n sigma (sigma + eps)^2)),
//     T1 = sum da, T2 = sum (a - mu) da over all n elements;
//   residuals add the previous tangent; the first edge layer keeps the forward's re-association
//   (dP = Wa dx_t, dQ = Wb dx_t; message dz1 = Wc de_t + dP[dst] + dQ[src], edge update Wc de_t + dP[src] + dQ[dst]).
//
// T1 / T2: every kernel that produces a pre-LayerNorm tangent da writes its block's (T1, T2) in fp64 (block_sum2:
// a wave's xor butterfly, the waves in order), the consumer reduces the nblocks pairs itself (tan_resolve: each wave
// the same lane-strided sums and butterfly, so every lane of every block holds the same bits).  No atomics, no
// launch between producer and consumer; two runs agree bitwise.  The normalisation's Jacobian is symmetric, so the
// form is ln_relu_bwd4's with g moved outside.
//
// Layout: pdg_ingrad.hip's (one block of 8 waves per contiguous row range, the 128 x 128 weights stationary in
// registers as bf16 terms, 32-row bf16x6 images of the operand rows in LDS, the unbiased product gemm_x6f, its
// rows through an fp32 row tile so that thread (rg, cg) meets columns 4cg .. 4cg + 3 of rows rg and rg + 16).
// Loads are clamped to the block's last row, row stores go through buffer resources that drop what lies past
// the block's range.  A first layout: no register pipeline across rounds but the encoder's; EXPERIMENTS.md
// has the measured time beside the forward's.
#include "pdg_coop.hpp"

using namespace pdg;

namespace {

constexpr unsigned DROP = 0x7ffffff0u;   // a buffer offset past every range: the store is dropped
// a block's buffer resources span (rows x 512) bytes in an int: pdg_node_net's bound
constexpr int TAN_MAX_ROWS = 1 << 22;

struct TanLn {
  float c1;   // T1 / n
  float c2;   // T2 / (n sigma (sigma + eps)^2), 0 for a constant tensor (as lnb_resolve)
};

// The LayerNorm-tangent scalars from the producer's np (T1, T2) pairs: lnb_resolve's order.
__device__ __forceinline__ TanLn tan_resolve(const double* __restrict__ pairs, int np,
                                             const pdg_ln_stat* __restrict__ stp) {
  double s1 = 0, s2 = 0;
  for (int b = lane_id(); b < np; b += 64) {
    const double2 v = reinterpret_cast<const double2*>(pairs)[b];
    s1 += v.x;
    s2 += v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  const double M = stp->count, sd = stp->std_d, den = sd + (double)LN_EPS;
  TanLn r;
  r.c1 = (float)(s1 / M);
  r.c2 = sd > 0 ? (float)(s2 / (M * sd * den * den)) : 0.f;
  return r;
}

// dLN of 4 features, without the weight g: (da - c1) / den - (a - mu) c2.
__device__ __forceinline__ f32x4 ln_tan4_nog(const f32x4& da, const f32x4& a, const LNStat& st, const TanLn& tl) {
  f32x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = div_den(da[j] - tl.c1, st.den, st.rstd) - (a[j] - st.mean) * tl.c2;
  return y;
}

// x_t's tangent: g dLN(da) [+ the residual's tangent].
template <bool RES>
__device__ __forceinline__ f32x4 ln_tan_res4(const f32x4& da, const f32x4& a, const f32x4& res, const LNStat& st,
                                             const TanLn& tl, const f32x4& g) {
  const f32x4 t = ln_tan4_nog(da, a, st, tl);
  f32x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = RES ? g[j] * t[j] + res[j] : g[j] * t[j];
  return y;
}

// The (T1, T2) partials of 4 features of one row: fp32 pair sums (ln_partial_add's association), fp64 across.
__device__ __forceinline__ void tan_partial_add(const f32x4& da, const f32x4& a, float mean, double& s1, double& s2) {
  s1 += (double)((da[0] + da[1]) + (da[2] + da[3]));
  s2 += (double)(((a[0] - mean) * da[0] + (a[1] - mean) * da[1]) + ((a[2] - mean) * da[2] + (a[3] - mean) * da[3]));
}

__device__ __forceinline__ f32x4 mask4(const f32x4& a, const f32x4& v) {
  f32x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = a[j] > 0.f ? v[j] : 0.f;
  return y;
}

__device__ __forceinline__ f32x4 add4(const f32x4& a, const f32x4& b) {
  f32x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = a[j] + b[j];
  return y;
}

// The product's output (D row = feature 16w + 4 (l >> 4) + j, column = staged row 16 nb + (l & 15)) into an
// fp32 row tile.
__device__ __forceinline__ void tile_put(float* tile, const f32x4 (&d)[2]) {
  const int l = lane_id(), oc = 16 * wave_id() + 4 * (l >> 4);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) *reinterpret_cast<f32x4*>(tile + (16 * nb + (l & 15)) * OT_STRIDE + oc) = d[nb];
}

// tile = W img (one 32-row round; the caller's barriers before and after).
__device__ __forceinline__ void product_to_tile(float* tile, const WSlice& ws, const unsigned char* img) {
  f32x4 d[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  gemm_x6f<2, X6_TERM>(d, ws, img);
  tile_put(tile, d);
}

__device__ __forceinline__ f32x4 tile_get(const float* tile, int r, int cg) {
  return *reinterpret_cast<const f32x4*>(tile + r * OT_STRIDE + 4 * cg);
}

__device__ __forceinline__ f32x4 row_load4(const float* __restrict__ p, int row, int cg) {
  return *reinterpret_cast<const f32x4*>(p + (size_t)row * L + 4 * cg);
}

// Sum over the 32 lanes that share a row (cg = lane & 31), the same value in each of them.
__device__ __forceinline__ float row_sum32(float x) {
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) x += __shfl_xor(x, o);
  return x;
}

// The block's (T1, T2) -> part[2 b], part[2 b + 1] (the images are dead: `sm` is the reduction scratch).
__device__ __forceinline__ void emit_partials(double s1, double s2, unsigned char* sm, double* __restrict__ part) {
  __syncthreads();
  write_block_partials(s1, s2, reinterpret_cast<double*>(sm), part);
}

// ============================================================================ encoder tangent
// da1 = [a1 > 0] W0 dx_in (narrow, per element), da2 = [a2 > 0] W2 da1, the (T1, T2) partials of da2.
// EDGE: din = de_in (M), x1 = e_in (M), w0 (128), b0 (128).  node: din = dx_in (M x 6), x1 = a1 (M x 128),
// w0 = W0 (128 x 6).
template <bool EDGE>
__global__ __launch_bounds__(EBW_THREADS, 1) void enc_tan_kernel(
    int M, const float* __restrict__ din, const float* __restrict__ x1, const float* __restrict__ w0,
    const float* __restrict__ b0, const float* __restrict__ W2, const float* __restrict__ a2,
    const pdg_ln_stat* __restrict__ stp, float* __restrict__ da2, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img = sm;                                    // da1
  float* tile = reinterpret_cast<float*>(sm + EBW_IMG);       // W2 da1 rows
  constexpr int K = EDGE ? 1 : 6;
  const int w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  int r0, r1;
  block_rows(M, r0, r1);
  f32x4 pa2[2], pa1[2];
  float pd[2][K], pe[2];
  auto issue = [&](int base) {   // clamped: M > 0 (an empty block reads row M - 1)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int rr = clamp_row(base + rg + 16 * u, r1);
      pa2[u] = row_load4(a2, rr, cg);
      if constexpr (EDGE) {
        pe[u] = x1[rr];
        pd[u][0] = din[rr];
      } else {
        pa1[u] = row_load4(x1, rr, cg);
#pragma unroll
        for (int c = 0; c < K; ++c) pd[u][c] = din[(size_t)rr * K + c];
      }
    }
  };
  issue(r0);
  WSlice ws;
  load_wslice(ws, W2, w);
  const float mean = stp->mean;
  float w0r[4][K], b0r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < K; ++c) w0r[j][c] = w0[(4 * cg + j) * K + c];
    b0r[j] = EDGE ? b0[4 * cg + j] : 0.f;
  }
  const __amdgpu_buffer_rsrc_t rs = rows_rsrc(da2, r0, r1);
  double s1 = 0, s2 = 0;
  for (int base = r0; base < r1; base += X6_ROWS) {
    f32x4 ca2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      f32x4 a, z;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) t = fmaf(w0r[j][c], pd[u][c], t);
        z[j] = t;
        a[j] = EDGE ? fmaf(w0r[j][0], pe[u], 0.f) + b0r[j] : pa1[u][j];   // encoder_kernel's a1 sign
      }
      const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
      img_store4(img, r, cg, base + r < r1 ? mask4(a, z) : zero);
      ca2[u] = pa2[u];
    }
    __syncthreads();   // the da1 image is complete (and the previous round's tile reads are done)
    issue(base + X6_ROWS);
    product_to_tile(tile, ws, img);
    __syncthreads();   // the tile is complete; the image is free for the next round
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      const f32x4 v = mask4(ca2[u], tile_get(tile, r, cg));
      rows_store4(rs, base + r - r0, 4 * cg, v);
      if (base + r < r1) tan_partial_add(v, ca2[u], mean, s1, s2);
    }
  }
  emit_partials(s1, s2, sm, part);
}

// ============================================================================ node pre-pass tangent
// dx_t = g dLN(da2_prev) [+ dx_{t-1}], dP = Wa dx_t, dQ = Wb dx_t (Wa / Wb: columns 0-127 / 128-255 of
// edge_net.0's 128 x 384 weight).
template <bool RES>
__global__ __launch_bounds__(EBW_THREADS, 1) void node_pre_tan_kernel(
    int N, const float* __restrict__ da2p, const float* __restrict__ a2p, const pdg_ln_stat* __restrict__ stp,
    const double* __restrict__ pairs, int np, const float* __restrict__ lg, const float* __restrict__ dxres,
    float* __restrict__ dx, const float* __restrict__ W1, float* __restrict__ dP, float* __restrict__ dQ) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img = sm;                                    // dx_t
  float* tile_p = reinterpret_cast<float*>(sm + EBW_IMG);
  float* tile_q = tile_p + EFC_TILE;
  const int w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  int r0, r1;
  block_rows(N, r0, r1);
  WSlice wa, wb;
  load_wslice(wa, W1, w, 3 * L);
  load_wslice(wb, W1 + L, w, 3 * L);
  const LNStat st = *reinterpret_cast<const LNStat*>(stp);
  const TanLn tl = tan_resolve(pairs, np, stp);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + 4 * cg);
  const __amdgpu_buffer_rsrc_t rs_x = rows_rsrc(dx, r0, r1);
  const __amdgpu_buffer_rsrc_t rs_p = rows_rsrc(dP, r0, r1);
  const __amdgpu_buffer_rsrc_t rs_q = rows_rsrc(dQ, r0, r1);
  for (int base = r0; base < r1; base += X6_ROWS) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, rr = clamp_row(base + r, r1);
      const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 x = ln_tan_res4<RES>(row_load4(da2p, rr, cg), row_load4(a2p, rr, cg),
                                       RES ? row_load4(dxres, rr, cg) : zero, st, tl, g4);
      rows_store4(rs_x, base + r - r0, 4 * cg, x);
      img_store4(img, r, cg, base + r < r1 ? x : zero);
    }
    __syncthreads();   // the dx_t image is complete (and the previous round's tile reads are done)
    product_to_tile(tile_p, wa, img);
    product_to_tile(tile_q, wb, img);
    __syncthreads();   // the tiles are complete; the image is free
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      rows_store4(rs_p, base + r - r0, 4 * cg, tile_get(tile_p, r, cg));
      rows_store4(rs_q, base + r - r0, 4 * cg, tile_get(tile_q, r, cg));
    }
  }
}

// ============================================================================ edge tangent
// de_t = g dLN(da2e_prev) [+ de_{t-1}], C = Wc de_t; message da2m = [a2m > 0] W2 [a1m > 0] (C + dP[dst] + dQ[src]);
// EU: edge update da2e = [a2e > 0] W2 [a1e > 0] (C + dP[src] + dQ[dst]); the (T1, T2) partials of both.
template <bool RES, bool EU>
__global__ __launch_bounds__(EBW_THREADS, 1) void edge_tan_kernel(
    int E, int N, const float* __restrict__ da2p, const float* __restrict__ a2p, const pdg_ln_stat* __restrict__ stp,
    const double* __restrict__ pairs, int np, const float* __restrict__ lg, const float* __restrict__ deres,
    float* __restrict__ de, const int* __restrict__ src, const int* __restrict__ dst, const float* __restrict__ dP,
    const float* __restrict__ dQ, const float* __restrict__ W1, const float* __restrict__ W2,
    const float* __restrict__ a1m, const float* __restrict__ a2m, const pdg_ln_stat* __restrict__ stm,
    const float* __restrict__ a1e, const float* __restrict__ a2e, const pdg_ln_stat* __restrict__ ste,
    float* __restrict__ da2m, float* __restrict__ da2e, double* __restrict__ part_m, double* __restrict__ part_e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img_e = sm;                                  // de_t
  unsigned char* img_m = sm + EBW_IMG;                        // the message's da1
  unsigned char* img_u = sm + 2 * EBW_IMG;                    // the edge update's da1
  float* tile_c = reinterpret_cast<float*>(sm + 3 * EBW_IMG); // C rows, then the edge update's W2 rows
  float* tile_m = tile_c + EFC_TILE;                          // the message's W2 rows
  const int w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  int r0, r1;
  block_rows(E, r0, r1);
  WSlice wc, w2;
  load_wslice(wc, W1 + 2 * L, w, 3 * L);
  load_wslice(w2, W2, w);
  const LNStat st = *reinterpret_cast<const LNStat*>(stp);
  const TanLn tl = tan_resolve(pairs, np, stp);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + 4 * cg);
  const float mean_m = stm->mean, mean_e = EU ? ste->mean : 0.f;
  const __amdgpu_buffer_rsrc_t rs_e = rows_rsrc(de, r0, r1);
  const __amdgpu_buffer_rsrc_t rs_m = rows_rsrc(da2m, r0, r1);
  const __amdgpu_buffer_rsrc_t rs_u = rows_rsrc(EU ? da2e : nullptr, r0, r1);
  double sm1 = 0, sm2 = 0, se1 = 0, se2 = 0;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = r0; base < r1; base += X6_ROWS) {
    f32x4 gm[2], gu[2], xa1m[2], xa2m[2], xa1e[2], xa2e[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, rr = clamp_row(base + r, r1);
      // endpoints kept inside the node arrays whatever the index arrays hold
      const int is = min(max(src[rr], 0), N - 1), id = min(max(dst[rr], 0), N - 1);
      const f32x4 pd = row_load4(dP, id, cg), qs = row_load4(dQ, is, cg);
      gm[u] = add4(pd, qs);
      xa1m[u] = row_load4(a1m, rr, cg);
      xa2m[u] = row_load4(a2m, rr, cg);
      if constexpr (EU) {
        const f32x4 ps = row_load4(dP, is, cg), qd = row_load4(dQ, id, cg);
        gu[u] = add4(ps, qd);
        xa1e[u] = row_load4(a1e, rr, cg);
        xa2e[u] = row_load4(a2e, rr, cg);
      }
      const f32x4 x = ln_tan_res4<RES>(row_load4(da2p, rr, cg), row_load4(a2p, rr, cg),
                                       RES ? row_load4(deres, rr, cg) : zero, st, tl, g4);
      rows_store4(rs_e, base + r - r0, 4 * cg, x);
      img_store4(img_e, r, cg, base + r < r1 ? x : zero);
    }
    __syncthreads();   // the de_t image is complete (and the previous round's tile reads are done)
    product_to_tile(tile_c, wc, img_e);
    __syncthreads();   // C is complete
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      const bool ok = base + r < r1;
      const f32x4 c = tile_get(tile_c, r, cg);
      img_store4(img_m, r, cg, ok ? mask4(xa1m[u], add4(c, gm[u])) : zero);
      if constexpr (EU) img_store4(img_u, r, cg, ok ? mask4(xa1e[u], add4(c, gu[u])) : zero);
    }
    __syncthreads();   // both da1 images are complete; C is consumed
    product_to_tile(tile_m, w2, img_m);
    if constexpr (EU) product_to_tile(tile_c, w2, img_u);
    __syncthreads();   // the W2 rows are complete
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      const bool ok = base + r < r1;
      const f32x4 vm = mask4(xa2m[u], tile_get(tile_m, r, cg));
      rows_store4(rs_m, base + r - r0, 4 * cg, vm);
      if (ok) tan_partial_add(vm, xa2m[u], mean_m, sm1, sm2);
      if constexpr (EU) {
        const f32x4 vu = mask4(xa2e[u], tile_get(tile_c, r, cg));
        rows_store4(rs_u, base + r - r0, 4 * cg, vu);
        if (ok) tan_partial_add(vu, xa2e[u], mean_e, se1, se2);
      }
    }
  }
  emit_partials(sm1, sm2, sm, part_m);
  if constexpr (EU) emit_partials(se1, se2, sm + 1024, part_e);
}

// ============================================================================ aggregation tangent
// daggr[n] = g sum over the edges of destination n (dst-sorted: rowptr) of dLN(da2m), in edge order.  32 lanes
// per node, four features each.
__global__ __launch_bounds__(EBW_THREADS) void segsum_tan_kernel(
    int N, int E, const int* __restrict__ rowptr, const float* __restrict__ da2m, const float* __restrict__ a2m,
    const pdg_ln_stat* __restrict__ stp, const double* __restrict__ pairs, int np, const float* __restrict__ lg,
    float* __restrict__ daggr) {
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const LNStat st = *reinterpret_cast<const LNStat*>(stp);
  const TanLn tl = tan_resolve(pairs, np, stp);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + 4 * cg);
  for (int n = blockIdx.x * 16 + rg; n < N; n += gridDim.x * 16) {
    const int k0 = min(max(rowptr[n], 0), E), k1 = min(max(rowptr[n + 1], k0), E);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = k0; k < k1; ++k) s = add4(s, ln_tan4_nog(row_load4(da2m, k, cg), row_load4(a2m, k, cg), st, tl));
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] *= g4[j];
    *reinterpret_cast<f32x4*>(daggr + (size_t)n * L + 4 * cg) = s;
  }
}

// ============================================================================ node-net tangent
// da1n = [a1n > 0] (Wn1a daggr + Wn1b dx_t), da2n = [a2n > 0] Wn2 da1n, the (T1, T2) partials of da2n
// (Wn1a / Wn1b: columns 0-127 / 128-255 of node_net.0's 128 x 256 weight).
__global__ __launch_bounds__(EBW_THREADS, 1) void node_net_tan_kernel(
    int N, const float* __restrict__ daggr, const float* __restrict__ dx, const float* __restrict__ W1,
    const float* __restrict__ W2, const float* __restrict__ a1n, const float* __restrict__ a2n,
    const pdg_ln_stat* __restrict__ stp, float* __restrict__ da2n, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img_a = sm;                                   // daggr, then da1n
  unsigned char* img_x = sm + EBW_IMG;                         // dx_t
  float* tile = reinterpret_cast<float*>(sm + 2 * EBW_IMG);
  const int w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  int r0, r1;
  block_rows(N, r0, r1);
  WSlice wa, wb, w2;
  load_wslice(wa, W1, w, 2 * L);
  load_wslice(wb, W1 + L, w, 2 * L);
  load_wslice(w2, W2, w);
  const float mean = stp->mean;
  const __amdgpu_buffer_rsrc_t rs = rows_rsrc(da2n, r0, r1);
  double s1 = 0, s2 = 0;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = r0; base < r1; base += X6_ROWS) {
    f32x4 xa1[2], xa2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, rr = clamp_row(base + r, r1);
      const bool ok = base + r < r1;
      xa1[u] = row_load4(a1n, rr, cg);
      xa2[u] = row_load4(a2n, rr, cg);
      img_store4(img_a, r, cg, ok ? row_load4(daggr, rr, cg) : zero);
      img_store4(img_x, r, cg, ok ? row_load4(dx, rr, cg) : zero);
    }
    __syncthreads();   // both operand images are complete (and the previous round's tile reads are done)
    {
      f32x4 d[2] = {zero, zero};
      gemm_x6f<2, X6_TERM>(d, wa, img_a);
      gemm_x6f<2, X6_TERM>(d, wb, img_x);
      tile_put(tile, d);
    }
    __syncthreads();   // the first layer's rows are complete; the images are free
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      img_store4(img_a, r, cg, base + r < r1 ? mask4(xa1[u], tile_get(tile, r, cg)) : zero);
    }
    __syncthreads();   // the da1n image is complete; the tile is consumed
    product_to_tile(tile, w2, img_a);
    __syncthreads();   // the second layer's rows are complete
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u;
      const f32x4 v = mask4(xa2[u], tile_get(tile, r, cg));
      rows_store4(rs, base + r - r0, 4 * cg, v);
      if (base + r < r1) tan_partial_add(v, xa2[u], mean, s1, s2);
    }
  }
  emit_partials(s1, s2, sm, part);
}

// ============================================================================ decoder tangent
// dx_S = g dLN(da2_prev) [+ dx_{S-1}], dy = Wd2 [a1d > 0] Wd1 dx_S [* std_local_stress]: the three outputs of a
// row as the thread's four products in order, then an xor butterfly over the 32 lanes of the row.
template <bool RES>
__global__ __launch_bounds__(EBW_THREADS, 1) void decoder_tan_kernel(
    int N, const float* __restrict__ da2p, const float* __restrict__ a2p, const pdg_ln_stat* __restrict__ stp,
    const double* __restrict__ pairs, int np, const float* __restrict__ lg, const float* __restrict__ dxres,
    const float* __restrict__ Wd1, const float* __restrict__ a1d, const float* __restrict__ Wd2,
    const float* __restrict__ std_out, int scale, float* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* img = sm;                                    // dx_S
  float* tile = reinterpret_cast<float*>(sm + EBW_IMG);       // Wd1 dx_S rows
  const int w = wave_id();
  const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
  int r0, r1;
  block_rows(N, r0, r1);
  WSlice ws;
  load_wslice(ws, Wd1, w);
  const LNStat st = *reinterpret_cast<const LNStat*>(stp);
  const TanLn tl = tan_resolve(pairs, np, stp);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(lg + 4 * cg);
  f32x4 w2r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w2r[c] = *reinterpret_cast<const f32x4*>(Wd2 + c * L + 4 * cg);
  const float ys = scale ? std_out[0] : 1.f;
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(dy, (short)0, N * 3 * 4, 0x00020000);
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int base = r0; base < r1; base += X6_ROWS) {
    f32x4 xa1[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, rr = clamp_row(base + r, r1);
      xa1[u] = row_load4(a1d, rr, cg);
      const f32x4 x = ln_tan_res4<RES>(row_load4(da2p, rr, cg), row_load4(a2p, rr, cg),
                                       RES ? row_load4(dxres, rr, cg) : zero, st, tl, g4);
      img_store4(img, r, cg, base + r < r1 ? x : zero);
    }
    __syncthreads();   // the dx_S image is complete (and the previous round's tile reads are done)
    product_to_tile(tile, ws, img);
    __syncthreads();   // the tile is complete; the image is free
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = rg + 16 * u, row = base + r;
      const f32x4 z = mask4(xa1[u], tile_get(tile, r, cg));
      float y[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) t = fmaf(w2r[c][j], z[j], t);
        y[c] = row_sum32(t);
      }
      float v = cg == 1 ? y[1] : (cg == 2 ? y[2] : y[0]);   // lane cg writes output cg
      if (scale) v *= ys;
      const unsigned off = row < r1 && cg < 3 ? (unsigned)(row * 3 + cg) * 4u : DROP;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_y, off, 0, 0);
    }
  }
}

// ============================================================================ edge-length tangent
// d len_k = (pos[s] - pos[d]) . (dpos[s] - dpos[d]) / edge_attr[k] where edge_attr[k] > 0, else 0 (periodic
// pairs and coincident nodes: a constant length 0).  fp64 from the fp32 inputs, rounded once.
__global__ __launch_bounds__(256) void edge_len_tan_kernel(int E, int N, const int64_t* __restrict__ src,
                                                           const int64_t* __restrict__ dst,
                                                           const float* __restrict__ pos, const float* __restrict__ dpos,
                                                           const float* __restrict__ len, float* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= E) return;
  const int64_t s = src[k], d = dst[k];
  const float ln = len[k];
  float v = 0.f;
  if (ln > 0.f && s >= 0 && s < N && d >= 0 && d < N) {
    const double ax = (double)pos[2 * s] - (double)pos[2 * d], ay = (double)pos[2 * s + 1] - (double)pos[2 * d + 1];
    const double bx = (double)dpos[2 * s] - (double)dpos[2 * d], by = (double)dpos[2 * s + 1] - (double)dpos[2 * d + 1];
    v = (float)((ax * bx + ay * by) / (double)ln);
  }
  out[k] = v;
}

size_t tan_lds(int images, int tiles) { return (size_t)images * EBW_IMG + (size_t)tiles * EFC_TILE * sizeof(float); }

}  // namespace

#define TAN_CHECK_SIZES(name, rows, what)                                                                   \
  PDG_CHECK_ARG((rows) > 0 && (rows) < TAN_MAX_ROWS, name ": " what " must be in 1 .. 2^22 - 1");            \
  PDG_CHECK_ARG(nblocks > 0 && nblocks <= MAX_BLOCKS, name ": bad sizes (nblocks)")

extern "C" int pdg_node_enc_tan(int n_nodes, const float* dx_in, const float* a1, const float* W0, const float* W2,
                                const float* a2, const pdg_ln_stat* st, float* da2, double* partials, int nblocks,
                                void* stream) {
  TAN_CHECK_SIZES("pdg_node_enc_tan", n_nodes, "n_nodes");
  PDG_CHECK_ARG(dx_in && a1 && W0 && W2 && a2 && st && da2 && partials, "pdg_node_enc_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(a1) && PDG_ALIGNED(W2) && PDG_ALIGNED(a2) && PDG_ALIGNED(da2),
                "pdg_node_enc_tan: misaligned pointer");
  hipLaunchKernelGGL(enc_tan_kernel<false>, dim3(nblocks), dim3(EBW_THREADS), tan_lds(1, 1), (hipStream_t)stream,
                     n_nodes, dx_in, a1, W0, (const float*)nullptr, W2, a2, st, da2, partials);
  PDG_CHECK_LAUNCH("pdg_node_enc_tan");
  return PDG_OK;
}

extern "C" int pdg_edge_enc_tan(int n_edges, const float* de_in, const float* e_in, const float* w0, const float* b0,
                                const float* W2, const float* a2, const pdg_ln_stat* st, float* da2, double* partials,
                                int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_edge_enc_tan", n_edges, "n_edges");
  PDG_CHECK_ARG(de_in && e_in && w0 && b0 && W2 && a2 && st && da2 && partials, "pdg_edge_enc_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(W2) && PDG_ALIGNED(a2) && PDG_ALIGNED(da2), "pdg_edge_enc_tan: misaligned pointer");
  hipLaunchKernelGGL(enc_tan_kernel<true>, dim3(nblocks), dim3(EBW_THREADS), tan_lds(1, 1), (hipStream_t)stream,
                     n_edges, de_in, e_in, w0, b0, W2, a2, st, da2, partials);
  PDG_CHECK_LAUNCH("pdg_edge_enc_tan");
  return PDG_OK;
}

extern "C" int pdg_node_pre_tan(int n_nodes, const float* da2_prev, const float* a2_prev, const pdg_ln_stat* st,
                                const double* pairs, int npairs, const float* ln_g, const float* dx_res, float* dx_out,
                                const float* W1, float* dP, float* dQ, int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_node_pre_tan", n_nodes, "n_nodes");
  PDG_CHECK_ARG(npairs > 0 && npairs <= MAX_BLOCKS, "pdg_node_pre_tan: bad sizes (npairs)");
  PDG_CHECK_ARG(da2_prev && a2_prev && st && pairs && ln_g && dx_out && W1 && dP && dQ,
                "pdg_node_pre_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(da2_prev) && PDG_ALIGNED(a2_prev) && PDG_ALIGNED(pairs) && PDG_ALIGNED(ln_g) &&
                    PDG_ALIGNED(dx_res) && PDG_ALIGNED(dx_out) && PDG_ALIGNED(W1) && PDG_ALIGNED(dP) && PDG_ALIGNED(dQ),
                "pdg_node_pre_tan: misaligned pointer");
  dispatch_bools(
      [&](auto R) {
        hipLaunchKernelGGL(node_pre_tan_kernel<decltype(R)::value>, dim3(nblocks), dim3(EBW_THREADS), tan_lds(1, 2),
                           (hipStream_t)stream, n_nodes, da2_prev, a2_prev, st, pairs, npairs, ln_g, dx_res, dx_out,
                           W1, dP, dQ);
      },
      dx_res != nullptr);
  PDG_CHECK_LAUNCH("pdg_node_pre_tan");
  return PDG_OK;
}

extern "C" int pdg_edge_tan(int n_edges, int n_nodes, const float* da2_prev, const float* a2_prev,
                            const pdg_ln_stat* st, const double* pairs, int npairs, const float* ln_g,
                            const float* de_res, float* de_out, const int* src, const int* dst, const float* dP,
                            const float* dQ, const float* W1, const float* W2, const float* a1m, const float* a2m,
                            const pdg_ln_stat* st_m, const float* a1e, const float* a2e, const pdg_ln_stat* st_e,
                            float* da2m, float* da2e, double* part_m, double* part_e, int with_edge_update,
                            int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_edge_tan", n_edges, "n_edges");
  PDG_CHECK_ARG(n_nodes > 0 && n_nodes < TAN_MAX_ROWS, "pdg_edge_tan: n_nodes must be in 1 .. 2^22 - 1");
  PDG_CHECK_ARG(npairs > 0 && npairs <= MAX_BLOCKS, "pdg_edge_tan: bad sizes (npairs)");
  PDG_CHECK_ARG(da2_prev && a2_prev && st && pairs && ln_g && de_out && src && dst && dP && dQ && W1 && W2 && a1m &&
                    a2m && st_m && da2m && part_m,
                "pdg_edge_tan: null argument");
  PDG_CHECK_ARG(!with_edge_update || (a1e && a2e && st_e && da2e && part_e),
                "pdg_edge_tan: null argument (edge update)");
  PDG_CHECK_ARG(PDG_ALIGNED(da2_prev) && PDG_ALIGNED(a2_prev) && PDG_ALIGNED(pairs) && PDG_ALIGNED(ln_g) &&
                    PDG_ALIGNED(de_res) && PDG_ALIGNED(de_out) && PDG_ALIGNED(dP) && PDG_ALIGNED(dQ) &&
                    PDG_ALIGNED(W1) && PDG_ALIGNED(W2) && PDG_ALIGNED(a1m) && PDG_ALIGNED(a2m) && PDG_ALIGNED(a1e) &&
                    PDG_ALIGNED(a2e) && PDG_ALIGNED(da2m) && PDG_ALIGNED(da2e),
                "pdg_edge_tan: misaligned pointer");
  dispatch_bools(
      [&](auto R, auto U) {
        hipLaunchKernelGGL((edge_tan_kernel<decltype(R)::value, decltype(U)::value>), dim3(nblocks),
                           dim3(EBW_THREADS), tan_lds(3, 2), (hipStream_t)stream, n_edges, n_nodes, da2_prev, a2_prev,
                           st, pairs, npairs, ln_g, de_res, de_out, src, dst, dP, dQ, W1, W2, a1m, a2m, st_m, a1e, a2e,
                           st_e, da2m, da2e, part_m, part_e);
      },
      de_res != nullptr, with_edge_update != 0);
  PDG_CHECK_LAUNCH("pdg_edge_tan");
  return PDG_OK;
}

extern "C" int pdg_segment_sum_tan(int n_nodes, int n_edges, const int* rowptr, const float* da2m, const float* a2m,
                                   const pdg_ln_stat* st, const double* pairs, int npairs, const float* ln_g,
                                   float* daggr, int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_segment_sum_tan", n_nodes, "n_nodes");
  PDG_CHECK_ARG(n_edges > 0 && n_edges < TAN_MAX_ROWS, "pdg_segment_sum_tan: n_edges must be in 1 .. 2^22 - 1");
  PDG_CHECK_ARG(npairs > 0 && npairs <= MAX_BLOCKS, "pdg_segment_sum_tan: bad sizes (npairs)");
  PDG_CHECK_ARG(rowptr && da2m && a2m && st && pairs && ln_g && daggr, "pdg_segment_sum_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(da2m) && PDG_ALIGNED(a2m) && PDG_ALIGNED(pairs) && PDG_ALIGNED(ln_g) && PDG_ALIGNED(daggr),
                "pdg_segment_sum_tan: misaligned pointer");
  hipLaunchKernelGGL(segsum_tan_kernel, dim3(nblocks), dim3(EBW_THREADS), 0, (hipStream_t)stream, n_nodes, n_edges,
                     rowptr, da2m, a2m, st, pairs, npairs, ln_g, daggr);
  PDG_CHECK_LAUNCH("pdg_segment_sum_tan");
  return PDG_OK;
}

extern "C" int pdg_node_net_tan(int n_nodes, const float* daggr, const float* dx, const float* W1, const float* W2,
                                const float* a1n, const float* a2n, const pdg_ln_stat* st, float* da2n,
                                double* partials, int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_node_net_tan", n_nodes, "n_nodes");
  PDG_CHECK_ARG(daggr && dx && W1 && W2 && a1n && a2n && st && da2n && partials, "pdg_node_net_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(daggr) && PDG_ALIGNED(dx) && PDG_ALIGNED(W1) && PDG_ALIGNED(W2) && PDG_ALIGNED(a1n) &&
                    PDG_ALIGNED(a2n) && PDG_ALIGNED(da2n),
                "pdg_node_net_tan: misaligned pointer");
  hipLaunchKernelGGL(node_net_tan_kernel, dim3(nblocks), dim3(EBW_THREADS), tan_lds(2, 1), (hipStream_t)stream,
                     n_nodes, daggr, dx, W1, W2, a1n, a2n, st, da2n, partials);
  PDG_CHECK_LAUNCH("pdg_node_net_tan");
  return PDG_OK;
}

extern "C" int pdg_decoder_tan(int n_nodes, const float* da2_prev, const float* a2_prev, const pdg_ln_stat* st,
                               const double* pairs, int npairs, const float* ln_g, const float* dx_res,
                               const float* Wd1, const float* a1d, const float* Wd2, const float* std_out,
                               int scale_output, float* dy, int nblocks, void* stream) {
  TAN_CHECK_SIZES("pdg_decoder_tan", n_nodes, "n_nodes");
  PDG_CHECK_ARG(npairs > 0 && npairs <= MAX_BLOCKS, "pdg_decoder_tan: bad sizes (npairs)");
  PDG_CHECK_ARG(da2_prev && a2_prev && st && pairs && ln_g && Wd1 && a1d && Wd2 && dy && (std_out || !scale_output),
                "pdg_decoder_tan: null argument");
  PDG_CHECK_ARG(PDG_ALIGNED(da2_prev) && PDG_ALIGNED(a2_prev) && PDG_ALIGNED(pairs) && PDG_ALIGNED(ln_g) &&
                    PDG_ALIGNED(dx_res) && PDG_ALIGNED(Wd1) && PDG_ALIGNED(a1d) && PDG_ALIGNED(Wd2),
                "pdg_decoder_tan: misaligned pointer");
  dispatch_bools(
      [&](auto R) {
        hipLaunchKernelGGL(decoder_tan_kernel<decltype(R)::value>, dim3(nblocks), dim3(EBW_THREADS), tan_lds(1, 1),
                           (hipStream_t)stream, n_nodes, da2_prev, a2_prev, st, pairs, npairs, ln_g, dx_res, Wd1, a1d,
                           Wd2, std_out, scale_output, dy);
      },
      dx_res != nullptr);
  PDG_CHECK_LAUNCH("pdg_decoder_tan");
  return PDG_OK;
}

extern "C" int pdg_edge_len_tan(int n_edges, int n_nodes, const int64_t* src, const int64_t* dst, const float* pos,
                                const float* dpos, const float* edge_attr, float* dlen, void* stream) {
  PDG_CHECK_ARG(n_edges > 0, "pdg_edge_len_tan: n_edges must be > 0");
  PDG_CHECK_ARG(n_nodes > 0, "pdg_edge_len_tan: n_nodes must be > 0");
  PDG_CHECK_ARG(src && dst && pos && dpos && edge_attr && dlen, "pdg_edge_len_tan: null argument");
  hipLaunchKernelGGL(edge_len_tan_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_edges,
                     n_nodes, src, dst, pos, dpos, edge_attr, dlen);
  PDG_CHECK_LAUNCH("pdg_edge_len_tan");
  return PDG_OK;
}
