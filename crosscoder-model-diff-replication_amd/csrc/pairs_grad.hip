// The backward of the sparse decode (decode_pairs.hip) and the per-latent accumulator of LatentAttribution.  gfx950.
// Three gather kernels; none forms a [rows][h] matrix.  The range check, the grouped lists' chain order and their
// pieces are pairs_common.h's.
//
// cc_pairs_grad_values: the sampled dot product  dot[r][s][m] = sum over model m's columns of g[r][c] * W_dec[idx[r][s]][c].
//   Form.  A workgroup of PAIRS_THREADS lanes takes rows in turn (row = blockIdx.x + i * gridDim.x) and stages the row
//   of g once in LDS as raw bits (its first PG_STAGE_GROUPS 8-column groups; a longer row's remainder is read from
//   global memory: the same bits).  Wave w takes the slots s = w, w + PAIRS_NW, ...; the slot's index is wave-uniform,
//   and the range check decides whether its W_dec row is read at all.  The wave reads the latent's row with 16-byte
//   loads: lane l owns the 8-column groups G with G % 64 == l (d % 8 == 0: a group lies in one model).
//   Order.  Per model m: lane l folds its groups of the model in ascending G, and a group's 8 columns in column order,
//   into ONE fp32 fma chain from +0; the 64 lane sums meet in the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum; a lane
//   with no group of the model adds +0).  With val the model's sum is then multiplied once by float(val[r][s]).
//   total[r][s] = +0 + dot[r][s][0] + dot[r][s][1] + ..., the (multiplied) sums in model order.
//
// cc_pairs_grad_decoder: dW[j] = sum over the pairs p of latent j's list of val[perm[p]] * g[perm[p] / k], in the
//   grouped lists' order, lane t owning 8 consecutive columns.  Launch 1 (pgd_piece_kernel) writes the full pieces'
//   sums to the workspace, launch 2 (pgd_row_kernel) every row of dW.
//
// cc_pairs_latent_sums: thread (j, m) walks latent j's list in order: sum[j][m] += (double)a[perm[p]][m],
//   abs_sum[j][m] += fabs(that), plain fp64 adds onto the stored value; thread (j, 0) adds the number of entries to count[j].
#include "pairs_common.h"

namespace cc {

constexpr int PG_STAGE_GROUPS = 1024;  // 8-column groups of g staged in LDS: 8192 columns, 16 KiB (bf16) / 32 KiB (fp32)
constexpr int LS_UNROLL = 32;  // a values in flight per thread of the latent sums (a list is one thread's: only loads overlap)

template <int DT> CC_DEV float fma8(const Vec8<DT>& a, const Vec8<DT>& b, float acc) {
  uint32_t x[8], y[8];
  vec8_bits<DT>(a, x);
  vec8_bits<DT>(b, y);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(bits_float<DT>(x[j]), bits_float<DT>(y[j]), acc);
  return acc;
}

// ng = K / 8 and gd = d / 8: the row and a model in 8-column groups
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_grad_values_kernel(
    const int32_t* __restrict__ idx, const void* __restrict__ val, int64_t B, int k, const void* __restrict__ W,
    int64_t ldw, uint32_t h, const void* __restrict__ g, int64_t ldg, uint32_t ng, uint32_t gd, uint32_t n,
    float* __restrict__ dot, float* __restrict__ total) {
  typedef typename Elem<DT>::T T;
  __shared__ Vec8<DT> s_g[PG_STAGE_GROUPS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t staged = ng < (uint32_t)PG_STAGE_GROUPS ? ng : (uint32_t)PG_STAGE_GROUPS;

  for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
    const int64_t grow = row * ldg;
    __syncthreads();  // (the previous row's reads of s_g are done)
    for (uint32_t G = tid; G < staged; G += PAIRS_THREADS) s_g[G] = load_vec8<DT>(g, grow + (int64_t)G * 8, true);
    __syncthreads();
    for (int s = w; s < k; s += PAIRS_NW) {
      const int64_t slot = row * k + s;
      const int32_t i = __builtin_amdgcn_readfirstlane(idx[slot]);
      const bool ok = (uint32_t)i < h;  // the range check
      const float v = val ? Elem<DT>::to_f(((const T*)val)[slot]) : 1.f;
      const int64_t wrow = (int64_t)i * ldw;
      float tot = 0.f;
      for (uint32_t m = 0; m < n; ++m) {
        float sum = 0.f;
        if (ok) {  // (uniform)
          const uint32_t Gb = m * gd, Ge = Gb + gd;
          float acc = 0.f;
          for (uint32_t G0 = Gb & ~63u; G0 < Ge; G0 += 64 * PAIRS_UNROLL) {
            Vec8<DT> wv[PAIRS_UNROLL];
#pragma unroll
            for (int u = 0; u < PAIRS_UNROLL; ++u) {
              const uint32_t G = G0 + u * 64 + lane;
              wv[u] = load_vec8<DT>(W, wrow + (int64_t)G * 8, G >= Gb && G < Ge);
            }
#pragma unroll
            for (int u = 0; u < PAIRS_UNROLL; ++u) {
              const uint32_t G = G0 + u * 64 + lane;
              if (G >= Gb && G < Ge) {
                const Vec8<DT> gv = G < staged ? s_g[G] : load_vec8<DT>(g, grow + (int64_t)G * 8, true);
                acc = fma8<DT>(gv, wv[u], acc);
              }
            }
          }
          sum = wave_sum(acc);
          if (val) sum *= v;
        }
        tot += sum;
        if (dot && lane == 0) dot[slot * n + m] = sum;
      }
      if (total && lane == 0) total[slot] = tot;
    }
  }
}

// launch 1: workspace row t = the sum of the full piece that starts in perm[t L .. (t + 1) L), if there is one
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pgd_piece_kernel(
    const int32_t* __restrict__ perm, int64_t P, const int64_t* __restrict__ seg, int64_t h,
    const void* __restrict__ val, uint32_t Bk, uint32_t k, const void* __restrict__ g, int64_t ldg, uint32_t ng,
    float* __restrict__ ws, int64_t nrows) {
  const PairList a{perm, val, nullptr, Bk, k, g, nullptr, ldg, 0};
  list_pieces<DT, false>(a, P, seg, h, ng, ws, nrows);
}

// launch 2: every row of dW (PAIRS_UNROLL workspace rows in flight)
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pgd_row_kernel(
    const int32_t* __restrict__ perm, int64_t P, const int64_t* __restrict__ seg, int64_t h,
    const void* __restrict__ val, uint32_t Bk, uint32_t k, const void* __restrict__ g, int64_t ldg, uint32_t ng,
    const float* __restrict__ ws, void* __restrict__ dW, int64_t ldo) {
  const PairList a{perm, val, nullptr, Bk, k, g, nullptr, ldg, 0};
  for (int64_t j = blockIdx.x; j < h; j += gridDim.x) {
    const int64_t b = seg_at(seg, j, P), e = seg_at(seg, j + 1, P);
    for (uint32_t G = threadIdx.x; G < ng; G += PAIRS_THREADS) {
      const int64_t col = (int64_t)G * 8;
      ListAcc acc;
      list_sum<DT, false, PAIRS_UNROLL>(a, b, e, ws, (int64_t)ng * 8, col, acc);
      store8<DT>(dW, j * ldo + col, acc.d);
    }
  }
}

__global__ __launch_bounds__(PAIRS_THREADS) void pairs_latent_sums_kernel(
    const float* __restrict__ a, uint32_t Bk, int64_t n, const int32_t* __restrict__ perm, int64_t P,
    const int64_t* __restrict__ seg, int64_t h, double* __restrict__ sum, double* __restrict__ abs_sum,
    int64_t* __restrict__ count) {
  const int64_t all = h * n;
  for (int64_t t = (int64_t)blockIdx.x * PAIRS_THREADS + threadIdx.x; t < all; t += (int64_t)gridDim.x * PAIRS_THREADS) {
    const int64_t j = t / n, m = t - j * n;
    const int64_t b = seg_at(seg, j, P), e = seg_at(seg, j + 1, P);
    if (e <= b) continue;
    double s = sum[t], sa = abs_sum[t];
    int64_t cnt = 0;
    for (int64_t p0 = b; p0 < e; p0 += LS_UNROLL) {
      // (no branch around a load: every address is clamped into range, so the loads of a batch are all issued
      // before the first add waits)
      uint32_t slot[LS_UNROLL];
      float v[LS_UNROLL];
      bool ok[LS_UNROLL];
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) slot[u] = (uint32_t)perm[p0 + u < e ? p0 + u : e - 1];
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) {
        ok[u] = p0 + u < e && slot[u] < Bk;
        v[u] = a[(int64_t)(ok[u] ? slot[u] : 0u) * n + m];
      }
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u)
        if (ok[u]) {
          const double x = (double)v[u];
          s += x;
          sa += fabs(x);
          ++cnt;
        }
    }
    sum[t] = s;
    abs_sum[t] = sa;
    if (m == 0) count[j] += cnt;
  }
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_pairs_grad_values(const int32_t* idx, const void* val, int64_t B, int k, const void* W_dec, int64_t ldw,
                         int64_t h, const void* g, int64_t ldg, int64_t n, int64_t d, int dtype, float* dot,
                         float* total, void* stream) {
  const int rc = pairs_check(B, k, h, n, d, {ldw, ldg}, false, 0, true, idx && W_dec && g && (dot || total), &dtype,
                             true, {W_dec, g}, {idx, dot, total}, {}, {val});
  if (rc != CC_OK) return rc;
  const int64_t K = n * d;
  const dim3 grid((unsigned)(B < PAIRS_ROW_GROUPS ? B : PAIRS_ROW_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(pairs_grad_values_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream,
                     idx, val, B, k, W_dec, ldw, (uint32_t)h, g, ldg, (uint32_t)(K / 8), (uint32_t)(d / 8), (uint32_t)n,
                     dot, total);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_pairs_grad_decoder_ws_floats(int64_t P, int64_t K) {
  if (P < PAIRS_SPLIT || K < 1) return 0;
  return (P / PAIRS_SPLIT) * piece_pitch<false>(K);
}

int cc_pairs_grad_decoder(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, int64_t B,
                          int k, const void* g, int64_t ldg, int64_t K, int dtype, void* dW, int64_t ldo, float* ws,
                          void* stream) {
  const int64_t nrows = P / PAIRS_SPLIT;
  const int rc = pairs_check(B, k, h, 1, K, {ldg, ldo}, true, P, true,
                             seg && val && g && dW && (perm || P == 0) && (ws || nrows <= 0), &dtype, true, {g, dW, ws},
                             {perm}, {seg}, {val});
  if (rc != CC_OK) return rc;
  const uint32_t Bk = (uint32_t)(B * k), ng = (uint32_t)(K / 8);
  if (nrows > 0) {
    const dim3 grid((unsigned)(nrows < PAIRS_LIST_GROUPS ? nrows : PAIRS_LIST_GROUPS));
    hipLaunchKernelGGL(CC_BY_DTYPE(pgd_piece_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream, perm, P,
                       seg, h, val, Bk, (uint32_t)k, g, ldg, ng, ws, nrows);
    CC_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)(h < PAIRS_LIST_GROUPS ? h : PAIRS_LIST_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(pgd_row_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream, perm, P, seg,
                     h, val, Bk, (uint32_t)k, g, ldg, ng, ws, dW, ldo);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_pairs_latent_sums(const float* a, int64_t B, int k, int64_t n, const int32_t* perm, int64_t P,
                         const int64_t* seg, int64_t h, double* sum, double* abs_sum, int64_t* count, void* stream) {
  // (no rows of K columns: n = 1, d = 8)
  const int rc = pairs_check(B, k, h, 1, 8, {}, true, P, n >= 1, a && seg && sum && abs_sum && count && (perm || P == 0),
                             nullptr, n <= INT32_MAX, {}, {a, perm}, {seg, sum, abs_sum, count});
  if (rc != CC_OK) return rc;
  const int64_t blocks = (h * n + PAIRS_THREADS - 1) / PAIRS_THREADS;
  const dim3 grid((unsigned)(blocks < PAIRS_LIST_GROUPS ? blocks : PAIRS_LIST_GROUPS));
  hipLaunchKernelGGL(pairs_latent_sums_kernel, grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream, a, (uint32_t)(B * k), n,
                     perm, P, seg, h, sum, abs_sum, count);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
