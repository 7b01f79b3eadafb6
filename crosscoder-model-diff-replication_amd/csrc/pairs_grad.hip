// The backward of the sparse decode (decode_pairs.hip) and the per-latent accumulator of LatentAttribution.  gfx950.
// Three gather kernels; none forms a [rows][h] matrix.  No float atomics, no spin waits; every summation order below is
// fixed by the arguments alone, so two calls give equal bits.
//
// cc_pairs_grad_values: the sampled dot product  dot[r][s][m] = sum over model m's columns of g[r][c] * W_dec[idx[r][s]][c].
//   Form.  A workgroup of PG_THREADS lanes takes rows in turn (row = blockIdx.x + i * gridDim.x) and stages the row of
//   g once in LDS as raw bits (its first PG_STAGE_GROUPS 8-column groups; a longer row's remainder is read from global
//   memory: the same bits).  Wave w takes the slots s = w, w + PG_NW, ...; the slot's index is wave-uniform, and the
//   one unsigned compare decides whether its W_dec row is read at all.  The wave reads the latent's row with 16-byte
//   loads: lane l owns the 8-column groups G with G % 64 == l (d % 8 == 0: a group lies in one model).
//   Order.  Per model m: lane l folds its groups of the model in ascending G, and a group's 8 columns in column order,
//   into ONE fp32 fma chain from +0; the 64 lane sums meet in the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum; a lane
//   with no group of the model adds +0).  With val the model's sum is then multiplied once by float(val[r][s]).
//   total[r][s] = +0 + dot[r][s][0] + dot[r][s][1] + ..., the (multiplied) sums in model order.
//
// cc_pairs_grad_decoder: dW[j] = sum over the pairs p of latent j's segment of val[perm[p]] * g[perm[p] / k], from the
//   pairs grouped by latent (perm, seg): latent j's list is perm[seg[j] .. seg[j+1]).  Lane t owns 8 consecutive columns.
//   Order.  A segment of at most PGD_SPLIT entries: one fp32 fma chain per column from +0 in segment order, rounded
//   once.  A longer segment: its consecutive pieces of PGD_SPLIT entries (the last one shorter), each such a chain from
//   +0; the piece sums are added in piece order onto +0 (fp32), and that sum is rounded once.  An entry outside
//   [0, B k) is skipped.  Launch 1 (pgd_piece_kernel) writes the FULL pieces' sums to the workspace: a full piece that
//   starts at perm position s owns workspace row s / PGD_SPLIT (full pieces are disjoint and PGD_SPLIT long, so no two
//   share a row); workgroup t finds the one segment that can own row t by a binary search of seg for position
//   (t + 1) PGD_SPLIT - 1, which every piece starting in [t PGD_SPLIT, (t + 1) PGD_SPLIT) covers.  Launch 2
//   (pgd_row_kernel) writes every row of dW: a short segment's chain, or a long segment's workspace rows in piece
//   order plus its last, shorter piece, which it sums itself.  seg values are clamped to [0, P]; end < begin is empty.
//
// cc_pairs_latent_sums: thread (j, m) walks latent j's segment in order: sum[j][m] += (double)a[perm[p]][m],
//   abs_sum[j][m] += fabs(that), plain fp64 adds onto the stored value; thread (j, 0) adds the number of entries to count[j].
#include "mask_common.h"

namespace cc {

constexpr int PG_THREADS = 256;
constexpr int PG_NW = PG_THREADS / 64;
constexpr int PG_STAGE_GROUPS = 1024;  // 8-column groups of g staged in LDS: 8192 columns, 16 KiB (bf16) / 32 KiB (fp32)
constexpr int PG_UNROLL = 4;           // 16-byte W_dec loads in flight per lane
constexpr int PG_MAX_GROUPS = 2048;    // workgroups: 8 per CU of a 256-CU part
constexpr int PG_MAX_K = 1 << 17;

constexpr int PGD_SPLIT = CC_PAIRS_GRAD_SPLIT;  // L: a longer segment is summed in pieces of L
constexpr int PGD_UNROLL = 4;                   // g rows in flight per lane
constexpr int PGD_MAX_GROUPS = 1 << 16;
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
__global__ __launch_bounds__(PG_THREADS) void pairs_grad_values_kernel(
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
    for (uint32_t G = tid; G < staged; G += PG_THREADS) s_g[G] = load_vec8<DT>(g, grow + (int64_t)G * 8, true);
    __syncthreads();
    for (int s = w; s < k; s += PG_NW) {
      const int64_t slot = row * k + s;
      const int32_t i = __builtin_amdgcn_readfirstlane(idx[slot]);
      const bool ok = (uint32_t)i < h;  // the one range check: negative padding and anything >= h
      const float v = val ? Elem<DT>::to_f(((const T*)val)[slot]) : 1.f;
      const int64_t wrow = (int64_t)i * ldw;
      float tot = 0.f;
      for (uint32_t m = 0; m < n; ++m) {
        float sum = 0.f;
        if (ok) {  // (uniform)
          const uint32_t Gb = m * gd, Ge = Gb + gd;
          float acc = 0.f;
          for (uint32_t G0 = Gb & ~63u; G0 < Ge; G0 += 64 * PG_UNROLL) {
            Vec8<DT> wv[PG_UNROLL];
#pragma unroll
            for (int u = 0; u < PG_UNROLL; ++u) {
              const uint32_t G = G0 + u * 64 + lane;
              wv[u] = load_vec8<DT>(W, wrow + (int64_t)G * 8, G >= Gb && G < Ge);
            }
#pragma unroll
            for (int u = 0; u < PG_UNROLL; ++u) {
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

// seg[j] clamped to [0, P]
CC_DEV int64_t seg_at(const int64_t* __restrict__ seg, int64_t j, int64_t P) {
  const int64_t v = seg[j];
  return v < 0 ? 0 : (v > P ? P : v);
}

// acc (8 columns at col) += the fma chain over perm[p0 .. p1) in order; entries outside [0, Bk) are skipped
template <int DT>
CC_DEV void pgd_chain(const int32_t* __restrict__ perm, int64_t p0, int64_t p1, const void* __restrict__ val,
                      uint32_t Bk, uint32_t k, const void* __restrict__ g, int64_t ldg, int64_t col,
                      float (&acc)[8]) {
  typedef typename Elem<DT>::T T;
  for (int64_t q0 = p0; q0 < p1; q0 += PGD_UNROLL) {
    Vec8<DT> gv[PGD_UNROLL];
    float v[PGD_UNROLL];
    bool ok[PGD_UNROLL];
#pragma unroll
    for (int u = 0; u < PGD_UNROLL; ++u) {
      ok[u] = false;
      if (q0 + u < p1) {  // (uniform)
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane(perm[q0 + u]);
        ok[u] = slot < Bk;
        if (ok[u]) {
          v[u] = Elem<DT>::to_f(((const T*)val)[slot]);
          gv[u] = load_vec8<DT>(g, (int64_t)(slot / k) * ldg + col, true);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PGD_UNROLL; ++u) {
      if (ok[u]) {
        uint32_t b[8];
        vec8_bits<DT>(gv[u], b);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v[u], bits_float<DT>(b[j]), acc[j]);
      }
    }
  }
}

// launch 1: workspace row t = the sum of the full piece that starts in perm[t L .. (t + 1) L), if there is one
template <int DT>
__global__ __launch_bounds__(PG_THREADS) void pgd_piece_kernel(
    const int32_t* __restrict__ perm, int64_t P, const int64_t* __restrict__ seg, int64_t h,
    const void* __restrict__ val, uint32_t Bk, uint32_t k, const void* __restrict__ g, int64_t ldg, uint32_t ng,
    float* __restrict__ ws, int64_t nrows) {
  constexpr int64_t L = PGD_SPLIT;
  for (int64_t t = blockIdx.x; t < nrows; t += gridDim.x) {
    const int64_t x = t * L + L - 1;  // (< P: nrows = P / L)
    // the last j in [0, h) with seg[j] <= x: the segment that holds position x when seg is non-decreasing
    int64_t lo = 0, hi = h;  // seg[lo] <= x (taken as given for lo = 0), seg[hi] > x (likewise for hi = h)
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (seg_at(seg, mid, P) <= x) lo = mid; else hi = mid;
    }
    const int64_t b = seg_at(seg, lo, P), e = seg_at(seg, lo + 1, P);
    if (e - b <= L || b > x) continue;  // not a split segment, or it begins behind this window
    const int64_t s = b >= t * L ? b : b + (t * L - b + L - 1) / L * L;  // the piece start in the window
    if (s > x || s + L > e) continue;  // (the segment's last, shorter piece is the row kernel's)
    for (uint32_t G = threadIdx.x; G < ng; G += PG_THREADS) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      pgd_chain<DT>(perm, s, s + L, val, Bk, k, g, ldg, (int64_t)G * 8, acc);
      store_cols8(ws + t * ((int64_t)ng * 8) + (int64_t)G * 8, acc);
    }
  }
}

// launch 2: every row of dW
template <int DT>
__global__ __launch_bounds__(PG_THREADS) void pgd_row_kernel(
    const int32_t* __restrict__ perm, int64_t P, const int64_t* __restrict__ seg, int64_t h,
    const void* __restrict__ val, uint32_t Bk, uint32_t k, const void* __restrict__ g, int64_t ldg, uint32_t ng,
    const float* __restrict__ ws, void* __restrict__ dW, int64_t ldo) {
  constexpr int64_t L = PGD_SPLIT;
  for (int64_t j = blockIdx.x; j < h; j += gridDim.x) {
    const int64_t b = seg_at(seg, j, P), e = seg_at(seg, j + 1, P);
    for (uint32_t G = threadIdx.x; G < ng; G += PG_THREADS) {
      const int64_t col = (int64_t)G * 8;
      float acc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = 0.f;
      if (e - b <= L) {  // (uniform; an empty or reversed segment leaves +0)
        pgd_chain<DT>(perm, b, e, val, Bk, k, g, ldg, col, acc);
      } else {
        const int64_t nfull = (e - b) / L;
        for (int64_t q0 = 0; q0 < nfull; q0 += PGD_UNROLL) {
          float part[PGD_UNROLL][8];
#pragma unroll
          for (int u = 0; u < PGD_UNROLL; ++u)
            if (q0 + u < nfull) load8f(ws, ((b + (q0 + u) * L) / L) * ((int64_t)ng * 8) + col, part[u]);
#pragma unroll
          for (int u = 0; u < PGD_UNROLL; ++u)
            if (q0 + u < nfull) {
#pragma unroll
              for (int c = 0; c < 8; ++c) acc[c] += part[u][c];
            }
        }
        if (b + nfull * L < e) {
          float last[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) last[c] = 0.f;
          pgd_chain<DT>(perm, b + nfull * L, e, val, Bk, k, g, ldg, col, last);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] += last[c];
        }
      }
      store8<DT>(dW, j * ldo + col, acc);
    }
  }
}

__global__ __launch_bounds__(PG_THREADS) void pairs_latent_sums_kernel(
    const float* __restrict__ a, uint32_t Bk, int64_t n, const int32_t* __restrict__ perm, int64_t P,
    const int64_t* __restrict__ seg, int64_t h, double* __restrict__ sum, double* __restrict__ abs_sum,
    int64_t* __restrict__ count) {
  const int64_t all = h * n;
  for (int64_t t = (int64_t)blockIdx.x * PG_THREADS + threadIdx.x; t < all; t += (int64_t)gridDim.x * PG_THREADS) {
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

// the checks the two grouped entry points share, in the house order up to (not including) alignment
static int grouped_check(int64_t B, int k, int64_t h, int64_t P, bool shape_ok, bool ptrs_ok, const int* dtype,
                         bool small_ok) {
  if (B < 1 || k < 1 || h < 1 || P < 0 || !shape_ok) return CC_ERR_SHAPE;
  if (!ptrs_ok) return CC_ERR_NULL;
  if (dtype && *dtype != CC_BF16 && *dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > PG_MAX_K || B > INT32_MAX / k || P > INT32_MAX || !small_ok) return CC_ERR_TOO_LARGE;
  return CC_OK;
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_pairs_grad_values(const int32_t* idx, const void* val, int64_t B, int k, const void* W_dec, int64_t ldw,
                         int64_t h, const void* g, int64_t ldg, int64_t n, int64_t d, int dtype, float* dot,
                         float* total, void* stream) {
  if (B < 1 || k < 1 || h < 1 || n < 1 || d < 8 || (d & 7)) return CC_ERR_SHAPE;
  // (K saturates where n * d would leave int64: no pitch reaches it)
  const int64_t K = n > INT64_MAX / d ? INT64_MAX : n * d;
  if (ldw < K || ldg < K) return CC_ERR_SHAPE;
  if (!idx || !W_dec || !g || (!dot && !total)) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > PG_MAX_K || K > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({W_dec, g}, 15) || (((ldw | ldg) * es) & 15) || !aligned({idx, dot, total}, 3) ||
      !aligned({val}, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  const dim3 grid((unsigned)(B < PG_MAX_GROUPS ? B : PG_MAX_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(pairs_grad_values_kernel, dtype), grid, dim3(PG_THREADS), 0, (hipStream_t)stream, idx,
                     val, B, k, W_dec, ldw, (uint32_t)h, g, ldg, (uint32_t)(K / 8), (uint32_t)(d / 8), (uint32_t)n, dot,
                     total);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_pairs_grad_decoder_ws_floats(int64_t P, int64_t K) {
  if (P < PGD_SPLIT || K < 1) return 0;
  return (P / PGD_SPLIT) * K;
}

int cc_pairs_grad_decoder(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, int64_t B,
                          int k, const void* g, int64_t ldg, int64_t K, int dtype, void* dW, int64_t ldo, float* ws,
                          void* stream) {
  const int64_t nrows = P >= 0 ? P / PGD_SPLIT : 0;
  const int rc = grouped_check(B, k, h, P, K >= 8 && !(K & 7) && ldg >= K && ldo >= K,
                               seg && val && g && dW && (perm || P == 0) && (ws || nrows == 0), &dtype, K <= INT32_MAX);
  if (rc != CC_OK) return rc;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({g, dW, ws}, 15) || (((ldg | ldo) * es) & 15) || !aligned({seg}, 7) || !aligned({perm}, 3) ||
      !aligned({val}, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  const uint32_t Bk = (uint32_t)(B * k), ng = (uint32_t)(K / 8);
  if (nrows > 0) {
    const dim3 grid((unsigned)(nrows < PGD_MAX_GROUPS ? nrows : PGD_MAX_GROUPS));
    hipLaunchKernelGGL(CC_BY_DTYPE(pgd_piece_kernel, dtype), grid, dim3(PG_THREADS), 0, (hipStream_t)stream, perm, P, seg,
                       h, val, Bk, (uint32_t)k, g, ldg, ng, ws, nrows);
    CC_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)(h < PGD_MAX_GROUPS ? h : PGD_MAX_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(pgd_row_kernel, dtype), grid, dim3(PG_THREADS), 0, (hipStream_t)stream, perm, P, seg, h,
                     val, Bk, (uint32_t)k, g, ldg, ng, ws, dW, ldo);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_pairs_latent_sums(const float* a, int64_t B, int k, int64_t n, const int32_t* perm, int64_t P,
                         const int64_t* seg, int64_t h, double* sum, double* abs_sum, int64_t* count, void* stream) {
  const int rc = grouped_check(B, k, h, P, n >= 1, a && seg && sum && abs_sum && count && (perm || P == 0), nullptr,
                               n <= INT32_MAX);
  if (rc != CC_OK) return rc;
  if (!aligned({seg, sum, abs_sum, count}, 7) || !aligned({a, perm}, 3)) return CC_ERR_ALIGN;
  const int64_t blocks = (h * n + PG_THREADS - 1) / PG_THREADS;
  const dim3 grid((unsigned)(blocks < PGD_MAX_GROUPS ? blocks : PGD_MAX_GROUPS));
  hipLaunchKernelGGL(pairs_latent_sums_kernel, grid, dim3(PG_THREADS), 0, (hipStream_t)stream, a, (uint32_t)(B * k), n,
                     perm, P, seg, h, sum, abs_sum, count);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
