// Dead-latent resampling (LatentResampler, resample.py): the row norms of a weight matrix, the
// loss-weighted choice of pool rows, and the re-seeding write into the parameter, moment and master arenas.  gfx950.
//
// No float atomics, no spin waits, no hand-off between workgroups inside a launch: what one launch leaves for the
// next goes through the stream's order.  Every sum has an order fixed by the shape alone.
//
//   row norms   one wave per row; lane t owns the 8 columns 8 (c * 64 + t) of every 512-column chunk c and folds their
//               squares into one fma chain, chunk after chunk; the 64 lane sums meet in the xor butterfly (wave_sum).
//   pick        weights w_r = loss_r^2 in fp64 (0 for a loss that is negative or not finite) and their inclusive
//               prefix sum in cdf, built so that it is non-decreasing and a zero weight repeats its predecessor's
//               bits (below): the smallest r with cdf[r] > t then never has weight 0, whatever the rounding did.
//               A chunk of RS_CHUNK rows per workgroup: a lane adds its RS_ITEMS weights one after the other (p_k), one
//               thread adds the RS_THREADS lane totals one after the other (base_t), an element is base_t + p_k; a
//               second launch (one workgroup) adds the chunk totals one after the other (off_c) and rewrites every
//               chunk's last element; a third adds off_c to the rest of chunk c; the fourth searches.
//   write       one workgroup per re-seeded latent: the source row's squared sum (lane chains over 2048-column chunks,
//               wave_sum, the waves in order), then one pass that scales the row into W_dec and W_enc (and the fp32
//               masters) and zeroes the latent's rows of both moments and its b_enc entries.
#include "mask_common.h"

namespace cc {

constexpr int RN_THREADS = 256;  // row norms: 4 rows per workgroup, one per wave
constexpr int RN_UNROLL = 4;     // chunks in flight per lane

template <int DT>
__global__ __launch_bounds__(RN_THREADS) void row_norms_kernel(const void* __restrict__ W, int64_t ld, int64_t rows,
                                                               uint32_t ng, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (RN_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;  // (whole waves: no barrier follows)
  const int64_t base = row * ld;
  float q = 0.f;
  for (uint32_t g0 = 0; g0 < ng; g0 += 64 * RN_UNROLL) {
    Vec8<DT> v[RN_UNROLL];
#pragma unroll
    for (int u = 0; u < RN_UNROLL; ++u) {
      const uint32_t g = g0 + u * 64 + lane;
      v[u] = load_vec8<DT>(W, base + (int64_t)g * 8, g < ng);  // (zeros past the row: they add +0)
    }
#pragma unroll
    for (int u = 0; u < RN_UNROLL; ++u) {
      uint32_t b[8];
      vec8_bits<DT>(v[u], b);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bits_float<DT>(b[j]);
        q = __builtin_fmaf(f, f, q);
      }
    }
  }
  q = wave_sum(q);
  if (lane == 0) out[row] = sqrtf(q);
}

// ---- pick
constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 16;                      // consecutive rows per lane
constexpr int RS_CHUNK = RS_THREADS * RS_ITEMS;   // rows per workgroup
constexpr int RS_TILE = 1024;                     // chunk totals staged at a time by the offsets launch

CC_DEV double loss_weight(float l) {
  const uint32_t b = __float_as_uint(l);
  const bool ok = (b & 0x7F800000u) != 0x7F800000u && !(b >> 31);  // finite and sign clear
  return ok ? (double)l * (double)l : 0.0;
}
CC_DEV int64_t chunk_last(int64_t c, int64_t R) {
  const int64_t e = (c + 1) * RS_CHUNK;
  return (e < R ? e : R) - 1;
}

// cdf[i] = base_t + p_k within the chunk (its last element: the chunk's total)
__global__ __launch_bounds__(RS_THREADS) void pick_scan_kernel(const float* __restrict__ loss, int64_t R,
                                                               double* __restrict__ cdf) {
  __shared__ double s_tot[RS_THREADS];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * RS_CHUNK + (int64_t)tid * RS_ITEMS;
  double p[RS_ITEMS];
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    run += i0 + k < R ? loss_weight(loss[i0 + k]) : 0.0;
    p[k] = run;
  }
  s_tot[tid] = run;
  __syncthreads();
  if (tid == 0) {  // the lane totals one after the other: s_tot[t] becomes base_t
    double b = 0.0;
#pragma unroll 16
    for (int t = 0; t < RS_THREADS; ++t) {
      const double v = s_tot[t];
      s_tot[t] = b;
      b += v;
    }
  }
  __syncthreads();
  const double base = s_tot[tid];
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k)
    if (i0 + k < R) cdf[i0 + k] = base + p[k];
}

// one workgroup: off_c = off_{c-1} + total_{c-1} one after the other; every chunk's last element becomes
// off_c + total_c = off_{c+1}
__global__ __launch_bounds__(RS_THREADS) void pick_offsets_kernel(int64_t R, int64_t nchunks, double* __restrict__ cdf) {
  __shared__ double s_t[RS_TILE];
  __shared__ double s_carry;
  const int tid = threadIdx.x;
  if (tid == 0) s_carry = 0.0;
  for (int64_t c0 = 0; c0 < nchunks; c0 += RS_TILE) {
    for (int i = tid; i < RS_TILE; i += RS_THREADS)
      s_t[i] = c0 + i < nchunks ? cdf[chunk_last(c0 + i, R)] : 0.0;
    __syncthreads();
    if (tid == 0) {
      double off = s_carry;
      const int m = (int)(nchunks - c0 < RS_TILE ? nchunks - c0 : RS_TILE);
#pragma unroll 16
      for (int i = 0; i < m; ++i) {
        off += s_t[i];
        s_t[i] = off;
      }
      s_carry = off;
    }
    __syncthreads();
    for (int i = tid; i < RS_TILE; i += RS_THREADS)
      if (c0 + i < nchunks) cdf[chunk_last(c0 + i, R)] = s_t[i];
    __syncthreads();
  }
}

// chunk c >= 1: off_c (the last element of chunk c - 1, which this launch does not write) onto every element but
// the chunk's last
__global__ __launch_bounds__(RS_THREADS) void pick_add_kernel(int64_t R, double* __restrict__ cdf) {
  const int64_t c = (int64_t)blockIdx.x + 1;
  const double off = cdf[c * RS_CHUNK - 1];
  const int64_t last = chunk_last(c, R);
  const int64_t i0 = c * RS_CHUNK + (int64_t)threadIdx.x * RS_ITEMS;
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k)
    if (i0 + k < last) cdf[i0 + k] = off + cdf[i0 + k];
}

__global__ __launch_bounds__(RS_THREADS) void pick_search_kernel(const double* __restrict__ cdf, int64_t R,
                                                                 const double* __restrict__ u, int64_t J,
                                                                 int64_t* __restrict__ rows_out) {
  const int64_t j = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (j >= J) return;
  const double total = cdf[R - 1];
  if (!(total > 0.0)) {
    rows_out[j] = -1;
    return;
  }
  double uj = u[j];
  if (!(uj >= 0.0)) uj = 0.0;  // (NaN and negatives: the first row with weight)
  double t = uj * total;
  // (u at or beyond 1, or a product rounded up to the total: the last row with weight)
  if (!(t < total)) t = __longlong_as_double(__double_as_longlong(total) - 1);
  int64_t lo = 0, hi = R - 1;  // cdf[hi] > t holds
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  rows_out[j] = lo;
}

// ---- write
constexpr int RW_THREADS = 256;
constexpr int RW_NW = RW_THREADS / 64;

// The four arenas share one layout: [ W_enc [h][K] | b_enc [h] | W_dec [h][K] | b_dec [K] ].
template <int DT, int SDT>
__global__ __launch_bounds__(RW_THREADS) void resample_write_kernel(
    const void* __restrict__ X, int64_t ldx, int64_t R, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ latents, int64_t h, uint32_t ng, float enc_norm, float dec_norm, void* __restrict__ P,
    float* __restrict__ master, void* __restrict__ M, void* __restrict__ V, int32_t* __restrict__ done) {
  typedef typename Elem<DT>::T T;
  typedef typename Elem<SDT>::T ST;
  __shared__ float s_w[RW_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t j = blockIdx.x;
  const int64_t r = rows[j], l = latents[j];
  const int64_t K = (int64_t)ng * 8;
  const bool in_range = r >= 0 && r < R && l >= 0 && l < h;  // (uniform)
  float s = 0.f;
  if (in_range) {
    const int64_t xb = r * ldx;
    float q = 0.f;
    for (uint32_t g0 = 0; g0 < ng; g0 += RW_THREADS) {
      const uint32_t g = g0 + tid;
      uint32_t b[8];
      vec8_bits<DT>(load_vec8<DT>(X, xb + (int64_t)g * 8, g < ng), b);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float f = bits_float<DT>(b[c]);
        q = __builtin_fmaf(f, f, q);
      }
    }
    q = wave_sum(q);
    if (lane == 0) s_w[w] = q;
  }
  __syncthreads();
  if (in_range) {
#pragma unroll
    for (int q = 0; q < RW_NW; ++q) s += s_w[q];  // (the waves in order; every lane the same bits)
  }
  // a zero row has no direction, and a sum that is not finite would write NaN: both leave the latent as it is
  const bool go = in_range && s > 0.f && s <= 3.4028234663852886e38f;
  if (tid == 0 && done) done[j] = go ? 1 : 0;
  if (!go) return;
  const float root = sqrtf(s);
  const float es = enc_norm / root, ds = dec_norm / root;
  const int64_t xb = r * ldx;
  const int64_t o_enc = l * K, o_benc = h * K + l, o_dec = h * K + h + l * K;
  const uint32_t zero[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  for (uint32_t g0 = 0; g0 < ng; g0 += RW_THREADS) {
    const uint32_t g = g0 + tid;
    if (g >= ng) break;
    const int64_t col = (int64_t)g * 8;
    uint32_t b[8];
    vec8_bits<DT>(load_vec8<DT>(X, xb + col, true), b);
    float e[8], d[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float f = bits_float<DT>(b[c]);
      e[c] = f * es;
      d[c] = f * ds;
    }
    store8<DT>(P, o_enc + col, e);
    store8<DT>(P, o_dec + col, d);
    if (master) {
      store_cols8(master + o_enc + col, e);
      store_cols8(master + o_dec + col, d);
    }
    if (M) {
      store_bits8<SDT>(M, o_enc + col, zero);
      store_bits8<SDT>(M, o_dec + col, zero);
    }
    if (V) {
      store_bits8<SDT>(V, o_enc + col, zero);
      store_bits8<SDT>(V, o_dec + col, zero);
    }
  }
  if (tid == 0) {
    ((T*)P)[o_benc] = Elem<DT>::from_f(0.f);
    if (master) master[o_benc] = 0.f;
    if (M) ((ST*)M)[o_benc] = Elem<SDT>::from_f(0.f);
    if (V) ((ST*)V)[o_benc] = Elem<SDT>::from_f(0.f);
  }
}

template <int DT> static void launch_write(int state_dtype, dim3 grid, hipStream_t st, const void* X, int64_t ldx,
                                           int64_t R, const int64_t* rows, const int64_t* latents, int64_t h,
                                           uint32_t ng, float enc_norm, float dec_norm, void* P, float* master, void* M,
                                           void* V, int32_t* done) {
  hipLaunchKernelGGL((state_dtype == CC_BF16 ? resample_write_kernel<DT, CC_BF16> : resample_write_kernel<DT, CC_F32>),
                     grid, dim3(RW_THREADS), 0, st, X, ldx, R, rows, latents, h, ng, enc_norm, dec_norm, P, master, M,
                     V, done);
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_row_norms(const void* W, int64_t ld, int64_t rows, int64_t K, int dtype, float* out, void* stream) {
  if (rows < 1 || K < 8 || (K & 7) || ld < K) return CC_ERR_SHAPE;
  if (!W || !out) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (K > INT32_MAX || rows > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({W}, 15) || ((ld * es) & 15) || !aligned({out}, 3)) return CC_ERR_ALIGN;
  const dim3 grid((unsigned)((rows + RN_THREADS / 64 - 1) / (RN_THREADS / 64)));
  hipLaunchKernelGGL(CC_BY_DTYPE(row_norms_kernel, dtype), grid, dim3(RN_THREADS), 0, (hipStream_t)stream, W, ld, rows,
                     (uint32_t)(K / 8), out);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_resample_pick(const float* loss, int64_t R, const double* u, int64_t J, double* cdf, int64_t* rows_out,
                     void* stream) {
  if (R < 1 || J < 1) return CC_ERR_SHAPE;
  if (!loss || !u || !cdf || !rows_out) return CC_ERR_NULL;
  if (R > INT32_MAX || J > INT32_MAX) return CC_ERR_TOO_LARGE;
  if (!aligned({loss}, 3) || !aligned({u, cdf, rows_out}, 7)) return CC_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nchunks = (R + RS_CHUNK - 1) / RS_CHUNK;
  hipLaunchKernelGGL(pick_scan_kernel, dim3((unsigned)nchunks), dim3(RS_THREADS), 0, st, loss, R, cdf);
  if (nchunks > 1) {
    hipLaunchKernelGGL(pick_offsets_kernel, dim3(1), dim3(RS_THREADS), 0, st, R, nchunks, cdf);
    hipLaunchKernelGGL(pick_add_kernel, dim3((unsigned)(nchunks - 1)), dim3(RS_THREADS), 0, st, R, cdf);
  }
  hipLaunchKernelGGL(pick_search_kernel, dim3((unsigned)((J + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, st,
                     cdf, R, u, J, rows_out);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_resample_write(const void* X, int64_t ldx, int64_t R, const int64_t* rows, const int64_t* latents, int64_t J,
                      int64_t h, int64_t K, int dtype, float enc_norm, float dec_norm, void* params, float* master,
                      void* exp_avg, void* exp_avg_sq, int state_dtype, int32_t* done, void* stream) {
  if (R < 1 || J < 1 || h < 8 || (h & 7) || K < 8 || (K & 7) || ldx < K) return CC_ERR_SHAPE;
  if (!X || !rows || !latents || !params || (exp_avg == nullptr) != (exp_avg_sq == nullptr)) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (exp_avg && state_dtype != CC_BF16 && state_dtype != CC_F32) return CC_ERR_DTYPE;
  if (K > INT32_MAX || h > INT32_MAX || J > INT32_MAX || R > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({X, params, master, exp_avg, exp_avg_sq}, 15) || ((ldx * es) & 15) || !aligned({rows, latents}, 7) ||
      !aligned({done}, 3))
    return CC_ERR_ALIGN;
  const int sdt = exp_avg ? state_dtype : CC_F32;
  (dtype == CC_BF16 ? launch_write<CC_BF16> : launch_write<CC_F32>)(
      sdt, dim3((unsigned)J), (hipStream_t)stream, X, ldx, R, rows, latents, h, (uint32_t)(K / 8), enc_norm, dec_norm,
      params, master, exp_avg, exp_avg_sq, done);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
