// Sparse decode from (value, latent) pairs (CrossCoder.decode_pairs / pairs_sq_err): the consumer of cc_topk_rows'
// compact output.  gfx950.  The range check, the chain order and the staged gather are pairs_common.h's.
//
//   recon[r][c] = dtype(b_dec[c] + sum_s val[r][s] * W_dec[idx[r][s]][c])      slots s = 0 .. k-1 in that order.
// W_dec is [h][n d], so a latent's decoder vector over all models is one contiguous row: the kernel is a whole-row
// gather (k rows of K elements per token) plus the chain.  No [rows][h] activation matrix exists anywhere.
//
// Form.  A workgroup of PAIRS_THREADS lanes takes rows in turn (row = blockIdx.x + i * gridDim.x); lane t owns the 8
// consecutive columns 8 (c * PAIRS_THREADS + t) of every chunk c (one 16-B load in bf16, two in fp32; d % 8 == 0, so
// a lane's columns lie in one model).  A row's pairs are read once where k <= PAIRS_THREADS (the usual case): the
// staged list is built for the first chunk and serves every chunk.
//
// sq_err[r][m] = sum over model m's columns of (float(dtype(acc)) - x)^2, in an order fixed by (K, d): a lane folds
// its 8 columns in column order; a wave folds, per model its lanes touch, the lanes of that model (xor butterfly,
// the other lanes add +0); the workgroup adds the waves' sums in wave order, chunk after chunk (the running sum of
// a model that continues in the next chunk is carried through LDS).
#include "pairs_common.h"

namespace cc {

// ng = K / 8 and g = d / 8: the row and a model in 8-column groups (one lane's share)
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void decode_pairs_kernel(
    const void* __restrict__ val, const int32_t* __restrict__ idx, int64_t B, int k, const void* __restrict__ W,
    int64_t ldw, uint32_t h, const void* __restrict__ b_dec, uint32_t ng, uint32_t g, int64_t n,
    void* __restrict__ recon, int64_t ldr, const void* __restrict__ x, int64_t ldx, float* __restrict__ sq_err) {
  typedef typename Elem<DT>::T T;
  __shared__ PairStage st;
  __shared__ float s_wp[PAIRS_NW][PAIRS_THREADS];
  __shared__ float s_carry[2];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t nch = (ng + PAIRS_THREADS - 1) / PAIRS_THREADS;

  for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
    const T* const vrow = (const T*)val + row * k;
    const int32_t* const irow = idx + row * k;
    int cnt = 0;  // in-range slots of the staged tile
    for (uint32_t c = 0; c < nch; ++c) {
      const uint32_t G0 = c * PAIRS_THREADS, G = G0 + tid;
      const bool on = G < ng;
      const int64_t col = (int64_t)G * 8;
      float acc[8];
      if (on) {
        load8<DT>(b_dec, col, acc);
      } else {
        zero8(acc);
      }
      stage_gather<DT>(st, vrow, irow, k, h, W, ldw, col, on, c == 0, cnt, acc);

      float sq = 0.f;
      if (on) {
        if (recon) store8<DT>(recon, row * ldr + col, acc);
        if (sq_err) {
          float xv[8];
          load8_nt<DT>(x, row * ldx + col, xv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float e = Elem<DT>::round(acc[j]) - xv[j];
            sq = __builtin_fmaf(e, e, sq);
          }
        }
      }
      if (sq_err) {  // (uniform) this chunk's groups folded into their models
        const uint32_t Gend = min(G0 + PAIRS_THREADS - 1, ng - 1), mc0 = G0 / g;
        const uint32_t m = on ? G / g : 0xffffffffu;
        const uint32_t Gw = G0 + w * 64;
        if (Gw < ng) {
          const uint32_t mhi = min(Gw + 63, ng - 1) / g;
          for (uint32_t mm = Gw / g; mm <= mhi; ++mm) {
            const float s = wave_sum(m == mm ? sq : 0.f);
            if (lane == 0) s_wp[w][mm - mc0] = s;
          }
        }
        __syncthreads();
        if ((uint32_t)tid <= Gend / g - mc0) {  // lane t: the chunk's t-th model
          const uint32_t mm = mc0 + tid;
          float tot = mm * g < G0 ? s_carry[c & 1] : 0.f;  // (it began in an earlier chunk: lane 0 only)
#pragma unroll
          for (int q = 0; q < PAIRS_NW; ++q) {
            const uint32_t Gq = G0 + q * 64;
            if (Gq < ng && Gq / g <= mm && mm <= min(Gq + 63, ng - 1) / g) tot += s_wp[q][tid];
          }
          if ((mm + 1) * g - 1 <= Gend) sq_err[row * n + mm] = tot;
          else s_carry[(c + 1) & 1] = tot;  // (it goes on in the next chunk: the last lane only)
        }
        __syncthreads();
      }
    }
  }
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_decode_pairs(const void* val, const int32_t* idx, int64_t B, int k, const void* W_dec, int64_t ldw, int64_t h,
                    const void* b_dec, int64_t n, int64_t d, int dtype, void* recon, int64_t ldr, const void* x,
                    int64_t ldx, float* sq_err, void* stream) {
  const bool ptrs_ok = val && idx && W_dec && b_dec && (recon || sq_err) && (x == nullptr) == (sq_err == nullptr) &&
                       !(recon && recon == x);
  // (the pitch of an absent matrix does not count)
  const int rc = pairs_check(B, k, h, n, d, {ldw, recon ? ldr : ldw, x ? ldx : ldw}, false, 0, true, ptrs_ok, &dtype,
                             true, {W_dec, b_dec, x, recon}, {idx, sq_err}, {}, {val});
  if (rc != CC_OK) return rc;
  const int64_t K = n * d;
  const dim3 grid((unsigned)(B < PAIRS_ROW_GROUPS ? B : PAIRS_ROW_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(decode_pairs_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream, val, idx,
                     B, k, W_dec, ldw, (uint32_t)h, b_dec, (uint32_t)(K / 8), (uint32_t)(d / 8), n, recon, ldr, x, ldx,
                     sq_err);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
