// Sparse decode from (value, latent) pairs (CrossCoder.decode_pairs / pairs_sq_err): the consumer of cc_topk_rows'
// compact output.  gfx950.
//
//   recon[r][c] = dtype(b_dec[c] + sum_s val[r][s] * W_dec[idx[r][s]][c])      slots s = 0 .. k-1 in that order,
// one fp32 fma chain per output element; a slot whose index is outside [0, h) adds nothing and reads nothing.
// W_dec is [h][n d], so a latent's decoder vector over all models is one contiguous row: the kernel is a whole-row
// gather (k rows of K elements per token) plus the chain.  No [rows][h] activation matrix exists anywhere.
//
// Form.  A workgroup of DP_THREADS lanes takes rows in turn (row = blockIdx.x + i * gridDim.x); lane t owns the 8
// consecutive columns 8 (c * DP_THREADS + t) of every chunk c (one 16-B load in bf16, two in fp32; d % 8 == 0, so a
// lane's columns lie in one model).  A row's pairs are read once: DP_TILE slots at a time, one slot per lane, the in-range
// ones compacted in slot order into LDS (CC_BLOCK_EXCL_SCAN: the prefix count is the slot's place) as (index, fp32
// value).  The chain then walks the compacted list DP_UNROLL entries at a time: the entries are wave-uniform (LDS
// broadcast reads, the row offset in scalar registers, 64-bit: 2^17 x 4608 elements exceed 2^31), the DP_UNROLL row
// loads are issued before the first fma, and the fmas consume them in slot order.  k <= DP_TILE (the usual case):
// the list is built once per row and serves every chunk.
//
// sq_err[r][m] = sum over model m's columns of (float(dtype(acc)) - x)^2, in an order fixed by (K, d): a lane folds
// its 8 columns in column order; a wave folds, per model its lanes touch, the lanes of that model (xor butterfly,
// the other lanes add +0); the workgroup adds the waves' sums in wave order, chunk after chunk (the running sum of
// a model that continues in the next chunk is carried through LDS).  No atomics, no spin waits.
#include "mask_common.h"

namespace cc {

constexpr int DP_THREADS = 256;
constexpr int DP_NW = DP_THREADS / 64;
constexpr int DP_TILE = DP_THREADS;    // slots staged at a time: one per lane
constexpr int DP_UNROLL = 4;           // W_dec rows in flight per lane
constexpr int DP_MAX_GROUPS = 2048;    // workgroups: 8 per CU of a 256-CU part
constexpr int DP_MAX_K = 1 << 17;

// ng = K / 8 and g = d / 8: the row and a model in 8-column groups (one lane's share)
template <int DT>
__global__ __launch_bounds__(DP_THREADS) void decode_pairs_kernel(
    const void* __restrict__ val, const int32_t* __restrict__ idx, int64_t B, int k, const void* __restrict__ W,
    int64_t ldw, uint32_t h, const void* __restrict__ b_dec, uint32_t ng, uint32_t g, int64_t n,
    void* __restrict__ recon, int64_t ldr, const void* __restrict__ x, int64_t ldx, float* __restrict__ sq_err) {
  typedef typename Elem<DT>::T T;
  __shared__ int32_t s_idx[DP_TILE];
  __shared__ float s_val[DP_TILE];
  __shared__ uint32_t s_wtot[DP_NW];
  __shared__ float s_wp[DP_NW][DP_THREADS];
  __shared__ float s_carry[2];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t nch = (ng + DP_THREADS - 1) / DP_THREADS;

  for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
    const T* const vrow = (const T*)val + row * k;
    const int32_t* const irow = idx + row * k;
    int cnt = 0;  // in-range slots of the staged tile
    for (uint32_t c = 0; c < nch; ++c) {
      const uint32_t G0 = c * DP_THREADS, G = G0 + tid;
      const bool on = G < ng;
      const int64_t col = (int64_t)G * 8;
      float acc[8];
      if (on) {
        load8<DT>(b_dec, col, acc);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      }
      for (int t0 = 0; t0 < k; t0 += DP_TILE) {
        if (c == 0 || k > DP_TILE) {  // (uniform) stage the tile: the in-range pairs, compacted in slot order
          const int s = t0 + tid;
          const int32_t i = s < k ? irow[s] : -1;
          const bool ok = (uint32_t)i < h;  // the one range check: negative padding and anything >= h
          const uint32_t one = ok ? 1u : 0u;
          // (its barrier also ends the previous tile's reads of s_idx / s_val)
          CC_BLOCK_EXCL_SCAN(DP_NW, one, lane, w, s_wtot, before, all);
          if (ok) {
            s_idx[before] = i;
            s_val[before] = Elem<DT>::to_f(vrow[s]);
          }
          __syncthreads();  // (s_wtot is next written after this barrier: one set is enough)
          cnt = (int)all;
        }
        for (int s0 = 0; s0 < cnt; s0 += DP_UNROLL) {
          Vec8<DT> wv[DP_UNROLL];
          float v[DP_UNROLL];
#pragma unroll
          for (int u = 0; u < DP_UNROLL; ++u) {
            if (s0 + u < cnt) {  // (uniform)
              const int64_t i = __builtin_amdgcn_readfirstlane(s_idx[s0 + u]);
              v[u] = s_val[s0 + u];
              wv[u] = load_vec8<DT>(W, i * ldw + col, on);
            }
          }
#pragma unroll
          for (int u = 0; u < DP_UNROLL; ++u) {
            if (s0 + u < cnt) {
              uint32_t b[8];
              vec8_bits<DT>(wv[u], b);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v[u], bits_float<DT>(b[j]), acc[j]);
            }
          }
        }
      }

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
        const uint32_t Gend = min(G0 + DP_THREADS - 1, ng - 1), mc0 = G0 / g;
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
          for (int q = 0; q < DP_NW; ++q) {
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
  if (B < 1 || k < 1 || h < 1 || n < 1 || d < 8 || (d & 7)) return CC_ERR_SHAPE;
  // (K saturates where n * d would leave int64: no pitch reaches it)
  const int64_t K = n > INT64_MAX / d ? INT64_MAX : n * d;
  if (ldw < K || (recon && ldr < K) || (x && ldx < K)) return CC_ERR_SHAPE;
  if (!val || !idx || !W_dec || !b_dec || (!recon && !sq_err) || (x == nullptr) != (sq_err == nullptr) ||
      (recon && recon == x))
    return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > DP_MAX_K || K > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  const int64_t pitches = ldw | (recon ? ldr : 0) | (x ? ldx : 0);
  if (!aligned({W_dec, b_dec, x, recon}, 15) || ((pitches * es) & 15) || !aligned({idx, sq_err}, 3) ||
      !aligned({val}, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  const dim3 grid((unsigned)(B < DP_MAX_GROUPS ? B : DP_MAX_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(decode_pairs_kernel, dtype), grid, dim3(DP_THREADS), 0, (hipStream_t)stream, val, idx,
                     B, k, W_dec, ldw, (uint32_t)h, b_dec, (uint32_t)(K / 8), (uint32_t)(d / 8), n, recon, ldr, x, ldx,
                     sq_err);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
