// Per-latent activation statistics (the notebook's latent dashboards: firing counts, activation
// histograms, the rows where a latent fires hardest) from ONE HBM pass over acts [B][ld], folded into
// caller-owned state that persists across batches.  gfx950.
//
// A workgroup (8 or 16 waves) owns a strip of 64 latents outright.  A lane holds 2 adjacent columns, so each
// 32-lane half of a wave reads one whole 128-B line (bf16) of a row; the G = 16 or 32 half-waves of the workgroup
// take the rows round-robin (row b belongs to group b % G).  Each lane keeps, per column, a sorted top-K list
// (value, row id) in registers -- every index below is static after unrolling -- plus its count and fp32
// sum.  The G lists of a column are then merged pairwise (a bitonic top-K merge: K + K/2 log2 K
// compare-exchanges): the two halves of a wave through lane shuffles, the waves in log2 rounds through LDS,
// the batch's list with the stored one last.  All orderings are by (value descending, row id ascending), a
// strict total order on real entries, so the result is the list a full sort of every candidate would give,
// whatever the order in which the candidates arrive.  Sums: per lane in row order, then the G groups in
// index order -- fixed by (B, h) and G (k <= 4 or not) alone.  No global atomics; the histogram uses integer LDS atomics.
#include "cc_common.h"

namespace cc {

constexpr int LS_COLS = 64;                     // latents per workgroup
constexpr int LS_BINS = 32;
constexpr int LS_UNROLL = 8;                    // row loads in flight per lane
constexpr int LS_MAX_K = 16;

// a beats b: the larger value; ties go to the smaller row id.  An empty slot is (0, -1): every real entry
// (value > 0) beats it and it beats nothing.
CC_DEV bool ls_beats(float va, int64_t ia, float vb, int64_t ib) { return va > vb || (va == vb && ia < ib); }

// Sorted insertion into a list held in registers.
template <int K> CC_DEV void ls_insert(float (&v)[K], int64_t (&id)[K], float nv, int64_t nid) {
  bool stay[K + 1];  // stay[j + 1]: slot j keeps its entry
  stay[0] = true;
#pragma unroll
  for (int j = 0; j < K; ++j) stay[j + 1] = ls_beats(v[j], id[j], nv, nid);
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    if (!stay[j + 1]) {
      v[j] = stay[j] ? nv : v[j > 0 ? j - 1 : 0];
      id[j] = stay[j] ? nid : id[j > 0 ? j - 1 : 0];
    }
  }
}

// (v, id) <- the K best of (v, id) and another sorted list read through other(j, value, id).  Skipped by the
// whole wave when no lane's other list has anything to add.  upd = false: the lane only serves its list to
// the others (it must not change while they read it).
template <int K, class F> CC_DEV void ls_merge(float (&v)[K], int64_t (&id)[K], F other, bool upd = true) {
  float ov;
  int64_t oi;
  other(0, ov, oi);
  if (__builtin_amdgcn_ballot_w64(upd && ls_beats(ov, oi, v[K - 1], id[K - 1])) == 0) return;
#pragma unroll
  for (int i = 0; i < K; ++i) {  // the K best of the union, as a bitonic sequence
    other(K - 1 - i, ov, oi);
    if (upd && ls_beats(ov, oi, v[i], id[i])) {
      v[i] = ov;
      id[i] = oi;
    }
  }
#pragma unroll
  for (int s = K / 2; s >= 1; s >>= 1) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if ((i & s) == 0 && ls_beats(v[i + s], id[i + s], v[i], id[i])) {
        const float tv = v[i];
        const int64_t ti = id[i];
        v[i] = v[i + s];
        id[i] = id[i + s];
        v[i + s] = tv;
        id[i + s] = ti;
      }
    }
  }
}

// One activation of column slot `cl` (0..63) in row b.
template <int K>
CC_DEV void ls_elem(float x, int b, int cl, const int64_t* __restrict__ row_ids, int64_t row0, float thr_old,
                    float (&v)[K], int64_t (&id)[K], int& cnt, float& sum, unsigned* lhist) {
  if (!(x > 0.f)) return;  // negatives, zeros and NaN take no part
  cnt += 1;
  sum += x;
  if (lhist) {
    int bin = (int)((__float_as_uint(x) >> 23) & 0xffu) - 111;  // floor(log2 x) + 16
    bin = bin < 0 ? 0 : bin > LS_BINS - 1 ? LS_BINS - 1 : bin;
    atomicAdd(lhist + bin * LS_COLS + cl, 1u);
  }
  // fast reject: below the stored list's k-th value or this lane's own K-th (an equal value may still win
  // on its row id)
  if (x < thr_old || x < v[K - 1]) return;
  ls_insert<K>(v, id, x, row_ids ? row_ids[b] : row0 + b);
}

// NW waves per workgroup: 16 for K = 4; 8 for K = 16, whose lists (96 registers) leave no room under the 128
// registers a 16-wave workgroup may use.
template <int DT, int K, int NW>
__global__ __launch_bounds__(NW * 64) void latent_stats_kernel(
    const void* __restrict__ acts, int64_t ld, int B, int64_t h, const int64_t* __restrict__ row_ids, int64_t row0,
    int k, int64_t* __restrict__ count, float* __restrict__ sum, int64_t* __restrict__ hist,
    float* __restrict__ topk_val, int64_t* __restrict__ topk_row) {
  constexpr int LS_THREADS = NW * 64, LS_GROUPS = NW * 2;  // row groups: half-waves
  // lists in flight between waves: [slot][column of the lane][entry][lane]
  __shared__ float mv[LS_GROUPS / 4][2][K][32];
  __shared__ unsigned mlo[LS_GROUPS / 4][2][K][32], mhi[LS_GROUPS / 4][2][K][32];
  __shared__ unsigned lhist[LS_BINS * LS_COLS];
  __shared__ int lcnt[LS_GROUPS][LS_COLS];
  __shared__ float lsum[LS_GROUPS][LS_COLS];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l32 = lane & 31;
  const int g = tid >> 5;
  const int64_t col0 = (int64_t)blockIdx.x * LS_COLS, col = col0 + 2 * l32;
  const bool ok0 = col < h, ok1 = col + 1 < h;

  if (hist) {
    for (int e = tid; e < LS_BINS * LS_COLS; e += LS_THREADS) lhist[e] = 0u;
    __syncthreads();
  }
  unsigned* const lh = hist ? lhist : nullptr;

  float v0[K], v1[K];
  int64_t i0[K], i1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    v0[j] = v1[j] = 0.f;
    i0[j] = i1[j] = -1;
  }
  // the stored k-th values (0 while a list is not full)
  const float thr0 = ok0 ? topk_val[col * k + k - 1] : 0.f, thr1 = ok1 ? topk_val[(col + 1) * k + k - 1] : 0.f;
  int c0 = 0, c1 = 0;
  float s0 = 0.f, s1 = 0.f;

  if (ok0) {
    for (int b0 = g; b0 < B; b0 += LS_GROUPS * LS_UNROLL) {
      float x0[LS_UNROLL], x1[LS_UNROLL];
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) {
        const int b = b0 + LS_GROUPS * u;
        x0[u] = x1[u] = 0.f;
        if (b < B) {
          const int64_t e = (int64_t)b * ld + col;  // even: the pair is one aligned 4-B / 8-B load
          if constexpr (DT == CC_BF16) {
            const uint32_t r = *(const uint32_t*)((const bf16_t*)acts + e);
            x0[u] = __uint_as_float(r << 16);
            x1[u] = __uint_as_float(r & 0xffff0000u);
          } else {
            const float2 r = *(const float2*)((const float*)acts + e);
            x0[u] = r.x;
            x1[u] = r.y;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) {
        const int b = b0 + LS_GROUPS * u;  // (rows past B loaded as 0: no part)
        ls_elem<K>(x0[u], b, 2 * l32, row_ids, row0, thr0, v0, i0, c0, s0, lh);
        if (ok1) ls_elem<K>(x1[u], b, 2 * l32 + 1, row_ids, row0, thr1, v1, i1, c1, s1, lh);
      }
    }
  }
  lcnt[g][2 * l32] = c0;
  lcnt[g][2 * l32 + 1] = c1;
  lsum[g][2 * l32] = s0;
  lsum[g][2 * l32 + 1] = s1;

  // the two halves of the wave: lanes 0..31 take in the lists of lanes 32..63
  {
    const int src = (lane + 32) & 63;
    ls_merge<K>(v0, i0, [&](int j, float& ov, int64_t& oi) {
      ov = __shfl(v0[j], src, 64);
      oi = __shfl(i0[j], src, 64);
    }, lane < 32);
    ls_merge<K>(v1, i1, [&](int j, float& ov, int64_t& oi) {
      ov = __shfl(v1[j], src, 64);
      oi = __shfl(i1[j], src, 64);
    }, lane < 32);
  }
  // the waves: in the round of stride s, wave w with (w mod 2s) == s hands its lists to wave w - s
#pragma unroll 1
  for (int s = 1; s < LS_THREADS / 64; s <<= 1) {
    const int slot = w / (2 * s);
    const bool writer = (w & (2 * s - 1)) == s, reader = (w & (2 * s - 1)) == 0;
    if (writer && lane < 32) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        mv[slot][0][j][l32] = v0[j];
        mlo[slot][0][j][l32] = (unsigned)(uint64_t)i0[j];
        mhi[slot][0][j][l32] = (unsigned)((uint64_t)i0[j] >> 32);
        mv[slot][1][j][l32] = v1[j];
        mlo[slot][1][j][l32] = (unsigned)(uint64_t)i1[j];
        mhi[slot][1][j][l32] = (unsigned)((uint64_t)i1[j] >> 32);
      }
    }
    __syncthreads();
    if (reader && lane < 32) {
      ls_merge<K>(v0, i0, [&](int j, float& ov, int64_t& oi) {
        ov = mv[slot][0][j][l32];
        oi = (int64_t)(((uint64_t)mhi[slot][0][j][l32] << 32) | mlo[slot][0][j][l32]);
      });
      ls_merge<K>(v1, i1, [&](int j, float& ov, int64_t& oi) {
        ov = mv[slot][1][j][l32];
        oi = (int64_t)(((uint64_t)mhi[slot][1][j][l32] << 32) | mlo[slot][1][j][l32]);
      });
    }
    __syncthreads();
  }

  // the owner updates the strip's state
  if (w == 0 && lane < 32) {
    if (ok0) {
      ls_merge<K>(v0, i0, [&](int j, float& ov, int64_t& oi) {
        ov = j < k ? topk_val[col * k + j] : 0.f;
        oi = j < k ? topk_row[col * k + j] : -1;
      });
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < k) {
          topk_val[col * k + j] = v0[j];
          topk_row[col * k + j] = i0[j];
        }
    }
    if (ok1) {
      ls_merge<K>(v1, i1, [&](int j, float& ov, int64_t& oi) {
        ov = j < k ? topk_val[(col + 1) * k + j] : 0.f;
        oi = j < k ? topk_row[(col + 1) * k + j] : -1;
      });
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < k) {
          topk_val[(col + 1) * k + j] = v1[j];
          topk_row[(col + 1) * k + j] = i1[j];
        }
    }
  }
  if (w == 1 && col0 + lane < h) {  // counts and sums: the groups in index order
    int c = 0;
    float s = 0.f;
#pragma unroll 8
    for (int q = 0; q < LS_GROUPS; ++q) {
      c += lcnt[q][lane];
      s += lsum[q][lane];
    }
    count[col0 + lane] += c;
    sum[col0 + lane] += s;
  }
  if (hist) {
    for (int e = tid; e < LS_BINS * LS_COLS; e += LS_THREADS) {  // e = (column slot, bin): hist[h][32] order
      const int cl = e >> 5, bin = e & 31;
      if (col0 + cl < h) hist[col0 * LS_BINS + e] += (int64_t)lhist[bin * LS_COLS + cl];
    }
  }
}

template <int DT>
static void ls_launch(const void* acts, int64_t ld, int64_t B, int64_t h, const int64_t* row_ids, int64_t row0, int k,
                      int64_t* count, float* sum, int64_t* hist, float* topk_val, int64_t* topk_row,
                      hipStream_t st) {
  const dim3 grid((unsigned)((h + LS_COLS - 1) / LS_COLS));
  if (k <= 4)
    hipLaunchKernelGGL((latent_stats_kernel<DT, 4, 16>), grid, dim3(1024), 0, st, acts, ld, (int)B, h, row_ids, row0, k, count,
                       sum, hist, topk_val, topk_row);
  else
    hipLaunchKernelGGL((latent_stats_kernel<DT, LS_MAX_K, 8>), grid, dim3(512), 0, st, acts, ld, (int)B, h, row_ids, row0, k,
                       count, sum, hist, topk_val, topk_row);
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_latent_stats_max_k(void) { return LS_MAX_K; }

int cc_latent_stats_update(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const int64_t* row_ids,
                           int64_t row0, int k, int64_t* count, float* sum, int64_t* hist, float* topk_val,
                           int64_t* topk_row, void* stream) {
  if (k < 1 || k > LS_MAX_K || h < 1 || ld < h || (ld & 1) || B < 1) return CC_ERR_SHAPE;
  if (!acts || !count || !sum || !topk_val || !topk_row) return CC_ERR_NULL;
  if (B > (1 << 30) || (h + LS_COLS - 1) / LS_COLS > 0x7fffffff) return CC_ERR_TOO_LARGE;
  if ((uintptr_t)acts & (dtype == CC_F32 ? 7 : 3)) return CC_ERR_ALIGN;  // one column pair per load
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CC_BF16)
    ls_launch<CC_BF16>(acts, ld, B, h, row_ids, row0, k, count, sum, hist, topk_val, topk_row, st);
  else if (dtype == CC_F32)
    ls_launch<CC_F32>(acts, ld, B, h, row_ids, row0, k, count, sum, hist, topk_val, topk_row, st);
  else
    return CC_ERR_DTYPE;
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
