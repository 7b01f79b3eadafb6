// The three kernels the sparse TopK training step adds to the pairs kernels (topk.hip, decode_pairs.hip, pairs_grad.hip;
// DESIGN.md section 3.20).  gfx950.  No float atomics, no spin waits; every float summation order below is fixed by the
// arguments alone, so two calls give equal bits.
//
// cc_pairs_group: the pairs idx [B][k] grouped by latent -> perm, seg (ops.pairs_by_latent's: flat slot numbers sorted by
//   (latent, row, slot)), a counting sort over cells (latent, row block of PG_ROWS rows), five launches after a memset:
//     count   cells[j * nblk + b] += 1 per valid slot (integer atomics: a count does not depend on arrival order)
//     sums    the sum of every chunk of PG_CHUNK cells
//     scan    cells <- their exclusive prefix sums in (latent, block) order: a workgroup adds the chunk sums before
//             its chunk, then scans the chunk (thread t owns PG_ITEMS consecutive cells); seg[j] = the prefix at cell
//             (j, 0), seg[h] = the total
//     place   tmp[cells[cell]++] = slot: a cell's slots land in its range of tmp in arrival order, and afterwards
//             cells[c] is the end of cell c's range = the start of cell c + 1's
//     rank    one thread per valid slot p: perm[start + #(slots of its cell below p)] = p -- the slots of a cell are
//             distinct, so the ranks are a permutation of the range and the arrival order is gone.  A cell holds at most
//             PG_ROWS entries where a row names a latent once (a latent that fires in every row is nblk cells of
//             PG_ROWS, ranked by PG_ROWS threads each); positions from seg[h] on are written as 0.
//
// cc_decode_pairs_partial: recon[r][c] (fp32) = the fp32 fma chain +0 + sum_s val[r][s] * W_dec[idx[r][s]][c] over the
//   slots in order, no bias, no rounding: cc_decode_pairs' chain from +0, what the dense cc_decode_partial hands to
//   cc_loss_fwd_bwd.  cc_decode_pairs' form (the row's in-range pairs compacted in slot order in LDS, DP_UNROLL
//   decoder rows in flight).
//
// cc_pairs_wgrad: both weight gradients and b_enc's from one walk of every latent's list, in cc_pairs_grad_decoder's
//   order (pairs_grad.hip): a list of at most L = CC_PAIRS_GRAD_SPLIT entries is one fp32 chain per element from +0 in
//   list order -- fma(val, g_recon) for dW_dec, fma(g_pre, x) for dW_enc, a plain add of g_pre for db_enc -- rounded
//   once; a longer list in pieces of L (launch 1 writes the full pieces' sums to the workspace, a row of 2 K + 8
//   floats per piece; launch 2 adds them in piece order onto +0, then the last, shorter piece, and rounds once).
//   g_pre is given in fp32 and rounded to the dtype where it is read (the step's d_acts pairs are cc_pairs_grad_values'
//   fp32 totals, rounded once).  The list entry and its two coefficients are wave-uniform and read once for both
//   gradients.  Squared sums of the STORED values: a lane folds its elements in the order it stores them
//   (fma(r, r, sq)), the 64 lanes meet in the xor butterfly, thread 0 adds the four waves in order: one partial per
//   workgroup of launch 2 and parameter, at sq_*[blockIdx.x].
#include "mask_common.h"

namespace cc {

constexpr int SS_THREADS = 256;
constexpr int SS_NW = SS_THREADS / 64;
constexpr int64_t SS_MAX_GROUPS = 1 << 16;

// ---------------------------------------------------------------------------------------------- cc_pairs_group
constexpr int PG_ROWS = 256;                        // rows of a row block
constexpr int PG_ITEMS = 16;                        // consecutive cells of a thread of the scan
constexpr int PG_CHUNK = SS_THREADS * PG_ITEMS;     // cells of a workgroup of the scan
constexpr int64_t PG_MAX_CELLS = (int64_t)1 << 28;  // h * nblk: 2^16 chunks at the most
constexpr int PG_SLOT_GROUPS = 4096;                // workgroups of the launches over the slots
constexpr int PG_RANK_UNROLL = 4;

struct GroupDims {
  int64_t nblk, N, nchunks;
};
static GroupDims group_dims(int64_t B, int64_t h) {
  GroupDims g;
  g.nblk = (B + PG_ROWS - 1) / PG_ROWS;
  g.N = h * g.nblk;
  g.nchunks = (g.N + PG_CHUNK - 1) / PG_CHUNK;
  return g;
}

__global__ __launch_bounds__(SS_THREADS) void pg_count_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                              uint32_t h, uint32_t nblk, uint32_t* __restrict__ cells) {
  for (uint32_t p = blockIdx.x * SS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * SS_THREADS) {
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) atomicAdd(cells + ((uint64_t)j * nblk + (p / k) / PG_ROWS), 1u);
  }
}

__global__ __launch_bounds__(SS_THREADS) void pg_sums_kernel(const uint32_t* __restrict__ cells, uint32_t N,
                                                             uint32_t* __restrict__ sums, uint32_t nchunks) {
  __shared__ uint32_t wred[SS_NW];
  const int tid = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t s = 0u;
#pragma unroll
    for (int u = 0; u < PG_ITEMS; ++u) {
      const uint32_t e = c * PG_CHUNK + u * SS_THREADS + tid;
      s += e < N ? cells[e] : 0u;
    }
    s = wave_sum_u(s);
    if ((tid & 63) == 0) wred[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) sums[c] = wred[0] + wred[1] + wred[2] + wred[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(SS_THREADS) void pg_scan_kernel(uint32_t* __restrict__ cells, uint32_t N,
                                                             const uint32_t* __restrict__ sums, uint32_t nchunks,
                                                             uint32_t nblk, int64_t* __restrict__ seg, int64_t h) {
  __shared__ uint32_t wbase[SS_NW];
  __shared__ uint32_t wtot[SS_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t b = 0u;
    for (uint32_t i = tid; i < c; i += SS_THREADS) b += sums[i];
    b = wave_sum_u(b);
    if (lane == 0) wbase[w] = b;
    const uint32_t e0 = c * PG_CHUNK + tid * PG_ITEMS;
    uint32_t v[PG_ITEMS], local = 0u;
#pragma unroll
    for (int u = 0; u < PG_ITEMS; ++u) {
      v[u] = e0 + u < N ? cells[e0 + u] : 0u;
      local += v[u];
    }
    // (its barrier also publishes wbase)
    CC_BLOCK_EXCL_SCAN(SS_NW, local, lane, w, wtot, before, all);
    const uint32_t base = wbase[0] + wbase[1] + wbase[2] + wbase[3];
    uint32_t run = base + before;
#pragma unroll
    for (int u = 0; u < PG_ITEMS; ++u) {
      const uint32_t e = e0 + u;
      if (e < N) {
        cells[e] = run;
        if (e % nblk == 0u) seg[e / nblk] = (int64_t)run;
        run += v[u];
      }
    }
    if (c == nchunks - 1 && tid == 0) seg[h] = (int64_t)(base + all);
    __syncthreads();  // (wbase / wtot are rewritten by the next chunk)
  }
}

__global__ __launch_bounds__(SS_THREADS) void pg_place_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                              uint32_t h, uint32_t nblk, uint32_t* __restrict__ cells,
                                                              uint32_t* __restrict__ tmp) {
  for (uint32_t p = blockIdx.x * SS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * SS_THREADS) {
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) {
      const uint32_t pos = atomicAdd(cells + ((uint64_t)j * nblk + (p / k) / PG_ROWS), 1u);
      if (pos < Bk) tmp[pos] = p;  // (pos < the number of valid slots <= Bk by construction)
    }
  }
}

__global__ __launch_bounds__(SS_THREADS) void pg_rank_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                             uint32_t h, uint32_t nblk, const uint32_t* __restrict__ cells,
                                                             uint32_t N, const uint32_t* __restrict__ tmp,
                                                             int32_t* __restrict__ perm) {
  const uint32_t last = cells[N - 1];
  const uint32_t total = last < Bk ? last : Bk;  // the valid slots
  for (uint32_t p = blockIdx.x * SS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * SS_THREADS) {
    if (p >= total) perm[p] = 0;  // no segment's: any value inside [0, Bk)
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) {
      const uint64_t c = (uint64_t)j * nblk + (p / k) / PG_ROWS;
      uint32_t end = cells[c], start = c ? cells[c - 1] : 0u;
      end = end < total ? end : total;
      if (start >= end) continue;  // (never for scratch this call wrote)
      uint32_t rank = 0u;
      for (uint32_t q = start; q < end; q += PG_RANK_UNROLL) {
        uint32_t t[PG_RANK_UNROLL];
#pragma unroll
        for (int u = 0; u < PG_RANK_UNROLL; ++u) t[u] = tmp[q + u < end ? q + u : end - 1];
#pragma unroll
        for (int u = 0; u < PG_RANK_UNROLL; ++u) rank += (q + u < end && t[u] < p) ? 1u : 0u;
      }
      if (start + rank < end) perm[start + rank] = (int32_t)p;
    }
  }
}

// ---------------------------------------------------------------------------------------------- cc_decode_pairs_partial
constexpr int DPP_TILE = SS_THREADS;  // slots staged at a time: one per lane
constexpr int DPP_UNROLL = 4;         // W_dec rows in flight per lane
constexpr int DPP_MAX_GROUPS = 2048;

template <int DT>
__global__ __launch_bounds__(SS_THREADS) void decode_pairs_partial_kernel(
    const void* __restrict__ val, const int32_t* __restrict__ idx, int64_t B, int k, const void* __restrict__ W,
    int64_t ldw, uint32_t h, uint32_t ng, float* __restrict__ recon, int64_t ldr) {
  typedef typename Elem<DT>::T T;
  __shared__ int32_t s_idx[DPP_TILE];
  __shared__ float s_val[DPP_TILE];
  __shared__ uint32_t s_wtot[SS_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t nch = (ng + SS_THREADS - 1) / SS_THREADS;

  for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
    const T* const vrow = (const T*)val + row * k;
    const int32_t* const irow = idx + row * k;
    int cnt = 0;  // in-range slots of the staged tile
    for (uint32_t c = 0; c < nch; ++c) {
      const uint32_t G = c * SS_THREADS + tid;
      const bool on = G < ng;
      const int64_t col = (int64_t)G * 8;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int t0 = 0; t0 < k; t0 += DPP_TILE) {
        if (c == 0 || k > DPP_TILE) {  // (uniform) stage the tile: the in-range pairs, compacted in slot order
          const int s = t0 + tid;
          const int32_t i = s < k ? irow[s] : -1;
          const bool ok = (uint32_t)i < h;
          const uint32_t one = ok ? 1u : 0u;
          // (its barrier also ends the previous tile's reads of s_idx / s_val)
          CC_BLOCK_EXCL_SCAN(SS_NW, one, lane, w, s_wtot, before, all);
          if (ok) {
            s_idx[before] = i;
            s_val[before] = Elem<DT>::to_f(vrow[s]);
          }
          __syncthreads();
          cnt = (int)all;
        }
        for (int s0 = 0; s0 < cnt; s0 += DPP_UNROLL) {
          Vec8<DT> wv[DPP_UNROLL];
          float v[DPP_UNROLL];
#pragma unroll
          for (int u = 0; u < DPP_UNROLL; ++u) {
            if (s0 + u < cnt) {  // (uniform)
              const int64_t i = __builtin_amdgcn_readfirstlane(s_idx[s0 + u]);
              v[u] = s_val[s0 + u];
              wv[u] = load_vec8<DT>(W, i * ldw + col, on);
            }
          }
#pragma unroll
          for (int u = 0; u < DPP_UNROLL; ++u) {
            if (s0 + u < cnt) {
              uint32_t b[8];
              vec8_bits<DT>(wv[u], b);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v[u], bits_float<DT>(b[j]), acc[j]);
            }
          }
        }
      }
      if (on) store_cols8(recon + row * ldr + col, acc);
    }
  }
}

// ---------------------------------------------------------------------------------------------- cc_pairs_wgrad
constexpr int64_t PW_SPLIT = CC_PAIRS_GRAD_SPLIT;
constexpr int PW_UNROLL = 4;  // list entries (a row of g_recon and one of x each) in flight per lane

struct PwList {
  const int32_t* perm;
  const void* val;     // [B k] dtype
  const float* gpre;   // [B k] fp32, rounded to the dtype where read
  uint32_t Bk, k;
  const void* g;       // g_recon [B][ldg]
  const void* x;       // [B][ldx]
  int64_t ldg, ldx;
};

CC_DEV int64_t pw_seg_at(const int64_t* __restrict__ seg, int64_t j, int64_t P) {
  const int64_t v = seg[j];
  return v < 0 ? 0 : (v > P ? P : v);
}

// the chains over perm[p0 .. p1) in order onto ad (dW_dec), ae (dW_enc), the 8 columns at col, and ab (db_enc);
// entries outside [0, Bk) are skipped
template <int DT>
CC_DEV void pw_chain(const PwList& a, int64_t p0, int64_t p1, int64_t col, float (&ad)[8], float (&ae)[8], float& ab) {
  typedef typename Elem<DT>::T T;
  for (int64_t q0 = p0; q0 < p1; q0 += PW_UNROLL) {
    Vec8<DT> gv[PW_UNROLL], xv[PW_UNROLL];
    float v[PW_UNROLL], p[PW_UNROLL];
    bool ok[PW_UNROLL];
#pragma unroll
    for (int u = 0; u < PW_UNROLL; ++u) {
      ok[u] = false;
      if (q0 + u < p1) {  // (uniform)
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane(a.perm[q0 + u]);
        ok[u] = slot < a.Bk;
        if (ok[u]) {
          const int64_t row = (int64_t)(slot / a.k);
          v[u] = Elem<DT>::to_f(((const T*)a.val)[slot]);
          p[u] = Elem<DT>::round(a.gpre[slot]);
          gv[u] = load_vec8<DT>(a.g, row * a.ldg + col, true);
          xv[u] = load_vec8<DT>(a.x, row * a.ldx + col, true);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PW_UNROLL; ++u) {
      if (ok[u]) {
        uint32_t bg[8], bx[8];
        vec8_bits<DT>(gv[u], bg);
        vec8_bits<DT>(xv[u], bx);
#pragma unroll
        for (int j = 0; j < 8; ++j) ad[j] = __builtin_fmaf(v[u], bits_float<DT>(bg[j]), ad[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) ae[j] = __builtin_fmaf(p[u], bits_float<DT>(bx[j]), ae[j]);
        ab += p[u];
      }
    }
  }
}

CC_DEV void zero8(float (&a)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
}

// launch 1: workspace row t = the sums of the full piece that starts in perm[t L .. (t + 1) L), if there is one
// (pgd_piece_kernel's search); a row is [K dW_dec | K dW_enc | db_enc, 7 unused]
template <int DT>
__global__ __launch_bounds__(SS_THREADS) void pw_piece_kernel(PwList a, int64_t P, const int64_t* __restrict__ seg,
                                                              int64_t h, uint32_t ng, float* __restrict__ ws,
                                                              int64_t nrows) {
  constexpr int64_t L = PW_SPLIT;
  const int64_t K = (int64_t)ng * 8, pitch = 2 * K + 8;
  for (int64_t t = blockIdx.x; t < nrows; t += gridDim.x) {
    const int64_t x = t * L + L - 1;  // (< P: nrows = P / L)
    int64_t lo = 0, hi = h;
    while (hi - lo > 1) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (pw_seg_at(seg, mid, P) <= x) lo = mid; else hi = mid;
    }
    const int64_t b = pw_seg_at(seg, lo, P), e = pw_seg_at(seg, lo + 1, P);
    if (e - b <= L || b > x) continue;
    const int64_t s = b >= t * L ? b : b + (t * L - b + L - 1) / L * L;
    if (s > x || s + L > e) continue;
    float* const wrow = ws + t * pitch;
    for (uint32_t G = threadIdx.x; G < ng; G += SS_THREADS) {
      float ad[8], ae[8], ab = 0.f;
      zero8(ad);
      zero8(ae);
      pw_chain<DT>(a, s, s + L, (int64_t)G * 8, ad, ae, ab);
      store_cols8(wrow + (int64_t)G * 8, ad);
      store_cols8(wrow + K + (int64_t)G * 8, ae);
      if (G == 0) wrow[2 * K] = ab;
    }
  }
}

// launch 2: every row of dW_dec, dW_enc and db_enc, and the workgroup's squared-sum partials
template <int DT>
__global__ __launch_bounds__(SS_THREADS) void pw_row_kernel(PwList a, int64_t P, const int64_t* __restrict__ seg,
                                                            int64_t h, uint32_t ng, const float* __restrict__ ws,
                                                            void* __restrict__ dWd, int64_t ldd, void* __restrict__ dWe,
                                                            int64_t lde, void* __restrict__ db, float* __restrict__ sq_dec,
                                                            float* __restrict__ sq_enc, float* __restrict__ sq_b) {
  typedef typename Elem<DT>::T T;
  constexpr int64_t L = PW_SPLIT;
  __shared__ float wred[3][SS_NW];
  const int64_t K = (int64_t)ng * 8, pitch = 2 * K + 8;
  float sqd = 0.f, sqe = 0.f, sqb = 0.f;
  for (int64_t j = blockIdx.x; j < h; j += gridDim.x) {
    const int64_t b = pw_seg_at(seg, j, P), e = pw_seg_at(seg, j + 1, P);
    for (uint32_t G = threadIdx.x; G < ng; G += SS_THREADS) {
      const int64_t col = (int64_t)G * 8;
      float ad[8], ae[8], ab = 0.f;
      zero8(ad);
      zero8(ae);
      if (e - b <= L) {  // (uniform; an empty or reversed segment leaves +0)
        pw_chain<DT>(a, b, e, col, ad, ae, ab);
      } else {
        const int64_t nfull = (e - b) / L;
        for (int64_t q = 0; q < nfull; ++q) {
          const float* const wrow = ws + ((b + q * L) / L) * pitch;
          float pd[8], pe[8];
          load8f(wrow, col, pd);
          load8f(wrow, K + col, pe);
          const float pb = wrow[2 * K];
#pragma unroll
          for (int c = 0; c < 8; ++c) ad[c] += pd[c];
#pragma unroll
          for (int c = 0; c < 8; ++c) ae[c] += pe[c];
          ab += pb;
        }
        if (b + nfull * L < e) {
          float ld_[8], le[8], lb = 0.f;
          zero8(ld_);
          zero8(le);
          pw_chain<DT>(a, b + nfull * L, e, col, ld_, le, lb);
#pragma unroll
          for (int c = 0; c < 8; ++c) ad[c] += ld_[c];
#pragma unroll
          for (int c = 0; c < 8; ++c) ae[c] += le[c];
          ab += lb;
        }
      }
      store8<DT>(dWd, j * ldd + col, ad);
      store8<DT>(dWe, j * lde + col, ae);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float r = Elem<DT>::round(ad[c]);
        sqd = __builtin_fmaf(r, r, sqd);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float r = Elem<DT>::round(ae[c]);
        sqe = __builtin_fmaf(r, r, sqe);
      }
      if (G == 0) {  // (thread 0: K >= 8)
        const T q = Elem<DT>::from_f(ab);
        ((T*)db)[j] = q;
        const float r = Elem<DT>::to_f(q);
        sqb = __builtin_fmaf(r, r, sqb);
      }
    }
  }
  sqd = wave_sum(sqd);
  sqe = wave_sum(sqe);
  sqb = wave_sum(sqb);
  if ((threadIdx.x & 63) == 0) {
    wred[0][threadIdx.x >> 6] = sqd;
    wred[1][threadIdx.x >> 6] = sqe;
    wred[2][threadIdx.x >> 6] = sqb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < SS_NW; ++q) {
      t[0] += wred[0][q];
      t[1] += wred[1][q];
      t[2] += wred[2][q];
    }
    sq_dec[blockIdx.x] = t[0];
    sq_enc[blockIdx.x] = t[1];
    sq_b[blockIdx.x] = t[2];
  }
}

static int64_t pw_groups(int64_t h) { return h < SS_MAX_GROUPS ? h : SS_MAX_GROUPS; }

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_pairs_group_ws_bytes(int64_t B, int k, int64_t h) {
  if (B < 1 || k < 1 || h < 1 || h > INT32_MAX || k > (1 << 17) || B > INT32_MAX / k) return 0;
  const GroupDims g = group_dims(B, h);
  if (g.N > PG_MAX_CELLS) return 0;
  return (4 * (g.N + g.nchunks + B * k) + 15) / 16 * 16;
}

int cc_pairs_group(const int32_t* idx, int64_t B, int k, int64_t h, int32_t* perm, int64_t* seg, void* ws,
                   void* stream) {
  if (B < 1 || k < 1 || h < 1) return CC_ERR_SHAPE;
  if (!idx || !perm || !seg || !ws) return CC_ERR_NULL;
  if (h > INT32_MAX || k > (1 << 17) || B > INT32_MAX / k) return CC_ERR_TOO_LARGE;
  const GroupDims g = group_dims(B, h);
  if (g.N > PG_MAX_CELLS) return CC_ERR_TOO_LARGE;
  if (!aligned({ws}, 15) || !aligned({seg}, 7) || !aligned({idx, perm}, 3)) return CC_ERR_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* const cells = (uint32_t*)ws;
  uint32_t* const sums = cells + g.N;
  uint32_t* const tmp = sums + g.nchunks;
  const uint32_t Bk = (uint32_t)(B * k), N = (uint32_t)g.N, nchunks = (uint32_t)g.nchunks, nblk = (uint32_t)g.nblk;
  const hipError_t e = hipMemsetAsync(cells, 0, (size_t)g.N * 4, st);
  if (e != hipSuccess) return CC_ERR_HIP_BASE + (int)e;
  const int64_t sb = ((int64_t)Bk + SS_THREADS - 1) / SS_THREADS;
  const dim3 sgrid((unsigned)(sb < PG_SLOT_GROUPS ? sb : PG_SLOT_GROUPS));
  const dim3 cgrid((unsigned)(g.nchunks < 4096 ? g.nchunks : 4096)), block(SS_THREADS);
  hipLaunchKernelGGL(pg_count_kernel, sgrid, block, 0, st, idx, Bk, (uint32_t)k, (uint32_t)h, nblk, cells);
  CC_LAUNCH_CHECK();
  hipLaunchKernelGGL(pg_sums_kernel, cgrid, block, 0, st, cells, N, sums, nchunks);
  CC_LAUNCH_CHECK();
  hipLaunchKernelGGL(pg_scan_kernel, cgrid, block, 0, st, cells, N, sums, nchunks, nblk, seg, h);
  CC_LAUNCH_CHECK();
  hipLaunchKernelGGL(pg_place_kernel, sgrid, block, 0, st, idx, Bk, (uint32_t)k, (uint32_t)h, nblk, cells, tmp);
  CC_LAUNCH_CHECK();
  hipLaunchKernelGGL(pg_rank_kernel, sgrid, block, 0, st, idx, Bk, (uint32_t)k, (uint32_t)h, nblk, cells, N, tmp, perm);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_decode_pairs_partial(const void* val, const int32_t* idx, int64_t B, int k, const void* W_dec, int64_t ldw,
                            int64_t h, int64_t K, int dtype, float* recon, int64_t ldr, void* stream) {
  if (B < 1 || k < 1 || h < 1 || K < 8 || (K & 7) || ldw < K || ldr < K) return CC_ERR_SHAPE;
  if (!val || !idx || !W_dec || !recon) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > (1 << 17) || K > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({W_dec, recon}, 15) || ((ldw * es) & 15) || ((ldr * 4) & 15) || !aligned({idx}, 3) ||
      !aligned({val}, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  const dim3 grid((unsigned)(B < DPP_MAX_GROUPS ? B : DPP_MAX_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(decode_pairs_partial_kernel, dtype), grid, dim3(SS_THREADS), 0, (hipStream_t)stream,
                     val, idx, B, k, W_dec, ldw, (uint32_t)h, (uint32_t)(K / 8), recon, ldr);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_pairs_wgrad_ws_floats(int64_t P, int64_t K) {
  if (P < PW_SPLIT || K < 1) return 0;
  return (P / PW_SPLIT) * (2 * K + 8);
}

int64_t cc_pairs_wgrad_parts(int64_t h) { return h < 1 ? 0 : pw_groups(h); }

int cc_pairs_wgrad(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, const float* g_pre,
                   int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx, int64_t K, int dtype,
                   void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc, float* sq_dec,
                   float* sq_enc, float* sq_b_enc, float* ws, void* stream) {
  if (B < 1 || k < 1 || h < 1 || P < 0 || K < 8 || (K & 7) || ldg < K || ldx < K || ld_dec < K || ld_enc < K)
    return CC_ERR_SHAPE;
  const int64_t nrows = P / PW_SPLIT;
  if (!seg || !val || !g_pre || !g_recon || !x || !dW_dec || !dW_enc || !db_enc || !sq_dec || !sq_enc || !sq_b_enc ||
      (!perm && P > 0) || (!ws && nrows > 0))
    return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > (1 << 17) || B > INT32_MAX / k || P > INT32_MAX || K > INT32_MAX) return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({g_recon, x, dW_dec, dW_enc, ws}, 15) || (((ldg | ldx | ld_dec | ld_enc) * es) & 15) ||
      !aligned({seg}, 7) || !aligned({perm, g_pre, sq_dec, sq_enc, sq_b_enc}, 3) ||
      !aligned({val, db_enc}, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  const PwList a{perm, val, g_pre, (uint32_t)(B * k), (uint32_t)k, g_recon, x, ldg, ldx};
  const uint32_t ng = (uint32_t)(K / 8);
  const hipStream_t st = (hipStream_t)stream;
  if (nrows > 0) {
    const dim3 grid((unsigned)(nrows < SS_MAX_GROUPS ? nrows : SS_MAX_GROUPS));
    hipLaunchKernelGGL(CC_BY_DTYPE(pw_piece_kernel, dtype), grid, dim3(SS_THREADS), 0, st, a, P, seg, h, ng, ws, nrows);
    CC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(CC_BY_DTYPE(pw_row_kernel, dtype), dim3((unsigned)pw_groups(h)), dim3(SS_THREADS), 0, st, a, P, seg,
                     h, ng, ws, dW_dec, ld_dec, dW_enc, ld_enc, db_enc, sq_dec, sq_enc, sq_b_enc);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
