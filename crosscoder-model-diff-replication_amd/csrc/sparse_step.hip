// The three kernels the sparse TopK training step adds to the pairs kernels (topk.hip, decode_pairs.hip, pairs_grad.hip;
// DESIGN.md section 3.20).  gfx950.  The range check, the chain orders, the staged gather and the grouped lists'
// pieces are pairs_common.h's.
//
// cc_pairs_group: the pairs idx [B][k] grouped by latent -> perm, seg (ops.pairs_by_latent's: flat slot numbers sorted by
//   (latent, row, slot)), a counting sort over cells (latent, row block of GRP_ROWS rows), five launches after a memset:
//     count   cells[j * nblk + b] += 1 per valid slot (integer atomics: a count does not depend on arrival order)
//     sums    the sum of every chunk of GRP_CHUNK cells
//     scan    cells <- their exclusive prefix sums in (latent, block) order: a workgroup adds the chunk sums before
//             its chunk, then scans the chunk (thread t owns GRP_ITEMS consecutive cells); seg[j] = the prefix at cell
//             (j, 0), seg[h] = the total
//     place   tmp[cells[cell]++] = slot: a cell's slots land in its range of tmp in arrival order, and afterwards
//             cells[c] is the end of cell c's range = the start of cell c + 1's
//     rank    one thread per valid slot p: perm[start + #(slots of its cell below p)] = p -- the slots of a cell are
//             distinct, so the ranks are a permutation of the range and the arrival order is gone.  A cell holds at most
//             GRP_ROWS entries where a row names a latent once (a latent that fires in every row is nblk cells of
//             GRP_ROWS, ranked by GRP_ROWS threads each); positions from seg[h] on are written as 0.
//
// cc_decode_pairs_partial: recon[r][c] (fp32) = cc_decode_pairs' chain from +0, no bias, no rounding: what the dense
//   cc_decode_partial hands to cc_loss_fwd_bwd.  cc_decode_pairs' form.
//
// cc_pairs_wgrad: both weight gradients and b_enc's from one walk of every latent's list, in the grouped lists' order
//   -- fma(val, g_recon) for dW_dec, fma(g_pre, x) for dW_enc, a plain add of g_pre for db_enc -- each rounded once
//   (launch 1 writes the full pieces' sums to the workspace, a row of 2 K + 8 floats per piece; launch 2 the rows).
//   g_pre is given in fp32 and rounded to the dtype where it is read (the step's d_acts pairs are cc_pairs_grad_values'
//   fp32 totals, rounded once).  Squared sums of the STORED values: a lane folds its elements in the order it stores
//   them (fma(r, r, sq)), the 64 lanes meet in the xor butterfly, thread 0 adds the four waves in order: one partial
//   per workgroup of launch 2 and parameter, at sq_*[blockIdx.x].
//
// cc_pairs_wgrad_add: cc_pairs_wgrad whose launch 2 also takes, for a latent with a compact slot (the dead set of the
//   AuxK loss, auxk_compact.hip), a row of three addends into the fp32 sums before the one rounding (pw_row_body<ADD>).
#include "pairs_common.h"

namespace cc {

// ---------------------------------------------------------------------------------------------- cc_pairs_group
constexpr int GRP_ROWS = 256;                        // rows of a row block
constexpr int GRP_ITEMS = 16;                        // consecutive cells of a thread of the scan
constexpr int GRP_CHUNK = PAIRS_THREADS * GRP_ITEMS;  // cells of a workgroup of the scan
constexpr int64_t GRP_MAX_CELLS = (int64_t)1 << 28;  // h * nblk: 2^16 chunks at the most
constexpr int GRP_GROUPS = 4096;                     // workgroups of the launches over the slots and over the chunks
constexpr int GRP_RANK_UNROLL = 4;

struct GroupDims {
  int64_t nblk, N, nchunks;
};
static GroupDims group_dims(int64_t B, int64_t h) {
  GroupDims g;
  g.nblk = (B + GRP_ROWS - 1) / GRP_ROWS;
  g.N = h * g.nblk;
  g.nchunks = (g.N + GRP_CHUNK - 1) / GRP_CHUNK;
  return g;
}
// cc_pairs_group's checks (ws: null for the sizing function)
static int group_check(const int32_t* idx, int64_t B, int k, int64_t h, const int32_t* perm, const int64_t* seg,
                       const void* ws, bool ptrs_ok) {
  // (no rows of K columns: n = 1, d = 8; the cells are counted only where h * nblk stays inside int64)
  const bool cells_ok = B <= INT32_MAX && h <= INT32_MAX && group_dims(B, h).N <= GRP_MAX_CELLS;
  return pairs_check(B, k, h, 1, 8, {}, true, 0, true, ptrs_ok, nullptr, cells_ok, {ws}, {idx, perm}, {seg});
}

__global__ __launch_bounds__(PAIRS_THREADS) void pg_count_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                                 uint32_t h, uint32_t nblk, uint32_t* __restrict__ cells) {
  for (uint32_t p = blockIdx.x * PAIRS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * PAIRS_THREADS) {
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) atomicAdd(cells + ((uint64_t)j * nblk + (p / k) / GRP_ROWS), 1u);
  }
}

__global__ __launch_bounds__(PAIRS_THREADS) void pg_sums_kernel(const uint32_t* __restrict__ cells, uint32_t N,
                                                                uint32_t* __restrict__ sums, uint32_t nchunks) {
  __shared__ uint32_t wred[PAIRS_NW];
  const int tid = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t s = 0u;
#pragma unroll
    for (int u = 0; u < GRP_ITEMS; ++u) {
      const uint32_t e = c * GRP_CHUNK + u * PAIRS_THREADS + tid;
      s += e < N ? cells[e] : 0u;
    }
    s = wave_sum_u(s);
    if ((tid & 63) == 0) wred[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) sums[c] = wred[0] + wred[1] + wred[2] + wred[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(PAIRS_THREADS) void pg_scan_kernel(uint32_t* __restrict__ cells, uint32_t N,
                                                                const uint32_t* __restrict__ sums, uint32_t nchunks,
                                                                uint32_t nblk, int64_t* __restrict__ seg, int64_t h) {
  __shared__ uint32_t wbase[PAIRS_NW];
  __shared__ uint32_t wtot[PAIRS_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t b = 0u;
    for (uint32_t i = tid; i < c; i += PAIRS_THREADS) b += sums[i];
    b = wave_sum_u(b);
    if (lane == 0) wbase[w] = b;
    const uint32_t e0 = c * GRP_CHUNK + tid * GRP_ITEMS;
    uint32_t v[GRP_ITEMS], local = 0u;
#pragma unroll
    for (int u = 0; u < GRP_ITEMS; ++u) {
      v[u] = e0 + u < N ? cells[e0 + u] : 0u;
      local += v[u];
    }
    // (its barrier also publishes wbase)
    CC_BLOCK_EXCL_SCAN(PAIRS_NW, local, lane, w, wtot, before, all);
    const uint32_t base = wbase[0] + wbase[1] + wbase[2] + wbase[3];
    uint32_t run = base + before;
#pragma unroll
    for (int u = 0; u < GRP_ITEMS; ++u) {
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

__global__ __launch_bounds__(PAIRS_THREADS) void pg_place_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                                 uint32_t h, uint32_t nblk, uint32_t* __restrict__ cells,
                                                                 uint32_t* __restrict__ tmp) {
  for (uint32_t p = blockIdx.x * PAIRS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * PAIRS_THREADS) {
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) {
      const uint32_t pos = atomicAdd(cells + ((uint64_t)j * nblk + (p / k) / GRP_ROWS), 1u);
      if (pos < Bk) tmp[pos] = p;  // (pos < the number of valid slots <= Bk by construction)
    }
  }
}

__global__ __launch_bounds__(PAIRS_THREADS) void pg_rank_kernel(const int32_t* __restrict__ idx, uint32_t Bk, uint32_t k,
                                                                uint32_t h, uint32_t nblk,
                                                                const uint32_t* __restrict__ cells, uint32_t N,
                                                                const uint32_t* __restrict__ tmp,
                                                                int32_t* __restrict__ perm) {
  const uint32_t last = cells[N - 1];
  const uint32_t total = last < Bk ? last : Bk;  // the valid slots
  for (uint32_t p = blockIdx.x * PAIRS_THREADS + threadIdx.x; p < Bk; p += gridDim.x * PAIRS_THREADS) {
    if (p >= total) perm[p] = 0;  // no segment's: any value inside [0, Bk)
    const uint32_t j = (uint32_t)idx[p];
    if (j < h) {
      const uint64_t c = (uint64_t)j * nblk + (p / k) / GRP_ROWS;
      uint32_t end = cells[c], start = c ? cells[c - 1] : 0u;
      end = end < total ? end : total;
      if (start >= end) continue;  // (never for scratch this call wrote)
      uint32_t rank = 0u;
      for (uint32_t q = start; q < end; q += GRP_RANK_UNROLL) {
        uint32_t t[GRP_RANK_UNROLL];
#pragma unroll
        for (int u = 0; u < GRP_RANK_UNROLL; ++u) t[u] = tmp[q + u < end ? q + u : end - 1];
#pragma unroll
        for (int u = 0; u < GRP_RANK_UNROLL; ++u) rank += (q + u < end && t[u] < p) ? 1u : 0u;
      }
      if (start + rank < end) perm[start + rank] = (int32_t)p;
    }
  }
}

// ---------------------------------------------------------------------------------------------- cc_decode_pairs_partial
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void decode_pairs_partial_kernel(
    const void* __restrict__ val, const int32_t* __restrict__ idx, int64_t B, int k, const void* __restrict__ W,
    int64_t ldw, uint32_t h, uint32_t ng, float* __restrict__ recon, int64_t ldr) {
  typedef typename Elem<DT>::T T;
  __shared__ PairStage st;
  const int tid = threadIdx.x;
  const uint32_t nch = (ng + PAIRS_THREADS - 1) / PAIRS_THREADS;

  for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
    const T* const vrow = (const T*)val + row * k;
    const int32_t* const irow = idx + row * k;
    int cnt = 0;  // in-range slots of the staged tile
    for (uint32_t c = 0; c < nch; ++c) {
      const uint32_t G = c * PAIRS_THREADS + tid;
      const bool on = G < ng;
      const int64_t col = (int64_t)G * 8;
      float acc[8];
      zero8(acc);
      stage_gather<DT>(st, vrow, irow, k, h, W, ldw, col, on, c == 0, cnt, acc);
      if (on) store_cols8(recon + row * ldr + col, acc);
    }
  }
}

// ---------------------------------------------------------------------------------------------- cc_pairs_wgrad
// launch 1: workspace row t = the sums of the full piece that starts in perm[t L .. (t + 1) L), if there is one
template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pw_piece_kernel(PairList a, int64_t P, const int64_t* __restrict__ seg,
                                                                 int64_t h, uint32_t ng, float* __restrict__ ws,
                                                                 int64_t nrows) {
  list_pieces<DT, true>(a, P, seg, h, ng, ws, nrows);
}

// launch 2: every row of dW_dec, dW_enc and db_enc, and the workgroup's squared-sum partials (one workspace row in
// flight: with PAIRS_UNROLL of them the kernel leaves the 4-waves-per-SIMD register bracket)
// ADD (cc_pairs_wgrad_add): a latent j with a compact slot s = slot[j] in [0, d_pad) takes row s of the addends in --
// float(aWd[s]), float(aWe[s]), float(ab[s]) added to the lane's fp32 sums after the list's and before the one
// rounding; the squared sums stay those of the stored values
struct PairAddend {
  const int32_t* slot;  // [h]
  const void* aWd;      // [d_pad][lda_d]
  const void* aWe;      // [d_pad][lda_e]
  const void* ab;       // [d_pad]
  int64_t lda_d, lda_e;
  uint32_t d_pad;
};

template <int DT, bool ADD>
CC_DEV void pw_row_body(const PairList& a, int64_t P, const int64_t* __restrict__ seg, int64_t h, uint32_t ng,
                        const float* __restrict__ ws, void* __restrict__ dWd, int64_t ldd, void* __restrict__ dWe,
                        int64_t lde, void* __restrict__ db, float* __restrict__ sq_dec, float* __restrict__ sq_enc,
                        float* __restrict__ sq_b, const PairAddend& ad) {
  typedef typename Elem<DT>::T T;
  __shared__ float wred[3][PAIRS_NW];
  float sqd = 0.f, sqe = 0.f, sqb = 0.f;
  for (int64_t j = blockIdx.x; j < h; j += gridDim.x) {
    const int64_t b = seg_at(seg, j, P), e = seg_at(seg, j + 1, P);
    for (uint32_t G = threadIdx.x; G < ng; G += PAIRS_THREADS) {
      const int64_t col = (int64_t)G * 8;
      ListAcc acc;
      list_sum<DT, true, 1>(a, b, e, ws, (int64_t)ng * 8, col, acc);
      if constexpr (ADD) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane(ad.slot[j]);
        if (s < ad.d_pad) {  // (uniform; -1 and anything outside the addends add nothing)
          float t[8];
          load8<DT>(ad.aWd, (int64_t)s * ad.lda_d + col, t);
          add8(acc.d, t);
          load8<DT>(ad.aWe, (int64_t)s * ad.lda_e + col, t);
          add8(acc.e, t);
          if (G == 0) acc.b += Elem<DT>::to_f(((const T*)ad.ab)[s]);
        }
      }
      store8<DT>(dWd, j * ldd + col, acc.d);
      store8<DT>(dWe, j * lde + col, acc.e);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float r = Elem<DT>::round(acc.d[c]);
        sqd = __builtin_fmaf(r, r, sqd);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float r = Elem<DT>::round(acc.e[c]);
        sqe = __builtin_fmaf(r, r, sqe);
      }
      if (G == 0) {  // (thread 0: K >= 8)
        const T q = Elem<DT>::from_f(acc.b);
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
    for (int q = 0; q < PAIRS_NW; ++q) {
      t[0] += wred[0][q];
      t[1] += wred[1][q];
      t[2] += wred[2][q];
    }
    sq_dec[blockIdx.x] = t[0];
    sq_enc[blockIdx.x] = t[1];
    sq_b[blockIdx.x] = t[2];
  }
}

template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pw_row_kernel(PairList a, int64_t P, const int64_t* __restrict__ seg,
                                                               int64_t h, uint32_t ng, const float* __restrict__ ws,
                                                               void* __restrict__ dWd, int64_t ldd, void* __restrict__ dWe,
                                                               int64_t lde, void* __restrict__ db, float* __restrict__ sq_dec,
                                                               float* __restrict__ sq_enc, float* __restrict__ sq_b) {
  pw_row_body<DT, false>(a, P, seg, h, ng, ws, dWd, ldd, dWe, lde, db, sq_dec, sq_enc, sq_b, PairAddend{});
}

template <int DT>
__global__ __launch_bounds__(PAIRS_THREADS) void pw_row_add_kernel(PairList a, int64_t P, const int64_t* __restrict__ seg,
                                                                   int64_t h, uint32_t ng, const float* __restrict__ ws,
                                                                   void* __restrict__ dWd, int64_t ldd,
                                                                   void* __restrict__ dWe, int64_t lde,
                                                                   void* __restrict__ db, float* __restrict__ sq_dec,
                                                                   float* __restrict__ sq_enc, float* __restrict__ sq_b,
                                                                   PairAddend ad) {
  pw_row_body<DT, true>(a, P, seg, h, ng, ws, dWd, ldd, dWe, lde, db, sq_dec, sq_enc, sq_b, ad);
}

static int64_t pw_groups(int64_t h) { return h < PAIRS_LIST_GROUPS ? h : PAIRS_LIST_GROUPS; }

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_pairs_group_ws_bytes(int64_t B, int k, int64_t h) {
  if (group_check(nullptr, B, k, h, nullptr, nullptr, nullptr, true) != CC_OK) return 0;
  const GroupDims g = group_dims(B, h);
  return (4 * (g.N + g.nchunks + B * k) + 15) / 16 * 16;
}

int cc_pairs_group(const int32_t* idx, int64_t B, int k, int64_t h, int32_t* perm, int64_t* seg, void* ws,
                   void* stream) {
  const int rc = group_check(idx, B, k, h, perm, seg, ws, idx && perm && seg && ws);
  if (rc != CC_OK) return rc;
  const GroupDims g = group_dims(B, h);
  const hipStream_t st = (hipStream_t)stream;
  uint32_t* const cells = (uint32_t*)ws;
  uint32_t* const sums = cells + g.N;
  uint32_t* const tmp = sums + g.nchunks;
  const uint32_t Bk = (uint32_t)(B * k), N = (uint32_t)g.N, nchunks = (uint32_t)g.nchunks, nblk = (uint32_t)g.nblk;
  const hipError_t e = hipMemsetAsync(cells, 0, (size_t)g.N * 4, st);
  if (e != hipSuccess) return CC_ERR_HIP_BASE + (int)e;
  const int64_t sb = ((int64_t)Bk + PAIRS_THREADS - 1) / PAIRS_THREADS;
  const dim3 sgrid((unsigned)(sb < GRP_GROUPS ? sb : GRP_GROUPS));
  const dim3 cgrid((unsigned)(g.nchunks < GRP_GROUPS ? g.nchunks : GRP_GROUPS)), block(PAIRS_THREADS);
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
  const int rc = pairs_check(B, k, h, 1, K, {ldw}, false, 0, true, val && idx && W_dec && recon, &dtype, true,
                             {W_dec, recon}, {idx}, {}, {val}, {ldr});
  if (rc != CC_OK) return rc;
  const dim3 grid((unsigned)(B < PAIRS_ROW_GROUPS ? B : PAIRS_ROW_GROUPS));
  hipLaunchKernelGGL(CC_BY_DTYPE(decode_pairs_partial_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, (hipStream_t)stream,
                     val, idx, B, k, W_dec, ldw, (uint32_t)h, (uint32_t)(K / 8), recon, ldr);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_pairs_wgrad_ws_floats(int64_t P, int64_t K) {
  if (P < PAIRS_SPLIT || K < 1) return 0;
  return (P / PAIRS_SPLIT) * piece_pitch<true>(K);
}

int64_t cc_pairs_wgrad_parts(int64_t h) { return h < 1 ? 0 : pw_groups(h); }

// cc_pairs_wgrad and cc_pairs_wgrad_add (ad: its addends, all given or all null; d_pad: their rows)
static int pairs_wgrad(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, const float* g_pre,
                       int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx, int64_t K, int dtype,
                       void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc, float* sq_dec,
                       float* sq_enc, float* sq_b_enc, float* ws, const PairAddend* ad, void* stream) {
  const int64_t nrows = P / PAIRS_SPLIT;
  const bool add = ad && (ad->slot || ad->aWd || ad->aWe || ad->ab);
  const bool ptrs_ok = seg && val && g_pre && g_recon && x && dW_dec && dW_enc && db_enc && sq_dec && sq_enc &&
                       sq_b_enc && (perm || P <= 0) && (ws || nrows <= 0) &&
                       (!add || (ad->slot && ad->aWd && ad->aWe && ad->ab));
  const bool add_shape = !add || (ad->d_pad >= 1 && ad->lda_d >= K && ad->lda_e >= K);
  int rc = pairs_check(B, k, h, 1, K, {ldg, ldx, ld_dec, ld_enc}, true, P, add_shape, ptrs_ok, &dtype,
                       !add || ad->d_pad <= (uint32_t)INT32_MAX, {g_recon, x, dW_dec, dW_enc, ws},
                       {perm, g_pre, sq_dec, sq_enc, sq_b_enc}, {seg}, {val, db_enc});
  if (rc != CC_OK) return rc;
  if (add) {  // the addends' own alignment: the two matrices and their pitches 16 bytes, slot 4, ab its element
    const int64_t es = dtype == CC_BF16 ? 2 : 4;
    if (!aligned({ad->aWd, ad->aWe}, 15) || (((ad->lda_d | ad->lda_e) * es) & 15) || !aligned({ad->slot}, 3) ||
        !aligned({ad->ab}, (uintptr_t)es - 1))
      return CC_ERR_ALIGN;
  }
  const PairList a{perm, val, g_pre, (uint32_t)(B * k), (uint32_t)k, g_recon, x, ldg, ldx};
  const uint32_t ng = (uint32_t)(K / 8);
  const hipStream_t st = (hipStream_t)stream;
  if (nrows > 0) {
    const dim3 grid((unsigned)(nrows < PAIRS_LIST_GROUPS ? nrows : PAIRS_LIST_GROUPS));
    hipLaunchKernelGGL(CC_BY_DTYPE(pw_piece_kernel, dtype), grid, dim3(PAIRS_THREADS), 0, st, a, P, seg, h, ng, ws, nrows);
    CC_LAUNCH_CHECK();
  }
  if (add)
    hipLaunchKernelGGL(CC_BY_DTYPE(pw_row_add_kernel, dtype), dim3((unsigned)pw_groups(h)), dim3(PAIRS_THREADS), 0, st, a,
                       P, seg, h, ng, ws, dW_dec, ld_dec, dW_enc, ld_enc, db_enc, sq_dec, sq_enc, sq_b_enc, *ad);
  else
    hipLaunchKernelGGL(CC_BY_DTYPE(pw_row_kernel, dtype), dim3((unsigned)pw_groups(h)), dim3(PAIRS_THREADS), 0, st, a, P,
                       seg, h, ng, ws, dW_dec, ld_dec, dW_enc, ld_enc, db_enc, sq_dec, sq_enc, sq_b_enc);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_pairs_wgrad(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, const float* g_pre,
                   int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx, int64_t K, int dtype,
                   void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc, float* sq_dec,
                   float* sq_enc, float* sq_b_enc, float* ws, void* stream) {
  return pairs_wgrad(perm, P, seg, h, val, g_pre, B, k, g_recon, ldg, x, ldx, K, dtype, dW_dec, ld_dec, dW_enc, ld_enc,
                     db_enc, sq_dec, sq_enc, sq_b_enc, ws, nullptr, stream);
}

int cc_pairs_wgrad_add(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val,
                       const float* g_pre, int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx,
                       int64_t K, int dtype, void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc,
                       float* sq_dec, float* sq_enc, float* sq_b_enc, float* ws, const int32_t* slot, int64_t d_pad,
                       const void* aWd, int64_t lda_d, const void* aWe, int64_t lda_e, const void* ab, void* stream) {
  const bool big = d_pad > INT32_MAX;
  const PairAddend ad{slot, aWd, aWe, ab, lda_d, lda_e, (uint32_t)(d_pad < 0 ? 0 : (big ? 0xffffffffu : d_pad))};
  return pairs_wgrad(perm, P, seg, h, val, g_pre, B, k, g_recon, ldg, x, ldx, K, dtype, dW_dec, ld_dec, dW_enc, ld_enc,
                     db_enc, sq_dec, sq_enc, sq_b_enc, ws, &ad, stream);
}

}  // extern "C"
