// The compacted dead set of the sparse TopK step's AuxK loss.  gfx950.
//   cc_dead_compact    the dead latents of tokens_since_fired in ascending order -> ids [D_pad], slot [h], their count
//   cc_compact_gather  Wc[c] = W[ids[c]] (whole rows) and / or acts_c[r][c] = acts[r][ids[c]] (columns): bit copies,
//                      +0 where ids[c] is no latent
// (cc_pairs_wgrad_add, the list gradients that take the compact gradient rows in, is sparse_step.hip's.)
// No atomics: the order of ids is the latents' own (a scan), and every output element has one writer.
#include "mask_common.h"

namespace cc {

// ---------------------------------------------------------------------------------------------- cc_dead_compact
// One workgroup (cc_dead_update's form: h <= 2^17).  A tile is DC_NT consecutive latents, one per thread; its dead
// latents per wave come from one ballot.  Pass 1 counts every (tile, wave), the counts are scanned in that order --
// which is the latents' order -- and pass 2 reads the state again (1 MB at the most, from the L2) and places the
// latents: position = the scanned count + the dead lanes below this one.
constexpr int DC_NT = 1024;
constexpr int DC_NW = DC_NT / 64;
constexpr int DC_MAX_TILES = MASK_MAX_H / DC_NT;   // 128
constexpr int DC_CELLS = DC_MAX_TILES * DC_NW;     // 2048 (tile, wave) counts: two per thread

__global__ __launch_bounds__(DC_NT) void dead_compact_kernel(const int64_t* __restrict__ since_fired, int h, int h_real,
                                                             int64_t dead_after, int32_t* __restrict__ ids, int d_pad,
                                                             int32_t* __restrict__ slot, uint32_t* __restrict__ count) {
  __shared__ uint32_t cells[DC_CELLS];
  __shared__ uint32_t wtot[DC_NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ntiles = (h + DC_NT - 1) / DC_NT;
  cells[tid] = 0u;
  cells[tid + DC_NT] = 0u;
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int l = t * DC_NT + tid;
    const bool dead = l < h_real && since_fired[l] >= dead_after;  // (h_real <= h; padding latents are never dead)
    const uint64_t m = __ballot(dead);
    if (lane == 0) cells[t * DC_NW + w] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  // exclusive scan of the cells in (tile, wave) order: thread t owns cells 2 t and 2 t + 1
  const uint32_t c0 = cells[2 * tid], c1 = cells[2 * tid + 1];
  const uint32_t mine = c0 + c1;
  CC_BLOCK_EXCL_SCAN(DC_NW, mine, lane, w, wtot, before, all);
  cells[2 * tid] = before;
  cells[2 * tid + 1] = before + c0;
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int l = t * DC_NT + tid;
    const bool dead = l < h_real && since_fired[l] >= dead_after;
    const uint64_t m = __ballot(dead);
    if (l < h) {
      const uint32_t pos = cells[t * DC_NW + w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const bool placed = dead && pos < (uint32_t)d_pad;  // (a count above d_pad: the rest is dropped, never written)
      if (placed) ids[pos] = l;
      slot[l] = placed ? (int32_t)pos : -1;
    }
  }
  for (int c = (int)all + tid; c < d_pad; c += DC_NT) ids[c] = -1;
  if (tid == 0) *count = all;
}

// ---------------------------------------------------------------------------------------------- cc_compact_gather
// Rows: workgroup c copies row ids[c] of W, 16 bytes per lane and step.
constexpr int CG_NT = 256;

__global__ __launch_bounds__(CG_NT) void gather_rows_kernel(const int32_t* __restrict__ ids, int64_t d_pad,
                                                            uint32_t h, const uint4* __restrict__ W, int64_t ldw16,
                                                            uint4* __restrict__ Wc, int64_t ldc16, int row16) {
  for (int64_t c = blockIdx.x; c < d_pad; c += gridDim.x) {
    const uint32_t j = (uint32_t)ids[c];
    const bool ok = j < h;  // the range check: -1 and anything >= h give a +0 row
    for (int v = threadIdx.x; v < row16; v += CG_NT)
      Wc[c * ldc16 + v] = ok ? W[(int64_t)j * ldw16 + v] : uint4{0u, 0u, 0u, 0u};
  }
}

// Columns: a workgroup takes CG_COLS compact columns of a block of rows.  A lane keeps the CG_PER latents of columns
// c0 + u CG_NT + tid in registers (staged once for all its rows), so the lanes of a wave read ascending addresses of one
// row -- the dead latents lie ~h / D elements apart and neighbouring lanes share cache lines -- and the elements go
// through an LDS tile so that every lane stores 8 consecutive columns as 16-byte vectors.  CG_RB rows are in flight.
constexpr int CG_PER = 8;
constexpr int CG_COLS = CG_NT * CG_PER;  // 2048
constexpr int CG_RB = 4;
constexpr int CG_ROWS = 32;  // rows of a workgroup

template <int DT>
__global__ __launch_bounds__(CG_NT) void gather_cols_kernel(const int32_t* __restrict__ ids, int d_pad, uint32_t h,
                                                            const void* __restrict__ acts, int64_t lda, int64_t B,
                                                            void* __restrict__ out) {
  typedef typename Elem<DT>::T T;
  __shared__ __attribute__((aligned(16))) T tile[CG_RB][CG_COLS];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * CG_COLS;
  uint32_t id[CG_PER];
#pragma unroll
  for (int u = 0; u < CG_PER; ++u) {
    const int c = c0 + u * CG_NT + tid;
    id[u] = c < d_pad ? (uint32_t)ids[c] : 0xffffffffu;
  }
  const int cw = c0 + tid * CG_PER;  // the 8 columns this lane stores (d_pad % 8 == 0: all of them or none)
  const int64_t r_end = min(B, ((int64_t)blockIdx.y + 1) * CG_ROWS);
  for (int64_t r0 = (int64_t)blockIdx.y * CG_ROWS; r0 < r_end; r0 += CG_RB) {
    T v[CG_RB][CG_PER];
#pragma unroll
    for (int q = 0; q < CG_RB; ++q) {
      const bool row_ok = r0 + q < r_end;
      const T* const src = (const T*)acts + (r0 + q) * lda;
#pragma unroll
      for (int u = 0; u < CG_PER; ++u) v[q][u] = row_ok && id[u] < h ? src[id[u]] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < CG_RB; ++q)
#pragma unroll
      for (int u = 0; u < CG_PER; ++u) tile[q][u * CG_NT + tid] = v[q][u];
    __syncthreads();
    if (cw < d_pad) {
#pragma unroll
      for (int q = 0; q < CG_RB; ++q) {
        if (r0 + q < r_end) {
          T* const dst = (T*)out + (r0 + q) * (int64_t)d_pad + cw;
          const uint4* const s = (const uint4*)&tile[q][tid * CG_PER];
          ((uint4*)dst)[0] = s[0];
          if constexpr (DT == CC_F32) ((uint4*)dst)[1] = s[1];
        }
      }
    }
    __syncthreads();  // (the tile is rewritten by the next rows)
  }
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_dead_compact(const int64_t* since_fired, int64_t h, int64_t h_real, int64_t dead_after, int32_t* ids,
                    int64_t d_pad, int32_t* slot, uint32_t* count, void* stream) {
  if (h < 1 || h_real < 0 || h_real > h || d_pad < 8 || (d_pad & 7)) return CC_ERR_SHAPE;
  if (!since_fired || !ids || !slot || !count) return CC_ERR_NULL;
  if (h > MASK_MAX_H || d_pad > MASK_MAX_H) return CC_ERR_TOO_LARGE;
  if (!aligned({since_fired}, 7) || !aligned({ids, slot, count}, 3)) return CC_ERR_ALIGN;
  hipLaunchKernelGGL(dead_compact_kernel, dim3(1), dim3(DC_NT), 0, (hipStream_t)stream, since_fired, (int)h, (int)h_real,
                     dead_after, ids, (int)d_pad, slot, count);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_compact_gather(const int32_t* ids, int64_t d_pad, int64_t h, const void* W, int64_t ldw, int64_t K, void* Wc,
                      int64_t ldc, const void* acts, int64_t lda, int64_t B, void* acts_c, int dtype, void* stream) {
  const bool rows = W || Wc, cols = acts || acts_c;
  if (d_pad < 8 || (d_pad & 7) || h < 1) return CC_ERR_SHAPE;
  if (rows && (K < 8 || (K & 7) || ldw < K || ldc < K)) return CC_ERR_SHAPE;
  if (cols && (B < 1 || lda < h)) return CC_ERR_SHAPE;
  if (!ids || (!rows && !cols) || (rows && (!W || !Wc)) || (cols && (!acts || !acts_c)) || (rows && W == Wc) ||
      (cols && acts == acts_c))
    return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || d_pad > MASK_MAX_H || (rows && K > INT32_MAX) || (cols && B > ((int64_t)1 << 20)))
    return CC_ERR_TOO_LARGE;
  const int64_t es = dtype == CC_BF16 ? 2 : 4;
  if (!aligned({ids}, 3) || !aligned({W, Wc, acts_c}, 15) || !aligned({acts}, (uintptr_t)es - 1)) return CC_ERR_ALIGN;
  if (rows && (((ldw * es) & 15) || ((ldc * es) & 15))) return CC_ERR_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  if (cols) {
    const dim3 grid((unsigned)((d_pad + CG_COLS - 1) / CG_COLS), (unsigned)((B + CG_ROWS - 1) / CG_ROWS));
    hipLaunchKernelGGL(CC_BY_DTYPE(gather_cols_kernel, dtype), grid, dim3(CG_NT), 0, st, ids, (int)d_pad, (uint32_t)h,
                       acts, lda, B, acts_c);
    CC_LAUNCH_CHECK();
  }
  if (rows) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)d_pad), dim3(CG_NT), 0, st, ids, d_pad, (uint32_t)h,
                       (const uint4*)W, ldw * es / 16, (uint4*)Wc, ldc * es / 16, (int)(K * es / 16));
    CC_LAUNCH_CHECK();
  }
  return CC_OK;
}

}  // extern "C"
