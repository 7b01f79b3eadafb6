// HBM-bound kernels of the crosscoder training step (gfx950): input normalisation, the
// fused reconstruction loss + its gradient, decoder norms, deterministic slab reductions,
// the loss/EV finalisation, clip_grad_norm_ finalisation and the fused step tails.  (The Adam update: adam.hip.)
// All vector accesses are 16 B per lane; every cross-block sum goes through a fixed-order
// partial slab (bit-reproducible, no float atomics).
#include "cc_common.h"

#include <cmath>

namespace cc {

#include "grad_tail.h"
#include "prep_tile.h"

constexpr int LOSS_ROWS = 32;   // rows per loss block
constexpr int LOSS_COLS = 512;  // columns per loss block (64 lanes x 8)

// ---------------------------------------------------------------------------------------
// x_out = dtype(x_in * factor[model]);  colsum_part[rb][k] = sum over the block's rows.
// grid: (ceil(K/512), ceil(B/64)); block 256 = 4 waves; lane -> 8 columns, wave -> 16 rows.
// TR (bf16 out): also x_t [K][B] = x_out^T through a 32-row LDS tile (two halves per block; the
// column-sum slab shares the tile's LDS, so 32 KB per block: 5 blocks per CU, one round of blocks).
template <int DIN, int DF, int DT, bool TR = false>
__global__ __launch_bounds__(256) void prep_kernel(const void* __restrict__ x_in, const void* __restrict__ factor,
                                                   void* __restrict__ x_out, float* __restrict__ colsum_part, int B,
                                                   int n, int d, void* __restrict__ x_t) {
  __shared__ __attribute__((aligned(16))) char lds[TR ? 32 * 1024 : 4 * 512 * 4];
  float(*red)[512] = (float(*)[512])lds;
  const int K = n * d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 512 + lane * 8;
  const int r0 = blockIdx.y * PREP_ROWS;
  float cs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float f = 1.f;
  if (factor && col < K) f = Elem<DF>::load((const typename Elem<DF>::T*)factor + col / d);
  if constexpr (TR) {
    for (int half = 0; half < 2; ++half) {
      const int base = r0 + 32 * half;
      if (base >= B) break;  // block-uniform
      if (col < K) {
        // the wave's 8 rows of this half (base + w + 4k): all loads in flight; the column sums
        // still add rows in the order r0+w, r0+w+4, ...
        float v[8][8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (base + wave + 4 * k < B) load8<DIN>(x_in, (int64_t)(base + wave + 4 * k) * K + col, v[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int r = base + wave + 4 * k;
          if (r >= B) break;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[k][j] = Elem<DT>::round(v[k][j] * f);
          store8<DT>(x_out, (int64_t)r * K + col, v[k]);
          tile_put8(lds, r - base, lane, v[k]);
#pragma unroll
          for (int j = 0; j < 8; ++j) cs[j] += v[k][j];
        }
      }
      __syncthreads();
      tile_store_transposed<32, true>(lds, x_t, B, (int64_t)blockIdx.x * 512, K - blockIdx.x * 512, base,
                                B - base < 32 ? B - base : 32);
      __syncthreads();
    }
  } else if (col < K) {
    // 4 rows per trip (rows rb, rb+4, rb+8, rb+12): their loads are in flight together
    for (int rb = r0 + wave; rb < r0 + PREP_ROWS && rb < B; rb += 16) {
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (rb + 4 * u < B) load8<DIN>(x_in, (int64_t)(rb + 4 * u) * K + col, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rb + 4 * u;
        if (r >= B) break;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = Elem<DT>::round(v[u][j] * f);
        store8<DT>(x_out, (int64_t)r * K + col, v[u]);
#pragma unroll
        for (int j = 0; j < 8; ++j) cs[j] += v[u][j];
      }
    }
  }
  if (!colsum_part) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wave][lane * 8 + j] = cs[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += 256) {
    int c = blockIdx.x * 512 + i;
    if (c < K) colsum_part[(int64_t)blockIdx.y * K + c] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

template <int DT>
__global__ __launch_bounds__(256) void reduce_rows_kernel(const RedSeg a) {
  __shared__ float red[4][RED_COLS];
  reduce_rows_phase1(a, blockIdx.x, threadIdx.x, red);
  __syncthreads();
  reduce_rows_phase2<DT>(a, blockIdx.x, threadIdx.x, red);
}

// ---------------------------------------------------------------------------------------
// norms[h][m] = ||W_dec[h,m,:]||, total[h] = sum_m.  One wave per (h) row, all models.
// Summation order (shared with the fused W_dec^T transposition, cc_transpose_dec_norms, so both
// give the same bits): per 64-column block, each of 8 lanes sums its 8 squares in order (fma),
// the 8 lane sums combine by an xor-1/2/4 butterfly; block sums are added in ascending order.
template <int DT>
__global__ __launch_bounds__(256) void dec_norms_kernel(const void* __restrict__ W, float* __restrict__ norms,
                                                        float* __restrict__ total, float* __restrict__ inv_norms, int h,
                                                        int n, int d) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= h) return;
  float tot = 0.f;
  for (int m = 0; m < n; ++m) {
    const int64_t base = ((int64_t)row * n + m) * d;
    float s = 0.f;
    for (int c0 = 0; c0 < d; c0 += 512) {  // 8 blocks of 64 columns per pass
      const int c = c0 + lane * 8;
      float q = 0.f;
      if (c < d) {
        float v[8];
        load8<DT>(W, base + c, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) q = __fmaf_rn(v[j], v[j], q);
      }
      q = block8_sum(q);
#pragma unroll
      for (int g = 0; g < 8; ++g)
        if (c0 + 64 * g < d) s += __shfl(q, 8 * g, 64);
    }
    const float nr = sqrtf(s);
    if (lane == 0) {
      norms[(int64_t)row * n + m] = nr;
      if (inv_norms) inv_norms[(int64_t)row * n + m] = nr > 0.f ? 1.f / nr : 0.f;
    }
    tot += nr;
  }
  if (lane == 0) total[row] = tot;
}

// ---------------------------------------------------------------------------------------
// Reconstruction loss + gradient.  grid: (n * ncb, ceil(rows/32)); block 256 = 4 waves.
// Block covers model m = blockIdx.x / ncb, columns [m*d + cb*512, +512) ∩ model, 32 rows of the
// row range [row0, row_end) (row0 % 32 == 0).  The slabs keep the whole-batch layout, so disjoint
// row ranges can be separate launches: the latent-sharded step runs each batch slice as soon as
// its all-reduce has landed.  lane -> 8 columns; wave w -> rows r0 + w + 4i.
// TR (bf16): also g_recon_t [K][B] = g_recon^T (rows [row0, row_end)) through an LDS tile.
template <int DT, bool TR = false>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ recon, const void* __restrict__ b_dec,
                                                   const void* __restrict__ x, const float* __restrict__ x_mean,
                                                   void* __restrict__ g_recon, float* __restrict__ row_part,
                                                   float* __restrict__ col_part, float grad_scale, int B, int n,
                                                   int d, int ncb, int row0, int row_end, void* __restrict__ g_t) {
  // (TR: the column-sum slab reuses the transposition tile's LDS: 32 KB per block)
  __shared__ __attribute__((aligned(16))) char tile[TR ? LOSS_ROWS * 1024 : 4 * 512 * 4];
  float(*red)[512] = (float(*)[512])tile;
  using E = Elem<DT>;
  const int K = n * d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x / ncb, cb = blockIdx.x % ncb;
  const int jc = cb * LOSS_COLS + lane * 8;  // column within model
  const bool cv = jc < d;
  const int col = m * d + jc;
  const int r0 = row0 + blockIdx.y * LOSS_ROWS;
  float bd[8], mu[8], cs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bd[j] = mu[j] = cs[j] = 0.f;
  if (cv) {
    if (b_dec) load8<DT>(b_dec, col, bd);
    if (x_mean) load8f(x_mean, col, mu);
  }
  const int64_t plane = (int64_t)n * ncb * B;  // row_part [2][n*ncb][B]
  // LOSS_U rows per trip (r, r + 4, ...): their loads are in flight together (the column sums still
  // add the wave's rows in order)
  constexpr int LOSS_U = 2;
  for (int i = 0; i < LOSS_ROWS / 4; i += LOSS_U) {
    const int ra = r0 + wave + 4 * i;
    if (ra >= row_end) break;  // wave-uniform
    float rv[LOSS_U][8], xv[LOSS_U][8];
    if (cv) {
#pragma unroll
      for (int u = 0; u < LOSS_U; ++u)
        if (ra + 4 * u < row_end) {
          load8f(recon, (int64_t)(ra + 4 * u) * K + col, rv[u]);
          load8<DT>(x, (int64_t)(ra + 4 * u) * K + col, xv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < LOSS_U; ++u) {
      const int r = ra + 4 * u;
      if (r >= row_end) break;
      float l2 = 0.f, tv = 0.f;
      if (cv) {
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float diff = (rv[u][j] + bd[j]) - xv[u][j];
          l2 += diff * diff;
          float c = xv[u][j] - mu[j];
          tv += c * c;
          g[j] = E::round(grad_scale * diff);
          cs[j] += g[j];
        }
        store8<DT>(g_recon, (int64_t)r * K + col, g);
        if constexpr (TR) tile_put8(tile, r - r0, lane, g);
      }
      l2 = wave_sum(l2);
      tv = wave_sum(tv);
      if (lane == 0) {
        row_part[(int64_t)blockIdx.x * B + r] = l2;
        row_part[plane + (int64_t)blockIdx.x * B + r] = tv;
      }
    }
  }
  if constexpr (TR) {
    __syncthreads();
    const int nr = row_end - r0 < LOSS_ROWS ? row_end - r0 : LOSS_ROWS;
    tile_store_transposed<LOSS_ROWS>(tile, g_t, B, (int64_t)m * d + cb * LOSS_COLS, d - cb * LOSS_COLS, r0, nr);
    __syncthreads();  // (red reuses the tile)
  }
  if (!col_part) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wave][lane * 8 + j] = cs[j];
  __syncthreads();
  for (int i = threadIdx.x; i < LOSS_COLS; i += 256) {
    int jj = cb * LOSS_COLS + i;
    if (jj < d)
      col_part[(int64_t)(row0 / LOSS_ROWS + blockIdx.y) * K + m * d + jj] =
          ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

#include "loss_tail.h"

__global__ __launch_bounds__(256) void ev_kernel(const EvSeg a) {
  __shared__ float red[4][4];
  ev_phase1(a, blockIdx.x, threadIdx.x, red);
  __syncthreads();
  ev_phase2(a, blockIdx.x, threadIdx.x, red);
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_scalars_kernel(const ScalArgs a) {
  __shared__ double red[LOSS_THREADS / 64][6];
  loss_scalars_body<LOSS_THREADS>(a, red);
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAL_THREADS) void clip_kernel(const ClipArgs a) {
  __shared__ double red[8][SCAL_THREADS / 64];
  __shared__ float norms[8];
  clip_body<SCAL_THREADS>(a, red, norms);
}

// ---------------------------------------------------------------------------------------
// Arrival count of a fused tail launch: every workgroup publishes what it wrote, and the last one to arrive
// (device-scope counter, reset by that workgroup for the next launch) returns true with the others' writes
// visible.  The barrier's workgroup-scope release waits for every wave's stores to reach this XCD's L2; ONE
// agent-scope release (an L2 write-back) then publishes them all before the arrival count.  Call with every
// thread of the workgroup; `last` is LDS scratch.
CC_DEV bool arrive_last(unsigned* counter, int* last) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const bool is_last = atomicAdd(counter, 1u) == gridDim.x - 1;
    if (is_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop stale lines before the reads
    *last = is_last;
  }
  __syncthreads();
  return *last;
}

// Fused grad tail (TailArgs, grad_tail.h): one launch of 1024-thread blocks = 4 independent 256-thread groups, each
// running one block of a column reduction (RedSeg: b_enc.grad, b_dec.grad column sums + their sq partials) -- the same
// two phases as the stand-alone kernel, so the same bits -- then the last block to finish runs clip_body
// (or the segment sums) over the partials the whole grid wrote.  Saves the finaliser's launch per step.
template <int DT>
__global__ __launch_bounds__(SCAL_THREADS) void tail_kernel(const TailArgs a) {
  __shared__ float red[4][4][RED_COLS];
  __shared__ int last;
  const int grp = threadIdx.x >> 8, t = threadIdx.x & 255;
  int b = blockIdx.x * 4 + grp;
  // role of this group: reduction 0, reduction 1 or idle (uniform per group)
  int role = 2;
  if (b < a.red_blocks[0]) role = 0;
  else if ((b -= a.red_blocks[0]) < a.red_blocks[1]) role = 1;
  if (role < 2) reduce_rows_phase1(a.red[role], b, t, red[grp]);
  __syncthreads();
  if (role < 2) reduce_rows_phase2<DT>(a.red[role], b, t, red[grp]);
  if (!arrive_last(a.counter, &last)) return;
  __shared__ double cred[8][SCAL_THREADS / 64];
  __shared__ float cnorms[8];
  clip_body<SCAL_THREADS>(a.clip, cred, cnorms);
  if (threadIdx.x == 0) atomicExch(a.counter, 0u);
}

// Fused loss tail (crosscoder.py:106-128): the l1 partials, the per-row EV terms and the loss scalars in one
// launch of the LossTailArgs items (loss_tail.h), one 256-thread workgroup per item, whose workgroups fit beside a
// persistent GEMM workgroup (256 threads, few registers, < 0.5 KB of LDS); the last workgroup to arrive runs
// loss_scalars_body<LOSS_THREADS> (the stand-alone loss_scalars_kernel's).
__global__ __launch_bounds__(LOSS_THREADS) void loss_tail_kernel(const LossTailArgs a) {
  __shared__ float evred[4][4];
  __shared__ double sred[LOSS_THREADS / 64][6];
  __shared__ int last;
  loss_tail_item(a, blockIdx.x, threadIdx.x, evred);
  if (!arrive_last(a.counter, &last)) return;
  loss_scalars_body<LOSS_THREADS>(a.scal, sred);
  if (threadIdx.x == 0) atomicExch(a.counter, 0u);
}

}  // namespace cc

using namespace cc;

int cc::launch_grad_tail(const TailArgs& a, int dtype, hipStream_t st) {
  dim3 grid((unsigned)((a.red_blocks[0] + a.red_blocks[1] + 3) / 4));
  DISPATCH_DT(dtype, hipLaunchKernelGGL((tail_kernel<DT_>), grid, dim3(SCAL_THREADS), 0, st, a));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

// The only copy of the loss rows' argument checks: NULL, shape, then for the form that also writes g_recon^T
// (g_recon_t given: bf16, B % 8 == 0, rows % 8 == 0) its dtype, then alignment.  The plain form's dtype is checked
// where its kernel is chosen.
static int check_loss_rows(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                           const void* g_recon, const void* g_recon_t, const float* row_part, int64_t row0,
                           int64_t rows, int64_t B, int64_t n, int64_t d, int dtype) {
  if (!recon_f32 || !x || !g_recon || !row_part) return CC_ERR_NULL;
  if (B <= 0 || n <= 0 || d <= 0 || d % 8 || (g_recon_t && (B % 8 || rows % 8))) return CC_ERR_SHAPE;
  if (row0 < 0 || rows <= 0 || row0 + rows > B || row0 % LOSS_ROWS) return CC_ERR_SHAPE;
  if (g_recon_t && dtype != CC_BF16) return CC_ERR_DTYPE;
  if (!al16(recon_f32) || !al16(x) || !al16(g_recon) || !al16(g_recon_t) || (b_dec && !al16(b_dec)) ||
      (x_mean && !al16(x_mean)))
    return CC_ERR_ALIGN;
  return CC_OK;
}

extern "C" {

int cc_prep_input_t(const void* x_in, int in_dtype, const void* factor, int factor_dtype, void* x_out, void* x_t,
                    float* colsum_part, int64_t B, int64_t n, int64_t d, int dtype, void* stream) {
  if (!x_t) return cc_prep_input(x_in, in_dtype, factor, factor_dtype, x_out, colsum_part, B, n, d, dtype, stream);
  if (const int rc = check_prep(x_in, in_dtype, factor, factor_dtype, x_out, x_t, true, B, n, d, dtype)) return rc;
  dim3 grid((unsigned)((n * d + 511) / 512), (unsigned)cc_prep_part_rows(B));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_PREP(in_dtype, factor && factor_dtype == CC_BF16,
                hipLaunchKernelGGL((prep_kernel<DI_, DF_, CC_BF16, true>), grid, dim3(256), 0, st, x_in, factor, x_out,
                                   colsum_part, (int)B, (int)n, (int)d, x_t));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_prep_input(const void* x_in, int in_dtype, const void* factor, int factor_dtype, void* x_out,
                  float* colsum_part, int64_t B, int64_t n, int64_t d, int dtype, void* stream) {
  if (const int rc = check_prep(x_in, in_dtype, factor, factor_dtype, x_out, nullptr, false, B, n, d, dtype)) return rc;
  dim3 grid((unsigned)((n * d + 511) / 512), (unsigned)cc_prep_part_rows(B));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_PREP(in_dtype, factor && factor_dtype == CC_BF16,
                DISPATCH_DT(dtype, hipLaunchKernelGGL((prep_kernel<DI_, DF_, DT_>), grid, dim3(256), 0, st, x_in, factor,
                                                      x_out, colsum_part, (int)B, (int)n, (int)d, nullptr)));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_reduce_rows(const float* part, int64_t R, int64_t C, int64_t ld, float scale, float* out_f32, void* out_t,
                   int dtype, float* sq_part, const float* dot_w, float* dot_part, void* stream) {
  if (!part) return CC_ERR_NULL;
  if (R <= 0 || C <= 0) return CC_ERR_SHAPE;
  if (sq_part && !out_t) return CC_ERR_NULL;
  if (dot_part && !dot_w) return CC_ERR_NULL;
  dim3 grid((unsigned)((C + RED_COLS - 1) / RED_COLS));
  hipStream_t st = (hipStream_t)stream;
  const RedSeg a = {part, (int)R, (int)C, ld, scale, out_f32, out_t, sq_part, dot_w, dot_part};
  if (out_t) {
    DISPATCH_DT(dtype, hipLaunchKernelGGL((reduce_rows_kernel<DT_>), grid, dim3(256), 0, st, a));
  } else {
    hipLaunchKernelGGL((reduce_rows_kernel<CC_F32>), grid, dim3(256), 0, st, a);
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_dec_norms(const void* W_dec, float* norms, float* total, float* inv_norms, int64_t h, int64_t n, int64_t d,
                 int dtype, void* stream) {
  if (!W_dec || !norms || !total) return CC_ERR_NULL;
  if (h <= 0 || n <= 0 || d <= 0 || d % 8) return CC_ERR_SHAPE;
  if (!al16(W_dec)) return CC_ERR_ALIGN;
  dim3 grid((unsigned)((h + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_DT(dtype, hipLaunchKernelGGL((dec_norms_kernel<DT_>), grid, dim3(256), 0, st, W_dec, norms, total,
                                        inv_norms, (int)h, (int)n, (int)d));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_loss_fwd_bwd_rows_t(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                           void* g_recon, void* g_recon_t, float* row_part, float* col_part, float grad_scale,
                           int64_t row0, int64_t rows, int64_t B, int64_t n, int64_t d, int dtype, void* stream) {
  if (!g_recon_t)
    return cc_loss_fwd_bwd_rows(recon_f32, b_dec, x, x_mean, g_recon, row_part, col_part, grad_scale, row0, rows, B,
                                n, d, dtype, stream);
  if (const int rc = check_loss_rows(recon_f32, b_dec, x, x_mean, g_recon, g_recon_t, row_part, row0, rows, B, n, d,
                                     dtype))
    return rc;
  int ncb = (int)cc_loss_col_blocks(d);
  dim3 grid((unsigned)(n * ncb), (unsigned)cc_loss_part_rows(rows));
  hipLaunchKernelGGL((loss_kernel<CC_BF16, true>), grid, dim3(256), 0, (hipStream_t)stream, recon_f32, b_dec, x,
                     x_mean, g_recon, row_part, col_part, grad_scale, (int)B, (int)n, (int)d, ncb, (int)row0,
                     (int)(row0 + rows), g_recon_t);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_loss_fwd_bwd_rows(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                         void* g_recon, float* row_part, float* col_part, float grad_scale, int64_t row0,
                         int64_t rows, int64_t B, int64_t n, int64_t d, int dtype, void* stream) {
  if (const int rc = check_loss_rows(recon_f32, b_dec, x, x_mean, g_recon, nullptr, row_part, row0, rows, B, n, d,
                                     dtype))
    return rc;
  int ncb = (int)cc_loss_col_blocks(d);
  dim3 grid((unsigned)(n * ncb), (unsigned)cc_loss_part_rows(rows));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_DT(dtype, hipLaunchKernelGGL((loss_kernel<DT_>), grid, dim3(256), 0, st, recon_f32, b_dec, x, x_mean,
                                        g_recon, row_part, col_part, grad_scale, (int)B, (int)n, (int)d, ncb,
                                        (int)row0, (int)(row0 + rows), nullptr));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_loss_fwd_bwd(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean, void* g_recon,
                    float* row_part, float* col_part, float grad_scale, int64_t B, int64_t n, int64_t d, int dtype,
                    void* stream) {
  return cc_loss_fwd_bwd_rows(recon_f32, b_dec, x, x_mean, g_recon, row_part, col_part, grad_scale, 0, B, B, n, d,
                              dtype, stream);
}

int cc_loss_finalize(const float* row_part, const float* l1_part, int64_t n_l1, const float* l0_part, int64_t n_l0,
                     float* ev, float* ev_a, float* ev_b, float* scalars, float* l1l0_out, int64_t B, int64_t n,
                     int64_t d, void* stream) {
  return cc_loss_finalize_mapped(row_part, l1_part, n_l1, l0_part, n_l0, ev, ev_a, ev_b, scalars, l1l0_out, nullptr,
                                 0, B, n, d, stream);
}

int cc_loss_finalize_mapped(const float* row_part, const float* l1_part, int64_t n_l1, const float* l0_part,
                            int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars, float* l1l0_out,
                            float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, void* stream) {
  return cc_loss_finalize_nb(row_part, cc_loss_col_blocks(d), l1_part, n_l1, l0_part, n_l0, ev, ev_a, ev_b, scalars,
                             l1l0_out, host_out, seq, B, n, d, stream);
}

int cc_loss_finalize_nb(const float* row_part, int64_t ncb_rows, const float* l1_part, int64_t n_l1,
                        const float* l0_part, int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars,
                        float* l1l0_out, float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, void* stream) {
  if (!row_part || !scalars) return CC_ERR_NULL;
  if (B <= 0 || n <= 0 || d <= 0 || ncb_rows <= 0) return CC_ERR_SHAPE;
  // the per-block partials of the row terms use the tail of `scalars` (cc_loss_scalars_len)
  int ncb = (int)ncb_rows;
  int nblk = (int)((B + 255) / 256);
  float* ev_part = scalars + 8;
  hipStream_t st = (hipStream_t)stream;
  const EvSeg e = {row_part, (int)B, (int)n, ncb, ev, ev_a, ev_b, ev_part, nblk};
  hipLaunchKernelGGL(ev_kernel, dim3(nblk), dim3(256), 0, st, e);
  const ScalArgs s = {ev_part, nblk, l1_part, n_l1, l0_part, n_l0, (int)B, scalars, l1l0_out, host_out, (unsigned)seq};
  hipLaunchKernelGGL(loss_scalars_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, s);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_clip_finalize(const float* sq, const int64_t* off, int nparams, float max_norm, int emulate_bf16, float* out,
                     void* stream) {
  ClipArgs a;
  if (const int rc = make_clip_args(a, sq, off, nparams, out)) return rc;
  a.max_norm = max_norm;
  a.emulate_bf16 = emulate_bf16;
  hipLaunchKernelGGL(clip_kernel, dim3(1), dim3(SCAL_THREADS), 0, (hipStream_t)stream, a);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_segment_sums(const float* sq, const int64_t* off, int nparams, int zero_mask, float* out, void* stream) {
  ClipArgs a;
  if (const int rc = make_clip_args(a, sq, off, nparams, out)) return rc;
  a.sums_only = 1;
  a.zero_mask = zero_mask;
  hipLaunchKernelGGL(clip_kernel, dim3(1), dim3(SCAL_THREADS), 0, (hipStream_t)stream, a);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_grad_tail(const float* gpre_colpart, int64_t R_enc, int64_t h, void* g_b_enc, float* sq_b_enc,
                 const float* loss_colpart, int64_t R_dec, int64_t K, void* g_b_dec, float* sq_b_dec, int dtype,
                 const float* sq, const int64_t* off, int nparams, float max_norm, int emulate_bf16, float* clip_out,
                 uint32_t* counter, void* stream) {
  const GradTailIn in = {.gpre_colpart = gpre_colpart, .R_enc = R_enc, .h = h, .g_b_enc = g_b_enc, .sq_b_enc = sq_b_enc,
                         .loss_colpart = loss_colpart, .R_dec = R_dec, .K = K, .g_b_dec = g_b_dec, .sq_b_dec = sq_b_dec,
                         .sq = sq, .off = off, .nparams = nparams, .max_norm = max_norm, .emulate_bf16 = emulate_bf16,
                         .out = clip_out, .counter = counter};
  TailArgs a;
  const int rc = make_grad_tail_args(a, in);
  return rc ? rc : launch_grad_tail(a, dtype, (hipStream_t)stream);
}

int cc_grad_tail_sums(const float* gpre_colpart, int64_t R_enc, int64_t h, void* g_b_enc, float* sq_b_enc,
                      const float* loss_colpart, int64_t R_dec, int64_t K, void* g_b_dec, float* sq_b_dec, int dtype,
                      const float* sq, const int64_t* off, int nparams, int zero_mask, float* out, uint32_t* counter,
                      void* stream) {
  const GradTailIn in = {.gpre_colpart = gpre_colpart, .R_enc = R_enc, .h = h, .g_b_enc = g_b_enc, .sq_b_enc = sq_b_enc,
                         .loss_colpart = loss_colpart, .R_dec = R_dec, .K = K, .g_b_dec = g_b_dec, .sq_b_dec = sq_b_dec,
                         .sq = sq, .off = off, .nparams = nparams, .sums_only = 1, .zero_mask = zero_mask, .out = out,
                         .counter = counter};
  TailArgs a;
  const int rc = make_grad_tail_args(a, in);
  return rc ? rc : launch_grad_tail(a, dtype, (hipStream_t)stream);
}

int cc_loss_tail(const float* colsum_acts, const float* tn, int64_t h, float* l1_part, const float* row_part,
                 int64_t ncb, const float* l0_part, int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars,
                 float* l1l0_out, float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, uint32_t* counter,
                 void* stream) {
  if (!colsum_acts || !tn || !l1_part || !row_part || !scalars || !counter) return CC_ERR_NULL;
  if (h <= 0 || B <= 0 || n <= 0 || d <= 0 || ncb <= 0) return CC_ERR_SHAPE;
  const LossTailArgs a = make_loss_tail_args(colsum_acts, tn, h, l1_part, row_part, ncb, l0_part, n_l0, ev, ev_a, ev_b,
                                             scalars, l1l0_out, host_out, seq, B, n, counter);
  const int nblk = a.ev.nblk;
  hipLaunchKernelGGL(loss_tail_kernel, dim3((unsigned)(a.l1_wgs + nblk)), dim3(LOSS_THREADS), 0,
                     (hipStream_t)stream, a);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_version(void) { return 100; }

const char* cc_strerror(int code) {
  switch (code) {
    case CC_OK: return "ok";
    case CC_ERR_NULL: return "crosscoder_hip: required pointer is NULL";
    case CC_ERR_DTYPE: return "crosscoder_hip: unsupported dtype (expected CC_BF16 or CC_F32)";
    case CC_ERR_SHAPE: return "crosscoder_hip: unsupported shape (d_model and dict_size must be multiples of 8)";
    case CC_ERR_ALIGN: return "crosscoder_hip: pointer or leading dimension not 16-byte aligned";
    case CC_ERR_TOO_LARGE: return "crosscoder_hip: operand panel exceeds 2 GiB buffer-descriptor range";
    default: break;
  }
  if (code >= CC_ERR_HIP_BASE) return hipGetErrorString((hipError_t)(code - CC_ERR_HIP_BASE));
  return "crosscoder_hip: unknown error";
}

int64_t cc_prep_part_rows(int64_t B) { return (B + PREP_ROWS - 1) / PREP_ROWS; }
int64_t cc_loss_part_rows(int64_t B) { return (B + LOSS_ROWS - 1) / LOSS_ROWS; }
int64_t cc_loss_col_blocks(int64_t d) { return (d + LOSS_COLS - 1) / LOSS_COLS; }
int64_t cc_loss_scalars_len(int64_t B) { return 8 + 4 * ((B + 255) / 256); }
int64_t cc_reduce_parts(int64_t C) { return (C + RED_COLS - 1) / RED_COLS; }

}  // extern "C"
