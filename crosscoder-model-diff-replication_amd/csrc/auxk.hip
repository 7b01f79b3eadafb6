// The small kernels of the AuxK dead-latent loss (the selection itself is cc_auxk_rows in topk.hip).  gfx950.
//   cc_dead_update  tokens_since_fired <- fired ? 0 : + B, and the count of dead latents under the new state
//   cc_auxk_loss    num / den of the aux reconstruction e^ against the main residual e = x - r, and g_aux
//                   (pass 1 -> partial slabs, the squared column sums, the scalar finaliser, pass 2 -> g_aux)
//   cc_add_rows     dst = dtype(float(dst) + float(src))
// No float atomics anywhere: every sum goes through partial slabs added in a fixed order.
#include "mask_common.h"

namespace cc {

// ---------------------------------------------------------------------------------------------- dead update
// One workgroup: h <= 2^17 latents are 128 per thread at most, and the count needs no second launch.
constexpr int DU_NT = 1024;

__global__ __launch_bounds__(DU_NT) void dead_update_kernel(const float* __restrict__ colsum_acts,
                                                            int64_t* __restrict__ since_fired, int h, int h_real,
                                                            int64_t B, int64_t dead_after, uint8_t* __restrict__ was_dead,
                                                            int32_t* __restrict__ count_out, int32_t* __restrict__ host_out) {
  __shared__ int wsum[DU_NT / 64];
  const int tid = threadIdx.x;
  int mine = 0;
  for (int l = tid; l < h; l += DU_NT) {
    const int64_t old = since_fired[l];
    // fired: the main selection kept the latent in some row -- its column sum of positive terms is > 0
    const int64_t now = colsum_acts[l] > 0.f ? 0 : old + B;
    since_fired[l] = now;
    if (was_dead) was_dead[l] = old >= dead_after ? 1 : 0;
    mine += (l < h_real && now >= dead_after) ? 1 : 0;  // (padding latents never fire: not counted)
  }
  mine = (int)wave_sum_u((uint32_t)mine);
  if ((tid & 63) == 0) wsum[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < DU_NT / 64; ++w) total += wsum[w];
    *count_out = total;
    if (host_out) {
      *host_out = total;
      __threadfence_system();  // mapped host memory: there before whatever the stream releases next
    }
  }
}

// ---------------------------------------------------------------------------------------------- aux loss
// Pass 1: a workgroup takes AL_ROWS batch rows x AL_COLS columns (8 per thread) and writes, for its row block rb and
// column block cb, colpart[rb][k] = sum_rows e, and {sum (e^ - e)^2, sum e^2} over its tile into sqpart[rb][cb][2].
constexpr int AL_NT = 256, AL_ROWS = 32, AL_COLS = AL_NT * 8;

template <int DT> CC_DEV void al_residual(const float* __restrict__ recon, const float (&bd)[8], const void* __restrict__ x,
                                          const float* __restrict__ ehat, int64_t off, float (&e)[8], float (&dif)[8]) {
  float r[8], xv[8], eh[8];
  load8f(recon, off, r);
  load8<DT>(x, off, xv);
  load8f(ehat, off, eh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    e[j] = xv[j] - (r[j] + bd[j]);
    dif[j] = eh[j] - e[j];
  }
}

template <int DT>
__global__ __launch_bounds__(AL_NT) void auxk_pass1_kernel(const float* __restrict__ recon, const void* __restrict__ b_dec,
                                                           const void* __restrict__ x, const float* __restrict__ ehat,
                                                           int B, int K, float* __restrict__ colpart,
                                                           float* __restrict__ sqpart) {
  __shared__ float red[2][AL_NT / 64];
  const int tid = threadIdx.x, rb = blockIdx.x, cb = blockIdx.y;
  const int col = cb * AL_COLS + tid * 8;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, num = 0.f, e2 = 0.f;
  if (col < K) {
    float bd[8];
    load8<DT>(b_dec, col, bd);
    const int r1 = min(B, (rb + 1) * AL_ROWS);
    for (int row = rb * AL_ROWS; row < r1; ++row) {
      float e[8], dif[8];
      al_residual<DT>(recon, bd, x, ehat, (int64_t)row * K + col, e, dif);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cs[j] += e[j];
        num += dif[j] * dif[j];
        e2 += e[j] * e[j];
      }
    }
    float* const out = colpart + (int64_t)rb * K + col;
    *(float4*)out = float4{cs[0], cs[1], cs[2], cs[3]};
    *(float4*)(out + 4) = float4{cs[4], cs[5], cs[6], cs[7]};
  }
  num = wave_sum(num);
  e2 = wave_sum(e2);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = num;
    red[1][tid >> 6] = e2;
  }
  __syncthreads();
  if (tid < 2) {
    float s = 0.f;
    for (int w = 0; w < AL_NT / 64; ++w) s += red[tid][w];
    sqpart[((int64_t)rb * gridDim.y + cb) * 2 + tid] = s;
  }
}

// The squared column sums of e, fp64: a workgroup takes AL_CS_COLS columns; thread (c, q) adds the row blocks q, q + 4,
// ... of column c (independent loads), the four partials are added in order, squared, and the workgroup's columns
// summed in a fixed order into colsq[blockIdx.x] = sum_k (sum_b e[b][k])^2.
constexpr int AL_CS_COLS = 64;

__global__ __launch_bounds__(AL_NT) void auxk_colsq_kernel(const float* __restrict__ colpart, int nrb, int K,
                                                           double* __restrict__ colsq) {
  __shared__ double part[AL_NT / AL_CS_COLS][AL_CS_COLS];
  const int tid = threadIdx.x, c = tid & (AL_CS_COLS - 1), q = tid / AL_CS_COLS;
  const int k = blockIdx.x * AL_CS_COLS + c;
  double s = 0.0;
  if (k < K) {
    constexpr int Q = AL_NT / AL_CS_COLS, U = 8;
    for (int rb0 = q; rb0 < nrb; rb0 += Q * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = rb0 + u * Q < nrb ? colpart[(int64_t)(rb0 + u * Q) * K + k] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) s += (double)v[u];
    }
  }
  part[q][c] = s;
  __syncthreads();
  if (tid < AL_CS_COLS) {  // (one wave)
    double t = 0.0;
    for (int i = 0; i < AL_NT / AL_CS_COLS; ++i) t += part[i][tid];
    t = wave_sum_d(t * t);
    if (tid == 0) colsq[blockIdx.x] = t;
  }
}

// The finaliser, one workgroup, fp64: den = (sum e^2 - sum_k colsum_k^2 / B) / B, num = sum (e^ - e)^2 / B,
// scalars = {auxk_loss, den, scale, valid}; scale = 2 coeff / (B den).  The loss is forced to 0 (valid = 0,
// scale = 0) when den is not > 0 or the quotient is not finite.
__global__ __launch_bounds__(AL_NT) void auxk_finalize_kernel(const double* __restrict__ colsq, int ncs,
                                                              const float* __restrict__ sqpart, int nsq, int B,
                                                              float coeff, float* __restrict__ scalars,
                                                              float* __restrict__ host_out) {
  __shared__ double red[3][AL_NT / 64];
  const int tid = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};  // sum (e^ - e)^2, sum e^2, sum_k colsum_k^2
  for (int i = tid; i < nsq; i += AL_NT) {
    a[0] += (double)sqpart[2 * i];
    a[1] += (double)sqpart[2 * i + 1];
  }
  for (int i = tid; i < ncs; i += AL_NT) a[2] += colsq[i];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a[q] = wave_sum_d(a[q]);
    if ((tid & 63) == 0) red[q][tid >> 6] = a[q];
  }
  __syncthreads();
  if (tid == 0) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 3; ++q)
      for (int w = 0; w < AL_NT / 64; ++w) s[q] += red[q][w];
    const double den = (s[1] - s[2] / (double)B) / (double)B, num = s[0] / (double)B;
    const double loss = num / den;
    const bool valid = den > 0.0 && loss == loss && loss <= 3.4028234663852886e38 && loss >= 0.0;
    const float lossf = valid ? (float)loss : 0.f;
    scalars[0] = lossf;
    scalars[1] = (float)den;
    scalars[2] = valid ? (float)(2.0 * (double)coeff / ((double)B * den)) : 0.f;
    scalars[3] = valid ? 1.f : 0.f;
    if (host_out) {
      *host_out = lossf;
      __threadfence_system();
    }
  }
}

// Pass 2: g_aux = dtype(scale * (e^ - e)), all +0 when the loss was forced to 0.
template <int DT>
__global__ __launch_bounds__(AL_NT) void auxk_pass2_kernel(const float* __restrict__ recon, const void* __restrict__ b_dec,
                                                           const void* __restrict__ x, const float* __restrict__ ehat,
                                                           int B, int K, const float* __restrict__ scalars,
                                                           void* __restrict__ g_aux) {
  const int tid = threadIdx.x, rb = blockIdx.x, cb = blockIdx.y;
  const int col = cb * AL_COLS + tid * 8;
  if (col >= K) return;
  const float scale = scalars[2];
  const bool valid = scalars[3] != 0.f;
  float bd[8];
  load8<DT>(b_dec, col, bd);
  const int r1 = min(B, (rb + 1) * AL_ROWS);
  for (int row = rb * AL_ROWS; row < r1; ++row) {
    const int64_t off = (int64_t)row * K + col;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
      float e[8], dif[8];
      al_residual<DT>(recon, bd, x, ehat, off, e, dif);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = scale * dif[j];
    }
    store8<DT>(g_aux, off, g);
  }
}

// ---------------------------------------------------------------------------------------------- add rows
template <int DT>
__global__ __launch_bounds__(256) void add_rows_kernel(void* __restrict__ dst, const void* __restrict__ src, int64_t rows,
                                                       int cols8, int64_t ld) {
  const int64_t n = rows * cols8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t off = (i / cols8) * ld + (i % cols8) * 8;
    float a[8], b[8];
    load8<DT>(dst, off, a);
    load8<DT>(src, off, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += b[j];
    store8<DT>(dst, off, a);
  }
}

static int64_t al_row_blocks(int64_t B) { return (B + AL_ROWS - 1) / AL_ROWS; }
static int64_t al_col_blocks(int64_t K) { return (K + AL_COLS - 1) / AL_COLS; }
static int64_t al_colsq_blocks(int64_t K) { return (K + AL_CS_COLS - 1) / AL_CS_COLS; }

}  // namespace cc

using namespace cc;

extern "C" {

int cc_dead_update(const float* colsum_acts, int64_t* since_fired, int64_t h, int64_t h_real, int64_t B,
                   int64_t dead_after, uint8_t* was_dead, int32_t* count_out, int32_t* host_out, void* stream) {
  if (h < 1 || h_real < 0 || h_real > h || B < 1) return CC_ERR_SHAPE;
  if (!colsum_acts || !since_fired || !count_out) return CC_ERR_NULL;
  if (h > (1 << 17)) return CC_ERR_TOO_LARGE;
  if (((uintptr_t)colsum_acts & 3) || ((uintptr_t)since_fired & 7) || ((uintptr_t)count_out & 3) ||
      ((uintptr_t)host_out & 3))
    return CC_ERR_ALIGN;
  hipLaunchKernelGGL(dead_update_kernel, dim3(1), dim3(DU_NT), 0, (hipStream_t)stream, colsum_acts, since_fired, (int)h,
                     (int)h_real, B, dead_after, was_dead, count_out, host_out);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_auxk_part_floats(int64_t B, int64_t K) {
  // (the column-sum slab, the two squared sums per tile, one fp64 per AL_CS_COLS columns)
  return B < 1 || K < 1 ? 0 : al_row_blocks(B) * (K + 2 * al_col_blocks(K)) + 2 * al_colsq_blocks(K);
}

int cc_auxk_loss(const float* recon_f32, const void* b_dec, const void* x, const float* ehat_f32, void* g_aux,
                 float* part, float* scalars, float* host_out, float auxk_coeff, int64_t B, int64_t K, int dtype,
                 void* stream) {
  if (B < 1 || K < 8 || (K & 7)) return CC_ERR_SHAPE;
  if (!recon_f32 || !b_dec || !x || !ehat_f32 || !g_aux || !part || !scalars) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (B > (1 << 30) || K > (1 << 24)) return CC_ERR_TOO_LARGE;
  if (((uintptr_t)recon_f32 | (uintptr_t)b_dec | (uintptr_t)x | (uintptr_t)ehat_f32 | (uintptr_t)g_aux |
       (uintptr_t)part | (uintptr_t)scalars) & 15)
    return CC_ERR_ALIGN;
  if ((uintptr_t)host_out & 3) return CC_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int nrb = (int)al_row_blocks(B), ncb = (int)al_col_blocks(K);
  float* const colpart = part;
  float* const sqpart = part + (int64_t)nrb * K;
  double* const colsq = (double*)(sqpart + (int64_t)nrb * ncb * 2);  // (an even offset from 16-byte aligned `part`)
  const int ncs = (int)al_colsq_blocks(K);
  const dim3 grid(nrb, ncb);
  if (dtype == CC_BF16)
    hipLaunchKernelGGL(auxk_pass1_kernel<CC_BF16>, grid, dim3(AL_NT), 0, st, recon_f32, b_dec, x, ehat_f32, (int)B, (int)K,
                       colpart, sqpart);
  else
    hipLaunchKernelGGL(auxk_pass1_kernel<CC_F32>, grid, dim3(AL_NT), 0, st, recon_f32, b_dec, x, ehat_f32, (int)B, (int)K,
                       colpart, sqpart);
  hipLaunchKernelGGL(auxk_colsq_kernel, dim3(ncs), dim3(AL_NT), 0, st, (const float*)colpart, nrb, (int)K, colsq);
  hipLaunchKernelGGL(auxk_finalize_kernel, dim3(1), dim3(AL_NT), 0, st, (const double*)colsq, ncs, (const float*)sqpart,
                     nrb * ncb, (int)B, auxk_coeff, scalars, host_out);
  if (dtype == CC_BF16)
    hipLaunchKernelGGL(auxk_pass2_kernel<CC_BF16>, grid, dim3(AL_NT), 0, st, recon_f32, b_dec, x, ehat_f32, (int)B, (int)K,
                       (const float*)scalars, g_aux);
  else
    hipLaunchKernelGGL(auxk_pass2_kernel<CC_F32>, grid, dim3(AL_NT), 0, st, recon_f32, b_dec, x, ehat_f32, (int)B, (int)K,
                       (const float*)scalars, g_aux);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_add_rows(void* dst, const void* src, int64_t rows, int64_t cols, int64_t ld, int dtype, void* stream) {
  if (rows < 1 || cols < 8 || (cols & 7) || (ld & 7) || ld < cols) return CC_ERR_SHAPE;
  if (!dst || !src) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (rows > (1 << 30) || cols > (1 << 24)) return CC_ERR_TOO_LARGE;
  if (((uintptr_t)dst | (uintptr_t)src) & 15) return CC_ERR_ALIGN;
  const int64_t n = rows * (cols / 8);
  const int64_t blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
  if (dtype == CC_BF16)
    hipLaunchKernelGGL(add_rows_kernel<CC_BF16>, grid, dim3(256), 0, (hipStream_t)stream, dst, src, rows, (int)(cols / 8), ld);
  else
    hipLaunchKernelGGL(add_rows_kernel<CC_F32>, grid, dim3(256), 0, (hipStream_t)stream, dst, src, rows, (int)(cols / 8), ld);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
