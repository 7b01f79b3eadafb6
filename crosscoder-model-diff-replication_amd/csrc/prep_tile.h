// Prep building blocks shared by the stand-alone prep and loss kernels (step_kernels.hip) and the Adam launch that
// carries a prep in its first workgroups (adam.hip): the LDS tile that writes a block's output transposed, the narrow
// prep block (device side); the one copy of the prep's argument checks and of its dtype dispatch (host side).
// Included inside namespace cc.
#pragma once

constexpr int PREP_ROWS = 64;   // rows per prep block (column partial granularity)

// ---------------------------------------------------------------------------------------
// Transposed copy of a block's [R rows][512 columns] bf16 output, staged in LDS: 16-B chunk c of
// row r at r * 1024 + ((c ^ (r & 7)) << 4).  ds_read_b64_tr_b16 turns 4 rows x 16 columns into
// 16 lanes x 4 rows; two of them give a lane 8 consecutive rows of one column (one 16-B store of
// out_t[col0 + c][row0 + 8k ..]).  The batch-contiguous copies feed the weight-gradient GEMMs.
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_s;
CC_DEV void tile_put8(char* lds, int r, int chunk, const float v[8]) {
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = (short)f2bf(v[j]);
  *(bf16x8*)(lds + r * 1024 + ((chunk ^ (r & 7)) << 4)) = b;
}
// NT: non-temporal stores (prep's x^T: read once, by G5 at the step's end; kept out of the Infinity Cache it leaves
// room for what the step reads before that -- step -7 us, profiles/r04_ab_epilogue_store_policy.txt)
// (PITCH: bytes of a tile row, 1024 = 512 columns; a narrower tile keeps the chunk swizzle)
template <int R, bool NT = false, int PITCH = 1024>
CC_DEV void tile_store_transposed(const char* lds, void* out_t, int64_t ldt, int64_t col0, int ncols, int64_t row0,
                                  int nrows) {
  constexpr int RQ = R / 32;      // 32-row bands
  constexpr int NCG = PITCH / 32;  // 16-column groups
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  for (int it = wave; it < NCG * RQ; it += 4) {
    const int cg = it / RQ, rb = (it % RQ) * 32 + g * 8;  // 16-column group, first of the lane's 8 rows
    const int ca = cg * 16 + 4 * p, c = cg * 16 + i;
    const int l0 = rb + q, l1 = rb + 4 + q;
    const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_bf16x4_s*)(lds + l0 * PITCH + (((ca >> 3) ^ (l0 & 7)) << 4) + (ca & 4) * 2));
    const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_bf16x4_s*)(lds + l1 * PITCH + (((ca >> 3) ^ (l1 & 7)) << 4) + (ca & 4) * 2));
    if (c < ncols && rb < nrows) {
      const bf16x8 v = bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      bf16x8* dst = (bf16x8*)((bf16_t*)out_t + (col0 + c) * ldt + row0 + rb);
      if constexpr (NT) __builtin_nontemporal_store(v, dst);
      else *dst = v;
    }
  }
}

// prep_kernel<.., CC_BF16, true>'s block of 64 rows, 128 columns wide (grid (ceil(K/128), ceil(B/64))), for the
// workgroups of the Adam launch that carry the prep (adam_bulk_prep_kernel): 2 rows per thread in registers and an
// 8 KB tile, so the launch keeps the Adam's 8 workgroups per CU, and x^T still goes out in 64-byte runs (32 rows).
// lane & 15 -> 8 columns, thread >> 4 -> rows slot, slot + 16 of each half.  The same bits as prep_kernel: the
// column sums are re-read from the tile (the stored bf16 values are what prep_kernel adds), one (column, row class
// r % 4) per accumulator, adding rows in prep_kernel's order; the classes are combined as there.
constexpr int PREPN_COLS = 128, PREPN_LDS = 32 * PREPN_COLS * 2;
template <int DIN, int DF>
CC_DEV void prep_block_narrow(char* lds, int bx, int by, const void* __restrict__ x_in,
                              const void* __restrict__ factor, void* __restrict__ x_out,
                              float* __restrict__ colsum_part, int B, int n, int d, void* __restrict__ x_t) {
  constexpr int PITCH = PREPN_COLS * 2;
  const int K = n * d;
  const int ch = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int col = bx * PREPN_COLS + ch * 8;
  const int r0 = by * PREP_ROWS;
  const int scol = threadIdx.x & 127, sw = threadIdx.x >> 7;  // column-sum duty: row classes sw and sw + 2
  float acc[2] = {0.f, 0.f};
  float f = 1.f;
  if (factor && col < K) f = Elem<DF>::load((const typename Elem<DF>::T*)factor + col / d);
  for (int half = 0; half < 2; ++half) {
    const int base = r0 + 32 * half;
    if (base >= B) break;  // block-uniform
    const int nr = B - base < 32 ? B - base : 32;
    if (col < K) {
      float v[2][8];
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (slot + 16 * k < nr) load8<DIN>(x_in, (int64_t)(base + slot + 16 * k) * K + col, v[k]);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = slot + 16 * k;
        if (r >= nr) break;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = Elem<CC_BF16>::round(v[k][j] * f);
        store8<CC_BF16>(x_out, (int64_t)(base + r) * K + col, v[k]);
        bf16x8 b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (short)f2bf(v[k][j]);
        *(bf16x8*)(lds + r * PITCH + ((ch ^ (r & 7)) << 4)) = b;
      }
    }
    __syncthreads();
    tile_store_transposed<32, true, PITCH>(lds, x_t, B, (int64_t)bx * PREPN_COLS, K - bx * PREPN_COLS, base, nr);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int r = sw + 2 * c + 4 * k;
        if (r < nr)
          acc[c] += bf2f(*(const bf16_t*)(lds + r * PITCH + (((scol >> 3) ^ (r & 7)) << 4) + (scol & 7) * 2));
      }
    __syncthreads();
  }
  if (!colsum_part) return;
  float(*red)[PREPN_COLS] = (float(*)[PREPN_COLS])lds;
  red[sw][scol] = acc[0];
  red[sw + 2][scol] = acc[1];
  __syncthreads();
  if (threadIdx.x < PREPN_COLS) {
    const int c = bx * PREPN_COLS + threadIdx.x, i = threadIdx.x;
    if (c < K) colsum_part[(int64_t)by * K + c] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// ---------------------------------------------------------------------------------------
// The only copy of the prep's argument checks, for cc_prep_input (tr = false: either output dtype), cc_prep_input_t
// and cc_adam_step_prep (tr: x^T too, so bf16 out and B % 8 == 0), in the order NULL, shape, output dtype, alignment,
// factor dtype, input dtype.  (B and n * d reach the kernels as int.)
static inline int check_prep(const void* x_in, int in_dtype, const void* factor, int factor_dtype, const void* x_out,
                             const void* x_t, bool tr, int64_t B, int64_t n, int64_t d, int dtype) {
  if (!x_in || !x_out || (tr && !x_t)) return CC_ERR_NULL;
  if (B <= 0 || n <= 0 || d <= 0 || d % 8 || (tr && B % 8) || B > INT32_MAX || n * d > INT32_MAX) return CC_ERR_SHAPE;
  if (dtype != CC_BF16 && (tr || dtype != CC_F32)) return CC_ERR_DTYPE;
  if (!al16(x_in) || !al16(x_out) || (tr && !al16(x_t))) return CC_ERR_ALIGN;
  if (factor && factor_dtype != CC_BF16 && factor_dtype != CC_F32) return CC_ERR_DTYPE;
  if (in_dtype != CC_BF16 && in_dtype != CC_F32) return CC_ERR_DTYPE;
  return CC_OK;
}
// KERNEL_CALL with DI_ = in_dtype and DF_ = the factor's dtype as constants, for arguments check_prep has passed.
// factor_bf16: a factor is given and is bf16 (an absent factor takes the fp32 form; it is never read).
#define DISPATCH_PREP(in_dtype, factor_bf16, KERNEL_CALL)                                                      \
  do {                                                                                                         \
    if ((in_dtype) == CC_BF16 && (factor_bf16)) { constexpr int DI_ = CC_BF16, DF_ = CC_BF16; KERNEL_CALL; }   \
    else if ((in_dtype) == CC_BF16) { constexpr int DI_ = CC_BF16, DF_ = CC_F32; KERNEL_CALL; }                \
    else if (factor_bf16) { constexpr int DI_ = CC_F32, DF_ = CC_BF16; KERNEL_CALL; }                          \
    else { constexpr int DI_ = CC_F32, DF_ = CC_F32; KERNEL_CALL; }                                            \
  } while (0)
