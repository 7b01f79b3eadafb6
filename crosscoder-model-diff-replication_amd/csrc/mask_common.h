// Shared helpers of the activation-mask kernels (topk.hip, batch_topk.hip, jumprelu.hip, auxk.hip): the device
// primitives that fix their numerical contract, and the argument checks of their entry points.  gfx950.
//
// The three rules every mask kernel keeps; each is written once, here:
//   eligibility   an element counts iff it is > 0 on its bits: sign clear, not zero, not NaN; +inf and subnormals
//                 count (is_pos).  Positive floats order as their bit patterns, so the bits are the selection key.
//   tie order     equal keys are admitted in flat-index order.  A lane owns 8 consecutive elements, so the order
//                 inside a workgroup is (lane, element): a prefix count across the lanes of a wave, then across
//                 the waves (CC_BLOCK_EXCL_SCAN).
//   fixed sums    no float atomics.  A column sum is added by the lane that owns the column, in program order;
//                 lanes that share a column are folded through LDS in lane order (fold_cols8); counts are integers
//                 until the one conversion (count_to_part).  So every output is fixed by (B, h) and the inputs.
#pragma once
#include <initializer_list>

#include "cc_common.h"

namespace cc {

constexpr int MASK_MAX_H = 1 << 17;

// ---- 8 consecutive elements as raw bits: one 16-B (bf16) or two 16-B (fp32) accesses
template <int DT> struct Vec8 { uint4 q[DT == CC_F32 ? 2 : 1]; };
template <int DT> constexpr int ELEM_BITS = DT == CC_BF16 ? 16 : 32;

template <int DT> CC_DEV Vec8<DT> load_vec8(const void* base, int64_t e, bool ok) {
  Vec8<DT> v;
  if constexpr (DT == CC_BF16) {
    v.q[0] = ok ? *(const uint4*)((const bf16_t*)base + e) : uint4{0u, 0u, 0u, 0u};
  } else {
    v.q[0] = ok ? *(const uint4*)((const float*)base + e) : uint4{0u, 0u, 0u, 0u};
    v.q[1] = ok ? *(const uint4*)((const float*)base + e + 4) : uint4{0u, 0u, 0u, 0u};
  }
  return v;
}

// the 8 elements' bits
template <int DT> CC_DEV void vec8_bits(const Vec8<DT>& v, uint32_t (&u)[8]) {
  if constexpr (DT == CC_BF16) {
    const uint32_t w[4] = {v.q[0].x, v.q[0].y, v.q[0].z, v.q[0].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u[2 * j] = w[j] & 0xffffu;
      u[2 * j + 1] = w[j] >> 16;
    }
  } else {
    u[0] = v.q[0].x; u[1] = v.q[0].y; u[2] = v.q[0].z; u[3] = v.q[0].w;
    u[4] = v.q[1].x; u[5] = v.q[1].y; u[6] = v.q[1].z; u[7] = v.q[1].w;
  }
}

template <int DT> CC_DEV void store_bits8(void* base, int64_t e, const uint32_t (&u)[8]) {
  if constexpr (DT == CC_BF16) {
    *(uint4*)((bf16_t*)base + e) = uint4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
  } else {
    *(uint4*)((float*)base + e) = uint4{u[0], u[1], u[2], u[3]};
    *(uint4*)((float*)base + e + 4) = uint4{u[4], u[5], u[6], u[7]};
  }
}

// the eligibility rule: bits > 0 as a float of EB bits' width
template <int EB> CC_DEV bool is_pos(uint32_t u) {
  constexpr uint32_t INF = EB == 16 ? 0x7F80u : 0x7F800000u;
  return (u - 1u) < INF;
}
// the key: an eligible element's bits, else 0
template <int EB> CC_DEV uint32_t pos_key(uint32_t u) { return is_pos<EB>(u) ? u : 0u; }
template <int DT> CC_DEV float bits_float(uint32_t u) { return __uint_as_float(DT == CC_BF16 ? u << 16 : u); }

// 8 fp32 per-column values of a lane (zeros when !ok)
struct Cols8 { float v[8]; };
CC_DEV Cols8 load_cols8(const float* __restrict__ p, int col, bool ok) {
  const float4 a = ok ? *(const float4*)(p + col) : float4{0.f, 0.f, 0.f, 0.f};
  const float4 b = ok ? *(const float4*)(p + col + 4) : float4{0.f, 0.f, 0.f, 0.f};
  return Cols8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
CC_DEV void store_cols8(float* p, const float (&v)[8]) {
  *(float4*)p = float4{v[0], v[1], v[2], v[3]};
  *(float4*)(p + 4) = float4{v[4], v[5], v[6], v[7]};
}

// ---- integer sums over a wave and a workgroup
CC_DEV uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
CC_DEV uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the tie order: the sum of v over the lanes before this one (lane, then wave order) and, in `all`, over the
// workgroup: declares `uint32_t before, all`.  wtot: NW words of LDS that no lane still reads (callers alternate
// two sets); holds one barrier.  (A macro: written as a function, in each of the forms tried, hipcc pairs the
// unrolled LDS reads differently and bt_mask_kernel grows by 9 VGPRs.)
#define CC_BLOCK_EXCL_SCAN(NW, v, lane, w, wtot, before, all) \
  uint32_t before, all = 0u;                                   \
  {                                                            \
    const uint32_t incl_ = wave_incl_scan(v, lane);            \
    if ((lane) == 63) (wtot)[w] = incl_;                       \
    __syncthreads();                                           \
    before = incl_ - (v);                                      \
    _Pragma("unroll") for (int q_ = 0; q_ < (NW); ++q_) {      \
      const uint32_t t_ = (wtot)[q_];                          \
      if (q_ < (w)) before += t_;                              \
      all += t_;                                               \
    }                                                          \
  }

// the workgroup's count into *dst: a wave sum, then thread 0 adds the NW waves in order.  Holds one barrier.
template <int NW> CC_DEV void count_to_part(uint32_t n, uint32_t* wred, float* __restrict__ dst) {
  const uint32_t t = wave_sum_u(n);
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0u;
#pragma unroll
    for (int q = 0; q < NW; ++q) all += wred[q];
    *dst = (float)all;
  }
}

// ---- column-sum partial rows
// zero the workgroup's own partial row: lane tid owns columns c * ch + 8 tid of each of nch chunks
CC_DEV void zero_cols(float* row, int nch, int ch, int tid, int h) {
  for (int c = 0; c < nch; ++c) {
    const int col = c * ch + tid * 8;
    if (col < h) {
      *(float4*)(row + col) = float4{0.f, 0.f, 0.f, 0.f};
      *(float4*)(row + col + 4) = float4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// the 8 column sums of the lanes that share a column -- lane r * cpb + t for r < rp holds columns 8 t .. 8 t + 7 --
// added in lane order (r ascending) by lane t < cpb and stored at row[col].  red: 8 floats per lane of LDS that no
// lane still reads; holds one barrier.
CC_DEV void fold_cols8(const float (&acc)[8], float* red, int cpb, int rp, int tid, float* row, int col) {
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = acc[j];
  __syncthreads();
  if (tid < cpb) {
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = 0.f;
    for (int r = 0; r < rp; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] += red[(r * cpb + tid) * 8 + j];
    store_cols8(row + col, t);
  }
}

// ---- host: the entry points' argument checks
// [B][ld] activations with h columns, 8 elements per lane
static bool rows_shape_ok(int64_t ld, int64_t B, int64_t h) {
  return B >= 1 && h >= 8 && !(h & 7) && !(ld & 7) && ld >= h;
}
// h within the kernels' range and the flat extent B * h within 2^31
static bool dims_ok(int64_t B, int64_t h) {
  return B >= 1 && h >= 8 && !(h & 7) && h <= MASK_MAX_H && B <= ((int64_t)1 << 31) / h;
}
static bool aligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
  uintptr_t all = 0;
  for (const void* p : ptrs) all |= (uintptr_t)p;
  return !(all & mask);
}
// The CC_ERR_* code of an entry point over such activations, in the one order: shape (with the entry point's own
// condition), null (ptrs_ok: its required pointers), dtype, too large (flat: B * h within 2^31, else B within
// 2^30), alignment (p16 / p8 / p4: pointers by required alignment; null ones pass).
static int rows_check(int64_t ld, int64_t B, int64_t h, int dtype, bool shape_ok, bool ptrs_ok, bool flat,
                      std::initializer_list<const void*> p16, std::initializer_list<const void*> p4 = {},
                      std::initializer_list<const void*> p8 = {}) {
  if (!rows_shape_ok(ld, B, h) || !shape_ok) return CC_ERR_SHAPE;
  if (!ptrs_ok) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > MASK_MAX_H || B > (flat ? ((int64_t)1 << 31) / h : (int64_t)1 << 30)) return CC_ERR_TOO_LARGE;
  if (!aligned(p16, 15) || !aligned(p8, 7) || !aligned(p4, 3)) return CC_ERR_ALIGN;
  return CC_OK;
}

}  // namespace cc

// F<CC_BF16, ...> or F<CC_F32, ...> by the run-time dtype: a kernel or a launch function of one signature
#define CC_BY_DTYPE(F, dtype, ...) ((dtype) == CC_BF16 ? F<CC_BF16, ##__VA_ARGS__> : F<CC_F32, ##__VA_ARGS__>)
