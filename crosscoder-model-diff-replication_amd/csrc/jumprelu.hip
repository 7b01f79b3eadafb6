// JumpReLU crosscoders: f = a * H(a - theta[latent]) with one learned fp32 threshold per latent, and the pass of the
// backward that forms the threshold's gradient.  gfx950.
//
//   jr_mask_kernel  acts [B][ld], first h columns -> the masked activations (kept: a > 0 on its bits and
//                   float(a) > theta, strictly), the gate G3 masks with (a > 0 and a - theta > -eps/2: the kept
//                   elements plus the lower half of the straight-through window) and the step's side outputs of the
//                   kept elements (column-sum partials, counts).
//   jr_bwd_kernel   one pass over g_pre (G3's output under the gate) and the gate: the window's terms
//                   -(theta/eps) G - (l0_coeff/B)/eps into thr_part, g_pre zeroed where gated but not kept, and the
//                   column-sum partials of the resulting g_pre.
// Both are pure streaming kernels.  Work split: a row is h / 8 units of 8 consecutive columns; a workgroup owns
// min(h / 8, 256) units -- one per lane, several rows per pass when the row is narrower than the workgroup -- of one
// of `cb` column blocks, and the rows of one of `rg` row groups in a grid-stride (group g: row blocks g, g + rg, ...).
// So a lane owns the same 8 columns throughout: their thresholds and their column accumulators live in registers,
// and the loop has no barrier.  Afterwards a lane writes its sums to its row group's partial row; lanes that share a
// column (rows narrower than the workgroup) are first folded through LDS in lane order.  No float atomics: every output
// is fixed by (B, h) and the inputs.
#include "cc_common.h"

namespace cc {

constexpr int JR_NT = 256, JR_NW = JR_NT / 64;
constexpr int JR_MAX_RG = 256;  // row groups (= partial rows of the slabs)
constexpr int JR_MAX_H = 1 << 17;

struct JrMap {
  int U;    // 8-column units per row
  int cpb;  // units a workgroup owns (one per lane)
  int cb;   // column blocks
  int rp;   // rows per pass of a workgroup
  int rg;   // row groups
};

static JrMap jr_map(int64_t B, int64_t h) {
  JrMap m;
  m.U = (int)(h / 8);
  m.cpb = m.U < JR_NT ? m.U : JR_NT;
  m.cb = (m.U + m.cpb - 1) / m.cpb;
  m.rp = JR_NT / m.cpb;
  const int64_t nrb = (B + m.rp - 1) / m.rp;
  m.rg = (int)(nrb < JR_MAX_RG ? nrb : JR_MAX_RG);
  return m;
}

struct JrVec { uint4 q[2]; };

template <int DT> CC_DEV JrVec jr_load(const void* base, int64_t e, bool ok) {
  JrVec v;
  v.q[1] = uint4{0u, 0u, 0u, 0u};
  if constexpr (DT == CC_BF16) {
    v.q[0] = ok ? *(const uint4*)((const bf16_t*)base + e) : uint4{0u, 0u, 0u, 0u};
  } else {
    v.q[0] = ok ? *(const uint4*)((const float*)base + e) : uint4{0u, 0u, 0u, 0u};
    v.q[1] = ok ? *(const uint4*)((const float*)base + e + 4) : uint4{0u, 0u, 0u, 0u};
  }
  return v;
}

template <int DT> CC_DEV void jr_bits(const JrVec& v, uint32_t (&u)[8]) {
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

template <int DT> CC_DEV void jr_store(void* base, int64_t e, const uint32_t (&u)[8]) {
  if constexpr (DT == CC_BF16) {
    *(uint4*)((bf16_t*)base + e) = uint4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
  } else {
    *(uint4*)((float*)base + e) = uint4{u[0], u[1], u[2], u[3]};
    *(uint4*)((float*)base + e + 4) = uint4{u[4], u[5], u[6], u[7]};
  }
}

// a > 0 on the element's bits: sign clear, not zero, not NaN; +inf and subnormals count (cc_topk_rows' rule)
template <int DT> CC_DEV bool jr_pos(uint32_t u) {
  constexpr uint32_t INF = DT == CC_BF16 ? 0x7F80u : 0x7F800000u;
  return (u - 1u) < INF;
}
template <int DT> CC_DEV float jr_float(uint32_t u) { return __uint_as_float(DT == CC_BF16 ? u << 16 : u); }

// a lane's place: its unit of columns, its row inside a pass, and the first row block of its workgroup
struct JrLane {
  int col, r_in, g;
  bool col_ok;
};
CC_DEV JrLane jr_lane(const JrMap& m) {
  JrLane l;
  const int tid = threadIdx.x;
  const int cblk = blockIdx.x % m.cb;
  l.g = blockIdx.x / m.cb;
  l.r_in = tid / m.cpb;
  const int unit = cblk * m.cpb + (tid - l.r_in * m.cpb);
  l.col = unit * 8;
  l.col_ok = unit < m.U && l.r_in < m.rp;
  return l;
}

CC_DEV void jr_load_theta(const float* __restrict__ theta, const JrLane& l, float (&th)[8]) {
  const float4 a = l.col_ok ? *(const float4*)(theta + l.col) : float4{0.f, 0.f, 0.f, 0.f};
  const float4 b = l.col_ok ? *(const float4*)(theta + l.col + 4) : float4{0.f, 0.f, 0.f, 0.f};
  th[0] = a.x; th[1] = a.y; th[2] = a.z; th[3] = a.w;
  th[4] = b.x; th[5] = b.y; th[6] = b.z; th[7] = b.w;
}

// a lane's 8 column sums into its row group's partial row; lanes that share a column (m.rp > 1) in lane order
CC_DEV void jr_write_part(const JrMap& m, const JrLane& l, const float (&acc)[8], float* __restrict__ part, int64_t h,
                          float* red) {
  float* const row = part + (int64_t)l.g * h;
  if (m.rp == 1) {  // (uniform)
    if (l.col_ok) {
      *(float4*)(row + l.col) = float4{acc[0], acc[1], acc[2], acc[3]};
      *(float4*)(row + l.col + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
    }
    return;
  }
  const int tid = threadIdx.x;
  __syncthreads();  // (red may still be read by the fold before)
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid * 8 + j] = acc[j];
  __syncthreads();
  if (tid < m.cpb) {  // (rp > 1: one column block, cpb == U)
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = 0.f;
    for (int r = 0; r < m.rp; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] += red[(r * m.cpb + tid) * 8 + j];
    *(float4*)(row + tid * 8) = float4{t[0], t[1], t[2], t[3]};
    *(float4*)(row + tid * 8 + 4) = float4{t[4], t[5], t[6], t[7]};
  }
}

// ---- the forward mask (acts and acts_out may be the same buffer: no __restrict__ on them; a lane reads its elements
// of a row before it writes them, and no lane reads another's)
template <int DT>
__global__ __launch_bounds__(JR_NT) void jr_mask_kernel(const void* acts, int64_t ld, int B, int h,
                                                        const float* __restrict__ theta, float half, JrMap m,
                                                        void* acts_out, void* gate_out, float* __restrict__ colsum_part,
                                                        float* __restrict__ l0_part) {
  __shared__ float red[JR_NT * 8];
  __shared__ uint32_t wred[JR_NW];
  const JrLane l = jr_lane(m);
  float th[8], acc[8];
  jr_load_theta(theta, l, th);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  uint32_t kept_n = 0u;

  const int64_t stride = (int64_t)m.rg * m.rp;
  int64_t row = (int64_t)l.g * m.rp + l.r_in;
  bool ok = l.col_ok && row < B;
  JrVec cur = jr_load<DT>(acts, row * ld + l.col, ok);
  for (int64_t rb = (int64_t)l.g * m.rp; rb < B; rb += stride) {  // (uniform trip count)
    const int64_t row_n = row + stride;
    const bool ok_n = l.col_ok && row_n < B;
    const JrVec nxt = jr_load<DT>(acts, row_n * ld + l.col, ok_n);
    uint32_t u[8], o[8], gt[8];
    jr_bits<DT>(cur, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = jr_float<DT>(u[j]);
      const bool pos = jr_pos<DT>(u[j]);
      const float d = __fsub_rn(a, th[j]);
      const bool kept = pos && a > th[j];
      const bool gated = pos && d > -half;
      o[j] = kept ? u[j] : 0u;
      gt[j] = gated ? u[j] : 0u;
      acc[j] += kept ? a : 0.f;
      kept_n += kept ? 1u : 0u;
    }
    if (ok) {
      const int64_t e = row * ld + l.col;
      if (acts_out) jr_store<DT>(acts_out, e, o);
      if (gate_out) jr_store<DT>(gate_out, e, gt);
    }
    row = row_n;
    ok = ok_n;
    cur = nxt;
  }

  if (colsum_part) jr_write_part(m, l, acc, colsum_part, h, red);
  if (l0_part) {
    uint32_t t = kept_n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t all = 0u;
#pragma unroll
      for (int q = 0; q < JR_NW; ++q) all += wred[q];
      l0_part[blockIdx.x] = (float)all;
    }
  }
}

// ---- the backward pass over g_pre and the gate
template <int DT>
__global__ __launch_bounds__(JR_NT) void jr_bwd_kernel(void* __restrict__ g_pre, const void* __restrict__ gate,
                                                       int64_t ld, int B, int h, const float* __restrict__ theta,
                                                       float half, double inv_eps, double c0, JrMap m,
                                                       float* __restrict__ gpre_colsum_part,
                                                       float* __restrict__ thr_part) {
  __shared__ float red[JR_NT * 8];
  const JrLane l = jr_lane(m);
  // a window term is formed in fp64 and rounded once, so a partial sum of n terms is within n 2^-24 sum |term| of
  // the exact one whatever cancels inside a term
  float th[8], acc_g[8], acc_t[8];
  double c1[8];
  jr_load_theta(theta, l, th);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c1[j] = -((double)th[j] * inv_eps);  // -(theta / eps)
    acc_g[j] = 0.f;
    acc_t[j] = 0.f;
  }

  const int64_t stride = (int64_t)m.rg * m.rp;
  int64_t row = (int64_t)l.g * m.rp + l.r_in;
  bool ok = l.col_ok && row < B;
  JrVec cur_g = jr_load<DT>(g_pre, row * ld + l.col, ok);
  JrVec cur_a = jr_load<DT>(gate, row * ld + l.col, ok);
  for (int64_t rb = (int64_t)l.g * m.rp; rb < B; rb += stride) {  // (uniform trip count)
    const int64_t row_n = row + stride;
    const bool ok_n = l.col_ok && row_n < B;
    const JrVec nxt_g = jr_load<DT>(g_pre, row_n * ld + l.col, ok_n);
    const JrVec nxt_a = jr_load<DT>(gate, row_n * ld + l.col, ok_n);
    uint32_t ug[8], ua[8], o[8];
    jr_bits<DT>(cur_g, ug);
    jr_bits<DT>(cur_a, ua);
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = jr_float<DT>(ua[j]), G = jr_float<DT>(ug[j]);
      const bool gated = jr_pos<DT>(ua[j]);  // (the gate holds a's bits where a > 0 and d > -half, else +0)
      const float d = __fsub_rn(a, th[j]);
      const bool kept = gated && a > th[j];
      const bool window = gated && d < half;
      acc_t[j] += window ? (float)__builtin_fma(c1[j], (double)G, c0) : 0.f;
      const bool drop = gated && !kept;
      o[j] = drop ? 0u : ug[j];
      changed |= drop;
      acc_g[j] += drop ? 0.f : G;
    }
    if (ok && changed) jr_store<DT>(g_pre, row * ld + l.col, o);
    row = row_n;
    ok = ok_n;
    cur_g = nxt_g;
    cur_a = nxt_a;
  }
  if (thr_part) jr_write_part(m, l, acc_t, thr_part, h, red);
  if (gpre_colsum_part) jr_write_part(m, l, acc_g, gpre_colsum_part, h, red);
}

static bool jr_dims_ok(int64_t B, int64_t h) {
  return B >= 1 && h >= 8 && !(h & 7) && h <= JR_MAX_H && B <= ((int64_t)1 << 31) / h;
}

// cc_topk_rows' order: shape, null, dtype, too large, alignment
static int jr_check(const void* a, const void* b, bool needed, int64_t ld, int64_t B, int64_t h, int dtype, float eps,
                    const void* p16a, const void* p16b, const void* p16c, const void* p16d, const void* p4) {
  if (B < 1 || h < 8 || (h & 7) || (ld & 7) || ld < h || !(eps > 0.f) || !(eps < __builtin_inff())) return CC_ERR_SHAPE;
  if (!a || !b || !needed) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > JR_MAX_H || B > ((int64_t)1 << 31) / h) return CC_ERR_TOO_LARGE;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)p16a | (uintptr_t)p16b | (uintptr_t)p16c | (uintptr_t)p16d) & 15)
    return CC_ERR_ALIGN;
  if ((uintptr_t)p4 & 3) return CC_ERR_ALIGN;
  return CC_OK;
}

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_jumprelu_part_rows(int64_t B, int64_t h) { return jr_dims_ok(B, h) ? jr_map(B, h).rg : 0; }
int64_t cc_jumprelu_l0_parts(int64_t B, int64_t h) {
  if (!jr_dims_ok(B, h)) return 0;
  const JrMap m = jr_map(B, h);
  return (int64_t)m.rg * m.cb;
}

int cc_jumprelu_mask(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta, float eps,
                     void* acts_out, void* gate_out, float* colsum_part, float* l0_part, void* stream) {
  const int rc = jr_check(acts, theta, acts_out != nullptr, ld, B, h, dtype, eps, acts_out, gate_out, colsum_part,
                          nullptr, l0_part);
  if (rc != CC_OK) return rc;
  const JrMap m = jr_map(B, h);
  const dim3 grid((unsigned)(m.rg * m.cb)), blk(JR_NT);
  hipStream_t st = (hipStream_t)stream;
  const float half = 0.5f * eps;
  if (dtype == CC_BF16)
    hipLaunchKernelGGL((jr_mask_kernel<CC_BF16>), grid, blk, 0, st, acts, ld, (int)B, (int)h, theta, half, m, acts_out,
                       gate_out, colsum_part, l0_part);
  else
    hipLaunchKernelGGL((jr_mask_kernel<CC_F32>), grid, blk, 0, st, acts, ld, (int)B, (int)h, theta, half, m, acts_out,
                       gate_out, colsum_part, l0_part);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_jumprelu_bwd(void* g_pre, const void* gate, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta,
                    float eps, float l0_scale, float* gpre_colsum_part, float* thr_part, void* stream) {
  int rc = jr_check(g_pre, gate, theta != nullptr && g_pre != gate, ld, B, h, dtype, eps, theta, gpre_colsum_part,
                    thr_part, nullptr, nullptr);
  if (rc != CC_OK) return rc;
  const JrMap m = jr_map(B, h);
  const dim3 grid((unsigned)(m.rg * m.cb)), blk(JR_NT);
  hipStream_t st = (hipStream_t)stream;
  const float half = 0.5f * eps;
  const double inv_eps = 1.0 / (double)eps, c0 = -((double)l0_scale * inv_eps);
  if (dtype == CC_BF16)
    hipLaunchKernelGGL((jr_bwd_kernel<CC_BF16>), grid, blk, 0, st, g_pre, gate, ld, (int)B, (int)h, theta, half,
                       inv_eps, c0, m, gpre_colsum_part, thr_part);
  else
    hipLaunchKernelGGL((jr_bwd_kernel<CC_F32>), grid, blk, 0, st, g_pre, gate, ld, (int)B, (int)h, theta, half, inv_eps,
                       c0, m, gpre_colsum_part, thr_part);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
