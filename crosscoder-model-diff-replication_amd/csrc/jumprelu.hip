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
// column (rows narrower than the workgroup) are first folded (fold_cols8).  Eligibility (a > 0 on its bits) and the
// fixed sums are mask_common.h's rules.
#include "mask_common.h"

namespace cc {

constexpr int JR_NT = 256, JR_NW = JR_NT / 64;
constexpr int JR_MAX_RG = 256;  // row groups (= partial rows of the slabs)

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

// a lane's 8 column sums into its row group's partial row; lanes that share a column (m.rp > 1) in lane order
CC_DEV void jr_write_part(const JrMap& m, const JrLane& l, const float (&acc)[8], float* __restrict__ part, int64_t h,
                          float* red) {
  float* const row = part + (int64_t)l.g * h;
  if (m.rp == 1) {  // (uniform)
    if (l.col_ok) store_cols8(row + l.col, acc);
    return;
  }
  const int tid = threadIdx.x;
  __syncthreads();  // (red may still be read by the fold before)
  fold_cols8(acc, red, m.cpb, m.rp, tid, row, tid * 8);  // (rp > 1: one column block, cpb == U)
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
  const Cols8 th = load_cols8(theta, l.col, l.col_ok);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  uint32_t kept_n = 0u;

  const int64_t stride = (int64_t)m.rg * m.rp;
  int64_t row = (int64_t)l.g * m.rp + l.r_in;
  bool ok = l.col_ok && row < B;
  Vec8<DT> cur = load_vec8<DT>(acts, row * ld + l.col, ok);
  for (int64_t rb = (int64_t)l.g * m.rp; rb < B; rb += stride) {  // (uniform trip count)
    const int64_t row_n = row + stride;
    const bool ok_n = l.col_ok && row_n < B;
    const Vec8<DT> nxt = load_vec8<DT>(acts, row_n * ld + l.col, ok_n);
    uint32_t u[8], o[8], gt[8];
    vec8_bits<DT>(cur, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bits_float<DT>(u[j]);
      const bool pos = is_pos<ELEM_BITS<DT>>(u[j]);
      const float d = __fsub_rn(a, th.v[j]);
      const bool kept = pos && a > th.v[j];
      const bool gated = pos && d > -half;
      o[j] = kept ? u[j] : 0u;
      gt[j] = gated ? u[j] : 0u;
      acc[j] += kept ? a : 0.f;
      kept_n += kept ? 1u : 0u;
    }
    if (ok) {
      const int64_t e = row * ld + l.col;
      if (acts_out) store_bits8<DT>(acts_out, e, o);
      if (gate_out) store_bits8<DT>(gate_out, e, gt);
    }
    row = row_n;
    ok = ok_n;
    cur = nxt;
  }

  if (colsum_part) jr_write_part(m, l, acc, colsum_part, h, red);
  if (l0_part) count_to_part<JR_NW>(kept_n, wred, l0_part + blockIdx.x);
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
  const Cols8 th = load_cols8(theta, l.col, l.col_ok);
  float acc_g[8], acc_t[8];
  double c1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c1[j] = -((double)th.v[j] * inv_eps);  // -(theta / eps)
    acc_g[j] = 0.f;
    acc_t[j] = 0.f;
  }

  const int64_t stride = (int64_t)m.rg * m.rp;
  int64_t row = (int64_t)l.g * m.rp + l.r_in;
  bool ok = l.col_ok && row < B;
  Vec8<DT> cur_g = load_vec8<DT>(g_pre, row * ld + l.col, ok);
  Vec8<DT> cur_a = load_vec8<DT>(gate, row * ld + l.col, ok);
  for (int64_t rb = (int64_t)l.g * m.rp; rb < B; rb += stride) {  // (uniform trip count)
    const int64_t row_n = row + stride;
    const bool ok_n = l.col_ok && row_n < B;
    const Vec8<DT> nxt_g = load_vec8<DT>(g_pre, row_n * ld + l.col, ok_n);
    const Vec8<DT> nxt_a = load_vec8<DT>(gate, row_n * ld + l.col, ok_n);
    uint32_t ug[8], ua[8], o[8];
    vec8_bits<DT>(cur_g, ug);
    vec8_bits<DT>(cur_a, ua);
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bits_float<DT>(ua[j]), G = bits_float<DT>(ug[j]);
      const bool gated = is_pos<ELEM_BITS<DT>>(ua[j]);  // (the gate holds a's bits where a > 0 and d > -half, else +0)
      const float d = __fsub_rn(a, th.v[j]);
      const bool kept = gated && a > th.v[j];
      const bool window = gated && d < half;
      acc_t[j] += window ? (float)__builtin_fma(c1[j], (double)G, c0) : 0.f;
      const bool drop = gated && !kept;
      o[j] = drop ? 0u : ug[j];
      changed |= drop;
      acc_g[j] += drop ? 0.f : G;
    }
    if (ok && changed) store_bits8<DT>(g_pre, row * ld + l.col, o);
    row = row_n;
    ok = ok_n;
    cur_g = nxt_g;
    cur_a = nxt_a;
  }
  if (thr_part) jr_write_part(m, l, acc_t, thr_part, h, red);
  if (gpre_colsum_part) jr_write_part(m, l, acc_g, gpre_colsum_part, h, red);
}

// (eps is finite and > 0: the entry points' own shape condition)
static bool jr_eps_ok(float eps) { return eps > 0.f && eps < __builtin_inff(); }

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_jumprelu_part_rows(int64_t B, int64_t h) { return dims_ok(B, h) ? jr_map(B, h).rg : 0; }
int64_t cc_jumprelu_l0_parts(int64_t B, int64_t h) {
  if (!dims_ok(B, h)) return 0;
  const JrMap m = jr_map(B, h);
  return (int64_t)m.rg * m.cb;
}

int cc_jumprelu_mask(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta, float eps,
                     void* acts_out, void* gate_out, float* colsum_part, float* l0_part, void* stream) {
  const int rc = rows_check(ld, B, h, dtype, jr_eps_ok(eps), acts && theta && acts_out, true,
                            {acts, theta, acts_out, gate_out, colsum_part}, {l0_part});
  if (rc != CC_OK) return rc;
  const JrMap m = jr_map(B, h);
  const dim3 grid((unsigned)(m.rg * m.cb)), blk(JR_NT);
  hipStream_t st = (hipStream_t)stream;
  const float half = 0.5f * eps;
  const auto kern = CC_BY_DTYPE(jr_mask_kernel, dtype);
  hipLaunchKernelGGL(kern, grid, blk, 0, st, acts, ld, (int)B, (int)h, theta, half, m, acts_out, gate_out, colsum_part,
                     l0_part);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_jumprelu_bwd(void* g_pre, const void* gate, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta,
                    float eps, float l0_scale, float* gpre_colsum_part, float* thr_part, void* stream) {
  const int rc = rows_check(ld, B, h, dtype, jr_eps_ok(eps), g_pre && gate && theta && g_pre != gate, true,
                            {g_pre, gate, theta, gpre_colsum_part, thr_part});
  if (rc != CC_OK) return rc;
  const JrMap m = jr_map(B, h);
  const dim3 grid((unsigned)(m.rg * m.cb)), blk(JR_NT);
  hipStream_t st = (hipStream_t)stream;
  const float half = 0.5f * eps;
  const double inv_eps = 1.0 / (double)eps, c0 = -((double)l0_scale * inv_eps);
  const auto kern = CC_BY_DTYPE(jr_bwd_kernel, dtype);
  hipLaunchKernelGGL(kern, grid, blk, 0, st, g_pre, gate, ld, (int)B, (int)h, theta, half, inv_eps, c0, m,
                     gpre_colsum_part, thr_part);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
