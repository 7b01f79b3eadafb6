// The Adam update of the crosscoder training step (gfx950): the fused clip-multiply + Adam kernels -- bulk, the bulk
// form that carries the next batch's prep, the capped grid-stride and pipelined forms that run beside a GEMM, the
// fp32-master form and the decoder form that also writes W_dec^T -- their launch helpers and entry points, and the
// test library's hooks (-DCC_DEBUG_HOOKS).  All vector accesses are 16 B per lane; no float atomics.
#include "cc_common.h"

#include <cfloat>
#include <cmath>

namespace cc {

#include "grad_tail.h"
#include "prep_tile.h"

// ---------------------------------------------------------------------------------------
// Fused clip-multiply + Adam (torch/optim/adam.py _single_tensor_adam, no wd/amsgrad), with the
// dtype rounding after each of torch's tensor ops:
//   g = R(g*coef); m = R(lerp(m, g, 1-b1)); v = R(R(v*b2) + (1-b2)*g*g);
//   den = R(R(R(sqrt v) / bc2s) + eps); p = R(p + (-step_size) * (m / den))
struct AdamArgs {
  void* p;
  const void* g;
  void* m;
  void* v;
  int64_t numel;
  const float* coef;
  float w1;         // 1 - beta1 (lerp weight)
  float beta2, omb2, eps;
  float bc2s;       // sqrt(1 - beta2^t)
  float rb;         // float(1 / (double)bc2s): the bf16 kernels divide by bc2s with it (adam_udiv)
  float neg_step;   // -lr / (1 - beta1^t)
  // bf16 only: the scalars are inside the fast arithmetic's domain (adam_args); 0 sends every chunk to adam_elem
  // (the test library's cc_debug_set_adam_ref does that on purpose)
  int fast;
#ifdef CC_DEBUG_HOOKS
  unsigned long long* redo_ctr;  // test library: counts the 8-element chunks redone with adam_elem
#endif
  // clip coefficient formed in the kernel (instead of read from coef): clip_grad_norm_ over the clip_np
  // per-parameter squared sums clip_sums (e.g. all-reduced over the latent shards); block 0 writes clip_out
  // [coef, total, norms...] like cc_clip_finalize
  const float* clip_sums;
  int clip_np, clip_emulate;
  float clip_max_norm;
  float* clip_out;
  // decoder norms' per-(row, 64-column block) squared sums of the UPDATED parameters over the first
  // norm_rows x norm_ld elements (W_dec [h][K]), in cc_dec_norms' order, into norm_part[row][K / 64]
  // (adam_kernel only; nullptr: none)
  float* norm_part;
  int norm_rows, norm_ld;
  // the capped grid-stride forms: each workgroup, when its stores are done, releases them (agent scope) and adds
  // 1 here -- a reader launched on another stream (G2, cc_decode_loss's wait_ctr) waits for the count in its
  // kernel instead of for an event (nullptr: none)
  unsigned* done_ctr;
};
// Every thread of the workgroup: its stores drained, the barrier, one agent-scope release (writes the XCD's L2
// back), then the arrival count.
CC_DEV void adam_signal_done(unsigned* ctr) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// The step's clip coefficient: read (coef), formed from squared sums (clip_sums), or 1
CC_DEV float adam_coef(const AdamArgs& a) {
  if (a.clip_sums) {
    float norms[8], total;
    bool aborted = false;  // (a negative squared sum: a rank's step was aborted -- ClipArgs::sums_only writes -inf)
    for (int p = 0; p < a.clip_np; ++p) {
      aborted |= a.clip_sums[p] < 0.f;
      norms[p] = clip_param_norm((double)a.clip_sums[p], a.clip_emulate, p);
    }
    const float c = aborted ? CC_CLIP_ABORTED : clip_coef(norms, a.clip_np, a.clip_max_norm, a.clip_emulate, total);
    if (a.clip_out && blockIdx.x == 0 && threadIdx.x == 0) {
      a.clip_out[0] = c;
      a.clip_out[1] = total;
      for (int p = 0; p < a.clip_np; ++p) a.clip_out[2 + p] = norms[p];
    }
    return c;
  }
  return a.coef ? *a.coef : 1.f;
}
// adam_coef for the whole block: from the squared sums it is ~100 dependent VALU ops (fp64 square roots), so
// one wave forms it and the others read it from LDS -- with one 8-element chunk per thread (the bulk
// kernel) every wave forming it costs the launch ~20 us.  Call with every thread of the block.  (Not for a
// kernel meant to share CUs with the GEMMs: any LDS keeps its workgroups off a CU whose LDS a GEMM
// workgroup holds.)
CC_DEV float adam_coef_block(const AdamArgs& a) {
  if (!a.clip_sums) return a.coef ? *a.coef : 1.f;
  __shared__ float s_coef;
  if (threadIdx.x < 64) {
    const float c = adam_coef(a);
    if (threadIdx.x == 0) s_coef = c;
  }
  __syncthreads();
  return s_coef;
}
// One Adam element update with torch's rounding points (see adam_kernel).
template <int DT>
CC_DEV void adam_elem(const AdamArgs& a, float coef, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
  using E = Elem<DT>;
  float gj = E::round(g * coef);
  float w = a.w1;
  float mj = w < 0.5f ? __builtin_fmaf(w, gj - m, m) : __builtin_fmaf(-(gj - m), 1.f - w, gj);
  mj = E::round(mj);
  float vj = E::round(v * a.beta2);
  vj = E::round(vj + a.omb2 * gj * gj);
  float den = E::round(sqrtf(vj));
  den = E::round(den / a.bc2s);
  den = E::round(den + a.eps);
  p = E::round(p + a.neg_step * (mj / den));
  m = mj;
  v = vj;
}

// ---------------------------------------------------------------------------------------
// The bf16 element update with half of adam_elem's vector instructions and the same bits.  Beside G1 the
// side-stream Adam is bound by vector-instruction issue, not by HBM; adam_elem<CC_BF16>
// spends most of its instructions on two IEEE divisions and a correctly rounded sqrtf whose results are rounded
// to bf16 or formed from bf16 operands:
//   sqrt      vj is a bf16 value: its exact root is never within 2^-19 (relative) of a bf16 rounding boundary,
//             so the 1-ulp v_sqrt_f32 rounds to the same bf16 as sqrtf
//   / bc2s    the divisor is uniform: q = den * rb, corrected once with the exact residual (adam_udiv)
//   mj / den  both bf16 values: fp64 reciprocal, two corrections with the exact residual, one rounding to
//             fp32 (adam_quot): no operand scaling, exact for any normal operands
// Each primitive is exact on a domain (zero or normal operands of the right sign); every
// lane checks its operands, and a wave in which any lane is outside redoes the chunk with adam_elem (one ballot
// per chunk, the cold block out of line), so the bits are adam_elem's for every input.  The roundings convert two
// elements per v_cvt_pk_bf16_f32.  The statements are asm so that the kernels keep one instruction per
// operation: hipcc otherwise pairs adjacent f32 operations into v_pk_*_f32, which beside MFMAs costs more than
// the two plain instructions.
constexpr int FPC_NEG_NORMAL = 0x008, FPC_NEG_ZERO = 0x020, FPC_POS_ZERO = 0x040, FPC_POS_NORMAL = 0x100;
template <int MASK> CC_DEV bool fp_class(float x) { return __builtin_amdgcn_classf(x, MASK); }
CC_DEV float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
CC_DEV float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
// x rounded to bf16, as a float: the conversion's high half with a zero low half
CC_DEV float round1(float x) {
  float r;
  asm("v_cvt_pk_bf16_f32 %0, 0, %1" : "=v"(r) : "v"(x));
  return r;
}
// (x, y) rounded to bf16, as floats; returns the packed pair
CC_DEV uint32_t round2(float& x, float& y) {
  uint32_t u;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u) : "v"(x), "v"(y));
  x = bf_lo(u);
  y = bf_hi(u);
  return u;
}
// One instruction each, opaque to the SLP vectoriser.  `s` operands are wave-uniform (an SGPR: the update's
// scalars cost no vector registers; one per instruction)
CC_DEV float op_mul(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
CC_DEV float op_mul_s(float s, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(b)); return r; }
CC_DEV float op_add(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
CC_DEV float op_add_s(float s, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(b)); return r; }
CC_DEV float op_sub(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
CC_DEV float op_fma(float a, float b, float c) {  // a * b + c
  float r;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
CC_DEV float op_fma_s(float a, float s, float c) {  // a * s + c
  float r;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(c));
  return r;
}
CC_DEV float op_fma_nc(float a, float b, float c) {  // a * b - c
  float r;
  asm("v_fma_f32 %0, %1, %2, -%3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
CC_DEV float op_fma_na(float a, float b, float c) {  // -a * b + c
  float r;
  asm("v_fma_f32 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
CC_DEV float op_fma_na_s(float a, float s, float c) {  // -a * s + c
  float r;
  asm("v_fma_f32 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(c));
  return r;
}
CC_DEV float uniform(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// the update's wave-uniform scalars (AdamArgs' and the clip coefficient), in SGPRs
struct AdamU {
  float coef, w1, omw, beta2, omb2, bc2s, rb, eps, neg_step;
};
CC_DEV AdamU adam_uniforms(const AdamArgs& a, float coef) {
  return {uniform(coef),   uniform(a.w1), uniform(1.f - a.w1), uniform(a.beta2),   uniform(a.omb2),
          uniform(a.bc2s), uniform(a.rb), uniform(a.eps),      uniform(a.neg_step)};
}
// den / bc2s for den = +0 or a positive normal bf16 value >= 2^-67, rb = float(1 / (double)bc2s), bc2s in
// [2^-20, 1]: the residual is exact, so the corrected quotient is the correctly rounded one (Markstein)
CC_DEV float adam_udiv(float den, float bc2s, float rb) {
  const float q = op_mul_s(rb, den);
  const float r = op_fma_na_s(q, bc2s, den);
  return op_fma_s(r, rb, q);
}
// A VALU instruction that reads a transcendental's result needs one instruction between the two, and the
// compiler's hazard pass does not look into asm statements.  So the square roots and their first readers sit in
// one asm statement that handles two elements: both transcendentals, then both readers (adam_sqrt2).
//
// mj / den for bf16 values, two at a time; ok = mj is a zero or normal and den a positive normal.  The quotient
// is formed in fp64 and rounded once to fp32, so it is the correctly rounded one over that whole domain, overflow
// and denormal results included (fp32 arithmetic would need the operand scaling of the IEEE sequence there):
// v_rcp_f64 (about 2^-23 relative) and two corrections with the exact residual leave an error below 2^-60, so a
// quotient that fp64 holds exactly -- every fp32 rounding tie among them -- comes out exact, and every other
// quotient of two 8-bit significands is at least 2^-33 away from a rounding boundary.  The residual is formed
// negated (q * den - mj, then q - r * y), which keeps the sign of a zero mj as the division does.  (Plain C++:
// the compiler places the wait state after the transcendental itself, and has no packed fp64 to pair into.)
CC_DEV float adam_quot(float mj, float den) {
#pragma clang fp contract(off)
  const double d = den, m = mj;
  const double y = __builtin_amdgcn_rcp(d);
  double q = m * y;
  q = __builtin_fma(-__builtin_fma(q, d, -m), y, q);
  q = __builtin_fma(-__builtin_fma(q, d, -m), y, q);
  return (float)q;
}
CC_DEV bool adam_quot_ok(float mj, float den) {
  return fp_class<FPC_POS_NORMAL>(den) &&
         fp_class<FPC_NEG_NORMAL | FPC_NEG_ZERO | FPC_POS_ZERO | FPC_POS_NORMAL>(mj);
}
CC_DEV void adam_quot2(float m0, float m1, float d0, float d1, float& q0, float& q1, bool& ok0, bool& ok1) {
  q0 = adam_quot(m0, d0);
  q1 = adam_quot(m1, d1);
  ok0 = adam_quot_ok(m0, d0);
  ok1 = adam_quot_ok(m1, d1);
}
// R(sqrt vj) for vj = +0 or a positive normal bf16 value (ok = that), two at a time
CC_DEV void adam_sqrt2(float v0, float v1, float& s0, float& s1, bool& ok0, bool& ok1) {
  float t0, t1;
  asm("v_sqrt_f32 %0, %4\n\tv_sqrt_f32 %1, %5\n\tv_cvt_pk_bf16_f32 %2, 0, %0\n\tv_cvt_pk_bf16_f32 %3, 0, %1"
      : "=&v"(t0), "=&v"(t1), "=&v"(s0), "=&v"(s1)
      : "v"(v0), "v"(v1));
  ok0 = fp_class<FPC_POS_ZERO | FPC_POS_NORMAL>(v0);
  ok1 = fp_class<FPC_POS_ZERO | FPC_POS_NORMAL>(v1);
}
// Two elements, one dword of each packed operand, with adam_elem's operations and rounding points; adds the
// updated parameters' squares to q in element order.  LO: the lerp weight is below 0.5 (uniform, chosen by the
// caller).  The roundings whose result is stored convert both elements in one instruction; the others convert
// one element each straight into float form, which is cheaper than a pair plus two re-expansions.  Returns
// whether both elements stayed inside the primitives' domains.
template <bool LO>
CC_DEV bool adam_pair(const AdamU& u, uint32_t& up, uint32_t ug, uint32_t& um, uint32_t& uv, float& q) {
  const float g0 = round1(op_mul_s(u.coef, bf_lo(ug))), g1 = round1(op_mul_s(u.coef, bf_hi(ug)));
  float m0 = bf_lo(um), m1 = bf_hi(um);
  const float d0 = op_sub(g0, m0), d1 = op_sub(g1, m1);
  m0 = LO ? op_fma_s(d0, u.w1, m0) : op_fma_na_s(d0, u.omw, g0);
  m1 = LO ? op_fma_s(d1, u.w1, m1) : op_fma_na_s(d1, u.omw, g1);
  um = round2(m0, m1);
  float v0 = round1(op_mul_s(u.beta2, bf_lo(uv))), v1 = round1(op_mul_s(u.beta2, bf_hi(uv)));
  v0 = op_add(v0, op_mul(op_mul_s(u.omb2, g0), g0));
  v1 = op_add(v1, op_mul(op_mul_s(u.omb2, g1), g1));
  uv = round2(v0, v1);
  // den = R(R(R(sqrt vj) / bc2s) + eps)
  float s0, s1, x0, x1;
  bool in0, in1, in2, in3;
  adam_sqrt2(v0, v1, s0, s1, in0, in1);
  s0 = round1(op_add_s(u.eps, round1(adam_udiv(s0, u.bc2s, u.rb))));
  s1 = round1(op_add_s(u.eps, round1(adam_udiv(s1, u.bc2s, u.rb))));
  adam_quot2(m0, m1, s0, s1, x0, x1, in2, in3);
  float p0 = op_add(bf_lo(up), op_mul_s(u.neg_step, x0));
  float p1 = op_add(bf_hi(up), op_mul_s(u.neg_step, x1));
  up = round2(p0, p1);
  q = op_fma(p0, p0, q);
  q = op_fma(p1, p1, q);
  return in0 && in1 && in2 && in3;
}
// One whole 8-element chunk at element i, packed, in place; returns the updated parameters' squares summed in
// element order (the decoder norms' per-lane term).  The cold block loads its operands again (nothing has been
// stored yet), so the originals need no registers while the fast arithmetic runs.
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
template <bool NT> CC_DEV bf16x8 ld_bf16x8(const void* base, int64_t i) {
  const bf16x8* q = (const bf16x8*)((const bf16_t*)base + i);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}
template <bool NT> CC_DEV void st_bf16x8(void* base, int64_t i, bf16x8 x) {
  bf16x8* q = (bf16x8*)((bf16_t*)base + i);
  if constexpr (NT) __builtin_nontemporal_store(x, q);
  else *q = x;
}
template <bool LO>
CC_DEV float adam_chunk_bf16(const AdamArgs& a, float coef, int64_t i, bf16x8& p, const bf16x8& g, bf16x8& m,
                             bf16x8& v) {
  u32x4 P = __builtin_bit_cast(u32x4, p), M = __builtin_bit_cast(u32x4, m), V = __builtin_bit_cast(u32x4, v);
  const u32x4 G = __builtin_bit_cast(u32x4, g);
  const AdamU u = adam_uniforms(a, coef);  // (loop-invariant in the callers)
  float q = 0.f;
  bool ok = a.fast != 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t pk = P[k], mk = M[k], vk = V[k];
    const bool in = adam_pair<LO>(u, pk, G[k], mk, vk, q);
    ok = ok && in;
    P[k] = pk; M[k] = mk; V[k] = vk;
  }
  p = __builtin_bit_cast(bf16x8, P);
  m = __builtin_bit_cast(bf16x8, M);
  v = __builtin_bit_cast(bf16x8, V);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
    const bf16x8 p0 = ld_bf16x8<true>(a.p, i), g0 = ld_bf16x8<true>(a.g, i), m0 = ld_bf16x8<true>(a.m, i),
                 v0 = ld_bf16x8<true>(a.v, i);
#ifdef CC_DEBUG_HOOKS
    if (a.redo_ctr) atomicAdd(a.redo_ctr, 1ull);
#endif
    q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pj = bf2f((bf16_t)p0[j]), mj = bf2f((bf16_t)m0[j]), vj = bf2f((bf16_t)v0[j]);
      adam_elem<CC_BF16>(a, coef, pj, bf2f((bf16_t)g0[j]), mj, vj);
      p[j] = (short)f2bf(pj);
      m[j] = (short)f2bf(mj);
      v[j] = (short)f2bf(vj);
      q = __fmaf_rn(pj, pj, q);
    }
  }
  return q;
}
// (row, column) of a thread's chunk in the decoder-norm matrix [norm_rows][norm_ld], carried through the
// grid-stride loop: one division per thread instead of a 64-bit one per chunk
struct NormPos {
  int row, col, drow, dcol;
};
CC_DEV NormPos norm_pos(const AdamArgs& a, int64_t i, int64_t stride) {
  NormPos n = {0, 0, 0, 0};
  if (a.norm_part) {
    n.row = (int)(i / a.norm_ld);
    n.col = (int)(i - (int64_t)n.row * a.norm_ld);
    n.drow = (int)(stride / a.norm_ld);
    n.dcol = (int)(stride - (int64_t)n.drow * a.norm_ld);
  }
  return n;
}
CC_DEV void norm_pos_next(NormPos& n, int ld) {
  n.row += n.drow;
  n.col += n.dcol;
  if (n.col >= ld) {
    n.col -= ld;
    ++n.row;
  }
}
// the chunk's partial of its (row, 64-column block): the 8 lanes of an aligned group hold one block (i % 64 ==
// 8 * (lane & 7): the grid stride is a multiple of 64, K % 64 == 0), all of them inside the matrix together
CC_DEV void norm_part_store(const AdamArgs& a, const NormPos& n, float q) {
  if (a.norm_part && n.row < a.norm_rows) {
    q = block8_sum(q);
    if ((threadIdx.x & 7) == 0) a.norm_part[(int64_t)n.row * (a.norm_ld >> 6) + (n.col >> 6)] = q;
  }
}

// cache policy of the bulk (encoder-half / whole-arena) Adam: g / m / v non-temporal, p temporal (the
// updated weights stay in the Infinity Cache for the next GEMM that reads them; measured faster than all
// temporal or all non-temporal)
constexpr int ADAM_U = 1;

// Bulk of the arena: U 8-element chunks per thread, all 4*U loads issued before any math, one
// pass over the grid (no grid-stride loop).  U = 1 measured fastest (390 us for the 151 M-element
// config-2 arena = 5.4 TB/s; U = 2: 398 us; the grid-stride loop: 431 us).
// (LO: the lerp form, chosen by the launcher like adam_pipe_kernel's; bf16 only)
constexpr bool ADAM_PN = false, ADAM_SN = true;
// the bf16 form's workgroup `block`: packed, the fast arithmetic (adam_chunk_bf16).  BLOCK_COEF: the coefficient
// through adam_coef_block (4 bytes of LDS); false: read from a.coef by every thread (no clip_sums)
template <int U, bool LO, bool BLOCK_COEF = true>
CC_DEV void adam_bulk_bf16(const AdamArgs& a, int64_t nchunks, int64_t block) {
  constexpr bool PN = ADAM_PN, SN = ADAM_SN;
  const int64_t c0 = block * 256 * U + threadIdx.x;
  bf16x8 p[U], g[U], m[U], v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t c = c0 + u * 256;
    if (c < nchunks) {
      p[u] = ld_bf16x8<PN>(a.p, c * 8); g[u] = ld_bf16x8<SN>(a.g, c * 8); m[u] = ld_bf16x8<SN>(a.m, c * 8);
      v[u] = ld_bf16x8<SN>(a.v, c * 8);
    }
  }
  float coef;  // (placed as in adam_bulk_kernel's fp32 form)
  if constexpr (BLOCK_COEF) coef = adam_coef_block(a);
  else coef = a.coef ? *a.coef : 1.f;
  if (coef < 0.f) return;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t c = c0 + u * 256;
    if (c < nchunks) {
      adam_chunk_bf16<LO>(a, coef, c * 8, p[u], g[u], m[u], v[u]);
      st_bf16x8<PN>(a.p, c * 8, p[u]); st_bf16x8<SN>(a.m, c * 8, m[u]); st_bf16x8<SN>(a.v, c * 8, v[u]);
    }
  }
}

template <int DT, int U, bool LO>
__global__ __launch_bounds__(256) void adam_bulk_kernel(const AdamArgs a, int64_t nchunks) {
  const int64_t c0 = (int64_t)blockIdx.x * 256 * U + threadIdx.x;
  constexpr bool PN = ADAM_PN, SN = ADAM_SN;
  if constexpr (DT == CC_BF16) {
    adam_bulk_bf16<U, LO>(a, nchunks, blockIdx.x);
    return;
  }
  float p[U][8], g[U][8], m[U][8], v[U][8];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t c = c0 + u * 256;
    if (c < nchunks) {
      ld8<DT, PN>(a.p, c * 8, p[u]); ld8<DT, SN>(a.g, c * 8, g[u]); ld8<DT, SN>(a.m, c * 8, m[u]);
      ld8<DT, SN>(a.v, c * 8, v[u]);
    }
  }
  // the coefficient after the element loads are in flight (its inputs' latency hides under theirs; formed
  // from the squared sums it also stores clip_out, which must not hold the loads back)
  const float coef = adam_coef_block(a);
  if (coef < 0.f) return;  // CC_CLIP_ABORTED: the step's update is not applied
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t c = c0 + u * 256;
    if (c < nchunks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) adam_elem<DT>(a, coef, p[u][j], g[u][j], m[u][j], v[u][j]);
      st8<DT, PN>(a.p, c * 8, p[u]); st8<DT, SN>(a.m, c * 8, m[u]); st8<DT, SN>(a.v, c * 8, v[u]);
    }
  }
}

// The bf16 bulk Adam whose first workgroups run a cc_prep_input_t (the NEXT batch's x, x^T and column-sum partials:
// nothing the step computes feeds them, and their previous readers finished before this launch), so the step has no
// prep launch of its own: blocks [0, prep_blocks) are prep_block_narrow's grid, x fastest (they come first, so
// they finish under the Adam's stream of traffic), the others adam_bulk_kernel's.  Same bits as the two launches.
// The Adam's workgroups run 8 to a CU (one 8-element chunk per thread: its bandwidth is its occupancy), so the prep
// blocks are the narrow form: 60 VGPRs and 8 KB of LDS keep that occupancy.  (prep_kernel's own block in 8-row
// passes does too, but its 16-byte runs of x^T cost the step 45 us; with its 32-row passes -- 106 VGPRs, 32 KB --
// the launch measured the same as this form.)
// An aborted step (coef < 0) applies no update; the prep blocks run regardless (idempotent).
struct PrepJob {
  const void* x_in;
  const void* factor;
  void* x_out;
  float* colsum_part;
  void* x_t;
  int B, n, d;
  int gx, blocks;  // prep grid's x extent, and its workgroups
};
template <bool LO, int DIN, int DF>
__global__ __launch_bounds__(256) void adam_bulk_prep_kernel(const AdamArgs a, int64_t nchunks, const PrepJob j) {
  __shared__ __attribute__((aligned(16))) char lds[PREPN_LDS];
  if ((int)blockIdx.x < j.blocks) {  // block-uniform
    prep_block_narrow<DIN, DF>(lds, blockIdx.x % j.gx, blockIdx.x / j.gx, j.x_in, j.factor, j.x_out, j.colsum_part,
                               j.B, j.n, j.d, j.x_t);
    return;
  }
  adam_bulk_bf16<ADAM_U, LO, false>(a, nchunks, (int64_t)blockIdx.x - j.blocks);
}

template <int DT, bool LO>
__global__ __launch_bounds__(256) void adam_kernel(const AdamArgs a) {
  using E = Elem<DT>;
  // (per thread, once before the grid-stride loop: no LDS, so its workgroups still fit beside a GEMM
  // workgroup that holds a CU's whole LDS -- the decoder half runs beside G1)
  const float coef = adam_coef(a);
  const int64_t stride = (int64_t)gridDim.x * 256 * 8;
  // (CC_CLIP_ABORTED: the step's update is not applied -- p / m / v and the norm partials stay as they are --
  // but the done count still arrives)
  const int64_t numel = coef < 0.f ? 0 : a.numel;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  NormPos np = norm_pos(a, i0, stride);
  for (int64_t i = i0; i < numel; i += stride, norm_pos_next(np, a.norm_ld)) {
    const bool full = i + 8 <= a.numel;
    if constexpr (DT == CC_BF16) {
      if (full) {  // packed, the fast arithmetic (adam_chunk_bf16)
        bf16x8 p = ld_bf16x8<true>(a.p, i), g = ld_bf16x8<true>(a.g, i), m = ld_bf16x8<true>(a.m, i),
               v = ld_bf16x8<true>(a.v, i);
        norm_part_store(a, np, adam_chunk_bf16<LO>(a, coef, i, p, g, m, v));
        st_bf16x8<true>(a.p, i, p); st_bf16x8<true>(a.m, i, m); st_bf16x8<true>(a.v, i, v);
        continue;
      }
    }
    float p[8], g[8], m[8], v[8];
    if (full) {
      load8_nt<DT>(a.p, i, p); load8_nt<DT>(a.g, i, g); load8_nt<DT>(a.m, i, m); load8_nt<DT>(a.v, i, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int64_t k = i + j < a.numel ? i + j : a.numel - 1;
        p[j] = E::load((const typename E::T*)a.p + k);
        g[j] = E::load((const typename E::T*)a.g + k);
        m[j] = E::load((const typename E::T*)a.m + k);
        v[j] = E::load((const typename E::T*)a.v + k);
      }
    }
    // torch's CPU/GPU kernels: lerp is an fma (Lerp.h vectorised path), every other op is a
    // separately rounded fp32 multiply/add -> no contraction (adam_elem).
#pragma unroll
    for (int j = 0; j < 8; ++j) adam_elem<DT>(a, coef, p[j], g[j], m[j], v[j]);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) q = __fmaf_rn(p[j], p[j], q);
    norm_part_store(a, np, q);
    if (full) {
      store8_nt<DT>(a.p, i, p);
      store8_nt<DT>(a.m, i, m); store8_nt<DT>(a.v, i, v);
    } else {
      for (int j = 0; j < 8 && i + j < a.numel; ++j) {
        ((typename E::T*)a.p)[i + j] = E::from_f(p[j]);
        ((typename E::T*)a.m)[i + j] = E::from_f(m[j]);
        ((typename E::T*)a.v)[i + j] = E::from_f(v[j]);
      }
    }
  }
  if (a.done_ctr) adam_signal_done(a.done_ctr);
}

// The capped-grid (side-stream) bf16 Adam with the next chunk's loads in flight during this chunk's math.
// Beside G1 its workgroups get one wave per SIMD (G1 holds 2 x 216 of the 512 registers), so it streams
// only as fast as one wave's loads in flight allow: this form keeps two chunks' loads in flight in the same
// 64 registers, the data kept packed (8 bf16 per 16 B) and unpacked one element at a time.  Same per-element
// arithmetic (adam_elem) and norm partials as adam_kernel.  numel % 8 == 0.
CC_DEV void adam_pipe_load(const AdamArgs& a, int64_t i, bf16x8& p, bf16x8& g, bf16x8& m, bf16x8& v) {
  p = __builtin_nontemporal_load((const bf16x8*)((const bf16_t*)a.p + i));
  g = __builtin_nontemporal_load((const bf16x8*)((const bf16_t*)a.g + i));
  m = __builtin_nontemporal_load((const bf16x8*)((const bf16_t*)a.m + i));
  v = __builtin_nontemporal_load((const bf16x8*)((const bf16_t*)a.v + i));
}
// LO: the lerp weight 1 - beta1 is below 0.5 (chosen by the launcher: adam_chunk_bf16).
// amdgpu_waves_per_eu(6): at most 80 VGPRs (78 used), the room G1's 2 x 216 leave on a SIMD; without it the
// scheduler interleaves the four pairs of a chunk and takes 104.
template <bool LO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void adam_pipe_kernel(const AdamArgs a) {
  const float coef = adam_coef(a);
  const int64_t stride = (int64_t)gridDim.x * 256 * 8;
  const int64_t numel = coef < 0.f ? 0 : a.numel;  // (CC_CLIP_ABORTED: as adam_kernel)
  int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  NormPos np = norm_pos(a, i, stride);
  bf16x8 p, g, m, v;
  if (i < numel) adam_pipe_load(a, i, p, g, m, v);
  for (; i < numel; i += stride, norm_pos_next(np, a.norm_ld)) {
    const int64_t nx = i + stride;
    bf16x8 p2 = p, g2 = g, m2 = m, v2 = v;
    if (nx < numel) adam_pipe_load(a, nx, p2, g2, m2, v2);
    const float q = adam_chunk_bf16<LO>(a, coef, i, p, g, m, v);
    norm_part_store(a, np, q);  // (as adam_kernel)
    __builtin_nontemporal_store(p, (bf16x8*)((bf16_t*)a.p + i));
    __builtin_nontemporal_store(m, (bf16x8*)((bf16_t*)a.m + i));
    __builtin_nontemporal_store(v, (bf16x8*)((bf16_t*)a.v + i));
    p = p2; g = g2; m = m2; v = v2;
  }
  if (a.done_ctr) adam_signal_done(a.done_ctr);
}

// The master-weight Adam (cc_adam_master_step): a bf16 crosscoder trained with fp32 masters and fp32 moments.
// adam_elem<CC_F32> on g = float(g16) over p32 / m32 / v32 -- the bits of the fp32 cc_adam_step -- then p16 = p32
// rounded (f2bf) into the bf16 arena the GEMMs read.  8 elements per thread: 16 B of g16, 2 x 16 B each of p32 /
// m32 / v32, one 16-byte store of p16.  g / m / v / p32 are touched once per step: non-temporal, as
// adam_bulk_kernel streams them; p16 stays temporal, G1 / G2 read it next.  No LDS (the capped form runs beside
// G1, see adam_kernel).
CC_DEV void adam_master_load(const AdamArgs& a, int64_t i, float p[8], bf16x8& g, float m[8], float v[8]) {
  load8_nt<CC_F32>(a.p, i, p);
  g = __builtin_nontemporal_load((const bf16x8*)((const bf16_t*)a.g + i));
  load8_nt<CC_F32>(a.m, i, m);
  load8_nt<CC_F32>(a.v, i, v);
}
CC_DEV void adam_master_chunk(const AdamArgs& a, float coef, int64_t i, float p[8], const bf16x8& g, float m[8],
                              float v[8], bf16_t* p16) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    adam_elem<CC_F32>(a, coef, p[j], bf2f((bf16_t)g[j]), m[j], v[j]);
    r[j] = (short)f2bf(p[j]);
  }
  store8_nt<CC_F32>(a.p, i, p);
  store8_nt<CC_F32>(a.m, i, m);
  store8_nt<CC_F32>(a.v, i, v);
  *(bf16x8*)(p16 + i) = r;
}
// STRIDE: the capped grid-stride form (the side stream's); false: one chunk per thread, its loads issued before
// the coefficient arrives (as adam_bulk_kernel).  The last numel % 8 elements: one thread each of block 0.
// coef < 0 (CC_CLIP_ABORTED): nothing is stored.
template <bool STRIDE>
__global__ __launch_bounds__(256) void adam_master_kernel(const AdamArgs a, bf16_t* __restrict__ p16) {
  const int64_t nfull = a.numel & ~(int64_t)7;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  float p[8], m[8], v[8], coef;
  bf16x8 g;
  if constexpr (STRIDE) {
    coef = a.coef ? *a.coef : 1.f;
    if (coef < 0.f) return;
    const int64_t stride = (int64_t)gridDim.x * 256 * 8;
    for (int64_t i = i0; i < nfull; i += stride) {
      adam_master_load(a, i, p, g, m, v);
      adam_master_chunk(a, coef, i, p, g, m, v, p16);
    }
  } else {
    const bool in = i0 < nfull;
    if (in) adam_master_load(a, i0, p, g, m, v);
    coef = a.coef ? *a.coef : 1.f;
    if (coef < 0.f) return;
    if (in) adam_master_chunk(a, coef, i0, p, g, m, v, p16);
  }
  const int64_t k = nfull + threadIdx.x;
  if (blockIdx.x == 0 && k < a.numel) {
    float pk = ((const float*)a.p)[k], mk = ((const float*)a.m)[k], vk = ((const float*)a.v)[k];
    adam_elem<CC_F32>(a, coef, pk, bf2f(((const bf16_t*)a.g)[k]), mk, vk);
    ((float*)a.p)[k] = pk;
    ((float*)a.m)[k] = mk;
    ((float*)a.v)[k] = vk;
    p16[k] = f2bf(pk);
  }
}

// Decoder-half Adam over W_dec [h][K] (bf16) in 64 x 64 tiles that also emits what the next
// step needs from the updated W_dec: W_dec^T [K][h] (LDS tile read back with ds_read_b64_tr_b16)
// and the decoder norms' per-(row, 64-column block) squared sums in dec_norms_kernel's order
// (8 sequential fma per lane, xor-1/2/4 butterfly) -- one HBM pass instead of Adam + a
// transpose/norms pass.  Persistent grid over the tiles, rows fast; every element gets
// adam_chunk_bf16, so p / m / v are the bits cc_adam_step produces.
// (90 VGPRs -- 66 with adam_elem alone, before the fast arithmetic and its cold block shared the kernel: one
// half-tile's 4 x 8 elements per thread at a time; it still fits the 96 a 2-wave-per-SIMD ping-pong GEMM's 2 x 208
// leave.  adam_kernel<CC_BF16> is at 89 for the same reason; it runs with the whole chip.)
template <bool LO>
__global__ __launch_bounds__(256) void adam_dec_tr_kernel(const AdamArgs a, int h, int K, char* __restrict__ wt,
                                                          float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) char tile[64 * 128];
  const float coef = adam_coef(a);
  if (coef < 0.f) return;  // CC_CLIP_ABORTED: the step's update is not applied
  const int nr = (h + 63) / 64, nblk = K / 64, ntiles = nr * nblk;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g4 = lane >> 4, i = lane & 15, q4 = i >> 2, p4 = i & 3;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int r0 = (t % nr) * 64, c0 = (t / nr) * 64;
#pragma unroll 1
    for (int k = 0; k < 2; ++k) {
      const int idx = threadIdx.x + 256 * k, r = idx >> 3, ch = idx & 7;
      float qs = 0.f;
      if (r0 + r < h) {
        const int64_t e = (int64_t)(r0 + r) * K + c0 + 8 * ch;
        bf16x8 b = ld_bf16x8<true>(a.p, e), g = ld_bf16x8<true>(a.g, e), m = ld_bf16x8<true>(a.m, e),
               v = ld_bf16x8<true>(a.v, e);
        qs = adam_chunk_bf16<LO>(a, coef, e, b, g, m, v);
        st_bf16x8<true>(a.p, e, b); st_bf16x8<true>(a.m, e, m); st_bf16x8<true>(a.v, e, v);
        *(bf16x8*)(tile + r * 128 + ((ch ^ (r & 7)) << 4)) = b;
      }
      qs = block8_sum(qs);
      if (ch == 0 && r0 + r < h) part[(int64_t)(r0 + r) * nblk + (c0 >> 6)] = qs;
    }
    __syncthreads();
    const int ca = 16 * w + 4 * p4, cch = ca >> 3, c = 16 * w + i;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int R = (4 * s2 + g4) * 8, l0 = R + q4, l1 = R + 4 + q4;
      const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4_s*)(tile + l0 * 128 + ((cch ^ (l0 & 7)) << 4) + (ca & 4) * 2));
      const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4_s*)(tile + l1 * 128 + ((cch ^ (l1 & 7)) << 4) + (ca & 4) * 2));
      if (r0 + R < h)
        *(bf16x8*)(wt + ((int64_t)(c0 + c) * h + r0 + R) * 2) =
            bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    }
    __syncthreads();
  }
}

}  // namespace cc

using namespace cc;

// the bf16 Adam kernels' lerp form (adam_pair): LO_ = the weight 1 - beta1 is below 0.5
#define ADAM_LO(args, KERNEL_CALL)                                              \
  do {                                                                          \
    if ((args).w1 < 0.5f) { constexpr bool LO_ = true; KERNEL_CALL; }           \
    else { constexpr bool LO_ = false; KERNEL_CALL; }                           \
  } while (0)

// The test-only debug build (-DCC_DEBUG_HOOKS, libcrosscoder_hip_dbg.so): every bf16 Adam entry on the reference
// arithmetic (adam_elem) on request, and the fast primitives against their references over whole domains.
#ifdef CC_DEBUG_HOOKS
#include <vector>
#define CC_DEBUG_API extern "C" __attribute__((visibility("default")))
static int g_adam_ref = 0;
CC_DEBUG_API void cc_debug_set_adam_ref(int on) { g_adam_ref = on; }
// The number of 8-element chunks the bf16 Adam launches redid with adam_elem since the last reset (synchronises
// the device; -1: a HIP error).  A test that compares the fast arithmetic with the reference reads it to know that
// the fast path produced the compared bits.
static unsigned long long* g_redo_ctr = nullptr;
static unsigned long long* debug_redo_ctr() {
  if (!g_redo_ctr && (hipMalloc((void**)&g_redo_ctr, 8) != hipSuccess || hipMemset(g_redo_ctr, 0, 8) != hipSuccess))
    g_redo_ctr = nullptr;
  return g_redo_ctr;
}
CC_DEBUG_API int64_t cc_debug_adam_redone(int reset) {
  unsigned long long n = 0;
  unsigned long long* ctr = debug_redo_ctr();
  if (!ctr || hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&n, ctr, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (reset && hipMemset(ctr, 0, 8) != hipSuccess) return -1;
  return (int64_t)n;
}

// out: [0] mismatches, [1] operands sent to the reference by the guard, [2] the smallest mismatching operand key
// (atomic min; ~0: none), [3] kind 1: mismatches before the bf16 rounding; kind 2: guarded pairs whose members
// are all normal or zero with den > 0 (none: adam_quot's guard is on the operands' classes alone)
struct PrimArgs {
  int kind;
  const float* div;  // kind 1: [gridDim.y][2] = (bc2s, rb)
  unsigned long long* out;
};
CC_DEV bool same_bits(float x, float y) { return __float_as_uint(x) == __float_as_uint(y) || (x != x && y != y); }
__global__ __launch_bounds__(256) void adam_prims_kernel(const PrimArgs a) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  unsigned long long bad = 0, guarded = 0, aux = 0, first = ~0ull;
  if (a.kind == 0) {  // sqrt then the bf16 round: idx = vj's bf16 pattern (the pair's other slot: idx ^ 0x5a5a)
    const float v0 = bf2f((bf16_t)idx), v1 = bf2f((bf16_t)(idx ^ 0x5a5a));
    float s0, s1;
    bool ok0, ok1;
    adam_sqrt2(v0, v1, s0, s1, ok0, ok1);
    guarded = !ok0;  // (every pattern is slot 0 of one thread)
    if ((ok0 && !same_bits(s0, Elem<CC_BF16>::round(sqrtf(v0)))) ||
        (ok1 && !same_bits(s1, Elem<CC_BF16>::round(sqrtf(v1))))) {
      bad = 1;
      first = idx;
    }
  } else if (a.kind == 1) {  // den / bc2s then the bf16 round: idx = den's pattern, blockIdx.y = divisor
    const float den = bf2f((bf16_t)idx);
    const float bc2s = uniform(a.div[2 * blockIdx.y]), rb = uniform(a.div[2 * blockIdx.y + 1]);
    // adam_udiv's domain: what R(sqrt(vj)) can be for a vj that passed adam_sqrt2's guard (+0, or 2^-63 .. 2^64),
    // with the margin its proof allows below
    const bool ok = den == 0.f ? fp_class<FPC_POS_ZERO>(den) : den >= 0x1p-67f && den <= 0x1p64f;
    const float fast = adam_udiv(den, bc2s, rb), ref = den / bc2s;
    guarded = !ok;
    if (ok && !same_bits(fast, ref)) aux = 1;
    if (ok && !same_bits(Elem<CC_BF16>::round(fast), Elem<CC_BF16>::round(ref))) {
      bad = 1;
      first = ((unsigned long long)blockIdx.y << 16) | idx;
    }
  } else {  // mj / den: idx = (den pattern << 12) | (mj pattern >> 4), 16 mj patterns per thread, two at a time
    const float den = bf2f((bf16_t)(idx >> 12));
    for (uint32_t j = 0; j < 16; j += 2) {
      const uint32_t mb = ((idx & 0xfffu) << 4) | j;
      const float m[2] = {bf2f((bf16_t)mb), bf2f((bf16_t)(mb + 1))};
      float fast[2];
      bool ok[2];
      adam_quot2(m[0], m[1], den, den, fast[0], fast[1], ok[0], ok[1]);
      for (int t = 0; t < 2; ++t) {
        const bool cls = fp_class<FPC_POS_NORMAL>(den) &&
                         fp_class<FPC_NEG_NORMAL | FPC_NEG_ZERO | FPC_POS_ZERO | FPC_POS_NORMAL>(m[t]);
        const bool in = cls && ok[t];  // (the update's den is never a denormal: adam_args' eps check)
        guarded += !in;
        aux += cls && !in;
        if (in && !same_bits(fast[t], m[t] / den)) {
          ++bad;
          const unsigned long long key = ((unsigned long long)(idx >> 12) << 16) | (mb + t);
          first = key < first ? key : first;
        }
      }
    }
  }
  // one atomic per wave and counter
  for (int o = 32; o > 0; o >>= 1) {
    bad += __shfl_xor(bad, o, 64);
    guarded += __shfl_xor(guarded, o, 64);
    aux += __shfl_xor(aux, o, 64);
    const unsigned long long f2 = __shfl_xor(first, o, 64);
    first = f2 < first ? f2 : first;
  }
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(a.out, bad);
    if (guarded) atomicAdd(a.out + 1, guarded);
    if (first != ~0ull) atomicMin(a.out + 2, first);
    if (aux) atomicAdd(a.out + 3, aux);
  }
}
// kind 0: sqrt over the 2^16 bf16 patterns; 1: the uniform divide over 2^16 patterns x the divisors of steps
// [step_lo, step_hi] at beta2 (as adam_args forms them); 2: the quotient over 2^16 x 2^16 pairs.  Synchronous;
// host_out[4] as PrimArgs::out.
CC_DEBUG_API int cc_debug_adam_prims(int kind, double beta2, int64_t step_lo, int64_t step_hi, uint64_t* host_out,
                                     void* stream) {
  if (!host_out) return CC_ERR_NULL;
  if (kind < 0 || kind > 2) return CC_ERR_SHAPE;
  if (kind == 1 && (step_lo <= 0 || step_hi < step_lo || step_hi - step_lo >= 65535)) return CC_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t ndiv = kind == 1 ? step_hi - step_lo + 1 : 0;
  char* buf = nullptr;
  hipError_t e = hipMalloc((void**)&buf, 32 + (size_t)ndiv * 8);
  if (e != hipSuccess) return CC_ERR_HIP_BASE + (int)e;
  const unsigned long long init[4] = {0, 0, ~0ull, 0};
  std::vector<float> div((size_t)ndiv * 2);
  for (int64_t s = 0; s < ndiv; ++s) {
    div[2 * s] = (float)sqrt(1.0 - pow(beta2, (double)(step_lo + s)));
    div[2 * s + 1] = (float)(1.0 / (double)div[2 * s]);
  }
  e = hipMemcpyAsync(buf, init, 32, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && ndiv) e = hipMemcpyAsync(buf + 32, div.data(), (size_t)ndiv * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const PrimArgs a = {kind, (const float*)(buf + 32), (unsigned long long*)buf};
    const dim3 grid(kind == 2 ? 1u << 20 : 256u, kind == 1 ? (unsigned)ndiv : 1u);
    hipLaunchKernelGGL(adam_prims_kernel, grid, dim3(256), 0, st, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, buf, 32, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  (void)hipFree(buf);
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? CC_OK : CC_ERR_HIP_BASE + (int)e;
}
#else
constexpr int g_adam_ref = 0;
#endif

static AdamArgs adam_args(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, double lr,
                          double beta1, double beta2, double eps, int64_t step) {
  AdamArgs a = {};
  a.p = p; a.g = g; a.m = m; a.v = v; a.numel = numel; a.coef = coef;
  // host-side scalars in double, as torch computes them from python floats (adam.py)
  double b1 = beta1, b2 = beta2;
  a.w1 = (float)(1.0 - b1);
  a.beta2 = beta2;
  a.omb2 = (float)(1.0 - b2);
  a.eps = eps;
  double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
  a.bc2s = (float)sqrt(bc2);
  a.rb = (float)(1.0 / (double)a.bc2s);
  a.neg_step = (float)(-((double)lr / bc1));
  // the domain of adam_udiv's divisor and of the sum den + eps (eps: +0 or a positive normal, so that the sum is
  // no denormal); anything else runs adam_elem
  a.fast = a.bc2s >= 0x1p-20f && a.bc2s <= 1.f && (a.eps == 0.f || (a.eps >= FLT_MIN && a.eps <= FLT_MAX)) &&
           !std::signbit(a.eps) && !g_adam_ref;
#ifdef CC_DEBUG_HOOKS
  a.redo_ctr = debug_redo_ctr();
#endif
  return a;
}
// the coefficient formed in the kernel from the per-parameter squared sums (AdamArgs::clip_sums; at most 6, which
// the entry points check), instead of read from coef
static void set_kernel_clip(AdamArgs& a, const float* sums, int nparams, float max_norm, int emulate_bf16,
                            float* clip_out) {
  a.clip_sums = sums;
  a.clip_np = nparams;
  a.clip_emulate = emulate_bf16;
  a.clip_max_norm = max_norm;
  a.clip_out = clip_out;
}
// workgroups of 256 threads, U 8-element chunks per thread, that cover nchunks
static int64_t adam_blocks(int64_t nchunks, int U = 1) { return (nchunks + 256 * U - 1) / (256 * U); }
// workgroups of the capped grid-stride forms (adam_launch's and cc_adam_master_step's)
static int64_t adam_capped_blocks(int64_t numel, int64_t max_blocks) {
  const int64_t blocks = adam_blocks((numel + 7) / 8);
  return blocks > max_blocks ? max_blocks : blocks;
}
static int adam_launch(const AdamArgs& a, int64_t max_blocks, int dtype, hipStream_t st) {
  const int64_t numel = a.numel;
  if (max_blocks > 0) {  // capped grid-stride form: leaves most CUs to a concurrent GEMM
    const int64_t blocks = adam_capped_blocks(numel, max_blocks);
    if (dtype == CC_BF16 && numel % 8 == 0) {
      ADAM_LO(a, hipLaunchKernelGGL(adam_pipe_kernel<LO_>, dim3((unsigned)blocks), dim3(256), 0, st, a));
      CC_LAUNCH_CHECK();
      return CC_OK;
    }
    ADAM_LO(a, DISPATCH_DT(dtype, hipLaunchKernelGGL((adam_kernel<DT_, DT_ != CC_BF16 || LO_>), dim3((unsigned)blocks),
                                                     dim3(256), 0, st, a)));
    CC_LAUNCH_CHECK();
    return CC_OK;
  }
  const int64_t nchunks = numel / 8;
  if (nchunks > 0) {
    const int64_t blocks = adam_blocks(nchunks, ADAM_U);
    ADAM_LO(a, DISPATCH_DT(dtype, hipLaunchKernelGGL((adam_bulk_kernel<DT_, ADAM_U, DT_ != CC_BF16 || LO_>),
                                                     dim3((unsigned)blocks), dim3(256), 0, st, a, nchunks)));
    CC_LAUNCH_CHECK();
  }
  if (numel % 8) {  // the last < 8 elements
    const int es = dtype == CC_BF16 ? 2 : 4;
    const int64_t off = nchunks * 8 * es;
    AdamArgs t = a;
    t.p = (char*)a.p + off; t.g = (const char*)a.g + off; t.m = (char*)a.m + off; t.v = (char*)a.v + off;
    t.numel = numel % 8;
    ADAM_LO(t, DISPATCH_DT(dtype, hipLaunchKernelGGL((adam_kernel<DT_, DT_ != CC_BF16 || LO_>), dim3(1), dim3(256), 0,
                                                     st, t)));
    CC_LAUNCH_CHECK();
  }
  return CC_OK;
}

extern "C" {

int cc_adam_step(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, double lr, double beta1,
                 double beta2, double eps, int64_t step, int64_t max_blocks, int dtype, void* stream) {
  if (!p || !g || !m || !v) return CC_ERR_NULL;
  if (numel <= 0 || step <= 0) return CC_ERR_SHAPE;
  if (!al16(p) || !al16(g) || !al16(m) || !al16(v)) return CC_ERR_ALIGN;
  return adam_launch(adam_args(p, g, m, v, numel, coef, lr, beta1, beta2, eps, step), max_blocks, dtype,
                     (hipStream_t)stream);
}

int cc_adam_step_clip(void* p, const void* g, void* m, void* v, int64_t numel, const float* sums, int nparams,
                      float max_norm, int emulate_bf16, float* clip_out, double lr, double beta1, double beta2,
                      double eps, int64_t step, int64_t max_blocks, int dtype, void* stream) {
  if (!p || !g || !m || !v || !sums) return CC_ERR_NULL;
  if (numel <= 0 || step <= 0 || nparams <= 0 || nparams > 6) return CC_ERR_SHAPE;
  if (!al16(p) || !al16(g) || !al16(m) || !al16(v)) return CC_ERR_ALIGN;
  AdamArgs a = adam_args(p, g, m, v, numel, nullptr, lr, beta1, beta2, eps, step);
  set_kernel_clip(a, sums, nparams, max_norm, emulate_bf16, clip_out);
  return adam_launch(a, max_blocks, dtype, (hipStream_t)stream);
}

int cc_adam_step_prep(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, double lr,
                      double beta1, double beta2, double eps, int64_t step, int dtype, const cc_prep_job* prep,
                      void* stream) {
  if (!prep)
    return cc_adam_step(p, g, m, v, numel, coef, lr, beta1, beta2, eps, step, 0, dtype, stream);
  if (!p || !g || !m || !v) return CC_ERR_NULL;
  if (dtype != CC_BF16) return CC_ERR_DTYPE;
  if (numel <= 0 || numel % 8 || step <= 0) return CC_ERR_SHAPE;
  if (!al16(p) || !al16(g) || !al16(m) || !al16(v)) return CC_ERR_ALIGN;
  const int64_t B = prep->B, n = prep->n, d = prep->d;
  if (const int rc = check_prep(prep->x_in, prep->in_dtype, prep->factor, prep->factor_dtype, prep->x_out, prep->x_t,
                                true, B, n, d, CC_BF16))
    return rc;
  const AdamArgs a = adam_args(p, g, m, v, numel, coef, lr, beta1, beta2, eps, step);
  const int64_t nchunks = numel / 8;
  const int64_t gx = (n * d + PREPN_COLS - 1) / PREPN_COLS, pblocks = gx * cc_prep_part_rows(B);
  const int64_t blocks = pblocks + adam_blocks(nchunks, ADAM_U);
  if (blocks > INT32_MAX) return CC_ERR_SHAPE;
  const PrepJob j = {prep->x_in, prep->factor, prep->x_out, prep->colsum_part, prep->x_t,
                     (int)B,     (int)n,       (int)d,      (int)gx,           (int)pblocks};
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_PREP(prep->in_dtype, prep->factor && prep->factor_dtype == CC_BF16,
                ADAM_LO(a, hipLaunchKernelGGL((adam_bulk_prep_kernel<LO_, DI_, DF_>), dim3((unsigned)blocks), dim3(256),
                                              0, st, a, nchunks, j)));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_adam_master_step(void* p32, const void* g16, void* m32, void* v32, void* p16, int64_t numel, const float* coef,
                        double lr, double beta1, double beta2, double eps, int64_t step, int64_t max_blocks,
                        void* stream) {
  if (!p32 || !g16 || !m32 || !v32 || !p16) return CC_ERR_NULL;
  if (numel <= 0 || step <= 0) return CC_ERR_SHAPE;
  if (!al16(p32) || !al16(g16) || !al16(m32) || !al16(v32) || !al16(p16)) return CC_ERR_ALIGN;
  const AdamArgs a = adam_args(p32, g16, m32, v32, numel, coef, lr, beta1, beta2, eps, step);
  hipStream_t st = (hipStream_t)stream;
  // (capped: the grid-stride form, which leaves most CUs to a concurrent GEMM; else one chunk per thread)
  const int64_t blocks = max_blocks > 0 ? adam_capped_blocks(numel, max_blocks) : adam_blocks((numel + 7) / 8);
  if (blocks > INT32_MAX) return CC_ERR_SHAPE;
  if (max_blocks > 0)
    hipLaunchKernelGGL(adam_master_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a, (bf16_t*)p16);
  else
    hipLaunchKernelGGL(adam_master_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a, (bf16_t*)p16);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_adam_dec_norms(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, const float* sums,
                      int nparams, float max_norm, int emulate_bf16, double lr, double beta1, double beta2,
                      double eps, int64_t step, int64_t max_blocks, float* norm_part, int64_t h, int64_t K, int dtype,
                      uint32_t* done_ctr, void* stream) {
  if (!p || !g || !m || !v || !norm_part || (!coef && !sums)) return CC_ERR_NULL;
  if (done_ctr && max_blocks <= 0) return CC_ERR_SHAPE;  // (the signal is the capped grid-stride forms')
  if (numel <= 0 || step <= 0 || h <= 0 || K <= 0 || K % 64 || h * K > numel || h * K >= ((int64_t)1 << 31))
    return CC_ERR_SHAPE;
  if (sums && (nparams <= 0 || nparams > 6)) return CC_ERR_SHAPE;
  if (!al16(p) || !al16(g) || !al16(m) || !al16(v) || !al16(norm_part)) return CC_ERR_ALIGN;
  AdamArgs a = adam_args(p, g, m, v, numel, sums ? nullptr : coef, lr, beta1, beta2, eps, step);
  if (sums) set_kernel_clip(a, sums, nparams, max_norm, emulate_bf16, nullptr);
  a.norm_part = norm_part;
  a.norm_rows = (int)h;
  a.norm_ld = (int)K;
  a.done_ctr = done_ctr;
  // (the grid-stride form: the bulk kernel does not form the partials)
  return adam_launch(a, max_blocks > 0 ? max_blocks : 1024, dtype, (hipStream_t)stream);
}

int cc_adam_dec_transposed(void* p, const void* g, void* m, void* v, int64_t h, int64_t K, const float* coef,
                           double lr, double beta1, double beta2, double eps, int64_t step, int64_t max_blocks,
                           void* W_dec_t, float* part, int dtype, void* stream) {
  if (!p || !g || !m || !v || !W_dec_t || !part) return CC_ERR_NULL;
  if (dtype != CC_BF16) return CC_ERR_DTYPE;
  if (h <= 0 || K <= 0 || h % 8 || K % 64 || step <= 0 || h > (1 << 30)) return CC_ERR_SHAPE;
  if (!al16(p) || !al16(g) || !al16(m) || !al16(v) || !al16(W_dec_t)) return CC_ERR_ALIGN;
  const AdamArgs a = adam_args(p, g, m, v, h * K, coef, lr, beta1, beta2, eps, step);
  const int64_t ntiles = ((h + 63) / 64) * (K / 64);
  const int64_t blocks = max_blocks > 0 && max_blocks < ntiles ? max_blocks : ntiles;
  ADAM_LO(a, hipLaunchKernelGGL(adam_dec_tr_kernel<LO_>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a,
                                (int)h, (int)K, (char*)W_dec_t, part));
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int64_t cc_adam_capped_blocks(int64_t numel, int64_t max_blocks) {
  return numel > 0 && max_blocks > 0 ? adam_capped_blocks(numel, max_blocks) : 0;
}

}  // extern "C"
