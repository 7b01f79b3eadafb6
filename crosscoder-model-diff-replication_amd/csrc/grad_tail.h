// Gradient-tail building blocks shared by the stand-alone tail kernels (step_kernels.hip) and the
// weight-gradient GEMM that runs the grad tail in its own launch (gemm.hip): fixed-order column
// reductions of partial slabs and the clip_grad_norm_ finaliser (device side); the tail's kernel
// arguments TailArgs, the one host builder that checks and fills them for every launch form
// (make_grad_tail_args, as make_loss_tail_args for the loss tail) and the stand-alone launcher's
// declaration (host side).  The Adam kernels that form the clip coefficient themselves (adam.hip: adam_coef) take
// clip_param_norm and clip_coef from here.  Included inside namespace cc.
#pragma once

// ---------------------------------------------------------------------------------------
// out[j] = scale * sum_i part[i*ld + j]; optional dtype copy, squared-sum partial per block and
// dot partial per block (sum_j out[j] * dot_w[j]: the L1 loss from the activation column sums).
// Block = 64 columns x 4 waves; wave w sums rows w, w+4, ... (independent loads in flight),
// then a fixed-order combine of the 4 wave partials.  One sq / dot partial per block.
constexpr int RED_COLS = 64;
// Phase 1 (all 4 waves of a 256-thread group, t = thread in the group): column sums into red;
// phase 2 (after a barrier, wave 0 of the group): outputs + the group's sq / dot partial.  The
// stand-alone kernel and the fused tail kernels (grad_tail / loss_tail) run the same two phases.
struct RedSeg {
  const float* part;
  int R, C;
  int64_t ld;
  float scale;
  float* out_f32;
  void* out_t;
  float* sq_part;
  const float* dot_w;
  float* dot_part;
};
CC_DEV void reduce_rows_phase1(const RedSeg& a, int blk, int t, float (*red)[RED_COLS]) {
  const int lane = t & 63, wave = t >> 6;
  const int j = blk * RED_COLS + lane;
  float s = 0.f;
  if (j < a.C) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int i = wave;
    for (; i + 12 < a.R; i += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] += a.part[(int64_t)(i + 4 * u) * a.ld + j];
    }
    for (; i < a.R; i += 4) v[0] += a.part[(int64_t)i * a.ld + j];
    s = (v[0] + v[1]) + (v[2] + v[3]);
  }
  red[wave][lane] = s;
}
template <int DT>
CC_DEV void reduce_rows_phase2(const RedSeg& a, int blk, int t, float (*red)[RED_COLS]) {
  if ((t >> 6) != 0) return;
  const int lane = t & 63;
  const int j = blk * RED_COLS + lane;
  float sq = 0.f, dot = 0.f;
  if (j < a.C) {
    float s = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * a.scale;
    if (a.out_f32) a.out_f32[j] = s;
    if (a.out_t) {
      typename Elem<DT>::T q = Elem<DT>::from_f(s);
      ((typename Elem<DT>::T*)a.out_t)[j] = q;
      float vq = Elem<DT>::to_f(q);
      sq = vq * vq;
    }
    if (a.dot_part) dot = s * a.dot_w[j];
  }
  if (a.sq_part) {
    sq = wave_sum(sq);
    if (lane == 0) a.sq_part[blk] = sq;
  }
  if (a.dot_part) {
    dot = wave_sum(dot);
    if (lane == 0) a.dot_part[blk] = dot;
  }
}
CC_DEV float bf16r(float f) { return bf2f(f2bf(f)); }

// clip_grad_norm_'s scalar arithmetic (torch/nn/utils/clip_grad.py): a parameter's norm from its squared sum
// (bf16-rounded as torch._foreach_norm on bf16 returns bf16), then the total norm and the coefficient.
// emulate_bf16 = 2 (CLIP_EMULATE_MIXED): torch on four bf16 gradients followed by fp32 ones -- the norms of the first
// four are bf16, the stack promotes to fp32, and the total and the coefficient stay fp32
constexpr int CLIP_EMULATE_MIXED = 2;
CC_DEV float clip_param_norm(double sq, int emulate_bf16, int p = 0) {
  const float nr = (float)sqrt(sq);
  return emulate_bf16 == CLIP_EMULATE_MIXED ? (p < 4 ? bf16r(nr) : nr) : emulate_bf16 ? bf16r(nr) : nr;
}
CC_DEV float clip_coef(const float* norms, int nparams, float max_norm, int emulate_bf16, float& total) {
  float s = 0.f;
  // (the mixed list: torch groups the gradients by dtype and stacks the groups' norms with the fp32 group first --
  // the order its device-and-dtype grouping yields for that list -- so the fp32 sum of squares runs in that order)
  if (emulate_bf16 == CLIP_EMULATE_MIXED)
    for (int p = 4; p < nparams; ++p) s += norms[p] * norms[p];
  for (int p = 0; p < (emulate_bf16 == CLIP_EMULATE_MIXED && nparams > 4 ? 4 : nparams); ++p) s += norms[p] * norms[p];
  total = sqrtf(s);
  if (emulate_bf16 && emulate_bf16 != CLIP_EMULATE_MIXED) {
    total = bf16r(total);                       // vector_norm(stack(bf16 norms)) -> bf16
    const float den = bf16r(total + 1e-6f);     // bf16 tensor + python scalar
    return fminf(bf16r(max_norm / den), 1.f);
  }
  return fminf(max_norm / (total + 1e-6f), 1.f);
}

struct ClipArgs {
  const float* sq;
  int64_t off[9];
  int nparams;
  float max_norm;
  int emulate_bf16;
  float* out;
  int sums_only;   // cc_segment_sums: out[p] = the raw per-parameter sum (0 where zero_mask has bit p)
  int zero_mask;
  // the step's abort word (a host-mapped word an earlier launch of the step sets when it could not run, e.g. G2's
  // in-kernel wait timing out): when set, the coefficient is written as CC_CLIP_ABORTED and every Adam launch
  // that reads it leaves p / m / v untouched (nullptr: none)
  const unsigned* abort;
};
// clip_out[0] of a step that must not update the parameters: clip_grad_norm_'s coefficient min(1, max_norm /
// (total + 1e-6)) is never negative (NaN / inf norms give NaN / 0), so a negative value is free to mean it
#define CC_CLIP_ABORTED (-1.0f)
// One block of NT threads; red / norms: LDS scratch of the caller (the GEMM kernel that runs it as
// its last workgroup's tail has no LDS to spare for static arrays of its own)
template <int NT>
CC_DEV void clip_finish(const ClipArgs& a, const double* s, double (*red)[NT / 64], float* norms);
template <int NT>
CC_DEV void clip_body(const ClipArgs& a, double (*red)[NT / 64], float* norms) {
  // all parameters in one pass: each thread keeps one running sum per parameter
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    if (p < a.nparams) {
      const int64_t lo = a.off[p], hi = a.off[p + 1];
      // 4 independent loads in flight per trip (clamped index, no branch around a load)
      for (int64_t i = lo + threadIdx.x; i < hi; i += 4 * NT) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t j = i + u * NT;
          v[u] = j < hi ? a.sq[j < hi ? j : lo] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s[p] += (double)v[u];
      }
    }
  }
  clip_finish<NT>(a, s, red, norms);
}

// The finaliser from per-thread partial sums s[p] (every thread of the block): fixed-order combine of
// the waves, per-parameter norms (bf16-rounded as torch's _foreach_norm on bf16), total, coefficient.
template <int NT>
CC_DEV void clip_finish(const ClipArgs& a, const double* s, double (*red)[NT / 64], float* norms) {
  // (the abort word may live in host memory: its load is issued first, its latency hides under the reductions)
  const unsigned aborted =
      threadIdx.x == 0 && a.abort ? __hip_atomic_load(a.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    double t = wave_sum_d(s[p]);
    if ((threadIdx.x & 63) == 0) red[p][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if (a.sums_only) {
    if (threadIdx.x < a.nparams) {
      const int p = threadIdx.x;
      // (the step was aborted -- G2's in-kernel wait timed out, ClipArgs::abort: -inf for every parameter, so the
      // sums' all-reduce carries the abort to every rank and each Adam launch that forms its coefficient from them
      // applies nothing, adam.hip's adam_coef.  Each of these threads reads the word itself.)
      const bool ab = a.abort && __hip_atomic_load(a.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
      double t = 0.0;
      for (int w = 0; w < NT / 64; ++w) t += red[p][w];
      a.out[p] = ab ? -__builtin_inff() : ((a.zero_mask >> p) & 1 ? 0.f : (float)t);
    }
    return;
  }
  if (threadIdx.x < a.nparams) {
    const int p = threadIdx.x;
    double t = 0.0;
    for (int w = 0; w < NT / 64; ++w) t += red[p][w];
    norms[p] = clip_param_norm(t, a.emulate_bf16, p);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total;
    const float coef = clip_coef(norms, a.nparams, a.max_norm, a.emulate_bf16, total);
    a.out[0] = aborted ? CC_CLIP_ABORTED : coef;
    a.out[1] = total;
    for (int p = 0; p < a.nparams; ++p) a.out[2 + p] = norms[p];
  }
}

// ---------------------------------------------------------------------------------------
// The grad tail's kernel arguments: two column reductions (RedSeg: b_enc.grad, b_dec.grad column sums + their sq
// partials) in 256-thread groups, then the last workgroup to arrive (counter) runs the clip finaliser or the segment
// sums over the partials the whole grid wrote.  tail_kernel (step_kernels.hip) takes them as they are; the G4G5
// launch that carries the tail appends its own words (gemm.hip WgradTail).
struct TailArgs {
  RedSeg red[2];
  int red_blocks[2];  // 256-thread groups per reduction (0: unused)
  ClipArgs clip;
  unsigned* counter;
};

// What a caller hands the grad tail, whichever launch runs it (cc_grad_tail, cc_grad_tail_sums, the fused G4G5
// entries and their fallback): the two slabs with their bias gradients and sq partials, the squared-sum segments sq /
// off / nparams, and either the clip's scalars or sums_only + zero_mask (ClipArgs).  abort: the step's abort word
// (ClipArgs::abort; nullptr: none).
struct GradTailIn {
  const float* gpre_colpart;  // [R_enc][h] -> g_b_enc, sq_b_enc
  int64_t R_enc, h;
  void* g_b_enc;
  float* sq_b_enc;
  const float* loss_colpart;  // [R_dec][K] -> g_b_dec, sq_b_dec
  int64_t R_dec, K;
  void* g_b_dec;
  float* sq_b_dec;
  const float* sq;
  const int64_t* off;
  int nparams;
  float max_norm;
  int emulate_bf16;
  int sums_only, zero_mask;
  float* out;
  uint32_t* counter;
  const uint32_t* abort;
};
// The squared-sum segments sq / off / nparams and the output of a ClipArgs, checked (NULL, then nparams) and filled;
// everything else zero.  Every launch that runs clip_body starts from it: cc_clip_finalize, cc_segment_sums and the
// grad tail.
static inline int make_clip_args(ClipArgs& a, const float* sq, const int64_t* off, int nparams, float* out) {
  if (!sq || !off || !out) return CC_ERR_NULL;
  if (nparams <= 0 || nparams > 8) return CC_ERR_SHAPE;
  a = ClipArgs{};
  a.sq = sq;
  for (int i = 0; i <= nparams; ++i) a.off[i] = off[i];
  a.nparams = nparams;
  a.out = out;
  return CC_OK;
}
// The only copy of the tail's argument checks (NULL, then the shapes, then nparams) and of the field fill.
static inline int make_grad_tail_args(TailArgs& a, const GradTailIn& in) {
  // (the clip's pointers too: a NULL one is reported before a wrong shape)
  if (!in.gpre_colpart || !in.g_b_enc || !in.sq_b_enc || !in.loss_colpart || !in.g_b_dec || !in.sq_b_dec || !in.sq ||
      !in.off || !in.out || !in.counter)
    return CC_ERR_NULL;
  if (in.R_enc <= 0 || in.R_dec <= 0 || in.h <= 0 || in.K <= 0) return CC_ERR_SHAPE;
  a = TailArgs{};
  if (const int rc = make_clip_args(a.clip, in.sq, in.off, in.nparams, in.out)) return rc;
  a.red[0] = {in.gpre_colpart, (int)in.R_enc, (int)in.h, in.h, 1.f, nullptr, in.g_b_enc, in.sq_b_enc, nullptr, nullptr};
  a.red[1] = {in.loss_colpart, (int)in.R_dec, (int)in.K, in.K, 1.f, nullptr, in.g_b_dec, in.sq_b_dec, nullptr, nullptr};
  a.red_blocks[0] = (int)((in.h + RED_COLS - 1) / RED_COLS);
  a.red_blocks[1] = (int)((in.K + RED_COLS - 1) / RED_COLS);
  a.clip.max_norm = in.max_norm;
  a.clip.emulate_bf16 = in.emulate_bf16;
  a.clip.sums_only = in.sums_only;
  a.clip.zero_mask = in.zero_mask;
  a.clip.abort = in.abort;
  a.counter = in.counter;
  return CC_OK;
}
// The stand-alone launch of tail_kernel<dtype> (step_kernels.hip; library-internal)
int launch_grad_tail(const TailArgs& a, int dtype, hipStream_t stream);
