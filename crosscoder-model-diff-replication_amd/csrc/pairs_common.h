// Shared helpers of the pair kernels (decode_pairs.hip, pairs_grad.hip, sparse_step.hip): the device pieces that fix
// their numerical contract, their limits, and the argument checks of their entry points.  gfx950.
//
// The three rules every pair kernel keeps; each is written once, here:
//   range check   a slot (value, latent) is valid iff (uint32_t)idx < h: one compare takes negative padding and
//                 anything >= h.  An invalid slot reads nothing and adds nothing.  (A list entry: iff
//                 (uint32_t)perm[p] < B k.)
//   chain order   one fp32 fma chain per output element, rounded once.  The decode takes a row's valid slots in
//                 slot order (stage_gather).  The grouped kernels take a latent's list perm[seg[j] .. seg[j + 1])
//                 in perm order (list_sum): a list of at most L = CC_PAIRS_GRAD_SPLIT entries is one chain from
//                 +0; a longer list is summed in its consecutive pieces of L (the last one shorter), each such a
//                 chain from +0, and the piece sums are added in piece order onto +0.
//   fixed sums    no float atomics, no spin waits: every summation order is fixed by the arguments alone, so two
//                 calls give equal bits.
#pragma once
#include "mask_common.h"

namespace cc {

constexpr int PAIRS_THREADS = 256;
constexpr int PAIRS_NW = PAIRS_THREADS / 64;
constexpr int PAIRS_MAX_K = 1 << 17;                 // slots per row
constexpr int64_t PAIRS_SPLIT = CC_PAIRS_GRAD_SPLIT;  // L: a longer list is summed in pieces of L
constexpr int PAIRS_UNROLL = 4;                      // rows (of W_dec, of g, of x) in flight per lane
constexpr int PAIRS_ROW_GROUPS = 2048;               // workgroups of a kernel over the batch rows: 8 per CU of a 256-CU part
constexpr int64_t PAIRS_LIST_GROUPS = 1 << 16;       // workgroups of a kernel over the latents' lists

CC_DEV void zero8(float (&a)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
}
CC_DEV void add8(float (&a)[8], const float (&b)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] += b[j];
}
// acc[j] = fma(v, element j of w, acc[j])
template <int DT> CC_DEV void fma_vec8(float v, const Vec8<DT>& w, float (&acc)[8]) {
  uint32_t b[8];
  vec8_bits<DT>(w, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v, bits_float<DT>(b[j]), acc[j]);
}

// ---- the staged gather of the decode kernels
// A tile of PAIRS_THREADS slots, one per lane: the in-range ones compacted in slot order as (index, fp32 value).
struct PairStage {
  int32_t idx[PAIRS_THREADS];
  float val[PAIRS_THREADS];
  uint32_t wtot[PAIRS_NW];
};

// acc (the lane's 8 columns at col; `on`: they exist) += the chain over a row's k slots (vrow, irow) in slot order.  The
// tile is staged for a row's first chunk of columns (`first`) and serves its other chunks; k > PAIRS_THREADS is
// staged again tile by tile for every chunk.  cnt: the in-range slots of the staged tile, kept by the caller from
// chunk to chunk.  The compacted entries are wave-uniform (LDS broadcast reads, the row offset in scalar registers,
// 64-bit: 2^17 x 4608 elements exceed 2^31); PAIRS_UNROLL row loads are issued before the first fma, and the fmas
// consume them in slot order.  Every lane of the workgroup calls it (barriers).  (A function, not a macro: against a
// copy written into the kernel it costs decode_pairs_partial_kernel 4 / 7 VGPRs, inside the 64-register bracket.)
template <int DT>
CC_DEV void stage_gather(PairStage& st, const typename Elem<DT>::T* __restrict__ vrow, const int32_t* __restrict__ irow,
                         int k, uint32_t h, const void* __restrict__ W, int64_t ldw, int64_t col, bool on, bool first,
                         int& cnt, float (&acc)[8]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int t0 = 0; t0 < k; t0 += PAIRS_THREADS) {
    if (first || k > PAIRS_THREADS) {  // (uniform) stage the tile
      const int s = t0 + tid;
      const int32_t i = s < k ? irow[s] : -1;
      const bool ok = (uint32_t)i < h;  // the range check
      const uint32_t one = ok ? 1u : 0u;
      // (its barrier also ends the previous tile's reads of st.idx / st.val)
      CC_BLOCK_EXCL_SCAN(PAIRS_NW, one, lane, w, st.wtot, before, all);
      if (ok) {
        st.idx[before] = i;
        st.val[before] = Elem<DT>::to_f(vrow[s]);
      }
      __syncthreads();  // (st.wtot is next written after this barrier: one set is enough)
      cnt = (int)all;
    }
    for (int s0 = 0; s0 < cnt; s0 += PAIRS_UNROLL) {
      Vec8<DT> wv[PAIRS_UNROLL];
      float v[PAIRS_UNROLL];
#pragma unroll
      for (int u = 0; u < PAIRS_UNROLL; ++u) {
        if (s0 + u < cnt) {  // (uniform)
          const int64_t i = __builtin_amdgcn_readfirstlane(st.idx[s0 + u]);
          v[u] = st.val[s0 + u];
          wv[u] = load_vec8<DT>(W, i * ldw + col, on);
        }
      }
#pragma unroll
      for (int u = 0; u < PAIRS_UNROLL; ++u)
        if (s0 + u < cnt) fma_vec8<DT>(v[u], wv[u], acc);
    }
  }
}

// ---- the pairs grouped by latent: perm [P], seg [h + 1]
// seg[j] clamped to [0, P] (end < begin is an empty list)
CC_DEV int64_t seg_at(const int64_t* __restrict__ seg, int64_t j, int64_t P) {
  const int64_t v = seg[j];
  return v < 0 ? 0 : (v > P ? P : v);
}

// Workspace row t (t < P / L) belongs to the full piece that starts in perm[t L .. (t + 1) L): full pieces are
// disjoint and L long, so no two share a row.  -> that piece's start, or -1 if there is none.  The one list that can
// own the row is found by a binary search of seg for position (t + 1) L - 1, which every piece starting in the
// window covers.
CC_DEV int64_t piece_start(const int64_t* __restrict__ seg, int64_t h, int64_t P, int64_t t) {
  constexpr int64_t L = PAIRS_SPLIT;
  const int64_t x = t * L + L - 1;
  // the last j in [0, h) with seg[j] <= x: the list that holds position x when seg is non-decreasing
  int64_t lo = 0, hi = h;  // seg[lo] <= x (taken as given for lo = 0), seg[hi] > x (likewise for hi = h)
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (seg_at(seg, mid, P) <= x) lo = mid; else hi = mid;
  }
  const int64_t b = seg_at(seg, lo, P), e = seg_at(seg, lo + 1, P);
  if (e - b <= L || b > x) return -1;  // not a split list, or it begins behind this window
  const int64_t s = b >= t * L ? b : b + (t * L - b + L - 1) / L * L;  // the piece start in the window
  return s > x || s + L > e ? -1 : s;  // (the list's last, shorter piece is the row kernel's)
}

// The operands of a list entry perm[p] = slot r k + s: val[slot] * g[r] (cc_pairs_grad_decoder, cc_pairs_wgrad's
// dW_dec) and, TWO: gpre[slot], rounded to the dtype where read, * x[r] and on its own (dW_enc, db_enc)
struct PairList {
  const int32_t* perm;
  const void* val;    // [B k] dtype
  const float* gpre;  // [B k] fp32
  uint32_t Bk, k;
  const void* g;  // [B][ldg]
  const void* x;  // [B][ldx]
  int64_t ldg, ldx;
};
// a lane's sums: 8 columns of val * g, of gpre * x, and the sum of gpre (the last two: TWO only)
struct ListAcc {
  float d[8], e[8], b;
};
CC_DEV void zero_acc(ListAcc& a) {
  zero8(a.d);
  zero8(a.e);
  a.b = 0.f;
}
// a workspace row holds a full piece's sums: [K d] or, TWO, [K d | K e | b, 7 unused]
template <bool TWO> constexpr int64_t piece_pitch(int64_t K) { return TWO ? 2 * K + 8 : K; }

// acc += the chains over perm[p0 .. p1) in order, the 8 columns at col; entries outside [0, Bk) are skipped.  The
// entry and its coefficients are wave-uniform and read once for every stream.
template <int DT, bool TWO>
CC_DEV void list_chain(const PairList& a, int64_t p0, int64_t p1, int64_t col, ListAcc& acc) {
  typedef typename Elem<DT>::T T;
  for (int64_t q0 = p0; q0 < p1; q0 += PAIRS_UNROLL) {
    Vec8<DT> gv[PAIRS_UNROLL], xv[PAIRS_UNROLL];
    float v[PAIRS_UNROLL], p[PAIRS_UNROLL];
    bool ok[PAIRS_UNROLL];
#pragma unroll
    for (int u = 0; u < PAIRS_UNROLL; ++u) {
      ok[u] = false;
      if (q0 + u < p1) {  // (uniform)
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane(a.perm[q0 + u]);
        ok[u] = slot < a.Bk;
        if (ok[u]) {
          const int64_t row = (int64_t)(slot / a.k);
          v[u] = Elem<DT>::to_f(((const T*)a.val)[slot]);
          gv[u] = load_vec8<DT>(a.g, row * a.ldg + col, true);
          if constexpr (TWO) {
            p[u] = Elem<DT>::round(a.gpre[slot]);
            xv[u] = load_vec8<DT>(a.x, row * a.ldx + col, true);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PAIRS_UNROLL; ++u) {
      if (ok[u]) {
        fma_vec8<DT>(v[u], gv[u], acc.d);
        if constexpr (TWO) {
          fma_vec8<DT>(p[u], xv[u], acc.e);
          acc.b += p[u];
        }
      }
    }
  }
}

// launch 1 of a grouped entry point: workspace row t = the sums of the full piece that owns it, if there is one
template <int DT, bool TWO>
CC_DEV void list_pieces(const PairList& a, int64_t P, const int64_t* __restrict__ seg, int64_t h, uint32_t ng,
                        float* __restrict__ ws, int64_t nrows) {
  const int64_t K = (int64_t)ng * 8;
  for (int64_t t = blockIdx.x; t < nrows; t += gridDim.x) {
    const int64_t s = piece_start(seg, h, P, t);
    if (s < 0) continue;
    float* const wrow = ws + t * piece_pitch<TWO>(K);
    for (uint32_t G = threadIdx.x; G < ng; G += PAIRS_THREADS) {
      const int64_t col = (int64_t)G * 8;
      ListAcc acc;
      zero_acc(acc);
      list_chain<DT, TWO>(a, s, s + PAIRS_SPLIT, col, acc);
      store_cols8(wrow + col, acc.d);
      if constexpr (TWO) {
        store_cols8(wrow + K + col, acc.e);
        if (G == 0) wrow[2 * K] = acc.b;
      }
    }
  }
}

// launch 2's sum of the list perm[b .. e), the 8 columns at col: a short list's chain, or a long list's workspace
// rows in piece order (AHEAD of them loaded before the first add) plus its last, shorter piece, summed here
template <int DT, bool TWO, int AHEAD>
CC_DEV void list_sum(const PairList& a, int64_t b, int64_t e, const float* __restrict__ ws, int64_t K, int64_t col,
                     ListAcc& acc) {
  constexpr int64_t L = PAIRS_SPLIT;
  zero_acc(acc);
  if (e - b <= L) {  // (uniform; an empty or reversed list leaves +0)
    list_chain<DT, TWO>(a, b, e, col, acc);
    return;
  }
  const int64_t nfull = (e - b) / L;
  for (int64_t q0 = 0; q0 < nfull; q0 += AHEAD) {
    ListAcc part[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
      if (q0 + u < nfull) {
        const int64_t at = ((b + (q0 + u) * L) / L) * piece_pitch<TWO>(K);
        load8f(ws, at + col, part[u].d);
        if constexpr (TWO) {
          load8f(ws, at + K + col, part[u].e);
          part[u].b = ws[at + 2 * K];
        }
      }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
      if (q0 + u < nfull) {
        add8(acc.d, part[u].d);
        if constexpr (TWO) {
          add8(acc.e, part[u].e);
          acc.b += part[u].b;
        }
      }
  }
  if (b + nfull * L < e) {
    ListAcc last;
    zero_acc(last);
    list_chain<DT, TWO>(a, b + nfull * L, e, col, last);
    add8(acc.d, last.d);
    if constexpr (TWO) {
      add8(acc.e, last.e);
      acc.b += last.b;
    }
  }
}

// ---- host: the entry points' argument checks
// The CC_ERR_* code of a pair entry point over B rows of k slots and h latents, in the house order:
//   shape      B, k, h >= 1; rows of K = n d columns, d a multiple of 8 (an entry point that takes K: n = 1, d = K; one
//              without such rows: n = 1, d = 8), K saturating where n * d would leave int64 (no pitch reaches it);
//              every pitch (lds: of the dtype's rows, lds32: of fp32 rows) >= K; P, the grouped list's length (0: it
//              takes none), >= 0; shape_ok, the entry point's own condition
//   null       ptrs_ok: its required pointers
//   dtype      bf16 or fp32 (null: it takes none)
//   too large  h, K and P within int32, k <= PAIRS_MAX_K; flat: the slot numbers, B k, within int32; small_ok
//   alignment  p16 / p8 / p4 / pes: pointers by required alignment (pes: one element; null ones pass); every pitch
//              a multiple of 16 bytes
static int pairs_check(int64_t B, int k, int64_t h, int64_t n, int64_t d, std::initializer_list<int64_t> lds, bool flat,
                       int64_t P, bool shape_ok, bool ptrs_ok, const int* dtype, bool small_ok,
                       std::initializer_list<const void*> p16, std::initializer_list<const void*> p4,
                       std::initializer_list<const void*> p8 = {}, std::initializer_list<const void*> pes = {},
                       std::initializer_list<int64_t> lds32 = {}) {
  if (B < 1 || k < 1 || h < 1 || n < 1 || d < 8 || (d & 7) || P < 0 || !shape_ok) return CC_ERR_SHAPE;
  const int64_t K = n > INT64_MAX / d ? INT64_MAX : n * d;
  int64_t all = 0, all32 = 0;
  for (const int64_t ld : lds) {
    if (ld < K) return CC_ERR_SHAPE;
    all |= ld;
  }
  for (const int64_t ld : lds32) {
    if (ld < K) return CC_ERR_SHAPE;
    all32 |= ld;
  }
  if (!ptrs_ok) return CC_ERR_NULL;
  if (dtype && *dtype != CC_BF16 && *dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > INT32_MAX || k > PAIRS_MAX_K || K > INT32_MAX || (flat && B > INT32_MAX / k) || P > INT32_MAX || !small_ok)
    return CC_ERR_TOO_LARGE;
  const int64_t es = dtype && *dtype == CC_BF16 ? 2 : 4;
  if (!aligned(p16, 15) || ((all * es) & 15) || ((all32 * 4) & 15) || !aligned(p8, 7) || !aligned(p4, 3) ||
      !aligned(pes, (uintptr_t)es - 1))
    return CC_ERR_ALIGN;
  return CC_OK;
}

}  // namespace cc
