// BatchTopK selection over the whole batch (BatchTopK crosscoders): acts [B][ld], first h columns, masked in place
// (or into acts_out) to the n_keep best (row, latent) pairs of the batch under score = act * weight[latent]
// (or the activation itself), plus the step's side outputs (column-sum partials, selected counts), the per-row
// counts and the threshold score; and the inference form, one pass that keeps score >= *theta.  gfx950.
//
// Eligibility, the tie order and the fixed sums are mask_common.h's rules.  Selection is a radix select on integer
// keys over the whole [B][h] extent (key: the bits of a score > 0 of an activation > 0, else 0).  Keys are the 16 element
// bits for unweighted bf16 (digits 8 + 8) and the 32 fp32 score bits otherwise (bit 31 is clear: digits
// 11 + 12 + 8, so three reads fix the threshold instead of four).
// The phases are separate launches on the one stream; no workgroup waits for another inside a kernel:
//   hist<p>    every workgroup histograms digit p of the keys that match the digits fixed so far (LDS, integer
//              atomics on per-lane copies: copy = lane % COPIES, 32 copies for 8-bit digits) and adds its non-zero
//              bins to the global histogram (integer atomics: order-free).  The last digit's per-workgroup
//              histogram is also left as a row of a [workgroups][256] slab.
//   select<p>  one workgroup scans the global histogram from the top for the digit that holds the wanted rank.
//   mask       admits every key above the threshold T and the first `need` keys equal to T in flat-index order:
//              a workgroup's tie base is the sum of the slab's column (T's last digit) over the workgroups before
//              it, its own ties are ordered by CC_BLOCK_EXCL_SCAN (only when some tie at T is left out; otherwise
//              key >= T decides and no workgroup barrier runs in the loop).
// Work split (the same in every phase, so the slab rows are the mask pass' workgroups): the flat extent is cut into
// segments of 1024 lanes x 8 consecutive columns in flat-index order -- h >= 8192: a segment is 8192 columns of one
// row; below: 1024 / (h / 8) whole rows -- and a workgroup takes a contiguous run of segments, so flat-index order
// is (workgroup, segment, lane, element) and a lane owns the same columns in every segment.
// Column sums: wide rows add the selected values to the workgroup's own partial row (zeroed and updated by the lane
// that owns the column); narrow rows keep 8 sums per lane and fold the lanes that share a column (fold_cols8).
#include "mask_common.h"

namespace cc {

constexpr int BT_NT = 1024, BT_NW = BT_NT / 64, BT_CH = BT_NT * 8;
constexpr int BT_MAX_G = 256;       // workgroups (= column-sum partial rows = count partials = slab rows)
constexpr int BT_HIST_WORDS = 8192;  // LDS histogram words: bins x copies
constexpr int BT_GBINS = 4096;       // global histogram words per pass
constexpr int BT_LAST_BINS = 256;    // the last digit is 8 bits in both plans
// workspace words: state | global histograms [3][BT_GBINS] | slab [G][BT_LAST_BINS]
// state: 0 prefix (finally T), 1 rank (finally need), 2 n_sel, 3 eligible, 4 keys equal to T
constexpr int BT_ST_WORDS = 16;
constexpr int BT_HEAD_WORDS = BT_ST_WORDS + 3 * BT_GBINS;

constexpr int bt_passes(int KB) { return KB == 16 ? 2 : 3; }
constexpr int bt_shift(int KB, int p) { return KB == 16 ? (p == 0 ? 8 : 0) : (p == 0 ? 20 : p == 1 ? 8 : 0); }
constexpr int bt_bits(int KB, int p) { return KB == 16 ? 8 : (p == 0 ? 11 : p == 1 ? 12 : 8); }
template <int DT, bool W> constexpr int bt_keybits() { return DT == CC_BF16 && !W ? 16 : 32; }

struct BtMap {
  int U;     // 8-column units per row
  int S;     // wide: segments per row
  int RP;    // narrow: rows per segment
  int wide;  // U >= BT_NT
  int nseg, spg, G;
};

static BtMap bt_map(int64_t B, int64_t h) {
  BtMap m;
  m.U = (int)(h / 8);
  m.wide = m.U >= BT_NT;
  int64_t nseg;
  if (m.wide) {
    m.S = (m.U + BT_NT - 1) / BT_NT;
    m.RP = 1;
    nseg = B * m.S;
  } else {
    m.S = 1;
    m.RP = BT_NT / m.U;
    nseg = (B + m.RP - 1) / m.RP;
  }
  const int64_t g0 = nseg < BT_MAX_G ? nseg : BT_MAX_G;
  const int64_t spg = (nseg + g0 - 1) / g0;
  m.nseg = (int)nseg;
  m.spg = (int)spg;
  m.G = (int)((nseg + spg - 1) / spg);
  return m;
}

// the 8 keys of a lane's elements: weighted, the bits of the fp32 product (one IEEE multiply) where both the
// activation and the product are > 0
template <int DT, bool W> CC_DEV void bt_keys(const uint32_t (&u)[8], const Cols8& w, uint32_t (&key)[8]) {
  constexpr int EB = ELEM_BITS<DT>;
  if constexpr (!W) {
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = pos_key<EB>(u[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t s = pos_key<32>(__float_as_uint(__fmul_rn(bits_float<DT>(u[j]), w.v[j])));
      key[j] = pos_key<EB>(u[j]) ? s : 0u;
    }
  }
}

// a lane's place in segment s: (row, first column, inside the extent)
struct BtPos { int row, col; bool ok; };
CC_DEV BtPos bt_pos_of(const BtMap& m, int s, int tid, int r_in, int c_in, int B, int h) {
  BtPos p;
  if (m.wide) {
    p.row = s / m.S;
    p.col = (s - p.row * m.S) * BT_CH + tid * 8;
    p.ok = p.col < h;
  } else {
    p.row = s * m.RP + r_in;
    p.col = c_in;
    p.ok = r_in < m.RP && p.row < B;
  }
  return p;
}

// ---- a histogram pass
template <int DT, bool W, int PASS>
__global__ __launch_bounds__(BT_NT) void bt_hist_kernel(const void* acts, int64_t ld, int B, int h,
                                                        const float* __restrict__ weight, BtMap m,
                                                        uint32_t* __restrict__ ws) {
  constexpr int KB = bt_keybits<DT, W>(), SHIFT = bt_shift(KB, PASS), BITS = bt_bits(KB, PASS);
  constexpr int NB = 1 << BITS, COPIES = BT_HIST_WORDS / NB;
  constexpr bool LAST = PASS == bt_passes(KB) - 1;
  __shared__ uint32_t hist[BT_HIST_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, g = blockIdx.x;
  uint32_t prefix = 0u;
  if constexpr (PASS > 0) {
    if (ws[2] == 0u) return;  // (uniform) nothing to select: the mask pass reads no slab then
    prefix = ws[0];
  }
  for (int e = tid; e < BT_HIST_WORDS; e += BT_NT) hist[e] = 0u;
  __syncthreads();
  uint32_t* const myhist = hist + (lane & (COPIES - 1));
  const int r_in = tid / m.U, c_in = (tid - r_in * m.U) * 8;
  const int s0 = g * m.spg, s1 = min(m.nseg, s0 + m.spg);

  BtPos pc = bt_pos_of(m, s0, tid, r_in, c_in, B, h);
  Vec8<DT> cur = load_vec8<DT>(acts, (int64_t)pc.row * ld + pc.col, pc.ok);
  Cols8 wc = {};
  if constexpr (W) wc = load_cols8(weight, pc.col, pc.ok);
  for (int s = s0; s < s1; ++s) {
    const BtPos pn = bt_pos_of(m, s + 1, tid, r_in, c_in, B, h);
    const bool okn = pn.ok && s + 1 < s1;
    const Vec8<DT> nxt = load_vec8<DT>(acts, (int64_t)pn.row * ld + pn.col, okn);
    Cols8 wn = {};
    if constexpr (W) wn = load_cols8(weight, pn.col, okn);
    uint32_t u[8], key[8];
    vec8_bits<DT>(cur, u);
    bt_keys<DT, W>(u, wc, key);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = key[j] != 0u && (PASS == 0 || (key[j] >> ((SHIFT + BITS) & 31)) == prefix);
      if (in) atomicAdd(myhist + ((key[j] >> SHIFT) & (uint32_t)(NB - 1)) * COPIES, 1u);
    }
    cur = nxt;
    wc = wn;
  }
  __syncthreads();
  uint32_t* const ghist = ws + BT_ST_WORDS + PASS * BT_GBINS;
  for (int bin = tid; bin < NB; bin += BT_NT) {
    uint32_t t = 0u;
#pragma unroll
    for (int c = 0; c < COPIES; ++c) t += hist[bin * COPIES + c];
    if (t) atomicAdd(ghist + bin, t);
    if constexpr (LAST) ws[BT_HEAD_WORDS + g * BT_LAST_BINS + bin] = t;
  }
}

// ---- the digit that holds the wanted rank: #(digit > d) < rank <= #(digit >= d)
template <int KB, int PASS>
__global__ __launch_bounds__(256) void bt_select_kernel(uint32_t* __restrict__ ws, int64_t n_keep,
                                                        uint32_t* __restrict__ info, float* __restrict__ ema,
                                                        float beta) {
  constexpr int BITS = bt_bits(KB, PASS), NB = 1 << BITS, PER = NB / 256;
  constexpr bool LAST = PASS == bt_passes(KB) - 1;
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t* const ghist = ws + BT_ST_WORDS + PASS * BT_GBINS;
  uint32_t prefix = 0u, rank = 0u, n_sel = 0u, eligible = 0u;
  if constexpr (PASS > 0) {
    prefix = ws[0];
    rank = ws[1];
    n_sel = ws[2];
    eligible = ws[3];
  }
  uint32_t cnt[PER], local = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    cnt[j] = ghist[NB - 1 - tid * PER - j];
    local += cnt[j];
  }
  CC_BLOCK_EXCL_SCAN(4, local, lane, w, wsum, before, total);
  if constexpr (PASS == 0) {
    eligible = total;
    n_sel = (int64_t)eligible < n_keep ? eligible : (uint32_t)n_keep;
    rank = n_sel;
  }
  if (n_sel == 0u) {  // (uniform)
    if (tid == 0) {
      ws[2] = 0u;
      ws[3] = eligible;
      if constexpr (LAST) {
        ws[0] = 0xFFFFFFFFu;
        ws[1] = 0u;
        ws[4] = 0u;
        if (info) {
          info[0] = 0u;
          info[1] = 0u;
          info[2] = 0u;
          info[3] = eligible;
        }
      }
    }
    return;
  }
  uint32_t run = before;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (run < rank && rank <= run + cnt[j]) {  // (exactly one thread and j: 1 <= rank <= total)
      const uint32_t d = (uint32_t)(NB - 1 - tid * PER - j);
      const uint32_t T = (prefix << BITS) | d, need = rank - run;
      ws[0] = T;
      ws[1] = need;
      ws[2] = n_sel;
      ws[3] = eligible;
      if constexpr (LAST) {
        ws[4] = cnt[j];
        if (info) {
          info[0] = KB == 16 ? T << 16 : T;
          info[1] = n_sel;
          info[2] = need;
          info[3] = eligible;
        }
        if (ema) {  // the running threshold: T itself while it is unset (< 0)
          const float Tf = __uint_as_float(KB == 16 ? T << 16 : T), cur = *ema;
          *ema = cur < 0.f ? Tf : beta * cur + (1.f - beta) * Tf;
        }
      }
    }
    run += cnt[j];
  }
}

// ---- the mask and the side outputs (THETA: keep score >= *theta, no workspace)
// (acts and acts_out may be the same buffer: no __restrict__ on them)
template <int DT, bool W, bool THETA>
__global__ __launch_bounds__(BT_NT) void bt_mask_kernel(const void* acts, int64_t ld, int B, int h,
                                                        const float* __restrict__ weight, BtMap m,
                                                        const uint32_t* __restrict__ ws, const float* __restrict__ theta,
                                                        void* acts_out, float* __restrict__ colsum_part,
                                                        float* __restrict__ l0_part, int32_t* __restrict__ row_count) {
  constexpr int KB = bt_keybits<DT, W>();
  __shared__ uint32_t wtot[2][BT_NW];
  __shared__ uint32_t wred[BT_NW];
  __shared__ float red[BT_NT * 8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = blockIdx.x;
  const int r_in = tid / m.U, c_in = (tid - r_in * m.U) * 8;
  const int s0 = g * m.spg, s1 = min(m.nseg, s0 + m.spg);

  uint32_t T = 0xFFFFFFFFu, need = 0u;
  bool ordered = false;
  float th = 0.f;
  uint32_t eq_base = 0u;  // keys equal to T before this workgroup's, then before the segment
  if constexpr (THETA) {
    th = *theta;
  } else {
    T = ws[0];
    need = ws[1];
    ordered = need < ws[4];  // (uniform) some key equal to T is left out: flat-index order decides
    if (ordered) {
      const uint32_t v = tid < g ? ws[BT_HEAD_WORDS + tid * BT_LAST_BINS + (T & (BT_LAST_BINS - 1))] : 0u;
      const uint32_t t = wave_sum_u(v);
      if (lane == 0) wred[w] = t;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < BT_NW; ++q) eq_base += wred[q];
      __syncthreads();
    }
  }

  float* const mypart = colsum_part ? colsum_part + (int64_t)g * h : nullptr;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (m.wide && mypart) zero_cols(mypart, m.S, BT_CH, tid, h);
  uint32_t selected = 0u;

  BtPos pc = bt_pos_of(m, s0, tid, r_in, c_in, B, h);
  Vec8<DT> cur = load_vec8<DT>(acts, (int64_t)pc.row * ld + pc.col, pc.ok);
  Cols8 wc = {};
  if constexpr (W) wc = load_cols8(weight, pc.col, pc.ok);
  for (int s = s0; s < s1; ++s) {
    const BtPos pn = bt_pos_of(m, s + 1, tid, r_in, c_in, B, h);
    const bool okn = pn.ok && s + 1 < s1;
    const Vec8<DT> nxt = load_vec8<DT>(acts, (int64_t)pn.row * ld + pn.col, okn);
    Cols8 wn = {};
    if constexpr (W) wn = load_cols8(weight, pn.col, okn);
    uint32_t u[8], key[8];
    vec8_bits<DT>(cur, u);
    bt_keys<DT, W>(u, wc, key);  // (outside the extent: zeros, key 0)

    uint32_t eq = 0u;
    if (ordered) {
      uint32_t mine = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) mine += key[j] == T ? 1u : 0u;
      CC_BLOCK_EXCL_SCAN(BT_NW, mine, lane, w, wtot[s & 1], before, all);
      eq = eq_base + before;
      eq_base += all;
    }
    uint32_t o[8], cnt = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bool sel;
      if constexpr (THETA) {
        sel = key[j] != 0u && __uint_as_float(KB == 16 ? key[j] << 16 : key[j]) >= th;
      } else {
        const bool is_eq = key[j] == T;
        sel = key[j] > T || (is_eq && (!ordered || eq < need));
        eq += is_eq ? 1u : 0u;
      }
      o[j] = sel ? u[j] : 0u;
      cnt += sel ? 1u : 0u;
      if (m.wide) {
        if (sel && mypart) mypart[pc.col + j] += bits_float<DT>(u[j]);
      } else {
        acc[j] += sel ? bits_float<DT>(u[j]) : 0.f;
      }
    }
    if (acts_out && pc.ok) store_bits8<DT>(acts_out, (int64_t)pc.row * ld + pc.col, o);
    selected += cnt;
    if (row_count) {
      const int r0 = __builtin_amdgcn_readfirstlane(pc.row);
      if (__builtin_amdgcn_ballot_w64(cnt != 0u && pc.row != r0) == 0ull) {  // the wave's selected share one row
        const uint32_t t = wave_sum_u(cnt);
        if (lane == 0 && t) atomicAdd(row_count + r0, (int)t);
      } else if (cnt) {
        atomicAdd(row_count + pc.row, (int)cnt);
      }
    }
    pc = pn;
    cur = nxt;
    wc = wn;
  }

  // the lanes that share a column: one per row of a segment
  if (!m.wide && mypart) fold_cols8(acc, red, m.U, m.RP, tid, mypart, c_in);
  if (l0_part) {
    __syncthreads();
    count_to_part<BT_NW>(selected, wred, l0_part + g);
  }
}

template <int DT, bool W>
static void bt_launch(const void* acts, int64_t ld, int64_t B, int64_t h, const float* weight, int64_t n_keep,
                      void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count, uint32_t* info,
                      float* ema, float beta, uint32_t* ws, hipStream_t st) {
  constexpr int KB = bt_keybits<DT, W>();
  const BtMap m = bt_map(B, h);
  const dim3 grid((unsigned)m.G), blk(BT_NT);
  if (hipMemsetAsync(ws, 0, sizeof(uint32_t) * BT_HEAD_WORDS, st) != hipSuccess) return;  // (CC_LAUNCH_CHECK reports)
  if (row_count && hipMemsetAsync(row_count, 0, sizeof(int32_t) * B, st) != hipSuccess) return;
#define BT_PASS(P)                                                                                         \
  hipLaunchKernelGGL((bt_hist_kernel<DT, W, P>), grid, blk, 0, st, acts, ld, (int)B, (int)h, weight, m, ws); \
  hipLaunchKernelGGL((bt_select_kernel<KB, P>), dim3(1), dim3(256), 0, st, ws, n_keep, info, ema, beta)
  BT_PASS(0);
  BT_PASS(1);
  if constexpr (KB == 32) {
    BT_PASS(2);
  }
#undef BT_PASS
  if (acts_out || colsum_part || l0_part || row_count)
    hipLaunchKernelGGL((bt_mask_kernel<DT, W, false>), grid, blk, 0, st, acts, ld, (int)B, (int)h, weight, m, ws,
                       (const float*)nullptr, acts_out, colsum_part, l0_part, row_count);
}

template <int DT, bool W>
static void bt_launch_theta(const void* acts, int64_t ld, int64_t B, int64_t h, const float* weight, const float* theta,
                            void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count, hipStream_t st) {
  const BtMap m = bt_map(B, h);
  if (row_count && hipMemsetAsync(row_count, 0, sizeof(int32_t) * B, st) != hipSuccess) return;
  hipLaunchKernelGGL((bt_mask_kernel<DT, W, true>), dim3((unsigned)m.G), dim3(BT_NT), 0, st, acts, ld, (int)B, (int)h,
                     weight, m, (const uint32_t*)nullptr, theta, acts_out, colsum_part, l0_part, row_count);
}

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_batch_topk_part_rows(int64_t B, int64_t h) { return dims_ok(B, h) ? bt_map(B, h).G : 0; }
int64_t cc_batch_topk_l0_parts(int64_t B, int64_t h) { return dims_ok(B, h) ? bt_map(B, h).G : 0; }

int64_t cc_batch_topk_ws_bytes(int64_t B, int64_t h, int dtype, int weighted) {
  (void)weighted;  // (one layout for both key widths)
  if (!dims_ok(B, h) || (dtype != CC_BF16 && dtype != CC_F32)) return 0;
  return (int64_t)sizeof(uint32_t) * (BT_HEAD_WORDS + (int64_t)bt_map(B, h).G * BT_LAST_BINS);
}

int cc_batch_topk(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* weight, int64_t n_keep,
                  void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count, uint32_t* info,
                  float* threshold_ema, float beta, void* ws, int64_t ws_bytes, void* stream) {
  const int rc = rows_check(ld, B, h, dtype, n_keep >= 1 && (!threshold_ema || (beta >= 0.f && beta < 1.f)),
                            acts && (acts_out || info || row_count) && ws, true, {acts, acts_out, colsum_part, weight},
                            {l0_part, ws, info, row_count, threshold_ema});
  if (rc != CC_OK) return rc;
  if (ws_bytes < cc_batch_topk_ws_bytes(B, h, dtype, weight != nullptr)) return CC_ERR_SHAPE;
  const auto launch = weight ? CC_BY_DTYPE(bt_launch, dtype, true) : CC_BY_DTYPE(bt_launch, dtype, false);
  launch(acts, ld, B, h, weight, n_keep, acts_out, colsum_part, l0_part, row_count, info, threshold_ema, beta,
         (uint32_t*)ws, (hipStream_t)stream);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_threshold_mask(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* weight,
                      const float* theta, void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count,
                      void* stream) {
  const int rc = rows_check(ld, B, h, dtype, true, acts && (acts_out || row_count) && theta, true,
                            {acts, acts_out, colsum_part, weight}, {l0_part, theta, row_count});
  if (rc != CC_OK) return rc;
  const auto launch = weight ? CC_BY_DTYPE(bt_launch_theta, dtype, true) : CC_BY_DTYPE(bt_launch_theta, dtype, false);
  launch(acts, ld, B, h, weight, theta, acts_out, colsum_part, l0_part, row_count, (hipStream_t)stream);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
