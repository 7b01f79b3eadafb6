// Per-row top-k of the activations (TopK crosscoders): acts [B][ld], first h columns, masked in place (or into
// acts_out) to each row's k largest positive values, plus the compact (latent, value) pairs and the side
// outputs of the step (column-sum partials and selected counts of the masked activations).  gfx950.
//
// Eligibility, the tie order and the fixed sums are mask_common.h's rules.  Selection is a radix select on the
// integer keys (pos_key: 0 is ineligible), 8-bit digits from the top: 2 passes for bf16, 4 for fp32.
// A workgroup takes rows in turn (row = blockIdx.x + i * gridDim.x); lane t owns the 8 consecutive columns
// c * 8 * NT + 8 t of every chunk c (one 16-B / 32-B load), so index order is (chunk, lane, element).
//   NCH > 0: the row (NCH chunks) stays in registers over all passes, the next row is loaded while this one is
//            selected, and the column sums of the masked rows are kept in registers (8 NCH per lane).
//   NCH = 0: h beyond 2 chunks (bf16) or 1 chunk (fp32): every pass re-reads the row (L2 hits); the workgroup's
//            column-sum row is zeroed and the selected values are added to it by the lane that owns the column
//            (program order).
// A pass: every lane adds its matching elements to a 256-bin histogram kept as 32 copies (copy = lane % 32:
// the address's bank is the lane's own, so integer LDS atomics of one half-wave never collide), the copies are
// summed, and every wave scans the 256 totals from the top for the digit that holds the wanted rank.
// The last pass admits every key above the threshold T and the first `need` keys equal to T in index order
// (per chunk: CC_BLOCK_EXCL_SCAN), which is also each element's output slot.
//
// AUX (cc_auxk_rows, the AuxK dead-latent loss): the same selection with a column predicate -- an element's key
// is 0 unless since_fired[column] >= dead_after.  A lane owns the same columns in every row, so the predicate is
// loaded once per workgroup (one int64 per owned column) and kept as bits over the row loop: 8 NCH bits in one
// register, or (NCH = 0, up to 16 chunks) 128 bits in two 64-bit registers.  It writes the dense output and the
// row counts only.
#include "mask_common.h"

namespace cc {

constexpr int TK_COPIES = 32;
constexpr int TK_BINS = 256;

// the key under the column predicate: db holds the dead bits of the 8 columns of this lane's chunk
template <int DT, bool AUX> CC_DEV uint32_t tk_key_if(uint32_t u, uint32_t db, int j) {
  if constexpr (AUX) return (db >> j) & 1u ? pos_key<ELEM_BITS<DT>>(u) : 0u;
  else return pos_key<ELEM_BITS<DT>>(u);
}

// (acts and acts_out may be the same buffer: no __restrict__ on them)
template <int DT, int NT, int NCH, bool AUX = false>
__global__ __launch_bounds__(NT) void topk_rows_kernel(const void* acts, int64_t ld, int B, int h, int k, void* acts_out,
                                                       int32_t* __restrict__ idx_out, void* __restrict__ val_out,
                                                       float* __restrict__ colsum_part, float* __restrict__ l0_part,
                                                       const int64_t* __restrict__ since_fired = nullptr,
                                                       int64_t dead_after = 0, int32_t* __restrict__ row_count = nullptr) {
  if constexpr (AUX) {  // (the dense output and the row counts only)
    idx_out = nullptr;
    colsum_part = nullptr;
    l0_part = nullptr;
  }
  constexpr int NW = NT / 64, CH = NT * 8, NPASS = DT == CC_BF16 ? 2 : 4;
  constexpr bool REG = NCH > 0;
  constexpr int NR = REG ? NCH : 1;
  __shared__ uint32_t hist[TK_BINS * TK_COPIES];
  __shared__ uint32_t tot[TK_BINS];
  __shared__ uint32_t wtot[2][NW];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nch = REG ? NCH : (h + CH - 1) / CH;
  // AUX: the dead bits of this lane's columns, chunk c in byte c (REG: of dead_lo's low word)
  uint64_t dead_lo = 0u, dead_hi = 0u;
  if constexpr (AUX) {
    for (int c = 0; c < nch; ++c) {
      const int col = c * CH + tid * 8;
      uint64_t b = 0u;
      if (col < h) {
#pragma unroll
        for (int j = 0; j < 8; ++j) b |= (uint64_t)(since_fired[col + j] >= dead_after ? 1u : 0u) << j;
      }
      if (c < 8) dead_lo |= b << (8 * c);
      else dead_hi |= b << (8 * (c - 8));
    }
  }
  auto dead_bits = [&](int c) -> uint32_t {
    if constexpr (!AUX) return 0xffu;
    else if constexpr (REG) return ((uint32_t)dead_lo >> (8 * c)) & 0xffu;
    else return (uint32_t)((c < 8 ? dead_lo : dead_hi) >> (8 * (c & 7))) & 0xffu;
  };
  uint32_t* const myhist = hist + (lane & (TK_COPIES - 1));

  for (int e = tid; e < TK_BINS * TK_COPIES; e += NT) hist[e] = 0u;

  float acc[NR][8];
#pragma unroll
  for (int c = 0; c < NR; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[c][j] = 0.f;
  float* const mypart = colsum_part ? colsum_part + (int64_t)blockIdx.x * h : nullptr;
  if (!REG && mypart) zero_cols(mypart, nch, CH, tid, h);
  uint32_t selected_rows = 0u;  // selected elements over this workgroup's rows
  __syncthreads();

  Vec8<DT> cur[NR];
  if constexpr (REG) {
    if ((int)blockIdx.x < B) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * CH + tid * 8;
        cur[c] = load_vec8<DT>(acts, (int64_t)blockIdx.x * ld + col, col < h);
      }
    }
  }

  for (int row = blockIdx.x; row < B; row += gridDim.x) {
    const int64_t roff = (int64_t)row * ld;
    Vec8<DT> nxt[NR];
    if constexpr (REG) {
      const int nrow = row + gridDim.x;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * CH + tid * 8;
        nxt[c] = load_vec8<DT>(acts, (int64_t)nrow * ld + col, nrow < B && col < h);
      }
    }
    // f(c, col, u): chunk c's 8 elements of this lane (column col .. col + 7 < h)
    auto chunks = [&](auto f) {
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int col = c * CH + tid * 8;
          uint32_t u[8];
          vec8_bits<DT>(cur[c], u);
          f(c, col, u);
        }
      } else {
        for (int c = 0; c < nch; ++c) {
          const int col = c * CH + tid * 8;
          uint32_t u[8];
          vec8_bits<DT>(load_vec8<DT>(acts, roff + col, col < h), u);
          f(c, col, u);
        }
      }
    };

    // ---- radix select: the threshold key T and how many keys equal to T are admitted
    uint32_t prefix = 0u, rank = 0u, n_sel = 0u;
#pragma unroll 1
    for (int p = 0; p < NPASS; ++p) {
      const int shift = 8 * (NPASS - 1 - p);
      chunks([&](int c, int, const uint32_t (&u)[8]) {
        const uint32_t db = dead_bits(c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t key = tk_key_if<DT, AUX>(u[j], db, j);
          const bool in = key != 0u && (p == 0 || (key >> ((shift + 8) & 31)) == prefix);
          if (in) atomicAdd(myhist + ((key >> shift) & 255u) * TK_COPIES, 1u);
        }
      });
      __syncthreads();
      // the 32 copies of a bin: 4 lanes x 8 words, which leave zero for the next pass
      for (int i = tid; i < TK_BINS * 4; i += NT) {
        uint4* const q = (uint4*)(hist + i * 8);
        const uint4 a = q[0], b = q[1];
        q[0] = uint4{0u, 0u, 0u, 0u};
        q[1] = uint4{0u, 0u, 0u, 0u};
        uint32_t s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if ((i & 3) == 0) tot[i >> 2] = s;
      }
      __syncthreads();
      // every wave: lane l holds bins 255 - 4 l .. 252 - 4 l; the digit d with  #(digit > d) < rank <= #(digit >= d)
      uint32_t cnt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[j] = tot[255 - 4 * lane - j];
      const uint32_t local = cnt[0] + cnt[1] + cnt[2] + cnt[3];
      const uint32_t incl = wave_incl_scan(local, lane);
      if (p == 0) {
        const uint32_t eligible = __shfl(incl, 63, 64);
        n_sel = eligible < (uint32_t)k ? eligible : (uint32_t)k;
        rank = n_sel;
      }
      if (n_sel == 0u) break;  // (uniform) nothing to select in this row
      uint32_t run = incl - local, d = 0u, rnew = 0u;
      bool found = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!found && run < rank && rank <= run + cnt[j]) {
          found = true;
          d = 255u - 4u * lane - j;
          rnew = rank - run;
        }
        run += cnt[j];
      }
      const unsigned long long m = __builtin_amdgcn_ballot_w64(found);
      const int src = m ? __builtin_ctzll(m) : 0;  // (exactly one lane: 1 <= rank <= total)
      d = __shfl(d, src, 64);
      rank = __shfl(rnew, src, 64);
      prefix = (prefix << 8) | d;
    }
    const uint32_t T = n_sel ? prefix : 0xFFFFFFFFu, need = n_sel ? rank : 0u;

    // ---- the mask, the pairs, the column sums
    uint32_t base_gt = 0u, base_eq = 0u;
    chunks([&](int c, int col, const uint32_t (&u)[8]) {
      uint32_t key[8], mine = 0u;  // mine: (#key > T) << 16 | #key == T, both <= 8
      const uint32_t db = dead_bits(c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        key[j] = tk_key_if<DT, AUX>(u[j], db, j);
        mine += key[j] > T ? 0x10000u : key[j] == T ? 1u : 0u;
      }
      CC_BLOCK_EXCL_SCAN(NW, mine, lane, w, wtot[c & 1], before, all);
      uint32_t gt = base_gt + (before >> 16), eq = base_eq + (before & 0xffffu);
      base_gt += all >> 16;
      base_eq += (all & 0xffffu);
      if (col < h) {
        uint32_t o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool is_gt = key[j] > T, is_eq = key[j] == T;
          const bool sel = is_gt || (is_eq && eq < need);
          const uint32_t slot = gt + (eq < need ? eq : need);
          o[j] = sel ? u[j] : 0u;
          if (sel && idx_out && slot < (uint32_t)k) {  // (slot < n_sel <= k by construction)
            idx_out[(int64_t)row * k + slot] = col + j;
            if constexpr (DT == CC_BF16) ((bf16_t*)val_out)[(int64_t)row * k + slot] = (bf16_t)u[j];
            else ((uint32_t*)val_out)[(int64_t)row * k + slot] = u[j];
          }
          if constexpr (REG) {
            acc[c][j] += sel ? bits_float<DT>(u[j]) : 0.f;
          } else {
            if (sel && mypart) mypart[col + j] += bits_float<DT>(u[j]);
          }
          gt += is_gt ? 1u : 0u;
          eq += is_eq ? 1u : 0u;
        }
        if (acts_out) store_bits8<DT>(acts_out, roff + col, o);
      }
    });
    if (idx_out)
      for (int s = (int)n_sel + tid; s < k; s += NT) {  // fewer than k eligible: (-1, 0)
        idx_out[(int64_t)row * k + s] = -1;
        if constexpr (DT == CC_BF16) ((bf16_t*)val_out)[(int64_t)row * k + s] = 0;
        else ((uint32_t*)val_out)[(int64_t)row * k + s] = 0u;
      }
    selected_rows += n_sel;
    if constexpr (AUX) {
      if (row_count && tid == 0) row_count[row] = (int32_t)n_sel;
    }
    if constexpr (REG) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) cur[c] = nxt[c];
    }
  }

  if constexpr (REG) {
    if (mypart) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * CH + tid * 8;
        if (col < h) store_cols8(mypart + col, acc[c]);
      }
    }
  }
  if (l0_part && tid == 0) l0_part[blockIdx.x] = (float)selected_rows;
}

// workgroups (= column-sum partial rows = count partials): narrow rows get more, smaller workgroups
static int64_t tk_groups(int64_t B, int64_t h) {
  const int64_t g = h <= 2048 ? 512 : 256;
  return B < g ? B : g;
}

// the form by h (AUX: cc_auxk_rows, which passes no pairs and no partials)
template <int DT, bool AUX>
static void tk_launch(const void* acts, int64_t ld, int64_t B, int64_t h, int k, void* acts_out, int32_t* idx_out,
                      void* val_out, float* colsum_part, float* l0_part, const int64_t* since_fired, int64_t dead_after,
                      int32_t* row_count, hipStream_t st) {
  // (fp32 rows beyond one chunk re-read: two chunks of fp32 in registers spill at the 128 VGPRs of 16 waves)
  constexpr int REG_H = DT == CC_BF16 ? 16384 : 8192;  // the widest row kept in registers
  auto kern = topk_rows_kernel<DT, 256, 1, AUX>;
  if (h > 2048) kern = topk_rows_kernel<DT, 1024, 1, AUX>;
  if constexpr (DT == CC_BF16) {
    if (h > 8192) kern = topk_rows_kernel<DT, 1024, 2, AUX>;
  }
  if (h > REG_H) kern = topk_rows_kernel<DT, 1024, 0, AUX>;
  hipLaunchKernelGGL(kern, dim3((unsigned)tk_groups(B, h)), dim3(h <= 2048 ? 256 : 1024), 0, st, acts, ld, (int)B,
                     (int)h, k, acts_out, idx_out, val_out, colsum_part, l0_part, since_fired, dead_after, row_count);
}

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_topk_part_rows(int64_t B, int64_t h) { return B < 1 || h < 1 ? 0 : tk_groups(B, h); }
int64_t cc_topk_l0_parts(int64_t B, int64_t h) { return B < 1 || h < 1 ? 0 : tk_groups(B, h); }

int cc_topk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k, void* acts_out,
                 int32_t* idx_out, void* val_out, float* colsum_part, float* l0_part, void* stream) {
  const int rc = rows_check(ld, B, h, dtype, k >= 1 && k <= h, acts && (idx_out == nullptr) == (val_out == nullptr),
                            false, {acts, acts_out, colsum_part});
  if (rc != CC_OK) return rc;
  CC_BY_DTYPE(tk_launch, dtype, false)(acts, ld, B, h, k, acts_out, idx_out, val_out, colsum_part, l0_part, nullptr, 0,
                                       nullptr, (hipStream_t)stream);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_auxk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k_aux, const int64_t* since_fired,
                 int64_t dead_after, void* aux_out, int32_t* row_count, void* stream) {
  const int rc = rows_check(ld, B, h, dtype, k_aux >= 1 && k_aux <= h, acts && since_fired && aux_out && aux_out != acts,
                            false, {acts, aux_out}, {row_count}, {since_fired});
  if (rc != CC_OK) return rc;
  CC_BY_DTYPE(tk_launch, dtype, true)(acts, ld, B, h, k_aux, aux_out, nullptr, nullptr, nullptr, nullptr, since_fired,
                                      dead_after, row_count, (hipStream_t)stream);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
