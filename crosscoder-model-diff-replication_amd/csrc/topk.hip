// Per-row top-k of the activations (TopK crosscoders): acts [B][ld], first h columns, masked in place (or into
// acts_out) to each row's k largest positive values, plus the compact (latent, value) pairs and the side
// outputs of the step (column-sum partials and selected counts of the masked activations).  gfx950.
//
// Positive floats order as their bit patterns, so selection is a radix select on integer keys (the element's
// bits when it is > 0, else 0: ineligible), 8-bit digits from the top: 2 passes for bf16, 4 for fp32.
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
// (per chunk: a prefix count across lanes, then across waves), which is also each element's output slot.
// No float atomics: the partial rows and counts are fixed by (B, h) and the input alone.
//
// AUX (cc_auxk_rows, the AuxK dead-latent loss): the same selection with a column predicate -- an element's key
// is 0 unless since_fired[column] >= dead_after.  A lane owns the same columns in every row, so the predicate is
// loaded once per workgroup (one int64 per owned column) and kept as bits over the row loop: 8 NCH bits in one
// register, or (NCH = 0, up to 16 chunks) 128 bits in two 64-bit registers.  It writes the dense output and the
// row counts only.
#include "cc_common.h"

namespace cc {

constexpr int TK_COPIES = 32;
constexpr int TK_BINS = 256;
constexpr int TK_MAX_H = 1 << 17;

template <int DT> struct TkVec { uint4 q[DT == CC_F32 ? 2 : 1]; };

template <int DT> CC_DEV TkVec<DT> tk_load(const void* base, int64_t e, bool ok) {
  TkVec<DT> v;
  if constexpr (DT == CC_BF16) {
    v.q[0] = ok ? *(const uint4*)((const bf16_t*)base + e) : uint4{0u, 0u, 0u, 0u};
  } else {
    v.q[0] = ok ? *(const uint4*)((const float*)base + e) : uint4{0u, 0u, 0u, 0u};
    v.q[1] = ok ? *(const uint4*)((const float*)base + e + 4) : uint4{0u, 0u, 0u, 0u};
  }
  return v;
}

// the 8 elements' bits
template <int DT> CC_DEV void tk_bits(const TkVec<DT>& v, uint32_t (&u)[8]) {
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

// the key: the bits of an element > 0 (sign clear, not zero, not NaN; +inf and subnormals count), else 0
template <int DT> CC_DEV uint32_t tk_key(uint32_t u) {
  constexpr uint32_t INF = DT == CC_BF16 ? 0x7F80u : 0x7F800000u;
  return (u - 1u) < INF ? u : 0u;
}
template <int DT> CC_DEV float tk_float(uint32_t u) { return __uint_as_float(DT == CC_BF16 ? u << 16 : u); }

template <int DT> CC_DEV void tk_store(void* base, int64_t e, const uint32_t (&u)[8]) {
  if constexpr (DT == CC_BF16) {
    *(uint4*)((bf16_t*)base + e) = uint4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
  } else {
    *(uint4*)((float*)base + e) = uint4{u[0], u[1], u[2], u[3]};
    *(uint4*)((float*)base + e + 4) = uint4{u[4], u[5], u[6], u[7]};
  }
}

CC_DEV uint32_t tk_wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// the key under the column predicate: db holds the dead bits of the 8 columns of this lane's chunk
template <int DT, bool AUX> CC_DEV uint32_t tk_key_if(uint32_t u, uint32_t db, int j) {
  if constexpr (AUX) return (db >> j) & 1u ? tk_key<DT>(u) : 0u;
  else return tk_key<DT>(u);
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
  if (!REG && mypart)
    for (int c = 0; c < nch; ++c) {
      const int col = c * CH + tid * 8;
      if (col < h) {
        *(float4*)(mypart + col) = float4{0.f, 0.f, 0.f, 0.f};
        *(float4*)(mypart + col + 4) = float4{0.f, 0.f, 0.f, 0.f};
      }
    }
  uint32_t selected_rows = 0u;  // selected elements over this workgroup's rows
  __syncthreads();

  TkVec<DT> cur[NR];
  if constexpr (REG) {
    if ((int)blockIdx.x < B) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * CH + tid * 8;
        cur[c] = tk_load<DT>(acts, (int64_t)blockIdx.x * ld + col, col < h);
      }
    }
  }

  for (int row = blockIdx.x; row < B; row += gridDim.x) {
    const int64_t roff = (int64_t)row * ld;
    TkVec<DT> nxt[NR];
    if constexpr (REG) {
      const int nrow = row + gridDim.x;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = c * CH + tid * 8;
        nxt[c] = tk_load<DT>(acts, (int64_t)nrow * ld + col, nrow < B && col < h);
      }
    }
    // f(c, col, u): chunk c's 8 elements of this lane (column col .. col + 7 < h)
    auto chunks = [&](auto f) {
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int col = c * CH + tid * 8;
          uint32_t u[8];
          tk_bits<DT>(cur[c], u);
          f(c, col, u);
        }
      } else {
        for (int c = 0; c < nch; ++c) {
          const int col = c * CH + tid * 8;
          uint32_t u[8];
          tk_bits<DT>(tk_load<DT>(acts, roff + col, col < h), u);
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
      const uint32_t incl = tk_wave_incl_scan(local, lane);
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
      const uint32_t incl = tk_wave_incl_scan(mine, lane);
      if (lane == 63) wtot[c & 1][w] = incl;
      __syncthreads();
      uint32_t before = incl - mine, all = 0u;
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const uint32_t t = wtot[c & 1][q];
        if (q < w) before += t;
        all += t;
      }
      uint32_t gt = base_gt + (before >> 16), eq = base_eq + (before & 0xffffu);
      base_gt += all >> 16;
      base_eq += all & 0xffffu;
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
            acc[c][j] += sel ? tk_float<DT>(u[j]) : 0.f;
          } else {
            if (sel && mypart) mypart[col + j] += tk_float<DT>(u[j]);
          }
          gt += is_gt ? 1u : 0u;
          eq += is_eq ? 1u : 0u;
        }
        if (acts_out) tk_store<DT>(acts_out, roff + col, o);
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
        if (col < h) {
          *(float4*)(mypart + col) = float4{acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
          *(float4*)(mypart + col + 4) = float4{acc[c][4], acc[c][5], acc[c][6], acc[c][7]};
        }
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

template <int DT>
static void tk_launch(const void* acts, int64_t ld, int64_t B, int64_t h, int k, void* acts_out, int32_t* idx_out,
                      void* val_out, float* colsum_part, float* l0_part, hipStream_t st) {
  const dim3 grid((unsigned)tk_groups(B, h));
#define TK_GO(NT, NCH)                                                                                              \
  hipLaunchKernelGGL((topk_rows_kernel<DT, NT, NCH>), grid, dim3(NT), 0, st, acts, ld, (int)B, (int)h, k, acts_out, \
                     idx_out, val_out, colsum_part, l0_part)
  // (fp32 rows beyond one chunk re-read: two chunks of fp32 in registers spill at the 128 VGPRs of 16 waves)
  if (h <= 2048) TK_GO(256, 1);
  else if (h <= 8192) TK_GO(1024, 1);
  else if (DT == CC_BF16 && h <= 16384) {
    if constexpr (DT == CC_BF16) TK_GO(1024, 2);
  } else TK_GO(1024, 0);
#undef TK_GO
}

template <int DT>
static void ak_launch(const void* acts, int64_t ld, int64_t B, int64_t h, int k, const int64_t* since_fired,
                      int64_t dead_after, void* aux_out, int32_t* row_count, hipStream_t st) {
  const dim3 grid((unsigned)tk_groups(B, h));
#define AK_GO(NT, NCH)                                                                                                \
  hipLaunchKernelGGL((topk_rows_kernel<DT, NT, NCH, true>), grid, dim3(NT), 0, st, acts, ld, (int)B, (int)h, k, aux_out, \
                     (int32_t*)nullptr, (void*)nullptr, (float*)nullptr, (float*)nullptr, since_fired, dead_after,    \
                     row_count)
  // (the four forms of tk_launch, by h)
  if (h <= 2048) AK_GO(256, 1);
  else if (h <= 8192) AK_GO(1024, 1);
  else if (DT == CC_BF16 && h <= 16384) {
    if constexpr (DT == CC_BF16) AK_GO(1024, 2);
  } else AK_GO(1024, 0);
#undef AK_GO
}

}  // namespace cc

using namespace cc;

extern "C" {

int64_t cc_topk_part_rows(int64_t B, int64_t h) { return B < 1 || h < 1 ? 0 : tk_groups(B, h); }
int64_t cc_topk_l0_parts(int64_t B, int64_t h) { return B < 1 || h < 1 ? 0 : tk_groups(B, h); }

int cc_topk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k, void* acts_out,
                 int32_t* idx_out, void* val_out, float* colsum_part, float* l0_part, void* stream) {
  if (B < 1 || h < 8 || (h & 7) || (ld & 7) || ld < h || k < 1 || k > h) return CC_ERR_SHAPE;
  if (!acts || (idx_out == nullptr) != (val_out == nullptr)) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > TK_MAX_H || B > (1 << 30)) return CC_ERR_TOO_LARGE;
  if (((uintptr_t)acts | (uintptr_t)acts_out | (uintptr_t)colsum_part) & 15) return CC_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CC_BF16)
    tk_launch<CC_BF16>(acts, ld, B, h, k, acts_out, idx_out, val_out, colsum_part, l0_part, st);
  else
    tk_launch<CC_F32>(acts, ld, B, h, k, acts_out, idx_out, val_out, colsum_part, l0_part, st);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

int cc_auxk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k_aux, const int64_t* since_fired,
                 int64_t dead_after, void* aux_out, int32_t* row_count, void* stream) {
  if (B < 1 || h < 8 || (h & 7) || (ld & 7) || ld < h || k_aux < 1 || k_aux > h) return CC_ERR_SHAPE;
  if (!acts || !since_fired || !aux_out || aux_out == acts) return CC_ERR_NULL;
  if (dtype != CC_BF16 && dtype != CC_F32) return CC_ERR_DTYPE;
  if (h > TK_MAX_H || B > (1 << 30)) return CC_ERR_TOO_LARGE;
  if ((((uintptr_t)acts | (uintptr_t)aux_out) & 15) || ((uintptr_t)since_fired & 7) || ((uintptr_t)row_count & 3))
    return CC_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CC_BF16) ak_launch<CC_BF16>(acts, ld, B, h, k_aux, since_fired, dead_after, aux_out, row_count, st);
  else ak_launch<CC_F32>(acts, ld, B, h, k_aux, since_fired, dead_after, aux_out, row_count, st);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
