// Decoder matching (crosscoder_amd.match_decoders): the merge of cc_decoder_match's key slabs.  gfx950.
//
// cc_decoder_match (gemm.hip, EPI_MATCH) leaves, per wave row block r of a candidate chunk and per query j, the best
// (score, candidate) pair as one 64-bit key whose unsigned order is (score descending, candidate index ascending);
// key 0 = no candidate.  This kernel folds a slab into the running best of every query:
//   best[j] = max(best[j], max_r part[r][j])
// in one streaming pass (one lane per query, coalesced 8-byte loads, MR_UNROLL rows in flight).  An integer max: the
// result does not depend on the chunking of the candidates or on the order of the slab rows.
#include "cc_common.h"

namespace cc {

constexpr int MR_THREADS = 256;
constexpr int MR_UNROLL = 8;

__global__ __launch_bounds__(MR_THREADS) void match_reduce_kernel(const uint64_t* __restrict__ part, int R, int64_t N,
                                                                  uint64_t* __restrict__ best) {
  const int64_t j = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (j >= N) return;
  uint64_t b = best[j];
  for (int r0 = 0; r0 < R; r0 += MR_UNROLL) {
    uint64_t v[MR_UNROLL];
#pragma unroll
    for (int u = 0; u < MR_UNROLL; ++u) v[u] = r0 + u < R ? part[(int64_t)(r0 + u) * N + j] : 0ull;
#pragma unroll
    for (int u = 0; u < MR_UNROLL; ++u) b = v[u] > b ? v[u] : b;
  }
  best[j] = b;
}

}  // namespace cc

using namespace cc;

extern "C" {

int cc_match_reduce(const uint64_t* part, int64_t R, int64_t N, uint64_t* best, void* stream) {
  if (!part || !best) return CC_ERR_NULL;
  if (R <= 0 || N <= 0) return CC_ERR_SHAPE;
  if (((uintptr_t)part & 7) || ((uintptr_t)best & 7)) return CC_ERR_ALIGN;
  if (R > INT32_MAX || (N + MR_THREADS - 1) / MR_THREADS > INT32_MAX) return CC_ERR_TOO_LARGE;
  dim3 grid((unsigned)((N + MR_THREADS - 1) / MR_THREADS));
  hipLaunchKernelGGL(match_reduce_kernel, grid, dim3(MR_THREADS), 0, (hipStream_t)stream, part, (int)R, N, best);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

}  // extern "C"
