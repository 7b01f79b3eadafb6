/* crosscoder_hip.h — C ABI of libcrosscoder_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for ONE crosscoder training step (fwd + bwd + grad-clip + Adam) of
 * mitroitskii/crosscoder-model-diff-replication.  The reference has no FFI: its "operators"
 * are the torch calls inside CrossCoder / Trainer.  Each entry point below names the
 * reference code it replaces (file:line under the reference tree).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (hipMalloc / torch tensor .data_ptr()), 16-byte aligned,
 *    row-major, rows contiguous.  The library never allocates or frees caller memory.
 *  - `dtype` selects the storage type of params / activations / grads: CC_BF16 or CC_F32
 *    (the reference's cfg["enc_dtype"] "bf16" / "fp32", crosscoder.py:12,30).
 *    All accumulations are fp32 (bf16 inputs go through bf16 MFMA with fp32 accumulate,
 *    fp32 inputs through the exact-f32 MFMA).
 *  - Shapes: B batch rows, n models, d d_model, h dict_size, K = n*d.
 *    Requirements: d % 8 == 0, h % 8 == 0 (16-byte vector rows); any B >= 1.  (The Python layer
 *    serves other dict_size / d_in on zero-padded dims: crosscoder_amd.engine.padded_dims.)
 *  - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); all launches are
 *    asynchronous on it.  No entry point synchronises, allocates, or keeps global state.
 *  - Return value: 0 = CC_OK, else a CC_ERR_* code (>= CC_ERR_HIP_BASE: hipError_t + base).
 *    cc_strerror() maps it to a message.
 *  - Partial-sum slabs ("*_part") are caller-allocated fp32 workspaces whose sizes come from
 *    cc_col_part_rows() / cc_wave_parts(); they make every reduction deterministic
 *    (fixed summation order, no float atomics).
 */
#ifndef CROSSCODER_HIP_H
#define CROSSCODER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#pragma GCC visibility push(default)

#define CC_BF16 1
#define CC_F32 2

#define CC_LAYOUT_KC 0 /* operand stored with the contraction index contiguous   */
#define CC_LAYOUT_MN 1 /* operand stored with the M (or N) index contiguous      */

enum {
  CC_OK = 0,
  CC_ERR_NULL = 1,
  CC_ERR_DTYPE = 2,
  CC_ERR_SHAPE = 3,
  CC_ERR_ALIGN = 4,
  CC_ERR_TOO_LARGE = 5,
  CC_ERR_HIP_BASE = 1000
};

int cc_version(void);
const char* cc_strerror(int code);

/* Workspace sizing.  Column-partial slabs written by GEMM epilogues have
 * cc_col_part_rows(M) rows of N floats; per-wave scalar partials have cc_wave_parts(M, N)
 * floats.  Row-block slabs of the elementwise kernels: cc_prep_part_rows(B) x K and
 * cc_loss_part_rows(B) x K; loss row stats: 2 * n * cc_loss_col_blocks(d) x B. */
int64_t cc_col_part_rows(int64_t M);
int64_t cc_wave_parts(int64_t M, int64_t N);    /* encode (B, h) per-wave partial count       */
int64_t cc_wgrad_parts(int64_t h, int64_t K, int dtype); /* wgrad_dec / wgrad_enc per-wave partials */
int64_t cc_prep_part_rows(int64_t B);
int64_t cc_loss_part_rows(int64_t B);
int64_t cc_loss_col_blocks(int64_t d);
int64_t cc_loss_scalars_len(int64_t B); /* floats in the `scalars` buffer of cc_loss_finalize */

/* Generic MFMA GEMM, fp32 output: C[M,N] = sum_k A(m,k) B(k,n).
 * a_layout KC: A at A[m*lda+k]; MN: A at A[k*lda+m].  b_layout KC: B at B[n*ldb+k];
 * MN: B at B[k*ldb+n].  (Test/diagnostic entry; the fused entries below use the same kernel.)
 * An operand's contiguous dimension (K for KC; M for an MN A, N for an MN B) and lda / ldb are whole 16-byte
 * vectors (multiples of 8 in bf16, 4 in fp32), N % 4 == 0 and ldc % 4 == 0, else CC_ERR_SHAPE / CC_ERR_ALIGN:
 * M = 1 runs with a KC A only. */
int cc_gemm_f32out(const void* A, int a_layout, int64_t lda, const void* Bm, int b_layout, int64_t ldb,
                   float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int dtype, void* stream);

/* Buffer.next normalisation + CrossCoder.get_losses cast (buffer.py:115-124, crosscoder.py:99):
 * x_out[b, m*d+j] = dtype( float(x_in[b,m,j]) * float(factor[m]) ), factor may be NULL (=1).
 * in_dtype / factor_dtype in {CC_BF16, CC_F32}.  colsum_part (optional): per 64-row block
 * column sums of x_out -> reduced by cc_reduce_rows into x.mean(0) (crosscoder.py:112). */
int cc_prep_input(const void* x_in, int in_dtype, const void* factor, int factor_dtype, void* x_out,
                  float* colsum_part, int64_t B, int64_t n, int64_t d, int dtype, void* stream);
/* cc_prep_input that also stores x_t [n*d][B] = x_out^T (bf16 out, B % 8 == 0; x_t NULL -> cc_prep_input). */
int cc_prep_input_t(const void* x_in, int in_dtype, const void* factor, int factor_dtype, void* x_out, void* x_t,
                    float* colsum_part, int64_t B, int64_t n, int64_t d, int dtype, void* stream);

/* out[j] = scale * sum_{i<R} part[i*ld + j] (fixed order).  Optional: out_f32, out_t (dtype),
 * sq_part [cc_reduce_parts(C)] (per column block: sum of dtype-rounded out^2, for clip_grad_norm_),
 * dot_part [cc_reduce_parts(C)] (per column block: sum of out[j] * dot_w[j]; with out = the column
 * sums of acts and dot_w = the total decoder norms this is B * l1_loss, crosscoder.py:126). */
int cc_reduce_rows(const float* part, int64_t R, int64_t C, int64_t ld, float scale, float* out_f32,
                   void* out_t, int dtype, float* sq_part, const float* dot_w, float* dot_part, void* stream);
int64_t cc_reduce_parts(int64_t C);

/* W_dec.norm(dim=-1) and its sum over models (crosscoder.py:123-125):
 * norms[h*n + m] = ||W_dec[h,m,:]||_2, total[h] = sum_m norms, inv_norms (optional) = 1/norms
 * (0 where a norm is 0: the norm backward's masked value).  fp32 results. */
int cc_dec_norms(const void* W_dec, float* norms, float* total, float* inv_norms, int64_t h, int64_t n,
                 int64_t d, int dtype, void* stream);

/* CrossCoder.encode (crosscoder.py:69-80): acts[B,h] = act(x[B,K] . W_enc + b_enc), W_enc stored
 * h-major [h][K] (its physical layout, crosscoder.py:55-58).  act = ReLU if apply_relu.
 * Optional fused side outputs (NULL to skip), all from the dtype-rounded acts:
 *   colsum_part [cc_col_part_rows(B) x h]  column sums  (-> sum_b acts, for dL1/dW_dec)
 *   l1_part     [cc_wave_parts(B,h)]        sum acts*tn  (l1_loss numerator, crosscoder.py:126)
 *   l0_part     [cc_wave_parts(B,h)]        count acts>0 (l0_loss numerator, crosscoder.py:128) */
int cc_encode_fwd(const void* x, const void* W_enc, const void* b_enc, const float* tn, void* acts,
                  int apply_relu, float* colsum_part, float* l1_part, float* l0_part, int64_t B, int64_t K,
                  int64_t h, int dtype, void* stream);

/* A column reduction a GEMM launch can carry before its tiles -- cc_reduce_rows(part, rows, cols, ld, scale,
 * out_f32 = out) with the same bits -- so the step saves that launch: out[j] = scale * sum_{i<rows} part[i*ld + j]. */
typedef struct cc_colsum_job {
  const float* part;
  int64_t rows, cols, ld;
  float scale;
  float* out;
} cc_colsum_job;

/* 1 when cc_encode_fwd_t / cc_dacts_bwd_t / cc_wgrad_both_t serve a step of this shape and dtype. */
int cc_transposed_ok(int64_t B, int64_t K, int64_t h, int dtype);

/* cc_encode_fwd that also stores acts transposed, acts_t [h][B] (the batch-contiguous operand of
 * cc_wgrad_both_t).  bf16 with B, K, h % 8 == 0 (else CC_ERR_SHAPE).
 * mask_bits (optional, cc_mask_bits_words(B, h) u32): the activation mask (acts > 0) as 1 bit per element in
 * the GEMM's accumulator order, which cc_dacts_bwd_t reads instead of the acts tile (autograd of the ReLU,
 * crosscoder.py:77).
 * tile_ctr (optional): CC_TILE_CTR_WORDS u32, zero before the first launch that uses them and left zero by
 * every launch: the persistent launch then hands out its output tiles dynamically, per XCD, so workgroups
 * that start late (their CUs held by another stream's kernel) take fewer tiles; NULL: a static tile order.
 * The results are the same bits either way.  Launches sharing tile_ctr must be ordered (one stream).
 * pre (optional): a column reduction the launch runs first (the step: x.mean(0) from cc_prep_input_t's
 * column partials, crosscoder.py:112). */
#define CC_TILE_CTR_WORDS 8
int cc_encode_fwd_t(const void* x, const void* W_enc, const void* b_enc, const float* tn, void* acts, void* acts_t,
                    int apply_relu, float* colsum_part, float* l1_part, float* l0_part, uint32_t* mask_bits,
                    uint32_t* tile_ctr, const cc_colsum_job* pre, int64_t B, int64_t K, int64_t h, int dtype,
                    void* stream);

/* u32 words of cc_encode_fwd_t's mask_bits for a [B][h] activation (256 x 256 tiles x 512 threads x 4). */
int64_t cc_mask_bits_words(int64_t B, int64_t h);

/* CrossCoder.decode (crosscoder.py:82-89): recon = acts[B,h] . W_dec[h][K] (+ b_dec).
 * recon_f32 (optional): fp32 [B][K]; b_dec NULL -> partial sum without bias (latent-sharded use).
 * recon_t (optional): dtype [B][K] = dtype(acc + b_dec). */
int cc_decode_fwd(const void* acts, const void* W_dec, const void* b_dec, float* recon_f32, void* recon_t,
                  int64_t B, int64_t h, int64_t K, int dtype, void* stream);

/* cc_decode_fwd's fp32 partial reconstruction (no bias), scheduled for whole 256-tile waves: the
 * column blocks that fill whole waves run in one launch, the leftover tiles as S-way split-K passes
 * over caller workspace `ws` (cc_decode_ws_floats(B, h, K, dtype) floats; 0 = no split for this
 * shape, ws may then be NULL) summed in fixed order -- deterministic.  Same results as
 * cc_decode_fwd up to fp32 summation order in the leftover columns. */
int64_t cc_decode_ws_floats(int64_t B, int64_t h, int64_t K, int dtype);
int cc_decode_fwd_ws(const void* acts, const void* W_dec, float* recon_f32, float* ws, int64_t ws_floats, int64_t B,
                     int64_t h, int64_t K, int dtype, void* stream);

/* cc_decode_fwd_ws with W_dec given transposed, W_dec_t [K][h] (a copy the optimizer keeps, see
 * cc_adam_step_t): both operands then contract over h contiguously.  Same results. */
int cc_decode_fwd_ws_t(const void* acts, const void* W_dec_t, float* recon_f32, float* ws, int64_t ws_floats,
                       int64_t B, int64_t h, int64_t K, int dtype, void* stream);
/* cc_decode_fwd_ws (W_dec [h][K] read as stored) for the latent-sharded step's partial reconstruction
 * (crosscoder.py:82-89 without b_dec, summed over the ranks), carrying two small jobs so the step saves their
 * launches: pre (optional) -- a cc_colsum_job the launch runs before its tiles (the step's sum_b acts,
 * crosscoder.py:126, from G1's column partials) -- and, norm_part given, the decoder norms' finaliser
 * (cc_dec_norms_finalize(norm_part, h, n, d, norms, tn, inv_norms), d % 64 == 0) as extra blocks of the
 * split-K leftover's reduction launch.  recon_f32 bit-identical to cc_decode_fwd_ws; the jobs' outputs to
 * their stand-alone launches.  wait_ctr (optional, bf16): the launch first waits IN ITS KERNEL until
 * *wait_ctr - wait_target >= 0 (mod 2^32) -- the side-stream decoder-half Adam's done count, cc_adam_dec_norms --
 * instead of the stream waiting for that Adam's event, as cc_decode_loss does; past ~1 s it runs no tile and sets
 * *wait_err (host-visible), which the same step's cc_wgrad_both_sums_t (abort) turns into -inf squared sums. */
int cc_decode_partial(const void* acts, const void* W_dec, float* recon_f32, float* ws, int64_t ws_floats,
                      const float* norm_part, float* norms, float* tn, float* inv_norms, const cc_colsum_job* pre,
                      const uint32_t* wait_ctr, uint32_t wait_target, uint32_t* wait_err, int64_t B, int64_t h,
                      int64_t n, int64_t d, int dtype, void* stream);

/* get_losses reconstruction terms + their backward (crosscoder.py:104-121, autograd):
 * r = recon_f32 + b_dec; g_recon = dtype(grad_scale * (r - x)) with grad_scale = 2/B.
 * row_part [2][n*cc_loss_col_blocks(d)][B]: [0] sum (r-x)^2, [1] sum (x - x_mean)^2 per
 * (model, column block, row).  col_part [cc_loss_part_rows(B)][K]: column sums of g_recon. */
int cc_loss_fwd_bwd(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                    void* g_recon, float* row_part, float* col_part, float grad_scale, int64_t B, int64_t n,
                    int64_t d, int dtype, void* stream);
/* cc_loss_fwd_bwd over the batch rows [row0, row0 + rows) only (row0 % 32 == 0, row0 + rows <= B).
 * The slabs keep the whole-batch layout, so disjoint row ranges may be separate calls: the
 * latent-sharded step processes each batch slice as soon as its all-reduce has landed. */
int cc_loss_fwd_bwd_rows(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                         void* g_recon, float* row_part, float* col_part, float grad_scale, int64_t row0,
                         int64_t rows, int64_t B, int64_t n, int64_t d, int dtype, void* stream);
/* cc_loss_fwd_bwd_rows that also stores g_recon_t [n*d][B] = g_recon^T for its rows (bf16, B and rows
 * % 8 == 0; g_recon_t NULL -> cc_loss_fwd_bwd_rows). */
int cc_loss_fwd_bwd_rows_t(const float* recon_f32, const void* b_dec, const void* x, const float* x_mean,
                           void* g_recon, void* g_recon_t, float* row_part, float* col_part, float grad_scale,
                           int64_t row0, int64_t rows, int64_t B, int64_t n, int64_t d, int dtype, void* stream);

/* G2 + the reconstruction loss in one pass (crosscoder.py:82-89 then :104-121 and their autograd),
 * the fused form of cc_decode_fwd_ws_t + cc_loss_fwd_bwd_rows_t over all rows: the whole-contraction
 * tiles run the loss as their GEMM epilogue (the fp32 reconstruction never reaches HBM), the split-K
 * leftover columns are summed in cc_decode_fwd_ws's fixed order and then run the same arithmetic.
 * g_recon / g_recon_t are bit-identical to the two-call form; the partial slabs use other blocks:
 *   row_part [2][n * ncb][B], ncb = cc_decode_loss_ncb(..) = d / 64 column blocks per model
 *   col_part [cc_col_part_rows(B)][K] (column sums of g_recon per 128-row group)
 * so their sums agree to fp32 reassociation (cc_loss_tail / cc_loss_finalize_nb take ncb; the b_dec
 * gradient sums cc_col_part_rows(B) rows).  ws: cc_decode_ws_floats(B, h, n*d, dtype) floats.
 * bf16, B % 8 == 0, d % 64 == 0; cc_decode_loss_ncb returns 0 for shapes this entry does not serve. */
int64_t cc_decode_loss_ncb(int64_t B, int64_t h, int64_t n, int64_t d, int dtype);
int cc_decode_loss_t(const void* acts, const void* W_dec_t, const void* b_dec, const void* x, const float* x_mean,
                     float grad_scale, void* g_recon, void* g_recon_t, float* row_part, float* col_part, float* ws,
                     int64_t ws_floats, int64_t B, int64_t h, int64_t n, int64_t d, int dtype, void* stream);
/* cc_decode_loss_t reading W_dec [h][K] itself (the parameter, no transposed copy; same bits): the GEMM's B
 * operand goes through transposed LDS reads.  g_recon_t may be NULL here (not written then).
 * norm_part (optional, with norms / tn / inv_norms as in cc_dec_norms_finalize): the decoder norms'
 * finaliser rides in the launch of the split-K leftover (or runs right after the GEMM where the shape has
 * none) -- the same bits as cc_dec_norms_finalize(norm_part, h, n, d, norms, tn, inv_norms), ordered before
 * whatever the stream runs next (crosscoder.py:123-125 for the backward and the loss tail).
 * pre (optional): a column reduction the launch runs before its tiles (the step: sum_b acts from the
 * encoder's column partials, which G4 and the l1 loss read, crosscoder.py:126).
 * wait_ctr (optional): W_dec / b_dec / norm_part come from a producer on another stream (the decoder-half Adam,
 * cc_adam_dec_norms' done_ctr): every workgroup waits in the kernel, after `pre`, until
 * (int32_t)(*wait_ctr - wait_target) >= 0 instead of the stream waiting for an event.  A wait past ~1 s gives
 * up and sets *wait_err (host-visible memory, e.g. mapped pinned) -- the results are then invalid. */
int cc_decode_loss(const void* acts, const void* W_dec, const void* b_dec, const void* x, const float* x_mean,
                   float grad_scale, void* g_recon, void* g_recon_t, float* row_part, float* col_part, float* ws,
                   int64_t ws_floats, const float* norm_part, float* norms, float* tn, float* inv_norms,
                   const cc_colsum_job* pre, const uint32_t* wait_ctr, uint32_t wait_target, uint32_t* wait_err,
                   int64_t B, int64_t h, int64_t n, int64_t d, int dtype, void* stream);

/* Loss reduction (crosscoder.py:106-128, trainer.py:51-61): per-row explained variances
 * ev/ev_a/ev_b [B] (fp32) and scalars[0:8] = {l2, l1, l0, mean ev, mean ev_a, mean ev_b, 0, 0};
 * `scalars` holds cc_loss_scalars_len(B) floats (the tail is workspace).
 * l1_part [n_l1] / l0_part [n_l0]: partial sums of B * l1 (cc_reduce_rows dot_part, or the per-wave
 * partials of cc_encode_fwd) and of the active count (cc_encode_fwd), scaled by 1/B (NULL -> 0). */
int cc_loss_finalize(const float* row_part, const float* l1_part, int64_t n_l1, const float* l0_part, int64_t n_l0,
                     float* ev, float* ev_a, float* ev_b, float* scalars, float* l1l0_out, int64_t B, int64_t n,
                     int64_t d, void* stream);
/* (l1l0_out, optional: a second copy of scalars[1:3] -- the latent-sharded step all-reduces it) */
/* cc_loss_finalize that also writes scalars[0:8] to host_out[0:8] (mapped, coherent pinned host
 * memory, hipHostMallocMapped | hipHostMallocCoherent) and then, after a system-scope release,
 * the 32-bit word `seq` to host_out[8]: the host polls that word instead of a copy + event. */
int cc_loss_finalize_mapped(const float* row_part, const float* l1_part, int64_t n_l1, const float* l0_part,
                            int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars, float* l1l0_out,
                            float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, void* stream);

/* cc_loss_finalize_mapped over a row_part of `ncb` column blocks per model (the producer's layout:
 * cc_loss_col_blocks(d) for cc_loss_fwd_bwd*, cc_decode_loss_ncb for cc_decode_loss_t).  host_out may
 * be NULL. */
int cc_loss_finalize_nb(const float* row_part, int64_t ncb, const float* l1_part, int64_t n_l1,
                        const float* l0_part, int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars,
                        float* l1l0_out, float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, void* stream);

/* One launch for the forward's tail (crosscoder.py:106-128): the L1 dot partials
 * l1_part[j] = sum over the 64 latents of block j of colsum_acts * tn (colsum_acts [h] = sum_b acts,
 * formed by cc_reduce_rows from the encoder's column slab), the per-row EV terms of row_part (`ncb`
 * column blocks per model) and the loss scalars -- bit-identical to cc_reduce_rows(.., dot_w = tn,
 * dot_part = l1_part) followed by cc_loss_finalize_nb(.., n_l1 = cc_reduce_parts(h), ..).  Its
 * workgroups (256 threads, few registers, < 0.5 KB of LDS) fit beside a persistent GEMM launch's, so a
 * side stream can run it during the backward's first GEMM.  The last workgroup to finish runs the
 * scalar finaliser; `counter` is one device uint32, zero before the first call, left zero by every
 * call (launches sharing a counter must be ordered, e.g. one stream).  host_out may be NULL. */
int cc_loss_tail(const float* colsum_acts, const float* tn, int64_t h, float* l1_part, const float* row_part,
                 int64_t ncb, const float* l0_part, int64_t n_l0, float* ev, float* ev_a, float* ev_b, float* scalars,
                 float* l1l0_out, float* host_out, uint32_t seq, int64_t B, int64_t n, int64_t d, uint32_t* counter,
                 void* stream);

/* Backward through decode + L1 + ReLU (autograd of crosscoder.py:77,84-89,126):
 * g_pre[B,h] = (g_recon . W_dec^T + l1_scale * tn[h]) * (acts > 0),  l1_scale = l1_coeff / B.
 * colsum_part [cc_col_part_rows(B) x h]: column sums of g_pre (-> b_enc.grad). */
int cc_dacts_bwd(const void* g_recon, const void* W_dec, const void* acts, const float* tn, float l1_scale,
                 void* g_pre, float* colsum_part, int64_t B, int64_t K, int64_t h, int dtype, void* stream);

/* cc_dacts_bwd writing g_pre TRANSPOSED only: g_pre_t[j][b], row stride ldt >= B (a batch slice
 * [r0, r1) passes g_pre_t + r0 and B = r1 - r0).  bf16 with B, K, h, ldt % 8 == 0.
 * mask_bits (optional): cc_encode_fwd_t's mask bits of these rows (a slice starting at row r0, r0 % 256 == 0,
 * passes mask_bits + (r0 / 256) * cc_mask_bits_words(256, h)); used instead of reading the acts tile when
 * the shape takes the whole-tile form (B, h % 256 == 0), same bits.  tile_ctr: as cc_encode_fwd_t.
 * tail (optional): the forward's loss tail -- cc_loss_tail with these arguments, the same bits -- run by the
 * launch's first workgroups before their tiles (the last of them to finish runs the loss-scalar finaliser;
 * the tile counters then even out its late start). */
typedef struct cc_loss_tail_job {
  const float* colsum_acts;
  const float* tn;
  int64_t h;
  float* l1_part;
  const float* row_part;
  int64_t ncb;
  const float* l0_part;
  int64_t n_l0;
  float* ev;
  float* ev_a;
  float* ev_b;
  float* scalars;
  float* l1l0_out;
  float* host_out;
  uint32_t seq;
  int64_t B, n;
  uint32_t* counter;
} cc_loss_tail_job;
int cc_dacts_bwd_t(const void* g_recon, const void* W_dec, const void* acts, const float* tn, float l1_scale,
                   const uint32_t* mask_bits, void* g_pre_t, int64_t ldt, float* colsum_part, uint32_t* tile_ctr,
                   const cc_loss_tail_job* tail, int64_t B, int64_t K, int64_t h, int dtype, void* stream);

/* W_dec.grad [h][K] = acts^T . g_recon + l1_scale * sum_b(acts[:,h]) * W_dec[h,m,:]/||W_dec[h,m,:]||
 * (norm backward is 0 where the norm is 0; inv_norms from cc_dec_norms).
 * sq_part [cc_wgrad_parts(h,K,dtype)]: sum of grad^2. */
int cc_wgrad_dec(const void* acts, const void* g_recon, const void* W_dec, const float* inv_norms,
                 const float* colsum_acts, float l1_scale, void* grad_W_dec, float* sq_part, int64_t B,
                 int64_t h, int64_t n, int64_t d, int dtype, void* stream);

/* W_enc.grad, h-major [h][K] (the param's physical layout) = g_pre^T . x.  sq_part as above. */
int cc_wgrad_enc(const void* g_pre, const void* x, void* grad_W_enc, float* sq_part, int64_t B, int64_t h,
                 int64_t K, int dtype, void* stream);

/* cc_wgrad_dec and cc_wgrad_enc with the same arguments and results, as ONE launch when the
 * ping-pong GEMM serves them (bf16, K % 8 == 0): the two tile sets fill whole waves together
 * (2 x 1152 tiles = 9 x 256 CUs at config 2); otherwise two launches. */
int cc_wgrad_both(const void* acts, const void* g_recon, const void* W_dec, const float* inv_norms,
                  const float* colsum_acts, float l1_scale, void* grad_W_dec, float* sq_dec, const void* g_pre,
                  const void* x, void* grad_W_enc, float* sq_enc, int64_t B, int64_t h, int64_t n, int64_t d,
                  int dtype, void* stream);

/* cc_wgrad_both with the batch-major operands TRANSPOSED: actsT / g_preT [h][B], g_reconT / xT [K][B]
 * (the contraction index B contiguous), so both GEMMs read row-contiguous (KC) operand tiles.
 * Same outputs as cc_wgrad_both (same k order per output element). */
int cc_wgrad_both_t(const void* actsT, const void* g_reconT, const void* W_dec, const float* inv_norms,
                    const float* colsum_acts, float l1_scale, void* grad_W_dec, float* sq_dec, const void* g_preT,
                    const void* xT, void* grad_W_enc, float* sq_enc, int64_t B, int64_t h, int64_t n, int64_t d,
                    int dtype, void* stream);

/* clip_grad_norm_(params, max_norm) (trainer.py:46; torch/nn/utils/clip_grad.py): per-param
 * norms from the squared-sum partials sq[off[i] .. off[i+1]) (nparams <= 8, off on the HOST),
 * total = ||(norm_i)||, coef = min(1, max_norm / (total + 1e-6)).  emulate_bf16 = 1 rounds the
 * intermediate norms/coef to bf16 as torch does for bf16 grads; emulate_bf16 = 2 is torch on a MIXED list -- four bf16
 * gradients followed by fp32 ones (a bf16 JumpReLU crosscoder's threshold): the norms i < 4 are rounded to bf16, the
 * stacked norms (the fp32 ones first, as torch stacks that list), the total and the coefficient are fp32.
 * out[0] = coef, out[1] = total norm, out[2 + i] = norm_i  (fp32, device). */
int cc_clip_finalize(const float* sq, const int64_t* off, int nparams, float max_norm, int emulate_bf16,
                     float* out, void* stream);

/* One launch for the backward's tail (trainer.py:45-46): the bias gradients
 * g_b_enc [h] = sum of gpre_colpart [R_enc x h], g_b_dec [K] = sum of loss_colpart [R_dec x K] (param
 * dtype) with their squared-sum partials sq_b_enc / sq_b_dec [cc_reduce_parts(.)] (which must be the
 * segments 2 and 3 of sq), then cc_clip_finalize over sq -- bit-identical to the two cc_reduce_rows
 * launches + cc_clip_finalize.  counter: as cc_loss_tail. */
int cc_grad_tail(const float* gpre_colpart, int64_t R_enc, int64_t h, void* g_b_enc, float* sq_b_enc,
                 const float* loss_colpart, int64_t R_dec, int64_t K, void* g_b_dec, float* sq_b_dec, int dtype,
                 const float* sq, const int64_t* off, int nparams, float max_norm, int emulate_bf16, float* clip_out,
                 uint32_t* counter, void* stream);
/* The end of the single-GPU backward (trainer.py:45-46) as ONE launch: cc_wgrad_both_t (dW_dec, dW_enc
 * + their sq partials) and cc_grad_tail (bias gradients + sq partials, clip_grad_norm_'s coefficient
 * into clip_out) -- the bias sums run before the GEMM tiles, the clip finaliser in the last workgroup
 * to finish.  Same outputs as cc_wgrad_both_t followed by cc_grad_tail (the clip coefficient up to
 * the order of its fp64 squared-sum accumulation).  nparams must be 4 (sq's segments W_enc, W_dec, b_enc,
 * b_dec); tile_sum: fp32 scratch of cc_wgrad_tile_sums(h, n*d) floats (each output tile's squared sum, which
 * the last workgroup adds in a fixed order: the coefficient's bits do not depend on which workgroup ran which
 * tile) followed by 4 uint64 words the launch accumulates -- shader-clock ticks, 100 MHz ticks and the launch
 * count over the lifetime of its last workgroup (the clock the chip held; zero them to start a window); tile_ctr:
 * as cc_encode_fwd_t.  abort_flag (optional, host-mapped or device word): when nonzero at the clip finaliser, clip_out[0] is
 * written as -1 (CC_CLIP_ABORTED: clip_grad_norm_'s coefficient is never negative) and every cc_adam_step /
 * cc_adam_dec_norms launch that reads that coefficient leaves p, m, v untouched -- the step's update is not applied
 * (the single-GPU step passes the word its G2 launch sets when its in-kernel wait times out).  Where the ping-pong
 * GEMM does not serve the shape (or dtype != bf16) it runs exactly those two entries. */
int64_t cc_wgrad_tile_sums(int64_t h, int64_t K);
int cc_wgrad_both_clip_t(const void* actsT, const void* g_reconT, const void* W_dec, const float* inv_norms,
                         const float* colsum_acts, float l1_scale, void* grad_W_dec, float* sq_dec, const void* g_preT,
                         const void* xT, void* grad_W_enc, float* sq_enc, int64_t B, int64_t h, int64_t n, int64_t d,
                         const float* gpre_colpart, int64_t R_enc, void* g_b_enc, float* sq_b_enc,
                         const float* loss_colpart, int64_t R_dec, void* g_b_dec, float* sq_b_dec, const float* sq,
                         const int64_t* off, int nparams, float max_norm, int emulate_bf16, float* clip_out,
                         uint32_t* counter, float* tile_sum, uint32_t* tile_ctr, const uint32_t* abort_flag, int dtype,
                         void* stream);
/* cc_wgrad_both_clip_t whose finaliser is cc_segment_sums instead of the clip (the latent-sharded step,
 * trainer.py:45-46 split across ranks): out[p] = the per-parameter squared sums, 0 where bit p of
 * zero_mask is set, to be all-reduced.  Equal to cc_wgrad_both_t + cc_grad_tail_sums (the sums up to the
 * order of their fp64 accumulation), which it runs itself where the ping-pong GEMM does not serve.  abort
 * (optional): the step's abort word (cc_decode_partial's wait_err); when set, out[p] = -inf for every p, so the
 * all-reduced sums carry the abort to every rank and cc_adam_step_clip (a negative sum) applies nothing. */
int cc_wgrad_both_sums_t(const void* actsT, const void* g_reconT, const void* W_dec, const float* inv_norms,
                         const float* colsum_acts, float l1_scale, void* grad_W_dec, float* sq_dec, const void* g_preT,
                         const void* xT, void* grad_W_enc, float* sq_enc, int64_t B, int64_t h, int64_t n, int64_t d,
                         const float* gpre_colpart, int64_t R_enc, void* g_b_enc, float* sq_b_enc,
                         const float* loss_colpart, int64_t R_dec, void* g_b_dec, float* sq_b_dec, const float* sq,
                         const int64_t* off, int nparams, int zero_mask, float* out, uint32_t* counter, float* tile_sum,
                         uint32_t* tile_ctr, const uint32_t* abort, int dtype, void* stream);
/* cc_grad_tail whose finaliser is cc_segment_sums instead of the clip (the latent-sharded step:
 * out[p] = the per-parameter squared sums, 0 where bit p of zero_mask is set, to be all-reduced). */
int cc_grad_tail_sums(const float* gpre_colpart, int64_t R_enc, int64_t h, void* g_b_enc, float* sq_b_enc,
                      const float* loss_colpart, int64_t R_dec, int64_t K, void* g_b_dec, float* sq_b_dec, int dtype,
                      const float* sq, const int64_t* off, int nparams, int zero_mask, float* out, uint32_t* counter,
                      void* stream);

/* Per-parameter sums of the squared-gradient partials, sq[off[p] .. off[p+1]) (nparams <= 8, off on
 * the HOST), for the latent-sharded step's all-reduce: out[p] = the sum (fp32), or 0 where bit p of
 * zero_mask is set (a replicated parameter counted on one rank only). */
int cc_segment_sums(const float* sq, const int64_t* off, int nparams, int zero_mask, float* out, void* stream);

/* torch.optim.Adam step (trainer.py:16-20,47; torch/optim/adam.py single-tensor path, no weight
 * decay / amsgrad) fused with the clip multiply: g' = dtype(g * coef[0]); m, v, p updated in place
 * over `numel` flat elements; step = the Adam step count AFTER increment; lr from LambdaLR.
 * dtype-rounding between torch's ops is reproduced (bf16 state like the reference).
 * max_blocks > 0: grid-stride over at most that many 256-thread workgroups (for an update that
 * runs beside a GEMM on another stream); 0: one pass, one 8-element chunk per thread.
 * coef[0] < 0 (CC_CLIP_ABORTED, see cc_wgrad_both_clip_t): nothing is updated (a done count still arrives). */
int cc_adam_step(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, double lr,
                 double beta1, double beta2, double eps, int64_t step, int64_t max_blocks, int dtype, void* stream);

/* A cc_prep_input_t(x_in, in_dtype, factor, factor_dtype, x_out, x_t, colsum_part, B, n, d, CC_BF16) that an Adam
 * launch carries in its first workgroups (cc_adam_step_prep): the NEXT batch's x, x^T and column-sum partials,
 * which depend on nothing the step computes.  x_t is required; the same bits as the launch of its own. */
typedef struct cc_prep_job {
  const void* x_in;
  int in_dtype;
  const void* factor; /* NULL: 1 */
  int factor_dtype;
  void* x_out;
  void* x_t;
  float* colsum_part; /* optional */
  int64_t B, n, d;
} cc_prep_job;

/* cc_adam_step(..., max_blocks = 0, ...) in its one-pass form whose launch also runs `prep` (NULL: cc_adam_step
 * itself): bf16, numel % 8 == 0.  The same bits as cc_adam_step followed by cc_prep_input_t, one launch fewer:
 * the step's encoder-half Adam carries the next step's prep.  coef[0] < 0 (CC_CLIP_ABORTED): no update; the
 * prep still runs. */
int cc_adam_step_prep(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, double lr,
                      double beta1, double beta2, double eps, int64_t step, int dtype, const cc_prep_job* prep,
                      void* stream);

/* cc_adam_step with clip_grad_norm_'s coefficient formed in the kernel from the per-parameter squared
 * gradient sums `sums` [nparams] (trainer.py:46 over parameters whose sums were combined elsewhere, e.g.
 * all-reduced over the latent shards): the arithmetic of cc_clip_finalize over one element per parameter.
 * clip_out (optional): [coef, total norm, per-parameter norms] as cc_clip_finalize writes them.  A negative
 * sum (an aborted step's -inf, cc_wgrad_both_sums_t's abort) makes the coefficient CC_CLIP_ABORTED: nothing is
 * updated. */
int cc_adam_step_clip(void* p, const void* g, void* m, void* v, int64_t numel, const float* sums, int nparams,
                      float max_norm, int emulate_bf16, float* clip_out, double lr, double beta1, double beta2,
                      double eps, int64_t step, int64_t max_blocks, int dtype, void* stream);

/* The Adam step of a bf16 crosscoder trained with fp32 master weights (cfg["master_weights"]): g16 is the step's
 * bf16 gradient, p32 / m32 / v32 the fp32 masters and moments, all `numel` flat elements.  p32 / m32 / v32 are
 * updated in place with the bits of cc_adam_step(p32, float(g16), m32, v32, ..., CC_F32); p16 (bf16, the parameter
 * arena the GEMMs read) receives p32 rounded to nearest even.  max_blocks as cc_adam_step's (0: one 8-element chunk
 * per thread; > 0: grid-stride over at most that many workgroups, no LDS, for the launch beside a GEMM).  Any
 * numel (the last numel % 8 elements are updated one per thread).  coef NULL: 1.  coef[0] < 0 (CC_CLIP_ABORTED):
 * p16, p32, m32 and v32 stay untouched.  All five pointers 16-byte aligned. */
int cc_adam_master_step(void* p32, const void* g16, void* m32, void* v32, void* p16, int64_t numel, const float* coef,
                        double lr, double beta1, double beta2, double eps, int64_t step, int64_t max_blocks,
                        void* stream);

/* ---- around the step ---- */

/* Buffer.refresh's shuffle (buffer.py:111-113: buffer = buffer[randperm(rows)]): dst[i] = src[perm[i]]
 * for `rows` rows of `row_bytes` bytes (multiple of 16); perm: int64 device array (an index outside
 * [0, src_rows) gives a zero row).  dst must not overlap src. */
/* dst[c][r] = src[r][c] for 16-bit elements: src [rows][ld_src], dst [cols][ld_dst];
 * rows, cols, ld_src, ld_dst % 8 == 0.  (The step's batch-contiguous copies x^T and g_recon^T.) */
int cc_transpose_b16(const void* src, int64_t rows, int64_t cols, int64_t ld_src, void* dst, int64_t ld_dst,
                     void* stream);

/* W_dec_t [K][h] = W_dec^T plus the decoder norms of cc_dec_norms (same bits) from the same pass
 * over W_dec [h][K] (bf16; d % 64 == 0, h % 8 == 0).  part: cc_dec_norms_part_floats(h, n, d)
 * floats of workspace (per-row, per-64-column-block squared sums). */
int64_t cc_dec_norms_part_floats(int64_t h, int64_t n, int64_t d);
int cc_transpose_dec_norms(const void* W_dec, int64_t h, int64_t n, int64_t d, void* W_dec_t, float* part,
                           float* norms, float* total, float* inv_norms, void* stream);

/* The rest of cc_dec_norms from per-(row, 64-column block) squared sums (cc_adam_dec_transposed). */
int cc_dec_norms_finalize(const float* part, int64_t h, int64_t n, int64_t d, float* norms, float* total,
                          float* inv_norms, void* stream);

/* cc_adam_step over the decoder matrix W_dec [h][K] only (p/g/m/v point at W_dec in each arena; same
 * bits as cc_adam_step), in 64 x 64 tiles that also write W_dec_t = the updated W_dec^T and `part`
 * (cc_dec_norms_part_floats floats) for cc_dec_norms_finalize: the next step's decoder norms and G2
 * operand from the same HBM pass.  bf16, K % 64 == 0, h % 8 == 0; max_blocks caps the grid. */
/* The decoder half of Adam (trainer.py:47 over W_dec and b_dec: p/g/m/v point at the decoder half of each
 * arena, numel elements, W_dec [h][K] first; same bits as cc_adam_step / cc_adam_step_clip) that also writes
 * `part` (cc_dec_norms_part_floats(h, n, d) floats) from the updated W_dec for cc_dec_norms_finalize: the next
 * step's decoder norms (crosscoder.py:123-125, same bits as cc_dec_norms) without another pass over W_dec.
 * The clip coefficient comes from `coef`, or (sums != NULL) is formed from the per-parameter squared sums as
 * in cc_adam_step_clip.  K % 64 == 0; max_blocks caps the grid (0: 1024).
 * done_ctr (optional, max_blocks > 0): each of the launch's cc_adam_capped_blocks(numel, max_blocks)
 * workgroups adds 1 to *done_ctr once its stores are released (agent scope): the count a cc_decode_loss
 * launch on another stream waits for (wait_ctr / wait_target). */
int cc_adam_dec_norms(void* p, const void* g, void* m, void* v, int64_t numel, const float* coef, const float* sums,
                      int nparams, float max_norm, int emulate_bf16, double lr, double beta1, double beta2,
                      double eps, int64_t step, int64_t max_blocks, float* part, int64_t h, int64_t K, int dtype,
                      uint32_t* done_ctr, void* stream);
/* Workgroups of the capped-grid Adam launch (max_blocks > 0) over numel elements. */
int64_t cc_adam_capped_blocks(int64_t numel, int64_t max_blocks);

int cc_adam_dec_transposed(void* p, const void* g, void* m, void* v, int64_t h, int64_t K, const float* coef,
                           double lr, double beta1, double beta2, double eps, int64_t step, int64_t max_blocks,
                           void* W_dec_t, float* part, int dtype, void* stream);

int cc_gather_rows(const void* src, int64_t src_rows, const int64_t* perm, void* dst, int64_t rows,
                   int64_t row_bytes, void* stream);

/* fold_activation_scaling_factor (Crosscoder_model_diff.ipynb:35368-35378), in place:
 * W_enc[m] *= scale[m], W_dec[:, m] /= scale[m], b_dec[m] /= scale[m] (W_dec / b_dec may be NULL), each op
 * rounded to the parameter dtype like torch.  W_enc / W_dec in their [h][n*d] physical layout;
 * scale: n fp32 device values. */
int cc_fold_scaling(void* W_enc, void* W_dec, void* b_dec, const float* scale, int64_t h, int64_t n, int64_t d,
                    int dtype, void* stream);

/* Decoder-norm analytics (analysis.py:9-12,40), one pass over W_dec [h][n][d]:
 * norms[h*n + m] = ||W_dec[h,m]||; relative[h] = norms[h,1] / sum_m norms[h,m] (optional);
 * cosine[h] = <W_dec[h,0], W_dec[h,1]> / (norms[h,0] norms[h,1]) (optional).  fp32 outputs. */
int cc_decoder_stats(const void* W_dec, int64_t h, int64_t n, int64_t d, int dtype, float* norms, float* relative,
                     float* cosine, void* stream);

/* Per-latent activation statistics (the notebook's latent dashboards), one pass over acts [B][ld]
 * (h <= ld, ld even; the layout cc_encode_fwd and the step write; acts aligned to one
 * column pair: 4 bytes bf16, 8 bytes fp32), folded into
 * caller-owned state for latents 0..h-1 that persists across calls.  Only elements > 0 take part
 * (negative pre-activations and NaN are ignored).
 *   count[h] (int64) += rows with a positive value;  sum[h] (fp32) += the batch's fp32 sum of them (a
 *   summation order fixed by (B, h) and by whether k <= 4);  hist[h][32] (int64, optional) += a log2 histogram, bin =
 *   clamp(floor(log2 v) + 16, 0, 31) from the exponent field;  topk_val[h][k] (fp32) / topk_row[h][k] (int64),
 *   1 <= k <= cc_latent_stats_max_k(): the k largest values seen so far with their row ids, sorted by value
 *   descending, ties by row id ascending -- exactly the first k of all candidates sorted that way, in
 *   whatever order the batches arrive; unused slots are (0, -1), which is also the initial state (count,
 *   sum and hist start at 0).  Row b of the batch has id row_ids[b] (int64 [B]) if row_ids != NULL, else
 *   row0 + b.  No global atomics; results are bit-reproducible.
 * CC_ERR_SHAPE: k out of range, ld < h, ld odd, B < 1, h < 1. */
int cc_latent_stats_max_k(void);
int cc_latent_stats_update(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const int64_t* row_ids,
                           int64_t row0, int k, int64_t* count, float* sum, int64_t* hist, float* topk_val,
                           int64_t* topk_row, void* stream);

/* Latent scaling's accumulators (crosscoder_amd.LatentScaling): per latent j, over the batch rows i,
 *   dot[j] = sum_i acts[i][j] * (W[j][:] . Y[i][:])   and, optionally,   sq[j] = sum_i acts[i][j]^2
 * as one GEMM whose [B][h] product is never stored: the epilogue multiplies the fp32 accumulator by the acts tile
 * and writes only its column sums per 128-row group.
 *   Y [B][ldy], W [h][ldw]: the contraction index d contiguous (the operand geometry of cc_dacts_bwd); one model's
 *     slice of a [.., n*d] matrix is passed as pointer + m*d with ld = n*d.   acts [B][lda], lda >= h.
 *   dot_part [cc_col_part_rows(B)][h] (fp32, dense), sq_part the same shape or NULL: cc_reduce_rows over their
 *     cc_col_part_rows(B) rows gives dot / sq.  Nothing else is written.
 * Any B >= 1; d % 8 == 0, h % 4 == 0, ldy >= d, ldw >= d, lda >= h (else CC_ERR_SHAPE); every operand pointer and
 * row pitch (ld * element size) 16-byte aligned (else CC_ERR_ALIGN); 256 rows of an operand within 2 GiB (else
 * CC_ERR_TOO_LARGE).  No float atomics: the same inputs give the same bits. */
int cc_latent_scaling(const void* Y, int64_t ldy, const void* W, int64_t ldw, const void* acts, int64_t lda,
                      float* dot_part, float* sq_part, int64_t B, int64_t d, int64_t h, int dtype, void* stream);

/* Decoder matching (crosscoder_amd.match_decoders): for every query row j of Wq, the candidate row of Wc with the
 * largest cosine, as one GEMM whose [M][N] similarity matrix is never stored.  Per output (i, j) the epilogue forms
 *   s = (acc[i][j] * q_scale[j]) * c_scale[row0 + i] + 0.0f        (fp32, that order; -0 becomes +0)
 * and keeps per query and 128-row group the best pair as a 64-bit key: high word = the bits b of s mapped to unsigned
 * order (b ^ 0xffffffff if the sign bit is set, b ^ 0x80000000 otherwise), low word = ~(row0 + i).  The unsigned max of
 * two keys is the larger score and, on equal scores, the smaller candidate index; key 0 = no candidate.  Scores are
 * assumed finite (finite operands and scales); a NaN score would be ordered by its bits.
 *   Wc [M][ldc]: this launch's M candidates, global indices row0 .. row0 + M - 1;  Wq [N][ldq]: the queries; the
 *     contraction index K contiguous in both; one model's slice of a [.., n*d] matrix is pointer + m*d with ld = n*d.
 *   c_scale [>= row0 + M], q_scale [N]: fp32 inverse norms, 0 where the norm is 0.  c_scale is the whole candidate
 *     set's vector (indexed by the global index), q_scale 16-byte aligned.
 *   key_part [cc_col_part_rows(M)][N] (dense): every element is written.
 * A candidate gives no key if c_scale[row0 + i] == 0, or if exclude_diag != 0 and row0 + i == j; rows past M never do.
 * cc_match_reduce folds a slab into the running state: best[j] = max(best[j], max_r part[r][j]) over R rows, N
 * columns; best [N] in/out (zero = nothing seen yet).  An integer max: any chunking of the candidates and any slab
 * row order give the same bits.
 * Any M >= 1; K % 8 == 0, N % 4 == 0, ldc >= K, ldq >= K, row0 >= 0 (else CC_ERR_SHAPE); Wc, Wq, q_scale, key_part and
 * the row pitches 16-byte aligned, c_scale 4-byte, part / best 8-byte (else CC_ERR_ALIGN); 256 rows of an operand within
 * 2 GiB and row0 + M < 2^32 (else CC_ERR_TOO_LARGE). */
int cc_decoder_match(const void* Wc, int64_t ldc, const void* Wq, int64_t ldq, const float* c_scale,
                     const float* q_scale, uint64_t* key_part, int64_t M, int64_t N, int64_t K, int64_t row0,
                     int exclude_diag, int dtype, void* stream);
int cc_match_reduce(const uint64_t* part, int64_t R, int64_t N, uint64_t* best, void* stream);

/* Per-row top-k of the activations (TopK crosscoders), one pass over acts [B][ld], first h columns
 * (1 <= k <= h <= 2^17, h % 8 == 0, ld % 8 == 0, ld >= h; acts 16-byte aligned).
 * An element is eligible iff it is > 0: sign clear, not zero, not NaN; +inf and subnormals are eligible, so the
 * output of cc_encode_fwd with apply_relu = 0 is legal input and zero padding latents are never selected.
 * Order: larger value first, among equal values the smaller latent index first (a strict total order); the
 * selected set of a row is its first min(k, #eligible) elements under that order.
 * Outputs, each optional (NULL to skip; idx_out and val_out go together):
 *   acts_out [B][ld]  selected elements keep their exact bits, the other of the h columns become +0; columns
 *                     >= h are not touched.  acts_out may be acts (in place).
 *   idx_out [B][k] (int32), val_out [B][k] (dtype): the selected pairs in ascending latent index, padded with
 *                     (-1, 0) where fewer than k are eligible.
 *   colsum_part [cc_topk_part_rows(B, h)][h] (fp32, 16-byte aligned): column-sum partials of the masked
 *                     activations; cc_reduce_rows over them gives sum_b acts.
 *   l0_part [cc_topk_l0_parts(B, h)] (fp32): selected counts per workgroup (exact integers below 2^24).
 * No float atomics: two calls on the same input give the same bits in every output.
 * CC_ERR_SHAPE: k < 1, k > h, h or ld not a multiple of 8, ld < h, B < 1;  CC_ERR_TOO_LARGE: h > 2^17. */
int64_t cc_topk_part_rows(int64_t B, int64_t h);
int64_t cc_topk_l0_parts(int64_t B, int64_t h);
int cc_topk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k, void* acts_out,
                 int32_t* idx_out, void* val_out, float* colsum_part, float* l0_part, void* stream);

/* BatchTopK selection (BatchTopK crosscoders): the n_keep best (row, latent) pairs of the whole batch, over
 * acts [B][ld], first h columns (h % 8 == 0, ld % 8 == 0, ld >= h, h <= 2^17, B * h <= 2^31, n_keep >= 1; acts,
 * acts_out, colsum_part and weight 16-byte aligned).
 * Score: weight == NULL: float(a).  Else the fp32 product float(a) * weight[l] (weight fp32 [h]; one IEEE multiply,
 * round to nearest).
 * Eligible: the activation is > 0 and the score is > 0, both on their bits (sign clear, not zero, not NaN; +inf
 * and subnormals count, the rule of cc_topk_rows).  So a positive activation whose product is 0 (a zero weight, an
 * underflow) is ineligible, and so is every element under a negative or NaN weight.
 * Order: larger score first, among equal scores the smaller flat index row * h + latent first (a strict total
 * order); selected are the first min(n_keep, #eligible) elements under it.
 * Outputs, each optional (NULL to skip), at least one of acts_out, info, row_count given:
 *   acts_out [B][ld]  selected elements keep their own activation bits, the other of the h columns become +0;
 *                     columns >= h are not touched.  acts_out may be acts (in place).
 *   colsum_part [cc_batch_topk_part_rows(B, h)][h] (fp32): column-sum partials of the masked activations;
 *                     cc_reduce_rows over them gives sum_b acts.
 *   l0_part [cc_batch_topk_l0_parts(B, h)] (fp32): selected counts per workgroup (exact integers below 2^24).
 *   row_count [B] (int32): the selected count of every row.
 *   info [4] (uint32): the fp32 bits of the threshold score T (the smallest selected score; 0 when nothing is
 *                     selected), the number selected, the number of elements with score T that were admitted, the
 *                     number eligible.
 *   threshold_ema (one fp32 on the device, with 0 <= beta < 1): the running threshold, updated by the launch that
 *                     writes info when something is selected: T if *threshold_ema < 0 (unset), else
 *                     beta * *threshold_ema + (1 - beta) * T.
 * ws: cc_batch_topk_ws_bytes(B, h, dtype, weight != NULL) bytes of device memory (4-byte aligned, any content: the
 * call zeroes what it needs); ws_bytes: its size.  A radix select in separate launches on `stream` (histogram
 * passes from the top digit -- two for unweighted bf16, else three -- then one mask pass); integer atomics only,
 * no float atomics: two calls on the same input give the same bits in every output.
 * cc_threshold_mask: the inference form, one pass: keeps an element iff it is eligible and score >= *theta (theta:
 * device pointer to one fp32; NaN keeps nothing); the same outputs without info, at least one of acts_out and
 * row_count given.
 * Errors, checked in this order before any launch: CC_ERR_SHAPE (B < 1, h < 8, h or ld not a multiple of 8, ld < h,
 * n_keep < 1, beta outside [0, 1) with threshold_ema given), CC_ERR_NULL (acts, ws / theta, or no output),
 * CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h > 2^17, B * h > 2^31), CC_ERR_ALIGN (16 bytes: acts, acts_out, colsum_part,
 * weight; 4 bytes: the rest); then CC_ERR_SHAPE for a ws_bytes below the size needed. */
int64_t cc_batch_topk_part_rows(int64_t B, int64_t h);
int64_t cc_batch_topk_l0_parts(int64_t B, int64_t h);
int64_t cc_batch_topk_ws_bytes(int64_t B, int64_t h, int dtype, int weighted);
int cc_batch_topk(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* weight, int64_t n_keep,
                  void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count, uint32_t* info,
                  float* threshold_ema, float beta, void* ws, int64_t ws_bytes, void* stream);
int cc_threshold_mask(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* weight,
                      const float* theta, void* acts_out, float* colsum_part, float* l0_part, int32_t* row_count,
                      void* stream);

/* ---- the AuxK dead-latent loss (TopK / BatchTopK training; Gao et al.'s auxiliary loss) ----
 * since_fired [h] (int64, device): tokens since each latent last fired.  A latent is dead iff its count is
 * >= dead_after.
 *
 * cc_auxk_rows: cc_topk_rows with a column predicate -- an element's key is 0 (ineligible) unless
 * since_fired[latent] >= dead_after; otherwise the same eligibility (> 0 on the bits), the same order (larger first,
 * ties to the smaller latent) and the same limits.  aux_out [B][ld] (must not be acts): each row's first
 * min(k_aux, #eligible dead) elements keep their bits, the other of the h columns become +0; columns >= h are not
 * touched; acts is not modified.  row_count (optional, int32 [B]): every row's selected count.  With every latent
 * dead aux_out has the bits of cc_topk_rows' acts_out for k = k_aux.  No float atomics, bit-reproducible.
 * Errors in cc_topk_rows' order: CC_ERR_SHAPE (k_aux < 1, k_aux > h, h or ld not a multiple of 8, ld < h, B < 1),
 * CC_ERR_NULL (acts, since_fired or aux_out missing, aux_out == acts), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h > 2^17),
 * CC_ERR_ALIGN (16 bytes: acts, aux_out; 8: since_fired; 4: row_count). */
int cc_auxk_rows(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, int k_aux, const int64_t* since_fired,
                 int64_t dead_after, void* aux_out, int32_t* row_count, void* stream);

/* After a step's column sums of the masked activations exist (colsum_acts [h] fp32: a latent fired in the step iff
 * its entry is > 0, positive terms cannot cancel): since_fired[l] = fired ? 0 : since_fired[l] + B for l < h, and
 * *count_out (device int32) = the number of latents l < h_real that are dead under the NEW state (the padding
 * latents h_real..h-1 never fire and are not counted).  was_dead (optional, uint8 [h]): 1 where the latent was
 * dead under the OLD state (the dead set the step's cc_auxk_rows used).  host_out (optional): one int32 word of
 * host-visible memory (e.g. mapped pinned) that also receives the count, released at system scope.  One small
 * launch (one workgroup, a fixed-order block reduction).  h <= 2^17. */
int cc_dead_update(const float* colsum_acts, int64_t* since_fired, int64_t h, int64_t h_real, int64_t B,
                   int64_t dead_after, uint8_t* was_dead, int32_t* count_out, int32_t* host_out, void* stream);

/* The aux loss and its gradient w.r.t. the aux reconstruction.  With r = recon_f32 + b_dec (the main
 * reconstruction, fp32 [B][K] and dtype [K]), e = x - r (a constant) and ehat_f32 = aux_acts . W_dec (fp32 [B][K],
 * no bias):  num = (1/B) sum (ehat - e)^2,  den = (1/B) sum (e - mean_b e)^2 formed as
 * (sum e^2 - sum_k colsum_k^2 / B) / B,  auxk_loss = num / den, forced to 0 when den is not > 0 or the quotient is
 * not finite.  scalars [4] (fp32, device) = {auxk_loss, den, scale, valid} with scale = 2 auxk_coeff / (B den)
 * (0 when forced); host_out (optional): one fp32 word of host-visible memory that also receives auxk_loss.
 * g_aux [B][K] (dtype) = dtype(scale * (ehat - e)), all +0 when the loss was forced to 0.
 * Four launches on `stream`: a pass writing per-row-block partial slabs (column sums of e, sum (ehat - e)^2,
 * sum e^2) into `part` (cc_auxk_part_floats(B, K) floats), the squared column sums and a one-workgroup finaliser
 * in fp64, and the g_aux pass reading the device-resident scale: fixed order, no float atomics, no host read.
 * K % 8 == 0. */
int64_t cc_auxk_part_floats(int64_t B, int64_t K);
int cc_auxk_loss(const float* recon_f32, const void* b_dec, const void* x, const float* ehat_f32, void* g_aux,
                 float* part, float* scalars, float* host_out, float auxk_coeff, int64_t B, int64_t K, int dtype,
                 void* stream);

/* dst[r][c] = dtype(float(dst[r][c]) + float(src[r][c])) over rows x cols elements of two [rows][ld] buffers
 * (cols, ld % 8 == 0; 16-byte aligned; dst and src distinct): folds the aux half of g_pre into the main half. */
int cc_add_rows(void* dst, const void* src, int64_t rows, int64_t cols, int64_t ld, int dtype, void* stream);

/* ---- JumpReLU crosscoders: f = a * H(a - theta[latent]), one learned fp32 threshold per latent, trained through
 * straight-through estimators of bandwidth eps (Rajamanoharan et al. 2024) ----
 * a is an activation as cc_encode_fwd (apply_relu = 1) stores it, theta fp32 [h], eps > 0 finite, half = 0.5f * eps,
 * d = float(a) - theta[l] (one fp32 subtract).  "a > 0" is cc_topk_rows' rule on the element's bits: sign clear, not
 * zero, not NaN; +inf and subnormals count.
 *
 * cc_jumprelu_mask, one pass over acts [B][ld], first h columns (h % 8 == 0, ld % 8 == 0, ld >= h, h <= 2^17,
 * B * h <= 2^31):
 *   acts_out [B][ld]  an element keeps its bits iff a > 0 and float(a) > theta[l] (strictly), else +0; columns >= h
 *                     are not touched.  acts_out may be acts (in place).  theta[l] <= 0 is plain ReLU for latent l.
 *   gate_out [B][ld]  (optional; not acts) an element keeps its bits iff a > 0 and d > -half: the kept elements plus
 *                     the lower half of the straight-through window (a > 0 and -half < d < half).  It is what
 *                     cc_dacts_bwd masks with in place of acts.  Columns >= h are not touched.
 *   colsum_part [cc_jumprelu_part_rows(B, h)][h] (optional, fp32): column-sum partials of the kept activations;
 *                     cc_reduce_rows over them gives sum_b acts.
 *   l0_part [cc_jumprelu_l0_parts(B, h)] (optional, fp32): kept counts per workgroup (exact integers below 2^24).
 * cc_jumprelu_bwd, one pass over g_pre [B][ld] (in/out) and gate [B][ld] (cc_jumprelu_mask's), where g_pre is
 * cc_dacts_bwd's output under the gate, G = dL/d acts (dtype-rounded) at gated elements:
 *   thr_part [cc_jumprelu_part_rows(B, h)][h] (optional, fp32): partial sums over the window's elements of
 *                     -(theta[l] / eps) * G - l0_scale / eps (formed in fp64, rounded once), l0_scale = l0_coeff / B;
 *                     cc_reduce_rows over them gives theta.grad of l2 + l1_coeff l1 + l0_coeff l0.
 *   g_pre             elements that are gated but not kept become +0 (the straight-through g_pre of the four
 *                     reference parameters); nothing else is written.
 *   gpre_colsum_part [cc_jumprelu_part_rows(B, h)][h] (optional, fp32): column-sum partials of the resulting g_pre
 *                     (-> b_enc.grad; cc_dacts_bwd's own include the gated elements that were dropped).
 * Streaming kernels in a fixed summation order, no float atomics: two calls on the same input give the same bits in
 * every output.  Errors, checked in cc_topk_rows' order before any launch: CC_ERR_SHAPE (B < 1, h < 8, h or ld not
 * a multiple of 8, ld < h, eps not a finite float > 0), CC_ERR_NULL (acts, theta or acts_out missing; g_pre, gate or
 * theta missing, g_pre == gate), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h > 2^17, B * h > 2^31), CC_ERR_ALIGN (16 bytes:
 * every [B][ld] buffer, theta and the slabs; 4 bytes: l0_part). */
int64_t cc_jumprelu_part_rows(int64_t B, int64_t h);
int64_t cc_jumprelu_l0_parts(int64_t B, int64_t h);
int cc_jumprelu_mask(const void* acts, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta, float eps,
                     void* acts_out, void* gate_out, float* colsum_part, float* l0_part, void* stream);
int cc_jumprelu_bwd(void* g_pre, const void* gate, int64_t ld, int64_t B, int64_t h, int dtype, const float* theta,
                    float eps, float l0_scale, float* gpre_colsum_part, float* thr_part, void* stream);

/* ---- Sparse decode from (value, latent) pairs: the consumer of cc_topk_rows' idx_out / val_out (CrossCoder.decode_pairs,
 * pairs_sq_err, LatentAblation).  A whole-row gather of W_dec plus one fp32 fma chain per output element; no [B][h]
 * activation matrix is formed.  K = n * d.
 *   val [B][k] (dtype), idx [B][k] (int32), both dense;  W_dec [h][ldw], b_dec [K], x [B][ldx], recon [B][ldr] (dtype);
 *   sq_err [B][n] (fp32).
 * For row r, column c:  acc = float(b_dec[c]);  for slots s = 0 .. k-1 in that order, if 0 <= idx[r][s] < h:
 *   acc = fmaf(float(val[r][s]), float(W_dec[idx[r][s]][c]), acc).
 * A slot whose index is outside [0, h) (the -1 padding or anything else; one unsigned compare) adds nothing and its
 * W_dec row is not read; duplicate indices add twice; a row with no valid slot gives b_dec's bits.
 *   recon[r][c] = dtype(acc), one round-to-nearest-even.  (bf16: a product of two bf16 values is exact in fp32, so
 *   the chain is a plain fp32 multiply-add loop.)
 *   sq_err[r][m] = sum over c in [m d, (m+1) d) of (float(dtype(acc)) - float(x[r][c]))^2 in fp32, in an order fixed
 *   by (K, d) alone (lanes, waves and LDS in lane order; no float atomics): two calls give the same bits, and the
 *   same bits whether or not recon is written.
 * recon and (x, sq_err) are each optional (NULL), at least one given; x and sq_err go together; recon != x.
 * Errors, checked in this order before any launch: CC_ERR_SHAPE (B, k, h or n < 1, d < 8 or d % 8 != 0, ldw < K, a
 * given recon's ldr < K, a given x's ldx < K), CC_ERR_NULL (val, idx, W_dec or b_dec missing, neither output, one of
 * x / sq_err without the other, recon == x), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h or K > 2^31 - 1, k > 2^17),
 * CC_ERR_ALIGN (16 bytes: W_dec, b_dec, x, recon and their row pitches; 4 bytes: idx, sq_err; val: its element). */
int cc_decode_pairs(const void* val, const int32_t* idx, int64_t B, int k, const void* W_dec, int64_t ldw, int64_t h,
                    const void* b_dec, int64_t n, int64_t d, int dtype, void* recon, int64_t ldr, const void* x,
                    int64_t ldx, float* sq_err, void* stream);

/* ---- Dead-latent resampling (LatentResampler; Anthropic's neuron resampling for L1 dictionaries): a dead latent is
 * re-seeded from an input the dictionary reconstructs badly.  No float atomics, no spin waits, fixed summation orders:
 * two calls on the same input give the same bits in every output.
 *
 * cc_row_norms: out[r] (fp32) = sqrt(sum_c float(W[r][c])^2) for a [rows][K] matrix of row pitch ld (elements), one
 * pass, no copy of W.  A lane folds its columns' squares into one fp32 fma chain (8 consecutive columns of every
 * 512-column chunk, chunk after chunk), the wave's 64 sums meet in an xor butterfly: at most 8 ceil(K / 512) + 6
 * roundings on any path.  Serves W_enc and W_dec alike (both [h][K]).
 * Errors in this order: CC_ERR_SHAPE (rows < 1, K < 8, K % 8 != 0, ld < K), CC_ERR_NULL, CC_ERR_DTYPE,
 * CC_ERR_TOO_LARGE (rows or K > 2^31 - 1), CC_ERR_ALIGN (W and its pitch 16 bytes, out 4).
 *
 * cc_resample_pick: J draws, with replacement, of a row of loss [R] (fp32) with probability proportional to
 * w_r = (double)loss_r^2; a loss that is negative (sign set) or not finite has weight 0.
 *   cdf [R] (fp64, caller scratch) receives the inclusive prefix sum of w, formed so that it is non-decreasing and an
 *   element of weight 0 has its predecessor's bits (cdf[0] = +0 for w_0 = 0): a lane adds 16 consecutive weights one
 *   after the other, one thread the 256 lane totals of a 4096-row chunk one after the other, one thread of a
 *   one-workgroup launch the chunk totals one after the other; an element is (chunk offset) + ((lane offset) + (the
 *   lane's running sum)).  Its relative error is below (16 + 256 + R / 4096 + 2) 2^-53.
 *   rows_out[j] (int64) = the smallest r with cdf[r] > t_j, t_j = u_j * cdf[R-1] (u fp64 [J] in [0, 1); a NaN or
 *   negative u_j counts as 0, and a t_j that is not below cdf[R-1] as the largest double below it), by binary search:
 *   never a row of weight 0.  cdf[R-1] == 0 (no row has weight): every rows_out[j] = -1.
 * Up to four launches on `stream` (chunk scans, chunk offsets, their addition, the searches).
 * Errors in this order: CC_ERR_SHAPE (R < 1, J < 1), CC_ERR_NULL, CC_ERR_TOO_LARGE (R or J > 2^31 - 1), CC_ERR_ALIGN
 * (loss 4 bytes; u, cdf, rows_out 8).
 *
 * cc_resample_write: one workgroup per j < J re-seeds latent l = latents[j] from the pool row x = X[rows[j]]
 * (X [R][ldx], dtype, its K columns).  The arenas -- params (dtype), master (fp32, optional), exp_avg and exp_avg_sq
 * (state_dtype, optional, together) -- share the layout [ W_enc [h][K] | b_enc [h] | W_dec [h][K] | b_dec [K] ].
 *   s = sum_c float(x_c)^2 in fp32 (a lane's fma chain over its 8 columns of every 2048-column chunk, the xor
 *   butterfly, the four waves in order).  If s is 0 or not finite, or rows[j] is outside [0, R) (the -1 of an empty
 *   pick) or l outside [0, h), nothing is written for j.  Otherwise, with es = enc_norm / sqrtf(s) and
 *   ds = dec_norm / sqrtf(s) (fp32):
 *     W_enc[l][c] = dtype(float(x_c) * es),  W_dec[l][c] = dtype(float(x_c) * ds),  b_enc[l] = 0;
 *     master: the same fp32 products unrounded (so a bf16 parameter is its master rounded to nearest-even) and 0;
 *     exp_avg, exp_avg_sq: row l of both halves and the b_enc entry become +0.
 *   b_dec and every other row are not touched.  done (optional, int32 [J]): 1 where j was written, else 0.
 * latents must be distinct (the caller's check: two workgroups would write one row); rows may repeat.
 * Errors in this order: CC_ERR_SHAPE (R or J < 1, h or K < 8 or not a multiple of 8, ldx < K), CC_ERR_NULL (X, rows,
 * latents or params missing, one moment arena without the other), CC_ERR_DTYPE (dtype; state_dtype where the moments
 * are given), CC_ERR_TOO_LARGE (R, J, h or K > 2^31 - 1), CC_ERR_ALIGN (16 bytes: X and its pitch and every arena;
 * 8: rows, latents; 4: done). */
int cc_row_norms(const void* W, int64_t ld, int64_t rows, int64_t K, int dtype, float* out, void* stream);
int cc_resample_pick(const float* loss, int64_t R, const double* u, int64_t J, double* cdf, int64_t* rows_out,
                     void* stream);
int cc_resample_write(const void* X, int64_t ldx, int64_t R, const int64_t* rows, const int64_t* latents, int64_t J,
                      int64_t h, int64_t K, int dtype, float enc_norm, float dec_norm, void* params, float* master,
                      void* exp_avg, void* exp_avg_sq, int state_dtype, int32_t* done, void* stream);

/* ---- The backward of cc_decode_pairs and the per-latent accumulator of LatentAttribution (CrossCoder.decode_pairs(...,
 * differentiable=True), pairs_attribution, LatentAttribution).  Gather kernels: no [B][h] or dense [B][h]-sized matrix is
 * formed.  No float atomics, no spin waits; every summation order is fixed by the arguments alone, so two calls give
 * the same bits.  K = n * d.
 *
 * cc_pairs_grad_values: the sampled dot product of g [B][ldg] (dtype; any [B][K] matrix, in practice the gradient on
 * the reconstruction) with the decoder rows the pairs name.  idx [B][k] (int32, dense), val [B][k] (dtype, dense,
 * optional), W_dec [h][ldw] (dtype); dot [B][k][n] and total [B][k] (fp32, dense, each optional, at least one given).
 *   dot[r][s][m] = sum over c in [m d, (m+1) d) of float(g[r][c]) * float(W_dec[idx[r][s]][c]):  a wave owns the slot;
 *   lane l folds the model's 8-column groups G (columns 8 G .. 8 G + 7) with G % 64 == l in ascending G, columns in
 *   order, into one fp32 fma chain from +0; the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.  With
 *   val, that sum is multiplied once in fp32 by float(val[r][s]): the pair's attribution.
 *   total[r][s] = +0 + dot[r][s][0] + dot[r][s][1] + ... in model order (the multiplied sums where val is given).
 * A slot whose index is outside [0, h) (one unsigned compare, as in cc_decode_pairs) gives +0 everywhere and its W_dec row
 * is not read; duplicate indices are computed independently.  The row of g is read from memory once per token (staged
 * in LDS; columns past the first 8192 are re-read through the caches).
 * Errors, checked in this order before any launch: CC_ERR_SHAPE (B, k, h or n < 1, d < 8 or d % 8 != 0, ldw < K,
 * ldg < K), CC_ERR_NULL (idx, W_dec or g missing, neither output), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h or K > 2^31 - 1,
 * k > 2^17), CC_ERR_ALIGN (16 bytes: W_dec, g and their row pitches; 4 bytes: idx, dot, total; val: its element).
 *
 * The two entry points below take the pairs grouped by latent: perm [P] (int32) holds flat slot numbers r * k + s and
 * seg [h + 1] (int64) offsets into it: latent j's pairs are perm[seg[j] .. seg[j+1]), in the caller's order (ops.
 * pairs_by_latent: by (r, s)).  idx is not read: segment j IS latent j.  seg values are clamped to [0, P], a segment
 * with end < begin is empty, and a perm entry outside [0, B k) is skipped: no input causes an out-of-range access.
 *
 * cc_pairs_grad_decoder: dW [h][ldo] (dtype; every row's K columns are written) = pairs^T . g:
 *   dW[j][c] = dtype(sum over p in [seg[j], seg[j+1]) of float(val[perm[p]]) * float(g[perm[p] / k][c])).
 *   A segment of at most L = CC_PAIRS_GRAD_SPLIT entries: one fp32 fma chain from +0 in segment order, rounded once.  A
 *   longer one: its consecutive pieces of L entries (the last piece shorter) are each such a chain from +0, the piece
 *   sums are added in piece order onto +0 in fp32, and that sum is rounded once; the pieces run in workgroups of
 *   their own (a latent that fires in every row does not serialise the launch).  An empty segment gives a row of +0.
 *   ws: cc_pairs_grad_decoder_ws_floats(P, K) = (P / L) * K floats of caller scratch for the full pieces' sums (may
 *   be NULL where that is 0).  Two launches on `stream`.
 * Errors in this order: CC_ERR_SHAPE (B, k or h < 1, P < 0, K < 8 or K % 8 != 0, ldg < K, ldo < K), CC_ERR_NULL (seg,
 * val, g or dW missing, perm missing with P > 0, ws missing with P >= L), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h, K, P or
 * B * k > 2^31 - 1, k > 2^17), CC_ERR_ALIGN (16 bytes: g, dW, their row pitches, ws; 8: seg; 4: perm; val: its element).
 *
 * cc_pairs_latent_sums: a [B k][n] (fp32, dense; cc_pairs_grad_values' dot) folded into the persistent per-latent state
 * sum [h][n], abs_sum [h][n] (fp64) and count [h] (int64): for latent j and each p of its segment in order,
 *   sum[j][m] += (double)a[perm[p]][m];  abs_sum[j][m] += fabs((double)a[perm[p]][m]);  count[j] += 1
 * -- plain fp64 adds onto the stored values, one thread per (j, m): a CPU fp64 loop gives the same bits.
 * Errors in this order: CC_ERR_SHAPE (B, k, h or n < 1, P < 0), CC_ERR_NULL (a, seg, sum, abs_sum or count missing,
 * perm missing with P > 0), CC_ERR_TOO_LARGE (h, n, P or B * k > 2^31 - 1, k > 2^17), CC_ERR_ALIGN (8 bytes: seg, sum,
 * abs_sum, count; 4: a, perm). */
#define CC_PAIRS_GRAD_SPLIT 128
int cc_pairs_grad_values(const int32_t* idx, const void* val, int64_t B, int k, const void* W_dec, int64_t ldw,
                         int64_t h, const void* g, int64_t ldg, int64_t n, int64_t d, int dtype, float* dot,
                         float* total, void* stream);
int64_t cc_pairs_grad_decoder_ws_floats(int64_t P, int64_t K);
int cc_pairs_grad_decoder(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, int64_t B,
                          int k, const void* g, int64_t ldg, int64_t K, int dtype, void* dW, int64_t ldo, float* ws,
                          void* stream);
int cc_pairs_latent_sums(const float* a, int64_t B, int k, int64_t n, const int32_t* perm, int64_t P,
                         const int64_t* seg, int64_t h, double* sum, double* abs_sum, int64_t* count, void* stream);

/* ---- The sparse TopK training step's own kernels (Trainer.step with cfg["sparse_step"]), beside
 * cc_topk_rows' pairs, cc_pairs_grad_values and the loss kernels.  No float atomics, no spin waits, no host reads; every
 * float summation order is fixed by the arguments alone, so two calls give the same bits.
 *
 * cc_pairs_group: the pairs idx [B][k] (int32, dense; a slot whose index is outside [0, h) is padding) grouped by latent:
 * seg [h + 1] (int64) and perm [B k] (int32) such that perm[seg[j] .. seg[j+1]) are the flat slot numbers r * k + s of
 * latent j's pairs in ascending order, i.e. the valid slots sorted by (latent, row, slot) -- ops.pairs_by_latent's seg
 * and perm[:seg[h]].  Entries of perm from seg[h] on are unspecified values inside [0, B k).  A counting sort over
 * (latent, 256-row block) cells: integer atomics count and place, and a rank by slot number inside each cell removes
 * their arrival order; a latent that fires in every row is ceil(B / 256) cells ranked by their own threads.
 * ws: cc_pairs_group_ws_bytes(B, k, h) bytes of caller scratch (0: the arguments are out of range).  A memset and five
 * launches on `stream`.
 * Errors in this order: CC_ERR_SHAPE (B, k or h < 1), CC_ERR_NULL, CC_ERR_TOO_LARGE (h or B * k > 2^31 - 1, k > 2^17,
 * h * ceil(B / 256) > 2^28), CC_ERR_ALIGN (16 bytes: ws; 8: seg; 4: idx, perm).
 *
 * cc_decode_pairs_partial: recon [B][ldr] (fp32; the K columns of every row are written) = the fp32 fma chain
 *   +0 + sum_s float(val[r][s]) * float(W_dec[idx[r][s]][c])   over the slots s = 0 .. k-1 in that order,
 * cc_decode_pairs' chain from +0 instead of b_dec[c] and without the rounding: the partial reconstruction the dense
 * cc_decode_partial hands to cc_loss_fwd_bwd.  A slot whose index is outside [0, h) adds nothing and reads nothing.
 * Errors in this order: CC_ERR_SHAPE (B, k or h < 1, K < 8 or K % 8 != 0, ldw < K, ldr < K), CC_ERR_NULL, CC_ERR_DTYPE,
 * CC_ERR_TOO_LARGE (h or K > 2^31 - 1, k > 2^17), CC_ERR_ALIGN (16 bytes: W_dec, recon and their row pitches; 4: idx;
 * val: its element).
 *
 * cc_pairs_wgrad: the step's three list gradients from one walk of the pairs grouped by latent (perm [P], seg [h + 1]:
 * the two entry points above this block describe them; the same clamping, so garbage gives garbage sums in bounds):
 *   dW_dec[j][c] = dtype(sum over latent j's list of float(val[slot]) * float(g_recon[slot / k][c]))
 *   dW_enc[j][c] = dtype(sum over latent j's list of p(slot) * float(x[slot / k][c]))
 *   db_enc[j]    = dtype(sum over latent j's list of p(slot))          p(slot) = float(dtype(g_pre[slot]))
 * val [B][k] (dtype, dense), g_pre [B][k] (fp32, dense: cc_pairs_grad_values' total, rounded to the dtype where it is
 * read), g_recon [B][ldg] and x [B][ldx] (dtype), dW_dec [h][ld_dec], dW_enc [h][ld_enc] (dtype; every row's K columns
 * are written), db_enc [h] (dtype).  Order: exactly cc_pairs_grad_decoder's -- a list of at most L =
 * CC_PAIRS_GRAD_SPLIT entries is one fp32 chain from +0 in list order (fma for the two matrices, a plain add for
 * db_enc), rounded once; a longer list in consecutive pieces of L, the piece sums added in piece order onto +0, rounded
 * once.  An empty list gives +0.  sq_dec, sq_enc, sq_b_enc: cc_pairs_wgrad_parts(h) floats each, the squared sums of
 * the stored (rounded) values: a lane's fma(r, r, sq) chain over the elements it stores in the order it stores them
 * (rows j = g, g + parts, ...; per row its 8-column groups t, t + 256, ...), the xor butterfly 32 .. 1, the four waves
 * in order; one partial per workgroup g at index g.
 * ws: cc_pairs_wgrad_ws_floats(P, K) = (P / L) * (2 K + 8) floats of caller scratch (may be NULL where that is 0).
 * Two launches on `stream`.
 * Errors in this order: CC_ERR_SHAPE (B, k or h < 1, P < 0, K < 8 or K % 8 != 0, a row pitch < K), CC_ERR_NULL (any
 * operand missing; perm with P > 0, ws with P >= L), CC_ERR_DTYPE, CC_ERR_TOO_LARGE (h, K, P or B * k > 2^31 - 1,
 * k > 2^17), CC_ERR_ALIGN (16 bytes: g_recon, x, dW_dec, dW_enc, their row pitches, ws; 8: seg; 4: perm, g_pre, the sq
 * partials; val, db_enc: their element). */
int64_t cc_pairs_group_ws_bytes(int64_t B, int k, int64_t h);
int cc_pairs_group(const int32_t* idx, int64_t B, int k, int64_t h, int32_t* perm, int64_t* seg, void* ws,
                   void* stream);
int cc_decode_pairs_partial(const void* val, const int32_t* idx, int64_t B, int k, const void* W_dec, int64_t ldw,
                            int64_t h, int64_t K, int dtype, float* recon, int64_t ldr, void* stream);
int64_t cc_pairs_wgrad_ws_floats(int64_t P, int64_t K);
int64_t cc_pairs_wgrad_parts(int64_t h);
int cc_pairs_wgrad(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val, const float* g_pre,
                   int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx, int64_t K, int dtype,
                   void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc, float* sq_dec,
                   float* sq_enc, float* sq_b_enc, float* ws, void* stream);

/* ---- the compacted dead set of the sparse step's AuxK loss (csrc/auxk_compact.hip, csrc/sparse_step.hip) ----
 * cc_dead_compact: the dead latents of since_fired [h] (int64; dead: since_fired >= dead_after, latents >= h_real
 * never) in ascending latent order: ids[c] (int32 [d_pad]) is the c-th dead latent for c < D and -1 from D on,
 * slot[j] (int32 [h]) the compact index of latent j or -1, *count (uint32) = D.  Dead latents from d_pad on are
 * dropped (slot -1): *count > d_pad says so.  One launch of one workgroup: a scan, no atomics, no arrival order.
 * Errors in this order: CC_ERR_SHAPE (h < 1, h_real outside 0..h, d_pad < 8 or not a multiple of 8), CC_ERR_NULL,
 * CC_ERR_TOO_LARGE (h or d_pad > 2^17), CC_ERR_ALIGN (8 bytes: since_fired; 4: ids, slot, count).
 *
 * cc_compact_gather: bit copies through ids [d_pad] -- either group may be left out (both of its pointers NULL):
 *   rows     Wc[c][0 .. K) = W[ids[c]][0 .. K)          W [h][ldw], Wc [d_pad][ldc] (dtype), 16-byte vectors
 *   columns  acts_c[r][c]  = acts[r][ids[c]]            acts [B][lda], acts_c [B][d_pad] (dtype, dense)
 * An ids[c] outside [0, h) gives a +0 row / column.  One launch per group on `stream` (columns first).
 * Errors in this order: CC_ERR_SHAPE (d_pad < 8 or not a multiple of 8, h < 1; rows: K < 8, K % 8 != 0, a pitch < K;
 * columns: B < 1, lda < h), CC_ERR_NULL (ids, no group, half a group, a group in place), CC_ERR_DTYPE,
 * CC_ERR_TOO_LARGE (h or K > 2^31 - 1, d_pad > 2^17, B > 2^20), CC_ERR_ALIGN (16 bytes: W, Wc, their pitches, acts_c;
 * 4: ids; acts: its element).
 *
 * cc_pairs_wgrad_add: cc_pairs_wgrad with three addends, given together or all NULL (then it is cc_pairs_wgrad): for a
 * latent j with s = slot[j] in [0, d_pad), float(aWd[s][c]), float(aWe[s][c]) and float(ab[s]) are added to the fp32
 * sums of dW_dec[j][c], dW_enc[j][c] and db_enc[j] after the list's and before the one rounding; any other slot adds
 * nothing.  slot int32 [h]; aWd [d_pad][lda_d], aWe [d_pad][lda_e] and ab [d_pad] in the dtype.  The squared sums are
 * those of the stored values, in cc_pairs_wgrad's order.
 * Errors: cc_pairs_wgrad's, with -- CC_ERR_SHAPE: d_pad < 1 or an addend pitch < K; CC_ERR_NULL: some addends without
 * the others; CC_ERR_TOO_LARGE: d_pad > 2^31 - 1; CC_ERR_ALIGN, after cc_pairs_wgrad's own: aWd, aWe and their pitches
 * 16 bytes, slot 4, ab its element. */
int cc_dead_compact(const int64_t* since_fired, int64_t h, int64_t h_real, int64_t dead_after, int32_t* ids,
                    int64_t d_pad, int32_t* slot, uint32_t* count, void* stream);
int cc_compact_gather(const int32_t* ids, int64_t d_pad, int64_t h, const void* W, int64_t ldw, int64_t K, void* Wc,
                      int64_t ldc, const void* acts, int64_t lda, int64_t B, void* acts_c, int dtype, void* stream);
int cc_pairs_wgrad_add(const int32_t* perm, int64_t P, const int64_t* seg, int64_t h, const void* val,
                       const float* g_pre, int64_t B, int k, const void* g_recon, int64_t ldg, const void* x, int64_t ldx,
                       int64_t K, int dtype, void* dW_dec, int64_t ld_dec, void* dW_enc, int64_t ld_enc, void* db_enc,
                       float* sq_dec, float* sq_enc, float* sq_b_enc, float* ws, const int32_t* slot, int64_t d_pad,
                       const void* aWd, int64_t lda_d, const void* aWe, int64_t lda_e, const void* ab, void* stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif
