/* libcsm_hip.so - C ABI of the MI355X (gfx950) hot path for CSM training / generation.
 *
 * The reference (imaginateit/csm-train-pytorch) is pure Python and has no FFI: its boundary for this path is
 * the Python API of csm.models.model / csm.training.utils / csm.training.trainer / csm.training.lora_trainer /
 * csm.generator.  The host-side mirror of that API lives in csm-train-pytorch_amd/csm/ and calls ONLY the entry
 * points below (through ctypes).  Each entry names the reference arithmetic it replaces (paths relative to the
 * reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (torch-allocated); the library owns nothing;
 *   - bf16 tensors are passed as void* (raw uint16 storage), row-major, 16-byte aligned;
 *   - all work is enqueued on the caller's hipStream_t; nothing synchronises, allocates or frees (graph-capturable);
 *   - return value 0 = ok, non-zero = error (1 bad argument, 2 launch failure, 3 no device, 4 wrong arch);
 *     csm_last_error() returns the text for the calling thread.  No exception crosses the boundary.
 */
#ifndef CSM_HIP_H
#define CSM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* csm_stream_t; /* == hipStream_t */

int csm_abi_version(void);
const char* csm_last_error(void);
int csm_device_check(int device);

/* ---- K3/K6/K7/K8/K9/K10/K11: every dense contraction -------------------------------------------------------
 * C[M,N] = alpha * opA(A) . opB(B)^T (+ R), bf16 in, fp32 accumulate, bf16 or fp32 out, optional batch.
 *   transA=0: A is [M][K] (lda)      transA=1: A is [K][M] (lda)
 *   transB=0: B is [N][K] (ldb)      transB=1: B is [K][N] (ldb)
 * Replaces torchtune nn.Linear q/k/v/output_proj, w1/w2/w3 (model.py:13-42), Model.projection, codebook0_head
 * and torch.mm(decoder_h, audio_head[i-1]) (src/csm/models/model.py:124-126,172,184,187), their autograd
 * backward products, and the LoRA A/B products of src/csm/mlx/components/lora.py:71-105.
 * R (bf16, ldr) may alias C (accumulate).  lda/ldb multiples of 8; the contiguous dimension of A and of B a
 * multiple of 8.  Under the SwiGLU-forward and RoPE epilogues below a residual needs ldr % 4 == 0 (refused otherwise). */
int csm_gemm_bf16(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int lda, int ldb, int ldc,
                  int ldr, int transA, int transB, int out_f32, float alpha, int batch, long long strideA,
                  long long strideB, long long strideC, long long strideR, csm_stream_t stream);

/* Same product with a fused epilogue (bf16 output only):
 *   epilogue 1, SwiGLU forward : C = [M][N] with gate/up interleaved along N (g0,u0,g1,u1,...) AND aux_out[M][N/2] =
 *                                silu(gate)*up  - the w1/w3 projection of torchtune FeedForward in one pass;
 *   epilogue 2, SwiGLU backward: the GEMM result is d(act) [M][N] (never stored); aux_in = gate/up [M][2N]; C receives
 *                                d(gate),d(up) interleaved [M][2N] (ldc >= 2N) - the w2 dgrad fused with the activation backward. */
int csm_gemm_bf16_ex(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int lda, int ldb, int ldc,
                     int ldr, int transA, int transB, int out_f32, float alpha, int batch, long long strideA,
                     long long strideB, long long strideC, long long strideR, int epilogue, const void* aux_in,
                     void* aux_out, int ld_aux, csm_stream_t stream);
/* Fused q|k|v projection + RoPE forward: C[M][N] = A[M][K] W[N][K]^T, interleaved pairs of columns [0, n_rope_cols) (the q and
 * k heads, head_dim features each) rotated by position (row % rows_per_seq) with the fp32 (cos, sin) table
 * [P][head_dim/2][2].  Replaces torchtune q_proj / k_proj / v_proj + Llama3ScaledRoPE as configured at reference
 * src/csm/models/model.py:13-25,30-42 (rope_base 500000, scale_factor 32) for positions arange(S)
 * (src/csm/training/utils.py:81-82). */
int csm_gemm_bf16_rope(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc,
                       const float* rope_table, int rows_per_seq, int n_rope_cols, int head_dim, csm_stream_t stream);
/* A frozen projection and its LoRA adapters as ONE product: C[M][N] = A . B (layouts by transA / transB as in csm_gemm_bf16)
 * + xA[M][kx] . xB[N][kx]^T (+ R), the extra kx / 32 k-steps taken after the main loop, in fp32, in the same accumulators,
 * before the epilogue (0 none; 1 / 2 SwiGLU forward / backward: aux_out / aux_in, ld_aux as in csm_gemm_bf16_ex; 3 RoPE: aux_in = table, ld_aux =
 * rows per sequence, rope_cols / head_dim as in csm_gemm_bf16_rope).  xA / xB: bf16, row-major, leading dimension kx (a
 * multiple of 32, <= 256; ranks padded with zeros), 16-byte aligned.  Replaces the two extra matmuls and the add of
 * LoRALinear.__call__ (reference src/csm/mlx/components/lora.py:85-105: y = x W0^T + scale (x A^T) B^T, with xA = scale x A^T
 * and xB = B) and of its input gradient (dx = dy W0 + (scale dy B) A: xA = scale dy B, xB = A^T). */
int csm_gemm_bf16_kext(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int lda, int ldb, int ldc, int ldr,
                       int transA, int transB, const void* xA, const void* xB, int kx, int epilogue, const void* aux_in,
                       void* aux_out, int ld_aux, int rope_cols, int head_dim, csm_stream_t stream);
/* csm_gemm_bf16 / _ex / _kext (bf16 output, one batch) on the 128x128 kernel whatever M is: there an output row's bits depend
 * on that row of A (xA, R) and on B only, not on the other rows of the launch, where the automatic choice moves to the 256x256
 * kernels (another summation order) once M fills the chip.  For callers that stack rows of independent sequences into one
 * product and owe each the bits it gets alone (DecodeState.append_rows).  kx = 0: no K-extension; epilogue as in _kext. */
int csm_gemm_bf16_pinned(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int lda, int ldb, int ldc,
                         int ldr, int transA, int transB, float alpha, const void* xA, const void* xB, int kx, int epilogue,
                         const void* aux_in, void* aux_out, int ld_aux, int rope_cols, int head_dim, csm_stream_t stream);
/* out[M][N] = alpha * X[M][K] Wt[N][K]^T for N = 32 or 64 and K % 128 == 0: the skinny products of a LoRA group (x A^T and dy B of
 * reference src/csm/mlx/components/lora.py:85-105 with the group's ranks side by side), read-once bandwidth kernel. */
int csm_skinny_nt_bf16(const void* X, const void* Wt, void* out, int M, int N, int K, int ldx, int ldw, int ldo, float alpha,
                       csm_stream_t stream);
/* csm_skinny_nt_bf16 for a stack of LoRA adapters trained in one batch: Wt holds the adapters' blocks of blk columns side by side
 * (N a multiple of 32 in [32, 256], blk a multiple of 8) and row m keeps the block of its own adapter sel[m] (int32 on the device,
 * -1 = none):  out[m][n] = alpha * sum_k X[m][k] Wt[n][k] if sel[m] >= 0 and n / blk == sel[m], +0 otherwise.  The zeros are
 * chosen, not multiplied (Inf / NaN in X beside them does not matter); sel is compared only, never an index.  A kept element
 * has the bits csm_skinny_nt_bf16 gives it; only the 16-column tiles some row of a 16-row tile keeps are computed. */
int csm_skinny_nt_sel_bf16(const void* X, const void* Wt, void* out, const int* sel, int M, int N, int K, int blk, int ldx, int ldw,
                           int ldo, float alpha, csm_stream_t stream);
/* The two backward products of a Linear layer in one launch, their tiles interleaved over the chip:
 *   dX[M][Kin] = dY[M][Nout] W[Nout][Kin]   (dx_epilogue 0), or the SwiGLU backward of that product (dx_epilogue 2: W = w2,
 *   aux_in = gate/up [M][2 Kin], dX = d(gate/up) [M][2 Kin]);   dW[Nout][Kin] (+)= alpha_w * dY^T X[M][Kin].
 * Replaces autograd's two matmuls per nn.Linear in `loss.backward()` (reference src/csm/training/trainer.py:261-263). */
int csm_gemm_bf16_dgrad_wgrad(const void* dY, const void* W, void* dX, const void* X, void* dW, int M, int Nout, int Kin, int ld_dy,
                              int ldw, int ld_dx, int ldx, int ld_dw, int dx_epilogue, const void* aux_in, int ld_aux,
                              int accumulate, float alpha_w, csm_stream_t stream);
/* Two weight gradients sharing the token dimension, dW_i[N_i][K_i] (+)= alpha * dY_i[M][N_i]^T X_i[M][K_i], in one launch (for
 * outputs too small to fill the chip alone: attention output projection + fused q|k|v projection of one layer). */
int csm_gemm_bf16_two_wgrad(const void* dY1, const void* X1, void* dW1, int N1, int K1, int ld_dy1, int ldx1, int ld_dw1,
                            const void* dY2, const void* X2, void* dW2, int N2, int K2, int ld_dy2, int ldx2, int ld_dw2,
                            int M, int accumulate, float alpha, csm_stream_t stream);
/* n (1..12) such weight gradients in one launch, arrays of n entries each.  The attention projections' gradients of one layer
 * are 160 tiles of 256 x 256 - 0.63 of a round of the 256 CUs; the engine defers them and launches three layers' worth (480
 * tiles, 1.9 rounds) together.  Tile arithmetic as csm_gemm_bf16_two_wgrad: results do not depend on the grouping.
 * (autograd's per-Linear weight-gradient matmuls, reference src/csm/training/trainer.py:261-263) */
int csm_gemm_bf16_multi_wgrad(int n, const void* const* dY, const void* const* X, void* const* dW, const int* N, const int* K,
                              const int* ld_dy, const int* ldx, const int* ld_dw, int M, int accumulate, float alpha,
                              csm_stream_t stream);


/* tuning switch (A/B benchmarking): 0 register staging 128x128; 1 LDS-DMA 128x128; 2 auto = the 256x256 pipelined kernel
 * where its tiles fill the chip, else 128x128 (default); 3 force the 256x256 kernel; 4 force the four-wave 256x256 kernel
 * with the hand-scheduled K loop where it applies (batch 1, no K-extension), else as 3 */
int csm_set_gemm_variant(int v);
/* tuning switch: 1 (default) the 256x256 kernel runs one persistent workgroup per CU over its tile list (the next tile's first
 * loads are requested before the finished tile is stored); 0 one tile per workgroup */
int csm_set_gemm256_persistent(int v);
int csm_get_gemm256_persistent(void);
/* tuning switches for A/B runs: key 0 = the eight-wave 256x256 kernel touches the tile of a fused epilogue's read operand
 * (gate/up of the SwiGLU backward, a bf16 residual) during its K loop so that the epilogue's loads hit cache (default 1);
 * key 1 = the auto variant hands batch-1 products without K-extension to the four-wave kernel (default 1);
 * key 8 (round 4) = the four-wave kernel uses 256 x 192 output tiles where they fill the rounds of the 256 CUs better (default 1) */
int csm_set_gemm_tuning(int key, int value);
/* name of the kernel (rocprofv3 spelling, without the argument list) the most recent csm_gemm_* call on this host thread's
 * library instance launched - for benchmarks that attribute time to kernels; not thread-safe */
const char* csm_gemm_last_kernel(void);

/* ---- K2: torchtune RMSNorm (sa_norm / mlp_norm / norm; eps=1e-5 at model.py:22,39) -------------------------- */
int csm_rmsnorm_fwd(const void* x, const void* scale, void* y, float* rstd, int M, int D, float eps, csm_stream_t stream);
int csm_rmsnorm_bwd_blocks(void);
int csm_rmsnorm_bwd(const void* x, const void* scale, const float* rstd, const void* dy, const void* dres, void* dx,
                    float* dscale_partials /* [csm_rmsnorm_bwd_blocks()][D] or NULL */, int M, int D, csm_stream_t stream);
int csm_colsum_bf16(const float* partials, int rows, int D, void* dst, int accumulate, csm_stream_t stream);
/* the same reduction for n (1..8) pairs of one shape in one launch (the RMSNorm scale gradients of the layers whose small weight
 * gradients the engine launches together); per column the arithmetic of csm_colsum_bf16 */
int csm_colsum_bf16_multi(int n, const float* const* partials, void* const* dst, int rows, int D, int accumulate, csm_stream_t stream);

/* ---- LoRA side ops (reference mlx/components/lora.py:85-102): inverted dropout of the adapter input (mask is a pure
 * function of (seed, row*D+col), so the backward regenerates it; accumulate=1: out += dropout(in)), the optional
 * lora_bias add, and the bf16 column sums that give d(lora_bias) (finish with csm_colsum_bf16 on the partials). */
int csm_dropout_bf16(const void* in, int ld_in, void* out, int ld_out, long long M, int D, float p, unsigned long long seed,
                     int accumulate, csm_stream_t stream);
int csm_bias_add_bf16(void* y, int ld, const void* bias, long long M, int D, csm_stream_t stream);
int csm_colsum_rows_bf16(const void* x, int ld, long long M, int D, float* partials /* [slices][D] */, int slices,
                         csm_stream_t stream);

/* ---- K4: torchtune Llama3ScaledRoPE (rope_base=500000, scale_factor=32: model.py:23-24,40-41), interleaved
 * pairs, in place on the q and k heads of the fused qkv buffer; inverse=1 is the backward rotation.
 * table = [P][head_dim/2][2] (cos,sin) fp32; pos = int32 [M] or NULL (position = row % S). */
int csm_rope(void* qkv, const float* table, const int* pos, long long M, int S, int n_heads_qk, int head_dim, int ld,
             int inverse, csm_stream_t stream);

/* ---- K5: causal GQA attention replacing torchtune MultiHeadAttention -> F.scaled_dot_product_attention with the
 * mask of model.py:59-76 / training/utils.py:90-91.  qkv [B*S][(H+2KV)*HD]; out [B*S][H*HD]; lse [B][H][S]. */
int csm_set_attn_variant(int v); /* scheduling experiments: 0 = defaults; else bit fields (query tiles per wave, dK/dV key
                                  * tile and work order, heaviest-first order of the forward / dQ grid) - see attention.hip */
int csm_attn_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, int KV, int HD, csm_stream_t stream);
/* scratch of csm_attn_bwd / csm_attn_bwd_rope in BYTES (since ABI 2: 2 x [B][H][S] floats - the dQ pass leaves -delta and
 * -lse*log2(e) per query there for the dK/dV pass; ABI 1 needed half).  Allocate at least this much for delta_ws. */
long long csm_attn_bwd_workspace_bytes(int B, int S, int H);
int csm_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                 float* delta_ws /* scratch, csm_attn_bwd_workspace_bytes(B, S, H) */, int B, int S, int H, int KV, int HD, csm_stream_t stream);
/* the same with the backward of csm_rope fused into the dQ / dK epilogues (table as for csm_rope, position = row index
 * inside the sequence): dqkv comes out as the gradient of the UN-rotated projection output, no separate inverse pass. */
int csm_attn_bwd_rope(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                      const float* rope_table, int B, int S, int H, int KV, int HD, csm_stream_t stream);
/* which kernels the most recent csm_attn_bwd* call on this library instance launched (for tests and benchmarks; not
 * thread-safe; since ABI 3): bit 0 = the dK/dV pass, bit 1 = the dQ pass ran the generated-asm kernel of attention64_asm.hip
 * (head_dim 64, S % 64 == 0, 4 query heads per kv head); a clear bit = the compiler-scheduled kernel of attention64.hip /
 * attention.hip */
int csm_attn_last_dkv_kernel(void);
/* Packed rows (sequence packing; additive in ABI 3): several sequences share one row of S positions and key j is visible to
 * query i iff seg_start[i] <= j <= i.  seg_start / seg_end: int32 device arrays [B*S], the first / last position of the
 * position's segment, row-local, non-decreasing along a row and total (a row's padding is one more segment); the host builds
 * them and the kernels trust them.  head_dim 64 only.  There is no fused-RoPE form (packed positions are not arange(S)): rotate
 * with csm_rope(pos) before the forward and with inverse = 1 after the backward.  The backward always takes the
 * compiler-scheduled dQ and dK/dV kernels (csm_attn_last_dkv_kernel() answers 0 after it); delta_ws as for csm_attn_bwd.  One
 * segment per row gives the bits of csm_attn_fwd / of csm_attn_bwd under csm_set_attn_variant(default word | 1 << 10). */
int csm_attn_fwd_seg(const void* qkv, void* out, float* lse, const int* seg_start, int B, int S, int H, int KV, int HD, csm_stream_t stream);
int csm_attn_bwd_seg(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                     const int* seg_start, const int* seg_end, int B, int S, int H, int KV, int HD, csm_stream_t stream);
/* tools/probes only: a device buffer (>= grid x 4 waves x 8 rounds x 8 u64) that the asm dQ kernel fills with cycle stamps, or NULL */
int csm_attn64_set_debug(void* device_buffer);

/* ---- K7: SwiGLU of torchtune FeedForward: out = silu(gate) * up, gu = gate/up INTERLEAVED ([M][2F]: g0,u0,g1,u1,..) - */
int csm_swiglu_fwd(const void* gu, void* out, long long M, int F, csm_stream_t stream);
int csm_swiglu_bwd(const void* gu, const void* dout, void* dgu, long long M, int F, csm_stream_t stream);

/* ---- K1: Model._embed_tokens + mask-mul-sum (model.py:202-217, training/utils.py:85-87) ---------------------- *
 * tokens int64 [M][K+1] (K audio slots then the text slot), mask uint8 [M][K+1]; out bf16 [M][D].
 * The backward is csm_embed_bwd_sorted below. */
int csm_embed_fwd(const long long* tokens, const uint8_t* mask, const void* text_emb, const void* audio_emb, void* out,
                  long long M, int K, int D, int audio_vocab, csm_stream_t stream);

/* Deterministic, scratch-free form of the embedding backward: occurrences (embedding row, source row) sorted by
 * embedding row; text rows are [0, text_rows), audio rows follow; rows >= n_rows are padding.  Source index < M reads
 * dh[index], otherwise dseq[index - M].  Sums in fp32 registers, adds into the bf16 gradient tables once per row. */
int csm_embed_bwd_sorted(const long long* sorted_rows, const long long* src_index, long long n_occ, const void* dh,
                         const void* dseq, long long M, void* g_text, void* g_audio, long long text_rows, long long n_rows,
                         int D, csm_stream_t stream);
/* dst[rows[n]] += src[n * src_stride_rows] for unique rows (scatter of the decoder's position-0 gradient); rows[n] < 0 is
 * padding and is skipped */
int csm_rows_add_bf16(void* dst, const int* rows, const void* src, long long N, int src_stride_rows, int D, csm_stream_t stream);
/* out[n] = table[rows[n]], table[rows[n]] = 0 for unique rows (rows[n] < 0: out[n] = 0).  New capability (the reference has
 * no distributed code): the fixed-capacity exchange of touched text-embedding gradient rows between
 * data-parallel ranks (csm/training/dp.py), which replaces a 525 MB all-reduce of reference model.py:119's table. */
int csm_rows_take_bf16(void* table, const int* rows, void* out, long long N, int D, csm_stream_t stream);

/* depth-decoder teacher forcing (model.py:175-189): out[n][0]=hidden[rows[n]], out[n][i]=audio_emb[code_{i-1}+(i-1)V] */
int csm_decoder_input_fwd(const void* hidden, const int* rows, const long long* codes, const void* audio_emb, void* out,
                          long long N, int K, int D, int audio_vocab, csm_stream_t stream);

/* ---- K9/K11: F.cross_entropy (training/utils.py:102-105) fused with its backward ------------------------------ *
 * logits fp32 [R][ldl]; targets int64 [R] (<0 = row excluded); loss_rows fp32 [R]; dlogits bf16 [R][ldd] or NULL. */
int csm_ce_fwd_bwd(const float* logits, const long long* targets, float* loss_rows, void* dlogits, long long R, int V,
                   int ldl, int ldd, float grad_scale, csm_stream_t stream);
int csm_reduce_sum_f32(const float* x, long long n, float scale, float* out, csm_stream_t stream);

/* ---- K12/K13: clip_grad_norm_ + AdamW (training/trainer.py:166-173,271-277) ------------------------------------ */
int csm_sumsq_blocks(void);
int csm_sumsq_bf16(const void* g, long long n, float* partials /* [csm_sumsq_blocks()] */, csm_stream_t stream);
int csm_clip_coef(const float* partials, int n_partials, float max_norm, float* norm_and_coef /* [2] */, csm_stream_t stream);
/* norm_and_coef[1] < 0 on the device = skip this step: parameters and moments are left untouched, only zero_grad is honoured
 * (how a data-parallel step with incomplete gradients is dropped on every rank without a host sync). */
int csm_adamw_step(float* master, float* m, float* v, void* param, void* grad, long long n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, const float* norm_and_coef /* or NULL */,
                   float grad_mul, int zero_grad /* clear grad in the same pass */, csm_stream_t stream);
/* the same update with the fp32 master held as two 16-bit halves: `param` (bf16 working copy = upper half, rounded half-up)
 * and `master_lo` (lower 16 bits); master = ((hi - (lo >> 15)) << 16) | lo exactly.  26 instead of 28 bytes per parameter. */
int csm_adamw_step_split(void* master_lo, float* m, float* v, void* param, void* grad, long long n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, int step, const float* norm_and_coef, float grad_mul,
                         int zero_grad, csm_stream_t stream);
/* both with one flag byte per 2048-element block of the range, counted from its start (ceil(n / 2048) bytes): block_live[b] == 0
 * promises that m and v of block b are all-zero bits.  Such a block whose gradient is all-zero bits too only has its weights
 * decayed - m, v and the gradient are neither read (m, v) nor written, 10 B/param; any other block is marked live (a -0 gradient
 * counts) and updated in full.  Every output bit equals the un-flagged call's; a skipped step leaves the flags alone. */
int csm_adamw_step_live(float* master, float* m, float* v, void* param, void* grad, long long n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int step, const float* norm_and_coef, float grad_mul,
                        int zero_grad, void* block_live, csm_stream_t stream);
int csm_adamw_step_split_live(void* master_lo, float* m, float* v, void* param, void* grad, long long n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, const float* norm_and_coef, float grad_mul,
                              int zero_grad, void* block_live, csm_stream_t stream);

int csm_set_adamw_blocks(int blocks); /* tuning switch */

/* ---- K14: sample_topk + _multinomial_sample_one_no_sync (model.py:79-96), Exp(1) noise q supplied ---------------- */
int csm_sample_topk(const float* logits, const float* q, int* out, int rows, int V, int ldl, int topk, float temperature,
                    csm_stream_t stream);
/* Per-row parameters (additive, ABI 3): `topk` / `temperature` are DEVICE arrays of `rows` entries; row r is sampled exactly as
 * csm_sample_topk samples it with the scalars topk[r], temperature[r] (same bits).  The values cannot be checked on the host, so
 * the kernel bounds them: topk[r] is clamped into [1, V], a temperature[r] that is not a finite positive number counts as 1.0 -
 * with finite logits the written index is always in [0, V).  A captured graph that holds this launch serves every mix of
 * parameters: write the two arrays between replays. */
int csm_sample_topk_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                         const float* temperature, csm_stream_t stream);
/* Per-row nucleus (top-p) and min-p filters (additive, ABI 3): csm_sample_topk_rows with two more DEVICE arrays of `rows` floats.
 * With v = logits / temperature[r], e_i = exp(v_i - max v) and K the set csm_sample_topk_rows keeps (v_i >= the topk[r]-th
 * largest, ties included):  M = { i in K : e_i >= min_p[r] }  (p_i >= min_p * p_max);
 * N = { i in M : sum over j in M with v_j > v_i of e_j  <  top_p[r] * sum over M of e_j }  - a token stays while the mass of
 * the strictly larger values is below top_p, so the token that crosses top_p is kept, equal values stay or go together and no
 * index enters; the largest value always stays.  log_softmax -> softmax -> argmax p / q then run over N.  A row with
 * top_p = 1 and min_p = 0 writes the index csm_sample_topk_rows writes, for every input.  The kernel bounds what it reads: a
 * top_p[r] outside (0, 1] counts as 1, a min_p[r] outside [0, 1] as 0 (NaN is outside both), topk / temperature as above - with
 * finite logits the written index is always in [0, V).  Mass is summed in 64-bit fixed point (quantum 2^-40): the kept set does
 * not depend on the order of summation and a launch gives the same bits every time (error bound: DESIGN.md section 6). */
int csm_sample_filtered_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                             const float* temperature, const float* top_p, const float* min_p, csm_stream_t stream);
/* A windowed repetition penalty and the row's memory of its draws (additive, ABI 3): csm_sample_filtered_rows with, all in DEVICE
 * memory and indexed by row, penalty[r] (float), window[r] (int, frames), the row's ring hist + r * ldh (CSM_SAMPLE_HIST ints,
 * ldh >= CSM_SAMPLE_HIST: slot f % CSM_SAMPLE_HIST holds the code the row drew in frame f of its utterance), frame[r] (f, the
 * frame being sampled) and live[r].  With n = min(window[r], f, CSM_SAMPLE_HIST) and T the distinct ids among
 * ring[(f - 1 - j) % CSM_SAMPLE_HIST], j < n, that lie in [0, V):  x_t = x_t > 0 ? x_t / penalty : x_t * penalty  for t in T -
 * one correctly rounded fp32 operation on the raw logit, before the division by the temperature; then the draw of
 * csm_sample_filtered_rows.  A row with penalty 1 or n = 0 writes the index csm_sample_filtered_rows writes.  Afterwards a row
 * with live[r] != 0 stores its winner to ring[f % CSM_SAMPLE_HIST] (every read of the ring comes first) and, with `advance`
 * nonzero, f + 1 to frame[r]; a row with live[r] = 0 writes `out` only.  Made safe in the kernel: a penalty that is not a finite
 * positive number counts as 1, the window is clamped to [0, CSM_SAMPLE_HIST], ring ids outside [0, V) are ignored (an
 * uninitialised ring is harmless), any f addresses a slot inside the ring.  One launch may use a (hist, frame) pair for one
 * call at a time: only row r's workgroup touches row r's ring and counter. */
#define CSM_SAMPLE_HIST 64
int csm_sample_processed_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                              const float* temperature, const float* top_p, const float* min_p, const float* penalty,
                              const int* window, int* hist, int ldh, int* frame, const int* live, int advance,
                              csm_stream_t stream);
/* Locally typical sampling per row (additive, ABI 3): csm_sample_processed_rows with typical_p[r] (float, DEVICE memory), applied
 * last, on the set N the nucleus leaves.  With P_i = e_i / sum over N of e_j, h_i = -ln P_i, H = sum over N of P_i h_i and
 * delta_i = |h_i - H|:  T = { i in N : sum over j in N with delta_j < delta_i of P_j  <  typical_p[r] }  - a token stays while
 * the mass of the strictly more typical tokens is below typical_p, so the token that crosses it is kept, equal values stay or go
 * together and no index enters; T is never empty but need not hold the largest value.  log_softmax -> softmax -> argmax p / q
 * then run over T.  A row with typical_p = 1 writes what csm_sample_processed_rows writes - out, ring and counter - for every
 * input; a typical_p[r] outside (0, 1] (NaN included) counts as 1.  Mass and H are summed in 64-bit fixed point (quantum 2^-40):
 * a launch gives the same bits every time (error bound: DESIGN.md section 6). */
int csm_sample_typical_rows(const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk,
                            const float* temperature, const float* top_p, const float* min_p, const float* penalty,
                            const int* window, int* hist, int ldh, int* frame, const int* live, int advance,
                            const float* typical_p, csm_stream_t stream);
/* What the model thought of a drawn code (additive, ABI 3): row r reads x = logits + r * ldl, V floats (columns V .. ldl-1 are
 * never read) and codes[r].  With m = max x, S = sum exp(x_i - m), A = sum exp(x_i - m) (x_i - m):
 *   logprob[r] = x[codes[r]] - m - ln S   the model's own log-likelihood of the code: temperature 1, no filter, no penalty;
 *   entropy[r] = ln S - A / S             in nats;
 *   pmax[r]    = 1 / S                    the largest probability of the row.
 * A code outside [0, V) gives logprob = -inf; the other two are still written.  Any of the three output pointers may be NULL
 * (that output is not written); at least one must be given.  One workgroup per row, the row in registers, one pass over memory,
 * sums joined in a fixed order without atomics: a launch gives the same bits every time, and a row's three numbers do not depend
 * on `rows` or on the other rows.  Refused (1, nothing launched): null logits or codes, all three outputs null, rows < 1, V
 * outside 1..4096, ldl < V, a pointer that is not 4-byte aligned.  Error bound: DESIGN.md section 6. */
int csm_sample_stats_rows(const float* logits, const int* codes, float* logprob, float* entropy, float* pmax, int rows, int V,
                          int ldl, csm_stream_t stream);

/* ---- K15: batch-1 decode of Model.generate_frame (model.py:161-195) against KV caches ------------------------------ *
 * y[b][n] = sum_k x[b][k] W[n][k] (+ residual[b][n]), B <= 16 (weight-streaming matrix-vector product).  B <= 4: VALU kernels,
 * row b bit-identical to a one-row launch on that row.  B = 5..16 (ABI 3, additive range extension; needs K % 32 == 0): MFMA
 * tiles, row b bit-identical across every B in 5..16, every position in the batch and any other rows - not to the B <= 4 result */
/* tuning switches for A/B runs (since ABI 3): key 0 = one-row products keep x in registers (no LDS copy, no barrier; default 1),
 * key 1 = the 2048-wide stack's weights are loaded non-temporally in decode (default 1),
 * key 2 = gate/up pairs per wave in the depth decoder's w13 product (1, 2 or 4; default 1: measured equal or slower above),
 * key 3 = two to four batch rows: K = 1024 / 2048 products keep every row of x in registers (default 1; 0 = the LDS kernel),
 * key 4 = two to four batch rows through the B = 5..16 MFMA kernel (default 0; A/B measurement only) */
int csm_set_decode_tuning(int key, int value);
/* Layout and alignment of the decode products (every csm_gemv_* entry point below):
 *  - residual [B][ldy] shares ldy with y: the kernels read residual[b * ldy + n] (and may be y itself);
 *  - the SwiGLU form writes y [B][N / 2] with the same ldy (W and ext_B hold the N gate / up rows interleaved);
 *  - the bf16 entry points read x, W and norm_scale rows in 16-byte loads: x (the table under row_index), W and norm_scale must be
 *    16-byte aligned, ldx and ldw multiples of 8.  csm_gemv_bf16 / _ex / _kext / _kext_rows check the leading dimensions only -
 *    the alignment of the three bases is the caller's duty (csm_gemv_fp8w refuses a misaligned x, W8 or norm_scale).
 *    csm_gemv_t_bf16 reads W [K][ldw] in 16-byte loads (W 16-byte aligned, ldw a multiple of 8, ldw >= N rounded up to 8) and x
 *    element by element. */
int csm_gemv_bf16(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw, int ldx, int ldy,
                  int out_f32, csm_stream_t stream);
/* The decode product kernel launched last by csm_gemv_bf16 / _ex / _kext / _kext_rows, csm_gemv_fp8w, csm_lora_project_bf16 /
 * _rows_bf16 or csm_gemv_t_bf16, with its template arguments, e.g. "gemv_reg_kernel<4, bf16, 0, 1, 1, ext0>" (host bookkeeping
 * for tests and probes, like csm_gemm_last_kernel; "" before the first launch; not thread-safe).  gemv_reg_kernel<KCH, T, SWIGLU,
 * NT, RPW, ext>, gemv_regn_kernel<KCH, NB, T, SWIGLU, NT, SC, ext>, gemv_kernel<NB, T, SWIGLU, ext>, gemv_mfma_kernel<SEG, T,
 * SWIGLU, NT, ext>, gemv_fp8_kernel<KC, NB, T, SWIGLU, NT>, gemv_fp8_mfma_kernel<SEG, T, SWIGLU, NT> (csm_gemv_fp8w_kext_rows:
 * the same two with a trailing ", ext2"), lora_project_kernel<NB>,
 * lora_project_rows_kernel<NB>, gemv_t_kernel<NB, T>; ext0 = no K-extension, ext1 = csm_gemv_bf16_kext, ext2 = _kext_rows. */
const char* csm_gemv_last_kernel(void);
/* csm_gemv_bf16 with the neighbouring element-wise steps of a decode layer fused in: norm_scale != NULL applies torchtune
 * RMSNorm (eps) to x first; swiglu = 1 reads W as interleaved gate/up rows (N = 2F) and writes y[b][F] = silu(g) * u;
 * row_index != NULL takes batch row b of x from row (row_index[b] + row_offset) of the table x (embedding lookup of a
 * sampled code, model.py:189-191). */
int csm_gemv_bf16_ex(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw, int ldx, int ldy,
                     int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index, int row_offset,
                     csm_stream_t stream);
/* Weight-only FP8 decode (since ABI 3, additive).  csm_quantize_rows_fp8: W bf16 [N][ldw] -> W8 [N][ldw8] OCP e4m3fn codes (not
 * fnuz) + scale fp32 [N]: per row amax = max |w|, scale = amax / 448 (a correctly rounded fp32 division; 1.0 for an all-zero row),
 * code = e4m3fn(w / scale) rounded to nearest even and saturating at +-448 - finite weights never give a NaN code.  Rows keep W's
 * order (interleaved gate/up rows and fused qkv rows need no special case).  K, ldw, ldw8 multiples of 8. */
int csm_quantize_rows_fp8(const void* W, void* W8, void* scale, int N, int K, int ldw, int ldw8, csm_stream_t stream);
/* csm_gemv_bf16_ex with the weight operand replaced by (W8, scale): y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k]), bf16
 * activations, products and sum in fp32, the scale applied once after the reduction and before the epilogue (SwiGLU: gate and
 * up are each scaled and rounded to bf16 first).  Same fusions and the same invariants as the bf16 products: fixed reduction
 * order, no atomics; B <= 4: row b bit-identical to the one-row launch; B = 5..16 (MFMA tiles on weights converted to bf16 in
 * registers, exactly): a row's bits depend only on its own operands.  Needs K % 16 == 0, K <= 8192, ldw8 % 16 == 0, W8 and x
 * 16-byte aligned. */
int csm_gemv_fp8w(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N, int K, int ldw8,
                  int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index, int row_offset,
                  csm_stream_t stream);
/* LoRA groups at decode time (since ABI 3, additive): t[b][0:kx] = scale * x^[b] . At (At [K][lda], a group's arena matrix),
 * rounded to bf16 once; x^ = x, or with norm_scale != NULL the RMSNorm of x exactly as csm_gemv_bf16_ex's prologue computes it.
 * B <= 4, kx a multiple of 8. */
int csm_lora_project_bf16(const void* x, const void* At, void* t, int B, int K, int kx, int ldx, int lda, int ldt, float scale,
                          const void* norm_scale, float eps, csm_stream_t stream);
/* csm_gemv_bf16_ex with a K-extension: output row n also takes sum_j ext_t[b][j] ext_B[n][j] (+ bias[n], bias may be NULL) before
 * the residual / SwiGLU / fp32-output epilogue (ext_B rows in W's row order: interleaved gate/up for swiglu).  kx <= 512, a
 * multiple of 8, 16-byte aligned rows.  ext_B all zeros (no bias): bit-identical to csm_gemv_bf16_ex; row b of a B-row launch is
 * bit-identical to the one-row launch on that row.  B <= 4. */
int csm_gemv_bf16_kext(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw, int ldx, int ldy,
                       int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index, int row_offset,
                       const void* ext_t, const void* ext_B, int kx, int ld_ext_t, int ld_ext_B, const void* bias,
                       csm_stream_t stream);
/* Per-row LoRA adapters at decode time (since ABI 3, additive): a bank of n_adapters adapters that share kx and the strides; batch
 * row b uses adapter row_adapter[b] (int32 [B] on the device; -1 = none).  At / ext_B / bias are DEVICE arrays of n_adapters
 * pointers (each 16-byte aligned; a bias entry, or the whole bias table, may be NULL), scale fp32 [n_adapters] on the device.
 * B = 1..16.
 * csm_lora_project_rows_bf16: t[b] = scale[a] * x^[b] . At[a], a = row_adapter[b]; each row bit-identical to a one-row
 * csm_lora_project_bf16 launch with that row's At and scale; rows without adapter get zeros. */
int csm_lora_project_rows_bf16(const void* x, const void* const* At, void* t, const int* row_adapter, const float* scale,
                               int n_adapters, int B, int K, int kx, int ldx, int lda, int ldt, const void* norm_scale, float eps,
                               csm_stream_t stream);
/* csm_gemv_bf16_kext_rows: csm_gemv_bf16_ex with row b extended by its own adapter a = row_adapter[b]: sum_j ext_t[b][j]
 * ext_B[a][n][j] (+ bias[a][n]).  B <= 4: row b bit-identical to a one-row csm_gemv_bf16_kext with adapter a.  B = 5..16: a row's
 * bits depend only on its own operands (any B in 5..16, any position, any batch-mates).  A row without adapter is bit-identical to
 * csm_gemv_bf16_ex at the same B. */
int csm_gemv_bf16_kext_rows(const void* x, const void* W, void* y, const void* residual, int B, int N, int K, int ldw, int ldx,
                            int ldy, int out_f32, const void* norm_scale, float eps, int swiglu, const int* row_index, int row_offset,
                            const void* ext_t, const void* const* ext_B, const void* const* bias, const int* row_adapter,
                            int n_adapters, int kx, int ld_ext_t, int ld_ext_B, csm_stream_t stream);
/* csm_gemv_fp8w_kext_rows (since ABI 3, additive): csm_gemv_fp8w with row b extended by its own adapter a = row_adapter[b], the
 * bank of csm_gemv_bf16_kext_rows on the quantised base:  y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k] + sum_j ext_t[b][j]
 * ext_B[a][n][j] + bias[a][n]).  The scaled base sum is csm_gemv_fp8w's, operation for operation; the extension (never scaled: t
 * and ext_B are bf16 numbers the quantiser never saw) is summed in fp32 in a fixed order and added to it, then the adapter's bias,
 * then the epilogue (SwiGLU: gate and up rounded to bf16 after extension and bias).  B <= 4: row b bit-identical to the one-row
 * launch on that row with adapter a.  B = 5..16: a row's bits depend only on its own operands (any B in 5..16, any position, any
 * batch-mates and their adapters).  A row with a = -1 or a >= n_adapters takes no extension: bit-identical to csm_gemv_fp8w at
 * the same B.  Tables as for csm_gemv_bf16_kext_rows; kx <= 512 and a multiple of 8, extension rows 16-byte aligned; everything
 * csm_gemv_fp8w requires of K, ldw8 and alignment.  csm_gemv_last_kernel() names these launches with a trailing ext2, e.g.
 * "gemv_fp8_kernel<2, 4, bf16, 0, 1, ext2>"; csm_gemv_fp8w's launches keep their names without it. */
int csm_gemv_fp8w_kext_rows(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N, int K,
                            int ldw8, int ldx, int ldy, int out_f32, const void* norm_scale, float eps, int swiglu,
                            const int* row_index, int row_offset, const void* ext_t, const void* const* ext_B,
                            const void* const* bias, const int* row_adapter, int n_adapters, int kx, int ld_ext_t, int ld_ext_B,
                            csm_stream_t stream);
/* y[b][n] = sum_k x[b][k] W[k][n]  (K-major weights: audio_head[i] = [decoder_dim][vocab]) */
int csm_gemv_t_bf16(const void* x, const void* W, void* y, int B, int N, int K, int ldw, int ldx, int ldy, int out_f32,
                    csm_stream_t stream);
/* caches are [B][KV][S_max][HD] bf16; pos = int32 [B] on the device (graph-replayable): the new key/value row index */
/* a depth-decoder layer's rotate + cache append + attention (<= 64 cached positions, head_dim 128) + output projection
 * (+ residual) as ONE launch: y[B][N] = attention(qkv row, caches) . W[N][H*HD]^T + residual; bit-identical to
 * csm_attn_decode_rope followed by csm_gemv_bf16 (model.py:181-187 runs 31 such steps per frame). */
int csm_gemv_attn_bf16(const void* qkv, void* kcache, void* vcache, const int* pos, const float* rope_table, const void* W, void* y,
                       const void* residual, int B, int N, int H, int KV, int HD, int S_max, int ld_qkv, int ldw, int ldy,
                       csm_stream_t stream);
/* csm_attn_decode_rope for rows that share a position the host knows (round 4: the depth decoder's step i of a batch of utterances):
 * all loads of the prologue at once, coalesced key / value images; HD = 128, H = 4 KV, S_max <= 32; bit-identical to it. */
int csm_attn_decode_rope_at(const void* qkv, void* kcache, void* vcache, void* out, int pos, const float* rope_table, int B, int H,
                            int KV, int HD, int S_max, int ld, csm_stream_t stream);
/* the same for one utterance (B = 1) whose position the host knows (round 4: the depth decoder's step i is always at position i,
 * so a captured frame graph carries it as an argument): every address of the prologue is known at launch and all its loads
 * go out at once.  S_max <= 32, H * HD = 1024; bit-identical to csm_gemv_attn_bf16. */
int csm_gemv_attn_at_bf16(const void* qkv, void* kcache, void* vcache, int pos, const float* rope_table, const void* W, void* y,
                          const void* residual, int N, int H, int KV, int HD, int S_max, int ldw, csm_stream_t stream);
/* copies the (already rotated) new k and v heads of qkv[b] into row pos[b] of the caches; like csm_attn_decode, which reads them
 * back: HD 64 or 128, H % KV == 0, 1 <= S_max <= 8192, ld % 8 == 0 - anything else returns 1 */
int csm_kv_append(const void* qkv, void* kcache, void* vcache, const int* pos, int B, int H, int KV, int HD, int S_max, int ld,
                  csm_stream_t stream);
/* Context shift of a parked history (what DecodeState.park_row returns): src bf16 [layers][2][KV][len][HD], K plane before V
 * plane, -> dst bf16 [layers][2][KV][len - drop][HD] without positions keep .. keep+drop-1.  Positions p < keep and every V are
 * copied bit for bit; a K at p >= keep is src's K at p + drop with each interleaved pair rotated by -drop positions: (c, s) of
 * row `drop` of the table csm_rope reads, the sine negated, fp32 with one rounding to bf16 - the key rope(k, p + drop) becomes
 * rope(k, p).  Out of place: dst must not overlap src.  len / keep / drop are host integers.  Returns 1 (nothing launched) for
 * a null pointer, HD other than 64 / 128, layers or KV < 1, drop < 1, keep < 0, keep + drop > len, len - drop < 1,
 * drop >= table_rows, src or dst not 16-byte aligned, overlapping ranges. */
int csm_kv_shift(const void* src, void* dst, const float* rope_table, int table_rows, int layers, int KV, int HD, int len, int keep,
                 int drop, csm_stream_t stream);
/* The rows form of DecodeState.resume_row: R (1 .. 16) parked histories into R rows of a stack's cache allocation in ONE launch.
 * Segment r: src[r] bf16 [layers][2][KV][len[r]][HD] (what DecodeState.park_row returns) goes to positions 0 .. len[r]-1 of batch
 * row rows[r] of kv bf16 [layers][2][B][KV][S_max][HD], bit for bit, and pos[rows[r]] = len[r] - 1 (a device vector of B ints) is
 * written by the same launch.  Nothing else is written: not the row's positions from len[r] on, not another row, not another
 * row's pos.  The same source may be named by several segments (one voice prompt forked into many requests).  src / rows / len
 * are HOST arrays of R entries: they travel by value in the kernel arguments (no device table, no copy, no synchronisation).
 * Returns 1 (nothing launched) for a null pointer (src[r] included), R outside 1 .. 16, len[r] outside 1 .. S_max, a row outside
 * 0 .. B-1 or named twice, HD other than 64 / 128, layers / B / KV / S_max < 1, a source or cache that is not 16-byte aligned, a
 * source that overlaps the cache. */
int csm_kv_fork_rows(const void* const* src, void* kv, int* pos, const int* rows, const int* len, int R, int layers, int B, int KV,
                     int HD, int S_max, csm_stream_t stream);
/* The mirror of csm_kv_fork_rows, the rows form of DecodeState.park_row: positions 0 .. len[r]-1 of batch row rows[r] of kv bf16
 * [layers][2][B][KV][S_max][HD] go to dst[r] bf16 [layers][2][KV][len[r]][HD], bit for bit, R (1 .. 16) rows in ONE launch - what
 * a server takes out of its slots when it preempts utterances.  The cache is only read and no position vector is an argument
 * (the lengths come from the caller's host mirror); only the R destinations are written.  dst / rows / len are HOST arrays of R
 * entries and travel by value in the kernel arguments.  Returns 1 (nothing launched) for a null pointer (dst[r] included), R
 * outside 1 .. 16, len[r] outside 1 .. S_max, a row outside 0 .. B-1 or named twice, HD other than 64 / 128, layers / B / KV /
 * S_max < 1, a destination or cache that is not 16-byte aligned, a destination that overlaps the cache or another destination. */
int csm_kv_park_rows(void* const* dst, const void* kv, const int* rows, const int* len, int R, int layers, int B, int KV, int HD,
                     int S_max, csm_stream_t stream);
/* The rings of the processed / typical rows samplers, moved row by row in ONE launch: for r < R (1 .. 16) the ring
 * code_hist[rows[r]] (int32 [K][64] of code_hist [B][K][64]) and the counter hist_frame[rows[r]] against row r of packed int32
 * [R][K * 64 + 1] (the ring, then the counter).  to_state = 0 reads the state and writes only packed; to_state = 1 reads packed and
 * writes only the named rows' rings and counters.  hist_live is no argument.  rows is a HOST array, by value in the kernel
 * arguments.  Returns 1 (nothing launched) for a null pointer, R outside 1 .. 16, B < 1, K outside 1 .. 4096, a direction other than 0 / 1, a row
 * outside 0 .. B-1 or named twice, a buffer that is not 4-byte aligned, a packed buffer that overlaps the state's. */
int csm_sample_hist_move_rows(int* code_hist, int* hist_frame, int* packed, const int* rows, int R, int B, int K, int to_state,
                              csm_stream_t stream);
/* out[b][h*HD..] = softmax(q . K[0..pos[b]]^T / sqrt(HD)) V   for the single query row in qkv[b].  HD 64 or 128, H % KV == 0,
 * 1 <= S_max <= 8192 (the scores live in LDS), ld % 8 == 0 (16-byte loads from qkv + b * ld) - anything else returns 1 */
int csm_attn_decode(const void* qkv, const void* kcache, const void* vcache, void* out, const int* pos, int B, int H, int KV,
                    int HD, int S_max, int ld, csm_stream_t stream);
/* the same with what precedes it in a decode step fused in: q and the new k are rotated inside (table as for csm_rope,
 * position = pos[b]) and the new k / v are appended to the caches at pos[b] by the kernel itself - one launch instead of
 * csm_rope + csm_kv_append + csm_attn_decode. qkv is the UNROTATED fused projection row.  The same shapes as csm_attn_decode
 * (HD 64 / 128, H % KV == 0, 1 <= S_max <= 8192, ld % 8 == 0) and a non-null table; anything else returns 1. */
int csm_attn_decode_rope(const void* qkv, void* kcache, void* vcache, void* out, const int* pos, const float* rope_table, int B,
                         int H, int KV, int HD, int S_max, int ld, csm_stream_t stream);
/* n new positions pos0 .. pos0+n-1 of ONE sequence (batch row `row` of the caches) against what the cache already holds - a
 * conversation's next turn.  qkv [n][(H+2KV)*HD] with q and k ALREADY rotated for those positions (csm_rope with pos); the kernel
 * writes the n new K / V rows into cache rows pos0 .. pos0+n-1 and computes, for query i, softmax over cache positions 0 .. pos0+i
 * (fp32 statistics and accumulation) into out [n][H*HD].  Nothing is read back by the host.  HD = 64, H / KV in {1, 2, 4}.
 * The bits of an output row depend only on that row's q, its absolute position and the keys / values up to that position - not
 * on n, pos0 or the other rows of the launch: one launch of n rows equals any split of it into consecutive launches.
 * The number of batch rows of the caches is not an argument: `row` < B is the caller's to check (csm/hip/ops.py does). */
int csm_attn_append(const void* qkv, void* kcache, void* vcache, void* out, int row, int pos0, int n, int H, int KV, int HD,
                    int S_max, float scale, csm_stream_t stream);
/* The ragged form: R (1 .. 16) segments in ONE launch.  Segment r is n[r] >= 1 new positions from pos0[r] of the sequence in
 * batch row rows[r] of the caches; its q / k / v are rows off[r] .. off[r]+n[r]-1 of the stacked qkv [sum n][(H+2KV)*HD], off[r] =
 * n[0] + .. + n[r-1], and it writes the same rows of out [sum n][H*HD] and its K / V into its own cache row.  rows / pos0 / n are
 * HOST arrays of R ints: they travel by value in the kernel arguments (no device table, no copy, no synchronisation).  The tile
 * body is csm_attn_append's, so every output row and cache row has the bits the same segment gets from a csm_attn_append launch
 * of its own.  Returns 1 (nothing launched) for a null pointer, R outside 1 .. 16, n[r] < 1, positions outside the cache,
 * HD != 64, H / KV not in {1, 2, 4}, a negative row or a cache row named by two segments; rows[r] < B is the caller's to check. */
int csm_attn_append_rows(const void* qkv, void* kcache, void* vcache, void* out, const int* rows, const int* pos0, const int* n, int R,
                         int H, int KV, int HD, int S_max, float scale, csm_stream_t stream);

/* ---- K16 (RVQ part): Mimi split residual VQ behind generator.py:117,209 ------------------------------------------ */
int csm_rvq_encode(const float* x, const float* codebooks, long long* codes, int T, int K, int C, int D, int n_semantic,
                   csm_stream_t stream);
int csm_rvq_decode(const long long* codes, const float* codebooks, float* out, int T, int K, int C, int D,
                   csm_stream_t stream);

/* ---- K16 (rest): Mimi codec around the RVQ - SEANet convolutions and the two 8-layer codec transformers, fp32 -------- *
 * (moshi MimiModel.encode / decode behind generator.py:67-70,117,209).  Activations are [C][T] for the convolutions and
 * [T][D] for the transformers. */
int csm_conv1d_f32(const float* x, const float* w, const float* bias, const float* residual, float* y, int C_in, int C_out,
                   int T_in, int T_out, int k, int stride, int dilation, int pad_left, int pad_mode /*0 zero,1 replicate*/,
                   int groups, int elu_in, csm_stream_t stream);
int csm_conv_transpose1d_f32(const float* x, const float* w, const float* bias, float* y, int C_in, int C_out, int T_in, int T_out,
                             int k, int stride, int crop_left, int groups, int elu_in, csm_stream_t stream);
int csm_layernorm_f32(const float* x, const float* w, const float* b, float* y, int T, int D, float eps, csm_stream_t stream);
/* y = act(x W^T); scale != NULL: y = residual + scale[n] * y (layer scale); else y += residual when given; act 1 = GELU */
int csm_linear_f32(const float* x, const float* W, const float* scale, const float* residual, float* y, int T, int N, int K,
                   int ldx, int act, csm_stream_t stream);
int csm_rope_half_f32(float* qkv, int T, int H, int head_dim, float base, int pos0, csm_stream_t stream);
int csm_attn_window_f32(const float* qkv, float* out, int T, int H, int head_dim, int window, csm_stream_t stream);
int csm_transpose_f32(const float* in, float* out, int R, int C, csm_stream_t stream);
/* Streaming (chunk-by-chunk) forms of the causal decoder ops, additive since ABI 3.  Each computes every output with the same
 * arithmetic as its full-sequence twin, so a decoder that carries the state below is bit-identical to a whole-sequence decode.
 * conv1d: causal stride-1 conv over [hist | x], x = [C_in][n] new columns, hist = the previous (k-1)*dilation input columns
 * (zeros at the start of a sequence; may be NULL when k == 1); y = [C_out][n] (bias / residual / input ELU as csm_conv1d_f32);
 * the next history (last (k-1)*dilation columns of [hist | x]) goes to hist_out, which must not alias hist. */
int csm_conv1d_stream_f32(const float* hist, const float* x, const float* w, const float* bias, const float* residual, float* y,
                          float* hist_out, int C_in, int C_out, int n, int k, int dilation, int groups, int elu_in, csm_stream_t stream);
/* The same for stride >= 1 (the encoder's downsampling convs; additive since ABI 3): x = [C_in][n_in] new columns, n_in a
 * multiple of stride (refused otherwise); hist / hist_out = [C_in][H], H = (k-1)*dilation + 1 - stride >= 0 (csm_conv1d_f32's
 * pad_left; may exceed n_in; NULL when H == 0); y / residual = [C_out][n_in / stride], every output with the arithmetic
 * csm_conv1d_f32 uses for the same absolute output.  edge_first != 0: hist is not read (may be NULL) and every history column is
 * column 0 of x - pad_mode 1's left edge, for the first chunk of an edge-replicated conv. */
int csm_conv1d_stream_strided_f32(const float* hist, const float* x, const float* w, const float* bias, const float* residual, float* y,
                                  float* hist_out, int C_in, int C_out, int n_in, int k, int stride, int dilation, int groups,
                                  int elu_in, int edge_first, csm_stream_t stream);
/* transposed conv (causal: crop_left 0) for n new input columns at absolute input position pos0; hist = the previous
 * ceil(k/stride)-1 input columns; y = [C_out][n*stride]; next history to hist_out (as above). */
int csm_conv_transpose1d_stream_f32(const float* hist, const float* x, const float* w, const float* bias, float* y, float* hist_out,
                                    int C_in, int C_out, int n, int pos0, int k, int stride, int groups, int elu_in, csm_stream_t stream);
/* csm_attn_window_f32 for the n rows of qkv [n][3*H*head_dim] (post-RoPE) at positions pos0..pos0+n-1: keys before pos0 are read
 * from kcache / vcache ([ring][H*head_dim], position p in slot p % ring) and the n new k / v rows are appended there.  Needs
 * ring >= window + n - 1 (the slots read and written in one launch must not overlap). */
int csm_attn_window_stream_f32(const float* qkv, float* kcache, float* vcache, float* out, int n, int pos0, int H, int head_dim,
                               int window, int ring, csm_stream_t stream);
/* Rows forms of the streaming ops, additive since ABI 3: R = 1..16 utterances with the same chunk size n in ONE launch, each
 * with its own state slot.  Activations gain a leading row dimension (x [R][C_in][n], y [R][C_out][..]; qkv / out [R*n][..]);
 * state arenas gain a leading slot dimension of n_slots.  `slots`, `parity` and `pos0` are HOST arrays of R ints, handed to the
 * kernel by value: no device buffer, no copy, no synchronisation.  slots[r] in [0, n_slots), all distinct.  Every row is
 * computed with the arithmetic of the one-row op above on its own slot, so its output has that op's bits.
 * Convolutions: hist_arena = [n_slots][2][C_in][H] (H as above; NULL when H == 0): row r reads history buffer parity[r] of its
 * slot and writes the next history to buffer parity[r] ^ 1 (the caller flips its per-slot parity after the step). */
int csm_conv1d_stream_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias, const float* residual, float* y,
                               int R, const int* slots, const int* parity, int n_slots, int C_in, int C_out, int n, int k,
                               int dilation, int groups, int elu_in, csm_stream_t stream);
/* csm_conv1d_stream_strided_f32 for R rows with the same n_in (the encoder's downsampling convs; additive since ABI 3):
 * x = [R][C_in][n_in], y / residual = [R][C_out][n_in / stride], hist_arena = [n_slots][2][C_in][H], H = (k-1)*dilation + 1 - stride
 * (may exceed n_in; NULL when H == 0).  Bit r of edge_first_mask: row r is the first chunk of an edge-replicated conv - its
 * history is not read, every history column is column 0 of that row's x.  Refused, with nothing launched: R outside 1..16, a slot
 * out of range or named twice, a parity other than 0 / 1, a mask bit at or above R, n_in not a multiple of stride, H < 0, H > 0
 * with a NULL arena. */
int csm_conv1d_stream_strided_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias, const float* residual,
                                       float* y, int R, const int* slots, const int* parity, unsigned edge_first_mask, int n_slots,
                                       int C_in, int C_out, int n_in, int k, int stride, int dilation, int groups, int elu_in,
                                       csm_stream_t stream);
/* pos0[r]: absolute input position of row r's first new column */
int csm_conv_transpose1d_stream_rows_f32(float* hist_arena, const float* x, const float* w, const float* bias, float* y, int R,
                                         const int* slots, const int* parity, const int* pos0, int n_slots, int C_in, int C_out,
                                         int n, int k, int stride, int groups, int elu_in, csm_stream_t stream);
/* csm_rope_half_f32 on qkv [R*n][3*H*head_dim]: row r's n positions are pos0[r] .. pos0[r]+n-1 */
int csm_rope_half_rows_f32(float* qkv, int R, const int* pos0, int n, int H, int head_dim, float base, csm_stream_t stream);
/* kcache / vcache = [n_slots][ring][H*head_dim]; row r at positions pos0[r] .. pos0[r]+n-1 of slot slots[r] */
int csm_attn_window_stream_rows_f32(const float* qkv, float* kcache, float* vcache, float* out, int R, const int* slots,
                                    const int* pos0, int n_slots, int n, int H, int head_dim, int window, int ring,
                                    csm_stream_t stream);
/* out[b][c][r] = in[b][r][c] for b < batch */
int csm_transpose_rows_f32(const float* in, float* out, int batch, int R, int C, csm_stream_t stream);

/* Band-limited sample-rate conversion (csrc/resample.hip), additive since ABI 3: the windowed-sinc polyphase interpolation of
 * csm.data.resample.  A rate pair is given reduced - o / n = sr_in / sr_out in lowest terms - with its filter half-width `width`
 * in input samples; T = 2 * width + o taps per phase; taps = [n][T] fp32 on the device, built by the host.
 *     y[j] = sum_{t = 0 .. T-1} taps[j mod n][t] * xbar[(j div n) * o - width + t],   xbar = x inside [0, N), 0 outside,
 * summed in fp32 by one fmaf chain in ascending t - in every form below, so the forms agree bit for bit.
 * Refused for every form: o == n (equal rates), o / n not in lowest terms, T > 2048, n * T > 4 Mi table entries (16 MB).  Tables
 * of up to 14336 padded floats (56 KB) are staged in LDS, larger ones are read from global memory.
 * One-shot: x [R][N] -> y [R][M], M = ceil(n * N / o); N == 0 launches nothing. */
int csm_resample_f32(const float* x, const float* taps, float* y, int R, long long N, int o, int n, int width, csm_stream_t stream);
/* R = 1..16 streams in ONE launch.  `x` (R device pointers), `slots`, `parity`, `n_in` and `pos` are HOST arrays of R entries,
 * handed to the kernel by value: no device buffer, no copy, no synchronisation, nothing read back.  Row r continues the stream of
 * slot slots[r] (all distinct, in [0, n_slots)) with its next n_in[r] samples x[r][0 .. n_in[r]); pos[r] is the number of samples
 * the stream had before this call (the caller's integer mirror).  carry_arena = [n_slots][2][T - 1]: buffer parity[r] of the slot
 * holds the stream's last T - 1 samples (all zeros for a new stream: the caller zeroes the slot when it opens it) and the next
 * carry goes to buffer parity[r] ^ 1 (the caller flips its per-slot parity after the step).
 * After N' samples the output blocks q < max(0, floor((N' - width - o) / o) + 1) are computable (n outputs each); the call writes
 * the outputs of the blocks that became computable to y[r][0 ..) (y = [R][ldy]) - the caller knows how many from the same
 * integers.  Bit r of
 * final_mask: row r's stream ends with this call - the samples past its end are zeros and it emits every remaining j < M of its
 * total length.  Every output has the bits csm_resample_f32 gives it for the same absolute j, however the input was cut.
 * Refused, with nothing launched: R outside 1..16, a slot out of range or named twice, a parity other than 0 / 1, a mask bit at
 * or above R, n_in[r] above max_in (the capacity the stream was made with) or below 1 (0 is allowed with the row's final bit: a
 * flush with nothing new), a row that would emit more than ldy outputs, a negative position. */
int csm_resample_stream_rows_f32(float* carry_arena, const float* const* x, const float* taps, float* y, long long ldy, int R,
                                 const int* slots, const int* parity, const int* n_in, const long long* pos, unsigned final_mask,
                                 int n_slots, int max_in, int o, int n, int width, csm_stream_t stream);
/* The same for one stream: carry = [2][T - 1]; csm_resample_stream_rows_f32 with R = 1, slot 0 of 1. */
int csm_resample_stream_f32(float* carry, int parity, const float* x, int n_in, long long pos, int final, const float* taps, float* y,
                            long long ldy, int max_in, int o, int n, int width, csm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSM_HIP_H */
