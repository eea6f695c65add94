// Host entry points of the gfx950 kernels: every lwc_* launcher, declared once.
// The .hip file that defines a launcher includes this header, and so does bindings.cpp which calls it; the
// symbols have C linkage, so a definition whose parameters disagree with the declaration here does not compile.
// A launcher validates nothing but what only it can know (it returns non-zero when it refuses a shape); the
// pointers it takes are device pointers that bindings.cpp has checked.  Strides (ld*, *_stride) are in elements.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

extern "C" {

// ---- norm.hip: residual (in/out, optional) is updated in place; y optional in the quantising form
int lwc_rmsnorm(const void* x, void* residual, const void* w, void* y, int rows, int d, float eps, hipStream_t s);
int lwc_rmsnorm_quant_fp8(const void* x, void* residual, const void* w, void* y, int rows, int d, float eps, void* q,
                          float* qscale, hipStream_t s);
int lwc_layernorm(const void* x, const void* residual, const void* pre_bias, const void* g, const void* b, void* y,
                  int rows, int d, float eps, hipStream_t s);
int lwc_rms_rowsumsq(const void* x, float* ss, int rows, int d, hipStream_t s);

// ---- elementwise.hip, qknorm.hip: qkv [T, (Hq + 2 Hkv) * D]; kc [NB, Hkv, BS, D], vc [NB, Hkv, BS/4, D, 4]
int lwc_rope_kv_write(void* qkv, const int* positions, const int* slots, const float* cos_t, const float* sin_t,
                      void* kc, void* vc, int T, int Hq, int Hkv, int D, int BS, int rope_q, hipStream_t s);
int lwc_qknorm_rope_kv_write(void* qkv, const int* positions, const int* slots, const float* cos_t, const float* sin_t,
                             void* kc, void* vc, const void* bias, const void* qw, const void* kw, int T, int Hq,
                             int Hkv, int D, int BS, int rope_q, float eps, hipStream_t s);
int lwc_silu_mul(const void* in, void* out, int T, int F, int blk, hipStream_t s);
int lwc_embedding_gather(const void* table, const int* ids, void* out, int T, int d, int V, hipStream_t s);
int lwc_kv_gather(const void* kc, const void* vc, const long long* slots, void* ko, void* vo, int n, int Hkv, int D,
                  int BS, hipStream_t s);
// pairs [P, 2] (src block, dst block), applied to each of the LK [NB, block_elems] planes of cache
int lwc_kv_block_copy(void* cache, const int* pairs, int P, int LK, int NB, long long block_elems, hipStream_t s);

// ---- attention_decode.hip: q rows of q_stride elements; block_tables [B, max_blocks]
int lwc_set_decode_wave_min_items(int n);
int lwc_paged_decode(const void* q, int q_stride, const void* kc, const void* vc, const int* block_tables,
                     const int* ctx_lens, void* out, float* part_o, float* part_lse, int B, int Hq, int Hkv, int D,
                     int BS, int max_blocks, int num_splits, float scale, const float* rope_cos, const float* rope_sin,
                     const int* positions, hipStream_t s);
// tiles [max_tiles, 3] (row_start, nseq, prefix_blocks); out, or out8 (e4m3) + mx [Hq, mx_rows, 4] (e8m0)
int lwc_paged_decode_cascade(const void* q, int q_stride, const void* kc, const void* vc, const int* block_tables,
                             const int* ctx_lens, const int* tiles, int max_tiles, void* out, int Hq, int Hkv, int D,
                             int BS, int max_blocks, float scale, const float* rope_cos, const float* rope_sin,
                             const int* positions, void* out8, void* mx, int mx_rows, hipStream_t s);
int lwc_cascade_rows_per_tile(int G);

// ---- attention_prefill.hip: cu_seqlens [nseq + 1]; cu_seqlens_k optional
int lwc_prefill_attention(const void* q, const void* k, const void* v, void* out, const int* cu_seqlens,
                          const int* cu_seqlens_k, int nseq, int max_seqlen, int q_stride, int k_stride, int v_stride,
                          int o_stride, int Hq, int Hkv, int D, float scale, int causal, hipStream_t s);
int lwc_prefill_attention_mx(const void* q, const void* k, const void* v, void* out8, void* mx, int mx_rows,
                             const int* cu_seqlens, int nseq, int max_seqlen, int q_stride, int k_stride, int v_stride,
                             int o8_stride, int Hq, int Hkv, float scale, int causal, hipStream_t s);
int lwc_prefill_attention_paged(const void* q, const void* kc, const void* vc, void* out, const int* cu_seqlens,
                                const int* block_tables, const int* k_lens, int bt_stride, int nseq, int max_seqlen,
                                int q_stride, int o_stride, int Hq, int Hkv, int D, float scale, hipStream_t s);

// ---- gemm.hip, gemm8p.hip, gemm4w.hip, skinny.hip, gemm8g.hip: C = A . W^T, A / C rows of lda / ldc elements
// W [G, N, K] with w_group_stride elements per group; c32 [rows, N] fp32 when splits > 1
int lwc_grouped_gemm(const void* A, const void* W, void* C, const int* row_off, const float* a_scale,
                     const float* w_scale, const void* bias, const int* a_rows, int G, int max_slots, int N, int K,
                     int lda, int ldc, long long w_group_stride, int fp8, float* c32, int splits, long long rows,
                     hipStream_t s);
int lwc_gemm8p_slots();
// ws: one fp32 256 x 256 tile per slot; flags: one int per slot, zero between calls
int lwc_gemm8p(const void* A, const void* W, void* C, const void* R, float* ws, int* flags, int M, int N, int K,
               int lda, int ldc, int epi, hipStream_t s);
// ss [partials, ssld] fp32 row sums of squares (rs_mode 1 reads P of them, 2 writes N / 256); part / cnt: split-K
int lwc_gemm4w(const void* A, const void* W, void* C, const void* R, int M, int N, int K, int lda, int ldc, int epi,
               int bn, float* ss, int ssld, int rs_mode, int P, float eps, int var, int gm, int splits, int split_from,
               float* part, int* cnt, hipStream_t s);
int lwc_skinny_gemm(const void* A, const void* W, void* C, const void* R, int M, int N, int K, int lda, int ldc,
                    int epi, hipStream_t s);
// a_mx [K / 128, s_rows, 4] / mx_out [N / 256, s_rows, 4] e8m0 planes
int lwc_gemm8g_fp8(const void* A, const void* W, void* C, const int* row_off, const int* a_rows, const float* a_scale,
                   const float* w_scale, int G, int max_slots, int N, int K, int lda, int ldc, int rows_a, int rows_c,
                   int mode, const void* a_mx, void* mx_out, int s_rows, hipStream_t s);

// ---- mxfp4.hip, mxfp4_a8.hip: Q [N, K / 2] e2m1 pairs, S [N, K / 32] e8m0
int lwc_mxfp4_dequant(const void* q, const void* s, void* out, long long N, long long K, hipStream_t st);
int lwc_skinny_mxfp4(const void* A, const void* Q, const void* S, void* C, int M, int N, int K, int lda, int ldc,
                     int epi, hipStream_t s);
int lwc_gemm_mxfp4_a8(const void* A, const float* a_scale, const void* Q, const void* S, void* C, int M, int N, int K,
                      int lda, int ldc, int epi, hipStream_t s);

// ---- moe_mxfp4.hip: Q [E, N, K / 2], S [E, N, K / 32]; row_off [E + 1]; a_rows [rows] optional (else A has >= rows
// rows, expert-major); A has a_nrows rows
int lwc_moe_skinny_mxfp4(const void* A, const void* Q, const void* S, void* C, const int* row_off, const int* a_rows,
                         int E, long long rows, long long a_nrows, int N, int K, int lda, int ldc, int epi,
                         hipStream_t s);
// ---- moe_mxfp4_a8.hip: the same stack; A e4m3 [a_nrows, lda], a_scale [a_nrows] (both read through a_rows)
int lwc_moe_gemm_mxfp4_a8(const void* A, const float* a_scale, const void* Q, const void* S, void* C,
                          const int* row_off, const int* a_rows, int E, int rows, long long a_nrows, int N, int K,
                          int lda, int ldc, int epi, hipStream_t s);

// ---- lora.hip: A [n_adapters, R, K], B [n_adapters, N, R], ids [M]
int lwc_lora_shrink(const void* X, const void* A, const int* ids, void* T, int M, int K, int R, int ldx,
                    int n_adapters, hipStream_t s);
int lwc_lora_expand_add(void* Y, const void* T, const void* B, const int* ids, int M, int N, int R, int ldy,
                        int n_adapters, hipStream_t s);

// ---- moe.hip: topk_ids / topk_w / src_row / inv [T * k], row_off [E + 1]
int lwc_silu_mul_quant_fp8(const void* gu, int rows, int F, int blk, void* q, float* scale, hipStream_t s);
int lwc_moe_route(const void* logits, int T, int E, int k, int* topk_ids, float* topk_w, int* row_off, int* src_row,
                  int* inv, hipStream_t s);
int lwc_moe_router(const void* h, int ldh, const void* router, int T, int E, int d, int k, int* topk_ids,
                   float* topk_w, int* row_off, int* src_row, int* inv, void* logits, hipStream_t s);
int lwc_moe_combine(const void* Y, const int* inv, const float* w, int T, int k, int d, void* out, hipStream_t s);
int lwc_quant_fp8_rows(const void* x, int rows, int d, void* q, float* scale, hipStream_t s);

// ---- moe_wide.hip: the same outputs for 16 < E <= 128, 1 <= k <= 8; anything else is refused (-1)
int lwc_moe_route_wide(const void* logits, int T, int E, int k, int* topk_ids, float* topk_w, int* row_off,
                       int* src_row, int* inv, hipStream_t s);
int lwc_moe_router_wide(const void* h, int ldh, const void* router, int T, int E, int d, int k, int* topk_ids,
                        float* topk_w, int* row_off, int* src_row, int* inv, void* logits, hipStream_t s);
int lwc_moe_permute_wide(const int* topk_ids, int T, int E, int k, int* row_off, int* src_row, int* inv,
                         hipStream_t s);

// ---- ep.hip: send / recv [W, (C + 1) * RB] bytes; row_bytes / out_bytes: one row of x in bytes
int lwc_ep_pack(const void* x, const float* xs, const int* src, const int* row_off, int W, int El, int C, int RB,
                int row_bytes, void* send, hipStream_t s);
int lwc_ep_unpack(const void* recv, int W, int El, int C, int RB, int row_bytes, int has_scale, void* x_local,
                  float* s_local, int* map, int* row_off_local, hipStream_t s);
int lwc_ep_back(const void* y_local, const int* map, int W, int C, int out_bytes, void* back, hipStream_t s);
int lwc_ep_combine(const void* ret, const int* row_off, const int* inv, const float* w, int T, int E, int El, int C,
                   int k, int d, void* out, hipStream_t s);

// ---- sampler.hip: logits rows of ld elements; every per-row table holds >= B entries, the optional ones may be null
int lwc_sample(const void* logits, int ld, int V, int B, const float* temperature, const float* top_p,
               const int* top_k, const float* min_p, const float* top_a, const float* freq_pen, const float* pres_pen,
               const float* rep_pen, void* counts, const int* count_rows, const float* bias, const int* bias_rows,
               const unsigned int* mask, const int* mask_rows, const unsigned long long* seeds,
               const unsigned long long* offsets, int num_logprobs, int mask_logprobs, int need_logprob,
               int* out_token, float* out_logprob, int* out_topk_ids, float* out_topk_lp, hipStream_t s);

// ---- consensus.hip
int lwc_vote_tally(const double* V, const double* w, const unsigned char* valid, int R, int L, int C, double* cw,
                   double* conf, double* vconf, hipStream_t s);
int lwc_knn_topk(const float* E, int n, int d, const float* q, int k, float* part_v, int* part_i, float* vals,
                 int* rows, hipStream_t s);
int lwc_pool_l2norm(const void* hidden, int ld, const int* cu, int nseq, int d, int mode, float* out_f32,
                    void* out_bf16, hipStream_t s);
int lwc_cosine_consensus(const void* E, int R, int n, int d, float* S, float inv_tau, float* centrality,
                         float* weights, int* best, hipStream_t s);

// ---- allreduce.hip: bases [W] IPC regions of lwc_ar_region_bytes(W, cap) bytes each; err: one int flag
long long lwc_ar_region_bytes(int W, long long cap);
int lwc_ar_alloc(long long bytes, void** ptr, void* handle);
int lwc_ar_open(const void* handle, void** ptr);
int lwc_ar_close(void* ptr);
int lwc_ar_free(void* ptr);
int lwc_ar_handle_bytes();
int lwc_allreduce(void* const* bases, int me, int W, const void* x, void* out, long long n, long long cap, int* err,
                  int blocks, long long spin_limit, hipStream_t s);
int lwc_alltoall(void* const* bases, int me, int W, const void* send, void* recv, long long chunk, long long cap,
                 int* err, int blocks, long long spin_limit, hipStream_t s);

}  // extern "C"
