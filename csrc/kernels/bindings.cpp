// torch <-> HIP kernel bindings for llm_weighted_consensus_amd.ops._kernels.
// Every op: validates device/dtype/shape on the host (a kernel must never see operands whose shape
// disagrees with its grid), then launches on the caller's current HIP stream so it can be captured
// into a hipGraph by torch.cuda.CUDAGraph.
// The rule: every pointer handed to a launcher comes out of flat / strided / opt_flat / opt_strided below or out
// of a special-layout helper built on them (check_v_cache, q_rope, mxfp4_check_weight, plane_rows, ...), which
// check device, dtype and layout and name the binding and the operand when they refuse.  data_ptr appears
// nowhere else, except on tensors a binding has just allocated itself.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <climits>

#include "launchers.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHECK_RC(rc, name) TORCH_CHECK((rc) == 0, name, " launch failed with code ", (rc))

constexpr auto BF16 = at::kBFloat16, FP8 = at::kFloat8_e4m3fn, F32 = at::kFloat, I32 = at::kInt, U8 = at::kByte;
using OptTensor = c10::optional<at::Tensor>;

// ---- the operand vocabulary.  who: the binding, name: the operand, as the error message spells them.

bool present(const OptTensor& t) { return t.has_value() && t->defined(); }

struct Numel {
  int64_t n;
  bool exact;
};
Numel exactly(int64_t n) { return {n, true}; }
Numel at_least(int64_t n) { return {n, false}; }

void check_device_dtype(const at::Tensor& t, at::ScalarType dt, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda(), who, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, who, ": ", name, " has dtype ", t.scalar_type(), ", expected ", dt);
}

// Flat: a contiguous GPU tensor of dtype dt that the kernel indexes through one pointer.
template <typename T = void>
T* flat(const at::Tensor& t, at::ScalarType dt, const char* who, const char* name, Numel n = at_least(0)) {
  check_device_dtype(t, dt, who, name);
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK(n.exact ? t.numel() == n.n : t.numel() >= n.n, who, ": ", name, " has ", t.numel(),
              " elements, expected ", n.exact ? "" : "at least ", n.n);
  return static_cast<T*>(t.data_ptr());
}

// Rows: a 2-D GPU tensor of dtype dt with unit inner stride; the kernel takes the row stride ld (elements),
// which is a multiple of align.
struct Strided {
  void* p = nullptr;
  int ld = 0;
};
Strided strided(const at::Tensor& t, at::ScalarType dt, const char* who, const char* name, int64_t align = 1) {
  check_device_dtype(t, dt, who, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, who, ": ", name, " must be 2-D with unit inner stride");
  TORCH_CHECK(t.stride(0) % align == 0 && t.stride(0) <= INT_MAX, who, ": ", name, " rows must be ",
              align * t.element_size(), "-byte aligned (row stride ", t.stride(0), " elements, below 2^31)");
  return {t.data_ptr(), (int)t.stride(0)};
}

// Optional: absent gives null, present is checked like a required operand.
template <typename T = void>
T* opt_flat(const OptTensor& t, at::ScalarType dt, const char* who, const char* name, Numel n = at_least(0)) {
  return present(t) ? flat<T>(*t, dt, who, name, n) : nullptr;
}
Strided opt_strided(const OptTensor& t, at::ScalarType dt, const char* who, const char* name, int64_t align = 1) {
  return present(t) ? strided(*t, dt, who, name, align) : Strided{};
}

// ---- special layouts

// V cache of one layer: [NB, Hkv, BS/4, D, 4] bf16, the 4-token interleaved layout of the decode kernels.
void* check_v_cache(const at::Tensor& v, const at::Tensor& k, const char* who) {
  TORCH_CHECK(v.dim() == 5 && v.size(0) == k.size(0) && v.size(1) == k.size(1) && v.size(2) * 4 == k.size(2) &&
                  v.size(3) == k.size(3) && v.size(4) == 4,
              who, ": v_cache must be [NB, Hkv, BS/4, D, 4] matching k_cache [NB, Hkv, BS, D]");
  return flat(v, BF16, who, "v_cache");
}

// The decode attention kernels are instantiated for head_dim 64 and 128 and carry a KV head's query heads as
// MFMA rows, so at most 16 of them; the error names the shape that was asked for.
void check_decode_shape(int D, int Hq, int Hkv, const char* who) {
  TORCH_CHECK(D == 64 || D == 128, who, ": head_dim ", D, ": decode attention takes 64 or 128");
  TORCH_CHECK(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 16, who, ": ", Hq, " heads / ", Hkv,
              " kv heads (GQA group ", Hkv > 0 ? Hq / Hkv : 0, "): decode attention takes whole groups up to 16");
}

// Optional q rotation inside the decode kernels: (cos [max_pos, D/2] fp32, sin, positions [B] int32) all
// given or none.
struct QRope {
  const float* cos = nullptr;
  const float* sin = nullptr;
  const int* pos = nullptr;
};
QRope q_rope(const OptTensor& c, const OptTensor& s, const OptTensor& pos, int B, int D, const char* who) {
  if (!present(c) && !present(s) && !present(pos)) return {};
  TORCH_CHECK(present(c) && present(s) && present(pos), who, ": rope needs cos, sin and positions");
  TORCH_CHECK(c->dim() == 2 && c->size(1) == D / 2 && s->sizes() == c->sizes(), who, ": rope table shape");
  return {flat<float>(*c, F32, who, "rope_cos"), flat<float>(*s, F32, who, "rope_sin"),
          flat<int>(*pos, I32, who, "positions", at_least(B))};
}

// ---- norms

void rmsnorm(const at::Tensor& x, const OptTensor& residual, const at::Tensor& w, at::Tensor& out, double eps) {
  const char* who = "rmsnorm";
  const void* xp = flat(x, BF16, who, "x");
  const int d = (int)x.size(-1);
  const int rows = (int)(x.numel() / std::max<int64_t>(d, 1));
  CHECK_RC(lwc_rmsnorm(xp, opt_flat(residual, BF16, who, "residual", exactly(x.numel())),
                       flat(w, BF16, who, "w", exactly(d)), flat(out, BF16, who, "out", exactly(x.numel())), rows, d,
                       (float)eps, cur_stream()),
           who);
}

void rmsnorm_quant_fp8(const at::Tensor& x, const OptTensor& residual, const at::Tensor& w, const OptTensor& out,
                       at::Tensor& q, at::Tensor& scale, double eps) {
  // K1 + K11e: RMSNorm (+ residual update) whose output is also quantised per row to e4m3 (q, scale);
  // out (the bf16 output) is optional.  d in {2048, 4096, 8192}.
  const char* who = "rmsnorm_quant_fp8";
  const void* xp = flat(x, BF16, who, "x");
  const int d = (int)x.size(-1);
  const int rows = (int)(x.numel() / std::max<int64_t>(d, 1));
  TORCH_CHECK(d == 2048 || d == 4096 || d == 8192, who, ": d must be 2048, 4096 or 8192");
  CHECK_RC(lwc_rmsnorm_quant_fp8(xp, opt_flat(residual, BF16, who, "residual", exactly(x.numel())),
                                 flat(w, BF16, who, "w", exactly(d)),
                                 opt_flat(out, BF16, who, "out", exactly(x.numel())), rows, d, (float)eps,
                                 flat(q, FP8, who, "q", exactly(x.numel())),
                                 flat<float>(scale, F32, who, "scale", at_least(rows)), cur_stream()),
           who);
}

void layernorm(const at::Tensor& x, const OptTensor& residual, const at::Tensor& g, const at::Tensor& b,
               at::Tensor& out, double eps, const OptTensor& pre_bias) {
  const char* who = "layernorm";
  const void* xp = flat(x, BF16, who, "x");
  const int d = (int)x.size(-1);
  const int rows = (int)(x.numel() / std::max<int64_t>(d, 1));
  CHECK_RC(lwc_layernorm(xp, opt_flat(residual, BF16, who, "residual", exactly(x.numel())),
                         opt_flat(pre_bias, BF16, who, "pre_bias", exactly(d)), flat(g, BF16, who, "g", exactly(d)),
                         flat(b, BF16, who, "b", exactly(d)), flat(out, BF16, who, "out", exactly(x.numel())), rows, d,
                         (float)eps, cur_stream()),
           who);
}

// ss[r] = sum(x[r]^2): the single partial of the folded RMSNorm for the first projection of a chain
void rms_rowsumsq(const at::Tensor& x, at::Tensor& ss) {
  const char* who = "rms_rowsumsq";
  const void* xp = flat(x, BF16, who, "x");
  TORCH_CHECK(x.dim() == 2, who, ": x [M, d], ss [>= M]");
  CHECK_RC(lwc_rms_rowsumsq(xp, flat<float>(ss, F32, who, "ss", at_least(x.size(0))), (int)x.size(0), (int)x.size(1),
                            cur_stream()),
           who);
}

// ---- RoPE + KV write

// What rope_kv_write and qknorm_rope_kv_write (its Qwen form) share: qkv [T, (Hq + 2 Hkv) * D] bf16, positions
// and slots [T] int32, cos / sin [max_pos, D / 2] fp32, k_cache [NB, Hkv, BS, D], v_cache [NB, Hkv, BS/4, D, 4]
// (4-token interleaved).
struct RopeKv {
  void* qkv;
  const int *pos, *slots;
  const float *cos, *sin;
  void *kc, *vc;
  int T, BS;
};
RopeKv rope_kv_operands(const at::Tensor& qkv, const at::Tensor& positions, const OptTensor& slots,
                        const at::Tensor& cos_t, const at::Tensor& sin_t, const at::Tensor& k_cache,
                        const at::Tensor& v_cache, int64_t Hq, int64_t Hkv, int64_t D, const char* who) {
  RopeKv r;
  r.qkv = flat(qkv, BF16, who, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (Hq + 2 * Hkv) * D, who, ": qkv row is not (Hq+2Hkv)*D");
  r.T = (int)qkv.size(0);
  r.pos = flat<int>(positions, I32, who, "positions", exactly(r.T));
  r.slots = opt_flat<int>(slots, I32, who, "slots", exactly(r.T));
  r.cos = flat<float>(cos_t, F32, who, "cos_t");
  r.sin = flat<float>(sin_t, F32, who, "sin_t");
  TORCH_CHECK(cos_t.dim() == 2 && sin_t.dim() == 2 && cos_t.size(1) == D / 2 && sin_t.size(1) == D / 2 &&
                  cos_t.size(0) == sin_t.size(0),
              who, ": cos/sin table shape");
  r.kc = flat(k_cache, BF16, who, "k_cache");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(1) == Hkv && k_cache.size(3) == D, who, ": k_cache shape");
  r.vc = check_v_cache(v_cache, k_cache, who);
  r.BS = (int)k_cache.size(2);
  return r;
}

void rope_kv_write(at::Tensor& qkv, const at::Tensor& positions, const OptTensor& slots, const at::Tensor& cos_t,
                   const at::Tensor& sin_t, at::Tensor& k_cache, at::Tensor& v_cache, int64_t Hq, int64_t Hkv,
                   int64_t D, bool rope_q) {
  const char* who = "rope_kv_write";
  TORCH_CHECK(Hq > 0 && Hkv > 0 && D > 0 && D % 16 == 0, who, ": needs Hq, Hkv >= 1 and head_dim % 16 == 0");
  const RopeKv r = rope_kv_operands(qkv, positions, slots, cos_t, sin_t, k_cache, v_cache, Hq, Hkv, D, who);
  CHECK_RC(lwc_rope_kv_write(r.qkv, r.pos, r.slots, r.cos, r.sin, r.kc, r.vc, r.T, (int)Hq, (int)Hkv, (int)D, r.BS,
                             rope_q ? 1 : 0, cur_stream()),
           who);
}

// rope_kv_write with the Qwen attention-block steps in front of the rotation (csrc/kernels/qknorm.hip): the
// q|k|v projection bias and the per-head RMSNorm of q and k, each optional.  head_dim 128 only.
void qknorm_rope_kv_write(at::Tensor& qkv, const at::Tensor& positions, const OptTensor& slots,
                          const at::Tensor& cos_t, const at::Tensor& sin_t, at::Tensor& k_cache, at::Tensor& v_cache,
                          int64_t Hq, int64_t Hkv, int64_t D, bool rope_q, const OptTensor& bias,
                          const OptTensor& q_weight, const OptTensor& k_weight, double eps) {
  const char* who = "qknorm_rope_kv_write";
  TORCH_CHECK(D == 128, who, ": head_dim must be 128 (what the decode attention kernels take), got ", D);
  TORCH_CHECK(Hq > 0 && Hkv > 0 && Hkv * D <= 4096, who, ": needs 1 <= Hkv <= 32 and Hq >= 1");
  const RopeKv r = rope_kv_operands(qkv, positions, slots, cos_t, sin_t, k_cache, v_cache, Hq, Hkv, D, who);
  CHECK_RC(lwc_qknorm_rope_kv_write(r.qkv, r.pos, r.slots, r.cos, r.sin, r.kc, r.vc,
                                    opt_flat(bias, BF16, who, "bias", exactly((Hq + 2 * Hkv) * D)),
                                    opt_flat(q_weight, BF16, who, "q_weight", exactly(D)),
                                    opt_flat(k_weight, BF16, who, "k_weight", exactly(D)), r.T, (int)Hq, (int)Hkv,
                                    (int)D, r.BS, rope_q ? 1 : 0, (float)eps, cur_stream()),
           who);
}

// ---- elementwise, KV cache

void silu_mul(const at::Tensor& in, at::Tensor& out, int64_t block) {
  const char* who = "silu_mul";
  const void* ip = flat(in, BF16, who, "in");
  void* op = flat(out, BF16, who, "out");
  const int F = (int)out.size(-1);
  const int T = (int)(out.numel() / std::max(F, 1));
  TORCH_CHECK(in.size(-1) == 2 * F && in.numel() == 2 * out.numel(), who, ": shape mismatch");
  TORCH_CHECK(block == 0 || (block % 8 == 0 && F % block == 0), who, ": block must divide F, multiple of 8");
  CHECK_RC(lwc_silu_mul(ip, op, T, F, (int)block, cur_stream()), who);
}

void embedding(const at::Tensor& table, const at::Tensor& ids, at::Tensor& out) {
  const char* who = "embedding";
  const void* tp = flat(table, BF16, who, "table");
  const int T = (int)ids.numel(), d = (int)table.size(1);
  CHECK_RC(lwc_embedding_gather(tp, flat<int>(ids, I32, who, "ids"), flat(out, BF16, who, "out", exactly((int64_t)T * d)),
                                T, d, (int)table.size(0), cur_stream()),
           who);
}

void kv_gather(const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& slots, at::Tensor& ko, at::Tensor& vo) {
  // kc [NB, Hkv, BS, D], vc [NB, Hkv, BS/4, D, 4] (one layer), slots [n] int64 (< NB*BS, checked by the
  // caller's block manager), ko/vo [n, Hkv*D] contiguous bf16
  const char* who = "kv_gather";
  const void* kp = flat(kc, BF16, who, "kc");
  const void* vp = flat(vc, BF16, who, "vc");
  TORCH_CHECK(kc.dim() == 4 && vc.dim() == 5, who, ": cache layouts");
  const int Hkv = (int)kc.size(1), BS = (int)kc.size(2), D = (int)kc.size(3);
  const int n = (int)slots.numel();
  TORCH_CHECK(ko.dim() == 2 && vo.dim() == 2 && ko.size(0) == n && vo.size(0) == n && ko.size(1) == Hkv * D &&
                  vo.size(1) == Hkv * D,
              who, ": output shapes");
  CHECK_RC(lwc_kv_gather(kp, vp, flat<long long>(slots, at::kLong, who, "slots"), flat(ko, BF16, who, "ko"),
                         flat(vo, BF16, who, "vo"), n, Hkv, D, BS, cur_stream()),
           who);
}

void kv_block_copy(at::Tensor& cache, const at::Tensor& pairs) {
  // cache: [L*2, NB, ...block...]
  const char* who = "kv_block_copy";
  void* cp = flat(cache, BF16, who, "cache");
  const int* pp = flat<int>(pairs, I32, who, "pairs");
  TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, who, ": pairs must be [P, 2]");
  const int LK = (int)cache.size(0), NB = (int)cache.size(1);
  const long long be = cache.numel() / ((long long)LK * NB);
  CHECK_RC(lwc_kv_block_copy(cp, pp, (int)pairs.size(0), LK, NB, be, cur_stream()), who);
}

// ---- decode attention

void paged_decode(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                  const at::Tensor& block_tables, const at::Tensor& ctx_lens, at::Tensor& out, const OptTensor& part_o,
                  const OptTensor& part_lse, int64_t num_splits, double scale, const OptTensor& rope_cos,
                  const OptTensor& rope_sin, const OptTensor& positions) {
  // q: [B, >= Hq*D] with row stride; out: [B, Hq, D]
  const char* who = "paged_decode";
  const Strided qs = strided(q, BF16, who, "q");
  const void* kp = flat(k_cache, BF16, who, "k_cache");
  void* op = flat(out, BF16, who, "out");
  const int B = (int)out.size(0), Hq = (int)out.size(1), D = (int)out.size(2);
  const int Hkv = (int)k_cache.size(1), BS = (int)k_cache.size(2);
  check_decode_shape(D, Hq, Hkv, who);
  TORCH_CHECK(k_cache.size(3) == D, who, ": out is [B, Hq, ", D, "] but the cache has head_dim ", k_cache.size(3));
  TORCH_CHECK(q.size(0) == B && q.size(1) >= Hq * D, who, ": q shape");
  const void* vp = check_v_cache(v_cache, k_cache, who);
  const int* bt = flat<int>(block_tables, I32, who, "block_tables");
  TORCH_CHECK(block_tables.size(0) == B, who, ": batch mismatch");
  const int* cl = flat<int>(ctx_lens, I32, who, "ctx_lens", exactly(B));
  float* po = nullptr;
  float* pl = nullptr;
  if (num_splits > 1) {
    TORCH_CHECK(present(part_o) && present(part_lse), who, ": split-K needs workspaces");
    po = flat<float>(*part_o, F32, who, "part_o", at_least((int64_t)B * Hq * num_splits * D));
    pl = flat<float>(*part_lse, F32, who, "part_lse", at_least((int64_t)B * Hq * num_splits));
  }
  const QRope qr = q_rope(rope_cos, rope_sin, positions, B, D, who);
  CHECK_RC(lwc_paged_decode(qs.p, qs.ld, kp, vp, bt, cl, op, po, pl, B, Hq, Hkv, D, BS, (int)block_tables.size(1),
                            (int)num_splits, (float)scale, qr.cos, qr.sin, qr.pos, cur_stream()),
           who);
}

void paged_decode_cascade(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                          const at::Tensor& block_tables, const at::Tensor& ctx_lens, const at::Tensor& tiles,
                          const OptTensor& out, int64_t Hq, double scale, const OptTensor& rope_cos,
                          const OptTensor& rope_sin, const OptTensor& positions, const OptTensor& out8,
                          const OptTensor& mx) {
  // tiles: [max_tiles, 3] int32 super-tiles (row_start, nseq, prefix_blocks), nseq <= cascade_rows_per_tile(G);
  // the engine builds them on the host (rows must stay < B: the kernel trusts the table).
  // out8 + mx instead of out: e4m3 rows [B, Hq * D] with e8m0 scales [Hq, >= B, 4] (one per 32 dims of a head)
  const char* who = "paged_decode_cascade";
  const Strided qs = strided(q, BF16, who, "q");
  const void* kp = flat(k_cache, BF16, who, "k_cache");
  const bool mxo = present(out8);
  TORCH_CHECK(mxo == present(mx), who, ": out8 and mx go together");
  TORCH_CHECK(mxo || present(out), who, ": out or out8 + mx");
  const void* vp = check_v_cache(v_cache, k_cache, who);
  const int* tp = flat<int>(tiles, I32, who, "tiles");
  TORCH_CHECK(tiles.dim() == 2 && tiles.size(1) == 3, who, ": tiles must be [T, 3]");
  const int B = (int)q.size(0), D = (int)k_cache.size(3), Hkv = (int)k_cache.size(1), BS = (int)k_cache.size(2);
  check_decode_shape(D, (int)Hq, Hkv, who);
  TORCH_CHECK(q.size(1) >= Hq * D, who, ": q rows shorter than Hq * D");
  const int* bt = flat<int>(block_tables, I32, who, "block_tables");
  TORCH_CHECK(block_tables.size(0) >= B, who, ": batch tables too short");
  const int* cl = flat<int>(ctx_lens, I32, who, "ctx_lens", at_least(B));
  void* outp = nullptr;
  void* o8 = nullptr;
  void* mxp = nullptr;
  int mx_rows = 0;
  if (mxo) {
    o8 = flat(*out8, FP8, who, "out8", at_least((int64_t)B * Hq * D));
    mxp = flat(*mx, U8, who, "mx");
    TORCH_CHECK(D == 128, who, ": head_dim ", D, ": the MX output takes head_dim 128 only");
    TORCH_CHECK(mx->dim() == 3 && mx->size(0) == Hq && mx->size(1) >= B && mx->size(2) == 4, who,
                ": mx must be [Hq, B, 4] (head_dim 128)");
    mx_rows = (int)mx->size(1);
  } else {
    outp = flat(*out, BF16, who, "out", at_least((int64_t)B * Hq * D));
  }
  const QRope qr = q_rope(rope_cos, rope_sin, positions, B, D, who);
  CHECK_RC(lwc_paged_decode_cascade(qs.p, qs.ld, kp, vp, bt, cl, tp, (int)tiles.size(0), outp, (int)Hq, Hkv, D, BS,
                                    (int)block_tables.size(1), (float)scale, qr.cos, qr.sin, qr.pos, o8, mxp, mx_rows,
                                    cur_stream()),
           who);
}

// ---- GEMMs

void grouped_gemm(const at::Tensor& A, const at::Tensor& W, at::Tensor& C, const at::Tensor& row_off, int64_t max_slots,
                  const OptTensor& a_scale, const OptTensor& w_scale, const OptTensor& bias, const OptTensor& a_rows,
                  int64_t splits) {
  // A [rows, K] (bf16 | fp8 e4m3fn, unit inner stride), W [G, N, K] contiguous, C [rows, N] bf16,
  // row_off [G+1] int32 on the device (group boundaries; the kernel trusts them to be <= rows).
  const char* who = "grouped_gemm";
  const bool fp8 = A.scalar_type() == FP8;  // A / W both bf16 or both e4m3fn
  const Strided a = strided(A, fp8 ? FP8 : BF16, who, "A"), c = strided(C, BF16, who, "C");
  const void* wp = flat(W, fp8 ? FP8 : BF16, who, "W");
  TORCH_CHECK(W.dim() == 3, who, ": W must be [G, N, K]");
  const int G = (int)W.size(0), N = (int)W.size(1), K = (int)W.size(2);
  TORCH_CHECK(A.size(1) == K && C.size(1) == N, who, ": shape mismatch");
  const int* ar = opt_flat<int>(a_rows, I32, who, "a_rows", at_least(C.size(0)));
  TORCH_CHECK(present(a_rows) || C.size(0) >= A.size(0), who, ": C rows < A rows");
  const int* ro = flat<int>(row_off, I32, who, "row_off", exactly(G + 1));
  const float* as = nullptr;
  const float* ws = nullptr;
  if (fp8) {
    TORCH_CHECK(present(a_scale) && present(w_scale), who, ": fp8 needs a_scale and w_scale");
    as = flat<float>(*a_scale, F32, who, "a_scale", at_least(A.size(0)));
    ws = flat<float>(*w_scale, F32, who, "w_scale", exactly((int64_t)G * N));
  }
  const void* b = opt_flat(bias, BF16, who, "bias", exactly((int64_t)G * N));
  TORCH_CHECK(splits >= 1, who, ": splits must be >= 1");
  at::Tensor c32;  // split-K: fp32 accumulation buffer over all output rows
  if (splits > 1) c32 = at::zeros({C.size(0), N}, C.options().dtype(at::kFloat));
  CHECK_RC(lwc_grouped_gemm(a.p, wp, c.p, ro, as, ws, b, ar, G, (int)max_slots, N, K, a.ld, c.ld, (long long)N * K,
                            fp8 ? 1 : 0, splits > 1 ? c32.data_ptr<float>() : nullptr, (int)splits,
                            (long long)C.size(0), cur_stream()),
           who);
}

// Operand checks shared by the MFMA GEMM cores (who: gemm8p, gemm4w or skinny_gemm); r is the epilogue operand
// (residual / bias) or null.
struct GemmOperands {
  Strided a, c;
  const void *w, *r;
  int M, N, K;
};
GemmOperands gemm_operands(const at::Tensor& A, const at::Tensor& W, const at::Tensor& C, const OptTensor& R,
                           int64_t epi, const char* who) {
  // epi 0: C[M, N] = A . W^T; 1: + R; 2: C[M, N/2] = silu(gate) * up over a 32-row gate/up interleaved W;
  // 3: + bias (R = bias [N]); 4: gelu(. + bias)
  GemmOperands g;
  g.a = strided(A, BF16, who, "A", 8);
  g.c = strided(C, BF16, who, "C", 8);
  g.w = flat(W, BF16, who, "W");
  TORCH_CHECK(W.dim() == 2, who, ": W must be [N, K]");
  TORCH_CHECK(epi >= 0 && epi <= 4, who, ": epi must be 0..4");
  g.M = (int)A.size(0), g.K = (int)A.size(1), g.N = (int)W.size(0);
  const int NC = epi == 2 ? g.N / 2 : g.N;
  TORCH_CHECK(W.size(1) == g.K && C.size(0) == g.M && C.size(1) == NC, who, ": shape mismatch");
  TORCH_CHECK(g.K % 64 == 0 && g.N % (epi == 2 ? 64 : 8) == 0, who,
              ": needs K % 64 == 0, N % 8 == 0 (SwiGLU: N % 64 == 0)");
  g.r = nullptr;
  if (epi == 1) {
    g.r = opt_strided(R, BF16, who, "R").p;
    TORCH_CHECK(present(R) && R->sizes() == C.sizes() && R->strides() == C.strides(), who,
                ": epi 1 needs a residual that matches C");
  }
  if (epi == 3 || epi == 4) {
    TORCH_CHECK(present(R), who, ": bias epilogue needs a bias");
    g.r = flat(*R, BF16, who, "bias", exactly(g.N));
  }
  return g;
}

void gemm8p(const at::Tensor& A, const at::Tensor& W, at::Tensor& C, const OptTensor& R, int64_t epi, at::Tensor& ws,
            at::Tensor& flags) {
  const char* who = "gemm8p";
  const GemmOperands g = gemm_operands(A, W, C, R, epi, who);
  // stream-K workspace: one fp32 256x256 partial tile and one flag per workgroup (flags zero between calls)
  const int slots = lwc_gemm8p_slots();
  CHECK_RC(lwc_gemm8p(g.a.p, g.w, g.c.p, g.r, flat<float>(ws, F32, who, "ws", at_least((int64_t)slots * 65536)),
                      flat<int>(flags, I32, who, "flags", at_least(slots)), g.M, g.N, g.K, g.a.ld, g.c.ld, (int)epi,
                      cur_stream()),
           who);
}

// gemm4w: the 4-wave interleaved core (one wave per SIMD, data-parallel tiles of 256 x bn, bn = 256 | 192).
// Folded RMSNorm (gemm4w.hip head): rs_mode 1 (epi 0 / 2) reads ss [>= P, M] fp32 partial row sums of squares
// and scales the accumulator rows by rsqrt(sum / K + eps); rs_mode 2 (epi 1, bn 256) writes ss [N/256, M].
void gemm4w(const at::Tensor& A, const at::Tensor& W, at::Tensor& C, const OptTensor& R, int64_t epi, int64_t bn,
            const OptTensor& ss, int64_t rs_mode, int64_t P, double eps, int64_t var, int64_t gm, int64_t splits,
            int64_t split_from, const OptTensor& part, const OptTensor& cnt) {
  const char* who = "gemm4w";
  const GemmOperands g = gemm_operands(A, W, C, R, epi, who);
  const int M = g.M, N = g.N;
  TORCH_CHECK(bn == 256 || bn == 192, who, ": bn must be 256 or 192");
  TORCH_CHECK(epi != 2 || bn == 256, who, ": SwiGLU needs bn 256");
  float* ssp = nullptr;
  if (rs_mode) {
    TORCH_CHECK(present(ss), who, ": rs_mode needs ss");
    ssp = flat<float>(*ss, F32, who, "ss");
    TORCH_CHECK(ss->dim() == 2 && ss->size(1) >= M && ss->size(1) % 4 == 0, who, ": ss [partials, >= M (x4)]");
    if (rs_mode == 1) {
      TORCH_CHECK(epi == 0 || epi == 2, who, ": row scales go with the plain or SwiGLU epilogue");
      TORCH_CHECK(P >= 1 && P <= 16 && ss->size(0) >= P, who, ": ss needs P (1..16) partials");
    } else {
      TORCH_CHECK(rs_mode == 2 && epi == 1 && bn == 256, who, ": row sums of squares need the residual epilogue, bn 256");
      TORCH_CHECK(ss->size(0) >= (N + 255) / 256, who, ": ss needs N/256 partials");
    }
  }
  // split-K workspace, checked here against what the kernel will index (a short buffer would fault)
  const long long tiles = (long long)((M + 255) / 256) * ((N + bn - 1) / bn);
  const long long split_tiles = tiles - std::min<long long>(std::max<long long>(split_from, 0), tiles);
  TORCH_CHECK(splits <= 1 || (present(part) && present(cnt)), who, ": split-K needs part and cnt");
  float* pp = opt_flat<float>(part, F32, who, "part", at_least(splits > 1 ? split_tiles * (splits - 1) * 256 * bn : 0));
  int* cp = opt_flat<int>(cnt, I32, who, "cnt", at_least(splits > 1 ? 2 * tiles : 0));
  CHECK_RC(lwc_gemm4w(g.a.p, g.w, g.c.p, g.r, M, N, g.K, g.a.ld, g.c.ld, (int)epi, (int)bn, ssp,
                      ssp ? (int)ss->size(1) : 0, (int)rs_mode, (int)P, (float)eps, (int)var, (int)gm, (int)splits,
                      (int)split_from, pp, cp, cur_stream()),
           who);
}

// skinny GEMM (decode-sized M <= 64): C = A . W^T (epi 0), R + A . W^T (epi 1, R may be C) or the SwiGLU of
// a 32-row gate/up interleaved W (epi 2, C [M, N / 2])
void skinny_gemm(const at::Tensor& A, const at::Tensor& W, at::Tensor& C, const OptTensor& R, int64_t epi) {
  const char* who = "skinny_gemm";
  TORCH_CHECK(epi >= 0 && epi <= 2, who, ": epi 0 (plain), 1 (residual) or 2 (SwiGLU)");
  const GemmOperands g = gemm_operands(A, W, C, R, epi, who);
  TORCH_CHECK(g.M <= 64 && g.K % 2048 == 0 && g.N % 16 == 0, who, ": needs M <= 64, K % 2048 == 0, N % 16 == 0");
  CHECK_RC(lwc_skinny_gemm(g.a.p, g.w, g.c.p, g.r, g.M, g.N, g.K, g.a.ld, g.c.ld, (int)epi, cur_stream()), who);
}

// MXFP4 weight (mxfp4.hip): q [N, K / 2] uint8 (two e2m1 codes per byte), s [N, K / 32] uint8 (e8m0)
struct Mxfp4Weight {
  const void *q, *s;
};
Mxfp4Weight mxfp4_check_weight(const at::Tensor& q, const at::Tensor& s, const char* who) {
  const Mxfp4Weight w{flat(q, U8, who, "q"), flat(s, U8, who, "s")};
  TORCH_CHECK(q.dim() == 2 && s.dim() == 2 && s.size(0) == q.size(0) && q.size(1) == 16 * s.size(1), who,
              ": q must be [N, K / 2] and s [N, K / 32] with K % 32 == 0");
  return w;
}

// out [N, K] bf16 (caller-owned) = the dequantised weight, exact
void mxfp4_dequant(const at::Tensor& q, const at::Tensor& s, at::Tensor& out) {
  const char* who = "mxfp4_dequant";
  const Mxfp4Weight w = mxfp4_check_weight(q, s, who);
  void* op = flat(out, BF16, who, "out");
  const int64_t N = q.size(0), K = 2 * q.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == N && out.size(1) == K, who, ": out must be [N, K] = [", N, ", ", K, "]");
  CHECK_RC(lwc_mxfp4_dequant(w.q, w.s, op, (long long)N, (long long)K, cur_stream()), who);
}

// skinny GEMM over an MXFP4 weight (M <= 64): C = A . W^T (epi 0) or the SwiGLU of a 32-row gate/up interleaved W
// (epi 2, C [M, N / 2])
void skinny_mxfp4(const at::Tensor& A, const at::Tensor& q, const at::Tensor& s, at::Tensor& C, int64_t epi) {
  const char* who = "skinny_mxfp4";
  TORCH_CHECK(epi == 0 || epi == 2, who, ": epi 0 (plain) or 2 (SwiGLU)");
  const Mxfp4Weight w = mxfp4_check_weight(q, s, who);
  const Strided a = strided(A, BF16, who, "A"), c = strided(C, BF16, who, "C");
  const int64_t M = A.size(0), K = A.size(1), N = q.size(0);
  const int64_t NC = epi == 2 ? N / 2 : N;
  TORCH_CHECK(2 * q.size(1) == K && C.size(0) == M && C.size(1) == NC, who, ": shape mismatch (A [", M, ", ", K,
              "], W [", N, ", ", 2 * q.size(1), "], C [", C.size(0), ", ", C.size(1), "])");
  TORCH_CHECK(M <= 64 && K % 128 == 0 && N % (epi == 2 ? 64 : 16) == 0, who,
              ": needs M <= 64, K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0); got M = ", M, ", K = ", K,
              ", N = ", N);
  TORCH_CHECK(a.ld % 4 == 0 && c.ld % 4 == 0 && a.ld >= K && c.ld >= NC && (uintptr_t)a.p % 8 == 0 &&
                  (uintptr_t)c.p % 8 == 0,
              who, ": rows of A / C must be 8-byte aligned and not overlap");
  CHECK_RC(lwc_skinny_mxfp4(a.p, w.q, w.s, c.p, (int)M, (int)N, (int)K, a.ld, c.ld, (int)epi, cur_stream()), who);
}

// W4A8 GEMM over an MXFP4 weight (mxfp4_a8.hip): C = (Aq . W^T) * a_scale[row] (epi 0) or the SwiGLU of a 32-row
// gate/up interleaved W (epi 2, C [M, N / 2]); Aq e4m3 rows, any M
void gemm_mxfp4_a8(const at::Tensor& A, const at::Tensor& a_scale, const at::Tensor& q, const at::Tensor& s,
                   at::Tensor& C, int64_t epi) {
  const char* who = "gemm_mxfp4_a8";
  TORCH_CHECK(epi == 0 || epi == 2, who, ": epi 0 (plain) or 2 (SwiGLU)");
  const Mxfp4Weight w = mxfp4_check_weight(q, s, who);
  TORCH_CHECK(A.scalar_type() == FP8, who, ": A must be float8_e4m3fn, got ", A.scalar_type());
  const Strided a = strided(A, FP8, who, "A"), c = strided(C, BF16, who, "C");
  const int64_t M = A.size(0), K = A.size(1), N = q.size(0);
  const int64_t NC = epi == 2 ? N / 2 : N;
  TORCH_CHECK(2 * q.size(1) == K && C.size(0) == M && C.size(1) == NC, who, ": shape mismatch (A [", M, ", ", K,
              "], W [", N, ", ", 2 * q.size(1), "], C [", C.size(0), ", ", C.size(1), "])");
  TORCH_CHECK(a_scale.numel() == M, who, ": a_scale must hold one scale per row of A (", M, "), got ", a_scale.numel());
  const float* as = flat<float>(a_scale, F32, who, "a_scale");
  TORCH_CHECK(K > 0 && K % 128 == 0 && N % (epi == 2 ? 64 : 16) == 0, who,
              ": needs K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0); got K = ", K, ", N = ", N);
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), who, ": M, N and K must be below 2^31");
  TORCH_CHECK(M <= 1 || (a.ld % 16 == 0 && a.ld >= K && c.ld >= NC), who,
              ": rows of A must be 16-byte aligned, rows of A / C must not overlap");
  TORCH_CHECK((uintptr_t)a.p % 16 == 0 && (uintptr_t)w.q % 16 == 0 && (uintptr_t)w.s % 4 == 0, who,
              ": A and the weight's codes must be 16-byte aligned, its scales 4-byte aligned");
  // (a single row's stride is arbitrary in torch: hand the kernel one that passes its own checks)
  const int64_t lda = M <= 1 ? K : a.ld, ldc = M <= 1 ? NC : c.ld;
  CHECK_RC(lwc_gemm_mxfp4_a8(a.p, as, w.q, w.s, c.p, (int)M, (int)N, (int)K, (int)lda, (int)ldc, (int)epi,
                             cur_stream()),
           who);
}

// grouped skinny GEMM over a stack of MXFP4 expert weights (moe_mxfp4.hip): q [E, N, K / 2], s [E, N, K / 32];
// rows [row_off[e], row_off[e + 1]) of C are expert e's, computed from A[a_rows[row]] (a_rows given) or A[row]
void moe_skinny_mxfp4(const at::Tensor& A, const at::Tensor& q, const at::Tensor& s, at::Tensor& C,
                      const at::Tensor& row_off, const OptTensor& a_rows, int64_t epi) {
  const char* who = "moe_skinny_mxfp4";
  TORCH_CHECK(epi == 0 || epi == 2, who, ": epi 0 (plain) or 2 (SwiGLU)");
  const void *qp = flat(q, U8, who, "q"), *sp = flat(s, U8, who, "s");
  TORCH_CHECK(q.dim() == 3 && s.dim() == 3 && s.size(0) == q.size(0) && s.size(1) == q.size(1) &&
                  q.size(2) == 16 * s.size(2),
              who, ": q must be [E, N, K / 2] and s [E, N, K / 32] with K % 32 == 0");
  const Strided a = strided(A, BF16, who, "A"), c = strided(C, BF16, who, "C");
  const int64_t E = q.size(0), N = q.size(1), K = A.size(1), rows = C.size(0);
  const int64_t NC = epi == 2 ? N / 2 : N;
  TORCH_CHECK(2 * q.size(2) == K && C.size(1) == NC, who, ": shape mismatch (A [", A.size(0), ", ", K, "], W [", E,
              ", ", N, ", ", 2 * q.size(2), "], C [", rows, ", ", C.size(1), "])");
  TORCH_CHECK(K > 0 && K % 128 == 0 && N % (epi == 2 ? 64 : 16) == 0, who,
              ": needs K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0); got K = ", K, ", N = ", N);
  TORCH_CHECK(E >= 1 && E <= 65535 && N <= INT_MAX && K <= INT_MAX, who,
              ": E must be in [1, 65535], N and K below 2^31");
  TORCH_CHECK(row_off.dim() == 1, who, ": row_off must be 1-D [E + 1]");
  const int* ro = flat<int>(row_off, I32, who, "row_off", exactly(E + 1));
  const int* ar = opt_flat<int>(a_rows, I32, who, "a_rows", exactly(rows));
  TORCH_CHECK(present(a_rows) || A.size(0) >= rows, who, ": without a_rows A must hold C's ", rows, " rows, has ",
              A.size(0));
  TORCH_CHECK(a.ld % 4 == 0 && c.ld % 4 == 0 && a.ld >= K && c.ld >= NC && (uintptr_t)a.p % 8 == 0 &&
                  (uintptr_t)c.p % 8 == 0,
              who, ": rows of A / C must be 8-byte aligned and not overlap");
  CHECK_RC(lwc_moe_skinny_mxfp4(a.p, qp, sp, c.p, ro, ar, (int)E, (long long)rows, (long long)A.size(0), (int)N, (int)K,
                                a.ld, c.ld, (int)epi, cur_stream()),
           who);
}

// grouped W4A8 GEMM over a stack of MXFP4 expert weights (moe_mxfp4_a8.hip): rows [row_off[e], row_off[e + 1]) of C
// are expert e's, computed from the e4m3 row A[a_rows[row]] and its scale a_scale[a_rows[row]] (a_rows given) or
// A[row], a_scale[row]; any segment lengths
void moe_gemm_mxfp4_a8(const at::Tensor& A, const at::Tensor& a_scale, const at::Tensor& q, const at::Tensor& s,
                       at::Tensor& C, const at::Tensor& row_off, const OptTensor& a_rows, int64_t epi) {
  const char* who = "moe_gemm_mxfp4_a8";
  TORCH_CHECK(epi == 0 || epi == 2, who, ": epi 0 (plain) or 2 (SwiGLU)");
  const void *qp = flat(q, U8, who, "q"), *sp = flat(s, U8, who, "s");
  TORCH_CHECK(q.dim() == 3 && s.dim() == 3 && s.size(0) == q.size(0) && s.size(1) == q.size(1) &&
                  q.size(2) == 16 * s.size(2),
              who, ": q must be [E, N, K / 2] and s [E, N, K / 32] with K % 32 == 0");
  TORCH_CHECK(A.scalar_type() == FP8, who, ": A must be float8_e4m3fn, got ", A.scalar_type());
  const Strided a = strided(A, FP8, who, "A"), c = strided(C, BF16, who, "C");
  const int64_t E = q.size(0), N = q.size(1), K = A.size(1), rows = C.size(0), a_nrows = A.size(0);
  const int64_t NC = epi == 2 ? N / 2 : N;
  TORCH_CHECK(2 * q.size(2) == K && C.size(1) == NC, who, ": shape mismatch (A [", a_nrows, ", ", K, "], W [", E, ", ",
              N, ", ", 2 * q.size(2), "], C [", rows, ", ", C.size(1), "])");
  TORCH_CHECK(a_scale.numel() == a_nrows, who, ": a_scale must hold one scale per row of A (", a_nrows, "), got ",
              a_scale.numel());
  const float* as = flat<float>(a_scale, F32, who, "a_scale");
  TORCH_CHECK(K > 0 && K % 128 == 0 && N % (epi == 2 ? 64 : 16) == 0, who,
              ": needs K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0); got K = ", K, ", N = ", N);
  TORCH_CHECK(E >= 1 && E <= INT_MAX && rows <= INT_MAX && N <= INT_MAX && K <= INT_MAX, who,
              ": E must be at least 1; E, rows, N and K below 2^31");
  TORCH_CHECK(row_off.dim() == 1, who, ": row_off must be 1-D [E + 1]");
  const int* ro = flat<int>(row_off, I32, who, "row_off", exactly(E + 1));
  const int* ar = opt_flat<int>(a_rows, I32, who, "a_rows", exactly(rows));
  TORCH_CHECK(present(a_rows) || a_nrows >= rows, who, ": without a_rows A must hold C's ", rows, " rows, has ",
              a_nrows);
  TORCH_CHECK((a_nrows <= 1 || (a.ld % 16 == 0 && a.ld >= K)) && (rows <= 1 || c.ld >= NC), who,
              ": rows of A must be 16-byte aligned, rows of A / C must not overlap");
  TORCH_CHECK((uintptr_t)a.p % 16 == 0 && (uintptr_t)qp % 16 == 0 && (uintptr_t)sp % 4 == 0, who,
              ": A and the weights' codes must be 16-byte aligned, their scales 4-byte aligned");
  const long long slots = (rows + 127) / 128 + E, n8 = ((N + 127) / 128 + 7) / 8;
  TORCH_CHECK(slots * n8 * 8 < (1LL << 31), who, ": the grid of ", slots, " m-tile slots x ", n8 * 8,
              " n-tiles is past 2^31 - 1 workgroups");
  // (a single row's stride is arbitrary in torch: hand the kernel one that passes its own checks)
  const int64_t lda = a_nrows <= 1 ? K : a.ld, ldc = rows <= 1 ? NC : c.ld;
  CHECK_RC(lwc_moe_gemm_mxfp4_a8(a.p, as, qp, sp, c.p, ro, ar, (int)E, (int)rows, (long long)a_nrows, (int)N, (int)K,
                                 (int)lda, (int)ldc, (int)epi, cur_stream()),
           who);
}

// batched LoRA (lora.hip): T[m] = X[m] . A[ids[m]]^T, then Y[m] += T[m] . B[ids[m]]^T; ids outside
// [0, n_adapters) (-1) mean no adapter: the row of T is not written, the row of Y not touched
const int* lora_check_ids(const at::Tensor& ids, int64_t M, const char* who) {
  TORCH_CHECK(ids.dim() == 1, who, ": ids must be int32 [M]");
  return flat<int>(ids, I32, who, "ids", exactly(M));
}

void lora_shrink(const at::Tensor& X, const at::Tensor& A, const at::Tensor& ids, at::Tensor& T) {
  const char* who = "lora_shrink";
  const Strided x = strided(X, BF16, who, "X");  // rows may be strided
  const void* ap = flat(A, BF16, who, "A");
  void* tp = flat(T, BF16, who, "T");
  TORCH_CHECK(A.dim() == 3 && T.dim() == 2, who, ": X [M, K], A [n, R, K], T [M, R]");
  const int64_t M = X.size(0), K = X.size(1), R = A.size(1), n = A.size(0);
  TORCH_CHECK(A.size(2) == K && T.size(0) == M && T.size(1) == R, who, ": shape mismatch");
  TORCH_CHECK(M >= 1 && K % 64 == 0 && R % 16 == 0 && R >= 16 && R <= 192 && n >= 1 && n <= 64, who,
              ": needs M >= 1, K % 64 == 0, R a multiple of 16 up to 192, at most 64 adapters");
  CHECK_RC(lwc_lora_shrink(x.p, ap, lora_check_ids(ids, M, who), tp, (int)M, (int)K, (int)R, x.ld, (int)n,
                           cur_stream()),
           who);
}

void lora_expand_add(at::Tensor& Y, const at::Tensor& T, const at::Tensor& B, const at::Tensor& ids) {
  const char* who = "lora_expand_add";
  const Strided y = strided(Y, BF16, who, "Y");  // rows may be strided
  const void* tp = flat(T, BF16, who, "T");
  const void* bp = flat(B, BF16, who, "B");
  TORCH_CHECK(B.dim() == 3 && T.dim() == 2, who, ": Y [M, N], T [M, R], B [n, N, R]");
  const int64_t M = Y.size(0), N = Y.size(1), R = B.size(2), n = B.size(0);
  TORCH_CHECK(B.size(1) == N && T.size(0) == M && T.size(1) == R, who, ": shape mismatch");
  TORCH_CHECK(M >= 1 && N % 8 == 0 && R % 16 == 0 && R >= 16 && R <= 192 && n >= 1 && n <= 64, who,
              ": needs M >= 1, N % 8 == 0, R a multiple of 16 up to 192, at most 64 adapters");
  CHECK_RC(lwc_lora_expand_add(y.p, tp, bp, lora_check_ids(ids, M, who), (int)M, (int)N, (int)R, y.ld, (int)n,
                               cur_stream()),
           who);
}

// MX scale planes [K / 128][rows][4] bytes; a row-range view of a larger tensor is accepted (the plane stride,
// returned as ld in rows, is then the full tensor's row count)
Strided plane_rows(const at::Tensor& t, const char* who, const char* name) {
  check_device_dtype(t, U8, who, name);
  TORCH_CHECK(t.dim() == 3 && t.size(2) == 4 && t.stride(2) == 1 && t.stride(1) == 4 && t.stride(0) % 4 == 0 &&
                  t.stride(0) / 4 >= t.size(1) && t.stride(0) / 4 <= INT_MAX,
              who, ": ", name, ": MX scales must be [K / 128, rows, 4] bytes with rows contiguous");
  return {t.data_ptr(), (int)(t.stride(0) / 4)};
}

void gemm8g_fp8(const at::Tensor& A, const at::Tensor& W, at::Tensor& C, const OptTensor& row_off, int64_t max_slots,
                const OptTensor& a_rows, const OptTensor& a_scale, const at::Tensor& w_scale, int64_t mode,
                const OptTensor& a_mx, const OptTensor& mx_out) {
  // grouped fp8 GEMM on the 8-phase schedule (gemm8g.hip): A [rows_a, K] e4m3, W [G, N, K] e4m3, C [rows, N] bf16;
  // row_off None: the dense projection (G = 1, every output row).  mode 1: SwiGLU epilogue, C [rows, N / 2] bf16;
  // mode 2: SwiGLU epilogue with MX output, C [rows, N / 2] e4m3 + mx_out [N / 256, rows, 4] e8m0 (uint8);
  // a_mx [K / 128, rows_a, 4] e8m0: A's MX block scales (mode 0, no a_rows; a_scale unused)
  const char* who = "gemm8g";
  TORCH_CHECK(mode >= 0 && mode <= 2, who, ": mode 0, 1 or 2");
  const Strided a = strided(A, FP8, who, "A"), c = strided(C, mode == 2 ? FP8 : BF16, who, "C");
  const void* wp = flat(W, FP8, who, "W");
  TORCH_CHECK(W.dim() == 3, who, ": W must be [G, N, K]");
  const int G = (int)W.size(0), N = (int)W.size(1), K = (int)W.size(2);
  const int* ro = opt_flat<int>(row_off, I32, who, "row_off", exactly(G + 1));
  if (!present(row_off)) {
    TORCH_CHECK(G == 1, who, ": dense mode (no row_off) takes one weight");
    TORCH_CHECK(max_slots >= (C.size(0) + 255) / 256, who, ": dense mode needs ceil(rows / 256) slots");
  }
  TORCH_CHECK(A.size(1) == K && C.size(1) == (mode ? N / 2 : N), who, ": shape mismatch");
  TORCH_CHECK(A.size(0) * A.stride(0) < (int64_t(1) << 31), who, ": A spans >= 2 GiB (32-bit buffer range)");
  TORCH_CHECK(!mode || N % 64 == 0, who, ": SwiGLU needs whole 64-row gate / up block pairs");
  const float* ws = flat<float>(w_scale, F32, who, "w_scale", exactly((int64_t)G * N));
  const bool mxa = present(a_mx);
  TORCH_CHECK(mxa || present(a_scale), who, ": a_scale or a_mx required");
  const float* as = mxa ? nullptr : flat<float>(*a_scale, F32, who, "a_scale", at_least(A.size(0)));
  const int* ar = opt_flat<int>(a_rows, I32, who, "a_rows", at_least(C.size(0)));
  TORCH_CHECK(present(a_rows) || C.size(0) <= A.size(0), who, ": more output rows than A rows");
  Strided amx, mxo;  // the two never go together: one s_rows serves both
  if (mxa) {
    TORCH_CHECK(mode == 0 && !present(a_rows), who, ": MX A takes the plain epilogue and contiguous rows");
    amx = plane_rows(*a_mx, who, "a_mx");
    TORCH_CHECK(a_mx->size(0) == K / 128 && a_mx->size(1) >= A.size(0), who, ": a_mx must be [K / 128, rows_a, 4]");
  }
  if (mode == 2) {
    TORCH_CHECK(present(mx_out), who, ": mode 2 writes mx_out");
    mxo = plane_rows(*mx_out, who, "mx_out");
    TORCH_CHECK(N % 256 == 0 && mx_out->size(0) == N / 256 && mx_out->size(1) >= C.size(0) && c.ld % 16 == 0, who,
                ": mx_out must be [N / 256, rows, 4] (N % 256 == 0)");
  }
  CHECK_RC(lwc_gemm8g_fp8(a.p, wp, c.p, ro, ar, as, ws, G, (int)max_slots, N, K, a.ld, c.ld, (int)A.size(0),
                          (int)C.size(0), (int)mode, amx.p, mxo.p, mode == 2 ? mxo.ld : amx.ld, cur_stream()),
           who);
}

// ---- MoE routing and the fp8 row quantisers

// The router's outputs: topk_ids / topk_w / src_row / inv [>= T * k], row_off [E + 1]
struct RouteOutputs {
  int* topk_ids;
  float* topk_w;
  int *row_off, *src_row, *inv;
};
RouteOutputs route_outputs(at::Tensor& topk_ids, at::Tensor& topk_w, at::Tensor& row_off, at::Tensor& src_row,
                           at::Tensor& inv, int64_t T, int64_t k, int64_t E, const char* who) {
  const Numel n = at_least(T * k);
  return {flat<int>(topk_ids, I32, who, "topk_ids", n), flat<float>(topk_w, F32, who, "topk_w", n),
          flat<int>(row_off, I32, who, "row_off", exactly(E + 1)), flat<int>(src_row, I32, who, "src_row", n),
          flat<int>(inv, I32, who, "inv", n)};
}

void moe_route(const at::Tensor& logits, int64_t k, at::Tensor& topk_ids, at::Tensor& topk_w, at::Tensor& row_off,
               at::Tensor& src_row, at::Tensor& inv) {
  const char* who = "moe_route";
  const void* lp = flat(logits, BF16, who, "logits");
  TORCH_CHECK(logits.dim() == 2, who, ": logits must be [T, E]");
  const int T = (int)logits.size(0), E = (int)logits.size(1);
  const RouteOutputs o = route_outputs(topk_ids, topk_w, row_off, src_row, inv, T, k, E, who);
  CHECK_RC(lwc_moe_route(lp, T, E, (int)k, o.topk_ids, o.topk_w, o.row_off, o.src_row, o.inv, cur_stream()), who);
}

void moe_router(const at::Tensor& h, const at::Tensor& router, int64_t k, at::Tensor& topk_ids, at::Tensor& topk_w,
                at::Tensor& row_off, at::Tensor& src_row, at::Tensor& inv, const OptTensor& logits) {
  const char* who = "moe_router";
  const Strided hs = strided(h, BF16, who, "h");
  const void* rp = flat(router, BF16, who, "router");
  TORCH_CHECK(router.dim() == 2 && h.size(1) == router.size(1), who, ": h [T, d], router [E, d]");
  const int T = (int)h.size(0), E = (int)router.size(0), d = (int)h.size(1);
  const RouteOutputs o = route_outputs(topk_ids, topk_w, row_off, src_row, inv, T, k, E, who);
  CHECK_RC(lwc_moe_router(hs.p, hs.ld, rp, T, E, d, (int)k, o.topk_ids, o.topk_w, o.row_off, o.src_row, o.inv,
                          opt_flat(logits, BF16, who, "logits", exactly((int64_t)T * E)), cur_stream()),
           who);
}

// moe_wide.hip: 16 < E <= 128, k <= 8 (the launchers refuse the rest); h rows and router rows are read 16 B at a time
void moe_route_wide(const at::Tensor& logits, int64_t k, at::Tensor& topk_ids, at::Tensor& topk_w,
                    at::Tensor& row_off, at::Tensor& src_row, at::Tensor& inv) {
  const char* who = "moe_route_wide";
  const void* lp = flat(logits, BF16, who, "logits");
  TORCH_CHECK(logits.dim() == 2 && k >= 1, who, ": logits must be [T, E], k >= 1");
  const int T = (int)logits.size(0), E = (int)logits.size(1);
  const RouteOutputs o = route_outputs(topk_ids, topk_w, row_off, src_row, inv, T, k, E, who);
  CHECK_RC(lwc_moe_route_wide(lp, T, E, (int)k, o.topk_ids, o.topk_w, o.row_off, o.src_row, o.inv, cur_stream()),
           who);
}

void moe_router_wide(const at::Tensor& h, const at::Tensor& router, int64_t k, at::Tensor& topk_ids,
                     at::Tensor& topk_w, at::Tensor& row_off, at::Tensor& src_row, at::Tensor& inv,
                     const OptTensor& logits) {
  const char* who = "moe_router_wide";
  const Strided hs = strided(h, BF16, who, "h", 8);
  const void* rp = flat(router, BF16, who, "router");
  TORCH_CHECK(router.dim() == 2 && h.size(1) == router.size(1) && k >= 1, who, ": h [T, d], router [E, d], k >= 1");
  TORCH_CHECK(h.size(0) <= 1 || hs.ld >= h.size(1), who, ": h rows overlap (row stride ", hs.ld, " < d)");
  const int T = (int)h.size(0), E = (int)router.size(0), d = (int)h.size(1);
  const RouteOutputs o = route_outputs(topk_ids, topk_w, row_off, src_row, inv, T, k, E, who);
  CHECK_RC(lwc_moe_router_wide(hs.p, hs.ld, rp, T, E, d, (int)k, o.topk_ids, o.topk_w, o.row_off, o.src_row, o.inv,
                               opt_flat(logits, BF16, who, "logits", exactly((int64_t)T * E)), cur_stream()),
           who);
}

void moe_combine(const at::Tensor& Y, const at::Tensor& inv, const at::Tensor& w, int64_t k, at::Tensor& out) {
  const char* who = "moe_combine";
  const void* yp = flat(Y, BF16, who, "Y");
  void* op = flat(out, BF16, who, "out");
  TORCH_CHECK(Y.dim() == 2 && out.dim() == 2 && k >= 1, who, ": Y [rows, d], out [T, d], k >= 1");
  const int T = (int)out.size(0), d = (int)out.size(1);
  TORCH_CHECK(Y.size(1) == d, who, ": shapes");
  // the kernel indexes inv and w as flat [T * k]
  CHECK_RC(lwc_moe_combine(yp, flat<int>(inv, I32, who, "inv", at_least((int64_t)T * k)),
                           flat<float>(w, F32, who, "w", at_least((int64_t)T * k)), T, (int)k, d, op, cur_stream()),
           who);
}

void quant_fp8_rows(const at::Tensor& x, at::Tensor& q, at::Tensor& scale) {
  const char* who = "quant_fp8_rows";
  const void* xp = flat(x, BF16, who, "x");
  const int d = (int)x.size(-1), rows = (int)(x.numel() / d);
  CHECK_RC(lwc_quant_fp8_rows(xp, rows, d, flat(q, FP8, who, "q", exactly(x.numel())),
                              flat<float>(scale, F32, who, "scale", at_least(rows)), cur_stream()),
           who);
}

void silu_mul_quant_fp8(const at::Tensor& gu, at::Tensor& q, at::Tensor& scale, int64_t block) {
  // gu [rows, 2F] bf16 (gate | up, or interleaved in blocks) -> q [rows, F] e4m3fn, scale [rows] f32
  const char* who = "silu_mul_quant_fp8";
  const void* gp = flat(gu, BF16, who, "gu");
  void* qp = flat(q, FP8, who, "q");
  TORCH_CHECK(gu.dim() == 2 && q.dim() == 2, who, ": 2-D");
  const int rows = (int)gu.size(0), F = (int)q.size(1);
  TORCH_CHECK(gu.size(1) == 2 * F && q.size(0) == rows, who, ": shape mismatch");
  TORCH_CHECK(block == 0 || (block % 8 == 0 && F % block == 0), who, ": bad block");
  CHECK_RC(lwc_silu_mul_quant_fp8(gp, rows, F, (int)block, qp, flat<float>(scale, F32, who, "scale", at_least(rows)),
                                  cur_stream()),
           who);
}

// ---- C4 expert-parallel exchange buffers (csrc/kernels/ep.hip): send / recv are uint8 [W, (C + 1) * RB]; the
// token rows (x, x_local, y_local, back) are copied as bytes, so they are flat tensors of any one dtype.
int64_t row_bytes_of(const at::Tensor& x) { return x.size(1) * (int64_t)x.element_size(); }

void ep_pack(const at::Tensor& x, const OptTensor& xs, const OptTensor& src, const at::Tensor& row_off, int64_t W,
             int64_t El, int64_t C, at::Tensor& send) {
  const char* who = "ep_pack";
  const void* xp = flat(x, x.scalar_type(), who, "x");
  void* sp = flat(send, U8, who, "send");
  TORCH_CHECK(x.dim() == 2, who, ": x [rows, d], row_off [W*El+1]");
  TORCH_CHECK(send.dim() == 2 && send.size(0) == W && send.size(1) % (C + 1) == 0, who, ": send [W, (C+1)*RB]");
  CHECK_RC(lwc_ep_pack(xp, opt_flat<float>(xs, F32, who, "xs", exactly(x.size(0))),
                       opt_flat<int>(src, I32, who, "src"), flat<int>(row_off, I32, who, "row_off", exactly(W * El + 1)),
                       (int)W, (int)El, (int)C, (int)(send.size(1) / (C + 1)), (int)row_bytes_of(x), sp, cur_stream()),
           who);
}

void ep_unpack(const at::Tensor& recv, int64_t W, int64_t El, int64_t C, at::Tensor& x_local, const OptTensor& s_local,
               at::Tensor& map, at::Tensor& row_off_local) {
  const char* who = "ep_unpack";
  const void* rp = flat(recv, U8, who, "recv");
  void* xp = flat(x_local, x_local.scalar_type(), who, "x_local");
  TORCH_CHECK(recv.dim() == 2 && recv.size(0) == W && recv.size(1) % (C + 1) == 0, who, ": recv [W, (C+1)*RB]");
  TORCH_CHECK(x_local.dim() == 2 && x_local.size(0) == W * C, who, ": x_local [W*C, d]");
  CHECK_RC(lwc_ep_unpack(rp, (int)W, (int)El, (int)C, (int)(recv.size(1) / (C + 1)), (int)row_bytes_of(x_local),
                         present(s_local) ? 1 : 0, xp, opt_flat<float>(s_local, F32, who, "s_local", exactly(W * C)),
                         flat<int>(map, I32, who, "map", exactly(W * C)),
                         flat<int>(row_off_local, I32, who, "row_off_local", exactly(El + 1)), cur_stream()),
           who);
}

void ep_back(const at::Tensor& y_local, const at::Tensor& map, int64_t W, int64_t C, at::Tensor& back) {
  const char* who = "ep_back";
  const void* yp = flat(y_local, y_local.scalar_type(), who, "y_local");
  void* bp = flat(back, y_local.scalar_type(), who, "back");
  TORCH_CHECK(y_local.dim() == 2 && y_local.size(0) >= W * C && back.dim() == 2 && back.size(0) == W * C &&
                  back.size(1) == y_local.size(1),
              who, ": y_local [>= W*C, d], back [W*C, d], map [W*C]");
  CHECK_RC(lwc_ep_back(yp, flat<int>(map, I32, who, "map", exactly(W * C)), (int)W, (int)C, (int)row_bytes_of(y_local),
                       bp, cur_stream()),
           who);
}

void ep_combine(const at::Tensor& ret, const at::Tensor& row_off, const at::Tensor& inv, const at::Tensor& w,
                int64_t El, int64_t C, int64_t k, at::Tensor& out) {
  const char* who = "ep_combine";
  const void* rp = flat(ret, BF16, who, "ret");
  void* op = flat(out, BF16, who, "out");
  const int* ro = flat<int>(row_off, I32, who, "row_off", at_least(1));
  TORCH_CHECK(ret.dim() == 2 && out.dim() == 2, who, ": ret [W*C, d], out [T, d]");
  const int T = (int)out.size(0), d = (int)out.size(1);
  const int64_t E = row_off.numel() - 1;
  TORCH_CHECK(ret.size(1) == d && ret.size(0) == (E / El) * C, who, ": ret [W*C, d], inv / w [T*k]");
  CHECK_RC(lwc_ep_combine(rp, ro, flat<int>(inv, I32, who, "inv", at_least((int64_t)T * k)),
                          flat<float>(w, F32, who, "w", at_least((int64_t)T * k)), T, (int)E, (int)El, (int)C, (int)k,
                          d, op, cur_stream()),
           who);
}

// ---- prefill attention

void prefill_attention(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, at::Tensor& out,
                       const at::Tensor& cu_seqlens, int64_t max_seqlen, int64_t Hq, int64_t Hkv, int64_t D,
                       double scale, bool causal, const OptTensor& cu_seqlens_k) {
  // q/k/v: [T, *] 2-D views with unit inner stride (slices of the fused qkv row); out: [T, Hq*D].
  // cu_seqlens_k (optional): per-sequence key ranges in k/v, each at least as long as the sequence's query
  // range (the caller checks the lengths on the host; queries are the last rows of the key range).
  const char* who = "prefill_attention";
  const Strided qs = strided(q, BF16, who, "q"), ks = strided(k, BF16, who, "k"), vs = strided(v, BF16, who, "v");
  const Strided os = strided(out, BF16, who, "out");
  const int* cu = flat<int>(cu_seqlens, I32, who, "cu_seqlens", at_least(1));
  const int* cuk = opt_flat<int>(cu_seqlens_k, I32, who, "cu_seqlens_k", exactly(cu_seqlens.numel()));
  TORCH_CHECK(k.size(0) == v.size(0), who, ": k/v row mismatch");
  TORCH_CHECK(q.size(1) == Hq * D && k.size(1) == Hkv * D && v.size(1) == Hkv * D && out.size(1) == Hq * D, who,
              ": head shape mismatch");
  const int nseq = (int)cu_seqlens.numel() - 1;
  CHECK_RC(lwc_prefill_attention(qs.p, ks.p, vs.p, os.p, cu, cuk, nseq, (int)max_seqlen, qs.ld, ks.ld, vs.ld, os.ld,
                                 (int)Hq, (int)Hkv, (int)D, (float)scale, causal ? 1 : 0, cur_stream()),
           who);
}

void prefill_attention_mx(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, at::Tensor& out8, at::Tensor& mx,
                          const at::Tensor& cu_seqlens, int64_t max_seqlen, int64_t Hq, int64_t Hkv, double scale,
                          bool causal) {
  // D = 128; out8 [T, Hq*128] e4m3 (uint8 view, 16-B aligned row stride), mx [Hq, >= T, 4] uint8 contiguous
  const char* who = "prefill_attention_mx";
  const Strided qs = strided(q, BF16, who, "q"), ks = strided(k, BF16, who, "k"), vs = strided(v, BF16, who, "v");
  TORCH_CHECK(out8.element_size() == 1 && mx.element_size() == 1, who, ": byte outputs");
  const Strided os = strided(out8, out8.scalar_type(), who, "out8", 16);
  void* mxp = flat(mx, mx.scalar_type(), who, "mx");
  const int* cu = flat<int>(cu_seqlens, I32, who, "cu_seqlens", at_least(1));
  TORCH_CHECK(q.size(1) == Hq * 128 && k.size(1) == Hkv * 128 && v.size(1) == Hkv * 128 && out8.size(1) == Hq * 128 &&
                  out8.size(0) == q.size(0) && k.size(0) == v.size(0),
              who, ": head shape mismatch (head_dim 128)");
  TORCH_CHECK(mx.dim() == 3 && mx.size(0) == Hq && mx.size(1) >= q.size(0) && mx.size(2) == 4, who,
              ": mx [Hq, >= T, 4]");
  const int nseq = (int)cu_seqlens.numel() - 1;
  CHECK_RC(lwc_prefill_attention_mx(qs.p, ks.p, vs.p, os.p, mxp, (int)mx.size(1), cu, nseq, (int)max_seqlen, qs.ld,
                                    ks.ld, vs.ld, os.ld, (int)Hq, (int)Hkv, (float)scale, causal ? 1 : 0,
                                    cur_stream()),
           who);
}

void prefill_attention_paged(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache, at::Tensor& out,
                             const at::Tensor& cu_seqlens, const at::Tensor& block_tables, const at::Tensor& k_lens,
                             int64_t max_seqlen, int64_t Hq, double scale) {
  // q [T, >=Hq*D] (row stride allowed), out [T, Hq*D]; K [NB, Hkv, 16, 128], V [NB, Hkv, 4, 128, 4];
  // block_tables [nseq, W] int32 (W even and >= 2 * ceil(max k_len / 32): a 32-key tile reads 2 entries),
  // k_lens [nseq] int32 (>= each sequence's query count: the queries are the last positions).
  const char* who = "prefill_attention_paged";
  const Strided qs = strided(q, BF16, who, "q"), os = strided(out, BF16, who, "out");
  const void* kp = flat(k_cache, BF16, who, "k_cache");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == 16 && k_cache.size(3) == 128, who,
              ": K cache [NB, Hkv, 16, 128]");
  const void* vp = check_v_cache(v_cache, k_cache, who);
  const int Hkv = (int)k_cache.size(1), D = 128;
  const int* cu = flat<int>(cu_seqlens, I32, who, "cu_seqlens", at_least(1));
  const int nseq = (int)cu_seqlens.numel() - 1;
  const int* bt = flat<int>(block_tables, I32, who, "block_tables");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == nseq && block_tables.size(1) % 2 == 0, who,
              ": block_tables [nseq, even W] and k_lens [nseq]");
  TORCH_CHECK(q.size(1) >= Hq * D && out.size(1) == Hq * D && Hq % Hkv == 0, who, ": q / out shapes");
  CHECK_RC(lwc_prefill_attention_paged(qs.p, kp, vp, os.p, cu, bt, flat<int>(k_lens, I32, who, "k_lens", exactly(nseq)),
                                       (int)block_tables.size(1), nseq, (int)max_seqlen, qs.ld, os.ld, (int)Hq, Hkv, D,
                                       (float)scale, cur_stream()),
           who);
}

// ---- sampling and scoring

void sample(const at::Tensor& logits, const at::Tensor& temperature, const at::Tensor& top_p, const at::Tensor& top_k,
            const at::Tensor& min_p, const at::Tensor& top_a, const OptTensor& freq_pen, const OptTensor& pres_pen,
            const OptTensor& rep_pen, const OptTensor& counts, const OptTensor& count_rows, const OptTensor& bias,
            const OptTensor& bias_rows, const OptTensor& mask, const OptTensor& mask_rows, const at::Tensor& seeds,
            const at::Tensor& offsets, int64_t num_logprobs, at::Tensor& out_token, at::Tensor& out_logprob,
            at::Tensor& out_topk_ids, at::Tensor& out_topk_lp, bool mask_logprobs, bool need_logprob) {
  // logits [B, V] bf16 rows; one entry per row in every parameter table; counts int16 [*, V], bias f32 [*, V] and
  // mask int32 [*, V / 32] (bit words) are tables whose rows the *_rows operands pick per logits row
  const char* who = "sample";
  const Strided lg = strided(logits, BF16, who, "logits");
  const int B = (int)logits.size(0), V = (int)logits.size(1);
  const Numel per_row = at_least(B), topk = at_least(B * num_logprobs);
  if (present(counts)) TORCH_CHECK(counts->size(-1) == V, who, ": counts must be int16 [*, V]");
  if (present(bias)) TORCH_CHECK(bias->size(-1) == V, who, ": bias rows must be [*, V]");
  if (present(mask)) TORCH_CHECK(mask->size(-1) == V / 32, who, ": mask rows must be [*, V/32]");
  CHECK_RC(lwc_sample(lg.p, lg.ld, V, B, flat<float>(temperature, F32, who, "temperature", per_row),
                      flat<float>(top_p, F32, who, "top_p", per_row), flat<int>(top_k, I32, who, "top_k", per_row),
                      flat<float>(min_p, F32, who, "min_p", per_row), flat<float>(top_a, F32, who, "top_a", per_row),
                      opt_flat<float>(freq_pen, F32, who, "freq_pen", per_row),
                      opt_flat<float>(pres_pen, F32, who, "pres_pen", per_row),
                      opt_flat<float>(rep_pen, F32, who, "rep_pen", per_row), opt_flat(counts, at::kShort, who, "counts"),
                      opt_flat<int>(count_rows, I32, who, "count_rows", per_row), opt_flat<float>(bias, F32, who, "bias"),
                      opt_flat<int>(bias_rows, I32, who, "bias_rows", per_row),
                      opt_flat<unsigned int>(mask, I32, who, "mask"),
                      opt_flat<int>(mask_rows, I32, who, "mask_rows", per_row),
                      flat<unsigned long long>(seeds, at::kLong, who, "seeds", per_row),
                      flat<unsigned long long>(offsets, at::kLong, who, "offsets", per_row), (int)num_logprobs,
                      mask_logprobs ? 1 : 0, need_logprob ? 1 : 0, flat<int>(out_token, I32, who, "out_token", per_row),
                      flat<float>(out_logprob, F32, who, "out_logprob", per_row),
                      num_logprobs > 0 ? flat<int>(out_topk_ids, I32, who, "out_topk_ids", topk) : nullptr,
                      num_logprobs > 0 ? flat<float>(out_topk_lp, F32, who, "out_topk_lp", topk) : nullptr,
                      cur_stream()),
           who);
}

void pool_l2norm(const at::Tensor& hidden, const at::Tensor& cu_seqlens, int64_t mode, at::Tensor& out_f32,
                 const OptTensor& out_bf16) {
  const char* who = "pool_l2norm";
  const Strided h = strided(hidden, BF16, who, "hidden");
  // the kernel reads cu[s] and writes out[s * d + c] through flat pointers
  const int* cu = flat<int>(cu_seqlens, I32, who, "cu_seqlens", at_least(1));
  const int nseq = (int)cu_seqlens.numel() - 1, d = (int)hidden.size(1);
  CHECK_RC(lwc_pool_l2norm(h.p, h.ld, cu, nseq, d, (int)mode,
                           flat<float>(out_f32, F32, who, "out_f32", exactly((int64_t)nseq * d)),
                           opt_flat(out_bf16, BF16, who, "out_bf16", exactly((int64_t)nseq * d)), cur_stream()),
           who);
}

std::vector<at::Tensor> knn_topk(const at::Tensor& E, const at::Tensor& q, int64_t k) {
  // E [n, d] f32 (contiguous rows), q [d] f32 -> (values [k] f32, rows [k] int32), best first, ties to the lower row
  const char* who = "knn_topk";
  const float* ep = flat<float>(E, F32, who, "E");
  TORCH_CHECK(E.dim() == 2 && E.size(1) % 4 == 0, who, ": E [n, d] (d % 4 == 0), q [d]");
  const int n = (int)E.size(0), d = (int)E.size(1);
  const float* qp = flat<float>(q, F32, who, "q", exactly(d));
  TORCH_CHECK(k >= 1 && k <= 64 && k <= n, who, ": 1 <= k <= min(64, n)");
  const int slabs = (n + 255) / 256;
  auto opts = E.options();
  at::Tensor pv = at::empty({2 * (int64_t)slabs * k}, opts), vals = at::empty({k}, opts);
  at::Tensor pi = at::empty({2 * (int64_t)slabs * k}, opts.dtype(at::kInt)), rows = at::empty({k}, opts.dtype(at::kInt));
  CHECK_RC(lwc_knn_topk(ep, n, d, qp, (int)k, pv.data_ptr<float>(), pi.data_ptr<int>(), vals.data_ptr<float>(),
                        rows.data_ptr<int>(), cur_stream()),
           who);
  return {vals, rows};
}

std::vector<at::Tensor> vote_tally(const at::Tensor& V, const at::Tensor& w, const at::Tensor& valid) {
  // V [R, L, C] f64, w [R, L] f64, valid [R, L] u8 -> (choice weight [R, C], confidence [R, C],
  // voter confidence [R, L]; NaN where !valid)
  const char* who = "vote_tally";
  const double* vp = flat<double>(V, at::kDouble, who, "V");
  const double* wp = flat<double>(w, at::kDouble, who, "w");
  const unsigned char* mp = flat<unsigned char>(valid, U8, who, "valid");
  TORCH_CHECK(V.dim() == 3 && w.dim() == 2 && valid.dim() == 2, who, ": V [R, L, C], w / valid [R, L]");
  const int R = (int)V.size(0), L = (int)V.size(1), C = (int)V.size(2);
  TORCH_CHECK(w.size(0) == R && w.size(1) == L && valid.size(0) == R && valid.size(1) == L, who,
              ": w / valid must be [R, L]");
  TORCH_CHECK(C >= 1 && C <= 1024, who, ": 1 <= choices <= 1024");
  at::Tensor cw = at::empty({R, C}, V.options()), conf = at::empty({R, C}, V.options());
  at::Tensor vconf = at::empty({R, L}, V.options());
  CHECK_RC(lwc_vote_tally(vp, wp, mp, R, L, C, cw.data_ptr<double>(), conf.data_ptr<double>(),
                          vconf.data_ptr<double>(), cur_stream()),
           who);
  return {cw, conf, vconf};
}

void cosine_consensus(const at::Tensor& E, at::Tensor& S, double inv_tau, at::Tensor& centrality, at::Tensor& weights,
                      at::Tensor& best) {
  // E: [R, n, d] bf16; S: [R, n_pad, n_pad] f32; the outputs are written through flat pointers
  const char* who = "cosine_consensus";
  const void* ep = flat(E, BF16, who, "E");
  TORCH_CHECK(E.dim() == 3, who, ": E must be [R, n, d]");
  const int R = (int)E.size(0), n = (int)E.size(1), d = (int)E.size(2);
  const int n_pad = (n + 15) / 16 * 16;
  CHECK_RC(lwc_cosine_consensus(ep, R, n, d, flat<float>(S, F32, who, "S", at_least((int64_t)R * n_pad * n_pad)),
                                (float)inv_tau, flat<float>(centrality, F32, who, "centrality", at_least((int64_t)R * n)),
                                flat<float>(weights, F32, who, "weights", at_least((int64_t)R * n)),
                                flat<int>(best, I32, who, "best", at_least(R)), cur_stream()),
           who);
}

}  // namespace

// ---- C3 custom all-reduce (allreduce.hip): IPC regions are raw device pointers held by Python as ints
std::tuple<int64_t, py::bytes> ar_alloc(int64_t bytes) {
  void* ptr = nullptr;
  std::string h((size_t)lwc_ar_handle_bytes(), '\0');
  const int rc = lwc_ar_alloc(bytes, &ptr, h.data());
  TORCH_CHECK(rc == 0, "ar_alloc: HIP error ", rc);
  return {reinterpret_cast<int64_t>(ptr), py::bytes(h)};
}

int64_t ar_open(const py::bytes& handle) {
  std::string h = handle;
  TORCH_CHECK((int)h.size() == lwc_ar_handle_bytes(), "ar_open: bad handle size");
  void* ptr = nullptr;
  const int rc = lwc_ar_open(h.data(), &ptr);
  TORCH_CHECK(rc == 0, "ar_open: hipIpcOpenMemHandle failed with ", rc);
  return reinterpret_cast<int64_t>(ptr);
}

void ar_close(int64_t ptr) { (void)lwc_ar_close(reinterpret_cast<void*>(ptr)); }
void ar_free(int64_t ptr) { (void)lwc_ar_free(reinterpret_cast<void*>(ptr)); }
int64_t ar_region_bytes(int64_t W, int64_t cap) { return lwc_ar_region_bytes((int)W, cap); }

void allreduce(const std::vector<int64_t>& bases, int64_t me, const at::Tensor& x, at::Tensor& out, int64_t cap,
               at::Tensor& err, int64_t blocks, int64_t spin_limit) {
  const char* who = "allreduce";
  const void* xp = flat(x, BF16, who, "x");
  TORCH_CHECK(x.numel() % 8 == 0, who, ": numel must be a multiple of 8");
  std::vector<void*> b;
  for (int64_t v : bases) b.push_back(reinterpret_cast<void*>(v));
  CHECK_RC(lwc_allreduce(b.data(), (int)me, (int)b.size(), xp, flat(out, BF16, who, "out", exactly(x.numel())),
                         x.numel(), cap, flat<int>(err, I32, who, "err", at_least(1)), (int)blocks,
                         (long long)spin_limit, cur_stream()),
           who);
}

void alltoall(const std::vector<int64_t>& bases, int64_t me, const at::Tensor& send, at::Tensor& recv, int64_t cap,
              at::Tensor& err, int64_t blocks, int64_t spin_limit) {
  // equal-split all-to-all of raw bytes: send / recv [W, chunk] uint8 (chunk % 16 == 0)
  const char* who = "alltoall";
  const void* sp = flat(send, U8, who, "send");
  void* rp = flat(recv, U8, who, "recv");
  const int64_t W = (int64_t)bases.size();
  TORCH_CHECK(send.dim() == 2 && send.size(0) == W && recv.sizes() == send.sizes(), who, ": send / recv [W, chunk]");
  TORCH_CHECK(send.size(1) % 16 == 0 && send.size(1) <= cap, who, ": chunk % 16 == 0 and chunk <= cap");
  std::vector<void*> b;
  for (int64_t v : bases) b.push_back(reinterpret_cast<void*>(v));
  CHECK_RC(lwc_alltoall(b.data(), (int)me, (int)W, sp, rp, send.size(1), cap,
                        flat<int>(err, I32, who, "err", at_least(1)), (int)blocks, (long long)spin_limit, cur_stream()),
           who);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 HIP kernels of llm_weighted_consensus_amd";
  m.def("rmsnorm", &rmsnorm);
  m.def("rmsnorm_quant_fp8", &rmsnorm_quant_fp8);
  m.def("layernorm", &layernorm);
  m.def("rope_kv_write", &rope_kv_write);
  m.def("qknorm_rope_kv_write", &qknorm_rope_kv_write);
  m.def("silu_mul", &silu_mul);
  m.def("embedding", &embedding);
  m.def("kv_block_copy", &kv_block_copy);
  m.def("paged_decode", &paged_decode);
  m.def("grouped_gemm", &grouped_gemm);
  m.def("gemm8p", &gemm8p);
  m.def("gemm4w", &gemm4w);
  m.def("skinny_gemm", &skinny_gemm);
  m.def("mxfp4_dequant", &mxfp4_dequant);
  m.def("skinny_mxfp4", &skinny_mxfp4);
  m.def("gemm_mxfp4_a8", &gemm_mxfp4_a8);
  m.def("moe_skinny_mxfp4", &moe_skinny_mxfp4);
  m.def("moe_gemm_mxfp4_a8", &moe_gemm_mxfp4_a8);
  m.def("lora_shrink", &lora_shrink);
  m.def("lora_expand_add", &lora_expand_add);
  m.def("rms_rowsumsq", &rms_rowsumsq);
  m.def("gemm8p_slots", &lwc_gemm8p_slots);
  m.def("moe_route", &moe_route);
  m.def("moe_router", &moe_router);
  m.def("moe_route_wide", &moe_route_wide);
  m.def("moe_router_wide", &moe_router_wide);
  m.def("moe_combine", &moe_combine);
  m.def("quant_fp8_rows", &quant_fp8_rows);
  m.def("paged_decode_cascade", &paged_decode_cascade);
  m.def("cascade_rows_per_tile", &lwc_cascade_rows_per_tile, "sequences per cascade super-tile for a GQA ratio G");
  m.def("set_decode_wave_min_items", &lwc_set_decode_wave_min_items,
        "B*Hkv*splits threshold of the wave-per-item decode kernel; returns the previous value");
  m.def("prefill_attention", &prefill_attention);
  m.def("prefill_attention_mx", &prefill_attention_mx);
  m.def("prefill_attention_paged", &prefill_attention_paged);
  m.def("silu_mul_quant_fp8", &silu_mul_quant_fp8);
  m.def("kv_gather", &kv_gather);
  m.def("sample", &sample);
  m.def("pool_l2norm", &pool_l2norm);
  m.def("cosine_consensus", &cosine_consensus);
  m.def("knn_topk", &knn_topk);
  m.def("vote_tally", &vote_tally);
  m.def("gemm8g_fp8", &gemm8g_fp8);
  m.def("ar_alloc", &ar_alloc);
  m.def("ar_open", &ar_open);
  m.def("ar_close", &ar_close);
  m.def("ar_free", &ar_free);
  m.def("ar_region_bytes", &ar_region_bytes);
  m.def("allreduce", &allreduce);
  m.def("alltoall", &alltoall);
  m.def("ep_pack", &ep_pack);
  m.def("ep_unpack", &ep_unpack);
  m.def("ep_back", &ep_back);
  m.def("ep_combine", &ep_combine);
}
