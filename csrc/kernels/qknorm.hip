// K2q  qknorm_rope_kv_write: the attention-block prologue of the Qwen decoders in one pass over a token's
// fused qkv row — q/k/v projection bias (Qwen2 / Qwen2.5), per-head RMSNorm of q and k (Qwen3), rotate-half
// RoPE and the paged KV-cache write.  Buffers and layouts are those of rope_kv_write (elementwise.hip);
// every value is computed in fp32 from the bf16 it was loaded as and rounded to bf16 once, at its store.
//
// Work split (D = 128 only): one thread per (head, 8 + 8 dims) unit exactly as in rope_kv_write, so the
// 8 consecutive lanes of an aligned group hold one head and the head's sum of squares is a three-step
// DPP reduction inside the group (no LDS, no barrier).  Units come in whole groups (the unit count and
// the first unit are multiples of 8, the block size a multiple of 64), so the lanes of a group are always
// active together.
#include "common.h"
#include "launchers.h"

namespace lwc {

constexpr int kQnD = 128;       // head_dim (what both decode attention kernels take)
constexpr int kQnHalf = kQnD / 2;
constexpr int kQnUnits = kQnHalf / 8;  // threads per head: 8 dims of each rotate-half side
constexpr int kQnVMax = 4096;   // V row elements staged in LDS (Hkv * D <= 4096: checked by the launcher)

// sum over the 8 lanes of an aligned group: quad xor 1, quad xor 2, then the half-row mirror (lane i <-> 7 - i
// of the 8: the other quad, whose four lanes already agree).  Every lane of the group gets the same bits.
LWC_DEVICE float group8_sum(float x) {
  x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, false));
  x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, false));
  return x + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xF, 0xF, false));
}

LWC_DEVICE void load8f(const float* p, float (&f)[8]) {
  *reinterpret_cast<float4*>(f) = reinterpret_cast<const float4*>(p)[0];
  *reinterpret_cast<float4*>(f + 4) = reinterpret_cast<const float4*>(p)[1];
}

// qkv: [T, (Hq + 2*Hkv) * 128]; bias: [(Hq + 2*Hkv) * 128] or null; qw / kw: [128] or null;
// cos/sin: [max_pos, 64] f32; K cache [NB, Hkv, BS, 128]; V cache [NB, Hkv, BS/4, 128, 4]
__global__ void __launch_bounds__(256) qknorm_rope_kv_write_kernel(
    bf16_t* __restrict__ qkv, const int* __restrict__ positions, const int* __restrict__ slots,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, bf16_t* __restrict__ kc,
    bf16_t* __restrict__ vc, const bf16_t* __restrict__ bias, const bf16_t* __restrict__ qw,
    const bf16_t* __restrict__ kw, int Hq, int Hkv, int BS, int rope_q, int first_unit, float eps) {
  const int t = blockIdx.x;
  const int n_units = (Hq + Hkv) * kQnUnits;
  const int row_len = (Hq + 2 * Hkv) * kQnD;
  bf16_t* row = qkv + (size_t)t * row_len;
  const int pos = positions[t];
  const int slot = slots ? slots[t] : -1;
  const int blk = slot >= 0 ? slot / BS : 0, off = slot >= 0 ? slot % BS : 0;
  const bool kv_back = rope_q || slot < 0;  // rope_kv_write's condition for writing k back
  // first_unit: 0, or Hq * 8 when the q heads have nothing to do (rope_q = 0, no bias, no q weight)
  for (int i = threadIdx.x + first_unit; i < n_units; i += blockDim.x) {
    const int h = i / kQnUnits;        // 0..Hq+Hkv-1 (q heads then k heads)
    const int c = (i % kQnUnits) * 8;  // first-half dim offset
    const bool is_k = h >= Hq;
    bf16_t* hp = row + h * kQnD;
    uint4v* p1 = reinterpret_cast<uint4v*>(hp + c);
    uint4v* p2 = reinterpret_cast<uint4v*>(hp + c + kQnHalf);
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(*p1, x1);
    unpack8(*p2, x2);
    if (bias) {
      float b1[8], b2[8];
      unpack8(*reinterpret_cast<const uint4v*>(bias + h * kQnD + c), b1);
      unpack8(*reinterpret_cast<const uint4v*>(bias + h * kQnD + c + kQnHalf), b2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x1[j] += b1[j];
        x2[j] += b2[j];
      }
    }
    const bf16_t* w = is_k ? kw : qw;  // (the same for the 8 lanes of a group: they share h)
    if (w) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
      const float r = rsqrtf(group8_sum(ss) * (1.f / kQnD) + eps);
      float w1[8], w2[8];
      unpack8(*reinterpret_cast<const uint4v*>(w + c), w1);
      unpack8(*reinterpret_cast<const uint4v*>(w + c + kQnHalf), w2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x1[j] = x1[j] * r * w1[j];
        x2[j] = x2[j] * r * w2[j];
      }
    }
    if (is_k || rope_q) {
      float cs[8], sn[8];
      load8f(cos_t + (size_t)pos * kQnHalf + c, cs);
      load8f(sin_t + (size_t)pos * kQnHalf + c, sn);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1[j] = x1[j] * cs[j] - x2[j] * sn[j];
        o2[j] = x2[j] * cs[j] + x1[j] * sn[j];
      }
    } else {  // pure decode steps: the attention kernels rotate q as they load it
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1[j] = x1[j];
        o2[j] = x2[j];
      }
    }
    const uint4v n1 = pack8(o1), n2 = pack8(o2);
    if (!is_k || kv_back) {
      *p1 = n1;
      *p2 = n2;
    }
    if (is_k && slot >= 0) {
      bf16_t* dst = kc + (((size_t)blk * Hkv + (h - Hq)) * BS + off) * kQnD;
      *reinterpret_cast<uint4v*>(dst + c) = n1;
      *reinterpret_cast<uint4v*>(dst + c + kQnHalf) = n2;
    }
  }
  // V: through LDS as in rope_kv_write (16 B loads, then 2 B stores with consecutive threads on consecutive
  // dims of the 4-token-interleaved cache rows); the bias is added on the way in, and the biased row also
  // goes back to qkv where k does (prefill attention reads v there)
  if (slot >= 0 || bias) {
    bf16_t* vrow_g = row + (Hq + Hkv) * kQnD;
    __shared__ uint4v vrow[kQnVMax / 8];
    const int nv = Hkv * kQnD;
    for (int i = threadIdx.x; i < (nv >> 3); i += blockDim.x) {
      uint4v v = reinterpret_cast<const uint4v*>(vrow_g)[i];
      if (bias) {
        float x[8], b[8];
        unpack8(v, x);
        unpack8(reinterpret_cast<const uint4v*>(bias + (Hq + Hkv) * kQnD)[i], b);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += b[j];
        v = pack8(x);
        if (kv_back) reinterpret_cast<uint4v*>(vrow_g)[i] = v;
      }
      vrow[i] = v;
    }
    if (slot >= 0) {  // (block-uniform: one token per block)
      __syncthreads();
      const bf16_t* vl = reinterpret_cast<const bf16_t*>(vrow);
      for (int i = threadIdx.x; i < nv; i += blockDim.x) {
        const int vh = i / kQnD, d = i - vh * kQnD;
        vc[((size_t)blk * Hkv + vh) * kQnD * BS + ((off >> 2) * kQnD + d) * 4 + (off & 3)] = vl[i];
      }
    }
  }
}

}  // namespace lwc

extern "C" int lwc_qknorm_rope_kv_write(void* qkv, const int* positions, const int* slots, const float* cos_t,
                                        const float* sin_t, void* kc, void* vc, const void* bias, const void* qw,
                                        const void* kw, int T, int Hq, int Hkv, int D, int BS, int rope_q, float eps,
                                        hipStream_t s) {
  using namespace lwc;
  if (D != kQnD || Hq <= 0 || Hkv <= 0 || Hkv * D > kQnVMax || BS % 4 != 0 || T < 0) return -1;
  if (T == 0) return 0;
  // the q units run when q is rotated, biased or normalised here: 256 threads (rope_kv_write's block for a full
  // row; (Hq + Hkv) * 8 = 320 units at Llama-3-8B / Qwen3-8B head counts take a second, partial round).
  // k only (no q work): Hkv * 8 units + the V scatter, 128 threads as rope_kv_write's k-only launch.
  const bool q_work = rope_q || bias || qw;
  qknorm_rope_kv_write_kernel<<<T, q_work ? 256 : 128, 0, s>>>(
      (bf16_t*)qkv, positions, slots, cos_t, sin_t, (bf16_t*)kc, (bf16_t*)vc, (const bf16_t*)bias, (const bf16_t*)qw,
      (const bf16_t*)kw, Hq, Hkv, BS, rope_q, q_work ? 0 : Hq * kQnUnits, eps);
  return (int)hipGetLastError();
}
