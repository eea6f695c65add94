// K11w Wide MoE routing (Qwen3-MoE: 128 experts, top-8): the router projection on the MFMA, a top-k that
// spreads a token's logits over 16 lanes, and the dispatch permutation with 128-entry tables.
//
//   moe_router_wide  : h [T, d] . router [E, d]^T on mfma_f32_16x16x32_bf16, fused with the top-k;
//   moe_route_wide   : the same top-k from precomputed logits [T, E] bf16;
//   moe_permute_wide : row_off / src_row / inv from topk_ids (moe_permute_kernel of moe.hip, 128-entry tables).
// Domain of all three: 16 < E <= 128 (any E), 1 <= k <= 8, k <= E.  Narrower E belongs to moe.hip.
//
// The contract is route_token's (moe.hip): repeated arg-max with ties to the lower expert id, best first;
// weights = fp32 softmax over the selected logits (maximum subtracted, __expf, one division).
//
// Projection (one workgroup of 4 waves per 16 tokens).  MFMA lane map (lane l: r16 = l & 15, g = l >> 4):
//   A operand: token row r16, K chunk g (8 bf16 = 16 B);   B operand: expert row r16 of the tile, K chunk g;
//   C register r: token 4 g + r, expert r16 of the tile.
// Wave w takes the 32-wide K steps w, w + 4, ... straight from global memory (the router is at most 1 MB and
// L2-resident) and keeps ceil(E / 16) accumulator tiles; the four partial tiles meet in LDS and are added in
// the fixed order ((w0 + w1) + w2) + w3, so a launch is bitwise reproducible.  Each logit is rounded to bf16
// (RNE), as moe_router does, and the selection runs on the rounded values.
// Reads: a token row >= T is clamped to row T - 1 (computed, never stored); an expert row >= E and a K chunk
// at or past d are not read (the operand is zero), so every lane's read stays inside its tensor.
//
// Top-k: the 16 lanes of a DPP row hold one token, lane g the experts g, g + 16, ..., g + 112 as 32-bit keys
//   key = (order-preserving 16-bit code of the bf16 logit) << 8 | (255 - expert)
// so one unsigned max is the arg-max with ties to the lower id; 0 marks "taken" and experts >= E (every real
// expert's key is >= 128, so with k <= E a zero key never wins).  -0 is read as +0, as the float compare of
// route_token does.  k rounds of (7 local max, 4 xor-shuffles); every lane then holds the k winners and
// computes the softmax in route_token's order; lane j stores entry j.
#include "common.h"
#include "launchers.h"

namespace lwc {

constexpr int kWideMaxExperts = 128;
constexpr int kWideMinExperts = 17;  // E <= 16: moe_router / moe_route of moe.hip
constexpr int kWideTopK = 8;
constexpr int kWideSlots = kWideMaxExperts / 16;  // logits per lane of a token's 16-lane group
constexpr int kWideTok = 16;                      // tokens per workgroup (one MFMA tile of rows)
constexpr int kWideWaves = 4;                     // waves of a router workgroup: each takes every 4th K step
constexpr int kWideLd = kWideMaxExperts + 4;      // LDS row stride of a partial tile row (floats)
static_assert(kWideWaves * 64 == kWideTok * 16, "the router workgroup's threads are the top-k's 16 lanes per token");

typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));

LWC_DEVICE float4v mfma_bf16_w(const uint4v& a, const uint4v& b, const float4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wbf16x8, a), __builtin_bit_cast(wbf16x8, b), c, 0,
                                                 0, 0);
}

// bf16 bits -> key of expert e, and back to the logit
LWC_DEVICE uint32_t wide_key(uint32_t bits, int e) {
  if (bits == 0x8000u) bits = 0;  // -0 == +0
  const uint32_t code = (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
  return (code << 8) | (uint32_t)(255 - e);
}
LWC_DEVICE float wide_key_value(uint32_t key) {
  const uint32_t code = key >> 8;
  const uint32_t bits = (code & 0x8000u) ? (code & 0x7fffu) : (~code & 0xffffu);
  return bf2f((bf16_t)bits);
}

// Top-k of one token held as keys[i] = key of expert g + 16 i by the 16 lanes g of a DPP row (0: no expert).
// All 16 lanes must be active.  Lane j < k stores (t, j) when ``store``.
LWC_DEVICE void route_token_wide(uint32_t (&keys)[kWideSlots], int g, int k, int t, bool store,
                                 int* __restrict__ topk_ids, float* __restrict__ topk_w) {
  uint32_t win[kWideTopK];
#pragma unroll
  for (int j = 0; j < kWideTopK; ++j) {
    win[j] = 0;
    if (j >= k) continue;  // k is uniform
    uint32_t m = keys[0];
#pragma unroll
    for (int i = 1; i < kWideSlots; ++i) m = max(m, keys[i]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 16));
#pragma unroll
    for (int i = 0; i < kWideSlots; ++i) keys[i] = keys[i] == m ? 0u : keys[i];  // keys are distinct: one lane owns m
    win[j] = m;
  }
  const float vmax = wide_key_value(win[0]);
  float vals[kWideTopK];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kWideTopK; ++j) {
    if (j >= k) break;
    vals[j] = __expf(wide_key_value(win[j]) - vmax);
    sum += vals[j];
  }
#pragma unroll
  for (int j = 0; j < kWideTopK; ++j) {
    if (j >= k) break;
    if (store && g == j) {
      topk_ids[(size_t)t * k + j] = 255 - (int)(win[j] & 0xffu);
      topk_w[(size_t)t * k + j] = vals[j] / sum;
    }
  }
}

// top-k of precomputed router logits [T, E] bf16: 16 lanes per token, 16 tokens per workgroup
__global__ void __launch_bounds__(256) moe_topk_wide_kernel(const bf16_t* __restrict__ logits, int T, int E, int k,
                                                            int* __restrict__ topk_ids, float* __restrict__ topk_w) {
  const int g = threadIdx.x & 15;
  const int t = blockIdx.x * kWideTok + (threadIdx.x >> 4);
  const bf16_t* row = logits + (size_t)min(t, T - 1) * E;  // a token past T reads the last row, stores nothing
  uint32_t keys[kWideSlots];
#pragma unroll
  for (int i = 0; i < kWideSlots; ++i) {
    const int e = g + 16 * i;
    keys[i] = 0;
    if (e < E) keys[i] = wide_key(row[e], e);
  }
  route_token_wide(keys, g, k, t, t < T, topk_ids, topk_w);
}

// Router projection on the MFMA fused with the top-k (header).  NT: accumulator tiles compiled in (>= ceil(E / 16)).
template <int NT>
__global__ void __launch_bounds__(kWideWaves * 64) moe_router_wide_kernel(const bf16_t* __restrict__ h, int ldh,
                                                              const bf16_t* __restrict__ router, int T, int E, int d,
                                                              int k, int* __restrict__ topk_ids,
                                                              float* __restrict__ topk_w,
                                                              bf16_t* __restrict__ logits) {
  __shared__ float s_part[kWideWaves][kWideTok][kWideLd];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kg = lane >> 4;
  const int t0 = blockIdx.x * kWideTok;
  const int ntiles = (E + 15) >> 4;  // uniform
  const uint4v zero = {0u, 0u, 0u, 0u};
  float4v acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
  const bf16_t* hrow = h + (size_t)min(t0 + r16, T - 1) * ldh;
#pragma unroll 2
  for (int kk = wv * 32; kk < d; kk += kWideWaves * 32) {
    const int k0 = kk + kg * 8;   // this lane's K chunk of the step (d % 8 == 0: a chunk is inside or outside)
    const bool kin = k0 < d;
    uint4v a = zero, b[NT];
    if (kin) a = *reinterpret_cast<const uint4v*>(hrow + k0);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int e = n * 16 + r16;
      b[n] = zero;
      if (kin && e < E) b[n] = *reinterpret_cast<const uint4v*>(router + (size_t)e * d + k0);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
      if (n < ntiles) acc[n] = mfma_bf16_w(a, b[n], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    if (n < ntiles) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s_part[wv][4 * kg + r][n * 16 + r16] = acc[n][r];
    }
  }
  __syncthreads();
  // 16 lanes per token: lane g sums, rounds and keys the experts g + 16 i
  const int g = threadIdx.x & 15, j = threadIdx.x >> 4;
  const int t = t0 + j;
  const bool live = t < T;
  uint32_t keys[kWideSlots];
#pragma unroll
  for (int i = 0; i < kWideSlots; ++i) {
    const int e = g + 16 * i;
    keys[i] = 0;
    if (e < E) {  // fixed summation order over the waves: deterministic
      float sum = s_part[0][j][e];
#pragma unroll
      for (int w = 1; w < kWideWaves; ++w) sum += s_part[w][j][e];
      const bf16_t lb = f2bf(sum);
      if (logits != nullptr && live) logits[(size_t)t * E + e] = lb;
      keys[i] = wide_key(lb, e);
    }
  }
  route_token_wide(keys, g, k, t, live, topk_ids, topk_w);
}

// Expert segments + dispatch permutation from topk_ids: moe_permute_kernel (moe.hip) with 128-entry tables.
// One workgroup: LDS counts, a two-wave prefix scan, LDS cursors; the ids stay in registers up to 8192 routed
// rows and are re-read above that.  Row order inside an expert's segment is arbitrary (atomics).
__global__ void __launch_bounds__(1024) moe_permute_wide_kernel(const int* __restrict__ topk_ids, int n, int k, int E,
                                                                int* __restrict__ row_off, int* __restrict__ src_row,
                                                                int* __restrict__ inv) {
  __shared__ int s_count[kWideMaxExperts];
  __shared__ int s_cursor[kWideMaxExperts];
  __shared__ int s_half;
  constexpr int PT = 8;
  const int tid = threadIdx.x;
  const bool held = n <= 1024 * PT;
  int ids[PT];
  if (tid < E) s_count[tid] = 0;
  if (held) {
#pragma unroll
    for (int i = 0; i < PT; ++i) ids[i] = tid + 1024 * i < n ? topk_ids[tid + 1024 * i] : -1;
  }
  __syncthreads();
  if (held) {
#pragma unroll
    for (int i = 0; i < PT; ++i)
      if (ids[i] >= 0) atomicAdd(&s_count[ids[i]], 1);
  } else {
    for (int i = tid; i < n; i += 1024) atomicAdd(&s_count[topk_ids[i]], 1);
  }
  __syncthreads();
  // exclusive prefix of the counts by the first two waves (a serial walk of the 128 LDS entries by one thread
  // measured about 1 us slower): a shuffle scan per wave, the first wave's total through LDS
  int cnt = 0, incl = 0;
  if (tid < kWideMaxExperts) {
    cnt = tid < E ? s_count[tid] : 0;
    incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if ((tid & 63) >= o) incl += v;
    }
    if (tid == 63) s_half = incl;
  }
  __syncthreads();
  if (tid < E) {
    const int excl = incl - cnt + (tid >= 64 ? s_half : 0);
    row_off[tid] = excl;
    s_cursor[tid] = excl;
    if (tid == E - 1) row_off[E] = excl + cnt;
  }
  __syncthreads();
  if (held) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      if (ids[i] >= 0) {
        const int idx = tid + 1024 * i;
        const int pos = atomicAdd(&s_cursor[ids[i]], 1);
        src_row[pos] = idx / k;
        inv[idx] = pos;
      }
    }
  } else {
    for (int i = tid; i < n; i += 1024) {
      const int pos = atomicAdd(&s_cursor[topk_ids[i]], 1);
      src_row[pos] = i / k;
      inv[i] = pos;
    }
  }
}

static bool wide_domain(int T, int E, int k) {
  return E >= kWideMinExperts && E <= kWideMaxExperts && k >= 1 && k <= kWideTopK && k <= E && T >= 0 &&
         (long long)T * k <= 0x7fffffffLL;
}

}  // namespace lwc

extern "C" int lwc_moe_permute_wide(const int* topk_ids, int T, int E, int k, int* row_off, int* src_row, int* inv,
                                    hipStream_t s) {
  using namespace lwc;
  if (!wide_domain(T, E, k)) return -1;
  if (T == 0) {
    (void)hipMemsetAsync(row_off, 0, sizeof(int) * (E + 1), s);
    return (int)hipGetLastError();
  }
  moe_permute_wide_kernel<<<1, 1024, 0, s>>>(topk_ids, T * k, k, E, row_off, src_row, inv);
  return (int)hipGetLastError();
}

extern "C" int lwc_moe_route_wide(const void* logits, int T, int E, int k, int* topk_ids, float* topk_w, int* row_off,
                                  int* src_row, int* inv, hipStream_t s) {
  using namespace lwc;
  if (!wide_domain(T, E, k)) return -1;
  if (T == 0) {
    (void)hipMemsetAsync(row_off, 0, sizeof(int) * (E + 1), s);
    return (int)hipGetLastError();
  }
  moe_topk_wide_kernel<<<(T + kWideTok - 1) / kWideTok, 256, 0, s>>>((const bf16_t*)logits, T, E, k, topk_ids,
                                                                      topk_w);
  return lwc_moe_permute_wide(topk_ids, T, E, k, row_off, src_row, inv, s);
}

// h [T, d] bf16 (row stride ldh), router [E, d] bf16 contiguous; logits (optional) [T, E] bf16.
extern "C" int lwc_moe_router_wide(const void* h, int ldh, const void* router, int T, int E, int d, int k,
                                   int* topk_ids, float* topk_w, int* row_off, int* src_row, int* inv, void* logits,
                                   hipStream_t s) {
  using namespace lwc;
  if (!wide_domain(T, E, k) || d < 8 || d % 8 != 0 || ldh % 8 != 0) return -1;
  if (T == 0) {
    (void)hipMemsetAsync(row_off, 0, sizeof(int) * (E + 1), s);
    return (int)hipGetLastError();
  }
  const bf16_t* hp = (const bf16_t*)h;
  const bf16_t* rp = (const bf16_t*)router;
  const dim3 grid((T + kWideTok - 1) / kWideTok);
  const int ntiles = (E + 15) / 16;
#define LWC_ROUTER_WIDE(NT) \
  moe_router_wide_kernel<NT><<<grid, kWideWaves * 64, 0, s>>>(hp, ldh, rp, T, E, d, k, topk_ids, topk_w, (bf16_t*)logits)
  if (ntiles <= 2)
    LWC_ROUTER_WIDE(2);
  else if (ntiles <= 4)
    LWC_ROUTER_WIDE(4);
  else if (ntiles <= 6)
    LWC_ROUTER_WIDE(6);
  else
    LWC_ROUTER_WIDE(8);
#undef LWC_ROUTER_WIDE
  return lwc_moe_permute_wide(topk_ids, T, E, k, row_off, src_row, inv, s);
}
