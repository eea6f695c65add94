// Batched LoRA for rows that carry different adapters (one base model, many voters): per adapted projection
//   shrink:      T[m, :]  = X[m, :] . A[ids[m]]^T          X [M, K] bf16, A [n_adapters, R, K], T [M, R] bf16
//   expand-add:  Y[m, :] += T[m, :] . B[ids[m]]^T          Y [M, N] bf16 (in place), B [n_adapters, N, R]
// with fp32 accumulation; ids[m] outside [0, n_adapters) (the engine writes -1) means "no adapter": shrink
// does not write that row of T, expand-add does not read it and leaves the row of Y bitwise unchanged.
//
// Both kernels work on groups of 16-row tiles and `v_mfma_f32_16x16x32_bf16` with the adapter weights as the A
// operand (lane (r16, g): weight row r16, k 8g..8g+7 of the step) and the activations as the B operand (lane
// (r16, g): activation row r16, the same k), so the accumulator of lane (r16, g) holds, for activation row
// r16, the 4 consecutive output columns 4g..4g+3 of the 16-column tile: one 8-byte store of T, one 8-byte
// load and store of Y per lane, every element of Y touched by exactly one lane (no atomics).
//
// Adapters inside a group: rows of a decode batch arrive grouped by request, so a group usually has one
// adapter; any mixture is still handled: the adapters present in the group are collected into a 64-bit mask
// by wave ballots (wave-uniform, and equal in every wave of the workgroup: they read the same ids), the
// product is formed once per present adapter over the whole group and each lane keeps the result of its own
// row's adapter.  A group with no adapter at all returns before any access but the ids.
//
// Rows past M take id -1 and their addresses are formed from row 0 (never past the buffers); columns past N
// (N % 16 == 8) read weight row 0 and are not stored.
//
// shrink: a workgroup of NW waves owns MT 16-row tiles and splits K between its waves in chunks of 64 (lane
// (r16, g) reads the 32 contiguous bytes k = 64 c + 16 g .. + 15 of its row: two MFMA steps whose k order is
// permuted the same way in both operands); the NW partial tiles meet in LDS (at most 48 KiB) and are summed in
// wave order.  (MT, NW) by launch_shrink: the adapter's A rows (R x K, L2 resident) are read once per
// workgroup, so more rows per workgroup means fewer re-reads, more waves more loads in flight.
// expand-add: a workgroup owns 64 rows; each wave keeps the T fragments of the 4 row tiles in registers and
// walks 16-column tiles of Y, reading the adapter's B rows of that tile (16 x R) once for the 64 rows.
#include "common.h"
#include "launchers.h"

namespace lwc {
namespace lora {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int NWV = 4;  // waves per workgroup

LWC_DEVICE float4v mfma(const uint4v& a, const uint4v& b, const float4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                 0, 0);
}

LWC_DEVICE uint4v ld16(const bf16_t* p) { return *reinterpret_cast<const uint4v*>(p); }

// ids of this lane's row in each of the group's MT tiles (-1: none / past M), the row to form addresses from
// (row 0 when past M) and the wave-uniform mask of adapters present per tile
template <int MT>
struct Rows {
  int id[MT];
  long long row[MT];
  uint64_t present[MT];
  uint64_t any;
};

template <int MT>
LWC_DEVICE Rows<MT> load_rows(const int* ids, long long m0, int r16, int M, int n_adapters) {
  Rows<MT> r;
  r.any = 0;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const long long m = m0 + 16 * mt + r16;
    const bool ok = m < M;
    int id = ok ? ids[m] : -1;
    if (id < 0 || id >= n_adapters) id = -1;
    r.id[mt] = id;
    r.row[mt] = ok ? m : 0;
    r.present[mt] = 0;
  }
  for (int a = 0; a < n_adapters; ++a) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      if (__ballot(r.id[mt] == a) != 0) r.present[mt] |= 1ull << a;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) r.any |= r.present[mt];
  return r;
}

struct ShrinkParams {
  const bf16_t* X;
  const bf16_t* A;
  const int* ids;
  bf16_t* T;
  int M, K, R, ldx, n_adapters;
};

template <int NRT, int MT, int NW>
__global__ void __launch_bounds__(64 * NW) shrink_kernel(ShrinkParams p) {
  extern __shared__ float4v red[];  // [NW][NRT][MT][64]
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const long long m0 = (long long)blockIdx.x * (16 * MT);
  const Rows<MT> rows = load_rows<MT>(p.ids, m0, r16, p.M, p.n_adapters);
  if (rows.any == 0) return;
  const int nchunks = p.K / 64;
  const bf16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xp[mt] = p.X + (size_t)rows.row[mt] * p.ldx + 16 * g;

  for (uint64_t rem = rows.any; rem != 0; rem &= rem - 1) {
    const int a = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)rem) - 1);
    const bf16_t* ap = p.A + ((size_t)a * p.R + r16) * p.K + 16 * g;
    float4v acc[NRT][MT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = float4v{0.f, 0.f, 0.f, 0.f};
    for (int c = w; c < nchunks; c += NW) {
      const int k = c * 64;
      uint4v xf[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        xf[mt][0] = ld16(xp[mt] + k);
        xf[mt][1] = ld16(xp[mt] + k + 8);
      }
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        const bf16_t* q = ap + (size_t)(16 * rt) * p.K + k;
        const uint4v a0 = ld16(q), a1 = ld16(q + 8);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acc[rt][mt] = mfma(a0, xf[mt][0], acc[rt][mt]);
          acc[rt][mt] = mfma(a1, xf[mt][1], acc[rt][mt]);
        }
      }
    }
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[((w * NRT + rt) * MT + mt) * 64 + lane] = acc[rt][mt];
    __syncthreads();
    // wave (rt MT + mt) % NW finishes tile (rt, mt): the partials in wave order, rows of adapter a stored
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if ((rt * MT + mt) % NW != w) continue;
        float4v s = red[((0 * NRT + rt) * MT + mt) * 64 + lane];
#pragma unroll
        for (int k = 1; k < NW; ++k) s += red[((k * NRT + rt) * MT + mt) * 64 + lane];
        if (rows.id[mt] == a) {
          uint2 o;
          o.x = pack_bf16x2(s[0], s[1]);
          o.y = pack_bf16x2(s[2], s[3]);
          *reinterpret_cast<uint2*>(p.T + (size_t)rows.row[mt] * p.R + 16 * rt + 4 * g) = o;
        }
      }
    __syncthreads();
  }
}

template <int NRT, int MT, int NW>
int launch_shrink_as(const ShrinkParams& p, hipStream_t s) {
  static_assert(NW * NRT * MT <= 48, "LDS partials: 1 KiB per (wave, r-tile, row tile), at most 48 KiB");
  const unsigned grid = (unsigned)((p.M + 16 * MT - 1) / (16 * MT));
  shrink_kernel<NRT, MT, NW><<<dim3(grid), 64 * NW, NW * NRT * MT * 64 * sizeof(float4v), s>>>(p);
  return (int)hipGetLastError();
}

// Up to 8192 rows one 16-row tile per workgroup and as many waves splitting K as the LDS partials allow (16 / 8 /
// 4 for R <= 48 / 96 / 192): M / 16 workgroups are few for 256 CUs, so the waves have to come from inside
// them.  Beyond that the row tiles alone fill the device: 4 waves on 4 / 2 / 1 row tiles, the adapter's A rows
// read once for all of them.
template <int NRT>
int launch_shrink(const ShrinkParams& p, hipStream_t s) {
  if (p.M <= 8192) return launch_shrink_as < NRT, 1, NRT <= 3 ? 16 : (NRT <= 6 ? 8 : 4) > (p, s);
  return launch_shrink_as < NRT, NRT <= 3 ? 4 : (NRT <= 6 ? 2 : 1), 4 > (p, s);
}

struct ExpandParams {
  bf16_t* Y;
  const bf16_t* T;
  const bf16_t* B;
  const int* ids;
  int M, N, R, ldy, n_adapters;
};

// KS: k-steps of 32 covering R (the upper half of the last step is zero when R % 32 == 16)
template <int KS>
__global__ void __launch_bounds__(256) expand_kernel(ExpandParams p) {
  constexpr int MT = 4;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const long long m0 = (long long)blockIdx.x * (16 * MT);
  const Rows<MT> rows = load_rows<MT>(p.ids, m0, r16, p.M, p.n_adapters);
  if (rows.any == 0) return;
  const uint4v zero = uint4v{0u, 0u, 0u, 0u};
  uint4v tf[MT][KS];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 32 * s + 8 * g;
      tf[mt][s] = (k < p.R && rows.id[mt] >= 0) ? ld16(p.T + (size_t)rows.row[mt] * p.R + k) : zero;
    }
  const int nct = (p.N + 15) / 16;
  for (int ct = blockIdx.y * NWV + w; ct < nct; ct += gridDim.y * NWV) {
    const int n = ct * 16 + r16;
    const int brow = n < p.N ? n : 0;
    float4v acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = float4v{0.f, 0.f, 0.f, 0.f};
    for (uint64_t rem = rows.any; rem != 0; rem &= rem - 1) {
      const int a = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)rem) - 1);
      const bf16_t* bp = p.B + ((size_t)a * p.N + brow) * p.R + 8 * g;
      uint4v bf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) bf[s] = (32 * s + 8 * g < p.R) ? ld16(bp + 32 * s) : zero;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (((rows.present[mt] >> a) & 1) == 0) continue;
        float4v t = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) t = mfma(bf[s], tf[mt][s], t);
        if (rows.id[mt] == a) acc[mt] = t;
      }
    }
    const int col = ct * 16 + 4 * g;
    if (col < p.N) {  // N % 8 == 0: the 4 columns are all inside or all outside
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (rows.id[mt] < 0) continue;
        uint2* yp = reinterpret_cast<uint2*>(p.Y + (size_t)rows.row[mt] * p.ldy + col);
        const uint2 y = *yp;
        uint2 o;
        o.x = pack_bf16x2(__uint_as_float(y.x << 16) + acc[mt][0], __uint_as_float(y.x & 0xffff0000u) + acc[mt][1]);
        o.y = pack_bf16x2(__uint_as_float(y.y << 16) + acc[mt][2], __uint_as_float(y.y & 0xffff0000u) + acc[mt][3]);
        *yp = o;
      }
    }
  }
}

template <int KS>
int launch_expand(const ExpandParams& p, hipStream_t s) {
  const int gx = (p.M + 63) / 64;
  const int nct = (p.N + 15) / 16;
  // column tiles per wave: 4 once the row groups alone fill the device, else 1 (decode-sized M)
  const int per_wave = gx >= 32 ? 4 : 1;
  const int gy = (nct + NWV * per_wave - 1) / (NWV * per_wave);
  expand_kernel<KS><<<dim3((unsigned)gx, (unsigned)gy), 256, 0, s>>>(p);
  return (int)hipGetLastError();
}

inline bool shape_ok(int M, int R, int n_adapters) {
  return M >= 0 && R >= 16 && R <= 192 && R % 16 == 0 && n_adapters >= 1 && n_adapters <= 64;
}

}  // namespace lora
}  // namespace lwc

// T[m] = X[m] . A[ids[m]]^T for rows with an adapter.  -1: shape not taken.
extern "C" int lwc_lora_shrink(const void* X, const void* A, const int* ids, void* T, int M, int K, int R, int ldx,
                               int n_adapters, hipStream_t s) {
  using namespace lwc::lora;
  if (!shape_ok(M, R, n_adapters) || K <= 0 || K % 64 != 0 || ldx < K || ldx % 8 != 0) return -1;
  if (((uintptr_t)X | (uintptr_t)A) % 16 != 0 || (uintptr_t)T % 8 != 0) return -1;
  if (M == 0) return 0;
  ShrinkParams p{(const lwc::bf16_t*)X, (const lwc::bf16_t*)A, ids, (lwc::bf16_t*)T, M, K, R, ldx, n_adapters};
  switch (R / 16) {
    case 1: return launch_shrink<1>(p, s);
    case 2: return launch_shrink<2>(p, s);
    case 3: return launch_shrink<3>(p, s);
    case 4: return launch_shrink<4>(p, s);
    case 5: return launch_shrink<5>(p, s);
    case 6: return launch_shrink<6>(p, s);
    case 7: return launch_shrink<7>(p, s);
    case 8: return launch_shrink<8>(p, s);
    case 9: return launch_shrink<9>(p, s);
    case 10: return launch_shrink<10>(p, s);
    case 11: return launch_shrink<11>(p, s);
    case 12: return launch_shrink<12>(p, s);
  }
  return -1;
}

// Y[m] += T[m] . B[ids[m]]^T in place for rows with an adapter.  -1: shape not taken.
extern "C" int lwc_lora_expand_add(void* Y, const void* T, const void* B, const int* ids, int M, int N, int R, int ldy,
                                   int n_adapters, hipStream_t s) {
  using namespace lwc::lora;
  if (!shape_ok(M, R, n_adapters) || N <= 0 || N % 8 != 0 || ldy < N || ldy % 4 != 0) return -1;
  if (((uintptr_t)T | (uintptr_t)B) % 16 != 0 || (uintptr_t)Y % 8 != 0) return -1;
  if (M == 0) return 0;
  ExpandParams p{(lwc::bf16_t*)Y, (const lwc::bf16_t*)T, (const lwc::bf16_t*)B, ids, M, N, R, ldy, n_adapters};
  switch ((R + 31) / 32) {
    case 1: return launch_expand<1>(p, s);
    case 2: return launch_expand<2>(p, s);
    case 3: return launch_expand<3>(p, s);
    case 4: return launch_expand<4>(p, s);
    case 5: return launch_expand<5>(p, s);
    case 6: return launch_expand<6>(p, s);
  }
  return -1;
}
