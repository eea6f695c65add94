// MXFP4 weight-only projections: W [N, K] as OCP e2m1 codes (two per byte, k = 2j in the low nibble of byte j
// of a row) with one e8m0 scale byte per 32 consecutive k of a row (value 2^(s - 127)).  Every e2m1 x 2^e value
// is a bf16, and gfx950 converts two codes to two bf16 with the block scale applied in one VALU instruction
// (v_cvt_scalef32_pk_bf16_fp4: the selected byte's low nibble lands in the low half of the result).
//
//   * mxfp4_dequant: packed rows -> bf16 [N, K] in a caller-owned buffer (the M > 64 path: prefill and the
//     large decode buckets then run the bf16 GEMMs on it).  One thread per 8 codes: a 4-byte load, four
//     converts, one 16-byte store.
//   * skinny_mxfp4: the weight-stream GEMM of skinny.hip (M <= 64) reading W in this form, 3.76x fewer bytes
//     than bf16.  One workgroup per 16 (or 32) output columns, 8 waves splitting K, partials summed in LDS in
//     wave order; W is the MFMA A operand, so a lane's accumulator holds 4 consecutive output columns.
//     Per 128-k batch, lane (r16, g) loads the 16 contiguous bytes of row r16 at k in [128 b + 32 g, + 32):
//     exactly one MX block, so one scale per lane and batch.  Dword s of those bytes converts into the A
//     fragment of step s (8 bf16); the MFMA's k index (g, j) of step s is therefore k = 128 b + 32 g + 8 s + j,
//     and the activation fragment of that step is A[m, 128 b + 32 g + 8 s .. + 8) — the lane's four steps
//     read 64 contiguous bytes of its activation row.
//     K is split in whole batches: wave w takes batches [w nb / 8, (w + 1) nb / 8), any count from zero up
//     (K = 128: seven waves add a zero tile).  Rows past M read zeros (offsets past the activation
//     resource's end) and are not stored.
//
// Requires K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0), M <= 64, lda % 4 == 0, ldc % 4 == 0.
#include "common.h"
#include "launchers.h"
#include "mxfp4_cvt.h"

namespace lwc {
namespace mxfp4 {

// thread t: dword t of q (codes 8 t .. 8 t + 7 of the flat [N, K] weight), scale byte t / 4
__global__ void __launch_bounds__(256) dequant_kernel(const uint32_t* __restrict__ q, const uint8_t* __restrict__ s,
                                                      uint4v* __restrict__ out, long long n8) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n8) return;
  out[t] = cvt8(q[t], e8m0(s[t >> 2]));
}

struct Params {
  const bf16_t* A;
  const uint8_t* Q;  // [N, K / 2]
  const uint8_t* S;  // [N, K / 32]
  bf16_t* C;
  int M, N, K, lda, ldc;
};

// NW weight tiles of 16 rows per workgroup on the same activation fragments, as in skinny.hip: EPI 2 (SwiGLU, W
// = [gate; up] interleaved in blocks of 32 rows) takes its 16 output columns' gate rows 64 (x / 2) + 16 (x % 2)
// + [0, 16) and the up rows 32 further (NW = 2); EPI 0 takes 16 (NW = 1) or 32 adjacent output columns (NW = 2)
template <int MT, int EPI, int NW>
__global__ void __launch_bounds__(512) skinny_kernel(Params p) {
  static_assert(EPI != 2 || NW == 2, "SwiGLU pairs a gate and an up tile");
  constexpr int TS = EPI == 2 ? 32 : 16;  // W rows between the NW tiles
  __shared__ float4v red[KS][NW][MT][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (EPI == 2 ? 16 : 16 * NW);  // first output column
  const int wrow = EPI == 2 ? 64 * (blockIdx.x >> 1) + 16 * (blockIdx.x & 1) : n0;  // first W row
  const int nbt = p.K / 128;                 // 128-k batches in all
  const int b0 = (w * nbt) / KS;             // this wave's batches [b0, b0 + nb)
  const int nb = ((w + 1) * nbt) / KS - b0;
  const int rows = 16 + TS * (NW - 1);       // W rows the workgroup reads
  const int qrow = p.K / 2, srow = p.K / 32;  // bytes per row of Q / S
  const __amdgpu_buffer_rsrc_t rQ = uniform_rsrc(p.Q + (size_t)wrow * qrow, rows * qrow);
  const __amdgpu_buffer_rsrc_t rS = uniform_rsrc(p.S + (size_t)wrow * srow, rows * srow);
  const __amdgpu_buffer_rsrc_t rA = uniform_rsrc(p.A, ((p.M - 1) * p.lda + p.K) * 2);
  uint32_t voQ[NW], voS[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) {
    voQ[t] = (uint32_t)((r16 + TS * t) * qrow + b0 * 64 + 16 * g);
    voS[t] = (uint32_t)((r16 + TS * t) * srow + b0 * 4 + g);
  }
  uint32_t voA[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) voA[mt] = (uint32_t)(((mt * 16 + r16) * p.lda + b0 * 128 + 32 * g) * 2);

  float4v acc[NW][MT];
#pragma unroll
  for (int t = 0; t < NW; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = float4v{0.f, 0.f, 0.f, 0.f};
  // two register sets of U batches each: set s + 1's loads go out before set s's converts and MFMAs.  Up to 16
  // rows U = 2: a wave of a K = 4096 projection (4 batches) has all its loads in flight at once — at these row
  // counts the kernel is a few memory round trips long, and each one saved shows.  A batch index past the wave's
  // last (an odd count) loads from past the resources' ends: zeros, which add nothing
  constexpr int U = MT == 1 ? 2 : 1;
  uint4v wq[2][U][NW], af[2][U][4][MT];
  uint32_t ws[2][U][NW];
  auto load = [&](int sb, uint4v(&qb)[U][NW], uint32_t(&sc)[U][NW], uint4v(&ab)[U][4][MT]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int b = sb * U + u;
      const uint32_t past = (U > 1 && b >= nb) ? 0x80000000u : 0u;  // wave-uniform
#pragma unroll
      for (int t = 0; t < NW; ++t) {
        qb[u][t] = __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(rQ, voQ[t] + past, b * 64, 0));
        sc[u][t] = __builtin_amdgcn_raw_buffer_load_b8(rS, voS[t] + past, b * 4, 0);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          ab[u][s][mt] = __builtin_bit_cast(
              uint4v, __builtin_amdgcn_raw_buffer_load_b128(rA, voA[mt] + past, b * 256 + s * 16, 0));
    }
  };
  auto compute = [&](const uint4v(&qb)[U][NW], const uint32_t(&sc)[U][NW], const uint4v(&ab)[U][4][MT]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NW; ++t) {
        const float scale = e8m0(sc[u][t] & 0xffu);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const uint4v wf = cvt8(qb[u][t][s], scale);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[t][mt] = mfma(wf, ab[u][s][mt], acc[t][mt]);
        }
      }
  };
  // straight-line pairs in the steady state; the one or two sets left (and a wave with none) end under
  // wave-uniform branches
  const int ns = (nb + U - 1) / U;
  if (ns > 0) {
    load(0, wq[0], ws[0], af[0]);
    int b = 0;
    for (; b + 2 < ns; b += 2) {
      load(b + 1, wq[1], ws[1], af[1]);
      __builtin_amdgcn_sched_barrier(0);
      compute(wq[0], ws[0], af[0]);
      __builtin_amdgcn_sched_barrier(0);
      load(b + 2, wq[0], ws[0], af[0]);
      __builtin_amdgcn_sched_barrier(0);
      compute(wq[1], ws[1], af[1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (b + 2 == ns) {
      load(b + 1, wq[1], ws[1], af[1]);
      __builtin_amdgcn_sched_barrier(0);
      compute(wq[0], ws[0], af[0]);
      __builtin_amdgcn_sched_barrier(0);
      compute(wq[1], ws[1], af[1]);
    } else {
      compute(wq[0], ws[0], af[0]);
    }
  }
#pragma unroll
  for (int t = 0; t < NW; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) red[w][t][mt][lane] = acc[t][mt];
  __syncthreads();
  if (w < MT) {  // wave w finishes m-tile w: the 8 partials in wave order
    float4v sum[NW];
#pragma unroll
    for (int t = 0; t < NW; ++t) {
      sum[t] = red[0][t][w][lane];
#pragma unroll
      for (int k = 1; k < KS; ++k) sum[t] += red[k][t][w][lane];
    }
    constexpr int NO = EPI == 2 ? 1 : NW;  // 16-column output groups
    if constexpr (EPI == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[0][e] = sum[0][e] * __builtin_amdgcn_rcpf(1.f + __expf(-sum[0][e])) * sum[1][e];
    }
    const int m = w * 16 + r16;
    if (m < p.M) {
#pragma unroll
      for (int t = 0; t < NO; ++t) {
        const size_t off = (size_t)m * p.ldc + n0 + 16 * t + 4 * g;
        uint2 o;
        o.x = pack_bf16x2(sum[t][0], sum[t][1]);
        o.y = pack_bf16x2(sum[t][2], sum[t][3]);
        *reinterpret_cast<uint2*>(p.C + off) = o;
      }
    }
  }
}

template <int EPI, int NW>
int launch_nw(const Params& p, hipStream_t s) {
  const int mt = (p.M + 15) / 16;
  const dim3 grid(EPI == 2 ? p.N / 32 : p.N / (16 * NW));  // SwiGLU: N / 2 output columns, 16 per workgroup
  switch (mt) {
    case 1: skinny_kernel<1, EPI, NW><<<grid, 512, 0, s>>>(p); break;
    case 2: skinny_kernel<2, EPI, NW><<<grid, 512, 0, s>>>(p); break;
    case 3:
    case 4: skinny_kernel<4, EPI, NW><<<grid, 512, 0, s>>>(p); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace mxfp4
}  // namespace lwc

// out [N, K] bf16 = the MXFP4 weight (q [N, K / 2], s [N, K / 32]), exact.  -1: shape not taken.
extern "C" int lwc_mxfp4_dequant(const void* q, const void* s, void* out, long long N, long long K, hipStream_t st) {
  using namespace lwc::mxfp4;
  if (N < 0 || K < 0 || K % 32 != 0) return -1;
  const long long n8 = N * K / 8;
  if (n8 == 0) return 0;
  const long long blocks = (n8 + 255) / 256;
  if (blocks >= (1LL << 31)) return -1;
  dequant_kernel<<<dim3((unsigned)blocks), 256, 0, st>>>((const uint32_t*)q, (const uint8_t*)s, (lwc::uint4v*)out, n8);
  return (int)hipGetLastError();
}

// C = A . W^T (epi 0) or silu(A . Wg^T) * (A . Wu^T) over a 32-row gate/up interleaved W (epi 2, C [M, N / 2])
// for M <= 64 rows, W in MXFP4.  -1: shape not taken.
extern "C" int lwc_skinny_mxfp4(const void* A, const void* Q, const void* S, void* C, int M, int N, int K, int lda,
                                int ldc, int epi, hipStream_t s) {
  using namespace lwc::mxfp4;
  const int NC = epi == 2 ? N / 2 : N;
  if (epi != 0 && epi != 2) return -1;
  if (M < 0 || M > 64 || K <= 0 || K % 128 != 0 || N % (epi == 2 ? 64 : 16) != 0 || lda % 4 != 0 || ldc % 4 != 0 ||
      lda < K || ldc < NC)
    return -1;
  if ((long long)48 * K >= (1LL << 31) || (long long)M * lda * 2 >= (1LL << 31)) return -1;
  if (M == 0 || N == 0) return 0;
  Params p{(const lwc::bf16_t*)A, (const uint8_t*)Q, (const uint8_t*)S, (lwc::bf16_t*)C, M, N, K, lda, ldc};
  if (epi == 2) return launch_nw<2, 2>(p, s);
  // 32 output columns per workgroup when that still leaves >= 192 workgroups, at every row count: the
  // activation loads per weight byte halve (qkv at M = 8 / 16: 10.9 -> 9.1 / 13.7 -> 10.6 us); with 128
  // workgroups (o, down) it lost 10-40 % at every M
  if (N % 32 == 0 && N / 32 >= 192) return launch_nw<0, 2>(p, s);
  return launch_nw<0, 1>(p, s);
}
