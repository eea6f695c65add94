// MoE expert projections over MXFP4 weights: moe_skinny_mxfp4, the grouped form of skinny_mxfp4 (mxfp4.hip).
//
// W is an expert stack in the format of mxfp4.hip, Q [E, N, K / 2] and S [E, N, K / 32], read as stored.  One
// launch covers all experts: workgroup (x, e) computes 16 output columns of expert e (SwiGLU: a gate tile and an
// up tile, as EPI == 2 does in the dense kernel) for the rows [row_off[e], row_off[e + 1]) of the expert-major
// output, bounds it reads from device memory (the router's row_off: no host step, graph-capturable).
//   * An empty segment returns before any weight load (decode at B = 1: 120 of 128 experts).
//   * A segment is walked in chunks of at most 64 rows; the weight tile is streamed again for each chunk.  The
//     number of 16-row m-tiles of a chunk (1, 2 or 4) is a wave-uniform choice made here from the bounds: the host
//     does not know segment lengths.
//   * Output row i of the segment is row row_off[e] + i of C.  Its activation row is A[a_rows[row_off[e] + i]]
//     (the router's gather, gate|up) or, without a_rows, row row_off[e] + i of A (down).
//
// The contract:
//   1. Bitwise the dense kernel.  The K split (8 waves, whole 128-k batches: wave w takes batches [w nb / 8,
//      (w + 1) nb / 8)), the order of the MFMA steps into an accumulator, the fixed-order LDS reduction over the
//      8 waves and the SwiGLU expression are those of skinny_kernel, so for any chunk the output rows are bit for
//      bit what skinny_mxfp4(A[those rows], W[e]) returns.  (How many m-tiles or weight tiles share a workgroup
//      does not enter an output element's arithmetic: each (weight tile, m-tile) pair has its own accumulator.)
//   2. Row independence, which follows from 1: a row's result depends on its own activation row and its expert's
//      weights only, not on the segment's length, the row's position in a chunk or the neighbouring experts.
//
// Lanes of an m-tile past the segment's end: the rows after it belong to the next expert, so such a lane never
// stores; it does not use a_rows (whose entry there is another expert's, or past the array); and its activation
// loads go to an offset past the activation resource's end (bit 31 set; every valid offset is below 2^31, which
// the launcher checks), which returns zeros without touching memory.  a_rows itself is read through a resource of
// rows entries, and the bounds are clamped to [0, rows], so no index the kernel forms depends on the tensors'
// contents being right.
//
// Requires K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0), lda % 4 == 0, ldc % 4 == 0, and the per-expert weight
// bytes, the activation extent and 4 rows below 2^31 (the 32-bit buffer offsets); anything else is refused (-1).
#include "common.h"
#include "launchers.h"
#include "mxfp4_cvt.h"

namespace lwc {
namespace moe_mxfp4 {

using mxfp4::cvt8;
using mxfp4::e8m0;
using mxfp4::KS;
using mxfp4::mfma;

constexpr int MAXMT = 4;  // m-tiles of a 64-row chunk

struct Params {
  const bf16_t* A;
  const uint8_t* Q;  // [E, N, K / 2]
  const uint8_t* S;  // [E, N, K / 32]
  bf16_t* C;
  const int* row_off;  // [E + 1]
  const int* a_rows;   // [rows] or null
  int rows;            // rows of C (entries of a_rows)
  int a_bytes;         // extent of A in bytes
  int N, K, lda, ldc;
};

// One chunk: rows [m0, hi) of the segment, at most 16 MT of them, times the workgroup's NW weight tiles.  The
// loop over batches, the reduction and the epilogue are skinny_kernel's (mxfp4.hip), statement for statement.
template <int MT, int EPI, int NW>
LWC_DEVICE void chunk(const Params& p, float4v (&red)[KS][NW][MAXMT][64], const __amdgpu_buffer_rsrc_t rQ,
                      const __amdgpu_buffer_rsrc_t rS, const __amdgpu_buffer_rsrc_t rA,
                      const __amdgpu_buffer_rsrc_t rR, int m0, int hi, int n0) {
  constexpr int TS = EPI == 2 ? 32 : 16;  // W rows between the NW tiles
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int nbt = p.K / 128;                 // 128-k batches in all
  const int b0 = (w * nbt) / KS;             // this wave's batches [b0, b0 + nb)
  const int nb = ((w + 1) * nbt) / KS - b0;
  const int qrow = p.K / 2, srow = p.K / 32;  // bytes per row of Q / S
  uint32_t voQ[NW], voS[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t) {
    voQ[t] = (uint32_t)((r16 + TS * t) * qrow + b0 * 64 + 16 * g);
    voS[t] = (uint32_t)((r16 + TS * t) * srow + b0 * 4 + g);
  }
  uint32_t voA[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int i = m0 + mt * 16 + r16;  // this lane's row of C
    uint32_t src = (uint32_t)i;
    if (p.a_rows != nullptr) src = __builtin_amdgcn_raw_buffer_load_b32(rR, (uint32_t)i * 4u, 0, 0);
    voA[mt] = i < hi ? (src * (uint32_t)p.lda + (uint32_t)(b0 * 128 + 32 * g)) * 2u : 0x80000000u;
  }

  float4v acc[NW][MT];
#pragma unroll
  for (int t = 0; t < NW; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = float4v{0.f, 0.f, 0.f, 0.f};
  // two register sets of U batches each, as in the dense kernel (U = 2 up to 16 rows).  A batch index past the
  // wave's last loads from past the resources' ends: zeros, which add nothing
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
              uint4v, __builtin_amdgcn_raw_buffer_load_b128(rA, voA[mt] | past, b * 256 + s * 16, 0));
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
    const int m = m0 + w * 16 + r16;
    if (m < hi) {  // (a row past the segment's end is the next expert's)
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

// grid (column tiles, experts).  EPI 2 (SwiGLU, W[e] = [gate; up] interleaved in blocks of 32 rows): the 16 output
// columns' gate rows 64 (x / 2) + 16 (x % 2) + [0, 16) and the up rows 32 further (NW = 2); EPI 0: 16 columns
template <int EPI, int NW>
__global__ void __launch_bounds__(512) moe_skinny_kernel(Params p) {
  static_assert(EPI != 2 || NW == 2, "SwiGLU pairs a gate and an up tile");
  __shared__ float4v red[KS][NW][MAXMT][64];
  const int e = blockIdx.y;
  const int lo = __builtin_amdgcn_readfirstlane(max(p.row_off[e], 0));
  const int hi = __builtin_amdgcn_readfirstlane(min(p.row_off[e + 1], p.rows));
  if (lo >= hi) return;  // an idle expert: nothing of its weights is read
  constexpr int TS = EPI == 2 ? 32 : 16;
  const int n0 = blockIdx.x * (EPI == 2 ? 16 : 16 * NW);  // first output column
  const int wrow = EPI == 2 ? 64 * (blockIdx.x >> 1) + 16 * (blockIdx.x & 1) : n0;  // first W row of the expert
  const int rows = 16 + TS * (NW - 1);       // W rows the workgroup reads
  const int qrow = p.K / 2, srow = p.K / 32;
  const size_t first = (size_t)e * p.N + wrow;  // row of the stack
  const __amdgpu_buffer_rsrc_t rQ = uniform_rsrc(p.Q + first * qrow, rows * qrow);
  const __amdgpu_buffer_rsrc_t rS = uniform_rsrc(p.S + first * srow, rows * srow);
  const __amdgpu_buffer_rsrc_t rA = uniform_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rR = uniform_rsrc(p.a_rows, p.a_rows != nullptr ? p.rows * 4 : 0);
  for (int m0 = lo; m0 < hi; m0 += 64) {
    if (m0 != lo) __syncthreads();  // the last chunk's reduction has read red
    const int mt = (min(hi - m0, 64) + 15) >> 4;
    if (mt == 1)
      chunk<1, EPI, NW>(p, red, rQ, rS, rA, rR, m0, hi, n0);
    else if (mt == 2)
      chunk<2, EPI, NW>(p, red, rQ, rS, rA, rR, m0, hi, n0);
    else
      chunk<4, EPI, NW>(p, red, rQ, rS, rA, rR, m0, hi, n0);
  }
}

}  // namespace moe_mxfp4
}  // namespace lwc

// C[row_off[e] + i] = A[src(row_off[e] + i)] . W[e]^T (epi 0) or the SwiGLU of a 32-row gate/up interleaved W[e]
// (epi 2, C [rows, N / 2]) for every expert e and row i of its segment; src = a_rows[.] or the identity.  A has
// a_nrows rows of lda elements.  -1: shape not taken (nothing was launched).
extern "C" int lwc_moe_skinny_mxfp4(const void* A, const void* Q, const void* S, void* C, const int* row_off,
                                    const int* a_rows, int E, long long rows, long long a_nrows, int N, int K,
                                    int lda, int ldc, int epi, hipStream_t s) {
  using namespace lwc::moe_mxfp4;
  const int NC = epi == 2 ? N / 2 : N;
  if (epi != 0 && epi != 2) return -1;
  if (E <= 0 || E > 65535 || rows < 0 || a_nrows < 0 || K <= 0 || K % 128 != 0 || N < 0 ||
      N % (epi == 2 ? 64 : 16) != 0 || lda % 4 != 0 || ldc % 4 != 0 || lda < K || ldc < NC)
    return -1;
  if (a_rows == nullptr && a_nrows < rows) return -1;
  // what the 32-bit buffer offsets index: an expert's codes, the (gathered) activation extent, a_rows
  if ((long long)N * (K / 2) >= (1LL << 31) || a_nrows * lda * 2 >= (1LL << 31) || rows * 4 >= (1LL << 31)) return -1;
  if (rows == 0 || N == 0 || a_nrows == 0) return 0;
  const int a_bytes = (int)(((a_nrows - 1) * lda + K) * 2);
  Params p{(const lwc::bf16_t*)A, (const uint8_t*)Q, (const uint8_t*)S, (lwc::bf16_t*)C, row_off, a_rows,
           (int)rows,             a_bytes,           N,                 K,               lda,     ldc};
  const dim3 grid(epi == 2 ? N / 32 : N / 16, E);  // SwiGLU: N / 2 output columns, 16 per workgroup
  if (epi == 2)
    moe_skinny_kernel<2, 2><<<grid, 512, 0, s>>>(p);
  else
    moe_skinny_kernel<0, 1><<<grid, 512, 0, s>>>(p);
  return (int)hipGetLastError();
}
