// W4A8 projections over an MXFP4 weight: e4m3 activations x packed e2m1 weights on the block-scaled MFMA, for
// the row counts where the weight stream of mxfp4.hip no longer pays (M > 64: prefill, mixed steps, large decode
// batches).  The packed weight is read as it is stored (ops/mxfp4.py): no dequantisation pass, no scratch.
//
//   C[m, n] = bf16( a_scale[m] * sum_k e4m3(Aq[m, k]) * e2m1(Wq[n, k]) * 2^(S[n, k / 32] - 127) )
//
//   Aq [M, K] e4m3 (row stride lda >= K bytes, rows 16-byte aligned), a_scale [M] f32 (per-row, epilogue);
//   Wq [N, K / 2] bytes (k = 2j in the low nibble of byte j), S [N, K / 32] e8m0 bytes; C bf16 [M, N], or with the
//   SwiGLU epilogue (W rows gate|up interleaved in blocks of 32, as skinny_mxfp4 reads them) [M, N / 2].
//
// MFMA: v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (cbsz 0, 8 VGPRs, unit scale 127) and B = e2m1 (blgp 4,
// 4 VGPRs), the weight's e8m0 byte as B's scale operand: one instruction per 16 x 16 tile and 128 k, no convert.
// Operand maps of the MIXED form, measured on an MI355X with a one-wave one-hot probe over all 128 positions of
// each operand (bit-coded e2m1 columns, a distinct scale byte per lane group and byte position) and pinned by
// tests/test_mxfp4_a8_gpu.py::test_onehot_rows_read_single_weights_exactly:
//   * the instruction has ONE logical k and each format keeps its own lane map; element i of one operand does
//     NOT pair with element i of the other.  The e2m1 operand: lane (r16, g) holds the 32 codes of row r16 at
//     k = 32 g .. 32 g + 31, k ascending from the low nibble of byte 0 — the 16 contiguous stored bytes of one MX
//     block.  The e4m3 operand keeps the map it has against another e4m3 operand (gemm8g.hip): lane (r16, g) holds
//     k = 16 g .. 16 g + 15 in VGPRs 0-3 and k = 64 + 16 g .. + 15 in VGPRs 4-7 — the row's 16-byte chunks g and
//     4 + g, not the 32 bytes of the e2m1 lane's block.
//   * B's scale for the MX block k = [32 b, 32 b + 32) is read from lane (r16, b) — the lane that holds the block's
//     codes — and op_sel n picks byte n of that lane's scale VGPR.  The kernel uses op_sel 0: byte 0 carries the
//     scale, the other bytes are ignored (A's scale VGPR is 127 in byte 0: unit).
//   * C/D: col (n) = lane & 15, row (m) = 4 (lane >> 4) + reg, as every 16 x 16 MFMA.
//
// Schedule: gemm.hip's fp8 branch.  128 x 128 tile, K tile 128 (A rows 128 B, W rows 64 B of codes + 4 scale
// bytes), 4 waves as 2 x 2 with 4 x 4 MFMA tiles each, register-staged with ONE LDS stage (the next TWO K tiles' global
// loads in flight under this tile's MFMAs), 16-byte chunks XOR-swizzled by row (A: chunk ^ (row & 7) of 8; W:
// chunk ^ ((row >> 2) & 3) of 4, so 16 rows' reads of one chunk column cover all 64 banks).  1-D grid in
// the XCD-grouped order of gemm.hip: every m-tile of an n-tile runs back to back on one XCD and reuses the weight
// tile from its L2.  No workspace, no cross-workgroup hand-off, no host sync: capturable.  Rows past M and columns
// past N load zeros and are never stored.
//
// Addresses are 64-bit (plain global loads), so no operand has a 2^31-byte limit and nothing is run as row blocks;
// only a grid past 2^31 - 1 workgroups is refused.
// Requires K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0), lda % 16 == 0, lda >= K.
#include "common.h"
#include "launchers.h"

namespace lwc {
namespace mxa8 {

typedef int v8i32 __attribute__((ext_vector_type(8)));

constexpr int kTM = 128, kTN = 128;
constexpr int kABytes = kTM * 128;  // A tile: 128 rows x 128 e4m3
constexpr int kWBytes = kTN * 64;   // W tile: 128 rows x 128 e2m1

struct Params {
  const uint8_t* A;      // [M, lda] e4m3
  const uint8_t* Q;      // [N, K / 2]
  const uint8_t* S;      // [N, K / 32]
  const float* a_scale;  // [M]
  bf16_t* C;             // [M, ldc]
  int M, N, K, lda, ldc;
  int m_tiles, n_tiles;
};

LWC_DEVICE float silu(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

template <bool SWIGLU>
__global__ void __launch_bounds__(256, 2) gemm_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) uint8_t sA[kABytes];
  __shared__ __attribute__((aligned(16))) uint8_t sW[kWBytes];
  __shared__ __attribute__((aligned(16))) uint32_t sS[kTN];

  // XCD-grouped tile order (gemm.hip): workgroup ids are dealt round-robin to the 8 XCDs; XCD x walks the
  // n-tiles n = x (mod 8) with all m-tiles of an n-tile consecutive
  const int id = blockIdx.x, xcd = id & 7, local = id >> 3;
  const int ntile = (local / p.m_tiles) * 8 + xcd;
  const int mtile = local % p.m_tiles;
  if (ntile >= p.n_tiles) return;  // uniform
  const int m0 = mtile * kTM, n0 = ntile * kTN;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const int KT = p.K / 128;
  const int qrow = p.K / 2, srow = p.K / 32;  // bytes per row of Q / S

  // staging: A 1024 chunks (4 per thread), W 512 chunks (2 per thread), scales one dword per W row (threads
  // 0..127); rows past M / N stage zeros (codes 0 under any scale add nothing)
  const uint8_t* arow[4];
  const uint8_t* wrow[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
    arow[i] = m0 + row < p.M ? p.A + (size_t)(m0 + row) * p.lda + ch * 16 : nullptr;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i, row = c >> 2, ch = c & 3;
    wrow[i] = n0 + row < p.N ? p.Q + (size_t)(n0 + row) * qrow + ch * 16 : nullptr;
  }
  const uint8_t* srowp = tid < kTN && n0 + tid < p.N ? p.S + (size_t)(n0 + tid) * srow : nullptr;

  // two register sets: the loads of K tiles kt + 1 and kt + 2 are in flight under tile kt's MFMAs (with one set a
  // workgroup waits a whole memory round trip per K tile: ~1.1 us per tile measured where few workgroups share a CU)
  struct Stage {
    uint4v a[4], w[2];
    uint32_t s;
  };
  Stage st0, st1;
  auto gload = [&](Stage& r, int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      r.a[i] = arow[i] ? *reinterpret_cast<const uint4v*>(arow[i] + (size_t)kt * 128) : uint4v{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 2; ++i)
      r.w[i] = wrow[i] ? *reinterpret_cast<const uint4v*>(wrow[i] + (size_t)kt * 64) : uint4v{0, 0, 0, 0};
    r.s = srowp ? *reinterpret_cast<const uint32_t*>(srowp + (size_t)kt * 4) : 0u;
  };
  auto lstore = [&](const Stage& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4v*>(sA + row * 128 + ((ch ^ (row & 7)) << 4)) = r.a[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, row = c >> 2, ch = c & 3;
      *reinterpret_cast<uint4v*>(sW + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4)) = r.w[i];
    }
    if (tid < kTN) sS[tid] = r.s;
  };

  float4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};

  auto compute = [&]() {
    // W fragments: lane (r16, g) = row's MX block g (16 bytes of codes) and that block's scale byte
    v8i32 bw[4];  // (the builtin's operand type; the e2m1 form reads VGPRs 0-3 only)
    int bs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rb = wn * 64 + j * 16 + r16;
      const uint4v b = *reinterpret_cast<const uint4v*>(sW + rb * 64 + ((g ^ ((rb >> 2) & 3)) << 4));
      bw[j] = v8i32{(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
      bs[j] = (int)(sS[rb] >> (8 * g));  // byte 0 = block g's scale (op_sel 0 reads byte 0)
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // A fragment: the row's 16-byte chunks g (k = 16 g ..) and 4 + g (k = 64 + 16 g ..)
      const int ra_ = wm * 64 + i * 16 + r16;
      const uint4v a0 = *reinterpret_cast<const uint4v*>(sA + ra_ * 128 + ((g ^ (ra_ & 7)) << 4));
      const uint4v a1 = *reinterpret_cast<const uint4v*>(sA + ra_ * 128 + (((4 + g) ^ (ra_ & 7)) << 4));
      const v8i32 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bw[j], acc[i][j], /*cbsz: e4m3*/ 0,
                                                                     /*blgp: e2m1*/ 4, 0, 127, 0, bs[j]);
    }
  };
  // one K tile: the staged registers into LDS (after everyone has read the previous tile), the set refilled
  // from two tiles ahead, then the tile's MFMAs
  auto step = [&](Stage& r, int kt) {
    __syncthreads();
    lstore(r);
    __syncthreads();
    if (kt + 2 < KT) gload(r, kt + 2);
    compute();
  };

  gload(st0, 0);
  if (KT > 1) gload(st1, 1);
  for (int kt = 0; kt < KT; kt += 2) {
    step(st0, kt);
    if (kt + 1 < KT) step(st1, kt + 1);
  }

  // ---- epilogue: row scale, (SwiGLU,) bf16 store (lane reg r = C[row 4 g + r][col r16] of each 16 x 16) ----
  const int nw0 = n0 + wn * 64;  // the wave's first W row: 64 rows = one gate block + its up block (SwiGLU)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm * 64 + i * 16 + 4 * g + r;
      if (row >= p.M) continue;
      const float as = p.a_scale[row];
      bf16_t* crow = p.C + (size_t)row * p.ldc;
      if constexpr (SWIGLU) {
        if (nw0 < p.N) {  // N % 64 == 0: the wave's 64 W rows are all inside or all outside
#pragma unroll
          for (int j = 0; j < 2; ++j)
            crow[nw0 / 2 + j * 16 + r16] = f2bf(silu(acc[i][j][r] * as) * (acc[i][j + 2][r] * as));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = nw0 + j * 16 + r16;
          if (col < p.N) crow[col] = f2bf(acc[i][j][r] * as);  // N % 16 == 0: a 16-column tile is in or out
        }
      }
    }
}

}  // namespace mxa8
}  // namespace lwc

// C [M, N] = (Aq . W^T) * a_scale[row] (epi 0), or silu(.) * (.) over a 32-row gate/up interleaved W (epi 2,
// C [M, N / 2]); Aq e4m3, W in MXFP4.  -1: shape not taken.
extern "C" int lwc_gemm_mxfp4_a8(const void* A, const float* a_scale, const void* Q, const void* S, void* C, int M,
                                 int N, int K, int lda, int ldc, int epi, hipStream_t s) {
  using namespace lwc::mxa8;
  if (epi != 0 && epi != 2) return -1;
  const int NC = epi == 2 ? N / 2 : N;
  if (M < 0 || N < 0 || K <= 0 || K % 128 != 0 || N % (epi == 2 ? 64 : 16) != 0 || lda % 16 != 0 || lda < K ||
      ldc < NC)
    return -1;
  if (M == 0 || N == 0) return 0;
  const int m_tiles = (M + kTM - 1) / kTM, n_tiles = (N + kTN - 1) / kTN;
  const long long grid = (long long)((n_tiles + 7) / 8) * m_tiles * 8;
  if (grid >= (1LL << 31)) return -1;
  Params p{(const uint8_t*)A, (const uint8_t*)Q, (const uint8_t*)S, a_scale, (lwc::bf16_t*)C, M, N, K, lda, ldc,
           m_tiles, n_tiles};
  if (epi == 2)
    gemm_kernel<true><<<dim3((unsigned)grid), 256, 0, s>>>(p);
  else
    gemm_kernel<false><<<dim3((unsigned)grid), 256, 0, s>>>(p);
  return (int)hipGetLastError();
}
