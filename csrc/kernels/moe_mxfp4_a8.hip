// W4A8 MoE expert projections over MXFP4 weights: moe_gemm_mxfp4_a8, the grouped form of gemm_mxfp4_a8
// (mxfp4_a8.hip), for the steps past the weight stream's row limit (moe_mxfp4.hip).  e4m3 token rows x the packed
// e2m1 expert stack on the block-scaled MFMA, the stack read as it is stored: no dequantisation, no scratch.
//
//   C[r, n] = bf16( a_scale[src(r)] * sum_k e4m3(Aq[src(r), k]) * e2m1(Q[e, n, k]) * 2^(S[e, n, k / 32] - 127) )
//   for expert e and its rows r in [row_off[e], row_off[e + 1]); src(r) = a_rows[r] if a_rows is given, else r
//
//   Aq [a_nrows, K] e4m3 (row stride lda >= K bytes, rows 16-byte aligned), a_scale [a_nrows] f32: the TOKENS'
//   rows and scales, indexed through the gather as gemm.hip's fp8 branch does; Q [E, N, K / 2], S [E, N, K / 32]
//   (ops.Mxfp4Experts); row_off [E + 1] and the optional a_rows [rows] int32 on the device, read on the device: no
//   host sync, capturable; C bf16 [rows, N], or with the SwiGLU epilogue (W rows gate|up interleaved in blocks of
//   32) [rows, N / 2].
//
// Tile, K loop, fragments and epilogue are mxa8::gemm_kernel's (operand lane maps: that file's header): 128 x 128
// tile, one MFMA per 16 x 16 tile and 128 k, K tiles ascending into one accumulator, no split-K, two register
// stages and one LDS stage, the two XOR swizzles.  So a row's result depends on the row, its scale and its expert's
// weights alone: bit for bit gemm_mxfp4_a8 of those rows over W[e], wherever the row sits in its tile.
//
// Grouping is gemm.hip's: a workgroup owns an m-tile SLOT and finds its (expert, tile) from row_off; the host
// passes slots = ceil(rows / 128) + E (>= sum_e ceil(M_e / 128) for any split), a surplus slot returns before any
// weight load, an idle expert owns no slot.  The search is lane-parallel: each wave takes 64 experts per step (tile
// counts, a prefix sum by shuffles, one ballot) where a serial scan at E = 128 would put 128 dependent loads in front
// of the tile.  1-D grid in the XCD-grouped order with `slots` in place of m_tiles.  The a_rows gather is
// resolved once per staged row, before the K loop.  Rows of a tile past the segment's end stage zeros and are never
// stored (the next row is the next expert's); rows >= rows and columns >= N are never stored.  row_off is clamped
// to [0, rows]; a gathered row outside [0, a_nrows) reads nothing and stores zero.
//
// Addresses are 64-bit; only a grid past 2^31 - 1 workgroups is refused.
// Requires K % 128 == 0, N % 16 == 0 (SwiGLU: N % 64 == 0), lda % 16 == 0, lda >= K.
#include "common.h"
#include "launchers.h"

namespace lwc {
namespace moe_mxa8 {

typedef int v8i32 __attribute__((ext_vector_type(8)));

constexpr int kTM = 128, kTN = 128;
constexpr int kABytes = kTM * 128;  // A tile: 128 rows x 128 e4m3
constexpr int kWBytes = kTN * 64;   // W tile: 128 rows x 128 e2m1

struct Params {
  const uint8_t* A;      // [a_nrows, lda] e4m3
  const uint8_t* Q;      // [E, N, K / 2]
  const uint8_t* S;      // [E, N, K / 32]
  const float* a_scale;  // [a_nrows]
  bf16_t* C;             // [rows, ldc]
  const int* row_off;    // [E + 1]
  const int* a_rows;     // optional [rows]
  int E, rows;
  long long a_nrows;
  int N, K, lda, ldc;
  int slots, n_tiles;
};

LWC_DEVICE float silu(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

template <bool SWIGLU>
__global__ void __launch_bounds__(256, 2) moe_gemm_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) uint8_t sA[kABytes];
  __shared__ __attribute__((aligned(16))) uint8_t sW[kWBytes];
  __shared__ __attribute__((aligned(16))) uint32_t sS[kTN];

  // XCD-grouped order (gemm.hip): XCD x walks the n-tiles n = x (mod 8) with all m-slots of an n-tile consecutive
  const int id = blockIdx.x, xcd = id & 7, local = id >> 3;
  const int ntile = (local / p.slots) * 8 + xcd;
  int slot = local % p.slots;
  if (ntile >= p.n_tiles) return;  // uniform

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // ---- locate (expert, m-tile) of this slot: every wave runs the same search, 64 experts per step ----
  int e = -1, m_begin = 0, m_end = 0;
  for (int base = 0; base < p.E; base += 64) {
    const int ge = base + lane;
    int r0 = 0, r1 = 0;
    if (ge < p.E) {
      r0 = min(max(p.row_off[ge], 0), p.rows);
      r1 = min(max(p.row_off[ge + 1], 0), p.rows);
    }
    const int nt = r1 > r0 ? (r1 - r0 + kTM - 1) / kTM : 0;
    int incl = nt;  // inclusive prefix sum of the tile counts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    const int total = __shfl(incl, 63, 64);
    if (slot < total) {
      const unsigned long long hit = __ballot(incl > slot);
      const int l = __ffsll((long long)hit) - 1;  // the first expert whose tiles reach past the slot
      const int before = __shfl(incl - nt, l, 64);
      e = base + l;
      m_begin = __shfl(r0, l, 64) + (slot - before) * kTM;
      m_end = __shfl(r1, l, 64);
      break;
    }
    slot -= total;
  }
  if (e < 0) return;  // surplus slot (the same for every wave of the workgroup): nothing of the weights is read
  e = __builtin_amdgcn_readfirstlane(e);
  m_begin = __builtin_amdgcn_readfirstlane(m_begin);
  m_end = __builtin_amdgcn_readfirstlane(m_end);
  const int n0 = ntile * kTN;

  const int r16 = lane & 15, g = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const int KT = p.K / 128;
  const int qrow = p.K / 2, srow = p.K / 32;  // bytes per row of Q / S
  const uint8_t* Q = p.Q + (size_t)e * p.N * qrow;
  const uint8_t* S = p.S + (size_t)e * p.N * srow;

  // staging: A 1024 chunks (4 per thread), W 512 chunks (2 per thread), scales one dword per W row (threads
  // 0..127); rows past the segment / N stage zeros.  The gather is resolved here, once per staged row: an index load
  // per K tile would put a dependent round trip in front of every A load
  const uint8_t* arow[4];
  const uint8_t* wrow[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
    const int ar = m_begin + row;
    arow[i] = nullptr;
    if (ar < m_end) {
      const long long src = p.a_rows ? p.a_rows[ar] : ar;
      if (src >= 0 && src < p.a_nrows) arow[i] = p.A + (size_t)src * p.lda + ch * 16;
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i, row = c >> 2, ch = c & 3;
    wrow[i] = n0 + row < p.N ? Q + (size_t)(n0 + row) * qrow + ch * 16 : nullptr;
  }
  const uint8_t* srowp = tid < kTN && n0 + tid < p.N ? S + (size_t)(n0 + tid) * srow : nullptr;

  // two register sets: the loads of K tiles kt + 1 and kt + 2 are in flight under tile kt's MFMAs
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

  // ---- epilogue: the token's scale, (SwiGLU,) bf16 store (lane reg r = C[row 4 g + r][col r16] of each 16 x 16) ----
  const int nw0 = n0 + wn * 64;  // the wave's first W row: 64 rows = one gate block + its up block (SwiGLU)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m_begin + wm * 64 + i * 16 + 4 * g + r;
      if (row >= m_end) continue;
      const long long src = p.a_rows ? p.a_rows[row] : row;
      const float as = src >= 0 && src < p.a_nrows ? p.a_scale[src] : 0.f;
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

}  // namespace moe_mxa8
}  // namespace lwc

// C[r] = (Aq[src(r)] . W[e]^T) * a_scale[src(r)] (epi 0) or the SwiGLU of a 32-row gate/up interleaved W[e] (epi 2,
// C [rows, N / 2]) for every expert e and row r of its segment; src = a_rows[.] or the identity.  Aq has a_nrows
// rows of lda bytes.  -1: shape not taken (nothing was launched).
extern "C" int lwc_moe_gemm_mxfp4_a8(const void* A, const float* a_scale, const void* Q, const void* S, void* C,
                                     const int* row_off, const int* a_rows, int E, int rows, long long a_nrows, int N,
                                     int K, int lda, int ldc, int epi, hipStream_t s) {
  using namespace lwc::moe_mxa8;
  if (epi != 0 && epi != 2) return -1;
  const int NC = epi == 2 ? N / 2 : N;
  if (E <= 0 || rows < 0 || a_nrows < 0 || N < 0 || K <= 0 || K % 128 != 0 || N % (epi == 2 ? 64 : 16) != 0 ||
      lda % 16 != 0 || lda < K || ldc < NC)
    return -1;
  if (a_rows == nullptr && a_nrows < rows) return -1;
  if (rows == 0 || N == 0) return 0;
  const long long slots = ((long long)rows + kTM - 1) / kTM + E;
  const int n_tiles = (N + kTN - 1) / kTN;
  const long long grid = (long long)((n_tiles + 7) / 8) * slots * 8;
  if (grid >= (1LL << 31)) return -1;
  Params p{(const uint8_t*)A, (const uint8_t*)Q, (const uint8_t*)S, a_scale, (lwc::bf16_t*)C, row_off, a_rows, E,
           rows,              a_nrows,           N,                 K,       lda,             ldc,     (int)slots,
           n_tiles};
  if (epi == 2)
    moe_gemm_kernel<true><<<dim3((unsigned)grid), 256, 0, s>>>(p);
  else
    moe_gemm_kernel<false><<<dim3((unsigned)grid), 256, 0, s>>>(p);
  return (int)hipGetLastError();
}
