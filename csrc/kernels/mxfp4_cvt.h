// Device helpers shared by the MXFP4 weight-stream kernels (mxfp4.hip, moe_mxfp4.hip): the e8m0 scale operand, the
// 8-code convert and the bf16 MFMA step.  The grouped kernel's contract is to compute bit for bit what the dense
// one does, so both take these from one place.
#pragma once
#include "common.h"

namespace lwc {
namespace mxfp4 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int KS = 8;  // waves per workgroup (split-K)

// the e8m0 byte as the convert's f32 scale operand: 2^(s - 127) is the float with exponent field s.  Byte 0 makes
// this the float 0.0, and the convert still scales by 2^-127 (it takes the operand's exponent field as the e8m0
// byte), keeps bf16 subnormal results and gives inf where byte 253 / 254 overflow: the host function on all
// 16 x 255 pairs, pinned on an MI355X by tests/test_mxw_probes_gpu.py
LWC_DEVICE float e8m0(uint32_t s) { return __uint_as_float(s << 23); }

// 8 codes (one dword: k ascending from the low nibble of byte 0) -> 8 bf16 in k order, times the block scale
LWC_DEVICE uint4v cvt8(uint32_t q, float scale) {
  uint4v r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3));
  return r;
}

LWC_DEVICE float4v mfma(const uint4v& a, const uint4v& b, const float4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                 0, 0);
}

}  // namespace mxfp4
}  // namespace lwc
