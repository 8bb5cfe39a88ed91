// gs_split_mfma.h -- fp32-equivalent contractions on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16).  Every fp32 operand is split into three bf16
// pieces, x = p0 + p1 + p2 + r, each piece the bf16 rounding of what the
// previous ones leave (the remainders are exact in fp32), so |r| <= 2^-27 |x|:
// x is carried to fp32's 24 bits.  A product a*b is summed as the piece
// products p_i q_j with i + j < 3 (six; the dropped ones are <= 2^-26 |ab|,
// under fp32's own rounding of a product), smallest first, into the fp32
// accumulator; each bf16 x bf16 product is exact in fp32.  An operand that is
// exact in bf16 needs three.  The technique is gs_render.hip's; that file
// keeps its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {
namespace smf {

constexpr int NSP = 3;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct bsplit {
  bf16x8 p[NSP];
};

__device__ inline f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// one v_cvt_pk_bf16_f32 rounds two operands (RNE)
__device__ inline uint32_t cvt_pk_bf16(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ inline float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ inline float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// eight values that are exact in bf16 (signs, small integers)
__device__ inline bf16x8 pack_exact(const float (&x)[8]) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = cvt_pk_bf16(x[2 * j], x[2 * j + 1]);
  return __builtin_bit_cast(bf16x8, w);
}
__device__ inline void split_bf16(const float (&x)[8], bsplit& s) {
  u32x4 w[NSP];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float a = x[2 * j], b = x[2 * j + 1];
#pragma unroll
    for (int i = 0; i < NSP; ++i) {
      const uint32_t u = cvt_pk_bf16(a, b);
      w[i][j] = u;
      if (i + 1 < NSP) {
        a = a - bf16_lo(u);
        b = b - bf16_hi(u);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NSP; ++i) s.p[i] = __builtin_bit_cast(bf16x8, w[i]);
}
// c += a * b over the split pieces (i + j < NSP), the smallest products first
__device__ inline f32x16 mfma_split(const bsplit& a, const bsplit& b, f32x16 c) {
#pragma unroll
  for (int o = NSP - 1; o >= 0; --o)
#pragma unroll
    for (int i = 0; i <= o; ++i) c = mfma_bf16(a.p[i], b.p[o - i], c);
  return c;
}
// c += a * b for an operand a (or b) that is exact in bf16, the other split
__device__ inline f32x16 mfma_exact_split(const bf16x8& a, const bsplit& b, f32x16 c) {
#pragma unroll
  for (int i = NSP - 1; i >= 0; --i) c = mfma_bf16(a, b.p[i], c);
  return c;
}
__device__ inline f32x16 mfma_split_exact(const bsplit& a, const bf16x8& b, f32x16 c) {
#pragma unroll
  for (int i = NSP - 1; i >= 0; --i) c = mfma_bf16(a.p[i], b, c);
  return c;
}

}  // namespace smf
}  // namespace gs
