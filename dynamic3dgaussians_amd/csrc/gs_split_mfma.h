// gs_split_mfma.h -- fp32-equivalent contractions on the bf16 / fp16 matrix
// cores (16x the fp32 MFMA rate), for the blend kernels (gs_render.hip) and
// the feature decoder (gs_feature_decoder.hip).
//
// bf16: every fp32 operand is split into NSP bf16 pieces, x = p0 + p1 + p2 + r,
// each piece the bf16 rounding of what the previous ones leave (x - p0 and
// x - p0 - p1 are exact in fp32), so |r| <= 2^-27 |x| for three pieces: x is
// carried to fp32's 24 bits.  A product a*b is summed as the piece products
// p_i q_j with i + j < NSP (NSP = 3: 6 products; the dropped ones are
// <= 2^-26 |ab|, under fp32's own 2^-24 rounding of a product), smallest
// first, into the fp32 accumulator.  Each bf16 x bf16 product is exact in
// fp32.  An operand that is exact in bf16 (signs, small integers) needs three.
// (Round 2 used a two-piece split: 3 products, ~2^-17 per product; DESIGN.md
// section 4.)
//
// fp16 (further down): two pieces for operands whose range is known.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {
namespace smf {

constexpr int NSP = 3;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct bsplit {
  bf16x8 p[NSP];
};

__device__ inline float4_t mfma_bf16(const bf16x8& a, const bf16x8& b, float4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ inline f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// Two operands at a time: one v_cvt_pk_bf16_f32 rounds both (RNE, as the
// scalar conversion), and each piece is read back to fp32 from the packed
// word by a shift (low half) or a mask (high half) -- 5.5 vector
// instructions per operand for 3 pieces instead of the 7.5 the compiler
// emits for the per-element form (a one-element conversion plus a shift per
// piece and operand).  Bit-identical pieces.
__device__ inline uint32_t cvt_pk_bf16(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ inline float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ inline float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
// How a remainder is taken is the caller's choice (ONE_SUB), the value is the
// same.  The blend kernels take each with a single v_sub_f32 (inline asm, so
// the compiler does not pair them into v_pk_add_f32, which issues beside the
// matrix instructions at a higher price and cost registers: F = 32 forward
// 126 VGPRs and no scratch vs 128 and 24 B).  27-camera step
// (profiles/r03q_ab_split.log): render_fwd 3.21-3.30 vs 3.44-3.48 ms
// per-element, render_bwd 5.02-5.06 vs 5.24-5.35; the v_pk_add_f32 pairing
// 3.37-3.40 / 5.04-5.11.  The feature decoder leaves the subtraction to the
// compiler, which is free to pair it there.
__device__ inline float split_sub(float a, float h) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(h));
  return r;
}
template <bool ONE_SUB = false>
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
        a = ONE_SUB ? split_sub(a, bf16_lo(u)) : a - bf16_lo(u);
        b = ONE_SUB ? split_sub(b, bf16_hi(u)) : b - bf16_hi(u);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NSP; ++i) s.p[i] = __builtin_bit_cast(bf16x8, w[i]);
}
// eight values that are exact in bf16 (signs, small integers)
__device__ inline bf16x8 pack_exact(const float (&x)[8]) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = cvt_pk_bf16(x[2 * j], x[2 * j + 1]);
  return __builtin_bit_cast(bf16x8, w);
}
// c += a * b over the split pieces (i + j < NSP), the smallest products first
template <class Acc>
__device__ inline Acc mfma_split(const bsplit& a, const bsplit& b, Acc c) {
#pragma unroll
  for (int o = NSP - 1; o >= 0; --o)
#pragma unroll
    for (int i = 0; i <= o; ++i) c = mfma_bf16(a.p[i], b.p[o - i], c);
  return c;
}
// c += a * x with x split here, one piece at a time (fewer live registers
// than mfma_split: x's pieces never coexist); largest products first.  The
// blend backward's: its remainders are split_sub's.
template <class Acc>
__device__ inline Acc mfma_split_x(const bsplit& a, const float (&x)[8], Acc c) {
  float r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = x[e];
#pragma unroll
  for (int j = 0; j < NSP; ++j) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t u = cvt_pk_bf16(r[2 * e], r[2 * e + 1]);
      w[e] = u;
      if (j + 1 < NSP) {
        r[2 * e] = split_sub(r[2 * e], bf16_lo(u));
        r[2 * e + 1] = split_sub(r[2 * e + 1], bf16_hi(u));
      }
    }
    const bf16x8 b = __builtin_bit_cast(bf16x8, w);
#pragma unroll
    for (int i = 0; i + j < NSP; ++i) c = mfma_bf16(a.p[i], b, c);
  }
  return c;
}
// c += a * b for an operand a (or b) that is exact in bf16, the other split
template <class Acc>
__device__ inline Acc mfma_exact_split(const bf16x8& a, const bsplit& b, Acc c) {
#pragma unroll
  for (int i = NSP - 1; i >= 0; --i) c = mfma_bf16(a, b.p[i], c);
  return c;
}
template <class Acc>
__device__ inline Acc mfma_split_exact(const bsplit& a, const bf16x8& b, Acc c) {
#pragma unroll
  for (int i = NSP - 1; i >= 0; --i) c = mfma_bf16(a.p[i], b, c);
  return c;
}

// ------------------------------------------------------------------ fp16 split products
// The same contraction on the fp16 matrix cores (the bf16 rate) for operands
// whose range is known: fp16 keeps 11 significant bits, so TWO pieces carry
// an operand to 22-24 bits (x = h0 + h1 + r, h0 the fp16 rounding of x, h1
// of x - h0; |r| <= 2^-24 |x| while x - h0 is a normal fp16) and a product
// a*b is summed as h0 g0 + h0 g1 + h1 g0 (3 matrix instructions instead of
// the bf16 split's 6; the dropped h1 g1 and remainders are ~3 * 2^-24 |ab|,
// fp32's own rounding of a product), each piece product exact in fp32.
// Range: an operand is scaled by a power of two into [2^-3, 2^16) wherever
// its size allows (exact, undone on the fp32 sums), so h0 stays normal and
// h1 exact; fp16 subnormals pass the conversions and the matrix inputs
// unflushed (MODE.denorm, hipcc's default), so smaller values lose relative
// precision only below 2^-24 of the operand's scale in absolute terms.
// Per 8 values: 4 v_cvt_pk_f16_f32 + 8 v_fma_mix_f32 (the remainder x - h0
// read straight from the packed half, negated, in one instruction) + 4
// v_cvt_pk_f16_f32 = 2 vector instructions per value (the 3-piece bf16
// split: 5.5).
constexpr int NSH = 2;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
struct hsplit {
  f16x8 p[NSH];
};
__device__ inline float4_t mfma_f16(const f16x8& a, const f16x8& b, float4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ inline f32x16 mfma_f16(const f16x8& a, const f16x8& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ inline uint32_t cvt_pk_f16(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, f16x2));
}
// a - (the fp16 in the low / high half of u), exact, one v_fma_mix_f32
__device__ inline float f16_rem_lo(float a, uint32_t u) {
  float r;
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(u), "v"(a));
  return r;
}
__device__ inline float f16_rem_hi(float a, uint32_t u) {
  float r;
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(u), "v"(a));
  return r;
}
__device__ inline void split_f16(const float (&x)[8], hsplit& s) {
  u32x4 w0, w1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t u = cvt_pk_f16(x[2 * j], x[2 * j + 1]);
    w0[j] = u;
    w1[j] = cvt_pk_f16(f16_rem_lo(x[2 * j], u), f16_rem_hi(x[2 * j + 1], u));
  }
  s.p[0] = __builtin_bit_cast(f16x8, w0);
  s.p[1] = __builtin_bit_cast(f16x8, w1);
}
// c += a * b over the pieces (h1 g0 and h0 g1 first, then h0 g0)
__device__ inline float4_t mfma_hsplit(const hsplit& a, const hsplit& b, float4_t c) {
  c = mfma_f16(a.p[1], b.p[0], c);
  c = mfma_f16(a.p[0], b.p[1], c);
  return mfma_f16(a.p[0], b.p[0], c);
}
// c += a * x with x split here (its two pieces made one after the other):
// h1 g0 first, then h0 g1, h0 g0
__device__ inline f32x16 mfma_hsplit_x(const hsplit& a, const float (&x)[8], f32x16 c) {
  u32x4 w0, w1;
#pragma unroll
  for (int j = 0; j < 4; ++j) w0[j] = cvt_pk_f16(x[2 * j], x[2 * j + 1]);
  const f16x8 b0 = __builtin_bit_cast(f16x8, w0);
  c = mfma_f16(a.p[1], b0, c);
#pragma unroll
  for (int j = 0; j < 4; ++j) w1[j] = cvt_pk_f16(f16_rem_lo(x[2 * j], w0[j]), f16_rem_hi(x[2 * j + 1], w0[j]));
  c = mfma_f16(a.p[0], __builtin_bit_cast(f16x8, w1), c);
  return mfma_f16(a.p[0], b0, c);
}

}  // namespace smf
}  // namespace gs
