// The arithmetic of the f16f6 operand pass, shared by md_wino_prep2_f6_kernel (wino_prep2.hip) and md_block_pass_kernel
// (block_pass.hip): both must write the same bits, so the activation, the equaliser multiply and the F(2,3) input transform are
// compiled from ONE source expression each.  The multiply of the equaliser and the add / subtract of the transform are kept out
// of FMA contraction explicitly: in the two-phase pass an LDS round trip separates them from their neighbours, in the one-pass
// kernel nothing does.
#pragma once
#include "md_common.h"

// folded GroupNorm affine a x + c, then SiLU (layers.py:676-682)
__device__ __forceinline__ float md_prep_act(float t, float a, float c, int silu) {
  t = t * a + c;
  if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t * -1.4426950408889634f));
  return t;
}

// the static power-of-two equaliser of the f16f8 / f16f6 operand
__device__ __forceinline__ float md_prep_eq(float y, float s) {
#pragma clang fp contract(off)
  return y * s;
}

// frequency f of the F(2,3) input transform along w: d_k = the activated input at x - 1 + k of the pair at (x, x + 1)
__device__ __forceinline__ float md_wino_bt(int f, float d0, float d1, float d2, float d3) {
#pragma clang fp contract(off)
  return f == 0 ? d0 - d2 : f == 1 ? d1 + d2 : f == 2 ? d2 - d1 : d1 - d3;
}
