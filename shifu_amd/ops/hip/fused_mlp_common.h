// fused_mlp_common.h — device helpers shared by the LDS-resident MLP kernels
// (fused_mlp.hip: scoring, fused_mlp_grad.hip: forward+loss+backward).
//
// Everything here is header-only and lives in an anonymous namespace, so each
// translation unit gets its own copy and the scoring kernels compile exactly
// as they did when these helpers were local to fused_mlp.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define FMLP_DEVINL __device__ __forceinline__

constexpr int FMLP_MAX_LAYERS = 8;

// activation ids shared with shifu_amd/ops/linear.py and shifu_ops.hip
enum { FACT_NONE = 0, FACT_SIGMOID = 1, FACT_TANH = 2, FACT_RELU = 3, FACT_LEAKY = 4 };
constexpr float FMLP_LEAKY_SLOPE = 0.01f;

FMLP_DEVINL float fmlp_act(float z, int act) {
  switch (act) {
    case FACT_SIGMOID: return 1.0f / (1.0f + __expf(-z));
    case FACT_TANH:    return tanhf(z);
    case FACT_RELU:    return z > 0.0f ? z : 0.0f;
    case FACT_LEAKY:   return z > 0.0f ? z : FMLP_LEAKY_SLOPE * z;
    default:           return z;
  }
}

// fp32 -> bf16 bits, round-to-nearest-even (NaN stays a quiet NaN)
FMLP_DEVINL unsigned fmlp_bf16_bits(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

FMLP_DEVINL unsigned fmlp_pack2(float lo, float hi) {
  return fmlp_bf16_bits(lo) | (fmlp_bf16_bits(hi) << 16);
}

// LDS traffic between layers is wave-private and the LDS serves one wave's
// instructions in issue order; this only stops the compiler from moving a
// fragment read above the stores (from other lanes) that produce it.
FMLP_DEVINL void fmlp_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Byte offset, inside a fragment-ordered 16-row operand buffer, of the 4
// consecutive reduction indices k0..k0+3 (k0 % 4 == 0) of row m: fragment
// slot (k/32, lane' = (k%32/8)*16 + m), element k%8 (0 or 4).
FMLP_DEVINL int fmlp_frag_off(int k0, int m) {
  return (((k0 >> 5) * 64 + ((k0 & 31) >> 3) * 16 + m) << 4) + ((k0 & 7) << 1);
}

inline int ceil_to(int v, int a) { return (v + a - 1) / a * a; }

}  // namespace
