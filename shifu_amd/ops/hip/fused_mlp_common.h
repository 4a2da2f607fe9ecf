// fused_mlp_common.h — device helpers shared by the LDS-resident MLP kernels
// (fused_mlp.hip: scoring, fused_mlp_grad.hip: forward+loss+backward,
// eval_hist.hip: forward+loss+score histogram).  Include after torch/extension.h.
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


// ---- the packed forward image of fused_mlp.py::pack_mlp ----
struct MlpLayer {
  int w_off;   // byte offset of the fragment-ordered bf16 [Npad, Kpad] image
  int b_off;   // byte offset of the fp32 bias[Npad]
  int nt;      // Npad / 16
  int ks;      // Kpad / 32
  int act;
};

struct MlpTable {
  int n_layers;
  int blob_bytes;    // multiple of 16
  int act_bytes;     // bytes of ONE per-wave activation buffer (two per wave)
  MlpLayer l[FMLP_MAX_LAYERS];
};

// Epilogue of one 16-feature tile: + bias, activation, then either the fp32
// score store (head) or the bf16 hand-off to the next layer's B fragments.
FMLP_DEVINL void fmlp_epilogue(f32x4 acc, const MlpLayer& L, int nt, bool last,
                               const unsigned char* smem, unsigned char* dst,
                               float* __restrict__ out, long row, long B,
                               int m, int kg) {
  const int n0 = nt * 16 + kg * 4;            // first of this lane's 4 features
  const float4 bias = *(const float4*)(smem + L.b_off + n0 * 4);
  if (last) {
    // head: feature 0 of every row sits in r=0 of lanes 0..15; logit stays fp32
    if (kg == 0 && row < B)
      out[row] = 1.0f / (1.0f + __expf(-(acc[0] + bias.x)));
    return;
  }
  const float v0 = fmlp_act(acc[0] + bias.x, L.act);
  const float v1 = fmlp_act(acc[1] + bias.y, L.act);
  const float v2 = fmlp_act(acc[2] + bias.z, L.act);
  const float v3 = fmlp_act(acc[3] + bias.w, L.act);
  uint2 p;
  p.x = fmlp_pack2(v0, v1);
  p.y = fmlp_pack2(v2, v3);
  // feature n is reduction index k of the next layer: fragment slot
  // (k/32, lane' = (k%32/8)*16 + m), element k%8 (0 or 4 here)
  const int off = (((n0 >> 5) * 64 + ((n0 & 31) >> 3) * 16 + m) << 4) + ((n0 & 7) << 1);
  *(uint2*)(dst + off) = p;
}

// Zero the 16-feature tile `nt` of the next layer's input (Kpad = ceil32(N)
// can exceed Npad = ceil16(N); stale LDS there could hold NaN bit patterns).
FMLP_DEVINL void fmlp_zero_tile(unsigned char* dst, int nt, int m, int kg) {
  const int n0 = nt * 16 + kg * 4;
  const int off = (((n0 >> 5) * 64 + ((n0 & 31) >> 3) * 16 + m) << 4) + ((n0 & 7) << 1);
  *(uint2*)(dst + off) = make_uint2(0u, 0u);
}

// layer_table  CPU int32 [L, 4]: byte offset, N, K, activation id (pack_mlp)
// Re-derives every offset of a packed blob of `blob_bytes` bytes for K0-wide
// rows; a table that does not describe the blob exactly is an error.
inline MlpTable fmlp_parse_table(const at::Tensor& layer_table, int K0,
                                 long blob_bytes, int max_ks0) {
  TORCH_CHECK(!layer_table.is_cuda() && layer_table.scalar_type() == at::kInt &&
              layer_table.dim() == 2 && layer_table.size(1) == 4 &&
              layer_table.is_contiguous(),
              "layer_table must be a CPU int32 [L, 4] tensor");
  const long L = layer_table.size(0);
  TORCH_CHECK(L >= 1 && L <= FMLP_MAX_LAYERS, "fused MLP supports 1..",
              FMLP_MAX_LAYERS, " layers, got ", L);
  const int* tab = layer_table.data_ptr<int>();
  MlpTable t{};
  t.n_layers = (int)L;
  t.blob_bytes = (int)blob_bytes;
  int prev = K0, max_kpad = 32;
  long expect_off = 0;
  for (long i = 0; i < L; ++i) {
    const int off = tab[i * 4 + 0], N = tab[i * 4 + 1], K = tab[i * 4 + 2],
              act = tab[i * 4 + 3];
    TORCH_CHECK(N >= 1 && K >= 1 && K == prev, "layer ", i, ": K=", K,
                " does not chain from ", prev);
    TORCH_CHECK(act >= FACT_NONE && act <= FACT_LEAKY, "layer ", i, ": bad act ", act);
    const int npad = ceil_to(N, 16), kpad = ceil_to(K, 32);
    const long wbytes = (long)npad * kpad * 2, bbytes = (long)npad * 4;
    TORCH_CHECK(off == expect_off && off + wbytes + bbytes <= blob_bytes,
                "layer ", i, ": offset ", off, " outside the packed blob");
    t.l[i] = MlpLayer{off, (int)(off + wbytes), npad / 16, kpad / 32, act};
    expect_off = off + wbytes + bbytes;
    if (i > 0 && kpad > max_kpad) max_kpad = kpad;
    prev = N;
  }
  TORCH_CHECK(expect_off == blob_bytes, "packed blob has trailing bytes");
  TORCH_CHECK(prev == 1, "fused MLP needs a 1-unit head, got ", prev);
  TORCH_CHECK(t.l[0].ks <= max_ks0, "input width ", K0, " > ", max_ks0 * 32);
  t.act_bytes = 32 * max_kpad;           // 16 rows x Kpad bf16
  return t;
}

}  // namespace
