// fused_mlp.hip — whole-network MLP scoring in ONE kernel (gfx950 / MI355X).
//
// Scoring a small exported ShifuMLP (e.g. 200 -> [50, 50] -> 1, ~25 KB of
// weights) through the training kernels costs L+3 launches and a memory
// round trip per intermediate.  Here the complete packed weight set lives in
// LDS for the lifetime of a block and rows stream through MFMA: fp32 input in,
// fp32 score out, nothing else touches memory.
//
// Packed image (built once by shifu_amd/ops/fused_mlp.py::pack_mlp, copied
// verbatim into LDS): per layer, bf16 W zero-padded to [Npad=ceil16(N),
// Kpad=ceil32(K)] stored in MFMA FRAGMENT ORDER, then fp32 bias[Npad].
// Fragment order: for n-tile nt, k-step ks the 64 lanes' 16-byte operand
// fragments are contiguous,
//     byte = ((nt * KS + ks) * 64 + lane) * 16,  lane = (k%32/8)*16 + n%16
// so the operand read is one ds_read_b128 per lane over a contiguous 1 KiB:
// each of the instruction's four 16-lane groups ({0-3,12-15,20-27}, ...)
// covers 16 distinct 16-byte slots = all 64 banks once -> conflict-free with
// no row padding and no swizzle arithmetic.
//
// The product is computed transposed, D[n][m] = sum_k W[n][k] * X[m][k]
// (W is the MFMA A operand, the activations the B operand; both have the same
// per-lane fragment shape).  D then puts 4 CONSECUTIVE features of one row in
// each lane (col = lane&15 = row m, row = (lane>>4)*4 + r = feature n), so the
// bias/activation epilogue rounds them to bf16 and hands them to the next
// layer with ONE 8-byte LDS store per lane instead of four 2-byte scatters.
// Activations ping-pong between two per-wave LDS buffers, also in fragment
// order; a wave owns its 16-row tile end to end, so no block barrier is
// needed after the initial weight copy.
//
// No atomics, no grid sync, no inline assembly, plain vector stores only.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define FMLP_DEVINL __device__ __forceinline__

constexpr int FMLP_MAX_LAYERS = 8;
constexpr int FMLP_MAX_WAVES = 8;           // 512 threads
constexpr int FMLP_LDS_LIMIT = 131072;      // same ceiling as V4_LDS_BYTES
constexpr int FMLP_MAX_KS0 = 32;            // layer-0 fragments live in VGPRs

// activation ids shared with shifu_amd/ops/linear.py and shifu_ops.hip
enum { FACT_NONE = 0, FACT_SIGMOID = 1, FACT_TANH = 2, FACT_RELU = 3, FACT_LEAKY = 4 };
constexpr float FMLP_LEAKY_SLOPE = 0.01f;

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

// KS0: compile-time bound on the layer-0 k-steps (its fragments stay in VGPRs)
// VEC : rows are 16-byte aligned (K0 % 4 == 0 and aligned base) -> float4 loads
template <int KS0, bool VEC>
__global__ __launch_bounds__(FMLP_MAX_WAVES * 64)
void mlp_score_fused_kernel(const float* __restrict__ x,
                            const uint4* __restrict__ blob,
                            float* __restrict__ out, long B, int K0,
                            MlpTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  for (int i = tid; i < (t.blob_bytes >> 4); i += blockDim.x)
    ((uint4*)smem)[i] = blob[i];
  __syncthreads();

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int nwaves = blockDim.x >> 6;
  const int m = lane & 15;        // row within the tile
  const int kg = lane >> 4;       // k-group (operands) / feature group (D)
  unsigned char* abuf[2];
  abuf[0] = smem + t.blob_bytes + (wave * 2) * t.act_bytes;
  abuf[1] = abuf[0] + t.act_bytes;

  const long n_tiles = (B + 15) >> 4;
  const MlpLayer L0 = t.l[0];
  const int nl = t.n_layers;

  for (long tile = (long)blockIdx.x * nwaves + wave; tile < n_tiles;
       tile += (long)gridDim.x * nwaves) {
    const long row = tile * 16 + m;
    const bool row_ok = row < B;
    const float* xr = x + row * (long)K0;

    // ---- layer-0 B fragments: fp32 global -> bf16 (RNE) in registers ----
    bf16x8 xf[KS0];
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) {
      const int c = ks * 32 + kg * 8;
      float v[8];
      if (VEC) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (row_ok && c < K0) a = *(const float4*)(xr + c);
        if (row_ok && c + 4 < K0) b = *(const float4*)(xr + c + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (row_ok && c + j < K0) ? xr[c + j] : 0.0f;
      }
      uint4 p;
      p.x = fmlp_pack2(v[0], v[1]);
      p.y = fmlp_pack2(v[2], v[3]);
      p.z = fmlp_pack2(v[4], v[5]);
      p.w = fmlp_pack2(v[6], v[7]);
      xf[ks] = *(bf16x8*)&p;
    }

    // ---- layer 0 ----
    {
      const bool last = (nl == 1);
      const unsigned char* w = smem + L0.w_off + lane * 16;
      for (int nt = 0; nt < L0.nt; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS0; ++ks) {
          if (ks < L0.ks) {
            const bf16x8 a = *(const bf16x8*)(w + ((nt * L0.ks + ks) << 10));
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc, 0, 0, 0);
          }
        }
        fmlp_epilogue(acc, L0, nt, last, smem, abuf[0], out, row, B, m, kg);
      }
      if (!last && (L0.nt & 1)) fmlp_zero_tile(abuf[0], L0.nt, m, kg);
    }

    // ---- layers 1 .. nl-1: both operands from LDS ----
    for (int li = 1; li < nl; ++li) {
      fmlp_wave_lds_fence();
      const MlpLayer L = t.l[li];
      const bool last = (li == nl - 1);
      const unsigned char* src = abuf[(li - 1) & 1] + lane * 16;
      unsigned char* dst = abuf[li & 1];
      const unsigned char* w = smem + L.w_off + lane * 16;
      for (int nt = 0; nt < L.nt; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int ks = 0; ks < L.ks; ++ks) {
          const bf16x8 a = *(const bf16x8*)(w + ((nt * L.ks + ks) << 10));
          const bf16x8 b = *(const bf16x8*)(src + (ks << 10));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
        fmlp_epilogue(acc, L, nt, last, smem, dst, out, row, B, m, kg);
      }
      if (!last && (L.nt & 1)) fmlp_zero_tile(dst, L.nt, m, kg);
    }
    // the next tile's layer 0 stores to abuf[0]; order them after this
    // tile's last reads of it
    fmlp_wave_lds_fence();
  }
}

// ---------------------------------------------------------------------------
// Bagged ensembles: one group of member networks scored per launch.
//
// The LDS image is the members' packed images back to back (each exactly the
// single-model layout above).  The layer-0 input fragments of a 16-row tile
// are loaded and converted once and every member consumes them before the
// next tile is touched, so M members cost one read of the rows and one
// launch.  Each member's score is accumulated, in member order, into one fp32
// register per lane; the sum starts from `carry` (the previous group's raw
// partial sum, or 0) and is scaled once by the final group, so the result is
// bitwise independent of how the members were split into groups.
constexpr int FENS_MAX_MEMBERS = 8;         // per group
constexpr int FENS_MAX_LAYERS = 32;         // per group, heads included
constexpr int FENS_MAX_TOTAL = 64;          // members over all groups
constexpr int FENS_MAX_KS0 = 16;            // fragments stay live over all members

struct EnsTable {
  int n_members;
  int blob_bytes;    // multiple of 16
  int act_bytes;     // ONE per-wave activation buffer: widest hidden Kpad of ANY member
  int m_total;       // row stride of members_out
  int col0;          // first members_out column of this group
  int first[FENS_MAX_MEMBERS + 1];   // member mi owns l[first[mi] .. first[mi+1])
  MlpLayer l[FENS_MAX_LAYERS];
};

// Head tile of one member: fp32 logit of feature 0 (r=0 of lanes 0..15), then
// the sigmoid — the same expression fmlp_epilogue stores for a single model.
FMLP_DEVINL float fmlp_head_score(f32x4 acc, const MlpLayer& L,
                                  const unsigned char* smem, int kg) {
  const float4 bias = *(const float4*)(smem + L.b_off + kg * 16);
  return 1.0f / (1.0f + __expf(-(acc[0] + bias.x)));
}

// out and carry may alias (in place: each row is read and written by the same
// lane), so neither is __restrict__.
template <int KS0, bool VEC>
__global__ __launch_bounds__(FMLP_MAX_WAVES * 64)
void mlp_score_fused_ensemble_kernel(const float* __restrict__ x,
                                     const uint4* __restrict__ blob,
                                     float* out, const float* carry,
                                     float* __restrict__ members_out,
                                     long B, int K0, float scale, EnsTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  for (int i = tid; i < (t.blob_bytes >> 4); i += blockDim.x)
    ((uint4*)smem)[i] = blob[i];
  __syncthreads();

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int nwaves = blockDim.x >> 6;
  const int m = lane & 15;
  const int kg = lane >> 4;
  unsigned char* const abuf0 = smem + t.blob_bytes + (wave * 2) * t.act_bytes;

  const long n_tiles = (B + 15) >> 4;
  const int nm = t.n_members;

  for (long tile = (long)blockIdx.x * nwaves + wave; tile < n_tiles;
       tile += (long)gridDim.x * nwaves) {
    const long row = tile * 16 + m;
    const bool row_ok = row < B;
    const bool writer = row_ok && kg == 0;
    const float* xr = x + row * (long)K0;

    // ---- layer-0 B fragments, once for all members ----
    bf16x8 xf[KS0];
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) {
      const int c = ks * 32 + kg * 8;
      float v[8];
      if (VEC) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (row_ok && c < K0) a = *(const float4*)(xr + c);
        if (row_ok && c + 4 < K0) b = *(const float4*)(xr + c + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (row_ok && c + j < K0) ? xr[c + j] : 0.0f;
      }
      uint4 p;
      p.x = fmlp_pack2(v[0], v[1]);
      p.y = fmlp_pack2(v[2], v[3]);
      p.z = fmlp_pack2(v[4], v[5]);
      p.w = fmlp_pack2(v[6], v[7]);
      xf[ks] = *(bf16x8*)&p;
    }

    float sum = 0.0f;
    if (carry != nullptr && writer) sum = carry[row];

    for (int mi = 0; mi < nm; ++mi) {
      // this member's layer 0 stores to abuf0, which the previous member's
      // later layers may still be reading
      if (mi) fmlp_wave_lds_fence();
      const int lbase = t.first[mi];
      const int nl = t.first[mi + 1] - lbase;
      float p = 0.0f;

      // ---- layer 0: B operand from the shared registers ----
      {
        const MlpLayer L0 = t.l[lbase];
        const unsigned char* w = smem + L0.w_off + lane * 16;
        if (nl == 1) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS0; ++ks) {
            if (ks < L0.ks) {
              const bf16x8 a = *(const bf16x8*)(w + (ks << 10));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc, 0, 0, 0);
            }
          }
          p = fmlp_head_score(acc, L0, smem, kg);
        } else {
          for (int nt = 0; nt < L0.nt; ++nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS0; ++ks) {
              if (ks < L0.ks) {
                const bf16x8 a = *(const bf16x8*)(w + ((nt * L0.ks + ks) << 10));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc, 0, 0, 0);
              }
            }
            fmlp_epilogue(acc, L0, nt, false, smem, abuf0, nullptr, row, B, m, kg);
          }
          if (L0.nt & 1) fmlp_zero_tile(abuf0, L0.nt, m, kg);
        }
      }

      // ---- layers 1 .. nl-1: both operands from LDS ----
      for (int li = 1; li < nl; ++li) {
        fmlp_wave_lds_fence();
        const MlpLayer L = t.l[lbase + li];
        const unsigned char* src = abuf0 + ((li - 1) & 1) * t.act_bytes + lane * 16;
        unsigned char* dst = abuf0 + (li & 1) * t.act_bytes;
        const unsigned char* w = smem + L.w_off + lane * 16;
        if (li == nl - 1) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
          for (int ks = 0; ks < L.ks; ++ks) {
            const bf16x8 a = *(const bf16x8*)(w + (ks << 10));
            const bf16x8 b = *(const bf16x8*)(src + (ks << 10));
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
          }
          p = fmlp_head_score(acc, L, smem, kg);
        } else {
          for (int nt = 0; nt < L.nt; ++nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int ks = 0; ks < L.ks; ++ks) {
              const bf16x8 a = *(const bf16x8*)(w + ((nt * L.ks + ks) << 10));
              const bf16x8 b = *(const bf16x8*)(src + (ks << 10));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
            }
            fmlp_epilogue(acc, L, nt, false, smem, dst, nullptr, row, B, m, kg);
          }
          if (L.nt & 1) fmlp_zero_tile(dst, L.nt, m, kg);
        }
      }

      sum += p;
      if (members_out != nullptr && writer)
        members_out[row * (long)t.m_total + t.col0 + mi] = p;
    }
    if (writer) out[row] = sum * scale;
    // the next tile's first member stores to abuf0; order that after this
    // tile's last reads
    fmlp_wave_lds_fence();
  }
}

inline int ceil_to(int v, int a) { return (v + a - 1) / a * a; }

template <int KS0, bool VEC>
void launch(int blocks, int threads, int lds, hipStream_t s, const float* x,
            const uint4* blob, float* out, long B, int K0, const MlpTable& t) {
  auto kern = mlp_score_fused_kernel<KS0, VEC>;
  if (lds > 65536)
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FMLP_LDS_LIMIT));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, s, x, blob, out, B,
                     K0, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <bool VEC>
void launch_ks0(int ks0, int blocks, int threads, int lds, hipStream_t s,
                const float* x, const uint4* blob, float* out, long B, int K0,
                const MlpTable& t) {
  if (ks0 <= 2)       launch<2, VEC>(blocks, threads, lds, s, x, blob, out, B, K0, t);
  else if (ks0 <= 8)  launch<8, VEC>(blocks, threads, lds, s, x, blob, out, B, K0, t);
  else if (ks0 <= 16) launch<16, VEC>(blocks, threads, lds, s, x, blob, out, B, K0, t);
  else                launch<32, VEC>(blocks, threads, lds, s, x, blob, out, B, K0, t);
}

template <int KS0, bool VEC>
void launch_ens(int blocks, int threads, int lds, hipStream_t s, const float* x,
                const uint4* blob, float* out, const float* carry,
                float* members_out, long B, int K0, float scale,
                const EnsTable& t) {
  auto kern = mlp_score_fused_ensemble_kernel<KS0, VEC>;
  if (lds > 65536)
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FMLP_LDS_LIMIT));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, s, x, blob, out,
                     carry, members_out, B, K0, scale, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// no KS0 = 32 here: its fragments already spill for one model, and in the
// ensemble kernel they stay live across every member
template <bool VEC>
void launch_ens_ks0(int ks0, int blocks, int threads, int lds, hipStream_t s,
                    const float* x, const uint4* blob, float* out,
                    const float* carry, float* members_out, long B, int K0,
                    float scale, const EnsTable& t) {
  if (ks0 <= 2)
    launch_ens<2, VEC>(blocks, threads, lds, s, x, blob, out, carry, members_out, B, K0, scale, t);
  else if (ks0 <= 8)
    launch_ens<8, VEC>(blocks, threads, lds, s, x, blob, out, carry, members_out, B, K0, scale, t);
  else
    launch_ens<16, VEC>(blocks, threads, lds, s, x, blob, out, carry, members_out, B, K0, scale, t);
}

}  // namespace

// x            fp32 [B, K0] on the GPU
// packed       uint8 blob on the GPU (layout above; pack_mlp builds it)
// layer_table  int32 [L, 4] on the CPU: byte offset, N, K, activation id
// max_blocks   > 0 caps the grid (tests force the grid-stride loop to wrap)
// waves        waves per block sharing one weight copy (2, 4 or 8)
// Every offset the kernel uses is re-derived and bounds-checked here, so a
// malformed table is an error, never an out-of-range LDS or global access.
at::Tensor mlp_score_fused(at::Tensor x, at::Tensor packed,
                           at::Tensor layer_table, int64_t max_blocks,
                           int64_t waves) {
  TORCH_CHECK(x.is_cuda() && packed.is_cuda(), "x and packed must be on GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 2 && x.is_contiguous(),
              "x must be contiguous fp32 [B, K0]");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1 &&
              packed.is_contiguous(), "packed must be a contiguous uint8 blob");
  TORCH_CHECK(!layer_table.is_cuda() && layer_table.scalar_type() == at::kInt &&
              layer_table.dim() == 2 && layer_table.size(1) == 4 &&
              layer_table.is_contiguous(),
              "layer_table must be a CPU int32 [L, 4] tensor");
  TORCH_CHECK(waves == 2 || waves == 4 || waves == 8, "waves must be 2, 4 or 8");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
  const long L = layer_table.size(0);
  TORCH_CHECK(L >= 1 && L <= FMLP_MAX_LAYERS, "fused MLP supports 1..",
              FMLP_MAX_LAYERS, " layers, got ", L);
  const long B = x.size(0);
  const int K0 = (int)x.size(1);
  const long blob_bytes = packed.numel();
  TORCH_CHECK(blob_bytes % 16 == 0 && blob_bytes <= FMLP_LDS_LIMIT,
              "bad packed blob size ", blob_bytes);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(packed.data_ptr()) & 15) == 0,
              "packed blob must be 16-byte aligned");

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
  TORCH_CHECK(t.l[0].ks <= FMLP_MAX_KS0, "input width ", K0, " > ",
              FMLP_MAX_KS0 * 32);
  t.act_bytes = 32 * max_kpad;           // 16 rows x Kpad bf16
  // eligibility is defined for the full 8-wave block
  const long lds_full = blob_bytes + 2L * FMLP_MAX_WAVES * t.act_bytes;
  TORCH_CHECK(lds_full <= FMLP_LDS_LIMIT, "fused MLP needs ", lds_full,
              " B of LDS > ", FMLP_LDS_LIMIT);
  const int lds = (int)(blob_bytes + 2L * waves * t.act_bytes);

  auto out = at::empty({B}, x.options());
  if (B == 0) return out;

  const long n_tiles = (B + 15) / 16;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  // resident blocks per CU: LDS-bound, and at most 16 waves per CU
  long per_cu = (160 * 1024) / lds;
  if (per_cu > 16 / waves) per_cu = 16 / waves;
  if (per_cu < 1) per_cu = 1;
  long blocks = (n_tiles + waves - 1) / waves;
  if (blocks > cus * per_cu) blocks = cus * per_cu;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;

  const bool vec = (K0 % 4 == 0) &&
                   (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const float* xp = x.data_ptr<float>();
  const uint4* bp = (const uint4*)packed.data_ptr();
  float* op = out.data_ptr<float>();
  if (vec)
    launch_ks0<true>(t.l[0].ks, (int)blocks, (int)waves * 64, lds, s, xp, bp, op, B, K0, t);
  else
    launch_ks0<false>(t.l[0].ks, (int)blocks, (int)waves * 64, lds, s, xp, bp, op, B, K0, t);
  return out;
}

// Bagged-ensemble scoring: mean over all members of the per-member scores.
// x            fp32 [B, K0] on the GPU
// blobs        one uint8 blob per group on the GPU: the members' packed
//              images back to back (pack_ensemble builds them)
// tables       one CPU int32 [Lg, 5] per group: member index within the
//              group, byte offset, N, K, activation id
// Returns {mean [B]} or, with return_members, {mean [B], members [B, M]}.
// One launch per group on the current stream; non-final groups leave the raw
// partial sum in `out`, which the next launch reads back in place, and the
// final launch scales by float(1 / M).  Every group is validated before the
// first launch, so a malformed table is an error and nothing runs.
std::vector<at::Tensor> mlp_score_fused_ensemble(
    at::Tensor x, std::vector<at::Tensor> blobs, std::vector<at::Tensor> tables,
    bool return_members, int64_t max_blocks, int64_t waves) {
  TORCH_CHECK(x.is_cuda(), "x must be on GPU");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 2 && x.is_contiguous(),
              "x must be contiguous fp32 [B, K0]");
  TORCH_CHECK(waves == 2 || waves == 4 || waves == 8, "waves must be 2, 4 or 8");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
  const size_t G = blobs.size();
  TORCH_CHECK(G >= 1 && G == tables.size(), "need one table per blob, got ",
              blobs.size(), " blobs and ", tables.size(), " tables");
  TORCH_CHECK(G <= (size_t)FENS_MAX_TOTAL, "too many groups: ", G);
  const long B = x.size(0);
  const int K0 = (int)x.size(1);
  TORCH_CHECK(K0 >= 1 && ceil_to(K0, 32) / 32 <= FENS_MAX_KS0,
              "ensemble input width ", K0, " > ", FENS_MAX_KS0 * 32);

  std::vector<EnsTable> ts(G);
  int max_kpad = 32;
  long m_total = 0;
  for (size_t g = 0; g < G; ++g) {
    const at::Tensor& packed = blobs[g];
    const at::Tensor& table = tables[g];
    TORCH_CHECK(packed.is_cuda() && packed.device() == x.device(),
                "group ", g, ": blob must be on the rows' GPU");
    TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1 &&
                packed.is_contiguous(), "group ", g,
                ": blob must be a contiguous uint8 tensor");
    TORCH_CHECK(!table.is_cuda() && table.scalar_type() == at::kInt &&
                table.dim() == 2 && table.size(1) == 5 && table.is_contiguous(),
                "group ", g, ": table must be a CPU int32 [L, 5] tensor");
    const long L = table.size(0);
    TORCH_CHECK(L >= 1 && L <= FENS_MAX_LAYERS, "group ", g, ": ", L,
                " layers, a group holds 1..", FENS_MAX_LAYERS);
    const long blob_bytes = packed.numel();
    TORCH_CHECK(blob_bytes % 16 == 0 && blob_bytes <= FMLP_LDS_LIMIT,
                "group ", g, ": bad packed blob size ", blob_bytes);
    TORCH_CHECK((reinterpret_cast<uintptr_t>(packed.data_ptr()) & 15) == 0,
                "group ", g, ": packed blob must be 16-byte aligned");

    const int* tab = table.data_ptr<int>();
    EnsTable& t = ts[g];
    t = EnsTable{};
    t.blob_bytes = (int)blob_bytes;
    int cur = -1, prev = 0, depth = 0;
    long expect_off = 0;
    for (long i = 0; i < L; ++i) {
      const int mi = tab[i * 5 + 0], off = tab[i * 5 + 1], N = tab[i * 5 + 2],
                K = tab[i * 5 + 3], act = tab[i * 5 + 4];
      TORCH_CHECK(mi == cur || mi == cur + 1, "group ", g, " layer ", i,
                  ": member index ", mi, " out of order");
      if (mi != cur) {
        TORCH_CHECK(cur < 0 || prev == 1, "group ", g, " member ", cur,
                    ": needs a 1-unit head, got ", prev);
        TORCH_CHECK(mi < FENS_MAX_MEMBERS, "group ", g, ": more than ",
                    FENS_MAX_MEMBERS, " members in one group");
        cur = mi;
        t.first[mi] = (int)i;
        prev = K0;
        depth = 0;
      }
      ++depth;
      TORCH_CHECK(depth <= FMLP_MAX_LAYERS, "group ", g, " member ", mi,
                  ": more than ", FMLP_MAX_LAYERS, " layers");
      TORCH_CHECK(N >= 1 && K >= 1 && K == prev, "group ", g, " member ", mi,
                  " layer ", depth - 1, ": K=", K, " does not chain from ", prev);
      TORCH_CHECK(act >= FACT_NONE && act <= FACT_LEAKY, "group ", g,
                  " layer ", i, ": bad act ", act);
      const int npad = ceil_to(N, 16), kpad = ceil_to(K, 32);
      const long wbytes = (long)npad * kpad * 2, bbytes = (long)npad * 4;
      TORCH_CHECK(off == expect_off && off + wbytes + bbytes <= blob_bytes,
                  "group ", g, " member ", mi, " layer ", depth - 1,
                  ": offset ", off, " outside the packed blob or not contiguous");
      t.l[i] = MlpLayer{off, (int)(off + wbytes), npad / 16, kpad / 32, act};
      expect_off = off + wbytes + bbytes;
      if (depth > 1 && kpad > max_kpad) max_kpad = kpad;
      prev = N;
    }
    TORCH_CHECK(prev == 1, "group ", g, " member ", cur,
                ": needs a 1-unit head, got ", prev);
    TORCH_CHECK(expect_off == blob_bytes, "group ", g,
                ": packed blob has trailing bytes");
    t.n_members = cur + 1;
    t.first[cur + 1] = (int)L;
    t.col0 = (int)m_total;
    m_total += t.n_members;
  }
  TORCH_CHECK(m_total >= 1 && m_total <= FENS_MAX_TOTAL, "ensemble has ", m_total,
              " members, supported 1..", FENS_MAX_TOTAL);
  const int act_bytes = 32 * max_kpad;     // 16 rows x the widest hidden Kpad
  for (size_t g = 0; g < G; ++g) {
    ts[g].act_bytes = act_bytes;
    ts[g].m_total = (int)m_total;
    // eligibility is defined for the full 8-wave block
    const long lds_full = ts[g].blob_bytes + 2L * FMLP_MAX_WAVES * act_bytes;
    TORCH_CHECK(lds_full <= FMLP_LDS_LIMIT, "group ", g, " needs ", lds_full,
                " B of LDS > ", FMLP_LDS_LIMIT);
  }

  auto out = at::empty({B}, x.options());
  at::Tensor members;
  if (return_members) members = at::empty({B, m_total}, x.options());
  std::vector<at::Tensor> ret{out};
  if (return_members) ret.push_back(members);
  if (B == 0) return ret;

  const long n_tiles = (B + 15) / 16;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const bool vec = (K0 % 4 == 0) &&
                   (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const float* xp = x.data_ptr<float>();
  float* op = out.data_ptr<float>();
  float* mp = return_members ? members.data_ptr<float>() : nullptr;
  const float inv_m = (float)(1.0 / (double)m_total);
  const int ks0 = ceil_to(K0, 32) / 32;
  for (size_t g = 0; g < G; ++g) {
    const EnsTable& t = ts[g];
    const int lds = (int)(t.blob_bytes + 2L * waves * act_bytes);
    long per_cu = (160 * 1024) / lds;
    if (per_cu > 16 / waves) per_cu = 16 / waves;
    if (per_cu < 1) per_cu = 1;
    long blocks = (n_tiles + waves - 1) / waves;
    if (blocks > cus * per_cu) blocks = cus * per_cu;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    const float* carry = g == 0 ? nullptr : op;
    const float scale = g + 1 == G ? inv_m : 1.0f;
    const uint4* bp = (const uint4*)blobs[g].data_ptr();
    if (vec)
      launch_ens_ks0<true>(ks0, (int)blocks, (int)waves * 64, lds, s, xp, bp, op,
                           carry, mp, B, K0, scale, t);
    else
      launch_ens_ks0<false>(ks0, (int)blocks, (int)waves * 64, lds, s, xp, bp, op,
                            carry, mp, B, K0, scale, t);
  }
  return ret;
}
