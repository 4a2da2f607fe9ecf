// fused_mlp_stream.hip — whole-network MLP scoring in ONE kernel for networks
// whose weights do NOT fit in LDS (gfx950 / MI355X).
//
// fused_mlp.hip keeps the whole packed weight image in LDS and gives every
// wave a private 16-row tile; that stops at 128 KiB of weights + buffers.
// This kernel makes the opposite residency choice: ACTIVATIONS live in LDS,
// WEIGHTS never do.
//
//   * An 8-wave block owns a tile of BM rows (BM = 64, 32 or 16) and takes
//     tiles grid-stride.  LDS holds two activation buffers only, each BM/16
//     fragment-ordered 16-row groups: buffer A is the input of layers 0, 2,
//     4, ..., buffer B the input of layers 1, 3, ...
//   * The block loads its BM x K0 input tile once, rounds it to bf16 (RNE) in
//     registers and writes it into buffer A in fragment order, zero-filled up
//     to ceil32(K0) and for rows past B.  After that every layer looks alike,
//     and K0 is bounded by LDS, not by registers.
//   * Per layer the 16-feature tiles are dealt to the waves in groups of T
//     (1, 2 or 4, chosen per layer by the launcher).  For every k-step a wave
//     reads the BM/16 activation fragments from LDS (one ds_read_b128 each,
//     the same addresses for all waves) and its own T weight fragments
//     straight from global memory into registers: in pack_mlp's fragment
//     order all k-steps of one feature tile are one contiguous run of 1 KiB
//     fragments, so each is one fully coalesced wave load, served by L2/MALL
//     once the first row tile has pulled it in.  Weight loads run
//     FSTREAM_DEPTH k-steps ahead through a register ring.
//   * D = W * X^T as in fused_mlp.hip: 4 consecutive features of one row per
//     lane, so the epilogue (fp32 bias from global, activation, bf16 RNE) is
//     one 8-byte LDS store per lane into the OTHER buffer, again in fragment
//     order.  One __syncthreads() between layers, none inside, no atomics.
//
// Every output element is summed over k ascending in one accumulator, for
// every BM and T, so scores are bitwise independent of both.
//
// No inline assembly, no grid sync, plain vector stores only.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

// Device code of this file is built without packed fp32 instructions, as
// fused_mlp_grad.hip and eval_hist.hip are.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "fused_mlp_common.h"

namespace {

constexpr int FSTREAM_WAVES = 8;              // 512 threads
constexpr int FSTREAM_LDS_LIMIT = 160 * 1024; // all of a gfx950 CU's LDS
constexpr int FSTREAM_MAX_WIDTH = 4096;       // K0 and every layer width
// k-steps a weight fragment is requested ahead of its MFMA.  At the largest
// instantiation (BM = 64, T = 4) the ring is 4*4*4 = 64 VGPRs next to 64
// accumulator and 16 activation-fragment VGPRs; the compiler's report
// (profiles/streamed_mlp_scoring.md) shows no instantiation spilling.
constexpr int FSTREAM_DEPTH = 4;

struct StreamTable {
  int n_layers;
  int buf_b_off;     // LDS byte offset of buffer B (= size of buffer A)
  MlpLayer l[FMLP_MAX_LAYERS];
  int tpw[FMLP_MAX_LAYERS];   // T of each layer: feature tiles per wave group
};

// how the block reads its input rows
enum { XIN_F32_VEC = 0, XIN_F32 = 1, XIN_BF16_VEC = 2, XIN_BF16 = 3 };

// The 8 input values k = c .. c+7 of one row as a bf16x8 fragment (uint4);
// indices >= K0 and rows past B give zeros.  The VEC modes need K0 % 4 == 0
// and an aligned base, so a 4-element load is never split by K0.
FMLP_DEVINL uint4 fstream_load8(const void* __restrict__ x, int mode, long row,
                                bool row_ok, int c, int K0) {
  uint4 p = make_uint4(0u, 0u, 0u, 0u);
  if (!row_ok) return p;
  if (mode == XIN_F32_VEC) {
    const float* xr = (const float*)x + row * (long)K0;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c < K0) a = *(const float4*)(xr + c);
    if (c + 4 < K0) b = *(const float4*)(xr + c + 4);
    p.x = fmlp_pack2(a.x, a.y); p.y = fmlp_pack2(a.z, a.w);
    p.z = fmlp_pack2(b.x, b.y); p.w = fmlp_pack2(b.z, b.w);
  } else if (mode == XIN_F32) {
    const float* xr = (const float*)x + row * (long)K0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (c + j < K0) ? xr[c + j] : 0.0f;
    p.x = fmlp_pack2(v[0], v[1]); p.y = fmlp_pack2(v[2], v[3]);
    p.z = fmlp_pack2(v[4], v[5]); p.w = fmlp_pack2(v[6], v[7]);
  } else if (mode == XIN_BF16_VEC) {
    const unsigned short* xr = (const unsigned short*)x + row * (long)K0;
    uint2 a = make_uint2(0u, 0u), b = a;
    if (c < K0) a = *(const uint2*)(xr + c);
    if (c + 4 < K0) b = *(const uint2*)(xr + c + 4);
    p = make_uint4(a.x, a.y, b.x, b.y);
  } else {
    const unsigned short* xr = (const unsigned short*)x + row * (long)K0;
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (c + j < K0) ? (unsigned)xr[c + j] : 0u;
    p.x = v[0] | (v[1] << 16); p.y = v[2] | (v[3] << 16);
    p.z = v[4] | (v[5] << 16); p.w = v[6] | (v[7] << 16);
  }
  return p;
}

// Hidden-layer epilogue of one wave's T feature tiles x RG row groups: + bias,
// activation (ACT is a constant here, so the switch in fmlp_act folds away),
// bf16 RNE, one 8-byte store per lane into the next layer's input buffer.
template <int ACT, int RG, int T>
FMLP_DEVINL void fstream_store_hidden(const f32x4 (&acc)[T][RG],
                                      const float* __restrict__ bias, int nt0,
                                      int NT, unsigned char* dst, int dst_stride,
                                      int m, int kg) {
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (nt0 + t < NT) {
      const int n0 = (nt0 + t) * 16 + kg * 4;   // first of this lane's 4 features
      const float4 b = *(const float4*)(bias + n0);
      const int off = fmlp_frag_off(n0, m);
#pragma unroll
      for (int g = 0; g < RG; ++g) {
        uint2 p;
        p.x = fmlp_pack2(fmlp_act(acc[t][g][0] + b.x, ACT),
                         fmlp_act(acc[t][g][1] + b.y, ACT));
        p.y = fmlp_pack2(fmlp_act(acc[t][g][2] + b.z, ACT),
                         fmlp_act(acc[t][g][3] + b.w, ACT));
        *(uint2*)(dst + g * dst_stride + off) = p;
      }
    }
  }
}

// One layer for one block tile.  src: this layer's input, RG groups of
// L.ks 1-KiB fragments; dst: the next layer's input (groups of dst_stride
// bytes).  The head (last) stores fp32 scores instead.
template <int RG, int T>
FMLP_DEVINL void fstream_layer(const unsigned char* __restrict__ blob,
                               const MlpLayer L, bool last,
                               const unsigned char* src, unsigned char* dst,
                               int dst_stride, float* __restrict__ out,
                               long row0, long B, int wave, int lane) {
  constexpr int D = FSTREAM_DEPTH;
  const int m = lane & 15;        // row within a 16-row group
  const int kg = lane >> 4;       // k-group (operands) / feature group (D)
  const int KS = L.ks, NT = L.nt;
  const int n_groups = (NT + T - 1) / T;
  const int src_stride = KS << 10;
  const float* bias = (const float*)(blob + L.b_off);
  const unsigned char* sl = src + lane * 16;

  for (int gi = wave; gi < n_groups; gi += FSTREAM_WAVES) {
    const int nt0 = gi * T;
    // a ragged last group re-reads tile NT-1 (in bounds) and drops the result
    const unsigned char* wp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int nt = nt0 + t < NT ? nt0 + t : NT - 1;
      wp[t] = blob + L.w_off + ((long)nt * KS << 10) + lane * 16;
    }

    f32x4 acc[T][RG];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int g = 0; g < RG; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    bf16x8 ring[D][T] = {};
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (d < KS)
#pragma unroll
        for (int t = 0; t < T; ++t)
          ring[d][t] = *(const bf16x8*)(wp[t] + (d << 10));

    for (int ks0 = 0; ks0 < KS; ks0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int ks = ks0 + d;
        if (ks < KS) {
          bf16x8 a[T], b[RG];
#pragma unroll
          for (int t = 0; t < T; ++t) a[t] = ring[d][t];
          if (ks + D < KS)
#pragma unroll
            for (int t = 0; t < T; ++t)
              ring[d][t] = *(const bf16x8*)(wp[t] + ((ks + D) << 10));
#pragma unroll
          for (int g = 0; g < RG; ++g)
            b[g] = *(const bf16x8*)(sl + g * src_stride + (ks << 10));
#pragma unroll
          for (int t = 0; t < T; ++t)
#pragma unroll
            for (int g = 0; g < RG; ++g)
              acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[g],
                                                                  acc[t][g], 0, 0, 0);
        }
      }
    }

    if (last) {
      // head: feature 0 of every row sits in r=0 of lanes 0..15; logit stays fp32
      const float b0 = bias[0];
      if (kg == 0 && nt0 == 0) {
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          const long row = row0 + g * 16 + m;
          if (row < B) out[row] = 1.0f / (1.0f + __expf(-(acc[0][g][0] + b0)));
        }
      }
    } else {
      switch (L.act) {
        case FACT_SIGMOID:
          fstream_store_hidden<FACT_SIGMOID, RG, T>(acc, bias, nt0, NT, dst, dst_stride, m, kg);
          break;
        case FACT_TANH:
          fstream_store_hidden<FACT_TANH, RG, T>(acc, bias, nt0, NT, dst, dst_stride, m, kg);
          break;
        case FACT_RELU:
          fstream_store_hidden<FACT_RELU, RG, T>(acc, bias, nt0, NT, dst, dst_stride, m, kg);
          break;
        case FACT_LEAKY:
          fstream_store_hidden<FACT_LEAKY, RG, T>(acc, bias, nt0, NT, dst, dst_stride, m, kg);
          break;
        default:
          fstream_store_hidden<FACT_NONE, RG, T>(acc, bias, nt0, NT, dst, dst_stride, m, kg);
          break;
      }
    }
  }

  // Kpad = ceil32(N) of the next layer can exceed Npad = ceil16(N): the wave
  // next in the deal zeroes that pad tile (stale LDS could hold NaN patterns)
  if (!last && (NT & 1) && wave == n_groups % FSTREAM_WAVES) {
    const int off = fmlp_frag_off(NT * 16 + kg * 4, m);
#pragma unroll
    for (int g = 0; g < RG; ++g)
      *(uint2*)(dst + g * dst_stride + off) = make_uint2(0u, 0u);
  }
}

template <int BM>
__global__ __launch_bounds__(FSTREAM_WAVES * 64)
void mlp_score_stream_kernel(const void* __restrict__ x, int xmode,
                             const unsigned char* __restrict__ blob,
                             float* __restrict__ out, long B, int K0,
                             StreamTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int RG = BM / 16;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = lane & 15;
  const int kg = lane >> 4;
  const int nl = t.n_layers;
  const int KS0 = t.l[0].ks;
  const long n_tiles = (B + BM - 1) / BM;

  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long row0 = tile * BM;

    // ---- layer-0 input: global -> bf16 (RNE) -> buffer A, fragment order.
    // One unit = one 1-KiB fragment (16 rows x 32 k): lane (m, kg) loads 8
    // consecutive values of row m, the four k-groups of a row cover one
    // 128-byte line of fp32 input, and the wave's 16-byte LDS stores are
    // contiguous.
    for (int u = wave; u < RG * KS0; u += FSTREAM_WAVES) {
      const int g = u / KS0, ks = u - g * KS0;
      const long row = row0 + g * 16 + m;
      const uint4 p = fstream_load8(x, xmode, row, row < B, ks * 32 + kg * 8, K0);
      *(uint4*)(smem + ((long)u << 10) + lane * 16) = p;
    }
    __syncthreads();

    for (int li = 0; li < nl; ++li) {
      const MlpLayer L = t.l[li];
      const bool last = (li == nl - 1);
      const unsigned char* src = smem + ((li & 1) ? t.buf_b_off : 0);
      unsigned char* dst = smem + ((li & 1) ? 0 : t.buf_b_off);
      // the next layer's input groups are ceil32(N) wide
      const int dst_stride = last ? 0 : (t.l[li + 1].ks << 10);
      switch (t.tpw[li]) {
        case 4:
          fstream_layer<RG, 4>(blob, L, last, src, dst, dst_stride, out, row0, B, wave, lane);
          break;
        case 2:
          fstream_layer<RG, 2>(blob, L, last, src, dst, dst_stride, out, row0, B, wave, lane);
          break;
        default:
          fstream_layer<RG, 1>(blob, L, last, src, dst, dst_stride, out, row0, B, wave, lane);
          break;
      }
      // layer li+1 (or the next tile's input load) overwrites what this
      // layer read
      __syncthreads();
    }
  }
}

// Bytes of the two activation buffers for a BM-row tile: BM * 2 B * the
// widest ceil32(K) among the even layers (A) and among the odd layers (B) —
// fused_mlp.py::_stream_lds_bytes is the same arithmetic.
inline void fstream_lds_map(const StreamTable& t, int bm, long* a_bytes,
                            long* b_bytes) {
  long ka = 0, kb = 0;
  for (int i = 0; i < t.n_layers; ++i) {
    long& k = (i & 1) ? kb : ka;
    if (t.l[i].ks * 32L > k) k = t.l[i].ks * 32L;
  }
  *a_bytes = bm * 2L * ka;
  *b_bytes = bm * 2L * kb;
}

template <int BM>
void fstream_launch(int blocks, int lds, hipStream_t s, const void* x, int xmode,
                    const unsigned char* blob, float* out, long B, int K0,
                    const StreamTable& t) {
  auto kern = mlp_score_stream_kernel<BM>;
  if (lds > 65536)
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FSTREAM_LDS_LIMIT));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(FSTREAM_WAVES * 64), lds, s, x,
                     xmode, blob, out, B, K0, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace

// x            fp32 or bf16 [B, K0] on the GPU, contiguous
// packed       uint8 blob on the GPU in pack_mlp's per-layer layout
//              (pack_mlp_stream builds it; any size)
// layer_table  int32 [L, 4] on the CPU: byte offset, N, K, activation id
// max_blocks   > 0 caps the grid (tests force the grid-stride loop to wrap)
// row_tile     0 = choose BM here; 16, 32 or 64 forces it (tests, A/B runs)
// Every offset the kernel uses is re-derived and bounds-checked here, so a
// malformed table is an error, never an out-of-range LDS or global access.
at::Tensor mlp_score_stream(at::Tensor x, at::Tensor packed,
                            at::Tensor layer_table, int64_t max_blocks,
                            int64_t row_tile) {
  TORCH_CHECK(x.is_cuda() && packed.is_cuda() && x.device() == packed.device(),
              "x and packed must be on the same GPU");
  TORCH_CHECK((x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16) &&
              x.dim() == 2 && x.is_contiguous(),
              "x must be contiguous fp32 or bf16 [B, K0]");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1 &&
              packed.is_contiguous(), "packed must be a contiguous uint8 blob");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
  TORCH_CHECK(row_tile == 0 || row_tile == 16 || row_tile == 32 || row_tile == 64,
              "row_tile must be 0, 16, 32 or 64");
  const long B = x.size(0);
  const int K0 = (int)x.size(1);
  const long blob_bytes = packed.numel();
  TORCH_CHECK(blob_bytes % 16 == 0 && blob_bytes > 0 && blob_bytes < (1L << 31),
              "bad packed blob size ", blob_bytes);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(packed.data_ptr()) & 15) == 0,
              "packed blob must be 16-byte aligned");
  TORCH_CHECK(K0 >= 1 && K0 <= FSTREAM_MAX_WIDTH, "input width ", K0,
              " outside 1..", FSTREAM_MAX_WIDTH);

  // ---- the layer table, as fmlp_parse_table reads it, minus the limits of
  // the LDS-resident kernels
  TORCH_CHECK(!layer_table.is_cuda() && layer_table.scalar_type() == at::kInt &&
              layer_table.dim() == 2 && layer_table.size(1) == 4 &&
              layer_table.is_contiguous(),
              "layer_table must be a CPU int32 [L, 4] tensor");
  const long L = layer_table.size(0);
  TORCH_CHECK(L >= 1 && L <= FMLP_MAX_LAYERS, "streamed MLP supports 1..",
              FMLP_MAX_LAYERS, " layers, got ", L);
  const int* tab = layer_table.data_ptr<int>();
  StreamTable t{};
  t.n_layers = (int)L;
  int prev = K0;
  long expect_off = 0;
  for (long i = 0; i < L; ++i) {
    const int off = tab[i * 4 + 0], N = tab[i * 4 + 1], K = tab[i * 4 + 2],
              act = tab[i * 4 + 3];
    TORCH_CHECK(N >= 1 && N <= FSTREAM_MAX_WIDTH && K >= 1 && K == prev,
                "layer ", i, ": N=", N, " K=", K, " does not chain from ", prev,
                " or is wider than ", FSTREAM_MAX_WIDTH);
    TORCH_CHECK(act >= FACT_NONE && act <= FACT_LEAKY, "layer ", i, ": bad act ", act);
    const int npad = ceil_to(N, 16), kpad = ceil_to(K, 32);
    const long wbytes = (long)npad * kpad * 2, bbytes = (long)npad * 4;
    TORCH_CHECK(off == expect_off && off + wbytes + bbytes <= blob_bytes,
                "layer ", i, ": offset ", off, " outside the packed blob");
    t.l[i] = MlpLayer{off, (int)(off + wbytes), npad / 16, kpad / 32, act};
    // T: the widest group that still leaves all 8 waves a group each
    const int nt = npad / 16;
    t.tpw[i] = nt >= 4 * FSTREAM_WAVES ? 4 : nt >= 2 * FSTREAM_WAVES ? 2 : 1;
    expect_off = off + wbytes + bbytes;
    prev = N;
  }
  TORCH_CHECK(expect_off == blob_bytes, "packed blob has trailing bytes");
  TORCH_CHECK(prev == 1, "streamed MLP needs a 1-unit head, got ", prev);

  auto out = at::empty({B}, x.options().dtype(at::kFloat));
  if (B == 0) return out;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;

  // ---- row tile.  The weights are re-read from L2 once per row tile, so the
  // largest BM whose two buffers fit the LDS ceiling is the default; it is
  // halved while the batch has fewer tiles than the device has CUs, because
  // a small batch is better spread over more CUs than packed into few.
  long a_bytes = 0, b_bytes = 0;
  int bm = (int)row_tile;
  if (bm == 0) {
    bm = 64;
    for (;;) {
      fstream_lds_map(t, bm, &a_bytes, &b_bytes);
      const bool fits = a_bytes + b_bytes <= FSTREAM_LDS_LIMIT;
      const bool covers = (B + bm - 1) / bm >= cus;
      if (bm == 16 || (fits && covers)) break;
      bm >>= 1;
    }
  }
  fstream_lds_map(t, bm, &a_bytes, &b_bytes);
  const long lds = a_bytes + b_bytes;
  TORCH_CHECK(lds <= FSTREAM_LDS_LIMIT, "streamed MLP needs ", lds,
              " B of LDS at row tile ", bm, " > ", FSTREAM_LDS_LIMIT);
  t.buf_b_off = (int)a_bytes;

  const long n_tiles = (B + bm - 1) / bm;
  // resident blocks per CU: LDS-bound, and at most 2 (16 waves per CU)
  long per_cu = FSTREAM_LDS_LIMIT / lds;
  if (per_cu > 2) per_cu = 2;
  long blocks = n_tiles;
  if (blocks > cus * per_cu) blocks = cus * per_cu;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;

  const bool bf16_in = x.scalar_type() == at::kBFloat16;
  const bool vec = (K0 % 4 == 0) &&
                   (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  const int xmode = bf16_in ? (vec ? XIN_BF16_VEC : XIN_BF16)
                            : (vec ? XIN_F32_VEC : XIN_F32);
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const void* xp = x.data_ptr();
  const unsigned char* bp = (const unsigned char*)packed.data_ptr();
  float* op = out.data_ptr<float>();
  if (bm == 64)
    fstream_launch<64>((int)blocks, (int)lds, s, xp, xmode, bp, op, B, K0, t);
  else if (bm == 32)
    fstream_launch<32>((int)blocks, (int)lds, s, xp, xmode, bp, op, B, K0, t);
  else
    fstream_launch<16>((int)blocks, (int)lds, s, xp, xmode, bp, op, B, K0, t);
  return out;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
