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

#include "fused_mlp_stream_common.h"

namespace {

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

  StreamTable t = fstream_parse_table(layer_table, K0, blob_bytes);

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
