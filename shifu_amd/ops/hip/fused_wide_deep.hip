// fused_wide_deep.hip — Wide&Deep scoring in ONE kernel (gfx950 / MI355X):
// id fold, embedding gather, wide term, tower, head and sigmoid.
//
// The tower runs through the streamed-weight layer loop of
// fused_mlp_stream_common.h (activations in LDS, weights from L2 into a
// register ring, 16x16x32 bf16 MFMAs).  What this file adds is everything in
// front of it and the wide term behind it:
//
//   * An 8-wave block owns a tile of BM rows (64, 32 or 16), tiles grid-stride.
//     LDS = buffer A | buffer B | wide[BM] fp32 | idx[BM x F] int32.
//   * Fold.  The block reads the tile's BM x F ids once, folds each one as
//     MultiEmbedding.forward does, row = offset_f + (max(id, 0) mod size_f),
//     and keeps the arena row index in idx[].  Every gather below is then an
//     independent load from an LDS-resident index instead of an id -> row ->
//     value chain, and every index is in bounds for any id value.
//   * Tile.  Buffer A receives [dense | emb_0 | .. | emb_{F-1}] rounded to
//     bf16 (RNE) in fragment order, zero-filled up to ceil32(K0) and for rows
//     past B.  One unit is one 1-KiB fragment; lane (m, kg) produces the 8
//     tower columns c .. c+7 of row m.  With nd % 8 == 0 and D % 8 == 0 a chunk
//     never straddles a source: it is fstream_load8 on the dense row or one
//     16-byte load from a bf16 arena row.  Any other nd or D takes the scalar
//     loader, which resolves each of the 8 columns on its own.
//   * Wide term.  wide[r] = bias + sum_k w[k] * dense[r, k] + sum_f
//     wide_vec[idx[r, f]] in fp32 from the dense values as given.  The waves
//     divide the tile's rows; within a row lane l takes k = l, l+64, .. then
//     f = l, l+64, .., and a xor butterfly sums the 64 partials.  Neither the
//     lane assignment nor the order depends on BM, the grid or B.
//   * Head.  fstream_layer<.., ADD_WIDE> adds wide[r] to the fp32 logit.
//
// Scores are bitwise independent of BM, T, the grid and the batch a row
// arrives in.  No inline assembly, no grid sync, no atomics, plain vector
// stores only.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

// Device code of this file is built without packed fp32 instructions, as
// fused_mlp_stream.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "fused_mlp_stream_common.h"

namespace {

struct WdArgs {
  const void* dense;              // [B, nd] fp32 or bf16 (the kernel's XMODE)
  const void* ids;                // [B, F] int64 or int32 per-feature local ids
  const unsigned short* arena;    // [R, D] bf16 deep arena
  const float* wide_vec;          // [R] fp32 wide arena
  const float* wd_w;              // [nd] fp32 wide-dense weights
  const long* feat;               // [F, 2] (offset, size) of every feature
  float wide_bias;
  int ids64;
  int nd, F, D, K0;
  int R;                          // arena rows, < 2^31
  int wide_off, idx_off;          // LDS byte offsets of wide[] and idx[]
};

// offset + (max(id, 0) mod size).  Most ids and all sizes fit 32 bits, where
// the divide is a fraction of the 64-bit one.  The clamp to [0, R) changes
// nothing for the table the launcher checked on the host; it keeps the gather
// in bounds if the device copy of that table ever disagrees with it.
FMLP_DEVINL int wd_fold(long id, long off, long size, int R) {
  if (id < 0) id = 0;
  if (size < 1) size = 1;
  const long local = ((id | size) >> 32) == 0
                         ? (long)((unsigned)id % (unsigned)size) : id % size;
  long r = off + local;
  r = r < 0 ? 0 : r;
  return (int)(r < R ? r : R - 1);
}

// The 8 tower columns c .. c+7 of tile row r (global row `row`), c % 8 == 0.
template <int XMODE>
FMLP_DEVINL uint4 wd_load8(const WdArgs& a, const int* idx, int r, long row,
                           bool row_ok, int c) {
  constexpr bool VEC = (XMODE == XIN_F32_VEC || XMODE == XIN_BF16_VEC);
  uint4 p = make_uint4(0u, 0u, 0u, 0u);
  if (!row_ok || c >= a.K0) return p;
  if (VEC) {
    if (c < a.nd) return fstream_load8(a.dense, XMODE, row, true, c, a.nd);
    const int e = c - a.nd, f = e / a.D, j = e - f * a.D;
    return *(const uint4*)(a.arena + (long)idx[r * a.F + f] * a.D + j);
  }
  unsigned v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int cc = c + q;
    v[q] = 0u;
    if (cc < a.nd) {
      v[q] = XMODE == XIN_F32
                 ? fmlp_bf16_bits(((const float*)a.dense)[row * a.nd + cc])
                 : (unsigned)((const unsigned short*)a.dense)[row * a.nd + cc];
    } else if (cc < a.K0) {
      const int e = cc - a.nd, f = e / a.D, j = e - f * a.D;
      v[q] = (unsigned)a.arena[(long)idx[r * a.F + f] * a.D + j];
    }
  }
  p.x = v[0] | (v[1] << 16); p.y = v[2] | (v[3] << 16);
  p.z = v[4] | (v[5] << 16); p.w = v[6] | (v[7] << 16);
  return p;
}

template <int BM, int XMODE>
__global__ __launch_bounds__(FSTREAM_WAVES * 64)
void wd_score_stream_kernel(WdArgs a, const unsigned char* __restrict__ blob,
                            float* __restrict__ out, long B, StreamTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int RG = BM / 16;
  constexpr bool F32_ROWS = (XMODE == XIN_F32_VEC || XMODE == XIN_F32);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = lane & 15;
  const int kg = lane >> 4;
  const int nl = t.n_layers;
  const int KS0 = t.l[0].ks;
  const long n_tiles = (B + BM - 1) / BM;
  float* wide = (float*)(smem + a.wide_off);
  int* idx = (int*)(smem + a.idx_off);

  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long row0 = tile * BM;

    // ---- fold the tile's ids into arena row indices (rows past B: row 0,
    // never gathered)
    for (int i = threadIdx.x; i < BM * a.F; i += FSTREAM_WAVES * 64) {
      const int r = i / a.F, f = i - r * a.F;
      const long row = row0 + r;
      int v = 0;
      if (row < B) {
        const long id = a.ids64 ? ((const long*)a.ids)[row * a.F + f]
                                : (long)((const int*)a.ids)[row * a.F + f];
        v = wd_fold(id, a.feat[2 * f], a.feat[2 * f + 1], a.R);
      }
      idx[i] = v;
    }
    __syncthreads();

    // ---- layer-0 input -> buffer A in fragment order, two units in flight
    // per wave so the second unit's gathers do not wait for the first store
    const int units = RG * KS0;
    for (int u = wave; u < units; u += 2 * FSTREAM_WAVES) {
      const int u1 = u + FSTREAM_WAVES;
      const int g0 = u / KS0, ks0 = u - g0 * KS0;
      const int r0 = g0 * 16 + m;
      const uint4 p0 = wd_load8<XMODE>(a, idx, r0, row0 + r0, row0 + r0 < B,
                                       ks0 * 32 + kg * 8);
      uint4 p1 = make_uint4(0u, 0u, 0u, 0u);
      if (u1 < units) {
        const int g1 = u1 / KS0, ks1 = u1 - g1 * KS0;
        const int r1 = g1 * 16 + m;
        p1 = wd_load8<XMODE>(a, idx, r1, row0 + r1, row0 + r1 < B,
                             ks1 * 32 + kg * 8);
      }
      *(uint4*)(smem + ((long)u << 10) + lane * 16) = p0;
      if (u1 < units) *(uint4*)(smem + ((long)u1 << 10) + lane * 16) = p1;
    }

    // ---- wide term: one wave per row, fixed lane assignment and order
    for (int r = wave; r < BM; r += FSTREAM_WAVES) {
      const long row = row0 + r;
      float s = 0.0f;
      if (row < B) {
        for (int k = lane; k < a.nd; k += 64) {
          float x;
          if (F32_ROWS) {
            x = ((const float*)a.dense)[row * a.nd + k];
          } else {
            x = __uint_as_float(
                (unsigned)((const unsigned short*)a.dense)[row * a.nd + k] << 16);
          }
          s = fmaf(a.wd_w[k], x, s);
        }
        for (int f = lane; f < a.F; f += 64) s += a.wide_vec[idx[r * a.F + f]];
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) wide[r] = row < B ? a.wide_bias + s : 0.0f;
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
          fstream_layer<RG, 4, true>(blob, L, last, src, dst, dst_stride, out,
                                     row0, B, wave, lane, wide);
          break;
        case 2:
          fstream_layer<RG, 2, true>(blob, L, last, src, dst, dst_stride, out,
                                     row0, B, wave, lane, wide);
          break;
        default:
          fstream_layer<RG, 1, true>(blob, L, last, src, dst, dst_stride, out,
                                     row0, B, wave, lane, wide);
          break;
      }
      // layer li+1 (or the next tile's fold, tile and wide term) overwrites
      // what this layer read
      __syncthreads();
    }
  }
}

// LDS of one block at a BM-row tile: the two activation buffers, BM floats
// of wide term, BM x F row indices — fused_wide_deep.py::_wd_lds_bytes is the
// same arithmetic.
inline long wd_lds_map(const StreamTable& t, int bm, int F, long* a_bytes,
                       long* b_bytes) {
  fstream_lds_map(t, bm, a_bytes, b_bytes);
  return *a_bytes + *b_bytes + bm * 4L + (long)bm * F * 4L;
}

template <int BM, int XMODE>
void wd_launch(int blocks, int lds, hipStream_t s, const WdArgs& a,
               const unsigned char* blob, float* out, long B,
               const StreamTable& t) {
  auto kern = wd_score_stream_kernel<BM, XMODE>;
  if (lds > 65536)
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FSTREAM_LDS_LIMIT));
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(FSTREAM_WAVES * 64), lds, s, a,
                     blob, out, B, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <int BM>
void wd_launch_mode(int xmode, int blocks, int lds, hipStream_t s,
                    const WdArgs& a, const unsigned char* blob, float* out,
                    long B, const StreamTable& t) {
  switch (xmode) {
    case XIN_F32_VEC: wd_launch<BM, XIN_F32_VEC>(blocks, lds, s, a, blob, out, B, t); break;
    case XIN_F32: wd_launch<BM, XIN_F32>(blocks, lds, s, a, blob, out, B, t); break;
    case XIN_BF16_VEC: wd_launch<BM, XIN_BF16_VEC>(blocks, lds, s, a, blob, out, B, t); break;
    default: wd_launch<BM, XIN_BF16>(blocks, lds, s, a, blob, out, B, t); break;
  }
}

}  // namespace

// dense        fp32 or bf16 [B, nd] on the GPU, contiguous
// ids          int64 or int32 [B, F] on the GPU: per-feature local ids, any value
// arena        bf16 [R, D] deep arena, wide_vec fp32 [R], wd_w fp32 [nd]
// feat_table   int64 [F, 2] on the CPU: (offset, size) of every feature;
//              feat_table_dev is the same table on the GPU (the kernel reads it)
// packed / layer_table   the tower in pack_mlp's layout, K0 = nd + F * D
// max_blocks   > 0 caps the grid; row_tile 0 = choose BM here, else 16, 32, 64
// Every offset the kernel uses is re-derived and bounds-checked here, so a
// malformed table is an error, never an out-of-range LDS or global access.
at::Tensor wd_score_stream(at::Tensor dense, at::Tensor ids, at::Tensor arena,
                           at::Tensor wide_vec, at::Tensor wd_w, double wide_bias,
                           at::Tensor feat_table, at::Tensor feat_table_dev,
                           at::Tensor packed, at::Tensor layer_table,
                           int64_t max_blocks, int64_t row_tile) {
  TORCH_CHECK(dense.is_cuda(), "dense must be on the GPU");
  for (const at::Tensor* p : {&ids, &arena, &wide_vec, &wd_w, &feat_table_dev, &packed})
    TORCH_CHECK(p->is_cuda() && p->device() == dense.device() && p->is_contiguous(),
                "ids, arena, wide_vec, wd_w, feat_table_dev and packed must be "
                "contiguous on the rows' GPU");
  TORCH_CHECK((dense.scalar_type() == at::kFloat || dense.scalar_type() == at::kBFloat16) &&
              dense.dim() == 2 && dense.is_contiguous(),
              "dense must be contiguous fp32 or bf16 [B, nd]");
  TORCH_CHECK((ids.scalar_type() == at::kLong || ids.scalar_type() == at::kInt) &&
              ids.dim() == 2 && ids.size(0) == dense.size(0),
              "ids must be int64 or int32 [B, F]");
  TORCH_CHECK(arena.scalar_type() == at::kBFloat16 && arena.dim() == 2,
              "arena must be bf16 [R, D]");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
  TORCH_CHECK(row_tile == 0 || row_tile == 16 || row_tile == 32 || row_tile == 64,
              "row_tile must be 0, 16, 32 or 64");
  const long B = dense.size(0);
  const long nd = dense.size(1), F = ids.size(1), R = arena.size(0), D = arena.size(1);
  TORCH_CHECK(nd >= 1 && F >= 1 && D >= 1 && R >= 1 && R < (1L << 31),
              "need nd, F, D >= 1 and 1 <= R < 2^31, got nd=", nd, " F=", F,
              " D=", D, " R=", R);
  TORCH_CHECK(nd + F * D <= FSTREAM_MAX_WIDTH, "tower input width ", nd + F * D,
              " > ", FSTREAM_MAX_WIDTH);
  const int K0 = (int)(nd + F * D);
  TORCH_CHECK(wide_vec.scalar_type() == at::kFloat && wide_vec.dim() == 1 &&
              wide_vec.size(0) == R, "wide_vec must be fp32 [R]");
  TORCH_CHECK(wd_w.scalar_type() == at::kFloat && wd_w.dim() == 1 &&
              wd_w.size(0) == nd, "wd_w must be fp32 [nd]");
  TORCH_CHECK(!feat_table.is_cuda() && feat_table.scalar_type() == at::kLong &&
              feat_table.dim() == 2 && feat_table.size(0) == F &&
              feat_table.size(1) == 2 && feat_table.is_contiguous(),
              "feat_table must be a CPU int64 [F, 2] tensor");
  TORCH_CHECK(feat_table_dev.scalar_type() == at::kLong && feat_table_dev.dim() == 2 &&
              feat_table_dev.size(0) == F && feat_table_dev.size(1) == 2,
              "feat_table_dev must be int64 [F, 2]");
  const long* ft = feat_table.data_ptr<long>();
  for (long f = 0; f < F; ++f)
    TORCH_CHECK(ft[2 * f] >= 0 && ft[2 * f + 1] >= 1 && ft[2 * f] <= R &&
                ft[2 * f + 1] <= R - ft[2 * f],
                "feature ", f, ": rows [", ft[2 * f], ", +", ft[2 * f + 1],
                ") outside the ", R, "-row arena");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1,
              "packed must be a contiguous uint8 blob");
  const long blob_bytes = packed.numel();
  TORCH_CHECK(blob_bytes % 16 == 0 && blob_bytes > 0 && blob_bytes < (1L << 31),
              "bad packed blob size ", blob_bytes);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(packed.data_ptr()) & 15) == 0,
              "packed blob must be 16-byte aligned");

  StreamTable t = fstream_parse_table(layer_table, K0, blob_bytes);

  auto out = at::empty({B}, dense.options().dtype(at::kFloat));
  if (B == 0) return out;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;

  // ---- row tile, as in mlp_score_stream: the largest BM whose LDS map fits,
  // halved while the batch has fewer tiles than the device has CUs
  long a_bytes = 0, b_bytes = 0;
  int bm = (int)row_tile;
  if (bm == 0) {
    bm = 64;
    for (;;) {
      const bool fits = wd_lds_map(t, bm, (int)F, &a_bytes, &b_bytes) <= FSTREAM_LDS_LIMIT;
      const bool covers = (B + bm - 1) / bm >= cus;
      if (bm == 16 || (fits && covers)) break;
      bm >>= 1;
    }
  }
  const long lds = wd_lds_map(t, bm, (int)F, &a_bytes, &b_bytes);
  TORCH_CHECK(lds <= FSTREAM_LDS_LIMIT, "Wide&Deep scoring needs ", lds,
              " B of LDS at row tile ", bm, " > ", FSTREAM_LDS_LIMIT);
  t.buf_b_off = (int)a_bytes;

  const long n_tiles = (B + bm - 1) / bm;
  // resident blocks per CU: LDS-bound, and at most 2 (16 waves per CU)
  long per_cu = FSTREAM_LDS_LIMIT / lds;
  if (per_cu > 2) per_cu = 2;
  long blocks = n_tiles;
  if (blocks > cus * per_cu) blocks = cus * per_cu;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;

  WdArgs a{};
  a.dense = dense.data_ptr();
  a.ids = ids.data_ptr();
  a.arena = (const unsigned short*)arena.data_ptr();
  a.wide_vec = wide_vec.data_ptr<float>();
  a.wd_w = wd_w.data_ptr<float>();
  a.feat = feat_table_dev.data_ptr<long>();
  a.wide_bias = (float)wide_bias;
  a.ids64 = ids.scalar_type() == at::kLong;
  a.nd = (int)nd; a.F = (int)F; a.D = (int)D; a.K0 = K0; a.R = (int)R;
  a.wide_off = (int)(a_bytes + b_bytes);
  a.idx_off = a.wide_off + bm * 4;

  // the vector loader: no 8-column chunk straddles a source, and every
  // 16-byte (fp32: two of them) load is aligned
  const bool bf16_in = dense.scalar_type() == at::kBFloat16;
  const bool vec = nd % 8 == 0 && D % 8 == 0 &&
                   (reinterpret_cast<uintptr_t>(dense.data_ptr()) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(arena.data_ptr()) & 15) == 0;
  const int xmode = bf16_in ? (vec ? XIN_BF16_VEC : XIN_BF16)
                            : (vec ? XIN_F32_VEC : XIN_F32);
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const unsigned char* bp = (const unsigned char*)packed.data_ptr();
  float* op = out.data_ptr<float>();
  if (bm == 64)
    wd_launch_mode<64>(xmode, (int)blocks, (int)lds, s, a, bp, op, B, t);
  else if (bm == 32)
    wd_launch_mode<32>(xmode, (int)blocks, (int)lds, s, a, bp, op, B, t);
  else
    wd_launch_mode<16>(xmode, (int)blocks, (int)lds, s, a, bp, op, B, t);
  return out;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
