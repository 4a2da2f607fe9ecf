// fused_mlp_stream_common.h — the streamed-weight layer loop shared by the
// single-kernel scoring paths whose ACTIVATIONS live in LDS and whose WEIGHTS
// never do (fused_mlp_stream.hip: dense MLP bundles, fused_wide_deep.hip:
// Wide&Deep bundles).  Include after torch/extension.h.
//
// Header-only and in an anonymous namespace, like fused_mlp_common.h: each
// translation unit gets its own copy, so mlp_score_stream_kernel compiles to
// the arithmetic it had when these helpers were local to fused_mlp_stream.hip.
#pragma once

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
// bytes).  The head (last) stores fp32 scores instead; with ADD_WIDE it first
// adds the tile's per-row fp32 term wide[0 .. 16*RG) (LDS) to the logit.
template <int RG, int T, bool ADD_WIDE = false>
FMLP_DEVINL void fstream_layer(const unsigned char* __restrict__ blob,
                               const MlpLayer L, bool last,
                               const unsigned char* src, unsigned char* dst,
                               int dst_stride, float* __restrict__ out,
                               long row0, long B, int wave, int lane,
                               const float* wide = nullptr) {
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
          float z = acc[0][g][0] + b0;
          if constexpr (ADD_WIDE) z += wide[g * 16 + m];
          if (row < B) out[row] = 1.0f / (1.0f + __expf(-z));
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

// layer_table  CPU int32 [L, 4]: byte offset, N, K, activation id (pack_mlp)
// The table as fmlp_parse_table reads it, minus the limits of the
// LDS-resident kernels: every offset of a `blob_bytes` blob for K0-wide rows
// is re-derived, and a table that does not describe the blob exactly is an
// error.  Also picks each layer's T.
inline StreamTable fstream_parse_table(const at::Tensor& layer_table, int K0,
                                       long blob_bytes) {
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
  return t;
}

}  // namespace
