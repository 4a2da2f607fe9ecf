// fused_mlp_grad.hip — forward + loss + backward of a small MLP in ONE kernel
// (gfx950 / MI355X), plus a device-side packer and a fixed-order reduce.
//
// The training counterpart of fused_mlp.hip for nets whose whole weight set
// fits in one CU's LDS (Shifu's default 200 -> [50, 50] -> 1).  A block keeps
// three things in LDS for its lifetime:
//
//   images   the forward image of fused_mlp.hip (per layer bf16 W in MFMA
//            fragment order + fp32 bias) and, for layers >= 1, a second
//            fragment-ordered image of W^T (the dgrad A operand).  Both are
//            built from the live fp32 parameters by mlp_grad_pack_kernel, so
//            a training step never touches the host.
//   per wave every hidden layer's output H_l in fragment order (the next
//            layer's B operand AND the source of act'), and two ping-pong
//            buffers for dZ_l in fragment order (the dgrad B operand).
//   staging  per layer, the block's 64 rows of the layer INPUT (X_0 or
//            H_{l-1}) and of dZ_l, stored m-CONTIGUOUS ("transposed"): for a
//            16-feature tile ft and 32-row step ms the 64 lanes' fragments
//            are contiguous, lane = (m%32/8)*16 + f%16, 8 consecutive rows
//            each — exactly the A/B fragment of a product that reduces over
//            rows, read with one conflict-free ds_read_b128 per lane.
//
// One pass over a 64-row block tile (4 waves x 16 rows):
//   phase 1 (wave-private, no block barrier): each wave runs its 16 rows
//     forward with fused_mlp.hip's rounding points, evaluates loss and
//     dlogit, then walks back down: dH_{l-1}^T = W_l^T-image x dZ_l, times
//     act'(H_{l-1}) read back from the fragment buffer, rounded to bf16.
//     Every epilogue stores twice: 8 bytes into the wave's fragment buffer
//     and four 2-byte stores into the block staging.
//   barrier
//   phase 2 (block level): wgrad reduces over ROWS, and layer 0's dW alone
//     is 4x13 16x16 tiles, so the dW (and db) tiles of ALL layers are dealt
//     round-robin to the 4 waves.  A wave owns its tiles for the whole
//     grid-stride loop and keeps their fp32 accumulators in registers:
//     dW_l[n][k] += dZ_l^T-frag(nt, ms) x X_l^T-frag(kt, ms) over the two
//     32-row steps.  db_l is one more "k tile" whose B operand is all ones.
//   barrier (staging is rewritten by the next pass)
//
// After its last pass a block stores its accumulators once, with plain vector
// stores, as row `blockIdx.x` of an fp32 slab [blocks, P], plus its loss sum
// and nonzero-weight count.  mlp_grad_reduce_kernel sums the slab in block
// order and divides by the count (SUM_BY_NONZERO_WEIGHTS) from device memory.
// No atomics, no grid sync, no inline assembly: the result is bitwise
// reproducible at a fixed grid.
//
// Rows past B are loaded as zeros with weight 0, so their dZ is exactly zero
// and they add nothing; padded features have zero weights in both images.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

// Device code of this file is built without packed fp32 instructions: the
// scalar forms are what the rounding analysis of the kernels assumes.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "fused_mlp_common.h"

namespace {

constexpr int FG_WAVES = 4;                 // waves per block
constexpr int FG_ROWS = FG_WAVES * 16;      // rows per block pass
constexpr int FG_MS = FG_ROWS / 32;         // 32-row reduction steps per pass
constexpr int FG_TILE = FG_MS * 1024;       // staging bytes of one 16-feature tile
constexpr int FG_LDS_LIMIT = 160 * 1024;    // gfx950: 160 KiB of LDS per CU / workgroup
constexpr int FG_MAX_KS0 = 16;              // layer-0 fragments live in VGPRs
constexpr int FG_MAX_SLOTS = 40;            // wgrad accumulator tiles per wave
constexpr int FG_TAIL = 64;                 // per-wave loss/count scratch

enum { FLOSS_WMSE = 0, FLOSS_CE = 1 };      // ops/loss.py LOSS_WMSE / LOSS_SIGMOID_CE

struct GradLayer {
  int w_off, b_off;   // forward image: fragment-ordered W [Npad16, Kpad32], fp32 bias
  int wt_off;         // W^T image [Kpad16, Npad32] in fragment order (layers >= 1)
  int nt, ks;         // Npad16 / 16, Kpad32 / 32   (forward tiles / k-steps)
  int kt, ns;         // Kpad16 / 16, Npad32 / 32   (dgrad tiles / k-steps)
  int N, K, act;
  int h_off;          // this layer's H fragment buffer inside the wave region
  int xT_off;         // staging: this layer's input, m-contiguous, kt tiles
  int dzT_off;        // staging: this layer's dZ, m-contiguous, nt tiles
  int p_off;          // float offset of dW in a slab row; db follows at p_off + N*K
  int tile0;          // first wgrad tile id: layer l owns nt * (kt + 1) ids
};

struct GradTable {
  int n_layers;
  int img_bytes;      // multiple of 16
  int lds_bytes;      // multiple of 16
  int wave_base;      // first wave region
  int wave_bytes;     // one wave region: H buffers, then the two dZ buffers
  int dz_off;         // first dZ buffer inside the wave region
  int dz_bytes;       // one dZ buffer
  int tail_off;       // FG_TAIL bytes of reduction scratch
  int n_tiles;        // wgrad tiles over all layers
  int P;              // floats per slab row
  GradLayer l[FMLP_MAX_LAYERS];
};

struct GradParams {
  const float* w[FMLP_MAX_LAYERS];
  const float* b[FMLP_MAX_LAYERS];
};

// ---------------------------------------------------------------------------
// Packer: one thread per 16-byte chunk of the image, straight from the fp32
// parameters (RNE to bf16, the same values the layer path's bf16 mirror has).
__global__ void mlp_grad_pack_kernel(GradParams p, uint4* __restrict__ img,
                                     GradTable t) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (t.img_bytes >> 4)) return;
  const int byte = c << 4;
  uint4 out = make_uint4(0u, 0u, 0u, 0u);
  for (int li = 0; li < t.n_layers; ++li) {
    const GradLayer L = t.l[li];
    const float* W = p.w[li];
    const int w_end = L.w_off + L.nt * L.ks * 1024;
    if (byte >= L.w_off && byte < w_end) {
      // forward image: chunk (nt, ks, lane) = W[n][k0 .. k0+8)
      const int q = (byte - L.w_off) >> 4;
      const int lane = q & 63;
      const int n = (q >> 6) / L.ks * 16 + (lane & 15);
      const int k0 = (q >> 6) % L.ks * 32 + (lane >> 4) * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (n < L.N && k0 + j < L.K) ? W[(long)n * L.K + k0 + j] : 0.0f;
      out = make_uint4(fmlp_pack2(v[0], v[1]), fmlp_pack2(v[2], v[3]),
                       fmlp_pack2(v[4], v[5]), fmlp_pack2(v[6], v[7]));
    } else if (byte >= L.b_off && byte < L.b_off + L.nt * 64) {
      const int n0 = (byte - L.b_off) >> 2;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (n0 + j < L.N) ? p.b[li][n0 + j] : 0.0f;
      out = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]),
                       __float_as_uint(v[2]), __float_as_uint(v[3]));
    } else if (li > 0 && byte >= L.wt_off && byte < L.wt_off + L.kt * L.ns * 1024) {
      // W^T image: chunk (kt, ns, lane) = W[n0 .. n0+8)[k]
      const int q = (byte - L.wt_off) >> 4;
      const int lane = q & 63;
      const int k = (q >> 6) / L.ns * 16 + (lane & 15);
      const int n0 = (q >> 6) % L.ns * 32 + (lane >> 4) * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (k < L.K && n0 + j < L.N) ? W[(long)(n0 + j) * L.K + k] : 0.0f;
      out = make_uint4(fmlp_pack2(v[0], v[1]), fmlp_pack2(v[2], v[3]),
                       fmlp_pack2(v[4], v[5]), fmlp_pack2(v[6], v[7]));
    }
  }
  img[c] = out;
}

// ---------------------------------------------------------------------------
FMLP_DEVINL float fg_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
FMLP_DEVINL float fg_bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// act'(z) from the (bf16-rounded) layer output y, as act_grad_colsum_kernel does
FMLP_DEVINL float fg_act_grad(float y, int act) {
  switch (act) {
    case FACT_SIGMOID: return y * (1.0f - y);
    case FACT_TANH:    return 1.0f - y * y;
    case FACT_RELU:    return y > 0.0f ? 1.0f : 0.0f;
    case FACT_LEAKY:   return y > 0.0f ? 1.0f : FMLP_LEAKY_SLOPE;
    default:           return 1.0f;
  }
}

// The second store of an epilogue: this lane's features f0..f0+3 (f0 % 4 == 0,
// bf16 bits in p) of its row into the m-contiguous staging of tile f0/16.
// st_lane already holds the row part of the address.
FMLP_DEVINL void fg_stage4(unsigned char* stage, int st_lane, int f0, uint2 p) {
  unsigned char* d = stage + (f0 >> 4) * FG_TILE + st_lane + ((f0 & 15) << 4);
  *(unsigned short*)(d) = (unsigned short)(p.x & 0xffffu);
  *(unsigned short*)(d + 16) = (unsigned short)(p.x >> 16);
  *(unsigned short*)(d + 32) = (unsigned short)(p.y & 0xffffu);
  *(unsigned short*)(d + 48) = (unsigned short)(p.y >> 16);
}

// wgrad tile id -> (layer, nt, kt); kt == l[li].kt is the bias tile
FMLP_DEVINL void fg_tile_of(const GradTable& t, int g, int& li, int& nt, int& kt) {
  li = 0;
  while (li + 1 < t.n_layers && g >= t.l[li + 1].tile0) ++li;
  const int local = g - t.l[li].tile0;
  const int per = t.l[li].kt + 1;
  nt = local / per;
  kt = local - nt * per;
}

// KS0  : compile-time bound on the layer-0 k-steps (fragments stay in VGPRs)
// ACC  : compile-time bound on the wgrad tiles one wave owns
// XBF16: rows are bf16 (else fp32)
// VEC  : rows are 16-byte aligned and a whole number of 16-byte pieces
template <int KS0, int ACC, bool XBF16, bool VEC>
__global__ __launch_bounds__(FG_WAVES * 64)
void mlp_grad_fused_kernel(const void* __restrict__ xv,
                           const float* __restrict__ target,
                           const float* __restrict__ weight,
                           const uint4* __restrict__ img,
                           float* __restrict__ slab, float* __restrict__ parts,
                           long B, int K0, int kind, GradTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  for (int i = tid; i < (t.img_bytes >> 4); i += blockDim.x)
    ((uint4*)smem)[i] = img[i];
  // everything behind the images starts as zeros: padded tiles that no
  // epilogue ever writes must not hold stale NaN bit patterns
  for (int i = (t.img_bytes >> 4) + tid; i < (t.lds_bytes >> 4); i += blockDim.x)
    ((uint4*)smem)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15;        // row within the wave's tile
  const int kg = lane >> 4;       // k-group (operands) / feature group (D)
  const int nl = t.n_layers;
  unsigned char* const wbase = smem + t.wave_base + wave * t.wave_bytes;
  unsigned char* const dzbuf0 = wbase + t.dz_off;
  // row part of a staging address: block row = wave*16 + m
  const int st_lane = (((wave >> 1) * 64 + ((wave & 1) * 2 + (m >> 3)) * 16) << 4) +
                      ((m & 7) << 1);
  const GradLayer L0 = t.l[0];

  // ---- the wgrad tiles this wave owns: operand offsets, fixed for the run ----
  int slot_a[ACC], slot_b[ACC];
  f32x4 wacc[ACC];
#pragma unroll
  for (int i = 0; i < ACC; ++i) {
    wacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    slot_a[i] = -1;
    slot_b[i] = -1;
    const int g = i * FG_WAVES + wave;
    if (g < t.n_tiles) {
      int li, nt, kt;
      fg_tile_of(t, g, li, nt, kt);
      slot_a[i] = t.l[li].dzT_off + nt * FG_TILE;
      if (kt < t.l[li].kt) slot_b[i] = t.l[li].xT_off + kt * FG_TILE;
    }
  }
  const unsigned one2 = 0x3f803f80u;          // two bf16 1.0
  const uint4 ones_u = make_uint4(one2, one2, one2, one2);
  const bf16x8 ones = *(const bf16x8*)&ones_u;

  float lsum = 0.0f, csum = 0.0f;
  const long n_bt = (B + FG_ROWS - 1) / FG_ROWS;

  for (long bt = blockIdx.x; bt < n_bt; bt += gridDim.x) {
    const long row = bt * FG_ROWS + wave * 16 + m;
    const bool row_ok = row < B;

    // ================= phase 1: this wave's 16 rows =================
    // ---- layer-0 B fragments: global -> bf16 (RNE) in registers, and the
    //      same bits into the X_0 staging ----
    bf16x8 xf[KS0];
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) {
      const int c = ks * 32 + kg * 8;
      uint4 p = make_uint4(0u, 0u, 0u, 0u);
      if (XBF16) {
        const unsigned short* xr = (const unsigned short*)xv + row * (long)K0;
        if (VEC) {
          if (row_ok && c < K0) p = *(const uint4*)(xr + c);
        } else {
          unsigned short h[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            h[j] = (row_ok && c + j < K0) ? xr[c + j] : (unsigned short)0;
          p.x = h[0] | ((unsigned)h[1] << 16);
          p.y = h[2] | ((unsigned)h[3] << 16);
          p.z = h[4] | ((unsigned)h[5] << 16);
          p.w = h[6] | ((unsigned)h[7] << 16);
        }
      } else {
        const float* xr = (const float*)xv + row * (long)K0;
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
        p.x = fmlp_pack2(v[0], v[1]);
        p.y = fmlp_pack2(v[2], v[3]);
        p.z = fmlp_pack2(v[4], v[5]);
        p.w = fmlp_pack2(v[6], v[7]);
      }
      xf[ks] = *(bf16x8*)&p;
      // staging holds kt = ceil16(K0)/16 tiles; Kpad32 may reach one further
      if (c < L0.kt * 16) {
        fg_stage4(smem + L0.xT_off, st_lane, c, make_uint2(p.x, p.y));
        fg_stage4(smem + L0.xT_off, st_lane, c + 4, make_uint2(p.z, p.w));
      }
    }

    // ---- forward ----
    float z = 0.0f;                 // head logit of row m (lanes kg == 0)
    for (int li = 0; li < nl; ++li) {
      if (li) fmlp_wave_lds_fence();
      const GradLayer L = t.l[li];
      const bool last = (li == nl - 1);
      const unsigned char* w = smem + L.w_off + lane * 16;
      const unsigned char* src = wbase + (li ? t.l[li - 1].h_off : 0) + lane * 16;
      unsigned char* hdst = wbase + L.h_off;
      unsigned char* hstage = smem + (last ? 0 : t.l[li + 1].xT_off);
      for (int nt = 0; nt < L.nt; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (li == 0) {
#pragma unroll
          for (int ks = 0; ks < KS0; ++ks) {
            if (ks < L.ks) {
              const bf16x8 a = *(const bf16x8*)(w + ((nt * L.ks + ks) << 10));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc, 0, 0, 0);
            }
          }
        } else {
#pragma unroll 2
          for (int ks = 0; ks < L.ks; ++ks) {
            const bf16x8 a = *(const bf16x8*)(w + ((nt * L.ks + ks) << 10));
            const bf16x8 b = *(const bf16x8*)(src + (ks << 10));
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
          }
        }
        const int n0 = nt * 16 + kg * 4;
        const float4 bias = *(const float4*)(smem + L.b_off + n0 * 4);
        if (last) {
          z = acc[0] + bias.x;      // feature 0: r = 0 of lanes 0..15
        } else {
          uint2 p;
          p.x = fmlp_pack2(fmlp_act(acc[0] + bias.x, L.act),
                           fmlp_act(acc[1] + bias.y, L.act));
          p.y = fmlp_pack2(fmlp_act(acc[2] + bias.z, L.act),
                           fmlp_act(acc[3] + bias.w, L.act));
          *(uint2*)(hdst + fmlp_frag_off(n0, m)) = p;
          fg_stage4(hstage, st_lane, n0, p);
        }
      }
      // Kpad32 of the next layer can exceed this layer's Npad16
      if (!last && (L.nt & 1))
        *(uint2*)(hdst + fmlp_frag_off(L.nt * 16 + kg * 4, m)) = make_uint2(0u, 0u);
    }

    // ---- loss and dlogit (every lane of a row computes the same values) ----
    z = __shfl(z, m);
    const float y = row_ok ? target[row] : 0.0f;
    const float sw = row_ok ? weight[row] : 0.0f;
    const float pr = 1.0f / (1.0f + __expf(-z));
    float per, dl;
    if (kind == FLOSS_WMSE) {
      const float d = pr - y;
      per = sw * d * d;
      dl = sw * 2.0f * d * pr * (1.0f - pr);
    } else {
      per = sw * (fmaxf(z, 0.0f) - z * y + log1pf(__expf(-fabsf(z))));
      dl = sw * (pr - y);
    }
    if (kg == 0) {
      lsum += per;
      csum += (sw != 0.0f) ? 1.0f : 0.0f;
    }
    const unsigned dlb = fmlp_bf16_bits(dl);
    // head dZ: feature 0 only.  Staging features 1..15 stay at their initial
    // zeros; the fragment buffer is one full k-step, written whole.
    if (kg == 0)
      *(unsigned short*)(smem + t.l[nl - 1].dzT_off + st_lane) = (unsigned short)dlb;
    *(uint4*)(dzbuf0 + lane * 16) = make_uint4(kg == 0 ? dlb : 0u, 0u, 0u, 0u);

    // ---- backward: dZ_{l-1} = (W_l^T x dZ_l) * act'(H_{l-1}) ----
    int cur = 0;
    for (int li = nl - 1; li >= 1; --li) {
      fmlp_wave_lds_fence();
      const GradLayer L = t.l[li];
      const GradLayer Lp = t.l[li - 1];
      const unsigned char* wt = smem + L.wt_off + lane * 16;
      const unsigned char* src = dzbuf0 + cur * t.dz_bytes + lane * 16;
      unsigned char* dst = dzbuf0 + (cur ^ 1) * t.dz_bytes;
      const unsigned char* hb = wbase + Lp.h_off;
      unsigned char* dstage = smem + Lp.dzT_off;
      const bool more = (li - 1 >= 1);    // layer 0 needs no dgrad
      for (int kt = 0; kt < L.kt; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int ns = 0; ns < L.ns; ++ns) {
          const bf16x8 a = *(const bf16x8*)(wt + ((kt * L.ns + ns) << 10));
          const bf16x8 b = *(const bf16x8*)(src + (ns << 10));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
        const int k0 = kt * 16 + kg * 4;
        const int off = fmlp_frag_off(k0, m);
        const uint2 hp = *(const uint2*)(hb + off);
        uint2 p;
        p.x = fmlp_pack2(acc[0] * fg_act_grad(fg_bf16_lo(hp.x), Lp.act),
                         acc[1] * fg_act_grad(fg_bf16_hi(hp.x), Lp.act));
        p.y = fmlp_pack2(acc[2] * fg_act_grad(fg_bf16_lo(hp.y), Lp.act),
                         acc[3] * fg_act_grad(fg_bf16_hi(hp.y), Lp.act));
        if (more) *(uint2*)(dst + off) = p;
        fg_stage4(dstage, st_lane, k0, p);
      }
      if (more && (L.kt & 1))
        *(uint2*)(dst + fmlp_frag_off(L.kt * 16 + kg * 4, m)) = make_uint2(0u, 0u);
      cur ^= 1;
    }

    __syncthreads();

    // ================= phase 2: block-level wgrad =================
    const unsigned char* const frag = smem + lane * 16;
#pragma unroll
    for (int i = 0; i < ACC; ++i) {
      if (slot_a[i] >= 0) {
#pragma unroll
        for (int ms = 0; ms < FG_MS; ++ms) {
          const bf16x8 a = *(const bf16x8*)(frag + slot_a[i] + (ms << 10));
          bf16x8 b = ones;
          if (slot_b[i] >= 0) b = *(const bf16x8*)(frag + slot_b[i] + (ms << 10));
          wacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, wacc[i], 0, 0, 0);
        }
      }
    }

    // the next pass rewrites the staging
    __syncthreads();
  }

  // ---- this block's slab row: D[n][k], n = nt*16 + kg*4 + r, k = kt*16 + m ----
  float* const mine = slab + (long)blockIdx.x * t.P;
#pragma unroll
  for (int i = 0; i < ACC; ++i) {
    const int g = i * FG_WAVES + wave;
    if (g < t.n_tiles) {
      int li, nt, kt;
      fg_tile_of(t, g, li, nt, kt);
      const GradLayer L = t.l[li];
      const int k = kt * 16 + m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nt * 16 + kg * 4 + r;
        if (n < L.N) {
          if (kt == L.kt) {
            if (m == 0) mine[L.p_off + L.N * L.K + n] = wacc[i][r];
          } else if (k < L.K) {
            mine[L.p_off + n * L.K + k] = wacc[i][r];
          }
        }
      }
    }
  }

  // ---- loss sum and nonzero-weight count, in a fixed order ----
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    lsum += __shfl_xor(lsum, s);
    csum += __shfl_xor(csum, s);
  }
  float* tail = (float*)(smem + t.tail_off);
  if (lane == 0) {
    tail[wave * 2] = lsum;
    tail[wave * 2 + 1] = csum;
  }
  __syncthreads();
  if (tid == 0) {
    float a = 0.0f, c = 0.0f;
    for (int w = 0; w < FG_WAVES; ++w) {
      a += tail[w * 2];
      c += tail[w * 2 + 1];
    }
    parts[blockIdx.x * 2] = a;
    parts[blockIdx.x * 2 + 1] = c;
  }
}

// ---------------------------------------------------------------------------
// grads[p] = (sum over blocks, in block order, of slab[b][p]) / count and
// loss = (sum of the blocks' loss sums) / count, count clamped as ops/loss.py.
__global__ __launch_bounds__(256)
void mlp_grad_reduce_kernel(const float* __restrict__ slab,
                            const float* __restrict__ parts,
                            float* __restrict__ grads, float* __restrict__ loss,
                            int nb, int P) {
  __shared__ float s_cnt;
  if (threadIdx.x == 0) {
    double c = 0.0;                 // whole numbers: exact
    for (int b = 0; b < nb; ++b) c += (double)parts[b * 2 + 1];
    s_cnt = fmaxf((float)c, 1e-12f);
    if (blockIdx.x == 0) {
      float a = 0.0f;
      for (int b = 0; b < nb; ++b) a += parts[b * 2];
      loss[0] = a / s_cnt;
    }
  }
  __syncthreads();
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float a = 0.0f;
  for (int b = 0; b < nb; ++b) a += slab[(long)b * P + p];
  grads[p] = a / s_cnt;
}

template <int KS0, int ACC, bool XBF16, bool VEC>
void launch_grad(int blocks, int lds, hipStream_t s, const void* x,
                 const float* y, const float* w, const uint4* img, float* slab,
                 float* parts, long B, int K0, int kind, const GradTable& t) {
  auto kern = mlp_grad_fused_kernel<KS0, ACC, XBF16, VEC>;
  // once per instantiation, so a step captured into a graph records launches only
  static bool big_lds = false;
  if (lds > 65536 && !big_lds) {
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FG_LDS_LIMIT));
    big_lds = true;
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(FG_WAVES * 64), lds, s, x, y, w,
                     img, slab, parts, B, K0, kind, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// two shapes of kernel: the default-sized nets (<= 256 inputs, <= 24 tiles a
// wave) get the instantiation with the small register footprint
template <bool XBF16, bool VEC>
void launch_grad_size(bool small, int blocks, int lds, hipStream_t s,
                      const void* x, const float* y, const float* w,
                      const uint4* img, float* slab, float* parts, long B,
                      int K0, int kind, const GradTable& t) {
  if (small)
    launch_grad<8, 24, XBF16, VEC>(blocks, lds, s, x, y, w, img, slab, parts, B, K0, kind, t);
  else
    launch_grad<FG_MAX_KS0, FG_MAX_SLOTS, XBF16, VEC>(blocks, lds, s, x, y, w, img, slab, parts, B, K0, kind, t);
}

}  // namespace

// x        fp32 or bf16 [B, K0] on the GPU
// target   fp32 [B], weight fp32 [B] on the GPU
// weights  per layer (head last) fp32 [N, K] on the GPU, biases fp32 [N]
// acts     per layer activation id
// kind     0 = weighted_mse, 1 = sigmoid_ce
// max_blocks > 0 caps the grid (tests force several passes per block)
// Returns {loss (0-d fp32), grads fp32 [P]}: grads holds, layer by layer, dW
// [N, K] then db [N], already divided by the nonzero-weight count.
// The whole LDS map is derived and bounds-checked here; a net that does not
// fit is an error, never an out-of-range access.
std::vector<at::Tensor> mlp_loss_grad_fused(
    at::Tensor x, at::Tensor target, at::Tensor weight,
    std::vector<at::Tensor> weights, std::vector<at::Tensor> biases,
    std::vector<int64_t> acts, int64_t kind, int64_t max_blocks) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
              (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16),
              "x must be a contiguous fp32 or bf16 [B, K0] GPU tensor");
  const long B = x.size(0);
  const int K0 = (int)x.size(1);
  for (const at::Tensor* v : {&target, &weight})
    TORCH_CHECK(v->is_cuda() && v->device() == x.device() &&
                v->scalar_type() == at::kFloat && v->dim() == 1 &&
                v->size(0) == B && v->is_contiguous(),
                "target and weight must be contiguous fp32 [B] on the rows' GPU");
  TORCH_CHECK(kind == FLOSS_WMSE || kind == FLOSS_CE, "bad loss kind ", kind);
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
  const long L = (long)weights.size();
  TORCH_CHECK(L >= 1 && L <= FMLP_MAX_LAYERS, "fused MLP supports 1..",
              FMLP_MAX_LAYERS, " layers, got ", L);
  TORCH_CHECK((long)biases.size() == L && (long)acts.size() == L,
              "need one bias and one activation per layer");
  TORCH_CHECK(K0 >= 1 && ceil_to(K0, 32) / 32 <= FG_MAX_KS0, "input width ", K0,
              " > ", FG_MAX_KS0 * 32);

  GradTable t{};
  GradParams gp{};
  t.n_layers = (int)L;
  int prev = K0, max_npad32 = 32;
  long off = 0, p_off = 0, tiles = 0;
  for (long i = 0; i < L; ++i) {
    const at::Tensor& W = weights[i];
    const at::Tensor& b = biases[i];
    TORCH_CHECK(W.is_cuda() && W.device() == x.device() &&
                W.scalar_type() == at::kFloat && W.dim() == 2 && W.is_contiguous(),
                "layer ", i, ": weight must be a contiguous fp32 [N, K] GPU tensor");
    const int N = (int)W.size(0), K = (int)W.size(1);
    TORCH_CHECK(N >= 1 && K == prev, "layer ", i, ": K=", K,
                " does not chain from ", prev);
    TORCH_CHECK(N <= 4096, "layer ", i, ": width ", N, " cannot fit LDS");
    TORCH_CHECK(b.is_cuda() && b.device() == x.device() &&
                b.scalar_type() == at::kFloat && b.dim() == 1 && b.size(0) == N &&
                b.is_contiguous(), "layer ", i, ": bias must be fp32 [N]");
    const int act = (int)acts[i];
    TORCH_CHECK(act >= FACT_NONE && act <= FACT_LEAKY, "layer ", i, ": bad act ", act);
    GradLayer& G = t.l[i];
    G.N = N; G.K = K; G.act = act;
    G.nt = ceil_to(N, 16) / 16; G.ks = ceil_to(K, 32) / 32;
    G.kt = ceil_to(K, 16) / 16; G.ns = ceil_to(N, 32) / 32;
    G.w_off = (int)off;
    off += (long)G.nt * G.ks * 1024;
    G.b_off = (int)off;
    off += (long)G.nt * 64;
    G.p_off = (int)p_off;
    p_off += (long)N * K + N;
    G.tile0 = (int)tiles;
    tiles += (long)G.nt * (G.kt + 1);
    if (i > 0 && G.ns * 32 > max_npad32) max_npad32 = G.ns * 32;
    gp.w[i] = W.data_ptr<float>();
    gp.b[i] = b.data_ptr<float>();
    prev = N;
  }
  TORCH_CHECK(prev == 1, "fused MLP needs a 1-unit head, got ", prev);
  for (long i = 1; i < L; ++i) {
    t.l[i].wt_off = (int)off;
    off += (long)t.l[i].kt * t.l[i].ns * 1024;
  }
  t.l[0].wt_off = -1;
  TORCH_CHECK(off <= FG_LDS_LIMIT, "weight images need ", off, " B of LDS > ",
              FG_LDS_LIMIT);
  t.img_bytes = (int)off;
  // wave regions: every hidden layer's H (16 rows x Npad32 bf16), two dZ buffers
  long wb = 0;
  for (long i = 0; i + 1 < L; ++i) {
    t.l[i].h_off = (int)wb;
    wb += 32L * t.l[i].ns * 32;
  }
  t.l[L - 1].h_off = 0;             // the head has no H buffer
  t.dz_off = (int)wb;
  t.dz_bytes = 32 * max_npad32;
  wb += 2L * t.dz_bytes;
  t.wave_base = t.img_bytes;
  t.wave_bytes = (int)wb;
  off += FG_WAVES * wb;
  // block staging: per layer its input (kt tiles) and its dZ (nt tiles);
  // layer l's input is layer l-1's output: Kpad16(l) == Npad16(l-1)
  for (long i = 0; i < L; ++i) {
    t.l[i].xT_off = (int)off;
    off += (long)t.l[i].kt * FG_TILE;
    t.l[i].dzT_off = (int)off;
    off += (long)t.l[i].nt * FG_TILE;
  }
  t.tail_off = (int)off;
  off += FG_TAIL;
  TORCH_CHECK(off <= FG_LDS_LIMIT, "fused MLP training step needs ", off,
              " B of LDS > ", FG_LDS_LIMIT);
  t.lds_bytes = (int)off;
  t.n_tiles = (int)tiles;
  t.P = (int)p_off;
  const long slots = (tiles + FG_WAVES - 1) / FG_WAVES;
  TORCH_CHECK(slots <= FG_MAX_SLOTS, "fused MLP training step needs ", slots,
              " gradient tiles per wave > ", FG_MAX_SLOTS);

  const auto f32 = x.options().dtype(at::kFloat);
  auto loss = at::empty({}, f32);
  auto grads = at::empty({t.P}, f32);
  const long n_bt = (B + FG_ROWS - 1) / FG_ROWS;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  long per_cu = (160 * 1024) / t.lds_bytes;
  if (per_cu > 2) per_cu = 2;
  if (per_cu < 1) per_cu = 1;
  long blocks = n_bt < 1 ? 1 : n_bt;
  if (blocks > cus * per_cu) blocks = cus * per_cu;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;

  auto image = at::empty({t.img_bytes}, x.options().dtype(at::kByte));
  auto slab = at::empty({blocks, (long)t.P}, f32);
  auto parts = at::empty({blocks, 2}, f32);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(image.data_ptr()) & 15) == 0,
              "image buffer must be 16-byte aligned");

  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const int chunks = t.img_bytes >> 4;
  hipLaunchKernelGGL(mlp_grad_pack_kernel, dim3((chunks + 255) / 256), dim3(256),
                     0, s, gp, (uint4*)image.data_ptr(), t);
  C10_HIP_KERNEL_LAUNCH_CHECK();

  const bool bf = x.scalar_type() == at::kBFloat16;
  const bool vec = (K0 % (bf ? 8 : 4) == 0) &&
                   (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  const bool small = t.l[0].ks <= 8 && slots <= 24;
  const void* xp = x.data_ptr();
  const float* yp = target.data_ptr<float>();
  const float* wp = weight.data_ptr<float>();
  const uint4* ip = (const uint4*)image.data_ptr();
  float* sp = slab.data_ptr<float>();
  float* pp = parts.data_ptr<float>();
  const int k = (int)kind, nb = (int)blocks;
  if (bf && vec)       launch_grad_size<true, true>(small, nb, t.lds_bytes, s, xp, yp, wp, ip, sp, pp, B, K0, k, t);
  else if (bf)         launch_grad_size<true, false>(small, nb, t.lds_bytes, s, xp, yp, wp, ip, sp, pp, B, K0, k, t);
  else if (vec)        launch_grad_size<false, true>(small, nb, t.lds_bytes, s, xp, yp, wp, ip, sp, pp, B, K0, k, t);
  else                 launch_grad_size<false, false>(small, nb, t.lds_bytes, s, xp, yp, wp, ip, sp, pp, B, K0, k, t);

  hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((t.P + 255) / 256), dim3(256), 0,
                     s, sp, pp, grads.data_ptr<float>(), loss.data_ptr<float>(),
                     nb, t.P);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {loss, grads};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
