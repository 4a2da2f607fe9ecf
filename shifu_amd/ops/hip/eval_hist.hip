// eval_hist.hip — the device-side evaluation pass (gfx950 / MI355X): weighted
// loss and a pair of score histograms, accumulated on the GPU across the
// batches of one evaluation, and AUC / KS computed from the histograms.
//
// The statistic, shared by both producers and by the CPU emulation in
// shifu_amd/ops/eval_hist.py:
//   p    = 1 / (1 + __expf(-logit))                (fmlp_epilogue's expression)
//   bin  = min(NB - 1, (int)(p * NB)), NB a power of two (the multiply is
//          exact); a NaN p goes to bin 0
//   cls  = target >= 0.5
//   count[cls][bin] += 1 (integer)     wsum[cls][bin] += w (fp32)
//   loss_sum += w * (p - y)^2  |  w * bce_with_logits     nonzero += (w != 0)
//
// Producers.  Each block keeps its histogram in LDS (integer and fp32 LDS
// atomics), its loss sum and nonzero count in registers, and at the end
// plain-stores ONE slab row [2NB counts | 2NB weight sums | loss | nonzero] to
// global memory: no global atomics.
//   mlp_eval_fused_kernel  the forward pass of mlp_score_fused_kernel (same
//     packed blob, 8-wave block, wave-private 16-row tiles) with the statistic
//     folded into the head epilogue: lanes 0..15 of a wave hold one row's
//     logit each and issue the two LDS atomics.  No score or logit is stored.
//     16 atomics per wave per tile, behind ~100 MFMAs: contention is no
//     concern and the block keeps a single histogram.
//   eval_hist_kernel       the same statistic for logits already in memory
//     (any model).  16-byte loads, grid capped at the CU count.  Here every
//     lane issues atomics back to back and a trained model's scores pile into
//     a few bins, so the block keeps R = min(32, 4096 / NB) copies of the
//     histogram (64 KiB in all) and lane l uses copy l % R.  A copy is 4NB + 1
//     words long: the odd stride puts the same bin of the R copies into R
//     different LDS banks, so lanes that hit one bin neither share an address
//     nor a bank.  The copies are folded, in copy order, before the slab store.
// eval_hist_reduce_kernel adds the slab rows, in block order, INTO a persistent
// state (int64 counts, fp64 weight sums and loss sum, int64 nonzero count), so
// the batches of an evaluation accumulate with no host involvement.  Counts
// and everything derived from them are bitwise reproducible; weight sums
// inherit the order of the fp32 LDS atomics within a block and are not.
// eval_finish_kernel turns the state into loss, AUC, KS (and their weighted
// forms) in fp64 with one block.
//
// No inline assembly, no grid sync, plain vector stores to global memory.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>

// Device code of this file is built without packed fp32 instructions, as
// fused_mlp_grad.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "fused_mlp_common.h"

namespace {

constexpr int EH_WAVES = 8;                 // fused kernel: waves per block
constexpr int EH_MAX_KS0 = 32;              // layer-0 fragments live in VGPRs
constexpr int EH_LDS_LIMIT = 160 * 1024;    // gfx950: 160 KiB of LDS per CU / workgroup
constexpr int EH_MIN_BINS = 32, EH_MAX_BINS = 4096;
constexpr int EH_STREAM_THREADS = 256;
constexpr int EH_MAX_COPIES = 32;
constexpr int EH_OUT = 8;                   // loss, auc, ks, wauc, wks, n, P, N
constexpr int EH_FIN_THREADS = 256;

enum { ELOSS_WMSE = 0, ELOSS_CE = 1 };      // ops/loss.py LOSS_WMSE / LOSS_SIGMOID_CE

// One row into a histogram at `cnt` (u32 [2][NB]) / `ws` (f32 [2][NB]) in LDS.
FMLP_DEVINL void eh_row(float z, float y, float w, int kind, int NB,
                        unsigned* cnt, float* ws, float& lsum, unsigned& nz) {
  const float p = 1.0f / (1.0f + __expf(-z));
  const float s = p * (float)NB;
  int bin = 0;
  if (s == s) {
    bin = (int)s;
    bin = bin < 0 ? 0 : (bin > NB - 1 ? NB - 1 : bin);
  }
  const int slot = (y >= 0.5f ? NB : 0) + bin;
  __hip_atomic_fetch_add(cnt + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(ws + slot, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  float per;
  if (kind == ELOSS_WMSE) {
    const float d = p - y;
    per = w * d * d;
  } else {
    per = w * (fmaxf(z, 0.0f) - z * y + log1pf(__expf(-fabsf(z))));
  }
  lsum += per;
  nz += (w != 0.0f) ? 1u : 0u;
}

// Block tail shared by both producers: wave-reduce the loss sum and nonzero
// count, sum the waves in wave order, store them behind the histogram words.
// The barrier inside also orders every wave's LDS atomics before the caller
// reads the histogram back.
FMLP_DEVINL void eh_block_tail(float lsum, unsigned nz, unsigned* scratch,
                               unsigned* __restrict__ row, int NB) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    lsum += __shfl_xor(lsum, s);
    nz += __shfl_xor(nz, s);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    scratch[wave * 2] = __float_as_uint(lsum);
    scratch[wave * 2 + 1] = nz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f;
    unsigned c = 0u;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      a += __uint_as_float(scratch[w * 2]);
      c += scratch[w * 2 + 1];
    }
    row[4 * NB] = __float_as_uint(a);
    row[4 * NB + 1] = c;
  }
}

// ---------------------------------------------------------------------------
// KS0  : compile-time bound on the layer-0 k-steps (fragments stay in VGPRs)
// XBF16: rows are bf16 (else fp32)
// VEC  : rows are 16-byte aligned and a whole number of 16-byte pieces
// LDS  : blob | EH_WAVES x 2 activation buffers | 16 NB B histogram | scratch
template <int KS0, bool XBF16, bool VEC>
__global__ __launch_bounds__(EH_WAVES * 64)
void mlp_eval_fused_kernel(const void* __restrict__ xv,
                           const float* __restrict__ target,
                           const float* __restrict__ weight,
                           const uint4* __restrict__ blob,
                           unsigned* __restrict__ slab, long B, int K0, int kind,
                           int NB, MlpTable t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  unsigned* const hist = (unsigned*)(smem + t.blob_bytes + 2 * EH_WAVES * t.act_bytes);
  for (int i = tid; i < (t.blob_bytes >> 4); i += blockDim.x)
    ((uint4*)smem)[i] = blob[i];
  for (int i = tid; i < 4 * NB; i += blockDim.x) hist[i] = 0u;
  __syncthreads();

  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int m = lane & 15;        // row within the tile
  const int kg = lane >> 4;       // k-group (operands) / feature group (D)
  unsigned char* abuf[2];
  abuf[0] = smem + t.blob_bytes + (wave * 2) * t.act_bytes;
  abuf[1] = abuf[0] + t.act_bytes;
  float* const wsum = (float*)(hist + 2 * NB);

  const long n_tiles = (B + 15) >> 4;
  const int nl = t.n_layers;
  float lsum = 0.0f;
  unsigned nz = 0u;

  for (long tile = (long)blockIdx.x * EH_WAVES + wave; tile < n_tiles;
       tile += (long)gridDim.x * EH_WAVES) {
    const long row = tile * 16 + m;
    const bool row_ok = row < B;

    // ---- layer-0 B fragments: global -> bf16 (RNE) in registers ----
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
    }

    // ---- forward: layer 0 from the registers, the rest from LDS ----
    float z = 0.0f;               // head logit of row m (lanes kg == 0)
    for (int li = 0; li < nl; ++li) {
      if (li) fmlp_wave_lds_fence();
      const MlpLayer L = t.l[li];
      const bool last = (li == nl - 1);
      const unsigned char* w = smem + L.w_off + lane * 16;
      const unsigned char* src = abuf[(li + 1) & 1] + lane * 16;
      unsigned char* dst = abuf[li & 1];
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
        if (last) {
          // head: feature 0 of every row sits in r=0 of lanes 0..15
          z = acc[0] + *(const float*)(smem + L.b_off + kg * 16);
        } else {
          fmlp_epilogue(acc, L, nt, false, smem, dst, nullptr, row, B, m, kg);
        }
      }
      if (!last && (L.nt & 1)) fmlp_zero_tile(dst, L.nt, m, kg);
    }

    // ---- head epilogue: the evaluation statistic, 16 lanes per wave ----
    if (kg == 0 && row_ok)
      eh_row(z, target[row], weight[row], kind, NB, hist, wsum, lsum, nz);

    // the next tile's layer 0 stores to abuf[0]; order them after this
    // tile's last reads of it
    fmlp_wave_lds_fence();
  }

  unsigned* const mine = slab + (long)blockIdx.x * (4 * NB + 2);
  eh_block_tail(lsum, nz, hist + 4 * NB, mine, NB);
  for (int i = tid; i < 4 * NB; i += blockDim.x) mine[i] = hist[i];
}

// ---------------------------------------------------------------------------
// ZBF16: logits are bf16 (else fp32)
// VEC  : logits, targets and weights are 16-byte aligned -> 16-byte loads of
//        V = 8 (bf16) or 4 (fp32) rows per lane; the last, partial piece and
//        the unaligned case take dword / word loads
// LDS  : R copies of (4NB + 1) words | scratch
template <bool ZBF16, bool VEC>
__global__ __launch_bounds__(EH_STREAM_THREADS)
void eval_hist_kernel(const void* __restrict__ zv, const float* __restrict__ target,
                      const float* __restrict__ weight, unsigned* __restrict__ slab,
                      long n, int kind, int NB, int R) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* const words = (unsigned*)smem;
  const int tid = threadIdx.x;
  const int stride = 4 * NB + 1;
  for (int i = tid; i < R * stride; i += blockDim.x) words[i] = 0u;
  __syncthreads();

  unsigned* const cnt = words + (tid & (R - 1)) * stride;
  float* const wsum = (float*)(cnt + 2 * NB);
  constexpr int V = ZBF16 ? 8 : 4;
  const long nv = (n + V - 1) / V;
  float lsum = 0.0f;
  unsigned nz = 0u;

  for (long v = (long)blockIdx.x * blockDim.x + tid; v < nv;
       v += (long)gridDim.x * blockDim.x) {
    const long base = v * V;
    float z[V], y[V], w[V];
    if (VEC && base + V <= n) {
      if (ZBF16) {
        const uint4 q = *(const uint4*)((const unsigned short*)zv + base);
        const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          z[2 * j] = __uint_as_float(u[j] << 16);
          z[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
        }
      } else {
        const float4 q = *(const float4*)((const float*)zv + base);
        z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
      }
#pragma unroll
      for (int j = 0; j < V; j += 4) {
        const float4 a = *(const float4*)(target + base + j);
        const float4 b = *(const float4*)(weight + base + j);
        y[j] = a.x; y[j + 1] = a.y; y[j + 2] = a.z; y[j + 3] = a.w;
        w[j] = b.x; w[j + 1] = b.y; w[j + 2] = b.z; w[j + 3] = b.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool ok = base + j < n;
        if (ZBF16)
          z[j] = ok ? __uint_as_float((unsigned)((const unsigned short*)zv)[base + j] << 16) : 0.0f;
        else
          z[j] = ok ? ((const float*)zv)[base + j] : 0.0f;
        y[j] = ok ? target[base + j] : 0.0f;
        w[j] = ok ? weight[base + j] : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (base + j < n) eh_row(z[j], y[j], w[j], kind, NB, cnt, wsum, lsum, nz);
  }

  unsigned* const mine = slab + (long)blockIdx.x * (4 * NB + 2);
  eh_block_tail(lsum, nz, words + R * stride, mine, NB);
  // fold the copies in copy order: counts as integers, weight sums in fp32
  for (int i = tid; i < 4 * NB; i += blockDim.x) {
    if (i < 2 * NB) {
      unsigned c = 0u;
      for (int r = 0; r < R; ++r) c += words[r * stride + i];
      mine[i] = c;
    } else {
      float a = 0.0f;
      for (int r = 0; r < R; ++r) a += __uint_as_float(words[r * stride + i]);
      mine[i] = __float_as_uint(a);
    }
  }
}

// ---------------------------------------------------------------------------
// state (8-byte words): [0, 2NB) int64 counts | [2NB, 4NB) fp64 weight sums |
// [4NB] fp64 loss sum | [4NB+1] int64 nonzero count | EH_OUT fp64 results.
// One thread per word adds the slab column, in block order, to the state.
__global__ __launch_bounds__(256)
void eval_hist_reduce_kernel(const unsigned* __restrict__ slab, int nb, int NB,
                             long long* __restrict__ state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int W = 4 * NB + 2;
  if (i >= W) return;
  if (i < 2 * NB || i == W - 1) {
    long long c = 0;
    for (int b = 0; b < nb; ++b) c += (long long)slab[(long)b * W + i];
    state[i] += c;
  } else {
    double a = 0.0;
    for (int b = 0; b < nb; ++b) a += (double)__uint_as_float(slab[(long)b * W + i]);
    double* const d = (double*)state + i;
    *d += a;
  }
}

// AUC and KS of one [2][NB] histogram held as doubles (h0 = negatives, h1 =
// positives), scanned from the top bin down.  Thread t owns the CH = NB /
// active consecutive bins that end at bin NB - 1 - t * CH.
//   AUC = sum_b neg_b * (pos_above_b + pos_b / 2) / (P * N)   (0.5 if P or N is 0)
//   KS  = max over bin edges |pos_above / P - neg_above / N|   (0 if P or N is 0)
template <typename T>
__device__ void eh_auc_ks(const T* __restrict__ h0, const T* __restrict__ h1, int NB,
                          double (*red)[EH_FIN_THREADS], double* res) {
  const int tid = threadIdx.x;
  const int active = NB < EH_FIN_THREADS ? NB : EH_FIN_THREADS;
  const int CH = NB / active;
  const int top = NB - 1 - tid * CH;
  double tp = 0.0, tn = 0.0;
  if (tid < active)
    for (int j = 0; j < CH; ++j) {
      tp += (double)h1[top - j];
      tn += (double)h0[top - j];
    }
  red[0][tid] = tp;
  red[1][tid] = tn;
  __syncthreads();
  double pa = 0.0, na = 0.0, P = 0.0, N = 0.0;     // above this thread's chunk; totals
  for (int u = 0; u < active; ++u) {
    if (u < tid) { pa += red[0][u]; na += red[1][u]; }
    P += red[0][u];
    N += red[1][u];
  }
  __syncthreads();
  const bool both = P > 0.0 && N > 0.0;
  double area = 0.0, ks = 0.0;
  if (tid < active && both)
    for (int j = 0; j < CH; ++j) {
      const double pb = (double)h1[top - j], nb = (double)h0[top - j];
      area += nb * (pa + 0.5 * pb);
      pa += pb;
      na += nb;
      ks = fmax(ks, fabs(pa / P - na / N));
    }
  red[0][tid] = area;
  red[1][tid] = ks;
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, k = 0.0;
    for (int u = 0; u < active; ++u) {
      a += red[0][u];
      k = fmax(k, red[1][u]);
    }
    res[0] = both ? a / (P * N) : 0.5;
    res[1] = k;
    res[2] = P;
    res[3] = N;
  }
  __syncthreads();
}

__global__ __launch_bounds__(EH_FIN_THREADS)
void eval_finish_kernel(long long* __restrict__ state, int NB) {
  __shared__ double red[2][EH_FIN_THREADS];
  __shared__ double rc[4], rw[4];
  const double* const ws = (const double*)state + 2 * NB;
  eh_auc_ks<long long>(state, state + NB, NB, red, rc);
  eh_auc_ks<double>(ws, ws + NB, NB, red, rw);
  if (threadIdx.x == 0) {
    double* const out = (double*)state + 4 * NB + 2;
    const double cnt = (double)state[4 * NB + 1];
    out[0] = ((const double*)state)[4 * NB] / fmax(cnt, 1e-12);
    out[1] = rc[0];
    out[2] = rc[1];
    out[3] = rw[0];
    out[4] = rw[1];
    out[5] = rc[2] + rc[3];
    out[6] = rc[2];
    out[7] = rc[3];
  }
}

// ---------------------------------------------------------------------------
void check_common(const at::Tensor& target, const at::Tensor& weight,
                  const at::Tensor& state, const at::Device& dev, long B,
                  int64_t n_bins, int64_t kind, int64_t max_blocks) {
  for (const at::Tensor* v : {&target, &weight})
    TORCH_CHECK(v->is_cuda() && v->device() == dev &&
                v->scalar_type() == at::kFloat && v->dim() == 1 &&
                v->size(0) == B && v->is_contiguous(),
                "target and weight must be contiguous fp32 [B] on the rows' GPU");
  TORCH_CHECK(n_bins >= EH_MIN_BINS && n_bins <= EH_MAX_BINS &&
              (n_bins & (n_bins - 1)) == 0, "n_bins must be a power of two in [",
              EH_MIN_BINS, ", ", EH_MAX_BINS, "], got ", n_bins);
  TORCH_CHECK(state.is_cuda() && state.device() == dev &&
              state.scalar_type() == at::kLong && state.dim() == 1 &&
              state.is_contiguous() && state.numel() == 4 * n_bins + 2 + EH_OUT,
              "state must be a contiguous int64 [4 * n_bins + 2 + ", EH_OUT,
              "] tensor on the rows' GPU");
  TORCH_CHECK(kind == ELOSS_WMSE || kind == ELOSS_CE, "bad loss kind ", kind);
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
}

void launch_reduce(const at::Tensor& slab, int blocks, int NB, at::Tensor& state,
                   hipStream_t s) {
  const int W = 4 * NB + 2;
  hipLaunchKernelGGL(eval_hist_reduce_kernel, dim3((W + 255) / 256), dim3(256), 0, s,
                     (const unsigned*)slab.data_ptr(), blocks, NB,
                     (long long*)state.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <typename K>
void allow_big_lds(K kern, int lds) {
  if (lds > 65536)
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      EH_LDS_LIMIT));
}

template <int KS0, bool XBF16, bool VEC>
void launch_mlp(int blocks, int lds, hipStream_t s, const void* x, const float* y,
                const float* w, const uint4* blob, unsigned* slab, long B, int K0,
                int kind, int NB, const MlpTable& t) {
  auto kern = mlp_eval_fused_kernel<KS0, XBF16, VEC>;
  allow_big_lds(kern, lds);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(EH_WAVES * 64), lds, s, x, y, w, blob,
                     slab, B, K0, kind, NB, t);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <bool XBF16, bool VEC>
void launch_mlp_ks0(int ks0, int blocks, int lds, hipStream_t s, const void* x,
                    const float* y, const float* w, const uint4* blob,
                    unsigned* slab, long B, int K0, int kind, int NB,
                    const MlpTable& t) {
  if (ks0 <= 8)
    launch_mlp<8, XBF16, VEC>(blocks, lds, s, x, y, w, blob, slab, B, K0, kind, NB, t);
  else
    launch_mlp<EH_MAX_KS0, XBF16, VEC>(blocks, lds, s, x, y, w, blob, slab, B, K0, kind, NB, t);
}

template <bool ZBF16, bool VEC>
void launch_stream(int blocks, int lds, hipStream_t s, const void* z, const float* y,
                   const float* w, unsigned* slab, long n, int kind, int NB, int R) {
  auto kern = eval_hist_kernel<ZBF16, VEC>;
  allow_big_lds(kern, lds);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(EH_STREAM_THREADS), lds, s, z, y, w,
                     slab, n, kind, NB, R);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace

// logits   fp32 or bf16 [B] on the GPU; target, weight fp32 [B]
// state    int64 [4 * n_bins + 2 + 8] on the GPU (layout above), added to in place
// kind     0 = weighted_mse, 1 = sigmoid_ce
// replicas 0 = min(32, 4096 / n_bins) LDS copies of the histogram, else a
//          power of two in [1, 32] whose copies fit the LDS ceiling
// max_blocks > 0 caps the grid below the CU count
void eval_hist_scores(at::Tensor logits, at::Tensor target, at::Tensor weight,
                      at::Tensor state, int64_t n_bins, int64_t kind,
                      int64_t replicas, int64_t max_blocks) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 1 && logits.is_contiguous() &&
              (logits.scalar_type() == at::kFloat ||
               logits.scalar_type() == at::kBFloat16),
              "logits must be a contiguous fp32 or bf16 [B] GPU tensor");
  const long n = logits.size(0);
  check_common(target, weight, state, logits.device(), n, n_bins, kind, max_blocks);
  const int NB = (int)n_bins;
  int64_t R = replicas;
  if (R == 0) R = EH_MAX_BINS / NB < EH_MAX_COPIES ? EH_MAX_BINS / NB : EH_MAX_COPIES;
  TORCH_CHECK(R >= 1 && R <= EH_MAX_COPIES && (R & (R - 1)) == 0,
              "replicas must be 0 or a power of two in [1, ", EH_MAX_COPIES, "], got ", R);
  const long lds = (R * (4L * NB + 1) + 2 * (EH_STREAM_THREADS / 64)) * 4;
  TORCH_CHECK(lds <= EH_LDS_LIMIT, R, " histogram copies of ", NB,
              " bins need ", lds, " B of LDS > ", EH_LDS_LIMIT);
  if (n == 0) return;

  const bool bf = logits.scalar_type() == at::kBFloat16;
  const int V = bf ? 8 : 4;
  const long nv = (n + V - 1) / V;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  long blocks = (nv + EH_STREAM_THREADS - 1) / EH_STREAM_THREADS;
  if (blocks > cus) blocks = cus;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  auto slab = at::empty({blocks, 4L * NB + 2}, logits.options().dtype(at::kInt));

  const bool vec = ((reinterpret_cast<uintptr_t>(logits.data_ptr()) |
                     reinterpret_cast<uintptr_t>(target.data_ptr()) |
                     reinterpret_cast<uintptr_t>(weight.data_ptr())) & 15) == 0;
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const void* zp = logits.data_ptr();
  const float* yp = target.data_ptr<float>();
  const float* wp = weight.data_ptr<float>();
  unsigned* sp = (unsigned*)slab.data_ptr();
  const int k = (int)kind, nb = (int)blocks, r = (int)R, l = (int)lds;
  if (bf && vec)  launch_stream<true, true>(nb, l, s, zp, yp, wp, sp, n, k, NB, r);
  else if (bf)    launch_stream<true, false>(nb, l, s, zp, yp, wp, sp, n, k, NB, r);
  else if (vec)   launch_stream<false, true>(nb, l, s, zp, yp, wp, sp, n, k, NB, r);
  else            launch_stream<false, false>(nb, l, s, zp, yp, wp, sp, n, k, NB, r);
  launch_reduce(slab, nb, NB, state, s);
}

// x            fp32 or bf16 [B, K0] on the GPU; target, weight fp32 [B]
// packed       uint8 blob on the GPU, layer_table CPU int32 [L, 4] (pack_mlp)
// state, kind, max_blocks as eval_hist_scores
// The whole LDS map is re-derived and bounds-checked here; a net whose blob,
// activation buffers and histogram do not fit is an error, never launched.
void eval_hist_mlp(at::Tensor x, at::Tensor target, at::Tensor weight,
                   at::Tensor packed, at::Tensor layer_table, at::Tensor state,
                   int64_t n_bins, int64_t kind, int64_t max_blocks) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
              (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16),
              "x must be a contiguous fp32 or bf16 [B, K0] GPU tensor");
  const long B = x.size(0);
  const int K0 = (int)x.size(1);
  check_common(target, weight, state, x.device(), B, n_bins, kind, max_blocks);
  TORCH_CHECK(packed.is_cuda() && packed.device() == x.device() &&
              packed.scalar_type() == at::kByte && packed.dim() == 1 &&
              packed.is_contiguous(),
              "packed must be a contiguous uint8 blob on the rows' GPU");
  const long blob_bytes = packed.numel();
  TORCH_CHECK(blob_bytes % 16 == 0 && blob_bytes <= EH_LDS_LIMIT,
              "bad packed blob size ", blob_bytes);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(packed.data_ptr()) & 15) == 0,
              "packed blob must be 16-byte aligned");
  const int NB = (int)n_bins;
  const MlpTable t = fmlp_parse_table(layer_table, K0, blob_bytes, EH_MAX_KS0);
  const long lds = blob_bytes + 2L * EH_WAVES * t.act_bytes + 16L * NB + 8L * EH_WAVES;
  TORCH_CHECK(lds <= EH_LDS_LIMIT, "fused MLP evaluation needs ", lds,
              " B of LDS > ", EH_LDS_LIMIT);
  if (B == 0) return;

  const long n_tiles = (B + 15) / 16;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long per_cu = 2 * lds <= EH_LDS_LIMIT ? 2 : 1;   // at most 16 waves per CU
  long blocks = (n_tiles + EH_WAVES - 1) / EH_WAVES;
  if (blocks > cus * per_cu) blocks = cus * per_cu;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  auto slab = at::empty({blocks, 4L * NB + 2}, x.options().dtype(at::kInt));

  const bool bf = x.scalar_type() == at::kBFloat16;
  const bool vec = (K0 % (bf ? 8 : 4) == 0) &&
                   (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  hipStream_t s = c10::hip::getCurrentHIPStream().stream();
  const void* xp = x.data_ptr();
  const float* yp = target.data_ptr<float>();
  const float* wp = weight.data_ptr<float>();
  const uint4* bp = (const uint4*)packed.data_ptr();
  unsigned* sp = (unsigned*)slab.data_ptr();
  const int k = (int)kind, nb = (int)blocks, ks0 = t.l[0].ks, l = (int)lds;
  if (bf && vec)  launch_mlp_ks0<true, true>(ks0, nb, l, s, xp, yp, wp, bp, sp, B, K0, k, NB, t);
  else if (bf)    launch_mlp_ks0<true, false>(ks0, nb, l, s, xp, yp, wp, bp, sp, B, K0, k, NB, t);
  else if (vec)   launch_mlp_ks0<false, true>(ks0, nb, l, s, xp, yp, wp, bp, sp, B, K0, k, NB, t);
  else            launch_mlp_ks0<false, false>(ks0, nb, l, s, xp, yp, wp, bp, sp, B, K0, k, NB, t);
  launch_reduce(slab, nb, NB, state, s);
}

// Writes loss, auc, ks, weighted auc, weighted ks, n, P, N (fp64) into the
// last 8 words of `state`.
void eval_hist_finish(at::Tensor state, int64_t n_bins) {
  TORCH_CHECK(n_bins >= EH_MIN_BINS && n_bins <= EH_MAX_BINS &&
              (n_bins & (n_bins - 1)) == 0, "n_bins must be a power of two in [",
              EH_MIN_BINS, ", ", EH_MAX_BINS, "], got ", n_bins);
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong &&
              state.dim() == 1 && state.is_contiguous() &&
              state.numel() == 4 * n_bins + 2 + EH_OUT,
              "state must be a contiguous int64 [4 * n_bins + 2 + ", EH_OUT,
              "] GPU tensor");
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(EH_FIN_THREADS), 0,
                     c10::hip::getCurrentHIPStream().stream(),
                     (long long*)state.data_ptr(), (int)n_bins);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
