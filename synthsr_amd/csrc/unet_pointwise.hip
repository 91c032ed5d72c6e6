// HBM-bound U-Net kernels (gfx950): ELU backward, BatchNorm (stats / apply / backward), fused
// BN+max-pool, fused BN+upsample+concat, 1x1x1 head + L1 loss, Keras-semantics Adam.
// NDHWC: a tensor is [nvox][C]; all kernels move float4 per lane (16 B x 64 lanes = 1 KiB per wave op).
//
// Channel reductions use 384-thread workgroups: every channel count of the U-Net (24..576, all
// multiples of 24) divided by 4 divides 96, so with a grid stride that is a multiple of 384 float4
// lanes each thread keeps a fixed group of 4 channels -> register partials, one LDS pass, one
// global atomic per (block, channel).
#include "common.h"

SYN_DET_SETTER(pointwise)

// workgroups of the channel-reduction kernels: every workgroup ends with one atomicAdd per channel sum on the SAME addresses,
// and same-address atomics serialise at the memory-side unit (~14 ns each): with 2048 workgroups the tail cost 0.6 ms per fp32
// step (29.36 -> 28.76 ms at 768 = 3 per CU; 512 and 1024 are within noise of it).  The grid-stride loops do the rest.
// The head kernels (one atomic per workgroup on the loss word) are insensitive between 256 and 1024.
static constexpr int red_grid() { return 768; }
static constexpr int head_grid() { return 1024; }

namespace {

constexpr int RB = 384;  // reduction block size (6 waves)

struct Shape3 {
  int d[3];
};

__device__ __forceinline__ float elu_grad_from_y(float y) { return y > 0.f ? 1.f : y + 1.f; }  // alpha = 1
// activation derivative through the output y: ELU (act 1) or, for the RELU instantiations (act 3), ReLU'(y) = 1 for y > 0
// else 0 (TF ReluGrad); a template parameter so that the ELU kernels stay the code they were
template <bool RELU>
__device__ __forceinline__ float act_grad_from_y(float y) {
  if constexpr (RELU) return y > 0.f ? 1.f : 0.f;
  else return elu_grad_from_y(y);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// bf16 activations (BASELINE configs[3] / [4]): the same kernels instantiated on bf16_t move 4 values = 8 bytes per lane and
// do all arithmetic (BatchNorm statistics, reductions, losses) in fp32; stores round to nearest even
struct bf16_t {
  uint16_t v;
};
__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ uint32_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ float4 ld4(const bf16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(bf2f(u.x & 0xffffu), bf2f(u.x >> 16), bf2f(u.y & 0xffffu), bf2f(u.y >> 16));
}
__device__ __forceinline__ void st4(bf16_t* p, float4 v) {
  uint2 u;
  u.x = f2bf(v.x) | (f2bf(v.y) << 16);
  u.y = f2bf(v.z) | (f2bf(v.w) << 16);
  *reinterpret_cast<uint2*>(p) = u;
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { p->v = (uint16_t)f2bf(v); }

// block-level channel reduction of NV float4 partials held by threads with a fixed channel group
template <int NV>
__device__ __forceinline__ void block_channel_reduce(float4 (&part)[NV], int c4, int C4, bool fixed, float* smem) {
  // smem: NV * C4 * 4 floats, zeroed by the caller before accumulation started
  if (fixed) {
    if (syn_det_on()) {
      // deterministic mode: the blockDim / C4 threads of a channel group add one after the other (LDS float atomics land
      // in arbitration order)
      const int rounds = (int)blockDim.x / C4, mine = (int)threadIdx.x / C4;
      for (int r = 0; r < rounds; ++r) {
        if (mine == r) {
#pragma unroll
          for (int k = 0; k < NV; ++k) {
            smem[(k * C4 + c4) * 4 + 0] += part[k].x;
            smem[(k * C4 + c4) * 4 + 1] += part[k].y;
            smem[(k * C4 + c4) * 4 + 2] += part[k].z;
            smem[(k * C4 + c4) * 4 + 3] += part[k].w;
          }
        }
        __syncthreads();
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      atomicAdd(&smem[(k * C4 + c4) * 4 + 0], part[k].x);
      atomicAdd(&smem[(k * C4 + c4) * 4 + 1], part[k].y);
      atomicAdd(&smem[(k * C4 + c4) * 4 + 2], part[k].z);
      atomicAdd(&smem[(k * C4 + c4) * 4 + 3], part[k].w);
    }
  }
  __syncthreads();
}

// one float per thread summed onto *slot (LDS; zeroed and synchronised by the caller).  Deterministic mode: wave butterflies,
// then the waves in order.  Workgroup-uniform call sites only.
__device__ __forceinline__ void block_scalar_add(float v, float* slot) {
  if (!syn_det_on()) {
    atomicAdd(slot, v);
    return;
  }
  __shared__ float wave_part[16];
  v = syn_wave_sum(v);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = *slot;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) t += wave_part[w];
    *slot = t;
  }
  __syncthreads();
}

// BatchNorm backward of one gradient value: gamma * invstd * (g - sum_dy / n - xhat * sum_dyxhat / n).  The roundings are spelled
// out (two fused multiply-adds, every other product rounded on its own) and contraction is off inside, so that every kernel that
// calls this gets the same bits from the same operands: left to the compiler, bn_pool_elu_bwd_kernel fused s0 * inv_n into the
// subtraction for the first voxel of a window and hoisted it as a rounded product for the other seven.
__device__ __forceinline__ float bn_bwd_map(float g, float xh, float gam, float inv, float s0, float s1, float inv_n) {
#pragma clang fp contract(off)
  const float t = fmaf(-(xh * s1), inv_n, fmaf(-s0, inv_n, g));
  return gam * inv * t;
}

// ------------------------------------------------------------------------------------------ ELU backward
// dz = (dy [+ dy2]) * elu'(y); dbias[c] += sum dz
// Optional fused BatchNorm backward (bn_sums != nullptr): the incoming gradient is w.r.t. the BN OUTPUT of y and is
// first mapped to the BN input, g <- gamma*invstd*(g - sum_dy/n - xhat*sum_dyxhat/n), saving one full pass.
template <typename T, bool RELU = false>
__global__ __launch_bounds__(RB) void elu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dy2,
                                                     const T* __restrict__ y, T* __restrict__ dz,
                                                     float* __restrict__ dbias, int64_t n4, int C4,
                                                     const float* __restrict__ bn_stats,
                                                     const float* __restrict__ bn_gamma,
                                                     const float* __restrict__ bn_sums, float eps, float inv_n,
                                                     const float* __restrict__ g1, const float* __restrict__ w1,
                                                     const float* __restrict__ drop = nullptr, int64_t n4ps = 0) {
  // drop != nullptr (feature-wise dropout with one mask per SAMPLE, batchsize > 1: KL.Dropout(noise_shape=[None,1,1,1,C]),
  // ext/neuron/models.py:320-324): y is the conv + ELU output, what followed it (the BatchNorm, or the next conv) read
  // d = s * y with s = drop[sample][c] (n4ps float4 per sample).  The incoming gradient is w.r.t. d (BatchNorm: w.r.t.
  // BN(d), xhat from s * y) and is multiplied by s; dy2 (the skip connection reads y itself) is added unscaled.
  extern __shared__ float smem[];
  const bool fixed = (RB % C4) == 0;
  if (dbias)
    for (int i = threadIdx.x; i < C4 * 4; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    float4 g;
    if (g1) {  // rank-1 gradient of the 1x1x1 head: dy[v][c] = g1[v] * w1[c], never materialised
      const float gv = g1[i / C4];
      const int c = (int)(i % C4) * 4;
      g = make_float4(gv * w1[c], gv * w1[c + 1], gv * w1[c + 2], gv * w1[c + 3]);
    } else {
      g = ld4(dy + i * 4);
    }
    const float4 a = ld4(y + i * 4);
    float4 sd = make_float4(1.f, 1.f, 1.f, 1.f);
    if (drop) sd = *reinterpret_cast<const float4*>(drop + (i / n4ps) * (C4 * 4) + (i % C4) * 4);
    if (bn_sums) {
      const int C = C4 * 4, c = (int)(i % C4) * 4;
      float gg[4] = {g.x, g.y, g.z, g.w};
      const float aa[4] = {a.x * sd.x, a.y * sd.y, a.z * sd.z, a.w * sd.w};  // the BatchNorm's input (sd = 1 without dropout)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float inv = rsqrtf(bn_stats[C + c + k] + eps);
        const float xh = (aa[k] - bn_stats[c + k]) * inv;
        gg[k] = bn_bwd_map(gg[k], xh, bn_gamma[c + k], inv, bn_sums[c + k], bn_sums[C + c + k], inv_n);
      }
      g = make_float4(gg[0], gg[1], gg[2], gg[3]);
    }
    if (drop) {
      g.x *= sd.x; g.y *= sd.y; g.z *= sd.z; g.w *= sd.w;
    }
    if (dy2) {
      const float4 g2 = ld4(dy2 + i * 4);
      g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
    }
    float4 r;
    r.x = g.x * act_grad_from_y<RELU>(a.x);
    r.y = g.y * act_grad_from_y<RELU>(a.y);
    r.z = g.z * act_grad_from_y<RELU>(a.z);
    r.w = g.w * act_grad_from_y<RELU>(a.w);
    st4(dz + i * 4, r);
    if (dbias) {
      if (fixed) {
        part[0].x += r.x; part[0].y += r.y; part[0].z += r.z; part[0].w += r.w;
      } else {
        const int c4 = (int)(i % C4);
        atomicAdd(&smem[c4 * 4 + 0], r.x);
        atomicAdd(&smem[c4 * 4 + 1], r.y);
        atomicAdd(&smem[c4 * 4 + 2], r.z);
        atomicAdd(&smem[c4 * 4 + 3], r.w);
      }
    }
  }
  if (dbias) {
    block_channel_reduce<1>(part, threadIdx.x % C4, C4, fixed, smem);
    if (syn_det_gather(smem, C4 * 4))
      for (int i = threadIdx.x; i < C4 * 4; i += RB) atomicAdd(&dbias[i], smem[i]);
    syn_det_gather_end(C4 * 4);
  }
}

// out[v][c] = x[v][c] * scale[sample(v)][c]: the dropped-out tensor of a batch with one feature mask per sample (and the same
// factor on a gradient); in place allowed
template <typename T>
__global__ __launch_bounds__(256) void scale_channels_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t n4,
                                                             int C4, const float* __restrict__ scale, int64_t n4ps) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = ld4(x + i * 4);
    const float4 sc = *reinterpret_cast<const float4*>(scale + (i / n4ps) * (C4 * 4) + (i % C4) * 4);
    st4(out + i * 4, make_float4(a.x * sc.x, a.y * sc.y, a.z * sc.z, a.w * sc.w));
  }
}

// ------------------------------------------------------------------------------------------ BN statistics
// Shifted data: the sums are those of x - k and (x - k)^2 with k[c] the mean of the channel's first (up to) 32 values, so that
// E[(x - k)^2] - E[x - k]^2 does not cancel when the mean dwarfs the spread (at mean 50, deviation 1 the fp32 squares ~2500
// each carried 1.5e-4 and the variance came back 7e-4 off); k lies inside the data, so |mean - k| is at most its range.
// Every workgroup and bn_stats_finalize_kernel, which adds k back to the mean, get k from bn_stats_shift: the same bits.
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(p->v); }
template <typename T>
__device__ __forceinline__ float bn_stats_shift(const T* __restrict__ x, int64_t nvox, int C, int c) {
  const int m = nvox < 32 ? (int)nvox : 32;
  float s = 0.f;
  for (int v = 0; v < m; ++v) s += ld1(x + (int64_t)v * C + c);
  return s / (float)m;
}
template <typename T>
__global__ __launch_bounds__(RB) void bn_stats_kernel(const T* __restrict__ x, int64_t n4, int C4,
                                                      double* __restrict__ ws) {
  extern __shared__ float smem[];  // [2][C4*4] sums, [C4*4] shift
  const bool fixed = (RB % C4) == 0;
  float* ks = smem + 2 * C4 * 4;
  for (int i = threadIdx.x; i < 2 * C4 * 4; i += RB) smem[i] = 0.f;
  for (int c = threadIdx.x; c < C4 * 4; c += RB) ks[c] = bn_stats_shift(x, n4 / C4, C4 * 4, c);
  __syncthreads();
  float4 part[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  const int64_t stride = (int64_t)gridDim.x * RB;
  const float4 kf = ld4(ks + (threadIdx.x % C4) * 4);  // fixed: a thread stays with one channel group
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    const float4 k = fixed ? kf : ld4(ks + (i % C4) * 4);
    float4 a = ld4(x + i * 4);
    a.x -= k.x; a.y -= k.y; a.z -= k.z; a.w -= k.w;
    if (fixed) {
      part[0].x += a.x; part[0].y += a.y; part[0].z += a.z; part[0].w += a.w;
      part[1].x += a.x * a.x; part[1].y += a.y * a.y; part[1].z += a.z * a.z; part[1].w += a.w * a.w;
    } else {
      const int c4 = (int)(i % C4);
      atomicAdd(&smem[c4 * 4 + 0], a.x);
      atomicAdd(&smem[c4 * 4 + 1], a.y);
      atomicAdd(&smem[c4 * 4 + 2], a.z);
      atomicAdd(&smem[c4 * 4 + 3], a.w);
      atomicAdd(&smem[(C4 + c4) * 4 + 0], a.x * a.x);
      atomicAdd(&smem[(C4 + c4) * 4 + 1], a.y * a.y);
      atomicAdd(&smem[(C4 + c4) * 4 + 2], a.z * a.z);
      atomicAdd(&smem[(C4 + c4) * 4 + 3], a.w * a.w);
    }
  }
  block_channel_reduce<2>(part, threadIdx.x % C4, C4, fixed, smem);
  if (syn_det_gather(smem, 2 * C4 * 4))
    for (int i = threadIdx.x; i < 2 * C4 * 4; i += RB) atomicAdd(&ws[i], (double)smem[i]);
  syn_det_gather_end(2 * C4 * 4);
}

template <typename T>
__global__ void bn_stats_finalize_kernel(const double* __restrict__ ws, const T* __restrict__ x, float* __restrict__ stats, int C,
                                         int64_t nvox) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const double inv_n = 1.0 / (double)nvox;
    const float k = bn_stats_shift(x, nvox, C, c);
    const double m = ws[c] * inv_n;  // mean and mean square of x - k
    double v = ws[C + c] * inv_n - m * m;
    if (v < 0.0) v = 0.0;
    stats[c] = (float)((double)k + m);
    stats[C + c] = (float)v;
  }
}

// per-channel affine of BN: y = x*sc + sh, sc = gamma*rsqrt(var+eps), sh = beta - mean*sc
__device__ __forceinline__ void bn_coeff(const float* stats, const float* gamma, const float* beta, float eps, int C,
                                         int c, float& sc, float& sh) {
  const float inv = rsqrtf(stats[C + c] + eps) * gamma[c];
  sc = inv;
  sh = beta[c] - stats[c] * inv;
}

__device__ __forceinline__ void bn_coeff4(const float* stats, const float* gamma, const float* beta, float eps, int C,
                                          int c, float4& sc, float4& sh) {
  bn_coeff(stats, gamma, beta, eps, C, c + 0, sc.x, sh.x);
  bn_coeff(stats, gamma, beta, eps, C, c + 1, sc.y, sh.y);
  bn_coeff(stats, gamma, beta, eps, C, c + 2, sc.z, sh.z);
  bn_coeff(stats, gamma, beta, eps, C, c + 3, sc.w, sh.w);
}

__device__ __forceinline__ float4 fma4(float4 a, float4 s, float4 h) {
  return make_float4(a.x * s.x + h.x, a.y * s.y + h.y, a.z * s.z + h.z, a.w * s.w + h.w);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n4,
                                                       int C, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps) {
  const int C4 = C / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    float4 sc, sh;
    bn_coeff4(stats, gamma, beta, eps, C, c, sc, sh);
    st4(y + i * 4, fma4(ld4(x + i * 4), sc, sh));
  }
}

// ------------------------------------------------------------------------------------------ BN + max-pool 2^3
template <typename T>
__global__ __launch_bounds__(256) void bn_maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, Shape3 s,
                                                         int C, const float* __restrict__ stats,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps) {
  const int C4 = C / 4;
  const int o0 = s.d[0] / 2, o1 = s.d[1] / 2, o2 = s.d[2] / 2;
  const int64_t n4 = (int64_t)o0 * o1 * o2 * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    const int p2 = (int)(v % o2);
    v /= o2;
    const int p1 = (int)(v % o1);
    const int p0 = (int)(v / o1);
    float4 sc, sh;
    bn_coeff4(stats, gamma, beta, eps, C, c, sc, sh);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int64_t vi = ((int64_t)(2 * p0 + a) * s.d[1] + (2 * p1 + b)) * s.d[2] + (2 * p2 + d);
          const float4 t = fma4(ld4(x + vi * C + c), sc, sh);
          m.x = fmaxf(m.x, t.x); m.y = fmaxf(m.y, t.y); m.z = fmaxf(m.z, t.z); m.w = fmaxf(m.w, t.w);
        }
    st4(y + i * 4, m);
  }
}

// gradient w.r.t. the BN output: routed to the FIRST maximum of each 2^3 window (raster order)
template <typename T>
__global__ __launch_bounds__(256) void bn_maxpool_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                             T* __restrict__ dbn, Shape3 s, int C,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps) {
  const int C4 = C / 4;
  const int o0 = s.d[0] / 2, o1 = s.d[1] / 2, o2 = s.d[2] / 2;
  const int64_t n4 = (int64_t)o0 * o1 * o2 * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    const int p2 = (int)(v % o2);
    v /= o2;
    const int p1 = (int)(v % o1);
    const int p0 = (int)(v / o1);
    float4 sc, sh;
    bn_coeff4(stats, gamma, beta, eps, C, c, sc, sh);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
      const float4 t = fma4(ld4(x + vi * C + c), sc, sh);
      if (t.x > m.x) { m.x = t.x; ax = k; }
      if (t.y > m.y) { m.y = t.y; ay = k; }
      if (t.z > m.z) { m.z = t.z; az = k; }
      if (t.w > m.w) { m.w = t.w; aw = k; }
    }
    const float4 g = ld4(dy + i * 4);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
      st4(dbn + vi * C + c, make_float4(ax == k ? g.x : 0.f, ay == k ? g.y : 0.f, az == k ? g.z : 0.f, aw == k ? g.w : 0.f));
    }
  }
}

// bn_maxpool_bwd + the channel sums of the NEXT BatchNorm backward (synthsr_bn_bwd_reduce of the routed gradient):
// the routed gradient is 7/8 zeros, every non-zero and its xhat are in registers here, so the separate reduction pass
// (a full read of dbn and x) is unnecessary.  RB threads so that each thread keeps a fixed channel group.
template <typename T>
__global__ __launch_bounds__(RB) void bn_maxpool_bwd_sums_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                 T* __restrict__ dbn, Shape3 s, int C,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 float* __restrict__ sums) {
  extern __shared__ float smem[];  // [2][C]
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  for (int i = threadIdx.x; i < 2 * C; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  const int o0 = s.d[0] / 2, o1 = s.d[1] / 2, o2 = s.d[2] / 2;
  const int64_t n4 = (int64_t)o0 * o1 * o2 * C4;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * RB) {
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    const int p2 = (int)(v % o2);
    v /= o2;
    const int p1 = (int)(v % o1);
    const int p0 = (int)(v / o1);
    float4 sc, sh;
    bn_coeff4(stats, gamma, beta, eps, C, c, sc, sh);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    float4 xa = make_float4(0.f, 0.f, 0.f, 0.f);  // raw input at the arg-max
    int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
      const float4 r = ld4(x + vi * C + c);
      const float4 t = fma4(r, sc, sh);
      if (t.x > m.x) { m.x = t.x; ax = k; xa.x = r.x; }
      if (t.y > m.y) { m.y = t.y; ay = k; xa.y = r.y; }
      if (t.z > m.z) { m.z = t.z; az = k; xa.z = r.z; }
      if (t.w > m.w) { m.w = t.w; aw = k; xa.w = r.w; }
    }
    const float4 g = ld4(dy + i * 4);
    if (dbn) {  // nullptr: the sums only -- the routed gradient is re-derived by bn_pool_elu_bwd_kernel
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
        st4(dbn + vi * C + c, make_float4(ax == k ? g.x : 0.f, ay == k ? g.y : 0.f, az == k ? g.z : 0.f, aw == k ? g.w : 0.f));
      }
    }
    float4 gx;  // g * xhat(arg-max)
    gx.x = g.x * (xa.x - stats[c + 0]) * rsqrtf(stats[C + c + 0] + eps);
    gx.y = g.y * (xa.y - stats[c + 1]) * rsqrtf(stats[C + c + 1] + eps);
    gx.z = g.z * (xa.z - stats[c + 2]) * rsqrtf(stats[C + c + 2] + eps);
    gx.w = g.w * (xa.w - stats[c + 3]) * rsqrtf(stats[C + c + 3] + eps);
    if (fixed) {
      part[0].x += g.x; part[0].y += g.y; part[0].z += g.z; part[0].w += g.w;
      part[1].x += gx.x; part[1].y += gx.y; part[1].z += gx.z; part[1].w += gx.w;
    } else {
      atomicAdd(&smem[c + 0], g.x); atomicAdd(&smem[c + 1], g.y);
      atomicAdd(&smem[c + 2], g.z); atomicAdd(&smem[c + 3], g.w);
      atomicAdd(&smem[C + c + 0], gx.x); atomicAdd(&smem[C + c + 1], gx.y);
      atomicAdd(&smem[C + c + 2], gx.z); atomicAdd(&smem[C + c + 3], gx.w);
    }
  }
  block_channel_reduce<2>(part, threadIdx.x % C4, C4, fixed, smem);
  if (syn_det_gather(smem, 2 * C))
    for (int i = threadIdx.x; i < 2 * C; i += RB) atomicAdd(&sums[i], smem[i]);
  syn_det_gather_end(2 * C);
}

// MaxPooling3D backward + BatchNormalization backward (pass 2) + ELU backward of an encoder level in ONE pass
// (ext/neuron/models.py:316-356: conv + ELU -> BatchNormalization -> MaxPooling3D): dz = (BN'(route(dpool)) + dy2) * ELU'(y).
// The gradient routed to the arg-max of every 2x2x2 window is 7/8 zeros; writing it out (bn_maxpool_bwd) and reading it back
// (elu_bwd) cost one write + one read of the level's largest tensor (2 x 393 MB at 160^3 x 24).  Here each thread owns a
// pooling window x 4 channels: it re-derives the arg-max from y (same arithmetic as bn_maxpool_kernel: first maximum in
// raster order of y * sc + sh), applies g <- gamma * invstd * (g - sum_dy / n - xhat * sum_dyxhat / n) to all 8 voxels
// (sums from bn_maxpool_bwd_sums_kernel with dbn = nullptr), adds the skip connection's gradient dy2 and multiplies by
// ELU'(y); dbias += sum dz.
template <typename T, bool RELU = false>
__global__ __launch_bounds__(RB) void bn_pool_elu_bwd_kernel(const T* __restrict__ dpool, const T* __restrict__ y,
                                                             const T* __restrict__ dy2, T* __restrict__ dz,
                                                             float* __restrict__ dbias, Shape3 s, int C,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ sums, float eps, float inv_n) {
  extern __shared__ float smem[];  // [C]
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  if (dbias)
    for (int i = threadIdx.x; i < C; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  const int o0 = s.d[0] / 2, o1 = s.d[1] / 2, o2 = s.d[2] / 2;
  const int64_t n4 = (int64_t)o0 * o1 * o2 * C4;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * RB) {
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    const int p2 = (int)(v % o2);
    v /= o2;
    const int p1 = (int)(v % o1);
    const int p0 = (int)(v / o1);
    float4 sc, sh;
    bn_coeff4(stats, gamma, beta, eps, C, c, sc, sh);
    float mean[4], inv[4], gam[4], s0[4], s1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mean[k] = stats[c + k];
      inv[k] = rsqrtf(stats[C + c + k] + eps);
      gam[k] = gamma[c + k];
      s0[k] = sums[c + k];
      s1[k] = sums[C + c + k];
    }
    float4 r[8];
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
      r[k] = ld4(y + vi * C + c);
      const float4 t = fma4(r[k], sc, sh);
      if (t.x > m.x) { m.x = t.x; ax = k; }
      if (t.y > m.y) { m.y = t.y; ay = k; }
      if (t.z > m.z) { m.z = t.z; az = k; }
      if (t.w > m.w) { m.w = t.w; aw = k; }
    }
    const float4 g = ld4(dpool + i * 4);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
      float gg[4] = {ax == k ? g.x : 0.f, ay == k ? g.y : 0.f, az == k ? g.z : 0.f, aw == k ? g.w : 0.f};
      const float aa[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float xh = (aa[q] - mean[q]) * inv[q];
        gg[q] = bn_bwd_map(gg[q], xh, gam[q], inv[q], s0[q], s1[q], inv_n);  // as elu_bwd_kernel, bit for bit
      }
      if (dy2) {
        const float4 g2 = ld4(dy2 + vi * C + c);
        gg[0] += g2.x; gg[1] += g2.y; gg[2] += g2.z; gg[3] += g2.w;
      }
      float4 o;
      o.x = gg[0] * act_grad_from_y<RELU>(aa[0]);
      o.y = gg[1] * act_grad_from_y<RELU>(aa[1]);
      o.z = gg[2] * act_grad_from_y<RELU>(aa[2]);
      o.w = gg[3] * act_grad_from_y<RELU>(aa[3]);
      st4(dz + vi * C + c, o);
      if (dbias) {
        if (fixed) {
          part[0].x += o.x; part[0].y += o.y; part[0].z += o.z; part[0].w += o.w;
        } else {
          atomicAdd(&smem[c + 0], o.x);
          atomicAdd(&smem[c + 1], o.y);
          atomicAdd(&smem[c + 2], o.z);
          atomicAdd(&smem[c + 3], o.w);
        }
      }
    }
  }
  if (dbias) {
    block_channel_reduce<1>(part, threadIdx.x % C4, C4, fixed, smem);
    if (syn_det_gather(smem, C))
      for (int i = threadIdx.x; i < C; i += RB) atomicAdd(&dbias[i], smem[i]);
    syn_det_gather_end(C);
  }
}

// ------------------------------------------------------------------------------------------ BN backward
template <typename T>
__global__ __launch_bounds__(RB) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           int64_t n4, int C, const float* __restrict__ stats,
                                                           float eps, float* __restrict__ sums) {
  extern __shared__ float smem[];  // [2][C]
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  for (int i = threadIdx.x; i < 2 * C; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % C4) * 4;
    const float4 g = ld4(dy + i * 4);
    const float4 a = ld4(x + i * 4);
    float4 xh;
    xh.x = (a.x - stats[c + 0]) * rsqrtf(stats[C + c + 0] + eps);
    xh.y = (a.y - stats[c + 1]) * rsqrtf(stats[C + c + 1] + eps);
    xh.z = (a.z - stats[c + 2]) * rsqrtf(stats[C + c + 2] + eps);
    xh.w = (a.w - stats[c + 3]) * rsqrtf(stats[C + c + 3] + eps);
    if (fixed) {
      part[0].x += g.x; part[0].y += g.y; part[0].z += g.z; part[0].w += g.w;
      part[1].x += g.x * xh.x; part[1].y += g.y * xh.y; part[1].z += g.z * xh.z; part[1].w += g.w * xh.w;
    } else {
      atomicAdd(&smem[c + 0], g.x); atomicAdd(&smem[c + 1], g.y);
      atomicAdd(&smem[c + 2], g.z); atomicAdd(&smem[c + 3], g.w);
      atomicAdd(&smem[C + c + 0], g.x * xh.x); atomicAdd(&smem[C + c + 1], g.y * xh.y);
      atomicAdd(&smem[C + c + 2], g.z * xh.z); atomicAdd(&smem[C + c + 3], g.w * xh.w);
    }
  }
  block_channel_reduce<2>(part, threadIdx.x % C4, C4, fixed, smem);
  if (syn_det_gather(smem, 2 * C))
    for (int i = threadIdx.x; i < 2 * C; i += RB) atomicAdd(&sums[i], smem[i]);
  syn_det_gather_end(2 * C);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           float* __restrict__ dx, int64_t n4, int C,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, float eps,
                                                           const float* __restrict__ sums, float inv_n) {
  const int C4 = C / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const float4 g = ld4(dy + i * 4);
    const float4 a = ld4(x + i * 4);
    float r[4];
    const float gg[4] = {g.x, g.y, g.z, g.w}, aa[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float inv = rsqrtf(stats[C + c + k] + eps);
      const float xh = (aa[k] - stats[c + k]) * inv;
      r[k] = gamma[c + k] * inv * (gg[k] - sums[c + k] * inv_n - xh * sums[C + c + k] * inv_n);
    }
    st4(dx + i * 4, make_float4(r[0], r[1], r[2], r[3]));
  }
}

// ------------------------------------------------------------------------------------------ upsample + concat
template <typename T>
__global__ __launch_bounds__(256) void upsample_concat_kernel(const T* __restrict__ skip,
                                                              const T* __restrict__ lo, T* __restrict__ out,
                                                              Shape3 s, int Cs, int Cl,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps) {
  const int C = Cs + Cl, C4 = C / 4;
  const int64_t n4 = (int64_t)s.d[0] * s.d[1] * s.d[2] * C4;
  const int l1 = s.d[1] / 2, l2 = s.d[2] / 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    float4 r;
    if (c < Cs) {
      r = ld4(skip + v * Cs + c);
    } else {
      const int i2 = (int)(v % s.d[2]);
      const int i1 = (int)((v / s.d[2]) % s.d[1]);
      const int i0 = (int)(v / ((int64_t)s.d[2] * s.d[1]));
      const int64_t lv = ((int64_t)(i0 >> 1) * l1 + (i1 >> 1)) * l2 + (i2 >> 1);
      float4 sc, sh;
      bn_coeff4(stats, gamma, beta, eps, Cl, c - Cs, sc, sh);
      r = fma4(ld4(lo + lv * Cl + (c - Cs)), sc, sh);
    }
    st4(out + i * 4, r);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void upsample_concat_bwd_kernel(const T* __restrict__ dcat,
                                                                  T* __restrict__ dskip,
                                                                  T* __restrict__ dlo, Shape3 s, int Cs, int Cl) {
  const int C = Cs + Cl;
  const int Cs4 = Cs / 4, Cl4 = Cl / 4;
  const int64_t nv = (int64_t)s.d[0] * s.d[1] * s.d[2];
  const int l0 = s.d[0] / 2, l1 = s.d[1] / 2, l2 = s.d[2] / 2;
  const int64_t nskip4 = nv * Cs4;
  const int64_t nlo4 = (int64_t)l0 * l1 * l2 * Cl4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nskip4 + nlo4;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nskip4) {
      const int c = (int)(i % Cs4) * 4;
      const int64_t v = i / Cs4;
      st4(dskip + v * Cs + c, ld4(dcat + v * C + c));
    } else {
      const int64_t j = i - nskip4;
      const int c = (int)(j % Cl4) * 4;
      int64_t v = j / Cl4;
      const int p2 = (int)(v % l2);
      v /= l2;
      const int p1 = (int)(v % l1);
      const int p0 = (int)(v / l1);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t vi = ((int64_t)(2 * p0 + (k >> 2)) * s.d[1] + (2 * p1 + ((k >> 1) & 1))) * s.d[2] + (2 * p2 + (k & 1));
        const float4 t = ld4(dcat + vi * C + Cs + c);
        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
      }
      st4(dlo + j * 4, acc);
    }
  }
}

// ------------------------------------------------------------------------------------------ head + regression loss
// unet_likelihood (1x1x1 conv on the last BatchNorm output, K output channels) + the loss of SynthSR/metrics_model.py:30-132
// with n regression targets (training(output_channel=[...]), target [nvox][n]):
//   kind 0  'l1'      mean |pred - target|                          (K = n)
//   kind 1  'l2'      mean (pred - target)^2                        (K = n)
//   kind 2  'laplace' mean( log(2 b) + |pred_k - target_k| / b ),  b = 1e-5 + 0.02 exp(pred_{n+k})     (K = 2 n)
// (means over voxels AND target channels, like K.mean in the reference)
// optionally evaluated on a centred box only (loss_cropping, metrics_model.py:70-90): voxels outside contribute neither
// loss nor gradient; inv_n = 1 / (voxels inside).  dpred [nvox][K] is the loss gradient w.r.t. pred.
struct HeadBox {
  int on, d1, d2;
  int lo[3], hi[3];
  int res_off[16];  // residual channel added to intensity channel k (work_with_residual_channel)
};

// CT = 24 (round 6): the 24-feature head of the benchmark network keeps the 72 BatchNorm / head coefficients of its dot product in
// SCALAR registers (readfirstlane: the values are uniform) instead of reading them from LDS per voxel -- 72 broadcast ds_read_b32
// per voxel and pass -- and requests the next 256-voxel slab before it computes on the current one: 0.184 -> 0.153 ms at 160^3
// (2.1 -> 2.6 TB/s; profiles/r06_head_kernel_ab.txt; the VGPR form of the same idea needs 189 registers and is slower).  Same
// products in the same order; the compiler's fma contraction may differ in the last bit.  CT = 0: any channel count, LDS.
template <typename T, int K, int CT = 0>
__global__ __launch_bounds__(256) void head_loss_fwd_kernel(const T* __restrict__ x, int64_t nvox, int C,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ residual, int rs,
                                                            const float* __restrict__ target, float* __restrict__ pred,
                                                            float* __restrict__ dpred, float* __restrict__ loss,
                                                            float inv_n, int kind, HeadBox box, float* __restrict__ ab) {
  // ab != nullptr (K == 1): also the two sums the backward pass of this head needs, A[c] = sum_v g[v] xhat[v][c] and
  // B = sum_v g[v] with g = d loss / d pred (ab[0 .. C) += A, ab[C] += B): the gradient w.r.t. the BatchNorm output is rank-1
  // (g[v] w[c]), so head-weight gradients and that BatchNorm's backward sums are linear in (A, B) (head_ab_finish_kernel) and
  // the separate pass over the last feature map (head_bwd_kernel, 393 MB at 160^3) is not needed.
  constexpr int NTMAX = K;
  const int NT = kind == 2 ? K / 2 : K;  // regression targets
  extern __shared__ float smem[];  // scale[C], shift[C], w[C][K], then the voxel tile
  float* weff = smem;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float sc, sh;
    bn_coeff(stats, gamma, beta, eps, C, c, sc, sh);
    weff[c] = sc;         // keep scale and shift separately: pred accumulates w*(x*sc+sh) like the unfused graph
    weff[C + c] = sh;
#pragma unroll
    for (int k = 0; k < K; ++k) weff[2 * C + k * C + c] = w[c * K + k];
  }
  __syncthreads();
  constexpr int CR = (CT > 0 && K == 1) ? CT : 1;
  float rsc[CR], rsh[CR], rw[CR];
  if constexpr (CT > 0 && K == 1) {
#pragma unroll
    for (int c = 0; c < CR; ++c) {
      rsc[c] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, weff[c])));       // scalar
      rsh[c] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, weff[C + c])));   // registers
      rw[c] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, weff[2 * C + c])));
    }
  }
  float lsum = 0.f;
  // second phase of a pass (ab): thread = (channel quad qa, voxel lane la); la walks the tile's voxels with stride LA
  __shared__ float gl[256];
  const int C4h = C / 4, LA = 256 / C4h;
  const int qa = (int)threadIdx.x % C4h, la = (int)threadIdx.x / C4h;
  float4 apart[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  float bsum = 0.f;
  float amean[4] = {0.f, 0.f, 0.f, 0.f}, ainv[4] = {0.f, 0.f, 0.f, 0.f};
  if (ab) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      amean[k] = stats[qa * 4 + k];
      ainv[k] = rsqrtf(stats[C + qa * 4 + k] + eps);
    }
  }
  // 256 voxels per pass: the [256][C] slab is contiguous in memory -> coalesced float4 loads into an LDS tile with rows
  // padded to C+4 floats (conflict-free 16-byte reads), then one thread per voxel (thread-per-voxel global loads touch 48
  // cache lines per instruction and ran at 1.7 TB/s)
  float* tile = smem + (2 + K) * C;
  const int C4 = C / 4, CP = C + 4;
  // round 6: the slab of the NEXT pass is requested (registers) before this pass computes, so that the loads of a workgroup
  // are in flight during its two compute phases instead of being waited for between three barriers
  constexpr int PF = 8;                 // float4 per thread of a prefetched slab: C <= 32
  const bool prefetch = C4 <= PF;
  float4 nxt[PF];
  auto fetch = [&](int64_t v0n) {
    const int nvn = v0n < nvox ? (int)min((int64_t)256, nvox - v0n) : 0;
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int i = (int)threadIdx.x + 256 * k;
      if (k < C4 && i < nvn * C4) nxt[k] = ld4(x + v0n * C + (int64_t)i * 4);
    }
  };
  if (prefetch) fetch((int64_t)blockIdx.x * 256);
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < nvox; v0 += (int64_t)gridDim.x * 256) {
    const int nv = (int)min((int64_t)256, nvox - v0);
    __syncthreads();
    if (prefetch) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (k < C4 && i < nv * C4) {
          const int vl = i / C4, q = i - vl * C4;
          *reinterpret_cast<float4*>(&tile[vl * CP + q * 4]) = nxt[k];
        }
      }
      fetch(v0 + (int64_t)gridDim.x * 256);
    } else {
      for (int i = threadIdx.x; i < nv * C4; i += 256) {
        const int vl = i / C4, q = i - vl * C4;
        *reinterpret_cast<float4*>(&tile[vl * CP + q * 4]) = ld4(x + v0 * C + (int64_t)i * 4);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
      const int64_t v = v0 + threadIdx.x;
      float acc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = 0.f;
      const float* xp = tile + threadIdx.x * CP;
      if constexpr (CT > 0 && K == 1) {
#pragma unroll
        for (int c = 0; c < CR; c += 4) {
          const float4 a = *reinterpret_cast<const float4*>(xp + c);
          const float n0 = a.x * rsc[c + 0] + rsh[c + 0], n1 = a.y * rsc[c + 1] + rsh[c + 1];
          const float n2 = a.z * rsc[c + 2] + rsh[c + 2], n3 = a.w * rsc[c + 3] + rsh[c + 3];
          acc[0] += rw[c + 0] * n0;
          acc[0] += rw[c + 1] * n1;
          acc[0] += rw[c + 2] * n2;
          acc[0] += rw[c + 3] * n3;
        }
      } else
      for (int c = 0; c < C; c += 4) {
        const float4 a = *reinterpret_cast<const float4*>(xp + c);
        const float n0 = a.x * weff[c + 0] + weff[C + c + 0], n1 = a.y * weff[c + 1] + weff[C + c + 1];
        const float n2 = a.z * weff[c + 2] + weff[C + c + 2], n3 = a.w * weff[c + 3] + weff[C + c + 3];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float* wk = weff + 2 * C + k * C + c;
          acc[k] += wk[0] * n0;
          acc[k] += wk[1] * n1;
          acc[k] += wk[2] * n2;
          acc[k] += wk[3] * n3;
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += b[k];
      if (residual) {
#pragma unroll
        for (int k = 0; k < NTMAX; ++k)
          if (k < NT) acc[k] += residual[v * rs + box.res_off[k]];
      }
      if (pred) {
#pragma unroll
        for (int k = 0; k < K; ++k) pred[v * K + k] = acc[k];
      }
      bool inside = true;
      if (box.on) {
        const int xx = (int)(v % box.d2), yy = (int)((v / box.d2) % box.d1), zz = (int)(v / ((int64_t)box.d1 * box.d2));
        inside = zz >= box.lo[0] && zz < box.hi[0] && yy >= box.lo[1] && yy < box.hi[1] && xx >= box.lo[2] && xx < box.hi[2];
      }
      float g[K];
#pragma unroll
      for (int k = 0; k < K; ++k) g[k] = 0.f;
      if (inside) {
#pragma unroll
        for (int k = 0; k < NTMAX; ++k) {
          if (k >= NT) continue;
          const float e = acc[k] - target[v * NT + k];
          const float sgn = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
          if (kind == 2) {  // laplace: spread channel NT + k
            if constexpr (K >= 2) {
              const int ks = (K / 2) + k;  // == NT + k
              const float ex = 0.02f * expf(acc[ks < K ? ks : 0]), bb = 1e-5f + ex, ib = 1.f / bb;
              lsum += logf(2.f * bb) + fabsf(e) * ib;
              g[k] = sgn * ib * inv_n;
              g[ks < K ? ks : 0] = (ib - fabsf(e) * ib * ib) * ex * inv_n;
            }
          } else if (kind == 1) {
            lsum += e * e;
            g[k] = 2.f * e * inv_n;
          } else {
            lsum += fabsf(e);
            g[k] = sgn * inv_n;
          }
        }
      }
      if (dpred) {
#pragma unroll
        for (int k = 0; k < K; ++k) dpred[v * K + k] = g[k];
      }
      if (ab) {
        gl[threadIdx.x] = g[0];
        bsum += g[0];
      }
    }
    if (ab) {
      __syncthreads();
      if (la < LA) {
        for (int vl = la; vl < nv; vl += LA) {
          const float gv = gl[vl];
          const float4 a = *reinterpret_cast<const float4*>(tile + vl * CP + qa * 4);
          apart[0].x += gv * ((a.x - amean[0]) * ainv[0]);
          apart[0].y += gv * ((a.y - amean[1]) * ainv[1]);
          apart[0].z += gv * ((a.z - amean[2]) * ainv[2]);
          apart[0].w += gv * ((a.w - amean[3]) * ainv[3]);
        }
      }
    }
  }
  // one atomic per BLOCK on the single loss word: 16k same-address atomics (one per wave of a 4096-block grid) used to
  // serialise into ~0.15 ms
  lsum = syn_wave_sum(lsum);
  __shared__ float wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) wsum[0] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * inv_n;
  __syncthreads();
  if (!ab) {
    if (syn_det_gather(wsum, 1))
      if (threadIdx.x == 0) atomicAdd(loss, wsum[0]);
    syn_det_gather_end(1);
    return;
  }
  // one row [A (C) | B | loss] per workgroup: ONE gather (two in a row would mix their arrival counts)
  __shared__ float row[128];
  for (int i = threadIdx.x; i < C + 2; i += 256) row[i] = 0.f;
  __syncthreads();
  block_scalar_add(bsum, &row[C]);
  if (la >= LA) apart[0] = make_float4(0.f, 0.f, 0.f, 0.f);
  block_channel_reduce<1>(apart, qa, C4h, true, row);
  if (threadIdx.x == 0) row[C + 1] = wsum[0];
  __syncthreads();
  if (syn_det_gather(row, C + 2)) {
    for (int i = threadIdx.x; i < C + 1; i += 256) atomicAdd(&ab[i], row[i]);
    if (threadIdx.x == 0) atomicAdd(loss, row[C + 1]);
  }
  syn_det_gather_end(C + 2);
}

// backward of the 1-channel head from the sums of head_loss_fwd_kernel (see there): dw = gamma A + beta B, db = B, and the
// BatchNorm-backward sums of the rank-1 gradient g[v] w[c]: sum = w B, sum * xhat = w A
__global__ void head_ab_finish_kernel(const float* __restrict__ ab, int C, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, const float* __restrict__ w, float* __restrict__ dw,
                                      float* __restrict__ db, float* __restrict__ sums) {
  const float B = ab[C];
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    const float A = ab[i];
    dw[i] += gamma[i] * A + beta[i] * B;
    if (sums) {
      sums[i] += w[i] * B;
      sums[C + i] += w[i] * A;
    }
  }
  if (threadIdx.x == 0) *db += B;
}

// K-channel head backward (K > 1, e.g. the intensity + spread channels of the 'laplace' loss): the gradient w.r.t. the
// BatchNorm output, dbn[v][c] = sum_k g[v][k] w[c][k], is written out; dw[c][k] += gamma[c] A_k[c] + beta[c] B_k,
// db[k] += B_k with A_k[c] = sum_v g_k xhat[v][c], B_k = sum_v g_k.
template <typename T, int K>
__global__ __launch_bounds__(RB) void head_multi_bwd_kernel(const float* __restrict__ dpred, const T* __restrict__ x,
                                                            int64_t n4, int C, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps,
                                                            const float* __restrict__ w, T* __restrict__ dbn,
                                                            float* __restrict__ dw, float* __restrict__ db) {
  extern __shared__ float smem[];  // A[K][C], B[K]
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  for (int i = threadIdx.x; i < K * C + K; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[K];
  float dbp[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    part[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    dbp[k] = 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    const float4 a = ld4(x + i * 4);
    float4 xh;
    xh.x = (a.x - stats[c + 0]) * rsqrtf(stats[C + c + 0] + eps);
    xh.y = (a.y - stats[c + 1]) * rsqrtf(stats[C + c + 1] + eps);
    xh.z = (a.z - stats[c + 2]) * rsqrtf(stats[C + c + 2] + eps);
    xh.w = (a.w - stats[c + 3]) * rsqrtf(stats[C + c + 3] + eps);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float g = dpred[v * K + k];
      d.x += g * w[(c + 0) * K + k]; d.y += g * w[(c + 1) * K + k];
      d.z += g * w[(c + 2) * K + k]; d.w += g * w[(c + 3) * K + k];
      if (fixed) {
        part[k].x += g * xh.x; part[k].y += g * xh.y; part[k].z += g * xh.z; part[k].w += g * xh.w;
      } else {
        atomicAdd(&smem[k * C + c + 0], g * xh.x); atomicAdd(&smem[k * C + c + 1], g * xh.y);
        atomicAdd(&smem[k * C + c + 2], g * xh.z); atomicAdd(&smem[k * C + c + 3], g * xh.w);
      }
      if (c == 0) dbp[k] += g;
    }
    st4(dbn + i * 4, d);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) block_scalar_add(dbp[k], &smem[K * C + k]);
  block_channel_reduce<K>(part, threadIdx.x % C4, C4, fixed, smem);
  if (syn_det_gather(smem, K * C + K)) {
    for (int i = threadIdx.x; i < C * K; i += RB) {
      const int c = i / K, k = i - c * K;
      atomicAdd(&dw[i], gamma[c] * smem[k * C + c] + beta[c] * smem[K * C + k]);
    }
    if (threadIdx.x < K) atomicAdd(&db[threadIdx.x], smem[K * C + threadIdx.x]);
  }
  syn_det_gather_end(K * C + K);
}

// ------------------------------------------------------------------------------------------ wide heads (5 <= K <= 16)
// training(output_channel=[...]) with five or more l1 / l2 targets, or three or more 'laplace' targets (intensity + spread
// channel each).  Two padded widths KB in {8, 16} serve every K <= KB at run time: the per-voxel arrays have KB elements and are
// indexed statically (registers, no scratch); the weight and bias slots k >= K are zero in LDS, so the padded lanes compute
// zeros, and every access to pred / dpred / target / residual is guarded by the real K.  Same contracts, same order of the
// products and the same deterministic-mode gather (of the real K C + K values) as the K <= 4 kernels above.

// a[k] <- a[k + s] (zeros shifted in), 0 <= s < N: a barrel shifter of wave-uniform steps, so that the spread channel NT + k of
// a 'laplace' head with a run-time number of targets NT is reached without a dynamic register index
template <int N>
__device__ __forceinline__ void shift_down(float (&a)[N], int s) {
#pragma unroll
  for (int bit = 1; bit < N; bit <<= 1) {
    if (s & bit) {
#pragma unroll
      for (int k = 0; k < N; ++k) a[k] = (k + bit < N) ? a[k + bit] : 0.f;
    }
  }
}
// a[k] <- a[k - s]
template <int N>
__device__ __forceinline__ void shift_up(float (&a)[N], int s) {
#pragma unroll
  for (int bit = 1; bit < N; bit <<= 1) {
    if (s & bit) {
#pragma unroll
      for (int k = N - 1; k >= 0; --k) a[k] = (k - bit >= 0) ? a[k - bit] : 0.f;
    }
  }
}

// head_loss_fwd_kernel for K <= KB channels.  vec4: K % 4 == 0 and pred / dpred are 16-byte aligned -- a voxel's K values
// are then stored as float4.  Dynamic LDS: scale[C], shift[C], w[KB][C], b[KB], then the voxel tile.
template <typename T, int KB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void head_loss_fwd_wide_kernel(const T* __restrict__ x, int64_t nvox, int C,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 const float* __restrict__ w, const float* __restrict__ b,
                                                                 int K, const float* __restrict__ residual, int rs,
                                                                 const float* __restrict__ target,
                                                                 float* __restrict__ pred, float* __restrict__ dpred,
                                                                 float* __restrict__ loss, float inv_n, int kind,
                                                                 HeadBox box, int vec4) {
  const int NT = kind == 2 ? K / 2 : K;  // regression targets
  extern __shared__ float smem[];
  float* weff = smem;
  float* wl = smem + 2 * C;
  float* bl = wl + KB * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float sc, sh;
    bn_coeff(stats, gamma, beta, eps, C, c, sc, sh);
    weff[c] = sc;
    weff[C + c] = sh;
#pragma unroll
    for (int k = 0; k < KB; ++k) wl[k * C + c] = k < K ? w[c * K + k] : 0.f;
  }
  if ((int)threadIdx.x < KB) bl[threadIdx.x] = (int)threadIdx.x < K ? b[threadIdx.x] : 0.f;
  __syncthreads();
  float lsum = 0.f;
  float* tile = bl + KB;
  const int C4 = C / 4, CP = C + 4;
  constexpr int PF = 8;  // float4 per thread of a prefetched slab (see head_loss_fwd_kernel)
  const bool prefetch = C4 <= PF;
  float4 nxt[PF];
  auto fetch = [&](int64_t v0n) {
    const int nvn = v0n < nvox ? (int)min((int64_t)256, nvox - v0n) : 0;
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int i = (int)threadIdx.x + 256 * k;
      if (k < C4 && i < nvn * C4) nxt[k] = ld4(x + v0n * C + (int64_t)i * 4);
    }
  };
  if (prefetch) fetch((int64_t)blockIdx.x * 256);
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < nvox; v0 += (int64_t)gridDim.x * 256) {
    const int nv = (int)min((int64_t)256, nvox - v0);
    __syncthreads();
    if (prefetch) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (k < C4 && i < nv * C4) {
          const int vl = i / C4, q = i - vl * C4;
          *reinterpret_cast<float4*>(&tile[vl * CP + q * 4]) = nxt[k];
        }
      }
      fetch(v0 + (int64_t)gridDim.x * 256);
    } else {
      for (int i = threadIdx.x; i < nv * C4; i += 256) {
        const int vl = i / C4, q = i - vl * C4;
        *reinterpret_cast<float4*>(&tile[vl * CP + q * 4]) = ld4(x + v0 * C + (int64_t)i * 4);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
      const int64_t v = v0 + threadIdx.x;
      float acc[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) acc[k] = 0.f;
      const float* xp = tile + threadIdx.x * CP;
#pragma unroll 1
      for (int c = 0; c < C; c += 4) {  // (not unrolled: 4 KB independent products per trip already)
        const float4 a = *reinterpret_cast<const float4*>(xp + c);
        const float n0 = a.x * weff[c + 0] + weff[C + c + 0], n1 = a.y * weff[c + 1] + weff[C + c + 1];
        const float n2 = a.z * weff[c + 2] + weff[C + c + 2], n3 = a.w * weff[c + 3] + weff[C + c + 3];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const float4 wk = *reinterpret_cast<const float4*>(wl + k * C + c);
          acc[k] += wk.x * n0;
          acc[k] += wk.y * n1;
          acc[k] += wk.z * n2;
          acc[k] += wk.w * n3;
        }
      }
#pragma unroll
      for (int k = 0; k < KB; ++k) acc[k] += bl[k];
      if (residual) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
          if (k < NT) acc[k] += residual[v * rs + box.res_off[k]];
      }
      if (pred) {
        if (vec4) {
#pragma unroll
          for (int k = 0; k < KB; k += 4)
            if (k < K) st4(pred + v * K + k, make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]));
        } else {
#pragma unroll
          for (int k = 0; k < KB; ++k)
            if (k < K) pred[v * K + k] = acc[k];
        }
      }
      bool inside = true;
      if (box.on) {
        const int xx = (int)(v % box.d2), yy = (int)((v / box.d2) % box.d1), zz = (int)(v / ((int64_t)box.d1 * box.d2));
        inside = zz >= box.lo[0] && zz < box.hi[0] && yy >= box.lo[1] && yy < box.hi[1] && xx >= box.lo[2] && xx < box.hi[2];
      }
      float g[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) g[k] = 0.f;
      if (inside) {
        if (kind == 2) {  // laplace: the spread of target k is channel NT + k
          float sp[KB], gs[KB];
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            sp[k] = acc[k];
            gs[k] = 0.f;
          }
          shift_down<KB>(sp, NT);
#pragma unroll
          for (int k = 0; k < KB / 2; ++k) {
            if (k < NT) {
              const float e = acc[k] - target[v * NT + k];
              const float sgn = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
              const float ex = 0.02f * expf(sp[k]), bb = 1e-5f + ex, ib = 1.f / bb;
              lsum += logf(2.f * bb) + fabsf(e) * ib;
              g[k] = sgn * ib * inv_n;
              gs[k] = (ib - fabsf(e) * ib * ib) * ex * inv_n;
            }
          }
          shift_up<KB>(gs, NT);
#pragma unroll
          for (int k = 0; k < KB; ++k)
            if (k >= NT) g[k] = gs[k];
        } else {
#pragma unroll
          for (int k = 0; k < KB; ++k) {
            if (k < NT) {
              const float e = acc[k] - target[v * NT + k];
              if (kind == 1) {
                lsum += e * e;
                g[k] = 2.f * e * inv_n;
              } else {
                lsum += fabsf(e);
                g[k] = (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) * inv_n;
              }
            }
          }
        }
      }
      if (dpred) {
        if (vec4) {
#pragma unroll
          for (int k = 0; k < KB; k += 4)
            if (k < K) st4(dpred + v * K + k, make_float4(g[k], g[k + 1], g[k + 2], g[k + 3]));
        } else {
#pragma unroll
          for (int k = 0; k < KB; ++k)
            if (k < K) dpred[v * K + k] = g[k];
        }
      }
    }
  }
  // one atomic per workgroup on the loss word, as in head_loss_fwd_kernel
  lsum = syn_wave_sum(lsum);
  __shared__ float wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) wsum[0] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * inv_n;
  __syncthreads();
  if (syn_det_gather(wsum, 1))
    if (threadIdx.x == 0) atomicAdd(loss, wsum[0]);
  syn_det_gather_end(1);
}

// head_multi_bwd_kernel for K <= KB channels.  vec4: K % 4 == 0 and dpred is 16-byte aligned.  Dynamic LDS: A[KB][C], B[KB],
// then the head weights as w[KB][C] (one 16-byte read per channel quad and k; rows k >= K zero).
template <typename T, int KB>
__global__ __launch_bounds__(RB) void head_multi_bwd_wide_kernel(const float* __restrict__ dpred, const T* __restrict__ x,
                                                                 int64_t n4, int C, int K, const float* __restrict__ stats,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 const float* __restrict__ w, T* __restrict__ dbn,
                                                                 float* __restrict__ dw, float* __restrict__ db, int vec4) {
  extern __shared__ float smem[];
  float* wl = smem + KB * C + KB;
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  for (int i = threadIdx.x; i < KB * C + KB; i += RB) smem[i] = 0.f;
  for (int i = threadIdx.x; i < KB * C; i += RB) {
    const int k = i / C, c = i - k * C;
    wl[i] = k < K ? w[c * K + k] : 0.f;
  }
  __syncthreads();
  float4 part[KB];
  float dbp[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    part[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    dbp[k] = 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    const float4 a = ld4(x + i * 4);
    float4 xh;
    xh.x = (a.x - stats[c + 0]) * rsqrtf(stats[C + c + 0] + eps);
    xh.y = (a.y - stats[c + 1]) * rsqrtf(stats[C + c + 1] + eps);
    xh.z = (a.z - stats[c + 2]) * rsqrtf(stats[C + c + 2] + eps);
    xh.w = (a.w - stats[c + 3]) * rsqrtf(stats[C + c + 3] + eps);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k0 = 0; k0 < KB; k0 += 4) {  // four channels at a time: only their four gradients are live
      float g[4];
      if (vec4) {
        const float4 t = k0 < K ? ld4(dpred + v * K + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = k0 + j < K ? dpred[v * K + k0 + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        const float4 wk = *reinterpret_cast<const float4*>(wl + k * C + c);
        d.x += g[j] * wk.x; d.y += g[j] * wk.y;
        d.z += g[j] * wk.z; d.w += g[j] * wk.w;
        if (fixed) {
          part[k].x += g[j] * xh.x; part[k].y += g[j] * xh.y; part[k].z += g[j] * xh.z; part[k].w += g[j] * xh.w;
        } else if (k < K) {
          atomicAdd(&smem[k * C + c + 0], g[j] * xh.x); atomicAdd(&smem[k * C + c + 1], g[j] * xh.y);
          atomicAdd(&smem[k * C + c + 2], g[j] * xh.z); atomicAdd(&smem[k * C + c + 3], g[j] * xh.w);
        }
        if (c == 0) dbp[k] += g[j];
      }
    }
    st4(dbn + i * 4, d);
  }
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (k < K) block_scalar_add(dbp[k], &smem[KB * C + k]);
  block_channel_reduce<KB>(part, threadIdx.x % C4, C4, fixed, smem);
  if (K < KB) {  // the gather takes A[K][C] | B[K] of the real K: move B up behind the last real row of A
    const float bv = (int)threadIdx.x < K ? smem[KB * C + threadIdx.x] : 0.f;
    __syncthreads();
    if ((int)threadIdx.x < K) smem[K * C + threadIdx.x] = bv;
    __syncthreads();
  }
  if (syn_det_gather(smem, K * C + K)) {
    for (int i = threadIdx.x; i < C * K; i += RB) {
      const int c = i / K, k = i - c * K;
      atomicAdd(&dw[i], gamma[c] * smem[k * C + c] + beta[c] * smem[K * C + k]);
    }
    if ((int)threadIdx.x < K) atomicAdd(&db[threadIdx.x], smem[K * C + threadIdx.x]);
  }
  syn_det_gather_end(K * C + K);
}

template <typename T>
__global__ __launch_bounds__(RB) void head_bwd_kernel(const float* __restrict__ dpred, const T* __restrict__ x,
                                                      int64_t n4, int C, const float* __restrict__ stats,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps,
                                                      const float* __restrict__ w, T* __restrict__ dbn,
                                                      float* __restrict__ dw, float* __restrict__ db,
                                                      float* __restrict__ sums) {
  // The gradient w.r.t. the BatchNorm output is rank-1, dbn[v][c] = g[v] w[c].  With A[c] = sum_v g xhat[v][c] and
  // B = sum_v g everything downstream is linear in (A, B):  dw = gamma A + beta B,  db = B, and the BN-backward sums
  // sum dbn = w B, sum dbn xhat = w A -- so dbn need not be written (dbn == nullptr) nor reduced again (sums != nullptr).
  extern __shared__ float smem[];  // [C] A partials + 1 B
  const int C4 = C / 4;
  const bool fixed = (RB % C4) == 0;
  for (int i = threadIdx.x; i < C + 1; i += RB) smem[i] = 0.f;
  __syncthreads();
  float4 part[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  float dbp = 0.f;
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t i = blockIdx.x * (int64_t)RB + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % C4) * 4;
    const int64_t v = i / C4;
    const float g = dpred[v];
    const float4 a = ld4(x + i * 4);
    float4 xh;
    xh.x = (a.x - stats[c + 0]) * rsqrtf(stats[C + c + 0] + eps);
    xh.y = (a.y - stats[c + 1]) * rsqrtf(stats[C + c + 1] + eps);
    xh.z = (a.z - stats[c + 2]) * rsqrtf(stats[C + c + 2] + eps);
    xh.w = (a.w - stats[c + 3]) * rsqrtf(stats[C + c + 3] + eps);
    if (dbn) st4(dbn + i * 4, make_float4(g * w[c + 0], g * w[c + 1], g * w[c + 2], g * w[c + 3]));
    if (fixed) {
      part[0].x += g * xh.x; part[0].y += g * xh.y; part[0].z += g * xh.z; part[0].w += g * xh.w;
    } else {
      atomicAdd(&smem[c + 0], g * xh.x); atomicAdd(&smem[c + 1], g * xh.y);
      atomicAdd(&smem[c + 2], g * xh.z); atomicAdd(&smem[c + 3], g * xh.w);
    }
    if (c == 0) dbp += g;
  }
  block_scalar_add(dbp, &smem[C]);
  block_channel_reduce<1>(part, threadIdx.x % C4, C4, fixed, smem);
  if (syn_det_gather(smem, C + 1)) {
    const float B = smem[C];
    for (int i = threadIdx.x; i < C; i += RB) {
      const float A = smem[i];
      atomicAdd(&dw[i], gamma[i] * A + beta[i] * B);
      if (sums) {
        atomicAdd(&sums[i], w[i] * B);
        atomicAdd(&sums[C + i], w[i] * A);
      }
    }
    if (threadIdx.x == 0) atomicAdd(db, B);
  }
  syn_det_gather_end(C + 1);
}

// ------------------------------------------------------------------ segmentation-regularised loss (metrics_model.py:136-215)
// Frozen segmentation U-Net head: probs[v][n] = softmax_n( sum_c W[c][n] * bn(x[v][c]) + b[n] )  (unet_likelihood, 1x1x1 conv +
// softmax, models.py:480-494).  One thread per voxel, weights in LDS.  C <= 64, N <= 64.
constexpr int SEG_MAXC = 64, SEG_MAXN = 64, SEG_MAXK = 64;

__global__ __launch_bounds__(256) void seg_head_fwd_kernel(const float* __restrict__ x, int64_t nvox, int C,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ W, const float* __restrict__ b, int N,
                                                           float* __restrict__ probs) {
  __shared__ float sw[SEG_MAXC * SEG_MAXN], ssc[SEG_MAXC], ssh[SEG_MAXC], sb[SEG_MAXN];
  for (int i = threadIdx.x; i < C * N; i += blockDim.x) sw[i] = W[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) bn_coeff(stats, gamma, beta, eps, C, i, ssc[i], ssh[i]);
  for (int i = threadIdx.x; i < N; i += blockDim.x) sb[i] = b[i];
  __syncthreads();
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    float* pr = probs + v * N;
    float mx = -INFINITY;
    for (int n = 0; n < N; ++n) {  // logits parked in the output row (L1/L2 resident), then normalised in place
      float acc = sb[n];
      for (int c = 0; c < C; ++c) acc = fmaf(fmaf(x[v * C + c], ssc[c], ssh[c]), sw[c * N + n], acc);
      pr[n] = acc;
      mx = fmaxf(mx, acc);
    }
    float den = 0.f;
    for (int n = 0; n < N; ++n) {
      const float e = expf(pr[n] - mx);
      pr[n] = e;
      den += e;
    }
    const float inv = 1.f / den;
    for (int n = 0; n < N; ++n) pr[n] *= inv;
  }
}

// Soft-Dice sums over the K generation labels that have an equivalent among the segmentation labels:
//   pred_k[v] = sum_j probs[v][cls_idx[k][j]] (up to 3 merged labels, -1 = unused),  gt_k[v] = (seg[v] == cls_gt[k])
//   sums[k] += 2 gt pred,  sums[K + k] += gt^2 + pred^2                                   (DiceLoss, layers.py:1343-1362)
__global__ __launch_bounds__(256) void seg_dice_sums_kernel(const float* __restrict__ probs, const int32_t* __restrict__ seg,
                                                            int64_t nvox, int N, const int32_t* __restrict__ cls_idx,
                                                            const int32_t* __restrict__ cls_gt, int K,
                                                            float* __restrict__ sums) {
  // per-wave partials in fixed LDS slots, added in wave order, then ONE flush per workgroup (syn_det_gather: in deterministic
  // mode the last workgroup adds all rows in id order) -- round 4: the LDS float atomics this kernel used made the Dice sums the
  // one reduction deterministic mode did not cover
  __shared__ float st[2 * SEG_MAXK], sw4[4][2 * SEG_MAXK];
  for (int k = 0; k < K; ++k) {
    const int i0 = cls_idx[3 * k], i1 = cls_idx[3 * k + 1], i2 = cls_idx[3 * k + 2], g = cls_gt[k];
    float top = 0.f, bot = 0.f;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
      const float* pr = probs + v * N;
      float p = pr[i0];
      if (i1 >= 0) p += pr[i1];
      if (i2 >= 0) p += pr[i2];
      const float gt = seg[v] == g ? 1.f : 0.f;
      top += 2.f * gt * p;
      bot += gt + p * p;
    }
    top = syn_wave_sum(top);
    bot = syn_wave_sum(bot);
    if ((threadIdx.x & 63) == 0) {
      sw4[threadIdx.x >> 6][k] = top;
      sw4[threadIdx.x >> 6][K + k] = bot;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K; i += blockDim.x) st[i] = (sw4[0][i] + sw4[1][i]) + (sw4[2][i] + sw4[3][i]);
  __syncthreads();
  if (syn_det_gather(st, 2 * K))
    for (int i = threadIdx.x; i < 2 * K; i += blockDim.x) atomicAdd(&sums[i], st[i]);
  syn_det_gather_end(2 * K);
}

// Backward of  scale * mean_k(1 - (T_k + e)/(B_k + e))  through the label merging, the softmax and the 1x1x1 head:
//   dpred_k = -scale/K * (2 gt_k (B_k+e) - 2 pred_k (T_k+e)) / (B_k+e)^2
//   dlogit_n = p_n (dprob_n - S),  dprob_n = dpred_{class(n)} (0 for labels without class),  S = sum_k dpred_k pred_k
//   dbn[v][c] = sum_n W[c][n] dlogit_n  = sum_k dpred_k sum_j W[c][idx_kj] p_idx_kj  -  S sum_n W[c][n] p_n
// T = the element type of dbn (float | bf16_t: the frozen network runs in bf16, one rounding to nearest even at the store)
template <typename T>
__global__ __launch_bounds__(256) void seg_dice_bwd_kernel(const float* __restrict__ probs, const int32_t* __restrict__ seg,
                                                           int64_t nvox, int C, int N, const float* __restrict__ W,
                                                           const int32_t* __restrict__ cls_idx,
                                                           const int32_t* __restrict__ cls_gt, int K,
                                                           const float* __restrict__ sums, float scale,
                                                           T* __restrict__ dbn) {
  __shared__ float sw[SEG_MAXC * SEG_MAXN], sT[SEG_MAXK], sB[SEG_MAXK];
  __shared__ int sidx[3 * SEG_MAXK], sgt[SEG_MAXK];
  for (int i = threadIdx.x; i < C * N; i += blockDim.x) sw[i] = W[i];
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    sT[i] = sums[i] + 1e-7f;
    sB[i] = sums[K + i] + 1e-7f;
    sgt[i] = cls_gt[i];
  }
  for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) sidx[i] = cls_idx[i];
  __syncthreads();
  const float coef = -scale / (float)K;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    const float* pr = probs + v * N;
    float out[SEG_MAXC];
#pragma unroll
    for (int c = 0; c < SEG_MAXC; ++c) out[c] = 0.f;
    float S = 0.f;
    const int lab = seg[v];
    for (int k = 0; k < K; ++k) {
      const int i0 = sidx[3 * k], i1 = sidx[3 * k + 1], i2 = sidx[3 * k + 2];
      const float p0 = pr[i0], p1 = i1 >= 0 ? pr[i1] : 0.f, p2 = i2 >= 0 ? pr[i2] : 0.f;
      const float pk = p0 + p1 + p2;
      const float gt = lab == sgt[k] ? 1.f : 0.f;
      const float dp = coef * (2.f * gt * sB[k] - 2.f * pk * sT[k]) / (sB[k] * sB[k]);
      S += dp * pk;
#pragma unroll
      for (int c = 0; c < SEG_MAXC; ++c)
        if (c < C) {
          float a = sw[c * N + i0] * p0;
          if (i1 >= 0) a += sw[c * N + i1] * p1;
          if (i2 >= 0) a += sw[c * N + i2] * p2;
          out[c] += dp * a;
        }
    }
    for (int n = 0; n < N; ++n) {
      const float sp = S * pr[n];
#pragma unroll
      for (int c = 0; c < SEG_MAXC; ++c)
        if (c < C) out[c] -= sw[c * N + n] * sp;
    }
#pragma unroll
    for (int c = 0; c < SEG_MAXC; ++c)
      if (c < C) st1(dbn + v * C + c, out[c]);
  }
}

// ------------------------------------------------------------------ trainable softmax head + soft Dice (fp32)
// Training a segmentation U-Net: head, softmax and DiceLoss (ext/lab2im/layers.py:1343-1376, enable_checks=False) fused, the
// ground truth taken from the raw label map through a lookup table (label value -> head channel, -1 / outside the table = no
// class: an all-zero one-hot row).  Both kernels work on tiles of 64 voxels per workgroup, 16 per wave, and form their small
// matrix products on the fp32 matrix instruction (v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15];
// result register r of lane l is D[4 (l >> 4) + r][l & 15]).  Each wave stages its 16 voxels in its own LDS rows, whose stride
// is (16 blocks + 4) floats = 4 x an odd number: the 16 rows x 4 consecutive columns of an A operand read down the voxel axis
// fall on 64 different banks, and the 4 rows x 16 consecutive columns of an operand read along a row on at most two per bank.
constexpr int SHD_TILE = 64;  // voxels per workgroup iteration (4 waves x 16)
typedef float shd_f32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int shd_stride(int blocks16) { return blocks16 * 16 + 4; }

// The dynamic LDS of these kernels, offsets and total in floats: a kernel takes its pointers from here and its launcher the byte
// count.  Forward and label-map kernels (wl at 0, <= 38 KB):
//   wl [C][SW] | xs [4][16][SX] | scale, shift [64 + 64] | bias [64] | class or label value [64]; dice: | red [4][RS] | st [RS]
// RS = 128 (rows T | B of 64); the weighted Dice: RS = 192 (T | B | V), then | boundary-mask words [64] (uint64: 128 floats)
struct ShdFwdLds {
  int SX, SW, xs, scale, shift, bias, cls, RS, red, st, msk, total;
  __host__ __device__ constexpr ShdFwdLds(int C, int N, bool dice, bool weighted = false)
      : SX(shd_stride((C + 15) >> 4)), SW(shd_stride((N + 15) >> 4)), xs(C * SW), scale(xs + SHD_TILE * SX), shift(scale + 64),
        bias(shift + 64), cls(bias + 64), RS(weighted ? 192 : 128), red(cls + 64), st(red + 4 * RS), msk(st + RS),
        total(dice ? (weighted ? msk + 128 : msk) : red) {}
};
// Backward kernel (wl at 0; at most 3 x 64 x 68 + 320 floats = 53.5 KB, with the deterministic gather's 8 KB of static LDS inside
// the 64 KB of a launch):
//   wl [16 NB][SW] (w transposed, zero padded) | dl [4][16][SN] | xs [4][16][SX] | ga, gb [64 + 64] | mean, rstd [64 + 64] | class [64]
// the weighted Dice: | boundary-mask words [64] (uint64: 128 floats; 54 KB + 8 KB at most)
struct ShdBwdLds {
  int NB, SX, SN, SW, dl, xs, ga, gb, mean, rstd, cls, msk, total;
  __host__ __device__ constexpr ShdBwdLds(int C, int N, bool weighted = false)
      : NB((N + 15) >> 4), SX(shd_stride((C + 15) >> 4)), SN(shd_stride(NB)), SW(SX), dl(NB * 16 * SW), xs(dl + SHD_TILE * SN),
        ga(xs + SHD_TILE * SX), gb(ga + 64), mean(gb + 64), rstd(mean + 64), cls(rstd + 64), msk(cls + 64),
        total(weighted ? msk + 128 : msk) {}
};
// the byte counts of the three launchers these structs replaced, at the corners of C in {4 .. 64} x N in {1 .. 64}
static_assert(ShdFwdLds(4, 1, true).total == 4 * 20 + 64 * 20 + 4 * 64 + 4 * 128 + 128 &&
              ShdFwdLds(64, 64, true).total == 64 * 68 + 64 * 68 + 4 * 64 + 4 * 128 + 128 &&
              ShdFwdLds(20, 17, false).total == 20 * 36 + 64 * 36 + 4 * 64 && ShdFwdLds(64, 64, false).total == 2 * 64 * 68 + 4 * 64 &&
              ShdBwdLds(4, 64).total == 64 * 20 + 64 * (68 + 20) + 5 * 64 && ShdBwdLds(64, 1).total == 16 * 68 + 64 * (20 + 68) + 5 * 64 &&
              ShdBwdLds(64, 64).total == 3 * 64 * 68 + 5 * 64,
              "LDS layout of the softmax-head kernels");
// the weighted forms: the same offsets, wider sum rows and the mask words (8-byte aligned) behind everything else
static_assert(ShdFwdLds(24, 33, true, true).cls == ShdFwdLds(24, 33, true).cls &&
              ShdFwdLds(64, 64, true, true).total == ShdFwdLds(64, 64, true).total + 5 * 64 + 128 &&
              ShdBwdLds(64, 64, true).total == ShdBwdLds(64, 64).total + 128 && ShdFwdLds(4, 1, true, true).msk % 2 == 0 &&
              ShdBwdLds(4, 1, true).msk % 2 == 0 && (ShdBwdLds(64, 64, true).total * 4 + 8192 + 16) <= 65536,
              "LDS layout of the weighted softmax-head kernels");

// The steps that the tile kernels share.  tid = 64 wave + lane, lane = 16 quad + col.
// Head into LDS: wl [C][SW] (columns n >= N zero), BatchNorm scale / shift, bias; column(n) = the head column behind channel n.
template <typename Column>
__device__ __forceinline__ void shd_stage_head(float* wl, float* ssc, float* ssh, float* sb, int SW, int C, int N,
                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float eps, const float* __restrict__ W,
                                               const float* __restrict__ b, Column column) {
  const int tid = threadIdx.x;
  for (int i = tid; i < C * SW; i += 256) {
    const int c = i / SW, n = i - c * SW;
    wl[i] = n < N ? W[c * N + column(n)] : 0.f;
  }
  for (int i = tid; i < C; i += 256) bn_coeff(stats, gamma, beta, eps, C, i, ssc[i], ssh[i]);
  for (int i = tid; i < 64; i += 256) sb[i] = i < N ? b[column(i)] : 0.f;
}

// xw [16][SX] <- op(x[v0 + r][c], c) of a wave's 16 voxels (rows past the volume: zeros).  T = float | bf16_t: a bf16 row is
// half as wide in global memory (4 channels = one 8-byte load); its fp32 image in LDS keeps the stride SX, so what the comment
// above SHD_TILE says about banks holds for both.
template <typename T, typename Op>
__device__ __forceinline__ void shd_stage_rows(float* xw, int SX, const T* __restrict__ x, int64_t v0, int64_t nvox, int C,
                                               Op op) {
  const int lane = threadIdx.x & 63, C4 = C >> 2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j;
    if (i < 16 * C4) {
      const int r = i / C4, c = (i - r * C4) * 4;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v0 + r < nvox) {
        const float4 a = ld4(x + (v0 + r) * C + c);
        o = make_float4(op(a.x, c), op(a.y, c + 1), op(a.z, c + 2), op(a.w, c + 3));
      }
      *reinterpret_cast<float4*>(xw + r * SX + c) = o;
    }
  }
}

// acc[nb] <- logits [16 voxels][16 classes] of class block nb < NB, K = channels
__device__ __forceinline__ void shd_logits(shd_f32x4 (&acc)[4], const float* xw, const float* wl, int SX, int SW, int C, int NB) {
  const int col = threadIdx.x & 15, quad = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < C; c0 += 4) {
    const float a = xw[col * SX + c0 + quad];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
      if (nb < NB) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wl[(c0 + quad) * SW + nb * 16 + col], acc[nb], 0, 0, 0);
  }
}

// voxel 4 quad + r of the wave: its classes sit in the 16 lanes of the quad x NB registers.  val[nb] <- logit of class
// 16 nb + col (-INFINITY past N)
__device__ __forceinline__ void shd_row_logits(float (&val)[4], const shd_f32x4 (&acc)[4], int r, const float* sb, int NB, int N) {
  const int col = threadIdx.x & 15;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int n = nb * 16 + col;
    val[nb] = (nb < NB && n < N) ? acc[nb][r] + sb[n] : -INFINITY;
  }
}

// softmax of that row: val[nb] <- exp(val[nb] - max) (0 past N); returns 1 / their sum, p = val[nb] * that.  mx <- the row's
// maximum: log p_n = z_n - mx + log(1 / sum), finite where p_n itself underflows
__device__ __forceinline__ float shd_row_softmax(float (&val)[4], int NB, int N, float& mx) {
  const int col = threadIdx.x & 15;
  mx = -INFINITY;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) mx = fmaxf(mx, val[nb]);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float den = 0.f;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    val[nb] = (nb < NB && nb * 16 + col < N) ? expf(val[nb] - mx) : 0.f;
    den += val[nb];
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) den += __shfl_xor(den, o, 64);
  return 1.f / den;
}
__device__ __forceinline__ float shd_row_softmax(float (&val)[4], int NB, int N) {
  float mx;
  return shd_row_softmax(val, NB, N, mx);
}

// probs[v][n] = softmax_n(bn(x[v]) . w + b), sums[n] += 2 gt p, sums[N + n] += gt^2 + p^2: one pass, every voxel read once.
// WEIGHTED (DiceLoss with boundary and / or class weights, ext/lab2im/layers.py:1347-1374): every term of voxel v and class n
// counts w_n(v) = 1 + bw * bit n of mask[v] times (mask: seg_boundary_mask_kernel; nullptr = no boundary voxels), and a third
// row sums[2 N + n] += w gt (the weighted volume of class n: dynamic class weights) is formed.  The mask word of a voxel is
// staged next to its class index.  WEIGHTED = false never touches mask / bw: the kernel as it was.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void seg_head_dice_fwd_kernel(const float* __restrict__ x, int64_t nvox, int C,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps,
                                                                const float* __restrict__ W, const float* __restrict__ b, int N,
                                                                const int32_t* __restrict__ seg,
                                                                const int32_t* __restrict__ lut, int lut_n,
                                                                float* __restrict__ probs, float* __restrict__ sums,
                                                                const uint64_t* __restrict__ mask, float bw) {
  extern __shared__ float smem[];
  const ShdFwdLds L(C, N, true, WEIGHTED);
  constexpr int ROWS = WEIGHTED ? 3 : 2, RS = 64 * ROWS;
  const int NB = (N + 15) >> 4, SX = L.SX, SW = L.SW;
  float *wl = smem, *ssc = smem + L.scale, *ssh = smem + L.shift, *sb = smem + L.bias, *red = smem + L.red, *st = smem + L.st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  shd_stage_head(wl, ssc, ssh, sb, SW, C, N, stats, gamma, beta, eps, W, b, [](int n) { return n; });
  __syncthreads();
  float* xw = smem + L.xs + wave * 16 * SX;
  int* cw = reinterpret_cast<int*>(smem + L.cls) + wave * 16;
  uint64_t* mw = reinterpret_cast<uint64_t*>(smem + L.msk) + wave * 16;  // (WEIGHTED only)
  float top[4] = {0.f, 0.f, 0.f, 0.f}, bot[4] = {0.f, 0.f, 0.f, 0.f}, vol[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return fmaf(a, ssc[c], ssh[c]); });  // BatchNorm output
    if (lane < 16) {
      cw[lane] = v0 + lane < nvox ? shd_class(seg[v0 + lane], lut, lut_n, N) : -1;
      if constexpr (WEIGHTED) mw[lane] = (mask && v0 + lane < nvox) ? mask[v0 + lane] : 0ull;
    }
    __syncthreads();
    shd_f32x4 acc[4];
    shd_logits(acc, xw, wl, SX, SW, C, NB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float lg[4];
      shd_row_logits(lg, acc, r, sb, NB, N);
      const float inv = shd_row_softmax(lg, NB, N);
      const int64_t v = v0 + 4 * quad + r;
      const int k = cw[4 * quad + r];
      uint64_t m = 0;
      if constexpr (WEIGHTED) m = mw[4 * quad + r];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const int n = nb * 16 + col;
        if (nb < NB && n < N && v < nvox) {
          const float p = lg[nb] * inv;
          probs[v * N + n] = p;
          const float gt = k == n ? 1.f : 0.f;
          if constexpr (WEIGHTED) {
            const float wgt = ((m >> n) & 1ull) ? 1.f + bw : 1.f, t = 2.f * gt * p, q = gt + p * p;
            top[nb] += wgt * t;
            bot[nb] += wgt * q;
            vol[nb] += wgt * gt;
          } else {
            top[nb] += 2.f * gt * p;
            bot[nb] += gt + p * p;
          }
        }
      }
    }
  }
  // the four quads of a wave, then the four waves in order, then ONE flush per workgroup
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    top[nb] += __shfl_xor(top[nb], 16, 64);
    top[nb] += __shfl_xor(top[nb], 32, 64);
    bot[nb] += __shfl_xor(bot[nb], 16, 64);
    bot[nb] += __shfl_xor(bot[nb], 32, 64);
    if constexpr (WEIGHTED) {
      vol[nb] += __shfl_xor(vol[nb], 16, 64);
      vol[nb] += __shfl_xor(vol[nb], 32, 64);
    }
    if (lane < 16) {
      red[wave * RS + nb * 16 + lane] = top[nb];
      red[wave * RS + 64 + nb * 16 + lane] = bot[nb];
      if constexpr (WEIGHTED) red[wave * RS + 128 + nb * 16 + lane] = vol[nb];
    }
  }
  __syncthreads();
  for (int i = tid; i < ROWS * N; i += 256) {
    const int row = i / N, k = 64 * row + i - row * N;
    st[i] = (red[k] + red[RS + k]) + (red[2 * RS + k] + red[3 * RS + k]);
  }
  __syncthreads();
  if (syn_det_gather(st, ROWS * N))
    for (int i = tid; i < ROWS * N; i += 256) atomicAdd(&sums[i], st[i]);
  syn_det_gather_end(ROWS * N);
}

// probs[v][n] = softmax_n(bn(x[v]) . w + b) of a bf16 feature map: seg_head_dice_fwd_kernel without labels and sums (the head of
// a frozen or inference bf16 network; BatchNorm, head and softmax in fp32 on the fp32 master weights).  LDS: ShdFwdLds(C, N, false).
__global__ __launch_bounds__(256) void seg_head_fwd_bf16_kernel(const bf16_t* __restrict__ x, int64_t nvox, int C,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps,
                                                                const float* __restrict__ W, const float* __restrict__ b, int N,
                                                                float* __restrict__ probs) {
  extern __shared__ float smem[];
  const ShdFwdLds L(C, N, false);
  const int NB = (N + 15) >> 4, SX = L.SX, SW = L.SW;
  float *wl = smem, *ssc = smem + L.scale, *ssh = smem + L.shift, *sb = smem + L.bias;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  shd_stage_head(wl, ssc, ssh, sb, SW, C, N, stats, gamma, beta, eps, W, b, [](int n) { return n; });
  __syncthreads();
  float* xw = smem + L.xs + wave * 16 * SX;
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return fmaf(a, ssc[c], ssh[c]); });  // BatchNorm output
    __syncthreads();
    shd_f32x4 acc[4];
    shd_logits(acc, xw, wl, SX, SW, C, NB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float lg[4];
      shd_row_logits(lg, acc, r, sb, NB, N);
      const float inv = shd_row_softmax(lg, NB, N);
      const int64_t v = v0 + 4 * quad + r;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const int n = nb * 16 + col;
        if (nb < NB && n < N && v < nvox) probs[v * N + n] = lg[nb] * inv;
      }
    }
  }
}

// Backward of scale * mean_n(1 - (T_n + e) / (B_n + e)) through the softmax, the head and into the last BatchNorm's output:
//   g_n = -(scale / N) (2 gt_n (B_n + e) - 2 p_n (T_n + e)) / (B_n + e)^2,   dlogit_n = p_n (g_n - sum_m g_m p_m)
//   dbn[v][c] = sum_n dlogit_n w[c][n]   (written);   A[n][c] = sum_v dlogit_n xhat[v][c],  Bs[n] = sum_v dlogit_n
//   dw[c][n] += gamma[c] A[n][c] + beta[c] Bs[n],  db[n] += Bs[n]            (the algebra of head_multi_bwd_wide_kernel)
// A wave keeps dlogit [16][SN] and xhat [16][SX] of its 16 voxels in LDS and forms dbn (K = classes) and A (K = voxels, the
// accumulators live in registers for the whole sweep) on the matrix instruction.  The workgroup's partial A [N][C] | Bs [N] is
// gathered in dl | xs after the sweep.
// WEIGHTED: the loss is scale * sum_n c_n (1 - dice_n) on the weighted sums of seg_head_dice_fwd_kernel<true>:
//   g_n = -scale c_n w_n(v) (2 gt_n (B_n + e) - 2 p_n (T_n + e)) / (B_n + e)^2,  w_n(v) = 1 + bw * bit n of mask[v]
// (cwt [N]: the class weights c, constants of the step; mask nullptr = no boundary voxels); everything behind g is unchanged.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void seg_head_dice_bwd_kernel(const float* __restrict__ probs, const int32_t* __restrict__ seg,
                                                                const int32_t* __restrict__ lut, int lut_n,
                                                                const float* __restrict__ x, int64_t nvox, int C, int N,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps,
                                                                const float* __restrict__ W, const float* __restrict__ sums,
                                                                float scale, float* __restrict__ dbn, float* __restrict__ dw,
                                                                float* __restrict__ db, const uint64_t* __restrict__ mask,
                                                                float bw, const float* __restrict__ cwt) {
  extern __shared__ float smem[];
  const ShdBwdLds L(C, N, WEIGHTED);
  const int NB = L.NB, CB = (C + 15) >> 4, SX = L.SX, SN = L.SN, SW = L.SW;
  float *wl = smem, *dl = smem + L.dl, *xs = smem + L.xs, *sga = smem + L.ga, *sgb = smem + L.gb, *smean = smem + L.mean,
        *srstd = smem + L.rstd;
  int* scls = reinterpret_cast<int*>(smem + L.cls);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  for (int i = tid; i < NB * 16 * SW; i += 256) {
    const int n = i / SW, c = i - n * SW;
    wl[i] = (n < N && c < C) ? W[c * N + n] : 0.f;
  }
  for (int i = tid; i < SHD_TILE * (SN + SX); i += 256) dl[i] = 0.f;  // the padding columns stay zero
  const float coef_mean = -scale / (float)N;
  for (int i = tid; i < 64; i += 256) {
    float ga = 0.f, gb = 0.f;
    if (i < N) {
      float coef = coef_mean;
      if constexpr (WEIGHTED) coef = -scale * cwt[i];
      const float T = sums[i] + 1e-7f, B = sums[N + i] + 1e-7f;
      ga = coef * 2.f / B;
      gb = coef * 2.f * T / (B * B);
    }
    sga[i] = ga;
    sgb[i] = gb;
    if (i < C) {
      smean[i] = stats[i];
      srstd[i] = rsqrtf(stats[C + i] + eps);
    }
  }
  __syncthreads();
  float* dlw = dl + wave * 16 * SN;
  float* xw = xs + wave * 16 * SX;
  int* cw = scls + wave * 16;
  uint64_t* mw = reinterpret_cast<uint64_t*>(smem + L.msk) + wave * 16;  // (WEIGHTED only)
  shd_f32x4 accA[4][4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) accA[nb][cb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
  float bs = 0.f;
  const int q64 = 64 / N, r64 = 64 - q64 * N;
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return (a - smean[c]) * srstd[c]; });  // xhat
    {  // their 16 N posteriors: one contiguous run (rows past the volume: zeros, so that their dlogit is zero)
      int r = lane / N, n = lane - r * N;
      for (int i = lane; i < 16 * N; i += 64) {
        dlw[r * SN + n] = v0 + r < nvox ? probs[v0 * N + i] : 0.f;
        r += q64;
        n += r64;
        if (n >= N) {
          n -= N;
          ++r;
        }
      }
    }
    if (lane < 16) {
      cw[lane] = v0 + lane < nvox ? shd_class(seg[v0 + lane], lut, lut_n, N) : -1;
      if constexpr (WEIGHTED) mw[lane] = (mask && v0 + lane < nvox) ? mask[v0 + lane] : 0ull;
    }
    __syncthreads();
    {  // four lanes per voxel: S = sum_n g_n p_n, then dlogit in place
      const int r = lane >> 2, q = lane & 3, k = cw[r];
      uint64_t m = 0;
      if constexpr (WEIGHTED) m = mw[r];
      const float wb = 1.f + bw;
      float S = 0.f;
      for (int n = q; n < N; n += 4) {
        const float p = dlw[r * SN + n];
        float g = (k == n ? sga[n] : 0.f) - p * sgb[n];
        if constexpr (WEIGHTED) g *= ((m >> n) & 1ull) ? wb : 1.f;
        S = fmaf(g, p, S);
      }
      S += __shfl_xor(S, 1, 64);
      S += __shfl_xor(S, 2, 64);
      for (int n = q; n < N; n += 4) {
        const float p = dlw[r * SN + n];
        float g = (k == n ? sga[n] : 0.f) - p * sgb[n];
        if constexpr (WEIGHTED) g *= ((m >> n) & 1ull) ? wb : 1.f;
        dlw[r * SN + n] = p * (g - S);
      }
    }
    __syncthreads();
    if (lane < N) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += dlw[r * SN + lane];
      bs += t;
    }
    shd_f32x4 accD[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) accD[cb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < NB * 16; n0 += 4) {  // dbn [16 voxels][16 channels] per channel block, K = classes
      const float a = dlw[col * SN + n0 + quad];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        if (cb < CB) accD[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wl[(n0 + quad) * SW + cb * 16 + col], accD[cb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int c = cb * 16 + col;
      if (cb < CB && c < C) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t v = v0 + 4 * quad + r;
          if (v < nvox) dbn[v * C + c] = accD[cb][r];
        }
      }
    }
#pragma unroll
    for (int k0 = 0; k0 < 16; k0 += 4) {  // A [16 classes][16 channels] per block pair, K = the 16 voxels
      float a[4], bx[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) a[nb] = nb < NB ? dlw[(k0 + quad) * SN + nb * 16 + col] : 0.f;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) bx[cb] = cb < CB ? xw[(k0 + quad) * SX + cb * 16 + col] : 0.f;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (nb < NB && cb < CB) accA[nb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nb], bx[cb], accA[nb][cb], 0, 0, 0);
    }
  }
  // the four waves add their A | Bs in wave order into part (over dl | xs), then ONE flush per workgroup
  __syncthreads();
  float* part = dl;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = nb * 16 + 4 * quad + r, c = cb * 16 + col;
            if (nb < NB && cb < CB && n < N && c < C) part[n * C + c] = (w ? part[n * C + c] : 0.f) + accA[nb][cb][r];
          }
      if (lane < N) part[N * C + lane] = (w ? part[N * C + lane] : 0.f) + bs;
    }
    __syncthreads();
  }
  if (syn_det_gather(part, N * C + N)) {
    for (int i = tid; i < C * N; i += 256) {
      const int c = i / N, n = i - c * N;
      atomicAdd(&dw[i], gamma[c] * part[n * C + c] + beta[c] * part[N * C + n]);
    }
    if (tid < N) atomicAdd(&db[tid], part[N * C + tid]);
  }
  syn_det_gather_end(N * C + N);
}

// ------------------------------------------------------------------ trainable softmax head + losses on the logits (fp32)
// WeightedL2Loss (ext/lab2im/layers.py:1408-1412) and CrossEntropyLoss (:1498-1526, enable_checks=False, no weights) of the
// logits z[v][n] = bn(x[v]) . w[:, n] + b[n] against the one-hot of k(v) = shd_class(seg[v]) (-1: an all-zero row).  The gradient
// of a voxel needs nothing of the other voxels but three sums, so neither kernel has a per-voxel intermediate: the forward one
// reads x and seg and writes three floats, the backward one reads x once, forms the logits again and writes dbn.  KIND is
// SYNTHSR_SEG_LOSS_WL2 / _CE (include/synthsr_hip.h).
//   WL2: a_v = 1e-8 where k(v) == 0, else 1 (1 - gt_0 + 1e-8 in fp32); sums[0] += a_v sum_n (z_n - t (2 gt_n - 1))^2,
//        sums[1] += [k != 0], sums[2] += [k == 0]; loss = sums[0] / (W N), W = sums[1] + 1e-8 sums[2];
//        dz_n = scale 2 a_v (z_n - t (2 gt_n - 1)) / (W N)
//   CE:  sums[0] += -log p_k(v) over the classed voxels as a log-softmax (z_k - max - log sum exp: finite where p_k underflows
//        and the reference's log gives inf), sums[1] += [k >= 0]; loss = sums[0] / nvox;
//        dz_n = scale (p_n - gt_n) / nvox on classed voxels, 0 elsewhere
constexpr int SHD_LOSS_WL2 = SYNTHSR_SEG_LOSS_WL2, SHD_LOSS_CE = SYNTHSR_SEG_LOSS_CE;
// their LDS: the three sums fit the Dice forward's red | st, the bias the mask words of the weighted Dice backward
static_assert(ShdFwdLds(4, 2, true).st - ShdFwdLds(4, 2, true).red >= 4 * 4 && ShdFwdLds(4, 2, true).RS >= 3 &&
              ShdBwdLds(64, 64, true).total - ShdBwdLds(64, 64, true).msk >= 64 &&
              ShdBwdLds(4, 2, true).total - ShdBwdLds(4, 2, true).msk >= 64,
              "LDS layout of the logit-loss kernels");

// LDS: ShdFwdLds(C, N, true); of red | st only [4][4] | [4] floats are used.  Nothing is written per voxel.
template <int KIND>
__global__ __launch_bounds__(256) void seg_head_logit_loss_fwd_kernel(const float* __restrict__ x, int64_t nvox, int C,
                                                                      const float* __restrict__ stats,
                                                                      const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, float eps,
                                                                      const float* __restrict__ W, const float* __restrict__ b,
                                                                      int N, const int32_t* __restrict__ seg,
                                                                      const int32_t* __restrict__ lut, int lut_n, float tv,
                                                                      float* __restrict__ sums) {
  extern __shared__ float smem[];
  const ShdFwdLds L(C, N, true);
  const int NB = (N + 15) >> 4, SX = L.SX, SW = L.SW;
  float *wl = smem, *ssc = smem + L.scale, *ssh = smem + L.shift, *sb = smem + L.bias, *red = smem + L.red, *st = smem + L.st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  shd_stage_head(wl, ssc, ssh, sb, SW, C, N, stats, gamma, beta, eps, W, b, [](int n) { return n; });
  __syncthreads();
  float* xw = smem + L.xs + wave * 16 * SX;
  int* cw = reinterpret_cast<int*>(smem + L.cls) + wave * 16;
  float s[3] = {0.f, 0.f, 0.f};
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return fmaf(a, ssc[c], ssh[c]); });  // BatchNorm output
    if (lane < 16) cw[lane] = v0 + lane < nvox ? shd_class(seg[v0 + lane], lut, lut_n, N) : -1;
    __syncthreads();
    shd_f32x4 acc[4];
    shd_logits(acc, xw, wl, SX, SW, C, NB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float lg[4];
      shd_row_logits(lg, acc, r, sb, NB, N);
      const bool in = v0 + 4 * quad + r < nvox;
      const int k = cw[4 * quad + r];
      if constexpr (KIND == SHD_LOSS_WL2) {
        float t = 0.f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const int n = nb * 16 + col;
          if (nb < NB && n < N) {
            const float d = lg[nb] - (k == n ? tv : -tv);
            t = fmaf(d, d, t);
          }
        }
        if (in) {
          s[0] += (k == 0 ? 1e-8f : 1.f) * t;
          if (col == 0) {
            s[1] += k == 0 ? 0.f : 1.f;
            s[2] += k == 0 ? 1.f : 0.f;
          }
        }
      } else {
        float zk = 0.f, mx;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          if (nb * 16 + col == k) zk = lg[nb];
        const float inv = shd_row_softmax(lg, NB, N, mx);
        if (in && k >= 0) {  // the lane that holds class k: -log p_k = max - z_k + log sum exp
          if ((k & 15) == col) s[0] += (mx - zk) - logf(inv);
          if (col == 0) s[1] += 1.f;
        }
      }
    }
  }
  // the 64 lanes of a wave, then the four waves in order, then ONE flush per workgroup
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s[i] += __shfl_xor(s[i], o, 64);
    if (lane == 0) red[wave * 4 + i] = s[i];
  }
  __syncthreads();
  if (tid < 3) st[tid] = (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]);
  __syncthreads();
  if (syn_det_gather(st, 3))
    if (tid < 3) atomicAdd(&sums[tid], st[tid]);
  syn_det_gather_end(3);
}

// Backward of scale * loss into the last BatchNorm's output and the head: dz as above, then as seg_head_dice_bwd_kernel does with
// its dlogit: dbn[v][c] = sum_n dz_n w[c][n] written, A[n][c] = sum_v dz_n xhat[v][c], Bs[n] = sum_v dz_n,
// dw[c][n] += gamma[c] A[n][c] + beta[c] Bs[n], db[n] += Bs[n].  x is read once, staged as xhat [16][SX] per wave; the A operand of
// the logits is gamma xhat + beta formed at the read, their B operand the transposed head wl [16 NB][SW] that dbn needs anyway
// (16 classes x 4 consecutive channels: 64 banks, the A operand's pattern), so that w is in LDS once.
// LDS: ShdBwdLds(C, N, true): ga | gb hold gamma | beta, the mask words' place the bias [64].
template <int KIND>
__global__ __launch_bounds__(256) void seg_head_logit_loss_bwd_kernel(const int32_t* __restrict__ seg,
                                                                      const int32_t* __restrict__ lut, int lut_n,
                                                                      const float* __restrict__ x, int64_t nvox, int C, int N,
                                                                      const float* __restrict__ stats,
                                                                      const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, float eps,
                                                                      const float* __restrict__ W, const float* __restrict__ b,
                                                                      float tv, const float* __restrict__ sums, float scale,
                                                                      float* __restrict__ dbn, float* __restrict__ dw,
                                                                      float* __restrict__ db) {
  extern __shared__ float smem[];
  const ShdBwdLds L(C, N, true);
  const int NB = L.NB, CB = (C + 15) >> 4, SX = L.SX, SN = L.SN, SW = L.SW;
  float *wl = smem, *dl = smem + L.dl, *xs = smem + L.xs, *sga = smem + L.ga, *sgb = smem + L.gb, *smean = smem + L.mean,
        *srstd = smem + L.rstd, *sb = smem + L.msk;
  int* scls = reinterpret_cast<int*>(smem + L.cls);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  for (int i = tid; i < NB * 16 * SW; i += 256) {
    const int n = i / SW, c = i - n * SW;
    wl[i] = (n < N && c < C) ? W[c * N + n] : 0.f;
  }
  for (int i = tid; i < SHD_TILE * (SN + SX); i += 256) dl[i] = 0.f;  // the padding columns stay zero
  for (int i = tid; i < 64; i += 256) {
    sga[i] = i < C ? gamma[i] : 0.f;
    sgb[i] = i < C ? beta[i] : 0.f;
    sb[i] = i < N ? b[i] : 0.f;
    if (i < C) {
      smean[i] = stats[i];
      srstd[i] = rsqrtf(stats[C + i] + eps);
    }
  }
  const float coef = KIND == SHD_LOSS_WL2 ? 2.f * scale / ((sums[1] + 1e-8f * sums[2]) * (float)N) : scale / (float)nvox;
  __syncthreads();
  float* dlw = dl + wave * 16 * SN;
  float* xw = xs + wave * 16 * SX;
  int* cw = scls + wave * 16;
  shd_f32x4 accA[4][4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) accA[nb][cb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
  float bs = 0.f;
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return (a - smean[c]) * srstd[c]; });  // xhat
    if (lane < 16) cw[lane] = v0 + lane < nvox ? shd_class(seg[v0 + lane], lut, lut_n, N) : -1;
    __syncthreads();
    {  // logits [16 voxels][16 classes] per class block, K = channels; then dz in the wave's dl rows
      shd_f32x4 acc[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
      for (int c0 = 0; c0 < C; c0 += 4) {
        const int c = c0 + quad;
        const float a = fmaf(xw[col * SX + c], sga[c], sgb[c]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          if (nb < NB) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wl[(nb * 16 + col) * SW + c], acc[nb], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float lg[4];
        shd_row_logits(lg, acc, r, sb, NB, N);
        const int row = 4 * quad + r, k = cw[row];
        const bool in = v0 + row < nvox;  // rows past the volume: dz = 0
        if constexpr (KIND == SHD_LOSS_WL2) {
          const float ca = in ? (k == 0 ? 1e-8f * coef : coef) : 0.f;
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) {
            const int n = nb * 16 + col;
            if (nb < NB && n < N) dlw[row * SN + n] = in ? ca * (lg[nb] - (k == n ? tv : -tv)) : 0.f;
          }
        } else {
          const float inv = shd_row_softmax(lg, NB, N);
          const float ca = (in && k >= 0) ? coef : 0.f;
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) {
            const int n = nb * 16 + col;
            if (nb < NB && n < N) dlw[row * SN + n] = ca * (lg[nb] * inv - (k == n ? 1.f : 0.f));
          }
        }
      }
    }
    __syncthreads();
    if (lane < N) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += dlw[r * SN + lane];
      bs += t;
    }
    shd_f32x4 accD[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) accD[cb] = shd_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < NB * 16; n0 += 4) {  // dbn [16 voxels][16 channels] per channel block, K = classes
      const float a = dlw[col * SN + n0 + quad];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        if (cb < CB) accD[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wl[(n0 + quad) * SW + cb * 16 + col], accD[cb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int c = cb * 16 + col;
      if (cb < CB && c < C) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t v = v0 + 4 * quad + r;
          if (v < nvox) dbn[v * C + c] = accD[cb][r];
        }
      }
    }
#pragma unroll
    for (int k0 = 0; k0 < 16; k0 += 4) {  // A [16 classes][16 channels] per block pair, K = the 16 voxels
      float a[4], bx[4];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) a[nb] = nb < NB ? dlw[(k0 + quad) * SN + nb * 16 + col] : 0.f;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) bx[cb] = cb < CB ? xw[(k0 + quad) * SX + cb * 16 + col] : 0.f;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (nb < NB && cb < CB) accA[nb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nb], bx[cb], accA[nb][cb], 0, 0, 0);
    }
  }
  // the four waves add their A | Bs in wave order into part (over dl | xs), then ONE flush per workgroup
  __syncthreads();
  float* part = dl;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = nb * 16 + 4 * quad + r, c = cb * 16 + col;
            if (nb < NB && cb < CB && n < N && c < C) part[n * C + c] = (w ? part[n * C + c] : 0.f) + accA[nb][cb][r];
          }
      if (lane < N) part[N * C + lane] = (w ? part[N * C + lane] : 0.f) + bs;
    }
    __syncthreads();
  }
  if (syn_det_gather(part, N * C + N)) {
    for (int i = tid; i < C * N; i += 256) {
      const int c = i / N, n = i - c * N;
      atomicAdd(&dw[i], gamma[c] * part[n * C + c] + beta[c] * part[N * C + n]);
    }
    if (tid < N) atomicAdd(&db[tid], part[N * C + tid]);
  }
  syn_det_gather_end(N * C + N);
}

// ------------------------------------------------------------------ boundary voxels of a label map (weighted soft Dice)
// DiceLoss's boundary map (ext/lab2im/layers.py:1349-1353) without its one-hot tensors: bit n of mask[v] says whether voxel v
// counts 1 + boundary_weights times for class n,
//   bnd_n(v) = [avg_n(v) > 0] [avg_n(v) < 1/3 - 1e-4],  avg_n = AvgPool3D(2 d + 1, strides 1, 'same') of the one-hot of lut[seg]
// (padding is not part of the divisor).  In integers: with k the voxels of class n and Wn the voxels inside the volume in the
// (2 d + 1)^3 window, bnd_n(v) = [0 < 3 k < Wn] -- the float rule exactly while Wn < 3333 (k / Wn < 1/3 is at most
// 1/3 - 1 / (3 Wn)), i.e. for d <= 5.  Voxels without a class count in Wn and in no k.  No floating point anywhere.
// A workgroup stages the class indices (one byte each, 255 = no class) of a 4 x 8 x 32 tile and its halo of d in LDS; a thread
// owns one (y, x) column of the tile.  Per voxel: one sweep of the window ORs the classes present and counts the classed voxels,
// then one counting sweep per class present but the last, whose count is what is left (an interior voxel: no second sweep).
// Taps outside the volume are neither read nor counted.
constexpr int SBM_TZ = 4, SBM_TY = 8, SBM_TX = 32, SBM_MAXD = 5;
constexpr int SBM_LDS = (SBM_TZ + 2 * SBM_MAXD) * (SBM_TY + 2 * SBM_MAXD) * (SBM_TX + 2 * SBM_MAXD);
__global__ __launch_bounds__(256) void seg_boundary_mask_kernel(const int32_t* __restrict__ seg, int d0, int d1, int d2,
                                                                const int32_t* __restrict__ lut, int lut_n, int N, int d,
                                                                int skip_bg, uint64_t* __restrict__ mask) {
  __shared__ uint8_t tile[SBM_LDS];
  const int HY = SBM_TY + 2 * d, HX = SBM_TX + 2 * d, HN = (SBM_TZ + 2 * d) * HY * HX;
  const int t0 = (d0 + SBM_TZ - 1) / SBM_TZ, t1 = (d1 + SBM_TY - 1) / SBM_TY, t2 = (d2 + SBM_TX - 1) / SBM_TX;
  const int tid = threadIdx.x, tx = tid & (SBM_TX - 1), ty = tid / SBM_TX;
  for (int t = blockIdx.x; t < t0 * t1 * t2; t += gridDim.x) {
    const int tz_ = t / (t1 * t2), tr = t - tz_ * (t1 * t2), ty_ = tr / t2;
    const int z0 = tz_ * SBM_TZ - d, y0 = ty_ * SBM_TY - d, x0 = (tr - ty_ * t2) * SBM_TX - d;  // origin of the staged block
    for (int i = tid; i < HN; i += 256) {
      const int hz = i / (HY * HX), hr = i - hz * (HY * HX), hy = hr / HX, hx = hr - hy * HX;
      const int z = z0 + hz, y = y0 + hy, xx = x0 + hx;
      int k = -1;
      if (z >= 0 && z < d0 && y >= 0 && y < d1 && xx >= 0 && xx < d2)
        k = shd_class(seg[((int64_t)z * d1 + y) * d2 + xx], lut, lut_n, N);
      tile[i] = (uint8_t)(k < 0 ? 255 : k);
    }
    __syncthreads();
    const int Y = y0 + d + ty, X = x0 + d + tx;
    if (Y < d1 && X < d2) {
      const int ya = max(Y - d, 0) - y0, yb = min(Y + d, d1 - 1) - y0, xa = max(X - d, 0) - x0, xb = min(X + d, d2 - 1) - x0;
      for (int tz = 0; tz < SBM_TZ; ++tz) {
        const int Z = z0 + d + tz;
        if (Z >= d0) break;
        const int za = max(Z - d, 0) - z0, zb = min(Z + d, d0 - 1) - z0;
        const int Wn = (zb - za + 1) * (yb - ya + 1) * (xb - xa + 1);
        uint64_t present = 0;
        int left = 0;
        for (int z = za; z <= zb; ++z)
          for (int y = ya; y <= yb; ++y) {
            const uint8_t* row = tile + (z * HY + y) * HX;
            for (int xx = xa; xx <= xb; ++xx) {
              const int c = row[xx];
              if (c < 64) {
                present |= 1ull << c;
                ++left;
              }
            }
          }
        uint64_t bits = 0;
        while (present) {
          const int n = __builtin_ctzll(present);
          present &= present - 1;
          int k = left;  // the last class present: what the others left
          if (present) {
            k = 0;
            for (int z = za; z <= zb; ++z)
              for (int y = ya; y <= yb; ++y) {
                const uint8_t* row = tile + (z * HY + y) * HX;
                for (int xx = xa; xx <= xb; ++xx) k += row[xx] == n ? 1 : 0;
              }
            left -= k;
          }
          if (3 * k < Wn) bits |= 1ull << n;
        }
        if (skip_bg) bits &= ~1ull;
        mask[((int64_t)Z * d1 + Y) * d2 + X] = bits;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ softmax head -> label map (inference, fp32)
// Segmenting with a trained segmentation U-Net: inference-mode BatchNorm, head and argmax over the N classes in one pass, on
// the tiles, LDS strides and matrix-instruction layout of seg_head_dice_fwd_kernel.  The label VALUE labels[n] of the winning
// channel is written (int32); on exactly equal values the lowest channel wins (numpy.argmax).
//   TTA = false: the argmax is taken on the logits (softmax is monotone): no expf, no posteriors anywhere.
//   TTA = true:  second pass of the flip-averaged prediction, run on the volume flipped along its first axis.  With prev
//                [nvox][N] the posteriors of the unflipped pass:  p[n] = 0.5 (softmax(logits)[perm[n]] + prev[mirror(v)][n]),
//                mirror(v) = voxel v with index 0 of [d0][plane] reversed, perm = the channel permutation that swaps left and
//                right structures (an entry outside [0, N) is read as the identity).  The head's columns are staged in
//                permuted order, so lane n holds the flipped pass's posterior of channel perm[n] and reads prev in place.
//                Label and, if probs_out, p are written at mirror(v): the outputs are in the unflipped frame.  probs_out
//                must not overlap prev.
// T = the element type of x (float | bf16_t); everything after the staging is the same fp32 code.
template <bool TTA, typename T>
__device__ __forceinline__ void shd_label_sweep(const T* __restrict__ x, int64_t nvox, int C,
                                                const float* __restrict__ stats, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, const float* __restrict__ W,
                                                const float* __restrict__ b, int N, const int32_t* __restrict__ labels,
                                                const float* __restrict__ prev, const int32_t* __restrict__ perm, int d0,
                                                int64_t plane, int32_t* __restrict__ out, float* __restrict__ probs_out) {
  extern __shared__ float smem[];
  const ShdFwdLds L(C, N, false);
  const int NB = (N + 15) >> 4, SX = L.SX, SW = L.SW;
  float *wl = smem, *ssc = smem + L.scale, *ssh = smem + L.shift, *sb = smem + L.bias;
  int* slab = reinterpret_cast<int*>(smem + L.cls);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  shd_stage_head(wl, ssc, ssh, sb, SW, C, N, stats, gamma, beta, eps, W, b, [&](int n) {  // (n < N)
    if (!TTA) return n;
    const int p = perm[n];
    return (p >= 0 && p < N) ? p : n;
  });
  for (int i = tid; i < 64; i += 256) slab[i] = i < N ? labels[i] : 0;
  __syncthreads();
  float* xw = smem + L.xs + wave * 16 * SX;
  for (int64_t base = (int64_t)blockIdx.x * SHD_TILE; base < nvox; base += (int64_t)gridDim.x * SHD_TILE) {
    const int64_t v0 = base + wave * 16;
    shd_stage_rows(xw, SX, x, v0, nvox, C, [&](float a, int c) { return fmaf(a, ssc[c], ssh[c]); });  // BatchNorm output
    __syncthreads();
    shd_f32x4 acc[4];
    shd_logits(acc, xw, wl, SX, SW, C, NB);
    int win = 0;  // lane col < 4 of a quad ends up with the winning channel of voxel 4 quad + col
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t v = v0 + 4 * quad + r;
      float val[4];
      shd_row_logits(val, acc, r, sb, NB, N);
      if (TTA) {
        int64_t m = 0;
        if (v < nvox) m = v + (int64_t)(d0 - 1 - 2 * (int)(v / plane)) * plane;
        const float inv = shd_row_softmax(val, NB, N);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const int n = nb * 16 + col;
          if (nb < NB && n < N && v < nvox) {
            val[nb] = 0.5f * (val[nb] * inv + prev[m * N + n]);
            if (probs_out) probs_out[m * N + n] = val[nb];
          } else {
            val[nb] = -INFINITY;
          }
        }
      }
      float bv = -INFINITY;
      int bi = 64;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (val[nb] > bv) {  // ascending channels, strictly greater: the lowest channel of equal values stays
          bv = val[nb];
          bi = nb * 16 + col;
        }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if (col == r) win = bi;
    }
    if (col < 4) {
      const int64_t v = v0 + 4 * quad + col;
      if (v < nvox) {
        const int64_t m = TTA ? v + (int64_t)(d0 - 1 - 2 * (int)(v / plane)) * plane : v;
        out[m] = slab[win < N ? win : 0];  // (no finite value at all: channel 0)
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void seg_head_argmax_kernel(const T* __restrict__ x, int64_t nvox, int C,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              const float* __restrict__ W, const float* __restrict__ b, int N,
                                                              const int32_t* __restrict__ labels, int32_t* __restrict__ out) {
  shd_label_sweep<false>(x, nvox, C, stats, gamma, beta, eps, W, b, N, labels, nullptr, nullptr, 1, nvox, out, nullptr);
}

template <typename T>
__global__ __launch_bounds__(256) void seg_head_tta_argmax_kernel(const T* __restrict__ x, int64_t nvox, int C,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps,
                                                                  const float* __restrict__ W, const float* __restrict__ b,
                                                                  int N, const int32_t* __restrict__ labels,
                                                                  const float* __restrict__ prev,
                                                                  const int32_t* __restrict__ perm, int d0, int64_t plane,
                                                                  int32_t* __restrict__ out, float* __restrict__ probs_out) {
  shd_label_sweep<true>(x, nvox, C, stats, gamma, beta, eps, W, b, N, labels, prev, perm, d0, plane, out, probs_out);
}

// Dice counts of two label maps: counts[0][k] += |a = k and b = k|, counts[1][k] += |a = k|, counts[2][k] += |b = k| over the
// voxels, k = shd_class of the label value (values outside the table or mapped to -1 count nowhere).  Per-workgroup histograms
// in LDS (integer atomics), one integer atomicAdd flush per workgroup: the sums are exact whatever the order.
__global__ __launch_bounds__(256) void seg_label_counts_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                               int64_t nvox, const int32_t* __restrict__ lut, int lut_n, int N,
                                                               unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long h[3 * SEG_MAXN];
  for (int i = threadIdx.x; i < 3 * SEG_MAXN; i += blockDim.x) h[i] = 0ull;
  __syncthreads();
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    const int ka = shd_class(a[v], lut, lut_n, N), kb = shd_class(b[v], lut, lut_n, N);
    if (ka >= 0) atomicAdd(&h[SEG_MAXN + ka], 1ull);
    if (kb >= 0) atomicAdd(&h[2 * SEG_MAXN + kb], 1ull);
    if (ka >= 0 && ka == kb) atomicAdd(&h[ka], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * N; i += blockDim.x) {
    const int row = i / N, k = i - row * N;
    const unsigned long long c = h[row * SEG_MAXN + k];
    if (c) atomicAdd(&counts[i], c);
  }
}

// ------------------------------------------------------------------------------------------ Adam (Keras 2.3.1)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr_t,
                                                   float b1, float b2, float eps, float gs) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * gs;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
  }
}

inline bool ok_c4(int C) { return C > 0 && (C % 4) == 0 && C <= 4096; }
inline bool bad_shape(const int s[3]) { return s[0] <= 0 || s[1] <= 0 || s[2] <= 0; }
inline bool odd_shape(const int s[3]) { return (s[0] | s[1] | s[2]) & 1; }
// float4 lanes of the 2^3-pooled tensor of a shape
inline int64_t pooled_n4(const Shape3& s, int C) { return (int64_t)(s.d[0] / 2) * (s.d[1] / 2) * (s.d[2] / 2) * (C / 4); }

}  // namespace

// ---- entry-point bodies, templated on the activation type (float | bf16_t)
// activation codes of the backward entry points: 1 ELU, 3 ReLU (the forward codes of synthsr_conv3d_fwd)
inline bool ok_act(int act) { return act == 1 || act == 3; }

// the one launcher of elu_bwd_kernel.  Optional groups, each all or nothing: BatchNorm backward (stats, gamma, sums), the rank-1
// head gradient (dpred, whead: in place of dy / dy2, on top of BatchNorm), per-sample dropout (drop, nvox_per_sample).  need: the
// groups that the calling entry point requires (one that has no parameters for a group passes nullptr).
enum { ACT_BN = 1, ACT_HEAD = 2, ACT_DROP = 4 };
template <typename T>
static int act_bwd_t(int need, const T* dy, const T* dy2, const T* y, T* dz, float* dbias, int64_t nvox, int C, const float* stats,
                     const float* gamma, float eps, const float* sums, const float* dpred, const float* whead, const float* drop,
                     int64_t nvox_per_sample, int act, synthsr_stream_t stream) {
  const bool bn = stats || gamma || sums, head = dpred || whead;
  if (!y || !dz || nvox < 1 || !ok_c4(C) || !ok_act(act) || (bn && (!stats || !gamma || !sums)) ||
      (head && (!dpred || !whead || !bn || dy || dy2)) || (!head && !dy) || (drop && (nvox_per_sample < 1 || (nvox % nvox_per_sample) != 0)) ||
      ((need & ACT_BN) && !bn) || ((need & ACT_HEAD) && !head) || ((need & ACT_DROP) && !drop))
    return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL((act == 3 ? elu_bwd_kernel<T, true> : elu_bwd_kernel<T>), dim3(syn_grid(n4, RB, red_grid())), dim3(RB),
                     C * sizeof(float), (hipStream_t)stream, dy, dy2, y, dz, dbias, n4, C / 4, stats, gamma, sums, eps,
                     bn ? (float)(1.0 / (double)nvox) : 0.f, dpred, whead, drop, drop ? nvox_per_sample * (C / 4) : (int64_t)0);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int bn_stats_t(const T* x, int64_t nvox, int C, float* stats, double* ws, synthsr_stream_t stream) {
  if (!x || !stats || !ws || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  if (hipMemsetAsync(ws, 0, 2 * C * sizeof(double), (hipStream_t)stream) != hipSuccess) return SYNTHSR_ELAUNCH;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(bn_stats_kernel<T>, dim3(syn_grid(n4, RB, red_grid())), dim3(RB), 3 * C * sizeof(float),
                     (hipStream_t)stream, x, n4, C / 4, ws);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_stats_finalize_kernel<T>, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, ws, x, stats, C,
                     nvox);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int bn_maxpool_t(const T* x, T* y, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  if (!x || !y || !stats || !gamma || !beta || bad_shape(shape) || odd_shape(shape) || !ok_c4(C)) return SYNTHSR_EINVAL;
  Shape3 s{{shape[0], shape[1], shape[2]}};
  hipLaunchKernelGGL(bn_maxpool_kernel<T>, dim3(syn_grid(pooled_n4(s, C), 256)), dim3(256), 0, (hipStream_t)stream, x, y, s, C,
                     stats, gamma, beta, eps);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

// sums == nullptr: the routed gradient only; with sums, dbn may be nullptr (the sums only)
template <typename T>
int bn_maxpool_bwd_ex_t(const T* dy, const T* x, T* dbn, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, float* sums, synthsr_stream_t stream) {
  if (!dy || !x || (!dbn && !sums) || !stats || !gamma || !beta || bad_shape(shape) || odd_shape(shape) || !ok_c4(C))
    return SYNTHSR_EINVAL;
  Shape3 s{{shape[0], shape[1], shape[2]}};
  const int64_t n4 = pooled_n4(s, C);
  if (sums)
    hipLaunchKernelGGL(bn_maxpool_bwd_sums_kernel<T>, dim3(syn_grid(n4, RB, red_grid())), dim3(RB), 2 * C * sizeof(float),
                       (hipStream_t)stream, dy, x, dbn, s, C, stats, gamma, beta, eps, sums);
  else
    hipLaunchKernelGGL(bn_maxpool_bwd_kernel<T>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dbn, s, C,
                       stats, gamma, beta, eps);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int bn_pool_elu_bwd_t(const T* dpool, const T* y, const T* dy2, T* dz, float* dbias, const int shape[3], int C,
                      const float* stats, const float* gamma, const float* beta, const float* sums, float eps,
                      synthsr_stream_t stream, int act) {
  if (!dpool || !y || !dz || !stats || !gamma || !beta || !sums || bad_shape(shape) || odd_shape(shape) || !ok_c4(C) ||
      !ok_act(act))
    return SYNTHSR_EINVAL;
  Shape3 s{{shape[0], shape[1], shape[2]}};
  const float inv_n = 1.0f / (float)((int64_t)s.d[0] * s.d[1] * s.d[2]);
  hipLaunchKernelGGL((act == 3 ? bn_pool_elu_bwd_kernel<T, true> : bn_pool_elu_bwd_kernel<T>), dim3(syn_grid(pooled_n4(s, C), RB, red_grid())),
                     dim3(RB), C * sizeof(float), (hipStream_t)stream, dpool, y, dy2, dz, dbias, s, C, stats, gamma, beta, sums, eps, inv_n);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int bn_bwd_reduce_t(const T* dy, const T* x, int64_t nvox, int C, const float* stats, float eps, float* sums, synthsr_stream_t stream) {
  if (!dy || !x || !stats || !sums || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(syn_grid(n4, RB, red_grid())), dim3(RB), 2 * C * sizeof(float),
                     (hipStream_t)stream, dy, x, n4, C, stats, eps, sums);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int upsample_concat_t(const T* skip, const T* lo, T* out, const int shape[3], int Cs, int Cl, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  if (!skip || !lo || !out || !stats || !gamma || !beta || bad_shape(shape) || odd_shape(shape) || !ok_c4(Cs) ||
      !ok_c4(Cl))
    return SYNTHSR_EINVAL;
  Shape3 s{{shape[0], shape[1], shape[2]}};
  const int64_t n4 = (int64_t)s.d[0] * s.d[1] * s.d[2] * ((Cs + Cl) / 4);
  hipLaunchKernelGGL(upsample_concat_kernel<T>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, skip, lo, out,
                     s, Cs, Cl, stats, gamma, beta, eps);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int upsample_concat_bwd_t(const T* dcat, T* dskip, T* dlo_bn, const int shape[3], int Cs, int Cl, synthsr_stream_t stream) {
  if (!dcat || !dskip || !dlo_bn || bad_shape(shape) || odd_shape(shape) || !ok_c4(Cs) || !ok_c4(Cl))
    return SYNTHSR_EINVAL;
  Shape3 s{{shape[0], shape[1], shape[2]}};
  const int64_t nv = (int64_t)s.d[0] * s.d[1] * s.d[2];
  const int64_t n4 = nv * (Cs / 4) + (nv / 8) * (Cl / 4);
  hipLaunchKernelGGL(upsample_concat_bwd_kernel<T>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, dcat,
                     dskip, dlo_bn, s, Cs, Cl);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int head_loss_fwd_t(const T* x, const int* shape, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b, int K, const float* residual, int res_stride, const int* res_offs, const float* target, float* pred, float* dpred, float* loss, int kind, const int* crop, synthsr_stream_t stream, float* ab = nullptr) {
  if (!x || !shape || !stats || !gamma || !beta || !w || !b || !target || !loss || !ok_c4(C)) return SYNTHSR_EINVAL;
  if (ab && (K != 1 || kind == 2 || C > 120)) return SYNTHSR_EINVAL;  // the fused backward sums exist for the 1-channel l1 / l2 head
  if (shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return SYNTHSR_EINVAL;
  if (kind < 0 || kind > 2 || K < 1 || K > 16 || (kind == 2 && (K & 1))) return SYNTHSR_EINVAL;
  const int NT = kind == 2 ? K / 2 : K;
  if (C > 116) return SYNTHSR_EINVAL;  // LDS: (2 + K) C + 256 (C + 4) floats
  const int64_t nvox = (int64_t)shape[0] * shape[1] * shape[2];
  HeadBox box;
  for (int k = 0; k < 16; ++k) box.res_off[k] = 0;
  if (residual) {
    if (res_stride < 1 || !res_offs) return SYNTHSR_EINVAL;
    for (int k = 0; k < NT; ++k) {
      if (res_offs[k] < 0 || res_offs[k] >= res_stride) return SYNTHSR_EINVAL;
      box.res_off[k] = res_offs[k];
    }
  }
  box.on = crop != nullptr;
  box.d1 = shape[1];
  box.d2 = shape[2];
  int64_t n_in = nvox;
  if (crop) {
    n_in = 1;
    for (int i = 0; i < 3; ++i) {
      if (crop[i] < 0 || crop[3 + i] < 1 || crop[i] + crop[3 + i] > shape[i]) return SYNTHSR_EINVAL;
      box.lo[i] = crop[i];
      box.hi[i] = crop[i] + crop[3 + i];
      n_in *= crop[3 + i];
    }
  } else {
    for (int i = 0; i < 3; ++i) {
      box.lo[i] = 0;
      box.hi[i] = shape[i];
    }
  }
  const size_t smem = ((2 + K) * C + 256 * (C + 4)) * sizeof(float);
  const float inv_n = (float)(1.0 / ((double)n_in * NT));
  const dim3 grid(syn_grid(nvox, 256, head_grid()));
#define SYN_HEAD_FWD(KK, CT)                                                                                                 \
  hipLaunchKernelGGL((head_loss_fwd_kernel<T, KK, CT>), grid, dim3(256), smem, (hipStream_t)stream, x, nvox, C, stats, gamma, beta, \
                     eps, w, b, residual, res_stride, target, pred, dpred, loss, inv_n, kind, box, ab)
  switch (K) {
    case 1:
      if (C == 24) SYN_HEAD_FWD(1, 24);
      else SYN_HEAD_FWD(1, 0);
      break;
    case 2: SYN_HEAD_FWD(2, 0); break;
    case 3: SYN_HEAD_FWD(3, 0); break;
    case 4: SYN_HEAD_FWD(4, 0); break;
    default: {  // 5 <= K <= 16: the padded kernels
      // LDS rule of the wide heads: ((2 + KB) C + KB + 256 (C + 4)) floats of dynamic LDS (KB = 8 for K <= 8, else 16) plus the
      // kernel's static LDS (the deterministic gather's column buffer, 8 KB) must fit the 64 KB a launch gets without an
      // attribute: C <= 48 at both widths, which is also the largest C that launches at K <= 4.  Anything wider is refused
      // here, before the launch.
      const bool k8 = K <= 8;
      const int KB = k8 ? 8 : 16;
      const auto fn = k8 ? head_loss_fwd_wide_kernel<T, 8> : head_loss_fwd_wide_kernel<T, 16>;
      const size_t smem_w = ((size_t)(2 + KB) * C + KB + 256 * (size_t)(C + 4)) * sizeof(float);
      static size_t static_lds[2] = {0, 0};  // per width; the same on every device
      size_t& st = static_lds[k8 ? 0 : 1];
      if (st == 0) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, (const void*)fn) != hipSuccess) return SYNTHSR_ELAUNCH;
        st = fa.sharedSizeBytes > 0 ? fa.sharedSizeBytes : 1;
      }
      if (smem_w + st > 65536) return SYNTHSR_EINVAL;
      const int vec4 = (K % 4 == 0) && ((uintptr_t)pred % 16 == 0) && ((uintptr_t)dpred % 16 == 0);
      hipLaunchKernelGGL(fn, grid, dim3(256), smem_w, (hipStream_t)stream, x, nvox, C, stats, gamma, beta, eps, w, b, K, residual,
                         res_stride, target, pred, dpred, loss, inv_n, kind, box, vec4);
      break;
    }
  }
#undef SYN_HEAD_FWD
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int head_bwd_multi_t(const float* dpred, const T* x, int64_t nvox, int C, int K, const float* stats, const float* gamma, const float* beta, float eps, const float* w, T* dbn, float* dw, float* db, synthsr_stream_t stream) {
  if (!dpred || !x || !stats || !gamma || !beta || !w || !dbn || !dw || !db || nvox < 1 || !ok_c4(C) || K < 2 || K > 16)
    return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  const dim3 grid(syn_grid(n4, RB, head_grid()));
  const size_t smem = (K * C + K) * sizeof(float);
#define SYN_HEAD_BWD(KK)                                                                                             \
  hipLaunchKernelGGL((head_multi_bwd_kernel<T, KK>), grid, dim3(RB), smem, (hipStream_t)stream, dpred, x, n4, C, stats, gamma, \
                     beta, eps, w, dbn, dw, db)
  switch (K) {
    case 2: SYN_HEAD_BWD(2); break;
    case 3: SYN_HEAD_BWD(3); break;
    case 4: SYN_HEAD_BWD(4); break;
    default: {  // 5 <= K <= 16: the padded kernels; LDS A[KB][C] | B[KB] | w[KB][C]
      const bool k8 = K <= 8;
      const int KB = k8 ? 8 : 16;
      const size_t smem_w = ((size_t)2 * KB * C + KB) * sizeof(float);
      if (smem_w > 48 * 1024) return SYNTHSR_EINVAL;  // C <= 380 at KB = 16; the forward kernel stops far below
      const int vec4 = (K % 4 == 0) && ((uintptr_t)dpred % 16 == 0);
      hipLaunchKernelGGL((k8 ? head_multi_bwd_wide_kernel<T, 8> : head_multi_bwd_wide_kernel<T, 16>), grid, dim3(RB), smem_w,
                         (hipStream_t)stream, dpred, x, n4, C, K, stats, gamma, beta, eps, w, dbn, dw, db, vec4);
      break;
    }
  }
#undef SYN_HEAD_BWD
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
int head_bwd_ex_t(const float* dpred, const T* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, T* dbn, float* dw, float* db, float* bn_sums, synthsr_stream_t stream) {
  if (!dpred || !x || !stats || !gamma || !beta || !w || !dw || !db || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(head_bwd_kernel<T>, dim3(syn_grid(n4, RB, red_grid())), dim3(RB), (C + 1) * sizeof(float),
                     (hipStream_t)stream, dpred, x, n4, C, stats, gamma, beta, eps, w, dbn, dw, db, bn_sums);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
static int scale_channels_t(const T* x, T* out, int64_t nvox, int C, const float* scale, int64_t nvox_per_sample, synthsr_stream_t stream) {
  if (!x || !out || !scale || nvox < 1 || !ok_c4(C) || nvox_per_sample < 1 || (nvox % nvox_per_sample) != 0) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(scale_channels_kernel<T>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, x, out, n4, C / 4, scale,
                     nvox_per_sample * (C / 4));
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

// ---- the softmax-head entry points that exist for float and bf16_t
template <typename T>
static int seg_dice_bwd_t(const float* probs, const int32_t* seg, int64_t nvox, int C, int N, const float* w,
                          const int32_t* cls_idx, const int32_t* cls_gt, int K, const float* sums, float scale, T* dbn,
                          synthsr_stream_t stream) {
  if (!probs || !seg || !w || !cls_idx || !cls_gt || !sums || !dbn || nvox < 1 || C < 1 || C > SEG_MAXC || N < 1 ||
      N > SEG_MAXN || K < 1 || K > SEG_MAXK)
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_dice_bwd_kernel<T>, dim3(syn_grid(nvox, 256)), dim3(256), 0, (hipStream_t)stream, probs, seg, nvox, C,
                     N, w, cls_idx, cls_gt, K, sums, scale, dbn);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

// limits of the tile kernels below (checked before any launch): C <= 64 in whole channel quads, N <= 64, x aligned to the
// vector load of one channel quad: 16 bytes for float, 8 bytes for bf16 (xalign)
static bool shd_ok(int64_t nvox, int C, int N, int lut_n, const void* x, int xalign = 16) {
  return nvox >= 1 && C >= 4 && C <= SEG_MAXC && (C % 4) == 0 && N >= 1 && N <= SEG_MAXN && lut_n >= 1 &&
         ((uintptr_t)x % xalign) == 0;
}

// the two label-map kernels: the limits of the Dice head, at least two classes; T = float | bf16_t, the element type of x
template <typename T>
static bool shd_label_ok(int64_t nvox, int C, int N, const T* x) { return N >= 2 && shd_ok(nvox, C, N, 1, x, 4 * sizeof(T)); }

template <typename T>
static int seg_head_argmax_t(const T* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                             float eps, const float* w, const float* b, int N, const int32_t* labels, int32_t* out,
                             synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !labels || !out || !shd_label_ok(nvox, C, N, x)) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_argmax_kernel<T>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdFwdLds(C, N, false).total * sizeof(float), (hipStream_t)stream, x, nvox, C, stats, gamma, beta, eps, w, b, N,
                     labels, out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

template <typename T>
static int seg_head_tta_argmax_t(const T* x, const int* shape, int C, const float* stats, const float* gamma,
                                 const float* beta, float eps, const float* w, const float* b, int N, const int32_t* labels,
                                 const float* prev, const int32_t* perm, int32_t* out, float* probs_out,
                                 synthsr_stream_t stream) {
  if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return SYNTHSR_EINVAL;
  const int64_t plane = (int64_t)shape[1] * shape[2], nvox = plane * shape[0];
  if (!x || !stats || !gamma || !beta || !w || !b || !labels || !prev || !perm || !out || !shd_label_ok(nvox, C, N, x))
    return SYNTHSR_EINVAL;
  if (probs_out) {  // written at the mirrored voxel while other workgroups still read prev: the two may not share memory
    const uintptr_t p0 = (uintptr_t)prev, q0 = (uintptr_t)probs_out, bytes = (uintptr_t)nvox * N * sizeof(float);
    if (p0 < q0 + bytes && q0 < p0 + bytes) return SYNTHSR_EINVAL;
  }
  hipLaunchKernelGGL(seg_head_tta_argmax_kernel<T>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdFwdLds(C, N, false).total * sizeof(float), (hipStream_t)stream, x, nvox, C, stats, gamma, beta, eps, w, b, N,
                     labels, prev, perm, shape[0], plane, out, probs_out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

extern "C" {

// ELU / ReLU backward (act 1 ELU, 3 ReLU; anything else SYNTHSR_EINVAL): four entry-point families on the one launcher.  The
// ELU-named exports (below) are these with act = 1.
#define BF(p) ((const bf16_t*)(p))
int synthsr_act_bwd(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C, int act,
                    synthsr_stream_t stream) {
  return act_bwd_t<float>(0, dy, dy2, y, dz, dbias, nvox, C, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, 0, act, stream);
}
int synthsr_act_bwd_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C, int act,
                         synthsr_stream_t stream) {
  return act_bwd_t<bf16_t>(0, BF(dy), BF(dy2), BF(y), (bf16_t*)dz, dbias, nvox, C, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr,
                           nullptr, 0, act, stream);
}
int synthsr_bn_act_bwd(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C,
                       const float* stats, const float* gamma, float eps, const float* sums, int act, synthsr_stream_t stream) {
  return act_bwd_t<float>(ACT_BN, dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, nullptr, nullptr, nullptr, 0, act, stream);
}
int synthsr_bn_act_bwd_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C,
                            const float* stats, const float* gamma, float eps, const float* sums, int act,
                            synthsr_stream_t stream) {
  return act_bwd_t<bf16_t>(ACT_BN, BF(dy), BF(dy2), BF(y), (bf16_t*)dz, dbias, nvox, C, stats, gamma, eps, sums, nullptr, nullptr,
                           nullptr, 0, act, stream);
}
int synthsr_bn_act_bwd_head(const float* dpred, const float* whead, const float* y, float* dz, float* dbias, int64_t nvox,
                            int C, const float* stats, const float* gamma, float eps, const float* sums, int act,
                            synthsr_stream_t stream) {
  return act_bwd_t<float>(ACT_BN | ACT_HEAD, nullptr, nullptr, y, dz, dbias, nvox, C, stats, gamma, eps, sums, dpred, whead, nullptr,
                          0, act, stream);
}
int synthsr_bn_act_bwd_head_bf16(const float* dpred, const float* whead, const void* y, void* dz, float* dbias, int64_t nvox,
                                 int C, const float* stats, const float* gamma, float eps, const float* sums, int act,
                                 synthsr_stream_t stream) {
  return act_bwd_t<bf16_t>(ACT_BN | ACT_HEAD, nullptr, nullptr, BF(y), (bf16_t*)dz, dbias, nvox, C, stats, gamma, eps, sums, dpred,
                           whead, nullptr, 0, act, stream);
}
int synthsr_act_bwd_drop(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C,
                         const float* stats, const float* gamma, float eps, const float* sums, const float* dpred,
                         const float* whead, const float* drop, int64_t nvox_per_sample, int act, synthsr_stream_t stream) {
  return act_bwd_t<float>(ACT_DROP, dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, dpred, whead, drop, nvox_per_sample, act,
                          stream);
}
int synthsr_act_bwd_drop_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C,
                              const float* stats, const float* gamma, float eps, const float* sums, const float* dpred,
                              const float* whead, const float* drop, int64_t nvox_per_sample, int act, synthsr_stream_t stream) {
  return act_bwd_t<bf16_t>(ACT_DROP, BF(dy), BF(dy2), BF(y), (bf16_t*)dz, dbias, nvox, C, stats, gamma, eps, sums, dpred, whead, drop,
                           nvox_per_sample, act, stream);
}
int synthsr_bn_pool_act_bwd(const float* dpool, const float* y, const float* dy2, float* dz, float* dbias, const int shape[3],
                            int C, const float* stats, const float* gamma, const float* beta, const float* sums, float eps,
                            int act, synthsr_stream_t stream) {
  return bn_pool_elu_bwd_t<float>(dpool, y, dy2, dz, dbias, shape, C, stats, gamma, beta, sums, eps, stream, act);
}
int synthsr_bn_pool_act_bwd_bf16(const void* dpool, const void* y, const void* dy2, void* dz, float* dbias, const int shape[3],
                                 int C, const float* stats, const float* gamma, const float* beta, const float* sums, float eps,
                                 int act, synthsr_stream_t stream) {
  return bn_pool_elu_bwd_t<bf16_t>(BF(dpool), BF(y), BF(dy2), (bf16_t*)dz, dbias, shape, C, stats, gamma, beta, sums, eps, stream, act);
}
#undef BF

int synthsr_elu_bwd(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C, synthsr_stream_t stream) {
  return synthsr_act_bwd(dy, dy2, y, dz, dbias, nvox, C, 1, stream);
}
int synthsr_elu_bwd_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C, synthsr_stream_t stream) {
  return synthsr_act_bwd_bf16(dy, dy2, y, dz, dbias, nvox, C, 1, stream);
}
int synthsr_bn_elu_bwd(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C, const float* stats, const float* gamma, float eps, const float* sums, synthsr_stream_t stream) {
  return synthsr_bn_act_bwd(dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, 1, stream);
}
int synthsr_bn_elu_bwd_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C, const float* stats, const float* gamma, float eps, const float* sums, synthsr_stream_t stream) {
  return synthsr_bn_act_bwd_bf16(dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, 1, stream);
}
int synthsr_bn_elu_bwd_head(const float* dpred, const float* whead, const float* y, float* dz, float* dbias, int64_t nvox, int C, const float* stats, const float* gamma, float eps, const float* sums, synthsr_stream_t stream) {
  return synthsr_bn_act_bwd_head(dpred, whead, y, dz, dbias, nvox, C, stats, gamma, eps, sums, 1, stream);
}
int synthsr_bn_elu_bwd_head_bf16(const float* dpred, const float* whead, const void* y, void* dz, float* dbias, int64_t nvox, int C, const float* stats, const float* gamma, float eps, const float* sums, synthsr_stream_t stream) {
  return synthsr_bn_act_bwd_head_bf16(dpred, whead, y, dz, dbias, nvox, C, stats, gamma, eps, sums, 1, stream);
}
int synthsr_elu_bwd_drop(const float* dy, const float* dy2, const float* y, float* dz, float* dbias, int64_t nvox, int C,
                         const float* stats, const float* gamma, float eps, const float* sums, const float* dpred,
                         const float* whead, const float* drop, int64_t nvox_per_sample, synthsr_stream_t stream) {
  return synthsr_act_bwd_drop(dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, dpred, whead, drop, nvox_per_sample, 1, stream);
}
int synthsr_elu_bwd_drop_bf16(const void* dy, const void* dy2, const void* y, void* dz, float* dbias, int64_t nvox, int C,
                              const float* stats, const float* gamma, float eps, const float* sums, const float* dpred,
                              const float* whead, const float* drop, int64_t nvox_per_sample, synthsr_stream_t stream) {
  return synthsr_act_bwd_drop_bf16(dy, dy2, y, dz, dbias, nvox, C, stats, gamma, eps, sums, dpred, whead, drop, nvox_per_sample, 1, stream);
}
int synthsr_bn_pool_elu_bwd(const float* dpool, const float* y, const float* dy2, float* dz, float* dbias, const int shape[3],
                            int C, const float* stats, const float* gamma, const float* beta, const float* sums, float eps,
                            synthsr_stream_t stream) {
  return synthsr_bn_pool_act_bwd(dpool, y, dy2, dz, dbias, shape, C, stats, gamma, beta, sums, eps, 1, stream);
}
int synthsr_bn_pool_elu_bwd_bf16(const void* dpool, const void* y, const void* dy2, void* dz, float* dbias, const int shape[3],
                                 int C, const float* stats, const float* gamma, const float* beta, const float* sums, float eps,
                                 synthsr_stream_t stream) {
  return synthsr_bn_pool_act_bwd_bf16(dpool, y, dy2, dz, dbias, shape, C, stats, gamma, beta, sums, eps, 1, stream);
}

int synthsr_scale_channels(const float* x, float* out, int64_t nvox, int C, const float* scale, int64_t nvox_per_sample,
                           synthsr_stream_t stream) {
  return scale_channels_t<float>(x, out, nvox, C, scale, nvox_per_sample, stream);
}
int synthsr_scale_channels_bf16(const void* x, void* out, int64_t nvox, int C, const float* scale, int64_t nvox_per_sample,
                                synthsr_stream_t stream) {
  return scale_channels_t<bf16_t>((const bf16_t*)x, (bf16_t*)out, nvox, C, scale, nvox_per_sample, stream);
}

int synthsr_bn_stats(const float* x, int64_t nvox, int C, float* stats, double* ws, synthsr_stream_t stream) {
  return bn_stats_t<float>(x, nvox, C, stats, ws, stream);
}
int synthsr_bn_stats_bf16(const void* x, int64_t nvox, int C, float* stats, double* ws, synthsr_stream_t stream) {
  return bn_stats_t<bf16_t>((const bf16_t*)x, nvox, C, stats, ws, stream);
}

// mean / variance from per-workgroup partial sums: partial[nwg][2C] (sum | sum of squares), accumulated in double
__global__ void bn_stats_partials_kernel(const float* __restrict__ partial, int nwg, float* __restrict__ stats, int C,
                                         double inv_n) {
  const int c = blockIdx.x;  // one block per channel
  double a = 0.0, q = 0.0;
  for (int b = threadIdx.x; b < nwg; b += blockDim.x) {
    a += (double)partial[(size_t)b * 2 * C + c];
    q += (double)partial[(size_t)b * 2 * C + C + c];
  }
  __shared__ double sa[64], sq[64];
  sa[threadIdx.x] = a;
  sq[threadIdx.x] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 64; ++i) {
      a += sa[i];
      q += sq[i];
    }
    const double m = a * inv_n;
    double v = q * inv_n - m * m;
    if (v < 0.0) v = 0.0;
    stats[c] = (float)m;
    stats[C + c] = (float)v;
  }
}

int synthsr_bn_stats_from_partials(const float* partial, int nwg, int64_t nvox, int C, float* stats,
                                   synthsr_stream_t stream) {
  if (!partial || !stats || nwg < 1 || nvox < 1 || C < 1) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(bn_stats_partials_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, partial, nwg, stats, C,
                     1.0 / (double)nvox);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_bn_apply(const float* x, float* y, int64_t nvox, int C, const float* stats, const float* gamma,
                     const float* beta, float eps, synthsr_stream_t stream) {
  if (!x || !y || !stats || !gamma || !beta || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(bn_apply_kernel<float>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n4, C, stats,
                     gamma, beta, eps);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}
int synthsr_bn_apply_bf16(const void* x, void* y, int64_t nvox, int C, const float* stats, const float* gamma,
                          const float* beta, float eps, synthsr_stream_t stream) {
  if (!x || !y || !stats || !gamma || !beta || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(bn_apply_kernel<bf16_t>, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (bf16_t*)y, n4, C, stats, gamma, beta, eps);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_bn_maxpool(const float* x, float* y, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return bn_maxpool_t<float>(x, y, shape, C, stats, gamma, beta, eps, stream);
}
int synthsr_bn_maxpool_bf16(const void* x, void* y, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return bn_maxpool_t<bf16_t>((const bf16_t*)x, (bf16_t*)y, shape, C, stats, gamma, beta, eps, stream);
}

int synthsr_bn_maxpool_bwd(const float* dy, const float* x, float* dbn, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return bn_maxpool_bwd_ex_t<float>(dy, x, dbn, shape, C, stats, gamma, beta, eps, nullptr, stream);
}
int synthsr_bn_maxpool_bwd_bf16(const void* dy, const void* x, void* dbn, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return bn_maxpool_bwd_ex_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dbn, shape, C, stats, gamma, beta, eps, nullptr, stream);
}

int synthsr_bn_maxpool_bwd_ex(const float* dy, const float* x, float* dbn, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, float* sums, synthsr_stream_t stream) {
  return bn_maxpool_bwd_ex_t<float>(dy, x, dbn, shape, C, stats, gamma, beta, eps, sums, stream);
}
int synthsr_bn_maxpool_bwd_ex_bf16(const void* dy, const void* x, void* dbn, const int shape[3], int C, const float* stats, const float* gamma, const float* beta, float eps, float* sums, synthsr_stream_t stream) {
  return bn_maxpool_bwd_ex_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dbn, shape, C, stats, gamma, beta, eps, sums, stream);
}

int synthsr_bn_bwd_reduce(const float* dy, const float* x, int64_t nvox, int C, const float* stats, float eps, float* sums, synthsr_stream_t stream) {
  return bn_bwd_reduce_t<float>(dy, x, nvox, C, stats, eps, sums, stream);
}
int synthsr_bn_bwd_reduce_bf16(const void* dy, const void* x, int64_t nvox, int C, const float* stats, float eps, float* sums, synthsr_stream_t stream) {
  return bn_bwd_reduce_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, nvox, C, stats, eps, sums, stream);
}

int synthsr_bn_bwd_apply(const float* dy, const float* x, float* dx, int64_t nvox, int C, const float* stats,
                         const float* gamma, float eps, const float* sums, synthsr_stream_t stream) {
  if (!dy || !x || !dx || !stats || !gamma || !sums || nvox < 1 || !ok_c4(C)) return SYNTHSR_EINVAL;
  const int64_t n4 = nvox * (C / 4);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(syn_grid(n4, 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, n4, C,
                     stats, gamma, eps, sums, (float)(1.0 / (double)nvox));
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_upsample_concat(const float* skip, const float* lo, float* out, const int shape[3], int Cs, int Cl, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return upsample_concat_t<float>(skip, lo, out, shape, Cs, Cl, stats, gamma, beta, eps, stream);
}
int synthsr_upsample_concat_bf16(const void* skip, const void* lo, void* out, const int shape[3], int Cs, int Cl, const float* stats, const float* gamma, const float* beta, float eps, synthsr_stream_t stream) {
  return upsample_concat_t<bf16_t>((const bf16_t*)skip, (const bf16_t*)lo, (bf16_t*)out, shape, Cs, Cl, stats, gamma, beta, eps, stream);
}

int synthsr_upsample_concat_bwd(const float* dcat, float* dskip, float* dlo_bn, const int shape[3], int Cs, int Cl, synthsr_stream_t stream) {
  return upsample_concat_bwd_t<float>(dcat, dskip, dlo_bn, shape, Cs, Cl, stream);
}
int synthsr_upsample_concat_bwd_bf16(const void* dcat, void* dskip, void* dlo_bn, const int shape[3], int Cs, int Cl, synthsr_stream_t stream) {
  return upsample_concat_bwd_t<bf16_t>((const bf16_t*)dcat, (bf16_t*)dskip, (bf16_t*)dlo_bn, shape, Cs, Cl, stream);
}

int synthsr_head_loss_fwd(const float* x, const int* shape, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b, int K, const float* residual, int res_stride, const int* res_offs, const float* target, float* pred, float* dpred, float* loss, int kind, const int* crop, synthsr_stream_t stream) {
  return head_loss_fwd_t<float>(x, shape, C, stats, gamma, beta, eps, w, b, K, residual, res_stride, res_offs, target, pred, dpred, loss, kind, crop, stream);
}
int synthsr_head_loss_fwd_ab(const float* x, const int* shape, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b, const float* residual, int res_stride, int res_off, const float* target, float* pred, float* dpred, float* loss, int kind, const int* crop, float* ab, synthsr_stream_t stream) {
  if (!ab) return SYNTHSR_EINVAL;
  return head_loss_fwd_t<float>(x, shape, C, stats, gamma, beta, eps, w, b, 1, residual, res_stride, &res_off, target, pred, dpred, loss, kind, crop, stream, ab);
}
int synthsr_head_loss_fwd_ab_bf16(const void* x, const int* shape, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b, const float* residual, int res_stride, int res_off, const float* target, float* pred, float* dpred, float* loss, int kind, const int* crop, float* ab, synthsr_stream_t stream) {
  if (!ab) return SYNTHSR_EINVAL;
  return head_loss_fwd_t<bf16_t>((const bf16_t*)x, shape, C, stats, gamma, beta, eps, w, b, 1, residual, res_stride, &res_off, target, pred, dpred, loss, kind, crop, stream, ab);
}
int synthsr_head_bwd_from_sums(const float* ab, int C, const float* gamma, const float* beta, const float* w, float* dw, float* db, float* bn_sums, synthsr_stream_t stream) {
  if (!ab || !gamma || !beta || !w || !dw || !db || C < 1) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(head_ab_finish_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, ab, C, gamma, beta, w, dw, db, bn_sums);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}
int synthsr_head_loss_fwd_bf16(const void* x, const int* shape, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, const float* b, int K, const float* residual, int res_stride, const int* res_offs, const float* target, float* pred, float* dpred, float* loss, int kind, const int* crop, synthsr_stream_t stream) {
  return head_loss_fwd_t<bf16_t>((const bf16_t*)x, shape, C, stats, gamma, beta, eps, w, b, K, residual, res_stride, res_offs, target, pred, dpred, loss, kind, crop, stream);
}

int synthsr_head_l1_fwd(const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                        float eps, const float* w, const float* b, const float* residual, int res_stride, int res_off,
                        const float* target, float* pred, float* dpred, float* loss, synthsr_stream_t stream) {
  if (nvox < 1 || nvox >= (1ll << 31)) return SYNTHSR_EINVAL;
  const int shape[3] = {1, 1, (int)nvox};
  return synthsr_head_loss_fwd(x, shape, C, stats, gamma, beta, eps, w, b, 1, residual, res_stride, &res_off, target, pred,
                               dpred, loss, 0, nullptr, stream);
}

int synthsr_head_bwd_multi(const float* dpred, const float* x, int64_t nvox, int C, int K, const float* stats, const float* gamma, const float* beta, float eps, const float* w, float* dbn, float* dw, float* db, synthsr_stream_t stream) {
  return head_bwd_multi_t<float>(dpred, x, nvox, C, K, stats, gamma, beta, eps, w, dbn, dw, db, stream);
}
int synthsr_head_bwd_multi_bf16(const float* dpred, const void* x, int64_t nvox, int C, int K, const float* stats, const float* gamma, const float* beta, float eps, const float* w, void* dbn, float* dw, float* db, synthsr_stream_t stream) {
  return head_bwd_multi_t<bf16_t>(dpred, (const bf16_t*)x, nvox, C, K, stats, gamma, beta, eps, w, (bf16_t*)dbn, dw, db, stream);
}

int synthsr_head_bwd_ex(const float* dpred, const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, float* dbn, float* dw, float* db, float* bn_sums, synthsr_stream_t stream) {
  return head_bwd_ex_t<float>(dpred, x, nvox, C, stats, gamma, beta, eps, w, dbn, dw, db, bn_sums, stream);
}
int synthsr_head_bwd_ex_bf16(const float* dpred, const void* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, void* dbn, float* dw, float* db, float* bn_sums, synthsr_stream_t stream) {
  return head_bwd_ex_t<bf16_t>(dpred, (const bf16_t*)x, nvox, C, stats, gamma, beta, eps, w, (bf16_t*)dbn, dw, db, bn_sums, stream);
}

int synthsr_head_bwd(const float* dpred, const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, float* dbn, float* dw, float* db, synthsr_stream_t stream) {
  return dbn ? synthsr_head_bwd_ex(dpred, x, nvox, C, stats, gamma, beta, eps, w, dbn, dw, db, nullptr, stream) : SYNTHSR_EINVAL;
}
int synthsr_head_bwd_bf16(const float* dpred, const void* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta, float eps, const float* w, void* dbn, float* dw, float* db, synthsr_stream_t stream) {
  return dbn ? synthsr_head_bwd_ex_bf16(dpred, x, nvox, C, stats, gamma, beta, eps, w, dbn, dw, db, nullptr, stream) : SYNTHSR_EINVAL;
}

int synthsr_seg_head_fwd(const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                         float eps, const float* w, const float* b, int N, float* probs, synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !probs || nvox < 1 || C < 1 || C > SEG_MAXC || N < 1 || N > SEG_MAXN)
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_fwd_kernel, dim3(syn_grid(nvox, 256)), dim3(256), 0, (hipStream_t)stream, x, nvox, C, stats,
                     gamma, beta, eps, w, b, N, probs);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_dice_sums(const float* probs, const int32_t* seg, int64_t nvox, int N, const int32_t* cls_idx,
                          const int32_t* cls_gt, int K, float* sums, synthsr_stream_t stream) {
  if (!probs || !seg || !cls_idx || !cls_gt || !sums || nvox < 1 || N < 1 || N > SEG_MAXN || K < 1 || K > SEG_MAXK)
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_dice_sums_kernel, dim3(syn_grid(nvox, 256, 1024)), dim3(256), 0, (hipStream_t)stream, probs, seg,
                     nvox, N, cls_idx, cls_gt, K, sums);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_dice_bwd(const float* probs, const int32_t* seg, int64_t nvox, int C, int N, const float* w,
                         const int32_t* cls_idx, const int32_t* cls_gt, int K, const float* sums, float scale, float* dbn,
                         synthsr_stream_t stream) {
  return seg_dice_bwd_t<float>(probs, seg, nvox, C, N, w, cls_idx, cls_gt, K, sums, scale, dbn, stream);
}
int synthsr_seg_dice_bwd_bf16(const float* probs, const int32_t* seg, int64_t nvox, int C, int N, const float* w,
                              const int32_t* cls_idx, const int32_t* cls_gt, int K, const float* sums, float scale, void* dbn,
                              synthsr_stream_t stream) {
  return seg_dice_bwd_t<bf16_t>(probs, seg, nvox, C, N, w, cls_idx, cls_gt, K, sums, scale, (bf16_t*)dbn, stream);
}

// posteriors of a bf16 feature map on the tile body (the fp32 synthsr_seg_head_fwd keeps its one-thread-per-voxel kernel)
int synthsr_seg_head_fwd_bf16(const void* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                              float eps, const float* w, const float* b, int N, float* probs, synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !probs || !shd_ok(nvox, C, N, 1, x, 8)) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_fwd_bf16_kernel, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdFwdLds(C, N, false).total * sizeof(float), (hipStream_t)stream, (const bf16_t*)x, nvox, C, stats, gamma,
                     beta, eps, w, b, N, probs);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_head_dice_fwd(const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                              float eps, const float* w, const float* b, int N, const int32_t* seg, const int32_t* lut,
                              int lut_n, float* probs, float* sums, synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !seg || !lut || !probs || !sums || !shd_ok(nvox, C, N, lut_n, x))
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_dice_fwd_kernel<false>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdFwdLds(C, N, true).total * sizeof(float), (hipStream_t)stream, x, nvox, C, stats, gamma, beta, eps, w, b, N,
                     seg, lut, lut_n, probs, sums, (const uint64_t*)nullptr, 0.f);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

// the weighted soft Dice: sums [3 N]; mask may be NULL (class weights without boundary weighting)
int synthsr_seg_head_dice_fwd_weighted(const float* x, int64_t nvox, int C, const float* stats, const float* gamma,
                                       const float* beta, float eps, const float* w, const float* b, int N, const int32_t* seg,
                                       const int32_t* lut, int lut_n, const uint64_t* mask, float boundary_weights, float* probs,
                                       float* sums, synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !seg || !lut || !probs || !sums || !shd_ok(nvox, C, N, lut_n, x) ||
      ((uintptr_t)mask % 8) != 0)
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_dice_fwd_kernel<true>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdFwdLds(C, N, true, true).total * sizeof(float), (hipStream_t)stream, x, nvox, C, stats, gamma, beta, eps,
                     w, b, N, seg, lut, lut_n, probs, sums, mask, boundary_weights);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_boundary_mask(const int32_t* seg, const int* shape, const int32_t* lut, int lut_n, int N, int boundary_dist,
                              int skip_background, uint64_t* mask, synthsr_stream_t stream) {
  if (!seg || !shape || !lut || !mask || lut_n < 1 || N < 1 || N > SEG_MAXN || boundary_dist < 1 || boundary_dist > SBM_MAXD ||
      shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || ((uintptr_t)mask % 8) != 0)
    return SYNTHSR_EINVAL;
  const int64_t tiles = syn_cdiv(shape[0], SBM_TZ) * syn_cdiv(shape[1], SBM_TY) * syn_cdiv(shape[2], SBM_TX);
  if (tiles > INT32_MAX) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_boundary_mask_kernel, dim3(syn_grid(tiles, 1, 256 * 32)), dim3(256), 0, (hipStream_t)stream, seg,
                     shape[0], shape[1], shape[2], lut, lut_n, N, boundary_dist, (skip_background && N > 1) ? 1 : 0, mask);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_head_dice_bwd(const float* probs, const int32_t* seg, const int32_t* lut, int lut_n, const float* x, int64_t nvox,
                              int C, int N, const float* stats, const float* gamma, const float* beta, float eps, const float* w,
                              const float* sums, float scale, float* dbn, float* dw, float* db, synthsr_stream_t stream) {
  if (!probs || !seg || !lut || !x || !stats || !gamma || !beta || !w || !sums || !dbn || !dw || !db ||
      !shd_ok(nvox, C, N, lut_n, x))
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_dice_bwd_kernel<false>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdBwdLds(C, N).total * sizeof(float), (hipStream_t)stream, probs, seg, lut, lut_n, x, nvox, C, N, stats, gamma,
                     beta, eps, w, sums, scale, dbn, dw, db, (const uint64_t*)nullptr, 0.f, (const float*)nullptr);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_head_dice_bwd_weighted(const float* probs, const int32_t* seg, const int32_t* lut, int lut_n, const float* x,
                                       int64_t nvox, int C, int N, const float* stats, const float* gamma, const float* beta,
                                       float eps, const float* w, const float* sums, const uint64_t* mask, float boundary_weights,
                                       const float* class_weights, float scale, float* dbn, float* dw, float* db,
                                       synthsr_stream_t stream) {
  if (!probs || !seg || !lut || !x || !stats || !gamma || !beta || !w || !sums || !class_weights || !dbn || !dw || !db ||
      !shd_ok(nvox, C, N, lut_n, x) || ((uintptr_t)mask % 8) != 0)
    return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_head_dice_bwd_kernel<true>, dim3(syn_grid(nvox, SHD_TILE, head_grid())), dim3(256),
                     ShdBwdLds(C, N, true).total * sizeof(float), (hipStream_t)stream, probs, seg, lut, lut_n, x, nvox, C, N,
                     stats, gamma, beta, eps, w, sums, scale, dbn, dw, db, mask, boundary_weights, class_weights);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

// WeightedL2Loss / CrossEntropyLoss on the logits: no posteriors, sums [3]
int synthsr_seg_head_logit_loss_fwd(const float* x, int64_t nvox, int C, const float* stats, const float* gamma,
                                    const float* beta, float eps, const float* w, const float* b, int N, const int32_t* seg,
                                    const int32_t* lut, int lut_n, int kind, float target_value, float* sums,
                                    synthsr_stream_t stream) {
  if (!x || !stats || !gamma || !beta || !w || !b || !seg || !lut || !sums || N < 2 || !shd_ok(nvox, C, N, lut_n, x) ||
      (kind != SYNTHSR_SEG_LOSS_WL2 && kind != SYNTHSR_SEG_LOSS_CE))
    return SYNTHSR_EINVAL;
  const dim3 grid(syn_grid(nvox, SHD_TILE, head_grid()));
  const size_t lds = ShdFwdLds(C, N, true).total * sizeof(float);
  if (kind == SYNTHSR_SEG_LOSS_WL2)
    hipLaunchKernelGGL(seg_head_logit_loss_fwd_kernel<SHD_LOSS_WL2>, grid, dim3(256), lds, (hipStream_t)stream, x, nvox, C, stats,
                       gamma, beta, eps, w, b, N, seg, lut, lut_n, target_value, sums);
  else
    hipLaunchKernelGGL(seg_head_logit_loss_fwd_kernel<SHD_LOSS_CE>, grid, dim3(256), lds, (hipStream_t)stream, x, nvox, C, stats,
                       gamma, beta, eps, w, b, N, seg, lut, lut_n, target_value, sums);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_head_logit_loss_bwd(const int32_t* seg, const int32_t* lut, int lut_n, const float* x, int64_t nvox, int C, int N,
                                    const float* stats, const float* gamma, const float* beta, float eps, const float* w,
                                    const float* b, int kind, float target_value, const float* sums, float scale, float* dbn,
                                    float* dw, float* db, synthsr_stream_t stream) {
  if (!seg || !lut || !x || !stats || !gamma || !beta || !w || !b || !sums || !dbn || !dw || !db || N < 2 ||
      !shd_ok(nvox, C, N, lut_n, x) || (kind != SYNTHSR_SEG_LOSS_WL2 && kind != SYNTHSR_SEG_LOSS_CE))
    return SYNTHSR_EINVAL;
  const dim3 grid(syn_grid(nvox, SHD_TILE, head_grid()));
  const size_t lds = ShdBwdLds(C, N, true).total * sizeof(float);
  if (kind == SYNTHSR_SEG_LOSS_WL2)
    hipLaunchKernelGGL(seg_head_logit_loss_bwd_kernel<SHD_LOSS_WL2>, grid, dim3(256), lds, (hipStream_t)stream, seg, lut, lut_n, x,
                       nvox, C, N, stats, gamma, beta, eps, w, b, target_value, sums, scale, dbn, dw, db);
  else
    hipLaunchKernelGGL(seg_head_logit_loss_bwd_kernel<SHD_LOSS_CE>, grid, dim3(256), lds, (hipStream_t)stream, seg, lut, lut_n, x,
                       nvox, C, N, stats, gamma, beta, eps, w, b, target_value, sums, scale, dbn, dw, db);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_seg_head_argmax(const float* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                            float eps, const float* w, const float* b, int N, const int32_t* labels, int32_t* out,
                            synthsr_stream_t stream) {
  return seg_head_argmax_t<float>(x, nvox, C, stats, gamma, beta, eps, w, b, N, labels, out, stream);
}
int synthsr_seg_head_argmax_bf16(const void* x, int64_t nvox, int C, const float* stats, const float* gamma, const float* beta,
                                 float eps, const float* w, const float* b, int N, const int32_t* labels, int32_t* out,
                                 synthsr_stream_t stream) {
  return seg_head_argmax_t<bf16_t>((const bf16_t*)x, nvox, C, stats, gamma, beta, eps, w, b, N, labels, out, stream);
}

int synthsr_seg_head_tta_argmax(const float* x, const int* shape, int C, const float* stats, const float* gamma,
                                const float* beta, float eps, const float* w, const float* b, int N, const int32_t* labels,
                                const float* prev, const int32_t* perm, int32_t* out, float* probs_out,
                                synthsr_stream_t stream) {
  return seg_head_tta_argmax_t<float>(x, shape, C, stats, gamma, beta, eps, w, b, N, labels, prev, perm, out, probs_out, stream);
}
int synthsr_seg_head_tta_argmax_bf16(const void* x, const int* shape, int C, const float* stats, const float* gamma,
                                     const float* beta, float eps, const float* w, const float* b, int N, const int32_t* labels,
                                     const float* prev, const int32_t* perm, int32_t* out, float* probs_out,
                                     synthsr_stream_t stream) {
  return seg_head_tta_argmax_t<bf16_t>((const bf16_t*)x, shape, C, stats, gamma, beta, eps, w, b, N, labels, prev, perm, out,
                                       probs_out, stream);
}

int synthsr_seg_label_counts(const int32_t* a, const int32_t* b, int64_t nvox, const int32_t* lut, int lut_n, int N,
                             uint64_t* counts, synthsr_stream_t stream) {
  if (!a || !b || !lut || !counts || nvox < 1 || lut_n < 1 || N < 1 || N > SEG_MAXN) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(seg_label_counts_kernel, dim3(syn_grid(nvox, 256, head_grid())), dim3(256), 0, (hipStream_t)stream, a, b,
                     nvox, lut, lut_n, N, reinterpret_cast<unsigned long long*>(counts));
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                      float eps, float grad_scale, synthsr_stream_t stream) {
  if (!p || !g || !m || !v || n < 1) return SYNTHSR_EINVAL;
  hipLaunchKernelGGL(adam_kernel, dim3(syn_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_t, beta1,
                     beta2, eps, grad_scale);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

}  // extern "C"
