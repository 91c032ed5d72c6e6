// What predict.py does to a volume around the U-Net, on the device (include/synthsr_hip.h: "inference volumes"): the anti-aliasing
// blur of volumes.resample_volume one axis at a time, trilinear resampling through a 3 x 4 matrix straight into the padded network
// input (with the minimum and maximum of what was written), min-max normalisation with zero padding, and the flip average, rescale,
// clip and crop of the network output.  All four are memory-bound; nothing is allocated and nothing waits on another workgroup.
//
//   blur, axis 2      blur_last_kernel: a workgroup takes 4 rows x 64 outputs, wave w row w.  The wave stages its 64 + 2 r inputs
//                     (reflected) in LDS with consecutive lanes on consecutive addresses, then lane l sums taps[t] * row[l + t].
//   blur, axis 0 / 1  blur_strided_kernel on the view [outer][n][inner] (axis 1: n0, n1, n2; axis 0: 1, n0, n1 n2): a workgroup takes
//                     32 outputs along the axis x 64 consecutive inner elements.  Lanes always run along the inner (contiguous)
//                     elements, for the staging of the 32 + 2 r input rows as for the stores; lane l reads column l of the LDS tile,
//                     one bank per lane.
//   resample          resample_kernel: tiles of 4 rows x 64 voxels of one output plane, wave w on row w, lanes along k, so a wave
//                     stores 64 consecutive voxels of the destination.  The tile list is cut into one contiguous part per workgroup
//                     (syn_block_range's XCD order); a workgroup keeps a running min / max of what it stored and leaves one pair in
//                     the workspace; minmax_final_kernel (one workgroup) reduces the pairs.  Min and max are exact in any order.
//   normalise / pad   normalise_pad_kernel, postprocess_kernel: one grid-stride sweep each, consecutive lanes on consecutive voxels.
#include "common.h"
#include <cmath>

namespace {

constexpr int VP_MAXSIDE = 1024, VP_MAXR = 16, VP_MAXCD = 2;
constexpr int VP_BR = 4, VP_BK = 64;            // blur along axis 2: rows x outputs of a workgroup
constexpr int VP_TA = 32, VP_TC = 64;           // blur along axis 0 / 1: outputs along the axis x inner elements
constexpr int VP_RJ = 4, VP_RK = 64;            // resample: rows x voxels of a tile
constexpr int VP_MAXWG = SYNTHSR_VOLUME_RESAMPLE_WORKSPACE_BYTES / 8;   // one (min, max) pair per workgroup
static_assert(VP_BR * 64 == 256 && VP_RJ * 64 == 256 && VP_TA % 4 == 0 && VP_MAXWG == 1024, "launch shapes");

struct Taps {
  float w[2 * VP_MAXR + 1];
};

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a), any distance from the grid
__device__ __forceinline__ int vp_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

__global__ __launch_bounds__(256) void blur_last_kernel(const float* __restrict__ in, float* __restrict__ out, const Taps taps,
                                                        const int r, const int rows, const int n2, const int tiles_k) {
  __shared__ float tile[VP_BR][VP_BK + 2 * VP_MAXR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tk = (int)blockIdx.x % tiles_k, tr = (int)blockIdx.x / tiles_k;
  const int row = tr * VP_BR + wave, k0 = tk * VP_BK;
  if (row < rows) {
    const float* rp = in + (int64_t)row * n2;
    for (int e = lane; e < VP_BK + 2 * r; e += 64) tile[wave][e] = rp[vp_reflect(k0 - r + e, n2)];
  }
  __syncthreads();
  const int k = k0 + lane;
  if (row < rows && k < n2) {
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc = fmaf(taps.w[t], tile[wave][lane + t], acc);
    out[(int64_t)row * n2 + k] = acc;
  }
}

__global__ __launch_bounds__(256) void blur_strided_kernel(const float* __restrict__ in, float* __restrict__ out, const Taps taps,
                                                           const int r, const int n, const int inner, const int tiles_a,
                                                           const int tiles_c) {
  __shared__ float tile[VP_TA + 2 * VP_MAXR][VP_TC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = (int)blockIdx.x;
  const int tc = b % tiles_c, br = b / tiles_c, ta = br % tiles_a, o = br / tiles_a;
  const int a0 = ta * VP_TA, c = tc * VP_TC + lane;
  const int na = min(VP_TA, n - a0);   // outputs of this tile along the axis
  const float* base = in + (int64_t)o * n * inner;
  if (c < inner)
    for (int e = wave; e < na + 2 * r; e += 4) tile[e][lane] = base[(int64_t)vp_reflect(a0 - r + e, n) * inner + c];
  __syncthreads();
  if (c >= inner) return;
  float* ob = out + (int64_t)o * n * inner;
  for (int q = wave; q < na; q += 4) {
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc = fmaf(taps.w[t], tile[q + t][lane], acc);
    ob[(int64_t)(a0 + q) * inner + c] = acc;
  }
}

struct RsvArgs {
  double M[12];
  int s[3];        // source sides
  int o[3];        // output sides
  int D1, D2, Cd;  // destination sides 1 and 2, channels
  int off[3], c;   // where the box starts, channel
  int t1, t2;      // tiles along output axes 1 and 2
  int ntiles;
  int zero_outside;
};

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ src, const RsvArgs a, float* __restrict__ dst,
                                                       float* __restrict__ partials) {
  __shared__ float s_mn[4], s_mx[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int pos = (G % 8 == 0) ? (b & 7) * (G >> 3) + (b >> 3) : b;   // one contiguous part of the tile list per XCD
  const int chunk = (a.ntiles + G - 1) / G;
  const int t_lo = pos * chunk, t_hi = min(t_lo + chunk, a.ntiles);
  float mn = INFINITY, mx = -INFINITY;
  for (int t = t_lo; t < t_hi; ++t) {
    const int tk = t % a.t2, tr = t / a.t2, tj = tr % a.t1, i = tr / a.t1;
    const int j = tj * VP_RJ + wave, k = tk * VP_RK + lane;
    if (j >= a.o[1] || k >= a.o[2]) continue;
    int i0[3], i1[3];
    float w[3];
    bool inside = true;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double p = a.M[4 * ax] * (double)i + a.M[4 * ax + 1] * (double)j + a.M[4 * ax + 2] * (double)k + a.M[4 * ax + 3];
      const double top = (double)(a.s[ax] - 1);
      inside = inside && p >= 0.0 && p <= top;
      p = fmin(fmax(p, 0.0), top);   // the indices below stay inside the source in either mode
      i0[ax] = min((int)floor(p), max(a.s[ax] - 2, 0));
      i1[ax] = min(i0[ax] + 1, a.s[ax] - 1);
      w[ax] = (float)(p - (double)i0[ax]);
    }
    float v = 0.f;
    if (inside || !a.zero_outside) {
      const int64_t r00 = ((int64_t)i0[0] * a.s[1] + i0[1]) * a.s[2], r01 = ((int64_t)i0[0] * a.s[1] + i1[1]) * a.s[2];
      const int64_t r10 = ((int64_t)i1[0] * a.s[1] + i0[1]) * a.s[2], r11 = ((int64_t)i1[0] * a.s[1] + i1[1]) * a.s[2];
      const float v000 = src[r00 + i0[2]], v001 = src[r00 + i1[2]], v010 = src[r01 + i0[2]], v011 = src[r01 + i1[2]];
      const float v100 = src[r10 + i0[2]], v101 = src[r10 + i1[2]], v110 = src[r11 + i0[2]], v111 = src[r11 + i1[2]];
      const float u2 = 1.f - w[2], u1 = 1.f - w[1], u0 = 1.f - w[0];
      const float c00 = v000 * u2 + v001 * w[2], c01 = v010 * u2 + v011 * w[2];
      const float c10 = v100 * u2 + v101 * w[2], c11 = v110 * u2 + v111 * w[2];
      const float d0 = c00 * u1 + c01 * w[1], d1 = c10 * u1 + c11 * w[1];
      v = d0 * u0 + d1 * w[0];
    }
    dst[((((int64_t)(a.off[0] + i) * a.D1 + (a.off[1] + j)) * a.D2) + (a.off[2] + k)) * a.Cd + a.c] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = syn_wave_min(mn);
  mx = syn_wave_max(mx);
  if (lane == 0) s_mn[wave] = mn, s_mx[wave] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * b] = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    partials[2 * b + 1] = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  }
}

__global__ __launch_bounds__(256) void minmax_final_kernel(const float* __restrict__ partials, const int n,
                                                           float* __restrict__ minmax) {
  __shared__ float s_mn[4], s_mx[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mn = INFINITY, mx = -INFINITY;
  for (int e = threadIdx.x; e < n; e += 256) {
    mn = fminf(mn, partials[2 * e]);
    mx = fmaxf(mx, partials[2 * e + 1]);
  }
  mn = syn_wave_min(mn);
  mx = syn_wave_max(mx);
  if (lane == 0) s_mn[wave] = mn, s_mx[wave] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    minmax[0] = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    minmax[1] = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  }
}

struct BoxArgs {
  int D[3];     // the buffer the offsets refer to
  int off[3];
  int s[3];     // the box
};

__global__ __launch_bounds__(256) void normalise_pad_kernel(float* __restrict__ dst, const BoxArgs a, const int Cd, const int c,
                                                            const float* __restrict__ minmax, const float gain) {
  const uint32_t nvox = (uint32_t)a.D[0] * a.D[1] * a.D[2];   // <= 2^30
  const float lo = minmax[0], d = minmax[1] - minmax[0];
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < nvox; e += gridDim.x * 256u) {
    const uint32_t z = e % (uint32_t)a.D[2], r = e / (uint32_t)a.D[2], y = r % (uint32_t)a.D[1], x = r / (uint32_t)a.D[1];
    const bool in_box = x - (uint32_t)a.off[0] < (uint32_t)a.s[0] && y - (uint32_t)a.off[1] < (uint32_t)a.s[1] &&
                        z - (uint32_t)a.off[2] < (uint32_t)a.s[2];
    float* p = dst + (int64_t)e * Cd + c;
    float v = 0.f;
    if (in_box && d > 0.f) v = gain * ((*p - lo) / d);
    *p = v;
  }
}

__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ net, const float* __restrict__ netf,
                                                          const BoxArgs a, const float* __restrict__ addend, const int64_t as0,
                                                          const int64_t as1, const int64_t as2, const float sa, const float sb,
                                                          const float lo, const float hi, float* __restrict__ out) {
  const uint32_t nvox = (uint32_t)a.s[0] * a.s[1] * a.s[2];   // <= 2^30
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < nvox; e += gridDim.x * 256u) {
    const uint32_t k = e % (uint32_t)a.s[2], r = e / (uint32_t)a.s[2], j = r % (uint32_t)a.s[1], i = r / (uint32_t)a.s[1];
    const int x = a.off[0] + (int)i, y = a.off[1] + (int)j, z = a.off[2] + (int)k;
    float p = net[((int64_t)x * a.D[1] + y) * a.D[2] + z];
    if (netf) p = 0.5f * p + 0.5f * netf[((int64_t)(a.D[0] - 1 - x) * a.D[1] + y) * a.D[2] + z];
    if (addend) p += addend[(int64_t)i * as0 + (int64_t)j * as1 + (int64_t)k * as2];
    out[e] = fminf(fmaxf(sa * p + sb, lo), hi);
  }
}

bool vp_sides_ok(const int* shape) {
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1 || shape[i] > VP_MAXSIDE) return false;
  return true;
}

// a box of `shape` at `off` inside a buffer of `D`
bool vp_box_ok(const int* D, const int* off, const int* shape) {
  for (int i = 0; i < 3; ++i)
    if (off[i] < 0 || off[i] > D[i] - shape[i]) return false;
  return true;
}

BoxArgs vp_box(const int* D, const int* off, const int* shape) {
  BoxArgs a;
  for (int i = 0; i < 3; ++i) a.D[i] = D[i], a.off[i] = off[i], a.s[i] = shape[i];
  return a;
}

}  // namespace

extern "C" int synthsr_volume_blur_axis(const float* in, const int* shape, int axis, const float* taps, int radius, float* out,
                                        synthsr_stream_t stream) {
  if (!in || !shape || !taps || !out || axis < 0 || axis > 2 || radius < 1 || radius > VP_MAXR || !vp_sides_ok(shape))
    return SYNTHSR_EINVAL;
  const int64_t nvox = (int64_t)shape[0] * shape[1] * shape[2];
  if (in < out + nvox && out < in + nvox) return SYNTHSR_EINVAL;   // the two volumes overlap
  Taps tp;
  for (int t = 0; t <= 2 * VP_MAXR; ++t) {
    tp.w[t] = t <= 2 * radius ? taps[t] : 0.f;
    if (!std::isfinite(tp.w[t])) return SYNTHSR_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (axis == 2) {
    const int rows = shape[0] * shape[1], n2 = shape[2];
    const int tiles_k = (n2 + VP_BK - 1) / VP_BK, tiles_r = (rows + VP_BR - 1) / VP_BR;   // <= 16 * 2^18
    hipLaunchKernelGGL(blur_last_kernel, dim3(tiles_k * tiles_r), dim3(256), 0, st, in, out, tp, radius, rows, n2, tiles_k);
  } else {
    const int outer = axis == 1 ? shape[0] : 1, n = shape[axis], inner = axis == 1 ? shape[2] : shape[1] * shape[2];
    const int tiles_a = (n + VP_TA - 1) / VP_TA, tiles_c = (inner + VP_TC - 1) / VP_TC;   // outer * tiles_a * tiles_c <= 2^19
    hipLaunchKernelGGL(blur_strided_kernel, dim3(outer * tiles_a * tiles_c), dim3(256), 0, st, in, out, tp, radius, n, inner,
                       tiles_a, tiles_c);
  }
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

extern "C" int synthsr_volume_resample(const float* src, const int* src_shape, const double* M, int mode, const int* out_shape,
                                       float* dst, const int* dst_shape, int Cd, const int* offset, int c, float* minmax,
                                       void* workspace, int64_t workspace_bytes, synthsr_stream_t stream) {
  if (!src || !src_shape || !M || !out_shape || !dst || !dst_shape || !offset || !minmax || !workspace ||
      (mode != SYNTHSR_RESAMPLE_CLAMP && mode != SYNTHSR_RESAMPLE_ZERO_OUTSIDE) || Cd < 1 || Cd > VP_MAXCD || c < 0 || c >= Cd ||
      !vp_sides_ok(src_shape) || !vp_sides_ok(out_shape) || !vp_sides_ok(dst_shape) || !vp_box_ok(dst_shape, offset, out_shape) ||
      workspace_bytes < SYNTHSR_VOLUME_RESAMPLE_WORKSPACE_BYTES || ((uintptr_t)workspace & 3))
    return SYNTHSR_EINVAL;
  RsvArgs a;
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(M[i])) return SYNTHSR_EINVAL;
    a.M[i] = M[i];
  }
  for (int i = 0; i < 3; ++i) a.s[i] = src_shape[i], a.o[i] = out_shape[i], a.off[i] = offset[i];
  a.D1 = dst_shape[1], a.D2 = dst_shape[2], a.Cd = Cd, a.c = c;
  a.t1 = (a.o[1] + VP_RJ - 1) / VP_RJ, a.t2 = (a.o[2] + VP_RK - 1) / VP_RK;
  a.ntiles = a.o[0] * a.t1 * a.t2;   // <= 1024 * 256 * 16
  a.zero_outside = mode == SYNTHSR_RESAMPLE_ZERO_OUTSIDE;
  const int G = a.ntiles < VP_MAXWG ? a.ntiles : VP_MAXWG;
  hipStream_t st = (hipStream_t)stream;
  float* partials = (float*)workspace;
  hipLaunchKernelGGL(resample_kernel, dim3(G), dim3(256), 0, st, src, a, dst, partials);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)partials, G, minmax);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

extern "C" int synthsr_volume_normalise_pad(float* dst, const int* dst_shape, int Cd, const int* offset, const int* box_shape,
                                            int c, const float* minmax, float gain, synthsr_stream_t stream) {
  if (!dst || !dst_shape || !offset || !box_shape || !minmax || Cd < 1 || Cd > VP_MAXCD || c < 0 || c >= Cd ||
      !std::isfinite(gain) || !vp_sides_ok(dst_shape) || !vp_sides_ok(box_shape) || !vp_box_ok(dst_shape, offset, box_shape))
    return SYNTHSR_EINVAL;
  const int64_t nvox = (int64_t)dst_shape[0] * dst_shape[1] * dst_shape[2];
  hipLaunchKernelGGL(normalise_pad_kernel, dim3(syn_grid(nvox, 256)), dim3(256), 0, (hipStream_t)stream, dst,
                     vp_box(dst_shape, offset, box_shape), Cd, c, minmax, gain);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

extern "C" int synthsr_sr_postprocess(const float* net, const float* netf, const int* net_shape, const int* offset,
                                      const int* out_shape, const float* addend, const int64_t* addend_stride, float a, float b,
                                      float lo, float hi, float* out, synthsr_stream_t stream) {
  if (!net || !net_shape || !offset || !out_shape || !out || (addend && !addend_stride) || !std::isfinite(a) || !std::isfinite(b) ||
      !(lo <= hi) || !vp_sides_ok(net_shape) || !vp_sides_ok(out_shape) || !vp_box_ok(net_shape, offset, out_shape))
    return SYNTHSR_EINVAL;
  int64_t as[3] = {0, 0, 0};
  if (addend)
    for (int i = 0; i < 3; ++i) {
      if (addend_stride[i] < 1) return SYNTHSR_EINVAL;
      as[i] = addend_stride[i];
    }
  const int64_t nvox = (int64_t)out_shape[0] * out_shape[1] * out_shape[2];
  hipLaunchKernelGGL(postprocess_kernel, dim3(syn_grid(nvox, 256)), dim3(256), 0, (hipStream_t)stream, net, netf,
                     vp_box(net_shape, offset, out_shape), addend, as[0], as[1], as[2], a, b, lo, hi, out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}
