// Label map on another voxel grid straight from the posteriors (include/synthsr_hip.h: synthsr_seg_resample_argmax): every output
// voxel is mapped into the source grid, the eight corner posteriors around it are interpolated in registers, all channels at
// once, and the label of the largest is written.  The resampled posteriors reach memory only when the caller asks for them.
//
// One launch, seg_resample_argmax_kernel<W, CPL>; no workgroup waits on another, no atomics, no LDS, no workspace.
//   tiles      the output is cut into tiles of 4 x 4 x 16 voxels, one workgroup of four waves per tile, wave w on the plane
//              i = w of the tile.  The tile list is dealt to the XCDs in eight contiguous parts (syn_block_range's mapping), so
//              tiles that share source rows meet in one L2.
//   geometry   lane l computes, once, the geometry of voxel (l >> 4, l & 15) of its plane: the position in double, the inside
//              rule, per axis the two source indices (already multiplied by the axis' stride in voxels) and the fp32 weight.
//   passes     the 64 voxels of a plane are worked through in W passes of 64 / W voxels; W lanes share a voxel, lane g of them
//              holds the channels g, g + W, ... (CPL = ceil(N / W) of them), so one load instruction reads W consecutive
//              floats of a source row per voxel.  The geometry comes from the lane that computed it by __shfl.
//   argmax     every lane keeps the first largest of its channels, then log2(W) __shfl_xor steps on (value, channel) in which
//              the lower channel wins on equal values.
// W = 8 for every N ("Label maps on the input's own grid" has the figures of W = 16).
#include "common.h"
#include <climits>
#include <cmath>

namespace {

constexpr int RS_MAXSIDE = 1024, RS_MINN = 2, RS_MAXN = 64;
constexpr int RS_TI = 4, RS_TJ = 4, RS_TK = 16;   // one wave per plane of RS_TJ * RS_TK = 64 voxels
constexpr int RS_W = 8;
static_assert(RS_TI * 64 == 256 && RS_TJ * RS_TK == 64, "launch shape");

struct RsArgs {
  double M[12];
  int lo[3], hi[3];
  int s1, s2;          // source sides 1 and 2
  int o0, o1, o2;      // output sides
  int t1, t2;          // tiles along output axes 1 and 2
  int N;
  int32_t fill_value;
};

template <int W, int CPL>
__global__ __launch_bounds__(256) void seg_resample_argmax_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                                  const RsArgs a, int32_t* __restrict__ out,
                                                                  float* __restrict__ probs_out) {
  constexpr int VPP = 64 / W;   // voxels per pass
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int t = (G % 8 == 0) ? (b & 7) * (G >> 3) + (b >> 3) : b;
  const int tk = t % a.t2, tr = t / a.t2, tj = tr % a.t1, ti = tr / a.t1;
  const int i = ti * RS_TI + wave;
  if (i >= a.o0) return;   // the whole wave: everything below is wave-local
  const int j0 = tj * RS_TJ, k0 = tk * RS_TK;

  // the geometry of this lane's voxel
  int flags, row[6];
  float wgt[3];
  {
    const int j = j0 + (lane >> 4), k = k0 + (lane & 15);
    const bool in_out = j < a.o1 && k < a.o2;
    bool inside = in_out;
    const int stride[3] = {a.s1 * a.s2, a.s2, 1};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double p = a.M[4 * ax] * (double)i + a.M[4 * ax + 1] * (double)j + a.M[4 * ax + 2] * (double)k + a.M[4 * ax + 3];
      const double lo = (double)a.lo[ax], hi = (double)a.hi[ax];
      inside = inside && p >= lo - 0.5 && p <= hi + 0.5;   // false for a NaN
      p = fmin(fmax(p, lo), hi);                            // a NaN becomes lo: the indices below stay inside the box
      const int i0 = min((int)floor(p), max(a.hi[ax] - 1, a.lo[ax]));
      const int i1 = min(i0 + 1, a.hi[ax]);
      wgt[ax] = (float)(p - (double)i0);
      row[2 * ax] = i0 * stride[ax];       // < 2^30 voxels in all
      row[2 * ax + 1] = i1 * stride[ax];
    }
    flags = (in_out ? 1 : 0) | (inside ? 2 : 0);
  }

  const int g = lane % W, N = a.N;
#pragma unroll 1
  for (int pass = 0; pass < W; ++pass) {
    const int src = pass * VPP + lane / W;   // the lane that holds the geometry of this group's voxel
    const int f = __shfl(flags, src);
    int r[6];
    float w[3];
#pragma unroll
    for (int e = 0; e < 6; ++e) r[e] = __shfl(row[e], src);
#pragma unroll
    for (int e = 0; e < 3; ++e) w[e] = __shfl(wgt[e], src);

    float acc[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
    if (f & 2) {
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int cz = corner >> 2, cy = (corner >> 1) & 1, cx = corner & 1;
        const float wt = (cz ? w[0] : 1.f - w[0]) * (cy ? w[1] : 1.f - w[1]) * (cx ? w[2] : 1.f - w[2]);
        const float* rp = probs + (int64_t)(r[cz] + r[2 + cy] + r[4 + cx]) * N + g;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
          if (g + W * c < N) acc[c] = fmaf(wt, rp[W * c], acc[c]);
      }
    }

    float bv = -INFINITY;
    int bn = INT_MAX;   // no channel yet
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int n = g + W * c;
      if (n < N && (bn == INT_MAX || acc[c] > bv)) bv = acc[c], bn = n;
    }
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int on = __shfl_xor(bn, o);
      if (ov > bv || (ov == bv && on < bn)) bv = ov, bn = on;
    }

    if (f & 1) {
      const int v = (i * a.o1 + j0 + (src >> 4)) * a.o2 + k0 + (src & 15);   // < 2^30
      if (g == 0) out[v] = (f & 2) ? labels[bn] : a.fill_value;
      if (probs_out) {
        float* po = probs_out + (int64_t)v * N + g;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
          if (g + W * c < N) po[W * c] = acc[c];   // zeros outside
      }
    }
  }
}

template <int W, int CPL>
int rs_launch(const float* probs, const int32_t* labels, const RsArgs& a, int ntiles, int32_t* out, float* probs_out,
              hipStream_t st) {
  hipLaunchKernelGGL((seg_resample_argmax_kernel<W, CPL>), dim3(ntiles), dim3(256), 0, st, probs, labels, a, out, probs_out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

bool rs_sides_ok(const int* shape) {
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1 || shape[i] > RS_MAXSIDE) return false;
  return true;
}

}  // namespace

extern "C" int synthsr_seg_resample_argmax(const float* probs, const int* src_shape, int N, const int* box, const double* M,
                                           const int* out_shape, const int32_t* labels, int32_t fill_value, int32_t* out,
                                           float* probs_out, synthsr_stream_t stream) {
  if (!probs || !src_shape || !box || !M || !out_shape || !labels || !out || N < RS_MINN || N > RS_MAXN ||
      !rs_sides_ok(src_shape) || !rs_sides_ok(out_shape))
    return SYNTHSR_EINVAL;
  RsArgs a;
  for (int i = 0; i < 3; ++i) {
    if (box[i] < 0 || box[i] > box[3 + i] || box[3 + i] >= src_shape[i]) return SYNTHSR_EINVAL;
    a.lo[i] = box[i];
    a.hi[i] = box[3 + i];
  }
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(M[i])) return SYNTHSR_EINVAL;
    a.M[i] = M[i];
  }
  a.s1 = src_shape[1], a.s2 = src_shape[2];
  a.o0 = out_shape[0], a.o1 = out_shape[1], a.o2 = out_shape[2];
  a.t1 = (a.o1 + RS_TJ - 1) / RS_TJ, a.t2 = (a.o2 + RS_TK - 1) / RS_TK;
  a.N = N;
  a.fill_value = fill_value;
  const int ntiles = (a.o0 + RS_TI - 1) / RS_TI * a.t1 * a.t2;   // <= 256 * 256 * 64
  hipStream_t st = (hipStream_t)stream;
  switch ((N + RS_W - 1) / RS_W) {
    case 1: return rs_launch<RS_W, 1>(probs, labels, a, ntiles, out, probs_out, st);
    case 2: return rs_launch<RS_W, 2>(probs, labels, a, ntiles, out, probs_out, st);
    case 3: return rs_launch<RS_W, 3>(probs, labels, a, ntiles, out, probs_out, st);
    case 4: return rs_launch<RS_W, 4>(probs, labels, a, ntiles, out, probs_out, st);
    case 5: return rs_launch<RS_W, 5>(probs, labels, a, ntiles, out, probs_out, st);
    case 6: return rs_launch<RS_W, 6>(probs, labels, a, ntiles, out, probs_out, st);
    case 7: return rs_launch<RS_W, 7>(probs, labels, a, ntiles, out, probs_out, st);
    default: return rs_launch<RS_W, 8>(probs, labels, a, ntiles, out, probs_out, st);
  }
}
