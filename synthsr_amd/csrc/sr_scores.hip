// Image-quality sums of a super-resolved volume against its ground truth (include/synthsr_hip.h: synthsr_sr_moments,
// synthsr_sr_errors, synthsr_sr_ssim3d).  fp32 volumes [d0][d1][d2] (d2 fastest), an optional int32 mask (a voxel counts where
// mask != 0), results as doubles on the device.
//
// Every reduction is: per thread in fp32 over a few dozen values, per workgroup in fp64 in a fixed order, ONE record of doubles
// per workgroup in the caller's workspace at slot [workgroup id], and a one-workgroup launch that adds the records up in slot
// order in fp64.  No float atomics, no allocation, no state: the same bits run after run, nothing for deterministic mode to do.
//
//   sr_moments_kernel   one pass: n, sums of p', t', p'^2, t'^2, p't' with p' = p - shift_p, t' = t - shift_t, min / max of p, t.
//                       The shift is per WORKGROUP (its first masked voxel), stored in the record; the combine re-bases every
//                       record onto the first non-empty one's shift in fp64.  An offset-dominated volume (1000 + unit noise)
//                       therefore keeps its variance: the fp32 sums only ever see values of the size of the noise.
//   sr_errors_kernel    one pass: sums of |d|, d^2 and max |d| with d = a p + b - t.
//   sr_ssim3d_kernel    the 3-D SSIM, 11^3 Gaussian window (sigma 1.5), 'valid' positions, one launch, no intermediate in HBM.
//
// sr_ssim3d_kernel: a workgroup owns a tile of SS_T1 x SS_T2 = 16 x 32 output positions in axes 1 and 2 and marches along axis 0
// over a chunk of output planes.  Per incoming input plane:
//   stage    the (16 + 10) x (32 + 10) window of x = (a p + b) / L and y = t / L into LDS (rows of 43 floats);
//   pass A   filter along axis 2: a thread takes 4 neighbouring outputs of one row, reads 14 x and 14 y once and forms the five
//            moment fields (x, y, x^2, y^2, x y) -> LDS [5][26][32].  208 of the 256 threads work.  Rows of 43 floats: the 32
//            lanes of a read group are 8 column quads of 4 rows, bank = (11 row + 4 quad + k) mod 32: no conflict;
//   pass B   filter along axis 1: a thread owns the two outputs (2 rp, c), (2 rp + 1, c), reads 12 values per field
//            (lanes = 32 consecutive columns: no conflict);
//   axis 0   the ring lives in registers as 10 running sums per field and output: the in-plane result of input plane z is the
//            tap-(z - zo) term of the output planes zo = z - 10 .. z, so every step finishes one output plane, moves the other
//            sums down one place (the fma writes the neighbouring register: no copies) and opens a new one.  The thread's two
//            outputs sit side by side in register pairs, so this part is packed fp32 fmas with the tap in a scalar register.
// 236 VGPRs, 25.6 KB LDS, no scratch: two workgroups (8 waves) per CU.
// Halo re-read: (26 * 42) / (16 * 32) = 2.13 in-plane, times (len + 10) / len along the march (chunks of >= 24 planes where the
// volume allows); the re-reads of neighbouring tiles come from L2 / Infinity Cache.
#include "common.h"
#include <math.h>

namespace {

constexpr int SRS_MAXSIDE = 4096;
constexpr int SRS_MAXWG = 4096;                           // workgroups (= records) of the two one-pass kernels
constexpr int SRS_MOM = 12, SRS_ERR = 4, SRS_SSIM = 2;    // doubles per record and per result
constexpr int SS_T1 = 16, SS_T2 = 32, SS_W = 11, SS_H1 = SS_T1 + SS_W - 1, SS_H2 = SS_T2 + SS_W - 1, SS_IS = 43;
constexpr int SS_MIN_CHUNK = 24, SS_TARGET_WG = 1024;

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, rounded to fp32
__host__ __device__ constexpr float ss_tap(int k) {
  const int a = k < 5 ? 5 - k : k - 5;
  return a == 0 ? 0.26601172486179436f
       : a == 1 ? 0.2130055377112537f
       : a == 2 ? 0.10936068950970002f
       : a == 3 ? 0.03600077212843083f
       : a == 4 ? 0.007598758135239185f
                : 0.00102838008447911f;
}

bool srs_shape_ok(const int* shape, int min_side) {
  if (!shape) return false;
  for (int i = 0; i < 3; ++i)
    if (shape[i] < min_side || shape[i] > SRS_MAXSIDE) return false;
  return true;
}

struct SsimGrid {
  int n0, n1, n2, t1, t2, nch, len;
  int64_t wgs;
  explicit SsimGrid(const int* shape) {
    n0 = shape[0] - (SS_W - 1);
    n1 = shape[1] - (SS_W - 1);
    n2 = shape[2] - (SS_W - 1);
    t1 = (n1 + SS_T1 - 1) / SS_T1;
    t2 = (n2 + SS_T2 - 1) / SS_T2;
    const int want = (SS_TARGET_WG + t1 * t2 - 1) / (t1 * t2), most = (n0 + SS_MIN_CHUNK - 1) / SS_MIN_CHUNK;
    nch = want < most ? want : most;
    len = (n0 + nch - 1) / nch;
    nch = (n0 + len - 1) / len;   // no empty chunk
    wgs = (int64_t)t1 * t2 * nch;
  }
};

int64_t srs_workspace_bytes(const int* shape) {
  int64_t recs = (int64_t)SRS_MAXWG * SRS_MOM;
  if (srs_shape_ok(shape, SS_W)) {
    const int64_t s = SsimGrid(shape).wgs * SRS_SSIM;
    if (s > recs) recs = s;
  }
  return recs * (int64_t)sizeof(double);
}

// ---- workgroup reductions of 256 threads in fp64: butterfly inside the wave, then the four waves in a fixed order ------------
enum { SRS_SUM = 0, SRS_MIN = 1, SRS_MAX = 2 };
template <int OP>
__device__ __forceinline__ double srs_op(double a, double b) {
  if constexpr (OP == SRS_SUM) return a + b;
  else if constexpr (OP == SRS_MIN) return fmin(a, b);
  else return fmax(a, b);
}
template <int OP>
__device__ __forceinline__ double srs_block(double v, double* s4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = srs_op<OP>(v, __shfl_xor(v, o, 64));
  __syncthreads();   // s4 may still be read by the previous reduction
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return srs_op<OP>(srs_op<OP>(s4[0], s4[1]), srs_op<OP>(s4[2], s4[3]));
}

// the contiguous voxel range [lo, hi) of this workgroup: chunks are multiples of 256
__device__ __forceinline__ void srs_range(int64_t n, int64_t& lo, int64_t& hi) {
  const int64_t chunk = ((n + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  lo = (int64_t)blockIdx.x * chunk;
  if (lo > n) lo = n;
  hi = lo + chunk < n ? lo + chunk : n;
}

// record: n, shift_p, shift_t, S p', S t', S p'^2, S t'^2, S p't', min p, max p, min t, max t
__global__ __launch_bounds__(256) void sr_moments_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                         const int32_t* __restrict__ mask, int64_t n, double* __restrict__ rec) {
  __shared__ int s_first;
  __shared__ double s4[4];
  const int tid = threadIdx.x;
  int64_t lo, hi;
  srs_range(n, lo, hi);
  if (tid == 0) s_first = INT32_MAX;
  __syncthreads();
  for (int64_t base = lo; base < hi; base += 256) {   // the first masked voxel of the range
    const int64_t v = base + tid;
    const int m = (v < hi && (!mask || mask[v] != 0)) ? 1 : 0;
    if (m) atomicMin(&s_first, (int)(v - lo));
    if (__syncthreads_or(m)) break;
  }
  const int first = s_first;
  double* __restrict__ r = rec + (int64_t)blockIdx.x * SRS_MOM;
  if (first == INT32_MAX) {   // nothing masked here (the same in every thread)
    if (tid < SRS_MOM) r[tid] = (tid == 8 || tid == 10) ? (double)INFINITY : ((tid == 9 || tid == 11) ? -(double)INFINITY : 0.0);
    return;
  }
  const float sp = p[lo + first], st = t[lo + first];
  float cnt = 0.f, a_p = 0.f, a_t = 0.f, a_pp = 0.f, a_tt = 0.f, a_pt = 0.f;   // cnt <= 2^24 / 256 per thread: exact
  float mnp = INFINITY, mxp = -INFINITY, mnt = INFINITY, mxt = -INFINITY;
  for (int64_t v = lo + (first & ~255) + tid; v < hi; v += 256) {
    if (mask && mask[v] == 0) continue;
    const float pv = p[v], tv = t[v];
    const float dp = pv - sp, dt = tv - st;
    cnt += 1.f;
    a_p += dp;
    a_t += dt;
    a_pp = fmaf(dp, dp, a_pp);
    a_tt = fmaf(dt, dt, a_tt);
    a_pt = fmaf(dp, dt, a_pt);
    mnp = fminf(mnp, pv);
    mxp = fmaxf(mxp, pv);
    mnt = fminf(mnt, tv);
    mxt = fmaxf(mxt, tv);
  }
  const double o0 = srs_block<SRS_SUM>(cnt, s4), o3 = srs_block<SRS_SUM>(a_p, s4), o4 = srs_block<SRS_SUM>(a_t, s4);
  const double o5 = srs_block<SRS_SUM>(a_pp, s4), o6 = srs_block<SRS_SUM>(a_tt, s4), o7 = srs_block<SRS_SUM>(a_pt, s4);
  const double o8 = srs_block<SRS_MIN>(mnp, s4), o9 = srs_block<SRS_MAX>(mxp, s4);
  const double o10 = srs_block<SRS_MIN>(mnt, s4), o11 = srs_block<SRS_MAX>(mxt, s4);
  if (tid == 0) {
    r[0] = o0; r[1] = sp; r[2] = st; r[3] = o3; r[4] = o4; r[5] = o5;
    r[6] = o6; r[7] = o7; r[8] = o8; r[9] = o9; r[10] = o10; r[11] = o11;
  }
}

// one workgroup: the records in slot order (thread i takes slots i, i + 256, ...), re-based onto the shift of the first non-empty
// record: with e = shift - shift0,  S(p' + e) = S p' + n e,  S(p' + e)^2 = S p'^2 + 2 e S p' + n e^2,  and the mixed term alike
__global__ __launch_bounds__(256) void sr_moments_combine_kernel(const double* __restrict__ rec, int nrec, double* __restrict__ out) {
  __shared__ int s_first;
  __shared__ double s4[4];
  const int tid = threadIdx.x;
  if (tid == 0) s_first = INT32_MAX;
  __syncthreads();
  for (int w = tid; w < nrec; w += 256)
    if (rec[(int64_t)w * SRS_MOM] > 0.0) {
      atomicMin(&s_first, w);
      break;
    }
  __syncthreads();
  const int first = s_first;
  const double P0 = first == INT32_MAX ? 0.0 : rec[(int64_t)first * SRS_MOM + 1];
  const double T0 = first == INT32_MAX ? 0.0 : rec[(int64_t)first * SRS_MOM + 2];
  double n = 0.0, a_p = 0.0, a_t = 0.0, a_pp = 0.0, a_tt = 0.0, a_pt = 0.0;
  double mnp = INFINITY, mxp = -INFINITY, mnt = INFINITY, mxt = -INFINITY;
  for (int w = tid; w < nrec; w += 256) {
    const double* __restrict__ r = rec + (int64_t)w * SRS_MOM;
    const double m = r[0];
    if (m <= 0.0) continue;
    const double ep = r[1] - P0, et = r[2] - T0;
    n += m;
    a_p += r[3] + m * ep;
    a_t += r[4] + m * et;
    a_pp += r[5] + 2.0 * ep * r[3] + m * ep * ep;
    a_tt += r[6] + 2.0 * et * r[4] + m * et * et;
    a_pt += r[7] + et * r[3] + ep * r[4] + m * ep * et;
    mnp = fmin(mnp, r[8]);
    mxp = fmax(mxp, r[9]);
    mnt = fmin(mnt, r[10]);
    mxt = fmax(mxt, r[11]);
  }
  const double o0 = srs_block<SRS_SUM>(n, s4), o3 = srs_block<SRS_SUM>(a_p, s4), o4 = srs_block<SRS_SUM>(a_t, s4);
  const double o5 = srs_block<SRS_SUM>(a_pp, s4), o6 = srs_block<SRS_SUM>(a_tt, s4), o7 = srs_block<SRS_SUM>(a_pt, s4);
  const double o8 = srs_block<SRS_MIN>(mnp, s4), o9 = srs_block<SRS_MAX>(mxp, s4);
  const double o10 = srs_block<SRS_MIN>(mnt, s4), o11 = srs_block<SRS_MAX>(mxt, s4);
  if (tid == 0) {
    out[0] = o0; out[1] = P0; out[2] = T0; out[3] = o3; out[4] = o4; out[5] = o5;
    out[6] = o6; out[7] = o7; out[8] = o8; out[9] = o9; out[10] = o10; out[11] = o11;
  }
}

// record: n, S |d|, S d^2, max |d|
__global__ __launch_bounds__(256) void sr_errors_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                        const int32_t* __restrict__ mask, int64_t n, float a, float b,
                                                        double* __restrict__ rec) {
  __shared__ double s4[4];
  const int tid = threadIdx.x;
  int64_t lo, hi;
  srs_range(n, lo, hi);
  float cnt = 0.f, a_abs = 0.f, a_sq = 0.f, mx = 0.f;
  for (int64_t v = lo + tid; v < hi; v += 256) {
    if (mask && mask[v] == 0) continue;
    const float d = fmaf(a, p[v], b) - t[v];
    cnt += 1.f;
    a_abs += fabsf(d);
    a_sq = fmaf(d, d, a_sq);
    mx = fmaxf(mx, fabsf(d));
  }
  const double o0 = srs_block<SRS_SUM>(cnt, s4), o1 = srs_block<SRS_SUM>(a_abs, s4), o2 = srs_block<SRS_SUM>(a_sq, s4);
  const double o3 = srs_block<SRS_MAX>(mx, s4);
  if (tid == 0) {
    double* __restrict__ r = rec + (int64_t)blockIdx.x * SRS_ERR;
    r[0] = o0; r[1] = o1; r[2] = o2; r[3] = o3;
  }
}

// one workgroup: out[q] = the records' column q added up (q < nsum) or their maximum (nsum <= q < NQ), in slot order
template <int NQ>
__global__ __launch_bounds__(256) void sr_combine_kernel(const double* __restrict__ rec, int64_t nrec, int nsum,
                                                         double* __restrict__ out) {
  __shared__ double s4[4];
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;   // every maximum here is of non-negative values
  for (int64_t w = threadIdx.x; w < nrec; w += 256) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double v = rec[w * NQ + q];
      if (q < nsum) acc[q] += v;
      else acc[q] = fmax(acc[q], v);
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double o = q < nsum ? srs_block<SRS_SUM>(acc[q], s4) : srs_block<SRS_MAX>(acc[q], s4);
    if (threadIdx.x == 0) out[q] = o;
  }
}

// grid (tiles along axis 2, tiles along axis 1, chunks of `len` output planes); record: S ssim, count
__global__ __launch_bounds__(256, 2) void sr_ssim3d_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                        const int32_t* __restrict__ mask, int d0, int d1, int d2, float a, float b,
                                                        float inv_range, int len, float* __restrict__ ssim_map,
                                                        double* __restrict__ rec) {
  __shared__ float sx[SS_H1 * SS_IS], sy[SS_H1 * SS_IS];
  __shared__ __attribute__((aligned(16))) float sa[5 * SS_H1 * SS_T2];
  __shared__ double s4[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = d0 - (SS_W - 1), n1 = d1 - (SS_W - 1), n2 = d2 - (SS_W - 1);
  const int o1 = blockIdx.y * SS_T1, o2 = blockIdx.x * SS_T2;
  const int zo0 = blockIdx.z * len, zo1 = min(zo0 + len, n0);
  const int64_t plane = (int64_t)d1 * d2;
  const int c = tid & 31, rp = tid >> 5;   // this thread's outputs: rows 2 rp and 2 rp + 1 of column c
  const int q1 = o1 + 2 * rp, q2 = o2 + c;
  const bool ok0 = q1 < n1 && q2 < n2, ok1 = q1 + 1 < n1 && q2 < n2;
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  typedef float f2 __attribute__((ext_vector_type(2)));   // the thread's two outputs side by side: packed fp32 fmas
  f2 acc[5][SS_W - 1];
#pragma unroll
  for (int f = 0; f < 5; ++f)
#pragma unroll
    for (int j = 0; j < SS_W - 1; ++j) acc[f][j] = f2{0.f, 0.f};
  float s_sum = 0.f, s_cnt = 0.f;

  for (int z = zo0; z < zo1 + SS_W - 1; ++z) {
    // stage: lanes along axis 2 (42 of 64), the four waves over the 26 rows
#pragma unroll
    for (int i = 0; i < (SS_H1 + 3) / 4; ++i) {
      const int r = wv + 4 * i;
      if (r < SS_H1 && lane < SS_H2) {
        const int i1 = o1 + r, i2 = o2 + lane;
        float x = 0.f, y = 0.f;
        if (i1 < d1 && i2 < d2) {
          const int64_t off = (int64_t)z * plane + (int64_t)i1 * d2 + i2;
          x = fmaf(a, pred[off], b) * inv_range;
          y = truth[off] * inv_range;
        }
        sx[r * SS_IS + lane] = x;
        sy[r * SS_IS + lane] = y;
      }
    }
    __syncthreads();
    // pass A: along axis 2
    if (tid < SS_H1 * (SS_T2 / 4)) {
      const int r = tid >> 3, c0 = (tid & 7) * 4;
      float xs[SS_W + 3], ys[SS_W + 3];
#pragma unroll
      for (int k = 0; k < SS_W + 3; ++k) {
        xs[k] = sx[r * SS_IS + c0 + k];
        ys[k] = sy[r * SS_IS + c0 + k];
      }
      float m[5][4];
#pragma unroll
      for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[f][j] = 0.f;
#pragma unroll
      for (int k = 0; k < SS_W + 3; ++k) {
        const float x = xs[k], y = ys[k];
        const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (k - j >= 0 && k - j < SS_W) {
            const float w = ss_tap(k - j);
            m[0][j] = fmaf(w, x, m[0][j]);
            m[1][j] = fmaf(w, y, m[1][j]);
            m[2][j] = fmaf(w, xx, m[2][j]);
            m[3][j] = fmaf(w, yy, m[3][j]);
            m[4][j] = fmaf(w, xy, m[4][j]);
          }
        }
      }
#pragma unroll
      for (int f = 0; f < 5; ++f)
        *reinterpret_cast<float4*>(&sa[(f * SS_H1 + r) * SS_T2 + c0]) = make_float4(m[f][0], m[f][1], m[f][2], m[f][3]);
    }
    __syncthreads();
    // pass B along axis 1, then axis 0 in registers
    f2 done[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      float v[SS_W + 1];
#pragma unroll
      for (int k = 0; k < SS_W + 1; ++k) v[k] = sa[(f * SS_H1 + 2 * rp + k) * SS_T2 + c];
      float m0 = 0.f, m1 = 0.f;
#pragma unroll
      for (int k = 0; k < SS_W; ++k) {
        m0 = fmaf(ss_tap(k), v[k], m0);
        m1 = fmaf(ss_tap(k), v[k + 1], m1);
      }
      const f2 mv = {m0, m1};
      done[f] = __builtin_elementwise_fma(f2{ss_tap(SS_W - 1), ss_tap(SS_W - 1)}, mv, acc[f][0]);
#pragma unroll
      for (int j = 0; j < SS_W - 2; ++j)
        acc[f][j] = __builtin_elementwise_fma(f2{ss_tap(SS_W - 2 - j), ss_tap(SS_W - 2 - j)}, mv, acc[f][j + 1]);
      acc[f][SS_W - 2] = ss_tap(0) * mv;
    }
    const int zo = z - (SS_W - 1);
    if (zo >= zo0) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u ? ok1 : ok0) {
          const float mux = done[0][u], muy = done[1][u];
          const float vx = done[2][u] - mux * mux, vy = done[3][u] - muy * muy, vxy = done[4][u] - mux * muy;
          const float S = ((2.f * mux * muy + C1) * (2.f * vxy + C2)) / ((mux * mux + muy * muy + C1) * (vx + vy + C2));
          if (ssim_map) ssim_map[((int64_t)zo * n1 + (q1 + u)) * n2 + q2] = S;
          if (!mask || mask[(int64_t)(zo + 5) * plane + (int64_t)(q1 + u + 5) * d2 + (q2 + 5)] != 0) {
            s_sum += S;
            s_cnt += 1.f;
          }
        }
      }
    }
  }
  const double t_sum = srs_block<SRS_SUM>(s_sum, s4), t_cnt = srs_block<SRS_SUM>(s_cnt, s4);
  if (tid == 0) {
    double* __restrict__ r = rec + (int64_t)syn_wg_linear() * SRS_SSIM;
    r[0] = t_sum;
    r[1] = t_cnt;
  }
}

bool srs_args_ok(const float* pred, const float* truth, const int* shape, double* out, void* workspace, int64_t workspace_bytes,
                 int min_side) {
  if (!pred || !truth || !out || !workspace || !srs_shape_ok(shape, min_side) || ((uintptr_t)workspace % 8) != 0) return false;
  return workspace_bytes >= srs_workspace_bytes(shape);
}

}  // namespace

extern "C" {

int64_t synthsr_sr_scores_workspace_bytes(const int* shape) {
  if (!srs_shape_ok(shape, 1)) return SYNTHSR_EINVAL;
  return srs_workspace_bytes(shape);
}

int synthsr_sr_moments(const float* pred, const float* truth, const int32_t* mask, const int* shape, double* out, void* workspace,
                       int64_t workspace_bytes, synthsr_stream_t stream) {
  if (!srs_args_ok(pred, truth, shape, out, workspace, workspace_bytes, 1)) return SYNTHSR_EINVAL;
  const int64_t n = (int64_t)shape[0] * shape[1] * shape[2];
  const int G = syn_grid(n, 256, SRS_MAXWG);
  hipStream_t st = (hipStream_t)stream;
  double* rec = (double*)workspace;
  hipLaunchKernelGGL(sr_moments_kernel, dim3(G), dim3(256), 0, st, pred, truth, mask, n, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(sr_moments_combine_kernel, dim3(1), dim3(256), 0, st, (const double*)rec, G, out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_sr_errors(const float* pred, const float* truth, const int32_t* mask, const int* shape, float a, float b, double* out,
                      void* workspace, int64_t workspace_bytes, synthsr_stream_t stream) {
  if (!srs_args_ok(pred, truth, shape, out, workspace, workspace_bytes, 1)) return SYNTHSR_EINVAL;
  const int64_t n = (int64_t)shape[0] * shape[1] * shape[2];
  const int G = syn_grid(n, 256, SRS_MAXWG);
  hipStream_t st = (hipStream_t)stream;
  double* rec = (double*)workspace;
  hipLaunchKernelGGL(sr_errors_kernel, dim3(G), dim3(256), 0, st, pred, truth, mask, n, a, b, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(sr_combine_kernel<SRS_ERR>, dim3(1), dim3(256), 0, st, (const double*)rec, (int64_t)G, 3, out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

int synthsr_sr_ssim3d(const float* pred, const float* truth, const int32_t* mask, const int* shape, float a, float b,
                      float inv_range, double* out, float* ssim_map, void* workspace, int64_t workspace_bytes,
                      synthsr_stream_t stream) {
  if (!srs_args_ok(pred, truth, shape, out, workspace, workspace_bytes, SS_W)) return SYNTHSR_EINVAL;
  const SsimGrid g(shape);
  hipStream_t st = (hipStream_t)stream;
  double* rec = (double*)workspace;
  hipLaunchKernelGGL(sr_ssim3d_kernel, dim3(g.t2, g.t1, g.nch), dim3(256), 0, st, pred, truth, mask, shape[0], shape[1], shape[2],
                     a, b, inv_range, g.len, ssim_map, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(sr_combine_kernel<SRS_SSIM>, dim3(1), dim3(256), 0, st, (const double*)rec, g.wgs, 2, out);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

}  // extern "C"
