// Surface distances of two label maps (include/synthsr_hip.h: synthsr_seg_surface_dist2): for every surface voxel of class k in
// one map the exact squared Euclidean distance, in voxels, to the nearest surface voxel of class k in the other.  Integers
// only: no result depends on the order in which workgroups run, and no workgroup waits on another.
//
//   seg_surface_kernel        both maps -> one byte per voxel (the class of a surface voxel, 255 otherwise), -1 / INT32_MAX into
//                             the two outputs, and per map and class the bounding box of the surface voxels
//   then, per chunk of SRF_CH classes, both directions in every launch (a slab = one class and one source map):
//   seg_surface_scan_x_kernel pass 1: distance along x (the fastest axis) to the nearest surface voxel of the row, as uint16
//   seg_surface_edt_y_kernel  pass 2: g2(z, y, x) = min_j g1(z, j, x)^2 + (y - j)^2 on lines along y staged in LDS
//   seg_surface_edt_z_kernel  pass 3: min_j g2(j, y, x) + (z - j)^2 on lines along z staged in LDS, evaluated only at the
//                             surface voxels of the class in the OTHER map and written straight into d2_ab / d2_ba
// Every pass works inside the union of the class's two bounding boxes only: all sources and all queries of both directions lie
// in it, so the transform restricted to the box is the transform of the volume.  The grids cover the volume (the host never
// reads the boxes back); a workgroup outside the box of its class leaves at once.
#include "common.h"

namespace {

constexpr int SRF_MAXN = 64, SRF_MAXSIDE = 1024;
constexpr int SRF_CH = 8;             // classes per launch: the workspace holds 2 SRF_CH slabs of 6 bytes per voxel
constexpr int SRF_NONE = 255;         // "no surface voxel here" in the byte maps
constexpr int SRF_FAR = 1 << 30;      // "no surface voxel on this line": SRF_FAR + 1023^2 < 2^31
constexpr int SRF_LDS_INTS = 12288;   // staged lines: 48 KiB
constexpr int SRF_BOX_INTS = 2 * SRF_MAXN * 6;   // [map][class][z0, y0, x0, z1, y1, x1]

// lines of `len` voxels staged TX abreast: the widest power of two that fits the LDS budget
inline int srf_tx(int len) { return len <= 192 ? 64 : (len <= 384 ? 32 : (len <= 768 ? 16 : 8)); }
static_assert(192 * 64 <= SRF_LDS_INTS && 384 * 32 <= SRF_LDS_INTS && 768 * 16 <= SRF_LDS_INTS &&
              SRF_MAXSIDE * 8 <= SRF_LDS_INTS, "a staged line set fits the LDS budget");

struct SrfLayout {
  int64_t nvox, sa, sb, g2, g1, total;
  int ch;
  SrfLayout(const int* shape, int N) {
    nvox = (int64_t)shape[0] * shape[1] * shape[2];
    ch = N < SRF_CH ? N : SRF_CH;
    const int64_t pad = (nvox + 15) / 16 * 16;
    sa = SRF_BOX_INTS * 4;
    sb = sa + pad;
    g2 = sb + pad;
    g1 = g2 + 2 * ch * nvox * 4;
    total = g1 + 2 * ch * nvox * 2;
  }
};

bool srf_shape_ok(const int* shape, int N) {
  if (!shape || N < 1 || N > SRF_MAXN) return false;
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1 || shape[i] > SRF_MAXSIDE) return false;
  return true;
}

// what a workgroup does for class c with source map `src` (0: a, 1: b): nothing unless both maps have surface voxels of the
// class; otherwise the union of the two bounding boxes
struct SrfBox {
  int z0, y0, x0, z1, y1, x1;
  bool active;
};
__device__ __forceinline__ SrfBox srf_box(const int* __restrict__ boxes, int c) {
  const int* p = boxes + c * 6;
  const int* q = boxes + (SRF_MAXN + c) * 6;
  SrfBox r;
  r.active = p[3] >= 0 && q[3] >= 0;
  r.z0 = min(p[0], q[0]);
  r.y0 = min(p[1], q[1]);
  r.x0 = min(p[2], q[2]);
  r.z1 = max(p[3], q[3]);
  r.y1 = max(p[4], q[4]);
  r.x1 = max(p[5], q[5]);
  return r;
}

__global__ void seg_surface_box_init_kernel(int* __restrict__ boxes) {
  for (int e = threadIdx.x; e < SRF_BOX_INTS; e += blockDim.x) boxes[e] = (e % 6) < 3 ? INT32_MAX : -1;
}

__global__ __launch_bounds__(256) void seg_surface_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int d0,
                                                          int d1, int d2, const int32_t* __restrict__ lut, int lut_n, int N,
                                                          uint8_t* __restrict__ sa, uint8_t* __restrict__ sb,
                                                          int32_t* __restrict__ d2_ab, int32_t* __restrict__ d2_ba,
                                                          int* __restrict__ boxes) {
  __shared__ int sbox[SRF_BOX_INTS];
  for (int e = threadIdx.x; e < SRF_BOX_INTS; e += 256) sbox[e] = (e % 6) < 3 ? INT32_MAX : -1;
  __syncthreads();
  const int plane = d1 * d2, nvox = d0 * plane;   // <= 2^30
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    const int z = v / plane, r = v - z * plane, y = r / d2, x = r - y * d2;
    const bool edge = z == 0 || z == d0 - 1 || y == 0 || y == d1 - 1 || x == 0 || x == d2 - 1;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int32_t* __restrict__ map = m ? b : a;
      const int lab = map[v];
      const int k = shd_class(lab, lut, lut_n, N);
      bool surf = false;
      if (k >= 0) {
        surf = edge;
        if (!surf) {   // all six neighbours are inside the volume; an equal label value is an equal class
          const int off[6] = {-plane, plane, -d2, d2, -1, 1};
#pragma unroll
          for (int t = 0; t < 6; ++t) {
            const int nl = map[v + off[t]];
            if (nl != lab && shd_class(nl, lut, lut_n, N) != k) surf = true;
          }
        }
      }
      (m ? sb : sa)[v] = (uint8_t)(surf ? k : SRF_NONE);
      (m ? d2_ba : d2_ab)[v] = surf ? INT32_MAX : -1;
      if (surf) {
        int* bx = sbox + (m * SRF_MAXN + k) * 6;
        atomicMin(bx + 0, z);
        atomicMin(bx + 1, y);
        atomicMin(bx + 2, x);
        atomicMax(bx + 3, z);
        atomicMax(bx + 4, y);
        atomicMax(bx + 5, x);
      }
    }
  }
  __syncthreads();
  // one flush per workgroup; bounds only ever move one way, so a plain (possibly stale) read filters what cannot improve them
  for (int e = threadIdx.x; e < SRF_BOX_INTS; e += 256) {
    const int val = sbox[e];
    if ((e % 6) < 3) {
      if (val < __hip_atomic_load(boxes + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(boxes + e, val);
    } else {
      if (val > __hip_atomic_load(boxes + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(boxes + e, val);
    }
  }
}

// Pass 1.  Grid (rows z * d1 + y, source map).  The row's class bytes sit in registers (x = 256 q + tid: register q of wave w
// is the 64-voxel segment 4 q + w); per class, one ballot per segment gives the row's surface voxels as a bit mask of at most
// 16 words, and the nearest one to the left / right of x is a bit scan over the words: the forward and the backward scan of
// the 1-D distance, one word at a time.
__global__ __launch_bounds__(256) void seg_surface_scan_x_kernel(const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb,
                                                                 int d0, int d1, int d2, const int* __restrict__ boxes, int c0,
                                                                 int nc, uint16_t* __restrict__ g1) {
  __shared__ unsigned long long bits[SRF_CH][16];
  const int row = blockIdx.x, z = row / d1, y = row - z * d1, src = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned need = 0;
  for (int cs = 0; cs < nc; ++cs) {
    const SrfBox bx = srf_box(boxes, c0 + cs);
    if (bx.active && z >= bx.z0 && z <= bx.z1 && y >= bx.y0 && y <= bx.y1) need |= 1u << cs;
  }
  if (!need) return;   // the same in every thread
  const uint8_t* __restrict__ s = (src ? sb : sa) + (int64_t)row * d2;
  int cls[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int x = q * 256 + tid;
    cls[q] = x < d2 ? s[x] : SRF_NONE;
  }
  for (int cs = 0; cs < nc; ++cs) {
    if (!(need >> cs & 1)) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q * 256 >= d2) break;
      const unsigned long long word = __ballot(cls[q] == c0 + cs);
      if (lane == 0) bits[cs][q * 4 + wave] = word;
    }
  }
  __syncthreads();
  const int nseg = (d2 + 63) >> 6;
  const int64_t nvox = (int64_t)d0 * d1 * d2;
  for (int cs = 0; cs < nc; ++cs) {
    if (!(need >> cs & 1)) continue;
    const SrfBox bx = srf_box(boxes, c0 + cs);
    uint16_t* __restrict__ out = g1 + (int64_t)(cs * 2 + src) * nvox + (int64_t)row * d2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = q * 256 + tid;
      if (x < bx.x0 || x > bx.x1 || x >= d2) continue;
      const int w0 = x >> 6, bit = x & 63;
      int best = 0xFFFF;
      unsigned long long m = bits[cs][w0] & (~0ull >> (63 - bit));   // x and what lies to its left
      int k = w0;
      while (m == 0 && k > 0) m = bits[cs][--k];
      if (m) best = x - (k * 64 + 63 - __builtin_clzll(m));
      m = bits[cs][w0] & (~0ull << bit);                             // x and what lies to its right
      k = w0;
      while (m == 0 && k < nseg - 1) m = bits[cs][++k];
      if (m) best = min(best, k * 64 + __builtin_ctzll(m) - x);
      out[x] = (uint16_t)best;
    }
  }
}

// min_j line[j] + (i - j)^2 over j in [0, len) for the line of column tx among TX staged abreast (lds[j * TX + tx]), searched
// outwards from i and stopped at (i - j)^2 >= best: every term left out is at least (i - j)^2, the values being non-negative,
// so the result is that of the minimum over the whole line.  Lanes of a wave that share i read consecutive words.
__device__ __forceinline__ int srf_line_min(const int* __restrict__ lds, int TX, int tx, int len, int i) {
  int best = lds[i * TX + tx];
  const int rmax = max(i, len - 1 - i);
  for (int r = 1; r <= rmax; ++r) {
    const int rr = r * r;
    if (rr >= best) break;
    if (i - r >= 0) best = min(best, lds[(i - r) * TX + tx] + rr);
    if (i + r < len) best = min(best, lds[(i + r) * TX + tx] + rr);
  }
  return best;
}

// Pass 2.  Grid (tiles of TX columns x, z, slab); dynamic LDS: (y1 - y0 + 1) * TX ints.
__global__ __launch_bounds__(256) void seg_surface_edt_y_kernel(const uint16_t* __restrict__ g1, int d0, int d1, int d2,
                                                                const int* __restrict__ boxes, int c0, int TX,
                                                                int32_t* __restrict__ g2) {
  extern __shared__ int lds[];
  const int sl = blockIdx.z, z = blockIdx.y, xb = blockIdx.x * TX, tid = threadIdx.x;
  const SrfBox bx = srf_box(boxes, c0 + (sl >> 1));
  if (!bx.active || z < bx.z0 || z > bx.z1 || xb > bx.x1 || xb + TX - 1 < bx.x0) return;
  const int sh = __builtin_ctz(TX), len = bx.y1 - bx.y0 + 1;
  const int64_t base = (int64_t)sl * d0 * d1 * d2 + ((int64_t)z * d1 + bx.y0) * d2;
  for (int idx = tid; idx < len * TX; idx += 256) {
    const int j = idx >> sh, x = xb + (idx & (TX - 1));
    int val = SRF_FAR;
    if (x >= bx.x0 && x <= bx.x1 && x < d2) {
      const int g = g1[base + (int64_t)j * d2 + x];
      if (g != 0xFFFF) val = g * g;
    }
    lds[idx] = val;
  }
  __syncthreads();
  const int tx = tid & (TX - 1), x = xb + tx;
  if (x < bx.x0 || x > bx.x1 || x >= d2) return;
  for (int i = tid >> sh; i < len; i += 256 >> sh)
    g2[base + (int64_t)i * d2 + x] = min(srf_line_min(lds, TX, tx, len, i), SRF_FAR);
}

// Pass 3.  Grid (tiles of TX columns x, y, slab); dynamic LDS: (z1 - z0 + 1) * TX ints.  The slab's source map is `sl & 1`; the
// queries are the surface voxels of the class in the other map, and a tile without one stages nothing.
__global__ __launch_bounds__(256) void seg_surface_edt_z_kernel(const int32_t* __restrict__ g2, const uint8_t* __restrict__ sa,
                                                                const uint8_t* __restrict__ sb, int d0, int d1, int d2,
                                                                const int* __restrict__ boxes, int c0, int TX,
                                                                int32_t* __restrict__ d2_ab, int32_t* __restrict__ d2_ba) {
  extern __shared__ int lds[];
  const int sl = blockIdx.z, y = blockIdx.y, xb = blockIdx.x * TX, tid = threadIdx.x, c = c0 + (sl >> 1);
  const SrfBox bx = srf_box(boxes, c);
  if (!bx.active || y < bx.y0 || y > bx.y1 || xb > bx.x1 || xb + TX - 1 < bx.x0) return;
  const uint8_t* __restrict__ query = (sl & 1) ? sa : sb;
  int32_t* __restrict__ out = (sl & 1) ? d2_ab : d2_ba;
  const int sh = __builtin_ctz(TX), len = bx.z1 - bx.z0 + 1, tx = tid & (TX - 1), x = xb + tx;
  const int64_t plane = (int64_t)d1 * d2;
  const int64_t col = (int64_t)bx.z0 * plane + (int64_t)y * d2;   // voxel (z0, y, 0)
  const bool inx = x >= bx.x0 && x <= bx.x1 && x < d2;
  int any = 0;
  if (inx)
    for (int i = tid >> sh; i < len; i += 256 >> sh) any |= query[col + i * plane + x] == c ? 1 : 0;
  if (!__syncthreads_or(any)) return;
  const int64_t base = (int64_t)sl * d0 * plane + col;
  for (int idx = tid; idx < len * TX; idx += 256) {
    const int j = idx >> sh, xx = xb + (idx & (TX - 1));
    lds[idx] = (xx >= bx.x0 && xx <= bx.x1 && xx < d2) ? g2[base + j * plane + xx] : SRF_FAR;
  }
  __syncthreads();
  if (!inx) return;
  for (int i = tid >> sh; i < len; i += 256 >> sh) {
    if (query[col + i * plane + x] != c) continue;
    const int best = srf_line_min(lds, TX, tx, len, i);
    out[col + i * plane + x] = best >= SRF_FAR ? INT32_MAX : best;
  }
}

}  // namespace

extern "C" {

int64_t synthsr_seg_surface_workspace_bytes(const int* shape, int N) {
  if (!srf_shape_ok(shape, N)) return SYNTHSR_EINVAL;
  return SrfLayout(shape, N).total;
}

int synthsr_seg_surface_dist2(const int32_t* a, const int32_t* b, const int* shape, const int32_t* lut, int lut_n, int N,
                              int32_t* d2_ab, int32_t* d2_ba, void* workspace, int64_t workspace_bytes,
                              synthsr_stream_t stream) {
  if (!a || !b || !lut || !d2_ab || !d2_ba || !workspace || lut_n < 1 || !srf_shape_ok(shape, N) ||
      ((uintptr_t)workspace % 16) != 0)
    return SYNTHSR_EINVAL;
  const SrfLayout L(shape, N);
  if (workspace_bytes < L.total) return SYNTHSR_EINVAL;
  const int d0 = shape[0], d1 = shape[1], d2 = shape[2];
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* boxes = (int*)ws;
  uint8_t *sa = (uint8_t*)(ws + L.sa), *sb = (uint8_t*)(ws + L.sb);
  int32_t* g2 = (int32_t*)(ws + L.g2);
  uint16_t* g1 = (uint16_t*)(ws + L.g1);
  hipLaunchKernelGGL(seg_surface_box_init_kernel, dim3(1), dim3(256), 0, st, boxes);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_surface_kernel, dim3(syn_grid(L.nvox, 256)), dim3(256), 0, st, a, b, d0, d1, d2, lut, lut_n, N, sa, sb,
                     d2_ab, d2_ba, boxes);
  SYN_CHECK_LAUNCH();
  const int ty = srf_tx(d1), tz = srf_tx(d0);
  for (int c0 = 0; c0 < N; c0 += L.ch) {
    const int nc = N - c0 < L.ch ? N - c0 : L.ch;
    hipLaunchKernelGGL(seg_surface_scan_x_kernel, dim3(d0 * d1, 2), dim3(256), 0, st, sa, sb, d0, d1, d2, boxes, c0, nc, g1);
    SYN_CHECK_LAUNCH();
    hipLaunchKernelGGL(seg_surface_edt_y_kernel, dim3((d2 + ty - 1) / ty, d0, 2 * nc), dim3(256), (size_t)d1 * ty * 4, st, g1, d0,
                       d1, d2, boxes, c0, ty, g2);
    SYN_CHECK_LAUNCH();
    hipLaunchKernelGGL(seg_surface_edt_z_kernel, dim3((d2 + tz - 1) / tz, d1, 2 * nc), dim3(256), (size_t)d0 * tz * 4, st, g2, sa,
                       sb, d0, d1, d2, boxes, c0, tz, d2_ab, d2_ba);
    SYN_CHECK_LAUNCH();
  }
  return SYNTHSR_OK;
}

}  // extern "C"
