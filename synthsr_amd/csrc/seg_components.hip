// Connected components of a label map and the largest component per group (include/synthsr_hip.h: synthsr_seg_components,
// synthsr_seg_keep_largest).  Integers only; comp[v] is the smallest linear index of v's component, which is unique, so no
// result depends on the order in which workgroups run.  No workgroup waits on another and no launch depends on the map.
//
// synthsr_seg_components, three launches, union-find with parent[v] <= v kept in `comp` itself (seg_components_uf.h):
//   seg_cc_tile_kernel     one workgroup per tile of 8 x 8 x 32 voxels: the group of every voxel by the lookup table, unions with
//                          the preceding neighbours inside the tile on tile-local indices in LDS, then comp[v] = the linear
//                          index of v's tile root (-1: in no group) and the group as one byte per voxel
//   seg_cc_border_kernel   unions across tile faces, edges and corners in global memory.  Every read of comp in this launch is a
//                          device-scope atomic load or the value an atomicMin returned: a plain load could be served from the
//                          vector L1 of a CU that another CU's atomic never reaches.
//   seg_cc_flatten_kernel  comp[v] = root of v, in place.  Plain loads: whatever value of comp[u] a thread meets, the parent left
//                          by the border launch or the root another thread has just stored, is an ancestor of u in the same tree.
// synthsr_seg_keep_largest, four launches:
//   seg_cc_clear_kernel    sizes[r] = 0 at every root r; the per-group records = 0
//   seg_cc_count_kernel    sizes[r] = voxels of the component, counted per run of equal roots within a wave, summed per
//                          workgroup (4096 consecutive voxels) in an LDS hash table and flushed with one atomicAdd per distinct
//                          root; per group the voxels and the roots
//   seg_cc_pick_kernel     per group one 64-bit atomicMax on (size << 32 | ~root): the largest size, then the smallest root
//   seg_cc_filter_kernel   out[v] = fill_value where v's root is not the one kept for its group, labels[v] elsewhere; stats
#include "common.h"
#include "seg_components_uf.h"

namespace {

constexpr int CC_MAXG = 64, CC_MAXSIDE = 1024;
constexpr int CC_TZ = 8, CC_TY = 8, CC_TX = 32, CC_TILE = CC_TZ * CC_TY * CC_TX;   // x: 5 bits, y: 3 bits, z: 3 bits
constexpr int CC_NONE = 255;                 // "in no group" in the byte map
constexpr int CC_REC = 4;                    // int64 per group in the workspace: (size << 32 | ~root), roots, voxels, unused
constexpr int64_t CC_HDR_BYTES = CC_MAXG * CC_REC * 8;
constexpr int CC_CHUNK = 4096, CC_SLOTS = 512, CC_PROBES = 8;
static_assert(CC_TILE == 8 * 256 && CC_CHUNK % 256 == 0 && (CC_SLOTS & (CC_SLOTS - 1)) == 0, "launch shapes");

bool cc_shape_ok(const int* shape) {
  if (!shape) return false;
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1 || shape[i] > CC_MAXSIDE) return false;
  return true;
}

// workspace: the per-group records, then 4 bytes per voxel (keep_largest: int32 sizes; components: the byte map in its front)
int64_t cc_workspace_bytes(const int* shape) {
  const int64_t nvox = (int64_t)shape[0] * shape[1] * shape[2];
  return CC_HDR_BYTES + (nvox * 4 + 15) / 16 * 16;
}

struct CcLds {   // LDS: one workgroup
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
struct CcGlobal {   // global memory shared by all workgroups of the launch
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// Grid (tiles along x, y, z); thread t holds the voxels (lz, t >> 5, t & 31), lz = 0 .. 7, local index lz * 256 + t.  Local and
// linear order agree inside a tile, so the smallest local index of a component is its smallest linear index in the tile.
template <int CONN>
__global__ __launch_bounds__(256) void seg_cc_tile_kernel(const int32_t* __restrict__ labels, int d0, int d1, int d2,
                                                          const int32_t* __restrict__ lut, int lut_n, int G,
                                                          int32_t* __restrict__ comp, uint8_t* __restrict__ grp) {
  __shared__ int par[CC_TILE];
  __shared__ uint8_t sg[CC_TILE];
  const int tid = threadIdx.x, lx = tid & (CC_TX - 1), ly = tid >> 5;
  const int x0 = blockIdx.x * CC_TX, y0 = blockIdx.y * CC_TY, z0 = blockIdx.z * CC_TZ;
  const int x = x0 + lx, y = y0 + ly;
  const bool in_xy = x < d2 && y < d1;
#pragma unroll
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int l = lz * 256 + tid, z = z0 + lz;
    int g = -1;
    if (in_xy && z < d0) g = shd_class(labels[(z * d1 + y) * d2 + x], lut, lut_n, G);
    sg[l] = (uint8_t)(g < 0 ? CC_NONE : g);   // voxels of the tile beyond the volume are in no group
    par[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int l = lz * 256 + tid, g = sg[l];
    if (g == CC_NONE) continue;
#pragma unroll
    for (int k = 0; k < CCU_PRECEDING; ++k) {
      int dz, dy, dx;
      ccu_step(k, dz, dy, dx);
      if (!ccu_adjacent(CONN, dz, dy, dx)) continue;
      const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
      if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;   // the border launch joins these
      const int nl = l + dz * 256 + dy * CC_TX + dx;
      if (sg[nl] == g) ccu_union<CcLds>(par, l, nl);
    }
  }
  __syncthreads();
#pragma unroll
  for (int lz = 0; lz < CC_TZ; ++lz) {
    const int l = lz * 256 + tid, z = z0 + lz;
    if (!in_xy || z >= d0) continue;
    const int v = (z * d1 + y) * d2 + x, g = sg[l];
    int c = -1;
    if (g != CC_NONE) {
      const int r = ccu_find<CcLds>(par, l);
      c = ((z0 + (r >> 8)) * d1 + y0 + ((r >> 5) & (CC_TY - 1))) * d2 + x0 + (r & (CC_TX - 1));
    }
    comp[v] = c;
    grp[v] = (uint8_t)g;
  }
}

// Grid (64-voxel segments along x, 4 rows y, z).  A voxel joins every preceding neighbour of its group that lies in another
// tile; the pairs inside a tile are joined already.
template <int CONN>
__global__ __launch_bounds__(256) void seg_cc_border_kernel(const uint8_t* __restrict__ grp, int d0, int d1, int d2, int32_t* comp) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (x >= d2 || y >= d1) return;
  const int v = (z * d1 + y) * d2 + x, g = grp[v];
  if (g == CC_NONE) return;
#pragma unroll
  for (int k = 0; k < CCU_PRECEDING; ++k) {
    int dz, dy, dx;
    ccu_step(k, dz, dy, dx);
    if (!ccu_adjacent(CONN, dz, dy, dx)) continue;
    const int nz = z + dz, ny = y + dy, nx = x + dx;
    if (nz < 0 || ny < 0 || ny >= d1 || nx < 0 || nx >= d2) continue;
    if ((nz >> 3) == (z >> 3) && (ny >> 3) == (y >> 3) && (nx >> 5) == (x >> 5)) continue;
    const int n = (nz * d1 + ny) * d2 + nx;
    if (grp[n] == g) ccu_union<CcGlobal>(comp, v, n);
  }
}

__global__ __launch_bounds__(256) void seg_cc_flatten_kernel(int32_t* comp, int nvox) {
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    int x = comp[v];
    if (x < 0) continue;
    // terminates: comp[x] <= x for every voxel in a group, before and after any store of this launch, so x strictly decreases
    for (int p = comp[x]; p != x; p = comp[x]) x = p;
    comp[v] = x;
  }
}

// a component index a caller hands in is used as an address only when it is one
__device__ __forceinline__ bool cc_is_voxel(int c, int nvox) { return (unsigned)c < (unsigned)nvox; }

__global__ __launch_bounds__(256) void seg_cc_clear_kernel(const int32_t* __restrict__ comp, int nvox, int32_t* __restrict__ sizes,
                                                           unsigned long long* __restrict__ rec) {
  if (blockIdx.x == 0) rec[threadIdx.x] = 0;   // CC_MAXG * CC_REC = 256 words
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256)
    if (comp[v] == v) sizes[v] = 0;
}

// Grid: chunks of CC_CHUNK consecutive voxels.  Equal roots that follow one another in a wave are one run; its first lane adds
// the run's length to the root's slot of the hash table (open addressing; a root that finds no slot in CC_PROBES steps goes to
// global memory directly).  A root is always the first voxel of a run: comp[v - 1] <= v - 1.
__global__ __launch_bounds__(256) void seg_cc_count_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                           int nvox, const int32_t* __restrict__ lut, int lut_n, int G,
                                                           int32_t* __restrict__ sizes, unsigned long long* __restrict__ rec) {
  __shared__ int hkey[CC_SLOTS], hcnt[CC_SLOTS], gvox[CC_MAXG], groots[CC_MAXG];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < CC_SLOTS; e += 256) hkey[e] = -1, hcnt[e] = 0;
  if (tid < CC_MAXG) gvox[tid] = 0, groots[tid] = 0;
  __syncthreads();
  const int base = blockIdx.x * CC_CHUNK;   // < nvox <= 2^30
  for (int it = 0; it < CC_CHUNK / 256; ++it) {
    const int v = base + it * 256 + tid;    // every lane of a wave runs every round: the shuffle and the ballot are wave-wide
    int r = -1, g = -1;
    if (v < nvox) {
      r = comp[v];
      if (cc_is_voxel(r, nvox)) g = shd_class(labels[v], lut, lut_n, G);
      if (g < 0) r = -1;
    }
    const int before = __shfl_up(r, 1);
    const bool head = lane == 0 || before != r;
    const unsigned long long heads = __ballot(head);
    if (head && r >= 0) {
      const unsigned long long later = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
      const int len = (later ? __builtin_ctzll(later) : 64) - lane;
      atomicAdd(&gvox[g], len);
      if (r == v) atomicAdd(&groots[g], 1);
      int slot = (r * 0x9E3779B1u) >> 23;   // the top 9 bits
      bool placed = false;
      for (int t = 0; t < CC_PROBES && !placed; ++t) {   // terminates: at most CC_PROBES rounds
        const int was = atomicCAS(&hkey[slot], -1, r);
        if (was == -1 || was == r) {
          atomicAdd(&hcnt[slot], len);
          placed = true;
        }
        slot = (slot + 1) & (CC_SLOTS - 1);
      }
      if (!placed) atomicAdd(&sizes[r], len);
    }
  }
  __syncthreads();
  for (int e = tid; e < CC_SLOTS; e += 256)
    if (hkey[e] >= 0) atomicAdd(&sizes[hkey[e]], hcnt[e]);
  if (tid < G) {
    if (groots[tid]) atomicAdd(&rec[tid * CC_REC + 1], (unsigned long long)groots[tid]);
    if (gvox[tid]) atomicAdd(&rec[tid * CC_REC + 2], (unsigned long long)gvox[tid]);
  }
}
static_assert(CC_SLOTS == 1 << 9, "the hash keeps 9 bits");

__global__ __launch_bounds__(256) void seg_cc_pick_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                          int nvox, const int32_t* __restrict__ lut, int lut_n, int G,
                                                          const int32_t* __restrict__ sizes, unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long best[CC_MAXG];
  if (threadIdx.x < CC_MAXG) best[threadIdx.x] = 0;
  __syncthreads();
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    if (comp[v] != v) continue;
    const int g = shd_class(labels[v], lut, lut_n, G);
    if (g < 0) continue;
    // size first, then the smaller root: of two keys of equal size the one with the larger ~root wins
    atomicMax(&best[g], ((unsigned long long)(unsigned)sizes[v] << 32) | (0xFFFFFFFFu - (unsigned)v));
  }
  __syncthreads();
  if (threadIdx.x < G) {
    // one flush per workgroup; the record only grows, so a possibly stale read filters what cannot raise it
    const unsigned long long key = best[threadIdx.x];
    unsigned long long* p = rec + threadIdx.x * CC_REC;
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, key);
  }
}

// `out` may be `labels`: a thread reads labels[v] before it writes out[v] and touches no other voxel
__global__ __launch_bounds__(256) void seg_cc_filter_kernel(const int32_t* labels, const int32_t* __restrict__ comp, int nvox,
                                                            const int32_t* __restrict__ lut, int lut_n, int G, int32_t fill_value,
                                                            const unsigned long long* __restrict__ rec, int32_t* out,
                                                            int64_t* __restrict__ stats) {
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    const int lab = labels[v], c = comp[v];
    int val = lab;
    if (c >= 0) {
      const int g = shd_class(lab, lut, lut_n, G);
      if (g >= 0 && (unsigned)c != 0xFFFFFFFFu - (unsigned)rec[g * CC_REC]) val = fill_value;
    }
    out[v] = val;
  }
  if (blockIdx.x == 0 && threadIdx.x < G) {
    const int g = threadIdx.x;
    const unsigned long long key = rec[g * CC_REC];   // 0: the group is empty (a component has at least one voxel)
    stats[g * 4 + 0] = key ? (int64_t)(0xFFFFFFFFu - (unsigned)key) : -1;
    stats[g * 4 + 1] = (int64_t)(key >> 32);
    stats[g * 4 + 2] = (int64_t)rec[g * CC_REC + 1];
    stats[g * 4 + 3] = (int64_t)rec[g * CC_REC + 2];
  }
}

template <int CONN>
int cc_label(const int32_t* labels, int d0, int d1, int d2, const int32_t* lut, int lut_n, int G, int32_t* comp, uint8_t* grp,
             hipStream_t st) {
  hipLaunchKernelGGL(seg_cc_tile_kernel<CONN>, dim3((d2 + CC_TX - 1) / CC_TX, (d1 + CC_TY - 1) / CC_TY, (d0 + CC_TZ - 1) / CC_TZ),
                     dim3(256), 0, st, labels, d0, d1, d2, lut, lut_n, G, comp, grp);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_cc_border_kernel<CONN>, dim3((d2 + 63) / 64, (d1 + 3) / 4, d0), dim3(256), 0, st, grp, d0, d1, d2, comp);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_cc_flatten_kernel, dim3(syn_grid((int64_t)d0 * d1 * d2, 256)), dim3(256), 0, st, comp, d0 * d1 * d2);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

}  // namespace

extern "C" {

int64_t synthsr_seg_components_workspace_bytes(const int* shape) {
  if (!cc_shape_ok(shape)) return SYNTHSR_EINVAL;
  return cc_workspace_bytes(shape);
}

int synthsr_seg_components(const int32_t* labels, const int* shape, const int32_t* lut, int lut_n, int G, int connectivity,
                           int32_t* comp, void* workspace, int64_t workspace_bytes, synthsr_stream_t stream) {
  if (!labels || !lut || !comp || !workspace || lut_n < 1 || G < 1 || G > CC_MAXG || !cc_shape_ok(shape) ||
      (connectivity != 6 && connectivity != 18 && connectivity != 26) || ((uintptr_t)workspace % 16) != 0 ||
      workspace_bytes < cc_workspace_bytes(shape))
    return SYNTHSR_EINVAL;
  uint8_t* grp = (uint8_t*)workspace + CC_HDR_BYTES;
  hipStream_t st = (hipStream_t)stream;
  if (connectivity == 6) return cc_label<6>(labels, shape[0], shape[1], shape[2], lut, lut_n, G, comp, grp, st);
  if (connectivity == 18) return cc_label<18>(labels, shape[0], shape[1], shape[2], lut, lut_n, G, comp, grp, st);
  return cc_label<26>(labels, shape[0], shape[1], shape[2], lut, lut_n, G, comp, grp, st);
}

int synthsr_seg_keep_largest(const int32_t* labels, const int32_t* comp, const int* shape, const int32_t* lut, int lut_n, int G,
                             int32_t fill_value, int32_t* out, int64_t* stats, void* workspace, int64_t workspace_bytes,
                             synthsr_stream_t stream) {
  if (!labels || !comp || !lut || !out || !stats || !workspace || lut_n < 1 || G < 1 || G > CC_MAXG || !cc_shape_ok(shape) ||
      ((uintptr_t)workspace % 16) != 0 || workspace_bytes < cc_workspace_bytes(shape))
    return SYNTHSR_EINVAL;
  const int nvox = shape[0] * shape[1] * shape[2];   // <= 2^30
  unsigned long long* rec = (unsigned long long*)workspace;
  int32_t* sizes = (int32_t*)((char*)workspace + CC_HDR_BYTES);
  hipStream_t st = (hipStream_t)stream;
  const int grid = syn_grid(nvox, 256);
  hipLaunchKernelGGL(seg_cc_clear_kernel, dim3(grid), dim3(256), 0, st, comp, nvox, sizes, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_cc_count_kernel, dim3((nvox + CC_CHUNK - 1) / CC_CHUNK), dim3(256), 0, st, labels, comp, nvox, lut, lut_n,
                     G, sizes, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_cc_pick_kernel, dim3(grid), dim3(256), 0, st, labels, comp, nvox, lut, lut_n, G, sizes, rec);
  SYN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_cc_filter_kernel, dim3(grid), dim3(256), 0, st, labels, comp, nvox, lut, lut_n, G, fill_value, rec, out,
                     stats);
  SYN_CHECK_LAUNCH();
  return SYNTHSR_OK;
}

}  // extern "C"
