// shared helpers for the gfx950 kernels of libsynthsr_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/synthsr_hip.h"

#define SYN_CHECK_LAUNCH()                                 \
  do {                                                     \
    hipError_t e__ = hipGetLastError();                    \
    if (e__ != hipSuccess) return SYNTHSR_ELAUNCH;         \
  } while (0)

static inline int64_t syn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// grid for a grid-stride elementwise kernel: enough workgroups to fill 256 CUs several times over
static inline int syn_grid(int64_t n, int block, int max_blocks = 256 * 16) {
  int64_t g = syn_cdiv(n, block);
  if (g > max_blocks) g = max_blocks;
  if (g < 1) g = 1;
  return (int)g;
}

#ifdef __HIPCC__
// Contiguous element range [lo, hi) of this workgroup for a 1-D sweep over n elements, laid out XCD-contiguously:
// consecutive workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2), so XCD k gets ids k, k+8, ...;
// mapping id -> position (id & 7) * G/8 + id/8 gives every XCD ONE contiguous eighth of the volume instead of a comb
// over all of it (a gather / stencil sweep otherwise pulls the whole input through all 8 L2s: measured 7.3x the label
// volume in FETCH_SIZE for deform_gmm_kernel).  Chunks are multiples of 256 elements (block size): coalescing unchanged.
__device__ static inline void syn_block_range(int64_t n, int64_t& lo, int64_t& hi) {
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int pos = (G % 8 == 0) ? (b & 7) * (G >> 3) + (b >> 3) : b;
  const int64_t chunk = (((n + G - 1) / G) + 255) / 256 * 256;
  lo = (int64_t)pos * chunk;
  hi = lo + chunk < n ? lo + chunk : n;
}

// ---- deterministic mode (synthsr_set_deterministic, include/synthsr_hip_tuning.h) ------------------------------------------
// Every cross-workgroup float accumulation in the library is "reduce inside the workgroup in a fixed order, then ONE flush of
// atomicAdd per workgroup onto the shared target": the only run-to-run freedom is the order in which the flushes land.
// Deterministic mode removes it in one of two ways.
//  * syn_det_gather (small partials: channel sums, losses): every workgroup parks its partial row in scratch; the workgroup
//    that arrives LAST adds the rows up in workgroup-id order and alone performs the flush.  No serialisation.
//  * syn_turn_begin / syn_turn_end (large partials: weight gradients): the workgroups that share target addresses form a chain
//    and flush one after the other in chain position order -- a workgroup waits until the chain's ticket equals its position,
//    flushes, fences, passes the ticket on (the last one resets it for the next launch).  Workgroups are dispatched in id
//    order (per XCD as well) and every predecessor in a chain has a lower id, so the lowest unfinished id is always resident:
//    no deadlock; the wait is bounded anyway (`timeout` is raised when it gives up).
// One state block for the whole library: deterministic mode is for single-stream use.  g_syn_det == nullptr (the default)
// costs one scalar load per workgroup.
constexpr int SYN_DET_CHAINS = 8192;
struct SynDet {
  int arrivals;           // syn_det_gather: workgroups that parked their row
  int timeout;            // raised when an ordered wait gave up (results may then be unordered)
  long long scratch_floats;
  float* scratch;
  int chain[SYN_DET_CHAINS];  // tickets
};
static __device__ SynDet* g_syn_det = nullptr;  // one copy per translation unit, set through SYN_DET_SETTER(name)

__device__ __forceinline__ int syn_wg_linear() { return blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); }
__device__ __forceinline__ int syn_wg_count() { return gridDim.x * gridDim.y * gridDim.z; }
__device__ __forceinline__ bool syn_tid0() { return threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0; }
__device__ __forceinline__ bool syn_det_on() { return g_syn_det != nullptr; }

// Ordered flush: chain = id of the group of workgroups that share target addresses, pos / len = this workgroup's place in it.
// Call from workgroup-uniform control flow, by EVERY workgroup of the grid exactly once.
__device__ __forceinline__ int* syn_turn_begin(int chain, int pos) {
  SynDet* d = g_syn_det;
  if (!d) return nullptr;
  int* tk = &d->chain[chain % SYN_DET_CHAINS];
  if (syn_tid0()) {
    int spins = 0;
    while (__hip_atomic_load(tk, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != pos) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 24)) {  // ~1 s: report and go on unordered rather than hang the device
        d->timeout = 1;
        break;
      }
    }
  }
  __syncthreads();
  return tk;
}

__device__ __forceinline__ void syn_turn_end(int* tk, int pos, int len) {
  if (tk) {
    __threadfence();  // this workgroup's atomics are performed before the next workgroup starts its own
    __syncthreads();
    if (syn_tid0()) __hip_atomic_store(tk, pos + 1 == len ? 0 : pos + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the weight-gradient kernels: grid (voxel split, slice [, slice]) -- workgroups with equal (y, z) accumulate the same slice
__device__ __forceinline__ int* syn_turn_begin_x() { return syn_turn_begin(blockIdx.y + gridDim.y * blockIdx.z, blockIdx.x); }
__device__ __forceinline__ void syn_turn_end_x(int* tk) { syn_turn_end(tk, blockIdx.x, gridDim.x); }

// Small partials: part[0..n) is this workgroup's partial (LDS, complete and synchronised).  Default mode: returns true for
// every workgroup (all of them flush with atomics).  Deterministic mode: returns true only in the workgroup that arrived last,
// with part[] replaced by the sum over ALL workgroups in id order (double accumulation, one rounding).  Workgroup-uniform.
__device__ __forceinline__ bool syn_det_gather(float* part, int n) {
  SynDet* d = g_syn_det;
  if (!d) return true;
  const int wg = syn_wg_linear(), nwg = syn_wg_count();
  const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z), nt = blockDim.x * blockDim.y * blockDim.z;
  __shared__ int s_last;
  if ((long long)nwg * n > d->scratch_floats) {  // does not fit: one chain over the whole grid instead
    (void)syn_turn_begin(SYN_DET_CHAINS - 1, wg);
    return true;  // the caller flushes with atomics; syn_det_gather_end passes the ticket on
  }
  float* row = d->scratch + (size_t)wg * n;
  for (int i = tid; i < n; i += nt) row[i] = part[i];
  __threadfence();
  __syncthreads();
  if (syn_tid0()) s_last = (atomicAdd(&d->arrivals, 1) == nwg - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  // the last workgroup adds the rows up.  One thread per column walking all nwg rows is a chain of ~1000 dependent
  // load + add steps with most of the workgroup idle (0.3-0.5 ms per reduction launch, 10 ms per 160^3 step); instead
  // P = nt / n threads share a column, thread p takes rows p, p + P, ... and the P partial sums are added in p order:
  // the grouping depends on the launch geometry only, so the result is still the same run after run.
  __shared__ double s_col[1024];
  const int P = (n <= nt) ? min(nt / n, 1024 / n) : 0;
  if (P >= 2) {
    if (tid < n * P) {
      const int col = tid % n, p = tid / n;
      // four independent accumulators (rows p, p + P, p + 2P, p + 3P of every group of 4 P): the loads of a group are in
      // flight together instead of one row's latency after the other; combined in a fixed order
      double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
      const float* base = d->scratch + col;
      int w = p;
      for (; w + 3 * P < nwg; w += 4 * P) {
        const float a0 = __builtin_nontemporal_load(base + (size_t)w * n);
        const float a1 = __builtin_nontemporal_load(base + (size_t)(w + P) * n);
        const float a2 = __builtin_nontemporal_load(base + (size_t)(w + 2 * P) * n);
        const float a3 = __builtin_nontemporal_load(base + (size_t)(w + 3 * P) * n);
        t0 += (double)a0;
        t1 += (double)a1;
        t2 += (double)a2;
        t3 += (double)a3;
      }
      for (; w < nwg; w += P) t0 += (double)__builtin_nontemporal_load(base + (size_t)w * n);
      s_col[tid] = (t0 + t1) + (t2 + t3);
    }
    __syncthreads();
    if (tid < n) {
      double t = 0.0;
      for (int p = 0; p < P; ++p) t += s_col[p * n + tid];
      part[tid] = (float)t;
    }
  } else {
    for (int i = tid; i < n; i += nt) {
      double t = 0.0;
      for (int w = 0; w < nwg; ++w) t += (double)__builtin_nontemporal_load(d->scratch + (size_t)w * n + i);
      part[i] = (float)t;
    }
  }
  if (syn_tid0()) d->arrivals = 0;
  __syncthreads();
  return true;
}

// after the flush that follows a `true` from syn_det_gather (no-op unless the oversize fallback took a ticket)
__device__ __forceinline__ void syn_det_gather_end(int n) {
  SynDet* d = g_syn_det;
  if (d && (long long)syn_wg_count() * n > d->scratch_floats)
    syn_turn_end(&d->chain[SYN_DET_CHAINS - 1], syn_wg_linear(), syn_wg_count());
}

// A kernel attribute (hipFuncSetAttribute: the dynamic LDS size) is set once per kernel AND DEVICE (max_dyn_smem below keeps one of
// these per kernel): the guard returned by first() marks the device when the if statement that holds it ENDS.
// The device's bit is set only AFTER the attribute call returned: a second thread that launches on the same device meanwhile
// sets the (idempotent, cheap) attribute again instead of launching without it.  Device ids beyond 63 never cache.
#include <atomic>
struct SynOncePerDevice {
  std::atomic<uint64_t> bits{0};
  bool needed() const {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;
    return !(bits.load(std::memory_order_acquire) & (1ull << dev));
  }
  void done() {
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev <= 63) bits.fetch_or(1ull << dev, std::memory_order_release);
  }
  struct Guard {
    SynOncePerDevice* o;
    bool need;
    ~Guard() { if (need) o->done(); }
    explicit operator bool() const { return need; }
  };
  Guard first() { return Guard{this, needed()}; }
};
// Raises the dynamic-LDS limit of Kern before its launch.  The kernel is a template VALUE: every instantiation, RELU or not, has
// its own flag.
template <auto Kern>
void max_dyn_smem(size_t bytes) {
  static SynOncePerDevice done;
  if (auto once_ = done.first()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  }
}
// launches Kern, or KernR (its RELU instantiation) when `relu`, with `smem` bytes of dynamic LDS
template <auto Kern, auto KernR, class... Args>
void launch_smem(bool relu, dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args) {
  if (relu) {
    max_dyn_smem<KernR>(smem);
    hipLaunchKernelGGL(KernR, grid, block, smem, st, args...);
  } else {
    max_dyn_smem<Kern>(smem);
    hipLaunchKernelGGL(Kern, grid, block, smem, st, args...);
  }
}

// host side of the deterministic WEIGHT-GRADIENT flush (conv3d.hip: det_prepare / det_finish): private planes per workgroup
// column + an ordered reduction; shared by the fp32 and the bf16 weight-gradient launchers
struct DetRun {
  float* planes = nullptr;
  float* dw = nullptr;
  float* dbias = nullptr;
  int64_t dw_elems = 0, stride = 0;
  int cout = 0, gx = 0;
};
extern "C" int syn_det_enabled();
extern "C" int syn_det_prepare(DetRun* d, float** dw, float** dbias, int64_t dw_elems, int cout, int gx, hipStream_t st);
extern "C" int syn_det_finish(const DetRun* d, hipStream_t st);

#define SYN_DET_SETTER(name)                                                                              \
  extern "C" __attribute__((visibility("hidden"))) int syn_det_set_##name(SynDet* p) {                   \
    return hipMemcpyToSymbol(HIP_SYMBOL(g_syn_det), &p, sizeof(p)) == hipSuccess ? 0 : 1;                 \
  }
#endif

// Nearest-upsample folding (conv3d.hip: weight_value; conv_bf16.hip: pack_bf16_value): a 3-tap axis of a conv applied to
// UpSampling(2)(x) acts, for output parity p, on x through a 2-tap window -- low-res slot s (offset s - 1) collects the
// original taps t[0 .. n): p = 0: slot 0 <- {0}, slot 1 <- {1, 2};  p = 1: slot 1 <- {0, 1}, slot 2 <- {2}.
__host__ __device__ static inline int syn_up_axis_taps(int p, int s, int t[2]) {
  if (p == 0) {
    if (s == 0) { t[0] = 0; return 1; }
    if (s == 1) { t[0] = 1; t[1] = 2; return 2; }
    return 0;
  }
  if (s == 1) { t[0] = 0; t[1] = 1; return 2; }
  if (s == 2) { t[0] = 2; return 1; }
  return 0;
}

// monotone uint32 encoding of float (total order incl. negatives) for atomicMin/atomicMax
__host__ __device__ static inline uint32_t syn_f2ord(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
__host__ __device__ static inline float syn_ord2f(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return c.f;
}

#ifdef __HIPCC__
// running [min, max] pair (ordered-uint encoding) shared by the whole grid.  Thousands of atomics on the same two words
// serialise at the memory-side atomic unit (8192 waves x 2: most of deform_gmm_kernel's 220 us); min / max only ever move
// one way, so a plain (possibly stale) read filters out every wave that cannot improve them -- a stale value is only ever
// LESS extreme than the current one, so nothing that matters is skipped and the result is exact.
__device__ __forceinline__ void syn_minmax_update(uint32_t* mm, float mn, float mx) {
  const uint32_t lo = syn_f2ord(mn), hi = syn_f2ord(mx);
  if (lo < __hip_atomic_load(&mm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&mm[0], lo);
  if (hi > __hip_atomic_load(&mm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&mm[1], hi);
}
#endif

#ifdef __HIPCC__
// head channel of a label value, or -1 (the softmax-head kernels of unet_pointwise.hip, seg_surface.hip)
__device__ __forceinline__ int shd_class(int lab, const int32_t* __restrict__ lut, int lut_n, int N) {
  const int k = (lab >= 0 && lab < lut_n) ? lut[lab] : -1;
  return (k >= 0 && k < N) ? k : -1;
}
#endif

#ifdef __HIPCC__
// two fp32 values -> their three bf16 pieces (packed pairs, low half = first value): a = a0 + a1 + a2 exactly, every piece
// rounded to nearest even from what the previous ones left (conv_split.hip; one v_cvt_pk_bf16_f32 + two subtractions each)
__device__ __forceinline__ uint32_t syn_pack_bf16x2(float lo, float hi) {
  typedef __bf16 syn_bf16x2 __attribute__((ext_vector_type(2)));
  const syn_bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ void syn_split3(float f0, float f1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = syn_pack_bf16x2(f0, f1);
  float r0 = f0 - __uint_as_float(p0 << 16), r1 = f1 - __uint_as_float(p0 & 0xffff0000u);
  p1 = syn_pack_bf16x2(r0, r1);
  r0 -= __uint_as_float(p1 << 16);
  r1 -= __uint_as_float(p1 & 0xffff0000u);
  p2 = syn_pack_bf16x2(r0, r1);
}
#endif

#ifdef __HIPCC__
// ---- shared by the conv kernels (conv3d.hip, conv_split.hip, conv_bf16.hip) ---------------------------------------------------
// compile-time loop: f(std::integral_constant<int, I>) for I in [I, N)
template <int I, int N, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor<I + 1, N>(f);
  }
}

// ELU(alpha = 1) for the fused fp32 epilogues.  Vector-ALU instructions next to MFMAs are not free on gfx950, so instead of
// libm's expm1f (~22 instructions) the negative branch is 2^(v log2 e) - 1 through v_exp_f32, switched to a degree-5 Taylor
// polynomial on (-1/8, 0] where the subtraction would cancel.  |error| < 2e-7 absolute and < 2e-6 relative to expm1
// (tests/test_unet_gpu.py::test_elu_epilogue_accuracy).  The bf16 kernels round the result and keep a shorter one (elu_bf16_f).
__device__ __forceinline__ float elu_f(float v) {
  const float e = __builtin_amdgcn_exp2f(v * 1.44269504088896341f) - 1.f;
  const float p = v * fmaf(v, fmaf(v, fmaf(v, fmaf(v, 1.f / 120.f, 1.f / 24.f), 1.f / 6.f), 0.5f), 1.f);
  const float n = v > -0.125f ? p : e;
  return v > 0.f ? v : n;
}
// derivative of ELU expressed through its output y: 1 for y > 0, y + 1 (= e^x) otherwise
__device__ __forceinline__ float elu_dy(float y) { return y > 0.f ? 1.f : y + 1.f; }
// ReLU (act 3 / 4, Keras activation='relu'): the fp32 kernels take the activation family as a template parameter RELU and run it
// under the ELU family's act codes 1 / 2, so the ELU instantiations stay the code they were
template <bool RELU>
__device__ __forceinline__ float act_f(float v) {
  if constexpr (RELU) return fmaxf(v, 0.f);
  else return elu_f(v);
}
// derivative through the output: ReLU'(y) = 1 for y > 0, else 0 (TF ReluGrad)
template <bool RELU>
__device__ __forceinline__ float act_dy(float y) {
  if constexpr (RELU) return y > 0.f ? 1.f : 0.f;
  else return elu_dy(y);
}

// ---- the 4x4x16-voxel tiles of the split and the bf16 kernels and their order ------------------------------------------------
// Tiles are enumerated (z-slab of SLAB_Z tile planes, y, z within the slab, x): neighbours in all three directions are close in
// the list.  The list is cut into 8 contiguous parts, one per XCD (consecutive workgroup ids are dealt round-robin to the XCDs,
// each with a private L2), and the workgroups of an XCD walk their part (tile_walk of either file): the ~64 tiles an XCD works on
// at any time form a compact block, so the halo voxels they share are fetched from HBM once (with the plain z-major order every
// tile pulled its 2.5x halo through on its own: FETCH ~2.5x the tensor).
constexpr int TZ = 4, TY = 4, TX = 16, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, HVOX = HZ * HY * HX;
constexpr int SLAB_Z = 4;
__device__ __forceinline__ void tile_decode(int p, int tiles0, int tiles1, int tiles2, int& z0, int& y0, int& x0) {
  const int t12 = tiles1 * tiles2;
  const int s = p / (SLAB_Z * t12), r = p - s * SLAB_Z * t12;
  const int sz = min(SLAB_Z, tiles0 - s * SLAB_Z);
  const int t1 = r / (sz * tiles2), rr = r - t1 * sz * tiles2;
  const int zz = rr / tiles2, t2 = rr - zz * tiles2;
  z0 = (s * SLAB_Z + zz) * TZ;
  y0 = t1 * TY;
  x0 = t2 * TX;
}
#endif
// Workgroups along x of a launch whose persistent workgroups walk `ntiles` tiles, given `slots` workgroup slots for them (what the
// CUs hold at once, divided by the grid's y and z): a multiple of 8 (one share per XCD), and never narrower than the tile count
// where that is possible -- 296 workgroups for 300 tiles made 8 stragglers walk two tiles = twice the kernel's critical path.
static inline int syn_tile_grid_x(int slots, int ntiles) {
  int gx = slots / 8 * 8;
  if (gx < 8) gx = 8;
  while (gx > 8 && gx - 8 >= ntiles) gx -= 8;
  if (ntiles < 8) gx = ntiles;
  return gx;
}

// Output-channel tiles (of 16) per co-chunk of a plain split conv (conv3d.hip plans and packs with it, conv_split.hip launches
// with it).  Up to three tiles per workgroup (registers), whole co-chunks.  Round 6: a layer whose units (4x4x16 voxel tiles x
// co-chunks of 48) fall between one and one and a half rounds of the 512 workgroup slots (40^3 with 96 output channels: 600)
// takes co-chunks of 32 instead -- 900 shorter units in two rounds cost 2 x 2/3 of a unit-time where 600 cost two full ones
// (4-wave kernel) or three half ones (8-wave kernel): -11 ... -18 % on the 40^3 layers, -0.36 ms per training step, same box
// (profiles/r06_plan_40cubed_ab.txt).
__host__ __device__ inline bool syn_split_replanned(int vox_tiles, int co_tiles, int mt) {
  if (mt != 2 || co_tiles <= 3 || (co_tiles % 3) != 0 || (co_tiles % 2) != 0) return false;
  const long long u3 = (long long)vox_tiles * (co_tiles / 3);
  return u3 > 512 && u3 < 768;
}
// (`replan`: plain convs and, since the A/B of profiles/r06_folded_dgrad_replan_ab.txt, the data gradient of a folded decoder conv --
// 40^3 96 <- 48: 0.326 -> 0.252 ms; not the folded forward pass, whose kernel takes one co-chunk)
__host__ __device__ inline int syn_split_plan_mt(int vox_tiles, int co_tiles, bool replan) {
  const int mt = co_tiles <= 3 ? co_tiles : ((co_tiles % 3) == 0 ? 3 : ((co_tiles % 2) == 0 ? 2 : 1));
  if (replan && mt == 3 && syn_split_replanned(vox_tiles, co_tiles, 2)) return 2;
  return mt;
}

// K order of the split forward kernel (conv_split.hip): K slot 4 * step + g (g = lane >> 4) -> tap 0..26, or -1 for the one
// spare slot (zero weights).  ds_read_b128 serves lanes {0-3, 12-15} of one 16-lane quarter together with lanes {4-11} of the
// NEXT quarter (MI355X_MICROARCH.md, LDS): with the even x-voxels on the first set and the odd ones on the second, the two taps
// of a slot pair (g, g ^ 1) hit disjoint banks exactly when their halo offsets differ by an even number of voxels, i.e. when
// their x taps have the same parity.  Pairs 0..8: taps (tz, ty, 0) and (tz, ty, 2); pairs 9..13: the x-centre taps two by two.
__host__ __device__ constexpr int syn_split_tap(int slot) {
  const int p = slot >> 1, h = slot & 1;
  if (p < 9) return p * 3 + 2 * h;
  const int i = 2 * (p - 9) + h;
  return i < 9 ? i * 3 + 1 : -1;
}
// K order of the folded (nearest-upsample) variants: K slot 4 * step + g of the 2 steps of a parity -> tap (a, b, c) in {0, 1}^3
// of the parity's 2x2x2 window as 4 a + 2 b + c; the two slots of a pair differ in b (one halo row apart: an even number of
// voxels, see syn_split_tap)
__host__ __device__ constexpr int syn_split_tap8(int slot) {
  const int p = slot >> 1, h = slot & 1;
  return 4 * (p & 1) + 2 * h + (p >> 1);
}
// x-voxel of lane m (= lane & 15) of a 16-voxel row under that scheme
__host__ __device__ constexpr int syn_split_voxel(int m) { return m < 4 ? 2 * m : (m >= 12 ? 2 * m - 16 : 2 * m - 7); }

// 64-lane wave reductions (CDNA wavefront = 64)
__device__ static inline float syn_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ static inline float syn_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ static inline float syn_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
