// Union-find on a parent array, shared by the kernels of seg_components.hip and by the sequential host check
// (tools/seg_components_host_check.cpp).  The one invariant is parent[v] <= v: a link only ever points to a smaller index, so
// the root of a set is its smallest member that was ever made a root, and after all unions the smallest index of the set.
//
// Mem says how an element is read and lowered:
//   Mem::load(p)          a value that *p holds or held (never one that was never stored)
//   Mem::fetch_min(p, v)  *p = min(*p, v) in one indivisible step; returns the value before
// CcuSeq is the sequential form; the kernels supply LDS (workgroup scope) and global (device scope) atomics.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCU_FN __host__ __device__ __forceinline__
#else
#define CCU_FN inline
#endif

struct CcuSeq {
  static int load(const int* p) { return *p; }
  static int fetch_min(int* p, int v) {
    const int old = *p;
    if (v < old) *p = v;
    return old;
  }
};

template <class Mem>
CCU_FN int ccu_find(int* parent, int x) {
  // terminates: parent[x] <= x, so x strictly decreases until parent[x] == x (index 0 is always its own parent)
  for (;;) {
    const int p = Mem::load(parent + x);
    if (p == x) return x;
    x = p;
  }
}

// Joins the sets of a and b.  Either argument may be stale or no root.  With a > b the roots as this thread saw them,
// old = fetch_min(&parent[a], b):
//   old == a   a was a root and now points to b: done
//   old <  a   another thread linked a to `old` first.  parent[a] is now min(old, b): where that is b the link a -> old is
//              gone, where it is old the link a -> b was never made; either way what is left to join is old and b.
template <class Mem>
CCU_FN void ccu_union(int* parent, int a, int b) {
  // terminates: a round ends the loop or replaces the pair (a, b), a > b, by (old, b) with old < a: max(a, b) strictly decreases
  for (;;) {
    a = ccu_find<Mem>(parent, a);
    b = ccu_find<Mem>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = Mem::fetch_min(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// The 13 neighbours that precede a voxel in linear order (x fastest) are the codes k = 0 .. 12 of the 27-neighbourhood
// k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1); k = 13 is the voxel itself.  Adjacent under connectivity 6 / 18 / 26: at most
// 1 / 2 / 3 of the three steps are non-zero.
constexpr int CCU_PRECEDING = 13;
CCU_FN void ccu_step(int k, int& dz, int& dy, int& dx) {
  dz = k / 9 - 1;
  dy = (k / 3) % 3 - 1;
  dx = k % 3 - 1;
}
CCU_FN bool ccu_adjacent(int connectivity, int dz, int dy, int dx) {
  const int n = (dz != 0) + (dy != 0) + (dx != 0);
  return n >= 1 && n <= (connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3));
}
