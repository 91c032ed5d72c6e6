// Sequential check of the union-find of synthsr_amd/csrc/seg_components_uf.h against a flood fill, on the host.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I synthsr_amd/csrc tools/seg_components_host_check.cpp -o check && ./check
//
// Two schedules per map and connectivity: the kernels' own (unions inside 8 x 8 x 32 tiles on tile-local indices, the tile
// roots written out as global indices, unions across tile borders, flatten), and every union of the map in a random order
// with stale non-root arguments.  Both must give, at every voxel, the smallest linear index of its component.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "seg_components_uf.h"

namespace {

constexpr int TZ = 8, TY = 8, TX = 32;

struct Map {
  int d0, d1, d2;
  std::vector<int> grp;   // group per voxel, -1: none
  int at(int z, int y, int x) const { return (z * d1 + y) * d2 + x; }
  bool inside(int z, int y, int x) const { return z >= 0 && z < d0 && y >= 0 && y < d1 && x >= 0 && x < d2; }
};

std::vector<int> flood_fill(const Map& m, int conn) {
  const int n = m.d0 * m.d1 * m.d2;
  std::vector<int> comp(n, -1), stack;
  for (int v = 0; v < n; ++v) {     // ascending: the seed is the smallest index of its component
    if (m.grp[v] < 0 || comp[v] >= 0) continue;
    comp[v] = v;
    stack.assign(1, v);
    while (!stack.empty()) {
      const int u = stack.back();
      stack.pop_back();
      const int z = u / (m.d1 * m.d2), y = u / m.d2 % m.d1, x = u % m.d2;
      for (int k = 0; k < 27; ++k) {
        int dz, dy, dx;
        ccu_step(k, dz, dy, dx);
        if (!ccu_adjacent(conn, dz, dy, dx) || !m.inside(z + dz, y + dy, x + dx)) continue;
        const int w = m.at(z + dz, y + dy, x + dx);
        if (m.grp[w] == m.grp[v] && comp[w] < 0) {
          comp[w] = v;
          stack.push_back(w);
        }
      }
    }
  }
  return comp;
}

std::vector<int> tiled(const Map& m, int conn) {
  const int n = m.d0 * m.d1 * m.d2;
  std::vector<int> parent(n, -1);
  for (int z0 = 0; z0 < m.d0; z0 += TZ)
    for (int y0 = 0; y0 < m.d1; y0 += TY)
      for (int x0 = 0; x0 < m.d2; x0 += TX) {
        int par[TZ * TY * TX], g[TZ * TY * TX];
        for (int l = 0; l < TZ * TY * TX; ++l) {
          const int z = z0 + l / (TY * TX), y = y0 + l / TX % TY, x = x0 + l % TX;
          par[l] = l;
          g[l] = m.inside(z, y, x) ? m.grp[m.at(z, y, x)] : -1;
        }
        for (int l = 0; l < TZ * TY * TX; ++l) {
          if (g[l] < 0) continue;
          const int lz = l / (TY * TX), ly = l / TX % TY, lx = l % TX;
          for (int k = 0; k < CCU_PRECEDING; ++k) {
            int dz, dy, dx;
            ccu_step(k, dz, dy, dx);
            const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
            if (!ccu_adjacent(conn, dz, dy, dx) || nz < 0 || ny < 0 || ny >= TY || nx < 0 || nx >= TX) continue;
            const int nl = (nz * TY + ny) * TX + nx;
            if (g[nl] == g[l]) ccu_union<CcuSeq>(par, l, nl);
          }
        }
        for (int l = 0; l < TZ * TY * TX; ++l) {
          if (g[l] < 0) continue;
          const int r = ccu_find<CcuSeq>(par, l);
          parent[m.at(z0 + l / (TY * TX), y0 + l / TX % TY, x0 + l % TX)] =
              m.at(z0 + r / (TY * TX), y0 + r / TX % TY, x0 + r % TX);
        }
      }
  for (int v = 0; v < n; ++v) {
    if (m.grp[v] < 0) continue;
    const int z = v / (m.d1 * m.d2), y = v / m.d2 % m.d1, x = v % m.d2;
    for (int k = 0; k < CCU_PRECEDING; ++k) {
      int dz, dy, dx;
      ccu_step(k, dz, dy, dx);
      const int nz = z + dz, ny = y + dy, nx = x + dx;
      if (!ccu_adjacent(conn, dz, dy, dx) || !m.inside(nz, ny, nx)) continue;
      if (nz / TZ == z / TZ && ny / TY == y / TY && nx / TX == x / TX) continue;
      if (m.grp[m.at(nz, ny, nx)] == m.grp[v]) ccu_union<CcuSeq>(parent.data(), v, m.at(nz, ny, nx));
    }
  }
  for (int v = 0; v < n; ++v)
    if (m.grp[v] >= 0) parent[v] = ccu_find<CcuSeq>(parent.data(), v);
  return parent;
}

std::vector<int> shuffled(const Map& m, int conn, std::mt19937& rng) {
  const int n = m.d0 * m.d1 * m.d2;
  std::vector<int> parent(n, -1);
  std::vector<std::pair<int, int>> edges;
  for (int v = 0; v < n; ++v) {
    if (m.grp[v] < 0) continue;
    parent[v] = v;
    const int z = v / (m.d1 * m.d2), y = v / m.d2 % m.d1, x = v % m.d2;
    for (int k = 0; k < CCU_PRECEDING; ++k) {
      int dz, dy, dx;
      ccu_step(k, dz, dy, dx);
      if (!ccu_adjacent(conn, dz, dy, dx) || !m.inside(z + dz, y + dy, x + dx)) continue;
      const int w = m.at(z + dz, y + dy, x + dx);
      if (m.grp[w] == m.grp[v]) edges.push_back(rng() & 1 ? std::make_pair(v, w) : std::make_pair(w, v));
    }
  }
  for (size_t i = edges.size(); i > 1; --i) std::swap(edges[i - 1], edges[rng() % i]);
  for (const auto& e : edges) ccu_union<CcuSeq>(parent.data(), e.first, e.second);
  for (int v = 0; v < n; ++v)
    if (m.grp[v] >= 0) parent[v] = ccu_find<CcuSeq>(parent.data(), v);
  return parent;
}

int failures = 0;

void check(const char* what, const Map& m, std::mt19937& rng) {
  for (int conn : {6, 18, 26}) {
    const std::vector<int> want = flood_fill(m, conn);
    const bool ok = tiled(m, conn) == want && shuffled(m, conn, rng) == want;
    if (!ok) ++failures;
    std::printf("%-12s %3d x %3d x %3d  connectivity %2d  %s\n", what, m.d0, m.d1, m.d2, conn, ok ? "ok" : "DIFFERS");
  }
}

}  // namespace

int main() {
  std::mt19937 rng(5);
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 70}, {5, 7, 9}, {9, 33, 65}, {7, 1, 33}, {17, 9, 31}, {8, 8, 32}, {16, 17, 64}};
  for (const auto& s : shapes) {
    Map m{s[0], s[1], s[2], {}};
    const int n = s[0] * s[1] * s[2];
    for (double density : {0.2, 0.31, 0.9}) {
      m.grp.resize(n);
      for (int v = 0; v < n; ++v) m.grp[v] = (rng() % 1000) < density * 1000 ? (int)(rng() % 3) : -1;
      check("random", m, rng);
    }
    m.grp.assign(n, 0);
    check("solid", m, rng);
    for (int v = 0; v < n; ++v) {
      const int z = v / (s[1] * s[2]), y = v / s[2] % s[1], x = v % s[2];
      m.grp[v] = (z + y + x) & 1 ? -1 : 0;
    }
    check("checkerboard", m, rng);
    for (int v = 0; v < n; ++v) {   // a comb: every other row along x, joined at alternating ends, planes joined likewise
      const int z = v / (s[1] * s[2]), y = v / s[2] % s[1], x = v % s[2];
      const bool row = y % 2 == 0, link = y % 2 == 1 && x == (y / 2 % 2 ? 0 : s[2] - 1);
      m.grp[v] = (z % 2 == 0 && (row || link)) || (z % 2 == 1 && y == 0 && x == (z / 2 % 2 ? 0 : s[2] - 1)) ? 1 : -1;
    }
    check("serpentine", m, rng);
  }
  std::printf(failures ? "%d FAILED\n" : "all equal\n", failures);
  return failures ? 1 : 0;
}
