// surface_edges of pucfem_host.hpp on synthetic rings (tests/test_loads_host.py; built with
// -fsanitize=address,undefined and run as its own program).  A ring of n marker-2 nodes inside a ring of n marker-1
// nodes, 2 n triangles between them, numbered so that the surface edges sit at changing local positions: the list has
// n edges in ascending (triangle, local edge) order, every inner node is once a and once b, opp is the third vertex;
// after red_refine the count doubles; a mesh without marker 2 has none; an edge between two marker-2 nodes that two
// triangles share is left out.  One line per case.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pucfem_host.hpp"

using namespace pucfem;

static HostMesh ring(int n, int inner_marker) {
  HostMesh m;
  m.N = 2 * n;
  m.x.resize(m.N);
  m.y.resize(m.N);
  m.mk.resize(m.N);
  const double pi = std::acos(-1.0);
  for (int i = 0; i < n; ++i) {
    const double th = 2 * pi * i / n;
    m.x[i] = 0.5 + 0.25 * std::cos(th);
    m.y[i] = 0.5 + 0.25 * std::sin(th);
    m.mk[i] = inner_marker;
    m.x[n + i] = 0.5 + 0.45 * std::cos(th);
    m.y[n + i] = 0.5 + 0.45 * std::sin(th);
    m.mk[n + i] = 1;
  }
  for (int i = 0; i < n; ++i) {
    const i32 a = i, b = (i + 1) % n, A = n + i, B = n + (i + 1) % n;
    // (a, A, B) and (a, B, b), rotated by i so that the inner edge b -> a is local edge 2, 0, 1, ...
    const i32 t1[3] = {a, A, B}, t2[3] = {a, B, b};
    for (int k = 0; k < 3; ++k) m.tri.push_back(t1[(k + i) % 3]);
    for (int k = 0; k < 3; ++k) m.tri.push_back(t2[(k + i) % 3]);
  }
  m.T = (i64)m.tri.size() / 3;
  return m;
}

static int check(const char* name, const HostMesh& m, i64 want) {
  SurfaceEdges S;
  surface_edges(m, S);
  int bad = S.size() != want || S.a.size() != S.tri.size() || S.b.size() != S.tri.size() || S.opp.size() != S.tri.size();
  std::vector<int> as_a(m.N, 0), as_b(m.N, 0);
  i64 prev = -1;
  for (i64 e = 0; e < S.size() && !bad; ++e) {
    const i64 t = S.tri[e];
    int k = -1;
    for (int q = 0; q < 3; ++q)
      if (m.tri[3 * t + q] == S.a[e] && m.tri[3 * t + (q + 1) % 3] == S.b[e]) k = q;
    bad |= k < 0 || m.tri[3 * t + (k + 2) % 3] != S.opp[e];
    bad |= m.mk[S.a[e]] != 2 || m.mk[S.b[e]] != 2;
    bad |= 3 * t + k <= prev;
    prev = 3 * t + k;
    ++as_a[S.a[e]];
    ++as_b[S.b[e]];
  }
  for (i64 i = 0; i < m.N && !bad; ++i) {
    const int on = m.mk[i] == 2 && want > 0 ? 1 : 0;
    bad |= as_a[i] != on || as_b[i] != on;
  }
  std::printf("%s %s edges=%lld\n", bad ? "FAIL" : "ok", name, (long long)S.size());
  return bad;
}

int main() {
  int bad = 0;
  for (int n : {3, 7, 60}) {
    HostMesh m = ring(n, 2);
    bad += check("ring", m, n);
    HostMesh r;
    red_refine(m, r);
    bad += check("ring refined", r, 2 * n);
    HostMesh r2;
    red_refine(r, r2);
    bad += check("ring refined twice", r2, 4 * n);
  }
  bad += check("no inner marker", ring(9, 1), 0);
  {  // a filled disc of marker-2 nodes: the spokes are shared by two triangles, the rim edges by one
    HostMesh m;
    const int n = 6;
    m.N = n + 1;
    m.x.assign(m.N, 0.5);
    m.y.assign(m.N, 0.5);
    m.mk.assign(m.N, 2);
    for (int i = 0; i < n; ++i) {
      m.x[i] += 0.25 * std::cos(i);
      m.y[i] += 0.25 * std::sin(i);
      m.tri.insert(m.tri.end(), {(i32)n, (i32)i, (i32)((i + 1) % n)});
    }
    m.T = n;
    SurfaceEdges S;
    surface_edges(m, S);
    int b = S.size() != n;
    for (i64 e = 0; e < S.size(); ++e) b |= S.a[e] == n || S.b[e] == n || S.opp[e] != n;
    std::printf("%s shared spokes edges=%lld\n", b ? "FAIL" : "ok", (long long)S.size());
    bad += b;
  }
  return bad ? 1 : 0;
}
