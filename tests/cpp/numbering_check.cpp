// The caller <-> internal numbering helpers of pucfem_host.hpp (to_internal / to_caller) against a direct
// restatement with a random permutation (tests/test_numbering_host.py).  Every case: internal -> caller into a
// sentinel-filled array equals the restatement and touches nothing outside the window's rows; caller -> internal of
// that result gives the window back bit for bit and touches nothing between or behind the planes; and caller ->
// internal of random caller data equals the restatement (with the element type's rounding).  One line per case.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pucfem_host.hpp"

using namespace pucfem;

template <class T>
static bool same(const T& a, const T& b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

// I: the internal side's element type, C: the caller's
template <class I, class C>
static int run(const char* types, i64 n, i64 r0, i64 N, int comp, bool split, i64 planes) {
  std::mt19937_64 rng((uint64_t)(n * 1000003 + r0 * 101 + N * 7 + comp * 3 + (split ? 1 : 0) + planes * 13));
  Ordering ord;
  ord.new2old.resize((size_t)N);
  for (i64 g = 0; g < N; ++g) ord.new2old[g] = (i32)g;
  std::shuffle(ord.new2old.begin(), ord.new2old.end(), rng);
  ord.old2new.resize((size_t)N);
  for (i64 g = 0; g < N; ++g) ord.old2new[ord.new2old[g]] = (i32)g;
  const i64 cstride = comp * N + 5;                    // (larger than a field: the caller's planes have gaps)
  const i64 per = (split ? 1 : comp) * n, istride = per + 2;
  const size_t clen = (size_t)(planes * cstride), ilen = (size_t)(planes * istride);
  const I isent = (I)-77;
  const C csent = (C)-99;
  auto val = [&] { return (double)((int64_t)(rng() % 2000001) - 1000000) / (sizeof(I) == 4 || sizeof(C) == 4 ? 1.0 : 977.0); };
  // internal data X (values every type here holds exactly, or doubles)
  std::vector<I> X0(ilen, isent), X1(split ? ilen : 0, isent);
  for (i64 p = 0; p < planes; ++p)
    for (i64 k = 0; k < per; ++k) {
      X0[p * istride + k] = (I)val();
      if (split) X1[p * istride + k] = (I)val();
    }
  // the internal element of (plane, window row, component)
  auto at = [&](std::vector<I>& a0, std::vector<I>& a1, i64 p, i64 i, int q) -> I& {
    return split ? (q ? a1 : a0)[p * istride + i] : a0[p * istride + comp * i + q];
  };
  bool ok = true;
  // 1. internal -> caller: the restatement, and the sentinel everywhere else
  std::vector<C> cal(clen, csent), want(clen, csent);
  to_caller(ord, r0, n, comp, planes, cstride, cal.data(), istride, X0.data(), split ? X1.data() : nullptr);
  for (i64 p = 0; p < planes; ++p)
    for (i64 i = 0; i < n; ++i)
      for (int q = 0; q < comp; ++q) want[p * cstride + comp * ord.new2old[r0 + i] + q] = (C)at(X0, X1, p, i, q);
  for (size_t k = 0; k < clen; ++k) ok &= same(cal[k], want[k]);
  // 2. and back: the identity on the window, nothing else written
  std::vector<I> Y0(ilen, isent), Y1(split ? ilen : 0, isent);
  to_internal(ord, r0, n, comp, planes, cstride, (const C*)cal.data(), istride, Y0.data(), split ? Y1.data() : nullptr);
  for (size_t k = 0; k < ilen; ++k) ok &= same(Y0[k], X0[k]) && (!split || same(Y1[k], X1[k]));
  // 3. caller -> internal of random caller data: the restatement (rounded to I)
  std::vector<C> src(clen);
  for (auto& v : src) v = (C)(val() / 3.0);
  std::vector<I> Z0(ilen, isent), Z1(split ? ilen : 0, isent), W0(ilen, isent), W1(split ? ilen : 0, isent);
  to_internal(ord, r0, n, comp, planes, cstride, (const C*)src.data(), istride, Z0.data(), split ? Z1.data() : nullptr);
  for (i64 p = 0; p < planes; ++p)
    for (i64 i = 0; i < n; ++i)
      for (int q = 0; q < comp; ++q) at(W0, W1, p, i, q) = (I)src[p * cstride + comp * ord.new2old[r0 + i] + q];
  for (size_t k = 0; k < ilen; ++k) ok &= same(Z0[k], W0[k]) && (!split || same(Z1[k], W1[k]));
  std::printf("%s n=%ld r0=%ld N=%ld comp=%d split=%d planes=%ld ok=%d\n", types, (long)n, (long)r0, (long)N, comp,
              split ? 1 : 0, (long)planes, ok ? 1 : 0);
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  for (i64 n : {0, 1, 2, 257})
    for (int win = 0; win < 3; ++win) {  // the whole range; a window at the start; one inside (r0 > 0, r0 + n < N)
      const i64 r0 = win == 2 ? 3 : 0, N = win == 0 ? n : n + 7;
      for (i64 planes : {1, 3})
        for (int lay = 0; lay < 3; ++lay) {  // scalar; interleaved pairs; pairs split into two arrays
          const int comp = lay == 0 ? 1 : 2;
          const bool split = lay == 2;
          bad += run<double, double>("f64<-f64", n, r0, N, comp, split, planes);
          bad += run<float, double>("f32<-f64", n, r0, N, comp, split, planes);
          bad += run<int32_t, int32_t>("i32<-i32", n, r0, N, comp, split, planes);
          bad += run<int32_t, double>("i32<-f64", n, r0, N, comp, split, planes);
        }
    }
  std::printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
