// Stand-alone check of the packed layout (bigkrls_amd/csrc/layout.h), built and run by tests/test_layout_cpu.py with
// -fsanitize=address,undefined. The declarations below repeat those of marginal_effects_impl (csrc/margeff.hip) and
// interaction_effects_impl (csrc/inteff.hip); the tables are written by hand for n = 7, p = 3, u = 5, nj = 2, m = 3,
// k = 4. Every pointer the layout hands out is written through, so the sanitizer sees a region that leaves its buffer.
#include "layout.h"

#include <cstdio>
#include <cstring>
#include <vector>

using bk::Layout;
using bk::Region;

struct Col { double bin, z0, z1, col; };   // the size of MeCol: 4 doubles
struct Pair { int a, b; };                 // the size of IePair: 1 double
struct Odd { int a, b, c; };               // 12 bytes: 3 records need 36 bytes, 5 doubles

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void check_table(const Layout& L, const std::vector<Region>& got, const std::vector<Region>& want, int n_up) {
  std::vector<double> dev((size_t)L.slot_doubles(), 0.0), pin((size_t)L.up_doubles(), 0.0);
  Layout B = L;
  B.bind_device(dev.data());
  B.bind_host(pin.data());
  CHECK(got.size() == want.size());
  for (size_t i = 0; i < got.size(); ++i) {
    CHECK(got[i].off == want[i].off && got[i].len == want[i].len);
    CHECK(B.d(got[i]) == dev.data() + want[i].off);
    for (int64_t e = 0; e < got[i].len; ++e) B.d(got[i])[e] += 1.0;              // every device double exactly once
    if ((int)i < n_up) {
      CHECK(B.h(got[i]) - pin.data() == B.d(got[i]) - dev.data());              // host and device offsets agree
      for (int64_t e = 0; e < got[i].len; ++e) B.h(got[i])[e] += 1.0;
    }
  }
  for (int64_t e = 0; e < L.slot_doubles() - 64; ++e) CHECK(dev[(size_t)e] == 1.0);   // no gap, no overlap
  for (int64_t e = 0; e < L.up_doubles(); ++e) CHECK(pin[(size_t)e] == 1.0);
}

int main() {
  const int64_t n = 7, p = 3, u = 5, nj = 2, m = 3, k = 4;
  {   // bigkrls_marginal_effects: q = 1 + nj
    const int64_t q = 1 + nj;
    Layout L;
    const Region Xs = L.up(n * p), Zs = L.up(u * p), B = L.up(n * q), Bs = L.up(u * q), cols = L.up_records<Col>(nj),
                 w = L.up(k);
    const Region R = L.dev(u * q), C = L.dev(n * q), D = L.dev(u * nj), S = L.dev(n * nj), T = L.dev(n * nj),
                 var = L.dev(nj);
    check_table(L, {Xs, Zs, B, Bs, cols, w, R, C, D, S, T, var},
                {{0, 21}, {21, 15}, {36, 21}, {57, 15}, {72, 8}, {80, 4}, {84, 15}, {99, 21}, {120, 10}, {130, 14},
                 {144, 14}, {158, 2}}, 6);
    CHECK(L.up_doubles() == 84 && L.slot_doubles() == 160 + 64 && L.down_doubles() == 0 && L.valid());
  }
  {   // bigkrls_interaction_effects: q = 1 + nj + m
    const int64_t q = 1 + nj + m;
    Layout L;
    const Region Xs = L.up(n * p), Zs = L.up(u * p), c = L.up(n), cols = L.up_records<Col>(nj),
                 pairs = L.up_records<Pair>(m), w = L.up(k);
    const Region S = L.dev(n * nj), R = L.dev(u * nj), T = L.dev(u * nj), B = L.dev(n * q), Bs = L.dev(u * q),
                 Rm = L.dev(u * q), Cm = L.dev(n * q), I = L.dev(u * m), Sv = L.dev(n * m), Tv = L.dev(n * m),
                 var = L.dev(m);
    check_table(L, {Xs, Zs, c, cols, pairs, w, S, R, T, B, Bs, Rm, Cm, I, Sv, Tv, var},
                {{0, 21}, {21, 15}, {36, 7}, {43, 8}, {51, 3}, {54, 4}, {58, 14}, {72, 10}, {82, 10}, {92, 42}, {134, 30},
                 {164, 30}, {194, 42}, {236, 15}, {251, 21}, {272, 21}, {293, 3}}, 6);
    CHECK(L.up_doubles() == 58 && L.slot_doubles() == 296 + 64 && L.valid());
  }
  {   // records are rounded up to whole doubles
    Layout L;
    const Region a = L.up_records<Odd>(3), b = L.up_records<Pair>(1), c = L.up_records<Odd>(0), d = L.up(2);
    CHECK(a.len == 5 && b.off == 5 && b.len == 1 && c.off == 6 && c.len == 0 && d.off == 6 && L.up_doubles() == 8);
    std::vector<double> pin((size_t)L.up_doubles());
    L.bind_host(pin.data());
    std::memset(L.h<Odd>(a), 0, (size_t)a.len * sizeof(double));
    L.h<Odd>(a)[2].c = 7;                                             // the last record lies inside its region
    CHECK((char*)(L.h<Odd>(a) + 3) <= (char*)L.h(b));
  }
  {   // zero-length regions (no factors, no covariance), an aliased region (newdata == nullptr), a read-back range
      // over several adjacent regions: the layout of bigkrls_partial_dependence with T = 6 grid values
    const int64_t T = 6, kq = 0, cov_doubles = 0;
    for (int with_newdata = 0; with_newdata < 2; ++with_newdata) {
      Layout L;
      const Region Xs = L.up(n * p), Zs = with_newdata ? L.up(u * p) : Xs, c = L.up(n), w = L.up(kq), vs = L.up(T);
      const Region M = L.dev(n * nj), val = L.down(T), var = L.down(T), cov = L.down(cov_doubles);
      const int64_t zs = with_newdata ? u * p : 0;
      CHECK(Zs.off == (with_newdata ? n * p : 0) && c.off == n * p + zs);
      CHECK(w.len == 0 && w.off == vs.off && cov.len == 0);
      CHECK(L.up_doubles() == n * p + zs + n + kq + T && M.off == L.up_doubles());
      CHECK(L.down_off() == val.off && L.down_doubles() == 2 * T + cov_doubles && var.off == val.off + T);
      CHECK(L.slot_doubles() == L.up_doubles() + n * nj + L.down_doubles() + 64);
      CHECK(L.valid() && L.down_adjacent());
    }
  }
  {   // out of order: an uploaded region after a device one; read-back regions that are not adjacent
    Layout L;
    L.up(3);
    L.dev(2);
    L.up(1);
    CHECK(!L.valid());
    Layout M;
    M.up(3);
    M.down(2);
    M.dev(1);
    M.down(2);
    CHECK(M.valid() && !M.down_adjacent() && M.down_doubles() == 4);
  }
  if (failures == 0) std::printf("layout_check: ok\n");
  return failures == 0 ? 0 : 1;
}
