// ppcheck.cpp -- chomp_pp_plan.h on the host: where the tabulated redshift distributions of a
// batch of projection sets go in the sets' arena.  A program of its own (built and run by
// tests/test_pp_plan_cpu.py with the address and undefined-behaviour sanitizers); exits 0 when
// every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../chomp_amd/csrc/chomp_pp_plan.h"

using namespace chomp;

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

// A table of n pieces of order k in exactly-sized heap blocks (the sanitizer sees a read past
// either end), its values a function of `seed`.
struct Table {
  std::vector<double> breaks, coef;
  int n, order;
  Table(int n_, int order_, double seed) : n(n_), order(order_) {
    breaks.resize((size_t)n + 1);
    coef.resize((size_t)n * (order + 1));
    for (size_t i = 0; i < breaks.size(); ++i) breaks[i] = seed + 0.001 * (double)i;
    for (size_t i = 0; i < coef.size(); ++i) coef[i] = seed * 3.0 + (double)(i % 97) - 0.5 * (double)i;
  }
  PpTable view() const { return PpTable{breaks.data(), coef.data(), n, order}; }
};
static const PpTable kNone{nullptr, nullptr, 0, 0};

// The plan's invariants: analytic windows at -1; every table inside [0, total), at the place of
// an equal one or clear of every other; total the sum of the distinct tables; and the packed
// arena holds, at every window's place, that window's breaks and coefficients.
static void check_plan(const std::vector<PpTable>& t, const PpPlan& plan, size_t distinct) {
  CHECK(plan.offset.size() == t.size());
  CHECK(plan.owner.size() == distinct);
  size_t sum = 0;
  for (size_t q = 0; q < plan.owner.size(); ++q) sum += pp_doubles(t[plan.owner[q]]);
  CHECK(sum == plan.total);
  for (size_t i = 0; i < t.size(); ++i) {
    if (!t[i].breaks) { CHECK(plan.offset[i] == -1); continue; }
    CHECK(plan.offset[i] >= 0);
    CHECK((size_t)plan.offset[i] + pp_doubles(t[i]) <= plan.total);
    for (size_t j = 0; j < i; ++j) {
      if (!t[j].breaks) continue;
      const size_t a0 = (size_t)plan.offset[i], a1 = a0 + pp_doubles(t[i]);
      const size_t b0 = (size_t)plan.offset[j], b1 = b0 + pp_doubles(t[j]);
      if (a0 == b0) CHECK(detail::pp_same(t[i], t[j]));
      else CHECK(a1 <= b0 || b1 <= a0);
    }
  }
  std::vector<double> arena(plan.total);      // (exactly sized: a write past the end is seen)
  pp_pack(t.data(), plan, arena.data());
  for (size_t i = 0; i < t.size(); ++i) {
    if (!t[i].breaks) continue;
    const double* at = arena.data() + plan.offset[i];
    const size_t nb = (size_t)t[i].pp_n + 1, nc = (size_t)t[i].pp_n * (t[i].pp_order + 1);
    CHECK(std::memcmp(at, t[i].breaks, nb * sizeof(double)) == 0);
    CHECK(std::memcmp(at + nb, t[i].coef, nc * sizeof(double)) == 0);
  }
}

int main() {
  PpPlan plan;
  {   // no window at all, and no table among four windows
    CHECK(pp_plan(nullptr, 0, &plan) && plan.total == 0 && plan.offset.empty());
    std::vector<PpTable> t(4, kNone);
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 0);
    check_plan(t, plan, 0);
  }
  {   // one table
    Table a(16, 2, 0.25);
    std::vector<PpTable> t{kNone, a.view()};
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 16 * 4 + 1 && plan.offset[1] == 0);
    check_plan(t, plan, 1);
  }
  {   // equal bytes at two addresses, and the same addresses twice: one place
    Table a(16, 2, 0.25), b(16, 2, 0.25);
    CHECK(a.breaks.data() != b.breaks.data());
    std::vector<PpTable> t{a.view(), b.view(), kNone, a.view()};
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 65 && plan.offset[0] == 0 && plan.offset[1] == 0 && plan.offset[3] == 0);
    check_plan(t, plan, 1);
  }
  {   // equal length, other bytes (one coefficient, then one break): two places
    Table a(16, 2, 0.25), b(16, 2, 0.25), c(16, 2, 0.25);
    b.coef.back() += 1e-9;
    c.breaks[7] += 1e-12;
    std::vector<PpTable> t{a.view(), b.view(), c.view()};
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 3 * 65);
    check_plan(t, plan, 3);
  }
  {   // equal doubles in all, other shape: 5 pieces of order 1 and 3 pieces of order 3 are 16 each
    Table a(5, 1, 0.5), b(3, 3, 0.5);
    CHECK(pp_doubles(a.view()) == pp_doubles(b.view()));
    std::vector<PpTable> t{a.view(), b.view()};
    CHECK(pp_plan(t.data(), t.size(), &plan));
    check_plan(t, plan, 2);
  }
  {   // mixed lengths and orders 0 to 5, the five bins of 15 kernels among them
    std::vector<Table> own;
    for (int k = 0; k <= 5; ++k) own.emplace_back(3 + 7 * k, k, 0.1 * (k + 1));
    std::vector<PpTable> t;
    for (int i = 0; i < 5; ++i)
      for (int j = i; j < 5; ++j) { t.push_back(own[i].view()); t.push_back(own[j].view()); }
    t.push_back(kNone);
    t.push_back(own[5].view());
    CHECK(t.size() == 32);
    CHECK(pp_plan(t.data(), t.size(), &plan));
    check_plan(t, plan, 6);
  }
  {   // one piece, and the most pieces the C API takes
    Table a(1, 2, 0.75), b(65536, 5, 0.125), c(1, 0, 0.75);
    std::vector<PpTable> t{a.view(), b.view(), c.view(), b.view()};
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 5 + 458753 + 3);   // (pieces (order + 2) + 1 doubles each)
    check_plan(t, plan, 3);
  }
  {   // the cap: nine of the largest tables fit, the tenth does not; a small cap of its own
    std::vector<Table> own;
    for (int i = 0; i < 10; ++i) own.emplace_back(65536, 5, 1.0 + i);
    std::vector<PpTable> t;
    for (int i = 0; i < 9; ++i) t.push_back(own[i].view());
    CHECK(pp_plan(t.data(), t.size(), &plan));
    CHECK(plan.total == 9 * (size_t)458753 && plan.total <= kPpArenaMax);
    t.push_back(own[9].view());
    CHECK(!pp_plan(t.data(), t.size(), &plan));
    // (1024 sets of two tables each: equal ones are one table, distinct ones are refused)
    std::vector<PpTable> same(2048, own[0].view());
    CHECK(pp_plan(same.data(), same.size(), &plan));
    CHECK(plan.total == 458753);
    Table a(16, 2, 0.25), b(16, 2, 0.5);
    std::vector<PpTable> two{a.view(), b.view()};
    CHECK(pp_plan(two.data(), two.size(), &plan, 130));
    CHECK(!pp_plan(two.data(), two.size(), &plan, 129));
    CHECK(!pp_plan(two.data(), two.size(), &plan, 64));
  }
  if (failures) {
    std::printf("ppcheck: %d failures\n", failures);
    return 1;
  }
  std::printf("ppcheck ok\n");
  return 0;
}
