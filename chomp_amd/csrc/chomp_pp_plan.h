// The arena of tabulated redshift distributions behind the projection sets
// (chomp_kernel_setup_sets / chomp_kernel_setup_pairs): where each window's table goes.
// Host code only, nothing of HIP: a stand-alone program can include it
// (tests/hostcheck/ppcheck.cpp).
//
// A table is what DndzDev::pp points at: breaks[pp_n + 1], then coef[pp_n][pp_order + 1], that
// is pp_n (pp_order + 2) + 1 doubles.  Tables equal in pp_n, pp_order and bytes share one place,
// whatever their host addresses: the five bins behind the 15 kernels of a tomographic analysis
// are five tables, and the one window pair of chomp_kernel_setup_sets is two at most.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace chomp {

// One window's table as the caller holds it (breaks null: an analytic distribution, no table).
struct PpTable {
  const double* breaks;   // [pp_n + 1]
  const double* coef;     // [pp_n][pp_order + 1]
  int pp_n, pp_order;
};

// The arena's cap, in doubles (32 MiB): nine distinct tables of the largest kind (65536 pieces of
// order 5, 458753 doubles) fit, 1024 sets of two such tables (7 GiB) are refused before anything
// is allocated or copied.
constexpr size_t kPpArenaMax = (size_t)1 << 22;

inline size_t pp_doubles(const PpTable& t) {
  return (size_t)t.pp_n * ((size_t)t.pp_order + 2) + 1;
}

struct PpPlan {
  std::vector<long long> offset;   // per window: its table's first double in the arena, -1 for none
  std::vector<size_t> owner;       // per distinct table, in arena order: a window that holds it
  size_t total = 0;                // doubles of the arena
};

namespace detail {
inline std::uint64_t pp_hash(const PpTable& t) {   // FNV-1a over the table's bytes
  std::uint64_t h = 1469598103934665603ull;
  auto eat = [&h](const double* p, size_t n) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n * sizeof(double); ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  eat(t.breaks, (size_t)t.pp_n + 1);
  eat(t.coef, (size_t)t.pp_n * ((size_t)t.pp_order + 1));
  return h;
}
inline bool pp_same(const PpTable& a, const PpTable& b) {
  if (a.pp_n != b.pp_n || a.pp_order != b.pp_order) return false;
  if (a.breaks == b.breaks && a.coef == b.coef) return true;
  return std::memcmp(a.breaks, b.breaks, ((size_t)a.pp_n + 1) * sizeof(double)) == 0 &&
         std::memcmp(a.coef, b.coef, (size_t)a.pp_n * ((size_t)a.pp_order + 1) * sizeof(double)) == 0;
}
}  // namespace detail

// Lay the tables of n windows out.  The callers have validated them (proj_check_args: 1 <= pp_n
// <= 65536, 0 <= pp_order <= 5, non-null arrays).  Returns false, with the plan unusable, when the
// distinct tables exceed `cap` doubles; a table is only read (hashed) while the arena still has
// room for it, and one at the addresses of an earlier window is never read at all.
inline bool pp_plan(const PpTable* t, size_t n, PpPlan* plan, size_t cap = kPpArenaMax) {
  plan->offset.assign(n, -1);
  plan->owner.clear();
  plan->total = 0;
  std::vector<std::uint64_t> hash;   // per distinct table
  for (size_t i = 0; i < n; ++i) {
    if (!t[i].breaks) continue;
    const size_t nd = pp_doubles(t[i]);
    size_t hit = plan->owner.size();
    for (size_t q = 0; q < plan->owner.size() && hit == plan->owner.size(); ++q) {
      const PpTable& o = t[plan->owner[q]];
      if (o.breaks == t[i].breaks && o.coef == t[i].coef && o.pp_n == t[i].pp_n &&
          o.pp_order == t[i].pp_order)
        hit = q;
    }
    if (hit == plan->owner.size()) {
      if (nd > cap) return false;
      const std::uint64_t h = detail::pp_hash(t[i]);
      for (size_t q = 0; q < plan->owner.size() && hit == plan->owner.size(); ++q)
        if (hash[q] == h && detail::pp_same(t[plan->owner[q]], t[i])) hit = q;
      if (hit == plan->owner.size()) {
        if (plan->total + nd > cap) return false;
        plan->owner.push_back(i);
        hash.push_back(h);
        plan->offset[i] = (long long)plan->total;
        plan->total += nd;
        continue;
      }
    }
    plan->offset[i] = plan->offset[plan->owner[hit]];
  }
  return true;
}

// The arena's contents: every distinct table at its place, breaks then coefficients.
// arena: plan.total doubles.
inline void pp_pack(const PpTable* t, const PpPlan& plan, double* arena) {
  for (size_t q = 0; q < plan.owner.size(); ++q) {
    const PpTable& o = t[plan.owner[q]];
    double* dst = arena + plan.offset[plan.owner[q]];
    const size_t nb = (size_t)o.pp_n + 1, nc = (size_t)o.pp_n * ((size_t)o.pp_order + 1);
    std::memcpy(dst, o.breaks, nb * sizeof(double));
    std::memcpy(dst + nb, o.coef, nc * sizeof(double));
  }
}

}  // namespace chomp
