// chain_host_main.cpp -- a stand-alone check of ngsf-hmm_amd/csrc/capi_chain_host.hpp, the host
// logic that the IBD entry points of the C ABI share.  tests/test_chain_host_cpu.py builds it with
// the address and undefined-behaviour sanitizers and runs it; it exits 0 when every check holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_chain_host.hpp"

static std::string g_msg;
void capi::set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_msg = buf;
}

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

using capi::align256;

// ---- the carver --------------------------------------------------------------------------------

// hands back a host buffer of exactly the bytes asked for: a write behind it is the sanitizer's
struct FakeOwner {
  std::unique_ptr<uint8_t[]> buf;
  uint8_t* p = nullptr;
  uint64_t asked = 0;
  int fail = 0;
  int reserve(uint64_t n) {
    if (fail) return fail;
    asked = n;
    buf.reset(new uint8_t[n ? n : 1]);
    p = buf.get();
    return NGHMM_OK;
  }
};

struct Rec48 {
  double v[6];
};

static void test_carver() {
  double* a = nullptr;
  uint32_t* b = nullptr;
  uint64_t* c = nullptr;
  uint8_t* d = nullptr;
  Rec48* e = nullptr;
  double* z = nullptr;
  const uint64_t na = 3, nb = 0, nc = 33, nd = 256, ne = 7, nz = 0;
  capi::Carver cv;
  cv.add(&a, na);
  cv.add(&b, nb);
  cv.add(&c, nc);
  cv.add(&d, nd);
  cv.add(&e, ne);
  cv.add(&z, nz);
  const uint64_t want[6] = {align256(na * 8), align256(nb * 4), align256(nc * 8), align256(nd), align256(ne * 48),
                            align256(nz * 8)};
  CHECK(want[0] == 256 && want[1] == 0 && want[2] == 512 && want[3] == 256 && want[4] == 512 && want[5] == 0);
  uint64_t total = 0;
  for (uint64_t w : want) total += w;
  CHECK(cv.bytes() == total);
  FakeOwner own;
  CHECK(cv.reserve(own) == NGHMM_OK);
  CHECK(own.asked == total);
  // registration order, every part a multiple of 256 behind the base, an empty part where the next lies
  uint8_t* at[6] = {reinterpret_cast<uint8_t*>(a), reinterpret_cast<uint8_t*>(b), reinterpret_cast<uint8_t*>(c), d,
                    reinterpret_cast<uint8_t*>(e), reinterpret_cast<uint8_t*>(z)};
  uint64_t off = 0;
  for (int k = 0; k < 6; ++k) {
    CHECK(at[k] == own.p + off);
    CHECK((at[k] - own.p) % 256 == 0);
    off += want[k];
  }
  CHECK(reinterpret_cast<uint8_t*>(b) == reinterpret_cast<uint8_t*>(c));
  CHECK(reinterpret_cast<uint8_t*>(z) == own.p + total);   // the last part, empty: the end of the buffer
  // every element of every part lies inside the buffer (the sanitizer judges) and in no other part
  for (uint64_t i = 0; i < na; ++i) a[i] = 1.0;
  for (uint64_t i = 0; i < nc; ++i) c[i] = ~0ull;
  for (uint64_t i = 0; i < nd; ++i) d[i] = 0x5a;
  for (uint64_t i = 0; i < ne; ++i)
    for (double& v : e[i].v) v = 2.0;
  for (uint64_t i = 0; i < na; ++i) CHECK(a[i] == 1.0);
  for (uint64_t i = 0; i < nc; ++i) CHECK(c[i] == ~0ull);
  for (uint64_t i = 0; i < nd; ++i) CHECK(d[i] == 0x5a);
  // an owner that cannot reserve: its code comes back and no pointer is touched
  double* q = nullptr;
  capi::Carver cv2;
  cv2.add(&q, 5);
  FakeOwner bad;
  bad.fail = NGHMM_ERR_NOMEM;
  CHECK(cv2.reserve(bad) == NGHMM_ERR_NOMEM && q == nullptr);
  // nothing registered: nothing reserved
  capi::Carver cv3;
  FakeOwner none;
  CHECK(cv3.reserve(none) == NGHMM_OK && none.asked == 0);
}

// ---- the region cut ----------------------------------------------------------------------------

struct Cut {
  std::vector<nghmm::ExpectRegion> parts;
  std::vector<uint64_t> owner;
  uint64_t n_pieces = 0;
};

// site by site: label every site of the shard with its region, open a part where the label
// changes, count a piece where the lane-chunk (local site / T) changes inside a part
static Cut brute_force(const std::vector<uint64_t>& begin, const std::vector<uint64_t>& end, uint64_t lo,
                       uint64_t hi, uint64_t T) {
  Cut c;
  int64_t prev = -1;
  for (uint64_t s = lo; s < hi; ++s) {
    int64_t label = -1;
    for (size_t k = 0; k < begin.size(); ++k)
      if (begin[k] <= s && s < end[k]) label = (int64_t)k;
    const uint64_t local = s - lo;
    if (label >= 0 && label != prev) {
      c.parts.push_back({local, local + 1, c.n_pieces, 0});
      c.owner.push_back((uint64_t)label);
      if (T) ++c.n_pieces;
    } else if (label >= 0) {
      c.parts.back().end = local + 1;
      if (T && local / T != (local - 1) / T) ++c.n_pieces;
    }
    prev = label;
  }
  return c;
}

static void test_cut() {
  const uint64_t sizes[3] = {5, 1, 130};   // cuts at sites 5 and 6
  const std::vector<std::vector<std::pair<uint64_t, uint64_t>>> sets = {
      // ends on the cut at 5 | starts on the cut at 6 | inside one lane-chunk of 2 sites of the third
      // shard (its sites 4, 5) | inside one lane-chunk of 64 sites (its sites 64 .. 68)
      {{1, 5}, {6, 9}, {10, 12}, {70, 75}},
      {{3, 8}},       // covers the one-site shard and spills over both sides
      {{0, 136}},     // everything
      {{4, 5}, {5, 6}, {6, 7}, {30, 40}, {40, 50}},   // one site each side of both cuts; adjacent regions
      {},             // R = 0
  };
  for (uint64_t T : {0ull, 1ull, 2ull, 64ull})
    for (const auto& set : sets) {
      std::vector<uint64_t> begin, end;
      for (const auto& g : set) {
        begin.push_back(g.first);
        end.push_back(g.second);
      }
      uint64_t lo = 0;
      for (uint64_t size : sizes) {
        const uint64_t hi = lo + size;
        Cut got;
        got.n_pieces = capi::cut_regions(begin.data(), end.data(), begin.size(), lo, hi, T, got.parts, got.owner);
        const Cut want = brute_force(begin, end, lo, hi, T);
        CHECK(got.n_pieces == want.n_pieces);
        CHECK(got.owner == want.owner);
        CHECK(got.parts.size() == want.parts.size());
        for (size_t k = 0; k < got.parts.size() && k < want.parts.size(); ++k) {
          CHECK(got.parts[k].begin == want.parts[k].begin && got.parts[k].end == want.parts[k].end);
          CHECK(got.parts[k].piece0 == want.parts[k].piece0 && got.parts[k].pad == 0);
        }
        if (T == 0) CHECK(got.n_pieces == 0);
        lo = hi;
      }
    }
  // the counts themselves, by hand, so that the brute force is not the only witness: set 0, third
  // shard (local [0, 3), [4, 6), [64, 69)), T = 2: 2 + 1 + 3 pieces
  {
    const uint64_t begin[4] = {1, 6, 10, 70}, end[4] = {5, 9, 12, 75};
    Cut got;
    got.n_pieces = capi::cut_regions(begin, end, 4, 6, 136, 2, got.parts, got.owner);
    CHECK(got.n_pieces == 6 && got.parts.size() == 3);
    CHECK(got.owner == (std::vector<uint64_t>{1, 2, 3}));
    CHECK(got.parts.size() == 3 && got.parts[1].piece0 == 2 && got.parts[2].piece0 == 3);
  }
}

// ---- the tract records -------------------------------------------------------------------------

static void test_records() {
  const char* who = "nghmm_tract_support";
  const uint64_t I = 3, S = 100;
  auto run = [&](std::vector<nghmm_tract> t) {
    g_msg.clear();
    return capi::check_tract_records(t.data(), t.size(), I, S, who);
  };
  auto rec = [](uint32_t ind, uint64_t first, uint64_t len) {
    nghmm_tract t;
    std::memset(&t, 0, sizeof t);
    t.ind = ind;
    t.first_site = first;
    t.n_sites = len;
    return t;
  };
  CHECK(run({rec(0, 0, 10), rec(0, 10, 5), rec(1, 0, 100), rec(2, 99, 1)}) == NGHMM_OK && g_msg.empty());
  CHECK(run({}) == NGHMM_OK && g_msg.empty());
  CHECK(run({rec(0, 4, 0)}) == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_support: record 0 has n_sites = 0");
  CHECK(run({rec(0, 0, 10), rec(7, 0, 10)}) == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_support: record 1 has ind = 7, of 3 individuals");
  CHECK(run({rec(0, 90, 20)}) == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_support: record 0, sites [90, 90 + 20), is outside the data's 100 sites");
  CHECK(run({rec(0, 100, 1)}) == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_support: record 0, sites [100, 100 + 1), is outside the data's 100 sites");
  const char* order =
      "nghmm_tract_support: record 1 (ind 0, first_site 5) is out of order or overlaps record 0: the "
      "records are ordered by (ind, first_site) and disjoint within an individual";
  CHECK(run({rec(0, 0, 10), rec(0, 5, 10)}) == NGHMM_ERR_ARG);   // overlaps
  CHECK(g_msg == order);
  CHECK(run({rec(1, 0, 10), rec(0, 5, 10)}) == NGHMM_ERR_ARG);   // out of order
  CHECK(g_msg == order);
  // the first failing record gives the message, and within a record the first failing check
  CHECK(run({rec(0, 0, 10), rec(0, 0, 0), rec(9, 0, 1)}) == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_support: record 1 has n_sites = 0");
  // one record at a time, as nghmm_tract_bounds walks them
  const std::vector<nghmm_tract> two = {rec(0, 0, 10), rec(9, 0, 1)};
  g_msg.clear();
  CHECK(capi::check_tract_record(two.data(), 0, I, S, "nghmm_tract_bounds") == NGHMM_OK && g_msg.empty());
  CHECK(capi::check_tract_record(two.data(), 1, I, S, "nghmm_tract_bounds") == NGHMM_ERR_ARG);
  CHECK(g_msg == "nghmm_tract_bounds: record 1 has ind = 9, of 3 individuals");
}

// ---- the merge ---------------------------------------------------------------------------------

static void test_merge() {
  double d[2] = {7.0, -0.0};
  const double s[2] = {-0.0, 3.0};
  auto fields = [&](auto op) {
    op(d[0], s[0]);
    op(d[1], s[1]);
  };
  capi::assign_or_add(true, fields);    // the first part's value itself, the sign of a zero included
  CHECK(d[0] == 0.0 && std::signbit(d[0]) && d[1] == 3.0);
  capi::assign_or_add(false, fields);
  CHECK(d[0] == 0.0 && std::signbit(d[0]) && d[1] == 6.0);
}

int main() {
  test_carver();
  test_cut();
  test_records();
  test_merge();
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("chain host logic: all checks hold\n");
  return 0;
}
