// Host-only self-test + fuzz harness for the native runtime core (rt_core.h, json_lite.h) and the
// route service's host code (route_core.h: route-request parsing, Python-exact float fast paths;
// alternatives.h: via-node candidates and scores; route_store.h + history_db.h: the route service's
// SQLite writer fills a database with fuzzed rows, the native history reads run over it with
// fuzzed limits / ids, and the two run against each other on two threads; map_match.h: the map
// matcher's node and edge candidate searches against a scan and its Viterbi against full enumeration).
// Built with -fsanitize=address,undefined by `tools/build_ext.py --sanitize` or the CMake `asan`
// preset (the reference has no race detection / sanitizers at all), and run by
// tests/test_sanitize_cpu.py.  Exit code 0 = all invariants held and no sanitizer report.
//
//   rt_selftest [iterations] [seed]
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "alternatives.h"
#include "avoid.h"
#include "history_db.h"
#include "map_match.h"
#include "route_core.h"
#include "route_store.h"
#include "rt_core.h"

using namespace rtc;

static int g_fail = 0;
#define CHECK(c, ...)                                      \
  do {                                                     \
    if (!(c)) {                                            \
      std::fprintf(stderr, "CHECK failed %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      ++g_fail;                                            \
    }                                                      \
  } while (0)

static const char* SEEDS[] = {
    R"({"summary":{"distance":12345},"pickup_time":"2025-08-25T08:30:00","driver_age":34,"weather":"Sunny","traffic":"Medium"})",
    R"([{"summary":{"distance":1000.5}},{"summary":{"distance":"2500"},"traffic":"Jam","pickup_time":"2024-02-29 23:59:59.999999+05:30"}])",
    R"({"items":[{"summary":null,"driver_age":0,"weather":"Hail"},{"pickup_time":"2025-01-01T00:00:00Z"}]})",
    R"({"summary":{"distance":1e308},"driver_age":"abc","pickup_time":"not-a-date"})",
    R"([1, "x", null, true, {"a":[1,2,{"b":NaN}],"c":Infinity,"d":-Infinity,"e":"é\"\\"}])",
};

static void fuzz_json(std::mt19937_64& rng, int iters) {
  const Stamp now{1756110600, 123456, false, 0, 0};
  for (int it = 0; it < iters; ++it) {
    std::string s = SEEDS[rng() % (sizeof SEEDS / sizeof *SEEDS)];
    const int muts = (int)(rng() % 6);
    for (int k = 0; k < muts && !s.empty(); ++k) {
      const size_t p = rng() % s.size();
      switch (rng() % 4) {
        case 0: s[p] = (char)(rng() & 0xFF); break;                       // flip a byte
        case 1: s.erase(p, 1 + rng() % 8); break;                          // delete a run
        case 2: s.insert(p, s.substr(rng() % s.size(), 1 + rng() % 16)); break;  // duplicate
        default: s.resize(p); break;                                       // truncate
      }
    }
    rtj::Value root;
    bool full_ok = true;
    try {
      root = rtj::Parser(s.data(), s.size()).parse();
    } catch (...) {
      full_ok = false;  // malformed JSON is rejected, never read out of bounds
    }
    // the parallel item splitter must agree with the full parser whenever it accepts a body
    std::vector<std::pair<size_t, size_t>> spans;
    if (split_top_array(s.data(), s.size(), spans)) {
      bool items_ok = true;
      for (auto& sp : spans) {
        try {
          rtj::Parser(s.data() + sp.first, sp.second - sp.first).parse();
        } catch (...) {
          items_ok = false;
        }
      }
      CHECK(items_ok == full_ok, "splitter/parser disagree on validity: %s", s.c_str());
      if (items_ok && full_ok)
        CHECK(root.kind == rtj::Value::Arr && root.arr.size() == spans.size(), "item count %zu vs %zu",
              root.arr.size(), spans.size());
    }
    if (!full_ok) continue;
    std::vector<const rtj::Value*> items;
    if (root.kind == rtj::Value::Arr)
      for (auto& v : root.arr) items.push_back(&v);
    else
      items.push_back(&root);
    std::string out;
    for (const rtj::Value* v : items) {
      EtaRecord r{};
      Stamp st;
      std::string err = pack_item(*v, now, r, st);
      if (err.empty()) {
        CHECK(r.weather <= 3 || r.weather == 255, "weather code %d", r.weather);
        CHECK(r.traffic <= 3 || r.traffic == 255, "traffic code %d", r.traffic);
      }
      static const double MINS[] = {17.25, 0.0, -3.5, 1e30, NAN, INFINITY, 1234567.891};
      format_one(out, MINS[rng() % 7], st.secs, st.us, st.has_tz, st.tz_sec, err);
    }
  }
}

static void fuzz_iso(std::mt19937_64& rng, int iters) {
  static const char alpha[] = "0123456789-:T .Z+z,";
  for (int it = 0; it < iters; ++it) {
    std::string s;
    const int n = (int)(rng() % 40);
    for (int k = 0; k < n; ++k) s += alpha[rng() % (sizeof alpha - 1)];
    Stamp st;
    if (parse_iso(s, st)) {
      // a parsed stamp re-formats to a string that parses to the same instant
      std::string f = isoformat(st.secs, st.us, st);
      Stamp st2;
      CHECK(parse_iso(f, st2) && st2.secs == st.secs && st2.us == st.us && st2.tz_sec == st.tz_sec,
            "iso round trip '%s' -> '%s'", s.c_str(), f.c_str());
    }
  }
  // calendar round trip over 600 years
  for (int64_t d = -80000; d < 140000; d += 17) {
    int64_t y;
    unsigned m, dd;
    civil_from_days(d, y, m, dd);
    CHECK(days_from_civil(y, m, dd) == d, "civil round trip %lld", (long long)d);
  }
}

static void fuzz_float(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters; ++it) {
    double v;
    switch (rng() % 3) {
      case 0: { uint64_t b = rng(); std::memcpy(&v, &b, 8); break; }         // any bit pattern
      case 1: v = std::ldexp((double)(rng() % 100000), (int)(rng() % 80) - 40); break;
      default: v = (double)(float)((rng() % 200000) / 997.0); break;           // float32 minutes
    }
    std::string o;
    append_pyfloat(o, v);
    if (std::isfinite(v)) {
      CHECK(std::strtod(o.c_str(), nullptr) == v, "repr round trip %.17g -> %s", v, o.c_str());
    }
    const int64_t us = timedelta_minutes_us(std::isfinite(v) && std::fabs(v) < 1e9 ? v : 1.5);
    (void)us;
  }
  CHECK(timedelta_minutes_us(0.5) == 30000000, "timedelta 0.5 min");
  CHECK(timedelta_minutes_us(1.0 / 60000000.0 * 2.5) == 2, "half-even rounding");
}

// route_core.h: py_round(x, 1)'s fast path, put_float's integer-tenths path and put_coord's
// six-decimal path must give the bits / text of their slow (CPython-equivalent) references, and
// parse_route_request must survive any mutated request body.
// route_core.h CoordCache: a route's coordinates copied from the per-node strings equal the
// formatted ones, byte for byte (nodes near 0, negative, with trailing zeros, repr-form values)
static void fuzz_coord_cache(std::mt19937_64& rng, int iters) {
  const size_t N = 512;
  std::vector<double> lat(N), lon(N);
  std::uniform_real_distribution<double> U(-180.0, 180.0);
  for (size_t n = 0; n < N; ++n) {
    switch (n % 5) {
      case 0: lat[n] = U(rng) / 2; lon[n] = U(rng); break;
      case 1: lat[n] = std::round(U(rng) * 1e3) / 1e3; lon[n] = std::round(U(rng) * 10) / 10; break;
      case 2: lat[n] = U(rng) * 1e-6; lon[n] = -U(rng) * 1e-5; break;
      case 3: lat[n] = 14.5 + U(rng) * 1e-4; lon[n] = 121.0 + U(rng) * 1e-4; break;
      default: lat[n] = 0.0; lon[n] = -0.0; break;
    }
  }
  rtr::CoordCache cc;
  cc.build(lat.data(), lon.data(), N);
  for (int it = 0; it < iters; ++it) {
    std::vector<double> xy;
    std::vector<uint8_t> raw;
    std::vector<int32_t> node;
    const int len = 1 + (int)(rng() % 40);
    for (int i = 0; i < len; ++i) {
      if (rng() % 4 == 0) {
        xy.push_back(U(rng));
        xy.push_back(U(rng) / 2);
        raw.push_back(1);
        node.push_back(-1);
      } else {
        const int n = (int)(rng() % N);
        xy.push_back(rtr::np_round6(lon[n]));
        xy.push_back(rtr::np_round6(lat[n]));
        raw.push_back(0);
        node.push_back(n);
      }
    }
    std::string a, b;
    rtr::put_coords(a, xy, raw);
    rtr::put_coords(b, xy, raw, &node, &cc);
    CHECK(a == b, "coord cache: %s vs %s", a.c_str(), b.c_str());
  }
}

static void fuzz_route(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters; ++it) {
    double x;
    switch (rng() % 4) {
      case 0: x = ((double)(int64_t)(rng() % 2000000000) - 1e9) / 997.0; break;
      case 1: x = ((double)(int64_t)(rng() % 20000001) - 1e7 + 0.5) / 10.0; break;     // midpoints
      case 2: x = std::nextafter(((double)(rng() % 100000) + 0.05), rng() & 1 ? 1e9 : -1e9); break;
      default: { uint64_t b = rng(); std::memcpy(&x, &b, 8); break; }
    }
    if (!std::isfinite(x)) continue;
    char b[64];
    std::snprintf(b, sizeof b, "%.1f", x);
    const double slow = std::strtod(b, nullptr);
    const double fast = rtr::py_round(x, 1);
    CHECK(std::memcmp(&slow, &fast, 8) == 0 || (slow == 0.0 && fast == 0.0 && std::signbit(slow) == std::signbit(fast)),
          "py_round(%.17g, 1): fast %.17g, slow %.17g", x, fast, slow);
    std::string a1, a2;
    rtr::put_float(a1, fast);
    rtc::append_pyfloat(a2, fast);
    CHECK(a1 == a2, "put_float(%.17g): %s vs repr %s", fast, a1.c_str(), a2.c_str());
    const double c = rtr::np_round6(x / 1000.0);
    std::string c1, c2;
    rtr::put_coord(c1, c);
    rtc::append_pyfloat(c2, c);
    CHECK(c1 == c2, "put_coord(%.17g): %s vs repr %s", c, c1.c_str(), c2.c_str());
  }
  static const char* RSEEDS[] = {
      R"({"source_point":{"lat":14.55,"lon":121.02},"destination_points":[{"lat":14.56,"lon":121.03,"payload":2},{"lat":14.57,"lon":121.0}],"vehicle_capacity":5,"maximum_distance":90000,"use_ml_eta":true,"context":{"weather":"Stormy","traffic":"High"},"alternatives":3})",
      R"({"source_point":{"lat":"14.5","lon":121},"destination_points":[],"vehicle_type":"motorcycle","driver_details":{"driver_age":"41"},"meta":{"origin_id":7,"destination_ids":[1,2]}})",
      R"({"source_point":null,"destination_points":[{"lat":1e308,"lon":-1e308}],"vehicle_capacity":-1,"alternatives":1e30})",
  };
  for (int it = 0; it < iters; ++it) {
    std::string s = RSEEDS[rng() % (sizeof RSEEDS / sizeof *RSEEDS)];
    const int muts = (int)(rng() % 5);
    for (int k = 0; k < muts && !s.empty(); ++k) {
      const size_t p = rng() % s.size();
      switch (rng() % 3) {
        case 0: s[p] = (char)(rng() & 0xFF); break;
        case 1: s.erase(p, 1 + rng() % 6); break;
        default: s.insert(p, s.substr(rng() % s.size(), 1 + rng() % 12)); break;
      }
    }
    try {
      rtj::Value root = rtj::Parser(s.data(), s.size()).parse();
      const rtr::RouteReq r = rtr::parse_route_request(&root);
      CHECK(r.error.empty() || r.dst.empty() || true, "unreachable");
    } catch (...) {
    }
  }
}

// route_core.h improve_trips: on random matrices (asymmetric, with NaN / inf / negative entries)
// over the greedy's own trips every trip keeps its stops and ends, the quantized length never
// grows, the statistics add up, and a second pass finds nothing more unless the first reverted
static void fuzz_improve(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 100; ++it) {
    const int n1 = 2 + (int)(rng() % 40);
    std::vector<double> d((size_t)n1 * n1, 0.0), dem(n1, 1.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
    if (rng() % 4 == 0 && n1 > 3) {
      d[(size_t)1 * n1 + 2] = NAN;
      d[(size_t)2 * n1 + 3] = INFINITY;
      d[(size_t)3 * n1 + 1] = -5.0;
    }
    const double cap = 1.0 + (double)(rng() % 50);
    std::vector<std::vector<int>> trips, before;
    std::vector<int> inf;
    if (!rtr::greedy_trips(d, n1, dem, cap, 9e12, trips, inf)) continue;
    before = trips;
    const double maxd = rng() % 3 == 0 ? 1500.0 * n1 : 9e12;
    const rtr::ImproveStats st = rtr::improve_trips(d, n1, maxd, trips);
    CHECK(trips.size() == before.size(), "improve_trips changed the trip count");
    long long changed = 0;
    for (size_t t = 0; t < trips.size() && t < before.size(); ++t) {
      std::vector<int> a = trips[t], b = before[t];
      CHECK(a.size() == b.size() && a.front() == 0 && a.back() == 0, "improve_trips broke a trip's ends");
      changed += a != b;
      std::sort(a.begin(), a.end());
      std::sort(b.begin(), b.end());
      CHECK(a == b, "improve_trips changed a trip's stops");
    }
    CHECK(changed == st.trips_changed && st.len_after_q <= st.len_before_q && (st.moves > 0) == (changed > 0),
          "improve_trips statistics: %lld changed vs %lld, %lld -> %lld", changed, st.trips_changed, st.len_before_q,
          st.len_after_q);
    const rtr::ImproveStats again = rtr::improve_trips(d, n1, 9e12, trips);
    CHECK(again.len_before_q == st.len_after_q, "improve_trips: length after %lld, measured again %lld",
          st.len_after_q, again.len_before_q);
    if (maxd == 9e12) CHECK(again.moves == 0, "improve_trips left %lld moves", again.moves);
  }
}

// route_core.h exchange_trips: on random matrices (asymmetric, with NaN / inf / negative entries),
// random hand-made trips and random limits every stop stays exactly once, trips keep their depot
// ends, no trip is created, the reported length is the measured one, every trip that changed passes
// the greedy's float walks, and a search that ended on its own leaves nothing to a second call
// (under the same limits; a third of the runs have none at all)
static void fuzz_exchange(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 100; ++it) {
    const int n1 = 2 + (int)(rng() % 30);
    std::vector<double> d((size_t)n1 * n1, 0.0), dem(n1, 0.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
    if (rng() % 4 == 0 && n1 > 3) {
      d[(size_t)1 * n1 + 2] = NAN;
      d[(size_t)2 * n1 + 3] = INFINITY;
      d[(size_t)3 * n1 + 1] = -5.0;
    }
    for (int s = 1; s < n1; ++s) dem[s] = (double)(1 + rng() % 3);
    if (rng() % 16 == 0) dem[1 + rng() % (n1 - 1)] = rng() % 2 ? NAN : -1.0;   // the stage is skipped
    // hand-made trips: a random permutation cut at random places (some trips empty)
    std::vector<int> perm(n1 - 1);
    for (int s = 1; s < n1; ++s) perm[s - 1] = s;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<std::vector<int>> trips(1, std::vector<int>{0});
    for (int s : perm) {
      if (rng() % 4 == 0) {
        trips.back().push_back(0);
        trips.push_back({0});
      }
      trips.back().push_back(s);
    }
    trips.back().push_back(0);
    const std::vector<std::vector<int>> before = trips;
    const bool free_run = rng() % 3 == 0;
    const double cap = free_run ? 9e12 : (double)(2 + rng() % 30);
    const double maxd = free_run ? 9e12 : (rng() % 8 == 0 ? NAN : 20000.0 + (double)(rng() % 400000));
    const long long move_cap = rng() % 8 == 0 ? (long long)(rng() % 4) : -1;
    const rtr::ExchangeStats st = rtr::exchange_trips(d, n1, dem, cap, maxd, trips, move_cap);
    std::vector<int> seen(n1, 0);
    long long len = 0;
    for (const auto& t : trips) {
      CHECK(t.size() >= 2 && t.front() == 0 && t.back() == 0, "exchange_trips broke a trip's ends");
      for (size_t p = 1; p + 1 < t.size(); ++p)
        if (t[p] >= 1 && t[p] < n1) ++seen[t[p]];
      for (size_t p = 0; p + 1 < t.size(); ++p) len += rtr::improve_q(d[(size_t)t[p] * n1 + t[p + 1]]);
      if (std::find(before.begin(), before.end(), t) == before.end()) {  // a changed trip: the greedy's walks
        double s = 0.0, load = 0.0;
        const int k = (int)t.size() - 2;
        for (int p = 0; p < k; ++p) s += d[(size_t)t[p] * n1 + t[p + 1]];
        for (int p = 1; p <= k; ++p) load += dem[t[p]];
        CHECK(s + d[(size_t)t[k] * n1] <= maxd && load <= cap, "exchange_trips kept a trip that fails the float walks");
      }
    }
    bool once = true;
    for (int s = 1; s < n1; ++s) once = once && seen[s] == 1;
    CHECK(once, "exchange_trips lost or repeated a stop");
    CHECK(st.trips_before == (long long)before.size() && st.trips_after == (long long)trips.size() &&
              st.trips_after <= st.trips_before,
          "exchange_trips trip counts: %lld -> %lld, %zu -> %zu", st.trips_before, st.trips_after, before.size(), trips.size());
    CHECK(len == st.len_after_q && st.len_after_q <= st.len_before_q, "exchange_trips: length after %lld, measured %lld, before %lld",
          st.len_after_q, len, st.len_before_q);
    CHECK(st.moves > 0 || trips == before || st.trips_after < st.trips_before, "exchange_trips changed trips without a move");
    if (!st.rejected && move_cap < 0 && st.moves < 4LL * (n1 - 1)) {
      std::vector<std::vector<int>> again = trips;
      const rtr::ExchangeStats st2 = rtr::exchange_trips(d, n1, dem, cap, maxd, again, -1);
      CHECK(st2.moves == 0 && again == trips, "exchange_trips left %lld moves", st2.moves);
      CHECK(st2.len_before_q == st.len_after_q, "exchange_trips: length after %lld, measured again %lld", st.len_after_q,
            st2.len_before_q);
    }
  }
}

// route_core.h tw_trips: on random metres / seconds matrices (asymmetric, with NaN / inf / negative /
// huge entries) and random windows and service times, either some stop is reported infeasible alone
// (indices in range, ascending) or every stop is placed exactly once, every trip re-simulates as
// feasible on usable entries only, the reported arrivals / starts are the re-simulated ones, and the
// statistics are the measured ones
static void fuzz_tw(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 100; ++it) {
    const int n1 = 1 + (int)(rng() % 34);
    std::vector<double> d((size_t)n1 * n1, 0.0), t((size_t)n1 * n1, 0.0), dem(n1, 0.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) {
          d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
          t[(size_t)a * n1 + b] = 10.0 + (double)(rng() % 100000) / 53.0;
        }
    if (rng() % 3 == 0 && n1 > 4) {
      const double bad[6] = {NAN, INFINITY, -5.0, 2147483.647, 3e9, 1e300};
      for (int x = 0; x < 6; ++x) {
        std::vector<double>& m = rng() % 2 ? d : t;
        // mostly between stops; now and then on a depot leg, which makes a stop infeasible alone
        const int a = rng() % 8 == 0 ? 0 : 1 + (int)(rng() % (n1 - 1)), b = 1 + (int)(rng() % (n1 - 1));
        if (a != b) m[(size_t)a * n1 + b] = bad[rng() % 6];
      }
    }
    std::vector<long long> open(n1, 0), close(n1, rtr::kExchangeUnbounded), sv(n1, 0);
    for (int s = 1; s < n1; ++s) {
      dem[s] = (double)(1 + rng() % 3);
      if (rng() % 10 < 7) {
        open[s] = (long long)(rng() % 20000000);
        close[s] = open[s] + (long long)(rng() % 3 == 0 ? 0 : rng() % 8000000);
        if (rng() % 4 == 0) open[s] = 0;
      }
      if (rng() % 2) sv[s] = (long long)(rng() % 600000);
    }
    if (rng() % 16 == 0 && n1 > 1) dem[1 + rng() % (n1 - 1)] = rng() % 2 ? NAN : -1.0;
    const bool free_run = rng() % 3 == 0;
    const double cap = free_run ? 9e12 : (rng() % 16 == 0 ? NAN : (double)(3 + rng() % 30));
    const double maxd = free_run ? 9e12 : (rng() % 16 == 0 ? -1.0 : 60000.0 + (double)(rng() % 400000));
    std::vector<std::vector<int>> trips;
    std::vector<std::vector<long long>> arr, sta;
    std::vector<int> bad;
    rtr::TwStats st;
    if (!rtr::tw_trips(d, t, n1, dem, cap, maxd, open, close, sv, trips, arr, sta, bad, st)) {
      CHECK(!bad.empty() && trips.empty(), "tw_trips failed without naming a stop");
      for (size_t x = 0; x < bad.size(); ++x)
        CHECK(bad[x] >= 0 && bad[x] < n1 - 1 && (x == 0 || bad[x] > bad[x - 1]), "tw_trips infeasible index %d", bad[x]);
      continue;
    }
    std::vector<int> seen(n1, 0);
    long long len = 0, waiting = 0;
    CHECK(trips.size() == arr.size() && trips.size() == sta.size() && st.trips == (long long)trips.size(), "tw_trips trip counts");
    for (size_t k = 0; k < trips.size(); ++k) {
      const std::vector<int>& tr = trips[k];
      CHECK(tr.size() >= 3 && tr.front() == 0 && tr.back() == 0, "tw_trips broke a trip's ends");
      CHECK(arr[k].size() + 2 == tr.size() && sta[k].size() + 2 == tr.size(), "tw_trips schedule length");
      long long clock = 0;
      bool ok = true;
      for (size_t p = 0; p + 1 < tr.size(); ++p) {
        const int a = tr[p], b = tr[p + 1];
        if (a < 0 || a >= n1 || b < 0 || b >= n1) { ok = false; break; }
        const long long q = rtr::tw_q(d[(size_t)a * n1 + b]), qt = rtr::tw_q(t[(size_t)a * n1 + b]);
        ok = ok && q < rtr::kImproveBig && qt < rtr::kImproveBig;
        len += q;
        if (b == 0) break;
        ++seen[b];
        const long long ar = clock + qt, s0 = std::max(ar, open[b]);
        ok = ok && s0 <= close[b] && p < arr[k].size() && arr[k][p] == ar && sta[k][p] == s0;
        waiting += s0 - ar;
        clock = s0 + sv[b];
      }
      CHECK(ok, "tw_trips built a trip that does not re-simulate as feasible");
      double s = 0.0, load = 0.0;
      const int kk = (int)tr.size() - 2;
      for (int p = 0; p < kk; ++p) s += d[(size_t)tr[p] * n1 + tr[p + 1]];
      for (int p = 1; p <= kk; ++p) load += dem[tr[p]];
      CHECK(s + d[(size_t)tr[kk] * n1] <= maxd && load <= cap, "tw_trips kept a trip that fails the float walks");
    }
    bool once = true;
    for (int s = 1; s < n1; ++s) once = once && seen[s] == 1;
    CHECK(once, "tw_trips lost or repeated a stop");
    CHECK(len == st.len_q && waiting == st.waiting_q, "tw_trips statistics: len %lld / %lld, waiting %lld / %lld", st.len_q, len,
          st.waiting_q, waiting);
    CHECK(st.insertions + st.trips == (long long)(n1 - 1), "tw_trips: %lld insertions + %lld trips != %d stops", st.insertions,
          st.trips, n1 - 1);
  }
}

// route_core.h tw_improve_trips on tw_trips' output (instances as in fuzz_tw, half as many): every
// kept trip re-simulates as feasible on usable entries with the reported arrivals / starts, both
// float walks hold, no stop is lost or repeated, the length never grows, the statistics are the
// measured ones, and a search that ended on its own leaves nothing for a second run
static void fuzz_tw_improve(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 200; ++it) {
    const int n1 = 2 + (int)(rng() % 33);
    std::vector<double> d((size_t)n1 * n1, 0.0), t((size_t)n1 * n1, 0.0), dem(n1, 0.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) {
          d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
          t[(size_t)a * n1 + b] = 10.0 + (double)(rng() % 100000) / 53.0;
        }
    if (rng() % 3 == 0 && n1 > 4) {
      const double bad[6] = {NAN, INFINITY, -5.0, 2147483.647, 3e9, 1e300};
      for (int x = 0; x < 6; ++x) {
        std::vector<double>& m = rng() % 2 ? d : t;
        const int a = 1 + (int)(rng() % (n1 - 1)), b = 1 + (int)(rng() % (n1 - 1));
        if (a != b) m[(size_t)a * n1 + b] = bad[rng() % 6];
      }
    }
    std::vector<long long> open(n1, 0), close(n1, rtr::kExchangeUnbounded), sv(n1, 0);
    for (int s = 1; s < n1; ++s) {
      dem[s] = rng() % 8 == 0 ? 0.1 : (double)(1 + rng() % 3);
      if (rng() % 10 < 6) {
        open[s] = (long long)(rng() % 20000000);
        close[s] = open[s] + (long long)(rng() % 3 == 0 ? 0 : rng() % 8000000);
        if (rng() % 4 == 0) open[s] = 0;
      }
      if (rng() % 2) sv[s] = (long long)(rng() % 600000);
    }
    if (rng() % 32 == 0) dem[1 + rng() % (n1 - 1)] = -1.0;
    const bool free_run = rng() % 3 == 0;
    const double cap = free_run ? 9e12 : (double)(3 + rng() % 30) + (rng() % 4 == 0 ? 0.3 : 0.0);
    const double maxd = free_run ? 9e12 : 60000.0 + (double)(rng() % 400000);
    std::vector<std::vector<int>> trips;
    std::vector<std::vector<long long>> arr, sta;
    std::vector<int> bad;
    rtr::TwStats st0;
    if (!rtr::tw_trips(d, t, n1, dem, cap, maxd, open, close, sv, trips, arr, sta, bad, st0)) continue;
    const std::vector<std::vector<int>> before = trips;
    const rtr::TwImproveStats st = rtr::tw_improve_trips(d, t, n1, dem, cap, maxd, open, close, sv, trips, arr, sta);
    std::vector<int> seen(n1, 0);
    long long len = 0, waiting = 0;
    CHECK(trips.size() == arr.size() && trips.size() == sta.size(), "tw_improve_trips schedule count");
    for (size_t k = 0; k < trips.size(); ++k) {
      const std::vector<int>& tr = trips[k];
      CHECK(tr.size() >= 3 && tr.front() == 0 && tr.back() == 0, "tw_improve_trips broke a trip's ends");
      CHECK(arr[k].size() + 2 == tr.size() && sta[k].size() + 2 == tr.size(), "tw_improve_trips schedule length");
      long long clock = 0;
      bool ok = true;
      for (size_t p = 0; p + 1 < tr.size(); ++p) {
        const int a = tr[p], b = tr[p + 1];
        if (a < 0 || a >= n1 || b < 0 || b >= n1) { ok = false; break; }
        const long long q = rtr::tw_q(d[(size_t)a * n1 + b]), qt = rtr::tw_q(t[(size_t)a * n1 + b]);
        ok = ok && q < rtr::kImproveBig && qt < rtr::kImproveBig;
        len += q;
        if (b == 0) break;
        ++seen[b];
        const long long ar = clock + qt, s0 = std::max(ar, open[b]);
        ok = ok && s0 <= close[b] && p < arr[k].size() && arr[k][p] == ar && sta[k][p] == s0;
        waiting += s0 - ar;
        clock = s0 + sv[b];
      }
      CHECK(ok, "tw_improve_trips kept a trip that does not re-simulate as feasible");
      double s = 0.0, load = 0.0;
      const int kk = (int)tr.size() - 2;
      for (int p = 0; p < kk; ++p) s += d[(size_t)tr[p] * n1 + tr[p + 1]];
      for (int p = 1; p <= kk; ++p) load += dem[tr[p]];
      CHECK(s + d[(size_t)tr[kk] * n1] <= maxd && load <= cap, "tw_improve_trips kept a trip that fails the float walks");
    }
    bool once = true;
    for (int s = 1; s < n1; ++s) once = once && seen[s] == 1;
    CHECK(once, "tw_improve_trips lost or repeated a stop");
    CHECK(st.trips_before == (long long)before.size() && st.trips_after == (long long)trips.size() &&
              st.trips_after <= st.trips_before && st.len_before_q == st0.len_q,
          "tw_improve_trips trip counts: %lld -> %lld, %zu -> %zu", st.trips_before, st.trips_after, before.size(), trips.size());
    CHECK(len == st.len_after_q && st.len_after_q <= st.len_before_q && waiting == st.waiting_q,
          "tw_improve_trips: length after %lld, measured %lld, before %lld; waiting %lld / %lld", st.len_after_q, len,
          st.len_before_q, st.waiting_q, waiting);
    CHECK(st.moves >= 0 && st.moves <= 4LL * (n1 - 1) && (st.rejected == 0 || st.rejected == 1), "tw_improve_trips move count");
    CHECK(st.moves > 0 || trips == before, "tw_improve_trips changed trips without a move");
    CHECK(st.moves == 0 || st.len_after_q < st.len_before_q, "tw_improve_trips: moves without a shorter length");
    if (st.rejected == 0 && st.moves < 4LL * (n1 - 1)) {
      std::vector<std::vector<int>> again = trips;
      std::vector<std::vector<long long>> arr2, sta2;
      const rtr::TwImproveStats st2 = rtr::tw_improve_trips(d, t, n1, dem, cap, maxd, open, close, sv, again, arr2, sta2);
      CHECK(st2.moves == 0 && again == trips && arr2 == arr && sta2 == sta, "tw_improve_trips left %lld moves", st2.moves);
    }
  }
}

// map_match.h mm_candidates: on random node sets (clusters, duplicates, one line) and fixes inside,
// on and far outside the grid the answer equals a scan of all nodes sorted by (d2, node id)
static void fuzz_mm_candidates(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 200; ++it) {
    const size_t n = 1 + rng() % 400;
    const int64_t span = 1 + (int64_t)(rng() % 3000000), ox = (int64_t)(rng() % 4000000000ULL) - 2000000000LL;
    const bool line = rng() % 8 == 0;
    std::vector<int64_t> qy(n), qx(n);
    for (size_t i = 0; i < n; ++i) {
      qy[i] = 162000000 + (int64_t)(rng() % span);
      qx[i] = line ? ox : ox + (int64_t)(rng() % span);
      if (i && rng() % 16 == 0) {   // a node on top of another one
        qy[i] = qy[i - 1];
        qx[i] = qx[i - 1];
      }
    }
    rtr::MmGrid g;
    g.build(qy.data(), qx.data(), n);
    CHECK(g.start.back() == (int32_t)n && (int64_t)g.ny * g.nx < 5000000, "MmGrid: %d x %d cells", g.ny, g.nx);
    const size_t P = 1 + rng() % 40;
    const int k = 1 + (int)(rng() % 16);
    const int64_t radius = 1 + (int64_t)(rng() % 100000);
    std::vector<int64_t> py(P), px(P);
    for (size_t p = 0; p < P; ++p) {
      const size_t v = rng() % n;
      switch (rng() % 4) {
        case 0: py[p] = qy[v]; px[p] = qx[v]; break;                                     // on a node
        case 1: py[p] = qy[v] + radius; px[p] = qx[v]; break;                            // exactly at the radius
        case 2: py[p] = qy[v] + (int64_t)(rng() % 4000000) - 2000000; px[p] = qx[v] - 3 * radius; break;
        default: py[p] = qy[v] + (int64_t)(rng() % (2 * radius + 1)) - radius;
                 px[p] = qx[v] + (int64_t)(rng() % (2 * radius + 1)) - radius; break;
      }
    }
    std::vector<int32_t> cand(P * k), nc(P);
    std::vector<int64_t> d2(P * k);
    rtr::mm_candidates(g, py.data(), px.data(), P, radius, k, cand.data(), d2.data(), nc.data());
    for (size_t p = 0; p < P; ++p) {
      std::vector<std::pair<int64_t, int32_t>> all;
      for (size_t v = 0; v < n; ++v) {
        const int64_t dy = qy[v] - py[p], dx = qx[v] - px[p];
        if (std::llabs(dy) <= radius && std::llabs(dx) <= radius && dy * dy + dx * dx <= radius * radius)
          all.emplace_back(dy * dy + dx * dx, (int32_t)v);
      }
      std::sort(all.begin(), all.end());
      const size_t want = std::min(all.size(), (size_t)k);
      bool same = nc[p] == (int32_t)want;
      for (size_t j = 0; same && j < (size_t)k; ++j)
        same = j < want ? (cand[p * k + j] == all[j].second && d2[p * k + j] == all[j].first)
                        : (cand[p * k + j] == -1 && d2[p * k + j] == -1);
      CHECK(same, "mm_candidates differs from the scan (n=%zu k=%d radius=%lld fix %zu)", n, k, (long long)radius, p);
    }
  }
}

// map_match.h mm_edge_candidates: on random edge sets (short and long edges, zero-length ones, both
// directions, edges over the span or length limit) under random cell sizes the answer equals a scan
// of all matchable edges sorted by (d2, edge id), and the projection's distance is the true
// point-to-segment distance up to the rounding of fq and Q
static void fuzz_mm_edge_candidates(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 200; ++it) {
    const size_t n = 2 + rng() % 200, E = 1 + rng() % 500;
    const int64_t span = 1 + (int64_t)(rng() % 3000000), ox = (int64_t)(rng() % 4000000000ULL) - 2000000000LL;
    std::vector<int64_t> qy(n), qx(n), lc(E);
    for (size_t i = 0; i < n; ++i) {
      qy[i] = 162000000 + (int64_t)(rng() % span);
      qx[i] = ox + (int64_t)(rng() % span);
    }
    if (rng() % 4 == 0) {   // two far nodes: edges to them exceed the 2^22 span
      qy[0] += 5000000;
      qx[1] -= 4194305;
    }
    std::vector<int32_t> tail(E), head(E);
    for (size_t e = 0; e < E; ++e) {
      tail[e] = (int32_t)(rng() % n);
      head[e] = rng() % 16 == 0 ? tail[e] : (int32_t)(rng() % n);   // a zero-length edge now and then
      if (e && rng() % 8 == 0) {                                     // the other direction of the previous edge
        tail[e] = head[e - 1];
        head[e] = tail[e - 1];
      }
      lc[e] = rng() % 32 == 0 ? -1 : (rng() % 32 == 0 ? rtr::kMmMaxEdgeLc + 1 : (int64_t)(rng() % 5000000));
    }
    rtr::MmEdgeGrid g;
    g.build(qy.data(), qx.data(), n, tail.data(), head.data(), lc.data(), E, 1 + (int64_t)(rng() % (2 * span)));
    CHECK(g.ny <= 2049 && g.nx <= 2049 && g.start.back() == (int32_t)g.items.size(), "MmEdgeGrid: %d x %d cells", g.ny,
          g.nx);
    const size_t P = 1 + rng() % 30;
    const int k = 1 + (int)(rng() % 16);
    const int64_t radius = 1 + (int64_t)(rng() % 100000);
    std::vector<int64_t> py(P), px(P);
    for (size_t p = 0; p < P; ++p) {
      const size_t e = rng() % E;
      const int64_t t = (int64_t)(rng() % 1001);   // a point along edge e, then moved
      py[p] = qy[tail[e]] + (qy[head[e]] - qy[tail[e]]) * t / 1000;
      px[p] = qx[tail[e]] + (qx[head[e]] - qx[tail[e]]) * t / 1000;
      switch (rng() % 4) {
        case 0: break;                                                     // on the edge
        case 1: py[p] += radius; break;                                    // about the radius away
        case 2: py[p] += (int64_t)(rng() % 4000000) - 2000000; px[p] -= 3 * radius; break;
        default: py[p] += (int64_t)(rng() % (2 * radius + 1)) - radius;
                 px[p] += (int64_t)(rng() % (2 * radius + 1)) - radius; break;
      }
    }
    std::vector<int32_t> cand(P * k), fq(P * k), nc(P);
    std::vector<int64_t> d2(P * k);
    rtr::mm_edge_candidates(g, py.data(), px.data(), P, radius, k, cand.data(), d2.data(), fq.data(), nc.data());
    for (size_t p = 0; p < P; ++p) {
      std::vector<std::tuple<int64_t, int32_t, int32_t>> all;
      for (size_t e = 0; e < E; ++e) {
        if (!g.ok[e]) continue;
        const rtr::MmEdge& ed = g.edges[e];
        const int64_t by0 = ed.ay + std::min<int64_t>(ed.wy, 0), by1 = ed.ay + std::max<int64_t>(ed.wy, 0);
        const int64_t bx0 = ed.ax + std::min<int64_t>(ed.wx, 0), bx1 = ed.ax + std::max<int64_t>(ed.wx, 0);
        if (py[p] < by0 - radius || py[p] > by1 + radius || px[p] < bx0 - radius || px[p] > bx1 + radius) continue;
        int64_t dd;
        int32_t q;
        rtr::mm_edge_project(ed, py[p], px[p], &dd, &q);
        CHECK(q >= 0 && q <= rtr::kMmOne, "mm_edge_project: fq %d", q);
        // against the true distance to the segment: fq rounds down by at most span / 2^16 along the
        // edge, Q rounds by half a centimetre per axis
        const long double wy = ed.wy, wx = ed.wx, ey = py[p] - ed.ay, ex = px[p] - ed.ax, l2 = wy * wy + wx * wx;
        long double t = l2 > 0 ? (ey * wy + ex * wx) / l2 : 0;
        t = std::min<long double>(1, std::max<long double>(0, t));
        const long double truth = std::sqrt((ey - t * wy) * (ey - t * wy) + (ex - t * wx) * (ex - t * wx));
        CHECK(std::fabs(std::sqrt((long double)dd) - truth) <= 1.0L + std::sqrt(l2) / 65536.0L,
              "mm_edge_project: %lld cm2 against a true distance of %.3Lf cm", (long long)dd, truth);
        if (dd <= radius * radius) all.emplace_back(dd, (int32_t)e, q);
      }
      std::sort(all.begin(), all.end());
      const size_t want = std::min(all.size(), (size_t)k);
      bool same = nc[p] == (int32_t)want;
      for (size_t j = 0; same && j < (size_t)k; ++j)
        same = j < want ? (d2[p * k + j] == std::get<0>(all[j]) && cand[p * k + j] == std::get<1>(all[j]) &&
                           fq[p * k + j] == std::get<2>(all[j]))
                        : (cand[p * k + j] == -1 && d2[p * k + j] == -1 && fq[p * k + j] == -1);
      CHECK(same, "mm_edge_candidates differs from the scan (E=%zu k=%d radius=%lld fix %zu)", E, k, (long long)radius, p);
    }
  }
}

// map_match.h mm_viterbi: on random costs (infeasible routes, detours beyond the limit, equal
// costs, costs at the parameter maxima) the result is a valid segmentation — choices inside
// n_cand, segment indices rising by at most one, feasible transitions inside a segment, none
// possible from the previous segment's live end across a break — the reported cost is the chosen
// states' own cost, and for short traces it is the minimum over all state sequences
static void fuzz_mm_viterbi(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 50; ++it) {
    const bool tiny = it % 2 == 0;
    const int T = tiny ? 1 + (int)(rng() % 5) : 1 + (int)(rng() % 80);
    const int K = tiny ? 1 + (int)(rng() % 3) : 1 + (int)(rng() % 16);
    const int n = rng() % 8 == 0 ? (int)(rng() % (T + 1)) : T;
    const bool maxed = rng() % 4 == 0;
    const rtr::MmCosts c{maxed ? 10000 : 1 + (int64_t)(rng() % 10000), maxed ? 20000 : 1 + (int64_t)(rng() % 20000),
                         maxed ? 500000 : 1 + (int64_t)(rng() % 500000)};
    const int64_t coarse = rng() % 2 ? 1 : 1 + c.max_detour_cm / 3;   // coarse values make equal costs
    std::vector<int64_t> cd((size_t)T * K), route((size_t)(T > 1 ? T - 1 : 0) * K * K), g(T > 1 ? T - 1 : 0);
    std::vector<int32_t> nc(T);
    for (auto& v : cd) v = maxed ? 10000000000LL : (int64_t)(rng() % 1000) * coarse;
    for (auto& v : nc) v = 1 + (int32_t)(rng() % K);
    for (auto& v : g) v = (int64_t)(rng() % 300000);
    const int infeasible = (int)(rng() % 4);
    for (size_t e = 0; e < route.size(); ++e) {
      const int64_t gt = g[e / ((size_t)K * K)];
      if (infeasible == 3 || (infeasible && rng() % (infeasible == 1 ? 8 : 2) == 0)) route[e] = -1;
      else if (maxed) route[e] = gt + c.max_detour_cm + (rng() % 8 == 0);
      else route[e] = std::max<int64_t>(0, gt + ((int64_t)(rng() % 5) - 2) * coarse * (1 + (int64_t)(rng() % 3)));
    }
    std::vector<int32_t> choice(T), seg(T);
    int32_t nseg = 0;
    const int64_t cost = rtr::mm_viterbi(cd.data(), nc.data(), route.data(), g.data(), T, K, n, c, choice.data(),
                                         seg.data(), &nseg);
    auto trans = [&](int t, int i, int j) -> int64_t {   // -1 infeasible
      const int64_t r = route[((size_t)(t - 1) * K + i) * K + j];
      if (r < 0) return -1;
      const int64_t dev = r > g[t - 1] ? r - g[t - 1] : g[t - 1] - r;
      return dev > c.max_detour_cm ? -1 : 2 * c.sigma_cm * c.sigma_cm * dev;
    };
    int64_t own = 0;
    bool ok = n == 0 ? nseg == 0 : nseg >= 1;
    for (int t = 0; ok && t < T; ++t) {
      if (t >= n) {
        ok = choice[t] == -1 && seg[t] == -1;
        continue;
      }
      ok = choice[t] >= 0 && choice[t] < nc[t] && seg[t] == (t == 0 ? 0 : seg[t - 1]) + (t && seg[t] != seg[t - 1]);
      if (!ok) break;
      own += c.beta_cm * cd[(size_t)t * K + choice[t]];
      if (t && seg[t] == seg[t - 1]) {
        const int64_t tr = trans(t, choice[t - 1], choice[t]);
        ok = tr >= 0;
        own += tr;
      } else if (t) {   // a break: the chosen end of the previous segment reaches nothing here
        for (int j = 0; ok && j < nc[t]; ++j) ok = trans(t, choice[t - 1], j) < 0;
      }
    }
    CHECK(ok && (n == 0 || seg[n - 1] == nseg - 1), "mm_viterbi: not a valid segmentation (T=%d K=%d n=%d)", T, K, n);
    CHECK(!ok || own == cost, "mm_viterbi: cost %lld, the chosen states cost %lld", (long long)cost, (long long)own);
    if (tiny && ok && n > 0) {   // full enumeration, segment by segment
      int64_t total = 0;
      int a = 0, segs = 0;
      while (a < n) {
        // the longest stretch from a that some state sequence survives, and its cheapest sequence
        int reach = a;
        int64_t best_at[6];
        std::vector<int> s(n - a, 0);
        for (int q = 0; q < 6; ++q) best_at[q] = -1;
        for (;;) {
          int64_t sum = 0;
          int len = 0;
          for (int t = a; t < n; ++t) {
            if (s[t - a] >= nc[t]) break;
            if (t > a) {
              const int64_t tr = trans(t, s[t - 1 - a], s[t - a]);
              if (tr < 0) break;
              sum += tr;
            }
            sum += c.beta_cm * cd[(size_t)t * K + s[t - a]];
            ++len;
            if (best_at[len] < 0 || sum < best_at[len]) best_at[len] = sum;
          }
          int d = 0;
          while (d < n - a && ++s[d] == K) s[d++] = 0;
          if (d == n - a) break;
        }
        for (int len = 1; len <= n - a; ++len)
          if (best_at[len] >= 0) reach = a + len;
        total += best_at[reach - a];
        a = reach;
        ++segs;
      }
      CHECK(total == cost && segs == nseg, "mm_viterbi: cost %lld in %d segments, enumeration %lld in %d",
            (long long)cost, nseg, (long long)total, segs);
    }
  }
}

// avoid.h: the mask is symmetric in edge direction, an edge with an endpoint on a polygon vertex is
// closed, a far-away set closes nothing; damaged blobs are refused (never read out of bounds)
static void fuzz_avoid_mask(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 20; ++it) {
    const int N = 2 + (int)(rng() % 40);
    std::vector<int32_t> qx(N), qy(N);
    for (int i = 0; i < N; ++i) {
      qx[i] = 121000000 + (int32_t)(rng() % 13) - 6;
      qy[i] = 14500000 + (int32_t)(rng() % 13) - 6;
    }
    // CSR with both directions of every undirected edge (and a self loop now and then)
    std::vector<std::vector<int32_t>> adj(N);
    const int und = 1 + (int)(rng() % (2 * N));
    for (int k = 0; k < und; ++k) {
      const int u = (int)(rng() % N), v = (int)(rng() % N);
      adj[u].push_back(v);
      if (u != v) adj[v].push_back(u);
    }
    std::vector<int32_t> indptr(N + 1, 0), indices;
    for (int u = 0; u < N; ++u) {
      for (int32_t v : adj[u]) indices.push_back(v);
      indptr[u + 1] = (int32_t)indices.size();
    }
    const int P = 1 + (int)(rng() % 3);
    std::vector<int32_t> nring(P), nvert, xy;
    for (int p = 0; p < P; ++p) {
      nring[p] = 1 + (int32_t)(rng() % 2);
      for (int r = 0; r < nring[p]; ++r) {
        const int nv = 3 + (int)(rng() % 4);
        nvert.push_back(nv);
        for (int i = 0; i < nv; ++i) {
          xy.push_back(121000000 + (int32_t)(rng() % 13) - 6);
          xy.push_back(14500000 + (int32_t)(rng() % 13) - 6);
        }
      }
    }
    std::vector<int32_t> blob{P, (int32_t)nvert.size(), (int32_t)(xy.size() / 2)};
    blob.insert(blob.end(), nring.begin(), nring.end());
    blob.insert(blob.end(), nvert.begin(), nvert.end());
    blob.insert(blob.end(), xy.begin(), xy.end());
    std::vector<uint8_t> mask(indices.size(), 2);
    rtr::avoid_mask(N, indptr.data(), indices.data(), qx.data(), qy.data(), blob.data(), (int64_t)blob.size(), mask.data());
    for (int u = 0; u < N; ++u)
      for (int32_t e = indptr[u]; e < indptr[u + 1]; ++e) {
        const int32_t v = indices[e];
        CHECK(mask[e] <= 1, "avoid_mask: edge %d not written", e);
        for (int32_t f = indptr[v]; f < indptr[v + 1]; ++f)
          if (indices[f] == u) CHECK(mask[f] == mask[e], "avoid_mask: %d->%d and back differ", u, v);
        bool on_vertex = false;
        for (size_t i = 0; i + 1 < xy.size(); i += 2)
          on_vertex |= (xy[i] == qx[u] && xy[i + 1] == qy[u]) || (xy[i] == qx[v] && xy[i + 1] == qy[v]);
        if (on_vertex) CHECK(mask[e] == 1, "avoid_mask: edge %d touches a vertex and is open", e);
      }
    // the same set moved away closes nothing
    std::vector<int32_t> far(blob);
    for (size_t i = 3 + (size_t)P + nvert.size(); i < far.size(); i += 2) far[i] += 1000;
    rtr::avoid_mask(N, indptr.data(), indices.data(), qx.data(), qy.data(), far.data(), (int64_t)far.size(), mask.data());
    for (size_t e = 0; e < mask.size(); ++e) CHECK(mask[e] == 0, "avoid_mask: far set closes edge %zu", e);
    // damage: one word changed, or cut short — parsed within bounds or refused
    std::vector<int32_t> bad(blob);
    if (rng() % 2) bad[rng() % (3 + (size_t)P + nvert.size())] = (int32_t)(rng() % 4096) - 8;
    else bad.resize(rng() % bad.size());
    try {
      rtr::avoid_mask(N, indptr.data(), indices.data(), qx.data(), qy.data(), bad.data(), (int64_t)bad.size(), mask.data());
    } catch (const std::invalid_argument&) {
    }
  }
}

// alternatives.h: via nodes stay in range, unique, within the detour band, and reproducible; the
// argmin treats non-finite scores as +inf
static void fuzz_alternatives(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 50; ++it) {
    const int N = 1 + (int)(rng() % 2000);
    std::vector<double> lat(N), lon(N);
    for (int i = 0; i < N; ++i) {
      lat[i] = 14.5 + (double)(rng() % 100000) * 1e-6 * (rng() % 5 == 0 ? 0.0 : 1.0);
      lon[i] = 121.0 + (double)(rng() % 100000) * 1e-6;
    }
    const int s = (int)(rng() % (N + 4)) - 2, t = (int)(rng() % (N + 4)) - 2, n = (int)(rng() % 12) - 1;
    const double stretch = 1.0 + (double)(rng() % 1000) / 1000.0;
    const std::vector<int> v = ralt::via_nodes(lat.data(), lon.data(), N, s, t, n, stretch);
    CHECK((int)v.size() <= std::max(n, 0), "via_nodes: %zu > n %d", v.size(), n);
    std::vector<int> seen(v);
    std::sort(seen.begin(), seen.end());
    CHECK(std::unique(seen.begin(), seen.end()) == seen.end(), "via_nodes: duplicate candidate");
    for (int w : v) {
      CHECK(w >= 0 && w < N, "via_nodes: %d out of [0, %d)", w, N);
      if (w < 0 || w >= N) break;
      const double d_st = rtr::haversine_m(lat[s], lon[s], lat[t], lon[t]);
      const double det = rtr::haversine_m(lat[s], lon[s], lat[w], lon[w]) + rtr::haversine_m(lat[w], lon[w], lat[t], lon[t]);
      CHECK(det <= stretch * d_st && det >= 1.03 * d_st, "via_nodes: detour %.3f outside band of %.3f", det, d_st);
    }
    CHECK(v == ralt::via_nodes(lat.data(), lon.data(), N, s, t, n, stretch), "via_nodes: not reproducible");
    std::vector<double> sc(rng() % 9);
    for (double& x : sc) {
      const int k = (int)(rng() % 4);
      x = k == 0 ? NAN : k == 1 ? INFINITY : (double)(rng() % 1000);
    }
    const int b = ralt::argmin_score(sc);
    CHECK(sc.empty() ? b == -1 : (b >= 0 && b < (int)sc.size()), "argmin_score: %d of %zu", b, sc.size());
  }
}

// A database file with the store's schema (routest_amd/store/store.py SCHEMA) in the temporary
// directory, removed with its WAL files when the object goes.
struct TempDb {
  std::string path;
  bool ok = false;
  explicit TempDb(rtsql::Api& sql, const char* tag) {
    const char* tmp = std::getenv("TMPDIR");
    path = std::string(tmp && *tmp ? tmp : "/tmp") + "/rt_selftest_" + tag + "_" + std::to_string((long)getpid()) + ".db";
    remove_files();
    void* db = nullptr;
    if (sql.open_v2(path.c_str(), &db, rtsql::OPEN_READWRITE | rtsql::OPEN_CREATE, nullptr) != rtsql::OK) {
      if (db) sql.close(db);
      return;
    }
    const char* ddl =
        "PRAGMA journal_mode=WAL;"
        "CREATE TABLE locations (id TEXT PRIMARY KEY, name TEXT NOT NULL, latitude REAL NOT NULL, longitude REAL NOT NULL, created_at TEXT);"
        "CREATE TABLE route_requests (id TEXT PRIMARY KEY, origin_id TEXT, stops TEXT NOT NULL, request_time TEXT NOT NULL,"
        " status TEXT NOT NULL DEFAULT 'pending', engine TEXT, vehicle_id TEXT, driver_age REAL);"
        "CREATE TABLE route_results (id TEXT PRIMARY KEY, request_id TEXT NOT NULL REFERENCES route_requests(id) ON DELETE CASCADE,"
        " optimized_order TEXT, total_distance REAL, total_duration REAL, legs TEXT, geometry TEXT, eta_minutes_ml REAL,"
        " eta_completion_time_ml TEXT, created_at TEXT);";
    ok = sql.exec(db, ddl, nullptr, nullptr, nullptr) == rtsql::OK;
    sql.close(db);
  }
  void remove_files() {
    for (const char* ext : {"", "-wal", "-shm"}) std::remove((path + ext).c_str());
  }
  ~TempDb() { remove_files(); }
};

// One row for the writer (route_store.h): a parsed request and the pieces of its two rows.
struct SelfRow {
  rtj::Value root;
  rts::StoreRow row;
};

static std::unique_ptr<SelfRow> make_row(std::mt19937_64& rng) {
  auto r = std::make_unique<SelfRow>();
  std::string body = "{\"destination_points\":[{\"lat\":14.5,\"lon\":121.0}],\"use_ml_eta\":";
  body += rng() % 2 ? "true" : "false";
  if (rng() % 4) body += ",\"meta\":{\"origin_id\":" + (rng() % 2 ? std::string("null") : std::to_string(rng() % 100)) +
                         ",\"destination_ids\":[1,2]}";
  if (rng() % 3) body += ",\"driver_details\":{\"driver_name\":\"d\",\"driver_age\":" + std::to_string(rng() % 90) + "}";
  body += "}";
  r->root = rtj::Parser(body.data(), body.size()).parse();
  r->row.root = &r->root;
  r->row.asmb.ok = true;
  r->row.asmb.order = "[0]";
  r->row.asmb.segments = "[]";
  r->row.asmb.coords = "[[121.0,14.5],[121.01,14.51]]";
  r->row.asmb.dist = (double)(rng() % 100000) / 7.0;
  r->row.asmb.dur = (double)(rng() % 100000) / 3.0;
  return r;
}

// history_db.h over a database the route service's writer (route_store.h RouteStore) filled: rows
// with fuzzed texts (any bytes, non-JSON stops, junk records), committed in groups on both sides of
// the multi-row thresholds, then list / detail / delete / locations with fuzzed limit strings and
// ids — every reply a valid status, nothing read out of bounds.  Skipped when libsqlite3 cannot be
// loaded.
static void fuzz_history(std::mt19937_64& rng, int iters) {
  rtsql::Api sql;
  std::string err;
  if (!sql.load(err)) {
    std::printf("fuzz_history: skipped (%s)\n", err.c_str());
    return;
  }
  TempDb tdb(sql, "hist");
  CHECK(tdb.ok, "history schema");
  if (!tdb.ok) return;
  auto junk = [&](size_t maxlen) {
    static const char* frags[] = {"{\"destination_ids\":[1,2],\"destination_points\":[[14.5,121.0]]}", "[0,2,1]", "null",
                                  "{\"type\":\"LineString\",\"coordinates\":[]}", "2026-10-17T00:00:00", "\"\\u00e9\"", "{"};
    std::string t = rng() % 2 ? frags[rng() % 7] : "";
    const size_t n = rng() % maxlen;
    for (size_t i = 0; i < n; ++i) t += (char)(rng() & 0xFF);
    return t;
  };
  std::vector<std::string> ids;
  {
    rts::RouteStore store;
    CHECK(store.open(tdb.path) && store.opened(), "store open");
    std::vector<std::unique_ptr<SelfRow>> rows;
    size_t refused = 0;
    for (size_t n : {1u, 3u, 4u, 33u, 19u}) {
      std::vector<rts::StoreRow*> g;
      for (size_t i = 0; i < n; ++i) {
        rows.push_back(make_row(rng));
        rts::StoreRow& r = rows.back()->row;
        CHECK(rts::RouteStore::prepare(r), "prepare");
        // what the history readers parse, fuzzed after prepare() built it
        r.stops = junk(40);
        r.asmb.order = junk(16);
        if (rng() % 3 == 0) r.rec = junk(64) + "x"; else { r.asmb.segments = junk(64); r.geom = junk(64); }
        if (rng() % 2) { r.eta_min = (float)(rng() % 1000) / 9.0f; r.eta_iso = junk(24) + "Z"; }
        if (rng() % 16 == 0) { r.ok = false; ++refused; }
        g.push_back(&r);
      }
      store.commit_group(g);
      for (rts::StoreRow* r : g) {
        CHECK(r->request_id.empty() == !r->ok, "commit_group: a row's id");
        if (!r->request_id.empty()) ids.push_back(r->request_id);
      }
    }
    CHECK(ids.size() + refused == rows.size() && store.rows_persisted() == (long long)ids.size(), "rows persisted");
  }
  void* db = nullptr;
  CHECK(sql.open_v2(tdb.path.c_str(), &db, rtsql::OPEN_READWRITE, nullptr) == rtsql::OK, "history db");
  void* ins_loc = nullptr;
  sql.prepare_v2(db, "INSERT INTO locations(id,name,latitude,longitude,created_at) VALUES(?,?,?,?,?)", -1, &ins_loc, nullptr);
  for (int i = 0; i < 10; ++i) {
    const std::string lid = "loc-" + std::to_string(i), name = junk(12);
    sql.reset(ins_loc);
    sql.clear_bindings(ins_loc);
    sql.bind_text(ins_loc, 1, lid.data(), (int)lid.size(), rtsql::TRANSIENT);
    sql.bind_text(ins_loc, 2, name.data(), (int)name.size(), rtsql::TRANSIENT);
    sql.bind_double(ins_loc, 3, 14.5);
    sql.bind_double(ins_loc, 4, 121.0);
    sql.bind_null(ins_loc, 5);
    CHECK(sql.step(ins_loc) == rtsql::DONE, "insert location");
  }
  sql.finalize(ins_loc);
  sql.close(db);
  rth::HistoryDb h;
  CHECK(h.open(tdb.path, err), "history open: %s", err.c_str());
  auto valid = [](const rth::Reply& r) { return r.fallback || (r.status >= 200 && r.status < 600); };
  static const char* LIMITS[] = {"", "0", "-2", "3", "20", "100000", "abc", "2.5", "1_0", " 7", "99999999999999999999999", "+4"};
  for (int it = 0; it < iters / 100; ++it) {
    switch (rng() % 5) {
      case 0: {
        const bool absent = rng() % 6 == 0;
        std::string lim = LIMITS[rng() % (sizeof LIMITS / sizeof *LIMITS)];
        if (rng() % 4 == 0) lim = junk(10);
        CHECK(valid(h.history(absent ? nullptr : lim.c_str())), "history(%s)", lim.c_str());
        break;
      }
      case 1: CHECK(valid(h.detail(rng() % 2 ? ids[rng() % ids.size()] : junk(50))), "detail"); break;
      case 2: CHECK(valid(h.del(rng() % 3 ? ids[rng() % ids.size()] : junk(50))), "delete"); break;
      default: CHECK(valid(h.locations()), "locations"); break;
    }
  }
  h.close();
}

// The writer commits groups (its checkpoint thread behind it) while a HistoryDb reads the same
// file on another thread: what the route service's persistence thread and the front end's history
// reads do to each other, for TSan / ASan.
static void store_while_reading() {
  rtsql::Api sql;
  std::string err;
  if (!sql.load(err)) return;
  TempDb tdb(sql, "rw");
  CHECK(tdb.ok, "store_while_reading schema");
  if (!tdb.ok) return;
  std::mutex mu;
  std::vector<std::string> ids;
  std::atomic<bool> writing{true};
  std::thread reader([&] {
    rth::HistoryDb h;
    std::string e;
    if (!h.open(tdb.path, e)) return;
    size_t seen = 0;
    while (writing.load() || seen == 0) {
      std::string id;
      {
        std::lock_guard<std::mutex> lk(mu);
        if (!ids.empty()) id = ids[seen++ % ids.size()];
      }
      const rth::Reply l = h.history("20");
      CHECK(l.fallback || l.status == 200, "history while writing: %d", l.status);
      if (!id.empty()) {
        const rth::Reply d = h.detail(id);      // committed before its id was published
        CHECK(d.fallback || d.status == 200, "detail while writing: %d", d.status);
      }
      if (!writing.load() && id.empty()) break;
    }
    h.close();
  });
  {
    std::mt19937_64 rng(99);
    rts::RouteStore store;
    CHECK(store.open(tdb.path), "store open");
    for (int g = 0; g < 40; ++g) {
      std::vector<std::unique_ptr<SelfRow>> rows;
      std::vector<rts::StoreRow*> grp;
      for (int i = 0; i < 1 + g % 8; ++i) {
        rows.push_back(make_row(rng));
        rts::RouteStore::prepare(rows.back()->row);
        grp.push_back(&rows.back()->row);
      }
      store.commit_group(grp);
      std::lock_guard<std::mutex> lk(mu);
      for (rts::StoreRow* r : grp) {
        CHECK(!r->request_id.empty(), "commit while reading");
        if (!r->request_id.empty()) ids.push_back(r->request_id);
      }
    }
  }
  writing.store(false);
  reader.join();
}

// The batched /predict path splits a big array with split_top_array and packs / formats items on
// parallel_chunks threads (rt.cpp); replay that shape here so TSan sees the real sharing pattern.
static void threaded_pack_format(int n_items) {
  std::string body = "[";
  for (int i = 0; i < n_items; ++i) {
    if (i) body += ',';
    body += "{\"summary\":{\"distance\":" + std::to_string(1000 + i) +
            "},\"pickup_time\":\"2025-08-25T08:30:00+02:00\",\"traffic\":\"High\"}";
  }
  body += "]";
  std::vector<std::pair<size_t, size_t>> spans;
  CHECK(split_top_array(body.data(), body.size(), spans) && (int)spans.size() == n_items, "split");
  const Stamp now{1756110600, 0, false, 0, 0};
  std::vector<EtaRecord> recs(spans.size());
  std::vector<Stamp> st(spans.size());
  std::vector<std::string> errs(spans.size());
  parallel_chunks(spans.size(), 64, 8, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      rtj::Value v = rtj::Parser(body.data() + spans[i].first, spans[i].second - spans[i].first).parse();
      errs[i] = pack_item(v, now, recs[i], st[i]);
    }
  });
  std::vector<std::string> parts(8);
  const size_t per = (spans.size() + 7) / 8;
  parallel_chunks(8, 1, 8, [&](size_t klo, size_t khi) {
    for (size_t k = klo; k < khi; ++k)
      for (size_t i = k * per; i < std::min(spans.size(), (k + 1) * per); ++i)
        format_one(parts[k], 12.5 + (double)i, st[i].secs, st[i].us, st[i].has_tz, st[i].tz_sec, errs[i]);
  });
  size_t ok = 0;
  for (auto& e : errs) ok += e.empty();
  CHECK(ok == spans.size(), "threaded pack errors");
  CHECK(recs[n_items - 1].distance_m == (float)(1000 + n_items - 1), "threaded pack record");
}

// route_core.h pd_trips (instances as in fuzz_tw, half as many, with random pickup -> delivery pairs):
// either some stop is reported infeasible alone (a pair with both indices) or every stop is routed
// exactly once, a pair in one trip with its pickup first, every trip re-simulates as feasible in time
// and in its integer load profile against the fixed-point capacity, and both float walks hold
static void fuzz_pd(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 200; ++it) {
    const int n1 = 1 + (int)(rng() % 34);
    std::vector<double> d((size_t)n1 * n1, 0.0), t((size_t)n1 * n1, 0.0), dem(n1, 0.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) {
          d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
          t[(size_t)a * n1 + b] = 10.0 + (double)(rng() % 100000) / 53.0;
        }
    if (rng() % 3 == 0 && n1 > 4) {
      const double bad[6] = {NAN, INFINITY, -5.0, 2147483.647, 3e9, 1e300};
      for (int x = 0; x < 6; ++x) {
        std::vector<double>& m = rng() % 2 ? d : t;
        const int a = rng() % 8 == 0 ? 0 : 1 + (int)(rng() % (n1 - 1)), b = 1 + (int)(rng() % (n1 - 1));
        if (a != b) m[(size_t)a * n1 + b] = bad[rng() % 6];
      }
    }
    std::vector<long long> open(n1, 0), close(n1, rtr::kExchangeUnbounded), sv(n1, 0);
    for (int s = 1; s < n1; ++s) {
      dem[s] = (double)(1 + rng() % 3);
      if (rng() % 10 < 5) {
        open[s] = (long long)(rng() % 20000000);
        close[s] = open[s] + (long long)(rng() % 3 == 0 ? 0 : rng() % 8000000);
        if (rng() % 4 == 0) open[s] = 0;
      }
      if (rng() % 2) sv[s] = (long long)(rng() % 600000);
    }
    // about half of the stops in pairs: consecutive entries of a shuffled order
    std::vector<int> order, pf(n1, -1);
    for (int s = 1; s < n1; ++s) order.push_back(s);
    for (size_t x = order.size(); x > 1; --x) std::swap(order[x - 1], order[rng() % x]);
    for (size_t x = 0; x < order.size() / 4; ++x) pf[order[2 * x + 1]] = order[2 * x];
    const bool odd_demand = rng() % 16 == 0 && n1 > 1;  // a negative demand passes the float test alone
    if (odd_demand) dem[1 + rng() % (n1 - 1)] = rng() % 2 ? NAN : -1.0;
    const bool free_run = rng() % 3 == 0;
    const double cap = free_run ? 9e12 : (rng() % 16 == 0 ? NAN : (double)(3 + rng() % 30));
    const double maxd = free_run ? 9e12 : (rng() % 16 == 0 ? -1.0 : 60000.0 + (double)(rng() % 400000));
    std::vector<int> kind, mate;
    CHECK(rtr::pd_kinds(pf, n1, kind, mate), "pd_kinds refused well-formed pairs");
    {  // malformed: a chain and a shared pickup
      std::vector<int> k2, m2, bad_pf = pf;
      if (n1 > 3) {
        bad_pf.assign(n1, -1);
        bad_pf[1] = 2;
        bad_pf[2] = 3;
        CHECK(!rtr::pd_kinds(bad_pf, n1, k2, m2), "pd_kinds took a chain");
        bad_pf[2] = -1;
        bad_pf[3] = 2;
        CHECK(!rtr::pd_kinds(bad_pf, n1, k2, m2), "pd_kinds took a shared pickup");
      }
    }
    std::vector<std::vector<int>> trips;
    std::vector<std::vector<long long>> arr, sta;
    std::vector<int> bad;
    rtr::TwStats st;
    if (!rtr::pd_trips(d, t, n1, dem, cap, maxd, open, close, sv, kind, mate, trips, arr, sta, bad, st)) {
      CHECK(!bad.empty() && trips.empty(), "pd_trips failed without naming a stop");
      for (size_t x = 0; x < bad.size(); ++x) {
        CHECK(bad[x] >= 0 && bad[x] < n1 - 1 && (x == 0 || bad[x] > bad[x - 1]), "pd_trips infeasible index %d", bad[x]);
        const int s = bad[x] + 1;
        if (s >= 1 && s < n1 && kind[s] != rtr::kPdPlain)
          CHECK(std::find(bad.begin(), bad.end(), mate[s] - 1) != bad.end(), "pd_trips reported half a pair (%d)", s);
      }
      continue;
    }
    long long cap_q = -1;
    if (!rtr::exchange_limit(cap, cap_q)) cap_q = -1;
    std::vector<int> seen(n1, 0), trip_of(n1, -1), pos_of(n1, -1);
    long long len = 0, waiting = 0, units = 0;
    CHECK(trips.size() == arr.size() && trips.size() == sta.size() && st.trips == (long long)trips.size(), "pd_trips trip counts");
    for (size_t k = 0; k < trips.size(); ++k) {
      const std::vector<int>& tr = trips[k];
      CHECK(tr.size() >= 3 && tr.front() == 0 && tr.back() == 0, "pd_trips broke a trip's ends");
      CHECK(arr[k].size() + 2 == tr.size() && sta[k].size() + 2 == tr.size(), "pd_trips schedule length");
      long long clock = 0, load = 0, top = 0;
      bool ok = true;
      for (size_t p = 1; p + 1 < tr.size(); ++p)
        if (tr[p] >= 1 && tr[p] < n1 && kind[tr[p]] == rtr::kPdPlain) load += rtr::improve_q(dem[tr[p]]);
      top = load;
      for (size_t p = 0; p + 1 < tr.size(); ++p) {
        const int a = tr[p], b = tr[p + 1];
        if (a < 0 || a >= n1 || b < 0 || b >= n1) { ok = false; break; }
        const long long q = rtr::tw_q(d[(size_t)a * n1 + b]), qt = rtr::tw_q(t[(size_t)a * n1 + b]);
        ok = ok && q < rtr::kImproveBig && qt < rtr::kImproveBig;
        len += q;
        if (b == 0) break;
        ++seen[b];
        trip_of[b] = (int)k;
        pos_of[b] = (int)p + 1;
        units += kind[b] != rtr::kPdDelivery;
        const long long ar = clock + qt, s0 = std::max(ar, open[b]);
        ok = ok && s0 <= close[b] && p < arr[k].size() && arr[k][p] == ar && sta[k][p] == s0;
        waiting += s0 - ar;
        clock = s0 + sv[b];
        load += kind[b] == rtr::kPdPickup ? rtr::improve_q(dem[mate[b]]) : -rtr::improve_q(dem[b]);
        top = std::max(top, load);
      }
      CHECK(ok, "pd_trips built a trip that does not re-simulate as feasible");
      // a seed is admitted by the float test alone; every longer trip passed the integer profile
      if (!odd_demand && (tr.size() > 4 || (tr.size() == 4 && kind[tr[1]] == rtr::kPdPlain)))
        CHECK(top <= cap_q, "pd_trips overloaded a trip: %lld > %lld", top, cap_q);
      double s = 0.0;
      const int kk = (int)tr.size() - 2;
      for (int p = 0; p < kk; ++p) s += d[(size_t)tr[p] * n1 + tr[p + 1]];
      CHECK(s + d[(size_t)tr[kk] * n1] <= maxd && rtr::pd_load_feasible(dem, kind, mate, tr, cap),
            "pd_trips kept a trip that fails the float walks");
    }
    bool once = true, paired = true;
    for (int s = 1; s < n1; ++s) {
      once = once && seen[s] == 1;
      if (kind[s] == rtr::kPdPickup)
        paired = paired && trip_of[s] == trip_of[mate[s]] && pos_of[s] < pos_of[mate[s]];
    }
    CHECK(once, "pd_trips lost or repeated a stop");
    CHECK(paired, "pd_trips split a pair or delivered before the pickup");
    CHECK(len == st.len_q && waiting == st.waiting_q, "pd_trips statistics: len %lld / %lld, waiting %lld / %lld", st.len_q, len,
          st.waiting_q, waiting);
    CHECK(st.insertions + st.trips == units, "pd_trips: %lld insertions + %lld trips != %lld units", st.insertions, st.trips,
          units);
  }
}

// route_core.h pd_improve_trips on pd_trips' output (instances as in fuzz_pd, half as many).  After
// the search every stop is present exactly once, every pair sits in one trip with its pickup first
// and every trip re-simulates as feasible (legs and time always; load and length for the trips a
// move touched: a seed is admitted by the float tests alone).  The applied sequence is replayed from
// pd_trips' trips by the definition: each move's trips re-simulate as integer-feasible, its gain is
// positive, and the replay ends in the trips and the length that came out.
static void fuzz_pd_improve(std::mt19937_64& rng, int iters) {
  for (int it = 0; it < iters / 400; ++it) {
    const int n1 = 1 + (int)(rng() % 34);
    std::vector<double> d((size_t)n1 * n1, 0.0), t((size_t)n1 * n1, 0.0), dem(n1, 0.0);
    for (int a = 0; a < n1; ++a)
      for (int b = 0; b < n1; ++b)
        if (a != b) {
          d[(size_t)a * n1 + b] = 100.0 + (double)(rng() % 1000000) / 37.0;
          t[(size_t)a * n1 + b] = 10.0 + (double)(rng() % 100000) / 53.0;
        }
    if (rng() % 3 == 0 && n1 > 4) {
      const double bad[6] = {NAN, INFINITY, -5.0, 2147483.647, 3e9, 1e300};
      for (int x = 0; x < 6; ++x) {
        std::vector<double>& m = rng() % 2 ? d : t;
        const int a = rng() % 8 == 0 ? 0 : 1 + (int)(rng() % (n1 - 1)), b = 1 + (int)(rng() % (n1 - 1));
        if (a != b) m[(size_t)a * n1 + b] = bad[rng() % 6];
      }
    }
    std::vector<long long> open(n1, 0), close(n1, rtr::kExchangeUnbounded), sv(n1, 0);
    for (int s = 1; s < n1; ++s) {
      dem[s] = (double)(1 + rng() % 3);
      if (rng() % 10 < 4) {
        open[s] = (long long)(rng() % 20000000);
        close[s] = open[s] + (long long)(rng() % 3 == 0 ? 0 : rng() % 8000000);
        if (rng() % 4 == 0) open[s] = 0;
      }
      if (rng() % 2) sv[s] = (long long)(rng() % 600000);
    }
    std::vector<int> order, pf(n1, -1);
    for (int s = 1; s < n1; ++s) order.push_back(s);
    for (size_t x = order.size(); x > 1; --x) std::swap(order[x - 1], order[rng() % x]);
    for (size_t x = 0; x < order.size() / 4; ++x) pf[order[2 * x + 1]] = order[2 * x];
    const bool free_run = rng() % 3 == 0;
    const double cap = free_run ? 9e12 : (rng() % 16 == 0 ? NAN : (double)(3 + rng() % 30));
    const double maxd = free_run ? 9e12 : (rng() % 16 == 0 ? -1.0 : 60000.0 + (double)(rng() % 400000));
    std::vector<int> kind, mate;
    CHECK(rtr::pd_kinds(pf, n1, kind, mate), "pd_kinds refused well-formed pairs");
    std::vector<std::vector<int>> trips;
    std::vector<std::vector<long long>> arr, sta;
    std::vector<int> bad;
    rtr::TwStats st0;
    if (!rtr::pd_trips(d, t, n1, dem, cap, maxd, open, close, sv, kind, mate, trips, arr, sta, bad, st0)) continue;
    const std::vector<std::vector<int>> given = trips;
    long long cap_q = -1, max_q = -1;
    if (!rtr::exchange_limit(cap, cap_q)) cap_q = -1;
    if (!rtr::exchange_limit(maxd, max_q)) max_q = -1;
    // the definition's tests of one trip, independent of route_core.h's walk
    auto simulate = [&](const std::vector<int>& tr, long long& len, bool& timed, bool& within) {
      len = 0;
      timed = within = true;
      if (tr.size() < 3) return;
      long long clock = 0, load = 0;
      for (size_t p = 1; p + 1 < tr.size(); ++p)
        if (kind[tr[p]] == rtr::kPdPlain) load += rtr::improve_q(dem[tr[p]]);
      within = load <= cap_q;
      for (size_t p = 0; p + 1 < tr.size(); ++p) {
        const int a = tr[p], b = tr[p + 1];
        const long long q = rtr::tw_q(d[(size_t)a * n1 + b]), qt = rtr::tw_q(t[(size_t)a * n1 + b]);
        timed = timed && q < rtr::kImproveBig && qt < rtr::kImproveBig;
        len += q;
        if (b == 0) break;
        const long long s0 = std::max(clock + qt, open[b]);
        timed = timed && s0 <= close[b];
        clock = s0 + sv[b];
        load += kind[b] == rtr::kPdPickup ? rtr::improve_q(dem[mate[b]]) : -rtr::improve_q(dem[b]);
        within = within && load <= cap_q;
      }
      within = within && len <= max_q;
    };
    std::vector<rtr::PdMove> applied;
    const rtr::PdImproveStats st =
        rtr::pd_improve_trips(d, t, n1, dem, cap, maxd, open, close, sv, kind, mate, trips, arr, sta, &applied);
    CHECK(st.moves == (long long)applied.size() && st.moves <= 4LL * (n1 - 1), "pd_improve: %lld moves, %zu applied", st.moves,
          applied.size());
    CHECK(st.trips_before == (long long)given.size() && st.trips_after == (long long)trips.size(), "pd_improve trip counts");
    // the replay
    std::vector<std::vector<int>> cur = given;
    std::vector<char> touched(given.size(), 0);
    long long pairs = 0, total = 0;
    bool replayed = true;
    for (const rtr::PdMove& mv : applied) {
      if (mv.A < 0 || mv.A >= (int)cur.size() || mv.B < 0 || mv.B >= (int)cur.size() || mv.x < 1 ||
          mv.x + 1 >= (int)cur[mv.A].size() || (mv.type == 0) == (mv.A == mv.B)) {
        replayed = false;
        break;
      }
      const int u = cur[mv.A][mv.x], v = kind[u] == rtr::kPdPickup ? mate[u] : -1;
      if (kind[u] == rtr::kPdDelivery) { replayed = false; break; }
      pairs += v >= 0;
      long long before = 0, after = 0, len;
      bool timed, within;
      simulate(cur[mv.A], len, timed, within);
      before += len;
      if (mv.type == 0) {
        simulate(cur[mv.B], len, timed, within);
        before += len;
      }
      std::vector<int> rest;
      for (size_t p = 0; p < cur[mv.A].size(); ++p)
        if (p == 0 || p + 1 == cur[mv.A].size() || (cur[mv.A][p] != u && cur[mv.A][p] != v)) rest.push_back(cur[mv.A][p]);
      std::vector<int> into = mv.type == 0 ? cur[mv.B] : rest;
      const int k = (int)into.size() - 2;
      if (k < 1 || mv.i < 0 || mv.i > mv.j || mv.j > k || (v < 0 && mv.i != mv.j)) { replayed = false; break; }
      if (v >= 0) into.insert(into.begin() + mv.j + 1, v);
      into.insert(into.begin() + mv.i + 1, u);
      if (mv.type == 0) cur[mv.A] = rest;
      cur[mv.B] = into;
      touched[mv.A] = touched[mv.B] = 1;
      for (int x : {mv.A, mv.B}) {
        simulate(cur[x], len, timed, within);
        CHECK(timed && within, "pd_improve applied a move whose trip %d is not integer-feasible", x);
        if (x == mv.A || mv.type == 0) after += len;
        if (mv.type == 1) break;
      }
      CHECK(before - after > 0, "pd_improve applied a move of gain %lld", before - after);
    }
    CHECK(replayed, "pd_improve reported a move outside the definition's ranges");
    CHECK(pairs == st.pair_moves, "pd_improve pair moves: %lld / %lld", st.pair_moves, pairs);
    std::vector<std::vector<int>> kept;
    std::vector<char> kept_touched;
    for (size_t x = 0; x < cur.size(); ++x)
      if (cur[x].size() > 2) {
        kept.push_back(cur[x]);
        kept_touched.push_back(touched[x]);
      }
    CHECK(replayed && kept == trips, "pd_improve: the replay of the applied moves ends in other trips");
    // the invariants of what came out
    std::vector<int> seen(n1, 0), trip_of(n1, -1), pos_of(n1, -1);
    long long waiting = 0;
    CHECK(trips.size() == arr.size() && trips.size() == sta.size(), "pd_improve schedule count");
    for (size_t k = 0; k < trips.size(); ++k) {
      const std::vector<int>& tr = trips[k];
      CHECK(tr.size() >= 3 && tr.front() == 0 && tr.back() == 0, "pd_improve broke a trip's ends");
      CHECK(arr[k].size() + 2 == tr.size() && sta[k].size() + 2 == tr.size(), "pd_improve schedule length");
      long long len, clock = 0;
      bool timed, within;
      simulate(tr, len, timed, within);
      total += len;
      CHECK(timed, "pd_improve left a trip that does not re-simulate as feasible");
      if (kept == trips && kept_touched[k]) CHECK(within, "pd_improve left a touched trip over its load or length");
      for (size_t p = 1; p + 1 < tr.size() && p <= arr[k].size(); ++p) {
        const int b = tr[p];
        if (b < 1 || b >= n1) break;
        ++seen[b];
        trip_of[b] = (int)k;
        pos_of[b] = (int)p;
        const long long ar = clock + rtr::tw_q(t[(size_t)tr[p - 1] * n1 + b]), s0 = std::max(ar, open[b]);
        CHECK(arr[k][p - 1] == ar && sta[k][p - 1] == s0, "pd_improve schedule entry");
        waiting += s0 - ar;
        clock = s0 + sv[b];
      }
      double s = 0.0;
      const int kk = (int)tr.size() - 2;
      for (int p = 0; p < kk; ++p) s += d[(size_t)tr[p] * n1 + tr[p + 1]];
      CHECK(s + d[(size_t)tr[kk] * n1] <= maxd && rtr::pd_load_feasible(dem, kind, mate, tr, cap),
            "pd_improve kept a trip that fails the float walks");
    }
    bool once = true, paired = true;
    for (int s = 1; s < n1; ++s) {
      once = once && seen[s] == 1;
      if (kind[s] == rtr::kPdPickup) paired = paired && trip_of[s] == trip_of[mate[s]] && pos_of[s] < pos_of[mate[s]];
    }
    CHECK(once, "pd_improve lost or repeated a stop");
    CHECK(paired, "pd_improve split a pair or delivered before the pickup");
    CHECK(total == st.len_after_q && waiting == st.waiting_q && st.len_after_q <= st.len_before_q &&
              st.len_before_q == st0.len_q,
          "pd_improve statistics: len %lld -> %lld / %lld, waiting %lld / %lld", st.len_before_q, st.len_after_q, total,
          st.waiting_q, waiting);
  }
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1234);
  fuzz_json(rng, iters);
  fuzz_iso(rng, iters);
  fuzz_float(rng, iters);
  fuzz_route(rng, iters);
  fuzz_coord_cache(rng, iters);
  fuzz_improve(rng, iters);
  fuzz_exchange(rng, iters);
  fuzz_tw(rng, iters);
  fuzz_alternatives(rng, iters);
  fuzz_history(rng, iters);
  fuzz_mm_candidates(rng, iters);
  fuzz_mm_edge_candidates(rng, iters);
  fuzz_mm_viterbi(rng, iters);
  fuzz_avoid_mask(rng, iters);
  fuzz_tw_improve(rng, iters);
  fuzz_pd(rng, iters);
  fuzz_pd_improve(rng, iters);
  store_while_reading();
  threaded_pack_format(20000);
  std::printf("rt_selftest: %d iterations, %d failures\n", iters, g_fail);
  return g_fail ? 1 : 0;
}
