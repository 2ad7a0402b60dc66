// Native route assembly (host C++, no GPU): the reference's optimize_route response built without
// Python, byte-identical to the FastAPI handler's JSONResponse (routest_amd/routing/optimizer.py,
// providers.py, graph.py; reference RO/Flaskr/utils.py:10-201, RO/Flaskr/routes.py:29-50,89-127).
//
//  * Python-exact numerics: builtin round(x, n) (correctly rounded, half-even on exact ties),
//    numpy.round(x, 6) (rint(x * 1e6) / 1e6), float // and %, repr(float) (rt_core.h), and the
//    transcendental helpers (haversine, path length) that the Python providers call through
//    routest_amd._rt so both paths share one implementation of every libm-dependent value.
//  * A JSON writer with json.dumps(ensure_ascii=False, separators=(",", ":"), allow_nan=False)
//    semantics, so request fields echoed back (source, destinations, driver_name) keep Python's
//    int/float/str rendering and key order.
//  * RouteReq: the request fields with the reference's defaults and coercions.  Anything whose
//    Python semantics are not reproduced exactly here (a string where a number is expected, a
//    non-dict driver_details, ...) is marked `fallback` and the caller hands the request to the
//    Python app instead (csrc/native_server.hip proxies it), which owns those error semantics.
//  * Feature assembly for the haversine provider (densified straight lines) and the road-graph
//    provider (node paths from the batched A*), multi-trip concatenation, annotation.
//
// Compile with -ffp-contract=off (tools/build_ext.py): every expression must round like Python's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "json_lite.h"
#include "route_trips.h"
#include "rt_core.h"

namespace rtr {

using rtj::Value;

constexpr double EARTH_R = 6371000.0;
constexpr double PY_PI = 3.141592653589793238462643383279502884;

// ------------------------------------------------------------------ Python-exact numerics
// builtin round(x, nd): the correctly rounded decimal string, parsed back (CPython double_round).
inline double py_round(double x, int nd) {
  if (!std::isfinite(x)) return x;
  // fast path for one decimal (route step distances / durations): when x*10 is clearly away from a
  // rounding midpoint the integer is the correctly rounded one, and k/10 (one correctly rounded
  // division) is the double strtod would give for that decimal
  if (nd == 1 && std::fabs(x) < 1e9) {
    const double y = x * 10.0;
    const double k = std::nearbyint(y);
    if (std::fabs(y - k) < 0.49) return k / 10.0 == 0.0 ? std::copysign(0.0, x) : k / 10.0;
  }
  char b[64];
  std::snprintf(b, sizeof b, "%.*f", nd, x);
  return std::strtod(b, nullptr);
}
// numpy.round(x, 6) on float64: multiply, rint (half-even), true_divide
inline double np_round6(double x) { return std::nearbyint(x * 1e6) / 1e6; }

inline double py_mod(double vx, double wx) {
  double mod = std::fmod(vx, wx);
  if (mod != 0.0) {
    if ((wx < 0) != (mod < 0)) mod += wx;
  } else {
    mod = std::copysign(0.0, wx);
  }
  return mod;
}
inline double py_floordiv(double vx, double wx) {
  double mod = std::fmod(vx, wx);
  double div = (vx - mod) / wx;
  if (mod != 0.0) {
    if ((wx < 0) != (mod < 0)) div -= 1.0;
  }
  double fd;
  if (div != 0.0) {
    fd = std::floor(div);
    if (div - fd > 0.5) fd += 1.0;
  } else {
    fd = std::copysign(0.0, vx / wx);
  }
  return fd;
}

// numpy haversine_m (routing/providers.py) for scalars; the Python providers call this very
// function through routest_amd._rt, so both paths produce the same bits.
inline double haversine_m(double lat1, double lon1, double lat2, double lon2) {
  const double k = PY_PI / 180.0;
  const double p1 = lat1 * k, p2 = lat2 * k;
  const double dphi = p2 - p1;
  const double dl = lon2 * k - lon1 * k;
  const double s1 = std::sin(dphi / 2), s2 = std::sin(dl / 2);
  double a = s1 * s1 + std::cos(p1) * std::cos(p2) * (s2 * s2);
  a = a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
  return (2 * EARTH_R) * std::asin(std::sqrt(a));
}

// sum over consecutive nodes of the haversine length (sequential order), graph.py feature_from_legs
inline double path_length_m(const double* lat, const double* lon, const int32_t* p, size_t n) {
  double s = 0.0;
  for (size_t i = 0; i + 1 < n; ++i) s += haversine_m(lat[p[i]], lon[p[i]], lat[p[i + 1]], lon[p[i + 1]]);
  return s;
}

// providers.py _bearing_word (math.* == libm, like CPython's math module)
inline const char* bearing_word(double lat1, double lon1, double lat2, double lon2) {
  static const char* const W[8] = {"north", "northeast", "east", "southeast", "south", "southwest",
                                   "west", "northwest"};
  const double d2r = PY_PI / 180.0, r2d = 180.0 / PY_PI;
  const double y = std::sin((lon2 - lon1) * d2r) * std::cos(lat2 * d2r);
  const double x = std::cos(lat1 * d2r) * std::sin(lat2 * d2r) -
                   std::sin(lat1 * d2r) * std::cos(lat2 * d2r) * std::cos((lon2 - lon1) * d2r);
  const double b = py_mod(std::atan2(y, x) * r2d + 360.0, 360.0);
  long long i = (long long)py_floordiv(b + 22.5, 45.0);
  i %= 8;
  if (i < 0) i += 8;
  return W[i];
}

// ------------------------------------------------------------------ JSON writer (json.dumps)
inline void put_int(std::string& o, long long v) {
  char b[24];
  const auto r = std::to_chars(b, b + sizeof b, v);
  o.append(b, r.ptr);
}
// repr of a float that is numpy.round(x, 6) output: the decimal itself (shortest round-trip), laid
// out like repr; values below 1e-4 in magnitude take repr's exponent form via append_pyfloat.  The
// six-decimal form is repr only while it has at most 15 significant digits (|v| < 1e9): beyond, a
// double that k / 1e6 rounds back to can have a shorter repr (found by rt_selftest's fuzz_route)
inline void put_coord(std::string& o, double v) {
  const double a = std::fabs(v);
  if (!(a >= 1e-4 && a < 1e9)) { rtc::append_pyfloat(o, v); return; }
  long long k = (long long)std::nearbyint(v * 1e6);
  if ((double)k / 1e6 != v) { rtc::append_pyfloat(o, v); return; }   // not a 6-decimal value
  if (k < 0) { o += '-'; k = -k; }
  put_int(o, k / 1000000);
  long long f = k % 1000000;
  o += '.';
  if (f == 0) { o += '0'; return; }
  char d[6];
  for (int i = 5; i >= 0; --i) { d[i] = (char)('0' + f % 10); f /= 10; }
  int n = 6;
  while (n > 1 && d[n - 1] == '0') --n;
  o.append(d, n);
}
// repr: a value with at most one decimal (py_round(x, 1) output: step distances, durations,
// summaries) prints from its integer tenths; everything else through the shortest round-trip path
inline void put_float(std::string& o, double v) {
  const double a = std::fabs(v);
  if (a >= 1e-4 && a < 1e9) {
    long long k = (long long)std::nearbyint(v * 10.0);
    if ((double)k / 10.0 == v) {
      if (k < 0) { o += '-'; k = -k; }
      put_int(o, k / 10);
      o += '.';
      o += (char)('0' + k % 10);
      return;
    }
  }
  rtc::append_pyfloat(o, v);
}

// json.dumps(str, ensure_ascii=False)
inline void put_str(std::string& o, const std::string& s) {
  bool plain = true;                      // nothing to escape: one append
  for (unsigned char c : s)
    if (c < 0x20 || c == '"' || c == '\\') { plain = false; break; }
  if (plain) {
    o += '"';
    o += s;
    o += '"';
    return;
  }
  o += '"';
  for (unsigned char c : s) {
    switch (c) {
      case '"': o += "\\\""; break;
      case '\\': o += "\\\\"; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\t': o += "\\t"; break;
      case '\b': o += "\\b"; break;
      case '\f': o += "\\f"; break;
      default:
        if (c < 0x20) {
          char b[8];
          std::snprintf(b, sizeof b, "\\u%04x", c);
          o += b;
        } else {
          o += (char)c;
        }
    }
  }
  o += '"';
}

// A parsed JSON value re-serialised like json.dumps of its Python object.  Returns false where the
// Python rendering is not reproduced (NaN/inf: allow_nan=False raises; an integer token beyond
// the double's exact range is kept from its token text).
inline bool put_value(std::string& o, const Value& v) {
  switch (v.kind) {
    case Value::Null: o += "null"; return true;
    case Value::Bool: o += v.b ? "true" : "false"; return true;
    case Value::Str: put_str(o, v.str); return true;
    case Value::Num:
      if (!std::isfinite(v.num)) return false;
      if (v.is_int) {
        if (std::fabs(v.num) < 9.0e15) { put_int(o, (long long)v.num); return true; }
        return false;
      }
      put_float(o, v.num);
      return true;
    case Value::Arr: {
      o += '[';
      for (size_t i = 0; i < v.arr.size(); ++i) {
        if (i) o += ',';
        if (!put_value(o, v.arr[i])) return false;
      }
      o += ']';
      return true;
    }
    case Value::Obj: {
      o += '{';
      for (size_t i = 0; i < v.obj.size(); ++i) {
        if (i) o += ',';
        put_str(o, v.obj[i].first);
        o += ':';
        if (!put_value(o, v.obj[i].second)) return false;
      }
      o += '}';
      return true;
    }
  }
  return false;
}

// ------------------------------------------------------------------ request model
enum Profile { CAR = 0, HGV, CYCLING, ROADBIKE, FOOT };
inline const char* profile_name(int p) {
  static const char* const N[5] = {"driving-car", "driving-hgv", "cycling-regular", "cycling-road", "foot-walking"};
  return N[p];
}
inline double profile_speed(int p) {   // providers.py PROFILE_SPEED_MPS
  switch (p) {
    case HGV: return 24 / 3.6;
    case CYCLING: return 15 / 3.6;
    case ROADBIKE: return 22 / 3.6;
    case FOOT: return 5 / 3.6;
    default: return 30 / 3.6;
  }
}

inline bool is_num(const Value* v) { return v && v->kind == Value::Num; }

struct Pt {
  const Value* raw = nullptr;     // the point object (echoed back)
  double lat = 0, lon = 0;        // float(p["lat"]), float(p["lon"])
  double demand = 0;              // _float(p.get("payload", 0), 0.0)
};

struct RouteReq {
  bool fallback = false;          // hand to the Python app
  bool avoid = false;             // ... because it carries options.avoid_polygons
  bool time_windows = false;      // ... because a destination carries time_window / service
  std::string error;              // optimize_route's {"error": ...} (set instead of a route)
  const Value* root = nullptr;
  Pt src;
  std::vector<Pt> dst;
  std::string vehicle_type = "car";
  int profile = CAR;
  const Value* driver_name = nullptr;      // driver.get("driver_name") (nullptr -> null)
  double cap = 9e12, maxd = 9e12;          // multi-stop: _float semantics
  // point-to-point feasibility: `payload > cap` (TypeError -> skipped) and _float(maximum_distance)
  int p2p_cmp = 0;                         // 1: compare p2p_payload > p2p_cap, 0: skip
  double p2p_payload = 0, p2p_cap = 0;
  // use_ml_eta
  bool use_ml_eta = false;
  bool eta_ok = false;                     // driver_age coerced (else no ETA fields)
  double eta_age = 30.0;
  uint8_t eta_weather = 2, eta_traffic = 2;
  // routing context (routing/cch.py RouteContext.from_request): weather code, congestion 0..3 and
  // the pickup week-hour (-1: now) — read whether or not use_ml_eta is set
  int route_weather = 2, route_congestion = 0, route_weekhour = -1;
  // "alternatives": k (app.py _route: a non-bool number >= 2) -> 2..8, else 0 (plain optimizer)
  int alt_k = 0;
  // "improve": true (JSON true exactly; routing/improve.py wants_improve) on a multi-stop request
  // that does not ask for alternatives: intra-trip 2-opt / Or-opt after the greedy
  bool improve = false;
  // "exchange": true (same rule; routing/exchange.py wants_exchange): intra-trip improvement, the
  // inter-trip relocate / swap search, intra-trip improvement again; the value of `improve` is ignored
  bool exchange = false;
};

// _float(v, default): float(v) for numbers, default for None / missing / list / dict; strings and
// bools are converted by Python in ways not mirrored here -> fallback
inline bool coerce_float(const Value* v, double dflt, double& out) {
  if (!v || v->kind == Value::Null || v->kind == Value::Arr || v->kind == Value::Obj) { out = dflt; return true; }
  if (v->kind == Value::Num) { out = v->num; return std::isfinite(v->num) || true; }
  return false;
}

inline int code_of(const Value* v, const char* const names[4], const char* dflt) {
  return rtc::code_of(v, names, dflt);
}

// Parse the optimize_route payload (silent: non-dict -> {}).  `body_ok` is false when the body
// was not JSON (silent handlers treat it as {}).
inline RouteReq parse_route_request(const Value* root) {
  RouteReq r;
  r.root = root;
  const Value* dp = (root && root->kind == Value::Obj) ? root->get("destination_points") : nullptr;
  if (!root || root->kind != Value::Obj || !dp || !dp->truthy()) {
    r.error = "no destination points specified.";
    return r;
  }
  const Value* drv = root->get("driver_details");
  if (drv && drv->truthy() && drv->kind != Value::Obj) { r.fallback = true; return r; }
  // avoid areas (routing/avoid.py) re-weight the road graph per request: the app answers those
  const Value* opt = root->get("options");
  if (opt && opt->kind == Value::Obj && opt->get("avoid_polygons")) { r.fallback = r.avoid = true; return r; }
  // candidate routes ranked by the GCN scorer (routing/alternatives.py): a number >= 2 asks for
  // them (bools and strings do not: app.py _route); the route service answers them with the graph
  // provider once the scorer is ready, else the app does
  const Value* alt = root->get("alternatives");
  if (alt && alt->kind == Value::Num) {
    if (!std::isfinite(alt->num)) { r.fallback = true; return r; }
    if (alt->num >= 2) r.alt_k = alt->num >= 8 ? 8 : (int)alt->num;
  }
  const Value* imp = root->get("improve");
  r.improve = imp && imp->kind == Value::Bool && imp->b && r.alt_k == 0;
  const Value* exc = root->get("exchange");
  r.exchange = exc && exc->kind == Value::Bool && exc->b && r.alt_k == 0;
  if (drv && !drv->truthy()) drv = nullptr;
  // vehicle_type: (driver.get("vehicle_type") or "car"); str -> lower().strip()
  const Value* vt = drv ? drv->get("vehicle_type") : nullptr;
  if (vt && vt->truthy()) {
    if (vt->kind == Value::Str) {
      std::string s;
      for (unsigned char c : vt->str) {
        if (c >= 0x80 || (c < 0x20 && !(c == '\t' || c == '\n' || c == '\r' || c == 0x0b || c == 0x0c))) {
          r.fallback = true;           // Unicode lower()/strip() not mirrored
          return r;
        }
        s += (char)((c >= 'A' && c <= 'Z') ? c + 32 : c);
      }
      const char* ws = " \t\n\r\x0b\x0c";
      const size_t b = s.find_first_not_of(ws);
      s = b == std::string::npos ? std::string() : s.substr(b, s.find_last_not_of(ws) - b + 1);
      r.vehicle_type = s;
    } else {
      r.vehicle_type = "car";
    }
  }
  const std::string& v = r.vehicle_type;
  r.profile = v == "truck" || v == "hgv" ? HGV : v == "bike" ? CYCLING : v == "roadbike" ? ROADBIKE
            : v == "foot" ? FOOT : CAR;
  const Value* src = root->get("source_point");
  if (!src || src->kind != Value::Obj || !src->get("lat") || !src->get("lon")) {
    r.error = "source_point with lat/lon is required.";
    return r;
  }
  if (dp->kind != Value::Arr) { r.fallback = true; return r; }
  auto take = [&](const Value* p, Pt& out) -> bool {
    if (!p || p->kind != Value::Obj) return false;
    const Value* la = p->get("lat");
    const Value* lo = p->get("lon");
    if (!is_num(la) || !is_num(lo) || !std::isfinite(la->num) || !std::isfinite(lo->num)) return false;
    out.raw = p;
    out.lat = la->num;
    out.lon = lo->num;
    return true;
  };
  if (!take(src, r.src)) { r.fallback = true; return r; }
  r.dst.resize(dp->arr.size());
  for (size_t i = 0; i < dp->arr.size(); ++i) {
    if (!take(&dp->arr[i], r.dst[i])) { r.fallback = true; return r; }
    // time windows / service times (routing/timewindows.py wants_time_windows) are planned by the
    // app; single-destination and alternatives requests ignore the fields
    // (a destination carrying pickup_from makes a shipment request, routing/shipments.py: the same relay)
    if (dp->arr.size() > 1 && r.alt_k == 0 &&
        (dp->arr[i].get("time_window") || dp->arr[i].get("service") || dp->arr[i].get("pickup_from"))) {
      r.fallback = r.time_windows = true;
      return r;
    }
    double d;
    if (!coerce_float(dp->arr[i].get("payload"), 0.0, d)) { r.fallback = true; return r; }
    r.dst[i].demand = d;
  }
  r.driver_name = drv ? drv->get("driver_name") : nullptr;
  if (r.dst.size() == 1) {
    // point_to_point: payload = dest.get("payload", 0); cap = driver.get("vehicle_capacity", 999999)
    const Value* pl = r.dst[0].raw->get("payload");
    const Value* cp = drv ? drv->get("vehicle_capacity") : nullptr;
    const double plv = pl ? (is_num(pl) ? pl->num : NAN) : 0.0;
    const double cpv = cp ? (is_num(cp) ? cp->num : NAN) : 999999.0;
    const bool pl_null = pl && pl->kind == Value::Null, cp_null = cp && cp->kind == Value::Null;
    if ((pl && !is_num(pl) && !pl_null) || (cp && !is_num(cp) && !cp_null)) {
      // str > str compares, list > list compares, bool is an int: not mirrored
      if ((pl && (pl->kind == Value::Obj)) || (cp && (cp->kind == Value::Obj))) {
        r.p2p_cmp = 0;                 // dict comparisons raise TypeError -> skipped
      } else {
        r.fallback = true;
        return r;
      }
    } else if (pl_null || cp_null) {
      r.p2p_cmp = 0;                   // None > x raises TypeError -> skipped
    } else {
      r.p2p_cmp = 1;
      r.p2p_payload = plv;
      r.p2p_cap = cpv;
    }
    if (!coerce_float(drv ? drv->get("maximum_distance") : nullptr, 9e12, r.maxd)) { r.fallback = true; return r; }
  } else {
    if (!coerce_float(drv ? drv->get("vehicle_capacity") : nullptr, 9e12, r.cap) ||
        !coerce_float(drv ? drv->get("maximum_distance") : nullptr, 9e12, r.maxd)) {
      r.fallback = true;
      return r;
    }
  }
  // routing context: a non-dict context counts as {} (RouteContext.from_request)
  {
    const Value* rc = root->get("context");
    if (rc && rc->kind != Value::Obj) rc = nullptr;
    r.route_weather = code_of(rc ? rc->get("weather") : nullptr, rtc::WEATHERS, "Sunny");
    const int tc = code_of(rc ? rc->get("traffic") : nullptr, rtc::TRAFFICS, "Low");
    // TRAFFICS order (High, Jam, Low, Medium) -> congestion (2, 3, 0, 1); unknown -> Low
    r.route_congestion = tc == 0 ? 2 : tc == 1 ? 3 : tc == 3 ? 1 : 0;
    const Value* pt = rc ? rc->get("pickup_time") : nullptr;
    rtc::Stamp st;
    if (pt && pt->kind == Value::Str && rtc::parse_iso(pt->str, st)) {
      const int64_t days = (int64_t)std::floor((double)st.secs / 86400.0);
      const int64_t sod = st.secs - days * 86400;
      r.route_weekhour = (int)(((days + 3) % 7 + 7) % 7) * 24 + (int)(sod / 3600);
    }
  }
  // use_ml_eta (routes.py:97-116): context must be a dict (or falsy), driver_age float-coercible
  const Value* ue = root->get("use_ml_eta");
  r.use_ml_eta = ue && ue->truthy();
  if (r.use_ml_eta) {
    const Value* ctx = root->get("context");
    if (ctx && ctx->truthy() && ctx->kind != Value::Obj) { r.fallback = true; return r; }
    if (ctx && !ctx->truthy()) ctx = nullptr;
    r.eta_weather = (uint8_t)code_of(ctx ? ctx->get("weather") : nullptr, rtc::WEATHERS, "Sunny");
    r.eta_traffic = (uint8_t)code_of(ctx ? ctx->get("traffic") : nullptr, rtc::TRAFFICS, "Low");
    const Value* ag = drv ? drv->get("driver_age") : nullptr;
    if (!ag) { r.eta_ok = true; r.eta_age = 30.0; }
    else if (is_num(ag) && std::isfinite(ag->num)) { r.eta_ok = true; r.eta_age = ag->num == 0.0 ? 30.0 : ag->num; }
    else if (ag->kind == Value::Null || ag->kind == Value::Arr || ag->kind == Value::Obj) { r.eta_ok = false; }
    else { r.fallback = true; return r; }   // str / bool: float() semantics not mirrored
  }
  return r;
}

// ------------------------------------------------------------------ feature assembly
// One provider directions() result (an ORS-shaped Feature), kept as the pieces the multi-trip
// concatenation needs: coordinates, segments JSON, rounded summary.
struct Dir {
  std::vector<double> xy;     // lon, lat pairs (geometry coordinates)
  std::vector<uint8_t> raw;   // per point: 1 = an input coordinate (repr), 0 = rounded node/interp
  std::vector<int32_t> node;  // graph directions: per point its graph node (-1: not a node)
  std::string segments;       // JSON elements (no brackets), comma-joined
  std::vector<long long> way_points;
  double dist = 0, dur = 0;   // round(tot, 1)
};

inline void put_xy(std::string& o, double x, double y, bool raw) {
  o += '[';
  if (raw) put_float(o, x); else put_coord(o, x);
  o += ',';
  if (raw) put_float(o, y); else put_coord(o, y);
  o += ']';
}

// Every graph node's geometry point "[lon,lat]" (put_xy of its rounded coordinates), formatted
// once per graph: a route's coordinates are then copies, not ~10k float formats per response
// (the assembly stage's largest cost).  Byte-identical by construction.
struct CoordCache {
  std::string buf;
  std::vector<int64_t> ofs;   // node n at buf[ofs[n], ofs[n + 1])
  void build(const double* glat, const double* glon, size_t N) {
    buf.clear();
    buf.reserve(N * 24);
    ofs.assign(N + 1, 0);
    for (size_t n = 0; n < N; ++n) {
      put_xy(buf, np_round6(glon[n]), np_round6(glat[n]), false);
      ofs[n + 1] = (int64_t)buf.size();
    }
  }
};

inline void step_pair(std::string& seg, double d_r, double t_r, int k, int nlegs, const char* instr1,
                      long long start, long long end) {
  seg += "{\"distance\":"; put_float(seg, d_r);
  seg += ",\"duration\":"; put_float(seg, t_r);
  seg += ",\"steps\":[{\"distance\":"; put_float(seg, d_r);
  seg += ",\"duration\":"; put_float(seg, t_r);
  seg += ",\"type\":"; put_int(seg, k == 0 ? 11 : 1);
  seg += ",\"instruction\":"; put_str(seg, instr1);
  seg += ",\"name\":\"-\",\"way_points\":["; put_int(seg, start); seg += ','; put_int(seg, end);
  seg += "]},{\"distance\":0.0,\"duration\":0.0,\"type\":10,\"instruction\":";
  if (k == nlegs - 1) {
    put_str(seg, "Arrive at your destination");
  } else {
    std::string w = "Arrive at waypoint ";
    put_int(w, k + 1);
    put_str(seg, w);
  }
  seg += ",\"name\":\"-\",\"way_points\":["; put_int(seg, end); seg += ','; put_int(seg, end);
  seg += "]}]}";
}

// HaversineProvider.directions over waypoints (lon, lat) — providers.py
inline void haversine_directions(const std::vector<std::pair<double, double>>& c, int profile,
                                 double circuity, double step_m, Dir& out) {
  const double speed = profile_speed(profile);
  out.xy.assign({c[0].first, c[0].second});
  out.raw.assign({1});
  out.node.clear();                     // (interpolated points: no node strings)
  out.way_points.assign({0});
  out.segments.clear();
  double tot_d = 0.0;
  const int nlegs = (int)c.size() - 1;
  for (int k = 0; k < nlegs; ++k) {
    const double lon1 = c[k].first, lat1 = c[k].second, lon2 = c[k + 1].first, lat2 = c[k + 1].second;
    const double dist = haversine_m(lat1, lon1, lat2, lon2) * circuity;
    const long long n = std::max(1LL, (long long)std::ceil(dist / step_m));
    const long long start_wp = (long long)out.raw.size() - 1;
    const double dlon = lon2 - lon1, dlat = lat2 - lat1;
    for (long long i = 1; i <= n; ++i) {
      const double t = (double)i / (double)n;
      out.xy.push_back(np_round6(lon1 + dlon * t));
      out.xy.push_back(np_round6(lat1 + dlat * t));
      out.raw.push_back(0);
    }
    const long long end_wp = (long long)out.raw.size() - 1;
    out.way_points.push_back(end_wp);
    const double dur = dist / speed;
    const double d_r = py_round(dist, 1), t_r = py_round(dur, 1);
    if (k) out.segments += ',';
    std::string instr = "Head ";
    instr += bearing_word(lat1, lon1, lat2, lon2);
    step_pair(out.segments, d_r, t_r, k, nlegs, instr.c_str(), start_wp, end_wp);
    tot_d += dist;
  }
  out.dist = py_round(tot_d, 1);
  out.dur = py_round(tot_d / speed, 1);
}

// One searched leg: seconds (the f32 router cost), the node path and, from the CCH router, the
// metre length of that path (< 0: unknown -> summed from node coordinates, the A* legacy).
struct Leg {
  double sec = 0.0;               // (f32 search results widen exactly; alternatives sum two legs)
  const int32_t* path = nullptr;
  int len = 0;                    // 0 = not found
  double metres = -1.0;
  const int32_t* edges = nullptr; // the road edge of each hop (len - 1), when the router gave them
};

// Host view of the road graph for maneuvers: CSR, per-edge metres and seconds (the leg's routing
// context), road name ids (-1 unnamed) and the name table.
struct GraphHost {
  const int32_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const float* length = nullptr;
  const float* cost = nullptr;
  const int32_t* edge_name = nullptr;
  const std::vector<std::string>* names = nullptr;
  // per road edge (CSR order, tail -> head): its hop heading as leg_steps computes it (hop_heading),
  // formatted once per graph; nullptr: computed per hop
  const double* edge_heading = nullptr;
};

// leg_steps' hop heading from u to v: the local equirectangular bearing (one atan2 and one cos;
// the segments are metres long, so it agrees with the great-circle bearing to far below the 25 /
// 50 degree turn thresholds).  The Python provider runs this same code (_rt.GraphSteps).
inline double hop_heading(const double* glat, const double* glon, int32_t u, int32_t v) {
  const double d2r = PY_PI / 180.0, r2d = 180.0 / PY_PI;
  const double x = (glon[v] - glon[u]) * std::cos(0.5 * (glat[u] + glat[v]) * d2r), y = glat[v] - glat[u];
  return py_mod(std::atan2(x, y) * r2d + 360.0, 360.0);
}

// initial bearing (degrees, [0, 360)) — the same expression bearing_word rounds
inline double bearing_deg(double lat1, double lon1, double lat2, double lon2) {
  const double d2r = PY_PI / 180.0, r2d = 180.0 / PY_PI;
  const double y = std::sin((lon2 - lon1) * d2r) * std::cos(lat2 * d2r);
  const double x = std::cos(lat1 * d2r) * std::sin(lat2 * d2r) -
                   std::sin(lat1 * d2r) * std::cos(lat2 * d2r) * std::cos((lon2 - lon1) * d2r);
  return py_mod(std::atan2(y, x) * r2d + 360.0, 360.0);
}

// ORS maneuver type of a heading change (degrees, (-180, 180], positive = clockwise = right):
// 6 straight, 4/5 slight left/right, 0/1 left/right, 2/3 sharp left/right, 9 U-turn
inline int turn_type(double delta) {
  const double a = std::fabs(delta);
  if (a < 25.0) return 6;
  if (a < 50.0) return delta > 0 ? 5 : 4;
  if (a < 130.0) return delta > 0 ? 1 : 0;
  if (a < 170.0) return delta > 0 ? 3 : 2;
  return 9;
}
inline const char* turn_verb(int type) {
  switch (type) {
    case 0: return "Turn left";
    case 1: return "Turn right";
    case 2: return "Turn sharp left";
    case 3: return "Turn sharp right";
    case 4: return "Turn slight left";
    case 5: return "Turn slight right";
    case 9: return "Make a U-turn";
    default: return "Continue straight";
  }
}
inline double heading_change(double b_in, double b_out) {
  double d = py_mod(b_out - b_in + 180.0, 360.0) - 180.0;
  if (d == -180.0) d = 180.0;
  return d;
}

// the edge a path hop u -> v took: the cheapest under the leg's costs (lowest id on a tie — the
// router's own rule for parallel edges), -1 if none
inline int32_t hop_edge(const GraphHost& g, int32_t u, int32_t v) {
  int32_t best = -1;
  for (int32_t e = g.indptr[u]; e < g.indptr[u + 1]; ++e)
    if (g.indices[e] == v && (best < 0 || g.cost[e] < g.cost[best])) best = e;
  return best;
}

// One maneuver step of a graph leg (routing/graph.py leg_steps mirrors the fields).  The text is
// kept as parts — instruction = (head ? "Head " + head : verb) [+ (head ? " on " : " onto ") + name]
// when the road is named, name = the road name or "-" — and composed where it is written, so a
// step costs no string allocation.
struct Step {
  double dist = 0, dur = 0;       // rounded to 0.1
  int type = 11;
  const char* verb = "";          // turn verb ("Depart" for a one-node leg)
  const char* head = nullptr;     // first step: the compass word of "Head <dir>"
  const std::string* name = nullptr;   // road name (nullptr: unnamed, "-")
  long long wp0 = 0, wp1 = 0;
  std::string instruction() const {
    std::string o = head ? std::string("Head ") + head : std::string(verb);
    if (name) {
      o += head ? " on " : " onto ";
      o += *name;
    }
    return o;
  }
  std::string name_str() const { return name ? *name : std::string("-"); }
};

// Maneuver step durations in and out of leg_steps (csrc/runtime/route_record.h): the writer of a
// compact route record collects each step's rounded duration as integer tenths (`out`, with the
// step count per leg in `per_leg`); a reader replays them (`in`) instead of summing edge costs of a
// routing context it does not have.  `bad`: a duration not exactly k / 10 (never for py_round(x, 1)
// of a finite non-negative x) or a replay that ran out.
struct StepDurs {
  std::vector<uint64_t>* out = nullptr;
  std::vector<uint32_t>* per_leg = nullptr;
  const uint64_t* in = nullptr;
  size_t n_in = 0, pos = 0;
  bool bad = false;
  void put(double d) {
    if (!out) return;
    const double t = std::nearbyint(d * 10.0);
    if (!(t >= 0.0 && t < 9.0e15) || t / 10.0 != d || std::signbit(d)) { bad = true; return; }
    out->push_back((uint64_t)t);
  }
  bool take(double& d) {
    if (!in) return false;
    if (pos >= n_in) { bad = true; d = 0.0; return true; }
    d = (double)in[pos++] / 10.0;
    return true;
  }
};

// Maneuvers along one leg's node path.  A new step starts where the road name changes or the
// heading turns by >= 50 degrees; its type comes from the heading change at its first node, its
// instruction is "Head <dir>[ on <name>]" for the first step, "<verb>[ onto <name>]" after.
// Geometry indices: the leg's start coordinate is `start`, path node i is start + 1 + i, the
// destination coordinate `end`.  Distances / durations are the hop edges' metres / seconds.
inline void leg_steps(const GraphHost& g, const double* glat, const double* glon, const Leg& L, double speed_scale,
                      long long start, long long end, std::vector<Step>& out, StepDurs* sd = nullptr) {
  out.clear();
  const int n = L.len;
  if (n <= 1) {
    Step s;
    s.dist = 0.0;
    if (!(sd && sd->take(s.dur))) s.dur = py_round((double)L.sec * speed_scale, 1);
    if (sd) sd->put(s.dur);
    s.verb = "Depart";
    s.wp0 = start;
    s.wp1 = end;
    out.push_back(s);
    if (sd && sd->per_leg) sd->per_leg->push_back(1);
    return;
  }
  const int H = n - 1;
  thread_local std::vector<int32_t> hop, nm;
  thread_local std::vector<double> brg;
  hop.resize(H);
  nm.resize(H);
  brg.resize(H);
  // hop headings for the turn decisions (hop_heading; from the per-edge table when the hop's edge
  // is known: the same value, computed once per graph)
  for (int h = 0; h < H; ++h) {
    const int32_t u = L.path[h], v = L.path[h + 1];
    hop[h] = L.edges ? L.edges[h] : hop_edge(g, u, v);
    nm[h] = (hop[h] >= 0 && g.edge_name) ? g.edge_name[hop[h]] : -1;
    brg[h] = (g.edge_heading != nullptr && hop[h] >= 0 && g.indices != nullptr && g.indices[hop[h]] == v)
                 ? g.edge_heading[hop[h]]
                 : hop_heading(glat, glon, u, v);
  }
  auto name_of = [&](int32_t id) -> const std::string* {
    return (id >= 0 && g.names && id < (int32_t)g.names->size()) ? &(*g.names)[id] : nullptr;
  };
  int h0 = 0;
  while (h0 < H) {
    int h1 = h0 + 1;
    while (h1 < H && nm[h1] == nm[h1 - 1] && std::fabs(heading_change(brg[h1 - 1], brg[h1])) < 50.0) ++h1;
    Step s;
    double d = 0.0, t = 0.0;
    for (int h = h0; h < h1; ++h)
      if (hop[h] >= 0) {
        d += (double)g.length[hop[h]];
        if (g.cost) t += (double)g.cost[hop[h]];
      }
    s.dist = py_round(d, 1);
    if (!(sd && sd->take(s.dur))) s.dur = py_round(t * speed_scale, 1);
    if (sd) sd->put(s.dur);
    s.name = name_of(nm[h0]);
    if (h0 == 0) {
      s.type = 11;
      s.head = bearing_word(glat[L.path[0]], glon[L.path[0]], glat[L.path[1]], glon[L.path[1]]);
    } else {
      s.type = turn_type(heading_change(brg[h0 - 1], brg[h0]));
      s.verb = turn_verb(s.type);
    }
    s.wp0 = h0 == 0 ? start : start + 1 + h0;
    s.wp1 = h1 == H ? end : start + 1 + h1;
    out.push_back(s);
    h0 = h1;
  }
  if (sd && sd->per_leg) sd->per_leg->push_back((uint32_t)out.size());
}

// the characters of s as json.dumps would escape them inside a string (no quotes)
inline void put_str_body(std::string& o, const char* s, size_t n) {
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && (unsigned char)s[j] >= 0x20 && s[j] != '"' && s[j] != '\\') ++j;
    o.append(s + i, j - i);
    if (j >= n) break;
    const unsigned char c = (unsigned char)s[j];
    switch (c) {
      case '"': o += "\\\""; break;
      case '\\': o += "\\\\"; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\t': o += "\\t"; break;
      case '\b': o += "\\b"; break;
      case '\f': o += "\\f"; break;
      default: {
        char b[8];
        std::snprintf(b, sizeof b, "\\u%04x", c);
        o += b;
      }
    }
    i = j + 1;
  }
}

inline void put_step(std::string& o, const Step& s) {
  o += "{\"distance\":"; put_float(o, s.dist);
  o += ",\"duration\":"; put_float(o, s.dur);
  o += ",\"type\":"; put_int(o, s.type);
  o += ",\"instruction\":\"";
  if (s.head) {
    o += "Head ";
    o += s.head;
  } else {
    o += s.verb;
  }
  if (s.name) {
    o += s.head ? " on " : " onto ";
    put_str_body(o, s.name->data(), s.name->size());
  }
  o += "\",\"name\":\"";
  if (s.name) put_str_body(o, s.name->data(), s.name->size());
  else o += '-';
  o += "\",\"way_points\":["; put_int(o, s.wp0); o += ','; put_int(o, s.wp1); o += "]}";
}

// GraphProvider.feature_from_legs — graph.py.  Returns "" or the ProviderError text.
inline std::string graph_directions(const std::vector<std::pair<double, double>>& c, const int32_t* nodes,
                                    const std::vector<const Leg*>& legs, int profile, const double* glat,
                                    const double* glon, Dir& out, const GraphHost* gh = nullptr,
                                    StepDurs* sd = nullptr) {
  const double speed_scale = profile_speed(CAR) / profile_speed(profile);
  out.xy.assign({c[0].first, c[0].second});
  out.raw.assign({1});
  out.node.assign({-1});
  out.way_points.assign({0});
  out.segments.clear();
  double tot_d = 0.0, tot_t = 0.0;
  const int nlegs = (int)legs.size();
  for (int k = 0; k < nlegs; ++k) {
    const long long start = (long long)out.raw.size() - 1;
    const Leg& L = *legs[k];
    if (L.len <= 0) {
      std::string e = "no road path found between waypoints ";
      put_int(e, k); e += " and "; put_int(e, k + 1); e += " (graph nodes ";
      put_int(e, nodes[k]); e += " -> "; put_int(e, nodes[k + 1]); e += ")";
      return e;
    }
    const double dist = L.metres >= 0.f ? (double)L.metres
                      : L.len > 1 ? path_length_m(glat, glon, L.path, (size_t)L.len) * 1.15 : 0.0;
    for (int i = 0; i < L.len; ++i) {
      out.xy.push_back(np_round6(glon[L.path[i]]));
      out.xy.push_back(np_round6(glat[L.path[i]]));
      out.raw.push_back(0);
      out.node.push_back(L.path[i]);
    }
    out.xy.push_back(c[k + 1].first);
    out.xy.push_back(c[k + 1].second);
    out.raw.push_back(1);
    out.node.push_back(-1);
    const long long end = (long long)out.raw.size() - 1;
    out.way_points.push_back(end);
    const double dur = (double)L.sec * speed_scale;
    if (k) out.segments += ',';
    if (gh != nullptr && (gh->cost != nullptr || (sd != nullptr && sd->in != nullptr))) {
      // maneuvers along the path, then the arrival step (routing/graph.py feature_from_legs)
      std::vector<Step> steps;
      leg_steps(*gh, glat, glon, L, speed_scale, start, end, steps, sd);
      std::string& sg = out.segments;
      sg += "{\"distance\":"; put_float(sg, py_round(dist, 1));
      sg += ",\"duration\":"; put_float(sg, py_round(dur, 1));
      sg += ",\"steps\":[";
      for (const Step& st : steps) { put_step(sg, st); sg += ','; }
      sg += "{\"distance\":0.0,\"duration\":0.0,\"type\":10,\"instruction\":";
      if (k == nlegs - 1) {
        put_str(sg, "Arrive at your destination");
      } else {
        std::string w = "Arrive at waypoint ";
        put_int(w, k + 1);
        put_str(sg, w);
      }
      sg += ",\"name\":\"-\",\"way_points\":["; put_int(sg, end); sg += ','; put_int(sg, end);
      sg += "]}]}";
    } else {
      step_pair(out.segments, py_round(dist, 1), py_round(dur, 1), k, nlegs, "Follow the road network", start, end);
    }
    tot_d += dist;
    tot_t += dur;
  }
  out.dist = py_round(tot_d, 1);
  out.dur = py_round(tot_t, 1);
  return "";
}

inline void put_bbox(std::string& o, const std::vector<double>& xy) {
  double mnx = xy[0], mny = xy[1], mxx = xy[0], mxy = xy[1];
  for (size_t i = 2; i + 1 < xy.size(); i += 2) {   // Python min()/max(): first extreme wins
    if (xy[i] < mnx) mnx = xy[i];
    if (xy[i] > mxx) mxx = xy[i];
    if (xy[i + 1] < mny) mny = xy[i + 1];
    if (xy[i + 1] > mxy) mxy = xy[i + 1];
  }
  o += '[';
  put_float(o, mnx); o += ','; put_float(o, mny); o += ','; put_float(o, mxx); o += ','; put_float(o, mxy);
  o += ']';
}

inline void put_coords(std::string& o, const std::vector<double>& xy, const std::vector<uint8_t>& raw,
                       const std::vector<int32_t>* node = nullptr, const CoordCache* cc = nullptr) {
  const bool cached = cc != nullptr && node != nullptr && node->size() == raw.size();
  o.reserve(o.size() + raw.size() * 24 + 2);
  o += '[';
  for (size_t i = 0; i < raw.size(); ++i) {
    if (i) o += ',';
    const int32_t n = cached ? (*node)[i] : -1;
    if (n >= 0 && !raw[i] && (size_t)n + 1 < cc->ofs.size())
      o.append(cc->buf, (size_t)cc->ofs[n], (size_t)(cc->ofs[n + 1] - cc->ofs[n]));
    else
      put_xy(o, xy[2 * i], xy[2 * i + 1], raw[i] != 0);
  }
  o += ']';
}

// Trailing annotation (_annotate, optimizer.py): vehicle_type, driver_name, engine.
inline bool put_annotation(std::string& o, const RouteReq& r, const std::string& engine) {
  o += ",\"vehicle_type\":";
  put_str(o, r.vehicle_type);
  o += ",\"driver_name\":";
  if (r.driver_name) { if (!put_value(o, *r.driver_name)) return false; }
  else o += "null";
  o += ",\"engine\":";
  put_str(o, engine);
  return true;
}

// optimized_order / error text of an infeasible greedy (greedy.py InfeasibleStops)
inline std::string infeasible_msg(const std::vector<int>& stops) {
  std::string m = "infeasible stop(s) (payload exceeds vehicle capacity or round trip exceeds "
                  "maximum_distance): destination indices [";
  for (size_t i = 0; i < stops.size(); ++i) {
    if (i) m += ", ";
    put_int(m, stops[i]);
  }
  m += ']';
  return m;
}

inline std::string error_body(const std::string& msg) {
  std::string o = "{\"error\":";
  put_str(o, msg);
  o += '}';
  return o;
}

// Point-to-point feasibility after routing (optimizer.py point_to_point): "" if feasible
inline std::string p2p_errors(const RouteReq& r, double dist_m) {
  std::string e;
  if (r.p2p_cmp && r.p2p_payload > r.p2p_cap) e = "payload exceeds vehicle capacity";
  if (dist_m > r.maxd) {
    if (!e.empty()) e += " | ";
    e += "route distance exceeds maximum_distance";
  }
  return e;
}

// ------------------------------------------------------------------ whole-request assembly
// A planned request: the greedy trips (multi-stop) or the infeasible stops.
struct Plan {
  bool infeasible = false;
  std::vector<int> infeasible_stops;          // 0-based destination indices, greedy.py order
  std::vector<std::vector<int>> trips;        // index lists into [source] + destinations
  bool improved = false;                      // the trips went through improve_trips: `imp` is reported
  ImproveStats imp;
};

// properties.improvement (routing/improve.py improvement_properties)
inline void put_improvement(std::string& o, const ImproveStats& s) {
  if (s.exchange) {
    o += ",\"improvement\":{\"method\":\"2opt+oropt+exchange\",\"moves\":"; put_int(o, s.moves);
    o += ",\"exchange_moves\":"; put_int(o, s.exchange_moves);
    o += ",\"trips_before\":"; put_int(o, s.trips_before);
    o += ",\"trips_after\":"; put_int(o, s.trips_after);
  } else {
    o += ",\"improvement\":{\"method\":\"2opt+oropt\",\"moves\":"; put_int(o, s.moves);
    o += ",\"trips_changed\":"; put_int(o, s.trips_changed);
  }
  o += ",\"matrix_distance_before\":"; put_float(o, (double)s.len_before_q / 1000.0);
  o += ",\"matrix_distance_after\":"; put_float(o, (double)s.len_after_q / 1000.0);
  o += '}';
}

// The directions calls optimize_route makes, as waypoint lists [(lon, lat), ...]:
// point-to-point -> [source, dest]; multi-stop -> one list per trip.
inline void directions_calls(const RouteReq& r, const Plan& p,
                             std::vector<std::vector<std::pair<double, double>>>& calls) {
  calls.clear();
  if (!r.error.empty() || r.fallback || p.infeasible) return;
  if (r.dst.size() == 1) {
    calls.push_back({{r.src.lon, r.src.lat}, {r.dst[0].lon, r.dst[0].lat}});
    return;
  }
  for (const auto& t : p.trips) {
    std::vector<std::pair<double, double>> c;
    c.reserve(t.size());
    for (int i : t) c.emplace_back(i == 0 ? r.src.lon : r.dst[i - 1].lon, i == 0 ? r.src.lat : r.dst[i - 1].lat);
    calls.push_back(std::move(c));
  }
}

// The geometry coordinates and the segments array of a request's directions results, exactly as
// assemble() writes them (one call: its own; several trips: concatenated, empty segment lists
// skipped) — the compact route record's reader (route_record.h) rebuilds the persisted texts with it.
inline void dirs_geometry(const std::vector<Dir>& dirs, const CoordCache* cc, std::string& coords,
                          std::string& segments) {
  std::vector<double> xy;
  std::vector<uint8_t> raw;
  std::vector<int32_t> node;
  bool nodes_ok = cc != nullptr;
  for (const Dir& d : dirs) {
    xy.insert(xy.end(), d.xy.begin(), d.xy.end());
    raw.insert(raw.end(), d.raw.begin(), d.raw.end());
    nodes_ok = nodes_ok && d.node.size() == d.raw.size();
    if (nodes_ok) node.insert(node.end(), d.node.begin(), d.node.end());
  }
  coords.clear();
  put_coords(coords, xy, raw, nodes_ok ? &node : nullptr, cc);
  segments = "[";
  bool first = true;
  for (const Dir& d : dirs) {
    if (d.segments.empty()) continue;
    if (!first) segments += ',';
    first = false;
    segments += d.segments;
  }
  segments += ']';
}

// The assembled response (properties left open so ETA / persistence fields can follow) and the
// pieces the persistence rows reuse.
struct Assembled {
  bool ok = false;
  std::string error;                          // optimize_route {"error": ...}
  std::string body;                           // Feature JSON up to the open properties object
  std::string coords;                         // geometry.coordinates JSON
  std::string segments;                       // properties.segments JSON
  std::string order;                          // optimized_order JSON
  double dist = 0, dur = 0;                   // properties.summary distance / duration
};

// Assemble from the directions results `dirs` (one per directions_calls entry).
inline bool assemble(const RouteReq& r, const Plan& p, const std::vector<Dir>& dirs,
                     const std::string& engine, Assembled& a, const CoordCache* cc = nullptr) {
  a = Assembled();
  if (!r.error.empty()) { a.error = r.error; return true; }
  if (p.infeasible) { a.error = infeasible_msg(p.infeasible_stops); return true; }
  std::string& o = a.body;
  if (r.dst.size() == 1) {
    const Dir& d = dirs[0];
    const std::string e = p2p_errors(r, d.dist);
    if (!e.empty()) { a.error = e; return true; }
    put_coords(a.coords, d.xy, d.raw, &d.node, cc);
    a.segments = "[" + d.segments + "]";
    a.order = "[0]";
    a.dist = d.dist;
    a.dur = d.dur;
    o += "{\"type\":\"Feature\",\"bbox\":";
    put_bbox(o, d.xy);
    o += ",\"geometry\":{\"type\":\"LineString\",\"coordinates\":";
    o += a.coords;
    o += "},\"properties\":{\"segments\":";
    o += a.segments;
    o += ",\"summary\":{\"distance\":"; put_float(o, d.dist);
    o += ",\"duration\":"; put_float(o, d.dur);
    o += "},\"way_points\":[";
    for (size_t i = 0; i < d.way_points.size(); ++i) { if (i) o += ','; put_int(o, d.way_points[i]); }
    o += "],\"optimized_order\":[0],\"source\":";
    if (!put_value(o, *r.src.raw)) return false;
    o += ",\"destinations\":[";
    if (!put_value(o, *r.dst[0].raw)) return false;
    o += ']';
  } else {
    std::vector<double> xy;
    std::vector<uint8_t> raw;
    std::vector<int32_t> node;
    bool nodes_ok = cc != nullptr;
    double tot_d = 0.0, tot_t = 0.0;
    for (const Dir& d : dirs) {
      xy.insert(xy.end(), d.xy.begin(), d.xy.end());
      raw.insert(raw.end(), d.raw.begin(), d.raw.end());
      nodes_ok = nodes_ok && d.node.size() == d.raw.size();
      if (nodes_ok) node.insert(node.end(), d.node.begin(), d.node.end());
      tot_d += d.dist;
      tot_t += d.dur;
    }
    put_coords(a.coords, xy, raw, nodes_ok ? &node : nullptr, cc);
    a.segments = "[";
    bool first = true;
    for (const Dir& d : dirs) {
      if (d.segments.empty()) continue;
      if (!first) a.segments += ',';
      first = false;
      a.segments += d.segments;
    }
    a.segments += ']';
    a.order = "[";
    first = true;
    for (const auto& t : p.trips)
      for (size_t i = 1; i + 1 < t.size(); ++i) {
        if (!first) a.order += ',';
        first = false;
        put_int(a.order, t[i] - 1);
      }
    a.order += ']';
    a.dist = tot_d;
    a.dur = tot_t;
    o += "{\"bbox\":";
    put_bbox(o, xy);
    o += ",\"type\":\"Feature\",\"geometry\":{\"type\":\"LineString\",\"coordinates\":";
    o += a.coords;
    o += "},\"properties\":{\"source\":";
    if (!put_value(o, *r.src.raw)) return false;
    o += ",\"destinations\":";
    if (!put_value(o, *r.root->get("destination_points"))) return false;
    o += ",\"optimized_order\":";
    o += a.order;
    o += ",\"segments\":";
    o += a.segments;
    o += ",\"summary\":{\"distance\":"; put_float(o, tot_d);
    o += ",\"duration\":"; put_float(o, tot_t);
    o += ",\"trips\":"; put_int(o, (long long)p.trips.size());
    o += '}';
    if (p.improved) put_improvement(o, p.imp);
  }
  if (!put_annotation(o, r, engine)) return false;
  a.ok = true;
  return true;
}

// ------------------------------------------------------------------ nearest-node snapping
// Exact nearest neighbour on (lat, lon * c) — the metric of RoadGraph.nearest_nodes (a KD-tree
// over the same scaled coordinates) — with a uniform bucket grid.  Ties go to the lower node id.
struct NodeGrid {
  std::vector<double> y, x;              // lat, lon * c
  double y0 = 0, x0 = 0, cell = 1;
  int ny = 1, nx = 1;
  std::vector<int32_t> start, items;

  void build(const double* lat, const double* lon, size_t n, double c) {
    y.resize(n);
    x.resize(n);
    double y1 = -1e300, x1 = -1e300;
    y0 = x0 = 1e300;
    for (size_t i = 0; i < n; ++i) {
      y[i] = lat[i];
      x[i] = lon[i] * c;
      y0 = std::min(y0, y[i]); x0 = std::min(x0, x[i]);
      y1 = std::max(y1, y[i]); x1 = std::max(x1, x[i]);
    }
    const double area = std::max((y1 - y0) * (x1 - x0), 1e-18);
    cell = std::max(std::sqrt(area / std::max<double>(1.0, (double)n / 2.0)), 1e-9);
    ny = std::max(1, (int)((y1 - y0) / cell) + 1);
    nx = std::max(1, (int)((x1 - x0) / cell) + 1);
    std::vector<int32_t> cnt((size_t)ny * nx + 1, 0);
    for (size_t i = 0; i < n; ++i) ++cnt[cell_of(y[i], x[i]) + 1];
    for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
    start = cnt;
    items.resize(n);
    std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
    for (size_t i = 0; i < n; ++i) items[fill[cell_of(y[i], x[i])]++] = (int32_t)i;
  }
  size_t cell_of(double yy, double xx) const {
    int iy = (int)std::floor((yy - y0) / cell), ix = (int)std::floor((xx - x0) / cell);
    iy = std::min(std::max(iy, 0), ny - 1);
    ix = std::min(std::max(ix, 0), nx - 1);
    return (size_t)iy * nx + ix;
  }
  int32_t nearest(double lat, double lon, double c) const {
    const double qy = lat, qx = lon * c;
    double best = INFINITY;
    int32_t bi = -1;
    auto consider = [&](int32_t i) {
      const double dy = y[i] - qy, dx = x[i] - qx;
      const double d2 = dy * dy + dx * dx;
      if (d2 < best || (d2 == best && i < bi)) { best = d2; bi = i; }
    };
    // start at the query's cell clamped into the grid: a node in a cell r + 1 or more index steps
    // away (Chebyshev) from it is at least r cells from the query, inside or outside the grid
    double fcy = std::floor((qy - y0) / cell), fcx = std::floor((qx - x0) / cell);
    fcy = std::min(std::max(fcy, 0.0), (double)(ny - 1));
    fcx = std::min(std::max(fcx, 0.0), (double)(nx - 1));
    const int cy = (int)fcy, cx = (int)fcx;
    for (int r = 0;; ++r) {
      // ring r around (cy, cx), clamped to the grid
      for (int iy = cy - r; iy <= cy + r; ++iy) {
        if (iy < 0 || iy >= ny) continue;
        const bool edge_row = (iy == cy - r || iy == cy + r);
        for (int ix = cx - r; ix <= cx + r; ix += (edge_row ? 1 : std::max(1, 2 * r))) {
          if (ix < 0 || ix >= nx) continue;
          const size_t k = (size_t)iy * nx + ix;
          for (int32_t j = start[k]; j < start[k + 1]; ++j) consider(items[j]);
        }
      }
      // a node in ring r + 1 or beyond is at least r cells (Chebyshev) from the query's cell
      const double m = (double)r * cell;
      if (bi >= 0 && best <= m * m) return bi;
      if (r > ny + nx + 4) return bi;
    }
  }
};

}  // namespace rtr
