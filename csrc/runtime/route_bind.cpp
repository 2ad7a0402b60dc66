// routest_amd._rt bindings of the native route assembler (csrc/runtime/route_core.h).
//
//  * haversine_m / path_length_m / NodeGrid: the libm-dependent values of the Python providers
//    (routing/providers.py, routing/graph.py, data/graph.py) come from these, so the Python path
//    and the native front end (csrc/native_server.hip) produce identical bits.
//  * route_optimize_cpu: the whole haversine-provider request on the CPU in C++ (parse, matrix,
//    R21 greedy, directions, assembly) -> (status, body) or None (fallback to Python) — the CPU
//    reference the GPU service is tested against, and a fast path for GPU-less deployments.
//  * route_assemble_graph: graph-provider assembly from given trips + searched legs (tests);
//    `improvement`: the statistics of trips that were improved (routing/improve.py).
//  * MmGrid / mm_viterbi: the host reference of the map matcher (map_match.h; the definition is in
//    routing/mapmatch.py, the HIP kernels in csrc/map_match.hip); MmEdgeGrid / mm_edge_route_cm: the
//    edge-based matcher's (routing/mapmatch_edge.py, csrc/map_match_edge.hip).
//  * RouteStore / RowId: the route service's SQLite writer (route_store.h) over requests assembled
//    by the two functions above (as_row=True) — its CPU tests.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <map>
#include <memory>
#include <mutex>

#include "alternatives.h"
#include "history_db.h"
#include "map_match.h"
#include "route_core.h"
#include "route_record.h"
#include "route_store.h"

namespace py = pybind11;

namespace {

using rtr::Value;

double py_haversine(double lat1, double lon1, double lat2, double lon2) {
  return rtr::haversine_m(lat1, lon1, lat2, lon2);
}

double py_path_length(py::array_t<double, py::array::c_style | py::array::forcecast> lat,
                      py::array_t<double, py::array::c_style | py::array::forcecast> lon,
                      py::array_t<int32_t, py::array::c_style | py::array::forcecast> path) {
  const int64_t n = lat.shape(0);
  const int32_t* p = path.data();
  for (py::ssize_t i = 0; i < path.shape(0); ++i)
    if (p[i] < 0 || p[i] >= n) throw std::out_of_range("path node out of range");
  return rtr::path_length_m(lat.data(), lon.data(), p, (size_t)path.shape(0));
}

py::array_t<double> py_haversine_matrix(py::array_t<double, py::array::c_style | py::array::forcecast> lat,
                                        py::array_t<double, py::array::c_style | py::array::forcecast> lon,
                                        double circuity) {
  const py::ssize_t n = lat.shape(0);
  py::array_t<double> D({n, n});
  double* d = D.mutable_data();
  const double* la = lat.data();
  const double* lo = lon.data();
  for (py::ssize_t i = 0; i < n; ++i)
    for (py::ssize_t j = 0; j < n; ++j)
      d[i * n + j] = i == j ? 0.0 : rtr::haversine_m(la[i], lo[i], la[j], lo[j]) * circuity;
  return D;
}

class PyNodeGrid {
 public:
  PyNodeGrid(py::array_t<double, py::array::c_style | py::array::forcecast> lat,
             py::array_t<double, py::array::c_style | py::array::forcecast> lon, double c)
      : c_(c) {
    if (lat.shape(0) != lon.shape(0) || lat.shape(0) == 0) throw std::invalid_argument("lat/lon mismatch");
    g_.build(lat.data(), lon.data(), (size_t)lat.shape(0), c);
  }
  py::array_t<int32_t> nearest(py::array_t<double, py::array::c_style | py::array::forcecast> lats,
                               py::array_t<double, py::array::c_style | py::array::forcecast> lons) const {
    const py::ssize_t n = lats.shape(0);
    py::array_t<int32_t> out(n);
    int32_t* o = out.mutable_data();
    const double* la = lats.data();
    const double* lo = lons.data();
    {
      py::gil_scoped_release nogil;
      for (py::ssize_t i = 0; i < n; ++i) o[i] = g_.nearest(la[i], lo[i], c_);
    }
    return out;
  }

 private:
  rtr::NodeGrid g_;
  double c_;
};

// map_match.h: the bucket grid over a graph's quantized node coordinates and its radius queries
class PyMmGrid {
 public:
  PyMmGrid(py::array_t<int64_t, py::array::c_style | py::array::forcecast> qy,
           py::array_t<int64_t, py::array::c_style | py::array::forcecast> qx) {
    if (qy.ndim() != 1 || qx.ndim() != 1 || qy.shape(0) != qx.shape(0)) throw std::invalid_argument("qy/qx mismatch");
    g_.build(qy.data(), qx.data(), (size_t)qy.shape(0));
  }
  py::tuple candidates(py::array_t<int64_t, py::array::c_style | py::array::forcecast> py_,
                       py::array_t<int64_t, py::array::c_style | py::array::forcecast> px_, int64_t radius_cm,
                       int k) const {
    if (py_.ndim() != 1 || px_.ndim() != 1 || py_.shape(0) != px_.shape(0)) throw std::invalid_argument("py/px mismatch");
    if (k < 1 || k > rtr::kMmMaxK) throw std::invalid_argument("k in 1..16");
    const py::ssize_t P = py_.shape(0);
    py::array_t<int32_t> cand({P, (py::ssize_t)k});
    py::array_t<int64_t> d2({P, (py::ssize_t)k});
    py::array_t<int32_t> n(P);
    {
      const int64_t* a = py_.data();
      const int64_t* b = px_.data();
      int32_t* c = cand.mutable_data();
      int64_t* d = d2.mutable_data();
      int32_t* e = n.mutable_data();
      py::gil_scoped_release nogil;
      rtr::mm_candidates(g_, a, b, (size_t)P, radius_cm, k, c, d, e);
    }
    return py::make_tuple(cand, d2, n);
  }

 private:
  rtr::MmGrid g_;
};

// map_match.h: the bucket grid over a graph's matchable edges and its radius queries
class PyMmEdgeGrid {
 public:
  using I64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
  using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
  PyMmEdgeGrid(I64 qy, I64 qx, I32 tail, I32 head, I64 lc, int64_t cell) {
    if (qy.ndim() != 1 || qx.ndim() != 1 || qy.shape(0) != qx.shape(0)) throw std::invalid_argument("qy/qx mismatch");
    if (tail.ndim() != 1 || head.ndim() != 1 || lc.ndim() != 1 || tail.shape(0) != head.shape(0) ||
        tail.shape(0) != lc.shape(0))
      throw std::invalid_argument("tail/head/lc mismatch");
    if (cell < 1) throw std::invalid_argument("cell: at least one centimetre");
    g_.build(qy.data(), qx.data(), (size_t)qy.shape(0), tail.data(), head.data(), lc.data(), (size_t)tail.shape(0), cell);
  }
  py::tuple candidates(I64 py_, I64 px_, int64_t radius_cm, int k) const {
    if (py_.ndim() != 1 || px_.ndim() != 1 || py_.shape(0) != px_.shape(0)) throw std::invalid_argument("py/px mismatch");
    if (k < 1 || k > rtr::kMmMaxK) throw std::invalid_argument("k in 1..16");
    const py::ssize_t P = py_.shape(0);
    py::array_t<int32_t> cand({P, (py::ssize_t)k}), fq({P, (py::ssize_t)k});
    py::array_t<int64_t> d2({P, (py::ssize_t)k});
    py::array_t<int32_t> n(P);
    {
      const int64_t* a = py_.data();
      const int64_t* b = px_.data();
      int32_t* c = cand.mutable_data();
      int64_t* d = d2.mutable_data();
      int32_t* f = fq.mutable_data();
      int32_t* e = n.mutable_data();
      py::gil_scoped_release nogil;
      rtr::mm_edge_candidates(g_, a, b, (size_t)P, radius_cm, k, c, d, f, e);
    }
    return py::make_tuple(cand, d2, fq, n);
  }
  py::dict layout() const {   // the grid itself, for tests of its listing property
    py::dict d;
    d["y0"] = g_.y0;
    d["x0"] = g_.x0;
    d["cell"] = g_.cell;
    d["ny"] = g_.ny;
    d["nx"] = g_.nx;
    d["start"] = py::array_t<int32_t>((py::ssize_t)g_.start.size(), g_.start.data());
    d["items"] = py::array_t<int32_t>((py::ssize_t)g_.items.size(), g_.items.data());
    return d;
  }

 private:
  rtr::MmEdgeGrid g_;
};

// route_cm i64 [rows, K, K] (map_match.h mm_edge_route_cm)
py::array_t<int64_t> py_mm_edge_route_cm(py::array_t<float, py::array::c_style | py::array::forcecast> met,
                                         py::array_t<int32_t, py::array::c_style | py::array::forcecast> e1,
                                         py::array_t<int64_t, py::array::c_style | py::array::forcecast> off1,
                                         py::array_t<int64_t, py::array::c_style | py::array::forcecast> lc1,
                                         py::array_t<int32_t, py::array::c_style | py::array::forcecast> e2,
                                         py::array_t<int64_t, py::array::c_style | py::array::forcecast> off2) {
  if (met.ndim() != 3 || met.shape(1) != met.shape(2)) throw std::invalid_argument("met must be [rows, K, K]");
  const py::ssize_t rows = met.shape(0), K = met.shape(1);
  if (K < 1 || K > rtr::kMmMaxK) throw std::invalid_argument("K in 1..16");
  auto row_k = [&](const py::array& a) { return a.ndim() == 2 && a.shape(0) == rows && a.shape(1) == K; };
  if (!row_k(e1) || !row_k(off1) || !row_k(lc1) || !row_k(e2) || !row_k(off2))
    throw std::invalid_argument("edge, off and lc must be [rows, K]");
  py::array_t<int64_t> out({rows, K, K});
  {
    const float* m = met.data();
    const int32_t *a = e1.data(), *b = e2.data();
    const int64_t *o1 = off1.data(), *l1 = lc1.data(), *o2 = off2.data();
    int64_t* o = out.mutable_data();
    py::gil_scoped_release nogil;
    rtr::mm_edge_route_cm(m, a, o1, l1, b, o2, (size_t)rows, (int)K, o);
  }
  return out;
}

// (choice i32 [B, T], segment i32 [B, T], n_segments i32 [B], cost i64 [B])
py::tuple py_mm_viterbi(py::array_t<int64_t, py::array::c_style | py::array::forcecast> cand_d2,
                        py::array_t<int32_t, py::array::c_style | py::array::forcecast> n_cand,
                        py::array_t<int64_t, py::array::c_style | py::array::forcecast> route_cm,
                        py::array_t<int64_t, py::array::c_style | py::array::forcecast> g,
                        py::array_t<int32_t, py::array::c_style | py::array::forcecast> npts, int64_t beta_cm,
                        int64_t sigma_cm, int64_t max_detour_cm) {
  if (cand_d2.ndim() != 3) throw std::invalid_argument("cand_d2 must be [B, T, K]");
  const py::ssize_t B = cand_d2.shape(0), T = cand_d2.shape(1), K = cand_d2.shape(2);
  if (K < 1 || K > rtr::kMmMaxK || T < 1 || T > rtr::kMmMaxPoints) throw std::invalid_argument("K in 1..16, T in 1..2048");
  if (n_cand.ndim() != 2 || n_cand.shape(0) != B || n_cand.shape(1) != T) throw std::invalid_argument("n_cand must be [B, T]");
  if (route_cm.ndim() != 4 || route_cm.shape(0) != B || route_cm.shape(1) != T - 1 || route_cm.shape(2) != K ||
      route_cm.shape(3) != K)
    throw std::invalid_argument("route_cm must be [B, T-1, K, K]");
  if (g.ndim() != 2 || g.shape(0) != B || g.shape(1) != T - 1) throw std::invalid_argument("g must be [B, T-1]");
  if (npts.ndim() != 1 || npts.shape(0) != B) throw std::invalid_argument("npts must be [B]");
  const rtr::MmCosts c{beta_cm, sigma_cm, max_detour_cm};
  rtr::mm_check_costs(c);
  py::array_t<int32_t> choice({B, T}), seg({B, T});
  py::array_t<int32_t> nseg(B);
  py::array_t<int64_t> cost(B);
  {
    const int64_t* cd = cand_d2.data();
    const int32_t* nc = n_cand.data();
    const int64_t* rc = route_cm.data();
    const int64_t* gg = g.data();
    const int32_t* np = npts.data();
    int32_t* ch = choice.mutable_data();
    int32_t* sg = seg.mutable_data();
    int32_t* ns = nseg.mutable_data();
    int64_t* co = cost.mutable_data();
    py::gil_scoped_release nogil;
    for (py::ssize_t b = 0; b < B; ++b)
      co[b] = rtr::mm_viterbi(cd + b * T * K, nc + b * T, rc + b * (T - 1) * K * K, gg + b * (T - 1), (int)T, (int)K,
                              np[b], c, ch + b * T, sg + b * T, ns + b);
  }
  return py::make_tuple(choice, seg, nseg, cost);
}

// Maneuvers of graph legs (route_core.h leg_steps) for the Python GraphProvider: the graph's
// arrays are held once; per call the leg's node path, seconds and the context's edge costs.
class PyGraphSteps {
 public:
  PyGraphSteps(py::array_t<int32_t, py::array::c_style | py::array::forcecast> indptr,
               py::array_t<int32_t, py::array::c_style | py::array::forcecast> indices,
               py::array_t<float, py::array::c_style | py::array::forcecast> length,
               py::array_t<double, py::array::c_style | py::array::forcecast> lat,
               py::array_t<double, py::array::c_style | py::array::forcecast> lon, py::object edge_name,
               std::vector<std::string> names)
      : indptr_(indptr), indices_(indices), length_(length), lat_(lat), lon_(lon), names_(std::move(names)) {
    const py::ssize_t N = lat.shape(0), E = indices.shape(0);
    if (indptr.shape(0) != N + 1 || lon.shape(0) != N || length.shape(0) != E || indptr.data()[N] != E)
      throw std::invalid_argument("graph shapes");
    if (!edge_name.is_none()) {
      name_ = edge_name.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
      if (name_.shape(0) != E) throw std::invalid_argument("edge_name per edge");
    }
  }
  // the graph host view with the given per-edge costs (kept alive by the caller)
  rtr::GraphHost host(const py::array_t<float, py::array::c_style | py::array::forcecast>& cost) const {
    if (cost.shape(0) != indices_.shape(0)) throw std::invalid_argument("cost per edge");
    rtr::GraphHost g;
    g.indptr = indptr_.data();
    g.indices = indices_.data();
    g.length = length_.data();
    g.cost = cost.data();
    g.edge_name = name_.size() ? name_.data() : nullptr;
    g.names = &names_;
    return g;
  }
  // the compact route records' view of this graph (built on first use: CoordCache, headings,
  // fingerprint); shared with a HistoryDb
  std::shared_ptr<const rrec::RecordGraph> record_graph() const {
    std::lock_guard<std::mutex> lk(rg_mu_);
    if (!rg_) {
      auto g = std::make_shared<rrec::RecordGraph>();
      g->build((int)lat_.shape(0), lat_.data(), lon_.data(), indptr_.data(), indices_.data(), length_.data(),
               name_.size() ? name_.data() : nullptr, &names_);
      rg_ = g;
    }
    return rg_;
  }
  // (legs JSON, geometry JSON) of a record the native route service persisted (store.py)
  py::tuple decode_record(py::bytes rec) const {
    const std::string b = rec;
    auto g = record_graph();
    std::string seg, geo, err;
    bool ok;
    {
      py::gil_scoped_release nogil;
      ok = rrec::decode(*g, b.data(), b.size(), seg, geo, &err);
    }
    if (!ok) throw std::invalid_argument(err);
    return py::make_tuple(seg, geo);
  }
  std::string fingerprint() const { return std::to_string(record_graph()->fp); }
  py::list steps(py::array_t<int32_t, py::array::c_style | py::array::forcecast> path, double sec,
                 py::array_t<float, py::array::c_style | py::array::forcecast> cost, double speed_scale,
                 long long start, long long end) const {
    const py::ssize_t N = lat_.shape(0);
    if (cost.shape(0) != indices_.shape(0)) throw std::invalid_argument("cost per edge");
    for (py::ssize_t i = 0; i < path.shape(0); ++i)
      if (path.data()[i] < 0 || path.data()[i] >= N) throw std::out_of_range("path node");
    rtr::GraphHost g;
    g.indptr = indptr_.data();
    g.indices = indices_.data();
    g.length = length_.data();
    g.cost = cost.data();
    g.edge_name = name_.size() ? name_.data() : nullptr;
    g.names = &names_;
    rtr::Leg L;
    L.sec = sec;
    L.path = path.data();
    L.len = (int)path.shape(0);
    std::vector<rtr::Step> st;
    rtr::leg_steps(g, lat_.data(), lon_.data(), L, speed_scale, start, end, st);
    py::list out;
    for (const auto& x : st)
      out.append(py::make_tuple(x.dist, x.dur, x.type, x.instruction(), x.name_str(), x.wp0, x.wp1));
    return out;
  }

 private:
  py::array_t<int32_t, py::array::c_style | py::array::forcecast> indptr_, indices_;
  py::array_t<float, py::array::c_style | py::array::forcecast> length_;
  py::array_t<double, py::array::c_style | py::array::forcecast> lat_, lon_;
  py::array_t<int32_t, py::array::c_style | py::array::forcecast> name_;
  std::vector<std::string> names_;
  mutable std::mutex rg_mu_;
  mutable std::shared_ptr<const rrec::RecordGraph> rg_;
};

py::bytes to_bytes(const std::string& s) { return py::bytes(s); }

// The native history reader (history_db.h) for CPU tests: (status, body) or None (-> the app).
class PyHistoryDb {
 public:
  explicit PyHistoryDb(const std::string& path, py::object graph) {
    std::string err;
    if (!db_.open(path, err)) throw std::runtime_error("HistoryDb: " + err);
    if (!graph.is_none()) db_.set_graph(graph.cast<const PyGraphSteps&>().record_graph());
  }
  py::object wrap(const rth::Reply& r) {
    if (r.fallback) return py::none();
    return py::make_tuple(r.status, to_bytes(r.body));
  }
  py::object history(py::object limit) {
    if (limit.is_none()) return wrap(db_.history(nullptr));
    const std::string l = limit.cast<std::string>();
    return wrap(db_.history(l.c_str()));
  }
  py::object detail(const std::string& id) { return wrap(db_.detail(id)); }
  py::object del(const std::string& id) { return wrap(db_.del(id)); }
  py::object locations() { return wrap(db_.locations()); }

 private:
  rth::HistoryDb db_;
};

// Finish an assembled request as the FastAPI handler answers it (no ETA, no persistence).
std::pair<int, std::string> finish_plain(const rtr::Assembled& a, bool request_route_compat, bool is_request_route) {
  if (!a.error.empty()) {
    const int st = (is_request_route && request_route_compat) ? 200 : 400;
    return {st, rtr::error_body(a.error)};
  }
  return {200, a.body + "}}"};
}

// One request assembled on the CPU as a row for the native writer (route_store.h): the body and
// its parsed root stay with the row (StoreRow::root points into this object, which pybind11 keeps
// on the heap).
struct PyRouteRow {
  std::string body;
  Value root;
  rts::StoreRow row;
};

// false: the request is one for the Python app (-> None)
bool optimize_cpu(PyRouteRow& o, bool json_ok, const std::string& engine, double circuity, double step_m,
                  bool is_request_route) {
  const std::string& b = o.body;
  Value& root = o.root;
  bool parsed = false;
  if (json_ok && !b.empty()) {
    try {
      root = rtj::Parser(b.data(), b.size()).parse();
      parsed = true;
    } catch (const std::exception&) {
    }
  }
  if (is_request_route && (!json_ok || (!parsed && !b.empty()))) return false;   // 415 / 400: Python
  static const Value empty = [] { Value v; v.kind = Value::Obj; return v; }();
  const Value* rootp = parsed ? &root : (is_request_route ? nullptr : &empty);
  if (!is_request_route && parsed && root.kind != Value::Obj) rootp = &empty;   // silent: non-dict -> {}
  rtr::RouteReq r = rtr::parse_route_request(rootp);
  if (r.fallback || r.alt_k > 0) return false;     // alternatives: graph provider + scorer only
  o.row.root = rootp;
  rtr::Plan plan;
  if (r.error.empty() && r.dst.size() > 1) {
    const int n1 = (int)r.dst.size() + 1;
    std::vector<double> lat(n1), lon(n1), dem(n1, 0.0), D((size_t)n1 * n1, 0.0);
    lat[0] = r.src.lat;
    lon[0] = r.src.lon;
    for (int i = 1; i < n1; ++i) {
      lat[i] = r.dst[i - 1].lat;
      lon[i] = r.dst[i - 1].lon;
      dem[i] = r.dst[i - 1].demand;
    }
    for (int i = 0; i < n1; ++i)
      for (int j = 0; j < n1; ++j)
        D[(size_t)i * n1 + j] = i == j ? 0.0 : rtr::haversine_m(lat[i], lon[i], lat[j], lon[j]) * circuity;
    plan.infeasible = !rtr::greedy_trips(D, n1, dem, r.cap, r.maxd, plan.trips, plan.infeasible_stops);
    if (r.exchange && !plan.infeasible) {
      plan.imp = rtr::improve_exchange_trips(D, n1, dem, r.cap, r.maxd, plan.trips);
      plan.improved = true;
    } else if (r.improve && !plan.infeasible) {
      plan.imp = rtr::improve_trips(D, n1, r.maxd, plan.trips);
      plan.improved = true;
    }
  }
  std::vector<std::vector<std::pair<double, double>>> calls;
  rtr::directions_calls(r, plan, calls);
  std::vector<rtr::Dir> dirs(calls.size());
  for (size_t k = 0; k < calls.size(); ++k)
    rtr::haversine_directions(calls[k], r.profile, circuity, step_m, dirs[k]);
  return rtr::assemble(r, plan, dirs, engine, o.row.asmb);
}

py::object route_optimize_cpu(py::bytes body, bool json_ok, const std::string& engine, double circuity,
                              double step_m, bool is_request_route, bool compat200, bool as_row) {
  auto o = std::make_unique<PyRouteRow>();
  o->body = body;
  if (!optimize_cpu(*o, json_ok, engine, circuity, step_m, is_request_route)) return py::none();
  if (as_row) return py::cast(std::move(o));
  auto res = finish_plain(o->row.asmb, compat200, is_request_route);
  return py::make_tuple(res.first, to_bytes(res.second));
}

// Graph-provider assembly with given trips and searched legs: `trips` per request as index lists
// (None for point-to-point), `legs` {(s, t): (seconds, [nodes]) | (seconds, metres, [nodes])}
// (missing / empty = not found); with `steps` (GraphSteps) + `cost` the segments carry maneuvers.
// as_row: the assembled request (and its record, with_record) as a row for RouteStore.
py::object route_assemble_graph(py::bytes body, const std::string& engine,
                                py::array_t<double, py::array::c_style | py::array::forcecast> glat,
                                py::array_t<double, py::array::c_style | py::array::forcecast> glon,
                                py::array_t<int32_t, py::array::c_style | py::array::forcecast> nodes_of_calls,
                                py::object trips_obj, py::dict legs_obj, py::object steps_obj, py::object cost_obj,
                                bool with_record, bool as_row, py::object improvement) {
  auto o = std::make_unique<PyRouteRow>();
  o->body = body;
  const std::string& b = o->body;
  Value& root = o->root;
  root = rtj::Parser(b.data(), b.size()).parse();
  rtr::RouteReq r = rtr::parse_route_request(&root);
  if (r.fallback) return py::none();
  o->row.root = &root;
  rtr::Plan plan;
  if (!trips_obj.is_none()) plan.trips = trips_obj.cast<std::vector<std::vector<int>>>();
  if (!improvement.is_none() && py::len(improvement) == 6) {
    // the given trips went through the exchange pipeline:
    // (moves, exchange_moves, trips_before, trips_after, before_q, after_q)
    const auto st = improvement.cast<std::tuple<long long, long long, long long, long long, long long, long long>>();
    plan.imp.exchange = true;
    plan.imp.moves = std::get<0>(st);
    plan.imp.exchange_moves = std::get<1>(st);
    plan.imp.trips_before = std::get<2>(st);
    plan.imp.trips_after = std::get<3>(st);
    plan.imp.len_before_q = std::get<4>(st);
    plan.imp.len_after_q = std::get<5>(st);
    plan.improved = true;
  } else if (!improvement.is_none()) {  // the given trips were improved: (moves, trips_changed, before_q, after_q)
    const auto st = improvement.cast<std::tuple<long long, long long, long long, long long>>();
    plan.imp.moves = std::get<0>(st);
    plan.imp.trips_changed = std::get<1>(st);
    plan.imp.len_before_q = std::get<2>(st);
    plan.imp.len_after_q = std::get<3>(st);
    plan.improved = true;
  }
  std::vector<std::vector<std::pair<double, double>>> calls;
  rtr::directions_calls(r, plan, calls);
  // legs table
  std::map<std::pair<int, int>, std::pair<rtr::Leg, std::vector<int32_t>>> table;
  for (auto kv : legs_obj) {
    auto key = kv.first.cast<std::pair<int, int>>();
    py::tuple val = kv.second.cast<py::tuple>();
    auto& e = table[key];
    e.first.sec = val[0].cast<double>();
    if (val.size() == 3) {
      e.first.metres = val[1].cast<double>();
      e.second = val[2].cast<std::vector<int32_t>>();
    } else {
      e.second = val[1].cast<std::vector<int32_t>>();
    }
    e.first.len = (int)e.second.size();
    e.first.path = e.second.data();
  }
  rtr::GraphHost gh;
  const rtr::GraphHost* ghp = nullptr;
  py::array_t<float, py::array::c_style | py::array::forcecast> cost;
  std::shared_ptr<const rrec::RecordGraph> rg;
  if (!steps_obj.is_none()) {
    const PyGraphSteps& st = steps_obj.cast<const PyGraphSteps&>();
    if (with_record) rg = st.record_graph();
    if (!cost_obj.is_none()) {
      cost = cost_obj.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
      gh = st.host(cost);
      ghp = &gh;
    }
  }
  // (the compact record, as the route service writes it: route_record.h)
  rrec::Writer rw;
  bool rec_ok = rg != nullptr;
  if (rec_ok) rrec::begin(rw, *rg, ghp != nullptr, r.profile, calls.size());
  const int32_t* nodes = nodes_of_calls.data();
  std::vector<rtr::Dir> dirs(calls.size());
  size_t off = 0;
  rtr::Leg missing;
  for (size_t k = 0; k < calls.size(); ++k) {
    std::vector<const rtr::Leg*> legs;
    for (size_t i = 0; i + 1 < calls[k].size(); ++i) {
      auto it = table.find({nodes[off + i], nodes[off + i + 1]});
      legs.push_back(it == table.end() ? &missing : &it->second.first);
    }
    std::vector<uint64_t> durs;
    std::vector<uint32_t> per_leg;
    rtr::StepDurs sd;
    sd.out = &durs;
    sd.per_leg = &per_leg;
    const std::string e = rtr::graph_directions(calls[k], nodes + off, legs, r.profile, glat.data(), glon.data(), dirs[k],
                                                ghp, rec_ok && ghp ? &sd : nullptr);
    off += calls[k].size();
    if (!e.empty()) {
      r.error = e;
      rec_ok = false;
      break;
    }
    if (rec_ok) rec_ok = !sd.bad && rrec::add_call(rw, *rg, ghp, calls[k], legs, durs, per_leg);
  }
  rtr::Assembled& a = o->row.asmb;
  if (!rtr::assemble(r, plan, dirs, engine, a)) return py::none();
  if (rec_ok && a.ok) o->row.rec = std::move(rw.b);
  if (as_row) return py::cast(std::move(o));
  auto res = finish_plain(a, true, false);
  if (!with_record) return py::make_tuple(res.first, to_bytes(res.second));
  // (status, body, record bytes or None, the row's legs text, the row's geometry text)
  std::string geo = "{\"type\":\"LineString\",\"coordinates\":" + a.coords + "}";
  return py::make_tuple(res.first, to_bytes(res.second),
                        rec_ok && a.ok ? py::object(to_bytes(o->row.rec)) : py::object(py::none()), a.segments, geo);
}

// The native writer over a database the Python store created: the given rows committed as ONE
// group -> their request ids ("" = not stored).  `etas`: per row None or (eta_min, eta_iso).
class PyRouteStore {
 public:
  explicit PyRouteStore(const std::string& path) {
    if (!s_.open(path)) throw std::runtime_error("RouteStore: cannot open " + path);
  }
  std::vector<std::string> commit(std::vector<PyRouteRow*> rows, py::object etas) {
    std::vector<rts::StoreRow*> g;
    for (size_t i = 0; i < rows.size(); ++i) {
      rts::StoreRow& r = rows[i]->row;
      r.eta_min = NAN;
      r.eta_iso.clear();
      if (!etas.is_none() && !etas.cast<py::list>()[i].is_none()) {
        const auto eta = etas.cast<py::list>()[i].cast<std::pair<float, std::string>>();
        r.eta_min = eta.first;
        r.eta_iso = eta.second;
      }
      r.ok = false;               // as the service: only an assembled route is stored
      if (r.root != nullptr && r.asmb.ok) rts::RouteStore::prepare(r);
      g.push_back(&r);
    }
    {
      py::gil_scoped_release nogil;
      s_.commit_group(g);
    }
    std::vector<std::string> ids;
    for (rts::StoreRow* r : g) ids.push_back(r->request_id);
    return ids;
  }
 private:
  rts::RouteStore s_;
};

using F64 = py::array_t<double, py::array::c_style | py::array::forcecast>;
using I32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

std::vector<int> py_via_nodes(F64 lat, F64 lon, int s, int t, int n, double stretch) {
  if (lat.shape(0) != lon.shape(0)) throw std::invalid_argument("lat/lon length mismatch");
  py::gil_scoped_release nogil;
  return ralt::via_nodes(lat.data(), lon.data(), (int)lat.shape(0), s, t, n, stretch);
}

std::vector<double> py_alt_scores(F64 lat, F64 lon, F64 delay, std::vector<I32> paths, std::vector<double> seconds,
                                  int kind) {
  const int64_t N = lat.shape(0);
  if (lon.shape(0) != N || delay.shape(0) != N) throw std::invalid_argument("lat/lon/delay length mismatch");
  if (seconds.size() != paths.size()) throw std::invalid_argument("one seconds value per path");
  std::vector<double> out(paths.size());
  for (size_t i = 0; i < paths.size(); ++i) {
    const int32_t* p = paths[i].data();
    const size_t n = (size_t)paths[i].shape(0);
    for (size_t k = 0; k < n; ++k)
      if (p[k] < 0 || p[k] >= N) throw std::out_of_range("path node out of range");
    out[i] = ralt::candidate_score(lat.data(), lon.data(), delay.data(), p, n, seconds[i], kind);
  }
  return out;
}

}  // namespace

void bind_route(py::module& m) {
  m.def("via_nodes", &py_via_nodes, py::arg("lat"), py::arg("lon"), py::arg("s"), py::arg("t"), py::arg("n"),
        py::arg("stretch") = 1.35);
  m.def("alt_scores", &py_alt_scores, py::arg("lat"), py::arg("lon"), py::arg("delay"), py::arg("paths"),
        py::arg("seconds"), py::arg("kind"));
  m.def("haversine_m", &py_haversine);
  m.def("path_length_m", &py_path_length);
  m.def("haversine_matrix", &py_haversine_matrix);
  py::class_<PyNodeGrid>(m, "NodeGrid")
      .def(py::init<py::array_t<double, py::array::c_style | py::array::forcecast>,
                    py::array_t<double, py::array::c_style | py::array::forcecast>, double>())
      .def("nearest", &PyNodeGrid::nearest);
  py::class_<PyMmGrid>(m, "MmGrid")
      .def(py::init<py::array_t<int64_t, py::array::c_style | py::array::forcecast>,
                    py::array_t<int64_t, py::array::c_style | py::array::forcecast>>(),
           py::arg("qy"), py::arg("qx"))
      .def("candidates", &PyMmGrid::candidates, py::arg("py"), py::arg("px"), py::arg("radius_cm"), py::arg("k"));
  m.def("mm_candidates",   // one-off form: builds the grid for this call
        [](py::array_t<int64_t, py::array::c_style | py::array::forcecast> qy,
           py::array_t<int64_t, py::array::c_style | py::array::forcecast> qx,
           py::array_t<int64_t, py::array::c_style | py::array::forcecast> py_,
           py::array_t<int64_t, py::array::c_style | py::array::forcecast> px_, int64_t radius_cm, int k) {
          return PyMmGrid(qy, qx).candidates(py_, px_, radius_cm, k);
        },
        py::arg("qy"), py::arg("qx"), py::arg("py"), py::arg("px"), py::arg("radius_cm"), py::arg("k"));
  py::class_<PyMmEdgeGrid>(m, "MmEdgeGrid")
      .def(py::init<PyMmEdgeGrid::I64, PyMmEdgeGrid::I64, PyMmEdgeGrid::I32, PyMmEdgeGrid::I32, PyMmEdgeGrid::I64,
                    int64_t>(),
           py::arg("qy"), py::arg("qx"), py::arg("tail"), py::arg("head"), py::arg("lc"), py::arg("cell"))
      .def("candidates", &PyMmEdgeGrid::candidates, py::arg("py"), py::arg("px"), py::arg("radius_cm"), py::arg("k"))
      .def("layout", &PyMmEdgeGrid::layout);
  m.def("mm_edge_route_cm", &py_mm_edge_route_cm, py::arg("met"), py::arg("e1"), py::arg("off1"), py::arg("lc1"),
        py::arg("e2"), py::arg("off2"));
  m.def("mm_viterbi", &py_mm_viterbi, py::arg("cand_d2"), py::arg("n_cand"), py::arg("route_cm"), py::arg("g"),
        py::arg("npts"), py::arg("beta_cm"), py::arg("sigma_cm"), py::arg("max_detour_cm"));
  m.def("route_optimize_cpu", &route_optimize_cpu, py::arg("body"), py::arg("json_ok") = true,
        py::arg("engine") = "backend:mi355x", py::arg("circuity") = 1.3, py::arg("step_m") = 150.0,
        py::arg("is_request_route") = false, py::arg("compat200") = true, py::arg("as_row") = false);
  m.def("route_assemble_graph", &route_assemble_graph, py::arg("body"), py::arg("engine"), py::arg("glat"),
        py::arg("glon"), py::arg("nodes"), py::arg("trips"), py::arg("legs"), py::arg("steps") = py::none(),
        py::arg("cost") = py::none(), py::arg("with_record") = false, py::arg("as_row") = false,
        py::arg("improvement") = py::none());
  py::class_<PyRouteRow>(m, "RouteRow");
  py::class_<PyRouteStore>(m, "RouteStore")
      .def(py::init<const std::string&>(), py::arg("path"))
      .def("commit", &PyRouteStore::commit, py::arg("rows"), py::arg("etas") = py::none());
  py::class_<rts::RowId>(m, "RowId").def(py::init<>()).def("row_id", [](rts::RowId& r, uint64_t ms) { return r.next(ms); });
  m.def("py_round", &rtr::py_round);
  m.def("json_float", [](double v) {     // the native JSON writer's float (tests: == json.dumps)
    std::string o;
    rtr::put_float(o, v);
    return o;
  });
  py::class_<PyHistoryDb>(m, "HistoryDb")
      .def(py::init<const std::string&, py::object>(), py::arg("path"), py::arg("graph") = py::none())
      .def("history", &PyHistoryDb::history, py::arg("limit") = py::none())
      .def("detail", &PyHistoryDb::detail)
      .def("delete", &PyHistoryDb::del)
      .def("locations", &PyHistoryDb::locations);
  py::class_<PyGraphSteps>(m, "GraphSteps")
      .def(py::init<py::array_t<int32_t, py::array::c_style | py::array::forcecast>,
                    py::array_t<int32_t, py::array::c_style | py::array::forcecast>,
                    py::array_t<float, py::array::c_style | py::array::forcecast>,
                    py::array_t<double, py::array::c_style | py::array::forcecast>,
                    py::array_t<double, py::array::c_style | py::array::forcecast>, py::object,
                    std::vector<std::string>>(),
           py::arg("indptr"), py::arg("indices"), py::arg("length"), py::arg("lat"), py::arg("lon"),
           py::arg("edge_name") = py::none(), py::arg("names") = std::vector<std::string>())
      .def("steps", &PyGraphSteps::steps, py::arg("path"), py::arg("sec"), py::arg("cost"), py::arg("speed_scale"),
           py::arg("start"), py::arg("end"))
      .def("decode_record", &PyGraphSteps::decode_record, py::arg("record"))
      .def("fingerprint", &PyGraphSteps::fingerprint);
  m.def("bearing_word", [](double a, double b, double c, double d) { return std::string(rtr::bearing_word(a, b, c, d)); });
}
