"""The native route service's SQLite writer (csrc/runtime/route_store.h) on the CPU: through the
``_rt.RouteStore`` binding it writes the rows of requests assembled by ``route_optimize_cpu`` /
``route_assemble_graph`` into a database ``SQLiteStore`` created — the same rows as the Python
store, every group size around the multi-row thresholds, refused rows, a failed result insert,
compact record rows and the time-ordered row ids."""
import json
import sqlite3

import numpy as np
import pytest

from routest_amd.ops import _ext
from routest_amd.store.store import SQLiteStore

rt = _ext.runtime(required=False)
pytestmark = pytest.mark.skipif(rt is None, reason="native runtime not built")

REQ_COLS = ("origin_id", "stops", "status", "engine", "vehicle_id", "driver_age")
RES_COLS = ("optimized_order", "total_distance", "total_duration", "legs", "geometry", "eta_minutes_ml",
            "eta_completion_time_ml")
JSON_COLS = {"stops", "optimized_order", "legs", "geometry"}
ABSENT = object()


def _payload(i=0, **over):
    """A two-stop request (distinct total_distance per i); a key given as ABSENT is left out."""
    p = {"source_point": {"lat": 14.55, "lon": 121.02},
         "destination_points": [{"lat": 14.56 + 0.001 * i, "lon": 121.03, "payload": 1},
                                {"lat": 14.57, "lon": 121.0 + 0.001 * i, "payload": 1}],
         "driver_details": {"driver_name": f"d{i}", "driver_age": 30 + i, "vehicle_capacity": 9,
                            "maximum_distance": 1e7},
         "meta": {"origin_id": f"o{i}", "destination_ids": ["x", "y"]}, "use_ml_eta": False}
    p.update(over)
    return {k: v for k, v in p.items() if v is not ABSENT}


def _row(p):
    row = rt.route_optimize_cpu(json.dumps(p).encode(), as_row=True)
    assert row is not None
    return row


def _feature(p):
    st, body = rt.route_optimize_cpu(json.dumps(p).encode())
    assert st == 200
    return json.loads(body)


@pytest.fixture()
def store(tmp_path):
    s = SQLiteStore(str(tmp_path / "r.db"))
    yield s
    s.close()


def _con(store):
    return sqlite3.connect(store.sqlite_uri, isolation_level=None)


def _columns(con, rid):
    """{column: (typeof, value)} of a request and its result, JSON texts parsed."""
    out = {}
    for table, cols, key in (("route_requests", REQ_COLS, "id"), ("route_results", RES_COLS, "request_id")):
        sel = ",".join(f"typeof({c}),{c}" for c in cols)
        rows = con.execute(f"SELECT {sel} FROM {table} WHERE {key}=?", (rid,)).fetchall()
        assert len(rows) == 1
        for k, c in enumerate(cols):
            t, v = rows[0][2 * k], rows[0][2 * k + 1]
            out[c] = (t, json.loads(v) if c in JSON_COLS and v is not None else v)
    return out


def _counts(con):
    return (con.execute("SELECT COUNT(*) FROM route_requests").fetchone()[0],
            con.execute("SELECT COUNT(*) FROM route_results").fetchone()[0])


VALUES = [7, 7.5, True, "text", None, ABSENT]


def _same_rows_payloads():
    out = []
    for i, v in enumerate(VALUES):         # origin_id / driver_name / driver_age: every JSON scalar, absent
        meta = {"destination_ids": ["x", "y"]}
        drv = {"vehicle_capacity": 9, "maximum_distance": 1e7}
        if v is not ABSENT:
            meta["origin_id"] = v
            drv["driver_name"] = VALUES[(i + 1) % 5]
            drv["driver_age"] = VALUES[(i + 2) % 5]
        out.append(_payload(i, meta=meta, driver_details=drv))
    for k, v in enumerate((ABSENT, {}, None)):
        out.append(_payload(10 + k, meta=v))
        out.append(_payload(20 + k, driver_details=v))
    out.append(_payload(30, meta={"origin_id": "o"}))                             # destination_ids absent
    out.append(_payload(31, meta={"origin_id": "o", "destination_ids": []}))
    out.append(_payload(32, use_ml_eta=True))
    return out


def test_same_rows_as_the_python_store(store):
    payloads = _same_rows_payloads()
    eta = (12.5, "2026-10-19T09:00:00.500000")
    etas = [eta if p.get("use_ml_eta") else None for p in payloads]
    native_ids = rt.RouteStore(store.sqlite_uri).commit([_row(p) for p in payloads], etas)
    con = _con(store)
    for p, e, nid in zip(payloads, etas, native_ids):
        assert nid, p
        feature = _feature(p)
        if e is not None:
            feature["properties"]["eta_minutes_ml"], feature["properties"]["eta_completion_time_ml"] = e
        pid = store.persist_request_and_result(p, feature)
        assert _columns(con, nid) == _columns(con, pid), p
    assert _columns(con, native_ids[-1])["eta_minutes_ml"] == ("real", 12.5)
    assert _columns(con, native_ids[-1])["engine"] == ("text", "ml")
    con.close()


@pytest.mark.parametrize("n", [1, 3, 4, 31, 32, 33, 37])
def test_group_sizes(store, n):
    ids = rt.RouteStore(store.sqlite_uri).commit([_row(_payload(i)) for i in range(n)])
    assert len(ids) == n and all(ids) and len(set(ids)) == n
    assert all(len(i) == 36 for i in ids)
    con = _con(store)
    assert _counts(con) == (n, n)
    linked = con.execute("SELECT q.id, q.origin_id FROM route_results r JOIN route_requests q ON q.id=r.request_id").fetchall()
    assert sorted(linked) == sorted((rid, f"o{i}") for i, rid in enumerate(ids))
    con.close()


@pytest.mark.parametrize("n", [6, 33])
@pytest.mark.parametrize("bad", [{"meta": "x"}, {"meta": [1]}, {"meta": {"origin_id": [1, 2]}}],
                         ids=["meta-str", "meta-list", "origin-list"])
def test_refused_row_leaves_its_group_stored(store, n, bad):
    mid = n // 2
    rows = [_row(_payload(i, **(bad if i == mid else {}))) for i in range(n)]
    ids = rt.RouteStore(store.sqlite_uri).commit(rows)
    assert ids[mid] == ""
    assert all(ids[i] for i in range(n) if i != mid) and len(set(ids)) == n
    con = _con(store)
    assert _counts(con) == (n - 1, n - 1)
    stored = {r[0] for r in con.execute("SELECT id FROM route_requests")}
    assert stored == {i for i in ids if i}
    assert {r[0] for r in con.execute("SELECT request_id FROM route_results")} == stored
    con.close()


@pytest.mark.parametrize("n", [5, 1])
def test_failed_result_insert_removes_its_request(store, n):
    rows = [_row(_payload(i)) for i in range(n)]
    victim = n // 2
    dist = round(_feature(_payload(victim))["properties"]["summary"]["distance"], 2)
    con = _con(store)
    con.execute(f"CREATE TRIGGER refuse BEFORE INSERT ON route_results WHEN NEW.total_distance = {dist!r} "
                "BEGIN SELECT RAISE(ABORT, 'refused'); END")
    ids = rt.RouteStore(store.sqlite_uri).commit(rows)
    assert ids[victim] == ""
    assert all(ids[i] for i in range(n) if i != victim)
    assert _counts(con) == (n - 1, n - 1)
    orphans = con.execute("SELECT COUNT(*) FROM route_requests WHERE id NOT IN (SELECT request_id FROM route_results)")
    assert orphans.fetchone()[0] == 0
    assert {r[0] for r in con.execute("SELECT id FROM route_requests")} == {i for i in ids if i}
    con.close()


def _neutral_detail(reply):
    """A history detail reply with the ids and times of its two rows replaced."""
    st, body = reply
    d = json.loads(body)
    for v in (d["request"]["id"], d["request"]["request_time"], d["result"]["id"], d["result"]["created_at"]):
        body = body.replace(v.encode(), b"*")
    return st, body


def test_compact_record_row(tmp_path):
    from routest_amd.data.graph import synth_road_graph
    from routest_amd.routing.graph import GraphProvider
    from routest_amd.store.store import RECORD_MAGIC
    g = synth_road_graph(3000, seed=1)
    prov = GraphProvider(g, (g.length_m / 9.0).astype(np.float32), device=None)
    store = SQLiteStore(str(tmp_path / "r.db"))
    store.set_record_graph(prov._steps)
    pts = [{"lat": 14.57, "lon": 121.02, "payload": 1}, {"lat": 14.61, "lon": 121.05, "payload": 1}]
    p = {"source_point": pts[0], "destination_points": pts[1:],
         "driver_details": {"driver_name": "d", "vehicle_type": "car", "vehicle_capacity": 99,
                            "maximum_distance": 1e7, "driver_age": 30},
         "meta": {"origin_id": "o", "destination_ids": ["x"]}, "use_ml_eta": False}
    nodes = g.nearest_nodes([q["lat"] for q in pts], [q["lon"] for q in pts]).astype(np.int32)
    pair = (int(nodes[0]), int(nodes[1]))
    legs = {pair: tuple(prov.legs([pair])[0][0])}
    args = (json.dumps(p).encode(), "backend:mi355x", g.lat, g.lon, nodes, None, legs, prov._steps, prov.cost)
    st, resp, rec, seg, geo = rt.route_assemble_graph(*args, with_record=True)
    assert st == 200 and rec is not None and rec[:4] == RECORD_MAGIC
    text_id = store.persist_request_and_result(p, json.loads(resp))
    (rec_id,) = rt.RouteStore(store.sqlite_uri).commit([rt.route_assemble_graph(*args, with_record=True, as_row=True)])
    assert rec_id
    con = _con(store)
    t, legs_col, geom_null = con.execute("SELECT typeof(legs), legs, geometry IS NULL FROM route_results WHERE request_id=?",
                                         (rec_id,)).fetchone()
    assert (t, bytes(legs_col), geom_null) == ("blob", rec, 1)
    con.close()
    native = rt.HistoryDb(store.sqlite_uri, graph=prov._steps)
    assert native.detail(rec_id)[0] == 200
    assert _neutral_detail(native.detail(rec_id)) == _neutral_detail(native.detail(text_id))
    store.close()


def test_row_ids_are_ordered_uuid7():
    gen = rt.RowId()
    ms = 0x0190_0000_0000
    ids = [gen.row_id(ms) for _ in range(5000)]
    for i in ids:
        assert len(i) == 36 and i[14] == "7" and i[19] in "89ab"
        assert [len(x) for x in i.split("-")] == [8, 4, 4, 4, 12]
    assert all(a < b for a, b in zip(ids, ids[1:]))

    def time_seq(i):
        h = i.replace("-", "")
        return int(h[:12], 16), int(h[13:16], 16)

    ts = [time_seq(i) for i in ids]
    assert ts[0][0] == ms and ts[0][1] <= 0x3FF
    wraps = 0
    for (t0, s0), (t1, s1) in zip(ts, ts[1:]):
        if s0 == 0xFFF:                     # the 12-bit sequence is full: the time field takes the carry
            assert (t1, s1) == (t0 + 1, 0)
            wraps += 1
        else:
            assert (t1, s1) == (t0, s0 + 1)
    assert wraps == 1 and ts[-1][0] == ms + 1
    # the clock stepping back does not break the order
    assert gen.row_id(ms - 1000) > ids[-1]
    assert time_seq(gen.row_id(ms + 5))[0] == ms + 5
