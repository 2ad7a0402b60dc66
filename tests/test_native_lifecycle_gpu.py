"""Native front end lifecycle and failure semantics (verdict r3 item 4):

* model hot swap: /api/admin/reload_model (relayed to the app) re-packs the model for every GPU
  slot of the native front end; the main port then answers with the NEW model, byte-equal to the
  app;
* GPU quarantine + failover: with launches failing on one of two reactor GPU slots (a shared-GPU
  rehearsal: both slots on device 0), no request sees a 5xx — failed rounds re-run on the other
  slot, the failing slot is quarantined after ROUTEST_QUARANTINE_AFTER failures; with every slot
  failing the model's fp32 CPU forward answers;
* model coverage: wide MLPs (H = 1024) and tree ensembles are served natively (the main port stays
  native), matching the Python path;
* /api/health reports the native slots."""
import http.client
import json
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BODY = {"summary": {"distance": 12345}, "pickup_time": "2025-08-25T08:30:00", "driver_age": 34,
        "weather": "Sunny", "traffic": "Medium"}


def _req(port, method, path, body=None):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    raw = None if body is None else json.dumps(body).encode()
    c.request(method, path, body=raw, headers={"Content-Type": "application/json"} if raw else {})
    r = c.getresponse()
    return r.status, r.read()


def _stack(model, tmp_path=None):
    from routest_amd.api.app import build_services, create_app
    from routest_amd.config import load_settings
    from routest_amd.serve.eta_service import EtaService
    from routest_amd.serve.frontend import ServingStack
    s = load_settings(env={}, dotenv_path=None, devices=[0], warm_scorer=False)
    sv = build_services(s, eta=EtaService(model, devices=[0]), store=None)
    return ServingStack(sv, create_app(sv), model, [0], threads=2), sv


def test_reload_hot_swaps_the_native_model(tmp_path):
    from routest_amd.models.checkpoint import save_checkpoint
    from routest_amd.serve.eta_service import default_model
    m1, m2 = default_model(seed=1, steps=30), default_model(seed=2, steps=60)
    save_checkpoint(str(tmp_path / "m2"), m2, trainer_state={"step": 1})
    st, sv = _stack(m1)
    try:
        a0 = _req(st.port, "POST", "/api/predict_eta", BODY)
        r = _req(st.port, "POST", "/api/admin/reload_model", {"path": str(tmp_path / "m2")})
        assert r[0] == 200 and json.loads(r[1])["ok"]
        assert st.front.model_epoch == 2
        a1 = _req(st.port, "POST", "/api/predict_eta", BODY)
        b1 = _req(st.app_server.port, "POST", "/api/predict_eta", BODY)
        assert a1[0] == b1[0] == 200 and a1[1] == b1[1]          # the new model, byte-equal to the app
        assert a1[1] != a0[1]
        h = json.loads(_req(st.port, "GET", "/api/health")[1])
        assert h["checks"]["native"]["model_epoch"] == 2 and h["checks"]["native"]["status"] == "ok"
    finally:
        st.close()


def _hammer(port, n, threads=8):
    codes = []
    lock = threading.Lock()

    def run(k):
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        for i in range(n // threads):
            b = dict(BODY, summary={"distance": 1000 + 17 * (i + k)})
            c.request("POST", "/api/predict_eta", body=json.dumps(b).encode(),
                      headers={"Content-Type": "application/json"})
            r = c.getresponse()
            r.read()
            with lock:
                codes.append(r.status)
    ts = [threading.Thread(target=run, args=(k,)) for k in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return codes


def test_failing_gpu_slot_is_quarantined_without_5xx(monkeypatch):
    from routest_amd.serve.eta_service import default_model
    from routest_amd.serve.native_server import NativePredictServer
    monkeypatch.setenv("ROUTEST_QUARANTINE_AFTER", "3")
    monkeypatch.setenv("ROUTEST_PERSIST_IDLE_MS", "0")       # every round a normal launch
    model = default_model(steps=30)
    with NativePredictServer(model, device=[0, 0], threads=4) as srv:
        ref = _req(srv.port, "POST", "/api/predict_eta", BODY)
        assert srv.set_fault(1, True)
        codes = _hammer(srv.port, 400)
        assert codes.count(200) == len(codes) == 400          # 0 5xx: failed rounds ran on slot 0
        h = srv.health()
        assert h["slots"][1]["quarantined"] and h["slots"][1]["quarantines"] == 1, h
        assert not h["slots"][0]["quarantined"] and h["degraded"]
        assert h["stats"]["failovers"] >= 1
        assert _req(srv.port, "POST", "/api/predict_eta", BODY) == ref
        # every slot failing: the fp32 CPU forward answers (close to the bf16 kernel)
        assert srv.set_fault(0, True)
        codes = _hammer(srv.port, 80, threads=4)
        assert codes.count(200) == 80
        assert srv.stats()["cpu_rounds"] > 0
        st, body = _req(srv.port, "POST", "/api/predict_eta", BODY)
        assert st == 200
        np.testing.assert_allclose(json.loads(body)["eta_minutes_ml"], json.loads(ref[1])["eta_minutes_ml"],
                                   rtol=3e-2)
        # recovery: the fault cleared, a probe restores the slot
        srv.set_fault(0, False)
        srv.set_fault(1, False)


def test_env_fault_hook_reaches_the_native_path(monkeypatch):
    from routest_amd.serve.eta_service import default_model
    from routest_amd.serve.native_server import NativePredictServer
    monkeypatch.setenv("ROUTEST_FAULT", "gpu_fail@1")
    monkeypatch.setenv("ROUTEST_PERSIST_IDLE_MS", "0")
    with NativePredictServer(default_model(steps=20), device=[0, 0], threads=2) as srv:
        assert srv.health()["slots"][1]["fault_injected"] and not srv.health()["slots"][0]["fault_injected"]
        assert _hammer(srv.port, 64, threads=4).count(200) == 64


def test_wide_mlp_served_natively_matches_python():
    from routest_amd.models.mlp3 import EtaMLP
    from routest_amd.data.synth import synth_trips
    from routest_amd.ops.eta_mlp import EtaMlpKernel
    torch.manual_seed(0)
    m = EtaMLP(1024)
    x, y = synth_trips(4000, 0)
    m.fit_normalization(x, y)
    st, sv = _stack(m)
    try:
        assert st.front is not None
        items = [{"summary": {"distance": 500 + 97 * i}, "pickup_time": "2025-08-27T17:30:00",
                  "traffic": ["High", "Low", "Jam"][i % 3], "driver_age": 20 + i % 50} for i in range(300)]
        a = _req(st.port, "POST", "/predict", items)
        b = _req(st.app_server.port, "POST", "/predict", items)
        assert a[0] == b[0] == 200
        pa = [p["eta_minutes_ml"] for p in json.loads(a[1])["predictions"]]
        pb = [p["eta_minutes_ml"] for p in json.loads(b[1])["predictions"]]
        np.testing.assert_allclose(pa, pb, rtol=1e-5, atol=1e-4)
        assert st.front.stats()["predictions"] >= 300            # answered natively
        assert "wide" in st.front.health()["slots"][0]["model"]
    finally:
        st.close()


def test_forest_served_natively_matches_cpu_reference():
    from sklearn.ensemble import HistGradientBoostingRegressor
    from routest_amd.data.synth import synth_trips
    from routest_amd.models.forest import ForestModel
    x, y = synth_trips(5000, 1)
    hgb = HistGradientBoostingRegressor(max_iter=40, max_leaf_nodes=15, random_state=0).fit(x, y)
    fm = ForestModel.from_sklearn_hgb(hgb)
    st, sv = _stack(fm)
    try:
        assert st.front is not None and "forest" in st.front.health()["slots"][0]["model"]
        a = _req(st.port, "POST", "/api/predict_eta", BODY)
        b = _req(st.app_server.port, "POST", "/api/predict_eta", BODY)
        assert a[0] == b[0] == 200
        np.testing.assert_allclose(json.loads(a[1])["eta_minutes_ml"], json.loads(b[1])["eta_minutes_ml"],
                                   rtol=1e-5)
        assert st.front.stats()["predictions"] >= 1
    finally:
        st.close()


@pytest.mark.parametrize("le", [False, True])
def test_synthetic_forest_served_natively_is_exact(le):
    """make_forest_model + launch_forest (csrc/native_model.hip, forest.hip forest_kernel) behind
    the native front end, on a synthetic forest whose sums are exact in f32 (tests/_forest_synth.py:
    integer leaves, thresholds drawn from the requests' own feature values): the served minutes
    equal the numpy reference exactly, through the native port and through the app."""
    from _forest_synth import TreeGen
    from routest_amd.models.features import RECORD_DTYPE, records_to_features
    from routest_amd.models.forest import ForestModel
    from routest_amd.serve.eta_service import EtaService
    items = [{"summary": {"distance": [0, 1000, 2500, 500.5, 12345.678, 99999][i % 6]},
              "pickup_time": f"2025-08-{20 + i % 9:02d}T{(5 * i) % 24:02d}:30:00",
              "weather": ["Cloudy", "Stormy", "Sunny", "Windy", "Foggy"][i % 5],
              "traffic": ["High", "Jam", "Low", "Medium", "Unknown"][(i // 5) % 5],
              "driver_age": [18, 30, 45.5, 64][(i // 3) % 4]} for i in range(300)]
    rec = np.array([EtaService.make_record(weather=it["weather"], traffic=it["traffic"],
                                           distance_m=float(it["summary"]["distance"]), pickup_time=it["pickup_time"],
                                           driver_age=float(it["driver_age"]))[0] for it in items], dtype=RECORD_DTYPE)
    x = records_to_features(rec)
    g = TreeGen(x, 21)
    trees = [g.tree(s) for s in [("leaf",), ("chain", 64), ("grow", 200, 3, 12), ("full", 6), ("chain", 7)]
             + [("grow", 30, 2, 8)] * 30]
    fm = ForestModel._pack(trees, 5.0, le, list(range(12)))
    want = [float(v) for v in fm.predict_features(x)]
    flipped = ForestModel._pack(trees, 5.0, not le, list(range(12))).predict_features(x)
    assert np.mean(flipped != np.asarray(want, np.float32)) >= 0.10      # `<` for `<=` would show
    st, sv = _stack(fm)
    try:
        assert st.front is not None and "forest" in st.front.health()["slots"][0]["model"]
        a = _req(st.port, "POST", "/predict", items)
        b = _req(st.app_server.port, "POST", "/predict", items)
        assert a[0] == b[0] == 200
        assert [p["eta_minutes_ml"] for p in json.loads(a[1])["predictions"]] == want
        assert [p["eta_minutes_ml"] for p in json.loads(b[1])["predictions"]] == want
        assert st.front.stats()["predictions"] >= 300            # answered natively
    finally:
        st.close()


@pytest.mark.run_first
def test_hung_gpu_slot_watchdog_and_route_failover():
    """Verdict r4 item 5 / SURVEY §5.3 "a watchdog on batch latency": with gpu_hang@1 (slot 1's
    launches wait on a host flag) on a 2-slot shared-GPU rehearsal, no request waits longer than
    the deadline + one round, nothing answers 5xx, slot 1 is quarantined, and route requests keep
    being answered natively — slot 1's route service hands its flushes to slot 0's, and slot 0 is
    never quarantined (ROUTEST_ROUTE_TRACE_MS=20 in the child's environment prints the timeline)."""
    import gc
    import os
    import subprocess
    import sys
    # what earlier tests of this session left behind (routers, servers, their streams and builder
    # threads) goes before the child measures 100 ms deadlines on the shared GPU
    gc.collect()
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="32", ROUTEST_GPU_DEADLINE_MS="100", ROUTEST_ROUTE_DEADLINE_MS="300",
               ROUTEST_PERSIST_IDLE_MS="0", ROUTEST_QUARANTINE_PROBE_MS="60000",
               ROUTEST_HANG_ARM="1", ROUTEST_ROUTE_TRACE_MS="20")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_watchdog_child.py")], capture_output=True,
                       text=True, timeout=240, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("\n".join(ln for ln in r.stderr.splitlines() if ln.startswith("[route") or ln.startswith("[predict")))
    assert d["routes_on"]
    assert d["codes"] == [200] and d["route_codes"] == [200], d
    print(json.dumps(d))
    assert d["slot1"]["quarantined"] and d["slot1"]["deadline_timeouts"] >= 1, d
    # the healthy slot is untouched: its predictions and route flushes never wait behind the hung
    # one (the flush's copies run on its own queue, csrc/route_service.hip qcopy; the app's relayed
    # flushes on a non-blocking stream, routing/route_batcher.py)
    assert not d["slot0"]["quarantined"] and d["slot0"]["deadline_timeouts"] == 0, d
    # predictions: never longer than the deadline (0.1 s) + one round (failover / CPU forward)
    assert d["max_predict_s"] < 1.0, d
    # routes: the hung slot's flushes are handed to the other slot's route service natively, within
    # the route deadline (0.3 s) plus two flush periods; nothing is relayed to the app
    assert d["route_failed_over"] >= 1, d
    assert d["max_route_s"] < 0.3 + 0.2, d
    assert d["route_service_fallbacks"] == 0 and d["route_jobs"] >= d["n_routes"], d


def test_route_failover_is_bounded_when_every_service_fails():
    """a flush failure that repeats on every GPU's route service (not a timeout)
    must not bounce its jobs between the services forever.  ROUTEST_FAULT=route_fail makes every
    flush fail; each job is handed to the other slot's service at most once (2 slots: n-1 = 1 hop)
    and then relayed to the app, which answers it."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROUTEST_FAULT="route_fail", ROUTEST_PERSIST_IDLE_MS="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_watchdog_child.py"), "route_fail"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(d))
    assert d["routes_on"] and d["route_codes"] == [200] and d["codes"] == [200], d
    # every route request answered by the app after at most one hop each
    assert d["route_service_fallbacks"] == d["n_routes"], d
    assert d["route_failed_over"] <= d["n_routes"], d
    assert d["max_route_s"] < 5.0, d
    assert not d["slot0"]["quarantined"] and not d["slot1"]["quarantined"], d
