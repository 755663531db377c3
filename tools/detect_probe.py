"""What a detector program costs under spoofing and closed-loop PI dosing, four ways, at 10 000 x 8 over 120 steps of
10 s with a scan per step, both PI loops and the 4-slot injection program of inject_probe.py:
  (a) one fused call without a detector program, the reference point;
  (b) the same call with four OFF slots (the section's fixed cost: the flag, t_prev and four kind loads);
  (c) the same call with one slot of each kind plus a SENSOR cross-check;
  (d) the host way the study needs without the feature: the call of (a) with enable_sensors(history=K), a download
      of the whole reading history, and the injection and detector updates in numpy (tests/inject_ref.py,
      tests/detect_ref.py) over its scans.
The four alternate over five repeats in rotating order; the medians are reported: the step call alone for (b)/(a)
and (c)/(a), and the call plus what the study ends with -- the detector state download for (c), the history download and
the numpy loop for (d) -- for (d)/(c).  Checks that every plant state of
(b), (c) and (d) is bitwise (a)'s and that (c)'s detector state is bitwise (d)'s, and prints one JSON line.
   python tools/detect_probe.py [N] [n] [steps]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from detect_ref import DetectRef
from inject_ref import InjectRef
from program_helpers import HostScan
wt = importlib.import_module("ics-wt-physicsengine_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = int(sys.argv[3]) if len(sys.argv) > 3 else 120
DT = 10.0
cols, bc = wt.make_ensemble(N)
u = np.random.default_rng(3).random((8, N))
chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
span = K * DT
program = [wt.Injection("chlorine_outlet", "constant", start=0.25 * span, end=0.5 * span, a=0.0),      # spoofed low
           wt.Injection("pH_outlet", "freeze", start=span * u[4], end=span * u[4] + 0.3 * span),         # frozen probe
           wt.Injection("chlorine_outlet", "bias", start=0.6 * span, a=-0.5 * u[5]),
           wt.Injection("pH_inlet", "fault", start=0.8 * span, a=3)]
iblock = wt.injection_block(N, *program)
label = wt.attack_window(iblock)
limits = np.geomspace(1.0, 10.0, N)                              # one threshold per reactor: a ROC curve per call
detectors = [wt.Detector("chlorine_outlet", "cusum", limits, sigma=0.05, ref="track", tau=300.0, t_arm=60.0),
             wt.Detector("temp_outlet", "ewma", 0.5 * limits, sigma=0.1, ref_value=np.asarray(cols["temperature"]), source="field",
                         on_bad="alarm"),
             wt.Detector("pH_outlet", "flatline", 60.0),
             wt.Detector("chlorine_outlet", "cusum", limits, sigma=0.05, ref="chlorine_outlet", ref_source="field")]
off = [wt.Detector(k, "off", 1.0) for k in range(4)]
dblock = wt.detector_block(N, *detectors)


def outputs(ens):
    es = ens.state
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status) + ens.sensor_readings() + ens.input_image() + \
        (ens.boundary(), ens.control_state().block(), ens.injection_state().block())


def run(variant):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=1, history=K if variant == "host" else 0)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    ens.enable_control(chlorine, acid)
    ens.set_injections(*program)
    if variant in ("off", "four"):
        ens.set_detectors(*(off if variant == "off" else detectors), attack=label)
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(DT, n_steps=K, download=False)
    ens.synchronize()
    t_step = time.perf_counter() - t0
    st = None
    if variant == "host":
        vh, _, fh, _ = ens.sensor_history()
        ref = DetectRef(dblock, np.stack(label), np.zeros(N))
        hs = HostScan(N, inj=InjectRef(iblock), dt=DT)
        k = -1
        for steps in hs.calls(K, 1):
            k += steps
            vt, ft = hs.scan(vh[k], fh[k])
            ref.scan(vh[k], fh[k], hs.lt, image=(vt, ft))
        st = (ref.st, ref.t_prev)
    elif variant == "four":
        st = ens.detector_state().block()                       # the download the study ends with
    t_all = time.perf_counter() - t0
    out = outputs(ens)
    ens.close()
    return t_step, t_all, out, st


run("four")                                      # module load, first launches
VARIANTS, REPEATS = ("none", "off", "four", "host"), 5
times, totals, outs, states = {v: [] for v in VARIANTS}, {v: [] for v in VARIANTS}, {}, {}
for rep in range(REPEATS):
    for i in range(len(VARIANTS)):
        v = VARIANTS[(i + rep) % len(VARIANTS)]
        t, t_all, outs[v], st = run(v)
        times[v].append(t)
        totals[v].append(t_all)
        if st is not None:
            states[v] = st
med = {v: float(np.median(times[v])) for v in VARIANTS}
tot = {v: float(np.median(totals[v])) for v in VARIANTS}
same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
plant_equal = all(same(outs["none"], outs[v]) for v in VARIANTS[1:])
state_equal = same(states["four"], states["host"])
st = states["four"][0]
print(json.dumps({"N": N, "n": n, "steps": K, "repeats": REPEATS, "none_s": round(med["none"], 4), "off_s": round(med["off"], 4),
                  "four_s": round(med["four"], 4), "host_step_s": round(med["host"], 4), "four_total_s": round(tot["four"], 4),
                  "host_total_s": round(tot["host"], 4), "off_over_none": round(med["off"] / med["none"], 3),
                  "four_over_none": round(med["four"] / med["none"], 3), "host_over_four": round(tot["host"] / tot["four"], 2),
                  "step_all_s": {v: [round(t, 4) for t in times[v]] for v in VARIANTS},
                  "total_all_s": {v: [round(t, 4) for t in totals[v]] for v in ("four", "host")},
                  "reactors_detecting": int(np.isfinite(st[:, 12]).any(axis=0).sum()), "alarm_scans": st[:, 9].sum(axis=1).tolist(),
                  "plant_bitwise_equal": bool(plant_equal), "detector_state_bitwise_equal": bool(state_equal)}))
if not (plant_equal and state_equal):
    sys.exit(1)
