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
import json, sys, time
import numpy as np
from probe_common import arguments, injections, outputs, pi_loops, plant, rotate, same, timed_step, wt
from detect_ref import DetectRef
from inject_ref import InjectRef
from program_helpers import HostScan

N, n, K, cols, bc = arguments(120)
DT = 10.0
chlorine, acid, u = pi_loops(cols, N, 8)
program = injections(u, K * DT)
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


def run(variant):
    ens = plant(cols, bc, n, history=K if variant == "host" else 0)
    ens.enable_control(chlorine, acid)
    ens.set_injections(*program)
    if variant in ("off", "four"):
        ens.set_detectors(*(off if variant == "off" else detectors), attack=label)
    t0, t_step = timed_step(ens, DT, K)
    st = None
    if variant == "host":
        vh, _, fh, _ = ens.sensor_history()
        ref = DetectRef(dblock, np.stack(label), np.zeros(N))
        hs = HostScan(N, inj=InjectRef(iblock), det=ref, dt=DT)
        k = -1
        for steps in hs.calls(K, 1):
            k += steps
            hs.scan(vh[k], fh[k])
        st = (ref.st, ref.t_prev)
    elif variant == "four":
        st = ens.detector_state().block()                       # the download the study ends with
    t_all = time.perf_counter() - t0
    out = outputs(ens, "sensor_readings", "input_image", "boundary", "control_state", "injection_state")
    ens.close()
    return t_step, t_all, out, st


run("four")                                      # module load, first launches
VARIANTS, REPEATS = ("none", "off", "four", "host"), 5
totals = {v: [] for v in VARIANTS}


def timed(variant, rep):
    result = run(variant)
    totals[variant].append(result[1])
    return result


times, med, last = rotate(VARIANTS, REPEATS, timed)
tot = {v: float(np.median(t)) for v, t in totals.items()}
plant_equal = all(same(last["none"][2], last[v][2]) for v in VARIANTS[1:])
state_equal = same(last["four"][3], last["host"][3])
st = last["four"][3][0]
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
