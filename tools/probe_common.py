"""What the per-reactor program probes (control_, inject_, alarm_, actuator_, disturb_, score_, detect_, trend_probe.py)
share: the command line, the ensemble, the two PI loops and the four-slot injection program drawn from default_rng(3),
the plant with sensors and plant I/O at a scan per step, a run's outputs, the timed step call, the rotation of the
variants over the repeats, and the bitwise comparison.  A probe keeps its variants, its extra programs and its JSON line.
Importing it puts the repository, tests/ and oracle/ on the path, for the restatements a probe compares with."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import numpy as np
wt = importlib.import_module("ics-wt-physicsengine_amd")


def arguments(steps):
    """[N] [n] [steps] of the command line (10 000 x 8 over ``steps`` by default) and make_ensemble(N)'s columns and
    boundary."""
    N, n, K = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 10000), (2, 8), (3, steps)))
    return (N, n, K) + tuple(wt.make_ensemble(N))


def pi_loops(cols, N, rows=4):
    """The chlorine and the acid loop with per-reactor gains, and the (rows, N) uniform draws they take rows 0 to 3 of."""
    u = np.random.default_rng(3).random((rows, N))
    chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + 0.5, kp=0.5 + 1.5 * u[0], ki=1e-3 * u[1], bias=0.2)
    acid = wt.PILoop("pH_outlet", setpoint=7.0 + 0.4 * u[2], kp=0.5, ki=1e-4 + 1e-3 * u[3], direction=-1, bias=0.1)
    return chlorine, acid, u


def injections(u, span):
    """The four-slot injection program over a run of ``span`` seconds (rows 4 and 5 of ``pi_loops(cols, N, 8)``'s draws)."""
    return [wt.Injection("chlorine_outlet", "constant", start=0.25 * span, end=0.5 * span, a=0.0),      # spoofed low
            wt.Injection("pH_outlet", "freeze", start=span * u[4], end=span * u[4] + 0.3 * span),         # frozen probe
            wt.Injection("chlorine_outlet", "bias", start=0.6 * span, a=-0.5 * u[5]),
            wt.Injection("pH_inlet", "fault", start=0.8 * span, a=3)]


def ensemble(cols, bc, n):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    return ens


def plant(cols, bc, n, history=0):
    """Sensors, plant I/O, a scan per step."""
    ens = ensemble(cols, bc, n)
    ens.enable_sensors(seed=1, history=history)
    ens.enable_plant_io()
    ens.set_schedule(0, 1)
    return ens


def outputs(ens, *extra):
    """The state of every reactor and what the getters named in ``extra`` return (a state object gives its block)."""
    es = ens.state
    out = (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status)
    for name in extra:
        x = getattr(ens, name)()
        x = x.block() if hasattr(x, "block") else x
        out += tuple(x) if isinstance(x, tuple) else (x,)
    return out


def timed_step(ens, dt, steps, **kw):
    """One step call between two synchronisations: (its start, its seconds)."""
    ens.synchronize()
    t0 = time.perf_counter()
    ens.step(dt, n_steps=steps, download=False, **kw)
    ens.synchronize()
    return t0, time.perf_counter() - t0


def rotate(variants, repeats, run):
    """Every repeat runs all ``variants``, starting one further along each time.  ``run(variant, rep)`` returns a tuple
    that begins with the seconds.  Returns per variant the list of seconds, their median, and the last run's tuple."""
    times, last = {v: [] for v in variants}, {}
    for rep in range(repeats):
        for i in range(len(variants)):
            v = variants[(i + rep) % len(variants)]
            last[v] = run(v, rep)
            times[v].append(last[v][0])
    return times, {v: float(np.median(t)) for v, t in times.items()}, last


def same(a, b):
    """Two tuples of arrays are bitwise equal (NaN equals NaN)."""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
