"""The fused sensor suite off the 1 s / 30 s grid and on its rare branches, against oracle/sensor_oracle.py.

The method of test_gpu_sensors.py::test_suite_with_physics_vs_oracle: the oracle suite of every reactor is fed the
device's own per-step state, rounded to fp32, and the device's fp64 time, so only the sensor pipeline is compared.
Every case asserts the same things: the NaN pattern and the status and fault streams are equal, the values agree
within |dv| / (1 + |v|) < 2e-5 (the fp32 signal path), and where ``sensor_health()`` is compared the fp64 ageing
accumulators agree to rtol 1e-6, atol 1e-9.  The per-step state comes from one fused call under ``record(1, steps)``;
where it is cheap a second handle makes one-step calls and must show the same bits.  The 1 800 s pH warm-up is not
run through: after ``enable_sensors`` the clock is moved on by 1 800 s (the suite's enable time is copied once, at
enable), so every sensor is warm at the first read and both sensors of a sample line push from then on.

Packing.  The library spreads ensembles as small as these over one wavefront per reactor, so
every multi-reactor test runs twice: spread, under the id it always had, and packed (WT_FULL_WAVES: 64 // n reactors
per wavefront, identity placement, so reactor r is slot r % R of wavefront-group r // R).  "Reactors per wavefront", a
slot's position and the number of sensor passes are properties of the packed case; each case asserts through
``Packing.check`` which of the two it was, and the packed history must equal the spread one bit for bit (mismatches
named as (group, slot)).  The packed case shares the spread case's oracle run when the trajectories have the same bits.

Observed maxima of |dv| / (1 + |v|) on an MI355X are listed in each test's docstring and in DESIGN.md's sensor section
(7.1).  Before the sample lines carried fp64 timestamps the 0.8 s and 2.4 s cases stood at 0.08 and 1.06, and before
the RTD's resistance round trip lost its cancellation the 7.5 s ... 100 s and irregular cases at 2.0e-5 ... 3.3e-5.
"""
import numpy as np
import pytest

import sensor_oracle as SO
from program_helpers import (SENSOR_LINES, SENSOR_NS, both_packings, equals_spread, packing, ragged_size,  # noqa: F401
                             sensor_passes, spread_only)                                                   # (packing: a fixture)

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
BOUND = 2e-5                       # the project's bound on the fp32 signal path (test_gpu_sensors.py)
WARM = 1800.0
CIRCUIT = {SO.FL_OPEN_CIRCUIT: "open_circuit", SO.FL_SHORT_CIRCUIT: "short_circuit", SO.FL_POWER_LOW: "power_low",
           SO.FL_POWER_HIGH: "power_high"}


# ---------------------------------------------------------------- the oracle side, with the sample lines traced
class TracedLine(SO.SampleLine):
    """The oracle's sample line, recording for every transport who pushed, the absolute push index of the winner (what
    the device keeps as its cursor) and whether the pushed value moved against the same sensor's previous push by more
    than ten times the comparison bound."""

    def __init__(self):
        super().__init__()
        self.pushes, self.reader, self.last_pushed, self.trace = 0, -1, {}, []

    def transport_sample(self, value, temp, timestamp):
        out = super().transport_sample(value, temp, timestamp)
        self.pushes += 1
        target = timestamp - self.transport_delay_s
        d = [abs(s[0] - target) for s in self.buf]
        winner = self.pushes - len(d) + d.index(min(d))              # (the scan's strict < keeps the first of the minima)
        before = self.last_pushed.get(self.reader)
        moved = before is not None and abs(value - before) > 10.0 * BOUND * (1.0 + abs(value))
        self.last_pushed[self.reader] = value
        self.trace.append((self.reader, winner, moved))
        return out


class TracedSuite(SO.SensorSuite):
    def __init__(self, *a):
        super().__init__(*a)
        self.lines = (TracedLine(), TracedLine())

    def _base_read(self, i, st, t):
        line = self.sensors[i]["line"]
        if line is not None:
            self.lines[line].reader = i
        return super()._base_read(i, st, t)


def oracle_reads(suites, traj, first=0):
    """Records first .. of ``traj`` through the suites: (values, status, fault), (records, 7, N) each."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    pH0, pHN, Cl0, ClN = f32(traj.pH[:, :, 0]), f32(traj.pH[:, :, -1]), f32(traj.chlorine[:, :, 0]), f32(traj.chlorine[:, :, -1])
    T0, TN, flow = f32(traj.temperature[:, :, 0]), f32(traj.temperature[:, :, -1]), f32(traj.flow_rate)
    K, N = traj.time.shape
    ov = np.empty((K - first, 7, N)); os_ = np.empty((K - first, 7, N), dtype=np.uint8); of = np.empty_like(os_)
    for k in range(first, K):
        for r, suite in enumerate(suites):
            v, s, f = suite.read_all({0: float(pH0[k, r]), -1: float(pHN[k, r])}, {0: float(Cl0[k, r]), -1: float(ClN[k, r])},
                                     {0: float(T0[k, r]), -1: float(TN[k, r])}, float(flow[k, r]), float(traj.time[k, r]))
            ov[k - first, :, r], os_[k - first, :, r], of[k - first, :, r] = v, s, f
    return ov, os_, of


def compare(label, dev, ref):
    """NaN pattern, status and fault streams equal; values within BOUND.  Prints and returns the observed maximum."""
    (hv, hs, hf), (ov, os_, of) = dev, ref
    same_nan = np.array_equal(np.isnan(hv), np.isnan(ov))
    ok = ~np.isnan(ov) & ~np.isnan(hv)
    err = np.where(ok, np.abs(hv - ov) / (1.0 + np.abs(ov)), 0.0)
    k, i, r = np.unravel_index(np.argmax(err), err.shape)
    worst = float(err[k, i, r])
    print(f"{label}: max |dv| / (1 + |v|) = {worst:.3e} ({SO.SENSOR_NAMES[i]} of reactor {r} at read {k}: {hv[k, i, r]:.6f} against {ov[k, i, r]:.6f}) "
          f"over {int(ok.sum())} finite reads, {int((err >= BOUND).sum())} beyond the bound; status differs at {int((hs != os_).sum())}, "
          f"fault at {int((hf != of).sum())} reads")
    assert same_nan, label
    assert np.array_equal(hs, os_) and np.array_equal(hf, of), label
    assert worst < BOUND, label
    return worst


def compare_health(label, ens, suites):
    """sensor_health() against the oracle's fields: times, status and fault equal, the fp64 ageing accumulators to
    rtol 1e-6 / atol 1e-9 (as test_gpu_service.py)."""
    import service_ref as SR
    dev = ens.sensor_health()
    ref = np.stack([SR.health(s) for s in suites], axis=2)                   # (7, 8, N)
    assert np.array_equal(dev["cal_time"], ref[:, 1]) and np.array_equal(dev["power_on"], ref[:, 2]), label
    assert np.array_equal(dev["status"], ref[:, 6]) and np.array_equal(dev["fault"], ref[:, 7]), label
    slow_d, slow_r = np.stack([dev["slow0"], dev["slow1"], dev["slow2"]]), np.stack([ref[:, 3], ref[:, 4], ref[:, 5]])
    gap = np.abs(slow_d - slow_r) / (1e-9 + 1e-6 * np.abs(slow_r))
    print(f"{label}: ageing accumulators at most {float(gap.max()):.1e} of their tolerance (rtol 1e-6, atol 1e-9)")
    assert np.allclose(slow_d, slow_r, rtol=1e-6, atol=1e-9), label


# ---------------------------------------------------------------- the device side
def moving_plant(wt, n, N):
    """A plant whose line signals move at every step size from 0.1 s to 100 s: strong acid dosing into zone 0 (pH of zone
    0 falls through the carbonate buffer), an acid interior next to a neutral last zone (the outlet pH follows by mixing),
    chlorine dosing, a 22 degC temperature gradient over the height with the inlet 8 degC off the tank (the sign of
    both alternates from reactor to reactor).  No reactor raises or clamps (checked on the recorded status)."""
    cols, bc = wt.make_ensemble(N)
    bc = bc.copy()
    sign = np.where(np.arange(N) % 2 == 1, 1.0, -1.0)
    bc[4], bc[5], bc[6] = 2.0, 2.0, 1.0                                 # acid flow [L/min] and concentration [mol/L], chlorine flow
    bc[3] = cols["temperature"] + 8.0 * sign
    pH = np.full((N, n), 3.0)
    pH[:, 0] = 8.0 if n > 2 else 3.0
    pH[:, -1] = 7.6
    T = 20.0 + 11.0 * np.linspace(-1.0, 1.0, n)[None, :] * sign[:, None]
    Cl = np.repeat(cols["initial_chlorine"][:, None], n, axis=1)
    return cols, bc, (pH, Cl, T)


def quiet_plant(wt, n, N):
    """make_ensemble's population as it is (the plant of test_gpu_sensors.py and test_gpu_service.py)."""
    cols, bc = wt.make_ensemble(N)
    rep = lambda k: np.repeat(cols[k][:, None], n, axis=1)
    return cols, bc, (rep("initial_pH"), rep("initial_chlorine"), rep("temperature"))


def open_warm(wt, n, plant, base, history, seed=SEED, packing=None):
    """An ensemble with the suite enabled at t = 0 and the clock then moved on by WARM, recording every step."""
    cols, bc, (pH, Cl, T) = plant
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    if packing is not None:
        packing.place(ens)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=seed, reactor_base=base, history=history)
    ens.set_state(pH, Cl, T, np.array(ens.state.time) + WARM)
    ens.record(1, history)
    return ens


def suites_of(plant, base, seed=SEED):
    cols = plant[0]
    return [TracedSuite(float(cols["flow_rate"][r]), float(cols["initial_chlorine"][r]), float(cols["temperature"][r]), 0.0, seed, base + r)
            for r in range(len(cols["flow_rate"]))]


def history_of(ens, steps):
    hv, hs, hf, nf = ens.sensor_history()
    assert np.all(nf == steps)
    return hv[:steps].astype(np.float64), hs[:steps], hf[:steps]


def run_calls(wt, n, plant, base, calls, one_step=False, packing=None):
    """``calls``: (steps, dt) pairs, one fused call each (one_step: one call per step).  Returns the open handle, the
    trajectory and the history.  ``packing``: places the ensemble and asserts its wavefront-groups after the last step."""
    steps = sum(k for k, _ in calls)
    ens = open_warm(wt, n, plant, base, steps, packing=packing)
    for k, dt in calls:
        if one_step:
            for _ in range(k):
                ens.step(dt, n_steps=1, download=False)
        else:
            ens.step(dt, n_steps=k, download=False)
    traj = ens.trajectory()
    assert len(traj) == steps and not traj.status.any()
    if packing is not None:
        packing.check(ens)
    return ens, traj, history_of(ens, steps)


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def health_arrays(ens):
    """sensor_health() as a tuple of (7, N) arrays, in the order of its keys."""
    health = ens.sensor_health()
    return tuple(np.asarray(health[k]) for k in sorted(health))


TRAJ_FIELDS = ("time", "pH", "chlorine", "temperature", "flow_rate", "status")
_ORACLE = {}


def oracle_of(key, plant, base, traj):
    """(suites after the run, oracle_reads) of ``traj``, computed once per ``key`` and trajectory: the packed case of a
    test records the bits of the spread case's trajectory and then shares its oracle run.  A trajectory with other bits
    gets an oracle run of its own (and the packed case then fails where it compares itself with the spread one)."""
    bits = tuple(np.asarray(getattr(traj, f)).tobytes() for f in TRAJ_FIELDS)
    if key not in _ORACLE or _ORACLE[key][0] != bits:
        suites = suites_of(plant, base)
        ref = oracle_reads(suites, traj)
        for a in ref:
            a.setflags(write=False)
        _ORACLE[key] = (bits, suites, ref)
    return _ORACLE[key][1:]




def line_report(suites):
    """Over all suites: the share of pushes that moved by more than ten times the bound, for the pH electrodes and for
    the RTDs, and the largest advance of a line's winner between two transports, by the kind of sensor that read."""
    moved = {"pH": [], "T": []}
    jump = {"pH": 0, "T": 0}
    for s in suites:
        for line in s.lines:
            seen = set()
            for k, (reader, winner, mv) in enumerate(line.trace):
                kind = "pH" if reader in (SO.S_PH_IN, SO.S_PH_OUT) else "T"
                if reader in seen:                                   # (a sensor's first push has no predecessor)
                    moved[kind].append(mv)
                seen.add(reader)
                if k > 0:
                    jump[kind] = max(jump[kind], winner - line.trace[k - 1][1])
    share = {k: float(np.mean(v)) if v else 0.0 for k, v in moved.items()}
    return share, jump


# ---------------------------------------------------------------- A. the sample line off the grid
SHAPES = [(2, 33), (8, 9), (20, 4)]
OFF_GRID = [(0.1, 250), (0.8, 150), (2.4, 150), (7.5, 40), (45.0, 24), (100.0, 16)]


@both_packings("dt,steps,n,N", [g + s for g in OFF_GRID for s in SHAPES])
def test_sample_line_off_the_grid(gpu, wt, monkeypatch, dt, steps, n, N, packing):
    """Packed: 32, 8 and 3 reactors per wavefront with a partial last one that holds one reactor, four sensor passes at
    n = 2 and one at n = 8 and 20.  Spread (the library's own choice for ensembles this small): a wavefront per reactor
    on a card with more wavefront slots than reactors, one sensor pass each.  Every reactor compared; the packed history
    equals the spread one bit for bit.
    0.1 s: the 100-entry ring is shorter than the 30 s delay, the winner is the oldest entry held and the ring wraps;
    0.8 s and 2.4 s: 30 / dt is a half-integer, two timestamps lie at (nearly) the same distance from t - 30 and the
    reference's fp64 rounding settles which wins; 7.5 s: an exact hit four timestamps back; 45 s: the previous
    timestamp; 100 s: the entry just pushed.  The oracle's trajectory shows that more than half of the pushes of the pH
    electrodes and of the RTDs differ from the sensor's previous push by more than ten times the bound, so a sample
    from a neighbouring timestamp does not pass.  One fused call and a loop of one-step calls: the same bits.

    Observed on an MI355X (max |dv| / (1 + |v|), the largest of the three shapes): 0.1 s 4.1e-7, 0.8 s 4.9e-7, 2.4 s 3.7e-7,
    7.5 s 3.0e-7, 45 s 3.7e-7, 100 s 2.7e-7; pushes moving by more than ten times the bound: pH >= 0.98, RTD >= 0.62."""
    plant = moving_plant(wt, n, N)

    def fused(packing):
        ens, traj, dev = run_calls(wt, n, plant, 0, [(steps, dt)], packing=packing)
        ens.close()
        return traj, dev
    traj, dev = fused(packing)
    ens1, traj1, dev1 = run_calls(wt, n, plant, 0, [(steps, dt)], one_step=True, packing=packing)
    ens1.close()
    suites, ref = oracle_of(("off-grid", n, N, dt), plant, 0, traj)
    share, jump = line_report(suites)
    print(f"n = {n}, N = {N}, dt = {dt}: pushes moving by > 10 x bound: pH {share['pH']:.2f}, RTD {share['T']:.2f}; largest advance of a winner {jump}")
    assert share["pH"] >= 0.5 and share["T"] >= 0.5
    compare(f"off-grid n = {n} N = {N} dt = {dt}", dev, ref)
    assert same_bits(dev, dev1) and np.array_equal(traj.pH, traj1.pH) and np.array_equal(traj.time, traj1.time)
    equals_spread(monkeypatch, packing, ("off-grid", n, N, dt), n, dev, lambda p: fused(p)[1])


IRREGULAR = [(3, 45.0), (60, 0.1), (1, 20.0), (10, 1.0), (40, 0.8), (2, 100.0), (30, 0.3)]
PH_OUTLET_DIES_EARLY = 1831        # tools/sensor_event_scan.py --t0 1800 --dt 45 --reads 3 --count 6000: power_low on pH_outlet at read 1


IRREGULAR_SHAPES = [(8, 9, 3), (2, 33, 32)]
# packed only: a middle slot of a full wavefront at n = 2 (four passes), and at n = 6 a slot whose outlet RTD lane runs in
# the pass after its pH partner's, beside slots (0 ... 3) whose RTD shares the partner's pass
IRREGULAR_PACKED = IRREGULAR_SHAPES + [(2, 33, 17), (6, 21, 5)]


@both_packings("n,N,slot", IRREGULAR_SHAPES, packed=IRREGULAR_PACKED)
def test_sample_line_irregular_calls(gpu, wt, monkeypatch, n, N, slot, packing):
    """Reactor ``slot`` is the one whose pH_outlet dies.  Packed it sits in a middle slot of a full wavefront with live
    neighbours on both sides (8-9-3, 2-33-17, 6-21-5) or alone in the partial second wavefront (2-33-32); spread, on a
    card with more wavefront slots than reactors, every reactor has a wavefront to itself and the slot says nothing.
    Calls of different step sizes on one handle: 3 x 45 s, 60 x 0.1 s, one of 20 s, 10 x 1 s, 40 x 0.8 s, 2 x 100 s,
    30 x 0.3 s.  (The long steps first: the reads after a change of step size are RATE_FAULTs -- the delivered sample
    jumps by 45 s of signal within 0.1 s -- and such a read skips the circuit draw, so only an event before the first
    change is met for certain.)  After the stretch of 0.1 s steps the target sweeps over many entries per read, so the device's walk
    leaves the four entries it fetched up front; one reactor's pH_outlet sits in POWER_FAULT from its second read on, so
    on its outlet line the RTD walks alone (and takes its entries from memory, not from the pH lane's hand-off).  The
    oracle's trace shows a winner advancing by more than four entries for a pH electrode and for an RTD (78 and 39).
    Observed: 3.5e-7 (n = 8), 6.6e-7 (n = 2)."""
    plant = moving_plant(wt, n, N)
    base = PH_OUTLET_DIES_EARLY - slot
    R = 64 // n
    if packing.packed:                                  # where the dying electrode really sits
        assert (0 < slot % R < R - 1 and slot < R) or (slot == R and N == R + 1), (n, N, slot)
        assert n != 6 or (slot in sensor_passes(6).split[1] and 0 not in sensor_passes(6).split[1])

    def run(packing):
        ens, traj, dev = run_calls(wt, n, plant, base, IRREGULAR, packing=packing)
        ens.close()
        return traj, dev
    traj, dev = run(packing)
    suites, ref = oracle_of(("irregular", n, N, slot), plant, base, traj)
    share, jump = line_report(suites)
    print(f"irregular n = {n}, N = {N}: pushes moving {share}, largest advance of a winner {jump}")
    assert ref[2][1, SO.S_PH_OUT, slot] == SO.FL_POWER_LOW and np.isfinite(ref[0][-1, SO.S_T_OUT, slot])
    assert jump["pH"] > 4 and jump["T"] > 4
    compare(f"irregular n = {n} N = {N}", dev, ref)
    equals_spread(monkeypatch, packing, ("irregular", n, N, slot), n, dev, lambda p: run(p)[1])


# ---------------------------------------------------------------- B. rare faults from the random stream
# tools/sensor_event_scan.py --seed 0xC0FFEE --t0 1800 --dt 30 --reads 160 --first 0 --count 600 lists these (reactor,
# sensor, fault, read); tests/test_sensor_oracle.py holds the tool to this list.
EVENTS = [(141, SO.S_PH_IN, "power_high", 5, "pH"), (581, SO.S_PH_OUT, "power_low", 15, "pH"), (340, SO.S_PH_OUT, "short_circuit", 8, "pH"),
          (208, SO.S_PH_OUT, "open_circuit", 31, "pH"), (168, SO.S_T_IN, "power_low", 15, "rtd"), (168, SO.S_CL_OUT, "open_circuit", 27, "single"),
          (506, SO.S_T_IN, "open_circuit", 1, "rtd"), (540, SO.S_T_OUT, "short_circuit", 25, "rtd"), (68, SO.S_T_IN, "power_high", 87, "rtd"),
          (348, SO.S_FLOW, "power_low", 6, "single"), (552, SO.S_CL_OUT, "power_high", 5, "single"), (251, SO.S_FLOW, "short_circuit", 14, "single")]
# The position of an event: "pH" -- on a line's first sensor, the RTD of the line alive at that read; "rtd" -- on the RTD,
# the pH electrode alive; "single" -- on a sensor without a line.  Every fault in every position:
POSITIONS = {"pH": (SO.S_PH_IN, SO.S_PH_OUT), "rtd": (SO.S_T_IN, SO.S_T_OUT), "single": (SO.S_CL_IN, SO.S_CL_OUT, SO.S_FLOW)}
assert {(e[4], e[2]) for e in EVENTS} == {(p, f) for p in POSITIONS for f in CIRCUIT.values()} and all(e[1] in POSITIONS[e[4]] for e in EVENTS)
# (reactor, n, N, slot, steps).  In the packed cases: first and last slot of a wavefront (n = 8: 8 reactors, n = 2: 32,
# n = 20: 3), the first slot of a partial second wavefront; at n = 2 the sensors of a reactor spread over four passes of
# the wavefront (``fault_position`` asserts it from R and the slot).  Spread, a reactor has a wavefront to itself.
FAULT_RUNS = [(141, 2, 33, 31, 20), (581, 8, 9, 0, 28), (340, 20, 4, 2, 20), (208, 8, 9, 8, 44), (168, 2, 33, 32, 40),
              (506, 8, 9, 7, 14), (540, 2, 33, 0, 38), (68, 8, 9, 0, 100), (348, 20, 4, 0, 18), (552, 8, 9, 8, 18),
              (251, 8, 9, 7, 26)]
PARTNER = {SO.S_PH_IN: SO.S_T_IN, SO.S_PH_OUT: SO.S_T_OUT, SO.S_T_IN: SO.S_PH_IN, SO.S_T_OUT: SO.S_PH_OUT}


def fault_position(n, N, slot):
    """Where ``slot`` lies once the N reactors are packed 64 // n to a wavefront."""
    R = 64 // n
    assert N == R + 1 and 0 <= slot < N, (n, N, slot)
    return "lone" if slot == R else "first" if slot == 0 else "last" if slot == R - 1 else "middle"


assert [fault_position(n, N, slot) for _, n, N, slot, _ in FAULT_RUNS] == ["last", "first", "last", "lone", "lone", "last", "first", "first",
                                                                            "first", "lone", "last"]


@both_packings("reactor,n,N,slot,steps", FAULT_RUNS)
def test_rare_faults_vs_oracle(gpu, wt, monkeypatch, reactor, n, N, slot, steps, packing):
    """A reactor whose stream draws a power fault or an open / short circuit within the run (EVENTS), in a small ensemble
    with ``reactor_base = reactor - slot``; steps of 30 s, the whole ensemble compared, sensor_health() included.
    Packed, the reactor is the first or the last of a full wavefront beside live neighbours, or the lone one of the
    second wavefront (``fault_position``); spread, every reactor of these ensembles has its own wavefront.  The packed
    history and sensor_health() equal the spread run's bit for bit.  The
    reads after the event run the sticky POWER_FAULT return of read_begin, the NaN that feeds back through the lag, and
    a sample line with one sensor of the pair dead and the other pushing on.  The oracle's run contains the reactor's
    events of the list at their reads, the other sensor of the line alive; the list holds every fault in every position.
    Observed: at most 3.8e-7 over the eleven runs; the ageing accumulators equal to the digits compared."""
    plant = quiet_plant(wt, n, N)
    base = reactor - slot
    assert fault_position(n, N, slot) in ("first", "last", "lone")

    def run(packing):
        ens, traj, dev = run_calls(wt, n, plant, base, [(steps, 30.0)], packing=packing)
        return ens, traj, dev + health_arrays(ens)
    ens, traj, got = run(packing)
    dev = got[:3]
    suites, ref = oracle_of(("faults", reactor), plant, base, traj)
    mine = [e for e in EVENTS if e[0] == reactor]
    assert mine
    for _, i, name, k, _ in mine:                                       # (a condition on the oracle's run, not on the device)
        assert k < steps and CIRCUIT.get(ref[2][k, i, slot]) == name and (k == 0 or ref[2][k - 1, i, slot] == SO.FL_NONE), (i, name, k)
        assert i not in PARTNER or np.isfinite(ref[0][k, PARTNER[i], slot]), (i, name, k)
    compare(f"faults reactor {reactor} n = {n} N = {N} slot {slot}", dev, ref)
    compare_health(f"faults reactor {reactor}", ens, suites)
    ens.close()

    def twin(p):
        e, _, g = run(p)
        e.close()
        return g
    equals_spread(monkeypatch, packing, ("faults", reactor), n, got, twin)


# ---------------------------------------------------------------- C. deterministic statuses by host edits
def chlorine_for(reading, pH0, offset):
    """The chlorine concentration at which the inlet analyser settles at ``reading``: reading = Cl * (0.5 + 0.5 * HOCl
    fraction at pH0) + calibration offset (chlorine_sensor.py:189-227, base_sensor.py:612-626)."""
    ratio = 10.0 ** (7.5 - pH0)
    return (reading - offset) / (0.5 + 0.5 * ratio / (1.0 + ratio))


def test_statuses_by_host_edits(gpu, wt, monkeypatch):
    """The spread case of ``statuses_by_host_edits``: the library's own dealing of nine reactors (a wavefront each on a
    card with more wavefront slots than that)."""
    statuses_by_host_edits(wt, monkeypatch, spread_only(monkeypatch))


@pytest.mark.parametrize("packing", ["packed"], indirect=True)
def test_statuses_by_host_edits_packed(gpu, wt, monkeypatch, packing):
    """One full wavefront of eight reactors and a lone ninth: the edited reactors are slots 1 and 4 of the first, beside
    reactors that keep their state, and the lone one.  The histories equal the spread run's bit for bit."""
    statuses_by_host_edits(wt, monkeypatch, packing)


def statuses_by_host_edits(wt, monkeypatch, packing):
    """dt = 1 s, 9 reactors of 8 zones, three of them edited with set_state between calls and set back a few steps
    later: pH up by 2 (the electrodes answer 30 s later, through the sample line, with RATE_FAULT on the rise and on the
    fall), chlorine to where the amperometric analyser settles at 10.5 mg/L of its 0 .. 10 range (SATURATED), chlorine
    to where it settles at 14 mg/L (OUT_OF_RANGE beyond 11).  The oracle shows the three statuses on the edited reactors
    and NORMAL again after each; a twin run that makes the same calls with its own state shows the bits of the
    reactors that were not edited.  Observed: 2.9e-7."""
    n, N = 8, 9
    edited = np.array([1, 4, 8])
    kept = np.setdiff1d(np.arange(N), edited)
    cols, bc, (pH0, Cl0, T0) = quiet_plant(wt, n, N)
    # (an analyser calibrated against more than 1 mg/L from its zero reading carries an offset of a tenth of its span and
    # shows DRIFT_WARNING in place of NORMAL and of SATURATED: the edited reactors start below that)
    cols = dict(cols, initial_chlorine=np.where(np.isin(np.arange(N), edited), 0.5 + 0.04 * np.arange(N), cols["initial_chlorine"]))
    plant = (cols, bc, (pH0, np.repeat(cols["initial_chlorine"][:, None], n, axis=1), T0))
    # (steps before the edit, the edit, steps it is held, steps after it is set back)
    script = [(3, "pH", 3, 40), (2, "saturate", 6, 10), (2, "out_of_range", 6, 12)]
    total = sum(a + b + c for a, _, b, c in script)

    def run(packing):
        runs = {}
        for name in ("edited", "twin"):
            ens = open_warm(wt, n, plant, 0, total, packing=packing)
            for before, what, held, after in script:
                ens.step(1.0, n_steps=before, download=False)
                s = ens.state
                pH, Cl = s.pH.copy(), s.chlorine.copy()
                if name == "edited":
                    if what == "pH":
                        pH[edited] += 2.0
                    else:
                        offset = cols["initial_chlorine"][edited]                    # calibrated against it from a zero reading
                        Cl[edited] = chlorine_for(10.5 if what == "saturate" else 14.0, s.pH[edited, 0], offset)[:, None]
                ens.set_state(pH, Cl, s.temperature)
                ens.step(1.0, n_steps=held, download=False)
                h = ens.state
                if name == "edited":                                                 # back: the edited field as it was, the rest as it is
                    pH, Cl = h.pH.copy(), h.chlorine.copy()
                    if what == "pH":
                        pH[edited] = s.pH[edited]
                    else:
                        Cl[edited] = s.chlorine[edited]
                    ens.set_state(pH, Cl, h.temperature)
                else:
                    ens.set_state(h.pH, h.chlorine, h.temperature)
                ens.step(1.0, n_steps=after, download=False)
            traj = ens.trajectory()
            assert len(traj) == total and not traj.status.any()
            runs[name] = (traj, history_of(ens, total))
            packing.check(ens)
            ens.close()
        return runs
    runs = run(packing)
    traj, dev = runs["edited"]
    suites, ref = oracle_of("host edits", plant, 0, traj)
    ov, os_, of = ref
    marks = np.cumsum([0] + [a + b + c for a, _, b, c in script])
    for r in edited:
        alive = [i for i in (SO.S_PH_IN, SO.S_PH_OUT) if np.isfinite(ov[marks[1] - 1, i, r])]
        assert alive
        for i in alive:
            seg = os_[marks[0]:marks[1], i, r]
            assert (seg == SO.ST_RATE_FAULT).sum() >= 2 and seg[-1] == SO.ST_NORMAL, (r, i, seg)
        if np.isfinite(ov[-1, SO.S_CL_IN, r]):
            sat, oor = os_[marks[1]:marks[2], SO.S_CL_IN, r], os_[marks[2]:marks[3], SO.S_CL_IN, r]
            assert (sat == SO.ST_SATURATED).any() and not (sat == SO.ST_OUT_OF_RANGE).any() and sat[-1] == SO.ST_NORMAL, (r, sat)
            assert (oor == SO.ST_OUT_OF_RANGE).any() and (of[marks[2]:marks[3], SO.S_CL_IN, r] == SO.FL_OUT_OF_RANGE).any(), (r, oor)
            assert oor[-1] == SO.ST_NORMAL, (r, oor)
    assert np.isfinite(ov[-1, SO.S_CL_IN, edited]).any()
    compare("host edits", dev, ref)
    twin = runs["twin"][1]
    assert all(np.array_equal(a[:, :, kept], b[:, :, kept], equal_nan=True) for a, b in zip(dev, twin))
    assert not same_bits(dev, twin)
    both = lambda runs: runs["edited"][1] + runs["twin"][1]
    equals_spread(monkeypatch, packing, "host edits", n, both(runs), lambda p: both(run(p)))


# ---------------------------------------------------------------- E. every pass structure of a packed wavefront
PASS_STEPS, PASS_DT = 40, 0.8


@pytest.mark.parametrize("n", SENSOR_NS)
def test_every_pass_structure_vs_oracle(gpu, wt, monkeypatch, n, packing):
    """``moving_plant``, three full wavefronts of R = 64 // n reactors and a lone one, one fused call of 40 steps of 0.8 s
    (30 / dt is a half-integer: the line's winner hangs on the last bits), every reactor against the oracle.  Packed,
    the suite runs in the pass structure of ``sensor_passes(n)``: four aligned passes at n = 2 and two at n = 4, a pass
    boundary inside the DPD analyser's and the outlet RTD's runs at n = 3, inside the inlet RTD's at n = 5 (slots 4 ... 11
    take their line a pass after the pH lane left it) and inside the outlet RTD's at n = 6, one pass of 56 ... 14 lanes
    from n = 8 on; spread, one pass of seven lanes per reactor.  The oracle's trace shows that the pH electrode and the
    RTD of both lines transported in every slot (those behind a pass boundary among them), that winners advanced and
    that more than half of the pushes moved by more than ten times the bound.  Packed equals spread bit for bit,
    sensor_health() included."""
    R, N = ragged_size(n, 3)
    plant = moving_plant(wt, n, N)

    def run(packing):
        ens, traj, dev = run_calls(wt, n, plant, 0, [(PASS_STEPS, PASS_DT)], packing=packing)
        return ens, traj, dev + health_arrays(ens)
    ens, traj, got = run(packing)
    suites, ref = oracle_of(("passes", n), plant, 0, traj)
    share, jump = line_report(suites)
    print(f"passes n = {n}, N = {N}: pushes moving by > 10 x bound: pH {share['pH']:.2f}, RTD {share['T']:.2f}; largest advance of a winner {jump}")
    assert share["pH"] >= 0.5 and share["T"] >= 0.5
    assert jump["pH"] >= 1                                   # (an RTD reads just after its pH partner moved the winner on)
    p = sensor_passes(n)
    assert (p.R, N) == (R, 3 * R + 1)
    # transports per (sensor of a line, reactor): a sensor pushes at every read unless its stream draws a fault (a few
    # in ten thousand reads), so nine in ten pushed at all forty, on the whole and behind a pass boundary
    pushes = {i: np.array([sum(1 for reader, _, _ in s.lines[line].trace if reader == i) for s in suites])
              for line, pair in enumerate(SENSOR_LINES) for i in pair}
    for i, cnt in pushes.items():
        assert np.mean(cnt == PASS_STEPS) >= 0.9, (n, i, cnt.tolist())
    far = {i: [r for r in range(N) if r % R >= slot] for i, slot in p.cuts.items() if i >= 5}
    assert {i: len(rs) for i, rs in far.items()} == {3: {6: 3 * 19}, 5: {5: 3 * 8}, 6: {6: 3 * 6}}.get(n, {})
    for i, rs in far.items():
        assert np.mean(pushes[i][rs] == PASS_STEPS) >= 0.9 and np.isfinite(ref[0][-1, i, rs]).mean() >= 0.9, (n, i, pushes[i][rs].tolist())
    compare(f"passes n = {n} N = {N}", got[:3], ref)
    compare_health(f"passes n = {n}", ens, suites)
    ens.close()

    def twin(pk):
        e, _, g = run(pk)
        e.close()
        return g
    equals_spread(monkeypatch, packing, ("passes", n), n, got, twin)


# ---------------------------------------------------------------- D. the long horizon
LONG_REACTOR = 3                   # tools/sensor_event_scan.py --dt 3600 --reads 700: no event on pH_inlet or the DPD analyser


def test_long_horizon_ageing(gpu, wt):
    """One reactor of 4 zones, 700 steps of 3 600 s (29 days) under chlorine dosing: pH fouling crosses 0.05 after 25 days
    and takes the exponential branch of its bio term, the slope error and the reference contamination grow, the DPD
    reagent loses potency, the membrane ages, and every calibration expires after 24 h.  Readings and sensor_health()
    against the oracle.  The 700 steps take 2.5 s, oracle included, so the step stays 3 600 s.  Observed: 2.2e-7; fouling
    0.268, potency 0.607, membrane age 29.1 d at the end."""
    steps, dt = 700, 3600.0
    cfg = wt.ReactorConfiguration(n_zones=4, initial_pH=7.2)
    cols = {k: np.array([getattr(cfg, k)]) for k in ("flow_rate", "initial_chlorine", "temperature", "initial_pH")}
    ens = wt.ReactorEnsemble([cfg])
    ens.set_boundary(wt.BoundaryConditions(inlet_flow_rate=5.0, inlet_pH=7.5, chlorine_flow_rate=0.3, inlet_temperature=24.0))
    ens.enable_sensors(seed=SEED, reactor_base=LONG_REACTOR, history=steps)
    ens.record(1, steps)
    ens.step(dt, n_steps=steps, download=False)
    traj = ens.trajectory()
    assert len(traj) == steps and not traj.status.any()
    dev = history_of(ens, steps)
    suites = suites_of((cols,), LONG_REACTOR)
    fouling = np.empty(steps); potency = np.empty(steps)
    ov = np.empty((steps, 7, 1)); os_ = np.empty((steps, 7, 1), dtype=np.uint8); of = np.empty_like(os_)
    for k in range(steps):                                              # (read by read: the oracle's ageing fields after every read)
        one = type(traj)(*(getattr(traj, f)[k:k + 1] for f in ("time", "pH", "chlorine", "temperature", "flow_rate", "status")))
        ov[k:k + 1], os_[k:k + 1], of[k:k + 1] = oracle_reads(suites, one)
        fouling[k], potency[k] = suites[0].sensors[SO.S_PH_IN]["fouling"], suites[0].sensors[SO.S_CL_OUT]["potency"]
    assert ((fouling > 0.05) & np.isfinite(ov[:, SO.S_PH_IN, 0])).sum() >= 50
    assert (os_[:, SO.S_PH_IN, 0] == SO.ST_CAL_EXPIRED).any() and (os_[:, SO.S_CL_OUT, 0] == SO.ST_CAL_EXPIRED).any()
    assert potency[-1] < 0.9 and np.isfinite(ov[-1, SO.S_CL_OUT, 0]) and np.isfinite(ov[-1, SO.S_PH_IN, 0])
    print(f"long horizon: fouling {fouling[-1]:.4f}, potency {potency[-1]:.4f}, membrane age {suites[0].sensors[SO.S_CL_IN]['membrane_age']:.2f} d")
    compare("long horizon", dev, (ov, os_, of))
    compare_health("long horizon", ens, suites)
    ens.close()
