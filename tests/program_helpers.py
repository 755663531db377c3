"""Helpers of the GPU tests of the per-reactor scan programs (test_gpu_control.py, test_gpu_inject.py,
test_gpu_alarm.py): a plant with sensors and plant I/O, a pair of PI loops, the plant's observable state, the message
of a refused parameter block."""
import numpy as np

DT, K = 10.0, 300          # 3000 s: the pH sensors' 1800 s warm-up ends inside the run
MASTER = (0.5, 0.25, 6.0)  # acid, chlorine, inlet flow commands the master writes


def plant(wt, cols, bc, n, seed=11, history=0):
    ens = wt.ReactorEnsemble(cols, n_zones=n)
    ens.set_boundary(bc)
    ens.enable_sensors(seed=seed, history=history)
    ens.enable_plant_io()
    return ens


def pi_loops(wt, cols, seed=5):
    """Both loops on, per-reactor gains and setpoints: chlorine dosing on the outlet DPD reading, acid dosing (reverse
    acting: more acid while the pH is above its setpoint) on the outlet pH probe."""
    N = len(cols["initial_chlorine"])
    u = np.random.default_rng(seed).random((6, N))
    chlorine = wt.PILoop("chlorine_outlet", setpoint=cols["initial_chlorine"] + u[0], kp=0.2 + 1.8 * u[1],
                         ki=1e-4 + 2e-3 * u[2], bias=0.2)
    acid = wt.PILoop("pH_outlet", setpoint=6.8 + 0.6 * u[3], kp=0.1 + 0.9 * u[4], ki=1e-4 + 1e-3 * u[5], direction=-1,
                     bias=0.1)
    return chlorine, acid


def plant_state(ens):
    """State, sensor readings and boundary of every reactor."""
    es = ens.state
    v, s, f = ens.sensor_readings()
    return (es.pH, es.chlorine, es.temperature, es.time, es.flow_rate, es.status, v, s, f, ens.boundary())


def refused_as_checked(nat, program, block) -> bool:
    """The message of the set call just refused on ``block`` is the one wt_program_check gives for it."""
    msg = nat.lib().wt_last_error()
    return (nat.lib().wt_program_check(program, nat.dptr(block), block.shape[-1]) == nat.WT_E_ARG
            and nat.lib().wt_last_error() == msg)


def assert_all_equal(ref, got, what):
    for i, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a, b, equal_nan=True), (what, i)
