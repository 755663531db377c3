"""Checkpoint, copy and rewind of a whole ensemble (include/wtphys.h ``wt_ensemble_checkpoint_*``, ``wt_ensemble_copy``,
``wt_ensemble_mark``).  The yardstick throughout: the same further calls on the handle that was never
saved give the same bytes from every getter of the library."""
import ctypes

import numpy as np
import pytest

from checkpoint_helpers import (AFTER, HEADER, SAVE_AT, T_SAVE, both, build, continue_alike, header_of, info_codes,
                                program_params, same, snapshot, with_header)
from program_helpers import DT, instantiation, wavefront_groups

pytestmark = pytest.mark.gpu

#         n   N  train length  WT_FULL_WAVES
CASES = [(4, 33, 3, True), (4, 33, 3, False), (5, 26, 2, False), (8, 17, 0, True), (8, 17, 0, False), (20, 10, 2, False),
         (40, 3, 0, False)]
E_NO_MARK = "rewind: no mark is set (wt_ensemble_mark)"
E_CONSTANTS = "checkpoint_load: the reactor constants differ from the handle's"


def _refused(fn, *args):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    return str(ei.value)


def _warm(wt, n=8, N=17, length=0, seed=0, steps=SAVE_AT, **kw):
    cols, bc = wt.make_ensemble(N, seed=2000 + n + seed)
    ens = build(wt, cols, bc, n, length, **kw)
    ens.step(DT, n_steps=steps, download=False)
    return cols, bc, ens


def _size(ens):
    v = ctypes.c_int64(0)
    assert ens._h and gpu_lib().wt_ensemble_checkpoint_size(ens._h, ctypes.byref(v)) == 0
    return v.value


def gpu_lib():
    from program_helpers import _native
    return _native.lib()


# ---- 1. continuation with everything in flight
@pytest.mark.parametrize("n, N, length, full", CASES, ids=lambda v: str(v))
def test_continuation_with_everything_in_flight(gpu, wt, monkeypatch, n, N, length, full):
    if full:
        monkeypatch.setenv("WT_FULL_WAVES", "1")
    programs = n <= 32
    assert [instantiation(k) for k in (4, 5, 20, 40)] == [(2, True), (3, False), (5, False), (6, False)]
    cols, bc, a = _warm(wt, n, N, length, programs=programs)
    if (n, full) == (4, True):
        assert a.train_state().per_wavefront == 15         # wavefronts of 15, 15 and 3 reactors
    if programs:      # in flight at the save: the latched alarm has not tripped, the store and the history have wrapped
        assert not a.alarm_state().active[0].any() and (a.trend_state().n_recorded[0] > 16).all()
        assert a.injection_state().n_applied[:2].all() and np.isnan(a.injection_state().t_first[2]).all()
        assert (a.sensor_history()[3] >= 64).all() and len(a.trajectory()) == SAVE_AT // 3
    blob = a.checkpoint()
    b = wt.ReactorEnsemble(cols, n_zones=n)
    b.restore(blob)
    both((n, N, "after the load"), a, b)
    rng = np.random.default_rng(n)
    for i, k in enumerate(AFTER):
        if programs:
            cmd = rng.uniform(0.1, 0.9, (3, N)) * np.array([[2.0], [1.0], [8.0]])
            for ens in (a, b):
                ens.write_commands(*cmd) if i == 0 else ens.reset_alarms()
            both((n, N, "host call", i), a, b)
        continue_alike((n, N, "steps", i), a, b, steps=(k,))
    if programs:
        assert a.alarm_state().active[0].any() and a.injection_state().n_applied[2].all()
        assert len(a.trajectory()) == 80 and a.score_state().n_eval[0].all()
        if length:
            assert a.pipe_state().n_sent.max() > SAVE_AT and a.wire_state().n_routed.any()
    assert wavefront_groups(a) == wavefront_groups(b)
    a.close(); b.close()


# ---- 2. the packing is not in the blob
@pytest.mark.parametrize("saved_full", [True, False])
def test_the_packing_is_not_in_the_blob(gpu, wt, monkeypatch, saved_full):
    def make(full):
        monkeypatch.setenv("WT_FULL_WAVES", "1" if full else "0")
        return _warm(wt, 4, 33, 3, steps=SAVE_AT if full == saved_full else 0)
    cols, bc, a = make(saved_full)
    _, _, b = make(not saved_full)
    b.restore(a.checkpoint())
    assert a.train_state().per_wavefront != b.train_state().per_wavefront
    both("after the load", a, b, layout=False)
    continue_alike("other packing", a, b, layout=False)
    a.close(); b.close()


# ---- 3. deterministic blob, no addresses
def test_the_blob_is_deterministic(gpu, wt):
    cols, bc, a = _warm(wt, 4, 24, 3)
    blob = a.checkpoint()
    assert a.checkpoint() == blob and len(blob) == _size(a)
    h = header_of(blob)
    assert (h["magic"], h["format"], h["abi"], h["n_zones"], h["n_reactors"], h["bytes"]) == (b"WTCK", 1, 1, 4, 24, len(blob))
    b = wt.ReactorEnsemble(cols, n_zones=4)          # another handle: other addresses throughout
    b.restore(blob)
    assert b.checkpoint() == blob and _size(b) == len(blob)
    N, n = ctypes.c_int64(0), ctypes.c_int(0)
    assert gpu_lib().wt_checkpoint_check(blob, len(blob), ctypes.byref(N), ctypes.byref(n)) == 0 and (N.value, n.value) == (24, 4)
    a.close(); b.close()


# ---- 4. load replaces the configuration
def test_load_replaces_the_configuration(gpu, wt):
    n, N = 4, 24
    cols, bc = wt.make_ensemble(N, seed=2100)
    a = wt.ReactorEnsemble(cols, n_zones=n)          # sensors, plant I/O, one PI loop, trains of 3: no other program
    a.set_boundary(bc)
    a.enable_sensors(seed=3)
    a.enable_plant_io()
    a.set_trains(3)
    a.enable_control(wt.PILoop("chlorine_outlet", setpoint=2.0, kp=1.0, ki=1e-3))
    a.step(DT, n_steps=30, download=False)
    b = build(wt, cols, bc, n, 2, trend_capacity=64)  # everything, trains of 2
    b.step(DT, n_steps=10, download=False)
    assert not np.array_equal(info_codes(a), info_codes(b))
    b.restore(a.checkpoint())
    both("after the load", a, b)
    assert _refused(b.injection_state) == "no injection program is set (wt_ensemble_inject_set)"
    assert _refused(b.trend_state) == "no trend program is set (wt_ensemble_trend_set)"
    assert _refused(b.score_curve) == "no score program is set (wt_ensemble_score_set)"
    assert _refused(b.pipe_state) == "no pipe program is set (wt_ensemble_pipe_set)"
    assert _refused(b.wire_state) == "no wire program is set (wt_ensemble_wire_set)"
    with pytest.raises(gpu.WtError, match="recording is off"):
        b.trajectory()
    continue_alike("replaced", a, b)
    assert wavefront_groups(a) == wavefront_groups(b)
    a.close(); b.close()


# ---- 5. copy
def test_clone_shares_nothing(gpu, wt):
    cols, bc, a = _warm(wt, 5, 26, 2)
    _, _, twin = _warm(wt, 5, 26, 2)
    c = a.clone()
    assert set(vars(c)) == set(vars(a)) and c._h.value != a._h.value and c.info(gpu.WT_INFO_MARK) == 0
    continue_alike("clone", a, c)
    before = snapshot(a)
    c.step(DT, n_steps=30, download=False)
    c.clear_trends(); c.set_trains(2)
    same("the original after its clone went on", before, snapshot(a))
    twin.step(DT, n_steps=40, download=False)
    continue_alike("the original and a twin that was never cloned", a, twin)
    # refusals
    L = gpu.lib()
    assert (L.wt_ensemble_copy(a._h, a._h), L.wt_last_error()) == (gpu.WT_E_ARG, b"copy: dst and src are the same handle")
    cols2, _ = wt.make_ensemble(13, seed=1)
    small = wt.ReactorEnsemble(cols2, n_zones=5)
    assert (L.wt_ensemble_copy(small._h, a._h), L.wt_last_error()) == (gpu.WT_E_ARG, b"copy: the handles differ in n_reactors or n_zones")
    other = wt.ReactorEnsemble(dict(cols, total_carbonate=cols["total_carbonate"] + 0.5), n_zones=5)
    before = snapshot(other)
    assert (L.wt_ensemble_copy(other._h, a._h), L.wt_last_error()) == (gpu.WT_E_ARG, b"copy: the reactor constants differ")
    assert _refused(other.restore, a.checkpoint()) == E_CONSTANTS
    same("a refused copy and load change nothing", before, snapshot(other))
    for ens in (a, c, twin, small, other):
        ens.close()


# ---- 6. mark and rewind
@pytest.mark.parametrize("memcpy", [False, True], ids=["table_kernel", "WT_CKP_MEMCPY"])
def test_mark_and_rewind(gpu, wt, monkeypatch, memcpy):
    if memcpy:
        monkeypatch.setenv("WT_CKP_MEMCPY", "1")
    cols, bc, a = _warm(wt, 8, 17, steps=100)
    assert _refused(a.rewind) == E_NO_MARK and a.info(gpu.WT_INFO_MARK) == 0
    a.mark()
    assert a.info(gpu.WT_INFO_MARK) == 1
    marked = program_params(a, "inject")
    go = lambda: (a.step(DT, n_steps=50, download=False), snapshot(a))[1]
    X = go()
    a.rewind()
    same("rewind", X, go())
    a.rewind()
    a.set_injections(wt.Injection("chlorine_outlet", "bias", a=1.0))       # the same arrays, other parameters
    Y = go()
    assert any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(X, Y))
    a.rewind()
    assert np.array_equal(program_params(a, "inject"), marked, equal_nan=True)
    same("rewind over other parameters", X, go())
    a.clear_trends()
    a.rewind()
    same("rewind over a cleared program", X, go())
    a.set_trends(wt.Trend("alarm_word"), capacity=32)
    a.rewind()
    assert a.info(gpu.WT_INFO_TREND_CAPACITY) == 16
    same("rewind over another capacity", X, go())
    # a second mark replaces the first
    a.mark()
    Z = go()
    a.rewind()
    same("second mark", Z, go())
    assert a.clone().info(gpu.WT_INFO_MARK) == 0
    a.unmark(); a.unmark()
    assert a.info(gpu.WT_INFO_MARK) == 0 and _refused(a.rewind) == E_NO_MARK
    a.mark()
    a.close()                                         # with a mark set


# ---- 7. frozen and failed reactors travel
def test_frozen_reactors_travel(gpu, wt):
    from conftest import golden_json
    g = golden_json("g4_faults.json")["cold_run"]
    cold = wt.ReactorConfiguration(**g["config"])
    cb = wt.BoundaryConditions(**dict(zip(wt.params.BOUNDARY_FIELDS, g["bc"])))
    warm, wb = wt.ReactorConfiguration(n_zones=cold.n_zones), wt.BoundaryConditions()
    cfgs, bcs = [cold, warm, warm, warm], [cb, wb, wb, wb]
    a = wt.ReactorEnsemble(cfgs)
    a.set_boundary(bcs)
    a.set_trains(2, rows=("pH", "chlorine"))
    es = a.step(1.0, n_steps=60)
    assert es.status[0] & 1 and es.time[0] < 60 and not es.status[1:].any()
    b = wt.ReactorEnsemble(cfgs)
    b.restore(a.checkpoint())
    both("frozen", a, b)
    assert b.status()[0] & 1 and np.array_equal(a.bad_temperature(), b.bad_temperature()) and a.bad_temperature()[0] != 0
    for ens in (a, b):
        ens.step(1.0, n_steps=10, download=False)
    both("stays frozen", a, b)
    assert b.state.time[0] == es.time[0] and b.state.time[1] == 70
    for ens in (a, b):
        ens.clear_status()
        ens.step(1.0, n_steps=5, download=False)
    both("after clear_status", a, b)
    a.close(); b.close()


# ---- 8. refusals reach no device call
def test_refusals_change_nothing(gpu, wt):
    cols, bc, a = _warm(wt, 8, 17, steps=40)
    _, _, d = _warm(wt, 8, 17, steps=25)
    _, _, twin = _warm(wt, 8, 17, steps=25)
    blob = a.checkpoint()
    assert HEADER.size == 64
    flipped = bytearray(blob); flipped[-9] ^= 0x40
    n_parts = "checkpoint_load: the checkpoint's n_reactors or n_zones differ from the handle's"
    arrays = "checkpoint: a part's arrays do not match the capacities it declares"
    variants = [  # blob, wt_checkpoint_check's text, load's text
        (blob[:-1], "checkpoint: the header's byte count is not the blob's length", None),
        (bytes(flipped), "checkpoint: checksum mismatch", None),
        (with_header(blob, magic=b"WTCX"), "checkpoint: bad magic", None),
        (with_header(blob, format=2), "checkpoint: unknown format version", None),
        (with_header(blob, layout=header_of(blob)["layout"] ^ 1), "checkpoint: the layout fingerprint is not this library's", None),
        (with_header(blob, n_reactors=18), arrays, n_parts),
        (with_header(blob, n_zones=7), arrays, n_parts),
        (blob[:10], "checkpoint: shorter than its header", None),
    ]
    L = gpu.lib()
    before = snapshot(d)
    for bad, text, load_text in variants:
        assert (L.wt_checkpoint_check(bad, len(bad), None, None), L.wt_last_error().decode()) == (gpu.WT_E_ARG, text)
        assert _refused(d.restore, bad) == (load_text or text)
    buf = ctypes.create_string_buffer(len(blob))
    assert L.wt_ensemble_checkpoint_save(a._h, buf, len(blob) - 1) == gpu.WT_E_ARG
    assert L.wt_last_error() == b"checkpoint_save: the buffer is smaller than wt_ensemble_checkpoint_size"
    assert buf.raw == bytes(len(blob))                # nothing was written
    same("the refusals changed nothing", before, snapshot(d))
    continue_alike("after the refusals", d, twin, steps=(20,))
    d.restore(blob)                                   # the good blob still loads
    continue_alike("after the load", a, d, steps=(20,))
    for ens in (a, d, twin):
        ens.close()


# ---- 9. file round trip
def test_file_round_trip(gpu, wt, tmp_path):
    cols, bc, a = _warm(wt, 8, 17, steps=60)
    path = tmp_path / "p.npz"
    a.save(path)
    b = wt.ReactorEnsemble.load(path)
    assert set(vars(b)) == {"n_reactors", "n_zones", "device", "columns", "constants", "_h"}
    assert all(np.array_equal(a.columns[k], b.columns[k]) for k in a.columns) and np.array_equal(a.constants, b.constants)
    both("loaded from the file", a, b)
    continue_alike("file", a, b)
    with np.load(path) as f:
        entries = {k: f[k] for k in f.files if k != "checkpoint"}
    np.savez(tmp_path / "q.npz", **entries)
    assert "'checkpoint'" in _refused(wt.ReactorEnsemble.load, tmp_path / "q.npz")
    a.close(); b.close()


# ---- 10. the copy kernel alone
def test_the_copy_kernel_alone(gpu):
    L = gpu.lib()

    def run(sizes):
        arr = (ctypes.c_int64 * max(len(sizes), 1))(*sizes)
        bad = ctypes.c_int(-1)
        assert L.wt_selftest_copy_table(0, arr, len(sizes), ctypes.byref(bad)) == 0, L.wt_last_error()
        return bad.value

    assert run([]) == 0
    for sizes in ([1], [15], [16], [17], [35], [16384], [16385], [16384 * 3 + 5], [(1 << 20) + 1],
                  [1, 15, 16, 17, 35, 16384, 16385, 16384 * 3 + 5, (1 << 20) + 1, 0, 7]):
        assert run(sizes) == 0, sizes
    mixed = [int(x) for x in np.random.default_rng(0).choice([0, 1, 7, 16, 35, 255, 4096, 16383, 16384, 16400, 50001], 130)]
    assert len(mixed) > 128 and run(mixed) == 0       # more than one table
