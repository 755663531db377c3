"""ctypes binding of libwtphys.so (include/wtphys.h).

There is deliberately no fallback: if the shared library is missing, or no HIP
device is present, every compute entry point raises.  The CPU oracle under
``oracle/`` is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_PKG, "csrc")
LIB_PATH = os.environ.get("WTPHYS_LIB", os.path.join(CSRC, "libwtphys.so"))  # override: diagnostic builds

WT_OK, WT_E_ARG, WT_E_HIP, WT_E_NOGPU, WT_E_STATE = 0, 1, 2, 3, 4
(WT_PROG_CONTROL, WT_PROG_INJECT, WT_PROG_ALARM, WT_PROG_ACTUATOR, WT_PROG_DISTURB, WT_PROG_SCORE, WT_PROG_DETECT,
 WT_PROG_TREND, WT_PROG_SERVICE, WT_PROG_TUNE) = range(10)   # wt_program_check
(WT_INFO_PLANT_IO, WT_INFO_PROGRAM, WT_INFO_TRAIN, WT_INFO_PIPE, WT_INFO_SENSOR_HISTORY, WT_INFO_DISTURB_HISTORY,
 WT_INFO_SCORE_CURVE, WT_INFO_SCORE_BINS, WT_INFO_TREND_CAPACITY, WT_INFO_TRAIN_LENGTH, WT_INFO_WAVE_DIAG,
 WT_INFO_BOUNDARY_UPLOADS, WT_INFO_WIRE, WT_INFO_MARK, WT_INFO_JUNCTION, WT_INFO_SERVICE, WT_INFO_TUNE, WT_INFO_INSTALL, WT_INFO_MPC,
 WT_INFO_RESPOND, WT_INFO_LINK) = (0, 1) + tuple(range(9, 28))   # wt_ensemble_info; WT_INFO_PROGRAM + WT_PROG_*: 1..8


class WtError(RuntimeError):
    """A libwtphys call returned a non-zero code."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libwtphys error {code}: {message}")
        self.code = code
        self.message = message


class SolverStats(C.Structure):
    _fields_ = [("nfev", C.c_int32), ("njev", C.c_int32), ("nlu", C.c_int32),
                ("nsteps", C.c_int32), ("nrej", C.c_int32)]


# what libwtphys.so is built from: wtphys.hip and exactly the headers it includes
# (tests/test_host_api.py::test_build_staleness_list_matches_the_includes)
BUILD_SOURCES = ("wtphys.hip", "wt_device.hpp", "wt_tables.hpp", "wt_args.hpp", "wt_lanes.hpp", "wt_rhs.hpp", "wt_pcr.hpp", "wt_numjac.hpp", "wt_queue.hpp", "wt_step.hpp", "wt_sensors.hpp", "wt_ins.hpp", "wt_svc.hpp", "wt_plc.hpp", "wt_ctl.hpp", "wt_tun.hpp", "wt_mpc.hpp", "wt_inj.hpp", "wt_lnk.hpp", "wt_alm.hpp", "wt_det.hpp", "wt_rsp.hpp", "wt_trd.hpp", "wt_act.hpp", "wt_dst.hpp", "wt_scr.hpp", "wt_trn.hpp", "wt_wir.hpp", "wt_diag.hpp", "wt_place.hpp", "wt_ckp.hpp")


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/wtphys.hip for gfx950 into csrc/libwtphys.so (hipcc)."""
    srcs = [os.path.join(CSRC, f) for f in BUILD_SOURCES]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "wtphys.h"))
    stale = (not os.path.exists(LIB_PATH)
             or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs))
    if force or stale:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-o", LIB_PATH, os.path.join(CSRC, "wtphys.hip")]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return LIB_PATH


_dp, _fp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_void_p
_u8p, _u16p, _u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

# Every function include/wtphys.h declares, once: name -> argtypes, or (argtypes, restype) where the function does not
# return an int (tests/test_host_api.py::test_binding_table_is_the_header).
SIGNATURES = {
    "wt_abi_version": [],
    "wt_last_error": ([], C.c_char_p),
    "wt_device_count": [_ip],
    "wt_ensemble_create": [C.c_int64, C.c_int, C.c_int, _dp, C.POINTER(_vp)],
    "wt_ensemble_destroy": [_vp],
    "wt_ensemble_set_state": [_vp, _dp, _dp, _dp, _dp],
    "wt_ensemble_set_boundary": [_vp, _dp],
    "wt_ensemble_step": [_vp, C.c_double, C.c_int, C.c_int],
    "wt_ensemble_step_scheduled": [_vp, C.c_double, C.c_int, C.c_int, _dp],
    "wt_ensemble_record": [_vp, C.c_int, C.c_int],
    "wt_ensemble_get_record": [_vp, _dp, _dp, _dp, _dp, _dp, _u32p, _ip],
    "wt_ensemble_set_schedule": [_vp, C.c_int, C.c_int],
    "wt_ensemble_get_schedule": [_vp, _ip, _ip, _ip, _ip],
    "wt_ensemble_item_steps": [_vp, C.c_int],
    "wt_ensemble_queue_error": [_vp, _ip],
    "wt_ensemble_set_sync": [_vp, C.c_int],
    "wt_ensemble_set_placement": [_vp, C.c_int],
    "wt_ensemble_get_placement": [_vp, _ip, _i32p],
    "wt_ensemble_placement_info": [_vp, _i64p, _i64p],
    "wt_ensemble_set_step_limit": [_vp, C.c_int],
    "wt_ensemble_synchronize": [_vp],
    "wt_ensemble_get_state": [_vp, _dp, _dp, _dp, _dp, _dp],
    "wt_ensemble_get_snapshot": [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p],
    "wt_ensemble_get_derived": [_vp, _dp, _dp, _dp],
    "wt_ensemble_get_status": [_vp, _u32p],
    "wt_ensemble_get_bad_temperature": [_vp, _dp],
    "wt_ensemble_clear_status": [_vp],
    "wt_ensemble_get_stats": [_vp, C.POINTER(SolverStats)],
    "wt_ensemble_rhs": [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p],
    "wt_ensemble_export_state_device": [_vp, _vp],
    "wt_ensemble_set_stream": [_vp, _vp],
    "wt_ensemble_launch_timing": [_vp, C.c_int],
    "wt_ensemble_launch_stats": [_vp, _i64p, _dp, _dp],
    "wt_ensemble_timer_start": [_vp],
    "wt_ensemble_timer_stop": [_vp, _fp],
    "wt_ensemble_sensors_enable": [_vp, C.c_uint64, C.c_int64, _dp, _dp, _dp, C.c_int],
    "wt_ensemble_sensors_get": [_vp, _fp, _u8p, _u8p],
    "wt_ensemble_sensors_history": [_vp, _fp, _u8p, _u8p, _i32p],
    "wt_ensemble_plc_enable": [_vp],
    "wt_ensemble_plc_write_holding": [_vp, _u16p, C.c_int64, C.c_int64],
    "wt_ensemble_plc_read_inputs": [_vp, _u16p, _u8p],
    "wt_ensemble_plc_device": [_vp, C.POINTER(_vp), C.POINTER(_vp)],
    "wt_ensemble_get_boundary": [_vp, _dp],
    "wt_ensemble_info": [_vp, C.c_int, _i64p],
    "wt_ensemble_control_enable": [_vp, _dp],
    "wt_ensemble_control_retune": [_vp, _dp],
    "wt_ensemble_control_get": [_vp, _dp],
    "wt_ensemble_control_disable": [_vp],
    "wt_ensemble_inject_set": [_vp, _dp],
    "wt_ensemble_inject_get": [_vp, _dp],
    "wt_ensemble_inject_clear": [_vp],
    "wt_ensemble_alarm_set": [_vp, _dp],
    "wt_ensemble_alarm_get": [_vp, _dp, _dp],
    "wt_ensemble_alarm_reset": [_vp, _u8p],
    "wt_ensemble_alarm_words": [_vp, _u16p],
    "wt_ensemble_alarm_device": [_vp, C.POINTER(_vp)],
    "wt_ensemble_alarm_clear": [_vp],
    "wt_ensemble_actuator_set": [_vp, _dp],
    "wt_ensemble_actuator_get": [_vp, _dp, _dp, _dp],
    "wt_ensemble_actuator_clear": [_vp],
    "wt_ensemble_disturb_set": [_vp, _dp, C.c_uint64, C.c_int64, C.c_int],
    "wt_ensemble_disturb_get": [_vp, _dp, _dp, _dp],
    "wt_ensemble_disturb_history": [_vp, _dp, _i32p],
    "wt_ensemble_disturb_clear": [_vp],
    "wt_ensemble_score_set": [_vp, _dp, C.c_int, C.c_int, _dp, _dp],
    "wt_ensemble_score_get": [_vp, _dp, _dp],
    "wt_ensemble_score_curve": [_vp, _i32p, _i32p, _ip],
    "wt_ensemble_score_fan_range": [_vp, _dp, _dp],
    "wt_ensemble_score_reset": [_vp],
    "wt_ensemble_score_clear": [_vp],
    "wt_ensemble_detect_set": [_vp, _dp, _dp],
    "wt_ensemble_detect_get": [_vp, _dp, _dp],
    "wt_ensemble_detect_labels": [_vp, _dp],
    "wt_ensemble_detect_reset": [_vp],
    "wt_ensemble_detect_clear": [_vp],
    "wt_ensemble_trend_set": [_vp, _dp, C.c_int64, C.c_int],
    "wt_ensemble_trend_get": [_vp, _dp],
    "wt_ensemble_trend_data": [_vp, _dp, _dp],
    "wt_ensemble_trend_reset": [_vp],
    "wt_ensemble_trend_clear": [_vp],
    "wt_ensemble_train_set": [_vp, C.c_int, _dp],
    "wt_ensemble_train_get": [_vp, _ip, _ip, _dp],
    "wt_ensemble_train_params": [_vp, _dp],
    "wt_ensemble_train_clear": [_vp],
    "wt_train_check": [C.c_int, C.c_int, C.c_int64, _dp],
    "wt_ensemble_pipe_set": [_vp, _dp],
    "wt_ensemble_pipe_get": [_vp, _ip, _dp, _dp, _dp],
    "wt_ensemble_pipe_clear": [_vp],
    "wt_pipe_check": [C.c_int64, _dp, _dp],
    "wt_ensemble_wire_set": [_vp, _dp],
    "wt_ensemble_wire_get": [_vp, _dp, _dp],
    "wt_ensemble_wire_clear": [_vp],
    "wt_wire_check": [C.c_int, C.c_int64, _dp],
    "wt_ensemble_junction_set": [_vp, _dp, _dp],
    "wt_ensemble_junction_get": [_vp, _dp],
    "wt_ensemble_junction_params": [_vp, _dp, _dp],
    "wt_ensemble_junction_clear": [_vp],
    "wt_junction_check": [C.c_int, C.c_int64, _dp, _dp, _dp],
    "wt_ensemble_service_set": [_vp, _dp],
    "wt_ensemble_service_get": [_vp, _dp],
    "wt_ensemble_service_params": [_vp, _dp],
    "wt_ensemble_service_reset": [_vp],
    "wt_ensemble_service_clear": [_vp],
    "wt_service_check": [C.c_int64, _dp],
    "wt_ensemble_tune_set": [_vp, _dp],
    "wt_ensemble_tune_get": [_vp, _dp],
    "wt_ensemble_tune_params": [_vp, _dp],
    "wt_ensemble_tune_reset": [_vp],
    "wt_ensemble_tune_clear": [_vp],
    "wt_tune_check": [C.c_int64, _dp],
    "wt_mpc_check": [C.c_int64, _dp, _dp, _dp],
    "wt_ensemble_mpc_set": [_vp, _dp, _dp, _dp],
    "wt_ensemble_mpc_get": [_vp, _dp],
    "wt_ensemble_mpc_prediction": [_vp, _dp],
    "wt_ensemble_mpc_params": [_vp, _dp, _dp, _dp],
    "wt_ensemble_mpc_reset": [_vp],
    "wt_ensemble_mpc_clear": [_vp],
    "wt_respond_check": [C.c_int64, _dp],
    "wt_ensemble_respond_set": [_vp, _dp],
    "wt_ensemble_respond_state": [_vp, _dp, _dp],
    "wt_ensemble_respond_params": [_vp, _dp],
    "wt_ensemble_respond_reset": [_vp],
    "wt_ensemble_respond_clear": [_vp],
    "wt_link_check": [C.c_int64, _dp],
    "wt_ensemble_link_set": [_vp, _dp, C.c_uint64],
    "wt_ensemble_link_state": [_vp, _dp],
    "wt_ensemble_link_params": [_vp, _dp, C.POINTER(C.c_uint64)],
    "wt_ensemble_link_ring": [_vp, _dp, _dp, _dp],
    "wt_ensemble_link_reset": [_vp],
    "wt_ensemble_link_clear": [_vp],
    "wt_ensemble_install_set": [_vp, _dp],
    "wt_ensemble_install_get": [_vp, _dp],
    "wt_ensemble_install_clear": [_vp],
    "wt_install_check": [C.c_int64, _dp],
    "wt_ensemble_sensors_service": [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _u8p],
    "wt_ensemble_sensors_health": [_vp, _dp],
    "wt_program_check": [C.c_int, _dp, C.c_int64],
    "wt_ensemble_program_params": [_vp, C.c_int, _dp],
    "wt_ensemble_checkpoint_size": [_vp, _i64p],
    "wt_ensemble_checkpoint_save": [_vp, _vp, C.c_int64],
    "wt_ensemble_checkpoint_load": [_vp, _vp, C.c_int64],
    "wt_checkpoint_check": [_vp, C.c_int64, _i64p, _ip],
    "wt_ensemble_copy": [_vp, _vp],
    "wt_ensemble_mark": [_vp],
    "wt_ensemble_rewind": [_vp],
    "wt_ensemble_unmark": [_vp],
    "wt_selftest_copy_table": [C.c_int, _i64p, C.c_int, _ip],
    "wt_ensemble_diagnostics": [_vp, _dp],
    "wt_selftest_shuffles": [C.c_int, C.c_int, _ip],
    "wt_wave_diag_slots": [],
    "wt_ensemble_item_trace": [_vp, _i64p, C.c_int, _ip],
    "wt_ensemble_wave_diag": [_vp, _i64p, C.c_int64, _i64p],
    "wt_ensemble_size": ([_vp], C.c_int64),
    "wt_ensemble_zones": [_vp],
    "wt_ph_solve": [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int, _dp, _i32p, _i32p],
}

_lib = None


def lib():
    """Load libwtphys.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "There is no CPU fallback for the physics step.")
    L = C.CDLL(LIB_PATH)
    for name, sig in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
    if L.wt_abi_version() != 1:
        raise ImportError("libwtphys.so ABI version mismatch; rebuild it")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != WT_OK:
        raise WtError(rc, lib().wt_last_error().decode("utf-8", "replace"))


def dptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    # A ctypes array over the block's own memory passes as `double *` and costs a quarter of ``a.ctypes.data_as``:
    # the drop-in's step() marshals nine blocks per call.  A read-only array exports no writable buffer.
    if a.size and a.flags["WRITEABLE"]:
        return (C.c_double * a.size).from_buffer(a)
    return a.ctypes.data_as(_dp)


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().wt_device_count(C.byref(n))
    return n.value if rc == WT_OK else 0
