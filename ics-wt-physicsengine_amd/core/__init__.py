"""GPU-backed stand-in for the hot path of ``wt_simulator.core``
(export list modelled on /root/reference/src/wt_simulator/core/__init__.py:207-263,
restricted to the multi-zone CSTR step and its batched pH solver)."""
from .reactor import (BoundaryConditions, EnsembleState, IntegratedCSTR, PhysicsEngine,
                      ReactorConfiguration, ReactorEnsemble, ReactorState, Trajectory, boundary_block,
                      boundary_schedule_block)
from .control import ControlState, LoopState, PILoop, control_block
from .inject import Injection, InjectionState, attack_window, injection_block
from .alarm import Alarm, AlarmState, alarm_block
from .actuator import Actuator, ActuatorState, actuator_block
from .disturb import Disturbance, DisturbanceState, disturbance_block
from .score import Score, ScoreCurve, ScoreState, score_block
from .detect import Detector, DetectorState, detector_block
from .trend import Trend, TrendData, TrendState, trend_block
from .train import PipeState, TrainState, pipe_block, pipe_delay, train_block
from .wire import Wire, WireState, wire_block
from .junction import Junction, JunctionState, junction_block
from .service import Service, ServiceState, service_block
from .install import Installation, installation_block
from .tune import TUNE_RULES, LoopTune, RelayTune, TunerState, tune_block
from .mpc import DMCLoop, LoopMpc, MpcState, dmc_gain, fopdt_step, mpc_block
from .respond import Response, ResponseState, response_block
from . import link
from .link import Link, LinkState, link_block
from .chemistry import AqueousChemistry, BufferSystem, solve_pH
from .physics import (ArrheniusParameters, FlowParameters, GeometryParameters, SpatialModel, StratificationParameters,
                      TemperatureDependentKinetics, TransportModel, run_all_validations, validate_chemistry,
                      validate_integrated_reactor, validate_spatial, validate_thermodynamics, validate_transport)
from .synthetic import make_boundary_schedule, make_ensemble
from . import params, sharding
from .sharding import gather_state, shard_bounds

__all__ = ["BoundaryConditions", "EnsembleState", "IntegratedCSTR", "PhysicsEngine", "ReactorConfiguration",
           "ReactorEnsemble", "ReactorState", "Trajectory", "boundary_block", "boundary_schedule_block",
           "PILoop", "ControlState", "LoopState", "control_block", "Injection", "InjectionState", "injection_block",
           "Alarm", "AlarmState", "alarm_block", "Actuator", "ActuatorState", "actuator_block",
           "Disturbance", "DisturbanceState", "disturbance_block", "Score", "ScoreCurve", "ScoreState", "score_block",
           "Detector", "DetectorState", "detector_block", "attack_window",
           "Trend", "TrendData", "TrendState", "trend_block", "TrainState", "train_block", "PipeState", "pipe_block", "pipe_delay",
           "Wire", "WireState", "wire_block", "Junction", "JunctionState", "junction_block",
           "Service", "ServiceState", "service_block", "Installation", "installation_block",
           "RelayTune", "LoopTune", "TunerState", "TUNE_RULES", "tune_block",
           "DMCLoop", "LoopMpc", "MpcState", "dmc_gain", "fopdt_step", "mpc_block",
           "Response", "ResponseState", "response_block",
           "Link", "LinkState", "link_block", "link",
           "AqueousChemistry", "BufferSystem", "solve_pH", "make_ensemble", "make_boundary_schedule", "params", "sharding", "gather_state", "shard_bounds",
           # the rest of wt_simulator.core's export list (core/__init__.py:238-263)
           "TemperatureDependentKinetics", "ArrheniusParameters", "TransportModel", "GeometryParameters", "FlowParameters",
           "SpatialModel", "StratificationParameters", "validate_thermodynamics", "validate_chemistry", "validate_transport",
           "validate_spatial", "validate_integrated_reactor", "run_all_validations"]
