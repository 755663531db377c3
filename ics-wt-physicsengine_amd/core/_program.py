"""What the ten per-reactor programs (:mod:`.control`, :mod:`.inject`, :mod:`.alarm`, :mod:`.actuator`,
:mod:`.disturb`, :mod:`.score`, :mod:`.detect`, :mod:`.trend`, :mod:`.service`, :mod:`.tune`) share on the host: the
sensor names, names -> codes, the rows of one loop or slot, the packing of a slot program into its block, and the check
of a block.  Each module keeps its own fields, defaults and off rows; the rules a block must satisfy live only in the
library (``wt_program_check``)."""
from __future__ import annotations

import numpy as np

from . import _native

# the sensor suite's order: index = sensor code of every program block and row of ``sensor_readings``
SENSOR_NAMES = ("pH_inlet", "pH_outlet", "chlorine_inlet", "chlorine_outlet", "flow_main", "temp_inlet", "temp_outlet")


def codes(value, names, what) -> np.ndarray:
    """Names or indices -> float64 codes (their range is checked with the block, by :func:`check`)."""
    a = np.asarray(value)
    if a.dtype.kind in "US":
        bad = [s for s in a.ravel() if str(s) not in names]
        if bad:
            raise ValueError(f"unknown {what} {str(bad[0])!r}: one of {names}")
        return np.vectorize(lambda s: float(names.index(str(s))), otypes=[np.float64])(a)
    return a.astype(np.float64)


def field_rows(item, fields, n: int, name: str, **values) -> np.ndarray:
    """(len(fields), n) float64 rows of one loop or slot: each field of ``item`` (or its replacement in ``values``)
    broadcast to (n,)."""
    rows = np.empty((len(fields), n))
    for i, k in enumerate(fields):
        v = values[k] if k in values else getattr(item, k)
        try:
            rows[i] = np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))
        except ValueError:
            raise ValueError(f"{name}.{k}: expected a scalar or ({n},) values, got shape {np.shape(v)}") from None
    return rows


def check(program: int, block: np.ndarray) -> None:
    """The checks the set or enable call of ``program`` (``_native.WT_PROG_*``) makes on ``block``, a C-contiguous
    float64 [..][fields][N] block; ``ValueError`` names the first one that fails."""
    try:
        _native.check(_native.lib().wt_program_check(program, _native.dptr(block), block.shape[-1]))
    except _native.WtError as e:   # WT_E_ARG is the only error it returns
        raise ValueError(e.message) from None


def slot_block(items, n: int, slots: int, what: str, rows_of, off_rows: np.ndarray, program: int) -> np.ndarray:
    """The [slots][fields][n] float64 block of a slot program, checked by :func:`check`: slot k holds
    ``rows_of(items[k], n, name)``, the slots after the last item hold ``off_rows``."""
    if len(items) > slots:
        raise ValueError(f"at most {slots} {what}s per program, got {len(items)}")
    rows = [rows_of(item, n, f"{what} {k}") for k, item in enumerate(items)]
    rows += [off_rows] * (slots - len(items))
    block = np.ascontiguousarray(np.stack(rows))
    check(program, block)
    return block
