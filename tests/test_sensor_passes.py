"""The pass structure of the sensor suite in a packed wavefront: ``sensor_passes`` restates the
lane rule of ``wts::suite_step``, and ``SENSOR_NS`` -- the zone counts at which the sensor, service and plant I/O oracle
tests run packed -- reaches every shape of it.  No GPU."""
from program_helpers import SENSOR_LINES, SENSOR_NS, instantiation, ragged_size, sensor_passes

# n: (R, sensor lanes, passes, {cut sensor: first slot of the later pass})
TABLE = {2: (32, 224, 4, {}), 3: (21, 147, 3, {3: 1, 6: 2}), 4: (16, 112, 2, {}), 5: (12, 84, 2, {5: 4}), 6: (10, 70, 2, {6: 4})}


def test_the_pass_table_row_by_row():
    for n, (R, lanes, passes, cuts) in TABLE.items():
        p = sensor_passes(n)
        assert (p.R, p.lanes, p.passes, p.cuts) == (R, lanes, passes, cuts), n
    for n in range(7, 33):                                   # one pass, nothing cut, no line split
        p = sensor_passes(n)
        assert 2 <= p.R <= 9 and p.lanes <= 63 and p.passes == 1 and not p.cuts and not p.split, n
    assert sensor_passes(7).R == 9 and sensor_passes(32).R == 2


def test_where_the_rtd_takes_its_line():
    """The slots whose RTD lane runs in a later pass than its pH partner.  n = 5: the inlet RTD's slots 0...3 share the pH
    lane's pass, 4...11 take the next one; n = 6: the inlet line is whole in pass 0, the outlet RTD's slots 4...9 fall in
    pass 1; where a boundary lies between sensors (2, 4) and at n = 3 every RTD lane is in a later pass."""
    assert sensor_passes(5).split == {0: tuple(range(4, 12)), 1: tuple(range(12))}
    assert sensor_passes(6).split == {1: tuple(range(4, 10))}
    for n in (2, 3, 4):
        assert sensor_passes(n).split == {0: tuple(range(64 // n)), 1: tuple(range(64 // n))}, n
    # n = 3: the outlet RTD's run lies in passes 1 and 2, its pH partner's in pass 0
    p = sensor_passes(3)
    assert {p.pass_of(6, sl) for sl in range(p.R)} == {1, 2} and {p.pass_of(1, sl) for sl in range(p.R)} == {0}
    # a cut RTD run: the line it belongs to, for the tests that ask whether the far side transported
    assert {n: [(i, [ln for ln, pair in enumerate(SENSOR_LINES) if i in pair]) for i in sensor_passes(n).cuts if i >= 5]
            for n in (3, 5, 6)} == {3: [(6, [1])], 5: [(5, [0])], 6: [(6, [1])]}


def test_zone_counts_reach_every_pass_structure():
    sharing = {(1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True), (5, False)}
    assert {instantiation(n) for n in SENSOR_NS} == sharing
    shapes = {n: sensor_passes(n) for n in SENSOR_NS}
    assert any(p.passes > 1 and not p.cuts for p in shapes.values())                      # aligned multi-pass
    assert any(p.cuts for p in shapes.values())                                           # a cut sensor run
    assert any(any(i >= 5 for i in p.cuts) for p in shapes.values())                      # ... of an RTD
    assert any(any(0 < len(s) < p.R for s in p.split.values()) for p in shapes.values())  # a line split for some slots only
    assert any(p.passes > 1 and len(p.split) == 1 for p in shapes.values())               # a split line beside a whole one
    assert set(TABLE) <= set(SENSOR_NS)
    single = [p.R for p in shapes.values() if p.passes == 1]
    assert single == sorted(single, reverse=True) and single[0] == 8 and single[-1] == 2 and len(single) == 5
    assert all(ragged_size(n, 3) == (64 // n, 3 * (64 // n) + 1) for n in SENSOR_NS)
