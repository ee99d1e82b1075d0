"""
The inputs of tests/dynamics_cases.py on the CPU: the two references (the oracle and the host DynamicNumber) agree bit for bit on every case,
and every case does what the device tests rely on — FREEZING sets freeze inside the hold and move again, MOVING sets never freeze, the
coefficient branches are the stated ones, and every non-finite case tells a NaN-dropping early-out from np.max.
"""
import numpy as np
import pytest

from tests import dynamics_cases as D

HOST = {}


def references(n, params):
    """(targets, dts, oracle, host) of one float32 case, computed once"""
    targets, dts, _, oracle = D.scan_reference(n, tuple(params))
    if (n, tuple(params)) not in HOST:
        HOST[n, tuple(params)] = D.host_f32(params, targets, dts)
    return targets, dts, oracle, HOST[n, tuple(params)]


@pytest.mark.parametrize("n,params", D.SCAN_CASES)
def test_oracle_and_host_class_agree_and_the_case_does_what_it_says(n, params):
    targets, dts, oracle, host = references(n, params)
    assert np.array_equal(oracle.values, host.values)
    assert np.array_equal(oracle.derivatives, host.derivatives)
    assert np.array_equal(oracle.previous, host.previous[-1])
    assert np.isfinite(oracle.values).all() and np.isfinite(oracle.derivatives).all()
    # the clock: dt = 0 at the start and in the middle, a variable stretch
    assert dts[0] == 0 and dts[130] == 0 and len(set(dts[135:150])) == 15 and (dts[135:150] >= 0.002).all() and (dts[135:150] <= 0.04).all()
    assert D.branches(params, dts) == D.BRANCHES.get(tuple(params), {0, 1}), D.branches(params, dts)
    frozen = D.frozen_frames(oracle.values, dts, 20, D.HOLD[1])
    if tuple(params) in D.FREEZING:
        assert len(frozen) >= 20, len(frozen)
        assert not np.array_equal(oracle.values[D.HOLD[1]], oracle.values[D.HOLD[1] - 1]) and not np.array_equal(oracle.values[-1], oracle.values[-2])
        # frozen means frozen: `previous` and the derivative keep the bits of the last step
        assert np.array_equal(host.previous[frozen[-1]], host.previous[frozen[0]]) and np.array_equal(host.derivatives[frozen[-1]], host.derivatives[frozen[0]])
    else:
        # (from frame 2: the first step from rest moves the derivative only, value += 0*dt)
        assert not D.frozen_frames(oracle.values, dts, 2, D.FRAMES)
    # a dt = 0 frame leaves everything as it was
    assert np.array_equal(oracle.values[130], oracle.values[129]) and np.array_equal(oracle.derivatives[130], oracle.derivatives[129])


def test_the_freezing_sets_freeze_for_most_of_the_hold():
    """At n = 257 every FREEZING set is frozen for at least 55 of frames 20 to 124"""
    for params in D.FREEZING:
        _, dts, oracle, _ = references(257, params)
        assert len(D.frozen_frames(oracle.values, dts, 20, D.HOLD[1])) >= 55, params


def restated_scan(targets, coeff, worst_of, precision=np.float32(D.PRECISION)):
    """dynamics.py:197-250 in float32 numpy from the coefficient table, with the early-out's maximum taken by `worst_of`"""
    n = targets.shape[1]
    value, derivative, previous = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    values = np.empty_like(targets)
    with np.errstate(invalid="ignore"):
        for k, (dt, k1, k2, k3) in enumerate(coeff):
            target = targets[k]
            if dt and not worst_of(np.abs(target - value)) < precision:
                velocity = (target - previous)/dt
                previous = target
                value = value + derivative*dt
                acceleration = (target + k3*velocity - value - k1*derivative)/k2
                derivative = derivative + acceleration*dt
            values[k] = value
    return values


def nan_dropping_max(difference):
    """What fmaxf folds to: the largest number, 0 where every difference is NaN"""
    return np.nanmax(difference) if not np.isnan(difference).all() else np.float32(0.0)


@pytest.mark.parametrize("n,kind", D.NONFINITE_CASES)
def test_nonfinite_targets_tell_a_nan_dropping_maximum_from_numpys(n, kind):
    targets, dts, coeff = D.nonfinite_case(n, kind)
    oracle, host = D.oracle_f32(D.NONFINITE_PARAMS, targets, dts), D.host_f32(D.NONFINITE_PARAMS, targets, dts)
    assert np.array_equal(oracle.values, host.values, equal_nan=True)
    assert np.array_equal(oracle.derivatives, host.derivatives, equal_nan=True)
    assert np.array_equal(oracle.previous, host.previous[-1], equal_nan=True)
    # frozen before the NaN arrives, so that the early-out hangs on the NaN alone
    assert len(D.frozen_frames(oracle.values, dts, 40, 80)) >= 20
    assert np.array_equal(restated_scan(targets, coeff, np.max), oracle.values, equal_nan=True)     # the restatement is the recurrence
    dropped = restated_scan(targets, coeff, nan_dropping_max)
    assert np.array_equal(dropped[:80], oracle.values[:80])
    differs = [k for k in range(80, len(targets)) if not np.array_equal(dropped[k], oracle.values[k], equal_nan=True)]
    assert differs, "a NaN-dropping early-out gives the same trajectory: the input has no teeth"
    if kind != "c":
        # the finite values differ as well: a converged system that steps still moves its low bits
        finite = np.isfinite(oracle.values[differs[0]]) & np.isfinite(dropped[differs[0]])
        assert (oracle.values[differs[0]][finite] != dropped[differs[0]][finite]).any() or (oracle.values[-1][finite] != dropped[-1][finite]).any()


@pytest.mark.parametrize("n,where", D.EDGE_CASES)
def test_precision_edge_freezes_just_below_and_steps_at_the_precision(n, where):
    targets, dts, _ = D.precision_edge_case(n, where)
    oracle, host = D.oracle_f32(D.EDGE_PARAMS, targets, dts), D.host_f32(D.EDGE_PARAMS, targets, dts)
    assert np.array_equal(oracle.values, host.values) and np.array_equal(oracle.derivatives, host.derivatives)
    assert np.array_equal(oracle.previous, host.previous[-1])
    assert 0 < targets[3, where] < targets[4, where] == np.float32(D.PRECISION)
    assert not host.derivatives[:4].any() and not host.previous[:4].any()          # frozen: not even `previous` takes the target
    assert host.derivatives[4, where] != 0 and host.previous[4, where] == targets[4, where] and oracle.values[-1, where] != 0


@pytest.mark.parametrize("integrate", [0, 1])
@pytest.mark.parametrize("nsystems,with_nan", [(n, False) for n in D.F64_SYSTEMS] + [(9, True)])
def test_scalar_systems_oracle_and_host_class_agree(nsystems, with_nan, integrate):
    params, starts, targets, dts, coeff = D.scalar_case(nsystems, with_nan)
    assert coeff.shape == (len(params), D.FRAMES, 4) and targets.shape == (D.FRAMES, len(params))
    first_frozen = set()
    for k, p in enumerate(params):
        oracle = D.oracle_f64(p, starts[k], targets[:, k], dts, integrate)
        host = D.host_f64(p, starts[k], targets[:, k], dts, integrate)
        nan = with_nan and k == len(params) - 1
        assert np.array_equal(oracle[:, 0], host[:, 0], equal_nan=nan) and np.array_equal(oracle[:, 1], host[:, 5], equal_nan=nan)
        assert np.array_equal(oracle[:, 2], host[:, 3], equal_nan=nan) and np.array_equal(oracle[:, 3], host[:, 2], equal_nan=nan)
        assert nan == bool(np.isnan(oracle[80:, 0]).any())
        frozen = D.frozen_frames(oracle[:, 0], dts, 12, D.FRAMES)      # (the holds begin at frames 2 to 8)
        if p in D.FREEZING and not nan:
            assert len(frozen) >= 20 and oracle[-1, 0] != oracle[frozen[-1], 0], (k, p)
            first_frozen.add(frozen[0])
        if integrate and not nan:
            assert oracle[-1, 1] != 0 and oracle[frozen[-1] if frozen else -1, 1] != oracle[(frozen[-1] if frozen else -1) - 1, 1]
    assert len(first_frozen) >= 2            # the per-system early-out fires at different frames in different systems
