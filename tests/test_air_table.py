"""The block the single-gas lean tile kernels keep in LDS for the Cp_air lookup
(common.hpp: AirTable, air_table_build, air_table_eval), on the host: padding,
the mode of every table class, the gas constant, and the branch-free segment
search against table_eval bit for bit."""
import math
import struct

import numpy as np
import pytest

from tests.air_tables import TABLES, arguments, same_bits

PTS = 16


@pytest.fixture(scope="module")
def nat():
    import openhyperflow2d_amd as hf

    return hf.native()


def _ramp(n):
    return [100.0 + 50.0 * k for k in range(n)], [1000.0 + 3.0 * k * k for k in range(n)]


@pytest.mark.parametrize("n,mode", [(0, 0), (1, 0), (2, 1), (16, 1), (17, 0), (64, 0)])
def test_block_mode_and_padding(nat, n, mode):
    x, y = _ramp(n)
    b = nat.air_table_build(x, y)
    assert (b["n"], b["mode"]) == (n, mode)
    assert b["bytes"] == 8 * (2 + 2 * PTS) and len(b["x"]) == PTS and len(b["y"]) == PTS
    held = n if mode else 0   # a block in mode 0 holds the padding only
    assert b["x"][:held] == x[:held] and b["y"][:held] == y[:held]
    assert all(v == math.inf for v in b["x"][held:])
    assert all(v == 0.0 and math.copysign(1.0, v) == 1.0 for v in b["y"][held:])


def test_block_mode_of_knot_orders(nat):
    y = [1.0, 2.0, 3.0, 4.0]
    assert nat.air_table_build([1.0, 2.0, 3.0, 4.0], y)["mode"] == 1
    assert nat.air_table_build([1.0, 3.0, 2.0, 4.0], y)["mode"] == 0   # one descending knot
    assert nat.air_table_build([1.0, 2.0, 4.0, 3.0], y)["mode"] == 0
    assert nat.air_table_build([2.0, 1.0, 3.0, 4.0], y)["mode"] == 0
    assert nat.air_table_build([1.0, 2.0, 2.0, 4.0], y)["mode"] == 1   # repeated knots do not descend
    assert nat.air_table_build([1.0, 1.0, 2.0, 4.0], y)["mode"] == 1
    assert nat.air_table_build([1.0, math.nan, 2.0, 4.0], y)["mode"] == 0
    assert nat.air_table_build([math.nan, 1.0, 2.0, 4.0], y)["mode"] == 0
    assert nat.air_table_build([1.0, 2.0, 3.0, math.inf], y)["mode"] == 1


@pytest.mark.parametrize("R", [(296.8, 259.8, 188.9, 287.0), (1e-310, -3.5, 4124.2, 287.05287), (0.0, 0.0, 0.0, 0.1),
                               (math.inf, 1.0, 1.0, 287.0)])
def test_block_R_is_chemistry_single_gas_expression(nat, R):
    fu, ox, cp, air = R
    want = ((fu * 0. + ox * 0.) + cp * 0.) + air * 1.   # lean_euler.hpp chemistry_single_gas
    got = nat.air_table_build([1.0, 2.0], [3.0, 4.0], list(R))["R"]
    assert struct.pack("<d", got) == struct.pack("<d", want) or (math.isnan(got) and math.isnan(want))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_host_air_table_eval_equals_table_eval(nat, name):
    rows, mode = TABLES[name]
    x, y = [r[0] for r in rows], [r[1] for r in rows]
    xv = arguments(rows)
    got, m = nat.air_table_eval(x, y, xv)
    assert m == mode
    want = nat.table_eval(x, y, xv)
    assert same_bits(got, want), [(v, a, b) for v, a, b in zip(xv, got, want) if not same_bits([a], [b])]
    nan, _ = nat.air_table_eval(x, y, [math.nan])
    # (a one-point table is its value at every argument, table_eval's n == 1)
    assert np.isnan(nan).all() if len(rows) > 1 else nan == [y[0]]


def test_host_air_table_eval_random_arguments(nat):
    rng = np.random.default_rng(7)
    for name, (rows, mode) in sorted(TABLES.items()):
        if not mode:
            continue
        x, y = [r[0] for r in rows], [r[1] for r in rows]
        xv = rng.uniform(min(x) - 300.0, max(x) + 300.0, size=2000).tolist()
        got, _ = nat.air_table_eval(x, y, xv)
        assert same_bits(got, nat.table_eval(x, y, xv)), name
