"""Tables and arguments of the Cp_air lookup tests (a plain module, no
fixtures): test_air_table.py (host) and test_gpu_air_table.py (device)."""
import math

import numpy as np

# the deck's Cp_air (tests/fixtures/decks/Wedge.dat)
DECK = [(203.5, 1005.8), (300.0, 1004.5), (400.0, 1009.7), (1500.0, 1210.8), (2000.0, 1251.5), (2500.0, 1275.8),
        (3000.0, 1295.4), (3500.0, 1307.4)]


def _ramp(n, lo=150.0, hi=3200.0):
    x = np.linspace(lo, hi, n)
    return [(float(a), float(1000.0 + 0.11 * a + 40.0 * math.sin(0.003 * a))) for a in x]


# name -> (rows, AirTable mode): 1 from LDS, 0 table_eval on the species pack
TABLES = {
    "n2": (_ramp(2), 1),
    "n3": (_ramp(3), 1),
    "deck": (DECK, 1),
    "n16": (_ramp(16), 1),
    "repeat_mid": ([(200.0, 1001.0), (300.0, 1004.0), (300.0, 1009.0), (800.0, 1100.0), (800.0, 1105.0), (2000.0, 1250.0)], 1),
    "repeat_first": ([(200.0, 1001.0), (200.0, 1004.0), (900.0, 1110.0), (2000.0, 1250.0)], 1),
    "repeat_last": ([(200.0, 1001.0), (900.0, 1110.0), (2000.0, 1250.0), (2000.0, 1260.0)], 1),
    "n1": ([(300.0, 1004.5)], 0),
    "n17": (_ramp(17), 0),
    "descending": ([(200.0, 1001.0), (900.0, 1110.0), (600.0, 1050.0), (2000.0, 1250.0)], 0),
}


def arguments(rows):
    """Every knot, its two neighbours in double, one value below the first
    knot and one above the last, +-0, 1e300 and +inf (no NaN)."""
    xs = [r[0] for r in rows]
    out = []
    for x in xs:
        out += [x, math.nextafter(x, -math.inf), math.nextafter(x, math.inf)]
    out += [min(xs) - 57.25, max(xs) + 1234.5, 0.0, -0.0, 1e300, math.inf]
    return out


def same_bits(a, b):
    """a == b bit for bit, a NaN matching any NaN (a repeated knot divides
    0 / 0; the payload and sign of that NaN are the divider's, as in
    numpy.testing.assert_array_equal)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


def segment(xs, T):
    """Index 0 .. len(xs) of T among the knots xs: 0 at T <= xs[0], len(xs) at
    T >= xs[-1], k for xs[k-1] <= T < xs[k] in between."""
    xs, T = np.asarray(xs), np.asarray(T)
    s = np.searchsorted(xs, T, side="right")
    return np.where(T <= xs[0], 0, np.where(T >= xs[-1], len(xs), s))
