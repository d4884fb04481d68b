"""Helpers of the tile-shape tests (a plain module, no fixtures).

Every deck starts from a uniform stream, and a cell whose rho, U, V, p equal
those of its four neighbours bit for bit cannot tell a wrong neighbour, an
unstaged halo slot or a wrong ghost column from the right one.  perturb()
makes every cell differ from its neighbours; flat_fraction() measures what is
left of the flat regions; shape_sweep() lists the tile geometries and grid
sizes at the edges of the tiling (GPU: test_gpu_tile_shapes.py, host tile
emulation: test_steppers.py)."""
import numpy as np

RECORD = 1248      # bytes per cell record; S[0..3] are its first four doubles
FIELDS = ["rho", "U", "V", "p", "T", "k", "R", "CP"]
SCHEDULE = [(1, False), (4, True), (6, False), (3, True)]


def perturb(sim_or_case, seed, amp=0.05):
    """Scale the four conserved values of every cell by 1 + amp * r1 and the
    two momenta by a further 1 + 0.4 * amp * r2 (r1, r2 uniform in [-1, 1] per
    cell from default_rng(seed)), write the records back and, for a
    Simulation, upload them to its solver."""
    case = getattr(sim_or_case, "case", sim_or_case)
    rec = np.frombuffer(case.records(), dtype=np.uint8).reshape(-1, RECORD).copy()
    S = rec[:, :32].copy().view(np.float64)           # [ncell, 4]
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1.0, 1.0, size=(S.shape[0], 2))
    S *= (1.0 + amp * r[:, 0])[:, None]
    S[:, 1:3] *= (1.0 + 0.4 * amp * r[:, 1])[:, None]
    rec[:, :32] = S.view(np.uint8)
    case.set_records(rec.tobytes())
    if case is not sim_or_case:
        sim_or_case.solver.upload()


def flat_fraction(sim):
    """Fraction of the non-solid cells whose rho, U, V, p equal, bit for bit,
    those of all their (up to four) neighbours inside the grid."""
    flat = None
    for f in ("rho", "U", "V", "p"):
        a = np.ascontiguousarray(sim.field(f)).view(np.uint64)
        same = np.ones(a.shape, dtype=bool)
        same[1:, :] &= a[1:, :] == a[:-1, :]
        same[:-1, :] &= a[:-1, :] == a[1:, :]
        same[:, 1:] &= a[:, 1:] == a[:, :-1]
        same[:, :-1] &= a[:, :-1] == a[:, 1:]
        flat = same if flat is None else flat & same
    gas = np.asarray(sim.field("solid")) == 0.0
    return float(flat[gas].sum()) / max(int(gas.sum()), 1)


# (threads per tile workgroup, cells per thread, tile height override):
# TJ = 11 leaves 3 of 256 threads idle, (64, 1, 64) gives TI = 1
GEOMS = [(256, 1, 0), (256, 2, 0), (256, 1, 11), (128, 2, 16), (64, 1, 64), (64, 2, 8)]
# ny = 8: the lowest grid on the tile path; 32 / 33: one / two tile rows
NYS = [8, 9, 32, 33, 65]
MIN_NX = 22        # below it the wedge deck's ramp is too low for its solid seed point
MAX_CELLS = 5000


OPEN_TOP = "NT_D0Y_2D, TCT_dkdy_NULL_2D, TCT_depsdy_NULL_2D"


def sweep_deck(nx, ny, top="farfield"):
    """The wedge of the sweep; top = "open": a zero-gradient top boundary, so
    the grid's last row is live (the far-field row is constant after its first
    fill, and a tile row that never updates it goes unnoticed)."""
    from openhyperflow2d_amd.models import decks

    text = decks.wedge15(nx, ny, nmax=10 ** 6, nout=10 ** 5)
    return text if top == "farfield" else decks.set_key(text, "Contour1.Bound1.Cond", OPEN_TOP)


def shape_sweep(native):
    """[(nt, cpt, tj, nx, ny, top)]: every geometry at every ny, plus tj = 16
    at ny = 33 (tile rows of 16, 16 and one cell), each at nx = TI - 1 (a strip
    narrower than one tile), TI, TI + 1 and 2 TI + 1 with TI read from the
    native lean_tile_geom; combinations that clamp to a tiling of the same
    grid already listed are dropped.  Tilings of more than one tile row run
    once more, at nx = TI + 1, with the open top boundary."""
    combos = [(nt, cpt, tj, ny) for (nt, cpt, tj) in GEOMS for ny in NYS]
    combos += [(nt, cpt, 16, 33) for (nt, cpt) in sorted({(g[0], g[1]) for g in GEOMS})]
    seen, out = set(), []
    for nt, cpt, tj, ny in combos:
        TI = native.lean_tile_geom(100, ny, nt, tj, cpt)["TI"]
        for nx, top in [(TI - 1, "farfield"), (TI, "farfield"), (TI + 1, "farfield"), (2 * TI + 1, "farfield"),
                        (TI + 1, "open")]:
            nx = max(nx, MIN_NX)
            g = native.lean_tile_geom(nx, ny, nt, tj, cpt)
            key = (nt, cpt, g["TI"], g["TJ"], nx, ny, top)
            if key in seen or nx * ny > MAX_CELLS or (top == "open" and g["nbj"] < 2):
                continue
            seen.add(key)
            out.append((nt, cpt, tj, nx, ny, top))
    return out
