"""High-level simulation object: deck -> pre-processed case -> stepper.

Backends
  ``gpu``  DeviceSolver: HIP kernels on an MI355X (default when a GPU exists)
  ``cpu``  CpuSolver: the same per-cell kernels on the host (Jacobi order)
  ``ref``  RefSolver: the reference's in-place sweep order (golden oracle)
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np


def maybe_autotune(case, solver) -> str:
    """Deck key ThreadBlockSize = 0 (the reference's "auto-calibrate") tunes
    the lean kernel geometry on the device before the first step
    (DeviceSolver.autotune; results are unaffected).  HF2D_AUTOTUNE=0 skips
    (the solver's autotune_enabled knob, read when it was constructed)."""
    if case.thread_block_size != 0 or not solver.autotune_enabled:
        return ""
    return solver.autotune()


def parse_fault(spec: str):
    """``step:N[,rank:R][,kind:nan|kill]`` -> (N, R, kind); "" -> (-1, 0, "nan").

    Fault injection for the failure paths: ``nan`` poisons one
    active cell's energy at global iteration N on rank R (Tg < 0 -> error
    snapshot ``<Project>-err.plt``, the last good checkpoint is kept),
    ``kill`` SIGKILLs that rank (restart from the checkpoint)."""
    if not spec:
        return -1, 0, "nan"
    kv = {}
    for part in spec.split(","):
        k, _, v = part.partition(":")
        kv[k.strip()] = v.strip()
    if "step" not in kv:
        raise ValueError("fault spec needs step:N, got %r" % spec)
    kind = kv.get("kind", "nan")
    if kind not in ("nan", "kill"):
        raise ValueError("fault kind must be nan or kill, got %r" % kind)
    return int(kv["step"]), int(kv.get("rank", 0)), kind


PROBE_VARS = ("p", "T", "rho", "U", "V")   # column order of Simulation.probe_history()["values"]
LOAD_PARTS = ("Fx_p", "Fx_d", "Fy_p", "Fy_d")   # last axis of Simulation.load_history()["forces"]
# row order of Case.surface()["values"] and of Simulation.surface_history()["values"]
SURFACE_VARS = ("p", "Cp", "T", "tau_x", "tau_y", "Cf_x", "Cf_y", "q_y", "q_x", "St")
# variables of Case.frame() and of Simulation.record_frames()
FRAME_VARS = ("p", "T", "rho", "U", "V", "grad_rho", "grad_p", "vorticity", "dilatation", "ducros")
WALL_HEAT_X = ("Q", "Alpha", "Cp", "St")   # rows of Case.heat_flux_x() and of Simulation.wall_heat_history()["x"]


class Simulation:
    def __init__(self, deck_text: str, backend: Optional[str] = None, *, workdir: str = ".",
                 use_checkpoint: bool = False, device: int = 0, semantics: str = "mpi",
                 gi0: int = 0, gi1: int = -1, fused: bool = True, lean: Optional[bool] = None):
        from .. import native

        hf = native()
        self.hf = hf
        self.case = hf.Case.from_deck(deck_text, workdir, use_checkpoint)
        self.case.set_semantics(semantics)
        if backend is None:
            backend = "gpu" if hf.gpu_available() else "cpu"
        self.backend = backend
        if backend == "gpu":
            self.solver = hf.DeviceSolver(self.case, device, gi0, gi1)
            self.solver.fused = fused
            self.solver.lean = True if lean is None else bool(lean)
            self.autotune_log = maybe_autotune(self.case, self.solver)
        elif backend == "cpu":
            self.solver = hf.CpuSolver(self.case, gi0, gi1)
            self.solver.lean = False if lean is None else bool(lean)
        elif backend == "ref":
            self.solver = hf.RefSolver(self.case)
        else:
            raise ValueError("unknown backend %r" % backend)

    @classmethod
    def from_file(cls, path: str, backend: Optional[str] = None, **kw) -> "Simulation":
        with open(path, "r", errors="replace") as f:
            text = f.read()
        kw.setdefault("workdir", os.path.dirname(os.path.abspath(path)))
        return cls(text, backend, **kw)

    # -- time march ------------------------------------------------------
    def step(self, n: int = 1, residual: bool = False) -> None:
        self.solver.run_steps(int(n), bool(residual))

    def run(self, max_cycles: int = 1, outdir: str = ".", outputs: bool = True, checkpoint: bool = True,
            verbose: bool = True, metrics: str = "", profile: str = "", fault: str = ""):
        """Reference driver: outer cycles with outputs; returns (cycles, log text)."""
        step, rank, kind = parse_fault(fault)
        return self.solver.run(max_cycles, outdir, outputs, checkpoint, verbose, metrics, profile, step, rank, kind)

    def summary(self) -> dict:
        return dict(self.solver.summary())

    # -- data access -------------------------------------------------------
    def field(self, name: str) -> np.ndarray:
        self.solver.download()
        return np.asarray(self.case.field(name))

    def records(self) -> bytes:
        self.solver.download()
        return self.case.records()

    # -- per-step probe recorder --------------------------------------------
    def record_probes(self, cells, capacity: int = 4096) -> None:
        """Arm the per-step recorder on the global cells ``(i, j)`` (at most 64).

        From now on every step appends one row per probe, in the fixed
        variable order ``PROBE_VARS = ("p", "T", "rho", "U", "V")``, and the
        step's time to a ring of ``capacity`` rows kept by the backend (on the
        GPU: in device memory, written by one small kernel at the end of the
        step, so the steps stay in their graphs and the lean states are never
        materialised).  Each value is bit for bit what ``field(name)[i, j]``
        returns after that step.  Arming again replaces the recorder and
        restarts the count.  ``ValueError``: no cell, more than 64, a cell
        outside the grid, solid or unset, or ``capacity < 1``."""
        self.solver.record_probes([(int(i), int(j)) for i, j in cells], int(capacity))

    def probe_history(self) -> dict:
        """The recorded rows, oldest first: ``times`` [n], ``values``
        [n, nprobes, 5] (variables in ``PROBE_VARS`` order), ``total`` (steps
        recorded since arming; n = min(total, capacity), i.e. the last
        ``capacity`` steps once the ring has wrapped) and ``owned`` [nprobes]
        (False: the probe's column belongs to another strip and reads 0).
        ``times[k]`` equals ``summary()["time"]`` after that step.  Reading
        does not disturb the solver state."""
        h = dict(self.solver.probe_history())
        h["times"] = np.asarray(h["times"])
        h["values"] = np.asarray(h["values"])
        h["owned"] = np.asarray(h["owned"])
        h["total"] = int(h["total"])
        return h

    def clear_probe_history(self) -> None:
        """Drop the recorded rows; the recorder stays armed on the same cells."""
        self.solver.clear_probe_history()

    # -- per-step load recorder ---------------------------------------------
    def record_loads(self, boxes=(), cuts=(), capacity: int = 4096) -> None:
        """Arm the per-step load recorder on ``boxes`` ``(x0, y0, dx, dy)`` (the
        arguments of ``Case.x_force`` / ``y_force``) and ``cuts`` ``(x0, y0, dy)``
        (those of ``Case.mass_flow_x``): at most 16 of each, at least one of
        either.

        From now on every step appends, to a ring of ``capacity`` rows kept by
        the backend, the four parts ``LOAD_PARTS = ("Fx_p", "Fx_d", "Fy_p",
        "Fy_d")`` of every box (the pressure and the friction sum of the x and
        of the y force), the mass flow through every cut and the step's time.
        Every sum adds its terms in the order of the host integrals, so
        ``Fx_p + Fx_d`` is bit for bit ``case.x_force(*box)`` on a field
        downloaded after that step, ``Fy_p + Fy_d`` is ``case.y_force(*box)``
        and the mass flow is ``case.mass_flow_x(*cut)``.  On the GPU two small
        kernels run at the end of each step, inside the step graphs, and the
        lean states are never materialised.  Arming again replaces the ring.
        ``ValueError``: no box and no cut, more than 16 of either, ``capacity <
        1`` or a number that is not finite.  ``RuntimeError``: the solver is
        one strip of several (a one-process run only)."""
        b = [tuple(float(v) for v in q) for q in boxes]
        c = [tuple(float(v) for v in q) for q in cuts]
        if any(len(q) != 4 for q in b) or any(len(q) != 3 for q in c):
            raise ValueError("record_loads: a box is (x0, y0, dx, dy), a cut is (x0, y0, dy)")
        self.solver.record_loads(b, c, int(capacity))

    def load_history(self) -> dict:
        """The recorded rows, oldest first: ``times`` [n] (the clock of
        ``probe_history()``), ``forces`` [n, nboxes, 4] in ``LOAD_PARTS`` order,
        ``mass_flow`` [n, ncuts], ``terms`` (the static number of terms of
        every sum: ``box_terms`` [nboxes, 4], ``cut_terms`` [ncuts]), ``span``
        [nboxes] (the wall span of each box, static:
        ``Cx = (Fx_p + Fx_d) / body_pmax(span, flow)``) and ``total`` (steps
        recorded since arming; n = min(total, capacity)).  Reading does not
        disturb the solver state."""
        h = dict(self.solver.load_history())
        for k in ("times", "forces", "mass_flow", "span"):
            h[k] = np.asarray(h[k])
        h["terms"] = {k: np.asarray(v) for k, v in dict(h["terms"]).items()}
        h["total"] = int(h["total"])
        return h

    def clear_load_history(self) -> None:
        """Drop the recorded rows; the recorder stays armed on the same boxes and cuts."""
        self.solver.clear_load_history()

    # -- per-step wall heat recorder ------------------------------------------
    def record_wall_heat(self, x: bool = True, y: bool = True, cp_flow=None, rows=None, every: int = 1,
                         capacity: int = 1024, statistics: bool = True, weight: str = "time") -> None:
        """Arm the per-step wall heat recorder: the ``HeatFlux-X`` profile
        (``WALL_HEAT_X = ("Q", "Alpha", "Cp", "St")`` per column) when ``x``
        and the ``HeatFlux-Y`` profile (``Q`` per row) when ``y``.

        From now on every ``every``-th step appends both profiles and the
        step's time to a ring of ``capacity`` rows kept by the backend
        (``capacity=0``: statistics only), and with ``statistics`` folds every
        profile entry into a running mean, variance, peak and peak time
        (``weight``: ``"time"``, the span since the previous sample, or
        ``"step"``).  Every value is bit for bit ``case.heat_flux_x(cp_flow,
        rows)`` / ``case.heat_flux_y()`` on a field downloaded after that
        step.  ``cp_flow`` (1-based) and ``rows = (y_min, y_max)`` default to
        the deck's ``Cp_Flow_Index``, ``y_min`` and ``y_max``.  A profile that
        is not requested reads ``+0.0`` with node counts 0.  On the GPU up to
        three small kernels run at the end of each step, inside the step
        graphs, and the lean states are never materialised.  Arming again
        replaces the recorder.  ``ValueError``: neither profile, ``every <
        1``, ``capacity < 0``, an unknown ``weight``, or ``x`` with a flow
        index the case does not have.  ``RuntimeError``: the solver is one
        strip of several (a one-process run only), or the values could not
        be recorded exactly yet (see the README)."""
        if weight not in ("time", "step"):
            raise ValueError("record_wall_heat: weight is 'time' or 'step', not %r" % (weight,))
        keys = self.case.wall_heat_keys
        f = int(keys["Cp_Flow_Index"] if cp_flow is None else cp_flow)
        y0, y1 = (keys["y_min"], keys["y_max"]) if rows is None else rows
        self.solver.record_wall_heat(bool(x), bool(y), f, int(y0), int(y1), int(every), int(capacity),
                                     bool(statistics), weight == "step")

    def wall_heat_history(self) -> dict:
        """The recorded samples, oldest first: ``times`` [n] (the clock of
        ``probe_history()``), ``x`` [n, 4, nx] in ``WALL_HEAT_X`` order, ``y``
        [n, ny], ``total`` (samples taken since arming; n = min(total,
        capacity)), ``x_nodes`` [nx] and ``y_nodes`` [ny] (the static number
        of wall nodes of every column and row), and with statistics
        ``mean_x``, ``var_x``, ``peak_x``, ``peak_time_x`` [4, nx], the same
        four ``_y`` keys [ny], ``time`` (the weight sum) and ``samples``.
        Reading does not disturb the solver state."""
        h = dict(self.solver.wall_heat_history())
        for k, v in h.items():
            h[k] = int(v) if k in ("total", "samples") else float(v) if k == "time" else np.asarray(v)
        return h

    def clear_wall_heat(self) -> None:
        """Empty the ring and the statistics; the recorder stays armed."""
        self.solver.clear_wall_heat()

    # -- per-step surface recorder ---------------------------------------------
    def record_surface(self, boxes=None, cp_flow=None, every: int = 1, capacity: int = 1024,
                       statistics: bool = True, weight: str = "time") -> None:
        """Arm the per-step surface recorder: ``SURFACE_VARS = ("p", "Cp",
        "T", "tau_x", "tau_y", "Cf_x", "Cf_y", "q_y", "q_x", "St")`` of every
        wall node.

        A node is a set, non-solid cell that is a no-slip or wall-law wall or
        has a solid 4-neighbour.  ``boxes`` (at most 16, each ``(x0, y0, dx,
        dy)`` as for ``record_loads``) lists the nodes of each box in turn, in
        ``(i, j)`` order; ``boxes=None`` lists every node.  From now on every
        ``every``-th step appends the ten values of every listed node and the
        step's time to a ring of ``capacity`` rows kept by the backend
        (``capacity=0``: statistics only), and with ``statistics`` folds every
        entry into a running mean, variance, peak and peak time (``weight``:
        ``"time"`` or ``"step"``).  Every value is bit for bit
        ``case.surface(boxes, cp_flow)["values"]`` on a field downloaded after
        that step.  ``cp_flow`` (1-based) defaults to the deck's
        ``Cp_Flow_Index``.  On the GPU three small kernels run at the end of
        each step, inside the step graphs, and the lean states are never
        materialised.  Arming again replaces the recorder.  ``ValueError``:
        more than 16 boxes, a box that is not finite, ``every < 1``,
        ``capacity < 0``, ``capacity == 0`` without statistics, an unknown
        ``weight``, a flow index the case does not have, a ring of more than
        2^31 entries.  ``RuntimeError``: the solver is one strip of several,
        or the values could not be recorded exactly (see the README)."""
        if weight not in ("time", "step"):
            raise ValueError("record_surface: weight is 'time' or 'step', not %r" % (weight,))
        f = int(self.case.wall_heat_keys["Cp_Flow_Index"] if cp_flow is None else cp_flow)
        b = None if boxes is None else [tuple(float(v) for v in q) for q in boxes]
        self.solver.record_surface(b, f, int(every), int(capacity), bool(statistics), weight == "step")

    def surface_history(self) -> dict:
        """The recorded samples, oldest first: ``times`` [n] (the clock of
        ``probe_history()``), ``values`` [n, 10, nnodes] in ``SURFACE_VARS``
        order, ``total`` (samples taken since arming; n = min(total,
        capacity)), the static node table (``i``, ``j``, ``x``, ``y``,
        ``flags``, ``face_x``, ``face_y``, ``fric_x``, ``fric_y`` [nnodes],
        ``box_off`` [nboxes + 1]) and with statistics ``mean``, ``var``,
        ``peak``, ``peak_time`` [10, nnodes], ``time`` (the weight sum) and
        ``samples``.  Reading does not disturb the solver state."""
        h = dict(self.solver.surface_history())
        for k, v in h.items():
            h[k] = int(v) if k in ("total", "samples") else float(v) if k == "time" else np.asarray(v)
        return h

    def clear_surface(self) -> None:
        """Empty the ring and the statistics; the recorder stays armed."""
        self.solver.clear_surface()

    # -- per-step frame recorder -----------------------------------------------
    def record_frames(self, vars=("rho", "grad_rho"), region=None, stride=(1, 1), every: int = 1,
                      capacity: int = 16) -> None:
        """Arm the per-step frame recorder: a sequence of fields at a fixed
        step cadence (a schlieren movie), ``vars`` out of ``FRAME_VARS = ("p",
        "T", "rho", "U", "V", "grad_rho", "grad_p", "vorticity", "dilatation",
        "ducros")``.

        ``region = (i0, i1, j0, j1)`` is half-open and defaults to the whole
        grid; the output cells are ``i0 + a * stride[0]``, ``j0 + b *
        stride[1]``.  From now on every ``every``-th step appends one frame
        ``[nvars, ni, nj]`` and the step's time to a ring of ``capacity``
        frames kept by the backend.  The first five variables are the probe
        recorder's row, bit for bit ``field(name)`` after that step.  The
        other five are differences of the rows of the cell and its immediate
        gas neighbours (whatever the stride; gas: set and not solid), central
        with both neighbours of a direction, one-sided with one, ``+0`` with
        none::

            ddx(q) = (q_E - q_W) * ((1 / dx) / max(hasW + hasE, 1))     # ddy likewise
            grad_rho   = sqrt(ddx(rho)**2 + ddy(rho)**2)                # grad_p likewise
            vorticity  = ddx(V) - ddy(U)
            dilatation = ddx(U) + ddy(V)
            ducros     = dilatation**2 / ((dilatation**2 + vorticity**2) + 1e-30)

        Every value is bit for bit ``case.frame(vars, region, stride)`` on a
        field downloaded after that step; a cell that is not gas reads
        ``+0.0``.  Axisymmetric decks use the same planar expressions (no
        ``V / y`` term).  On the GPU three small kernels run at the end of each
        step, inside the step graphs, and the lean states are never
        materialised.  Arming again replaces the recorder; a refused call
        leaves an armed one as it was.  ``ValueError``: an unknown, repeated
        or empty ``vars``, a region that is empty or outside the grid, a
        stride below 1, ``every < 1``, ``capacity < 1``, a ring of more than
        2^31 entries.  A solver that is one strip of several records the
        first five variables over the output columns it owns and refuses the
        other five (``RuntimeError``)."""
        if isinstance(vars, str):
            vars = (vars,)
        r = None if region is None else [int(v) for v in region]
        if r is not None and len(r) != 4:
            raise ValueError("record_frames: a region is (i0, i1, j0, j1)")
        si, sj = stride
        self.solver.record_frames([str(v) for v in vars], r, (int(si), int(sj)), int(every), int(capacity))

    def frame_history(self) -> dict:
        """The recorded frames, oldest first: ``times`` [n] (the clock of
        ``probe_history()``), ``values`` [n, nvars, ni, nj] (float64), ``total``
        (samples taken since arming; n = min(total, capacity)), ``vars``, and
        the static ``i`` [ni], ``j`` [nj] (the output cells; on a strip the
        owned global columns of the region), ``x`` [ni], ``y`` [nj] (the field
        dump's coordinates) and ``gas`` [ni, nj].  Reading does not disturb
        the solver state."""
        h = dict(self.solver.frame_history())
        for k, v in h.items():
            h[k] = int(v) if k == "total" else tuple(str(s) for s in v) if k == "vars" else np.asarray(v)
        return h

    def clear_frames(self) -> None:
        """Empty the ring; the recorder stays armed."""
        self.solver.clear_frames()

    # -- time-averaged flow statistics ---------------------------------------
    def start_averaging(self, every: int = 1, second_moments: bool = True, weight: str = "time",
                        favre: bool = False, species=None) -> None:
        """Arm the whole-field accumulator.

        From now on every ``every``-th step (the first one ``every`` steps
        from here) folds ``(p, T, rho, U, V)`` of each owned gas cell, bit for
        bit what ``field(name)`` returns after that step, into a running
        weighted mean and, with ``second_moments``, the variances and the
        Reynolds shear stress u'v'.  All sums are float64 and follow the
        weighted incremental update of West / Welford::

            w = t_now - t_seen;  W1 = W + w;  r = w / W1;  W = W1
            d = x - m;  m = m + r * d;  e = x - m
            M = M + (w * d) * e;  C = C + (w * d_U) * e_V

        ``weight="time"`` weights a sample by the time since the previous one
        (since arming for the first), so ``every=k`` is a time-weighted average
        of every k-th state; ``weight="step"`` uses ``w = 1``.  On the GPU two
        small kernels run at the end of each step, inside the step graphs, and
        the lean states are never materialised.  Starting again restarts from
        zero.

        ``species`` (mechanism mode only): ``"all"`` or a sequence of species
        names whose mass fractions are averaged too.  With ``rho`` the row's
        density and ``rhoY_s`` the post-step partial density, for each listed
        species in list order::

            Y_s = rho != 0 ? rhoY_s / rho : 0          (what field("Y:<s>") returns)
            d = Y_s - mY_s;  mY_s = mY_s + r * d;  e = Y_s - mY_s
            MY_s = MY_s + (w * d) * e

        ``favre=True`` adds the density-weighted (Favre) averages of ``T, U, V``
        and the listed species, per cell with its own weight sum ``G``::

            om = w * rho;  G1 = G + om;  q = G1 > 0 ? om / G1 : 0;  G = G1
            for x in (T, U, V, Y_s...):
                d = x - f_x;  f_x = f_x + q * d;  e = x - f_x;  F_x = F_x + (om * d) * e
            CF = CF + (om * d_U) * e_V

        A call without the two options launches the same kernels and returns
        the same keys as before.  ``ValueError``: ``every < 1``, an unknown
        ``weight``, species on a deck that is not in mechanism mode, an unknown
        or repeated species name, an empty list, or more than 16 species."""
        if weight not in ("time", "step"):
            raise ValueError("start_averaging: weight must be 'time' or 'step', not %r" % (weight,))
        if int(every) < 1:
            raise ValueError("start_averaging: every must be at least 1")
        idx = self._species_indices(species)
        self.solver.start_averaging(int(every), bool(second_moments), weight == "step", bool(favre), idx)

    def _species_indices(self, species) -> list:
        """start_averaging's ``species`` -> mechanism indices (``None``: none)."""
        if species is None:
            return []
        if not self.case.mech_mode:
            raise ValueError("start_averaging: species statistics need a deck in mechanism mode")
        names = list(self.case.mech_species)
        if isinstance(species, str):
            if species != "all":
                raise ValueError("start_averaging: species must be None, 'all' or a sequence of names, not %r" % (species,))
            want = names
        else:
            want = [str(s) for s in species]
        if not want:
            raise ValueError("start_averaging: the species list is empty")
        idx = []
        for s in want:
            if s not in names:
                raise ValueError("start_averaging: unknown species %r (the mechanism has %s)" % (s, ", ".join(names)))
            if names.index(s) in idx:
                raise ValueError("start_averaging: species %r listed twice" % (s,))
            idx.append(names.index(s))
        if len(idx) > 16:
            raise ValueError("start_averaging: %d species, at most 16" % len(idx))
        return idx

    def averages(self) -> dict:
        """The accumulated statistics over the owned columns: ``mean``
        [5, nxl, ny] in ``PROBE_VARS`` order; with second moments ``var``
        [5, nxl, ny] = M / W and ``cov_uv`` [nxl, ny] = C / W; ``time`` (W: the
        averaged time span, or the sample count for ``weight="step"``),
        ``samples`` and ``columns`` = (gi0, gi1).  Solid cells are 0; before
        the first sample everything is 0.  Reading does not disturb the solver
        state.  ``RuntimeError`` when no accumulator was started.

        Only when armed with ``species``: ``species`` (the names, in list
        order), ``species_mean`` [ns, nxl, ny] and, with second moments,
        ``species_var`` = MY / W.  Only when armed with ``favre``:
        ``favre_vars`` = ``("T", "U", "V", "Y:<s>", ...)``, ``favre_mean``
        [nf, nxl, ny], ``favre_weight`` [nxl, ny] (G) and, with second moments,
        ``favre_var`` = F / G and ``favre_cov_uv`` = CF / G (0 where G == 0)."""
        a = dict(self.solver.averages())
        for k in ("mean", "var", "cov_uv", "species_mean", "species_var", "favre_mean", "favre_var", "favre_cov_uv",
                  "favre_weight"):
            if k in a:
                a[k] = np.asarray(a[k])
        for k in ("species", "favre_vars"):
            if k in a:
                a[k] = tuple(str(s) for s in a[k])
        a["time"] = float(a["time"])
        a["samples"] = int(a["samples"])
        a["columns"] = tuple(int(c) for c in a["columns"])
        return a

    def reset_averaging(self) -> None:
        """Restart the accumulation from zero with the same options."""
        self.solver.reset_averaging()

    def stop_averaging(self) -> None:
        """Stop accumulating; ``averages()`` keeps returning the frozen result."""
        self.solver.stop_averaging()

    def monitor_cells(self):
        """The deck's monitor points (NumMonitorPoints / Point-n.X/Y) as the
        cells the driver samples: ``i = int(x / dx)``, ``j = int(y / dy)``."""
        return [(int(i), int(j)) for i, j in self.case.monitor_cells]

    @property
    def shape(self):
        return (self.case.nx, self.case.ny)
