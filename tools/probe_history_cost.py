#!/usr/bin/env python3
"""Cost of the per-step probe recorder (Simulation.record_probes) on one GPU.

Times --steps steps between device synchronisations the way bench.py does
(warm-up, graph priming, barrier + synchronize around the timed call), once
per entry of --probes (0 = recorder off) in a fresh simulation each, and
prints one JSON line per entry with the us per step and the difference to the
recorder-off entry of the same invocation.

  python tools/probe_history_cost.py --config wedge15|resonator|scramjet
         [--probes 0,4,64] [--steps 2000] [--warmup 50] [--nx N --ny N]

--sample-monitors (any N-S config): instead, the cost of one call of the
driver's existing monitor sampling in the lean state -- flush, materialise,
gather, synchronous copy, and the re-entry of the next step -- as the
difference between calls of 12 steps with and without a sample after each.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = {"wedge15": (2000, 200), "resonator": (2000, 200), "scramjet": (6000, 400), "step": (1200, 400),
          "triple_point": (4000, 1000)}


def probe_cells(solid, n):
    """n non-solid cells spread over the grid (a lattice of columns and rows)."""
    import numpy as np

    nx, ny = solid.shape
    cells = []
    side = int(np.ceil(np.sqrt(n)))
    for i in np.linspace(1, nx - 2, side).astype(int):
        free = np.flatnonzero(solid[i] == 0.0)
        for j in free[np.linspace(0, len(free) - 1, side).astype(int)]:
            cells.append((int(i), int(j)))
    cells = list(dict.fromkeys(cells))[:n]
    if len(cells) != n:
        raise SystemExit("only %d distinct gas cells found for %d probes" % (len(cells), n))
    return cells


def make(args, hf, decks):
    nx, ny = args.nx or SHAPES[args.config][0], args.ny or SHAPES[args.config][1]
    text = decks.GENERATORS[args.config](nx, ny, nmax=10 ** 9, nout=10 ** 8)
    if args.sample_monitors:
        import numpy as np

        case = hf.native().Case.from_deck(text, ".", False)
        cells = probe_cells(np.asarray(case.field("solid")), 4)
        text = decks.set_key(text, "NumMonitorPoints", len(cells))
        for q, (i, j) in enumerate(cells):
            text = decks.set_key(text, "Point-%d.X" % (q + 1), (i + 0.5) * case.dx)
            text = decks.set_key(text, "Point-%d.Y" % (q + 1), (j + 0.5) * case.dy)
    return hf.Simulation(text, args.backend), nx, ny


def sync(sim):
    if hasattr(sim.solver, "synchronize"):   # (the CPU stepper has nothing in flight)
        sim.solver.synchronize()


def count(sim, name):
    return int(getattr(sim.solver, name, 0))


def prime(sim, args):
    sim.step(args.warmup)
    n = 0
    while n < 120 and getattr(sim.solver, "use_graph", False) and sim.solver.graph_launches < 2:
        sim.step(12)
        n += 12
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="wedge15", choices=sorted(SHAPES))
    ap.add_argument("--probes", default="0,4,64")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--sample-monitors", action="store_true")
    ap.add_argument("--backend", default="gpu", choices=["gpu", "cpu"], help="cpu: a dry run of the script")
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, as bench.py)

    import openhyperflow2d_amd as hf
    from openhyperflow2d_amd.models import decks

    if args.sample_monitors:
        sim, nx, ny = make(args, hf, decks)
        prime(sim, args)
        calls = max(1, args.steps // 12)
        out = {}
        for mode in ("plain", "sampled", "plain", "sampled"):
            sync(sim)
            lns0 = count(sim, "lns_steps") + count(sim, "lnm_steps")
            t0 = time.perf_counter()
            for _ in range(calls):
                sim.step(12)
                if mode == "sampled":
                    sim.solver.sample_monitors()
            sync(sim)
            out.setdefault(mode, []).append(((time.perf_counter() - t0) / calls * 1e6,
                                              count(sim, "lns_steps") + count(sim, "lnm_steps") - lns0))
        best = {m: min(v)[0] for m, v in out.items()}
        print(json.dumps({"config": args.config, "grid": "%dx%d" % (nx, ny), "calls_of_12_steps": calls,
                          "us_per_call_plain": [round(v[0], 2) for v in out["plain"]],
                          "us_per_call_with_sample": [round(v[0], 2) for v in out["sampled"]],
                          "lean_steps_per_block": {m: [v[1] for v in out[m]] for m in out},
                          "us_per_sample_monitors_call": round(best["sampled"] - best["plain"], 2)}), flush=True)
        return

    base = None
    for n in [int(x) for x in args.probes.split(",")]:
        sim, nx, ny = make(args, hf, decks)
        if n:
            sim.record_probes(probe_cells(sim.field("solid"), n), capacity=4096)
        primed = prime(sim, args)
        sync(sim)
        g0 = count(sim, "graph_launches")
        t0 = time.perf_counter()
        sim.step(args.steps)
        sync(sim)
        us = (time.perf_counter() - t0) / args.steps * 1e6
        if n == 0:
            base = us
        rec = {"config": args.config, "grid": "%dx%d" % (nx, ny), "probes": n, "steps": args.steps,
               "warmup": args.warmup, "prime_steps": primed, "us_per_step": round(us, 3),
               "added_us_per_step": None if base is None or n == 0 else round(us - base, 3),
               "graph_launches": count(sim, "graph_launches") - g0,
               "lean_steps": int(count(sim, "lns_steps") + count(sim, "lnm_steps")),
               "tile": dict(getattr(sim.solver, "lean_tile_last", {}))}
        if n:
            h = sim.probe_history()
            rec["recorded"] = h["total"]
            rec["finite"] = bool(np.isfinite(h["values"]).all())
        print(json.dumps(rec), flush=True)
        del sim


if __name__ == "__main__":
    main()
