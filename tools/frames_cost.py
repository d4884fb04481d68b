#!/usr/bin/env python3
"""Cost of the per-step frame recorder (Simulation.record_frames) on one GPU.

Six simulations of the same deck, all in step graphs with the unarmed one's
tile geometry, are timed in turn --rounds times (alternated), --steps steps
between device synchronisations the way bench.py does (warm-up, graph priming,
synchronize around the timed call):

  off       unarmed
  rho       ("rho",) at every = 1
  all1      all ten variables at every = 1
  all10     ... at every = 10
  all100    ... at every = 100
  idle      all ten variables at an `every` the run never reaches: a step that
            is not a sample, which pays the three launches alone

One JSON line gives the us per step of every round of the six, the added us per
step and per sample step (best rounds), the bytes per cell-sample computed from
the shapes, and the rate they amount to against the achievable HBM rate.

  python tools/frames_cost.py --config wedge15|step|resonator|scramjet
         [--steps 2000] [--rounds 3] [--warmup 50] [--nx N --ny N] [--capacity 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = {"wedge15": (2000, 200), "resonator": (2000, 200), "scramjet": (6000, 400), "step": (1200, 400)}
HBM_ACHIEVABLE = 6.3e12   # bytes/s
ROW = 5                   # p, T, rho, U, V


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
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=2)
    ap.add_argument("--backend", default="gpu", choices=["gpu", "cpu"], help="cpu: a dry run of the script")
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, as bench.py)

    import openhyperflow2d_amd as hf
    from openhyperflow2d_amd.models import decks
    from openhyperflow2d_amd.models.simulation import FRAME_VARS

    nx, ny = args.nx or SHAPES[args.config][0], args.ny or SHAPES[args.config][1]
    text = decks.GENERATORS[args.config](nx, ny, nmax=10 ** 9, nout=10 ** 8)
    armed = {"rho": (("rho",), 1), "all1": (FRAME_VARS, 1), "all10": (FRAME_VARS, 10), "all100": (FRAME_VARS, 100),
             "idle": (FRAME_VARS, 10 ** 9)}
    names = ("off",) + tuple(armed)
    sims = {k: hf.Simulation(text, args.backend) for k in names}
    # (the constructor's autotune picks the tile geometry: compare like with like, all in step graphs)
    for k in names:
        sv = sims[k].solver
        for knob in ("lean_cpt", "lean_tj", "lean_nt"):
            if hasattr(sv, knob):
                setattr(sv, knob, getattr(sims["off"].solver, knob))
        if hasattr(sv, "use_graph"):
            sv.use_graph = True
    for k, (vars, every) in armed.items():
        sims[k].record_frames(vars=vars, every=every, capacity=args.capacity)
    primed = {k: prime(s, args) for k, s in sims.items()}
    us = {k: [] for k in names}
    g0 = {k: count(s, "graph_launches") for k, s in sims.items()}
    for _ in range(args.rounds):
        for k in names:
            s = sims[k]
            sync(s)
            t0 = time.perf_counter()
            s.step(args.steps)
            sync(s)
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    h = {k: sims[k].frame_history() for k in armed}
    best = {k: min(v) for k, v in us.items()}
    idle = best["idle"] - best["off"]
    cells = nx * ny
    per_sample, nbytes, rate = {}, {}, {}
    for k, (vars, every) in armed.items():
        if k == "idle":
            continue
        per_sample[k] = (best[k] - best["idle"]) * every + idle
        stencil = any(v not in FRAME_VARS[:ROW] for v in vars)
        # per cell and sample, in 8-byte reals: the rows kernel reads CT and the row's inputs (five stored
        # values on the gather kinds) and writes five scratch planes; the store kernel reads CT and the five
        # planes (its neighbours' loads are other lanes' centre loads) and writes one plane per variable
        nbytes[k] = {"row_inputs": 8 * (1 + ROW), "scratch_written": 8 * ROW, "scratch_read": 8 * ROW + 8,
                     "output": 8 * len(vars), "stencil": stencil}
        total = sum(v for q, v in nbytes[k].items() if q != "stencil")
        nbytes[k]["total"] = total
        rate[k] = total * cells / (per_sample[k] * 1e-6)
    rec = {"config": args.config, "grid": "%dx%d" % (nx, ny), "steps": args.steps, "rounds": args.rounds,
           "warmup": args.warmup, "capacity": args.capacity, "prime_steps": primed,
           "us_per_step": {k: [round(v, 3) for v in us[k]] for k in names},
           "added_us_per_step": {k: round(best[k] - best["off"], 3) for k in armed},
           "added_us_per_sample_step": {k: round(v, 3) for k, v in per_sample.items()},
           "bytes_per_cell_sample": nbytes,
           "achieved_TB_per_s": {k: round(v / 1e12, 3) for k, v in rate.items()},
           "fraction_of_achievable_hbm": {k: round(v / HBM_ACHIEVABLE, 3) for k, v in rate.items()},
           "samples": {k: h[k]["total"] for k in h},
           "finite": bool(all(np.isfinite(v["values"]).all() for v in h.values())),
           "graph_launches": {k: count(s, "graph_launches") - g0[k] for k, s in sims.items()},
           "lean_steps": {k: count(s, "lns_steps") + count(s, "lnm_steps") for k, s in sims.items()},
           "tile": dict(getattr(sims["all1"].solver, "lean_tile_last", {}))}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
