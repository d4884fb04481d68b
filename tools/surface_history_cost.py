#!/usr/bin/env python3
"""Cost of the per-step surface recorder (Simulation.record_surface) on one GPU.

Three simulations of the same deck (its heat-flux keys set: flow 1), one
unarmed, one armed on every node with every=1 and one with every=10, all in
step graphs with the unarmed one's tile geometry, are timed in turn --rounds
times: --steps steps between device synchronisations the way bench.py does
(warm-up, graph priming, synchronize around the timed call).  One JSON line
gives the us per step of every round of the three, the differences of the best
rounds, the plan's sizes, and the only alternative without the recorder:
step(1), a download and the host oracle (Case.surface), per step over
--host-steps steps of a fourth simulation.

  python tools/surface_history_cost.py --config wedge15|step|resonator|scramjet
         [--steps 2000] [--rounds 3] [--warmup 50] [--host-steps 10] [--nx N --ny N]
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
KEYS = [("isOutHeatFluxX", 1), ("Cp_Flow_Index", 1), ("y_min", 0), ("y_max", 10 ** 6), ("isOutHeatFluxY", 1)]


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
    ap.add_argument("--config", default="resonator", choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--host-steps", dest="host_steps", type=int, default=10)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--backend", default="gpu", choices=["gpu", "cpu"], help="cpu: a dry run of the script")
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, as bench.py)

    import openhyperflow2d_amd as hf
    from openhyperflow2d_amd.models import decks

    nx, ny = args.nx or SHAPES[args.config][0], args.ny or SHAPES[args.config][1]
    text = decks.GENERATORS[args.config](nx, ny, nmax=10 ** 9, nout=10 ** 8)
    for k, v in KEYS:
        text = decks.set_key(text, k, v)
    names = ("off", "every1", "every10")
    sims = {k: hf.Simulation(text, args.backend) for k in names}
    # (the constructor's autotune picks the tile geometry: compare like with like, all three in step graphs)
    for k in names:
        sv = sims[k].solver
        for knob in ("lean_cpt", "lean_tj", "lean_nt"):
            if hasattr(sv, knob):
                setattr(sv, knob, getattr(sims["off"].solver, knob))
        if hasattr(sv, "use_graph"):
            sv.use_graph = True
    sims["every1"].record_surface(every=1, capacity=args.capacity)
    sims["every10"].record_surface(every=10, capacity=args.capacity)
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
    h = {k: sims[k].surface_history() for k in names[1:]}
    flags = h["every1"]["flags"]
    rec = {"config": args.config, "grid": "%dx%d" % (nx, ny), "steps": args.steps, "rounds": args.rounds,
           "warmup": args.warmup, "capacity": args.capacity, "prime_steps": primed,
           "us_per_step": {k: [round(v, 3) for v in us[k]] for k in names},
           "added_us_per_step": {k: round(min(us[k]) - min(us["off"]), 3) for k in names[1:]},
           "nodes": int(len(flags)), "nodes_no_slip": int((flags & 1 != 0).sum()),
           "nodes_friction": int((h["every1"]["fric_x"] != 0).sum()),
           "samples": {k: h[k]["total"] for k in h},
           "finite": bool(all(np.isfinite(v["values"]).all() for v in h.values())),
           "graph_launches": {k: count(s, "graph_launches") - g0[k] for k, s in sims.items()},
           "lean_steps": {k: count(s, "lns_steps") + count(s, "lnm_steps") for k, s in sims.items()},
           "tile": dict(getattr(sims["every1"].solver, "lean_tile_last", {}))}
    del sims
    # the alternative: a one-step call, a download and the host oracle, every step
    alt = hf.Simulation(text, args.backend)
    prime(alt, args)
    sync(alt)
    t0 = time.perf_counter()
    for _ in range(args.host_steps):
        alt.step(1)
        alt.solver.download()
        alt.case.surface()
    rec["us_per_step_download_and_host_oracle"] = round((time.perf_counter() - t0) / args.host_steps * 1e6, 1)
    rec["host_steps"] = args.host_steps
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
