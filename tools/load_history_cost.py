#!/usr/bin/env python3
"""Cost of the per-step load recorder (Simulation.record_loads) on one GPU.

Two simulations of the same deck, one armed with a whole-domain box and three
x cuts (a quarter, half and three quarters of the length, full height), one
not, are timed in turn --rounds times: --steps steps between device
synchronisations the way bench.py does (warm-up, graph priming, synchronize
around the timed call).  One JSON line gives the us per step of every round
of both, the difference of the best rounds, the number of terms per step, and
the only alternative without the recorder: step(1), a download and the host
integrals (Case.force_parts, Case.mass_flow_x), per step over --host-steps
steps of a third simulation.

  python tools/load_history_cost.py --config wedge15|step|scramjet|resonator|triple_point
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

SHAPES = {"wedge15": (2000, 200), "resonator": (2000, 200), "scramjet": (6000, 400), "step": (1200, 400),
          "triple_point": (4000, 1000)}


def targets(case):
    L, H = case.nx * case.dx, case.ny * case.dy
    return [(0.0, 0.0, 2 * L, 2 * H)], [(f * L, 0.0, 2 * H) for f in (0.25, 0.5, 0.75)]


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
    ap.add_argument("--host-steps", dest="host_steps", type=int, default=10)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--backend", default="gpu", choices=["gpu", "cpu"], help="cpu: a dry run of the script")
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, as bench.py)

    import openhyperflow2d_amd as hf
    from openhyperflow2d_amd.models import decks

    nx, ny = args.nx or SHAPES[args.config][0], args.ny or SHAPES[args.config][1]
    text = decks.GENERATORS[args.config](nx, ny, nmax=10 ** 9, nout=10 ** 8)
    sims = {"off": hf.Simulation(text, args.backend), "armed": hf.Simulation(text, args.backend)}
    # (the constructor's autotune times graphs on / off and the tile geometry: compare like with like)
    tuned = {k: [bool(getattr(s.solver, "use_graph", False))] for k, s in sims.items()}
    for knob in ("use_graph", "lean_cpt", "lean_tj", "lean_nt"):
        if hasattr(sims["off"].solver, knob):
            setattr(sims["armed"].solver, knob, getattr(sims["off"].solver, knob))
    boxes, cuts = targets(sims["armed"].case)
    sims["armed"].record_loads(boxes, cuts, capacity=4096)
    primed = {k: prime(s, args) for k, s in sims.items()}
    us = {"off": [], "armed": []}
    g0 = {k: count(s, "graph_launches") for k, s in sims.items()}
    for _ in range(args.rounds):
        for k in ("off", "armed"):
            s = sims[k]
            sync(s)
            t0 = time.perf_counter()
            s.step(args.steps)
            sync(s)
            us[k].append((time.perf_counter() - t0) / args.steps * 1e6)
    h = sims["armed"].load_history()
    for k, s in sims.items():
        tuned[k].append(bool(getattr(s.solver, "use_graph", False)))
    rec = {"use_graph_tuned_then_after": tuned, "config": args.config, "grid": "%dx%d" % (nx, ny), "steps": args.steps, "rounds": args.rounds,
           "warmup": args.warmup, "prime_steps": primed,
           "us_per_step_off": [round(v, 3) for v in us["off"]], "us_per_step_armed": [round(v, 3) for v in us["armed"]],
           "added_us_per_step": round(min(us["armed"]) - min(us["off"]), 3),
           "terms_per_step": int(h["terms"]["box_terms"].sum() + h["terms"]["cut_terms"].sum()),
           "box_terms": h["terms"]["box_terms"].tolist(), "cut_terms": h["terms"]["cut_terms"].tolist(),
           "recorded": h["total"], "finite": bool(np.isfinite(h["forces"]).all() and np.isfinite(h["mass_flow"]).all()),
           "graph_launches": {k: count(s, "graph_launches") - g0[k] for k, s in sims.items()},
           "lean_steps": {k: count(s, "lns_steps") + count(s, "lnm_steps") for k, s in sims.items()},
           "tile": dict(getattr(sims["armed"].solver, "lean_tile_last", {}))}
    del sims
    # the alternative: a one-step call, a download and the host integrals, every step
    alt = hf.Simulation(text, args.backend)
    prime(alt, args)
    sync(alt)
    t0 = time.perf_counter()
    for _ in range(args.host_steps):
        alt.step(1)
        alt.solver.download()
        for b in boxes:
            alt.case.force_parts(*b)
        for c in cuts:
            alt.case.mass_flow_x(*c)
    rec["us_per_step_download_and_host_integrals"] = round((time.perf_counter() - t0) / args.host_steps * 1e6, 1)
    rec["host_steps"] = args.host_steps
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
