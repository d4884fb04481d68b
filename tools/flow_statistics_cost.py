#!/usr/bin/env python3
"""Cost of the whole-field accumulator (Simulation.start_averaging) on one GPU.

One simulation per invocation (so every entry runs with the same tuned
kernel geometry), warmed up and primed the way bench.py does.  Each entry
times --steps steps between device synchronisations, --repeats times, and
prints one JSON line: the us per step of every repeat, their median and the
difference to the accumulator-off entry.  Entries: off, then second moments
on / off x every = 1 / 10, then off again.

From the every = 1 and every = 10 entries of one variant the accumulate
kernel's own time K follows without a profiler: a sample step adds L + K (L:
the two launches and the tick), a step that is no sample adds L, so
added(1) = L + K and added(10) = L + K / 10.

In the same run a plain device copy that moves the same byte count
((5 + listed species + 2 * planes) * 8 * cells, read + write: a copy of half of it) is timed
with the same sync points, and the kernel's bytes / s are set against the
copy's.

With --favre and / or --species (all | A,B,...; mechanism decks only) the
entries are instead: off, the base accumulator (second moments) every 1 / 10,
the same with the options armed (hf2d_stats_accum_x) every 1 / 10, off again,
so the extended pass stands next to the unarmed run and the base accumulator
of the same simulation.  Every kernel entry also gives planes * 16 B * cells
over the kernel's time (plane_GBps: the planes' read + write alone).

  python tools/flow_statistics_cost.py --config wedge15|resonator|scramjet
         [--steps 2000] [--warmup 50] [--repeats 3] [--nx N --ny N]
         [--favre] [--species all|A,B,...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = {"wedge15": (2000, 200), "resonator": (2000, 200), "scramjet": (6000, 400), "step": (1200, 400),
          "triple_point": (4000, 1000)}


def sync(sim):
    if hasattr(sim.solver, "synchronize"):   # (the CPU stepper has nothing in flight)
        sim.solver.synchronize()


def prime(sim, warmup):
    sim.step(warmup)
    n = 0
    while n < 120 and getattr(sim.solver, "use_graph", False) and sim.solver.graph_launches < 2:
        sim.step(12)
        n += 12


def timed(sim, steps, repeats):
    out = []
    for _ in range(repeats):
        sync(sim)
        t0 = time.perf_counter()
        sim.step(steps)
        sync(sim)
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return out


def copy_rate(nbytes, repeats):
    """us of one device copy that reads nbytes / 2 and writes nbytes / 2 (median of `repeats` blocks of 50)."""
    import torch

    n = max(nbytes // 16, 1)
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(10):
        dst.copy_(src)
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            dst.copy_(src)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / 50 * 1e6)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="wedge15", choices=sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--favre", action="store_true", help="also time the accumulator with favre=True")
    ap.add_argument("--species", default="", help="also time it with these species (all | A,B,...)")
    ap.add_argument("--backend", default="gpu", choices=["gpu", "cpu"], help="cpu: a dry run of the script")
    args = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (HIP runtime first, as bench.py)

    import openhyperflow2d_amd as hf
    from openhyperflow2d_amd.models import decks

    nx, ny = args.nx or SHAPES[args.config][0], args.ny or SHAPES[args.config][1]
    sim = hf.Simulation(decks.GENERATORS[args.config](nx, ny, nmax=10 ** 9, nout=10 ** 8), args.backend)
    gas = int((sim.field("solid") == 0.0).sum())
    prime(sim, args.warmup)
    head = {"config": args.config, "grid": "%dx%d" % (nx, ny), "cells": nx * ny, "gas_cells": gas,
            "steps": args.steps, "warmup": args.warmup}

    def entry(tag, **kw):
        us = timed(sim, args.steps, args.repeats)
        rec = dict(head, entry=tag, us_per_step=[round(u, 3) for u in us], median=round(statistics.median(us), 3),
                   graph=bool(getattr(sim.solver, "use_graph", False)),
                   lean_steps=int(getattr(sim.solver, "lns_steps", 0) + getattr(sim.solver, "lnm_steps", 0)), **kw)
        return rec

    species = None
    if args.species:
        species = "all" if args.species == "all" else [q for q in args.species.split(",") if q]
    ns = (len(sim.case.mech_species) if species == "all" else len(species)) if species else 0
    ext = args.favre or ns > 0

    def plane_count(second, favre, nsp):
        n = (11 if second else 5) + nsp * (2 if second else 1)
        if favre:
            n += 1 + (3 + nsp) * (2 if second else 1) + (1 if second else 0)
        return n

    # (second moments, favre, species): the base variants, or base and extended side by side
    variants = [(True, False, None), (True, args.favre, species) if ext else (False, False, None)]
    off = entry("off")
    print(json.dumps(off), flush=True)
    added = {}
    for second, favre, sp in variants:
        nsp = ns if sp else 0
        planes = plane_count(second, favre, nsp)
        nbytes = (5 + nsp + 2 * planes) * 8 * nx * ny   # the row, the listed partial densities, every plane read + written
        opts = dict(second_moments=second, favre=bool(favre), species=nsp, planes=planes)
        for every in (1, 10):
            sim.start_averaging(every=every, second_moments=second, favre=bool(favre), species=sp)
            prime(sim, 24)   # (arming dropped the cached graph windows)
            rec = entry("on", every=every, bytes_per_sample=nbytes, **opts)
            a = sim.averages()
            sim.stop_averaging()
            rec["added_us_per_step"] = round(rec["median"] - off["median"], 3)
            rec["samples"] = a["samples"]
            rec["finite"] = bool(all(np.isfinite(a[k]).all() for k in a if k.endswith("mean")))
            added[every] = rec["added_us_per_step"]
            print(json.dumps(rec), flush=True)
        a1, a10 = added[1], added[10]
        k_us = (a1 - a10) / 0.9
        rec = dict(head, entry="kernel", bytes_per_sample=nbytes, kernel_us=round(k_us, 3),
                   launch_us=round(a1 - k_us, 3), kernel_GBps=round(nbytes / max(k_us, 1e-9) / 1e3, 1),
                   plane_GBps=round(planes * 16 * nx * ny / max(k_us, 1e-9) / 1e3, 1), **opts)
        if args.backend == "gpu":
            cp = copy_rate(nbytes, args.repeats)
            rec["copy_us"] = [round(c, 3) for c in cp]
            rec["copy_GBps"] = round(nbytes / statistics.median(cp) / 1e3, 1)
            rec["kernel_over_copy_rate"] = round(rec["kernel_GBps"] / rec["copy_GBps"], 3)
        print(json.dumps(rec), flush=True)
    print(json.dumps(entry("off_again")), flush=True)


if __name__ == "__main__":
    main()
