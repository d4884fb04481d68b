"""Command-line front end.

  python -m openhyperflow2d_amd run  deck.dat [--backend gpu|cpu|ref] [--cycles N]
                                     [--outdir DIR] [--semantics mpi|serial]
                                     [--no-checkpoint] [--no-lean] [--metrics FILE]
                                     [--profile FILE] [--fault-inject step:N,rank:R,kind:nan|kill]
                                     [--transport p2p|rccl]
                                     [--probe-history FILE.npz [--probe-capacity N]]
                                     [--load-history FILE.npz [--load-capacity N]]
                                     [--wall-heat FILE.npz [--wall-heat-every K] [--wall-heat-capacity N]]
                                     [--surface FILE.npz [--surface-every K] [--surface-capacity N]]
                                     [--frames FILE.npz [--frames-vars a,b,...] [--frames-every K]
                                      [--frames-capacity N] [--frames-stride SI,SJ]]
                                     [--averages FILE.npz [--averages-every K] [--averages-favre]
                                      [--averages-species all|A,B,...]]
  python -m openhyperflow2d_amd deck wedge15 --nx 2000 --ny 200 -o w.dat
  python -m openhyperflow2d_amd info deck.dat
  python -m openhyperflow2d_amd build

`run` is the reference driver (hf2d_start.cpp:32-368: pre-processing, outer
cycles of Nmax DEEPS steps, RMS/monitor/field/transient outputs, .hf2d
checkpoint and restart, exit monitor).  Launched under torchrun
(WORLD_SIZE > 1) it runs one x-strip per rank -- one GPU per process with the
device halo exchange over RCCL, or CPU ranks over gloo -- and rank 0 writes
the gathered outputs.  SIGINT/SIGTERM finish the cycle, write the outputs
and the checkpoint, then exit 0.  The native CLI `openhyperflow2d_amd/bin/hf2d`
offers the same single-process driver without Python.
"""
from __future__ import annotations

import argparse
import os
import sys


def _cmd_run(a) -> int:
    import openhyperflow2d_amd as hf

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    with open(a.deck, errors="replace") as f:
        text = f.read()
    workdir = os.path.dirname(os.path.abspath(a.deck))
    outdir = a.outdir or workdir
    os.makedirs(outdir, exist_ok=True)
    nat = hf.native()
    backend = a.backend or ("gpu" if hf.gpu_available() else "cpu")
    if a.probe_history and world > 1:
        if rank == 0:
            print("--probe-history records in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if a.load_history and world > 1:
        if rank == 0:
            print("--load-history records in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if a.wall_heat and world > 1:
        if rank == 0:
            print("--wall-heat records in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if a.surface and world > 1:
        if rank == 0:
            print("--surface records in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if a.frames and world > 1:
        if rank == 0:
            print("--frames records in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if a.averages and world > 1:
        if rank == 0:
            print("--averages accumulates in one process only; this is a %d-rank launch "
                  "(run the deck without torchrun, or drop the option)" % world, file=sys.stderr, flush=True)
        return 2
    if world > 1:
        import torch
        import torch.distributed as dist

        from .parallel.dist import DistributedSimulation

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "gpu":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        sim = DistributedSimulation(text, backend, rank=rank, world=world, device=local_rank,
                                    semantics=a.semantics, lean=not a.no_lean, workdir=workdir,
                                    use_checkpoint=not a.no_checkpoint, transport=a.transport)
    else:
        sim = hf.Simulation(text, backend, workdir=workdir, use_checkpoint=not a.no_checkpoint,
                            semantics=a.semantics, device=a.device,
                            lean=(not a.no_lean) if backend != "ref" else None)
    nat.install_signal_handlers()
    if rank == 0:
        print("hf2d: %s  %dx%d  backend=%s  ranks=%d" % (os.path.basename(a.deck), sim.case.nx, sim.case.ny,
                                                          backend, world), flush=True)
    probe_cells = []
    if a.probe_history:
        # the deck's monitor points, every step (Monitors-<P>.plt keeps its NOutStep cadence)
        probe_cells = sim.monitor_cells()
        try:
            sim.record_probes(probe_cells, a.probe_capacity)
        except (ValueError, RuntimeError) as e:
            print("--probe-history: %s" % e, file=sys.stderr, flush=True)
            return 2
    load_boxes, load_cuts = [], []
    if a.load_history:
        # what the driver integrates once per cycle, every step: the body box
        # (is_Cx_calc), the X cuts and the nozzle cut (is_Cd_calc)
        load_boxes, load_cuts = (list(v) for v in sim.case.load_targets)
        try:
            sim.record_loads(load_boxes, load_cuts, a.load_capacity)
        except (ValueError, RuntimeError) as e:
            print("--load-history: %s" % e, file=sys.stderr, flush=True)
            return 2
    if a.wall_heat:
        # the deck's own profiles, every K-th step: X only where the driver writes HeatFlux-X
        keys = sim.case.wall_heat_keys
        try:
            sim.record_wall_heat(x=bool(keys["isOutHeatFluxX"]), y=True, every=a.wall_heat_every,
                                 capacity=a.wall_heat_capacity)
        except (ValueError, RuntimeError) as e:
            print("--wall-heat: %s" % e, file=sys.stderr, flush=True)
            return 2
    if a.surface:
        # the nodes of the deck's body box (is_Cx_calc), else every node; the deck's Cp flow where it names one
        boxes = sim.case.load_targets[0] or None
        keys = sim.case.wall_heat_keys
        flow = keys["Cp_Flow_Index"] if 1 <= keys["Cp_Flow_Index"] <= keys["flows"] else 1
        try:
            sim.record_surface(boxes=boxes, cp_flow=flow, every=a.surface_every, capacity=a.surface_capacity)
        except (ValueError, RuntimeError) as e:
            print("--surface: %s" % e, file=sys.stderr, flush=True)
            return 2
    if a.frames:
        try:
            stride = tuple(int(v) for v in a.frames_stride.split(","))
            if len(stride) != 2:
                raise ValueError("--frames-stride is SI,SJ, not %r" % a.frames_stride)
            sim.record_frames(vars=[v.strip() for v in a.frames_vars.split(",") if v.strip()], stride=stride,
                              every=a.frames_every, capacity=a.frames_capacity)
        except (ValueError, RuntimeError) as e:
            print("--frames: %s" % e, file=sys.stderr, flush=True)
            return 2
    if a.averages:
        try:
            sp = a.averages_species
            if sp is not None and sp != "all":
                sp = [s.strip() for s in sp.split(",") if s.strip()]
            sim.start_averaging(every=a.averages_every, favre=a.averages_favre, species=sp)
        except (ValueError, RuntimeError) as e:
            print("--averages: %s" % e, file=sys.stderr, flush=True)
            return 2
    try:
        cycles, log = sim.run(max_cycles=a.cycles, outdir=outdir, outputs=True, checkpoint=not a.no_checkpoint,
                              verbose=True, metrics=a.metrics or "", profile=a.profile or "",
                              fault=a.fault_inject or "")
    except RuntimeError as e:
        print(str(e), file=sys.stderr, flush=True)
        return 3
    if a.probe_history:
        import numpy as np

        from .models.simulation import PROBE_VARS

        h = sim.probe_history()
        with open(a.probe_history, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, times=h["times"], values=h["values"], cells=np.asarray(probe_cells, dtype=np.int64),
                     vars=np.asarray(PROBE_VARS), total=np.int64(h["total"]))
        print("probe history: %d of %d steps x %d points -> %s" % (h["values"].shape[0], h["total"], len(probe_cells),
                                                                    a.probe_history), flush=True)
    if a.load_history:
        import numpy as np

        from .models.simulation import LOAD_PARTS

        h = sim.load_history()
        with open(a.load_history, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, times=h["times"], forces=h["forces"], mass_flow=h["mass_flow"],
                     box_terms=h["terms"]["box_terms"], cut_terms=h["terms"]["cut_terms"], span=h["span"],
                     total=np.int64(h["total"]), boxes=np.asarray(load_boxes, dtype=np.float64).reshape(-1, 4),
                     cuts=np.asarray(load_cuts, dtype=np.float64).reshape(-1, 3), parts=np.asarray(LOAD_PARTS))
        print("load history: %d of %d steps x %d boxes, %d cuts -> %s" % (h["times"].shape[0], h["total"],
                                                                           len(load_boxes), len(load_cuts),
                                                                           a.load_history), flush=True)
    if a.wall_heat:
        import numpy as np

        from .models.simulation import WALL_HEAT_X

        h = sim.wall_heat_history()
        with open(a.wall_heat, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, vars=np.asarray(WALL_HEAT_X), **{k: np.asarray(v) for k, v in h.items()})
        print("wall heat: %d of %d samples x (4 x %d + %d) entries -> %s" % (h["times"].shape[0], h["total"],
                                                                            h["x"].shape[2], h["y"].shape[1],
                                                                            a.wall_heat), flush=True)
    if a.surface:
        import numpy as np

        from .models.simulation import SURFACE_VARS

        h = sim.surface_history()
        with open(a.surface, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, vars=np.asarray(SURFACE_VARS), **{k: np.asarray(v) for k, v in h.items()})
        print("surface: %d of %d samples x 10 x %d nodes -> %s" % (h["times"].shape[0], h["total"],
                                                                   h["values"].shape[2], a.surface), flush=True)
    if a.frames:
        import numpy as np

        h = sim.frame_history()
        with open(a.frames, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, **{k: np.asarray(v) for k, v in h.items()})
        print("frames: %d of %d samples x %d x %d x %d -> %s" % ((h["times"].shape[0], h["total"]) +
                                                                 h["values"].shape[1:] + (a.frames,)), flush=True)
    if a.averages:
        import numpy as np

        from .models.simulation import PROBE_VARS

        av = sim.averages()
        # (the keys of --averages-favre / --averages-species only when the flags were given)
        extra = {k: np.asarray(av[k]) for k in ("species", "species_mean", "species_var", "favre_vars", "favre_mean",
                                                 "favre_var", "favre_cov_uv", "favre_weight") if k in av}
        with open(a.averages, "wb") as f:   # (np.savez on a path would append ".npz")
            np.savez(f, mean=av["mean"], var=av["var"], cov_uv=av["cov_uv"], vars=np.asarray(PROBE_VARS),
                     time=np.float64(av["time"]), samples=np.int64(av["samples"]), **extra)
        print("averages: %d samples over t = %.6e -> %s" % (av["samples"], av["time"], a.averages), flush=True)
    if rank == 0:
        sys.stdout.write(log)
        print("\nReady. Computation finished (%d cycles)." % cycles, flush=True)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def _cmd_deck(a) -> int:
    from .models import decks

    gen = decks.GENERATORS[a.name]
    kw = {}
    if a.nx:
        kw["nx"] = a.nx
    if a.ny:
        kw["ny"] = a.ny
    text = gen(**kw)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


def _cmd_info(a) -> int:
    import openhyperflow2d_amd as hf

    nat = hf.native()
    with open(a.deck, errors="replace") as f:
        text = f.read()
    case = nat.Case.from_deck(text, os.path.dirname(os.path.abspath(a.deck)), False)
    import numpy as np

    solid = np.asarray(case.field("solid"))
    print("project      %s" % case.project)
    print("grid         %d x %d  (dx=%g, dy=%g)" % (case.nx, case.ny, case.dx, case.dy))
    print("problem      %s, %s" % ("Navier-Stokes" if case.problem_type == 1 else "Euler",
                                   "axisymmetric" if case.flow_type else "flat"))
    print("solid cells  %d (%.1f%%)" % (solid.sum(), 100 * solid.mean()))
    print("dt0          %g s" % case.dt0)
    print("Nmax         %d" % case.nmax)
    return 0


def _cmd_build(a) -> int:
    from . import _build

    print(_build.build(verbose=True))
    return 0


def _cmd_chem(a) -> int:
    """K12 kinetics operator on the GPU: time one call on a synthetic field, check vs the FP64 oracle."""
    import json

    from .ops import chemistry as ch
    from .ops import mechanism as mech

    m = mech.Mechanism.load(a.mech) if a.mech else mech.h2_air_li2004()
    if a.save_builtin:
        mech.h2_air_li2004().save(a.save_builtin)
        return 0
    res = ch.benchmark(m, a.nx * a.ny, a.dt, a.nsub, a.repeats, kernel=a.kernel)
    print(json.dumps(res))
    return 0 if res["incr_err_vs_numpy_fp64"] < 1e-7 else 1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m openhyperflow2d_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run", help="run a .dat deck (reference driver)")
    r.add_argument("deck")
    r.add_argument("--backend", choices=["gpu", "cpu", "ref"])
    r.add_argument("--cycles", type=int, default=-1, help="stop after N outer cycles (-1: exit monitor)")
    r.add_argument("--outdir")
    r.add_argument("--semantics", default="mpi", choices=["mpi", "serial"])
    r.add_argument("--no-checkpoint", action="store_true")
    r.add_argument("--no-lean", action="store_true")
    r.add_argument("--device", type=int, default=0)
    r.add_argument("--metrics", help="append per-output-step JSON lines to this file")
    r.add_argument("--profile", help="write per-phase wall-clock JSON (steps/sync/gather/outputs) to this file")
    r.add_argument("--fault-inject", dest="fault_inject", metavar="SPEC",
                   help="step:N[,rank:R][,kind:nan|kill] -- test hook for the failure/restart paths")
    r.add_argument("--transport", choices=["p2p", "rccl"], help="multi-GPU exchange (default p2p)")
    r.add_argument("--probe-history", dest="probe_history", metavar="FILE.npz",
                   help="record p, T, rho, U, V at the deck's monitor points after every step (one process only) "
                        "and write times / values / cells / vars to this file")
    r.add_argument("--probe-capacity", dest="probe_capacity", type=int, default=4096, metavar="N",
                   help="rows the recorder keeps: the last N steps (default 4096)")
    r.add_argument("--load-history", dest="load_history", metavar="FILE.npz",
                   help="record the body force parts of the deck's body box (is_Cx_calc) and the mass flow through "
                        "its X cuts and the nozzle cut after every step (one process only) and write times / forces / "
                        "mass_flow / box_terms / cut_terms / span / total / boxes / cuts / parts to this file")
    r.add_argument("--load-capacity", dest="load_capacity", type=int, default=4096, metavar="N",
                   help="rows the load recorder keeps: the last N steps (default 4096)")
    r.add_argument("--wall-heat", dest="wall_heat", metavar="FILE.npz",
                   help="record the HeatFlux-X profile (Q, Alpha, Cp, St per column; only when isOutHeatFluxX is set) "
                        "and the HeatFlux-Y profile with the deck's Cp_Flow_Index / y_min / y_max after every K-th "
                        "step (one process only) and write times / x / y / total / x_nodes / y_nodes, the running "
                        "mean_ / var_ / peak_ / peak_time_ of both, time, samples and vars to this file")
    r.add_argument("--wall-heat-every", dest="wall_heat_every", type=int, default=1, metavar="K",
                   help="sample every K-th step (default 1)")
    r.add_argument("--wall-heat-capacity", dest="wall_heat_capacity", type=int, default=4096, metavar="N",
                   help="rows the wall heat recorder keeps: the last N samples (default 4096; 0: statistics only)")
    r.add_argument("--surface", metavar="FILE.npz",
                   help="record p, Cp, T, tau_x, tau_y, Cf_x, Cf_y, q_y, q_x, St of every wall node of the deck's body "
                        "box (is_Cx_calc; else of the whole field) after every K-th step (one process only) and write "
                        "times / values / total, the node table (i, j, x, y, flags, face_x, face_y, fric_x, fric_y, "
                        "box_off), the running mean / var / peak / peak_time, time, samples and vars to this file")
    r.add_argument("--surface-every", dest="surface_every", type=int, default=1, metavar="K",
                   help="sample every K-th step (default 1)")
    r.add_argument("--surface-capacity", dest="surface_capacity", type=int, default=4096, metavar="N",
                   help="rows the surface recorder keeps: the last N samples (default 4096; 0: statistics only)")
    r.add_argument("--frames", metavar="FILE.npz",
                   help="record whole-field frames of the listed variables after every K-th step (one process only) "
                        "and write times / values [n, nvars, ni, nj] / total / vars / i / j / x / y / gas to this file")
    r.add_argument("--frames-vars", dest="frames_vars", default="rho,grad_rho", metavar="a,b,...",
                   help="variables out of p, T, rho, U, V, grad_rho, grad_p, vorticity, dilatation, ducros "
                        "(default rho,grad_rho)")
    r.add_argument("--frames-every", dest="frames_every", type=int, default=1, metavar="K",
                   help="sample every K-th step (default 1)")
    r.add_argument("--frames-capacity", dest="frames_capacity", type=int, default=16, metavar="N",
                   help="frames the recorder keeps: the last N samples (default 16)")
    r.add_argument("--frames-stride", dest="frames_stride", default="1,1", metavar="SI,SJ",
                   help="keep every SI-th column and SJ-th row (default 1,1; gradients use the immediate neighbours)")
    r.add_argument("--averages", metavar="FILE.npz",
                   help="accumulate time-averaged p, T, rho, U, V, their variances and the U-V covariance over the "
                        "whole field at every step (one process only) and write mean / var / cov_uv / vars / time / "
                        "samples to this file")
    r.add_argument("--averages-every", dest="averages_every", type=int, default=1, metavar="K",
                   help="sample every K-th step (default 1)")
    r.add_argument("--averages-favre", dest="averages_favre", action="store_true",
                   help="with --averages: also the density-weighted (Favre) means and variances of T, U, V and the "
                        "listed species and the Favre U-V covariance (favre_vars / favre_mean / favre_var / "
                        "favre_cov_uv / favre_weight)")
    r.add_argument("--averages-species", dest="averages_species", metavar="all|A,B,...",
                   help="with --averages, mechanism decks only: also the mean and variance of these species' mass "
                        "fractions (species / species_mean / species_var)")
    d = sub.add_parser("deck", help="write a generated deck")
    d.add_argument("name")
    d.add_argument("--nx", type=int)
    d.add_argument("--ny", type=int)
    d.add_argument("-o", "--output")
    i = sub.add_parser("info", help="pre-process a deck and print a summary")
    i.add_argument("deck")
    sub.add_parser("build", help="build the native extension and CLIs")
    c = sub.add_parser("chem", help="run/benchmark the K12 kinetics kernels on a mechanism")
    c.add_argument("--mech", help="mechanism file (.mech); default: the built-in Li et al. 2004 H2/air set")
    c.add_argument("--kernel", default="mfma", choices=["mfma", "fast"],
                   help="mfma: runtime-mechanism MFMA kernel; fast: compiled-mechanism kernel")
    c.add_argument("--save-builtin", dest="save_builtin", metavar="PATH", help="write the built-in mechanism and exit")
    c.add_argument("--nx", type=int, default=6000)
    c.add_argument("--ny", type=int, default=400)
    c.add_argument("--nsub", type=int, default=1)
    c.add_argument("--dt", type=float, default=1e-7)
    c.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args(argv)
    return {"run": _cmd_run, "deck": _cmd_deck, "info": _cmd_info, "build": _cmd_build, "chem": _cmd_chem}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())
