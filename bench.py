#!/usr/bin/env python3
"""Headline benchmark: particle-steps/s of the direct-sum leapfrog at N = 65 536, fp64.

    python bench.py --gpus 1 --steps 2000 --warmup 50
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one GalaxySimulation.step() (kick-drift-force-kick) over the whole galaxy:
BASELINE.json config 2 -- N=65 536 synthetic disk galaxy, fp32 initial conditions, FLOAT64
mode, G=1e-3, softening=0.1, dt=0.01.  With N GPUs the SAME galaxy is stepped with the pair
work partitioned over the ranks (snake-dealt target super-rows of the pair-symmetric kernel)
and one all-reduce of the force vectors per step (RCCL or the direct xGMI kernel; strong scaling).  The state is resident
in HBM before the timed region starts; the K timed steps are ONE native call (nb_step)
bracketed by barrier + device sync.  `python bench.py --gpus N` without RANK in the
environment starts the N ranks itself (a child `python -m torch.distributed.run`, before this
process touches torch or HIP) and relays rank 0's JSON line.

Rank 0 prints one JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...) with
  roofline      dominant kernel (force_sym_kernel<double,...>; the line names the one that ran)
                algorithmic fp64 flop (14 per ordered pair) / its HIP-event
                duration measured inside this run, against the fp64 vector peak of MI355X.
A plain run does only that: set-up, warm-up, the K timed steps, the line.  `--full` adds what takes
work of its own:
  energy_drift_rel_timed_region  total energy before / after the timed steps.
  collective    (runs with a communicator) what the per-step all-reduce is and costs on the node.
  cpu_baseline  the CPU oracle (oracle/, "port" of the reference's algorithm, OpenMP over all
                host cores) timed on a bounded sample of the same workload (rank 0, N=1 only),
                the energy drift of the GPU run against the oracle's over those same steps, and
                the reference's own materialised-tensor formulation timed per SURVEY.md 8(d).
  gpu_rows, modes  this engine at the cpu_baseline sizes, and every precision mode at N = 65 536.
`--dump-outputs DIR` writes the state the timed steps leave (positions, velocities, accelerations) as
DIR/<name>.npy; the inputs are seeded, so two builds can be compared array for array.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK_TFLOPS = 78.6     # MI355X fp64 vector (= fp64 matrix) peak, AMD spec; SURVEY.md 8d
FP32_VECTOR_PEAK_TFLOPS = 157.3    # /opt/skills/guides/MI355X_MICROARCH.md
FLOP_PER_PAIR_2D = 14              # 5*D + 4, SURVEY.md section 8d
SPINUP_EVALS = 40                  # untimed force evaluations (incl. warm-up steps) before the timed region
DUMP_BYTES = 60 * 10 ** 6          # --dump-outputs: at most this much in all (larger runs: a seeded sample of rows)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000, help="timed steps (default: the 2 000 ticks of BASELINE config 2)")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--n", "--particles", dest="n", type=int, default=65536,
                    help="particles (default: BASELINE config 2); use --particles under torch.distributed.run, whose\n"
                         "own parser takes --n for an abbreviation of --nnodes")
    ap.add_argument("--mode", default="float64")
    ap.add_argument("--full", action="store_true",
                    help="also the energy drift, the collective report, the CPU baseline, gpu_rows and modes")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the state the timed steps leave as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline, gpu_rows and modes")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline sample length (--full)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch plumbing only: rendezvous (gloo when there is no GPU), barrier, one JSON line; no HIP work")
    ap.add_argument("--ref-sizes", default="1024,4096,8192",
                    help="sizes at which the reference's materialised torch formulation is timed (SURVEY.md 8d, --full); "
                         "'' = skip")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def self_launch(args):
    """`python bench.py --gpus N` outside torch.distributed.run: start the N ranks as a CHILD process (nothing
    in this process has touched torch or HIP yet, and nothing will), relay its output, return its exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    json_lines = [ln for ln in lines if ln.lstrip().startswith("{")]
    for ln in lines:
        if ln not in json_lines:
            print(ln, file=sys.stderr)
    if json_lines:
        print(json_lines[-1], flush=True)          # rank 0's bench line
    return proc.returncode


def host_cores():
    """Cores this process may really use: the affinity mask, capped by the cgroup CPU quota when one is set
    (a 1-GPU box of the pool exposes 128 logical CPUs but grants a share of them)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(pos, vel, mass, target_s, ref_sizes, gpu_drift):
    """Oracle (C port of the reference algorithm, all host cores) on a bounded sample of the bench workload;
    `gpu_drift(steps)` returns the GPU engine's relative energy drift over the same steps from the same ICs."""
    import numpy as np
    cores = host_cores()
    os.environ.setdefault("OMP_NUM_THREADS", str(cores))       # before the oracle's OpenMP runtime starts
    from oracle import oracle as O
    p = np.ascontiguousarray(pos.double().numpy())
    v = np.ascontiguousarray(vel.double().numpy())
    m = np.ascontiguousarray(mass.double().numpy())
    n, d = p.shape
    lib = O.lib()
    try:                                  # torch has usually started the OpenMP runtime already: set it directly
        import ctypes
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(cores)
    except OSError:
        pass
    acc = np.empty_like(p)
    t0 = time.perf_counter()
    lib.nbo_accelerations_f64_fast(n, d, O._dp(p), O._dp(m), 0.001, 0.1 ** 2, 0, n, O._dp(acc))
    t_first = time.perf_counter() - t0
    steps = max(1, min(50, int(target_s / max(t_first, 1e-3))))

    def energy():
        ke = lib.nbo_kinetic_energy(n, d, O.F64, O._dp(v), O.F64, O._dp(m))
        return ke + O.potential_energy_f64_fast(p, m)

    e0 = energy()
    t0 = time.perf_counter()
    lib.nbo_step_f64_fast(n, d, O._dp(p), O._dp(v), O._dp(m), O._dp(acc), 0.001, 0.1 ** 2, 0.01, steps)
    dt = time.perf_counter() - t0
    drift_oracle = (energy() - e0) / abs(e0)
    drift_gpu = gpu_drift(steps)
    # The reference's own (materialised N x N x D torch) formulation cannot reach N = 65536; SURVEY.md section 8(d)
    # prescribes timing it at N in {1024, 4096, 8192}, fp64 and fp32, omega_point_test.py:305-319 idiom
    # (10 warm-up steps, perf_counter, >= 10 steps), thread count stated.
    ref_form = []
    try:
        import torch
        from oracle import torch_materialised as TM
        threads = min(torch.get_num_threads(), cores)
        for nr in ref_sizes:
            for mode in ("float64", "float32"):
                rt, used = TM.time_steps(pos[:nr].clone(), vel[:nr].clone(), mass[:nr].clone(), steps=10, warmup=10,
                                         mode=mode, threads=threads)
                ref_form.append({"n": nr, "mode": mode, "ms_per_step": rt / 10 * 1e3, "particle_steps_per_s": nr * 10 / rt,
                                 "pair_interactions_per_s": float(nr) * nr * 10 / rt, "threads": used})
    except Exception as exc:            # never let the context measurement break the bench line
        ref_form.append({"error": repr(exc)})
    return {
        "value": n * steps / dt, "unit": "particle-steps/s", "cores": O.num_threads(), "host_cores_available": cores, "kind": "port",
        "sample": f"N={n} fp64 disk galaxy, {steps} leapfrog steps of the oracle's OpenMP fast path "
                  f"({dt:.1f} s; the reference's own PyTorch formulation cannot run at this N)",
        "pair_interactions_per_s": float(n) * n * steps / dt,
        "energy_drift_rel_oracle": drift_oracle, "energy_drift_rel_gpu": drift_gpu,
        "energy_drift_vs_oracle": abs(drift_gpu - drift_oracle), "energy_drift_steps": steps,
        "energy_drift_note": "same fp64 initial conditions on both sides (fp32-representable values), "
                             "(E_k - E_0)/|E_0| after the k steps the oracle sample runs",
        "reference_formulation_torch_cpu": {
            "what": "the reference's formulation (materialised torch broadcasts, simulation.py:74-143) restated in "
                    "oracle/torch_materialised.py; 10 warm-up + 10 timed steps per row (omega_point_test.py:305-319 idiom)",
            "rows": ref_form},
    }


def collective_report(sim, runtime, nb, dist, world, n, pos, vel, mass, mode, dev):
    """What the per-step collective is and costs on THIS node, for every run with a communicator -- and never at the
    price of the bench line: every probe is wrapped, a failing one is reported by name.  Collective (every rank)."""
    import ctypes
    from nbody_cosmological_simulation_amd import _native, checkpoint
    rep = {"force_vector_bytes": n * pos.shape[1] * (8 if mode == nb.PrecisionMode.FLOAT64 else 4)}

    def probe(key, fn):
        try:
            rep[key] = fn()
        except Exception as exc:            # noqa: BLE001 -- the line must be printed whatever a probe does
            rep[key] = None
            rep.setdefault("probe_errors", {})[key] = repr(exc)[:300]

    def comm_info():
        info = (ctypes.c_int32 * 8)()
        _native.check(_native.lib().nb_comm_info(info))
        return {"ranks": info[0], "rank": info[1], "device": info[2], "direct_only": bool(info[3]),
                "rccl_nranks": info[4], "direct_state": {0: "none", 1: "attached", 2: "enabled"}[info[5]],
                "direct_nranks": info[6]}
    probe("communicator", comm_info)                     # rccl_nranks = ncclCommCount() of the communicator in use
    probe("carrier", runtime.allreduce_label)            # which path carries the force vectors of `sim`
    probe("direct_setup", lambda: runtime._p2p_log.get("state"))
    # back-to-back all-reduces of the force vector on zeroed scratch, per carrier (None: carrier not available)
    probe("rccl_us_per_allreduce", lambda: sim.allreduce_time("rccl"))
    probe("direct_us_per_allreduce", lambda: sim.allreduce_time("direct"))

    def identical():
        hashes = [checkpoint.state_hash(sim)]
        if world > 1:
            hashes = [None] * world
            dist.all_gather_object(hashes, checkpoint.state_hash(sim))
        return len(set(hashes)) == 1
    probe("ranks_hold_identical_state", identical)       # the invariant of the replicated integration
    # the two carriers against each other: five steps from the same initial conditions through the direct all-reduce
    # and through RCCL (NB_NO_P2P is read when a simulation is created) must agree to rounding (their summation orders
    # differ) -- a stale or torn read on the direct path would show here
    if rep.get("carrier") and rep["carrier"].startswith("direct") and rep.get("rccl_us_per_allreduce") is not None:
        def five_steps(rccl_only):
            if rccl_only:
                os.environ["NB_NO_P2P"] = "1"
            try:
                s2 = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=mode, G=0.001,
                                         softening=0.1, dt=0.01, device=dev)
            finally:
                os.environ.pop("NB_NO_P2P", None)
            s2.run(5)
            x = s2.positions.double().cpu()
            s2.close()
            return x

        def compare():
            xa, xb = five_steps(False), five_steps(True)
            return float((xa - xb).abs().max() / xb.abs().max())
        probe("direct_vs_rccl_relerr_5_steps", compare)
    return rep


def gpu_rows(nb, galaxy, dev, sizes):
    """The engine at the sizes the CPU rows of cpu_baseline.reference_formulation_torch_cpu are taken at (the reference
    harness's own range, density_limit_test.py:69-203): fp64 and fp32, omega_point_test.py:305-319 idiom (10 warm-up
    steps, perf_counter around >= 10 steps -- 200 here, the steps are microseconds)."""
    rows = []
    for nr in sizes:
        pos, vel, mass = galaxy.create_disk_galaxy(nr, seed=42, device="cpu")
        for mode in ("float64", "float32"):
            sim = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=nb.get_mode_from_string(mode),
                                      G=0.001, softening=0.1, dt=0.01, device=dev)
            sim.run(10)
            t = time.perf_counter()
            while time.perf_counter() - t < 0.05:        # past the clock ramp
                sim.run(50)
                sim.synchronize()
            steps = 200
            t0 = time.perf_counter()
            sim.run(steps)
            sim.synchronize()
            dt = time.perf_counter() - t0
            rows.append({"n": nr, "mode": mode, "ms_per_step": dt / steps * 1e3, "particle_steps_per_s": nr * steps / dt,
                         "pair_interactions_per_s": float(nr) * nr * steps / dt, "kernel": sim.force_kernel_name()})
            sim.close()
    return rows


def mode_rows(nb, pos, vel, mass, dev):
    """BASELINE config 3 (N = 65 536 precision sweep): every precision mode's force launch (HIP events on the dispatch)
    and whole step, against the peak of the type it computes in."""
    rows = []
    n = pos.shape[0]
    steps = 60
    for mode in nb.PrecisionMode:
        # two passes: with the timing events on the force dispatch (they cost a few us per step: the launch can no longer
        # overlap its neighbours) for the launch time, without them for the whole step
        res = {}
        for profile in (True, False):
            sim = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=mode, G=0.001, softening=0.1,
                                      dt=0.01, device=dev, profile=profile)
            tw = time.perf_counter()
            while time.perf_counter() - tw < 0.12:       # past the clock ramp (~40 ms of load, profiles/r01_v8_clock_ramp.txt)
                sim.run(30)
                sim.synchronize()
            sim.kernel_time()
            t0 = time.perf_counter()
            sim.run(steps)
            sim.synchronize()
            res[profile] = (time.perf_counter() - t0, sim.kernel_time(), sim.force_kernel_name())
            sim.close()
        ms, launches = res[True][1]
        peak = FP64_VECTOR_PEAK_TFLOPS if mode == nb.PrecisionMode.FLOAT64 else FP32_VECTOR_PEAK_TFLOPS
        avg = ms / max(launches, 1)
        tf = FLOP_PER_PAIR_2D * float(n) * n / (avg * 1e-3) / 1e12
        rows.append({"mode": mode.value, "ms_per_force_launch": avg, "launches": launches,
                     "ms_per_step": res[False][0] / steps * 1e3, "tflops": tf, "peak": peak, "frac": tf / peak,
                     "kernel": res[True][2]})
    return rows


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` from the COMMITTED rocprofv3 PMC summary (collected in separate
    --pmc passes as the MI355X guide prescribes) with its provenance, or (None, why) when not profiled."""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        summary = json.load(open(path))
    except OSError:
        return None, "no profiles/pmc_latest.json"
    meta = summary.get("_meta", {})
    for name, counters in summary.items():
        if name.startswith(kernel_name) and isinstance(counters, dict) and "FETCH_SIZE" in counters and "WRITE_SIZE" in counters:
            src = {"file": "profiles/pmc_latest.json (committed; NOT measured in this run)", "kernel": name}
            src.update(meta)
            return (2.0 * counters["FETCH_SIZE"]["avg"] + counters["WRITE_SIZE"]["avg"]) * 1024.0, src
    return None, "kernel not in profiles/pmc_latest.json"


def read_outputs(sim):
    """The arrays a caller of the timed path receives after its last step: fp64 state stays fp64, every other dtype
    becomes fp32.  Above DUMP_BYTES in all, the same seeded sample of rows of every array.  Called on every rank."""
    import numpy as np
    import torch
    arrays = {}
    for name in ("positions", "velocities", "accelerations"):
        t = getattr(sim, name).detach().cpu()
        arrays[name] = (t if t.dtype == torch.float64 else t.float()).numpy()
    n = sim.num_stars
    row_bytes = sum(a.nbytes for a in arrays.values()) // max(n, 1)
    keep = DUMP_BYTES // max(row_bytes, 1)
    if n > keep:
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
    return arrays


def write_outputs(arrays, out_dir):
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        return self_launch(args)          # before anything imports torch or touches HIP
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        if "RANK" in os.environ:
            dist.init_process_group(backend="gloo")
            t = torch.ones(1)
            dist.all_reduce(t)
            assert int(t.item()) == world
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "gpus_arg": args.gpus}), flush=True)
        return 0 if args.gpus == world else 1
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    # rehearsal of the multi-rank code path on a ONE-GPU box (tests only): all ranks on device 0, gloo as torch's
    # transport and the engine's direct-only communicator (RCCL / NCCL refuse several ranks per GPU)
    rehearsal = os.environ.get("NB_BENCH_ONE_GPU_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
        os.environ["NB_COMM"] = "direct"
    torch.cuda.set_device(local_rank)
    launched = "RANK" in os.environ          # under torch.distributed.run, also with one rank
    if launched and rehearsal:
        dist.init_process_group(backend="gloo")
    elif launched:
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")

    import nbody_cosmological_simulation_amd as nb
    from nbody_cosmological_simulation_amd import galaxy, runtime
    runtime.init_distributed(device=local_rank)

    n = args.n
    mode = nb.get_mode_from_string(args.mode)
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=42, device="cpu")       # fp32, like main.py:131-133
    dev = torch.device("cuda", local_rank)
    # HIP events on the force kernel's dispatch cost ~4 us per step (the launch can no longer overlap its
    # neighbours): measured at N=1, where the roofline is judged; multi-GPU runs bound the kernel by the step
    profile = os.environ.get("NB_BENCH_NOPROFILE") != "1" and (world == 1 or os.environ.get("NB_BENCH_PROFILE") == "1")
    sim = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=mode,
                              G=0.001, softening=0.1, dt=0.01, device=dev,
                              profile=profile)

    def barrier():
        if launched:
            dist.barrier()
        torch.cuda.synchronize()
        sim.synchronize()

    sim.run(args.warmup)
    # the chip needs ~30 launches (~40 ms) to settle at its sustained clock (profiles/r01_v8_clock_ramp.txt):
    # short warm-ups are topped up with force evaluations that leave the state untouched (untimed)
    spinup = max(0, SPINUP_EVALS - args.warmup) if n >= 16384 else 0
    sim.spin_up(spinup)
    e0 = sim.get_total_energy() if args.full else None
    sim.kernel_time()                 # reset the event accumulators
    barrier()
    t0 = time.perf_counter()
    sim.run(args.steps)               # one native call: K steps on the device
    sim.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearsal else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    kern_ms, launches = sim.kernel_time()
    kernel_name = sim.force_kernel_name()
    outputs = read_outputs(sim) if args.dump_outputs else None
    if outputs is not None and rank == 0:
        write_outputs(outputs, args.dump_outputs)
    e1 = sim.get_total_energy() if args.full else None
    collective = None
    if args.full and (world > 1 or runtime.force_comm()):
        collective = collective_report(sim, runtime, nb, dist, world, n, pos, vel, mass, mode, dev)

    if rank == 0:
        is64 = mode == nb.PrecisionMode.FLOAT64
        peak = FP64_VECTOR_PEAK_TFLOPS if is64 else FP32_VECTOR_PEAK_TFLOPS
        pairs_per_launch = float(n) * n / world                 # this rank's source block
        avg_ms = kern_ms / max(launches, 1)
        timing = "hip events on the kernel's dispatch (hipExtLaunchKernelGGL), on the engine's own stream"
        if launches == 0:                 # no events (multi-GPU / NB_BENCH_NOPROFILE=1): bound the kernel by the step
            avg_ms = elapsed / args.steps * 1e3
            timing = "events off: kernel time bounded above by the whole step (includes O(N) kernels and the all-reduce)"
        achieved = FLOP_PER_PAIR_2D * pairs_per_launch / (avg_ms * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic(kernel_name)
        traffic_valid = isinstance(traffic_src, dict) and traffic_src.get("n", n) == n and \
            traffic_src.get("mode", mode.value) == mode.value and traffic_src.get("n_gpus", 1) == world
        out = {
            "metric": f"particle-steps/sec (N={n} {'fp64' if is64 else args.mode} direct-sum leapfrog)",
            "value": n * args.steps / elapsed,
            "unit": "particle-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "spinup_force_evals": spinup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64" if is64 else "f32",
            "data": "synthetic",
            "config": {"workload": f"N={n} exponential-disk galaxy (seed 42), fp32 ICs, {mode.value} mode, "
                                   f"G=1e-3 eps=0.1 dt=0.01, KDK leapfrog, all-pairs direct sum",
                       "parallelism": runtime.partition_label(world)},
            "collective": collective,
            "pair_interactions_per_s": float(n) * n * args.steps / elapsed,
            "roofline": {
                "bound": "mfma",
                "bound_note": "compute-bound: priced against the dense fp64 (fp32 modes: fp32) MFMA peak, which on MI355X "
                              "equals the vector-ALU peak the kernel actually issues on (the pair loop is VALU code: "
                              "contraction dimension D = 2, DESIGN.md section 3); HBM traffic is O(N) per step",
                "kernel": kernel_name,
                "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "avg_launch_ms": avg_ms, "launches": launches, "timing": timing,
                "flop_per_launch": FLOP_PER_PAIR_2D * pairs_per_launch,
                "traffic": traffic if traffic_valid else None,
                "traffic_source": traffic_src,
                "traffic_note": "HBM bytes per launch from rocprofv3 PMC passes committed under profiles/ "
                                "(2*FETCH_SIZE + WRITE_SIZE, gfx950 correction), reported only when that profile's "
                                "N / mode / GPU count match this run; dominated by the slab writes that make the "
                                "sums order-deterministic, DESIGN.md section 2",
            },
        }
        if args.full:
            out["energy_drift_rel_timed_region"] = (e1 - e0) / abs(e0)
            out["energy_drift_note"] = ("raw drift over the timed steps (after warm-up), for the record only; the metric's "
                                        "rel-err against the oracle is cpu_baseline.energy_drift_vs_oracle")
        if args.full and world == 1 and not args.no_cpu_baseline and is64:
            def gpu_drift(k):
                s2 = nb.GalaxySimulation(pos.double().to(dev), vel.double().to(dev), mass.double().to(dev),
                                         precision_mode=mode, G=0.001, softening=0.1, dt=0.01, device=dev)
                ea = s2.get_total_energy()
                s2.run(k)
                eb = s2.get_total_energy()
                s2.close()
                return (eb - ea) / abs(ea)
            sizes = [int(v) for v in args.ref_sizes.split(",") if v.strip()]
            out["cpu_baseline"] = cpu_baseline(pos, vel, mass, args.cpu_seconds, sizes, gpu_drift)
            # the same sizes on the GPU, beside the CPU rows, and config 3's per-mode numbers
            try:
                out["gpu_rows"] = {"what": "this engine at the sizes of cpu_baseline.reference_formulation_torch_cpu.rows: "
                                           "10 warm-up + 200 timed steps per row, state resident in HBM",
                                   "rows": gpu_rows(nb, galaxy, dev, sizes)}
                if n == 65536:
                    out["modes"] = {"what": "BASELINE config 3: every precision mode at N = 65536 (0.12 s of warm-up steps + 60 timed steps; "
                                            "force launch by HIP events on the dispatch, whole step from a second pass "
                                            "without them; frac = 14 N^2 flop / launch / peak of the compute type)",
                                    "rows": mode_rows(nb, pos, vel, mass, dev)}
            except Exception as exc:            # noqa: BLE001 -- context rows never break the bench line
                out["gpu_rows_error"] = repr(exc)[:300]
        print(json.dumps(out), flush=True)
    sim.close()
    runtime.shutdown()                # the process communicator: collective, every rank, before the process group goes
    if launched:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
