#!/usr/bin/env python3
"""Benchmark: reference-equivalent env-steps/s of the fused HIP step.

One "step" = one SpatialKuramoto.step() (environment/env.py:415-454) for every
env of the batch: stim-ON + stim-OFF adaptive Dopri5 solves (~32 RHS sweeps
of the N x N coupling), 17-19 LFP samples, the 2340-sample window update and
the beta-band reward.  Workload: BASELINE.json configs[1] -- env0, N=1024
oscillators x 4096 envs per GPU, synthetic (random-seeded natural
frequencies / initial phases, reference grid coupling), actions U(-1, 1).

Multi-GPU: one process per GPU, each owning its own shard of 4096 envs
(global env id = rank*B + b seeds the env), no data-path collective; the only
collectives are the barrier and the max-over-ranks of the timed region (weak
scaling).  Either torchrun starts the ranks (WORLD_SIZE set; it must equal
--gpus), or `python bench.py --gpus N` does: the parent process never touches
the GPU, spawns N rank processes with RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* set (127.0.0.1), relays rank 0's JSON line and exits non-zero if any
rank fails.  The line reports the world size the process group saw and every
rank's own rate.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) sets up, warms up,
times the N steps and prints the line.  `--full` adds the bounded CPU
baselines (`cpu_baseline`, --cpu-seconds; ~40 s of host time) to the line.
`--dump-outputs DIR` writes what the last timed step() returned (obs, reward,
done) as DIR/<name>.npy: the same arguments give the same inputs and, the step
being deterministic, the same arrays.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3   # MI355X dense FP32 (vector == matrix), MI355X_MICROARCH.md
PEAK_BF16_TFLOPS = 2516.6  # MI355X dense BF16 MFMA (1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz; "~2.5 PF dense")
PEAK_HBM_GBS = 8000.0
# KURA_COUPLING_BF16X3 executes six bf16 products per fp32 product of the coupling
# (x1a1, x1a2, x2a1, x1a3, x2a2, x3a1; kura.h)
BF16X3_PRODUCTS = 6


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="env0", choices=["env0", "env1", "env2"])
    ap.add_argument("--osc", type=int, default=1024)
    ap.add_argument("--envs", type=int, default=4096, help="envs per GPU (weak scaling)")
    ap.add_argument("--global-envs", type=int, default=0,
                    help="total envs over all ranks (strong scaling: each rank owns global/world of them)")
    ap.add_argument("--part-osc", type=int, default=-1,
                    help="N > 1024: oscillators per workgroup of a split env group (256/512/1024; -1 = auto: "
                         "the largest that gives every CU a workgroup)")
    ap.add_argument("--episode", action="store_true",
                    help="also run one whole episode through KuraVectorEnv (autoreset included) -> extra.episode")
    ap.add_argument("--episode-steps", type=int, default=0, help="episode length for --episode (0 = the config's)")
    ap.add_argument("--episode-metrics", action="store_true",
                    help="--episode with episode_metrics=True (beta power + envelope of every finished episode)")
    ap.add_argument("--reward", default="bbpow_action")
    ap.add_argument("--coupling", default="auto", choices=["auto", "f32", "bf16x3"],
                    help="coupling arithmetic (kura.h KURA_COUPLING_*; auto = bf16x3 at every N)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the CPU baselines (--cpu-seconds)")
    ap.add_argument("--cpu-seconds", type=float, default=24.0,
                    help="--full: bounded CPU-baseline budget in seconds (0 = skip), split over its legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step() returned as DIR/<name>.npy (float32 / float64; "
                         "rank r > 0 writes <name>.rank<r>.npy)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reset-reps", type=int, default=1,
                    help="time this many resets of the same state (extra.reset_ms_warm: the fastest after the first)")
    ap.add_argument("--random-k", action="store_true", help="per-env K ~ U(0.3, 0.8) (north_star 'random K')")
    # rehearsal of the N>1 path on a one-GPU box: every rank on cuda:0, gloo for the
    # barrier / max-over-ranks (RCCL cannot put two ranks on one device)
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--share-device", action="store_true", help="every rank uses cuda:0 (rehearsal only)")
    ap.add_argument("--launcher-selftest", action="store_true",
                    help="(CPU test of the --gpus N launcher) ranks only join the process group and report")
    ap.add_argument("--rank-timeout", type=float, default=1800.0,
                    help="launcher: seconds before the spawned ranks are killed")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


DUMP_MAX_BYTES = 64 << 20   # --dump-outputs: upper bound of one rank's files together


def dump_outputs(path, outputs, rank=0, seed=0):
    """Write {name: array} (one leading env axis each) as path/<name>.npy:
    floats keep their width, everything else becomes float32 (exact for the
    0/1 done flags).  A set above DUMP_MAX_BYTES is cut to the same seeded,
    sorted sample of envs in every array, stored as env_index.npy."""
    os.makedirs(path, exist_ok=True)
    arrs = {k: np.ascontiguousarray(v, dtype=v.dtype if v.dtype in (np.float32, np.float64) else np.float32)
            for k, v in outputs.items()}
    B = next(iter(arrs.values())).shape[0]
    per_env = sum(a.nbytes for a in arrs.values()) / B + 4   # + its env_index entry
    keep = int((DUMP_MAX_BYTES - 256 * (len(arrs) + 1)) // per_env)   # 256 B cover each file's .npy header
    if keep < B:
        idx = np.sort(np.random.default_rng(seed).choice(B, size=max(keep, 1), replace=False))
        arrs = {k: np.ascontiguousarray(a[idx]) for k, a in arrs.items()}
        arrs["env_index"] = idx.astype(np.float32)
    sfx = f".rank{rank}" if rank else ""
    for k, a in arrs.items():
        np.save(os.path.join(path, f"{k}{sfx}.npy"), a)


def build_shard(args, rank):
    kura = importlib.import_module("dbs-gym_amd")
    sim_mod = importlib.import_module("dbs-gym_amd.sim")
    base = kura.synthetic_params(args.config, args.osc) if args.osc != 512 else kura.reference_params(args.config)
    B = args.envs
    plist = []
    for b in range(B):
        gid = rank * B + b
        p = dict(base)
        p["rand_seed"] = args.seed + gid
        if args.random_k:
            p["K"] = float(np.random.default_rng(args.seed * 7919 + gid).uniform(0.3, 0.8))
        plist.append(p)
    plist = kura.fill_driver_arrays_batch(plist, [10_000_000 + args.seed + rank * B + b for b in range(B)])
    hosts, shared = kura.build_batch(plist)
    omega, g_stim, g_rec, theta0 = kura.reset_arrays(hosts)
    cfg = sim_mod.make_config(base, B, reward_func=args.reward,
                              part_osc=(sim_mod.auto_part_osc(args.osc, B) if getattr(args, "part_osc", -1) < 0
                                        else args.part_osc), coupling=getattr(args, "coupling", "auto"))
    bins = kura.spectral.beta_bins(cfg.window, base["verbose_dt"])
    ctab, stab = kura.spectral.twiddles(cfg.window, bins)
    return cfg, shared["alpha"].astype(np.float32), omega, g_stim, g_rec, theta0, ctab, stab, shared["gain"]


def _time_oracle(args, cfg, alpha, omega, g_stim, g_rec, theta0, ctab, stab, gain, nb, seconds):
    """Steps/s of the oracle stepping nb envs (one env per OpenMP thread) for ~seconds after reset."""
    from oracle import kura_oracle as ko
    import copy
    c = copy.copy(cfg)
    c.n_envs = nb
    o = ko.Oracle(c, alpha)
    o.set_env_params(omega[:nb], g_stim[:nb], g_rec[:nb])
    o.set_gain(gain[:nb])
    o.set_spectral(ctab, stab)
    o.reset(theta0[:nb])
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    k = 0
    while True:
        o.step(rng.uniform(-1, 1, (nb, c.n_elec)).astype(np.float32))
        k += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            break
    o.close()
    return nb * k / el, k, el


def _host_cores():
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    return int(os.environ.get("OMP_NUM_THREADS", ncores))


def cpu_oracle_c(args, cfg, alpha, omega, g_stim, g_rec, theta0, ctab, stab, gain, seconds):
    """The bit-exact C oracle (factorised RHS, the HIP path's twin) on this
    host's cores: all cores (one env per OpenMP thread) and one core."""
    nthreads = _host_cores()
    nb = max(1, min(nthreads, cfg.n_envs))
    arrs = (args, cfg, alpha, omega, g_stim, g_rec, theta0, ctab, stab, gain)
    v, k, el = _time_oracle(*arrs, nb, seconds)
    v1, k1, el1 = _time_oracle(*arrs, 1, max(1.0, seconds / 3))
    return {"value": v, "cores": nthreads, "single_core_value": v1,
            "sample": f"oracle/kura_oracle.c, {args.config} N={cfg.n_osc}, {nb} envs x {k} steps ({el:.1f} s, OpenMP "
                      f"{nthreads} threads) and 1 env x {k1} steps ({el1:.1f} s)"}


_REF_ENV = None


def _ref_child(seconds):
    """(forked worker) steps/s of the reference-op-sequence env prepared by the parent."""
    from oracle.ref_numpy import time_steps
    v, k, el = time_steps(_REF_ENV, seconds, np.random.default_rng(os.getpid()))
    return v, k


def _ref_env(args, n_osc):
    """env 0 of the bench's workload at n_osc oscillators as an oracle/ref_numpy.RefOpEnv, started from the
    state reset() leaves (the transient is run by the C oracle: ~460 direct-sin RHS at N=1024 would take
    ~5 s per process)."""
    from oracle import kura_oracle as ko
    from oracle.ref_numpy import RefOpEnv
    import copy
    a = copy.copy(args)
    a.osc, a.envs, a.random_k = n_osc, 1, False
    a.coupling = "f32"   # only the starting state: the reference op sequence runs its own (direct-sin) arithmetic
    cfg, alpha, omega, gs, gr, th0, ct, st, gain = build_shard(a, 0)
    o = ko.Oracle(cfg, alpha)
    o.set_env_params(omega, gs, gr)
    o.set_spectral(ct, st)
    o.reset(th0)
    state = o.state()
    o.close()
    env = RefOpEnv(alpha, omega[0], gs[0], K=float(gain[0]) * n_osc if gain is not None else 0.52,
                   W=cfg.window, dbs_bounds=(cfg.dbs_lo, cfg.dbs_hi))
    env.sol = state["y"][0][None, :].astype(np.float32)
    env.t = float(state["t"][0])
    wp = int(state["wpos"][0])
    env.window = np.roll(state["ring"][0], -wp)
    return env


def cpu_baseline(args):
    """the reference's step() op sequence (direct N^2
    sin coupling, oracle/ref_numpy.py) on this host's cores, bounded samples,
    measured before this process touches the GPU (the all-cores leg forks):
      value        all cores, one env per process, N = the bench's N (1024);
      single_core  one core, same N;
      n512         one core at the reference configs' N=512 (the published
                   JAX-CPU notebook rate is 16.96-19.77 steps/s);
      oracle_c     the bit-exact C oracle (factorised RHS), all cores / one core."""
    import multiprocessing as mp
    global _REF_ENV
    sec = args.cpu_seconds
    nproc = _host_cores()
    out = {"unit": "env-steps/s", "kind": "port"}
    _REF_ENV = _ref_env(args, args.osc)
    from oracle.ref_numpy import time_steps
    v1, k1, el1 = time_steps(_REF_ENV, sec / 3)
    ctx = mp.get_context("fork")
    t0 = time.perf_counter()
    with ctx.Pool(nproc) as pool:
        res = pool.map(_ref_child, [sec / 3] * nproc)
    el = time.perf_counter() - t0
    out["value"] = float(sum(v for v, _ in res))
    out["cores"] = nproc
    out["sample"] = (f"oracle/ref_numpy.py (reference op sequence: fmod + direct N^2 sin coupling, env.py:252-256; "
                     f"Dopri5/PID/dense output; R1), {args.config} N={args.osc}: {nproc} processes x 1 env, "
                     f"{sum(k for _, k in res)} steps in {el:.1f} s wall, started from the reset() state")
    out["single_core_value"] = v1
    out["single_core_sample"] = f"1 env x {k1} steps, {el1:.1f} s, one core"
    if args.osc != 512:
        _REF_ENV = _ref_env(args, 512)
        v5, k5, el5 = time_steps(_REF_ENV, sec / 4)
        out["n512_single_core_value"] = v5
        out["n512_sample"] = f"N=512 reference env0 config, 1 env x {k5} steps, {el5:.1f} s, one core"
    _REF_ENV = None
    return out


def kernel_name(N, part=0, coupling="f32"):
    """The step kernel instantiation libkura launches for N oscillators (split
    groups of `part` oscillators per workgroup when N > 1024) in the given
    coupling arithmetic."""
    sp = "true" if coupling == "bf16x3" else "false"
    if N > 1024:
        return f"kura_step_kernel<{(part or 1024) // 256}, true, {sp}>"
    return f"kura_step_kernel<{N // 256}, false, {sp}>"


def pmc_traffic(workload, kernel):
    """Bytes per launch of the step kernel from the committed rocprofv3 PMC
    passes (tools/rocprof_run.sh + tools/summarize_rocprof.py: FETCH_SIZE x2 +
    WRITE_SIZE, the same bench command).  PMC counters cannot be read from
    inside this process, so the committed summary of this exact workload is
    quoted, with the effective clock of its GRBM_GUI_ACTIVE pass: one
    profiles/latest_rocprof*.json per workload (the headline in
    latest_rocprof.json, the N=8192 forms beside it), matched on the bench
    line's config.workload string and the kernel name; None when none
    matches."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "latest_rocprof*.json"))):
        try:
            with open(path) as f:
                d = json.load(f)
            if d["bench_under_trace"]["config"]["workload"] != workload:
                continue
            k = d["kernels"][kernel]
            return (k["traffic_bytes_per_dispatch"],
                    f"profiles/{os.path.basename(path)} ({d['source']}): FETCH_SIZE*2 + WRITE_SIZE",
                    k.get("effective_clock_ghz"))
        except (OSError, KeyError, ValueError):
            continue
    return None, None, None


def episode_bench(args, rank, world, local_rank):
    """One whole episode of B envs through the drop-in KuraVectorEnv: every
    step() of the episode plus the autoreset at its end (host reset draws,
    parameter upload, masked reset kernel; with --episode-metrics the
    per-episode beta power and envelope statistics).  Returns the
    episode-inclusive rate beside the breakdown of the episode boundary."""
    import torch
    import torch.distributed as dist
    kura = importlib.import_module("dbs-gym_amd")
    vec = importlib.import_module("dbs-gym_amd.vec_env")
    base = kura.synthetic_params(args.config, args.osc) if args.osc != 512 else kura.reference_params(args.config)
    if args.episode_steps:
        base["total_episode_len"] = args.episode_steps * (base["electrode_width"] + base["electrode_pause"])
    B = args.envs
    plist = []
    for b in range(B):
        gid = rank * B + b
        p = dict(base)
        p["rand_seed"] = args.seed + gid
        if args.random_k:
            p["K"] = float(np.random.default_rng(args.seed * 7919 + gid).uniform(0.3, 0.8))
        plist.append(p)
    t0 = time.perf_counter()
    env = vec.KuraVectorEnv(plist, device=local_rank, reward_func=args.reward, w0_seed=10_000_000 + args.seed + rank * B,
                            episode_metrics=args.episode_metrics, profile=True, coupling=args.coupling)
    setup_s = time.perf_counter() - t0
    dev = env.device
    env.reset()
    L = int(env.episode_steps)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed + 7 * rank + 1)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for k in range(L):
        env.step(torch.rand((B, 1), generator=gen, device=dev) * 2 - 1)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    bt = env.boundary_times[-1] if env.boundary_times else {}
    env.close()
    return {"workload": f"one episode of {L} steps x {B} envs per GPU through KuraVectorEnv, autoreset of every env "
                        f"at its end{' with episode metrics (bbpow + envelope)' if args.episode_metrics else ''}",
            "episode_steps": L, "value": world * B * L / el, "unit": "env-steps/s", "episode_s": el,
            "boundary": bt, "boundary_frac": (sum(v for k, v in bt.items() if k.endswith("_s")) / el) if bt else None,
            "setup_s": setup_s}


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args, argv) -> int:
    """`bench.py --gpus N` without torchrun: start N rank processes of this
    script (RANK = LOCAL_RANK = r, WORLD_SIZE = N, MASTER_ADDR 127.0.0.1 and a
    free port), relay rank 0's JSON line, return the first failing rank's exit
    status (killing the other ranks) or 0.  This process never initialises the
    GPU: it only counts devices (torch.cuda.device_count() does not initialise
    HIP on this image) and execs nothing."""
    import subprocess
    n = args.gpus
    if not args.launcher_selftest:
        import torch
        ndev = torch.cuda.device_count()
        need = 1 if args.share_device else n
        if ndev < need:
            print(f"[bench] --gpus {n} needs {need} visible GPU(s), {ndev} visible", file=sys.stderr)
            return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno()))
    deadline = time.time() + args.rank_timeout
    rc = 0
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        late = time.time() > deadline
        if bad or late:
            rc = 124 if not bad else (bad[0][1] if bad[0][1] > 0 else 128 - bad[0][1])
            print(f"[bench] {'rank %d exited with %s' % bad[0] if bad else 'rank timeout'}; stopping the other ranks",
                  file=sys.stderr)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        if all(c == 0 for c in codes):
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
    out = procs[0].stdout.read().decode()
    procs[0].stdout.close()
    if out:
        sys.stdout.write(out)
        sys.stdout.flush()
    return rc


def launcher_selftest(world, rank, local_rank):
    """--launcher-selftest: the rank joins the (gloo) process group and rank 0
    reports who joined -- the CPU test of the launcher (no GPU)."""
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
    if os.environ.get("KURA_BENCH_FAIL_RANK") == str(rank):   # test hook: a failing rank
        sys.exit(3)
    me = {"rank": rank, "local_rank": local_rank, "pid": os.getpid()}
    ranks = [None] * world
    if world > 1:
        dist.all_gather_object(ranks, me)
    else:
        ranks = [me]
    if rank == 0:
        print(json.dumps({"launcher_selftest": True, "n_gpus": world,
                          "dist_world_size": dist.get_world_size() if world > 1 else 1, "ranks": ranks}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def _exit_diagnostics():
    """KURA_EXIT_MAPS=<path>: make an exit-time fault attributable (VERDICT r05
    next #1).  A Python atexit hook copies /proc/self/maps to <path> -- it runs
    in Py_Finalize, before exit() runs the C atexit handlers and library
    destructors, so every library still mapped then is listed with its load
    base -- and faulthandler prints the Python stack of a fatal signal."""
    path = os.environ.get("KURA_EXIT_MAPS")
    if not path:
        return
    import atexit
    import faulthandler
    faulthandler.enable()

    def dump():
        with open("/proc/self/maps") as f, open(path, "w") as g:
            g.write(f.read())
    atexit.register(dump)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse(argv)
    _exit_diagnostics()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch(args, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.share_device else int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a different GPU count",
              file=sys.stderr)
        sys.exit(2)
    if args.launcher_selftest:
        launcher_selftest(world, rank, local_rank)
        return
    import torch
    import torch.distributed as dist
    if not args.share_device and local_rank >= torch.cuda.device_count():
        print(f"[bench] LOCAL_RANK={local_rank} but {torch.cuda.device_count()} visible GPU(s)", file=sys.stderr)
        sys.exit(2)
    # CPU baseline (--full) first: the reference-op leg forks worker processes,
    # which must happen before this process initialises the GPU
    cpu = cpu_baseline(args) if (args.full and world == 1 and args.cpu_seconds > 0) else None
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    if args.global_envs:
        if args.global_envs % world:
            raise SystemExit(f"--global-envs {args.global_envs} is not a multiple of WORLD_SIZE={world}")
        args.envs = args.global_envs // world
    sim_mod = importlib.import_module("dbs-gym_amd.sim")
    t_setup = time.perf_counter()
    cfg, alpha, omega, g_stim, g_rec, theta0, ctab, stab, gain = build_shard(args, rank)
    sim = sim_mod.KuraSim(cfg, local_rank)
    sim.set_coupling(alpha)
    sim.set_env_gain(gain)
    sim.set_env_params(omega, g_stim, g_rec)
    sim.set_spectral(ctab, stab)
    t_setup = time.perf_counter() - t_setup
    B, N = cfg.n_envs, cfg.n_osc
    coupling = sim_mod.abi.coupling_of(cfg)   # the arithmetic the handle runs

    th = torch.from_numpy(theta0).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.reset(th)
    torch.cuda.synchronize()
    t_reset = time.perf_counter() - t0
    reset_stats = sim.stats()
    t_reset_warm = []
    for _ in range(args.reset_reps - 1):
        t0 = time.perf_counter()
        sim.reset(th)
        torch.cuda.synchronize()
        t_reset_warm.append(time.perf_counter() - t0)

    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed + rank)
    acts = [torch.rand((B, cfg.n_elec), generator=gen, device=dev) * 2 - 1
            for _ in range(args.warmup + args.steps)]
    for k in range(args.warmup):
        sim.step(acts[k])
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    st0 = sim.stats()  # cumulative counters [5..7] bracket the timed launches (read outside the region)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        ev[k][0].record(stream)
        ret = sim.step(acts[args.warmup + k])
        ev[k][1].record(stream)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {k: v.cpu().numpy() for k, v in zip(("obs", "reward", "done"), ret)},
                     rank, args.seed)
    kern_ms = [a.elapsed_time(b) for a, b in ev]
    st1 = sim.stats()
    steps_attempted = int(st1[5] - st0[5]) // args.steps   # per launch, averaged over the timed launches
    rejected = int(st1[7] - st0[7])
    wg_sweeps = (st1[6] - st0[6]) / args.steps
    # useful RHS sweeps per launch: 2 initial sweeps per env (ON and OFF solve) + 6 per attempted Dopri step;
    # the kernel also sweeps finished envs of a workgroup in lockstep (16 env slots per workgroup sweep)
    useful_rhs = 2 * B + 6 * steps_attempted
    lockstep_eff = useful_rhs / (16.0 * wg_sweeps) if wg_sweeps else None
    el_max = elapsed
    el_ranks = [elapsed]
    dist_world = 1
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el_max = float(t.item())
        el_ranks = [None] * world
        dist.all_gather_object(el_ranks, elapsed)
        dist_world = dist.get_world_size()

    if rank == 0:
        value = world * B * args.steps / el_max
        avg_kernel_s = float(np.mean(kern_ms)) / 1e3
        flop_per_launch = useful_rhs * 4.0 * N * N   # 2 length-N dot products per oscillator per sweep
        achieved_tf = flop_per_launch / avg_kernel_s / 1e12   # fp32-equivalent (algorithmic) TFLOP/s
        # the roofline of the arithmetic the kernel executes: F32 products on the FP32 MFMA, or six bf16
        # products per fp32 product on the BF16 MFMA (KURA_COUPLING_BF16X3, fp32 accumulation)
        sp = coupling == "bf16x3"
        exec_flop = flop_per_launch * (BF16X3_PRODUCTS if sp else 1)
        exec_tf = exec_flop / avg_kernel_s / 1e12
        peak_tf = PEAK_BF16_TFLOPS if sp else PEAK_FP32_TFLOPS
        # algorithmic HBM bytes per launch: per env theta r/w, omega, g_stim/g_rec (f64),
        # window r/w (f64 ring + f32 obs), outputs; alpha once per launch
        bytes_env = 8 * N + 4 * N + 8 * cfg.n_elec * N + 8 * max(cfg.n_rec, 0) * N + (8 + 8 + 4) * cfg.window + 64
        bytes_launch = B * bytes_env + 4 * N * N
        workload = (f"{args.config} reference step(), N={N} oscillators x {B} envs per GPU, "
                    f"adaptive Dopri5 rtol=atol=1e-5, W={cfg.window}, reward={args.reward}"
                    + (", per-env K~U(0.3,0.8)" if args.random_k else ", K=0.52") + f", coupling={coupling}")
        traffic, traffic_src, clock_ghz = pmc_traffic(workload, kernel_name(N, cfg.part_osc, coupling))
        out = {
            "metric": (f"env steps/sec (whole node), N={N} osc x {world * B} envs over {world} GPUs" if args.global_envs
                       else f"env steps/sec (whole node), N={N} osc x {B} envs per GPU"),
            "value": value,
            "unit": "env-steps/s",
            "n_gpus": world,
            "dist_world_size": dist_world,
            "per_rank_value": [B * args.steps / e for e in el_ranks],
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": el_max / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong" if args.global_envs else "weak",
            "vs_baseline": None,
            "dtype": "f32 (bf16x3-split products, f32 accumulate)" if sp else "f32",
            "data": "synthetic (seeded reference-sampler natural frequencies, N(pi,0.6) phases, U(-1,1) actions)",
            "config": {"workload": workload,
                       "global_envs": world * B, "parallelism": f"env-shard x{world} (no collectives)"}
                      | ({"part_osc": cfg.part_osc or 1024} if N > 1024 else {}),
            "roofline": {"bound": "mfma_bf16" if sp else "mfma", "achieved": exec_tf, "peak": peak_tf,
                         "unit": "TFLOP/s", "frac": exec_tf / peak_tf, "traffic": traffic,
                         "traffic_source": traffic_src,
                         "kernel": kernel_name(N, cfg.part_osc, coupling), "avg_kernel_ms": avg_kernel_s * 1e3,
                         "flop_per_launch": exec_flop,
                         "flop_basis": (f"executed bf16 MFMA FLOP: {BF16X3_PRODUCTS} products x 4N^2 per useful RHS sweep"
                                        if sp else "4N^2 fp32 MFMA FLOP per useful RHS sweep"),
                         "useful_rhs_per_launch": useful_rhs,
                         "hbm_alg_bytes_per_launch": bytes_launch,
                         "hbm_alg_gbs": bytes_launch / avg_kernel_s / 1e9},
            "extra": {"coupling": coupling,
                      "fp32_equivalent_tflops": achieved_tf,
                      "fp32_equivalent_frac_of_fp32_peak": achieved_tf / PEAK_FP32_TFLOPS,
                      "rhs_sweeps_per_env_step": useful_rhs / B, "dopri_steps_attempted": steps_attempted,
                      "rejected": rejected, "lockstep_efficiency": lockstep_eff,
                      "executed_frac": ((16.0 * wg_sweeps * 4.0 * N * N * (BF16X3_PRODUCTS if sp else 1))
                                        / avg_kernel_s / 1e12) / peak_tf,
                      "phase_sweeps_per_s": world * useful_rhs / avg_kernel_s,
                      # the chip holds its clock below 2.4 GHz under this kernel (DVFS): effective clock from the
                      # committed GRBM_GUI_ACTIVE pass (tools/rocprof_run.sh) and the FP32 MFMA peak at that clock
                      "effective_clock_ghz": clock_ghz,
                      "frac_of_peak_at_effective_clock": (exec_tf / (peak_tf * clock_ghz / 2.4)
                                                          if clock_ghz else None),
                      "reset_ms": t_reset * 1e3,
                      "reset_ms_warm": min(t_reset_warm) * 1e3 if t_reset_warm else None, "reset_rhs_max": int(reset_stats[0]),
                      **({"xl_launch": "plain" if os.environ.get("KURA_XL_LAUNCH") == "plain" else "cooperative"}
                         if N > 1024 else {}),
                      "host_setup_s": t_setup},
        }
    if args.episode:
        sim.close()
        sim = None
        ep = episode_bench(args, rank, world, local_rank)
        if rank == 0:
            ep["steady_state_value"] = out["value"]
            ep["episode_vs_steady"] = ep["value"] / out["value"]
            out["extra"]["episode"] = ep
    if rank == 0:
        if cpu is not None:
            cpu["oracle_c"] = cpu_oracle_c(args, cfg, alpha, omega, g_stim, g_rec, theta0, ctab, stab, gain,
                                           max(2.0, args.cpu_seconds / 2))
        out["cpu_baseline"] = cpu
        print(json.dumps(out), flush=True)
    if sim is not None:
        sim.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
