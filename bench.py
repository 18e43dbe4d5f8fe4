"""bench.py -- env-steps/s of the native batched step on the BASELINE.json workload.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--workload humanoid|humanoid32k|ant|mesh|cartpole] [--dump-outputs DIR]

One process per GPU.  The driver launches N > 1 with torch.distributed.run; `python bench.py --gpus N` run directly spawns
that launch itself (as a child process, BEFORE this process touches the GPU) and relays rank 0's line.  Independent
environments are sharded across ranks with no data-path collective (weak scaling: B environments PER GPU).

A "step" is one `d = mujoco_torch.step(mx, d)` -- the reference's own signature (forward.py:463), fresh output storage every
call -- over the whole resident batch; state is carried across steps; inputs follow the reference's bench recipe
(benchmarks/_helpers.py:25-42: make_data state, qvel = 0.01 * RandomState(42).randn(B, nv), ctrl = 0).  `value` is that
loop; `out_buffers` reports the `step(..., out=)` ping-pong extension beside it.  Rank 0 prints ONE JSON line.

Before the W warm-up steps the step loop runs 100 untimed steps on a SCRATCH copy of the inputs (clocks, allocator pools, plan caches);
the warm-up and the timed steps then start from the original state.  Early steps of the trajectory are the expensive ones (all contacts
active, longer line searches): --steps 20 --warmup 5 reads ~18.3 M env-steps/s where the default 200 / 20 reads ~19 M.

`--dump-outputs DIR` (e.g. bench_outputs/, git-ignored) writes the Data the last timed step returned, one .npy per non-empty array,
after the timed region: the inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
DUMP_CAP_BYTES = 64 * 10**6  # --dump-outputs: all files together, .npy headers included
DUMP_SAMPLE_SEED = 0         # which environments a capped dump keeps


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0, help="environments per GPU (default: the workload's)")
    ap.add_argument("--workload", default="humanoid", choices=["humanoid", "humanoid32k", "ant", "mesh", "cartpole"])
    ap.add_argument("--dtype", default="", choices=["", "f32", "f64"], help="override the workload's dtype (experiments: e.g. the float64 twin of config 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-config4", action="store_true", help="N > 1 humanoid runs also time BASELINE config 4 (32768 envs/GPU); skip it")
    ap.add_argument("--no-other-workloads", action="store_true", help="the default humanoid run also times BASELINE configs 3 (ant) and 5 (mesh scene); skip them")
    ap.add_argument("--no-long-run", action="store_true", help="skip the 1000-step run of the headline workload reported beside `value`")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write every non-empty array of the Data the last timed step returned as DIR/<leaf>.npy (float32 / float64; rank 0's environments, "
                         f"a seeded sample of them when all would exceed {DUMP_CAP_BYTES // 10**6} MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start `torch.distributed.run` as a CHILD (this process has made no HIP call
    and makes none), one rank per GPU, and relay rank 0's JSON line and the exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    if lines:
        print(lines[-1])
    else:
        sys.stdout.write(r.stdout)
    sys.exit(r.returncode if r.returncode else (0 if lines else 1))


ARGS = parse_args() if __name__ == "__main__" else None
if ARGS is not None and ARGS.gpus > 1 and "WORLD_SIZE" not in os.environ:
    spawn_ranks(ARGS)  # never returns

for p in (os.path.join(ROOT, "mujoco-torch_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import mujoco_torch_amd as mt  # noqa: E402
from mujoco_torch_amd import native  # noqa: E402

WORKLOADS = {
    # BASELINE.json configs[1]: humanoid.xml, batch 4096, Euler + CG, float64 (XML iterations=1, ls_iterations=4)
    "humanoid": dict(xml="humanoid", overrides={"solver": 1}, dtype=torch.float64, batch=4096,
                     name="humanoid.xml batch=4096/GPU Euler+CG float64 (iterations=1, ls_iterations=4)"),
    # configs[3]: the same model at 262144 = 8 x 32768 environments
    "humanoid32k": dict(xml="humanoid", overrides={"solver": 1}, dtype=torch.float64, batch=32768,
                        name="humanoid.xml batch=32768/GPU Euler+CG float64 (iterations=1, ls_iterations=4; config 4 = 8 x 32768)"),
    # configs[2]: ant.xml, RK4 + Newton, elliptic, float32
    "ant": dict(xml="ant", overrides={"integrator": 1, "solver": 2, "cone": 1}, dtype=torch.float32, batch=16384,
                name="ant.xml batch=16384/GPU RK4+Newton elliptic float32"),
    # configs[4]: plane + free box + free dodecahedron mesh, condim 6, Newton, float32
    "mesh": dict(xml="mesh_contact", overrides={}, dtype=torch.float32, batch=8192,
                 name="mesh_contact.xml (plane + box + dodecahedron mesh, condim 6) batch=8192/GPU Euler+Newton float32"),
    "cartpole": dict(xml="cartpole", overrides={}, dtype=torch.float64, batch=4096, name="cartpole.xml Euler float64"),
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
# SURVEY.md section 8(d), "ALGORITHMIC bytes per env-step" as printed there (consumed + produced Data leaves; the survey's probe counts qpos under
# kinematics AND _advance and leaves sensordata out, so its figures sit 56 - 224 B off the leaf arithmetic of algorithmic_bytes_per_env_step below,
# which the line carries beside them).  `roofline.achieved` / `frac` are computed from THESE so that they can be reproduced from the survey's text.
SURVEY_8D_BYTES = {("humanoid", "f64"): 50392, ("humanoid32k", "f64"): 50392, ("ant", "f32"): 26392, ("mesh", "f32"): 13076, ("cartpole", "f64"): 2448}


def algorithmic_bytes_per_env_step(mx, dtype):
    """bytes of the Data leaves step() consumes + bytes of the leaves it produces."""
    from mujoco_torch_amd.forward import _written_names

    d = mt.make_data(mx)
    if dtype != torch.float64:
        d = d.to(dtype)
    written = _written_names(mx, step=True)
    nbytes = lambda n: native.data_field_tensor(d, n).numel() * native.data_field_tensor(d, n).element_size()
    out_b = sum(nbytes(n) for n in written)
    consumed = ["qpos", "qvel", "qacc", "act", "ctrl", "qfrc_applied", "xfrc_applied", "qacc_warmstart", "time", "qfrc_constraint"]
    in_b = sum(nbytes(n) for n in consumed)
    return in_b, out_b


KERNEL_NAME = {0: "mjh_phase_kernel<{r}, 0, W> (kinematics)", 1: "mjh_phase_kernel<{r}, 1, W> (crb / factor)", 2: "mjh_phase_kernel<{r}, 2, W> (collision / constraint)",
               3: "mjh_phase_kernel<{r}, 3, W> (velocity)", 4: "mjh_phase_kernel<{r}, 4, W> (solve / integrate)", 5: "mjh_phase_kernel<{r}, 5, W> (velocity + fluid)",
               6: "mjh_phase_kernel<{r}, 6, 64> (solve / integrate, general rows)", 7: "mjh_phase_kernel<{r}, 7, 64> (collision / constraint, general rows)",
               8: "mjh_phase_kernel<{r}, 8, W> (collision / constraint, rows straight to the leaf)",
               9: "mjh_sol2_kernel<{r}, NMAX, RPL> (solve / integrate: register solver, two environments per wavefront)", 10: "mjh_convex_kernel<{r}>", 11: "mjh_sensor_kernel<{r}>",
               12: "mjh_phase_kernel<{r}, 12, W> (kinematics + velocity in one launch)",
               13: "mjh_phase_kernel<{r}, 13, W> (kinematics + crb / factor + velocity in one launch)",
               14: "mjh_sol2_kernel<{r}, 28, 1, 33 | 35> (collision / constraint + register solver + integrator in one launch)",
               15: "mjh_sort_kernel (environments ordered by last step's solver iteration counts)",
               16: "mjh_sol2_kernel<{r}, 28, 1, 34 | 36> (the whole pass in one launch: kinematics + crb / factor + velocity + collision / constraint + register solver + integrator; 36: opt.iterations == 1)",
               17: "mjh_phase_kernel<{r}, 17, W> (kernel 13 on two wavefronts per workgroup: kinematics, then velocity beside crb / factor)",
               19: "mjh_sol2_kernel<{r}, NMAX, RPL, 18> (parts 2 | 4: collision / constraint + the register solver's first tier + integrator in one launch)",
               18: "mjh_sol2_kernel<{r}, 8, RPL, 18> (one RK4 stage in one launch: kinematics + crb / factor + velocity, collision / constraint, the register solver's first tier + integrator)"}


def kernel_algorithmic_bytes(nm):
    """{kernel id: (bytes read, bytes written) per environment and launch}: the library's own account of the global-memory
    extents each kernel touches (mjh_model_kernel_io: written next to the kernels' load / store code, csrc/mjh_io.h)."""
    import ctypes

    out = {}
    for k in range(20):
        rw = (ctypes.c_int64 * 2)()
        if nm.lib.mjh_model_kernel_io(nm.handle, k, rw) == 0:
            out[k] = (int(rw[0]), int(rw[1]))
    return out


def per_kernel_times(stepper, steps, device):
    """Average duration of every kernel of a step, from HIP events recorded on the launch stream around each launch."""
    import ctypes

    lib = native.load_library()
    lib.mjh_debug_phase_timing(1)
    ms = (ctypes.c_float * 96)()
    ids = (ctypes.c_int * 96)()
    tot, cnt = {}, {}
    try:
        for _ in range(steps):
            stepper()
            n = lib.mjh_debug_phase_times(ms, ids, 96)
            if n < 0:
                raise RuntimeError(lib.mjh_last_error().decode())
            for i in range(n):
                tot[ids[i]] = tot.get(ids[i], 0.0) + ms[i]
                cnt[ids[i]] = cnt.get(ids[i], 0) + 1
    finally:
        lib.mjh_debug_phase_timing(0)
    torch.cuda.synchronize(device)
    return {k: dict(avg_ms=tot[k] / cnt[k], launches_per_step=cnt[k] / steps, ms_per_step=tot[k] / steps) for k in tot}


def build_inputs(mx, B, dtype, device, seed=42):
    d = mt.make_data(mx).expand(B).clone()
    d = d.replace(qvel=torch.tensor(0.01 * np.random.RandomState(seed).randn(B, mx.nv)))
    if dtype != torch.float64:
        d = d.to(dtype)
    return d.to(device)


def data_arrays(d, prefix=""):
    """{name: tensor}: every per-environment array of a Data as its caller receives it; a nested container's leaves (contact) carry its name as
    a prefix.  The model constants a Data carries (UnbatchedTensor: ncon, nefc) are not step outputs and are not listed."""
    out = {}
    for k, v in d.items():
        if isinstance(v, mt.MjTensorClass):
            out.update(data_arrays(v, prefix + k + "_"))
        elif isinstance(v, torch.Tensor):
            out[prefix + k] = v
    return out


def dump_outputs(d, out_dir, batch):
    """--dump-outputs: every non-empty array of `d` as out_dir/<name>.npy, float32 arrays as float32 and all others (float64, integer, bool) as
    float64.  Zero-size arrays (a model without actuator activations, tendons, contacts, ...) hold no value and are left out.  When the batch's
    arrays would exceed DUMP_CAP_BYTES, every array keeps the same environments: a sorted sample drawn with DUMP_SAMPLE_SEED, identical from
    run to run.  Copies leaf by leaf to the host: no device allocation."""
    leaves = {n: t for n, t in data_arrays(d).items() if t.numel() > 0}
    kind = {n: np.float32 if t.dtype == torch.float32 else np.float64 for n, t in leaves.items()}
    per_env = sum(t.numel() // batch * np.dtype(kind[n]).itemsize for n, t in leaves.items())
    n_env = min(batch, (DUMP_CAP_BYTES - 256 * len(leaves)) // per_env)  # (256: bound on one .npy header)
    idx = None if n_env == batch else np.sort(np.random.RandomState(DUMP_SAMPLE_SEED).choice(batch, n_env, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in leaves.items():
        a = t.detach().cpu().numpy()
        if idx is not None:
            a = a[idx]
        path = os.path.join(out_dir, name + ".npy")
        np.save(path, a.astype(kind[name], copy=False))
        total += os.path.getsize(path)
    assert total <= DUMP_CAP_BYTES, f"--dump-outputs wrote {total} bytes"
    return {"dir": os.path.abspath(out_dir), "files": len(leaves), "bytes": total, "envs": n_env, "of_envs": batch,
            "sample_seed": None if idx is None else DUMP_SAMPLE_SEED}


def usable_cpus():
    """What this process may actually run on: the affinity mask, the cgroup CPU quota (v2 cpu.max / v1 cfs_quota_us) and the physical cores behind
    the mask (SMT siblings share one core's FP pipes).  `omp_get_max_threads()` reports none of these: round 5's all-threads leg ran 128 threads and
    scaled 6.2 x."""
    import math

    aff = sorted(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = float(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = float(f.read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    cores = set()
    try:
        for c in aff:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/core_id") as f:
                cid = f.read().strip()
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id") as f:
                pkg = f.read().strip()
            cores.add((pkg, cid))
    except OSError:
        cores = set()
    threads = len(aff)
    if quota is not None:
        threads = max(1, min(threads, int(math.floor(quota + 1e-9)) or 1))
    return {"affinity_cpus": len(aff), "cgroup_cpu_quota": quota, "physical_cores_in_mask": len(cores) or None, "os_cpu_count": os.cpu_count(),
            "loadavg_1min": os.getloadavg()[0], "threads": threads}


def cpu_baseline(mx, dtype, B_sample, steps):
    """Times the CPU oracle (scalar C restatement of the reference step, OpenMP over envs) on the host cores this process may use -- the affinity
    mask capped by the cgroup quota, NOT the machine's hardware-thread count -- and on ONE thread (load-independent).  When the
    all-threads leg scales worse than half of threads x single-thread (SMT siblings, a loaded shared host), smaller thread counts are tried and
    the BEST is reported with the count that produced it; if even that stays under half of (physical cores used) x single-thread the object says so
    loudly (`healthy: false`, stderr) instead of printing a strawman beside the GPU figure."""
    import pyoracle

    pyoracle.build()
    cpus = usable_cpus()
    threads = cpus["threads"]

    def sample(nB, nthreads, min_steps, t_min, t_max):
        d = mt.make_data(mx).expand(nB).clone()
        d = d.replace(qvel=torch.tensor(0.01 * np.random.RandomState(42).randn(nB, mx.nv)))
        if dtype != torch.float64:
            d = d.to(dtype)
        return pyoracle.time_steps(mx, d, nthreads, min_steps, t_min, t_max)  # the C step only: packed once, buffers ping-pong

    n1 = min(B_sample, 256)
    v1, done1, dt1 = sample(n1, 1, 2, 4.0, 12.0)
    tried = []
    v, done, dt = sample(B_sample, threads, steps, 8.0, 24.0)
    tried.append({"threads": threads, "value": v, "seconds": dt})
    best = (v, done, dt, threads)
    phys = cpus["physical_cores_in_mask"] or threads
    for t in sorted({max(1, min(threads, phys)), max(1, threads // 2), max(1, threads // 4)} - {threads}, reverse=True):
        if best[0] >= 0.5 * best[3] * v1:
            break
        vt, donet, dtt = sample(B_sample, t, steps, 4.0, 10.0)
        tried.append({"threads": t, "value": vt, "seconds": dtt})
        if vt > best[0]:
            best = (vt, donet, dtt, t)
    v, done, dt, used = best
    eff_threads = v / (used * v1)
    eff_cores = v / (min(used, phys) * v1)
    healthy = eff_cores >= 0.5
    out = dict(single_thread=dict(value=v1, unit="env-steps/s", cores=1, sample=f"{n1} envs x {done1} steps on one thread ({dt1:.1f} s)",
                                  note="load-independent: quote this one when comparing boxes"),
               value=v, unit="env-steps/s", cores=used, kind="port",
               sample=f"{B_sample} envs x {done} steps of one trajectory, oracle/mjoracle.c (mjo_step calls only) with OpenMP over environments on {used} threads ({dt:.1f} s)",
               host=cpus, thread_counts_tried=tried, scaling_vs_single_thread=v / v1, parallel_efficiency_per_thread=eff_threads,
               parallel_efficiency_per_physical_core=eff_cores, healthy=healthy)
    if not healthy:
        out["error"] = (f"all-threads CPU leg reached only {v / v1:.1f} x one thread on {used} threads ({min(used, phys)} physical cores): below half of linear; "
                        "the host is loaded or the mask / quota is wrong -- do not quote `value`, quote single_thread")
        print("bench.py: CPU BASELINE UNHEALTHY: " + out["error"], file=sys.stderr, flush=True)
    return out


class Loop:
    """The two ways to drive the step: the reference signature (fresh outputs per call) and ping-pong `out=` buffers."""

    def __init__(self, mdev, d):
        self.mdev, self.d = mdev, d
        self.bufs = None

    def dropin(self, n):
        d, m = self.d, self.mdev
        self.d = None  # (the loop holds the only reference: a second one kept the first input's storage alive for the whole loop -- one more slab in flight than the
        #                warm-up ever had, i.e. a driver-level allocation of 1.5 GB (B = 32768) inside the timed region that costs up to 40 ms when the driver is slow to serve it)
        for _ in range(n):
            d = mt.step(m, d)
        self.d = d

    def pingpong(self, n):
        if self.bufs is None:
            self.bufs, self.cur = [self.d.clone(), self.d.clone()], 0
        for _ in range(n):
            mt.step(self.mdev, self.bufs[self.cur], out=self.bufs[1 - self.cur])
            self.cur = 1 - self.cur


LAST_TIMED = {}


def timed(fn, steps, device, world, backend):
    """barrier + synchronize on both sides of exactly `steps` steps; wall time (max over ranks) and device time (events)."""
    torch.cuda.synchronize(device)
    if DIST_ON:
        dist.barrier()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # torch creates the HIP event behind an Event at its FIRST record(): 0.2 - 0.5 ms for the first timing events of a process (measured, tools/window_probe.py) -- inside the
    # bracket that was 7 - 15 % of the driver's 20-step window, charged to the steps.  Both events are recorded once here, outside the bracket; recording them again is cheap.
    ev0.record()
    ev1.record()
    torch.cuda.synchronize(device)
    ms0 = torch.cuda.memory_stats(device)
    a0, r0 = ms0.get("num_device_alloc", 0), ms0.get("reserved_bytes.all.current", 0)
    t0 = time.perf_counter()
    ev0.record()
    fn(steps)
    ev1.record()
    torch.cuda.synchronize(device)
    own = time.perf_counter() - t0      # this rank's own K steps (before the barrier: a straggler shows up in the per-rank spread below)
    if DIST_ON:
        dist.barrier()
    elapsed = time.perf_counter() - t0  # read BEFORE the allocator statistics are collected (building that dict costs ~0.1 ms: ADVICE r03)
    ms1 = torch.cuda.memory_stats(device)
    LAST_TIMED["device_allocs"] = [ms1.get("num_device_alloc", 0) - a0, (ms1.get("reserved_bytes.all.current", 0) - r0) >> 20]  # driver-level allocations inside the region and the MiB they added (0 once the caching allocator is warm)
    LAST_TIMED["per_rank_ms_per_step"] = None
    if DIST_ON:
        t = torch.tensor([elapsed, own, -own], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0].item())
        # fastest / slowest rank's own time for the same K steps: `value` is computed from the max-reduced bracket, which hides WHICH rank set it
        LAST_TIMED["per_rank_ms_per_step"] = {"min": 1e3 * -float(t[2].item()) / steps, "max": 1e3 * float(t[1].item()) / steps}
    return elapsed, ev0.elapsed_time(ev1) / steps


def lib_fingerprint():
    import hashlib

    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "mujoco-torch_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".h", ".hip")):
            with open(os.path.join(csrc, f), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


PROFILE_ROUND = "r06"   # profiles/<round>/: where this round's committed PMC traffic and parity summaries live


def setup_workload(key, B, device, rank):
    wl = WORKLOADS[key]
    B = B or wl["batch"]
    dtype = wl["dtype"]
    if ARGS is not None and getattr(ARGS, "dtype", "") and key == ARGS.workload:
        dtype = torch.float64 if ARGS.dtype == "f64" else torch.float32
        wl = dict(wl, dtype=dtype, name=wl["name"] + f" [dtype overridden: {ARGS.dtype}]")
    lite = mt.mjcf.from_xml_path(mt.test_data_path(wl["xml"] + ".xml"))
    for k, v in wl["overrides"].items():
        setattr(lite.opt, k, v)
    for kv in filter(None, os.environ.get("BENCH_OPT", "").split(",")):  # experiments only, e.g. BENCH_OPT=iterations=3 (the line's config.workload says so)
        k, v = kv.split("=")
        setattr(lite.opt, k, type(getattr(lite.opt, k))(float(v)))
        wl = dict(wl, name=wl["name"] + f" [BENCH_OPT {kv}]")
    mx = mt.device_put(lite, dtype=None if dtype == torch.float64 else dtype)
    mdev = mx.to(device)
    # different seeds per rank: independent environments, no collective on the data path
    loop = Loop(mdev, build_inputs(mx, B, dtype, device, seed=42 + rank))
    return wl, B, dtype, mx, mdev, loop


def spin_up(mdev, loop, n):
    """Clocks, allocator pools and the library's plan caches reach their steady state on a SCRATCH copy of the inputs (n untimed
    steps); the measured loop then starts from the original state."""
    scratch = Loop(mdev, loop.d.clone())
    scratch.dropin(n)
    del scratch


def roofline_of(key, B, dtype, mx, mdev, loop, device, kernel_ms, steps):
    """The `roofline` object of one workload (rank 0): per-kernel HIP-event times of the drop-in loop (outside the timed region), the
    library's own byte account per kernel, and -- when the committed PMC file was collected on THIS library -- the measured traffic."""
    nm = native.get_native_model(mdev, device, dtype)
    kernels = per_kernel_times(lambda: loop.dropin(1), min(steps, 50), device)  # events around every launch
    fp = lib_fingerprint()
    tag = f"{key}_b{B}_{'f64' if dtype == torch.float64 else 'f32'}"
    tfile = os.path.join(ROOT, "profiles", PROFILE_ROUND, f"hbm_traffic_{tag}.json")
    tj = None
    if os.path.exists(tfile):  # PMC counters cannot be collected from inside this process: the committed rocprofv3 result (tools/hbm_traffic.sh)
        with open(tfile) as f:
            tj = json.load(f)
    in_b, out_b = algorithmic_bytes_per_env_step(mx, dtype)
    alg_leaves = in_b + out_b
    dkey = "f64" if dtype == torch.float64 else "f32"
    plain = not os.environ.get("BENCH_OPT") and not (ARGS is not None and getattr(ARGS, "dtype", ""))
    alg = SURVEY_8D_BYTES.get((key, dkey), alg_leaves) if plain else alg_leaves
    achieved = alg * B / (kernel_ms * 1e-3) / 1e9
    rname = "double" if dtype == torch.float64 else "float"
    kio = kernel_algorithmic_bytes(nm)
    per_kernel = []
    for k, t in sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_step"]):
        rd, wr = kio.get(k, (0, 0))
        gbs = (rd + wr) * B / (t["avg_ms"] * 1e-3) / 1e9
        per_kernel.append({"kernel": KERNEL_NAME[k].format(r=rname), "id": k, "avg_us": 1e3 * t["avg_ms"], "launches_per_step": t["launches_per_step"],
                           "kernel_io_bytes_per_env": rd + wr, "read_bytes_per_env": rd, "written_bytes_per_env": wr, "kernel_io_achieved": gbs, "kernel_io_frac": gbs / HBM_PEAK_GBS})
    dom = per_kernel[0]
    # the step's algorithmic bytes over the launch(es) that move them.  A one-launch step (the headline humanoid) prices its kernel at the
    # whole figure: 50,392 B x B / that kernel's average launch duration.  A step of several launches has no per-kernel split of the figure in the survey
    # (RK4 stages 1..3 and the hand-overs between phases move no algorithmic byte at all), so the dominant kernel is priced at the step's figure over
    # the SUM of the step's launch durations -- the number VERDICT r05 computed by hand; the library's own per-kernel account stays as kernel_io_*.
    launches_ms = sum(t["ms_per_step"] for t in kernels.values())
    one_launch = len(kernels) == 1 and abs(dom["launches_per_step"] - 1.0) < 1e-9
    d8_ms = dom["avg_us"] * 1e-3 if one_launch else launches_ms
    d8_achieved = alg * B / (d8_ms * 1e-3) / 1e9
    ktraffic, traffic, tsrc = None, None, None
    if tj is not None:
        stale = tj.get("lib_fingerprint") != fp
        tsrc = {"file": os.path.relpath(tfile, ROOT), "git_commit": tj.get("git_commit"), "lib_fingerprint": tj.get("lib_fingerprint"),
                "measured_in_this_run": False, "kernels_changed_since": stale}
        if not stale:
            traffic = tj.get("hbm_bytes_per_step")
            best_disp = 0
            for name, v in tj.get("kernels", {}).items():  # PMC bytes per launch of the dominant kernel (FETCH_SIZE corrected x2)
                pat = "mjh_sol2_kernel<" if dom["id"] in (9, 14, 16, 18, 19) else ("mjh_convex_kernel<" if dom["id"] == 10 else ("mjh_sensor_kernel<" if dom["id"] == 11 else f"mjh_phase_kernel<{rname}, {dom['id']},"))
                if pat not in name:
                    continue
                kb = 2 * 1024 * v["FETCH_SIZE_KB_raw_mean"] + 1024 * v["WRITE_SIZE_KB_mean"]
                if dom["id"] == 9:  # the register solver's two row tiers are two kernels under one timing mark: their bytes add up
                    ktraffic = (ktraffic or 0) + kb * v.get("dispatches_per_step", 0) / max(dom["launches_per_step"], 1e-9)
                elif v.get("dispatches_per_step", 0) >= best_disp:  # (the packed variant, not the odd-tail launch)
                    best_disp = v.get("dispatches_per_step", 0)
                    ktraffic = kb
    # dominant kernel of the step: the global-memory bytes its code reads + writes per launch / its average launch duration (HIP
    # events around each launch, on the launch stream); "step" = the same for the whole launch sequence (SURVEY 8(d) per-unit figure)
    return {"bound": "hbm", "achieved": d8_achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": d8_achieved / HBM_PEAK_GBS, "traffic": ktraffic if one_launch else traffic,
            "kernel": dom["kernel"], "kernel_avg_us": dom["avg_us"], "algorithmic_bytes_per_launch": alg * B if one_launch else None,
            "frac_is": (f"SURVEY 8(d) {alg} B/env-step x {B} envs / the one launch of the step ({dom['avg_us']:.1f} us, HIP events on the launch stream)" if one_launch else
                        f"SURVEY 8(d) {alg} B/env-step x {B} envs / the sum of the step's launch durations ({1e3 * launches_ms:.1f} us over {sum(t['launches_per_step'] for t in kernels.values()):.0f} launches, HIP events on the launch stream); `kernel` names the longest of them"),
            "algorithmic_bytes_per_env_step": alg, "algorithmic_bytes_per_env_step_from_leaf_sizes": alg_leaves,
            "kernel_io_frac": dom["kernel_io_frac"], "kernel_io_achieved": dom["kernel_io_achieved"], "kernel_io_bytes_per_launch": dom["kernel_io_bytes_per_env"] * B,
            "kernel_io_is": "the library's own account of the global-memory extents the dominant kernel's code reads + writes (csrc/mjh_io.h; counts re-reads of leaves the same launch wrote): traffic-like, not SURVEY 8(d)",
            "traffic_source": tsrc, "per_kernel": per_kernel,
            "step": {"achieved": achieved, "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "algorithmic_bytes_per_env_step": alg,
                     "algorithmic_bytes_per_step": alg * B, "device_ms_per_step": kernel_ms,
                     "kernels": "every launch of one step (torch events on the launch stream over the timed region)"}}, nm


def secondary_workload(key, device, world, rank, backend, steps=200, warmup=20, spin=100, repeats=3):
    """BASELINE configs 3 / 5 timed by the same drop-in loop inside the headline run: a fixed recipe -- `spin`
    untimed steps on a scratch copy, then from the ORIGINAL state `warmup` untimed and `steps` timed steps -- independent of the headline's
    --steps / --warmup, so the figure is the same trajectory window whoever launches the bench.  The recipe runs `repeats` times from
    scratch (same seeds, same trajectory): device clocks on this pool move the same window by up to 8 % between repetitions
    (profiles/r03/notes.md); `value` is the MEDIAN repetition (round 3 reported the fastest, which is not how the single-shot headline is
    measured: ADVICE r03), `repeats` lists every one."""
    runs, best = [], None
    for _ in range(repeats):
        torch.cuda.empty_cache()  # the previous workload's cached blocks go back to the driver: this one allocates like a process of its own
        wl, B, dtype, mx, mdev, loop = setup_workload(key, 0, device, rank)
        spin_up(mdev, loop, spin)
        loop.dropin(warmup)
        elapsed, kernel_ms = timed(loop.dropin, steps, device, world, backend)
        assert torch.isfinite(loop.d.qpos).all(), f"{key}: non-finite state after the timed steps"
        runs.append({"value": B * world * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps, "device_ms_per_step": kernel_ms})
        if best is not None:
            del best
        best = (loop, mx, mdev)  # the per-kernel pass below runs on the last repetition's state (same trajectory window every time)
        del loop
    loop, mx, mdev = best
    med = sorted(runs, key=lambda r: r["ms_per_step"])[len(runs) // 2]
    elapsed, kernel_ms = med["ms_per_step"] * steps / 1e3, med["device_ms_per_step"]
    res = {"workload": wl["name"], "envs_per_gpu": B, "global_batch": B * world, "dtype": "f64" if dtype == torch.float64 else "f32",
           "steps": steps, "warmup": warmup, "spin_up_steps_on_a_scratch_state": spin,
           "value": B * world * steps / elapsed, "unit": "env-steps/s", "ms_per_step": 1e3 * elapsed / steps, "device_ms_per_step": kernel_ms,
           "value_is": f"median of {repeats} repetitions of the same window", "repeats": runs}
    if rank == 0:
        res["roofline"], _ = roofline_of(key, B, dtype, mx, mdev, loop, device, kernel_ms, steps)
    del loop
    torch.cuda.empty_cache()
    return res


def _cpulist(txt):
    out = []
    for part in txt.strip().split(","):
        if part:
            a, _, b = part.partition("-")
            out += list(range(int(a), int(b or a) + 1))
    return out


def gpu_numa_nodes():
    """[NUMA node of GPU 0, GPU 1, ...] from the KFD topology in sysfs -- NO HIP call (this runs before the process touches the GPU).  KFD lists the GPU nodes in the
    order the runtime enumerates them (the visible-devices variables select / reorder by index: honoured below); -1 where the kernel does not say."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    gpus = []
    for n in sorted(os.listdir(base), key=int):
        props = {}
        with open(os.path.join(base, n, "properties")) as f:
            for ln in f:
                k, _, v = ln.strip().partition(" ")
                props[k] = v
        if int(props.get("simd_count", "0")) == 0:
            continue  # a CPU node
        numa = -1
        minor = props.get("drm_render_minor")
        if minor:
            try:
                with open(f"/sys/class/drm/renderD{minor}/device/numa_node") as f:
                    numa = int(f.read())
            except OSError:
                pass
        gpus.append(numa)
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):  # applied in this order by the runtime
        sel = os.environ.get(var)
        if sel and all(x.strip().isdigit() for x in sel.split(",")):
            gpus = [gpus[int(x)] for x in sel.split(",") if int(x) < len(gpus)]
    return gpus


def pin_rank_to_its_gpus_cores(local_rank, local_world):
    """One rank per GPU on one node: bind this rank's host threads to a slice of the cores of ITS GPU's NUMA node (the ranks whose GPUs share the node split the node's
    allowed cores between them), before the first HIP call so that the runtime's own threads inherit the mask.  A step is 1 .. 13 launches issued from one host thread
    (50 us of host work per call): ranks that share cores or sit on the far socket show up as stragglers in `per_rank_ms_per_step`.  Returns what was done (for `ranks[]`)."""
    before = sorted(os.sched_getaffinity(0))
    info = {"cpus_before": len(before)}
    try:
        numa = gpu_numa_nodes()
        if local_rank >= len(numa):
            raise RuntimeError(f"{len(numa)} GPUs in the KFD topology, local rank {local_rank}")
        node = numa[local_rank]
        info["gpu_numa_node"] = node
        if node >= 0:
            with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
                cpus = [c for c in _cpulist(f.read()) if c in before]
        else:
            cpus = before
        sharers = [r for r in range(min(local_world, len(numa))) if numa[r] == node] if node >= 0 else list(range(local_world))
        k, n = sharers.index(local_rank) if local_rank in sharers else 0, max(1, len(sharers))
        per = len(cpus) // n
        mine = cpus[k * per:(k + 1) * per] if per >= 1 else cpus
        if not mine:
            raise RuntimeError("no allowed CPU on the GPU's NUMA node")
        os.sched_setaffinity(0, mine)
        info.update(pinned=True, cpus=len(mine), cpu_first=mine[0], cpu_last=mine[-1], ranks_sharing_the_node=n)
    except Exception as ex:  # noqa: BLE001  (a placement hint must never cost the run)
        info.update(pinned=False, note=f"{type(ex).__name__}: {ex}")
    return info


DIST_ON = False  # torch.distributed initialised: N > 1, or the one-GPU exercise of the RCCL path (MJH_BENCH_FORCE_DIST=1)


def main(args):
    global DIST_ON
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (python bench.py --gpus N spawns them itself)")
    # test hooks for a one-GPU box: MJH_BENCH_BACKEND=gloo + MJH_BENCH_SHARE_GPU=1 run every rank on cuda:0 (RCCL refuses
    # two ranks on one device); the driver's multi-GPU runs use the defaults (RCCL, one GPU per rank)
    backend = os.environ.get("MJH_BENCH_BACKEND", "nccl")
    if os.environ.get("MJH_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    elif world > 1 and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: --gpus {world} but only {torch.cuda.device_count()} devices are visible")
    # MJH_BENCH_FORCE_DIST=1 (tests/test_gpu_parity.py::test_bench_rccl_path_on_one_gpu): a world of ONE rank still goes through init_process_group("nccl", device_id=...),
    # every barrier / all_reduce / all_gather_object of the N > 1 path and destroy_process_group -- the RCCL code path had never executed anywhere (VERDICT r05 missing 1)
    DIST_ON = world > 1 or os.environ.get("MJH_BENCH_FORCE_DIST") == "1"
    pin = None
    if DIST_ON and os.environ.get("MJH_BENCH_PIN", "1") == "1":
        pin = pin_rank_to_its_gpus_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))  # BEFORE the first HIP call
    if DIST_ON:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    # which device every rank drives: one rank per GPU means `world` distinct (host, device uuid / index) pairs
    props = torch.cuda.get_device_properties(device)
    me = {"rank": rank, "local_rank": local_rank, "device_index": device.index, "device_name": torch.cuda.get_device_name(device), "visible_devices": torch.cuda.device_count(),
          "uuid": str(getattr(props, "uuid", "")), "cus": props.multi_processor_count, "HIP_VISIBLE_DEVICES": os.environ.get("HIP_VISIBLE_DEVICES"), "ROCR_VISIBLE_DEVICES": os.environ.get("ROCR_VISIBLE_DEVICES"),
          "host_affinity": pin, "backend": backend if DIST_ON else None}
    ranks = [me]
    if DIST_ON:
        try:
            gathered = [None] * world
            dist.all_gather_object(gathered, me)
            ranks = gathered
        except Exception as ex:  # noqa: BLE001  (a report field must never cost the run its measurement)
            ranks = [dict(me, note=f"all_gather_object failed: {type(ex).__name__}")]

    wl, B, dtype, mx, mdev, loop = setup_workload(args.workload, args.batch, device, rank)
    loop.bufs, loop.cur = [loop.d.clone(), loop.d.clone()], 0   # the out= loop starts from the same state (solver work depends on it)

    SPIN_UP = int(os.environ.get("BENCH_SPIN_UP", "100"))
    spin_up(mdev, loop, SPIN_UP)
    loop.dropin(args.warmup)
    elapsed, kernel_ms = timed(loop.dropin, args.steps, device, world, backend)       # THE measurement: d = step(mx, d)
    allocs_in_region = LAST_TIMED.get("device_allocs")
    per_rank = LAST_TIMED.get("per_rank_ms_per_step")
    assert torch.isfinite(loop.d.qpos).all(), "non-finite state after the timed steps"
    dumped = None
    if args.dump_outputs and rank == 0:  # before anything below steps `loop.d` further
        dumped = dump_outputs(loop.d, args.dump_outputs, B)
    loop.pingpong(args.warmup)
    elapsed_pp, kernel_ms_pp = timed(loop.pingpong, args.steps, device, world, backend)  # extension: step(mx, a, out=b)

    # SURVEY 8(d)'s recipe beside the headline figure: 1000 more steps of the same trajectory through the same loop, so that `value` (the
    # driver's --steps, 20 at round end = 4 ms) is not the only sample of the headline workload
    long_run = None
    if not args.no_long_run:
        nl = 1000
        el, kl = timed(loop.dropin, nl, device, world, backend)
        assert torch.isfinite(loop.d.qpos).all(), "non-finite state after the long run"
        long_run = {"steps": nl, "value": B * world * nl / el, "unit": "env-steps/s", "ms_per_step": 1e3 * el / nl, "device_ms_per_step": kl,
                    "starts_after": f"{args.warmup} warm-up + {args.steps} timed steps of the same trajectory"}

    config4 = None
    if DIST_ON and args.workload == "humanoid" and not args.batch and not args.no_config4:
        # BASELINE config 4 beside the headline batch: 32768 environments per GPU (262144 on 8 GPUs), same loop
        big = Loop(mdev, build_inputs(mx, 32768, dtype, device, seed=1042 + rank))
        big.dropin(max(3, args.warmup // 4))
        n4 = max(20, args.steps // 4)  # >= 20 steps (~26 ms) whatever --steps is
        e4, k4 = timed(big.dropin, n4, device, world, backend)
        config4 = {"per_rank_ms_per_step": LAST_TIMED.get("per_rank_ms_per_step"),"workload": WORKLOADS["humanoid32k"]["name"], "envs_per_gpu": 32768, "global_batch": 32768 * world, "steps": n4,
                   "value": 32768 * world * n4 / e4, "unit": "env-steps/s", "ms_per_step": 1e3 * e4 / n4, "device_ms_per_step": k4}
        del big
        torch.cuda.empty_cache()

    roof = None
    if rank == 0:
        roof, nm = roofline_of(args.workload, B, dtype, mx, mdev, loop, device, kernel_ms, args.steps)

    # BASELINE configs 3 and 5 in the same line (every rank takes part: the barrier-bracketed timing is collective)
    others = {}
    if args.workload == "humanoid" and not args.batch and not args.no_other_workloads:
        for key in ("ant", "mesh"):
            others[key] = secondary_workload(key, device, world, rank, backend)

    if rank == 0:
        value = B * world * args.steps / elapsed
        line = {
            "metric": "env-steps/sec", "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "f64" if dtype == torch.float64 else "f32", "data": "synthetic",
            "config": {"workload": wl["name"], "envs_per_gpu": B, "global_batch": B * world,
                       "call": "d = mujoco_torch.step(mx, d)  (reference signature, forward.py:463; fresh output storage every call)",
                       "spin_up_steps_on_a_scratch_state": SPIN_UP,
                       "parallelism": f"independent-envs x{world} (no collectives)",
                       "lds_bytes_per_env_by_phase": nm.lds_bytes},
            # the same loop through the `out=` extension (ping-pong buffers, no allocation): how far the drop-in call is from it
            "out_buffers": {"value": B * world * args.steps / elapsed_pp, "ms_per_step": 1e3 * elapsed_pp / args.steps, "device_ms_per_step": kernel_ms_pp,
                            "call": "mujoco_torch.step(mx, a, out=b)"},
            "roofline": roof,
            "device_allocations_in_timed_region": allocs_in_region,  # hipMalloc calls of torch's caching allocator between the two synchronizes (each one stalls the host for ~1 ms at these sizes)
        }
        line["ranks"] = ranks
        if DIST_ON:
            line["collectives"] = {"backend": backend, "initialised_with_device_id": backend == "nccl", "used": ["barrier", "all_reduce(MAX)", "all_gather_object"],
                                   "on_the_data_path": "none (independent environments)"}
        line["one_device_per_rank"] = len(ranks) == world and len({(r["uuid"] or r["device_index"]) for r in ranks}) == world  # false only under the one-GPU test hook (MJH_BENCH_SHARE_GPU=1)
        if per_rank is not None:
            line["per_rank_ms_per_step"] = per_rank  # every rank's own K steps, fastest and slowest (the bracket above is max-reduced)
        if long_run is not None:
            line["long_run"] = long_run
        if others:
            line["other_workloads"] = others
        if config4 is not None:
            line["config4"] = config4
        if dumped is not None:
            line["dump_outputs"] = dumped
        pfile = os.path.join(ROOT, "profiles", PROFILE_ROUND, "parity.json")
        if os.path.exists(pfile):  # "float64 max rel-err" half of BASELINE's metric: written by tests/test_gpu_parity.py::test_parity_report
            with open(pfile) as f:
                pj = json.load(f)
            line["parity"] = {"file": f"profiles/{PROFILE_ROUND}/parity.json", "measured_in_this_run": False, **{k: pj[k] for k in ("reference", "summary") if k in pj}}
        if not args.no_cpu_baseline and world == 1:
            nB = min(B, 4096)
            line["cpu_baseline"] = cpu_baseline(mx, dtype, nB, 20 if args.workload != "ant" else 4)
        print(json.dumps(line))
    if DIST_ON:
        dist.barrier()  # rank 0 runs the per-kernel pass after the timed region: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main(ARGS)
