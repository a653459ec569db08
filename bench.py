#!/usr/bin/env python3
"""Benchmark: edges subdivided / second on the north-star synthetic workload.

One "step" = one full pass of the hot path (tropical.subpoly's hyperplane
loop, subpoly.py:58-69) over one synthetic input: load the initial lattice
and its cached pre-activations (one forward over every lattice vertex), then
every hyperplane step (split, new-vertex forward, failover override,
connecting edges, pruning, compaction), all in HBM on the HIP engine.

Workload: synthetic random-weight trilinear net,
Net(num_layers=3, num_hidden=16, levels=2, r_min=G-1, r_max=G-1, T=19)
(G marks per axis; hash table U(-0.1,0.1), nn.Linear-bound MLP, numpy PCG64
seed 6 by default, see --seed), initial edges = the full G^3 lattice.  G = 128 at one GPU; at N GPUs
the lattice grows to round(128 * N^(1/3)) marks per axis and is cut into N
x-slabs of cells, each extracted with a halo of cells (as wide as halo_check needs) (weak scaling, one
process per GPU, RCCL only for the per-step 8-byte agreements; the slabs
are stitched into one complex after the timed region,
tropical/distributed.py).  value = edges subdivided by all ranks (each
split counted once, by the rank owning it) / max-over-ranks wall time.

Run: python bench.py [--gpus N --steps K --warmup W]  (N > 1: one process per GPU,
relaunched under torch.distributed.run unless already launched by it)

A plain run sets up, warms up, times the K passes and prints the result line.
--dump-outputs DIR also writes what the last timed pass computed (DIR/*.npy).
--full adds everything else: the per-kernel HIP-event pass and the roofline,
the final complex checked against the reference's fingerprint (N > 1: the
halo check and the stitch), the CPU baseline, and the bunny-scale, large-net
and finish-at-scale legs (--no-cpu leaves the CPU baseline and the legs out).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "tropical-nerf.pytorch_amd")
for _p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
# per-kernel HBM bytes per launch from the committed rocprofv3 --pmc passes of
# this workload (tools/pmc_session.sh + tools/pmc_table.py: 2*FETCH_SIZE +
# WRITE_SIZE, the gfx950 correction of MI355X_MICROARCH.md "HBM")
PMC_TABLE = os.path.join(ROOT, "profiles", "r06_bench128_seed6_pmc.json")
# engine timer name -> device kernel symbol (profiles' short names)
KERNEL_SYMBOL = {"forward_new": "k_forward_new", "prune": "k_prune_lb", "connect_win": "k_connect_win",
                 "bucket_group": "k_bucket_group", "split": "k_split_lb", "hits": "k_hit_lb",
                 "connect": "k_connect", "count_live": "k_count_flags", "override_new": "k_override_new"}


CLOCK_HZ = 2.4e9       # MI355X peak engine clock (MI355X_MICROARCH.md)
SIMDS = 256 * 4        # 256 CUs x 4 SIMD16: a wave64 VALU instruction issues over 4 cycles


def pmc_row(kernel: str, marks: int, seed: int):
    """The committed PMC counters per launch of `kernel` on the same workload
    (None: other workload, or no profile)."""
    if marks != 128 or seed != 6 or not os.path.isfile(PMC_TABLE):
        return None
    with open(PMC_TABLE) as f:
        ks = json.load(f)["kernels"]
    return ks.get(KERNEL_SYMBOL.get(kernel, "k_" + kernel))


def pmc_traffic(kernel: str, marks: int, seed: int):
    """HBM bytes per launch of `kernel` measured by the PMC passes of the
    same workload (None: other workload, or no profile)."""
    k = pmc_row(kernel, marks, seed)
    return None if k is None else k.get("traffic_bytes_per_launch")


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def synthetic_params(G: int, seed: int = 0, amp: float = 0.1):
    from tropical.synthetic import net_config_for_lattice, random_params
    from tropical.tropical import level_meta
    cfg = net_config_for_lattice(G)
    b = np.exp2(np.log2((cfg["r_max"] * 1.0) / cfg["r_min"]) / (cfg["levels"] - 1))
    n_params = level_meta(cfg["levels"], cfg["r_min"], b, cfg["T"])[-1] * 2
    nodes = [cfg["levels"] * 2] + [cfg["num_hidden"]] * (cfg["num_layers"] - 1) + [2]
    return cfg, random_params(n_params, nodes, seed, amp)


def make_net(G, device, seed=0):
    from tropical.stanford.model import Net
    cfg, p = synthetic_params(G, seed)
    net = Net(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return net.to(device)


def reference_fingerprint(G: int, seed: int):
    """(V, E, vertex-set hash, edge-set hash) of the reference's final
    complex on this workload, when a golden holds it (bench128: the
    reference run on the 128^3 seed-6 lattice in the build container)."""
    from golden_io import GOLDEN
    path = os.path.join(GOLDEN, "bench128.npz")
    if G != 128 or seed != 6 or not os.path.isfile(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        return tuple(int(x) for x in z["pre_VE"]) + tuple(int(x) for x in z["complex_hash"])


def algorithmic_bytes(st: dict, K: int) -> int:
    """SURVEY §8d per-step traffic model B_s (bytes the step must move)."""
    E_in, S, V_in = st["E_in"], st["S"], st["V_in"]
    C = 3 + K
    b = 16 * E_in
    if S > 0:
        b += (184 * S + math.ceil(2 * C / 8) * V_in + 8 * (E_in + 2 * S + st["X"])
              + 8 * st["E_out"] + 2 * (12 + 4 * K) * st["V_out"] + 56 * st["A"] + 34 * st["P"])
    return b


class Collective:
    """Per-step agreements between slab ranks (the reference's global
    decisions, subpoly.py:110 and subpoly_debug.py:43-49): ONE all_gather of
    each rank's few int64 words (RCCL over xGMI, or gloo on the host), reduced
    on the host -- OR for the 64-bit plane masks (RCCL has no bitwise-or
    reduction), MAX for {split count, failover flag}; one readback.  When
    every rank is on this node the words go through host shared memory
    instead (ShmCollective: no library call, no device copies)."""

    def __init__(self, device, shm: bool = None):
        import torch.distributed as dist
        self.dist = dist
        self.device = device
        self.world = dist.get_world_size()
        # every rank on this node (torchrun's LOCAL_WORLD_SIZE): the words go
        # through host shared memory instead (tropical.distributed.ShmCollective)
        if shm is None:
            shm = (os.environ.get("TNP_SHM_COLLECTIVE", "1") == "1" and
                   int(os.environ.get("LOCAL_WORLD_SIZE", "-1")) == self.world)
        self.shm = None
        if shm:
            from tropical.distributed import ShmCollective
            self.shm = ShmCollective()

    def __call__(self, vec: np.ndarray, op: str):
        if self.shm is not None:
            return self.shm(vec, op)
        words = np.ascontiguousarray(vec.astype(np.uint64 if op in ("or", "and") else np.int64)).view(np.int64)
        t = torch.from_numpy(words.copy()).to(self.device)
        out = torch.empty(self.world * t.numel(), dtype=torch.int64, device=self.device)
        self.dist.all_gather_into_tensor(out, t)
        a = out.cpu().numpy().reshape(self.world, -1)
        if op == "or":
            return np.bitwise_or.reduce(a.view(np.uint64), axis=0).astype(vec.dtype)
        if op == "and":
            return np.bitwise_and.reduce(a.view(np.uint64), axis=0).astype(vec.dtype)
        if op == "sum":
            return a.sum(axis=0)
        return a.max(axis=0)


def log(msg: str) -> None:
    """Progress on stderr (the JSON line alone goes to stdout)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def cpu_threads() -> int:
    """Host threads for the CPU baseline: the usable cores
    (sched_getaffinity), capped by the job's CPU share when the launcher
    states one (OMP_NUM_THREADS: the GPU box gives one GPU's job 16 of the
    host's cores; sched_getaffinity there lists the whole machine)."""
    n = len(os.sched_getaffinity(0))
    share = os.environ.get("OMP_NUM_THREADS")
    if share and share.isdigit() and int(share) > 0:
        n = min(n, int(share))
    return max(1, n)


def cpu_baseline(G: int, seed: int, threads: int):
    """The oracle (PyTorch-CPU restatement of the reference, same op sequence,
    pinned to the reference's goldens) on the whole G^3 lattice of the
    synthetic net of this seed (N = 64 when the budget is
    short), every hyperplane step."""
    import oracle.subdivide as od
    from tropical.synthetic import slab_lattice
    torch.set_num_threads(threads)
    cfg, p = synthetic_params(G, seed)
    ref = od.load_params(od.RefNet(**cfg), p)
    V, E = slab_lattice(ref.enc.marks.numpy(), 0, G - 1)
    V, E = torch.from_numpy(V), torch.from_numpy(E)
    stats = {}
    done = [0]

    def progress(V, E, cache):
        # one stderr line per step: the GPU box ends a command that prints
        # nothing for 3 minutes (round 5's 64^3 sample was killed that way)
        done[0] += 1
        log(f"CPU baseline: step {done[0]}: {V.shape[0]} vertices, {E.shape[0]} edges, "
            f"{time.perf_counter() - t0:.1f} s")

    # and a heartbeat inside a long step (64^3: one oracle step runs for
    # minutes on the box's 16-core share)
    import threading
    stop = threading.Event()

    def heartbeat():
        while not stop.wait(30.0):
            log(f"CPU baseline: step {done[0] + 1} running, {time.perf_counter() - t0:.0f} s")

    t0 = time.perf_counter()
    hb = threading.Thread(target=heartbeat, daemon=True)
    hb.start()
    try:
        with torch.no_grad():
            od.run_steps(V, E, ref, 1e-4, None, stats, on_step=progress)
    finally:
        stop.set()
        hb.join()
    dt = time.perf_counter() - t0
    S = sum(s["S"] for s in stats["steps"])
    return S / dt, S, dt


def parallelism(part) -> str:
    if part is None:
        return "single"
    if part.dims[1] == part.dims[2] == 1:
        return f"xslab{part.world}"
    return "blocks" + "x".join(str(p) for p in part.dims)


def shard_text(part) -> str:
    if part is None:
        return "one GPU"
    if part.dims[1] == part.dims[2] == 1:
        return "x-slab per GPU"
    return "{}x{}x{} blocks, one per GPU".format(*part.dims)


def halo_stats(part, halo: int) -> dict:
    """Per-rank redundancy of the decomposition (tropical.distributed.Blocks):
    the cells a rank extracts beyond the ones it owns (its halo), as a
    fraction of the cells it extracts."""
    if part is None or part.world <= 1:
        return {}
    fr = [part.redundant_frac(r, halo) for r in range(part.world)]
    return {"redundant_cell_frac_max": round(max(fr), 4), "redundant_cell_frac_mean": round(sum(fr) / part.world, 4)}


def gpu_same_workload(G: int, seed: int, dev, reps: int = 5):
    """The engine on the CPU baseline's workload (the whole G^3 lattice of
    the same net): splits per pass and the median pass time."""
    from tropical._engine import engine_for
    net = make_net(G, dev, seed)
    eng = engine_for(net)
    eng.set_owned()
    eng.set_shards(1)
    ts, S = [], 0
    for i in range(reps + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        stats = []
        eng.lattice()
        eng.run_steps(stats)
        torch.cuda.synchronize(dev)
        if i:  # the first pass warms the engine's buffers
            ts.append(time.perf_counter() - t0)
        S = sum(s["S"] for s in stats)
    return S, float(np.median(ts))


def reference_full_workload(G: int, seed: int):
    """The reference ITSELF on the exact benchmarked workload (128^3, seed 6),
    timed once when tests/golden/make_golden.py produced the bench128 golden
    in the build container (8-core Intel Xeon, torch CPU): its splits and
    seconds.  None for other workloads."""
    from golden_io import GOLDEN
    path = os.path.join(GOLDEN, "bench128.npz")
    if G != 128 or seed != 6 or not os.path.isfile(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        return float(z["ref_seconds"])


# kernels of the PMC profile that are not part of a pass (export / stitch /
# the first pass's buffer growth), left out of the whole-pass counter total
PMC_NOT_PER_PASS = ("k_gather_vertices", "k_remap_edges", "k_scan_lb", "k_i32_to_i64", "k_widen_flags",
                    "at", "__amd_rocclr_copyBuffer", "__amd_rocclr_copyBufferRectAligned")


def pmc_pass_bytes(marks: int, seed: int):
    """Sum of the committed PMC HBM bytes (2 FETCH_SIZE + WRITE_SIZE, per
    launch x launches) over the kernels of one pass, divided by the passes
    the profiled run made (k_forward: the lattice's full forward, once per
    pass).  None without a profile of this workload."""
    if marks != 128 or seed != 6 or not os.path.isfile(PMC_TABLE):
        return None
    with open(PMC_TABLE) as f:
        ks = json.load(f)["kernels"]
    passes = ks.get("k_forward", {}).get("launches")
    if not passes:
        return None
    tot = sum(v["traffic_bytes_per_launch"] * v["launches"] for k, v in ks.items()
              if k not in PMC_NOT_PER_PASS and "traffic_bytes_per_launch" in v)
    return tot / passes


def small_net_check(dev, force: bool = True):
    """The metric's named config at bunny scale: the stand-in small net
    (levels=4, r 2..32, 49 marks; fitted to a sphere, committed fixture),
    end to end through the drop-in subpoly() on the GPU.  force=True (flat,
    configs[0]) is checked against the oracle run live on the host (splits/s
    both ways); force=False (curve-approx on, configs[1]) against the golden
    produced by the reference itself.  Chamfer-L2 of the surfaces uses the
    chamfer_distance.py:39-48 formula."""
    import io
    import contextlib
    import tropical.subpoly as sp
    from golden_io import load
    from helpers import oracle_net, product_net
    name = "small_sphere" if force else "small_sphere_curve"
    d = load(name)
    net = product_net(d, dev)
    stats = []
    with contextlib.redirect_stdout(io.StringIO()):
        sp.subpoly(net, 3, 1.2, force=force)  # warm
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        faces, verts, tri = sp.subpoly(net, 3, 1.2, force=force, stats=stats)
        torch.cuda.synchronize(dev)
        t_gpu = time.perf_counter() - t0
        out = {"config": f"stand-in bunny small net (sphere-fitted, 49 marks), "
                         f"{'flat' if force else 'curve-approx on'}, subpoly() end to end"}
        S = sum(s["S"] for s in stats)
        out.update({"edges_subdivided": int(S), "gpu_s": round(t_gpu, 4),
                    "gpu_edges_per_s": round(S / t_gpu, 1)})
        if force:
            import oracle.subdivide as od
            ref = oracle_net(d)
            st = {}
            t0 = time.perf_counter()
            with torch.no_grad():
                _, rv, rtri = od.subpoly(ref, 3, 1.2, 1e-4, True, stats=st)
            t_cpu = time.perf_counter() - t0
            rv = rv.numpy()
            out.update({"cpu_s": round(t_cpu, 3), "cpu_edges_per_s": round(S / t_cpu, 1)})
        else:
            rv, rtri = d["surf_V"], d["tri"]
    # launches of the extraction (HIP events on every engine launch, one more
    # untimed run): how launch-bound the bunny scale is
    from tropical._engine import engine_for
    eng = engine_for(net)
    eng.kernel_timer(True)
    with contextlib.redirect_stdout(io.StringIO()):
        sp.subpoly(net, 3, 1.2, force=force)
    kt = eng.kernel_timer(False)
    nl = int(sum(x["launches"] for x in kt.values()))
    kms = float(sum(x["ms"] for x in kt.values()))
    # the hyperplane loop alone (the finish -- surface, export, and since
    # round 6 the faces kernels, on the timer too -- counted apart)
    fin = ("faces_", "surface", "gather_vertices", "remap_edges", "scan", "skel")
    loop = {k: v for k, v in kt.items() if not k.startswith(fin)}
    nll = int(sum(x["launches"] for x in loop.values()))
    out.update({"active_steps": len(stats), "timed_launches": nl,
                "loop_launches_per_step": round(nll / max(len(stats), 1), 1),
                "launches_per_step": round(nl / max(len(stats), 1), 1),
                "us_per_launch": round(kms * 1e3 / max(nl, 1), 2),
                "kernel_ms_total": round(kms, 3),
                "loop_kernel_ms": round(float(sum(x["ms"] for x in loop.values())), 3)})
    v = verts.cpu().numpy()
    out["chamfer_l2_vs_ref"] = chamfer(v, rv)
    out["faces_bit_exact"] = bool(np.array_equal(np.asarray(tri), np.asarray(rtri)))
    out["max_vertex_err"] = float(np.abs(v - rv).max()) if v.shape == rv.shape else None
    return out


def large_net_check(dev):
    """BASELINE config 3's net class, Net(3,16,4,8,128,T=19): the committed
    201-mark large net (sphere-fitted, tests/golden/large_sphere.npz, made by
    running the reference), subpoly() end to end on the GPU -- multi-tile
    skeleton, every step, surface and faces -- checked against the reference's
    own output hashes.  The reference's time is the one make_golden.py
    measured running it on the 8-core build container (not this host)."""
    import io
    import contextlib
    import tropical.subpoly as sp
    from golden_io import load, sha
    from helpers import product_net
    d = load("large_sphere")
    net = product_net(d, dev)
    stats = []
    with contextlib.redirect_stdout(io.StringIO()):
        sp.subpoly(net, 3, 1.2, force=True)  # warm
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        faces, verts, fwi = sp.subpoly(net, 3, 1.2, force=True, stats=stats)
        torch.cuda.synchronize(dev)
        t_gpu = time.perf_counter() - t0
    S = sum(s["S"] for s in stats)
    ok = (sha(verts.cpu().numpy()) == str(d["sha_surf"]) and
          sha(np.asarray(fwi, dtype=np.int64)) == str(d["sha_tri"]) and
          sha(np.asarray(faces, dtype=np.float32)) == str(d["sha_faces"]))
    ref_s = float(d["ref_seconds"])
    return {"config": "large net Net(3,16,4,8,128,T=19), 201 marks, sphere-fitted stand-in, flat, "
                      "subpoly() end to end", "edges_subdivided": int(S), "gpu_s": round(t_gpu, 4),
            "gpu_edges_per_s": round(S / t_gpu, 1), "reference_cpu_s": round(ref_s, 2),
            "reference_cpu_note": "the reference itself, run once on the 8-core build container "
                                  "(tests/golden/make_golden.py)",
            "gpu_over_reference": round(ref_s / t_gpu, 1), "surface_faces_match_reference": bool(ok)}


def finish_check(dev, reps: int = 5):
    """The finish phase at scale: extract_skeleton + extract_faces
    (subpoly.py:556-728, the a14/a15 kernels) on the synth64h complex (the
    64^3 hashed lattice after all 33 steps: 703,300 surface vertices),
    timed per phase and checked against the reference's own hashes of the
    surface, triangles and float faces (tests/golden/synth64h.npz)."""
    from golden_io import load, sha
    from helpers import product_net
    from tropical._engine import engine_for
    d = load("synth64h")
    net = product_net(d, dev)
    eng = engine_for(net)
    ts = {"surface": [], "export": [], "faces": []}
    v = tri = fc = None
    for i in range(reps + 1):
        eng.lattice()
        eng.run_steps([])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.surface()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        v, _, _ = eng.export(edges=False)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        tri, fc = eng.faces()
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        if i:  # the first round grows the engine's buffers
            ts["surface"].append(t1 - t0)
            ts["export"].append(t2 - t1)
            ts["faces"].append(t3 - t2)
    # per-kernel times of one more finish (HIP events on the engine's stream)
    eng.lattice()
    eng.run_steps([])
    eng.kernel_timer(True)
    eng.surface()
    eng.export(edges=False)
    eng.faces()
    kt = eng.kernel_timer(False)
    med = {k: float(np.median(x)) for k, x in ts.items()}
    nv, nt = int(v.shape[0]), int(tri.shape[0])
    ok = (sha(v.cpu().numpy()) == str(d["sha_surf"]) and sha(tri.cpu().numpy()) == str(d["sha_tri"]) and
          sha(fc.cpu().numpy()) == str(d["sha_faces"]))
    tot = sum(med.values())
    return {"config": "synth64h: 64^3 hashed synthetic lattice after all 33 steps (reference golden), "
                      "extract_skeleton + extract_faces on the device",
            "surface_vertices": nv, "triangles": nt, "ms": {k: round(x * 1e3, 3) for k, x in med.items()},
            "ms_total": round(tot * 1e3, 3), "ns_per_surface_vertex": round(tot * 1e9 / max(nv, 1), 2),
            "triangles_per_s": round(nt / max(med["faces"], 1e-12), 1),
            "kernel_ms": {k: round(x["ms"], 3) for k, x in sorted(kt.items(), key=lambda kv: -kv[1]["ms"])},
            "launches": int(sum(x["launches"] for x in kt.values())),
            "matches_reference": bool(ok)}


def design_independent_rates(ktime: dict, stats: list) -> dict:
    """Per-unit kernel times that do not depend on this build's byte model
    (VERDICT r03 weak #8): ns per (cell, member) entry and per member pair
    tested for the grouping kernel, per split for the new-vertex forward, per
    edge slot for the pruning, over one pass."""
    T = sum(s.get("T", 0) for s in stats)
    tests = sum(s.get("pair_tests", 0) for s in stats)
    S = sum(s["S"] for s in stats)
    slots = sum(s["E_in"] + 2 * s["S"] + s["X"] for s in stats)
    out = {"entries_per_pass": int(T), "pair_tests_per_pass": int(tests)}

    def rate(k, n):
        return None if k not in ktime or not n else round(ktime[k]["ms"] * 1e6 / n, 4)
    grp = ktime.get("bucket_group", {}).get("ms", 0.0) + ktime.get("bucket_refine", {}).get("ms", 0.0)
    out["bucket_group_ns_per_entry"] = round(grp * 1e6 / T, 4) if T else None
    out["bucket_group_ns_per_pair_test"] = round(grp * 1e6 / tests, 4) if tests else None
    out["bucket_entries_ns_per_entry"] = rate("bucket_entries", T)
    out["forward_new_ns_per_split"] = rate("forward_new", S)
    out["prune_ns_per_edge"] = rate("prune", slots)
    return out


DUMP_ROWS = 1 << 20   # rows kept of a larger output array
DUMP_SEED = 20240607  # of the row sample (fixed: two builds keep the same rows)


def sample_rows(n: int, stream: int):
    """Sorted row numbers of the fixed sample of an n-row array (None: the
    array is kept whole)."""
    if n <= DUMP_ROWS:
        return None
    rng = np.random.Generator(np.random.PCG64([DUMP_SEED, stream]))
    return np.sort(rng.choice(n, DUMP_ROWS, replace=False))


def dump_outputs(path: str, eng, stats: list, suffix: str = "") -> None:
    """What the last timed pass left to its caller, as path/<name>.npy: the
    compacted complex (Engine.export: vertices float32, edges as float64
    vertex numbers; of more than DUMP_ROWS rows a fixed seeded sample, the row
    numbers next to it), its sizes and order-free set hashes (each 64-bit
    hash as two 32-bit halves, exact in float64), and the pass's per-step
    counters.  At most 2^20 * (12 + 16 + 8 + 8) bytes = 46 MB."""
    from tropical._hip import TnpStepStats
    from tropical.distributed import complex_hash
    os.makedirs(path, exist_ok=True)
    V, E, _ = eng.export()
    hv, he = complex_hash(V, E)

    def save(name, a):
        np.save(os.path.join(path, f"{name}{suffix}.npy"), np.ascontiguousarray(a))

    for k, (name, t, dt) in enumerate((("vertices", V, np.float32), ("edges", E, np.float64))):
        rows = sample_rows(int(t.shape[0]), k)
        if rows is not None:
            t = t[torch.from_numpy(rows).to(t.device)]
            save(name + "_rows", rows.astype(np.float64))
        save(name, t.cpu().numpy().astype(dt))
    halves = [float(x) for h in (hv, he) for x in ((h >> 32) & 0xFFFFFFFF, h & 0xFFFFFFFF)]
    save("complex", np.array([V.shape[0], E.shape[0]] + halves, dtype=np.float64))
    # the 64-bit plane mask is not a count (and not exact in float64)
    cols = [k for k, _ in TnpStepStats._fields_ if k != "next_active"]
    save("step_stats", np.array([[s[k] for k in cols] for s in stats], dtype=np.float64).reshape(len(stats), len(cols)))


def chamfer(a: np.ndarray, b: np.ndarray) -> float:
    """chamfer_distance.py:39-48 formula (mean NN L2 both ways / 2)."""
    if len(a) == 0 or len(b) == 0:
        return 0.0 if len(a) == len(b) else float("inf")
    from scipy.spatial import cKDTree
    d1, _ = cKDTree(b).query(a)
    d2, _ = cKDTree(a).query(b)
    return float((d1.mean() + d2.mean()) / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--marks", type=int, default=128, help="marks per axis per GPU (weak scaling)")
    # seed 6: the first seed in 0..23 whose 128^3 run is non-degenerate (connecting
    # edges <= 5x splits per step) with a large final complex; seeds 0, 8, 11,
    # 12 contain regions of 1e5-1e7 vertices (seed 8: 5.5e13 in-region pairs)
    # that the reference's CPU path could not materialise (tools/seed_scan.py)
    ap.add_argument("--seed", type=int, default=6)
    # the CPU baseline's sample: the whole 48^3 lattice of the same net and
    # seed (7.9 s on the GPU box's 16-core share).  BASELINE.md §3's budget
    # fallback, 64^3, ran past three minutes there in round 5 (killed by the
    # box's 180-s silence limit: its larger regions grow the oracle's
    # pair materialisation faster than the lattice); 128 is the benchmarked
    # workload itself, ~18 min of the reference's CPU path
    ap.add_argument("--cpu-marks", type=int, default=int(os.environ.get("TNP_CPU_MARKS", 48)))
    ap.add_argument("--no-cpu", action="store_true", help="with --full: without the CPU baseline and the legs")
    ap.add_argument("--full", action="store_true",
                    help="also the per-kernel pass and roofline, the check of the final complex against the "
                         "reference, the CPU baseline and the bunny-scale / large-net / finish legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed pass computed as DIR/<name>.npy")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU: relaunch under torch.distributed.run as a CHILD
        # process (nothing here has touched the GPU yet) and exit with its code
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
               f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # one rank per GPU; TNP_DIST_BACKEND=gloo rehearses N ranks on fewer GPUs
    # (collectives then run on host copies)
    backend = os.environ.get("TNP_DIST_BACKEND", "nccl")
    local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    comm_dev = dev if backend == "nccl" else torch.device("cpu")
    coll = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        coll = Collective(comm_dev)

    from tropical._engine import engine_for
    G = args.marks if world == 1 else int(round(args.marks * world ** (1.0 / 3.0)))
    net = make_net(G, dev, args.seed)
    from tropical.distributed import HALOS, Blocks, block_dims, halo_check, slab_cuts
    # N > 1: one block of the lattice per rank from N = 4 (2 x 2 x 1, 2 x 2 x 2:
    # the smallest cut faces, so the fewest redundant halo cells); N = 2 is
    # one cut either way (x-slabs).  TNP_SHARD=blocks|xslab forces either.
    part = None
    if world > 1:
        dims = block_dims(world)
        shard = os.environ.get("TNP_SHARD", "blocks" if world >= 4 else "xslab")
        if shard not in ("blocks", "xslab"):
            raise SystemExit(f"TNP_SHARD={shard!r}: 'blocks' or 'xslab'")
        part = Blocks.xslabs(slab_cuts(G, world)) if shard == "xslab" else Blocks(G, dims)
    eng = engine_for(net)
    if world > 1:
        eng.set_owned_box(*part.owned(rank))  # halo splits -> S_dup
    eng.set_shards(world)
    box = [[0, 0, 0], [G - 1, G - 1, G - 1]]

    def one_pass():
        stats = []
        eng.lattice_box(*box)
        eng.run_steps(stats, coll)
        return stats

    halo = 0
    search = {"halo_search_passes": 0, "halo_search_ms": 0.0}
    if world > 1:
        # this rank's cells + a halo beyond every cut face, as wide as
        # halo_check needs (untimed: one pass per width tried, reported)
        t_s = time.perf_counter()
        for k, halo in enumerate(HALOS):
            box[:] = part.box(rank, halo)
            one_pass()
            search["halo_search_passes"] += 1
            Vl, El, _ = eng.export()
            ok = halo_check(Vl.to(comm_dev), El.to(comm_dev), net.enc.marks, part,
                            raise_=k == len(HALOS) - 1)
            if ok is not None:
                break
        search["halo_search_ms"] = round((time.perf_counter() - t_s) * 1e3, 1)

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    if os.environ.get("TNP_BENCH_MEM"):
        fr, tot = torch.cuda.mem_get_info(dev)
        log(f"rank {rank}: halo {halo}, box {box}, device memory {(tot - fr) / 2**30:.1f} of {tot / 2**30:.0f} GiB in use")
    log(f"rank {rank}: {G}^3 lattice, {args.warmup} warmup + {args.steps} timed passes")
    for _ in range(args.warmup):
        one_pass()
    barrier()
    if os.environ.get("TNP_BENCH_MEM"):
        fr, tot = torch.cuda.mem_get_info(dev)
        log(f"rank {rank}: after warmup, device memory {(tot - fr) / 2**30:.1f} GiB in use")
    t0 = time.perf_counter()
    all_stats = []
    for _ in range(args.steps):
        all_stats.append(one_pass())
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and args.steps > 0:
        # the engine still holds the last timed pass's complex
        dump_outputs(args.dump_outputs, eng, all_stats[-1], f"_rank{rank}" if world > 1 else "")
        barrier()
    ktime = {}
    if args.full:
        # one more pass with a HIP-event pair around every engine launch (kept out
        # of the timed region: the event records cost host time per launch)
        eng.kernel_timer(True)
        one_pass()
        ktime = eng.kernel_timer(False)
        barrier()

    from tropical.distributed import complex_hash
    stitched = None
    if args.full and world == 1:
        Vf, Ef, _ = eng.export()
        hv, he = complex_hash(Vf, Ef)
        stitched = {"vertices": int(Vf.shape[0]), "edges": int(Ef.shape[0]),
                    "vertex_set_hash": hv, "edge_set_hash": he}
        ref = reference_fingerprint(G, args.seed)
        if ref is not None:
            # parity of the measured workload: the reference itself, run on the
            # same net and lattice (tests/golden/make_golden.py bench128)
            got = (stitched["vertices"], stitched["edges"], hv, he)
            if got != ref:
                raise SystemExit(f"final complex {got} differs from the reference's {ref}")
            stitched["matches_reference"] = True
    elif args.full:
        # the complete sharded output: each slab exported, the neighbours'
        # views next to every cut compared (fails loudly if a halo was too
        # narrow), stitched into one global complex (tropical/distributed.py;
        # RCCL all_gathers), untimed
        from tropical.distributed import stitch
        Vl, El, _ = eng.export()
        halo_check(Vl.to(comm_dev), El.to(comm_dev), net.enc.marks, part)
        owned, first, gE, own, keep = stitch(Vl.to(comm_dev), El.to(comm_dev), net.enc.marks, part,
                                             masks=True)
        hv, he = complex_hash(Vl.to(comm_dev), El.to(comm_dev), own, keep)
        tot = torch.tensor([owned.shape[0], gE.shape[0], hv, he], device=comm_dev, dtype=torch.int64)
        torch.distributed.all_reduce(tot)  # int64 sums wrap like the 1-rank sums
        stitched = {"vertices": int(tot[0]), "edges": int(tot[1]),
                    "vertex_set_hash": int(tot[2]), "edge_set_hash": int(tot[3])}
        barrier()

    splits = sum(s["S"] - s["S_dup"] for st in all_stats for s in st)
    bytes_alg = sum(algorithmic_bytes(s, net.K) for st in all_stats for s in st)
    vec = torch.tensor([dt, float(splits), float(bytes_alg)], device=comm_dev, dtype=torch.float64)
    if world > 1:
        mx = vec.clone()
        torch.distributed.all_reduce(mx[:1], op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(vec[1:], op=torch.distributed.ReduceOp.SUM)
        vec[0] = mx[0]
    dt_max, splits_tot, bytes_tot = vec.tolist()

    if rank == 0:
        per_pass = splits_tot / args.steps
        value = splits_tot / dt_max
        st0 = all_stats[0]
        # dominant kernel: HIP events around each launch inside the engine,
        # among the hand-written HIP kernels (the *_sort entries are rocPRIM
        # radix sorts: several library launches each, no single rocprof row)
        own = {k: v for k, v in ktime.items() if not k.endswith("_sort")}
        dom = max(own, key=lambda k: own[k]["ms"]) if own else None
        dom_all = max(ktime, key=lambda k: ktime[k]["ms"]) if ktime else None
        roof = None
        loop_gbs = bytes_tot / dt_max / 1e9
        if dom:
            kt = ktime[dom]
            avg_ms = kt["ms"] / max(kt["launches"], 1)
            alg = kt["bytes"] / max(kt["launches"], 1)  # algorithmic bytes per launch
            ach = alg / (avg_ms * 1e-3) / 1e9
            traffic = pmc_traffic(dom, G, args.seed) if world == 1 else None
            roof = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic,
                    "traffic_gbs": None if traffic is None else round(traffic / (avg_ms * 1e-3) / 1e9, 1),
                    "avg_launch_us": round(avg_ms * 1e3, 2), "launches": kt["launches"],
                    "alg_bytes_per_launch": int(alg), "dominant_overall": dom_all,
                    # what else bounds it, from the same PMC passes: VALU issue
                    # (wave64 VALU instructions x 4 cycles over every SIMD) and
                    # the L2 hit rate
                    "valu_util": None, "l2_hit": None,
                    # the whole hyperplane loop against the same peak: SURVEY
                    # §8d's per-step model (bench.algorithmic_bytes) / pass time
                    "whole_loop_gbs": round(loop_gbs, 1),
                    "whole_loop_frac": round(loop_gbs / (HBM_PEAK_GBS * world), 4),
                    # the same pass against the counters: sum of the PMC HBM
                    # bytes of every kernel of one pass / pass time / peak
                    # (MALL hits included: an upper bound on HBM traffic)
                    "counter_bytes_per_pass": None, "counter_frac": None}
            pb = pmc_pass_bytes(G, args.seed) if world == 1 else None
            if pb is not None:
                roof["counter_bytes_per_pass"] = int(pb)
                roof["counter_frac"] = round(pb / (dt_max / args.steps) / 1e9 / HBM_PEAK_GBS, 4)
        if roof and world == 1:
            row = pmc_row(dom, G, args.seed)
            if row and "SQ_INSTS_VALU" in row:
                roof["valu_util"] = round(row["SQ_INSTS_VALU"] * 4 / (roof["avg_launch_us"] * 1e-6 * CLOCK_HZ * SIMDS), 3)
            if row and "TCC_HIT_sum" in row:
                roof["l2_hit"] = round(row["TCC_HIT_sum"] / max(row["TCC_HIT_sum"] + row["TCC_MISS_sum"], 1), 3)
        if roof:
            # what actually limits the kernel, from the counters: HBM is the
            # roof it is priced against ("bound"); below ~half of it with the
            # fabric traffic also well under peak, the kernel is issue/latency
            # bound (VALU share of the SIMD cycles, gathers waiting on L2/MALL)
            tg = roof["traffic_gbs"]
            if roof["frac"] >= 0.5 or (tg is not None and tg >= 0.5 * HBM_PEAK_GBS):
                roof["limiter"] = "hbm"
            elif roof["valu_util"] is not None:
                roof["limiter"] = (f"issue/latency: VALU busy {roof['valu_util']:.0%} of SIMD cycles, "
                                   f"L2 hit {roof['l2_hit']:.0%}, fabric traffic "
                                   f"{(tg or 0) / HBM_PEAK_GBS:.0%} of HBM peak")
            else:
                roof["limiter"] = "issue/latency (no PMC pass for this kernel)"
        out = {
            "metric": "edges subdivided/sec", "value": round(value, 1), "unit": "edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt_max / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"synthetic random-weight trilinear net, {G}^3 initial lattice "
                                   f"({shard_text(part)}), flat path, all "
                                   f"{net.K} hyperplane steps", "marks_per_axis": G,
                       "lattice_vertices": G ** 3, "edges_subdivided_per_pass": int(per_pass),
                       "seed": args.seed, "table_amp": 0.1, "parallelism": parallelism(part),
                       "halo_cells": halo, **halo_stats(part, halo), **search},
            "roofline": roof,
            "loop_model_bytes_per_pass": int(bytes_tot / args.steps),
            "loop_model_gbs": round(loop_gbs, 1),
            "kernel_ms_per_pass": {k: round(v["ms"], 3) for k, v in
                                   sorted(ktime.items(), key=lambda kv: -kv[1]["ms"])},
            "active_steps": len(st0),
            # ns per entry / pair test / split / edge, independent of the byte model
            "unit_rates": design_independent_rates(ktime, st0),
        }
        if not args.full:
            # a plain run made no HIP-event pass: nothing per kernel to report
            for k in ("roofline", "kernel_ms_per_pass", "unit_rates"):
                del out[k]
        if stitched:
            out["final_complex" if world == 1 else "stitched_complex"] = stitched
        if args.full and not args.no_cpu and world == 1:
            thr = cpu_threads()
            Gc = args.cpu_marks
            log(f"CPU baseline: the oracle on the {Gc}^3 lattice, {thr} threads")
            cps, S_cpu, t_cpu = cpu_baseline(Gc, args.seed, thr)
            log(f"CPU baseline: {S_cpu} splits in {t_cpu:.1f} s")
            S_g, t_g = gpu_same_workload(Gc, args.seed, dev)
            if S_g != S_cpu:
                raise SystemExit(f"CPU baseline workload: {S_cpu} splits on the host, {S_g} on the GPU")
            out["cpu_baseline"] = {
                "value": round(cps, 1), "unit": "edges/s", "cores": thr, "kind": "port",
                "cpu": cpu_model(),
                "threads_rule": "usable cores (sched_getaffinity), capped by the job's CPU share "
                                "(OMP_NUM_THREADS)",
                "sample": f"oracle (PyTorch-CPU restatement of the reference, pinned to its goldens) on the "
                          f"whole {Gc}^3 lattice of the seed-{args.seed} synthetic net, all hyperplane "
                          f"steps (BASELINE.md §3): {S_cpu} splits in {t_cpu:.1f}s",
                # the GPU on the SAME workload, so the ratio compares equal work
                "gpu_same_sample": {"edges_subdivided": int(S_g), "seconds": round(t_g, 5),
                                    "edges_per_s": round(S_g / t_g, 1)},
                "gpu_over_cpu_same_sample": round((S_g / t_g) / cps, 1)}
            ref_s = reference_full_workload(G, args.seed)
            if ref_s is not None:
                # the reference itself on the benchmarked workload (all of it)
                out["cpu_baseline"]["reference_full_workload"] = {
                    "value": round(per_pass / ref_s, 1), "unit": "edges/s", "kind": "reference",
                    "seconds": round(ref_s, 1), "edges_subdivided": int(per_pass), "cores": 8,
                    "cpu": "8-core Intel Xeon (the build container, not this host)",
                    "sample": f"the reference's subpoly_ loop on the full {G}^3 seed-{args.seed} lattice, "
                              "timed by tests/golden/make_golden.py when it produced the bench128 golden",
                    "gpu_over_reference": round(value / (per_pass / ref_s), 1)}
            engine_for(net)  # restore
        if args.full and not args.no_cpu and world == 1:
            log("bunny-scale and large-net legs")
            out["small_net"] = small_net_check(dev, force=True)
            out["small_net_curve"] = small_net_check(dev, force=False)
            out["large_net"] = large_net_check(dev)
            log("finish phase at scale (synth64h)")
            out["finish_synth64h"] = finish_check(dev)
            engine_for(net)  # restore
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
