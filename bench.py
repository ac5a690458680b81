#!/usr/bin/env python3
"""bench.py -- pairs/sec of the GFNet post-backbone hot path on MI355X (BASELINE.json metric).

One "step" = one batch of synthetic image pairs through the whole path on feature pyramids that are
already resident in HBM:
  global correlation + soft-argmax (scale 16) -> per scale and refiner iteration: refiner input (grid
  features, x_hat, displacement embedding, local correlation into the concat buffer) + flow update +
  inter-scale resize, for the first pass and the 1.25x refinement pass (test.py defaults: symmetric,
  upsample_preds, attenuate_cert) -> match post-processing -> balanced sampling (2 draws without
  replacement + KDE, N=M=20000) -> device RANSAC/DLT/LM homography solve -> (N>1) RCCL all-gather of H.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload 448b32|672b16|pyr-fp16] [--conv-stack off|fp32|fp16|amp]
                    [--dump-outputs DIR]

`--gpus N` with N > 1 works both ways: under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` (the ranks
are already there: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment) and as the bare command `python bench.py
--gpus N`: a parent that never touches the GPU starts N fresh rank processes, relays rank 0's JSON line and exits with the
worst return code of its children (the reference only ever starts ranks through torchrun, scripts/train_script.sh:1).

Workloads (BASELINE.json configs):
  448b32   (default, configs[1]) 448x448, 32 pairs per GPU, basic.json (num_itr 1), fp32 features
  672b16   (configs[2]) googlemap 672x672, 16 pairs per GPU, map.json (num_itr 2 per scale), grids by the rule of
           network.py:329 ([S/14, S/14, 2S/14, 4S/14, 8S/14] = 48/48/96/192/384, refinement pass at 840)
  pyr-fp16 (configs[4]) feature pyramids stored in fp16 at the 224 / 448 / 672 test-set sizes, 8 pairs each per step
The refiners' conv stacks are a stand-in by default (`config.excluded`); `--conv-stack fp32|fp16|amp`
runs the reference's architecture on the HIP conv-stack kernels inside the timed region (fp32: fp32 throughout; fp16: fp16
operands of the 1x1 convs; amp: fp16 operands and fp16 maps between the blocks -- the class the reference's amp=True refiners
run in, model/network.py:560-562).  A default single-GPU run also reports that last figure as `with_conv_stacks` next to
`value` (secondary measurement after the timed region; --no-stack-leg skips it).

Prints ONE JSON line on rank 0 (driver contract).  `roofline` is for the dominant kernel of the named config, the scale-4
local-correlation call of the first pass (c32, r=4), timed with HIP events on its launch stream inside the timed steps;
`cpu_baseline` is the C/OpenMP oracle (a port of the reference's algorithm, pinned on reference-generated goldens) on a
bounded sample of the same workload: 1 warm-up + median of 3, rank 0, N=1 only.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8 TB/s spec
HBM_ACHIEVABLE_GBS = 6290.0  # same guide: float4 copy, 79 % of spec


def algorithmic_bytes_local_corr(B, c, hs, G, r, feat_bytes=4):
    """f0 + f1 + flow + out: 3 489 792 B per pair-direction at scale 4 of the 448 pass in fp32.
    f0 is the grid_feature slice of the concat buffer (always fp32 there); f1 is stored in `feat_bytes`."""
    return B * (4 * c * G * G + feat_bytes * c * hs * hs + 8 * G * G + 4 * (2 * r + 1) ** 2 * G * G)


def cpu_baseline(scenes, n_pairs):
    """1 warm-up + median of 3 passes of `n_pairs` pairs of every scene through oracle/ (host cores)."""
    import numpy as np
    import oracle
    from oracle.scene import cpu_pair

    to_np = lambda p: {s: t[:n_pairs].float().cpu().numpy() for s, t in p.items()}  # noqa: E731
    prepared = []
    for sc in scenes:
        np_gt = {G: t.cpu().numpy() for G, t in sc.gt.items()}
        np_noise = {G: [n.numpy() for n in ns] for G, ns in sc.noise.items()}
        prepared.append((sc, (to_np(sc.pyr[0]), to_np(sc.pyr[1])), (to_np(sc.pyr_up[0]), to_np(sc.pyr_up[1])), np_gt, np_noise))
    times = []
    for rep in range(4):
        t0 = time.time()
        for sc, npyr, nup, ngt, nnoise in prepared:
            for b in range(n_pairs):
                cpu_pair(sc, b, npyr, nup, ngt, nnoise, seed=b)
        times.append(time.time() - t0)
    dt = float(np.median(times[1:]))
    return n_pairs * len(scenes) / dt, oracle.max_threads()


def solve_parity(scene, good, Hl, n):
    """Corner error (px) between the device H and the oracle H on identical (device-sampled) matches, and of the device H
    against the ground-truth H."""
    import numpy as np
    import oracle

    pts = oracle.convert_matches(good[:n].cpu().numpy(), *scene.sizes)
    Ho, _, _ = oracle.homography_ransac(pts, thresh=3.0, iters=2000, seed=0)
    Hd = Hl[:n].cpu().numpy()
    S = scene.size
    vs_oracle = [oracle.corner_error(Ho[i], Hd[i], S, S, clamp=1e9) for i in range(n)]
    vs_truth = [oracle.corner_error(scene.H[i], Hd[i], S, S, clamp=1e9) for i in range(n)]
    return float(np.mean(vs_oracle)), float(np.mean(vs_truth))


class stdout_to_stderr:
    """File descriptor 1 points at stderr inside the block: RCCL prints a version banner on stdout when its first communicator
    comes up, and the driver wants exactly ONE line there, the JSON."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def timed_loop(fn, n, sync):
    """n calls of fn between two sync()s, without collector pauses (one GC policy for every timed leg)."""
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for i in range(n):
            r = fn(i)
        sync()
        return time.perf_counter() - t0, r
    finally:
        gc.enable()


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=("448b32", "672b16", "pyr-fp16"), default="448b32")
    ap.add_argument("--pairs-per-gpu", type=int, default=0, help="override the workload's pairs per GPU (per size)")
    ap.add_argument("--cpu-pairs", type=int, default=-1, help="pairs per size for the CPU-oracle baseline leg (0 = skip; default: per workload)")
    ap.add_argument("--breakdown", action="store_true", help="print per-stage GPU times of one step to stderr")
    ap.add_argument("--no-stack-leg", action="store_true",
                    help="skip the secondary measurement `with_conv_stacks` (default single-GPU runs with --conv-stack off also time the same "
                         "step with the refiners' conv stacks in the reference's autocast class)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="skip the secondary legs `other_workloads` (default single-GPU 448b32 runs also time a few steps of 672b16 and pyr-fp16)")
    ap.add_argument("--conv-stack", choices=("off", "fp32", "fp16", "amp"), default="off",
                    help="also run the refiners' conv stacks (reference architecture, random-init) on the HIP conv-stack kernels, with "
                         "fp32 or fp16 1x1-conv operands; default off = the north-star hot path only")
    ap.add_argument("--flows", choices=("true", "noisy", "random"), default="true",
                    help="what the stand-in refiners return: true = the true warp + 0.5-px noise (default, the metric's workload); noisy = 4 / 4 / "
                         "2 / 1 / 0.5 image pixels of noise at scales 16 / 8 / 4 / 2 / 1; random = uniform flows out of the scale-8 refiner (the "
                         "scale-4 local correlation's windows scattered: second-launch / gather path).  The default single-GPU line also runs a few "
                         "steps of the two stress modes (`stress_flows`; --no-stress-legs skips them)")
    ap.add_argument("--no-stress-legs", action="store_true", help="skip the `stress_flows` legs of the default line")
    ap.add_argument("--graphs", action="store_true",
                    help="also time the secondary workloads as hipGraph replays IN THIS PROCESS (off by default since round 5, ADVICE r4: a graph "
                         "replay that faults -- DESIGN section 8 -- would take the headline line down with it; the eager legs always run)")
    ap.add_argument("--pipeline", dest="pipeline", action="store_true", help="force the multi-stream arrangement (see --no-pipeline)")
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false",
                    help="one stream per scene inside the timed region (default for one-scene workloads: the stages of a step on streams of "
                         "their own -- see --stages --, a step's later stages beside the next steps' earlier ones, the way a stream of "
                         "batches goes through the path; the roofline op is timed in separate, un-overlapped steps either way, and the "
                         "default line reports the one-stream rate as `unpipelined_steps`)")
    ap.add_argument("--stages", type=int, choices=(2, 3), default=3,
                    help="stages of the pipelined steps of a one-scene workload: 3 = first pass | refinement pass + post-processing | "
                         "sampling + solve on three streams (default), 2 = match | sampling + solve")
    ap.set_defaults(pipeline=None)  # None: the staged arrangement for one-scene workloads, one stream per scene for the three-scene pyramid workload
                                    # (six streams slow it down: 6.8 k -> 5.5 k pairs/s, round 3)
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL)")
    ap.add_argument("--force-launcher", action="store_true",
                    help="take the self-launch path (parent starts the rank processes, relays rank 0's line) also for --gpus 1: the "
                         "single child then runs inside a torch.distributed world of one, so barrier and time reduction go through RCCL")
    ap.add_argument("--dry-run", action="store_true",
                    help="no kernels: every rank contributes made-up 3x3 matrices, so that rank start-up, the H all-gather and the JSON relay "
                         "can be exercised without a GPU (tests/test_parallel_cpu.py, with --backend gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0: the gathered homographies and its own "
                         "sampled matches per image size) as DIR/<name>.npy, at most 64 MB in all, for output-by-output comparison of two builds")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


SAMPLER_SEED = 0        # torch's CPU generator, reset before every timed loop: the sampler draws its seeds from it (ops.sample_without_replacement)
DUMP_BYTES = 64 << 20   # --dump-outputs budget


def dump_outputs(path, arrays):
    """{name: array} -> path/<name>.npy in float32 (float64 stays float64), at most DUMP_BYTES in all: smallest first, every array
    gets an equal share of what is left; one larger than its share keeps a fixed, seeded sample of its rows (first axis), the same
    rows from run to run, in their original order."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    items = sorted(((k, np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)) for k, a in arrays.items()),
                   key=lambda kv: kv[1].nbytes)
    budget = DUMP_BYTES
    for i, (name, a) in enumerate(items):
        share = budget // (len(items) - i)
        if a.nbytes > share and a.shape[0] > 1:
            keep = max(1, share * a.shape[0] // a.nbytes)
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        budget -= a.nbytes
        np.save(os.path.join(path, name + ".npy"), a)


def self_launch(args):
    """`python bench.py --gpus N` typed as is (WORLD_SIZE unset): start the N ranks as fresh child processes -- nothing in this
    parent has initialised a GPU (torch is not even imported yet), nothing is exec'ed -- relay rank 0's JSON line, return the
    worst child return code."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GFN_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True if r == 0 else None))
    # Poll every child: if a rank dies at start-up (bad device, out of memory) the others would sit in the rendezvous or in the
    # first barrier until the process-group timeout; on the first non-zero exit the siblings are terminated and that code returned.
    import threading

    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    failed = 0
    while True:
        rcs = [p.poll() for p in procs]
        bad = [rc for rc in rcs if rc not in (None, 0)]
        if bad:
            failed = abs(bad[0])
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            break
        if all(rc == 0 for rc in rcs):
            break
        time.sleep(0.05)
    reader.join(timeout=10)
    out = chunks[0] if chunks else ""
    rcs = [p.returncode for p in procs]
    for line in out.splitlines():  # the JSON line on stdout, anything else a library wrote there on stderr
        print(line, file=sys.stdout if line.startswith("{") else sys.stderr)
    sys.stdout.flush()
    return failed or max((abs(rc) for rc in rcs if rc is not None), default=0)


def dry_run(args):
    """Launch + gather + JSON without kernels (CPU, gloo): every rank makes 4 fake H matrices tagged with its rank."""
    import torch
    import torch.distributed as dist

    from gfnet_amd import parallel

    # test hook (tests/test_parallel_cpu.py): the named rank dies before the rendezvous, as a rank with a bad device would
    if os.environ.get("GFN_BENCH_TEST_EXIT_RANK") == os.environ.get("RANK", "0"):
        sys.exit(3)
    rank, world, _ = parallel.init_from_env(backend=args.backend)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    Hl = torch.eye(3, dtype=torch.float64).repeat(4, 1, 1) * (rank + 1)
    t0 = time.perf_counter()
    Hall = parallel.gather_homographies(Hl)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    ok = bool(Hall.shape[0] == 4 * world and all(float(Hall[4 * r, 0, 0]) == r + 1 for r in range(world)))
    if rank == 0:
        print(json.dumps({"metric": "dry run (no kernels)", "value": 0.0, "unit": "pairs/s", "n_gpus": world, "steps": 0, "warmup": 0,
                          "ms_per_step": round(dt * 1e3, 3), "n_ranks_seen": dist.get_world_size() if world > 1 else 1,
                          "gather_ok": ok, "backend": args.backend if world > 1 else None, "data": "none"}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


class SceneRunner:
    """One step of every scene.
    * Scenes are independent (different image sizes of the pyramid workload): each runs on HIP streams of its own, so that the
      small scene's 16-64-workgroup launches overlap the large scene's wide ones (scratch is keyed by stream, gfnet_amd/_lib.py).
    * Inside a scene the batch goes through two stages on two streams: `match` (both passes of the coarse-to-fine loop: chip-wide
      launches) and `finish` (sampling + solve: a third of its time is one-workgroup-per-pair kernels -- curve sort, radix select,
      LM finish -- on 32 of 256 CUs).  A step's finish waits for its own match only, so it runs under the NEXT step's match: the
      way a stream of batches goes through the path in deployment (448b32: 3.53 -> 3.19 ms per step; --stages 2).  The roofline
      op is timed in separate one-stream steps (the overlapped kernels take CUs from it: 96.5 -> 107 us), and the three-scene
      workload keeps one stream per scene (four hardware queues; six streams slow it down).
    * Round 4, one-scene workloads: THREE stages on three streams -- first pass | refinement pass + post-processing | sampling + solve
      (GFNet.match_first_pass / match_second_pass): step k + 1's first pass runs beside step k's refinement pass, and every kernel
      still sees the whole batch.  The heavy kernels fill a CU's register file, so the overlap is workgroup by workgroup -- a
      memory-bound refiner_input launch of one stage fills in beside an instruction-bound local correlation of the other:
      10.56 k -> 11.32 k pairs/s (448b32).  stages=2 keeps the round-4 two-stage form (--stages 2)."""

    def __init__(self, scenes, pipeline=False, stages=3):
        import torch

        from gfnet_amd import parallel

        self.scenes = scenes
        self.pipeline = pipeline
        main = torch.cuda.current_stream()
        self.streams = []
        # streams TESTED to run side by side (the runtime deals streams onto 4 hardware queues, not one to one: parallel.py); the
        # same ones for every runner of the process
        self.stages3 = pipeline and len(scenes) == 1 and stages == 3
        pool = parallel.concurrent_streams(3 if self.stages3 else 2 * len(scenes) if pipeline else (len(scenes) if len(scenes) > 1 else 0))
        for k in range(len(scenes)):
            pair = (pool[2 * k], pool[2 * k + 1]) if pipeline else ((pool[k],) * 2 if len(scenes) > 1 else None)
            if self.stages3:
                pair = (pool[0], pool[2], pool[1])  # first pass, sampling + solve, refinement pass
            if pair is not None:
                for st in set(pair):
                    st.wait_stream(main)  # the scenes' inputs were produced on the current stream
            self.streams.append(pair)

    def step(self, seed):
        import torch

        main = torch.cuda.current_stream()
        outs = []
        for sc, pair in zip(self.scenes, self.streams):
            if pair is None:
                outs.append(sc.step(seed))
                continue
            if self.stages3:
                m1, fs, ms = pair
                with torch.cuda.stream(m1):
                    corresps = sc.match_first()
                    done1 = m1.record_event()
                with torch.cuda.stream(ms):
                    ms.wait_event(done1)
                    for per_itr in corresps.values():
                        for c in per_itr.values():
                            c["flow"].record_stream(ms)
                            c["certainty"].record_stream(ms)
                    warp, cert = sc.match_second(corresps)
                    done = ms.record_event()
            else:
                ms, fs = pair
                with torch.cuda.stream(ms):
                    warp, cert = sc.match()
                    done = ms.record_event()
            with torch.cuda.stream(fs):
                fs.wait_event(done)
                warp.record_stream(fs)
                cert.record_stream(fs)
                outs.append(sc.finish(warp, cert, seed))
        for o, pair in zip(outs, self.streams):
            if pair is not None:
                main.wait_stream(pair[1])  # (the sampling + solve stream in every arrangement)
                for t in o:
                    t.record_stream(main)
        return outs


def secondary_workload(key, conv_stack, dev, rank, steps, use_graphs=True):
    """A few steps of another BASELINE configuration after the timed region of the default line (configs[2] and
    configs[4] were builder-run only): whole-step rate and the roofline fraction of its own scale-4 local-correlation call."""
    import numpy as np
    import torch

    from gfnet_amd import ops, parallel
    from gfnet_amd._synthetic import WORKLOADS, Scene, side_of

    wl = WORKLOADS[key]
    dtype = torch.float16 if wl["dtype"] == "fp16" else torch.float32
    with torch.inference_mode(False):
        scenes = [Scene(S, wl["pairs"], wl["num_itr"], dtype, conv_stack, dev, rank) for S in wl["sizes"]]
    main_scene = scenes[min(1, len(scenes) - 1)]
    # eager steps: a one-scene workload in three stages on three streams (as its own run does by default), the three-scene workload
    # on one stream per scene
    runner = SceneRunner(scenes, pipeline=len(scenes) == 1)
    graphs, graph_note = False, None
    with torch.inference_mode():
        for i in range(4):  # (the three-scene workload needs more than two steps to settle: allocator, stream pools)
            runner.step(i)
        torch.cuda.synchronize()
        ops.kernel_events = {main_scene.roofline_key: []}
        # the three-scene workload is bound by the host's launch rate: no collector pauses inside the timed steps (the process holds
        # the main workload's scenes and tensors by now, a generation-2 pass walks all of them)
        gc.collect()
        gc.disable()
        try:
            t0 = time.perf_counter()
            for i in range(steps):
                runner.step(0)
            torch.cuda.synchronize()
            dt_eager = time.perf_counter() - t0
        finally:
            gc.enable()
        events = ops.kernel_events[main_scene.roofline_key]
        # the same op with nothing beside it: the middle scene alone on the current stream (with several scenes the timed steps run
        # their streams concurrently and the op shares the chip)
        ops.kernel_events = {main_scene.roofline_key: []}
        for i in range(3):
            main_scene.step(0)
        torch.cuda.synchronize()
        events_alone = ops.kernel_events[main_scene.roofline_key]
        ops.kernel_events = None
        dt = dt_eager
        if use_graphs:
            # every scene's step captured once into a hipGraph on a stream of its own, a timed step = one replay per scene: the
            # host issues 3 launches per step instead of ~300 (Scene.capture).  Eager stays the fallback: never re-exec'ed, and a
            # capture that fails only costs this leg its graph numbers.
            # With several scenes the largest one's chain of kernels sets the step: it gets the two-stage form (match and finish
            # captured apart, its sampling + solve under its next step's matching: Scene.capture_pipelined); two-stage graphs for
            # every scene put more streams on the chip than they find idle CUs for (pyr-fp16: 6.7 k against 8.2 k pairs/s).
            try:
                longest = max(scenes, key=lambda sc: sc.size)
                # (streams from the tested pool: one per scene and one more for the second stage -- parallel.concurrent_streams)
                pool = parallel.concurrent_streams(max(len(scenes) + 1, 3))
                for k, sc in enumerate(scenes):
                    if len(scenes) == 1:
                        sc.capture_pipelined(0, streams=pool[:3], stages=3)  # the three stages of the eager steps, as graphs
                    elif sc is longest:
                        sc.capture_pipelined(0, streams=(pool[k], pool[len(scenes)]))
                    else:
                        sc.capture(0, stream=pool[k])
                torch.cuda.synchronize()

                def replay_all():
                    for sc in scenes:
                        if sc is longest:
                            sc.replay_pipelined()
                        else:
                            sc.replay()

                for _ in range(4):
                    replay_all()
                torch.cuda.synchronize()
                gc.collect()
                gc.disable()
                try:
                    t0 = time.perf_counter()
                    for i in range(steps):
                        replay_all()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    gc.enable()
                graphs = True
            except Exception as e:  # noqa: BLE001 -- whatever the capture trips over, the eager numbers stand
                graph_note = f"graph capture failed, eager numbers reported: {type(e).__name__}: {str(e)[:200]}"
                torch.cuda.synchronize()
    pairs = wl["pairs"] * len(scenes)
    S0 = main_scene.size
    us = float(np.mean([a.elapsed_time(b) for a, b in events])) * 1e3
    fbytes = 2 if dtype == torch.float16 and ops.NATIVE_FP16 else 4
    nbytes = algorithmic_bytes_local_corr(2 * wl["pairs"], 32, side_of("4", S0), main_scene.grids[2], 4, fbytes)
    eager_mode = "eager launches" + (", three stages on three streams (first pass | refinement pass | sampling + solve)" if len(scenes) == 1 else ", one stream per scene")
    graph_mode = ("hipGraph replay (seeds of the capture): " +
                  ("one captured step per scene and stream; the largest scene as two graphs on two streams (match | sampling + solve), a step's "
                   "second stage under the next step's first" if len(scenes) > 1 else
                   "three graphs on three streams (first pass | refinement pass + post-processing | sampling + solve), two copies each"))
    dt_graph = dt if graphs else None
    dt = dt_eager  # `value` is ALWAYS the eager rate (fresh seeds per step) since round 5 (one arrangement per workload); the
                   # graph-replay rate, where --graphs asked for it, sits under `graphs`
    out = {"value": round(pairs * steps / dt, 2), "unit": "pairs/s", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
           "pairs_per_step": pairs, "workload": wl["label"], "mode": eager_mode,
           "roofline_op": f"scale-4 local correlation, c32, {side_of('4', S0)}x{side_of('4', S0)}, G{main_scene.grids[2]}, r4, {2 * wl['pairs']} directions",
           "roofline_timed_in": "the eager steps (HIP events around the C-ABI call; with several scenes their streams run concurrently)",
           "roofline_avg_launch_us": round(us, 2), "roofline_frac": round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    us_alone = float(np.mean([a.elapsed_time(b) for a, b in events_alone])) * 1e3
    out["roofline_avg_launch_us_alone"] = round(us_alone, 2)
    out["roofline_frac_alone"] = round(nbytes / (us_alone * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
    if graphs:
        out["graphs"] = {"value": round(pairs * steps / dt_graph, 2), "ms_per_step": round(dt_graph / steps * 1e3, 3), "mode": graph_mode}
    if graph_note:
        out["note"] = graph_note
    return out


def stress_leg(mode, wl, B, dtype, dev, rank, steps=5):
    """A few one-stream steps of the main workload with stress flows (gfnet_amd._synthetic.FLOW_MODES): pairs/s, the roofline op's
    call time and the routes its tiles took.  Nothing here is compared with an oracle (tests/ cover the parity of these routes)."""
    import numpy as np
    import torch

    from gfnet_amd import ops
    from gfnet_amd._synthetic import FLOW_MODES, Scene, side_of

    with torch.inference_mode(False):
        scenes = [Scene(S, B, wl["num_itr"], dtype, "off", dev, rank, flows=mode) for S in wl["sizes"]]
    sc0 = scenes[min(1, len(scenes) - 1)] if len(scenes) > 1 else scenes[0]
    with torch.inference_mode():
        for i in range(2):
            for sc in scenes:
                sc.step(i)
        torch.cuda.synchronize()
        ops.kernel_events = {sc0.roofline_key: []}
        dt, _ = timed_loop(lambda i: [sc.step(0) for sc in scenes], steps, torch.cuda.synchronize)
        ev = ops.kernel_events[sc0.roofline_key]
        ops.kernel_events = None
        ops.kernel_counters = {}
        for sc in scenes:
            sc.step(0)
        cs = ops.kernel_counters.get(sc0.roofline_key, [])
        ops.kernel_counters = None
    G4, hs4 = sc0.grids[2], side_of("4", sc0.size)
    tiles4 = 2 * B * ((G4 + 15) // 16) * ((G4 + 3) // 4)
    us = float(np.mean([a.elapsed_time(b) for a, b in ev])) * 1e3 if ev else float("nan")
    fbytes = 2 if dtype == torch.float16 and ops.NATIVE_FP16 else 4
    nbytes = algorithmic_bytes_local_corr(2 * B, 32, hs4, G4, 4, fbytes)
    del scenes
    return {"value": round(B * len(wl["sizes"]) * steps / dt, 2), "unit": "pairs/s", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "arrangement": "one stream per scene (compare with `unpipelined_steps`)",
            "flows": {"noisy": "stand-in increment = true warp + N(0, sigma^2) - flow with sigma = 4 / 4 / 2 / 1 / 0.5 image pixels at scales 16 / 8 / 4 / 2 / 1",
                      "random": "the scale-8 refiner returns flows uniform in [-0.9, 0.9]; every other scale true warp + 0.5 px"}[mode],
            "noise_multipliers": FLOW_MODES[mode],
            "roofline_op_avg_launch_us": round(us, 2), "roofline_op_frac": round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
            "roofline_op_irregular_tile_frac": float(np.mean([c[0] for c in cs])) / tiles4 if cs else None,
            "roofline_op_half_staged_tile_frac": float(np.mean([c[2] for c in cs])) / tiles4 if cs else None,
            "roofline_op_flagged_cell_frac": float(np.mean([c[1] for c in cs])) / (2 * B * G4 * G4) if cs else None}


def main():
    args = parse_args()
    if (args.gpus > 1 or args.force_launcher) and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.dry_run:
        sys.exit(dry_run(args))

    import numpy as np
    import torch
    import torch.distributed as dist

    from gfnet_amd import ops, parallel
    from gfnet_amd._synthetic import FLOW_NOISE_PX, WORKLOADS, Scene, side_of

    with stdout_to_stderr():
        rank, world, local = parallel.init_from_env(backend=args.backend)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}, or "
                         "unset WORLD_SIZE and let bench.py start the ranks itself")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the hot path)")
    torch.cuda.set_device(local)
    # a world of one under the self-launcher (--force-launcher): still a process group, so that the barrier and the reduction of
    # the step time below run through RCCL on the box the driver has (prove the relay with RCCL loaded)
    group_of_one = world == 1 and bool(os.environ.get("GFN_BENCH_CHILD")) and not dist.is_initialized()
    if group_of_one:
        with stdout_to_stderr():
            dist.init_process_group(backend=args.backend, rank=0, world_size=1)
    if world > 1 or group_of_one:
        with stdout_to_stderr():  # the communicator (and RCCL's banner) comes up with the first collective
            dist.barrier()
    dev = torch.device("cuda", local)
    wl = WORKLOADS[args.workload]
    if args.pipeline is None:
        args.pipeline = len(wl["sizes"]) == 1
    B = args.pairs_per_gpu or wl["pairs"]
    dtype = torch.float16 if wl["dtype"] == "fp16" else torch.float32

    # ---- synthetic workload, resident in HBM before the timed region -------------------------------
    scenes = [Scene(S, B, wl["num_itr"], dtype, args.conv_stack, dev, rank, flows=args.flows) for S in wl["sizes"]]
    main_scene = scenes[min(1, len(scenes) - 1)] if len(scenes) > 1 else scenes[0]  # the 448 scene of the pyramid workload
    pairs_per_step = B * len(scenes)

    runner = SceneRunner(scenes, pipeline=args.pipeline, stages=args.stages)

    def step(seed):
        outs = runner.step(seed)
        Hl = torch.cat([o[0] for o in outs])
        return parallel.gather_homographies(Hl), outs

    in_group = world > 1 or group_of_one

    def sync():
        if in_group:
            dist.barrier()
        torch.cuda.synchronize()

    n_ranks_seen = 1
    with torch.inference_mode():
        for i in range(args.warmup):
            step(i)
        sync()
        if in_group:
            n_ranks_seen = dist.get_world_size()  # after an RCCL barrier: the ranks the collective really had
        if args.breakdown and rank == 0:
            from gfnet_amd.estimation import estimate_homographies
            from gfnet_amd.model.network import sample_batched

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
                return r, e0.elapsed_time(e1)
            for sc in scenes:
                m = sc.model
                (warp, cert), t_match = timed(lambda: m.match_pyramids(sc.pyr[0], sc.pyr[1], sc.pyr_up[0], sc.pyr_up[1], batched=True))
                (gm, _), t_sample = timed(lambda: sample_batched(m, warp, cert, 5000))
                _, t_solve = timed(lambda: estimate_homographies(gm, sc.sizes, iters=m.ransac_iters, seed=0))
                print(f"[breakdown] {sc.size}: match({sc.size}+{sc.up}) {t_match:.2f} ms | sample {t_sample:.2f} ms | solve {t_solve:.2f} ms", file=sys.stderr)
        torch.manual_seed(SAMPLER_SEED)
        dt, (Hall, outs) = timed_loop(lambda i: step(0), args.steps, sync)
        last = (Hall, outs)  # what the timed path returned in its last step (--dump-outputs)
        # The roofline op is timed in steps of its own, on ONE stream per scene with nothing beside it (in the pipelined timed region
        # the previous step's sampling + solve share the chip with it: 96 -> 107 us in round 3), HIP events around the C-ABI call.
        plain = runner if not args.pipeline else SceneRunner(scenes, pipeline=False)

        def plain_step(seed):
            outs_ = plain.step(seed)
            return parallel.gather_homographies(torch.cat([o[0] for o in outs_])), outs_

        plain_step(0)
        torch.cuda.synchronize()
        ops.kernel_events = {main_scene.roofline_key: []}
        n_roof = max(3, min(args.steps, 10))
        dt_plain, (Hall, outs) = timed_loop(lambda i: plain_step(0), n_roof, torch.cuda.synchronize)
        events = ops.kernel_events[main_scene.roofline_key]
        # Guard on the stream pool (round 5: one run in a dozen read 7.8 k pairs/s on three streams against 9.4 k on one -- the pool's
        # 0.2-ms overlap probe had accepted streams that then serialised): three streams slower than one means the streams share a
        # hardware queue.  The pool is rebuilt once and the timed region repeated; both attempts are reported.
        retimed = None
        if args.pipeline and not in_group and dt / args.steps > 1.02 * dt_plain / n_roof:
            ops.kernel_events = None
            first_try = round(world * pairs_per_step * args.steps / dt, 2)
            parallel.release_streams()
            runner = SceneRunner(scenes, pipeline=args.pipeline, stages=args.stages)
            for i in range(args.warmup):
                step(i)
            sync()
            torch.manual_seed(SAMPLER_SEED)
            dt2, last = timed_loop(lambda i: step(0), args.steps, sync)
            retimed = {"first_pool_pairs_per_s": first_try, "second_pool_pairs_per_s": round(world * pairs_per_step * args.steps / dt2, 2),
                       "why": "the first stream pool ran the three-stage steps slower than one stream runs them: streams sharing a hardware queue"}
            dt = dt2  # `value` = the measurement on the rebuilt pool (one protocol, not the better of two: ADVICE r5); the first is on the line
        # The tile plan of the roofline op (bounding boxes, staging regions, second-launch list) is written by extra workgroups
        # of the refiner_input launch, outside the bracket above.  Three more, untimed, steps with the plan as the op's own launch
        # inside the bracket attribute it back; since round 6 that figure IS `roofline.frac`, so it gets as many
        # steps as the plan-less figure.
        ops.FUSE_PLAN = False
        ops.kernel_events = {main_scene.roofline_key: []}
        plain_step(0)
        torch.cuda.synchronize()
        ops.kernel_events = {main_scene.roofline_key: []}
        for i in range(n_roof):
            plain_step(0)
        torch.cuda.synchronize()
        events_plan = ops.kernel_events[main_scene.roofline_key]
        ops.FUSE_PLAN = True
        ops.kernel_events = None
        # one more, untimed, step with a device sync after every local-correlation call: how many tiles the second launch
        # took and how many cells were redone per tap (both depend on the flows the workload produces)
        ops.kernel_counters = {}
        plain_step(0)
        counters = ops.kernel_counters.get(main_scene.roofline_key, [])
        if args.breakdown and rank == 0:
            for name, cs in ops.kernel_counters.items():
                print(f"[counters] {name}: second-launch tiles / flagged cells / half-staged tiles per call: {cs}", file=sys.stderr)
        ops.kernel_counters = None
        # stress legs: the same workload under flows that are NOT near the truth -- one stream, 5 steps each, with the
        # roofline op's time and what its tiles did (second launch / halves / flagged cells)
        stress = None
        if args.flows == "true" and args.conv_stack == "off" and world == 1 and not args.no_stress_legs and not args.pairs_per_gpu:
            stress = {mode: stress_leg(mode, wl, B, dtype, dev, rank) for mode in ("noisy", "random")}
        # the other single-GPU configurations of BASELINE.json on the same line (secondary legs, 8 steps each).  They run before the
        # conv-stack and pipelined legs: the three-scene workload is bound by the host's launch rate and read 10 % lower behind them
        # (their extra streams and scenes stay alive in the process)
        others = None
        if args.workload == "448b32" and args.conv_stack == "off" and world == 1 and not args.no_other_workloads and not args.pairs_per_gpu:
            others = {k: secondary_workload(k, "off", dev, rank, 8, use_graphs=args.graphs) for k in ("672b16", "pyr-fp16")}
        # the three-scene workload as the main workload: `value` above is eager (fresh seeds every step); the same workload driven by
        # hipGraph replays (largest scene in two stages) is reported next to it, measured exactly like the default line's leg
        graph_leg = None
        if args.graphs and len(wl["sizes"]) > 1 and args.conv_stack == "off" and world == 1 and not args.no_other_workloads and not args.pairs_per_gpu:
            graph_leg = secondary_workload(args.workload, "off", dev, rank, max(8, min(args.steps, 20)), use_graphs=True)
        # secondary figure: the same step with the refiners' real conv stacks (reference architecture, random-init)
        # in the class the reference runs them in on a GPU -- `value` above replaces them by a one-op stand-in
        stack_leg = None
        if args.conv_stack == "off" and world == 1 and not args.no_stack_leg:
            with torch.inference_mode(False):  # module parameters must be ordinary tensors (the packed-parameter cache reads their versions)
                scenes2 = [Scene(S, B, wl["num_itr"], dtype, "amp", dev, rank) for S in wl["sizes"]]
            runner2 = SceneRunner(scenes2, pipeline=args.pipeline, stages=args.stages)  # the same arrangement as the timed region
            for i in range(2):
                runner2.step(i)
            torch.cuda.synchronize()
            n2 = max(3, min(args.steps, 10))
            dt2, _ = timed_loop(lambda i: runner2.step(0), n2, torch.cuda.synchronize)
            # second roofline object: the conv blocks of three more one-stream steps, HIP events around every
            # gfn_conv_block_half_fwd call, grouped by (channels, grid): the wide blocks against the dense fp16 MFMA peak, the narrow
            # ones against HBM on their map bytes (half map in + half map out)
            class _Conv(dict):
                def __contains__(self, k):
                    return k.startswith("conv_block_half_")

                def __missing__(self, k):
                    self[k] = []
                    return self[k]

            plain2 = SceneRunner(scenes2, pipeline=False)
            plain2.step(0)
            torch.cuda.synchronize()
            ops.kernel_events = _Conv()
            for i in range(3):
                plain2.step(0)
            torch.cuda.synchronize()
            cev, ops.kernel_events = ops.kernel_events, None
            conv_rows, conv_us = [], 0.0
            for name, evs in cev.items():
                Cc, Gc = (int(v[1:]) for v in name.split("_")[3:5])
                us_ = float(np.mean([a.elapsed_time(b_) for a, b_ in evs])) * 1e3
                nb = 2 * B   # directions per call
                flop = 2.0 * nb * Gc * Gc * (Cc * Cc + 25 * Cc)
                map_bytes = 2.0 * nb * ((Cc + 1) // 2) * Gc * Gc * 4
                conv_us += us_ * len(evs) / 3
                conv_rows.append({"channels": Cc, "grid": Gc, "calls_per_step": round(len(evs) / 3, 2), "avg_launch_us": round(us_, 1),
                                  "tflops": round(flop / us_ / 1e6, 1), "frac_of_fp16_mfma_peak_2500": round(flop / us_ / 1e6 / 2500.0, 4),
                                  "map_tb_per_s": round(map_bytes / us_ / 1e6, 2), "frac_of_hbm_8tbs": round(map_bytes / us_ / 1e6 / 8.0, 3)})
            conv_rows.sort(key=lambda r_: -r_["avg_launch_us"] * r_["calls_per_step"])
            wide = [r_ for r_ in conv_rows if r_["channels"] >= 128]
            narrow = [r_ for r_ in conv_rows if r_["channels"] < 128]
            wsum = sum(r_["avg_launch_us"] * r_["calls_per_step"] for r_ in wide) or 1.0
            nsum = sum(r_["avg_launch_us"] * r_["calls_per_step"] for r_ in narrow) or 1.0
            conv_roofline = {"what": "fused conv blocks (depthwise 5x5 + BatchNorm + ReLU + 1x1, fp16 maps) of a step, per (channels, grid); blocks whose "
                                     "first input is the fp32 concat or whose output is the 3-channel fp32 head count with the map bytes of a half map pair "
                                     "(an under-estimate of their traffic)",
                             "conv_us_per_step": round(conv_us, 1),
                             "wide_blocks": {"bound": "mfma", "peak": 2500.0, "unit": "TFLOP/s", "us_per_step": round(wsum, 1),
                                             "frac_time_weighted": round(sum(r_["frac_of_fp16_mfma_peak_2500"] * r_["avg_launch_us"] * r_["calls_per_step"] for r_ in wide) / wsum, 4)},
                             "narrow_blocks": {"bound": "hbm", "peak": 8000.0, "unit": "GB/s", "us_per_step": round(nsum, 1),
                                               "frac_time_weighted": round(sum(r_["frac_of_hbm_8tbs"] * r_["avg_launch_us"] * r_["calls_per_step"] for r_ in narrow) / nsum, 3)},
                             "rows": conv_rows}
            stack_leg = {"value": round(pairs_per_step * n2 / dt2, 2), "unit": "pairs/s", "ms_per_step": round(dt2 / n2 * 1e3, 3), "steps": n2,
                         "conv_roofline": conv_roofline,
                         "step_pipeline": "as the timed region" if args.pipeline else "off",
                         "refiner_conv_stack": "reference architecture, random-init, HIP conv_stack kernels, conv_precision='amp' (fp16 maps, "
                                               "fp16 operands, fp32 accumulation: model/network.py:560-562)"}
            del scenes2
    # secondary figure: the same steps on one stream per scene (what `value` was until round 3), from the roofline steps above
    pipe_leg = None
    if args.pipeline:
        pipe_leg = {"value": round(world * pairs_per_step * n_roof / dt_plain, 2), "unit": "pairs/s", "ms_per_step": round(dt_plain / n_roof * 1e3, 3),
                    "steps": n_roof, "what": "the same steps on ONE stream per scene (sampling + solve of a step not overlapped with the next "
                                             "step's match; HIP events around the roofline op inside, this rank only): rounds 1-3 reported this as `value`"}
    # what a hard pair costs: the timed scenes' matches are ~95 % inliers, so OpenCV's confidence bound ends RANSAC after <= 16 hypotheses
    # and the wide hypothesis / scoring kernels are no-ops.  Same sampled matches with every second correspondence replaced by a random
    # one: the bound stays at maxIters = 2000 for every pair.
    worst_leg = None
    if world == 1 and len(scenes) == 1 and args.conv_stack == "off":
        from gfnet_amd.estimation import estimate_homographies

        with torch.inference_mode():
            good = outs[0][1].clone()
            gen = torch.Generator(device=dev).manual_seed(99)
            bad = torch.rand(good.shape, device=dev, generator=gen) * 2 - 1
            good[:, ::2] = bad[:, ::2]
            for _ in range(2):
                estimate_homographies(good, main_scene.sizes, iters=main_scene.model.ransac_iters, seed=1)
            torch.cuda.synchronize()
            nw = 10
            dtw, Hw = timed_loop(lambda i: estimate_homographies(good, main_scene.sizes, iters=main_scene.model.ransac_iters, seed=1), nw,
                                 torch.cuda.synchronize)
            err = [float(np.abs(np.linalg.inv(main_scene.H[k]) @ Hw[k].cpu().numpy() / (np.linalg.inv(main_scene.H[k]) @ Hw[k].cpu().numpy())[2, 2] - np.eye(3)).max())
                   for k in range(min(4, B))]
        worst_leg = {"ms_per_batch": round(dtw / nw * 1e3, 3), "pairs": B, "outlier_frac": 0.5,
                     "what": "RANSAC + DLT + LM of one batch with half of every pair's 5000 correspondences replaced by random ones: 2000 "
                             "hypotheses scored per pair (the timed steps stop after <= 16); solve time only",
                     "max_abs_dev_of_H_from_truth_first_pairs": [round(e, 5) for e in err]}
    if in_group:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / args.steps * 1e3
    pairs_per_s = world * pairs_per_step * args.steps / dt

    S0 = main_scene.size
    hs4, G4 = side_of("4", S0), main_scene.grids[2]
    n_calls = wl["num_itr"][2]  # roofline op calls per step and scene (one per refiner iteration at scale 4)
    kern_us = float(np.mean([a.elapsed_time(b) for a, b in events])) * 1e3 if events else float("nan")
    plan_us = float(np.mean([a.elapsed_time(b) for a, b in events_plan])) * 1e3 if events_plan else float("nan")
    fbytes = 2 if dtype == torch.float16 and ops.NATIVE_FP16 else 4
    nbytes = algorithmic_bytes_local_corr(2 * B, 32, hs4, G4, 4, fbytes)
    achieved = nbytes / (kern_us * 1e-6) / 1e9 if events else float("nan")
    achieved_plan = nbytes / (plan_us * 1e-6) / 1e9 if events_plan else float("nan")
    traffic, traffic_src = None, None
    pmc = os.path.join(ROOT, "profiles", "local_corr_pmc.json")  # written from the rocprofv3 --pmc passes (tools/pmc_hbm_local_corr.sh)
    if os.path.exists(pmc) and args.workload == "448b32":
        try:
            j = json.load(open(pmc))
            traffic, traffic_src = j.get("hbm_bytes_per_launch"), "static: " + j.get("source", "profiles/local_corr_pmc.json")
        except Exception:
            traffic = None
    tiles4 = 2 * B * ((G4 + 15) // 16) * ((G4 + 3) // 4)
    irregular = float(np.mean([c[0] for c in counters])) / tiles4 if counters else None
    flagged = float(np.mean([c[1] for c in counters])) / (2 * B * G4 * G4) if counters else None
    halves = float(np.mean([c[2] for c in counters])) / tiles4 if counters else None

    out = {
        "metric": "image pairs/sec at 448x448 (post-backbone hot path: correlation -> flow -> sampling -> homography)"
                  if args.workload == "448b32" else f"image pairs/sec, workload {args.workload} (post-backbone hot path)",
        "value": round(pairs_per_s, 2), "unit": "pairs/s", "n_gpus": world, "n_ranks_seen": n_ranks_seen,
        "collective_backend": (args.backend + (" (RCCL)" if args.backend == "nccl" else "")) if in_group else None, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": wl["label"], "workload_key": args.workload, "pairs_per_gpu": pairs_per_step,
                   "image_sizes": wl["sizes"], "num_itr": wl["num_itr"], "feature_storage": wl["dtype"],
                   "symmetric": True, "upsample_pass": "1.25x (560 at 448)", "attenuate_cert": True,
                   "step_pipeline": ("off" if not args.pipeline else
                                     "three stages on three streams, every kernel on the whole batch: first pass | refinement pass + post-processing | "
                                     "sampling + solve; a step's later stages run beside the next steps' earlier ones" if runner.stages3 else
                                     "a step's sampling + solve (second stream) run under the next step's match"),
                   "flow_noise": f"stand-in increment = true warp + N(0,({FLOW_NOISE_PX}/S)^2) - flow, fresh realisation per iteration" +
                                 ("" if args.flows == "true" else f"; --flows {args.flows}: see gfnet_amd._synthetic.FLOW_MODES"),
                   "stages": "corr_softargmax, (refiner_input + local_corr + flow_update) x scales x num_itr for both passes, resize, "
                             "match_post, sample(2 draws without replacement + KDE 20000^2), RANSAC(<= 2000 hypotheses, OpenCV's confidence-0.99999 "
                             "bound)+DLT+LM, H all-gather",
                   "excluded": ("DINOv2/FPN backbone; refiner conv stacks replaced by the stand-in increment (1 torch elementwise op per "
                                "refiner call; --conv-stack fp32|fp16|amp runs them on the HIP conv-stack kernels)") if args.conv_stack == "off"
                   else "DINOv2/FPN backbone (PyTorch-ROCm host code)",
                   "refiner_conv_stack": "off" if args.conv_stack == "off" else
                   f"reference architecture (9 dw5x5+BN+ReLU+1x1 blocks + out conv per refiner call, C=417/361/177/73/24), random-init, "
                   f"HIP conv_stack kernels, " + {"fp32": "fp32 throughout", "fp16": "1x1 operands fp16, maps fp32",
                                               "amp": "fp16 maps between the blocks, depthwise and 1x1 operands fp16, fp32 accumulation "
                                                      "(the reference's autocast class)"}[args.conv_stack] +
                   "; output weighted 0 next to the stand-in increment",
                   "parallelism": f"pairs sharded over {world} GPU(s), RCCL all-gather of H only"},
        "roofline": {"bound": "hbm",
                     "kernel": f"gfn_local_corr_fwd_dt call (tile kernel, its first workgroups finish the tiles the plan left to the second "
                               f"launch; c32, {hs4}x{hs4}, G{G4}, r4, {2 * B} directions) INCLUDING its tile plan.  In the product the plan is "
                               f"written by extra workgroups of the preceding refiner_input launch; `achieved` / `frac` / `avg_launch_us` time the "
                               f"op with the plan as its own launch inside the bracket (the plan is work only this op needs: VERDICT r5); "
                               f"`*_excl_plan` = the product's call alone, the plan left in the refiner_input launch (rounds 2-5 reported "
                               f"that as `frac`).  Both timed in steps of their own on one stream per scene, nothing beside them (not in "
                               f"the pipelined timed region, where the previous step's sampling + solve share the chip with the op)",
                     "achieved": round(achieved_plan, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved_plan / HBM_PEAK_GBS, 4), "frac_excl_plan": round(achieved / HBM_PEAK_GBS, 4),
                     "frac_of_achievable_6p29": round(achieved_plan / HBM_ACHIEVABLE_GBS, 4),
                     "traffic": traffic, "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": nbytes, "avg_launch_us": round(plan_us, 2), "avg_launch_us_excl_plan": round(kern_us, 2),
                     "calls_per_step": n_calls,
                     "irregular_tile_frac": irregular, "half_staged_tile_frac": halves, "flagged_cell_frac": flagged},
    }
    n_cpu = wl["cpu_pairs"] if args.cpu_pairs < 0 else args.cpu_pairs
    if rank == 0 and world == 1 and n_cpu > 0:
        n_cpu = min(n_cpu, B)
        v, cores = cpu_baseline(scenes, n_cpu)
        out["cpu_baseline"] = {"value": round(v, 4), "unit": "pairs/s", "cores": cores, "kind": "port",
                               "sample": f"{n_cpu} pair(s) per image size of the same workload through oracle/ (C + OpenMP), "
                                         "1 warm-up + median of 3"}
        sc_i = scenes.index(main_scene)
        n_par = min(8, B)  # the CPU leg's cost is the oracle walk above, not the solve: eight pairs of the batch
        ace_o, ace_t = solve_parity(main_scene, outs[sc_i][1], outs[sc_i][0], n_par)
        out["corner_error_pairs"] = n_par
        out["mean_corner_error_vs_ref_px"] = ace_o
        out["mean_corner_error_vs_truth_px"] = ace_t
    if stack_leg is not None:
        out["with_conv_stacks"] = stack_leg
    if pipe_leg is not None:
        out["unpipelined_steps"] = pipe_leg
    if worst_leg is not None:
        out["solve_worst_case"] = worst_leg
    if retimed is not None:
        out["stream_pool_retimed"] = retimed
    if stress is not None:
        out["stress_flows"] = stress
    out["gc"] = "disabled inside every timed loop"
    out["value_definition"] = ("v2 (rounds 4-5): eager launches, fresh sampler / RANSAC seeds every step, the stages of a step on three HIP streams "
                               "(a step's later stages beside the next steps' earlier ones) for one-scene workloads, one stream per scene for "
                               "the three-scene workload; `unpipelined_steps` = v1 (rounds 1-3): the same steps on one stream.  Secondary "
                               "workloads: `value` = their eager rate, graph replays only under `graphs` (--graphs)")
    if others is not None:
        out["other_workloads"] = others
    if graph_leg is not None:
        out["graph_replay"] = graph_leg
    if rank == 0 and args.dump_outputs:
        Hall, outs = last
        arrays = {"homographies": Hall.cpu().numpy()}
        for sc, (_, good) in zip(scenes, outs):
            arrays[f"matches_{sc.size}"] = good.cpu().numpy()
        dump_outputs(args.dump_outputs, arrays)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if in_group:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
