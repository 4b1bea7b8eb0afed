#!/usr/bin/env python3
"""Device-resident batched Snappy benchmark (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3-decompress]
                    [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch resident in HBM.
A plain run sets up the batch, warms up, times the K steps and prints the
result line (metric, value, ms_per_step, config).  `--dump-outputs DIR` also
writes what the last timed step computed as DIR/<name>.npy (dump_outputs).
Everything else the benchmark measures or checks runs only with `--full`: the
oracle spot check and round-trip check (`correct`), the roofline figures, the
encode leg, the end-to-end legs, the CPU baselines, the multi-GPU all-gather
and root-scatter, the serial comparison of a pipelined run, and c1-echo's
other codec modes.  The --no-* switches trim a --full run.
Default workload (the north-star target config): decompress
65,536 x 64 KiB Zipf-text bodies; the same run also times C3 compress of the
same bodies (the `encode` object).  Other workloads: c2-decompress (65,536 x
4 KiB random), c3-compress, cm-decompress (power-law 256 B..1 MiB, strong
scaling by default), c5-compress, and c1-echo (config 1: example/echo
over loopback, QPS and latency; tools/echo_bench.cc).

Multi-GPU: one process per GPU.  `--gpus N` without a
WORLD_SIZE in the environment makes this process a launcher: it spawns N
ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1) before anything
touches the GPU and exits with their status.  Under torch.distributed.run the
environment is already set and the process is a rank.  Each rank owns a
contiguous range of messages (weak: a full batch per rank; strong: one batch
cut by cumulative bytes); there is no data-path collective.  RCCL carries the
measurement collectives (MAX of times, SUM of counters), the all-gather of
per-message (out_len, status), and the root-scatter variant (grouped
send/recv of compressed shards from rank 0, reported beside the pre-placed
rate).  Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import platform
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO / "flare-cpp_amd" / "py"))

import fsg  # noqa: E402
import shard  # noqa: E402

GIB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
METRIC = "GiB/s device-resident Snappy decode+encode, batched RPC bodies, 1/2/4/8 GPU"

WORKLOADS = {
    # name: (op, kind, n_msgs, size spec, default scaling, description)
    "c3-decompress": ("decompress", fsg.KIND_TEXT, 65536, 65536, "weak",
                      "C3 decompress: 65,536 x 64 KiB Zipf-text bodies (~2.0x), device-resident"),
    "c2-decompress": ("decompress", fsg.KIND_RANDOM, 65536, 4096, "weak",
                      "C2 decompress: 65,536 x 4 KiB random bodies, device-resident"),
    "c3-compress": ("compress", fsg.KIND_TEXT, 65536, 65536, "weak",
                    "C3 compress: 65,536 x 64 KiB Zipf-text bodies, device-resident"),
    "cm-decompress": ("decompress", fsg.KIND_MIXED, 1 << 20, "mixed", "strong",
                      "CM decompress: 1,048,576 power-law bodies 256 B..1 MiB, 1 in 4 random"),
    "c5-compress": ("compress", fsg.KIND_PROTO, 262144, "mixed", "strong",
                    "C5 compress: 262,144 synthetic SnappyMessageProto responses"),
}


def kernel_source_hash() -> str:
    h = hashlib.sha256()
    for p in sorted((REPO / "flare-cpp_amd" / "csrc").glob("*")):
        if p.is_file():
            h.update(p.read_bytes())
    return h.hexdigest()[:16]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c3-decompress", choices=sorted(WORKLOADS) + ["c1-echo"])
    ap.add_argument("--n-msgs", type=int, default=0, help="override messages per GPU (weak) / total (strong)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-encode", action="store_true", help="skip the encode leg of a decompress run")
    ap.add_argument("--no-root-scatter", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--verify-sample", type=int, default=64)
    ap.add_argument("--decode-kernel", type=int, default=0,
                    help="decoder variant (0 = library default, 1/3/4 = force; A/B runs)")
    ap.add_argument("--encode-kernel", type=int, default=0,
                    help="encoder variant (0 = library default, 1/3 = force; A/B runs)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="weak: every GPU owns a full batch; strong: one batch split by bytes "
                         "(default: per workload, strong for cm/c5)")
    ap.add_argument("--pipeline", type=int, default=0,
                    help="decompress on a GPU: time a stream of two alternating batches, batch k+1's "
                         "tag walk (pass 1, its own stream) beside batch k's execution "
                         "(fsg_decompress_batch_2s); 0 = one batch, both passes on one stream")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the checks and the secondary measurements (correct, roofline, encode, "
                         "end_to_end, cpu_baseline, multi_gpu); a plain run times the steps only")
    ap.add_argument("--device", choices=["cuda", "cpu"], default="cuda", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------
# Launcher: N ranks, spawned before any GPU call in this process.

def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(nprocs: int, argv: list[str], entry: str | None = None, env_extra: dict | None = None,
           timeout_s: float | None = None) -> int:
    """Start `nprocs` ranks of `entry` (default: this file) with torchrun's
    environment and wait for them.  A rank that fails ends the others (a
    collective would otherwise wait for it forever).  Returns the worst exit
    status."""
    port = _free_port()
    procs = []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(nprocs), LOCAL_WORLD_SIZE=str(nprocs),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.update(env_extra or {})
        procs.append(subprocess.Popen([sys.executable, entry or str(Path(__file__).resolve()), *argv], env=env))
    t0 = time.time()
    rc = 0
    try:
        while procs:
            for p in list(procs):
                code = p.poll()
                if code is None:
                    continue
                procs.remove(p)
                if code != 0:
                    rc = code if rc == 0 else rc
                    for q in procs:
                        q.terminate()
            if timeout_s is not None and time.time() - t0 > timeout_s:
                for q in procs:
                    q.kill()
                return 124
            time.sleep(0.05)
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    return rc if rc >= 0 else 128 - rc


# ---------------------------------------------------------------------------
# Timing: HIP events on the codec's stream (GPU) or wall clock (the CPU test
# ranks).

class _Timer:
    def __init__(self, torch, device, stream, n):
        self.torch, self.gpu = torch, device.type == "cuda"
        self.stream = stream
        if self.gpu:
            self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        else:
            self.t = [0.0] * (n + 1)

    def mark(self, k):
        if self.gpu:
            self.ev[k].record(self.stream)
        else:
            self.t[k] = time.perf_counter()

    def ms(self, k):
        if self.gpu:
            return self.ev[k].elapsed_time(self.ev[k + 1])
        return (self.t[k + 1] - self.t[k]) * 1e3


def _sync(torch, device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def batch_sizes(size_spec, first_index, n):
    if size_spec == "mixed":
        # shard of the CM/C5 size stream: regenerate the stream prefix and slice
        return fsg.mixed_sizes(first_index + n)[first_index:]
    return np.full(n, size_spec, dtype=np.uint32)


def time_steps(torch, device, stream, step, steps, warmup, world, dist):
    for _ in range(warmup):
        step()
    _sync(torch, device)
    if world > 1:
        dist.barrier()
    _sync(torch, device)
    tm = _Timer(torch, device, stream, steps)
    t0 = time.perf_counter()
    tm.mark(0)
    for k in range(steps):
        step()
        tm.mark(k + 1)
    _sync(torch, device)
    if world > 1:
        dist.barrier()
    _sync(torch, device)
    wall = time.perf_counter() - t0
    kern_ms = [tm.ms(k) for k in range(steps)]
    return wall / steps, float(np.mean(kern_ms)) / 1e3


def time_pipelined(torch, dev, stream, slots, issue, steps, warmup, world, dist):
    """Times `steps` decodes of a stream of batches: step k decodes slot
    k % len(slots) with its tag walk on a second stream (`issue(k, s1)`), so
    batch k+1's walk runs beside batch k's execution.  Step k+len(slots)
    reuses step k's buffers, so its walk waits for step k's execution (an
    event): one batch in flight ahead.  Returns (seconds per step, mean
    per-batch latency in seconds = walk start to execution end)."""
    s1 = torch.cuda.Stream(dev)
    nslot = len(slots)
    done = [None] * nslot

    def run(k, marks=None):
        sl = k % nslot
        if done[sl] is not None:
            s1.wait_event(done[sl])
        if marks is not None:
            marks[0][k].record(s1)
        issue(k, s1)
        ev = torch.cuda.Event()
        ev.record(stream)
        done[sl] = ev
        if marks is not None:
            marks[1][k].record(stream)

    for k in range(warmup):
        run(k)
    _sync(torch, dev)
    if world > 1:
        dist.barrier()
    _sync(torch, dev)
    done = [None] * nslot
    t_start = torch.cuda.Event(enable_timing=True)
    t_end = torch.cuda.Event(enable_timing=True)
    marks = ([torch.cuda.Event(enable_timing=True) for _ in range(steps)],
             [torch.cuda.Event(enable_timing=True) for _ in range(steps)])
    t0 = time.perf_counter()
    t_start.record(stream)
    s1.wait_stream(stream)  # the first walk starts after the start mark
    for k in range(steps):
        run(k, marks)
    t_end.record(stream)
    _sync(torch, dev)
    if world > 1:
        dist.barrier()
    _sync(torch, dev)
    wall = time.perf_counter() - t0
    lat = [marks[0][k].elapsed_time(marks[1][k]) for k in range(steps)]
    return wall / steps, t_start.elapsed_time(t_end) / 1e3 / steps, float(np.mean(lat)) / 1e3


def rank_main(args, codec_factory=None):
    """One rank of the benchmark.  `codec_factory(local_rank)` replaces the HIP
    codec only in the CPU launcher test (tests/test_distributed.py)."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    gpu = args.device == "cuda"
    # Test knob (tests/test_gpu_multirank.py): every rank on this one device
    # with gloo collectives, so the N-rank path runs the HIP codec on a
    # one-GPU box (RCCL refuses two ranks on one device).  Never a bench line.
    shared = os.environ.get("FSG_BENCH_SHARED_DEVICE")
    if gpu:
        local = int(shared) if shared is not None else local
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    else:
        dev = torch.device("cpu")
    backend = "nccl" if gpu and shared is None else "gloo"
    if world > 1:
        dist.init_process_group(backend, init_method="env://")
        world = dist.get_world_size()
    codec = codec_factory(local) if codec_factory else fsg.SnappyGPU(local)
    if args.decode_kernel or args.encode_kernel:  # else the library's choice (FSG_DECODE_KERNEL env)
        codec.select_kernels(args.decode_kernel, args.encode_kernel)

    op, kind, n_default, size_spec, scaling_default, desc = WORKLOADS[args.workload]
    scaling = args.scaling or scaling_default
    n_cfg = args.n_msgs or n_default
    t_gen = time.time()
    if scaling == "weak":
        first, last = shard.weak_range(n_cfg, rank)  # rank owns [rank*n, (rank+1)*n)
    else:
        first, last = shard.byte_balanced_ranges(batch_sizes(size_spec, 0, n_cfg), world)[rank]
    n = last - first
    batch = fsg.make_batch(kind, batch_sizes(size_spec, first, n), first_index=first)
    raw_total = batch.total

    def H(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    stream = torch.cuda.current_stream(dev) if gpu else None
    d_raw = H(batch.data)
    d_raw_off, d_raw_len = H(batch.offsets), H(batch.lens)
    caps = np.array([fsg.max_compressed_length(int(x)) for x in batch.lens], dtype=np.uint64)
    c_off, c_tot = fsg.slot_offsets(caps)
    d_comp = torch.zeros(c_tot, dtype=torch.uint8, device=dev)
    d_comp_off = H(c_off)
    d_comp_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    max_len = int(batch.lens.max()) if n else 0
    d_ws = codec.compress_workspace(n, max_len)
    # Compressed inputs come from the GPU encoder (checked against the oracle below).
    codec.compress(d_raw, d_raw_off, d_raw_len, n, max_len, d_comp, d_comp_off, d_comp_len, d_status,
                   stream=stream, workspace=d_ws)
    _sync(torch, dev)
    comp_len = d_comp_len.cpu().numpy()[:n].view(np.uint32).copy()
    comp_total = int(comp_len.astype(np.uint64).sum())
    full = args.full
    errors = int((d_status[:n] != 0).sum().item()) if full else 0

    # Oracle spot check of the compressed bytes (checker only, never timed).
    sample_ok = None
    if full and args.verify_sample > 0 and n:
        sys.path.insert(0, str(REPO / "oracle"))
        from bind import Oracle
        orc = Oracle()
        idx = np.linspace(0, n - 1, min(n, args.verify_sample)).astype(np.int64)
        host_comp = d_comp.cpu().numpy()
        sample_ok = all(
            host_comp[int(c_off[i]):int(c_off[i]) + int(comp_len[i])].tobytes() == orc.compress(batch.item(int(i)))
            for i in idx)
        del host_comp

    # Decode output slots (exact uncompressed sizes) -- laid out like the raw
    # batch, poisoned (0xA5) so a byte the decoder never writes fails the
    # round-trip check even where its true value is 0.
    d_out = torch.full((max(raw_total, 1),), 0xA5, dtype=torch.uint8, device=dev)
    d_out_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_dws = codec.decompress_workspace(n, c_tot)

    def decode_step():
        codec.decompress(d_comp, d_comp_off, d_comp_len, n, d_out, d_raw_off, d_raw_len, d_out_len,
                         d_status, stream=stream, workspace=d_dws)

    def encode_step():
        codec.compress(d_raw, d_raw_off, d_raw_len, n, max_len, d_comp, d_comp_off, d_comp_len,
                       d_status, stream=stream, workspace=d_ws)

    step = decode_step if op == "decompress" else encode_step
    algo_bytes = raw_total + comp_total  # each input byte read once, each output byte written once

    # Stream of batches (decompress on a GPU): a second, distinct batch of the
    # same shape (the next n bodies of the generator), with its own workspace
    # and outputs; batches alternate.
    pipe = None
    if op == "decompress" and gpu and args.pipeline and n:
        batch2 = fsg.make_batch(kind, batch_sizes(size_spec, first + n, n), first_index=first + n)
        d_raw2 = H(batch2.data)
        d_raw2_off, d_raw2_len = H(batch2.offsets), H(batch2.lens)
        caps2 = np.array([fsg.max_compressed_length(int(x)) for x in batch2.lens], dtype=np.uint64)
        c2_off, c2_tot = fsg.slot_offsets(caps2)
        d_comp2 = torch.zeros(c2_tot, dtype=torch.uint8, device=dev)
        d_comp2_off = H(c2_off)
        d_comp2_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_status2 = torch.zeros(n, dtype=torch.int32, device=dev)
        max_len2 = int(batch2.lens.max())
        d_ws2 = codec.compress_workspace(n, max_len2)
        codec.compress(d_raw2, d_raw2_off, d_raw2_len, n, max_len2, d_comp2, d_comp2_off, d_comp2_len,
                       d_status2, stream=stream, workspace=d_ws2)
        del d_ws2
        _sync(torch, dev)
        comp_len2 = d_comp2_len.cpu().numpy()[:n].view(np.uint32).copy()
        if full:
            errors += int((d_status2 != 0).sum().item())
        if full and args.verify_sample > 0:
            idx = np.linspace(0, n - 1, min(n, args.verify_sample)).astype(np.int64)
            host_comp2 = d_comp2.cpu().numpy()
            sample_ok = sample_ok and all(
                host_comp2[int(c2_off[i]):int(c2_off[i]) + int(comp_len2[i])].tobytes()
                == orc.compress(batch2.item(int(i))) for i in idx)
        d_out2 = torch.full((max(batch2.total, 1),), 0xA5, dtype=torch.uint8, device=dev)
        d_out_len2 = torch.zeros(n, dtype=torch.int32, device=dev)
        d_dws2 = codec.decompress_workspace(n, c2_tot)
        slots = [
            (d_comp, d_comp_off, d_comp_len, d_out, d_raw_off, d_raw_len, d_out_len, d_status, d_dws),
            (d_comp2, d_comp2_off, d_comp2_len, d_out2, d_raw2_off, d_raw2_len, d_out_len2, d_status2, d_dws2),
        ]

        def issue(k, s1):
            c, co, cl, o, oo, ocap, ol, st, ws = slots[k % 2]
            codec.decompress(c, co, cl, n, o, oo, ocap, ol, st, stream=stream, workspace=ws, pass1_stream=s1)

        pipe = {"slots": slots, "issue": issue, "raw2": d_raw2, "raw2_total": batch2.total,
                "comp2_total": int(comp_len2.astype(np.uint64).sum())}
    gen_s = time.time() - t_gen

    pipeline_info = None
    if pipe is not None:
        t_step, avg_kernel_s, lat_s = time_pipelined(torch, dev, stream, pipe["slots"], pipe["issue"],
                                                     args.steps, args.warmup, world, dist)
        if args.dump_outputs:  # the slot the last timed step decoded into
            _, _, _, o, _, _, ol, st, _ = pipe["slots"][(args.steps - 1) % 2]
            dump_outputs(torch, args.dump_outputs, rank, world, op, o,
                         raw_total if args.steps % 2 else pipe["raw2_total"], ol, st, n, None)
        # the same batch, both passes on one stream, for comparison (untimed in `value`)
        k_serial = time_steps(torch, dev, stream, step, args.steps, 1, world, dist)[1] if full else None
        # both batches' bytes per step pair: the mean over the stream
        algo_bytes = (raw_total + comp_total + pipe["raw2_total"] + pipe["comp2_total"]) / 2
        pipeline_info = {
            "batches": 2,
            "mode": "batch k+1's tag walk (pass 1) on a second stream beside batch k's execution "
                    "(fsg_decompress_batch_2s); one batch in flight ahead",
            "latency_ms_per_batch": round(lat_s * 1e3, 4),
            "serial_ms_per_step": round(k_serial * 1e3, 4) if full else None,
        }
    else:
        t_step, avg_kernel_s = time_steps(torch, dev, stream, step, args.steps, args.warmup, world, dist)
        if args.dump_outputs:
            if op == "decompress":
                dump_outputs(torch, args.dump_outputs, rank, world, op, d_out, raw_total, d_out_len,
                             d_status, n, None)
            else:
                dump_outputs(torch, args.dump_outputs, rank, world, op, d_comp, c_tot, d_comp_len,
                             d_status, n, c_off)

    # Correctness of the timed output (device-side, untimed).
    roundtrip_ok = None
    if full:
        errors += int((d_status[:n] != 0).sum().item())
        if op == "decompress":
            roundtrip_ok = bool(torch.equal(d_out[:raw_total], d_raw[:raw_total]))
            if pipe is not None:
                _, _, _, o2, _, _, _, st2, _ = pipe["slots"][1]
                errors += int((st2 != 0).sum().item())
                roundtrip_ok = roundtrip_ok and bool(torch.equal(o2[:pipe["raw2_total"]], pipe["raw2"]))
        else:
            roundtrip_ok = bool((d_comp_len.cpu().numpy()[:n].view(np.uint32) == comp_len).all())

    # Per-message (out_len, status) of every rank, gathered over RCCL.
    gather = gather_results(torch, dist, dev, world, rank, n, d_out_len, d_status,
                            batch.lens if op == "decompress" else comp_len) if full and world > 1 else None

    # Root-scatter variant: rank 0 is the only ingress; it sends each peer a
    # compressed shard with grouped send/recv, then every rank decodes.
    rscatter = None
    if full and world > 1 and op == "decompress" and not args.no_root_scatter:
        rscatter = root_scatter(torch, dist, dev, stream, world, rank, codec, d_comp, d_comp_off,
                                d_comp_len, n, d_raw, d_raw_len, d_raw_off, raw_total, c_tot)

    # bytes per step: a pipelined run alternates two batches (their mean)
    raw_v, comp_v = raw_total, comp_total
    if pipe is not None:
        raw_v = (raw_total + pipe["raw2_total"]) // 2
        comp_v = (comp_total + pipe["comp2_total"]) // 2
    if world > 1:
        t_step, avg_kernel_s, (raw_all, comp_all, errors, bad) = shard.reduce_measurements(
            dist, dev, t_step, avg_kernel_s, raw_v, comp_v, errors, int(full and not roundtrip_ok))
        roundtrip_ok = bad == 0 if full else None
    else:
        raw_all, comp_all = raw_v, comp_v

    # The encode leg of the default decode run (same bodies, already resident).
    enc = None
    if full and op == "decompress" and not args.no_encode and args.workload == "c3-decompress" and world == 1:
        enc = encode_leg(torch, dev, stream, encode_step, d_comp, d_comp_len, comp_len, raw_total,
                         comp_total, args, batch, c_off)

    # End-to-end (host pinned -> device -> kernel -> host pinned), untimed in `value`.
    e2e = None
    if full and not args.no_e2e and rank == 0 and gpu:
        e2e = end_to_end(torch, codec, op, batch, d_comp, c_off, comp_len, raw_total, comp_total, n,
                         max_len, dev, d_ws)

    cpu = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(op, batch, d_comp, c_off, comp_len, args.cpu_threads)

    if rank == 0:
        value = raw_all / t_step / GIB
        achieved = algo_bytes / avg_kernel_s / 1e9
        # PMC traffic is per launch of the full-size workload on one rank's shard
        pmc = (load_traffic(args.workload)
               if full and args.n_msgs == 0 and (scaling == "weak" or world == 1) else None)
        line = {
            "metric": METRIC,
            "value": round(value, 3),
            "unit": "GiB/s (uncompressed bytes)",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_step * 1e3, 4),
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic (splitmix64-seeded bodies, SURVEY.md §8(d)); compressed by the GPU "
                    "encoder" + (", byte-checked against the oracle" if full else ""),
            "config": {
                "workload": desc,
                "op": op,
                "messages_rank0": n,
                "global_batch": n * world if scaling == "weak" else n_cfg,
                "raw_bytes_all_ranks": raw_all,
                "compressed_bytes_all_ranks": comp_all,
                "ratio": round(raw_all / max(1, comp_all), 4),
                "parallelism": f"shard{world} ({scaling}: messages by index"
                               f"{', byte-balanced' if scaling == 'strong' else ''}; no data-path collective)",
                "world_size_seen_by_collectives": world,
                "backend": ("nccl (RCCL over xGMI)" if backend == "nccl" else
                            "gloo" + (" (shared device, test)" if shared is not None else "")) if world > 1 else None,
            },
            "roofline": {
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": pmc.get("traffic_bytes_per_launch") if pmc else None,
                "algorithmic_bytes_per_launch": algo_bytes,
                "avg_kernel_ms": round(avg_kernel_s * 1e3, 4),
                "read_frac": round((comp_v if op == "decompress" else raw_v) / avg_kernel_s / 1e9
                                   / HBM_PEAK_GBS, 4),
                "note": ("rank 0's bytes / MAX over ranks of the HIP-event launch time" if world > 1 else
                         "algorithmic bytes / average HIP-event duration of one launch on its stream")
                        + ("; pipelined: HIP-event time of the whole stream of batches / steps"
                           if pipeline_info else ""),
            },
            "cpu_baseline": cpu,
            "encode": enc,
            "end_to_end": e2e,
            "multi_gpu": {"allgather": gather, "root_scatter": rscatter} if world > 1 else None,
            "correct": {"status_errors": errors, "roundtrip_ok": roundtrip_ok, "oracle_sample_ok": sample_ok},
            "pipeline": pipeline_info,
            "kernel_src": kernel_source_hash(),
            "kernels": {"decode": args.decode_kernel, "encode": args.encode_kernel},
            "setup_s": round(gen_s, 2),
            "full": full,
        }
        if not full:  # a plain run reports the timed steps only
            line["roofline"] = line["correct"] = line["multi_gpu"] = None
        if args.dump_outputs:
            line["outputs"] = str(args.dump_outputs)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def gather_results(torch, dist, dev, world, rank, n, d_out_len, d_status, expect_len):
    """ncclAllGather of per-message (out_len, status): every rank ends with the
    whole batch's results.  Ranks hold different counts under strong scaling,
    so the rows are padded to the largest shard."""
    counts = torch.tensor([n], dtype=torch.int64, device=dev)
    allc = [torch.zeros_like(counts) for _ in range(world)]
    dist.all_gather(allc, counts)
    ns = [int(c.item()) for c in allc]
    mx = max(ns)
    mine = torch.full((mx, 2), -1, dtype=torch.int32, device=dev)
    if n:
        mine[:n, 0] = d_out_len[:n]
        mine[:n, 1] = d_status[:n]
    rows = [torch.empty_like(mine) for _ in range(world)]
    _sync(torch, dev)
    t0 = time.perf_counter()
    dist.all_gather(rows, mine)
    _sync(torch, dev)
    ms = (time.perf_counter() - t0) * 1e3
    both = torch.cat([r[:k] for r, k in zip(rows, ns)]).cpu().numpy()
    # each rank checks its own rows against its expected lengths; SUM the mismatches
    own = both[sum(ns[:rank]):sum(ns[:rank]) + n]
    bad = int((own[:, 1] != 0).sum()) + int(
        (own[:, 0].astype(np.int64) != np.asarray(expect_len[:n]).astype(np.int64)).sum())
    t = torch.tensor([bad], dtype=torch.int64, device=dev)
    dist.all_reduce(t)
    return {"messages": int(both.shape[0]), "bytes_per_rank": mx * 8, "ms": round(ms, 3),
            "mismatches": int(t.item()),
            "note": "all_gather of per-message (out_len:u32, status:i32) over all ranks"}


def root_scatter(torch, dist, dev, stream, world, rank, codec, d_comp, d_comp_off, d_comp_len, n,
                 d_raw, d_raw_len, d_raw_off, raw_total, c_tot):
    """One ingress, N decoders: rank 0 holds every rank's compressed shard (the
    ranks hand them over first, untimed) and sends each to its rank with
    grouped send/recv (RCCL has no scatterv); then every rank decodes its shard
    and checks the output against its own bodies.  Reported beside the
    pre-placed rate, never as `value`."""
    sizes = torch.tensor([c_tot], dtype=torch.int64, device=dev)
    alls = [torch.zeros_like(sizes) for _ in range(world)]
    dist.all_gather(alls, sizes)
    nb = [int(x.item()) for x in alls]
    ingress = None
    if rank == 0:  # untimed: collect the shards at the ingress rank
        ingress = [d_comp[:nb[0]]] + [torch.empty(nb[r], dtype=torch.uint8, device=dev) for r in range(1, world)]
        ops = [dist.P2POp(dist.irecv, ingress[r], r) for r in range(1, world)]
    else:
        ops = [dist.P2POp(dist.isend, d_comp[:c_tot], 0)]
    for w in dist.batch_isend_irecv(ops):
        w.wait()
    _sync(torch, dev)
    recv = d_comp if rank == 0 else torch.empty(c_tot, dtype=torch.uint8, device=dev)
    out = torch.empty(max(raw_total, 1), dtype=torch.uint8, device=dev)
    ol = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    st = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws = codec.decompress_workspace(n, c_tot)
    best = None
    for _ in range(2):
        if rank != 0:
            recv.zero_()
        _sync(torch, dev)
        dist.barrier()
        _sync(torch, dev)
        t0 = time.perf_counter()
        if rank == 0:
            ops = [dist.P2POp(dist.isend, ingress[r], r) for r in range(1, world)]
        else:
            ops = [dist.P2POp(dist.irecv, recv, 0)]
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        _sync(torch, dev)
        t_sc = time.perf_counter() - t0
        codec.decompress(recv, d_comp_off, d_comp_len, n, out, d_raw_off, d_raw_len, ol, st, stream=stream,
                         workspace=ws)
        _sync(torch, dev)
        t = torch.tensor([t_sc, time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if best is None or float(t[1]) < best[1]:
            best = (float(t[0]), float(t[1]))
    bad = int((st[:n] != 0).sum().item()) + int(not torch.equal(out[:raw_total], d_raw[:raw_total]))
    cnt = torch.tensor([bad, raw_total], dtype=torch.int64, device=dev)
    dist.all_reduce(cnt)
    sent = sum(nb[1:])
    return {"scatter_ms": round(best[0] * 1e3, 3), "scatter_plus_decode_ms": round(best[1] * 1e3, 3),
            "root_egress_gb_s": round(sent / best[0] / 1e9, 2),
            "gib_s_uncompressed_all_ranks": round(int(cnt[1]) / best[1] / GIB, 3),
            "mismatches": int(cnt[0].item()),
            "note": "rank 0 holds every compressed shard and sends each to its rank (grouped isend/irecv), "
                    "then all ranks decode; MAX over ranks; output checked against each rank's bodies"}


def encode_leg(torch, dev, stream, encode_step, d_comp, d_comp_len, comp_len, raw_total, comp_total,
               args, batch, c_off):
    """C3 compress of the same bodies: the encode half of the metric."""
    steps = max(3, min(args.steps, 10))
    t_step, avg_kernel_s = time_steps(torch, dev, stream, encode_step, steps, 1, 1, None)
    ok = bool((d_comp_len.cpu().numpy()[:len(comp_len)].view(np.uint32) == comp_len).all())
    achieved = (raw_total + comp_total) / avg_kernel_s / 1e9
    pmc = load_traffic("c3-compress")
    out = {
        "workload": "C3 compress: the same 65,536 x 64 KiB bodies, device-resident",
        "value": round(raw_total / t_step / GIB, 3),
        "unit": "GiB/s (uncompressed bytes)",
        "steps": steps,
        "ms_per_step": round(t_step * 1e3, 4),
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": pmc.get("traffic_bytes_per_launch") if pmc else None,
                     "algorithmic_bytes_per_launch": raw_total + comp_total,
                     "avg_kernel_ms": round(avg_kernel_s * 1e3, 4)},
        "lengths_match_first_encode": ok,
    }
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline("compress", batch, d_comp, c_off, comp_len, args.cpu_threads)
    return out


def load_traffic(workload: str):
    p = REPO / "profiles" / f"pmc_{workload}.json"
    if not p.exists():
        return None
    d = json.loads(p.read_text())
    return d if d.get("kernel_src") == kernel_source_hash() else None


DUMP_SAMPLE = 1 << 22  # output bytes sampled by --dump-outputs (all ranks together)
DUMP_BLOCK = 4096      # bytes per block sum (per rank; times the world size)
DUMP_SEED = 0x5EED


def dump_outputs(torch, outdir, rank, world, op, d_buf, total, d_len, d_status, n, slot_off):
    """--dump-outputs: what the last timed step handed its caller, as .npy files
    that two builds can compare array for array (the inputs are seeded, so
    equal arguments give equal arrays).  At most 64 MB over all ranks:

      out_len.npy         float64[n]  per-message output length
      status.npy          float32[n]  per-message status
      out_bytes.npy       float32[k]  output bytes at k fixed, seeded positions
                                      (every byte if the output has at most k)
      out_block_sums.npy  float64[b]  decompress: byte sum of every block of
                                      DUMP_BLOCK x world output bytes

    A decompress output is dense (`total` bytes, slot_off None).  A compress
    output sits in MaxCompressedLength slots at `slot_off`; only the out_len
    bytes the encoder produced in each slot are sampled.  Ranks of a
    multi-GPU run write <name>_rank<r>.npy."""
    out = Path(outdir)
    out.mkdir(parents=True, exist_ok=True)
    lens = d_len[:n].cpu().numpy().view(np.uint32).astype(np.int64)
    rng = np.random.default_rng(DUMP_SEED + rank)
    k = max(1, DUMP_SAMPLE // world)
    if slot_off is None:
        pos = np.arange(total) if total <= k else np.sort(rng.integers(0, total, size=k))
    else:
        live = np.flatnonzero(lens > 0)
        m = np.sort(rng.choice(live, size=k)) if len(live) else live
        pos = slot_off[m].astype(np.int64) + (rng.random(len(m)) * lens[m]).astype(np.int64)
    sample = d_buf[torch.from_numpy(pos).to(d_buf.device)].cpu().numpy() if len(pos) else np.zeros(0, np.uint8)
    arrays = {"out_len": lens.astype(np.float64),
              "status": d_status[:n].cpu().numpy().astype(np.float32),
              "out_bytes": sample.astype(np.float32)}
    if slot_off is None:
        block = DUMP_BLOCK * world
        nb = total // block
        sums = torch.zeros(nb + (1 if total % block else 0), dtype=torch.float64, device=d_buf.device)
        per = max(1, (1 << 28) // block)  # 256 MiB of output per reduction
        for b0 in range(0, nb, per):
            b1 = min(nb, b0 + per)
            sums[b0:b1] = d_buf[b0 * block:b1 * block].view(-1, block).sum(dim=1, dtype=torch.int64)
        if total % block:
            sums[nb] = d_buf[nb * block:total].sum(dtype=torch.int64)
        arrays["out_block_sums"] = sums.cpu().numpy()
    nbytes = sum(a.nbytes for a in arrays.values())
    if nbytes * world > 64_000_000:
        raise RuntimeError(f"--dump-outputs: {nbytes} bytes per rank x {world} ranks exceeds 64 MB")
    for name, a in arrays.items():
        np.save(out / (f"{name}.npy" if world == 1 else f"{name}_rank{rank}.npy"), a)


def pack_bodies(torch, d_comp, c_off, comp_len, comp_total):
    """Compressed bodies moved from their encoder slots to a packed buffer
    (gathered on the host, ~1 s): returns (offsets, device buffer)."""
    hc = d_comp.cpu().numpy()
    p_off = np.zeros(len(comp_len), np.uint64)
    if len(comp_len) > 1:
        p_off[1:] = np.cumsum(comp_len[:-1].astype(np.uint64))
    packed = np.concatenate([hc[int(o):int(o) + int(ln)] for o, ln in zip(c_off, comp_len)] + [np.zeros(1, np.uint8)])
    del hc
    return p_off, torch.from_numpy(packed[:max(1, comp_total)]).to(d_comp.device)


def end_to_end(torch, codec, op, batch, d_comp, c_off, comp_len, raw_total, comp_total, n, max_len, dev,
               d_ws):
    """Pinned host -> HBM -> kernel -> pinned host, one pass (reported in DESIGN.md)."""
    stream = torch.cuda.current_stream()
    d_dws = codec.decompress_workspace(n, d_comp.numel())
    if op == "decompress":
        # The bodies as a receiver holds them: packed back to back (comp_total
        # bytes).  Until round 3 the legs uploaded the encoder's whole slot
        # buffer (MaxCompressedLength slots, ~2.3x the compressed bytes) and
        # divided by the compressed bytes: the "24 GB/s H2D" of rounds 1-2 was
        # that accounting, the copy itself ran at ~57 GB/s.
        c_off, d_comp = pack_bodies(torch, d_comp, c_off, comp_len, comp_total)
        h_in = torch.empty(d_comp.numel(), dtype=torch.uint8, pin_memory=True)
        h_in.copy_(d_comp)  # device -> pinned, so the pages are touched before the timed H2D
        h_out = torch.empty(raw_total, dtype=torch.uint8, pin_memory=True)
        d_in = torch.empty_like(d_comp)
        d_out = torch.empty(raw_total, dtype=torch.uint8, device=dev)
        in_bytes, out_bytes = comp_total, raw_total
    else:
        h_in = torch.from_numpy(batch.data).pin_memory()
        h_out = torch.empty(d_comp.numel(), dtype=torch.uint8, pin_memory=True)
        d_in = torch.empty(h_in.numel(), dtype=torch.uint8, device=dev)
        d_out = torch.empty_like(d_comp)
        in_bytes, out_bytes = raw_total, comp_total
    d_off_in = torch.from_numpy(c_off if op == "decompress" else batch.offsets).to(dev)
    d_len_in = torch.from_numpy((comp_len if op == "decompress" else batch.lens).view(np.int32)).to(dev)
    d_off_out = torch.from_numpy(batch.offsets if op == "decompress" else c_off).to(dev)
    d_cap = torch.from_numpy(batch.lens.view(np.int32)).to(dev)
    d_ol = torch.empty(n, dtype=torch.int32, device=dev)
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        d_in.copy_(h_in, non_blocking=True)
        e[1].record(stream)
        if op == "decompress":
            codec.decompress(d_in, d_off_in, d_len_in, n, d_out, d_off_out, d_cap, d_ol, d_st, stream=stream,
                             workspace=d_dws)
        else:
            codec.compress(d_in, d_off_in, d_len_in, n, max_len, d_out, d_off_out, d_ol, d_st, stream=stream,
                           workspace=d_ws)
        e[2].record(stream)
        h_out.copy_(d_out[:h_out.numel()], non_blocking=True)
        e[3].record(stream)
        torch.cuda.synchronize()
        ms = [e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3])]
        if best is None or sum(ms) < sum(best):
            best = ms
    # the same H2D timed by the host clock around a synchronize (DESIGN.md
    # section 5: the event-timed figure above reads 24 GB/s in this process)
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_in.copy_(h_in, non_blocking=True)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    # where the slow H2D comes from: the same destination from a pinned buffer
    # filled on the host, and the same source into a fresh device buffer
    def h2d_rate(dst, src):
        bestw = 1e9
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            bestw = min(bestw, time.perf_counter() - t0)
        return round(src.numel() / bestw / 1e9, 2)
    h_fill = torch.empty(h_in.numel(), dtype=torch.uint8, pin_memory=True)
    h_fill.fill_(3)
    d_fresh = torch.empty(h_in.numel(), dtype=torch.uint8, device=dev)
    h2d_diag = {"host_filled_src": h2d_rate(d_in, h_fill), "fresh_dst": h2d_rate(d_fresh, h_in),
                "host_filled_src_fresh_dst": h2d_rate(d_fresh, h_fill),
                # the slow pair itself, timed again after the diagnostic copies
                "same_pair_after": h2d_rate(d_in, h_in)}
    del h_fill, d_fresh
    tot = sum(best) / 1e3
    out = {
        "gib_s_uncompressed": round(raw_total / tot / GIB, 3),
        "h2d_ms": round(best[0], 3), "kernel_ms": round(best[1], 3), "d2h_ms": round(best[2], 3),
        "h2d_gb_s": round(in_bytes / (best[0] / 1e3) / 1e9, 2),
        "h2d_gb_s_host_clock": round(in_bytes / min(walls) / 1e9, 2),
        "h2d_gb_s_diag": h2d_diag,
        "d2h_gb_s": round(out_bytes / (best[2] / 1e3) / 1e9, 2),
        "note": "serial pinned hipMemcpyAsync H2D + kernel + D2H on one stream, no overlap",
    }
    if op == "decompress":
        out["pipelined"] = [end_to_end_pipelined(torch, codec, h_in, h_out, d_in, d_out, c_off, comp_len,
                                                 batch, raw_total, n, dev, chunks=c) for c in (4, 16)]
    return out


def end_to_end_pipelined(torch, codec, h_in, h_out, d_in, d_out, c_off, comp_len, batch, raw_total,
                         n, dev, chunks=16):
    """The same pass cut into message-range chunks: chunk k's H2D, decode and
    D2H go to three streams with event dependencies, so chunk k+1's upload and
    chunk k-1's download overlap chunk k's kernels."""
    bounds = [n * k // chunks for k in range(chunks + 1)]
    s_up, s_k, s_down = (torch.cuda.Stream(device=dev) for _ in range(3))
    d_off_in = torch.from_numpy(c_off).to(dev)
    d_len_in = torch.from_numpy(comp_len.view(np.int32)).to(dev)
    d_off_out = torch.from_numpy(batch.offsets).to(dev)
    d_cap = torch.from_numpy(batch.lens.view(np.int32)).to(dev)
    d_ol = torch.empty(n, dtype=torch.int32, device=dev)
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    c_end = np.append(c_off[1:], np.uint64(d_in.numel())).astype(np.uint64)
    r_end = (batch.offsets.astype(np.uint64) + batch.lens.astype(np.uint64))
    wss = []
    for k in range(chunks):
        a, b = bounds[k], bounds[k + 1]
        wss.append(codec.decompress_workspace(b - a, int(c_end[b - 1] - c_off[a])) if b > a else None)
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record(s_up)
        s_k.wait_event(t0)
        s_down.wait_event(t0)
        for k in range(chunks):
            a, b = bounds[k], bounds[k + 1]
            if b == a:
                continue
            ca, cb = int(c_off[a]), int(c_end[b - 1])
            ra, rb = int(batch.offsets[a]), int(r_end[b - 1])
            with torch.cuda.stream(s_up):
                d_in[ca:cb].copy_(h_in[ca:cb], non_blocking=True)
                up = torch.cuda.Event()
                up.record(s_up)
            s_k.wait_event(up)
            codec.decompress(d_in, d_off_in[a:b], d_len_in[a:b], b - a, d_out, d_off_out[a:b], d_cap[a:b],
                             d_ol[a:b], d_st[a:b], stream=s_k, workspace=wss[k])
            kd = torch.cuda.Event()
            kd.record(s_k)
            s_down.wait_event(kd)
            with torch.cuda.stream(s_down):
                h_out[ra:rb].copy_(d_out[ra:rb], non_blocking=True)
        t1.record(s_down)
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        best = ms if best is None else min(best, ms)
    ok = bool((d_st == 0).all().item())
    return {"gib_s_uncompressed": round(raw_total / (best / 1e3) / GIB, 3), "ms": round(best, 3),
            "chunks": chunks, "status_ok": ok,
            "note": f"{chunks} message-range chunks; H2D / decode / D2H on three streams with event "
                    "dependencies"}


def _cpu_model() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def cpu_baseline(op, batch, d_comp, c_off, comp_len, threads, with_single=True):
    """The reference's own CPU Snappy (oracle/_ref, per-message Source/Sink path with
    8160-byte cord_buf fragments) on a bounded sample of the same workload, timed on
    this host's cores: `threads` (default: the box's share, at most 16), plus a
    1-thread and an nproc-thread figure.  Falls back to the C restatement ("port")
    if _ref is absent."""
    sys.path.insert(0, str(REPO / "oracle"))
    from bind import Oracle, Reference
    affinity = len(os.sched_getaffinity(0))
    nproc = os.cpu_count() or affinity
    nthreads = threads or max(1, min(16, affinity))
    n = len(batch)
    per_msg = batch.total / max(1, n)
    kind = "reference" if Reference.available() else "port"
    eng = Reference() if kind == "reference" else Oracle()
    host_all = None

    def run(nthr, target_bytes, min_wall):
        nonlocal host_all
        m = int(max(1, min(n, target_bytes // max(1, per_msg))))
        lens = batch.lens[:m].copy()
        offs = batch.offsets[:m].copy()
        if host_all is None:
            host_all = d_comp.cpu().numpy()
        host_comp = host_all[: int(c_off[m - 1] + comp_len[m - 1]) + 1]
        clen = comp_len[:m].copy()
        coff = c_off[:m].copy()
        out_len = np.zeros(m, np.uint32)
        passes, dt, ok = 0, 0.0, True
        while passes < 20 and (passes == 0 or dt < min_wall):
            if op == "decompress":
                out = np.zeros(max(1, int(lens.astype(np.uint64).sum())), np.uint8)
                if kind == "reference":
                    dt += eng.batch(1, host_comp, coff, clen, out, offs, lens, out_len, nthr)
                else:
                    st = np.zeros(m, np.int32)
                    dt += eng.uncompress_batch(host_comp, coff, clen, out, offs, lens, out_len, st, nthr)
                nraw = int(lens.astype(np.uint64).sum())
                ok = ok and bool(np.array_equal(out[:nraw], batch.data[:nraw]))
            else:
                caps = np.array([fsg.max_compressed_length(int(x)) for x in lens], np.uint64)
                oo, tot = fsg.slot_offsets(caps)
                out = np.zeros(tot, np.uint8)
                if kind == "reference":
                    dt += eng.batch(0, batch.data, offs, lens, out, oo, None, out_len, nthr)
                else:
                    dt += eng.compress_batch(batch.data, offs, lens, out, oo, out_len, nthr)
                ok = ok and bool(np.array_equal(out_len, clen))
            passes += 1
        raw = int(lens.astype(np.uint64).sum()) * passes
        return raw / dt / GIB, m, raw / passes, passes, dt, ok

    # bounded sample: ~1 GiB of decode work or ~0.25 GiB of encode work per pass
    target = (1 << 30) if op == "decompress" else (1 << 28)
    v, m, raw1, passes, dt, ok = run(nthreads, target, 1.0)
    res = {
        "value": round(v, 3),
        "unit": "GiB/s (uncompressed bytes)",
        "cores": nthreads,
        "kind": kind,
        "sample": f"first {m} messages of the same batch ({raw1 / GIB:.3f} GiB raw) x {passes} "
                  f"passes, {op}, {nthreads} threads x strided messages, 8160-B fragments; wall {dt:.3f} s "
                  f"(~{dt * nthreads:.0f} s of CPU work); output equal to GPU's: {ok}",
        "host": {"cpu_model": _cpu_model(), "nproc": nproc, "affinity_cpus": affinity},
    }
    if with_single:
        v1, m1, raw_s, p1, dt1, ok1 = run(1, target // 16, 1.0)
        res["single_thread"] = {"value": round(v1, 3), "cores": 1,
                                "sample": f"first {m1} messages ({raw_s / GIB:.3f} GiB raw) x {p1} passes, "
                                          f"wall {dt1:.3f} s; output equal: {ok1}"}
        if affinity > nthreads:
            vn, mn, raw_n, pn, dtn, okn = run(affinity, target, 0.5)
            res["all_cpus"] = {"value": round(vn, 3), "cores": affinity,
                               "sample": f"first {mn} messages ({raw_n / GIB:.3f} GiB raw) x {pn} passes, "
                                         f"wall {dtn:.3f} s; output equal: {okn}"}
    return res


def echo_main(args):
    """BASELINE config 1: example/echo over loopback with
    CompressType=snappy, 4 KiB request body, one client thread
    (tools/echo_bench.cc).  `value` = QPS through the drop-in handler (its
    host codec serves 4 KiB bodies: below the runtime's GPU threshold); the
    same harness also runs every body through the GPU ("gpu"), without
    compression ("none", the transport floor), and with the reference's own
    Snappy (cpu_baseline, oracle/_ref loaded by the harness only here)."""
    exe = REPO / "build" / "echo_bench"
    if not exe.exists():
        subprocess.run(["make", "-C", str(REPO), "echobench"], check=True, capture_output=True)
    calls = max(1000, args.steps * 1000)

    def run(codec, n):
        r = subprocess.run([str(exe), "--codec", codec, "--calls", str(n), "--warmup", str(max(100, n // 20))],
                           capture_output=True, text=True, timeout=600, cwd=str(REPO))
        if r.returncode != 0:
            raise RuntimeError(f"echo_bench --codec {codec}: rc {r.returncode}: {r.stdout} {r.stderr[-2000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    main_run = run("runtime", calls)
    # the other codec modes and the reference's Snappy: --full only
    modes = {"gpu": run("gpu", max(1000, calls // 4)), "none": run("none", calls)} if args.full else {}
    base = None
    if args.full and not args.no_cpu_baseline:
        ref = run("reference", calls)
        base = {"value": ref["qps"], "unit": "QPS", "cores": 1, "kind": "reference",
                "sample": f"{ref['calls']} echo calls through the reference's snappy.cc (oracle/_ref) on this "
                          f"host, same harness; p50 {ref['p50_us']} us, p99 {ref['p99_us']} us, codec share "
                          f"{ref['codec_share']}", "p50_us": ref["p50_us"], "p99_us": ref["p99_us"],
                "codec_share": ref["codec_share"], "host": {"cpu_model": _cpu_model(), "nproc": os.cpu_count()}}
    line = {
        "metric": "QPS example/echo over loopback, CompressType=snappy, 4 KiB request body, 1 client thread",
        "value": main_run["qps"], "unit": "QPS", "n_gpus": 1, "steps": main_run["calls"], "warmup": 0,
        "ms_per_step": round(1e3 / main_run["qps"], 4), "higher_is_better": True, "scaling": "none",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic (SURVEY.md §8(d) text generator, body 0, 4,093 B)",
        "config": {"workload": "C1 echo: baidu_std loopback, SNAPPY request and response, 4,096-byte body",
                   "codec": "drop-in handler (host codec below the GPU threshold)"},
        "p50_us": main_run["p50_us"], "p99_us": main_run["p99_us"], "codec_share": main_run["codec_share"],
        "modes": modes, "cpu_baseline": base,
        "correct": {"errors": main_run["errors"] + sum(m["errors"] for m in modes.values()),
                    "server_ok": main_run["server_ok"]},
    }
    print(json.dumps(line))


def main(argv=None):
    args = parse(argv)
    if args.workload == "c1-echo":
        if args.dump_outputs:
            sys.exit("bench.py: --dump-outputs needs a batch workload; c1-echo returns no arrays")
        echo_main(args)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launcher: spawn the ranks before this process touches the GPU
        sys.exit(launch(args.gpus, sys.argv[1:] if argv is None else list(argv)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and "WORLD_SIZE" in os.environ:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; measuring {world} ranks",
              file=sys.stderr)
    rank_main(args)


if __name__ == "__main__":
    main()
