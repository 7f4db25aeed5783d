#!/usr/bin/env python3
"""The replay-window update of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/replay_bench.py [--records N] [--reps R] [--warmup W] [--out FILE]

Two shapes of N authenticated records (default 2^20) with their sequence
numbers in order per SA:
  cfg1  one SA;
  cfg4  1024 SAs interleaved at random.
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin), each starting from the same windows:
  device  espgpu_replay_update_batch: HIP events around the call on one
          stream, windows and bitmaps staying in device memory;
  host    what a caller has without it, end to end on the wall clock: copy
          d_status and the descriptors back, espgpu_replay_update per record
          in arrival order on one core (tools/replay_walk.c, compiled here),
          copy the windows and bitmaps up again.  The sequence numbers are
          taken as already on the host, which favours this side.
Both produce the same windows (checked).  One line per shape with both times
and their ratio; --out also writes them to a file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

DESC = np.dtype([("off4", "<u4"), ("len", "<u2"), ("sa", "<u2"), ("esn_hi", "<u4"), ("salt", "<u4")])
WSIZE, WORDS = 32, 16          # a 256-packet window, bitmap sized as key.c does


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "replay_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "replay_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.replay_walk.restype = C.c_uint32
    w.replay_walk.argtypes = [C.c_void_p] + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from espgpu.batch import REPLAY_DTYPE, replay_update
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "replay_bench needs a GPU"
    walk = build_walk()
    drv = GpuCryptoDriver(device=0, max_sessions=64)
    n = args.records
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    lines = []
    for name, nsa in (("cfg1", 1), ("cfg4", 1024)):
        sa = np.zeros(n, dtype=np.uint16) if nsa == 1 else rng.integers(0, nsa, n).astype(np.uint16)
        seq = np.zeros(n, dtype=np.uint32)
        for s in range(nsa):                            # in order per SA, from 1
            at = np.flatnonzero(sa == s)
            seq[at] = 1 + np.arange(at.size)
        arena = np.zeros(n * 16 + 64, dtype=np.uint8)
        for k in range(4):
            arena[np.arange(n) * 16 + 4 + k] = (seq >> (24 - 8 * k)) & 0xFF
        desc = np.zeros(n, dtype=DESC)
        desc["off4"], desc["len"], desc["sa"] = np.arange(n) * 4, 16, sa
        tab = np.zeros(nsa, dtype=REPLAY_DTYPE)
        tab["wsize"], tab["bitmap_size"], tab["bitmap_off"] = WSIZE, WORDS, np.arange(nsa) * WORDS
        words = np.zeros(nsa * WORDS, dtype=np.uint32)
        with torch.cuda.stream(stream):
            d_arena = torch.from_numpy(arena).cuda()
            d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
            d_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_ust = torch.zeros(n, dtype=torch.uint8, device="cuda")
            tab0 = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
            words0 = torch.from_numpy(words.view(np.int32).copy()).cuda()
            d_tab, d_words = tab0.clone(), words0.clone()
            dev = []
            for it in range(args.warmup + args.reps):
                d_tab.copy_(tab0)
                d_words.copy_(words0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                replay_update(drv, d_arena, d_desc, n, d_status, d_tab, d_words, d_ust, stream=stream)
                e1.record(stream)
                e1.synchronize()
                if it >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            assert not d_ust.any().item(), "in-order records must all be accepted"
            dev_tab, dev_words = d_tab.cpu().numpy().copy(), d_words.cpu().numpy().copy()
            # host: D2H status + descriptors, the walk, H2D windows
            h_status = torch.empty(n, dtype=torch.uint8).pin_memory()
            h_desc = torch.empty(n * 16, dtype=torch.uint8).pin_memory()
            h_tab = torch.empty(tab0.numel(), dtype=torch.uint8).pin_memory()
            h_words = torch.empty(words0.numel(), dtype=torch.int32).pin_memory()
            h_ust = np.zeros(n, dtype=np.uint8)
            host, walk_only = [], []
            for it in range(args.warmup + args.reps):
                h_tab.copy_(tab0)
                h_words.copy_(words0)
                stream.synchronize()
                t0 = time.perf_counter()
                h_status.copy_(d_status, non_blocking=True)
                h_desc.copy_(d_desc, non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                refused = walk.replay_walk(h_tab.data_ptr(), nsa, h_words.data_ptr(), h_desc.data_ptr(),
                                           seq.ctypes.data, h_status.data_ptr(), h_ust.ctypes.data, n)
                t2 = time.perf_counter()
                d_tab.copy_(h_tab, non_blocking=True)
                d_words.copy_(h_words, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                assert refused == 0
                if it >= args.warmup:
                    host.append((t3 - t0) * 1e3)
                    walk_only.append((t2 - t1) * 1e3)
            assert np.array_equal(d_tab.cpu().numpy(), dev_tab) and np.array_equal(d_words.cpu().numpy(), dev_words), \
                "host and device windows differ"
        (dm, dlo, dhi), (hm, hlo, hhi), (wm, _, _) = stats(dev), stats(host), stats(walk_only)
        lines.append("%s n=%d sas=%d  device %.3f ms (min %.3f max %.3f)  host %.3f ms (min %.3f max %.3f; "
                     "walk alone %.3f ms)  host/device %.2f  reps=%d warmup=%d"
                     % (name, n, nsa, dm, dlo, dhi, hm, hlo, hhi, wm, hm / dm, args.reps, args.warmup))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    drv.close()


if __name__ == "__main__":
    main()
