#!/usr/bin/env python3
"""Inbound classification of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/classify_bench.py [--packets N] [--reps R] [--warmup W] [--out FILE]

Two shapes of N IPv4 ESP packets (default 2^20) of 1500 bytes at a 1500-byte
stride, header checksums verified (ESPGPU_CLS_IPCSUM):
  cfg1  one SA (a table of 2 slots);
  cfg4  1024 SAs interleaved at random (2048 slots).
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin):
  device  espgpu_esp_classify_batch: HIP events around the call on one stream,
          packets, table, descriptors and statuses staying in device memory;
          "warm" repeats the call back to back, so the 2^20 header lines
          (64-128 MiB) come from the 256-MiB last-level cache; "cold" writes a
          1-GiB buffer before each call, outside the timed window, so they
          come from HBM, as for packets that arrived a while ago;
  host    what a caller has without it, end to end on the wall clock: copy
          each packet's first 64 bytes back (a strided device-to-host copy),
          espgpu_esp_classify per packet on one core (tools/classify_walk.c,
          compiled here), copy the descriptors and the status bytes up.  The
          host is taken to know every packet's offset and length already.
Both produce the same descriptors and statuses (checked).  One line per shape
with both times and their ratio; --out also writes them to a file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

STRIDE, HDR = 1500, 64


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "classify_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "classify_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.classify_walk.restype = C.c_uint32
    w.classify_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def headers(spi, dst):
    """n 24-byte IPv4 headers + SPI for packets of STRIDE bytes, checksums right."""
    n = len(spi)
    h = np.zeros((n, 24), dtype=np.uint8)
    h[:, 0], h[:, 2], h[:, 3], h[:, 8], h[:, 9] = 0x45, STRIDE >> 8, STRIDE & 0xff, 64, 50
    h[:, 4:6] = np.arange(n, dtype=np.uint32).astype(">u2").view(np.uint8).reshape(n, 2)      # ip_id
    h[:, 12:16] = (10, 0, 0, 1)
    h[:, 16:20] = dst
    s = h[:, :20].copy().view(">u2").astype(np.uint32).sum(axis=1)
    s = (s & 0xffff) + (s >> 16)
    s = (s & 0xffff) + (s >> 16)
    h[:, 10:12] = (~s & 0xffff).astype(">u2").view(np.uint8).reshape(n, 2)
    h[:, 20:24] = np.asarray(spi, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from espgpu import _lib as L
    from espgpu.batch import DESC_DTYPE, PKT_DTYPE, SAD_DTYPE, esp_classify, sad_build
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "classify_bench needs a GPU"
    walk = build_walk()
    drv = GpuCryptoDriver(device=0, max_sessions=16)          # the classification reads no session
    rng = np.random.default_rng(1)
    maxsa, n, flags = 1024, args.packets, L.CLS_IPCSUM
    ent = np.zeros(maxsa, dtype=SAD_DTYPE)
    ent["spi"], ent["sa"], ent["proto"], ent["af"] = 0x1000 + 7 * np.arange(maxsa), np.arange(maxsa), 50, 4
    ent["salt"] = rng.integers(0, 2**32, maxsa)
    ent["dst"][:, :4] = rng.integers(1, 255, (maxsa, 4))
    pkt = np.zeros(n, dtype=PKT_DTYPE)
    pkt["off4"], pkt["len"] = np.arange(n, dtype=np.int64) * (STRIDE // 4), STRIDE
    stream = torch.cuda.Stream()
    lines = []
    for name, nsa in (("cfg1", 1), ("cfg4", maxsa)):
        table = sad_build(ent[:nsa], 2 * nsa)
        sa_of = np.zeros(n, dtype=np.int64) if nsa == 1 else rng.integers(0, nsa, n)
        hdr = headers(ent["spi"][sa_of], ent["dst"][sa_of, :4])
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
            rows = d_arena.view(n, STRIDE)
            rows[:, :24] = torch.from_numpy(hdr).cuda()
            d_pkt = torch.from_numpy(pkt.view(np.uint8).copy()).cuda()
            d_tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
            d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            d_cst = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            flush = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")
            dev, cold = [], []
            for it in range(2 * (args.warmup + args.reps)):
                if it & 1:
                    flush.fill_(it & 0xff)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                esp_classify(drv, d_arena, d_pkt, n, d_tab, d_desc, d_cst, flags=flags, stream=stream)
                e1.record(stream)
                e1.synchronize()
                if it >= 2 * args.warmup:
                    (cold if it & 1 else dev).append(e0.elapsed_time(e1))
            del flush
            assert not d_cst.any().item(), "every packet must be accepted"
            dev_desc = d_desc.cpu().numpy().copy()
            want = dev_desc.view(DESC_DTYPE)
            assert np.array_equal(want["sa"], sa_of) and (want["len"] == STRIDE - 20).all()
            # host: D2H of the header bytes, the walk, H2D of descriptors and statuses
            h_hdr = torch.empty((n, HDR), dtype=torch.uint8).pin_memory()
            h_desc = torch.zeros(n * 16, dtype=torch.uint8).pin_memory()
            h_cst = torch.zeros(n, dtype=torch.uint8).pin_memory()
            host, walk_only = [], []
            for it in range(args.warmup + args.reps):
                d_desc.zero_()
                stream.synchronize()
                t0 = time.perf_counter()
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                ok = walk.classify_walk(table.ctypes.data, len(table), h_hdr.data_ptr(), pkt.ctypes.data, n, flags,
                                        h_desc.data_ptr(), h_cst.data_ptr())
                t2 = time.perf_counter()
                d_desc.copy_(h_desc, non_blocking=True)
                d_cst.copy_(h_cst, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                assert ok == n
                if it >= args.warmup:
                    host.append((t3 - t0) * 1e3)
                    walk_only.append((t2 - t1) * 1e3)
            assert np.array_equal(d_desc.cpu().numpy(), dev_desc), "host and device descriptors differ"
            assert not d_cst.any().item()
            del d_arena, rows
        (dm, dlo, dhi), (cm, clo, chi), (hm, hlo, hhi), (wm, _, _) = stats(dev), stats(cold), stats(host), stats(walk_only)
        lines.append("%s n=%d sas=%d  device warm %.3f ms (min %.3f max %.3f) cold %.3f ms (min %.3f max %.3f)  "
                     "host %.3f ms (min %.3f max %.3f; walk alone %.3f ms)  host/device cold %.2f warm %.2f  "
                     "reps=%d warmup=%d"
                     % (name, n, nsa, dm, dlo, dhi, cm, clo, chi, hm, hlo, hhi, wm, hm / cm, hm / dm, args.reps,
                        args.warmup))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    drv.close()


if __name__ == "__main__":
    main()
