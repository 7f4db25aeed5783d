#!/usr/bin/env python3
"""The NAT-T checksum fix on a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/natt_bench.py [--packets N] [--reps R] [--warmup W] [--lanes 8,16,32] [--out FILE]

N decapsulated transport-mode IPv4 packets (default 2^20) of 1500 bytes at a
1500-byte stride, TCP and UDP alternating, every one of a NAT-T SA and taking
part; one SA, and 1024 SAs interleaved at random.  For both policies it
times, over --reps warmed repetitions in alternation (median, min, max; the
spread is the margin):
  device  espgpu_esp_natt_cksum_batch: HIP events around the call on one
          stream, everything staying in device memory;
  host    the only way without it, end to end on the wall clock: copy the
          packets back, espgpu_esp_natt_cksum per packet on one core
          (tools/natt_walk.c, compiled here), copy them up.
Both produce the same bytes (checked on the first run of each).  For the
recompute policy the achieved bytes/s of segment read stand beside the HBM
peak of the MI355X (8 TB/s), and --lanes repeats it with other lane groups
(set_tuning "natt_lanes").  One line per case; --out also writes them to a
file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

STRIDE, IHL = 1500, 20
HBM_PEAK = 8.0e12


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "natt_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "natt_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.natt_walk.restype = C.c_uint32
    w.natt_walk.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lanes", default="8,16,32")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from espgpu import _lib as L
    from espgpu.batch import DESC_DTYPE, INSA_DTYPE, PKT_DTYPE, esp_natt_cksum
    from espgpu.opencrypto import GpuCryptoDriver
    n = a.packets
    rng = np.random.default_rng(4500)
    walk = build_walk()
    drv = GpuCryptoDriver(max_sessions=8, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    arena = rng.integers(0, 256, n * STRIDE, dtype=np.uint8)
    rows = arena.reshape(n, STRIDE)
    rows[:, 0], rows[:, 2], rows[:, 3] = 0x45, STRIDE >> 8, STRIDE & 0xff
    proto = np.where(np.arange(n) & 1, 17, 6).astype(np.uint8)
    rows[:, 9] = proto
    udp = proto == 17
    rows[udp, IHL + 4], rows[udp, IHL + 5] = (STRIDE - IHL) >> 8, (STRIDE - IHL) & 0xff
    ipkt = np.zeros(n, dtype=PKT_DTYPE)
    ipkt["off4"], ipkt["len"] = np.arange(n, dtype=np.uint64) * (STRIDE // 4), STRIDE
    trailer = (proto.astype(np.uint32) | 0x200 | L.TR_VALID).astype(np.uint32)
    zero = np.zeros(n, dtype=np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()   # noqa: E731
    d_ipkt, d_tr, d_z = up(ipkt), torch.from_numpy(trailer.view(np.int32).copy()).cuda(), up(zero)
    lines = []
    for nsa in (1, 1024):
        insa = np.zeros(nsa, dtype=INSA_DTYPE)
        insa["flags"], insa["pad_"] = L.IN_TRANSPORT | L.IN_NATT, rng.integers(1, 65536, nsa)
        desc = np.zeros(n, dtype=DESC_DTYPE)
        desc["off4"], desc["sa"] = ipkt["off4"], rng.integers(0, nsa, n)
        d_desc, d_in = up(desc), up(insa)
        for policy in (0, 1):
            lanes = [0] + ([int(x) for x in a.lanes.split(",") if x] if policy and nsa == 1 else [])
            for ln in lanes:
                assert drv.set_tuning("natt_lanes", ln) == 0
                d_arena = up(arena)
                cf = np.zeros(n, dtype=np.uint8)
                pin = torch.empty(n * STRIDE, dtype=torch.uint8).pin_memory()
                dev_ms, host_ms = [], []
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for r in range(a.warmup + a.reps):
                    d_arena.copy_(torch.from_numpy(arena))
                    torch.cuda.synchronize()
                    ev0.record()
                    esp_natt_cksum(drv, d_arena, d_ipkt, d_desc, d_tr, d_z, d_z, n, d_in, policy=policy)
                    ev1.record()
                    torch.cuda.synchronize()
                    t_dev = ev0.elapsed_time(ev1)
                    got = d_arena.cpu().numpy() if r == 0 else None
                    # the host's way on the same input
                    d_arena.copy_(torch.from_numpy(arena))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pin.copy_(d_arena)
                    torch.cuda.synchronize()
                    h = pin.numpy()
                    took = walk.natt_walk(insa.ctypes.data, nsa, h.ctypes.data, ipkt.ctypes.data, desc.ctypes.data,
                                          trailer.ctypes.data, zero.ctypes.data, zero.ctypes.data, n, policy,
                                          cf.ctypes.data)
                    d_arena.copy_(pin)
                    torch.cuda.synchronize()
                    t_host = (time.perf_counter() - t0) * 1e3
                    assert took == n
                    if r == 0:
                        assert np.array_equal(got, h), "device and host results differ"
                        assert (got != arena).any()
                    if r >= a.warmup:
                        dev_ms.append(t_dev), host_ms.append(t_host)
                d, h_ = stats(dev_ms), stats(host_ms)
                line = ("natt_cksum n=%d sas=%d policy=%s lanes=%s: device %.3f ms (%.3f..%.3f), host %.1f ms "
                        "(%.1f..%.1f), ratio %.0fx" % (n, nsa, "recompute" if policy else "auto", ln or "default",
                                                       d[0], d[1], d[2], h_[0], h_[1], h_[2], h_[0] / d[0]))
                if policy:
                    bps = n * (STRIDE - IHL) / (d[0] * 1e-3)
                    line += ", %.2f TB/s of segment read (%.0f%% of the 8 TB/s HBM peak)" % (bps / 1e12,
                                                                                          100 * bps / HBM_PEAK)
                print(line, flush=True)
                lines.append(line)
    drv.set_tuning("natt_lanes", 0)
    drv.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
