#!/usr/bin/env python3
"""The two inbound AH stages of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/ah_in_bench.py [--packets N] [--reps R] [--warmup W] [--out FILE]

N IPv4 AH packets (default 2^20) of 1500 bytes at a 1500-byte stride, 20-byte
headers, HMAC-SHA2-256-128 sessions (ahsize 28), transport mode with next
header 6, every one accepted; one SA, and 1024 SAs interleaved at random.
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin), both stages:
  device  espgpu_ah_input_batch, and espgpu_ah_decap_batch on its result: HIP
          events around the whole call on one stream, everything staying in
          device memory;
  host    what a caller has without them, end to end on the wall clock: copy
          the descriptors (for the second stage the statuses too) and each
          packet's first 64 bytes back (a strided device-to-host copy),
          espgpu_ah_input / espgpu_ah_decap per packet on one core
          (tools/ah_in_walk.c, compiled here), copy the 64 bytes and the
          stage's results up.  The save slots stay on the host between the two
          stages, which favours the host.
Both produce the same headers, descriptors, records, statuses and counters
(checked on the first run of each).  One line per shape and stage with both
times and their ratio; --out also writes them to a file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

STRIDE, HDR, SKIP, MLEN, AHSIZE = 1500, 64, 20, 16, 28
Q = STRIDE - SKIP - AHSIZE


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "ah_in_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "ah_in_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.ah_input_walk.restype = w.ah_decap_walk.restype = C.c_uint32
    w.ah_input_walk.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_void_p]
    w.ah_decap_walk.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 3
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def headers(n):
    """n packet fronts of HDR bytes: a 20-byte IPv4 header (checksum right) and
    the AH header of an HMAC-SHA2-256-128 SA in front of a TCP segment."""
    h = np.zeros((n, HDR), dtype=np.uint8)
    h[:, 0], h[:, 1], h[:, 2], h[:, 3], h[:, 8], h[:, 9] = 0x45, 0x10, STRIDE >> 8, STRIDE & 0xff, 64, 51
    h[:, 4:6] = np.arange(n, dtype=np.uint32).astype(">u2").view(np.uint8).reshape(n, 2)      # ip_id
    h[:, 12:16], h[:, 16:20] = (10, 0, 0, 1), (10, 0, 0, 2)
    s = h[:, :SKIP].copy().view(">u2").astype(np.uint32).sum(axis=1)
    s = (s & 0xffff) + (s >> 16)
    s = (s & 0xffff) + (s >> 16)
    h[:, 10:12] = (~s & 0xffff).astype(">u2").view(np.uint8).reshape(n, 2)
    h[:, SKIP], h[:, SKIP + 1] = 6, (AHSIZE - 8) // 4
    h[:, SKIP + 8:SKIP + 12] = np.arange(1, n + 1, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.warmup = max(args.warmup, 1)                  # the first run is the checked one, not a timed one
    import torch
    from espgpu import _lib as L
    from espgpu.ah import AH_SHA256, AhSecAssoc
    from espgpu.batch import DESC_DTYPE, INSA_DTYPE, PKT_DTYPE, ah_decap, ah_input
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "ah_in_bench needs a GPU"
    walk = build_walk()
    rng = np.random.default_rng(1)
    maxsa, n = 1024, args.packets
    drv = GpuCryptoDriver(device=0, max_sessions=maxsa)
    for k in range(maxsa):
        rc, sid = drv.newsession(AhSecAssoc(0x1000 + k, AH_SHA256, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()).csp())
        assert rc == 0 and sid == k
    mlens = np.full(maxsa, MLEN, dtype=np.uint32)
    off4 = np.arange(n, dtype=np.int64) * (STRIDE // 4)
    hdr = headers(n)
    stream = torch.cuda.Stream()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    lines = []
    for name, nsa in (("one-sa", 1), ("1024-sa", maxsa)):
        desc = np.zeros(n, dtype=DESC_DTYPE)
        desc["off4"], desc["len"], desc["salt"] = off4, STRIDE, SKIP + 12
        desc["sa"] = 0 if nsa == 1 else rng.integers(0, nsa, n)
        status = np.zeros(n, dtype=np.uint8)
        insa = np.zeros(maxsa, dtype=INSA_DTYPE)
        insa["flags"] = L.IN_AH | L.IN_TRANSPORT
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
            rows = d_arena.view(n, STRIDE)
            d_hdr0 = torch.from_numpy(hdr).cuda()
            d_desc0, d_st, d_in = up(desc), up(status), up(insa)
            d_desc = d_desc0.clone()
            d_hs = torch.zeros(n * HDR, dtype=torch.uint8, device="cuda")
            d_ast = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
            d_dst = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            dev_in, dev_dc = [], []
            for it in range(args.warmup + args.reps):
                rows[:, :HDR] = d_hdr0                 # the packets as they arrived
                d_desc.copy_(d_desc0)
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(stream)
                ah_input(drv, d_arena, d_desc, n, d_in, d_hs, d_ast, stream=stream)
                e1.record(stream)
                if it == 0:
                    e1.synchronize()
                    first_in = (rows[:, :HDR].cpu().numpy().copy(), d_hs.cpu().numpy().copy())
                    assert not d_ast.any().item(), "every packet must be accepted"
                ah_decap(drv, d_arena, d_desc, d_st, n, d_in, d_hs, d_ipkt, d_dst, stream=stream)
                e2.record(stream)
                e2.synchronize()
                if it == 0:
                    first = (d_ipkt.cpu().numpy().copy(), rows[:, :HDR].cpu().numpy().copy(),
                             d_in.cpu().numpy().view(INSA_DTYPE).copy())
                    assert not d_dst.any().item(), "every packet must be accepted"
                if it >= args.warmup:
                    dev_in.append(e0.elapsed_time(e1))
                    dev_dc.append(e1.elapsed_time(e2))
            got = first[0].view(PKT_DTYPE)
            assert np.array_equal(got["off4"], off4 + AHSIZE // 4) and (got["len"] == SKIP + Q).all()
            assert int(first[2]["packets"].sum()) == n and int(first[2]["bytes"].sum()) == n * (SKIP + Q)
            assert np.array_equal(first_in[1].reshape(n, HDR)[:, :SKIP], hdr[:, :SKIP])
            # host: D2H of descriptors (statuses) and header bytes, the walk, H2D of the results
            d_in.copy_(up(insa))
            h_hdr = torch.empty((n, HDR), dtype=torch.uint8).pin_memory()
            h_desc = torch.zeros(n * 16, dtype=torch.uint8).pin_memory()
            h_st = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_ast = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_ipkt = torch.zeros(n * 8, dtype=torch.uint8).pin_memory()
            h_dst = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_in = torch.from_numpy(insa.view(np.uint8).copy()).pin_memory()
            h_hs = np.zeros(n * HDR, dtype=np.uint8)
            host_in, host_dc, walk_in, walk_dc = [], [], [], []
            for it in range(args.warmup + args.reps):
                rows[:, :HDR] = d_hdr0
                d_desc.copy_(d_desc0)
                stream.synchronize()
                t0 = time.perf_counter()
                h_desc.copy_(d_desc, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                ok = walk.ah_input_walk(h_in.data_ptr(), maxsa, mlens.ctypes.data, h_hdr.data_ptr(), h_desc.data_ptr(), n,
                                        h_hs.ctypes.data, h_ast.data_ptr())
                t2 = time.perf_counter()
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_desc.copy_(h_desc, non_blocking=True)
                d_ast.copy_(h_ast, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                assert ok == n
                if it == 0:
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first_in[0]), "massaged headers differ"
                    assert np.array_equal(h_hs.reshape(n, HDR)[:, :SKIP], hdr[:, :SKIP]), "saved headers differ"
                t4 = time.perf_counter()
                h_desc.copy_(d_desc, non_blocking=True)
                h_st.copy_(d_st, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t5 = time.perf_counter()
                ok = walk.ah_decap_walk(h_in.data_ptr(), maxsa, mlens.ctypes.data, h_hdr.data_ptr(), h_desc.data_ptr(),
                                        h_st.data_ptr(), n, h_hs.ctypes.data, h_ipkt.data_ptr(), h_dst.data_ptr())
                t6 = time.perf_counter()
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_ipkt.copy_(h_ipkt, non_blocking=True)
                d_dst.copy_(h_dst, non_blocking=True)
                d_in.copy_(h_in, non_blocking=True)
                stream.synchronize()
                t7 = time.perf_counter()
                assert ok == n
                if it == 0:
                    assert np.array_equal(d_ipkt.cpu().numpy(), first[0]), "host and device records differ"
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first[1]), "host and device headers differ"
                    assert np.array_equal(d_in.cpu().numpy().view(INSA_DTYPE), first[2]), "counters differ"
                    assert not d_dst.any().item()
                if it >= args.warmup:
                    host_in.append((t3 - t0) * 1e3)
                    walk_in.append((t2 - t1) * 1e3)
                    host_dc.append((t7 - t4) * 1e3)
                    walk_dc.append((t6 - t5) * 1e3)
            del d_arena, rows
        for stage, dev, host, wk in (("ah_input", dev_in, host_in, walk_in), ("ah_decap", dev_dc, host_dc, walk_dc)):
            (dm, dlo, dhi), (hm, hlo, hhi), (wm, _, _) = stats(dev), stats(host), stats(wk)
            lines.append("%-8s %-8s n=%d sas=%d  device %.3f ms (min %.3f max %.3f)  host %.3f ms (min %.3f max %.3f; "
                         "walk alone %.3f ms)  host/device %.1f  reps=%d warmup=%d"
                         % (name, stage, n, nsa, dm, dlo, dhi, hm, hlo, hhi, wm, hm / dm, args.reps, args.warmup))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    drv.close()


if __name__ == "__main__":
    main()
