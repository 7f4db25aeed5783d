#!/usr/bin/env python3
"""Inbound decapsulation of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/decap_bench.py [--packets N] [--reps R] [--warmup W] [--out FILE]

Four shapes of N decrypted IPv4 ESP packets (default 2^20) of 1500 bytes at a
1500-byte stride, AES-GCM-16 sessions (hlen 16, alen 16), every one accepted:
  one SA and 1024 SAs interleaved at random, each in tunnel mode (next header
  4: nothing of the packet is touched) and in transport mode (next header 6:
  the 20-byte header moves 16 bytes forward, fixed).
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin):
  device  espgpu_esp_decap_batch in place: HIP events around the whole call on
          one stream, everything staying in device memory;
  host    what a caller has without it, end to end on the wall clock: copy the
          descriptors, statuses, trailer words and each packet's first 64
          bytes back (a strided device-to-host copy), espgpu_esp_decap per
          packet on one core (tools/decap_walk.c, compiled here), copy the 64
          bytes, the resulting espgpu_pkt records, the status bytes and the
          SA counters up.
Both produce the same records, statuses, headers and counters (checked on the
first run of each).  One line per shape with both times and their ratio;
--out also writes them to a file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

STRIDE, HDR, SKIP, HLEN, ALEN, PADLEN = 1500, 64, 20, 16, 16, 2
Q = STRIDE - SKIP - HLEN - ALEN - PADLEN - 2


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "decap_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "decap_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.decap_walk.restype = C.c_uint32
    w.decap_walk.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_void_p]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def headers(n):
    """n 20-byte IPv4 headers of ESP packets of STRIDE bytes, checksums right."""
    h = np.zeros((n, SKIP), dtype=np.uint8)
    h[:, 0], h[:, 2], h[:, 3], h[:, 8], h[:, 9] = 0x45, STRIDE >> 8, STRIDE & 0xff, 64, 50
    h[:, 4:6] = np.arange(n, dtype=np.uint32).astype(">u2").view(np.uint8).reshape(n, 2)      # ip_id
    h[:, 12:16], h[:, 16:20] = (10, 0, 0, 1), (10, 0, 0, 2)
    s = h.copy().view(">u2").astype(np.uint32).sum(axis=1)
    s = (s & 0xffff) + (s >> 16)
    s = (s & 0xffff) + (s >> 16)
    h[:, 10:12] = (~s & 0xffff).astype(">u2").view(np.uint8).reshape(n, 2)
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
    from espgpu.batch import DESC_DTYPE, INSA_DTYPE, PKT_DTYPE, esp_decap
    from espgpu.esp import GCM, SecAssoc
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "decap_bench needs a GPU"
    walk = build_walk()
    rng = np.random.default_rng(1)
    maxsa, n = 1024, args.packets
    drv = GpuCryptoDriver(device=0, max_sessions=maxsa)
    for k in range(maxsa):
        rc, sid = drv.newsession(SecAssoc(0x1000 + k, GCM, rng.integers(0, 256, 20, dtype=np.uint8).tobytes()).csp())
        assert rc == 0 and sid == k
    shapes = (L.EShape * maxsa)(*[L.EShape(HLEN - 8, 4, ALEN)] * maxsa)
    pkt = np.zeros(n, dtype=PKT_DTYPE)
    pkt["off4"], pkt["len"] = np.arange(n, dtype=np.int64) * (STRIDE // 4), STRIDE
    hdr = headers(n)
    stream = torch.cuda.Stream()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    lines = []
    for name, nsa, mode, nxt in (("one-sa tunnel", 1, L.IN_TUNNEL, 4), ("one-sa transport", 1, L.IN_TRANSPORT, 6),
                                 ("1024-sa tunnel", maxsa, L.IN_TUNNEL, 4),
                                 ("1024-sa transport", maxsa, L.IN_TRANSPORT, 6)):
        desc = np.zeros(n, dtype=DESC_DTYPE)
        desc["off4"], desc["len"] = pkt["off4"] + SKIP // 4, STRIDE - SKIP
        desc["sa"] = 0 if nsa == 1 else rng.integers(0, nsa, n)
        trailer = np.full(n, nxt | PADLEN << 8 | L.TR_VALID, dtype=np.uint32)
        status = np.zeros(n, dtype=np.uint8)
        insa = np.zeros(maxsa, dtype=INSA_DTYPE)
        insa["flags"] = mode
        w_off, w_len = ((SKIP + HLEN) // 4, Q) if mode == L.IN_TUNNEL else (HLEN // 4, SKIP + Q)
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
            rows = d_arena.view(n, STRIDE)
            d_hdr0 = torch.from_numpy(hdr).cuda()
            rows[:, :SKIP] = d_hdr0
            d_pkt, d_desc, d_st, d_in = up(pkt), up(desc), up(status), up(insa)
            d_tr = torch.from_numpy(trailer.view(np.int32).copy()).cuda()
            d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
            d_dst = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            dev = []
            for it in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                esp_decap(drv, d_arena, d_arena, d_pkt, d_desc, d_tr, d_st, n, d_in, d_ipkt, d_dst, stream=stream)
                e1.record(stream)
                e1.synchronize()
                if it == 0:                       # the first run's results, from the packets as they arrived
                    first = (d_ipkt.cpu().numpy().copy(), rows[:, :HDR].cpu().numpy().copy(),
                             d_in.cpu().numpy().view(INSA_DTYPE).copy())
                    assert not d_dst.any().item(), "every packet must be accepted"
                if it >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            got = first[0].view(PKT_DTYPE)
            assert np.array_equal(got["off4"], pkt["off4"] + w_off) and (got["len"] == w_len).all()
            assert int(first[2]["packets"].sum()) == n and int(first[2]["bytes"].sum()) == n * w_len
            # host: D2H of descriptors, statuses, trailer words and header bytes, the walk, H2D of the results
            rows[:, :HDR] = 0
            rows[:, :SKIP] = d_hdr0
            d_in.copy_(up(insa))
            h_hdr = torch.empty((n, HDR), dtype=torch.uint8).pin_memory()
            h_desc = torch.zeros(n * 16, dtype=torch.uint8).pin_memory()
            h_st = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_tr = torch.zeros(n, dtype=torch.int32).pin_memory()
            h_ipkt = torch.zeros(n * 8, dtype=torch.uint8).pin_memory()
            h_dst = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_in = torch.from_numpy(insa.view(np.uint8).copy()).pin_memory()
            host, walk_only = [], []
            for it in range(args.warmup + args.reps):
                stream.synchronize()
                t0 = time.perf_counter()
                h_desc.copy_(d_desc, non_blocking=True)
                h_st.copy_(d_st, non_blocking=True)
                h_tr.copy_(d_tr, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                ok = walk.decap_walk(h_in.data_ptr(), maxsa, C.addressof(shapes), h_hdr.data_ptr(), pkt.ctypes.data,
                                     h_desc.data_ptr(), h_tr.data_ptr(), h_st.data_ptr(), n, h_ipkt.data_ptr(),
                                     h_dst.data_ptr())
                t2 = time.perf_counter()
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_ipkt.copy_(h_ipkt, non_blocking=True)
                d_dst.copy_(h_dst, non_blocking=True)
                d_in.copy_(h_in, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                assert ok == n
                if it == 0:
                    assert np.array_equal(d_ipkt.cpu().numpy(), first[0]), "host and device records differ"
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first[1]), "host and device headers differ"
                    assert np.array_equal(d_in.cpu().numpy().view(INSA_DTYPE), first[2]), "counters differ"
                    assert not d_dst.any().item()
                if it >= args.warmup:
                    host.append((t3 - t0) * 1e3)
                    walk_only.append((t2 - t1) * 1e3)
            del d_arena, rows
        (dm, dlo, dhi), (hm, hlo, hhi), (wm, _, _) = stats(dev), stats(host), stats(walk_only)
        lines.append("%-17s n=%d sas=%d  device %.3f ms (min %.3f max %.3f)  host %.3f ms (min %.3f max %.3f; "
                     "walk alone %.3f ms)  host/device %.1f  reps=%d warmup=%d"
                     % (name, n, nsa, dm, dlo, dhi, hm, hlo, hhi, wm, hm / dm, args.reps, args.warmup))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    drv.close()


if __name__ == "__main__":
    main()
