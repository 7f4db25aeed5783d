#!/usr/bin/env python3
"""Outbound framing of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/frame_bench.py [--records N] [--reps R] [--warmup W] [--out FILE]

Two shapes of N AES-GCM records (default 2^20) of 1460 payload bytes at a
1500-byte stride:
  cfg1  one SA;
  cfg4  1024 SAs interleaved at random.
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin), each starting from the same counters:
  device  espgpu_esp_frame_batch: HIP events around the call on one stream,
          counters, descriptors and records staying in device memory;
  host    what a caller has without it, end to end on the wall clock: copy
          the descriptors and frame words back, espgpu_esp_frame per record
          in arrival order on one core (tools/frame_walk.c, compiled here),
          copy the descriptors, the status bytes and a 40-byte slot of header
          and trailer bytes per record up again.  Placing those bytes into the
          records would take a kernel of the caller's own, which is not
          counted: that favours this side.
Both produce the same counters and descriptors (checked), and the same header
and trailer bytes in a sample of records.  One line per shape with both times
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
STRIDE, RLEN, SLOT = 1500, 1460, 40


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "frame_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "frame_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.frame_walk.restype = C.c_uint32
    w.frame_walk.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32]
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
    from espgpu import _lib as L
    from espgpu.batch import OUTSA_DTYPE, esp_frame
    from espgpu.esp import GCM, SecAssoc, esp_frame_shape
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "frame_bench needs a GPU"
    walk = build_walk()
    maxsa = 1024
    drv = GpuCryptoDriver(device=0, max_sessions=maxsa)
    rng = np.random.default_rng(1)
    flags = L.OUT_ESN | L.OUT_PAD_SEQ
    out_all = np.zeros(maxsa, dtype=OUTSA_DTYPE)
    for k in range(maxsa):
        sa = SecAssoc(0x1000 + k, GCM, rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), esn=True)
        rc, sid = drv.newsession(sa.csp())
        assert rc == 0 and sid == k
        out_all[k] = (k, 7 * k, sa.spi, int.from_bytes(sa.salt, "little"), flags, 0)
    shape = esp_frame_shape(sa, flags)
    shapes = (L.EShape * maxsa)(*[shape] * maxsa)
    n = args.records
    reclen = 8 + shape.ivlen + RLEN + (((shape.blks - ((RLEN + 2) % shape.blks)) % shape.blks) + 2) + shape.alen
    assert reclen <= STRIDE
    stream = torch.cuda.Stream()
    lines = []
    for name, nsa in (("cfg1", 1), ("cfg4", maxsa)):
        sa_of = np.zeros(n, dtype=np.uint16) if nsa == 1 else rng.integers(0, nsa, n).astype(np.uint16)
        desc = np.zeros(n, dtype=DESC)
        desc["off4"], desc["len"], desc["sa"] = np.arange(n, dtype=np.int64) * (STRIDE // 4), reclen, sa_of
        frame = np.full(n, RLEN | (4 << 16), dtype=np.uint32)
        outsa = out_all[:nsa]
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE + 64, dtype=torch.uint8, device="cuda")
            desc0 = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
            out0 = torch.from_numpy(outsa.view(np.uint8).copy()).cuda()
            d_frame = torch.from_numpy(frame.view(np.int32).copy()).cuda()
            d_desc, d_out = desc0.clone(), out0.clone()
            d_fst = torch.zeros(n, dtype=torch.uint8, device="cuda")
            dev = []
            for it in range(args.warmup + args.reps):
                d_desc.copy_(desc0)
                d_out.copy_(out0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                esp_frame(drv, d_arena, d_desc, d_frame, n, d_out, d_fst, stream=stream)
                e1.record(stream)
                e1.synchronize()
                if it >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
            assert not d_fst.any().item(), "every record must be accepted"
            dev_desc, dev_out = d_desc.cpu().numpy().copy(), d_out.cpu().numpy().copy()
            # host: D2H descriptors + frame words, the walk, H2D descriptors, status and the byte slots
            h_desc = torch.empty(n * 16, dtype=torch.uint8).pin_memory()
            h_frame = torch.empty(n, dtype=torch.int32).pin_memory()
            h_stage = torch.zeros(n * SLOT, dtype=torch.uint8).pin_memory()
            h_fst = torch.zeros(n, dtype=torch.uint8).pin_memory()
            d_stage = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
            host, walk_only = [], []
            for it in range(args.warmup + args.reps):
                d_desc.copy_(desc0)
                h_out = outsa.copy()                 # (the counters live on the host in this design)
                stream.synchronize()
                t0 = time.perf_counter()
                h_desc.copy_(d_desc, non_blocking=True)
                h_frame.copy_(d_frame, non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                refused = walk.frame_walk(h_out.ctypes.data, nsa, C.addressof(shapes), h_desc.data_ptr(),
                                          h_frame.data_ptr(), h_stage.data_ptr(), h_fst.data_ptr(), n)
                t2 = time.perf_counter()
                d_desc.copy_(h_desc, non_blocking=True)
                d_fst.copy_(h_fst, non_blocking=True)
                d_stage.copy_(h_stage, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                assert refused == 0
                if it >= args.warmup:
                    host.append((t3 - t0) * 1e3)
                    walk_only.append((t2 - t1) * 1e3)
            assert np.array_equal(d_desc.cpu().numpy(), dev_desc), "host and device descriptors differ"
            assert np.array_equal(h_out.view(np.uint8), dev_out), "host and device counters differ"
            stage = h_stage.numpy().reshape(n, SLOT)
            for i in rng.integers(0, n, 256):
                rec = d_arena[i * STRIDE:i * STRIDE + reclen].cpu().numpy()
                assert np.array_equal(rec[:16], stage[i, :16]) and np.array_equal(
                    rec[16 + RLEN:reclen - shape.alen], stage[i, 16:16 + reclen - shape.alen - 16 - RLEN]), i
            del d_arena
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
