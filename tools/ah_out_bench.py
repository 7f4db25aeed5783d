#!/usr/bin/env python3
"""The three outbound AH stages of a device-resident batch, device against
host (measurement only; needs a GPU, no fallback).

  python tools/ah_out_bench.py [--packets N] [--reps R] [--warmup W] [--out FILE]

N cleartext IPv4 packets (default 2^20) whose wire form has 1500 bytes, at a
1500-byte stride: 28 bytes of headroom, a 20-byte header, a TCP segment;
HMAC-SHA2-256-128 sessions (ahsize 28), transport mode, every one accepted; one
SA, and 1024 SAs interleaved at random.  For each it times, over --reps warmed
repetitions (median, min, max; the spread is the margin), the three stages:
  device  espgpu_ah_encap_batch, espgpu_ah_frame_batch and espgpu_ah_sent_batch
          (on the statuses of a batch that went through): HIP events around
          each call on one stream, everything staying in device memory;
  host    what a caller has without them, end to end on the wall clock: copy
          the stage's inputs and the first 64 bytes of each span back (a
          strided device-to-host copy), espgpu_ah_encap / espgpu_ah_frame /
          espgpu_ah_sent per packet on one core (tools/ah_out_walk.c, compiled
          here), copy the 64 bytes and the stage's results up.  The save slots
          and the SA tables stay on the host between the stages, which favours
          the host.
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
LEN = STRIDE - AHSIZE


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "ah_out_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "ah_out_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    w.ah_encap_walk.restype = w.ah_frame_walk.restype = w.ah_sent_walk.restype = u32
    w.ah_encap_walk.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp]
    w.ah_frame_walk.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp]
    w.ah_sent_walk.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def fronts(n):
    """n span fronts of HDR bytes: 28 bytes of headroom, then a 20-byte IPv4
    header (checksum right) in front of a TCP segment."""
    h = np.zeros((n, HDR), dtype=np.uint8)
    h[:, :AHSIZE] = 0xEE
    p = h[:, AHSIZE:]
    p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 8], p[:, 9] = 0x45, 0x10, LEN >> 8, LEN & 0xff, 64, 6
    p[:, 4:6] = np.arange(n, dtype=np.uint32).astype(">u2").view(np.uint8).reshape(n, 2)      # ip_id
    p[:, 12:16], p[:, 16:20] = (10, 0, 0, 1), (10, 0, 0, 2)
    s = p[:, :SKIP].copy().view(">u2").astype(np.uint32).sum(axis=1)
    s = (s & 0xffff) + (s >> 16)
    s = (s & 0xffff) + (s >> 16)
    p[:, 10:12] = (~s & 0xffff).astype(">u2").view(np.uint8).reshape(n, 2)
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
    from espgpu.batch import ENCSA_DTYPE, OUTSA_DTYPE, PKT_DTYPE, ah_encap, ah_frame, ah_sent
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "ah_out_bench needs a GPU"
    walk = build_walk()
    rng = np.random.default_rng(1)
    maxsa, n = 1024, args.packets
    drv = GpuCryptoDriver(device=0, max_sessions=maxsa)
    for k in range(maxsa):
        rc, sid = drv.newsession(AhSecAssoc(0x1000 + k, AH_SHA256, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()).csp())
        assert rc == 0 and sid == k
    mlens = np.full(maxsa, MLEN, dtype=np.uint32)
    base4 = (np.arange(n, dtype=np.int64) * (STRIDE // 4)).astype(np.uint32)
    hdr = fronts(n)
    stream = torch.cuda.Stream()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()     # noqa: E731
    pin = lambda k: torch.zeros(k, dtype=torch.uint8).pin_memory()                            # noqa: E731
    lines = []
    for name, nsa in (("one-sa", 1), ("1024-sa", maxsa)):
        rec = np.zeros(n, dtype=PKT_DTYPE)
        rec["off4"], rec["len"] = base4 + AHSIZE // 4, LEN
        sa = (np.zeros(n) if nsa == 1 else rng.integers(0, nsa, n)).astype(np.uint16)
        enc = np.zeros(maxsa, dtype=ENCSA_DTYPE)
        enc["flags"], enc["ttl"] = L.ENC_AH, 64
        enc["src"][:, :4], enc["dst"][:, :4] = (10, 0, 0, 1), (10, 0, 0, 2)
        outsa = np.zeros(maxsa, dtype=OUTSA_DTYPE)
        outsa["spi"] = 0x1000 + np.arange(maxsa)
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
            rows = d_arena.view(n, STRIDE)
            d_hdr0 = torch.from_numpy(hdr).cuda()
            d_rec, d_sa, d_st = up(rec), up(sa), torch.zeros(n, dtype=torch.uint8, device="cuda")
            d_enc, d_out = up(enc), up(outsa)
            d_enc0, d_out0 = d_enc.clone(), d_out.clone()
            d_hs = torch.zeros(n * HDR, dtype=torch.uint8, device="cuda")
            d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
            d_est, d_fst, d_sst = (torch.full((n,), 0x77, dtype=torch.uint8, device="cuda") for _ in range(3))
            dev = [[], [], []]
            for it in range(args.warmup + args.reps):
                rows[:, :HDR] = d_hdr0                 # the packets as the stack handed them over
                d_enc.copy_(d_enc0)
                d_out.copy_(d_out0)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record(stream)
                ah_encap(drv, d_arena, d_rec, d_sa.view(torch.int16), n, d_enc, AHSIZE, 0, d_hs, d_desc, d_opkt, d_est,
                         stream=stream)
                ev[1].record(stream)
                if it == 0:
                    ev[1].synchronize()
                    first_enc = (rows[:, :HDR].cpu().numpy().copy(), d_hs.cpu().numpy().copy(), d_desc.cpu().numpy().copy())
                    assert not d_est.any().item(), "every packet must be accepted"
                ah_frame(drv, d_arena, d_desc, n, d_out, d_fst, stream=stream)
                ev[2].record(stream)
                if it == 0:
                    ev[2].synchronize()
                    first_frm = (rows[:, :HDR].cpu().numpy().copy(), d_desc.cpu().numpy().copy(),
                                 d_out.cpu().numpy().view(OUTSA_DTYPE).copy())
                    assert not d_fst.any().item(), "every packet must be accepted"
                ah_sent(drv, d_arena, d_opkt, d_desc, d_st, n, d_enc, d_hs, d_sst, stream=stream)
                ev[3].record(stream)
                ev[3].synchronize()
                if it == 0:
                    first_snt = (rows[:, :HDR].cpu().numpy().copy(), d_enc.cpu().numpy().view(ENCSA_DTYPE).copy())
                    assert not d_sst.any().item(), "every packet must be restored"
                if it >= args.warmup:
                    for k in range(3):
                        dev[k].append(ev[k].elapsed_time(ev[k + 1]))
            assert int(first_snt[1]["packets"].sum()) == n and int(first_snt[1]["bytes"].sum()) == n * STRIDE
            assert int(first_frm[2]["count"].sum()) == n
            assert (first_snt[0][:, 9] == 51).all() and (first_snt[0][:, SKIP] == 6).all()
            # host: D2H of the stage's inputs and the span fronts, the walk, H2D of the results
            h_hdr = torch.empty((n, HDR), dtype=torch.uint8).pin_memory()
            h_rec, h_sa, h_st = pin(n * 8), pin(n * 2), pin(n)
            h_desc, h_opkt = pin(n * 16), pin(n * 8)
            h_est, h_fst, h_sst = pin(n), pin(n), pin(n)
            h_hs = np.zeros(n * HDR, dtype=np.uint8)
            host, wk = [[], [], []], [[], [], []]
            for it in range(args.warmup + args.reps):
                rows[:, :HDR] = d_hdr0
                h_enc, h_out = enc.copy(), outsa.copy()
                stream.synchronize()
                t = [time.perf_counter()]
                h_rec.copy_(d_rec, non_blocking=True)
                h_sa.copy_(d_sa, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                ok = walk.ah_encap_walk(h_enc.ctypes.data, maxsa, mlens.ctypes.data, h_hdr.data_ptr(), h_rec.data_ptr(),
                                        h_sa.data_ptr(), n, AHSIZE, 0, h_hs.ctypes.data, h_desc.data_ptr(),
                                        h_opkt.data_ptr(), h_est.data_ptr())
                t.append(time.perf_counter())
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_desc.copy_(h_desc, non_blocking=True)
                d_opkt.copy_(h_opkt, non_blocking=True)
                d_est.copy_(h_est, non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                assert ok == n
                if it == 0:
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first_enc[0]), "hashed headers differ"
                    assert np.array_equal(h_hs.reshape(n, HDR)[:, :SKIP], first_enc[1].reshape(n, HDR)[:, :SKIP])
                    assert np.array_equal(d_desc.cpu().numpy(), first_enc[2]), "descriptors differ"
                t.append(time.perf_counter())
                h_desc.copy_(d_desc, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                ok = walk.ah_frame_walk(h_out.ctypes.data, maxsa, mlens.ctypes.data, h_hdr.data_ptr(), base4.ctypes.data,
                                        h_desc.data_ptr(), n, h_fst.data_ptr())
                t.append(time.perf_counter())
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_desc.copy_(h_desc, non_blocking=True)
                d_fst.copy_(h_fst, non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                assert ok == n
                if it == 0:
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first_frm[0]), "numbered headers differ"
                    assert np.array_equal(d_desc.cpu().numpy(), first_frm[1]) and np.array_equal(h_out, first_frm[2])
                t.append(time.perf_counter())
                h_desc.copy_(d_desc, non_blocking=True)
                h_opkt.copy_(d_opkt, non_blocking=True)
                h_st.copy_(d_st, non_blocking=True)
                h_hdr.copy_(rows[:, :HDR], non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                ok = walk.ah_sent_walk(h_enc.ctypes.data, maxsa, mlens.ctypes.data, h_hdr.data_ptr(), base4.ctypes.data,
                                       h_opkt.data_ptr(), h_desc.data_ptr(), h_st.data_ptr(), n, h_hs.ctypes.data,
                                       h_sst.data_ptr())
                t.append(time.perf_counter())
                rows[:, :HDR].copy_(h_hdr, non_blocking=True)
                d_sst.copy_(h_sst, non_blocking=True)
                d_enc.copy_(torch.from_numpy(h_enc.view(np.uint8)), non_blocking=True)
                stream.synchronize()
                t.append(time.perf_counter())
                assert ok == n
                if it == 0:
                    assert np.array_equal(rows[:, :HDR].cpu().numpy(), first_snt[0]), "restored headers differ"
                    assert np.array_equal(d_enc.cpu().numpy().view(ENCSA_DTYPE), first_snt[1]), "counters differ"
                if it >= args.warmup:
                    for k in range(3):
                        host[k].append((t[4 * k + 3] - t[4 * k]) * 1e3)
                        wk[k].append((t[4 * k + 2] - t[4 * k + 1]) * 1e3)
            del d_arena, rows
        for k, stage in enumerate(("ah_encap", "ah_frame", "ah_sent")):
            (dm, dlo, dhi), (hm, hlo, hhi), (wm, _, _) = stats(dev[k]), stats(host[k]), stats(wk[k])
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
