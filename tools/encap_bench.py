#!/usr/bin/env python3
"""Outbound encapsulation of a device-resident batch, device against host
(measurement only; needs a GPU, no fallback).

  python tools/encap_bench.py [--packets N] [--reps R] [--warmup W] [--out FILE]

Four shapes of N cleartext IPv4 packets (default 2^20) of 1400 bytes, each with
64 bytes of room in front and 72 behind (a 1536-byte stride), AES-GCM-16
sessions (hlen 16, alen 16), every one accepted:
  one SA and 1024 SAs interleaved at random, each in tunnel mode (a 20-byte
  outer header in front, the inner header's length and checksum fixed) and in
  transport mode (the 20-byte header moves 16 bytes down, fixed).
For each it times, over --reps warmed repetitions (median, min, max; the
spread is the margin):
  device  espgpu_esp_encap_batch, and espgpu_esp_sent_batch on its results:
          HIP events around each call on one stream, everything staying in
          device memory;
  host    what a caller has without them, end to end on the wall clock: copy
          the espgpu_pkt records, the SA ids and each packet's 128 bytes from
          its room's start back (a strided device-to-host copy),
          espgpu_esp_encap per packet on one core (tools/encap_walk.c,
          compiled here), copy the 128 bytes, descriptors, frame words, wire
          records and status bytes up; and for `sent` the wire records,
          descriptors and statuses back, espgpu_esp_sent per packet, the SA
          table up.
Both produce the same descriptors, frame words, wire records, statuses, header
bytes and counters (checked on the first run of each).  One line per shape
with the times and their ratios; --out also writes them to a file."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

LEN, HEAD, TAIL, SPAN, SKIP, HLEN, ALEN = 1400, 64, 72, 128, 20, 16, 16
STRIDE = HEAD + LEN + TAIL


def build_walk():
    so = os.path.join(ROOT, "f-stack_amd", "build", "encap_walk.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    lib = os.path.join(ROOT, "f-stack_amd")
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "encap_walk.c"), "-o", so,
                    "-L", lib, "-lespgpu", "-Wl,-rpath," + lib], check=True)
    w = C.CDLL(so)
    w.encap_walk.restype = C.c_uint32
    w.encap_walk.argtypes = ([C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p] * 4)
    w.sent_walk.restype = C.c_uint32
    w.sent_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return w


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def headers(n, dst):
    """n 20-byte IPv4 headers of TCP packets of LEN bytes to dst[i], checksums right."""
    h = np.zeros((n, SKIP), dtype=np.uint8)
    h[:, 0], h[:, 2], h[:, 3], h[:, 8], h[:, 9] = 0x45, LEN >> 8, LEN & 0xff, 64, 6
    h[:, 4:6] = np.arange(n, dtype=np.uint32).astype(">u2").view(np.uint8).reshape(n, 2)      # ip_id
    h[:, 12:16], h[:, 16:20] = (10, 0, 0, 1), dst
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
    from espgpu.batch import DESC_DTYPE, ENCSA_DTYPE, OUTSA_DTYPE, PKT_DTYPE, esp_encap, esp_sent
    from espgpu.esp import GCM, SecAssoc
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "encap_bench needs a GPU"
    walk = build_walk()
    rng = np.random.default_rng(1)
    maxsa, n = 1024, args.packets
    drv = GpuCryptoDriver(device=0, max_sessions=maxsa)
    for k in range(maxsa):
        rc, sid = drv.newsession(SecAssoc(0x1000 + k, GCM, rng.integers(0, 256, 20, dtype=np.uint8).tobytes()).csp())
        assert rc == 0 and sid == k
    shapes = (L.EShape * maxsa)(*[L.EShape(HLEN - 8, 4, ALEN)] * maxsa)
    pkt = np.zeros(n, dtype=PKT_DTYPE)
    pkt["off4"], pkt["len"] = (np.arange(n, dtype=np.int64) * STRIDE + HEAD) // 4, LEN
    stream = torch.cuda.Stream()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()      # noqa: E731
    lines = []
    for name, nsa, tunnel in (("one-sa tunnel", 1, True), ("one-sa transport", 1, False),
                              ("1024-sa tunnel", maxsa, True), ("1024-sa transport", maxsa, False)):
        sa = np.zeros(n, dtype=np.uint16) if nsa == 1 else rng.integers(0, nsa, n).astype(np.uint16)
        enc = np.zeros(maxsa, dtype=ENCSA_DTYPE)
        enc["flags"], enc["ttl"] = (L.ENC_TUNNEL if tunnel else 0) | L.ENC_DF_COPY, 64
        enc["src"][:, :4] = (192, 0, 2, 1)
        enc["dst"][:, 0], enc["dst"][:, 1] = 198, 51
        enc["dst"][:, 2], enc["dst"][:, 3] = np.arange(maxsa) >> 8, np.arange(maxsa) & 0xff
        hdr = headers(n, enc["dst"][sa, :4])                 # every packet goes to its SA's address: transport unless TUNNEL
        front = HLEN + (20 if tunnel else 0)
        padding = ((4 - ((LEN if tunnel else LEN - SKIP) + 2) % 4) % 4) + 2
        total = (20 if tunnel else 0) + HLEN + LEN + padding + ALEN
        with torch.cuda.stream(stream):
            d_arena = torch.zeros(n * STRIDE + 64, dtype=torch.uint8, device="cuda")
            rows = d_arena[:n * STRIDE].view(n, STRIDE)
            d_hdr0 = torch.from_numpy(hdr).cuda()
            d_pkt, d_enc = up(pkt), up(enc)
            d_sa = torch.from_numpy(sa.view(np.int16).copy()).cuda()
            d_out = up(np.zeros(maxsa, dtype=OUTSA_DTYPE))
            d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            d_frame = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
            d_est = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")

            def reset():
                rows[:, :SPAN] = 0
                rows[:, HEAD:HEAD + SKIP] = d_hdr0
                d_enc.copy_(up(enc))

            dev, dev_sent = [], []
            for it in range(args.warmup + args.reps):
                reset()
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(stream)
                esp_encap(drv, d_arena, d_pkt, d_sa, n, d_enc, d_out, HEAD, TAIL, 0, d_desc, d_frame, d_opkt, d_est,
                          stream=stream)
                e1.record(stream)
                esp_sent(drv, d_opkt, d_desc, d_st, n, d_enc, stream=stream)
                e2.record(stream)
                e2.synchronize()
                if it == 0:                       # the first run's results
                    first = (d_opkt.cpu().numpy().copy(), rows[:, :SPAN].cpu().numpy().copy(),
                             d_enc.cpu().numpy().view(ENCSA_DTYPE).copy(), d_desc.cpu().numpy().copy(),
                             d_frame.cpu().numpy().copy())
                    assert not d_est.any().item(), "every packet must be accepted"
                if it >= args.warmup:
                    dev.append(e0.elapsed_time(e1))
                    dev_sent.append(e1.elapsed_time(e2))
            got = first[0].view(PKT_DTYPE)
            assert np.array_equal(got["off4"], pkt["off4"] - front // 4) and (got["len"] == total).all()
            assert int(first[2]["packets"].sum()) == n and int(first[2]["bytes"].sum()) == n * total
            # host: D2H of the records, SA ids and span bytes, the walk, H2D of the results; then the same for sent
            h_span = torch.empty((n, SPAN), dtype=torch.uint8).pin_memory()
            h_pkt = torch.zeros(n * 8, dtype=torch.uint8).pin_memory()
            h_sa = torch.zeros(n, dtype=torch.int16).pin_memory()
            h_desc = torch.zeros(n * 16, dtype=torch.uint8).pin_memory()
            h_frame = torch.zeros(n, dtype=torch.int32).pin_memory()
            h_opkt = torch.zeros(n * 8, dtype=torch.uint8).pin_memory()
            h_est = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_st = torch.zeros(n, dtype=torch.uint8).pin_memory()
            h_enc = torch.from_numpy(enc.view(np.uint8).copy()).pin_memory()
            host, walk_only, host_sent = [], [], []
            for it in range(args.warmup + args.reps):
                reset()
                h_enc.copy_(torch.from_numpy(enc.view(np.uint8).copy()))
                stream.synchronize()
                t0 = time.perf_counter()
                h_pkt.copy_(d_pkt, non_blocking=True)
                h_sa.copy_(d_sa, non_blocking=True)
                h_span.copy_(rows[:, :SPAN], non_blocking=True)
                stream.synchronize()
                t1 = time.perf_counter()
                ok = walk.encap_walk(h_enc.data_ptr(), maxsa, C.addressof(shapes), h_span.data_ptr(), h_pkt.data_ptr(),
                                     h_sa.data_ptr(), n, HEAD, TAIL, 0, h_desc.data_ptr(), h_frame.data_ptr(),
                                     h_opkt.data_ptr(), h_est.data_ptr())
                t2 = time.perf_counter()
                rows[:, :SPAN].copy_(h_span, non_blocking=True)
                d_desc.copy_(h_desc, non_blocking=True)
                d_frame.copy_(h_frame, non_blocking=True)
                d_opkt.copy_(h_opkt, non_blocking=True)
                d_est.copy_(h_est, non_blocking=True)
                stream.synchronize()
                t3 = time.perf_counter()
                h_opkt.copy_(d_opkt, non_blocking=True)
                h_desc.copy_(d_desc, non_blocking=True)
                h_st.copy_(d_st, non_blocking=True)
                stream.synchronize()
                booked = walk.sent_walk(h_enc.data_ptr(), maxsa, h_opkt.data_ptr(), h_desc.data_ptr(), h_st.data_ptr(), n)
                d_enc.copy_(h_enc, non_blocking=True)
                stream.synchronize()
                t4 = time.perf_counter()
                assert ok == n and booked == n
                if it == 0:
                    assert np.array_equal(d_opkt.cpu().numpy(), first[0]), "host and device wire records differ"
                    assert np.array_equal(rows[:, :SPAN].cpu().numpy(), first[1]), "host and device headers differ"
                    assert np.array_equal(d_enc.cpu().numpy().view(ENCSA_DTYPE), first[2]), "counters differ"
                    assert np.array_equal(d_desc.cpu().numpy(), first[3]), "descriptors differ"
                    assert np.array_equal(d_frame.cpu().numpy(), first[4]), "frame words differ"
                    assert not d_est.any().item()
                if it >= args.warmup:
                    host.append((t3 - t0) * 1e3)
                    walk_only.append((t2 - t1) * 1e3)
                    host_sent.append((t4 - t3) * 1e3)
            del d_arena, rows
        (dm, dlo, dhi), (sm, slo, shi) = stats(dev), stats(dev_sent)
        (hm, hlo, hhi), (wm, _, _), (hs, hslo, hshi) = stats(host), stats(walk_only), stats(host_sent)
        lines.append("%-17s n=%d sas=%d  encap: device %.3f ms (min %.3f max %.3f)  host %.3f ms (min %.3f max %.3f; "
                     "walk alone %.3f ms)  host/device %.1f  sent: device %.3f ms (min %.3f max %.3f)  host %.3f ms "
                     "(min %.3f max %.3f)  host/device %.1f  reps=%d warmup=%d"
                     % (name, n, nsa, dm, dlo, dhi, hm, hlo, hhi, wm, hm / dm, sm, slo, shi, hs, hslo, hshi, hs / sm,
                        args.reps, args.warmup))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    drv.close()


if __name__ == "__main__":
    main()
