#!/usr/bin/env python3
"""Kernel-time A/B of the AH digest kernel against its yardstick (measurement
only; needs a GPU, no fallback).

  python tools/ah_timing.py [--records N] [--sas S] [--lens 1500 64] [--reps R]

For each packet length and each of HMAC-SHA1-96 / HMAC-SHA2-256-128 it times,
with HIP events around the launches on one stream:
  ah    espgpu_decrypt_batch (verify) of N AH packets over S digest SAs
        (esp_ah.hip digest_kernel), grouped and through the planner;
  esp   the in-place espgpu_decrypt_batch of N ESP-NULL + the same HMAC
        records of equal length over S SAs (esp_cbc.hip eta_kernel<2, ...>):
        the same hash work through the kernel that holds the AES tables.
The two alternate step by step, so box drift hits both alike; each line is the
median of --reps warmed steps with their min and max (the spread is the
margin).  Records are random bytes: every ICV check fails, which is the same
work as a passing one.  Algorithmic bytes per AH packet: the packet and its
16-byte descriptor read, 1 status byte written.  One JSON line per variant."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "f-stack_amd"))

DESC = [("off4", "<u4"), ("len", "<u2"), ("sa", "<u2"), ("esn_hi", "<u4"), ("salt", "<u4")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--sas", type=int, default=1024)
    ap.add_argument("--lens", type=int, nargs="*", default=[1500, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from espgpu import ah as A
    from espgpu import esp as E
    from espgpu.batch import decrypt_batch
    from espgpu.opencrypto import GpuCryptoDriver
    assert torch.cuda.is_available(), "ah_timing needs a GPU"
    n, ns = args.records, args.sas
    assert n % ns == 0 and (n // ns) % 256 == 0, "grouped: whole 256-record runs per SA"
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    for alg_ah, alg_esp, name in ((A.AH_SHA1, E.NULL_SHA1, "hmac-sha1-96"), (A.AH_SHA256, E.NULL_SHA256, "hmac-sha2-256-128")):
        # one context per transform: a context without DIGEST sessions launches no digest kernel
        ctx = {}
        for kind in ("ah", "esp"):
            drv = GpuCryptoDriver(device=0, max_sessions=ns)
            sids = []
            for i in range(ns):
                key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
                csp = (A.AhSecAssoc(i + 256, alg_ah, key) if kind == "ah" else E.SecAssoc(i + 256, alg_esp, b"", key)).csp()
                rc, sid = drv.newsession(csp)
                assert rc == 0, drv.last_error()
                sids.append(sid)
            ctx[kind] = (drv, np.array(sids))
        for rl in args.lens:
            slot = (rl + 20 + 3) & ~3
            arena = torch.randint(0, 256, (n * slot + 64,), dtype=torch.uint8, device="cuda")
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            per = n // ns
            runs = {}
            for kind in ("ah", "esp"):
                drv, sids = ctx[kind]
                for grouped in (True, False):
                    d = np.zeros(n, dtype=DESC)
                    d["off4"] = (np.arange(n, dtype=np.int64) * slot + 20) // 4
                    d["len"] = rl
                    # grouped: runs of n / S records per SA; planner: SAs interleaved record by record
                    d["sa"] = sids[np.arange(n) // per] if grouped else sids[np.arange(n) % ns]
                    d["salt"] = 32 if kind == "ah" else 0
                    runs[(kind, grouped)] = (drv, torch.from_numpy(d.view(np.uint8).copy()).cuda(), [])
            order = [("ah", True), ("esp", True), ("ah", False), ("esp", False)]
            with torch.cuda.stream(stream):
                for step in range(args.warmup + args.reps):
                    for k in order:
                        drv, desc, ms = runs[k]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        decrypt_batch(drv, arena, desc, n, st, out=None, grouped=k[1], stream=stream)
                        e1.record(stream)
                        ms.append((e0, e1))
            torch.cuda.synchronize()
            algo = n * (rl + 16) + n
            for k in order:
                t = sorted(e0.elapsed_time(e1) for e0, e1 in runs[k][2][args.warmup:])
                med = t[len(t) // 2]
                print(json.dumps({"kernel": "digest_kernel" if k[0] == "ah" else "eta_kernel<2> esp-null", "auth": name,
                                  "path": "grouped" if k[1] else "planner", "records": n, "sas": ns, "rec_len": rl,
                                  "reps": len(t), "ms_median": round(med, 4), "ms_min": round(t[0], 4),
                                  "ms_max": round(t[-1], 4), "algo_GBps": round(algo / med / 1e6, 1)}), flush=True)
            del arena, st, runs
        for drv, _ in ctx.values():
            drv.close()


if __name__ == "__main__":
    main()
