// espgpu_ctx.h — the host runtime's context and what its translation units
// share: espgpu.cpp (staging slots, doorbell, failure path, process / flush /
// poll), espgpu_session.cpp (sessions) and espgpu_batch.cpp (kernel launches
// and the device-resident entry points).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "espgpu.h"
#include "espgpu_internal.h"
#include "fifo_arena.h"
#include "req_shape.h"

#ifndef GCM_BURST_DEFAULT
#define GCM_BURST_DEFAULT 4096
#endif

namespace espgpu {

struct Session : ReqSession {
  bool used = false;
  int klen = 0;
  bool whash = false;     // HMAC-SHA2-384/512 (128-byte hash blocks)
  bool wide = false;      // served by the two-pass ETA kernels only: HMAC-SHA2-384/512
                          // (128-byte hash blocks), no auth (CIPHER) or ESP-NULL
};

struct Pending {
  void *opaque;
  int etype_pre;              // -1: take the device status; else a host-side errno
  uint32_t rec;               // descriptor index in the batch
  uint32_t stage_off;         // byte offset of the staged record
  uint32_t stage_len;
  // where the result bytes go back (req_shape.h); up to 2 spans
  ReqSpan span[2];
  int nspan;
  uint32_t seg0, nsegs;       // the request's segments, copied into Slot::segpool
  // zero-copy: the record's start in registered host memory (device-mapped
  // address, espgpu_register_host); 0 = gathered into the staging buffer.
  // The record's layout there is the staged one, so span k's bytes go to
  // zc + span[k].stage_from.
  uint64_t zc;
};

// A request process() accepted while every staging slot was in flight
// (set_tuning "overflow_mb"): its bytes (unless zero-copy) wait in host
// memory and flush() moves it into the next free slot, in arrival order.
struct OvfEntry {
  Pending pd;                 // stage_off / seg0 index the overflow's own buffers
  espgpu_desc d;
  int32_t sid;
  uint8_t op, kind;
};
// The host overflow: entries in a fixed ring, their gathered bytes and segment
// lists in fixed FIFO arenas (fifo_arena.h), all sized at
// set_tuning("overflow_mb").
struct Overflow {
  std::unique_ptr<OvfEntry[]> ent;
  size_t ecap = 0, head = 0, count = 0;   // ring of entries; head = oldest
  FifoArena<uint8_t> bytes;
  FifoArena<espgpu_seg> segpool;
  size_t live_bytes = 0, peak_bytes = 0;
  bool empty() const { return count == 0; }
  OvfEntry &front() { return ent[head]; }
  // Reserve the three rings (the overflow must be empty).  All or nothing:
  // false leaves the old rings in place (the caller answers ENOMEM; no
  // exception crosses the C ABI).
  bool init(size_t cap_bytes) {
    // the byte ring holds overflow_mb of records; entries (a zero-copy record
    // needs no bytes) and segment lists get rings of their own beside it
    const size_t ne = cap_bytes ? std::max<size_t>(256, std::min<size_t>(cap_bytes / 512, (size_t)1 << 22)) : 0;
    std::unique_ptr<OvfEntry[]> e(ne ? new (std::nothrow) OvfEntry[ne] : nullptr);
    FifoArena<uint8_t> b;
    FifoArena<espgpu_seg> sg;
    if ((ne && !e) || !b.init(cap_bytes) || !sg.init(ne * 4)) return false;
    // the entry ring's pages committed now too, as the arenas' (fifo_arena.h)
    for (size_t o = 0; o < ne * sizeof(OvfEntry); o += 4096)
      reinterpret_cast<volatile uint8_t *>(e.get())[o] = 0;
    ent.swap(e);
    ecap = ne;
    bytes.swap(b);
    segpool.swap(sg);
    head = count = 0;
    live_bytes = peak_bytes = 0;
    return true;
  }
  size_t reserved() const {
    return ecap * sizeof(OvfEntry) + bytes.cap + segpool.cap * sizeof(espgpu_seg);
  }
  void pop() {
    OvfEntry &e = ent[head];
    if (!e.pd.zc) bytes.pop(e.pd.stage_off, (e.pd.stage_len + 15) & ~15u);
    segpool.pop(e.pd.seg0, e.pd.nsegs);
    live_bytes -= e.pd.zc ? 0 : ((e.pd.stage_len + 15) & ~15u);
    head = (head + 1) % ecap;
    if (--count == 0) {
      head = 0;
      bytes.clear();
      segpool.clear();
    }
  }
};

// Host memory registered with espgpu_register_host.
struct HostRegion {
  uintptr_t base;
  uint64_t len;
  uint64_t dev;               // device-mapped address of base
  bool owned;                 // hipHostRegister'ed here (else already pinned)
};

enum { SLOT_FREE = 0, SLOT_FILLING = 1, SLOT_INFLIGHT = 2 };

// A staging slot.  One pinned host buffer and its device mirror(s) hold, at
// flush time, [records: bytes][16 B slack][descriptors: nrec*16][status: nrec],
// so a batch is ONE H2D copy, the kernel(s), and ONE D2H copy (records and
// status together) -- what bounds a 32-record burst's latency is the number of
// queue operations, not bytes.
struct Slot {
  int state = SLOT_FREE;
  int op = -1;                // 0 decrypt, 1 encrypt
  uint8_t *h_arena = nullptr, *d_arena = nullptr, *d_out = nullptr;
  uint8_t *h_arena_dev = nullptr;           // h_arena's device-mapped address (xfer kernel)
  espgpu_desc *h_desc = nullptr;            // descriptors while filling
  // the xfer kernel's span lists (pinned, read by the kernel through the
  // mapping): [0, nin) before the crypto kernels, [nin, nin + nout) after
  XferSpan *h_xfer = nullptr, *h_xfer_dev = nullptr;
  uint32_t xfer_cap = 0;
  uint32_t nrec = 0, bytes = 0;
  uint32_t nstaged = 0;                     // records gathered (not zero-copy)
  uint32_t desc_off = 0, stat_off = 0;      // set by flush
  int32_t sid0 = -1;                        // session of the first record
  bool mixed = false;                       // more than one session staged
  uint32_t kinds = 0;                       // 1: GCM records, 2: ETA records, 4: DIGEST (AH) records
  std::vector<Pending> reqs;             // reserved to batch_records: no per-record allocation
  std::vector<espgpu_seg> segpool;       // segment lists of the staged requests
  hipEvent_t in_done = nullptr, k0 = nullptr, k1 = nullptr, kout = nullptr, done = nullptr;
  bool timed = false;                       // k0 / k1 recorded around the kernels
  hipStream_t st = nullptr;                 // small batches: copy, kernel, copy in order here
  // doorbell path (set_tuning "door"): the job number this slot's batch was
  // published as (-1: launched, or free), when, and its own E_K(J0) scratch
  // (jobs of different slots run at once)
  int64_t door_job = -1;
  uint64_t door_t0 = 0;
  uint4 *d_ej0 = nullptr;
  uint64_t t_launch = 0;                    // host clock (ns) when the batch was launched / published
  bool stuck = false;                       // fault injection: its completion is never seen (set_tuning "fault" 4)
  hipStream_t wq = nullptr;                 // launch in progress: the stream host-writing work went to
};

}  // namespace espgpu

struct espgpu_ctx {
  int device = 0;
  espgpu_config cfg{};
  // three streams so that batch k+1's H2D, batch k's kernels and batch k-1's
  // D2H overlap: stream (compute), s_in (host->device), s_out (device->host)
  hipStream_t stream = nullptr, s_in = nullptr, s_out = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // host-to-host pipeline (espgpu_decrypt_host) device mirrors
  uint8_t *e2e_arena = nullptr, *e2e_out = nullptr, *e2e_status = nullptr;
  espgpu_desc *e2e_desc = nullptr;
  uint64_t e2e_bytes = 0;
  uint32_t e2e_n = 0;
  hipEvent_t e2e_in[2] = {nullptr, nullptr}, e2e_k[2] = {nullptr, nullptr};
  espgpu::DevSA *d_sas = nullptr;
  uint8_t *d_gtab = nullptr;
  uint2 *d_tpair = nullptr, *d_dpair = nullptr;
  uint8_t *d_isbox = nullptr;
  uint32_t *d_queue = nullptr;   // work-queue regions (kQueueRegionWords apart): GCM, ETA, ETA aux, DIGEST (self-resetting)
  std::vector<espgpu::Session> sessions;
  // ETA sessions: all, and by kernel: narrow-hash (SHA-1 / SHA2-256) CBC and
  // CTR, wide-hash (SHA2-384/512) CBC and CTR
  int n_eta = 0, n_cbc = 0, n_ctr = 0, n_wcbc = 0, n_wctr = 0;
  int n_gcm = 0;                 // live AEAD (GCM) sessions
  int n_dig = 0, n_dig_wide = 0; // live DIGEST (AH) sessions: all, and the HMAC-SHA2-384/512 ones
  bool plan_dirty = true;        // planner key counts not known to be zero (plan_scan re-zeroes them)
  int n_whash = 0;   // ETA sessions with HMAC-SHA2-384/512 (the wide-hash two-pass kernels)
  // GCM lanes per record: 0 = by batch size, 4 or 8 forced (set_tuning
  // "gcm_lanes": the tests run both kernels at every batch size)
  int gcm_lanes = 0;
  // E_K(J0) scratch of the burst kernel
  uint4 *d_ej0 = nullptr;
  uint32_t ej0_cap = 0;
  // planner workspace
  uint32_t plan_cap = 0;
  uint32_t *d_work = nullptr, *d_order = nullptr, *d_nchunks = nullptr;
  espgpu::Chunk *d_chunks = nullptr;
  uint32_t max_chunks = 0;
  // the workspace of the stages that group by SA (window update, framing),
  // grown to the largest request seen
  void *d_stage_ws = nullptr;
  size_t stage_ws_bytes = 0;
  // staging
  std::vector<espgpu::Slot> slots;
  int cur = 0;
  espgpu::Overflow ovf;
  size_t ovf_cap = 0;            // set_tuning "overflow_mb" (0: ERESTART when the slots are busy)
  int xfer_small = 1;            // small batches: staging region moved by the xfer kernel (else hipMemcpyAsync)
  int stage_fused = 1;           // small single-session GCM batches stage their own records (one launch)
  uint32_t gcm_burst = GCM_BURST_DEFAULT;   // small GCM batches of <= this many records: burst kernel
  uint32_t natt_lanes = 0;       // set_tuning "natt_lanes": lanes per packet of the NAT-T recompute kernel (0: natt.h's)
  // doorbell burst path (set_tuning "door", espgpu_internal.h DoorCtl): a
  // persistent kernel of door_wg workgroups serves single-session GCM
  // batches of <= gcm_burst records with no launch per batch
  int door_wg = 0;
  uint32_t door_idle_us = 20000;             // the kernel exits after this long without a job
  bool door_retiring = false;                // kDoorStopIdle requested (door_retire)
  espgpu::DoorCtl *door_ctl = nullptr, *door_ctl_dev = nullptr;
  espgpu::DoorDev *d_door = nullptr;
  espgpu::DoorSlot *d_door_slots = nullptr;
  hipStream_t s_door = nullptr;
  hipEvent_t ev_door = nullptr;
  bool door_live = false;                    // launched and not seen to have exited
  uint32_t door_next = 0;                    // next job number
  uint64_t door_last_pub = 0;                // host clock (ns) of the last publish
  std::vector<espgpu::HostRegion> regions;   // sorted by base
  // completions not yet handed to poll(): ready[ready_head..] (host-side
  // rejects and finished batches), reserved so steady state does not allocate
  std::vector<espgpu_completion> ready;
  size_t ready_head = 0;
  // the stream the ctx last launched on and an event after that launch: the
  // work-queue counters and planner workspace are per ctx, so a launch on a
  // different stream first waits for it (stream-ordered, never concurrent)
  hipStream_t last_st = nullptr;
  bool launched = false;
  hipEvent_t ev_last = nullptr;
  // GPU failure (ctx_fail): once set the ctx launches nothing again; every
  // request it holds completes exactly once with ESPGPU_EIO
  bool failed = false;
  uint32_t fault = 0;            // set_tuning "fault": injected failures (ESPGPU_FAULT_*)
  uint32_t deadline_ms = 2000;   // set_tuning "deadline_ms": a batch outstanding this long is a GPU failure
  espgpu_stats stats{};
  float last_ms = 0.f;
  std::string err;
#ifdef ESPGPU_BOUNDS
  // the bounds-checked build (bounds_chk.h): the report in device memory
  // (allocated at the first launch) and the extents armed for the next one
  espgpu::ChkArm chk{};
  bool chk_armed = false;
#endif
};

namespace espgpu {

inline int fail(espgpu_ctx *c, int code, const char *fmt, ...) {
  if (c) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define HIPCHK(ctx, expr)                                                          \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(ctx, ESPGPU_EIO, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

inline uint64_t now_ns() {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
}

// Consume an injected launch failure (set_tuning "fault", ESPGPU_FAULT_LAUNCH):
// true, with the message set, if the launch about to be made is to fail.
inline bool take_launch_fault(espgpu_ctx *c) {
  if (!(c->fault & ESPGPU_FAULT_LAUNCH)) return false;
  c->fault &= ~(uint32_t)ESPGPU_FAULT_LAUNCH;
  fail(c, ESPGPU_EIO, "injected launch failure");
  return true;
}

// espgpu.cpp: the doorbell kernel and the failure path
bool door_exited(espgpu_ctx *c);
void door_stop(espgpu_ctx *c);
void door_retire(espgpu_ctx *c);
int ctx_fail(espgpu_ctx *c, const char *why);

// espgpu_session.cpp
extern int g_ah_offer;                   // set_tuning "ah_offer" (-1: the environment decides)
int probe_caps(const espgpu_session_params *csp);
// The mode and ICV length newsession files in DevSA for a session.
void session_filed(const espgpu_session_params *csp, uint32_t *mode, uint32_t *mlen);

// espgpu_batch.cpp
// The self-staging lists of a small single-session GCM process batch
// (GcmParams::xin / xout / hstat).
struct StageLists {
  const XferSpan *xin, *xout;
  uint8_t *hstat;
  const espgpu_desc *hdesc;
};
int run_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n, uint8_t *d_status,
              uint8_t *d_out, uint32_t flags, int encrypt, hipStream_t st, uint32_t *d_trailer = nullptr,
              uint32_t kinds = 1 | 2 | 8, const StageLists *stage = nullptr, uint32_t out_stride = 0);

}  // namespace espgpu
