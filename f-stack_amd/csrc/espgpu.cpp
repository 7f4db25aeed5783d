// espgpu.cpp — host runtime behind include/espgpu.h: the opencrypto-driver
// shaped C ABI's request path (process/flush/poll with pinned staging and
// async copies on a HIP stream), the doorbell kernel and the failure path.
// Sessions are espgpu_session.cpp, the kernel launches and device-resident
// batch entry points espgpu_batch.cpp, the request rule req_shape.h.
//
// Reference interfaces mirrored (F-Stack 1.25 tree):
//   process       cryptosoft.c:1429-1441 (swcr_process) -> swcr_gcm :465 / swcr_eta :874
//                 / swcr_authcompute :317 (CSP_MODE_DIGEST: AH, xform_ah.c)
//   completion    crypto_done, crypto.c:1802
#include <sched.h>
#include <stdlib.h>

#include "espgpu_ctx.h"
#include "host_crypto.h"

namespace espgpu {
namespace {

#ifndef GPU_TIME_SMALL
#define GPU_TIME_SMALL 0
#endif
// flush(): batches up to this many staged bytes run on one stream (latency)
constexpr uint32_t kSmallBatchBytes = 128u << 10;

int alloc_slot(espgpu_ctx *c, Slot &s) {
  const size_t recs = c->cfg.batch_records;
  const size_t bytes = c->cfg.batch_bytes + 64 + recs * (sizeof(espgpu_desc) + 1) + 64;
  HIPCHK(c, hipHostMalloc((void **)&s.h_arena, bytes, hipHostMallocDefault));
  HIPCHK(c, hipHostGetDevicePointer((void **)&s.h_arena_dev, s.h_arena, 0));
  s.h_desc = new espgpu_desc[recs];
  HIPCHK(c, hipMalloc(&s.d_arena, bytes));
  HIPCHK(c, hipMalloc(&s.d_out, bytes));
  HIPCHK(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming));
  HIPCHK(c, hipEventCreate(&s.k0));
  HIPCHK(c, hipEventCreate(&s.k1));
  HIPCHK(c, hipEventCreateWithFlags(&s.kout, hipEventDisableTiming));
  HIPCHK(c, hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
  s.reqs.reserve(recs);
  s.segpool.reserve(recs * 2);
  return 0;
}

void free_slot(Slot &s) {
  if (s.st) hipStreamSynchronize(s.st);
  hipHostFree(s.h_arena);
  hipHostFree(s.h_xfer);
  hipFree(s.d_ej0);
  delete[] s.h_desc;
  hipFree(s.d_arena); hipFree(s.d_out);
  for (hipEvent_t e : {s.done, s.in_done, s.k0, s.k1, s.kout})
    if (e) hipEventDestroy(e);
  if (s.st) hipStreamDestroy(s.st);
}

// The device-mapped address of [p, p + n) if it lies in one registered region, else 0.
uint64_t region_dev(const espgpu_ctx *c, const uint8_t *p, uint32_t n) {
  const uintptr_t a = (uintptr_t)p;
  auto it = std::upper_bound(c->regions.begin(), c->regions.end(), a,
                             [](uintptr_t v, const HostRegion &r) { return v < r.base; });
  if (it == c->regions.begin()) return 0;
  --it;
  if (a + n > it->base + it->len) return 0;
  return it->dev + (a - it->base);
}

// Append one request to a slot (its record bytes, unless zero-copy, already
// at h_arena + bytes).
void slot_commit(Slot &s, Pending pd, espgpu_desc d, const espgpu_seg *segs, int32_t sid, int op,
                 uint32_t kind) {
  if (s.state == SLOT_FREE) {
    s.state = SLOT_FILLING;
    s.op = op;
    s.nrec = 0;
    s.bytes = 0;
    s.nstaged = 0;
    s.reqs.clear();
    s.segpool.clear();
    s.sid0 = sid;
    s.mixed = false;
    s.kinds = 0;
  }
  pd.rec = s.nrec;
  pd.stage_off = s.bytes;
  pd.seg0 = (uint32_t)s.segpool.size();
  s.segpool.insert(s.segpool.end(), segs, segs + pd.nsegs);
  d.off4 = s.bytes / 4;
  s.h_desc[s.nrec] = d;
  s.bytes += (pd.stage_len + 15) & ~15u;
  s.nrec++;
  s.nstaged += pd.zc ? 0 : 1;
  s.mixed |= (sid != s.sid0);
  s.kinds |= kind;
  s.reqs.push_back(pd);
}

bool slot_full(const espgpu_ctx *c, const Slot &s, int op, uint32_t rlen) {
  return s.state == SLOT_FILLING &&
         (s.op != op || s.nrec >= c->cfg.batch_records || s.bytes + rlen + 16 > c->cfg.batch_bytes);
}

// ---- doorbell burst path (espgpu_internal.h DoorCtl) -------------------------
// A door batch's descriptors and statuses sit at fixed offsets of its slot
// (after the largest record region), so the device slot table never changes
// per batch; its xout spans start at h_xfer + batch_records.
uint32_t door_desc_off(const espgpu_ctx *c) { return c->cfg.batch_bytes + 16; }
uint32_t door_stat_off(const espgpu_ctx *c) { return door_desc_off(c) + c->cfg.batch_records * (uint32_t)sizeof(espgpu_desc); }
constexpr uint32_t kDoorChunk = 4;           // records per claimed chunk (the burst kernel's)

int door_write_slot(espgpu_ctx *c, size_t k) {
  const Slot &s = c->slots[k];
  const DoorSlot ds{s.d_arena, s.d_out, s.d_ej0, s.h_xfer_dev, s.h_xfer_dev + c->cfg.batch_records,
                    s.h_arena_dev + door_desc_off(c), s.h_arena_dev + door_stat_off(c), door_desc_off(c),
                    door_stat_off(c)};
  HIPCHK(c, hipMemcpy(c->d_door_slots + k, &ds, sizeof ds, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

// The kernel has exited (or was never launched): no workgroup reads the
// slot table or the SA table's cached state any more.
bool door_exited(espgpu_ctx *c) {
  // (an error other than "not ready": the device is gone, and so is the kernel)
  if (c->door_live && hipEventQuery(c->ev_door) != hipErrorNotReady) c->door_live = false;
  return !c->door_live;
}

// Stop the persistent kernel and wait for it (published jobs it did not
// claim stay in the ring for the next launch).  A failed ctx only asks: its
// kernel may never finish, and nothing waits on a failed device.
void door_stop(espgpu_ctx *c) {
  if (!c->door_live) return;
  __atomic_store_n(&c->door_ctl->stop, kDoorStopNow, __ATOMIC_SEQ_CST);
  if (c->failed) return;
  hipEventSynchronize(c->ev_door);
  __atomic_store_n(&c->door_ctl->stop, 0u, __ATOMIC_SEQ_CST);
  c->door_live = false;
  c->door_retiring = false;
}

// Before any other kernel or copy of this ctx is queued: the persistent
// kernel's stream may share a hardware queue with the stream that work goes
// to (GPU_MAX_HW_QUEUES is 4; a ctx has more streams), and a queue runs its
// packets in order, so work behind a resident door kernel would wait for its
// idle timeout.  Without waiting, ask it to exit once no published job is
// left (kDoorStopIdle): queued work starts right after its last chunk.  The
// next door job clears the request and relaunches the kernel if it exited.
void door_retire(espgpu_ctx *c) {
  if (!c->door_live || c->door_retiring) return;
  if (door_exited(c)) return;
  __atomic_store_n(&c->door_ctl->stop, kDoorStopIdle, __ATOMIC_SEQ_CST);
  c->door_retiring = true;
}

namespace {

// No launched work of the ctx is outstanding: its last launch (any stream)
// and every launched slot's batch have completed.  Until then a retire
// request must stand: the launched work may sit behind the door kernel on a
// shared hardware queue.
bool launched_idle(espgpu_ctx *c) {
  if (c->launched && hipEventQuery(c->ev_last) != hipSuccess) return false;
  for (const Slot &s : c->slots)
    if (s.state == SLOT_INFLIGHT && s.door_job < 0 && hipEventQuery(s.done) != hipSuccess) return false;
  return true;
}

int door_launch(espgpu_ctx *c) {
  DoorArgs a{};
  a.ctl = c->door_ctl_dev;
  a.dev = c->d_door;
  a.slots = c->d_door_slots;
  a.nslots = (uint32_t)c->slots.size();
  a.chunk = kDoorChunk;
  a.idle_ticks = c->door_idle_us * 100u;     // s_memrealtime: 100 MHz
  a.sas = c->d_sas;
  a.gtab = c->d_gtab;
  a.tpair = c->d_tpair;
  a.nsas = c->cfg.max_sessions;              // unused entries are zero (mode 0): EINVAL
  __atomic_store_n(&c->door_ctl->stop, 0u, __ATOMIC_SEQ_CST);
  c->door_retiring = false;
  if (launch_gcm_door(a, c->door_wg, c->s_door)) return fail(c, ESPGPU_EIO, "door kernel launch failed");
  HIPCHK(c, hipEventRecord(c->ev_door, c->s_door));
  c->door_live = true;
  return 0;
}

// Relaunch the kernel if it exited (idle timeout) while jobs are outstanding.
int door_ensure(espgpu_ctx *c) {
  return door_exited(c) ? door_launch(c) : 0;
}

int door_setup(espgpu_ctx *c) {
  if (c->door_ctl) return 0;
  if (c->slots.size() > kDoorRing) return fail(c, ESPGPU_EINVAL, "door: more staging slots than ring entries (%u)", kDoorRing);
  HIPCHK(c, hipHostMalloc((void **)&c->door_ctl, sizeof(DoorCtl), hipHostMallocMapped | hipHostMallocCoherent));
  memset(c->door_ctl, 0, sizeof(DoorCtl));
  HIPCHK(c, hipHostGetDevicePointer((void **)&c->door_ctl_dev, c->door_ctl, 0));
  HIPCHK(c, hipMalloc(&c->d_door, sizeof(DoorDev)));
  HIPCHK(c, hipMemset(c->d_door, 0, sizeof(DoorDev)));
  HIPCHK(c, hipMalloc(&c->d_door_slots, c->slots.size() * sizeof(DoorSlot)));
  HIPCHK(c, hipStreamCreateWithFlags(&c->s_door, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_door, hipEventDisableTiming));
  const uint32_t cap = 3 * c->cfg.batch_records;     // xin + 2 xout spans per record
  for (size_t k = 0; k < c->slots.size(); ++k) {
    Slot &s = c->slots[k];
    if (s.xfer_cap < cap) {
      hipHostFree(s.h_xfer);
      s.h_xfer = nullptr;
      s.xfer_cap = 0;
      HIPCHK(c, hipHostMalloc((void **)&s.h_xfer, (size_t)cap * sizeof(XferSpan), hipHostMallocDefault));
      HIPCHK(c, hipHostGetDevicePointer((void **)&s.h_xfer_dev, s.h_xfer, 0));
      s.xfer_cap = cap;
    }
    HIPCHK(c, hipMalloc(&s.d_ej0, (size_t)c->cfg.batch_records * sizeof(uint4)));
    int e = door_write_slot(c, k);
    if (e) return e;
  }
  c->door_next = 0;
  return 0;
}

void door_free(espgpu_ctx *c) {
  door_stop(c);
  if (c->door_ctl) hipHostFree(c->door_ctl);
  hipFree(c->d_door);
  hipFree(c->d_door_slots);
  if (c->ev_door) hipEventDestroy(c->ev_door);
  if (c->s_door) hipStreamDestroy(c->s_door);
  c->door_ctl = c->door_ctl_dev = nullptr;
  c->d_door = nullptr;
  c->d_door_slots = nullptr;
  c->ev_door = nullptr;
  c->s_door = nullptr;
}

bool door_done(const espgpu_ctx *c, int64_t job) {
  const uint32_t j = (uint32_t)job;
  return __atomic_load_n(&c->door_ctl->done[j % kDoorRing], __ATOMIC_ACQUIRE) == j + 1;
}

// ---- GPU failure --------------------------------------------
// A launch or copy that cannot be queued, a completion query that returns an
// error, or a batch outstanding for deadline_ms is a GPU failure.  The ctx
// then launches nothing again, and every request it holds completes exactly
// once (crypto_done once per cryptop, crypto.c:1802-1804): with ESPGPU_EIO
// -- which the kernel-domain driver maps to EIO, a clean drop for
// esp_input_cb / esp_output_cb (esps_noxform, xform_esp.c:514-520) -- unless
// its batch is seen to complete after all (then with its real result).
// espgpu_health() reports the state: the F-Stack shim's probe then declines,
// so new SAs go to cryptosoft, and process() refuses at once.

// Wait, at most deadline_ms, for a stream's queued work; true if it drained
// (or the device reports an error: nothing of it runs any more).
bool stream_settle(espgpu_ctx *c, hipStream_t st) {
  if (!st) return true;
  const uint64_t t0 = now_ns();
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q != hipErrorNotReady) return true;
    if (now_ns() - t0 > (uint64_t)c->deadline_ms * 1000000ull) return false;
    sched_yield();
  }
}

// A slot's requests complete with ESPGPU_EIO (their buffers untouched: results
// are copied back only for a batch that completed); the slot is free again.
void drop_slot(espgpu_ctx *c, Slot &s) {
  for (const Pending &pd : s.reqs) c->ready.push_back(espgpu_completion{pd.opaque, ESPGPU_EIO});
  c->stats.fail_eio += s.reqs.size();
  s.reqs.clear();
  s.segpool.clear();
  s.nrec = 0;
  s.bytes = 0;
  s.door_job = -1;
  s.stuck = false;
  s.state = SLOT_FREE;
}

// A batch about to be released as failed: work of it still queued may write
// the requests' host buffers (zero-copy results, the results' xfer kernel), so
// wait for its completion event, at most deadline_ms, first (as fail_launch
// does for a launch that failed part way).  A query error ends the wait: the
// device runs nothing of it any more.
void slot_settle(espgpu_ctx *c, Slot &s) {
  const uint64_t t0 = now_ns();
  while (hipEventQuery(s.done) == hipErrorNotReady) {
    if (now_ns() - t0 > (uint64_t)c->deadline_ms * 1000000ull) return;
    sched_yield();
  }
}

}  // namespace

// Mark the ctx failed (once) and release what was never handed to the
// device: the filling slot and the host overflow.  In-flight batches are
// retired by poll / drain (slot_check).  Returns ESPGPU_EIO.
int ctx_fail(espgpu_ctx *c, const char *why) {
  if (!c->failed) {
    const std::string cause = c->err;
    c->failed = true;
    c->stats.gpu_fail++;
    c->err = std::string("GPU failure: ") + why + (cause.empty() ? "" : " (" + cause + ")");
    fprintf(stderr, "espgpu: %s; nothing more is launched, held requests complete with EIO\n", c->err.c_str());
    if (c->door_ctl) door_stop(c);               // (failed: asks the kernel to exit, never waits)
  }
  for (Slot &s : c->slots)
    if (s.state == SLOT_FILLING) drop_slot(c, s);
  Overflow &o = c->ovf;
  while (!o.empty()) {
    c->ready.push_back(espgpu_completion{o.front().pd.opaque, ESPGPU_EIO});
    c->stats.fail_eio++;
    o.pop();
  }
  return ESPGPU_EIO;
}

namespace {

// Where an in-flight batch stands: 1 completed, 0 still running, -1 failed
// (its completion query returned an error, it outlived deadline_ms, or the ctx
// failed and the batch can no longer finish).  A doorbell job of a failed ctx
// is released only once the kernel has exited (a workgroup inside one of its
// chunks still writes results into host memory) or after the deadline; any
// other failed batch once its queued work has drained (slot_settle).
int slot_check(espgpu_ctx *c, Slot &s, uint64_t now) {
  const bool late = now > s.t_launch && now - s.t_launch > (uint64_t)c->deadline_ms * 1000000ull;
  if (s.door_job >= 0) {
    if (!s.stuck && door_done(c, s.door_job)) return 1;
    if (!c->failed && !late) return 0;
    if (!c->failed) ctx_fail(c, "doorbell job outstanding past deadline_ms");
    return (door_exited(c) || late) ? -1 : 0;
  }
  hipError_t q = s.stuck ? hipErrorNotReady : hipEventQuery(s.done);
  if (c->fault & ESPGPU_FAULT_QUERY) {
    c->fault &= ~(uint32_t)ESPGPU_FAULT_QUERY;
    q = hipErrorLaunchFailure;                   // injected: as a lost device reports it
  }
  if (q == hipSuccess) return 1;
  if (q != hipErrorNotReady) {
    if (!c->failed) {
      c->err = hipGetErrorString(q);
      ctx_fail(c, "batch completion query failed");
    }
    slot_settle(c, s);
    return -1;
  }
  if (!late) return 0;
  if (!c->failed) ctx_fail(c, "batch outstanding past deadline_ms");
  slot_settle(c, s);
  return -1;
}

// A slot whose launch failed part way: work already queued for it that
// writes host memory (a self-staging kernel, the results' xfer kernel or
// D2H copy) is waited for, boundedly, before its requests are released -- a
// released buffer must not be written afterwards.
int fail_launch(espgpu_ctx *c, Slot &s) {
  if (s.wq) stream_settle(c, s.wq);
  s.wq = nullptr;
  return ctx_fail(c, "batch launch failed");
}

// A slot's span list of at least `need` entries (the door's fixed layout
// keeps 3 x batch_records; a larger list moves the pinned buffer, so the
// door kernel is stopped first and the device slot table rewritten).
int xfer_reserve(espgpu_ctx *c, Slot &s, uint32_t need) {
  if (need <= s.xfer_cap) return 0;
  if (c->door_ctl) door_stop(c);
  hipHostFree(s.h_xfer);
  s.h_xfer = nullptr;
  s.xfer_cap = 0;
  const uint32_t cap = std::max(need, 256u) * 2;
  HIPCHK(c, hipHostMalloc((void **)&s.h_xfer, (size_t)cap * sizeof(XferSpan), hipHostMallocDefault));
  HIPCHK(c, hipHostGetDevicePointer((void **)&s.h_xfer_dev, s.h_xfer, 0));
  s.xfer_cap = cap;
  if (c->door_ctl) return door_write_slot(c, (size_t)(&s - c->slots.data()));
  return 0;
}

// The span lists of a batch whose kernel stages its own records (doorbell
// and fused paths): xin[rec] brings a record in from pinned staging or
// registered memory, xout[2 * rec + q] takes result span q back (n 0: none).
void stage_lists(const Slot &s, XferSpan *xin, XferSpan *xout, uint8_t *dres) {
  const uint64_t ha = (uint64_t)(uintptr_t)s.h_arena_dev, da = (uint64_t)(uintptr_t)s.d_arena;
  const uint64_t dr = (uint64_t)(uintptr_t)dres;
  for (const Pending &pd : s.reqs) {
    xin[pd.rec] = XferSpan{pd.zc ? pd.zc : ha + pd.stage_off, da + pd.stage_off, pd.stage_len, pd.rec};
    for (int q = 0; q < 2; ++q) {
      XferSpan &o = xout[2 * pd.rec + q];
      if (q < pd.nspan) {
        const ReqSpan &sp = pd.span[q];
        o = XferSpan{dr + pd.stage_off + sp.stage_from,
                     pd.zc ? pd.zc + sp.stage_from : ha + pd.stage_off + sp.stage_from, sp.n, pd.rec};
      } else {
        o = XferSpan{0, 0, 0, pd.rec};
      }
    }
  }
}

// The batch is now in flight (launched or published); the next slot fills.
void slot_launched(espgpu_ctx *c, Slot &s) {
  s.t_launch = now_ns();               // (the deadline counts from here: launch calls may load code)
  s.state = SLOT_INFLIGHT;
  c->stats.batches++;
  c->stats.zerocopy += s.nrec - s.nstaged;
  c->cur = (c->cur + 1) % (int)c->slots.size();
}

// Doorbell path (set_tuning "door"): a single-session GCM batch of up to
// gcm_burst records is published to the persistent kernel -- descriptors
// and span lists at the slot's fixed door offsets, then one 16-byte job in
// the ring -- with no HIP call at all; poll() sees done[] in host memory.
int launch_door(espgpu_ctx *c, Slot &s, uint8_t *dres) {
  int e = door_setup(c);
  if (e) return e;
  s.desc_off = door_desc_off(c);
  s.stat_off = door_stat_off(c);
  memcpy(s.h_arena + s.desc_off, s.h_desc, s.nrec * sizeof(espgpu_desc));
  stage_lists(s, s.h_xfer, s.h_xfer + c->cfg.batch_records, dres);
  // A kernel asked to retire (launched work went by) may still be running.
  // The request stands while that launched work is outstanding: the kernel
  // then serves the jobs published meanwhile and exits, so work queued
  // behind it on a shared hardware queue does not wait for door_idle_us.
  // Once the launched work is done the request is cancelled before the job
  // is visible.  A kernel that exited (the request, or an idle timeout since
  // the last job) is relaunched, which clears it.  All before the ring entry
  // is written, so a failed relaunch leaves nothing published.
  const uint64_t t_pub = now_ns();
  const bool was_retiring = c->door_retiring;
  if (was_retiring && launched_idle(c)) {
    __atomic_store_n(&c->door_ctl->stop, 0u, __ATOMIC_SEQ_CST);
    c->door_retiring = false;
  }
  if (!c->door_live || t_pub - c->door_last_pub > (uint64_t)c->door_idle_us * 500u ||
      (was_retiring && door_exited(c))) {
    e = door_ensure(c);
    if (e) return e;
  }
  const uint32_t j = c->door_next++;
  DoorJob &jb = c->door_ctl->ring[j % kDoorRing];
  const uint32_t so = (uint32_t)(&s - c->slots.data()) | ((uint32_t)s.op << 16);
  jb.n = s.nrec;
  jb.slot_op = so;
  jb.chk = s.nrec ^ so ^ (j + 1) ^ kDoorChk;
  __atomic_store_n(&jb.seq, j + 1, __ATOMIC_RELEASE);
  s.door_job = j;
  s.door_t0 = t_pub;
  c->door_last_pub = t_pub;
  s.timed = false;
  c->stats.door++;
  slot_launched(c, s);
  return 0;
}

// A small batch of one GCM session stages its own records: the kernel's
// workgroups copy each chunk's records in from the host (pinned staging or
// registered memory) and the results back, reading the descriptors and
// writing the statuses through the host mapping -- one launch per burst
// instead of copy, kernel, copy (set_tuning "stage_fused"; the small-batch
// GCM kernel, so not with gcm_lanes 4 forced)
int launch_fused(espgpu_ctx *c, Slot &s, uint8_t *dres) {
  int e = xfer_reserve(c, s, 3 * s.nrec);
  if (e) return e;
  stage_lists(s, s.h_xfer, s.h_xfer + s.nrec, dres);
  const StageLists stg{s.h_xfer_dev, s.h_xfer_dev + s.nrec, s.h_arena_dev + s.stat_off,
                       reinterpret_cast<const espgpu_desc *>(s.h_arena_dev + s.desc_off)};
  s.timed = GPU_TIME_SMALL;
  if (s.timed) hipEventRecord(s.k0, s.st);
  s.wq = s.st;                                     // the kernel writes results to host memory
#ifdef ESPGPU_BOUNDS
  espgpu_chk_arm(c, s.d_arena, s.bytes, s.op ? nullptr : s.d_out, s.bytes, 16);
#endif
  e = run_batch(c, s.d_arena, reinterpret_cast<const espgpu_desc *>(s.d_arena + s.desc_off), s.nrec,
                dres + s.stat_off, s.op ? nullptr : s.d_out, (uint32_t)ESPGPU_BATCH_GROUPED, s.op, s.st,
                nullptr, 1u, &stg);
  if (e) return e;
  if (s.timed) hipEventRecord(s.k1, s.st);
  HIPCHK(c, hipEventRecord(s.done, s.st));
  slot_launched(c, s);
  return 0;
}

// Copy or xfer kernel (kcopy) in, the crypto kernels, copy or xfer kernel out.
// Zero-copy records move by the xfer kernel on the compute stream either way.
int launch_copy(espgpu_ctx *c, Slot &s, bool small, bool kcopy, uint8_t *dres) {
  hipStream_t s_k = small ? s.st : c->stream;
  hipStream_t s_in = small ? s.st : c->s_in, s_out = small ? s.st : c->s_out;
  // region the copies move: all of it, or without records if every one is zero-copy
  const uint32_t in_lo = s.nstaged ? 0 : s.desc_off, out_lo = s.nstaged ? 0 : s.stat_off;
  const uint32_t out_hi = s.stat_off + s.nrec;
  auto pieces = [](uint32_t n) { return (n + kXferPiece - 1) / kXferPiece; };
  uint32_t nin = 0, nout = 0;
  for (const Pending &pd : s.reqs) {
    if (pd.zc) {
      nin += pieces(pd.stage_len);
      for (int k = 0; k < pd.nspan; ++k) nout += pieces(pd.span[k].n);
    } else if (kcopy) {
      nin += pieces(pd.stage_len);
      nout += pieces(pd.stage_len);
    }
  }
  if (kcopy) {
    nin += pieces(s.stat_off - s.desc_off);
    nout += pieces(s.nrec);
  }
  int e = xfer_reserve(c, s, nin + nout);
  if (e) return e;
  uint32_t k = 0;
  auto add = [&](uint64_t src, uint64_t dst, uint32_t n, uint32_t rec) {
    for (uint32_t o = 0; o < n; o += kXferPiece)
      s.h_xfer[k++] = XferSpan{src + o, dst + o, std::min(kXferPiece, n - o), rec};
  };
  const uint64_t ha = (uint64_t)(uintptr_t)s.h_arena_dev, da = (uint64_t)(uintptr_t)s.d_arena;
  const uint64_t dr = (uint64_t)(uintptr_t)dres;
  for (const Pending &pd : s.reqs)
    if (pd.zc) add(pd.zc, da + pd.stage_off, pd.stage_len, ~0u);
    else if (kcopy) add(ha + pd.stage_off, da + pd.stage_off, pd.stage_len, ~0u);
  if (kcopy) add(ha + s.desc_off, da + s.desc_off, s.stat_off - s.desc_off, ~0u);
  // results: only for records whose status is 0 (complete_slot's rule)
  for (const Pending &pd : s.reqs)
    if (pd.zc)
      for (int q = 0; q < pd.nspan; ++q)
        add(dr + pd.stage_off + pd.span[q].stage_from, pd.zc + pd.span[q].stage_from, pd.span[q].n, pd.rec);
    else if (kcopy) add(dr + pd.stage_off, ha + pd.stage_off, pd.stage_len, pd.rec);
  if (kcopy) add(dr + s.stat_off, ha + s.stat_off, s.nrec, ~0u);
  const uint8_t *d_stat = dres + s.stat_off;

  if (!kcopy) {
    HIPCHK(c, hipMemcpyAsync(s.d_arena + in_lo, s.h_arena + in_lo, s.stat_off - in_lo, hipMemcpyHostToDevice, s_in));
    if (!small) {
      HIPCHK(c, hipEventRecord(s.in_done, s_in));
      HIPCHK(c, hipStreamWaitEvent(s_k, s.in_done, 0));
    }
  }
  if (nin && launch_xfer(s.h_xfer_dev, nin, nullptr, s_k)) return fail(c, ESPGPU_EIO, "xfer kernel launch failed");
  // kernel timing events (stats.kernel_ns, espgpu_last_kernel_ms) only on
  // large batches: on a burst's own stream each marker adds to its latency
  s.timed = !small || GPU_TIME_SMALL;
  if (s.timed) hipEventRecord(s.k0, s_k);
  // a single-session batch skips the device planner (ESPGPU_BATCH_GROUPED:
  // one session trivially satisfies "one session per chunk")
#ifdef ESPGPU_BOUNDS
  espgpu_chk_arm(c, s.d_arena, s.bytes, s.op ? nullptr : s.d_out, s.bytes, 16);
#endif
  e = run_batch(c, s.d_arena, reinterpret_cast<const espgpu_desc *>(s.d_arena + s.desc_off), s.nrec,
                dres + s.stat_off, s.op ? nullptr : s.d_out, s.mixed ? 0u : (uint32_t)ESPGPU_BATCH_GROUPED,
                s.op, s_k, nullptr, s.kinds);
  if (e) return e;
  if (s.timed) hipEventRecord(s.k1, s_k);
  if (nout) s.wq = s_k;                          // results to host memory (zero-copy / staging)
  if (nout && launch_xfer(s.h_xfer_dev + nin, nout, d_stat, s_k)) return fail(c, ESPGPU_EIO, "xfer kernel launch failed");
  if (!kcopy) {
    if (!small) {
      HIPCHK(c, hipEventRecord(s.kout, s_k));
      HIPCHK(c, hipStreamWaitEvent(s_out, s.kout, 0));
    }
    HIPCHK(c, hipMemcpyAsync(s.h_arena + out_lo, dres + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, s_out));
  }
  HIPCHK(c, hipEventRecord(s.done, kcopy ? s_k : s_out));
  slot_launched(c, s);
  return 0;
}

// Launch one filled slot: its staging region and zero-copy records in, the
// crypto kernels, the results out; then the next slot becomes current.
int launch_slot(espgpu_ctx *c, Slot &s) {
  if (s.state != SLOT_FILLING || s.nrec == 0) return 0;
  s.wq = nullptr;
  if (take_launch_fault(c)) return ESPGPU_EIO;
  if (c->fault & ESPGPU_FAULT_STUCK) {            // its completion will never be seen
    c->fault &= ~(uint32_t)ESPGPU_FAULT_STUCK;
    s.stuck = true;
  }
  // [records][16 B slack][descriptors][status]: one H2D on s_in -> kernels on
  // the compute stream -> one D2H on s_out, chained by events, so consecutive
  // batches overlap their copies with each other's kernels.
  s.desc_off = s.bytes + 16;
  s.stat_off = s.desc_off + s.nrec * (uint32_t)sizeof(espgpu_desc);
  memset(s.h_arena + s.bytes, 0, 16);
  memcpy(s.h_arena + s.desc_off, s.h_desc, s.nrec * sizeof(espgpu_desc));
  // A small batch (an RX burst) runs in order on its slot's own stream:
  // cross-stream event hand-offs cost more latency than the copies; the next
  // slot's burst overlaps on the other slot's stream (kernels stay ordered
  // through run_batch's last-launch event).  Its staging region moves by the
  // xfer kernel (set_tuning "xfer", default) or hipMemcpyAsync.  Large
  // batches use the three ctx streams so batch k+1's H2D overlaps batch k's
  // kernels and batch k-1's D2H.
  const bool small = s.stat_off <= kSmallBatchBytes;
  const bool kcopy = small && c->xfer_small;
  uint8_t *dres = s.op ? s.d_arena : s.d_out;      // records out: in place (encrypt) or d_out
  // one GCM session, and not with gcm_lanes 4 forced: the doorbell and fused
  // paths run the small-batch GCM kernel
  const bool one_gcm = !s.mixed && s.kinds == 1 && c->gcm_lanes != kGcmLanesPerRec;
  if (c->door_wg && one_gcm && s.nrec <= c->gcm_burst) return launch_door(c, s, dres);
  door_retire(c);                                  // launched work from here on
  if (small && c->stage_fused && one_gcm) return launch_fused(c, s, dres);
  return launch_copy(c, s, small, kcopy, dres);
}

int complete_slot(espgpu_ctx *c, Slot &s) {
  float ms = 0.f;
  if (s.timed && hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) {
    c->last_ms = ms;
    c->stats.kernel_ns += (uint64_t)(ms * 1e6);
  }
  for (auto &pd : s.reqs) {
    int et = pd.etype_pre >= 0 ? pd.etype_pre : (int)s.h_arena[s.stat_off + pd.rec];
    if (et == 0) {
      const uint8_t *src = s.h_arena + pd.stage_off;
      for (int k = 0; k < pd.nspan && !pd.zc; ++k)     // zero-copy: the xfer kernel wrote them
        seg_copy_in(s.segpool.data() + pd.seg0, pd.nsegs, pd.span[k].buf_off, pd.span[k].n,
                    src + pd.span[k].stage_from);
      c->stats.bytes += pd.span[0].n;
    } else if (et == ESPGPU_EBADMSG) {
      c->stats.auth_fail++;
    } else {
      c->stats.einval++;
    }
    c->stats.records++;
    c->ready.push_back(espgpu_completion{pd.opaque, et});
  }
  s.reqs.clear();
  s.segpool.clear();
  s.nrec = 0;
  s.bytes = 0;
  s.state = SLOT_FREE;
  return 0;
}

}  // namespace
}  // namespace espgpu

using namespace espgpu;

extern "C" {

int espgpu_abi_version(void) { return ESPGPU_ABI_VERSION; }

int espgpu_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : ESPGPU_ENODEV;
}

const char *espgpu_last_error(espgpu_ctx *c) { return c ? c->err.c_str() : "no context"; }

int espgpu_health(espgpu_ctx *c) {
  if (!c) return ESPGPU_EINVAL;
  return c->failed ? ESPGPU_EIO : ESPGPU_OK;
}

int espgpu_init(const espgpu_config *cfg_in, espgpu_ctx **out) {
  if (!out) return ESPGPU_EINVAL;
  *out = nullptr;
  espgpu_ctx *c = new espgpu_ctx();
  espgpu_config cfg{};
  if (cfg_in) cfg = *cfg_in;
  if (!cfg.max_sessions) cfg.max_sessions = 1024;
  if (!cfg.batch_records) cfg.batch_records = 65536;
  if (!cfg.batch_bytes) cfg.batch_bytes = 64u << 20;
  if (!cfg.nbatches) cfg.nbatches = 2;
  c->cfg = cfg;
  c->device = cfg.device;
  int rc = 0;
  do {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg.device) {
      rc = fail(c, ESPGPU_ENODEV, "no HIP device %d (found %d)", cfg.device, ndev);
      break;
    }
    if (hipSetDevice(cfg.device) != hipSuccess) { rc = fail(c, ESPGPU_ENODEV, "hipSetDevice failed"); break; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking) != hipSuccess) {
      rc = fail(c, ESPGPU_EIO, "stream");
      break;
    }
    for (int k = 0; k < 2; ++k) {
      hipEventCreateWithFlags(&c->e2e_in[k], hipEventDisableTiming);
      hipEventCreateWithFlags(&c->e2e_k[k], hipEventDisableTiming);
    }
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming);
    c->ready.reserve((size_t)cfg.batch_records * cfg.nbatches + 1024);
    if (hipMalloc(&c->d_sas, (size_t)cfg.max_sessions * sizeof(DevSA)) != hipSuccess ||
        hipMalloc(&c->d_gtab, (size_t)cfg.max_sessions * kGhTableBytes) != hipSuccess ||
        hipMalloc(&c->d_tpair, 256 * sizeof(uint2)) != hipSuccess ||
        hipMalloc(&c->d_dpair, 256 * sizeof(uint2)) != hipSuccess ||
        hipMalloc(&c->d_isbox, 256) != hipSuccess ||
        hipMalloc(&c->d_queue, 4 * kQueueRegionWords * 4) != hipSuccess) {
      rc = fail(c, ESPGPU_ENOMEM, "device SA table allocation failed");
      break;
    }
    hipMemset(c->d_sas, 0, (size_t)cfg.max_sessions * sizeof(DevSA));
    hipMemset(c->d_queue, 0, 4 * kQueueRegionWords * 4);
    const hc::Tables &t = hc::tables();
    uint2 tp[256], dp[256];
    for (int x = 0; x < 256; ++x) {
      tp[x] = make_uint2(t.te0[x], (t.te0[x] >> 8) | (t.te0[x] << 24));
      dp[x] = make_uint2(t.td0[x], (t.td0[x] >> 8) | (t.td0[x] << 24));
    }
    hipMemcpy(c->d_tpair, tp, sizeof tp, hipMemcpyHostToDevice);
    hipMemcpy(c->d_dpair, dp, sizeof dp, hipMemcpyHostToDevice);
    hipMemcpy(c->d_isbox, t.isbox, 256, hipMemcpyHostToDevice);
    c->slots.resize(cfg.nbatches);
    for (auto &s : c->slots)
      if ((rc = alloc_slot(c, s))) break;
  } while (0);
  if (rc) {
    fprintf(stderr, "espgpu_init: %s\n", c->err.c_str());
    espgpu_fini(c);
    return rc;
  }
  *out = c;
  return 0;
}

void espgpu_fini(espgpu_ctx *c) {
  if (!c) return;
  if (c->failed) {
    // nothing waits unboundedly on a failed device: work that may still run
    // on it (a hung kernel) keeps its memory, which is then leaked rather
    // than freed under it
    bool idle = true;
    const uint64_t t0 = now_ns();
    while (c->door_live && !door_exited(c)) {
      if (now_ns() - t0 > (uint64_t)c->deadline_ms * 1000000ull) { idle = false; break; }
      sched_yield();
    }
    for (hipStream_t st : {c->s_in, c->stream, c->s_out}) idle = stream_settle(c, st) && idle;
    for (auto &s : c->slots) idle = stream_settle(c, s.st) && idle;
    if (!idle) {
      fprintf(stderr, "espgpu_fini: device work of a failed context never finished; its memory is leaked\n");
      delete c;
      return;
    }
  }
  door_free(c);
  for (hipStream_t st : {c->s_in, c->stream, c->s_out})
    if (st) hipStreamSynchronize(st);
  for (auto &s : c->slots) free_slot(s);
  for (const HostRegion &r : c->regions)
    if (r.owned) hipHostUnregister((void *)r.base);
  hipFree(c->e2e_arena); hipFree(c->e2e_out); hipFree(c->e2e_status); hipFree(c->e2e_desc);
  for (int k = 0; k < 2; ++k) {
    if (c->e2e_in[k]) hipEventDestroy(c->e2e_in[k]);
    if (c->e2e_k[k]) hipEventDestroy(c->e2e_k[k]);
  }
  hipFree(c->d_sas); hipFree(c->d_gtab); hipFree(c->d_tpair); hipFree(c->d_dpair); hipFree(c->d_isbox);
  hipFree(c->d_queue);
#ifdef ESPGPU_BOUNDS
  hipFree(c->chk.rep);
#endif
  hipFree(c->d_ej0);
  hipFree(c->d_work); hipFree(c->d_order); hipFree(c->d_chunks); hipFree(c->d_nchunks);
  hipFree(c->d_stage_ws);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->ev_last) hipEventDestroy(c->ev_last);
  for (hipStream_t st : {c->s_in, c->stream, c->s_out})
    if (st) hipStreamDestroy(st);
  delete c;
}

// Check a request against the ESP / AH request rule (req_shape.h: req_plan)
// and stage it as a wire record: in the filling slot, in the host overflow,
// or not at all (ERESTART).
int espgpu_process(espgpu_ctx *c, const espgpu_req *r, int hint) {
  (void)hint;
  if (!c || !r) return ESPGPU_EINVAL;
  if (c->failed) {
    // never ERESTART (nothing would retry it into a working slot) nor EAGAIN:
    // the caller completes it at once (ff_gpucrypto.c)
    c->stats.fail_eio++;
    return ESPGPU_EIO;
  }
  auto reject = [&](int etype) {
    c->ready.push_back(espgpu_completion{r->opaque, etype});
    if (etype == ESPGPU_EINVAL) c->stats.einval++;
    return 0;
  };
  const int sid = r->session;
  if (sid < 0 || (size_t)sid >= c->sessions.size() || !c->sessions[sid].used) return reject(ESPGPU_EINVAL);
  ReqPlan pl;
  if (req_plan(c->sessions[sid], *r, c->cfg.batch_bytes, &pl)) return reject(ESPGPU_EINVAL);
  const int op = pl.op;
  const uint32_t rlen = pl.rlen;
  // Zero-copy when the whole record lies in one segment of registered memory
  // with the layout the kernels read (the staged path takes a GCM record's
  // header and IV from crp_aad / crp_iv: they must equal the buffer's).
  uint64_t zc = 0;
  if (!c->regions.empty()) {
    const uint8_t *rp = seg_span(r->segs, (uint32_t)r->nsegs, pl.rec_start, rlen);
    if (rp && (!pl.gcm_gather || (memcmp(rp, pl.hdr, 8) == 0 && memcmp(rp + 8, r->crp_iv + 4, 8) == 0)))
      zc = region_dev(c, rp, rlen);
  }
  // (rec, stage_off, seg0 and off4 are set where the request is placed)
  Pending pd{r->opaque, -1, 0, 0, rlen, {pl.span[0], pl.span[1]}, pl.nspan, 0, (uint32_t)r->nsegs, zc};
  espgpu_desc d{0, (uint16_t)rlen, (uint16_t)sid, pl.esn_hi, pl.salt};
  // Where it goes: the filling slot; the overflow when the slots are all in
  // flight (or the overflow already holds requests: arrival order is kept);
  // else ERESTART.
  Slot *s = &c->slots[c->cur];
  bool to_ovf = !c->ovf.empty();
  if (!to_ovf) {
    if (slot_full(c, *s, op, rlen)) {
      int e = espgpu_flush(c);
      if (e) {
        if (c->failed) c->stats.fail_eio++;     // (this request: refused, completed by the caller)
        return e;
      }
      s = &c->slots[c->cur];
    }
    if (s->state == SLOT_INFLIGHT) {
      if (!c->ovf_cap) { c->stats.erestart++; return ESPGPU_ERESTART; }
      to_ovf = true;
    }
  }
  if (to_ovf) {
    // fixed rings reserved at set_tuning: nothing here allocates or moves
    const uint64_t t_in = now_ns();
    Overflow &o = c->ovf;
    const size_t blen = zc ? 0 : ((rlen + 15) & ~15u);
    if (o.count == o.ecap) { c->stats.erestart++; return ESPGPU_ERESTART; }
    const auto bm = o.bytes.mark();
    const auto sm = o.segpool.mark();
    const size_t boff = o.bytes.alloc(blen), soff = o.segpool.alloc((size_t)r->nsegs);
    if (boff == SIZE_MAX || soff == SIZE_MAX) {
      o.bytes.undo(bm);
      o.segpool.undo(sm);
      c->stats.erestart++;
      return ESPGPU_ERESTART;
    }
    pd.stage_off = (uint32_t)boff;
    if (!zc && !req_gather(pl, *r, o.bytes.buf.get() + boff)) {
      o.bytes.undo(bm);
      o.segpool.undo(sm);
      return reject(ESPGPU_EINVAL);
    }
    pd.seg0 = (uint32_t)soff;
    if (r->nsegs) memcpy(o.segpool.buf.get() + soff, r->segs, (size_t)r->nsegs * sizeof(espgpu_seg));
    o.ent[(o.head + o.count) % o.ecap] = OvfEntry{pd, d, sid, (uint8_t)op, pl.kind};
    o.count++;
    o.live_bytes += blen;
    o.peak_bytes = std::max(o.peak_bytes, o.live_bytes);
    c->stats.overflow++;
    c->stats.ovf_process_ns_max = std::max(c->stats.ovf_process_ns_max, now_ns() - t_in);
    return 0;
  }
  if (!zc && !req_gather(pl, *r, s->h_arena + s->bytes)) return reject(ESPGPU_EINVAL);
  slot_commit(*s, pd, d, r->segs, sid, op, pl.kind);
  return 0;
}

int espgpu_flush(espgpu_ctx *c) {
  if (!c) return ESPGPU_EINVAL;
  if (c->failed) return ESPGPU_EIO;
  // the filling slot, then the overflow (oldest first) into the free slots
  Overflow &o = c->ovf;
  for (;;) {
    Slot &s = c->slots[c->cur];
    if (s.state == SLOT_FILLING) {
      // a batch that cannot be launched is a GPU failure: its requests, the
      // overflow's and (through poll) the in-flight ones complete with EIO
      if (launch_slot(c, s)) return fail_launch(c, s);
      continue;
    }
    if (o.empty() || s.state != SLOT_FREE) break;
    while (!o.empty()) {
      const OvfEntry &en = o.front();
      if (slot_full(c, s, en.op, en.pd.stage_len)) break;
      if (!en.pd.zc) memcpy(s.h_arena + s.bytes, o.bytes.buf.get() + en.pd.stage_off, en.pd.stage_len);
      slot_commit(s, en.pd, en.d, o.segpool.buf.get() + en.pd.seg0, en.sid, en.op, en.kind);
      o.pop();
    }
  }
  return 0;
}

int espgpu_poll(espgpu_ctx *c, espgpu_completion *out, int max) {
  if (!c) return -ESPGPU_EINVAL;
  // completions of flushed batches, oldest first, and in arrival order: a
  // batch that finished before an older one (another stream's kernel, a
  // doorbell job another workgroup took) waits for it
  // (a batch whose completion fails, or that outlives deadline_ms, fails the
  // ctx and completes with EIO: slot_check)
  bool door_wait = false;
  const uint64_t now = now_ns();
  for (size_t k = 0; k < c->slots.size(); ++k) {
    Slot &s = c->slots[(c->cur + k) % c->slots.size()];
    if (s.state != SLOT_INFLIGHT) continue;
    const int r = slot_check(c, s, now);
    if (r == 0) {
      // a doorbell job outstanding for over 100 us: make sure the kernel is
      // still there (a workgroup that read a retire request just before the
      // job was published may have exited with it)
      door_wait = s.door_job >= 0 && now - s.door_t0 > 100000u;
      break;
    }
    if (r < 0) {
      drop_slot(c, s);
      continue;
    }
    s.door_job = -1;
    complete_slot(c, s);
  }
  if (door_wait && !c->failed && door_ensure(c)) ctx_fail(c, "door kernel relaunch failed");
  const int avail = (int)(c->ready.size() - c->ready_head);
  const int n = std::min(max, avail);
  for (int i = 0; i < n; ++i) out[i] = c->ready[c->ready_head + i];
  c->ready_head += n;
  if (c->ready_head == c->ready.size()) {
    c->ready.clear();
    c->ready_head = 0;
  }
  return n;
}

int espgpu_drain(espgpu_ctx *c) {
  if (!c) return ESPGPU_EINVAL;
  do {
    espgpu_flush(c);              // (a launch failure fails the ctx: the loop below retires the rest)
    // oldest first (slot cur is the next to fill, so cur+1.. are older
    // batches); every wait is bounded by deadline_ms (slot_check), so a
    // batch the GPU never finishes completes with EIO instead of hanging
    for (size_t k = 0; k < c->slots.size(); ++k) {
      Slot &s = c->slots[(c->cur + k) % c->slots.size()];
      if (s.state != SLOT_INFLIGHT) continue;
      int r;
      while ((r = slot_check(c, s, now_ns())) == 0) {
        // the persistent kernel's job: relaunch the kernel if it exited
        if (s.door_job >= 0 && !c->failed && door_ensure(c)) ctx_fail(c, "door kernel relaunch failed");
        sched_yield();
      }
      if (r < 0) {
        drop_slot(c, s);
        continue;
      }
      s.door_job = -1;
      complete_slot(c, s);
    }
  } while (!c->ovf.empty());     // the overflow goes into the slots just freed
  return c->failed ? ESPGPU_EIO : 0;
}

int espgpu_register_host(espgpu_ctx *c, void *base, uint64_t len) {
  if (!c || !base || !len) return ESPGPU_EINVAL;
  const uintptr_t b = (uintptr_t)base;
  for (const HostRegion &r : c->regions)
    if (b < r.base + r.len && r.base < b + len) return fail(c, ESPGPU_EINVAL, "overlaps a registered region");
  bool owned = true;
  hipError_t e = hipHostRegister(base, len, hipHostRegisterMapped);
  if (e == hipErrorHostMemoryAlreadyRegistered) {
    owned = false;                   // already pinned (hipHostMalloc): only map it
    (void)hipGetLastError();
  } else if (e != hipSuccess) {
    return fail(c, ESPGPU_EIO, "hipHostRegister: %s", hipGetErrorString(e));
  }
  void *dp = nullptr;
  if (hipHostGetDevicePointer(&dp, base, 0) != hipSuccess || !dp) {
    if (owned) hipHostUnregister(base);
    return fail(c, ESPGPU_EIO, "hipHostGetDevicePointer failed");
  }
  HostRegion r{b, len, (uint64_t)(uintptr_t)dp, owned};
  c->regions.insert(std::upper_bound(c->regions.begin(), c->regions.end(), r,
                                     [](const HostRegion &x, const HostRegion &y) { return x.base < y.base; }),
                    r);
  return 0;
}

int espgpu_unregister_host(espgpu_ctx *c, void *base) {
  if (!c) return ESPGPU_EINVAL;
  auto it = std::find_if(c->regions.begin(), c->regions.end(),
                         [&](const HostRegion &r) { return r.base == (uintptr_t)base; });
  if (it == c->regions.end()) return ESPGPU_EINVAL;
  // requests staged from it run to completion first (their completions wait for poll)
  int e = espgpu_drain(c);
  if (e) return e;
  if (it->owned) hipHostUnregister(base);
  c->regions.erase(it);
  return 0;
}

int espgpu_get_stats(espgpu_ctx *c, espgpu_stats *st) {
  if (!c || !st) return ESPGPU_EINVAL;
  *st = c->stats;
  st->ovf_reserved = c->ovf.reserved();
  st->ovf_peak = c->ovf.peak_bytes;
  return 0;
}

int espgpu_set_tuning(espgpu_ctx *c, const char *key, int value) {
  if (key && !strcmp(key, "ah_offer")) {           // process-wide: no context needed
    if (value < -1 || value > 1) return ESPGPU_EINVAL;
    g_ah_offer = value;
    return 0;
  }
  if (!c || !key) return ESPGPU_EINVAL;
  if (!strcmp(key, "grid")) { c->cfg.grid = (uint32_t)value; return 0; }
  if (!strcmp(key, "gcm_lanes")) {
    if (value != 0 && value != kGcmLanesPerRec && value != kGcmLanesSmall) return ESPGPU_EINVAL;
    c->gcm_lanes = value;
    return 0;
  }
  if (!strcmp(key, "overflow_mb")) {
    // offsets into the overflow's byte buffer are 32-bit (Pending::stage_off)
    if (value < 0 || value > 4095) return ESPGPU_EINVAL;
    // the rings are reserved whole here: growing the overflow inside
    // process() would copy it (hundreds of microseconds at a few MiB).
    // Resizing drains what the old rings hold first.
    if (!c->ovf.empty()) {
      int e = espgpu_drain(c);
      if (e) return e;
    }
    // all three rings or none: on ENOMEM the previous overflow stays
    if (!c->ovf.init((size_t)value << 20))
      return fail(c, ESPGPU_ENOMEM, "overflow_mb %d: host allocation failed", value);
    c->ovf_cap = (size_t)value << 20;
    return 0;
  }
  if (!strcmp(key, "fault")) {
    // fault injection (tests of the GPU-failure path): ESPGPU_FAULT_* bits,
    // each consumed by the next launch / completion query / launched batch
    if (value & ~(ESPGPU_FAULT_LAUNCH | ESPGPU_FAULT_QUERY | ESPGPU_FAULT_STUCK)) return ESPGPU_EINVAL;
    c->fault = (uint32_t)value;
    return 0;
  }
  if (!strcmp(key, "deadline_ms")) {
    if (value < 1 || value > 600000) return ESPGPU_EINVAL;
    c->deadline_ms = (uint32_t)value;
    return 0;
  }
  if (!strcmp(key, "natt_lanes")) {
    if (value != 0 && value != 8 && value != 16 && value != 32) return ESPGPU_EINVAL;
    c->natt_lanes = (uint32_t)value;
    return 0;
  }
  if (!strcmp(key, "gcm_burst")) {
    if (value < 0) return ESPGPU_EINVAL;
    c->gcm_burst = (uint32_t)value;
    return 0;
  }
  if (!strcmp(key, "stage_fused")) {
    if (value != 0 && value != 1) return ESPGPU_EINVAL;
    c->stage_fused = value;
    return 0;
  }
  if (!strcmp(key, "xfer")) {
    if (value != 0 && value != 1) return ESPGPU_EINVAL;
    c->xfer_small = value;
    return 0;
  }
  if (!strcmp(key, "door")) {
    // workgroups of the doorbell kernel (0 = off); changing it drains and
    // stops the running kernel (the next batch relaunches it)
    if (value < 0 || value > 256) return ESPGPU_EINVAL;
    if (value != c->door_wg && c->door_ctl) {
      int e = espgpu_drain(c);
      if (e) return e;
      door_stop(c);
    }
    c->door_wg = value;
    return value ? door_setup(c) : 0;
  }
  if (!strcmp(key, "door_idle_us")) {
    if (value < 100 || value > 10000000) return ESPGPU_EINVAL;
    door_stop(c);
    c->door_idle_us = (uint32_t)value;
    return 0;
  }
  if (!strcmp(key, "gcm_opts")) return set_gcm_opts((uint32_t)value) ? ESPGPU_ENOTSUP : 0;
  if (!strcmp(key, "eta_opts")) return set_eta_opts((uint32_t)value) ? ESPGPU_ENOTSUP : 0;
  return ESPGPU_ENOENT;
}

}  // extern "C"
