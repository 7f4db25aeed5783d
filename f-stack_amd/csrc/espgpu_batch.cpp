// espgpu_batch.cpp — the kernel launches of the host runtime (espgpu_ctx.h):
// run_batch, the device-resident batch entry points with their single-record
// counterparts beside them (the rules are classify.h's, decap.h's, encap.h's,
// frame.h's, natt.h's and replay.h's), and the host-to-host pipeline.
#include "espgpu_ctx.h"

#include "ah_in.h"         // (after the HIP runtime's vector types)
#include "ah_out.h"
#include "classify.h"
#include "decap.h"
#include "encap.h"
#include "frame.h"
#include "natt.h"
#include "replay.h"

namespace espgpu {
namespace {

int ensure_plan(espgpu_ctx *c, uint32_t n) {
  const uint32_t need_chunks = plan_max_chunks(n, c->cfg.max_sessions);
  if (n <= c->plan_cap && need_chunks <= c->max_chunks) return 0;
  hipFree(c->d_work);
  hipFree(c->d_order);
  hipFree(c->d_chunks);
  hipFree(c->d_nchunks);
  c->plan_cap = std::max(n, 1024u);
  c->max_chunks = plan_max_chunks(c->plan_cap, c->cfg.max_sessions);
  // key histograms sized for the SA table's capacity: sessions created after
  // this allocation must not outgrow it
  HIPCHK(c, hipMalloc(&c->d_work, plan_workspace_words(c->cfg.max_sessions) * 4));
  HIPCHK(c, hipMalloc(&c->d_order, (size_t)c->plan_cap * 4));
  HIPCHK(c, hipMalloc(&c->d_chunks, (size_t)c->max_chunks * sizeof(Chunk)));
  HIPCHK(c, hipMalloc(&c->d_nchunks, 16));
  c->plan_dirty = true;
  return 0;
}

// Around the launches that use what is per ctx (work-queue counters, planner
// and stage workspaces): stream-ordered after the ctx's last launch, which
// this one then becomes.
int launch_begin(espgpu_ctx *c, hipStream_t st) {
  if (c->launched && st != c->last_st) HIPCHK(c, hipStreamWaitEvent(st, c->ev_last, 0));
  return 0;
}
int launch_end(espgpu_ctx *c, hipStream_t st) {
  HIPCHK(c, hipEventRecord(c->ev_last, st));
  c->last_st = st;
  c->launched = true;
  return 0;
}

#ifdef ESPGPU_BOUNDS
int chk_report_reset(espgpu_ctx *c) {
  if (!c->chk.rep) {
    HIPCHK(c, hipMalloc(&c->chk.rep, sizeof(ChkReport)));
  }
  ChkReport zero{};
  zero.hw[0] = zero.hw[1] = kChkNoMark;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(c->chk.rep, &zero, sizeof zero, hipMemcpyHostToDevice));
  return 0;
}

// What the launches of one run_batch are checked against: the armed extents
// (consumed) or none, and the index bounds run_batch knows.
int chk_take(espgpu_ctx *c, uint32_t n, uint32_t nsas, uint32_t nchunks, ChkArm *out) {
  if (!c->chk.rep) {
    int e = chk_report_reset(c);
    if (e) return e;
  }
  if (!c->chk_armed) c->chk.lo[0] = c->chk.lo[1] = c->chk.hi[0] = c->chk.hi[1] = 0;
  c->chk_armed = false;
  c->chk.n = n;
  c->chk.nsas = nsas;
  c->chk.nchunks = nchunks;
  *out = c->chk;
  return 0;
}
#endif

}  // namespace

// Launch the crypto kernels for one batch of device-resident records.
// kinds: which kernels the batch needs (1 GCM, 2 ETA); the device-resident
// entry points do not know and pass both, with 8: DIGEST (AH) records under
// the batch path's semantics.  4: a process-path batch with DIGEST requests
// (swcr_authcompute's semantics: DigestParams::op 2).
int run_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n, uint8_t *d_status,
              uint8_t *d_out, uint32_t flags, int encrypt, hipStream_t st, uint32_t *d_trailer, uint32_t kinds,
              const StageLists *stage, uint32_t out_stride) {
  if (c->failed) return ESPGPU_EIO;
  if (n == 0) return 0;
  if (out_stride && (c->n_eta > 0 || c->n_dig > 0))
    return fail(c, ESPGPU_ENOTSUP, "packed output serves contexts with GCM sessions only");
  if (take_launch_fault(c)) return ESPGPU_EIO;
  door_retire(c);
  int e = launch_begin(c, st);
  if (e) return e;
  const uint32_t nsas = (uint32_t)c->sessions.size();
  GcmParams p{};
  p.arena = d_arena;
  p.out = encrypt ? d_arena : (d_out ? d_out : d_arena);
  p.desc = d_desc;
  p.n = n;
  p.sas = c->d_sas;
  p.gtab = c->d_gtab;
  p.tpair = c->d_tpair;
  p.status = d_status;
  p.nsas = nsas;
  p.queue = c->d_queue;
  p.trailer = encrypt ? nullptr : d_trailer;
  p.out_stride = out_stride;
  if (stage) {
    p.xin = stage->xin;
    p.xout = stage->xout;
    p.hstat = stage->hstat;
    p.hdesc = stage->hdesc;
  }
  if (!(flags & ESPGPU_BATCH_GROUPED)) {
    if ((e = ensure_plan(c, n))) return e;
    // the key counts start at zero: plan_scatter zeroes them after use, so
    // only a fresh workspace (or one a failed launch left behind) needs it
    if (c->plan_dirty) {
      HIPCHK(c, hipMemsetAsync(c->d_work, 0, plan_workspace_words(c->cfg.max_sessions) * 4, st));
      c->plan_dirty = false;
    }
    if (launch_plan(d_desc, n, c->d_sas, nsas, c->cfg.max_sessions, c->d_work, c->d_order, c->d_chunks, c->d_nchunks,
                    c->max_chunks, st)) {
      c->plan_dirty = true;
      return fail(c, ESPGPU_EIO, "planner launch failed (%u sessions)", nsas);
    }
    p.order = c->d_order;
    p.chunks = c->d_chunks;
    p.nchunks = c->d_nchunks;
  }
#ifdef ESPGPU_BOUNDS
  if ((e = chk_take(c, n, nsas, p.chunks ? c->max_chunks : 0u, &p.chk))) return e;
#endif
  const int in_place = (!encrypt && p.out == d_arena);
  // E_K(J0) scratch: the burst kernel (small batches of <= gcm_burst records,
  // out of place or encrypt; launch_gcm picks the kernel from it)
  const bool gsmall = c->gcm_lanes ? c->gcm_lanes == kGcmLanesSmall : n < kGcmSmallBatch;
  // (packed output: the fused kernel only)
  if ((kinds & 1) && !out_stride &&
      gsmall && !in_place && n <= c->gcm_burst) {
    if (n > c->ej0_cap) {
      hipFree(c->d_ej0);
      c->d_ej0 = nullptr;
      c->ej0_cap = 0;
      HIPCHK(c, hipMalloc(&c->d_ej0, (size_t)n * sizeof(uint4)));
      c->ej0_cap = n;
    }
    p.ej0 = c->d_ej0;
  }
  // beside a running doorbell kernel (one workgroup per CU on door_wg CUs)
  // the other kernels take the remaining CUs: every workgroup of theirs must
  // run for the launch to finish
  int grid = c->cfg.grid ? (int)c->cfg.grid : 256;
  if (c->door_live && !door_exited(c)) grid = std::max(1, grid - c->door_wg);
  // A context without GCM sessions still launches the GCM kernel for the
  // records whose session is invalid (EINVAL; the planner chunks them with the
  // GCM records), but a few workgroups do: the others would only draw a
  // ticket past the end (cfg3: ~9 us -> ~3 us per batch)
  const int ggrid = c->n_gcm > 0 ? grid : std::min(grid, 16);
  if ((kinds & 1) && launch_gcm(p, encrypt, in_place, ggrid, c->gcm_lanes, st))
    return fail(c, ESPGPU_EIO, "GCM kernel launch failed");
  if ((kinds & 2) && c->n_eta > 0) {
    EtaParams q{};
    q.arena = d_arena;
    q.out = p.out;
    q.desc = d_desc;
    q.order = p.order;
    q.chunks = p.chunks;
    q.nchunks = p.nchunks;
    q.queue = c->d_queue + kQueueRegionWords;
    q.trailer = p.trailer;
    q.n = n;
    q.sas = c->d_sas;
    q.tpair = c->d_tpair;
    q.dpair = c->d_dpair;
    q.isbox = c->d_isbox;
    q.status = d_status;
    q.nsas = nsas;
    const int ek = (c->n_cbc > 0 ? 1 : 0) | (c->n_ctr > 0 ? 2 : 0) | (c->n_wcbc > 0 ? 4 : 0) |
                   (c->n_wctr > 0 ? 8 : 0) | (c->n_whash > 0 ? 16 : 0);
    if (launch_eta(q, encrypt, ek, grid, st))
      return fail(c, ESPGPU_EIO, "ETA kernel launch failed");
  }
  // AH digest sessions: launched only while the context has some
  if (c->n_dig > 0 && (kinds & 12)) {
    DigestParams g{};
    g.arena = d_arena;
    g.icv_out = p.out;
    g.desc = d_desc;
    g.order = p.order;
    g.chunks = p.chunks;
    g.nchunks = p.nchunks;
    g.queue = c->d_queue + 3 * kQueueRegionWords;
    g.trailer = p.trailer;
    g.n = n;
    g.sas = c->d_sas;
    g.status = d_status;
    g.nsas = nsas;
    g.op = (kinds & 4) ? 2u : (encrypt ? 1u : 0u);
#ifdef ESPGPU_BOUNDS
    g.chk = p.chk;
#endif
    if (launch_digest(g, c->n_dig > c->n_dig_wide, c->n_dig_wide > 0, grid, st))
      return fail(c, ESPGPU_EIO, "digest kernel launch failed");
  }
  return launch_end(c, st);
}

namespace {

// The device-resident entry points: a launch that could not be queued (EIO)
// fails the ctx as a process-path launch does (later calls answer EIO).
int batch_rc(espgpu_ctx *c, int e) {
  if (e == ESPGPU_EIO && !c->failed) ctx_fail(c, "batch launch failed");
  return e;
}

// The workspace of the stages that group by SA: it grows to the largest
// request and is kept.  An allocation that fails is ENOMEM with nothing
// launched and the ctx healthy.
int ensure_stage_ws(espgpu_ctx *c, size_t bytes) {
  if (c->d_stage_ws && bytes <= c->stage_ws_bytes) return 0;
  hipFree(c->d_stage_ws);                // (waits for the launches that use it)
  c->d_stage_ws = nullptr;
  c->stage_ws_bytes = 0;
  if (hipMalloc(&c->d_stage_ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->d_stage_ws = nullptr;
    return fail(c, ESPGPU_ENOMEM, "replay update workspace: %zu bytes of device memory not available", bytes);
  }
  c->stage_ws_bytes = bytes;
  return 0;
}

// What the device-resident stages share around their launches.  ws_bytes != 0:
// the stage works in the ctx's workspace, so it is stream-ordered after the
// ctx's last launch and becomes it; 0: nothing of the ctx's is written, the
// caller's stream alone orders it.  `launch` returns nonzero if it could not
// queue; `what` is then the message.
template <class Launch>
int run_stage(espgpu_ctx *c, uint32_t n, size_t ws_bytes, hipStream_t st, const char *what, Launch launch) {
  if (c->failed) return ESPGPU_EIO;
  if (n == 0) return 0;
  int e = ws_bytes ? ensure_stage_ws(c, ws_bytes) : 0;
  if (e) return e;
  if (take_launch_fault(c)) return batch_rc(c, ESPGPU_EIO);
  if (ws_bytes && (e = launch_begin(c, st))) return batch_rc(c, e);
  if (launch()) return batch_rc(c, fail(c, ESPGPU_EIO, "%s", what));
  return ws_bytes ? batch_rc(c, launch_end(c, st)) : 0;
}

int host_pipeline(espgpu_ctx *c, const uint8_t *h_arena, uint64_t arena_bytes,
                  const espgpu_desc *h_desc, uint32_t n, uint8_t *h_status, uint8_t *h_out,
                  uint32_t chunk, uint32_t flags, int encrypt) {
  if (!c || !h_arena || !h_desc || !h_status || (!encrypt && !h_out)) return ESPGPU_EINVAL;
  if (n == 0) return 0;
  if (!chunk) chunk = 65536;
  if (arena_bytes + 64 > c->e2e_bytes || n > c->e2e_n) {
    hipFree(c->e2e_arena); hipFree(c->e2e_out); hipFree(c->e2e_status); hipFree(c->e2e_desc);
    c->e2e_bytes = arena_bytes + 64;
    c->e2e_n = n;
    HIPCHK(c, hipMalloc(&c->e2e_arena, c->e2e_bytes));
    HIPCHK(c, hipMalloc(&c->e2e_out, c->e2e_bytes));
    HIPCHK(c, hipMalloc(&c->e2e_status, n));
    HIPCHK(c, hipMalloc(&c->e2e_desc, (size_t)n * sizeof(espgpu_desc)));
  }
  // Chunks of consecutive records (descriptors in ascending arena order) map to
  // contiguous byte ranges, copied to the same offsets of a device mirror so the
  // descriptors are used unchanged.
  for (uint32_t i0 = 0, k = 0; i0 < n; i0 += chunk, ++k) {
    const uint32_t i1 = std::min(n, i0 + chunk), m = i1 - i0;
    uint64_t lo = (uint64_t)h_desc[i0].off4 * 4, hi = 0;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint64_t o = (uint64_t)h_desc[i].off4 * 4;
      lo = std::min(lo, o);
      hi = std::max(hi, o + h_desc[i].len);
    }
#ifdef ESPGPU_BOUNDS
    espgpu_chk_arm(c, c->e2e_arena + lo, hi - lo, encrypt ? nullptr : c->e2e_out + lo, hi - lo, 16);
#endif
    hi = std::min(arena_bytes, hi + 16);                 // partial-block loads read <= 16 B past
    hipEvent_t ein = c->e2e_in[k & 1], ek = c->e2e_k[k & 1];
    HIPCHK(c, hipMemcpyAsync(c->e2e_desc + i0, h_desc + i0, m * sizeof(espgpu_desc), hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipMemcpyAsync(c->e2e_arena + lo, h_arena + lo, hi - lo, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipEventRecord(ein, c->s_in));
    HIPCHK(c, hipStreamWaitEvent(c->stream, ein, 0));
    int e = run_batch(c, c->e2e_arena, c->e2e_desc + i0, m, c->e2e_status + i0,
                      encrypt ? nullptr : c->e2e_out, flags, encrypt, c->stream);
    if (e) return e;
    HIPCHK(c, hipEventRecord(ek, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_out, ek, 0));
    uint8_t *dst = encrypt ? (uint8_t *)h_arena : h_out;
    HIPCHK(c, hipMemcpyAsync(dst + lo, (encrypt ? c->e2e_arena : c->e2e_out) + lo, hi - lo, hipMemcpyDeviceToHost, c->s_out));
    HIPCHK(c, hipMemcpyAsync(h_status + i0, c->e2e_status + i0, m, hipMemcpyDeviceToHost, c->s_out));
  }
  HIPCHK(c, hipStreamSynchronize(c->s_out));
  return 0;
}

}  // namespace
}  // namespace espgpu

using namespace espgpu;

extern "C" {

int espgpu_replay_params_ok(const espgpu_replay *r) { return r && replay_params_ok(*r); }

int espgpu_replay_check_batch(espgpu_ctx *c, const uint8_t *d_arena, espgpu_desc *d_desc, uint32_t n,
                              const espgpu_replay *d_replay, uint32_t nreplay, const uint32_t *d_bitmap,
                              uint8_t *d_rstatus, void *stream) {
  if (!c || (n && (!d_arena || !d_desc || !d_rstatus || (nreplay && (!d_replay || !d_bitmap)))))
    return ESPGPU_EINVAL;
  if (launch_replay_check(d_arena, d_desc, n, d_replay, nreplay, d_bitmap, d_rstatus, stream))
    return fail(c, ESPGPU_EIO, "replay check kernel launch failed");
  return 0;
}

int espgpu_replay_merge(espgpu_ctx *c, uint8_t *d_status, const uint8_t *d_rstatus, uint32_t n, void *stream) {
  if (!c || (n && (!d_status || !d_rstatus))) return ESPGPU_EINVAL;
  if (launch_replay_merge(d_status, d_rstatus, n, stream))
    return fail(c, ESPGPU_EIO, "replay merge kernel launch failed");
  return 0;
}

// The single-record window updates; the rules are replay.h's.
int espgpu_replay_update(espgpu_replay *r, uint32_t *bitmap, uint32_t seq) {
  if (!r || (r->wsize && !bitmap)) return ESPGPU_EINVAL;
  return r->wsize == 0 ? 0 : replay_update_rule(r, bitmap, seq);
}

int espgpu_replay_update64(espgpu_replay *r, uint32_t *bitmap, uint64_t seq64) {
  if (!r || (r->wsize && !bitmap)) return ESPGPU_EINVAL;
  return r->wsize == 0 ? 0 : replay_update64_rule(r, bitmap, seq64);
}

int espgpu_replay_update_batch(espgpu_ctx *c, const uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n,
                               const uint8_t *d_status, espgpu_replay *d_replay, uint32_t nreplay,
                               uint32_t *d_bitmap, uint8_t *d_ustatus, void *stream) {
  if (!c || (n && (!d_arena || !d_desc || !d_status || !d_ustatus || (nreplay && (!d_replay || !d_bitmap)))))
    return ESPGPU_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return run_stage(c, n, replay_update_workspace_bytes(std::max(n, 1024u), nreplay), st,
                   "replay update launch failed", [&] {
                     return launch_replay_update(d_arena, d_desc, n, d_status, d_replay, nreplay, d_bitmap,
                                                 d_ustatus, c->d_stage_ws, st);
                   });
}

// ---- outbound framing ----------------------------------------------------------
// The shape from session parameters, through the fields newsession keeps in
// DevSA (mode, calg, mlen: session_filed), so the host rule and the kernels
// read one table.
int espgpu_esp_frame_shape(const espgpu_session_params *csp, uint32_t flags, espgpu_eshape *shape) {
  if (!csp || !shape || probe_caps(csp) >= 0) return ESPGPU_EINVAL;
  uint32_t mode, mlen;
  session_filed(csp, &mode, &mlen);
  espgpu_eshape s;
  if (!esp_shape_of(mode, (uint32_t)csp->csp_cipher_alg, mlen, flags, &s)) return ESPGPU_EINVAL;
  *shape = s;
  return 0;
}

// esp_output's framing of one record.  The rule espgpu_esp_frame_batch
// applies (frame.h).
int espgpu_esp_frame(espgpu_outsa *o, const espgpu_eshape *s, uint8_t *rec, uint32_t len, uint32_t rlen,
                     uint8_t next_header, uint32_t *esn_hi) {
  if (!o || !s || !rec || !esn_hi) return ESPGPU_EINVAL;
  if ((s->ivlen != 0 && s->ivlen != 8 && s->ivlen != 16) || (s->blks != 4 && s->blks != 16)) return ESPGPU_EINVAL;
  return esp_frame_rule(o, *s, rec, len, rlen, next_header, esn_hi);
}

int espgpu_esp_frame_batch(espgpu_ctx *c, uint8_t *d_arena, espgpu_desc *d_desc, const uint32_t *d_frame,
                           uint32_t n, espgpu_outsa *d_out, uint32_t nout, uint8_t *d_fstatus, void *stream) {
  if (!c || (n && (!d_arena || !d_desc || !d_frame || !d_fstatus || (nout && !d_out)))) return ESPGPU_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return run_stage(c, n, esp_frame_workspace_bytes(std::max(n, 1024u), nout), st, "esp frame launch failed", [&] {
    return launch_esp_frame(d_arena, d_desc, d_frame, n, d_out, nout, c->d_sas, c->cfg.max_sessions, d_fstatus,
                            c->d_stage_ws, st);
  });
}

// ---- inbound classification ----------------------------------------------------
int espgpu_sad_build(const espgpu_sad_entry *sas, uint32_t nsas, espgpu_sad_entry *table, uint32_t nslots) {
  return sad_build(sas, nsas, table, nslots);
}

// ip_input's header sanity, ipsec_common_input's lookup and esp_input's first
// checks for one packet.  The rule espgpu_esp_classify_batch applies (classify.h).
int espgpu_esp_classify(const espgpu_sad_entry *table, uint32_t nslots, const uint8_t *pkt, uint32_t len,
                        uint32_t off4, uint32_t flags, espgpu_desc *desc) {
  if (!desc) return ESPGPU_EINVAL;
  if (!table || nslots == 0 || (nslots & (nslots - 1)) || (!pkt && len) || (flags & ~kClsKnown)) {
    *desc = espgpu_desc{off4, 0, 0xffff, 0, 0};
    return ESPGPU_EINVAL;
  }
  return esp_classify_rule(table, nslots, pkt, len, off4, flags, desc);
}

int espgpu_esp_classify_batch(espgpu_ctx *c, const uint8_t *d_arena, const espgpu_pkt *d_pkt, uint32_t n,
                              const espgpu_sad_entry *d_table, uint32_t nslots, uint32_t flags, espgpu_desc *d_desc,
                              uint8_t *d_cstatus, void *stream) {
  if (!c || (flags & ~kClsKnown)) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_pkt || !d_table || !d_desc || !d_cstatus || nslots == 0 || (nslots & (nslots - 1)) ||
            ((uintptr_t)d_arena & 3) || ((uintptr_t)d_table & 15)))
    return ESPGPU_EINVAL;
  // no workspace and nothing of the ctx's is touched
  return run_stage(c, n, 0, nullptr, "classify kernel launch failed", [&] {
    return launch_esp_classify(d_arena, d_pkt, n, d_table, nslots, flags, d_desc, d_cstatus, stream);
  });
}

// ---- inbound decapsulation ----------------------------------------------------
// esp_input_cb's tail and ipsec4/6_common_input_cb for one packet.  The rule
// espgpu_esp_decap_batch applies (decap.h).
int espgpu_esp_decap(espgpu_insa *in, const espgpu_eshape *s, uint8_t *pkt, uint32_t skip, uint32_t rlen,
                     uint32_t trailer, uint32_t *out_off, uint32_t *out_len) {
  if (out_off) *out_off = 0;
  if (out_len) *out_len = 0;
  if (!in || !s || !pkt || !out_off || !out_len) return ESPGPU_EINVAL;
  if ((s->ivlen != 0 && s->ivlen != 8 && s->ivlen != 16) || s->alen > 0xffffu) return ESPGPU_EINVAL;
  DecapPlan p;
  const int st = esp_decap_rule(in->flags, s->ivlen, s->alen, pkt, pkt, skip, rlen, trailer, &p);
  if (st) return st;
  *out_off = p.off;
  *out_len = p.len;
  in->bytes += p.len;                                            // key.c:8429-8445
  in->packets += 1;
  return 0;
}

int espgpu_esp_decap_batch(espgpu_ctx *c, const uint8_t *d_arena, uint8_t *d_out, const espgpu_pkt *d_pkt,
                           const espgpu_desc *d_desc, const uint32_t *d_trailer, const uint8_t *d_status, uint32_t n,
                           espgpu_insa *d_in, uint32_t nin, espgpu_pkt *d_ipkt, uint8_t *d_dstatus, void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_out || !d_pkt || !d_desc || !d_trailer || !d_status || !d_ipkt || !d_dstatus ||
            (nin && !d_in) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_out & 3)))
    return ESPGPU_EINVAL;
  // no workspace; of the ctx only the session table is read, as the crypto
  // kernels read it
  return run_stage(c, n, 0, nullptr, "decap kernel launch failed", [&] {
    return launch_esp_decap(d_arena, d_out, d_pkt, d_desc, d_trailer, d_status, n, d_in, nin, c->d_sas,
                            c->cfg.max_sessions, d_ipkt, d_dstatus, stream);
  });
}

// ---- inbound AH -----------------------------------------------------------------
// ah_input's checks and ah_massage_headers for one packet, and ah_input_cb's
// tail with ipsec4/6_common_input_cb.  The rules espgpu_ah_input_batch and
// espgpu_ah_decap_batch apply (ah_in.h).

int espgpu_ah_input(const espgpu_insa *in, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t salt,
                    uint8_t *hsave) {
  if (!in || !pkt || !hsave || !ah_mlen_usable(mlen)) return ESPGPU_EINVAL;
  return ah_input_rule(in->flags, mlen, pkt, len, salt, hsave);
}

int espgpu_ah_input_batch(espgpu_ctx *c, uint8_t *d_arena, espgpu_desc *d_desc, uint32_t n, const espgpu_insa *d_in,
                          uint32_t nin, uint8_t *d_hsave, uint8_t *d_astatus, void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_desc || !d_hsave || !d_astatus || (nin && !d_in) || ((uintptr_t)d_arena & 3) ||
            ((uintptr_t)d_hsave & 3)))
    return ESPGPU_EINVAL;
  // no workspace; of the ctx only the session table is read
  return run_stage(c, n, 0, nullptr, "AH input kernel launch failed", [&] {
    return launch_ah_input(d_arena, d_desc, n, d_in, nin, c->d_sas, c->cfg.max_sessions, d_hsave, d_astatus, stream);
  });
}

int espgpu_ah_decap(espgpu_insa *in, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t salt, const uint8_t *hsave,
                    uint32_t *out_off, uint32_t *out_len) {
  if (out_off) *out_off = 0;
  if (out_len) *out_len = 0;
  if (!in || !pkt || !hsave || !out_off || !out_len || !ah_mlen_usable(mlen)) return ESPGPU_EINVAL;
  DecapPlan p;
  const int st = ah_decap_rule(in->flags, mlen, pkt, len, salt, hsave, &p);
  if (st) return st;
  *out_off = p.off;
  *out_len = p.len;
  in->bytes += p.len;                                            // key.c:8429-8445
  in->packets += 1;
  return 0;
}

int espgpu_ah_decap_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, const uint8_t *d_status,
                          uint32_t n, espgpu_insa *d_in, uint32_t nin, const uint8_t *d_hsave, espgpu_pkt *d_ipkt,
                          uint8_t *d_dstatus, void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_desc || !d_status || !d_hsave || !d_ipkt || !d_dstatus || (nin && !d_in) ||
            ((uintptr_t)d_arena & 3) || ((uintptr_t)d_hsave & 3)))
    return ESPGPU_EINVAL;
  return run_stage(c, n, 0, nullptr, "AH decap kernel launch failed", [&] {
    return launch_ah_decap(d_arena, d_desc, d_status, n, d_in, nin, c->d_sas, c->cfg.max_sessions, d_hsave, d_ipkt,
                           d_dstatus, stream);
  });
}

// ---- the NAT-T checksum fix (step 5b) -----------------------------------------
// udp_ipsec_adjust_cksum for one decapsulated packet.  The rule
// espgpu_esp_natt_cksum_batch applies (natt.h).
int espgpu_esp_natt_cksum(const espgpu_insa *in, uint8_t *pkt, uint32_t len, uint32_t trailer, uint32_t policy,
                          uint8_t *out_cflags) {
  if (out_cflags) *out_cflags = 0;
  if (!in || !pkt) return ESPGPU_EINVAL;
  if (!(in->flags & ESPGPU_IN_NATT)) return 0;
  const uint32_t cf = natt_cksum_rule(pkt, len, trailer & 0xffu, policy, in->natt_cksum);
  if (out_cflags) *out_cflags = (uint8_t)cf;
  return 0;
}

int espgpu_esp_natt_cksum_batch(espgpu_ctx *c, uint8_t *d_out, const espgpu_pkt *d_ipkt, const espgpu_desc *d_desc,
                                const uint32_t *d_trailer, const uint8_t *d_status, const uint8_t *d_dstatus,
                                uint32_t n, const espgpu_insa *d_in, uint32_t nin, uint32_t policy, uint8_t *d_cflags,
                                void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_out || !d_ipkt || !d_desc || !d_trailer || !d_status || !d_dstatus || (nin && !d_in) ||
            ((uintptr_t)d_out & 3)))
    return ESPGPU_EINVAL;
  // no workspace and nothing of the ctx's is touched
  return run_stage(c, n, 0, nullptr, "NAT-T checksum kernel launch failed", [&] {
    return launch_esp_natt_cksum(d_out, d_ipkt, d_desc, d_trailer, d_status, d_dstatus, n, d_in, nin, policy,
                                 c->natt_lanes, d_cflags, stream);
  });
}

// ---- outbound encapsulation ---------------------------------------------------
// ipsec4/6_perform_request, ipsec_encap and the header work of esp_output and
// ipsec_process_done for one packet.  The rule espgpu_esp_encap_batch applies
// (encap.h).
int espgpu_esp_encap(const espgpu_encsa *e, const espgpu_eshape *s, uint8_t *pkt, uint32_t len, uint32_t headroom,
                     uint32_t tailroom, uint16_t ip_id, uint32_t *out_front, uint32_t *out_total,
                     uint32_t *out_reclen, uint32_t *out_frame) {
  for (uint32_t *r : {out_front, out_total, out_reclen, out_frame})
    if (r) *r = 0;
  if (!e || !s || !pkt || !out_front || !out_total || !out_reclen || !out_frame) return ESPGPU_EINVAL;
  if ((s->ivlen != 0 && s->ivlen != 8 && s->ivlen != 16) || (s->blks != 4 && s->blks != 16) || s->alen > 0xffffu)
    return ESPGPU_EINVAL;
  EncapOut o;
  const int st = esp_encap_rule(e, *s, pkt, len, headroom, tailroom, ip_id, &o);
  if (st) return st;
  *out_front = o.front;
  *out_total = o.total;
  *out_reclen = o.reclen;
  *out_frame = o.frame;
  return 0;
}

int espgpu_esp_sent(espgpu_encsa *e, uint8_t status, uint32_t len) {
  if (!e) return ESPGPU_EINVAL;
  if (status == 0) {
    // a NAT-T SA: key_sa_recordxfer runs before the UDP header exists (ipsec_output.c:770, :808)
    if ((e->flags & ESPGPU_ENC_NATT) && len >= 8) len -= 8;
    e->bytes += len;                                               // key.c:8429-8445
    e->packets += 1;
  }
  return 0;
}

int espgpu_esp_encap_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_pkt *d_pkt, const uint16_t *d_sa, uint32_t n,
                           const espgpu_encsa *d_enc, const espgpu_outsa *d_out, uint32_t nenc, uint32_t headroom,
                           uint32_t tailroom, uint32_t id0, espgpu_desc *d_desc, uint32_t *d_frame,
                           espgpu_pkt *d_opkt, uint8_t *d_estatus, void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_pkt || !d_sa || !d_desc || !d_frame || !d_opkt || !d_estatus ||
            (nenc && (!d_enc || !d_out)) || ((uintptr_t)d_arena & 3)))
    return ESPGPU_EINVAL;
  // no workspace; of the ctx only the session table is read, as the crypto
  // kernels read it
  return run_stage(c, n, 0, nullptr, "encap kernel launch failed", [&] {
    return launch_esp_encap(d_arena, d_pkt, d_sa, n, d_enc, d_out, nenc, c->d_sas, c->cfg.max_sessions, headroom,
                            tailroom, id0, d_desc, d_frame, d_opkt, d_estatus, stream);
  });
}

int espgpu_esp_sent_batch(espgpu_ctx *c, const espgpu_pkt *d_opkt, const espgpu_desc *d_desc, const uint8_t *d_status,
                          uint32_t n, espgpu_encsa *d_enc, uint32_t nenc, void *stream) {
  if (!c || (n && (!d_opkt || !d_desc || !d_status || (nenc && !d_enc)))) return ESPGPU_EINVAL;
  return run_stage(c, n, 0, nullptr, "sent kernel launch failed", [&] {
    return launch_esp_sent(d_opkt, d_desc, d_status, n, d_enc, nenc, stream);
  });
}

// ---- outbound AH ----------------------------------------------------------------
// The transport-or-tunnel decision, ipsec_encap and ah_output's header work
// with ah_massage_headers (out = 1) for one packet, ah_output's sequence number
// and ah_output_cb's restore with key_sa_recordxfer.  The rules
// espgpu_ah_encap_batch, espgpu_ah_frame_batch and espgpu_ah_sent_batch apply
// (ah_out.h).
int espgpu_ah_encap(const espgpu_encsa *e, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t headroom,
                    uint16_t ip_id, uint8_t *hsave, uint32_t *out_front, uint32_t *out_total, uint32_t *out_salt) {
  for (uint32_t *r : {out_front, out_total, out_salt})
    if (r) *r = 0;
  if (!e || !pkt || !hsave || !out_front || !out_total || !out_salt) return ESPGPU_EINVAL;
  AhOutPlan p;
  const int st = ah_encap_rule(e, mlen, pkt, len, headroom, ip_id, hsave, &p);
  if (st) return st;
  *out_front = p.ahsize + p.oh;
  *out_total = p.total;
  *out_salt = (p.tunnel ? p.oh : p.skip) + 12;
  return 0;
}

int espgpu_ah_frame(espgpu_outsa *o, uint8_t *pkt, uint32_t len, uint32_t salt, uint32_t *esn_hi) {
  if (!o || !pkt || !esn_hi) return ESPGPU_EINVAL;
  return ah_frame_rule(o, pkt, len, salt, esn_hi);
}

int espgpu_ah_sent(espgpu_encsa *e, uint8_t status, uint8_t *pkt, uint32_t len, uint32_t salt,
                   const uint8_t *hsave) {
  if (!e || !pkt || !hsave) return ESPGPU_EINVAL;
  if (status != 0 || !(e->flags & ESPGPU_ENC_AH)) return 0;
  const int st = ah_sent_rule(e->flags, pkt, len, salt, hsave);
  if (st) return st;
  e->bytes += len;                                               // key.c:8429-8445
  e->packets += 1;
  return 0;
}

int espgpu_ah_encap_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_pkt *d_pkt, const uint16_t *d_sa, uint32_t n,
                          const espgpu_encsa *d_enc, uint32_t nenc, uint32_t headroom, uint32_t id0,
                          uint8_t *d_hsave, espgpu_desc *d_desc, espgpu_pkt *d_opkt, uint8_t *d_estatus,
                          void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_pkt || !d_sa || !d_hsave || !d_desc || !d_opkt || !d_estatus || (nenc && !d_enc) ||
            ((uintptr_t)d_arena & 3) || ((uintptr_t)d_hsave & 3)))
    return ESPGPU_EINVAL;
  // no workspace; of the ctx only the session table is read
  return run_stage(c, n, 0, nullptr, "AH encap kernel launch failed", [&] {
    return launch_ah_encap(d_arena, d_pkt, d_sa, n, d_enc, nenc, c->d_sas, c->cfg.max_sessions, headroom, id0,
                           d_hsave, d_desc, d_opkt, d_estatus, stream);
  });
}

int espgpu_ah_frame_batch(espgpu_ctx *c, uint8_t *d_arena, espgpu_desc *d_desc, uint32_t n, espgpu_outsa *d_out,
                          uint32_t nout, uint8_t *d_fstatus, void *stream) {
  if (!c || (n && (!d_arena || !d_desc || !d_fstatus || (nout && !d_out) || ((uintptr_t)d_arena & 3))))
    return ESPGPU_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return run_stage(c, n, ah_frame_workspace_bytes(std::max(n, 1024u), nout), st, "AH frame launch failed", [&] {
    return launch_ah_frame(d_arena, d_desc, n, d_out, nout, c->d_sas, c->cfg.max_sessions, d_fstatus, c->d_stage_ws,
                           st);
  });
}

int espgpu_ah_sent_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_pkt *d_opkt, const espgpu_desc *d_desc,
                         const uint8_t *d_status, uint32_t n, espgpu_encsa *d_enc, uint32_t nenc,
                         const uint8_t *d_hsave, uint8_t *d_sstatus, void *stream) {
  if (!c) return ESPGPU_EINVAL;
  if (n && (!d_arena || !d_opkt || !d_desc || !d_status || !d_hsave || !d_sstatus || (nenc && !d_enc) ||
            ((uintptr_t)d_arena & 3) || ((uintptr_t)d_hsave & 3)))
    return ESPGPU_EINVAL;
  return run_stage(c, n, 0, nullptr, "AH sent kernel launch failed", [&] {
    return launch_ah_sent(d_arena, d_opkt, d_desc, d_status, n, d_enc, nenc, c->d_sas, c->cfg.max_sessions, d_hsave,
                          d_sstatus, stream);
  });
}

int espgpu_decrypt_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n,
                         uint8_t *d_status, uint8_t *d_out, uint32_t flags, void *stream) {
  if (!c || (!d_arena && n) || (!d_desc && n) || (!d_status && n)) return ESPGPU_EINVAL;
  return batch_rc(c, run_batch(c, d_arena, d_desc, n, d_status, d_out ? d_out : d_arena, flags, 0,
                             reinterpret_cast<hipStream_t>(stream)));
}

int espgpu_decrypt_batch_trailer(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc,
                                 uint32_t n, uint8_t *d_status, uint8_t *d_out, uint32_t *d_trailer,
                                 uint32_t flags, void *stream) {
  if (!c || (!d_arena && n) || (!d_desc && n) || (!d_status && n) || (!d_trailer && n)) return ESPGPU_EINVAL;
  return batch_rc(c, run_batch(c, d_arena, d_desc, n, d_status, d_out ? d_out : d_arena, flags, 0,
                             reinterpret_cast<hipStream_t>(stream), d_trailer));
}

int espgpu_decrypt_batch_packed(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n,
                                uint8_t *d_status, uint8_t *d_out, uint32_t out_stride, uint32_t flags,
                                void *stream) {
  if (!c || (!d_arena && n) || (!d_desc && n) || (!d_status && n) || (!d_out && n) || d_out == d_arena ||
      out_stride == 0 || out_stride % 128 != 0 || ((uintptr_t)d_out & 127))
    return ESPGPU_EINVAL;
  return batch_rc(c, run_batch(c, d_arena, d_desc, n, d_status, d_out, flags, 0, reinterpret_cast<hipStream_t>(stream),
                             nullptr, 3, nullptr, out_stride));
}

int espgpu_encrypt_batch(espgpu_ctx *c, uint8_t *d_arena, const espgpu_desc *d_desc, uint32_t n,
                         uint8_t *d_status, uint32_t flags, void *stream) {
  if (!c || (!d_arena && n) || (!d_desc && n) || (!d_status && n)) return ESPGPU_EINVAL;
  return batch_rc(c, run_batch(c, d_arena, d_desc, n, d_status, nullptr, flags, 1, reinterpret_cast<hipStream_t>(stream)));
}

float espgpu_last_kernel_ms(espgpu_ctx *c) { return c ? c->last_ms : 0.f; }

int espgpu_decrypt_host(espgpu_ctx *c, const uint8_t *h_arena, uint64_t arena_bytes,
                        const espgpu_desc *h_desc, uint32_t n, uint8_t *h_status, uint8_t *h_out,
                        uint32_t chunk, uint32_t flags) {
  if (c && c->failed) return ESPGPU_EIO;
  if (c && c->n_dig > 0)
    return fail(c, ESPGPU_ENOTSUP, "the host pipeline does not serve contexts with DIGEST sessions");
  return batch_rc(c, host_pipeline(c, h_arena, arena_bytes, h_desc, n, h_status, h_out, chunk, flags, 0));
}

#ifdef ESPGPU_BOUNDS
// ---- the bounds-checked build (espgpu_internal.h, bounds_chk.h) ----------------
__attribute__((visibility("default"))) int espgpu_chk_arm(espgpu_ctx *c, const void *arena_base,
                                                          uint64_t arena_bytes, const void *out_base,
                                                          uint64_t out_bytes, uint32_t pad) {
  if (!c || !arena_base) return ESPGPU_EINVAL;
  c->chk.lo[0] = (uint64_t)(uintptr_t)arena_base;
  c->chk.hi[0] = c->chk.lo[0] + arena_bytes;
  c->chk.lo[1] = out_base ? (uint64_t)(uintptr_t)out_base : c->chk.lo[0];
  c->chk.hi[1] = out_base ? c->chk.lo[1] + out_bytes : c->chk.hi[0];
  c->chk.pad = pad;
  c->chk_armed = true;
  return 0;
}

__attribute__((visibility("default"))) int espgpu_chk_report(espgpu_ctx *c, void *buf, uint32_t cap) {
  if (!c || !buf) return -ESPGPU_EINVAL;
  if (!c->chk.rep && chk_report_reset(c)) return -ESPGPU_EIO;
  if (hipDeviceSynchronize() != hipSuccess) return -ESPGPU_EIO;
  const uint32_t nb = std::min<uint32_t>(cap, (uint32_t)sizeof(ChkReport));
  if (hipMemcpy(buf, c->chk.rep, nb, hipMemcpyDeviceToHost) != hipSuccess) return -ESPGPU_EIO;
  return (int)nb;
}

__attribute__((visibility("default"))) int espgpu_chk_reset(espgpu_ctx *c) {
  return c ? chk_report_reset(c) : ESPGPU_EINVAL;
}
#endif

}  // extern "C"
