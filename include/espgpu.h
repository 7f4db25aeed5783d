/*
 * espgpu.h — C ABI of the MI355X-native ESP bulk-crypto engine (libespgpu.so).
 *
 * Drop-in boundary: this library plays the part of an opencrypto *driver*
 * (freebsd/opencrypto/cryptodev_if.m) beneath the unchanged opencrypto
 * framework, i.e. it replaces the software driver "cryptosoft"
 * (freebsd/opencrypto/cryptosoft.c) for the ESP ciphers F-Stack's IPsec uses:
 *   AES-GCM-16 (CSP_MODE_AEAD)                  -> swcr_gcm      cryptosoft.c:465-645
 *   AES-CBC, AES-CTR (RFC 3686) or NULL + HMAC-SHA1-96
 *     or HMAC-SHA2-256-128 / -384-192 / -512-256
 *     (CSP_MODE_ETA)                            -> swcr_eta      cryptosoft.c:874-888
 *                                                  (NULL: swcr_authcompute, :1394-1398)
 *   AES-CBC or AES-CTR with no auth, or NULL
 *     (CSP_MODE_CIPHER)                         -> swcr_encdec   cryptosoft.c:101-284
 *                                                  (NULL: swcr_null, :91-95)
 * and for AH (netipsec/xform_ah.c):
 *   HMAC-SHA1 or HMAC-SHA2-256 / -384 / -512 over the whole packet
 *     (CSP_MODE_DIGEST)                         -> swcr_authcompute cryptosoft.c:317-382
 * Every entry point is plain C: integers, pointers, sizes.  No exceptions,
 * no C++ or torch types cross it.  Errors are errno values, as in opencrypto.
 * One espgpu_ctx per lcore thread (thread-compatible, not thread-safe), the
 * way F-Stack runs one FreeBSD stack per lcore (lib/ff_dpdk_if.c:2235).
 *
 * Two ways in:
 *  (1) the opencrypto driver path (host buffers): probesession / newsession /
 *      freesession / process / flush / poll  — what a kernel-domain driver shim
 *      in F-Stack binds;
 *  (2) the device-resident batch path: records already in HBM, a 16-byte
 *      descriptor per record — what bench.py times and what a GPU-direct RX
 *      path would call.
 */
#ifndef ESPGPU_H
#define ESPGPU_H

#if defined(_KERNEL) && defined(__FreeBSD__)
/* F-Stack's kernel domain (lib/Makefile: -nostdinc, FreeBSD headers only):
 * the driver ff_gpucrypto.c includes this header for the request mirrors */
#include <sys/types.h>
#else
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ESPGPU_ABI_VERSION 6
#define ESPGPU_HAS_NATT 1   /* the NAT-T block below is built; the ABI version stays: new symbols and
                             flag bits that were refused before, no layout change */
#define ESPGPU_HAS_AH_BATCH 1   /* the inbound AH block below is built (ESPGPU_CLS_AH, ESPGPU_REPLAY_AH,
                                 espgpu_ah_input, espgpu_ah_decap); the ABI version stays, as above */
#define ESPGPU_HAS_AH_OUT 1     /* the outbound AH block below is built (ESPGPU_ENC_AH, espgpu_ah_encap,
                                 espgpu_ah_frame, espgpu_ah_sent); the ABI version stays, as above */

/* ---- constants, numerically identical to freebsd/opencrypto/cryptodev.h ---- */
#define ESPGPU_CSP_MODE_CIPHER      2        /* cryptodev.h:362: ESP without auth */
#define ESPGPU_CSP_MODE_DIGEST      3        /* cryptodev.h:363: AH (xform_ah.c ah_init) */
#define ESPGPU_CSP_MODE_AEAD        4        /* cryptodev.h:364 */
#define ESPGPU_CSP_MODE_ETA         5        /* cryptodev.h:365 */
#define ESPGPU_CSP_F_SEPARATE_AAD   0x0002   /* cryptodev.h:370 */
#define ESPGPU_CSP_F_ESN            0x0004   /* cryptodev.h:371 */
#define ESPGPU_CRYPTO_SHA1_HMAC     7        /* cryptodev.h:150 */
#define ESPGPU_CRYPTO_AES_CBC       11       /* cryptodev.h:155 */
#define ESPGPU_CRYPTO_NULL_CBC      16       /* cryptodev.h:160: ESP-NULL (enc_xform_null) */
#define ESPGPU_CRYPTO_SHA2_256_HMAC 18     /* cryptodev.h:162 */
#define ESPGPU_CRYPTO_SHA2_384_HMAC 19     /* cryptodev.h:163 */
#define ESPGPU_CRYPTO_SHA2_512_HMAC 20     /* cryptodev.h:164 */
#define ESPGPU_CRYPTO_AES_ICM       23       /* AES-CTR, cryptodev.h:167 */
#define ESPGPU_CRYPTO_AES_NIST_GCM_16 25     /* cryptodev.h:169 */
#define ESPGPU_CRYPTO_OP_DECRYPT    0x0      /* cryptodev.h:598 */
#define ESPGPU_CRYPTO_OP_ENCRYPT    0x1
#define ESPGPU_CRYPTO_OP_VERIFY_DIGEST 0x2
#define ESPGPU_CRYPTO_OP_COMPUTE_DIGEST 0x0  /* cryptodev.h:603 */
#define ESPGPU_CRYPTO_F_IV_SEPARATE 0x0200   /* cryptodev.h:470 */
#define ESPGPU_CRYPTO_HINT_MORE     0x1      /* cryptodev.h:612 */
#define ESPGPU_PROBE_HARDWARE       (-100)   /* CRYPTODEV_PROBE_HARDWARE, cryptodev.h:345 */

/*
 * Error codes returned by every entry point and written as the per-record
 * status byte.  They are this ABI's own numbers (they coincide with Linux
 * errno, the host the library runs on), NOT FreeBSD kernel errno: a
 * kernel-domain shim translates them before they reach opencrypto, e.g.
 * ESPGPU_EBADMSG -> EBADMSG (89), ESPGPU_ERESTART -> ERESTART (-1),
 * ESPGPU_EAGAIN -> EAGAIN (35); see integration/ff_gpucrypto.c
 * gpucrypto_errno().
 */
#define ESPGPU_OK       0
#define ESPGPU_ENOENT   2     /* unknown tuning key                            */
#define ESPGPU_EIO      5     /* HIP runtime failure (espgpu_last_error says)  */
#define ESPGPU_ENXIO    6
#define ESPGPU_EAGAIN   11
#define ESPGPU_ENOMEM   12    /* SA table full / allocation failure            */
#define ESPGPU_ENODEV   19    /* no HIP device                                 */
#define ESPGPU_EINVAL   22    /* malformed request or unsupported parameters   */
#define ESPGPU_EBADMSG  74    /* ICV mismatch (status byte / crp_etype)        */
#define ESPGPU_ERESTART 85    /* process(): staging full, requeue (cc_qblocked) */
#define ESPGPU_ENOTSUP  95
#define ESPGPU_ENOBUFS  105   /* F-Stack mode: host overflow full, request dropped */

/* Mirror of struct crypto_session_params (cryptodev.h:357-384). */
struct espgpu_session_params {
	int         csp_mode;
	int         csp_flags;
	int         csp_ivlen;
	int         csp_cipher_alg;
	int         csp_cipher_klen;
	const void *csp_cipher_key;
	int         csp_auth_alg;
	int         csp_auth_klen;
	const void *csp_auth_key;
	int         csp_auth_mlen;
};

/* One buffer segment (an mbuf in the chain, or the whole contiguous buffer). */
struct espgpu_seg {
	void    *base;
	uint32_t len;
};

/*
 * Mirror of the struct cryptop fields a driver consumes (cryptodev.h:427-504).
 * The buffer is crp_buf (CRYPTO_BUF_CONTIG = 1 segment, CRYPTO_BUF_MBUF = the
 * chain as segments), processed in place.  `opaque` comes back in the
 * completion (a kernel-domain shim passes the cryptop pointer itself).
 */
struct espgpu_req {
	int32_t                  session;
	int                      crp_op;
	int                      crp_flags;
	const struct espgpu_seg *segs;
	int                      nsegs;
	const void              *crp_aad;          /* separate AAD or NULL */
	int                      crp_aad_start;
	int                      crp_aad_length;
	uint8_t                  crp_esn[4];
	int                      crp_iv_start;
	int                      crp_payload_start;
	int                      crp_payload_length;
	int                      crp_digest_start;
	uint8_t                  crp_iv[16];
	void                    *opaque;
};

struct espgpu_completion {
	void *opaque;
	int   etype;            /* crp_etype: 0, EBADMSG, EINVAL, EIO (GPU failure) */
};

/* Device-resident descriptor: one per ESP record (16 bytes). */
struct espgpu_desc {
	uint32_t off4;          /* record start in the arena, in 4-byte units       */
	uint16_t len;           /* ESP record length: SPI|SN|IV|payload|ICV          */
	uint16_t sa;            /* session slot (espgpu_newsession's id)             */
	uint32_t esn_hi;        /* high 32 bits of the ESN (SAs with CSP_F_ESN/SEP)  */
	uint32_t salt;          /* GCM salt / AES-CTR nonce = crp_iv[0..3], in memory order;
	                           DIGEST (AH) SAs: the byte offset of the ICV field inside
	                           the record, a multiple of 4 with salt + mlen <= len */
};

struct espgpu_config {
	int      device;          /* HIP device ordinal                               */
	uint32_t max_sessions;    /* SA table capacity (default 1024)                 */
	uint32_t batch_records;   /* records per host batch (default 65536)           */
	uint32_t batch_bytes;     /* staging bytes per host batch (default 64 MiB)    */
	uint32_t nbatches;        /* staging slots in flight (default 2)              */
	uint32_t grid;            /* workgroups for the crypto kernels (0 = auto)     */
};

struct espgpu_stats {
	uint64_t records, bytes, auth_fail, einval;
	uint64_t batches, kernel_ns;   /* kernel_ns: device time measured with events */
	uint64_t erestart;
	uint64_t overflow;             /* requests staged through the host overflow      */
	uint64_t zerocopy;             /* records moved from / to registered memory      */
	uint64_t door;                 /* batches served by the doorbell kernel (ABI 3)  */
	uint64_t ovf_reserved;         /* host bytes the overflow's fixed rings hold (ABI 4):
	                                  set once by set_tuning "overflow_mb", never grown */
	uint64_t ovf_peak;             /* most record bytes the overflow held at once    */
	uint64_t ovf_process_ns_max;   /* longest overflow placement inside process()    */
	uint64_t gpu_fail;             /* GPU failures detected (ABI 5): 0, or 1 once failed */
	uint64_t fail_eio;             /* requests completed or refused with EIO because of it */
};

typedef struct espgpu_ctx espgpu_ctx;

/* ---- lifecycle (a kernel-domain shim calls crypto_get_driverid(...,
 *      CRYPTOCAP_F_HARDWARE|CRYPTOCAP_F_SYNC), crypto.c:989, around these) ---- */
int  espgpu_abi_version(void);
/* Visible HIP devices (>= 0), or ESPGPU_ENODEV.  One F-Stack process (lcore)
 * opens one context; process k of a node takes device k mod count
 * (ff_gpucrypto_host_init_proc). */
int  espgpu_device_count(void);
int  espgpu_init(const struct espgpu_config *cfg, espgpu_ctx **out);
void espgpu_fini(espgpu_ctx *ctx);
const char *espgpu_last_error(espgpu_ctx *ctx);
/* GPU health: ESPGPU_OK, or ESPGPU_EIO once the context has seen a GPU
 * failure -- a launch or copy that could not be queued, a completion query
 * that returned an error, or a batch outstanding longer than set_tuning
 * "deadline_ms" (default 2000).  From then on the context launches nothing:
 * every request it held completes exactly once through espgpu_poll with
 * etype ESPGPU_EIO (unless its batch is seen to complete after all),
 * espgpu_process / flush / drain / newsession and the batch entry points
 * answer ESPGPU_EIO, and espgpu_last_error names the cause.  The F-Stack
 * shim's probe declines on a failed context, so new sessions go to
 * cryptosoft. */
int  espgpu_health(espgpu_ctx *ctx);

/* ---- opencrypto driver methods (cryptodev_if.m) ---- */
/* CRYPTODEV_PROBESESSION (cryptodev_if.m:72-75): ESPGPU_PROBE_HARDWARE or EINVAL.
 * Host-only; no device needed.  The driver's bid: every session kind the
 * engine serves, except that AH (CSP_MODE_DIGEST) sessions are bid for only
 * when offered -- set_tuning "ah_offer" 1, or FF_GPUCRYPTO_AH=1 in the
 * environment -- so that a binary linked before the engine knew the mode
 * keeps AH on cryptosoft.  espgpu_newsession serves them either way. */
int  espgpu_probesession(const struct espgpu_session_params *csp);
/* CRYPTODEV_NEWSESSION (cryptodev_if.m:93-97): expands keys (AES schedule,
 * GHASH power tables, HMAC ipad/opad states) into the device SA table. */
int  espgpu_newsession(espgpu_ctx *ctx, const struct espgpu_session_params *csp,
                       int32_t *session_out);
/* CRYPTODEV_FREESESSION (cryptodev_if.m:113-116) */
void espgpu_freesession(espgpu_ctx *ctx, int32_t session);
/* Free SA-table slots (ABI 6; >= 0, or ESPGPU_EINVAL without a context):
 * at 0 espgpu_newsession answers ESPGPU_ENOMEM.  The F-Stack shim's probe
 * declines then, so crypto_newsession selects cryptosoft instead of failing
 * the SA in CRYPTODEV_NEWSESSION (crypto.c:954-958). */
int  espgpu_session_room(espgpu_ctx *ctx);
/* CRYPTODEV_PROCESS (cryptodev_if.m:143-147): never blocks.  On a failed
 * context (espgpu_health) it answers ESPGPU_EIO at once: never ERESTART or
 * EAGAIN, which would hand the request back to this dead engine.  Stages the
 * request; returns 0, or ERESTART when every staging slot is in flight (the
 * framework then sets cc_qblocked and requeues, crypto.c:1451-1459).  With
 * set_tuning "overflow_mb" > 0 such a request is kept in a host overflow
 * instead (ERESTART only once that many MiB are held), which the next
 * espgpu_flush moves into the slots as they free: F-Stack runs no
 * crypto_proc thread to requeue.  A record lying
 * in one segment of memory registered with espgpu_register_host is not
 * copied by the CPU: the GPU reads it and writes the results back in place.
 * Malformed requests complete with crp_etype = EINVAL via poll(), as
 * crypto_done would.  A DIGEST (AH) session's request is swcr_authcompute's:
 * the message is [crp_payload_start, +crp_payload_length) as it stands (1 ..
 * 65535 bytes, any byte length, no AAD), then crp_esn for ESN sessions; the
 * digest field [crp_digest_start, +mlen) lies inside it at a multiple of 4
 * from crp_payload_start.  COMPUTE_DIGEST writes those mlen bytes and nothing
 * else; VERIFY_DIGEST writes nothing and completes with 0 or EBADMSG.  `hint` (CRYPTO_HINT_MORE) is accepted and ignored:
 * staged requests launch at espgpu_flush (once per RX burst) or when a
 * staging slot fills. */
int  espgpu_process(espgpu_ctx *ctx, const struct espgpu_req *req, int hint);
/* Launch everything staged so far, then move the overflow into the slots
 * that are free: a small batch runs copy, kernels, copy in order on its
 * slot's stream; a large one H2D, kernels and D2H on three ctx streams
 * chained by events, so consecutive batches overlap copies with kernels.
 * Never waits.  F-Stack's main_loop calls this once per RX burst
 * (lib/ff_dpdk_if.c:2363). */
int  espgpu_flush(espgpu_ctx *ctx);
/* Complete finished requests: copies results back into the caller's segments
 * (only for etype 0: EBADMSG leaves the buffer unchanged) and returns up to
 * `max` completions; the shim calls crypto_done() for each. */
int  espgpu_poll(espgpu_ctx *ctx, struct espgpu_completion *out, int max);
/* Block until everything staged, flushed or in the overflow has completed
 * (teardown / tests); the completions wait for espgpu_poll. */
int  espgpu_drain(espgpu_ctx *ctx);
/* Register host memory the requests' buffers live in (DPDK mbuf pools:
 * F-Stack's mbuf data is the mbuf's own hugepage buffer, lib/ff_veth.c:
 * 367-389; ff_dpdk_register_gpu_mem walks the pools with
 * rte_mempool_mem_iter).  hipHostRegister maps it
 * for the device once; process() then stages a record that lies in it by
 * reference, and the xfer kernel reads it into the device batch and writes
 * the results back (payload; ICV when encrypting; nothing for a record that
 * fails) with no CPU copy.  Memory already pinned (hipHostMalloc) is mapped
 * as is.  Regions must not overlap: EINVAL.  Unregister drains first. */
int  espgpu_register_host(espgpu_ctx *ctx, void *base, uint64_t len);
int  espgpu_unregister_host(espgpu_ctx *ctx, void *base);
int  espgpu_get_stats(espgpu_ctx *ctx, struct espgpu_stats *st);

/* ---- device-resident batch path ----
 * d_arena: device buffer holding the records (padded by >= 16 bytes at its
 * end); d_desc[n]; d_status[n] receives one errno byte per record.
 * The arena (and d_out) may be up to 16 GiB: off4 counts 4-byte units and its
 * whole 32-bit range is valid, here and in espgpu_pkt; every kernel and every
 * batch stage forms a record's address as d_arena + (size_t)off4 * 4.
 * decrypt: plaintext goes to d_out at the same offsets (d_out may equal
 * d_arena: verify-first in place; an EBADMSG record ends byte-identical to
 * its ciphertext: AES-GCM in one pass that XORs the keystream back over a
 * failed record, CBC/CTR + HMAC verifying before it decrypts).
 * encrypt: payload encrypted in place, ICV written.
 * DIGEST (AH) SAs: one record is one packet, len = the hashed bytes (any
 * value 1..65535, off4 the packet start), salt = the byte offset of the ICV
 * field inside it (a multiple of 4, salt + mlen <= len; else EINVAL).  In
 * both directions the ICV field reads as zeros while the packet is hashed
 * (ah_input's save-and-zero, ah_output's zeroing); the mutable IP header
 * fields are the caller's business (ah_massage_headers; inbound,
 * espgpu_ah_input_batch does it on the device: the inbound AH block below).  encrypt: the ICV is
 * written at salt, status 0, nothing else moves.  decrypt (and _trailer): the
 * stored ICV is compared (ah_input_cb), status 0 or EBADMSG, and nothing is
 * written to d_arena or d_out, in place or out of place; the trailer word is
 * ESPGPU_TR_VALID alone, or 0.  A batch may mix GCM, ETA and DIGEST SAs.
 * `flags`: ESPGPU_BATCH_GROUPED if d_desc is already grouped by session with
 * at most one session per aligned run of 256 records (skips the device
 * planner; records of another session than their run's come back EINVAL).
 * `stream` is a hipStream_t (NULL = default stream).  Asynchronous.
 * Launches on one ctx are stream-ordered by the library: the work-queue
 * counters and planner workspace belong to the ctx, so a launch on a stream
 * other than the ctx's previous one first waits on an event recorded after
 * that launch (never two kernels of one ctx at once).  Use one ctx per
 * stream for concurrent batches. */
#define ESPGPU_BATCH_GROUPED 0x1
int  espgpu_decrypt_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_desc *d_desc,
                          uint32_t n, uint8_t *d_status, uint8_t *d_out, uint32_t flags,
                          void *stream);
int  espgpu_encrypt_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_desc *d_desc,
                          uint32_t n, uint8_t *d_status, uint32_t flags, void *stream);

/* espgpu_decrypt_batch with a packed output: the plaintext (ESP payload) of
 * record i lands at d_out + i * out_stride instead of the record's own offset,
 * every 128-byte line of it written whole (out_stride a nonzero multiple of
 * 128; d_out 128-byte aligned, n * out_stride bytes, not overlapping d_arena:
 * EINVAL for an unaligned d_out or d_out == d_arena; a partial overlap cannot
 * be detected and races with the ciphertext reads).  A record whose payload
 * is longer than out_stride is EINVAL.  Single pass, like the out-of-place
 * espgpu_decrypt_batch: a record whose status is nonzero (EBADMSG) still has
 * its unverified plaintext in its slot, which the consumer must ignore
 * (swcr_gcm releases no plaintext for it, cryptosoft.c:600-603).  For a
 * device-side consumer of the plaintext; the line-aligned stores make the
 * kernel ≈ 4-6 % faster than the record layout's.  GCM
 * contexts only: ENOTSUP when the context has ETA or DIGEST sessions.  No esp_input_cb
 * trailer words. */
int  espgpu_decrypt_batch_packed(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_desc *d_desc,
                                 uint32_t n, uint8_t *d_status, uint8_t *d_out, uint32_t out_stride,
                                 uint32_t flags, void *stream);

/* Decrypt + the ESP trailer checks of esp_input_cb (xform_esp.c:597-630)
 * fused into the kernels: d_trailer[i] (one 32-bit word per record) gets
 *   bits 0-7  next header, bits 8-15 pad length (the last 3 plaintext bytes),
 *   ESPGPU_TR_BADLEN  pad length + 2 > payload length       (esps_badilen),
 *   ESPGPU_TR_BADPAD  last pad byte != pad length != 0       (esps_badenc; the
 *                     caller ignores it for SADB_X_EXT_PRAND SAs),
 *   ESPGPU_TR_NONE    next header == IPPROTO_NONE (59)       (silent drop),
 *   ESPGPU_TR_VALID   set for every record whose status is 0;
 * and 0 for records that failed (status != 0).  Otherwise as
 * espgpu_decrypt_batch. */
#define ESPGPU_TR_BADLEN 0x00010000u
#define ESPGPU_TR_BADPAD 0x00020000u
#define ESPGPU_TR_NONE   0x00040000u
#define ESPGPU_TR_VALID  0x80000000u
int  espgpu_decrypt_batch_trailer(espgpu_ctx *ctx, uint8_t *d_arena,
                                  const struct espgpu_desc *d_desc, uint32_t n,
                                  uint8_t *d_status, uint8_t *d_out, uint32_t *d_trailer,
                                  uint32_t flags, void *stream);

/* Host-to-host pipelined decrypt of a large host-resident batch (the shape of
 * an offload from DPDK hugepage mbufs): records in h_arena (pinned: hipHostMalloc
 * or hipHostRegister), descriptors in ascending arena order; `chunk` records per
 * step (0 = 65536).  Step k's H2D, step k-1's kernels and step k-2's D2H run
 * concurrently on three HIP streams.  Plaintext lands in h_out at the same
 * offsets; returns when everything is back.  ENOTSUP while the context has
 * DIGEST (AH) sessions: their records produce no output to carry back. */
int  espgpu_decrypt_host(espgpu_ctx *ctx, const uint8_t *h_arena, uint64_t arena_bytes,
                         const struct espgpu_desc *h_desc, uint32_t n, uint8_t *h_status,
                         uint8_t *h_out, uint32_t chunk, uint32_t flags);

/* ---- replay window (esp_input's pre-crypto check and esp_input_cb's
 *      update, freebsd/netipsec/xform_esp.c:329-340, :565-580) ----
 * One SA's window as ipsec_chkreplay reads it (struct secreplay,
 * netipsec/keydb.h:206-213): `last` = ESN high << 32 | low of the window
 * top, `wsize` in bytes (window = wsize * 8 packets, 0 = no replay check),
 * `bitmap_size` u32 words (a power of two, key.c:3346-3351) starting at word
 * `bitmap_off` of a shared bitmap array.
 *
 * The inbound sequence on a device-resident batch, windows and bitmaps in
 * device memory from one batch to the next, all on one stream:
 *   0. espgpu_esp_classify_batch   header sanity, SPI lookup; builds d_desc
 *                                  from received packets (below; a caller that
 *                                  has descriptors already starts at 1)
 *   1. espgpu_replay_check_batch   ipsec_chkreplay; fills desc.esn_hi
 *   2. espgpu_decrypt_batch        ICV check, decrypt (trailer checks)
 *   3. espgpu_replay_update_batch  ipsec_updatereplay for what authenticated
 *   4. espgpu_replay_merge, once with 1's and once with 3's result, and a
 *      third time with 0's: espgpu_replay_merge(d_status, d_cstatus, n).
 *   5. espgpu_esp_decap_batch      esp_input_cb's tail and ipsec4/6_common_
 *                                  input_cb: trailer verdict, strip, header fix,
 *                                  SA lifetime counters (the decapsulation block
 *                                  below; reads d_status as 4 left it)
 *  5b. espgpu_esp_natt_cksum_batch udp_ipsec_adjust_cksum for the transport
 *                                  packets of NAT-T SAs (the NAT-T block below;
 *                                  reads d_status and 5's d_dstatus); only for
 *                                  a caller with such SAs
 *   6. espgpu_replay_merge         with 5's: (d_status, d_dstatus, n).
 * espgpu_replay_update / _update64 are the same update on the host, one
 * record per call.  AH records have a sequence of their own (the inbound AH
 * block below).
 *
 * ESPGPU_REPLAY_AH marks the window of an AH SA.  An AH record is the whole
 * packet, so byte 4 of it is ip_id / ip_off; for a window with this flag the
 * check and the update read the sequence number big-endian at byte
 * desc.salt - 4 of the record (newah.ah_seq, directly before the ICV field),
 * and the record takes part if 12 <= desc.salt <= desc.len, in place of len >=
 * 8.  Windows without the flag behave as before; the host functions take the
 * sequence number as an argument and ignore the flag. */
#define ESPGPU_REPLAY_ESN    0x1     /* SADB_X_SAFLAGS_ESN  */
#define ESPGPU_REPLAY_CYCSEQ 0x2     /* SADB_X_EXT_CYCSEQ   */
#define ESPGPU_REPLAY_AH     0x4     /* the sequence number is at desc.salt - 4 (xform_ah.c:565, :776) */
#define ESPGPU_EACCES        13      /* replayed (esp_input's EACCES, esps_replay) */
struct espgpu_replay {
	uint64_t last;
	uint32_t wsize;
	uint32_t bitmap_size;
	uint32_t bitmap_off;
	uint32_t flags;
};

/* 1 if r's window parameters are usable: wsize 0 (no check), or bitmap_size
 * a power of two with bitmap_size * 32 >= wsize * 8 bits; else 0.  Both the
 * batch check and espgpu_replay_update index the bitmap with
 * bitmap_size - 1 as a mask: the caller of espgpu_replay_check_batch must
 * pass only windows this accepts (espgpu_replay_update returns EINVAL). */
int  espgpu_replay_params_ok(const struct espgpu_replay *r);
/* Pre-filter a device-resident batch against the windows as they stand
 * (ipsec_chkreplay, ipsec.c:1248-1331, for every record in parallel; the
 * record's SA indexes d_replay[nreplay]): d_rstatus[i] = 0 or ESPGPU_EACCES.
 * A replayed record's descriptor gets len = 0, so the decrypt kernels drop
 * it (status EINVAL) without crypto work; an accepted record of an ESN SA
 * gets esn_hi = the window's high word, as esp_input fills crp_esn.  Run it
 * before espgpu_decrypt_batch, then espgpu_replay_merge.  Asynchronous. */
int  espgpu_replay_check_batch(espgpu_ctx *ctx, const uint8_t *d_arena, struct espgpu_desc *d_desc,
                               uint32_t n, const struct espgpu_replay *d_replay, uint32_t nreplay,
                               const uint32_t *d_bitmap, uint8_t *d_rstatus, void *stream);
/* d_status[i] = d_rstatus[i] where that is nonzero. */
int  espgpu_replay_merge(espgpu_ctx *ctx, uint8_t *d_status, const uint8_t *d_rstatus, uint32_t n,
                         void *stream);
/* Host: ipsec_updatereplay (ipsec.c:1338-1436) for one authenticated record,
 * in arrival order per SA: 0 (window advanced / bit set) or ESPGPU_EACCES. */
int  espgpu_replay_update(struct espgpu_replay *r, uint32_t *bitmap, uint32_t seq);
/* Host: the same update on the 64-bit sequence number the record was
 * authenticated under: seq64 = esn_hi << 32 | seq for an ESN window, seq for
 * any other (the high word is ignored).  With T = r->last, W = wsize * 8:
 *   wsize == 0                         0
 *   !espgpu_replay_params_ok(r), or no redundant block
 *   (bitmap_size * 32 < W + 32; key.c:3343-3351 always allocates one)
 *                                      ESPGPU_EINVAL, nothing touched
 *   seq64 == 0 && T == 0               ESPGPU_EACCES
 *   seq64 > T                          advance, set the bit, last = seq64: 0
 *   seq64 + W > T (in the window)      ESPGPU_EACCES if its bit is set, else set it: 0
 *   otherwise (below the window)       ESPGPU_EACCES, nothing changes.
 * This is ipsec_updatereplay(seq) whenever seq64 is what that function infers
 * from seq (the value congruent to seq in [T-W+1, T-W+2^32]; for a non-ESN SA
 * with the high word unchanged), which holds for every record that passed
 * ipsec_chkreplay against the window of the moment.  The one deliberate
 * difference: an ESN record that was authenticated under high word h and has
 * fallen below the window since (earlier records of its batch moved the top)
 * is ESPGPU_EACCES here.  ipsec_updatereplay would infer h + 1 for it and
 * move the window by about 2^32, under a high word its ICV was never checked
 * with. */
int  espgpu_replay_update64(struct espgpu_replay *r, uint32_t *bitmap, uint64_t seq64);
/* esp_input_cb's window update for a device-resident batch, after
 * espgpu_decrypt_batch.  Record i takes part if d_status[i] == 0 (it
 * authenticated), d_desc[i].sa < nreplay, its len >= 8 and its window has
 * wsize != 0; seq is read big-endian at byte 4 of the record and esn_hi from
 * the descriptor, where espgpu_replay_check_batch put it.  d_ustatus[i] is
 * what espgpu_replay_update64 returns when applied to each SA's taking-part
 * records one after another in index (arrival) order, starting from
 * d_replay[sa] and d_bitmap as they stand; 0 for records that take no part.
 * When the work completes, every d_replay[sa].last and every window's bitmap
 * words equal that sequential run's; words outside the windows are untouched.
 * The records of a window with unusable parameters get ESPGPU_EINVAL and the
 * window is not touched.  espgpu_replay_merge(d_status, d_ustatus, n) folds
 * the result in.  Asynchronous, no host round trip; stream-ordered on the
 * ctx like the other batch entries (the workspace belongs to the ctx and
 * grows with n and nreplay: ESPGPU_ENOMEM, with nothing launched and the ctx
 * healthy, if it cannot be allocated). */
int  espgpu_replay_update_batch(espgpu_ctx *ctx, const uint8_t *d_arena,
                                const struct espgpu_desc *d_desc, uint32_t n, const uint8_t *d_status,
                                struct espgpu_replay *d_replay, uint32_t nreplay, uint32_t *d_bitmap,
                                uint8_t *d_ustatus, void *stream);

/* ---- outbound framing (what esp_output does between m_makespace and
 *      crypto_dispatch, freebsd/netipsec/xform_esp.c:703-716, :782-887) ----
 * One SA's outbound state as esp_output reads and advances it under the SA
 * lock (struct secasvar / secreplay, netipsec/keydb.h).  The entry at index
 * `sa` belongs to the session with that id.
 *
 * The outbound sequence on a device-resident batch, the per-SA counters in
 * device memory from one batch to the next, all on one stream:
 *   1. espgpu_esp_frame_batch   SPI, sequence number, counter IV, padding,
 *                               trailer; fills desc.esn_hi and desc.salt
 *   2. espgpu_encrypt_batch     encrypt, ICV
 *   3. espgpu_replay_merge      with 1's result (d_status, d_fstatus, n).
 * A caller that holds cleartext IP packets puts espgpu_esp_encap_batch in
 * front and espgpu_esp_sent_batch behind (the encapsulation block below).
 * espgpu_esp_frame is the same rule on the host, one record per call. */
#define ESPGPU_OUT_ESN       0x01    /* SADB_X_SAFLAGS_ESN: esn_hi = count >> 32 (:799)        */
#define ESPGPU_OUT_CYCSEQ    0x02    /* SADB_X_EXT_CYCSEQ: the sequence number may cycle       */
#define ESPGPU_OUT_WRAPCHECK 0x04    /* refuse at the end of the number space, as ah_output
                                        does (xform_ah.c:940-950); esp_output has no such check */
#define ESPGPU_OUT_CTRCOMPAT 0x08    /* V_esp_ctr_compatibility (:710-713): an AES-CTR SA
                                        pads to 16 instead of 4                                */
#define ESPGPU_OUT_PAD_SEQ   0x10    /* SADB_X_EXT_PSEQ (:831-834): pad bytes 1, 2, 3, ...     */
#define ESPGPU_OUT_PAD_ZERO  0x20    /* SADB_X_EXT_PZERO (:828-829): pad bytes zero            */
#define ESPGPU_OUT_PAD_RAND  0x40    /* SADB_X_EXT_PRAND (:825-826): the pad bytes are the
                                        caller's (random data), as with no pad flag at all;
                                        PAD_SEQ goes before PAD_ZERO if both are set           */
struct espgpu_outsa {
	uint64_t count;         /* sav->replay->count: the last sequence number given out   */
	uint64_t cntr;          /* sav->cntr: the next explicit IV of a CTR/GCM SA           */
	uint32_t spi;           /* host order; written big-endian                            */
	uint32_t salt;          /* as espgpu_desc.salt; copied into it for CTR/GCM SAs       */
	uint32_t flags;         /* ESPGPU_OUT_*                                              */
	uint32_t pad_;
};
/* esp_output's lengths for one SA: hlen = 8 + ivlen (struct newesp + IV; 8
 * for CTR/GCM, whose IV is the counter, 16 for CBC, 0 for NULL), blks =
 * MAX(4, blocksize) (:710-713), alen = xform_ah_authsize (:718). */
struct espgpu_eshape {
	uint32_t ivlen, blks, alen;
};
/* The shape of an ESP session the engine serves (AEAD; ETA with CBC, CTR or
 * NULL; CIPHER) under the SA's ESPGPU_OUT_* flags (CTRCOMPAT matters): 0, or
 * ESPGPU_EINVAL for a DIGEST (AH) session or parameters espgpu_newsession
 * refuses.  Host-only. */
int  espgpu_esp_frame_shape(const struct espgpu_session_params *csp, uint32_t flags,
                            struct espgpu_eshape *shape);
/* Host: frame one record for SA `o`, in arrival order per SA.  `rec` holds
 * `len` bytes with the rlen raw payload bytes at rec + hlen; the record takes
 * part if len == hlen + rlen + padding + alen with padding = ((blks - ((rlen +
 * 2) % blks)) % blks) + 2 (:716), else ESPGPU_EINVAL with nothing touched.
 *   Default: esp_output to the letter.  count++ (:793); the SPI goes to byte 0
 *     and the low 32 bits of count big-endian to byte 4 (:783-797); *esn_hi =
 *     count >> 32 for an ESN SA, else 0.  No wrap check.
 *   With WRAPCHECK and without CYCSEQ: if count == ~0, or for a non-ESN SA
 *     (uint32_t)count == ~0, ESPGPU_EINVAL and nothing is touched: not rec,
 *     not *o, not *esn_hi.
 *   CTR/GCM SAs (ivlen 8): cntr++ and its value before that big-endian into
 *     the 8 IV bytes at byte 8 (:802-803, :869-881); the caller copies o->salt
 *     into the descriptor.  CBC SAs: the 16 IV bytes are the caller's
 *     (arc4rand, :884) and stay as they are.
 *   Padding (:824-835): PAD_SEQ writes 1, 2, 3, ..., PAD_ZERO zeros; otherwise
 *     the padding - 2 pad bytes stay as they are.  Then pad[padding - 2] =
 *     padding - 2 and pad[padding - 1] = next_header (:838-839).
 * The payload, the ICV field and everything outside the record are untouched. */
int  espgpu_esp_frame(struct espgpu_outsa *o, const struct espgpu_eshape *shape, uint8_t *rec,
                      uint32_t len, uint32_t rlen, uint8_t next_header, uint32_t *esn_hi);
/* Frame a device-resident batch for espgpu_encrypt_batch.  d_desc[i] carries
 * off4, len (the full record) and sa from the caller; d_frame[i] holds rlen
 * in bits 0-15 and the next header in bits 16-23; d_out[nout] is indexed by
 * the session id.  The shape is the ctx's own session `sa`'s, so a record
 * takes part if sa < nout, the session exists and is not a DIGEST one, and
 * len fits as for espgpu_esp_frame.  The result is espgpu_esp_frame applied
 * to each SA's taking-part records one after another in index (arrival)
 * order, starting from d_out[sa] as it stands: the record bytes, d_desc[i].
 * esn_hi, d_desc[i].salt = d_out[sa].salt for CTR/GCM SAs, d_fstatus[i] = 0,
 * and the SA's count / cntr when the work completes.  A record that takes no
 * part or is refused by WRAPCHECK (then so is the rest of its SA's batch)
 * gets d_fstatus[i] = ESPGPU_EINVAL and d_desc[i].len = 0, so the encrypt
 * kernels drop it; it consumes no number and nothing else of it is written.
 * The entries of SAs with no accepted record are untouched.  Asynchronous, no
 * host round trip; stream-ordered on the ctx like the other batch entries
 * (it shares espgpu_replay_update_batch's workspace: ESPGPU_ENOMEM, with
 * nothing launched and the ctx healthy, if that cannot grow). */
int  espgpu_esp_frame_batch(espgpu_ctx *ctx, uint8_t *d_arena, struct espgpu_desc *d_desc,
                            const uint32_t *d_frame, uint32_t n, struct espgpu_outsa *d_out,
                            uint32_t nout, uint8_t *d_fstatus, void *stream);

/* ---- inbound classification (ip_input's header sanity, ipsec4_input /
 *      ipsec6_input, ipsec_common_input's SPI lookup and esp_input's first
 *      checks: freebsd/netinet/ip_input.c:488-561, :807,
 *      netipsec/ipsec_input.c:116-226, key.c:1091-1133, xform_esp.c:279-284) ----
 * Step 0 of the inbound sequence (replay block above): from received packets
 * in the arena to the espgpu_desc every later step takes.
 *
 * The SPI table is open addressing with linear probing.  The home slot of an
 * SPI is key_u32hash(spi) & (nslots - 1), the hash of the reference's SPI
 * hash (key.c:258-259, :295-299: FNV-1 over the SPI's four network-order
 * bytes); a slot with spi == 0 is free and ends a probe.  There is one SPI
 * namespace for all protocols, and protocol, family and destination are
 * compared only after the SPI matched, as key_allocsa does.  The table is
 * read-only to every entry point: a changed SA set is a table rebuilt in
 * another buffer, and stream order makes the switch safe. */
struct espgpu_pkt {            /* 8 B: one received packet in the arena               */
	uint32_t off4;             /* start of the IP header, in 4-byte units              */
	uint32_t len;              /* bytes the buffer holds from there (m_pkthdr.len)     */
};
struct espgpu_sad_entry {      /* 32 B: one slot of the SPI table; spi == 0: free      */
	uint32_t spi;              /* host order                                           */
	uint16_t sa;               /* session id (espgpu_newsession's)                     */
	uint8_t  proto;            /* 50 (ESP) or 51 (AH): saidx.proto                     */
	uint8_t  af;               /* 4 or 6                                               */
	uint32_t salt;             /* as espgpu_desc.salt; copied into the descriptor      */
	uint32_t flags;            /* 0 or ESPGPU_SAD_NATT                                 */
	uint8_t  dst[16];          /* saidx.dst: 4 bytes + 12 zeros for af 4; with
	                              ESPGPU_SAD_NATT natt->sport in dst[4..5] and
	                              natt->dport in dst[6..7], network order           */
};
#define ESPGPU_CLS_IPCSUM 0x1  /* verify the IPv4 header checksum (ip_input.c:518-530) */
#define ESPGPU_SAD_NATT   0x2  /* sav->natt != NULL (keydb.h:94-103): proto 50, af 4 only */
#define ESPGPU_CLS_AH     0x4  /* classify ip_p / ip6_nxt 51 packets too (2b, 3b below); clear: ENOTSUP */
/* Bits 16-31 of the classification flags: the local UDP encapsulation port in
 * host order (the socket with UF_ESPINUDP, udp_usrreq.c:335); 0: off. */
#define ESPGPU_CLS_NATT_PORT(p) ((uint32_t)((p) & 0xffffu) << 16)
/* Host: zero table[nslots] and insert sas[nsas] in order.  ESPGPU_EINVAL
 * (table contents then unspecified) unless nslots is a power of two with
 * nslots >= 2 * nsas (so a free slot ends every probe), and for an entry with
 * spi 0, an SPI seen before (key.c:1106-1109), proto not 50 or 51, af not 4
 * or 6, flags other than 0 or ESPGPU_SAD_NATT, ESPGPU_SAD_NATT on an entry
 * that is not proto 50 and af 4 (udpencap.c:155-163: IPv4 outer only), an af
 * 4 entry without the flag whose dst[4..15] is not zero, or one with it whose
 * dst[8..15] is not zero. */
int  espgpu_sad_build(const struct espgpu_sad_entry *sas, uint32_t nsas,
                      struct espgpu_sad_entry *table, uint32_t nslots);
/* Host: classify one packet of `len` bytes at `pkt`; `off4` is where it lies
 * in the arena the descriptor will index.  Status 0 fills *desc = {off4 +
 * skip / 4, record length, entry.sa, 0, entry.salt}; any other status fills
 * {off4, 0, 0xffff, 0, 0}, which the replay check, the decrypt kernels and the
 * window update all pass over.  Nothing is read outside [pkt, pkt + len), and
 * of the packet nothing beyond the IP header, a UDP header and the SPI.  The checks, in
 * order; the first that fires decides:
 *   1. len < 20, version nibble neither 4 nor 6                      EINVAL
 *   2. IPv4: hlen = ip_hl * 4 < 20, or hlen > len                    EINVAL
 *      with ESPGPU_CLS_IPCSUM in flags, header checksum wrong        EINVAL
 *      ip_len < hlen, or ip_len > len                                EINVAL
 *        (bytes past ip_len are ignored: the trim, ip_input.c:555-561)
 *      a fragment, ip_off & (IP_MF | IP_OFFMASK)                     ENOTSUP
 *      ip_p == 17 with a port in flags: 2a below decides
 *      ip_p != 50 (AH, IPComp, non-IPsec; UDP without a port set)    ENOTSUP
 *      ip_len - hlen < 8 (ipsec_input.c:141)                         EINVAL
 *      ip_len & 3 (xform_esp.c:279)                                  EINVAL
 *      skip = hlen, record length = ip_len - hlen
 *  2a. ESP in UDP (RFC 3948), only with ESPGPU_CLS_NATT_PORT(port) in flags
 *      (port 0: off, and every UDP packet is ENOTSUP as above); udp_input up
 *      to the UF_ESPINUDP socket (udp_usrreq.c:335-339, :468-474) and
 *      udp_ipsec_input (udpencap.c:115-210):
 *      ip_len - hlen < 8, or uh_dport != port (an ordinary datagram)  ENOTSUP
 *      uh_ulen < 8, or uh_ulen > ip_len - hlen (:468-472)            EINVAL
 *        (bytes past uh_ulen are ignored: the trim, :474; ulen = uh_ulen)
 *      uh_sum != 0 (udp_input would verify it over the whole
 *        datagram, :489-520; RFC 3948 senders send 0)                ENOTSUP
 *      ulen - 8 < 8 (the keepalive, udpencap.c:131-132)              ENOTSUP
 *      the SPI dword is 0 (the non-ESP marker: IKE, :135)            ENOTSUP
 *      (ulen - 8) & 3 (xform_esp.c:279)                              EINVAL
 *      skip = hlen + 8, record length = ulen - 8; after the lookup of 4:
 *      the entry lacks ESPGPU_SAD_NATT, or uh_sport / uh_dport are not
 *        its dst[4..5] / dst[6..7] (udpencap.c:173-181)              ENOENT
 *  2b. AH, only with ESPGPU_CLS_AH in flags (without it ip_p 51 is ENOTSUP as
 *      above), after the sanity and fragment checks of 2:
 *      ip_len - hlen < 12 (struct newah up to the ICV)               EINVAL
 *        (a deliberate difference, one code before the lookup: the reference
 *        answers EINVAL below 8, ipsec_input.c:141, and ENOBUFS from ah_input's
 *        pullup for 8..11, xform_ah.c:551-558.  No & 3 check: that is ESP's.)
 *      skip = hlen, record length = ip_len: the whole packet
 *   3. IPv6: len < 40                                                EINVAL
 *      payload length 0 (jumbogram)                                  ENOTSUP
 *      40 + plen > len                                               EINVAL
 *      next header != 50 (extension headers are the host's)          ENOTSUP
 *      destination in fe80::/10 (scope, ipsec_input.c:184-189)       ENOTSUP
 *      plen < 8, or plen & 3                                         EINVAL
 *      skip = 40, record length = plen
 *  3b. AH, only with ESPGPU_CLS_AH: next header 51 passes the next-header row
 *      and the fe80::/10 row of 3, then
 *      plen < 12                                                     EINVAL
 *      40 + plen > 65535 (espgpu_desc.len has 16 bits)               ENOTSUP
 *      skip = 40, record length = 40 + plen
 *   4. the SPI (big-endian dword at skip; for AH at skip + 4,
 *      ipsec_input.c:151-153) is 0, no slot holds it, or the slot's proto is
 *      not the packet's (50, or 51 for AH), its af is not the packet's, or its
 *      dst is not the packet's destination (4 or 16 bytes)           ENOENT
 *      a plain ip_p 50 packet whose entry has ESPGPU_SAD_NATT        ENOTSUP
 *        (a deliberate difference: ipsec_common_input would take it, but the
 *        later steps tell a UDP-encapsulated packet by its SA alone, so the
 *        host stack decides)
 *   An accepted AH packet's descriptor is {off4, record length, entry.sa, 0,
 *   skip + 12}: the DIGEST record of the batch path, the whole packet with the
 *   ICV field's offset in salt; the entry's salt is ignored for proto 51.
 * Fragments, AH without ESPGPU_CLS_AH, UDP-encapsulated ESP with a nonzero UDP checksum, NAT-T
 * keepalives, IKE and everything else answered ENOTSUP are the host stack's
 * packets; IPv6 NAT-T does not exist in the reference either.  Not re-checked: the per-transform lengths (the decrypt kernels'
 * EINVAL), whether session `sa` exists (theirs too), loopback and other
 * address filters (ip_input's; the caller's).  A null or unusable table
 * (nslots not a power of two) is EINVAL. */
int  espgpu_esp_classify(const struct espgpu_sad_entry *table, uint32_t nslots,
                         const uint8_t *pkt, uint32_t len, uint32_t off4, uint32_t flags,
                         struct espgpu_desc *desc);
/* The same rule for n packets of a device-resident arena: d_desc[i] and
 * d_cstatus[i] are what espgpu_esp_classify gives for the packet at d_arena +
 * d_pkt[i].off4 * 4.  d_table is the uploaded result of espgpu_sad_build, 16-
 * byte aligned; d_arena is 4-byte aligned (EINVAL otherwise).  Writes d_desc
 * and d_cstatus only.  Asynchronous, no workspace, no host round trip; n == 0
 * is a no-op that returns 0. */
int  espgpu_esp_classify_batch(espgpu_ctx *ctx, const uint8_t *d_arena,
                               const struct espgpu_pkt *d_pkt, uint32_t n,
                               const struct espgpu_sad_entry *d_table, uint32_t nslots,
                               uint32_t flags, struct espgpu_desc *d_desc,
                               uint8_t *d_cstatus, void *stream);

/* ---- inbound decapsulation (esp_input_cb after the window update and
 *      ipsec4_common_input_cb / ipsec6_common_input_cb up to netisr_queue:
 *      freebsd/netipsec/xform_esp.c:581-648, ipsec_input.c:298-417, :531-566,
 *      key_sa_recordxfer, key.c:8429-8445) ----
 * Steps 5 and 6 of the inbound sequence (replay block above): from a decrypted
 * record, its status and its trailer word to the packet the stack takes next.
 * One SA's inbound state as those functions read and advance it; the entry at
 * index `sa` belongs to the session with that id.  Left to the caller or the
 * host stack: the hhooks / enc(4), ipsec_if_input, ip_input of the inner
 * packet and the SPD check.  The NAT-T checksum adjustment is step 5b, the
 * NAT-T block below. */
#define ESPGPU_IN_TRANSPORT 0x1   /* saidx.mode == IPSEC_MODE_TRANSPORT                      */
#define ESPGPU_IN_TUNNEL    0x2   /* IPSEC_MODE_TUNNEL; neither bit: IPSEC_MODE_ANY; both: unusable */
#define ESPGPU_IN_PAD_RAND  0x4   /* SADB_X_EXT_PRAND: ESPGPU_TR_BADPAD is ignored (:613)    */
#define ESPGPU_IN_AF6       0x8   /* saidx.dst is AF_INET6 (esp_input_cb picks the callback
                                     by the SA's family, :638-648); clear: AF_INET           */
#define ESPGPU_IN_NATT      0x20  /* sav->natt != NULL: the packet came UDP-encapsulated
                                     (the NAT-T block below); AF_INET only                   */
#define ESPGPU_IN_AH        0x40  /* an AH SA: espgpu_ah_input / espgpu_ah_decap take it (the inbound
                                     AH block below); espgpu_esp_decap refuses it                */
#define ESPGPU_IN_AH_KEEPTOS 0x80 /* V_ah_cleartos == 0: ip_tos is hashed as it came; clear (the
                                     reference default): zeroed.  Only with ESPGPU_IN_AH        */
#define ESPGPU_ENODATA      61    /* next header IPPROTO_NONE: RFC 4303 2.6 dummy, dropped   */
#define ESPGPU_EPFNOSUPPORT 96    /* ipsec4_common_input_cb: "cannot handle inner ip proto"  */
struct espgpu_insa {              /* 24 B, indexed by session id, lives in device memory     */
	uint64_t bytes;               /* lft_c_bytes                                             */
	uint64_t packets;             /* lft_c_allocations                                       */
	uint32_t flags;               /* ESPGPU_IN_*                                             */
	uint32_t natt_cksum;          /* low 16 bits: sav->natt->cksum, the raw value that is
	                                 added to the checksum field's two bytes as they lie in
	                                 memory; read by espgpu_esp_natt_cksum only              */
};
/* Host: decapsulate one packet of SA `in`.  `pkt` points at the outer IP
 * header (`skip` bytes), the decrypted record lies at pkt + skip and is rlen
 * bytes long, `shape` is the session's (hlen = 8 + ivlen, alen; blks is not
 * read) and `trailer` the word espgpu_decrypt_batch_trailer gave for the
 * record.  With plen = rlen - hlen - alen, padlen and nxt from the trailer
 * word and q = plen - padlen - 2, the checks in order; the first that fires
 * decides, and a refused packet has nothing written, books nothing and gets
 * *out_off = *out_len = 0:
 *   1. flags with unknown bits or both mode bits                     EINVAL
 *      ESPGPU_IN_NATT with ESPGPU_IN_AF6                             EINVAL
 *      skip & 3; skip not in 20..60 (AF_INET), 28..68 (AF_INET with
 *        ESPGPU_IN_NATT: the IP header and the 8 UDP bytes), or not
 *        40 (AF6)                                                    EINVAL
 *      plen < 2 (also ivlen not 0, 8 or 16)                          EINVAL
 *      the trailer word without ESPGPU_TR_VALID                      EINVAL
 *      ESPGPU_TR_BADLEN (xform_esp.c:601, esps_badilen)              EINVAL
 *      ESPGPU_TR_BADPAD without ESPGPU_IN_PAD_RAND (:613-614)        EINVAL
 *      ESPGPU_TR_NONE (:629)                                         ENODATA
 *   2. AF_INET SA (ipsec_input.c:333-365, :395-417):
 *      nxt 4 and not TRANSPORT: q < 20 EINVAL (:336), else tunnel (:342)
 *      nxt 41 and not TRANSPORT: q < 40 EINVAL (:348), else tunnel (:354)
 *      else TRANSPORT or ANY: transport (:357-365, :395-396)
 *      else (TUNNEL, any other nxt)                                  EPFNOSUPPORT (:411-416)
 *   3. AF6 SA (:538-566):
 *      nxt 41 and not TRANSPORT: q < 40 EINVAL (:541), else tunnel (:547)
 *      nxt 4 and not TRANSPORT: q < 20 EINVAL (:554), else tunnel (:560)
 *      else transport: the protocol loop takes the packet in place (:564-566, :639-646)
 *   4. tunnel: the packet is neither read nor written; the result is
 *      {skip + hlen, q} and the SA books q bytes (m_pkthdr.len after :342 / :547).
 *   5. transport: the outer header's skip bytes move forward by hlen, to end
 *      where the plaintext starts (m_striphdr, xform_esp.c:588).
 *      IPv4: ip_hl * 4 != skip or version nibble not 4               EINVAL
 *        ip_len = skip + q (ipsec_input.c:312), ip_p = nxt (xform_esp.c:636),
 *        ip_sum zeroed and recomputed over skip bytes as in_cksum does
 *        (:313-314), never updated incrementally.
 *      IPv6: version nibble not 6                                    EINVAL
 *        ip6_plen = q (:532), ip6_nxt = nxt (xform_esp.c:636).
 *      Every header byte is loaded before any is stored (the two ranges
 *      overlap whenever hlen < skip).  The result is {hlen, skip + q} and the
 *      SA books skip + q bytes.  [pkt, pkt + hlen), the padding, the trailer
 *      and the ICV stay as they are (m_adj only shortens, :633).
 *      ESPGPU_IN_NATT: the IP header is the first skip - 8 bytes and moves
 *      forward by hlen + 8, over the UDP header too (the m_striphdr of
 *      udpencap.c:196 and that of xform_esp.c:588); ip_hl * 4 != skip - 8 is
 *      EINVAL, ip_len = skip - 8 + q, and the result is {hlen + 8, skip - 8 +
 *      q} with as many bytes booked.  A tunnel result is {skip + hlen, q} as
 *      ever.
 *   6. accepted: in->bytes += booked, in->packets += 1 (key.c:8429-8445).
 * *out_off is relative to pkt, *out_len the new m_pkthdr.len.  Null pointers
 * are EINVAL. */
int  espgpu_esp_decap(struct espgpu_insa *in, const struct espgpu_eshape *shape,
                      uint8_t *pkt, uint32_t skip, uint32_t rlen, uint32_t trailer,
                      uint32_t *out_off, uint32_t *out_len);
/* The same rule for a device-resident batch, after the merges of the check's
 * and the update's results into d_status.  Record i takes part if d_status[i]
 * == 0, d_desc[i].sa < nin and the ctx holds an ESP session with that id (as
 * espgpu_esp_frame_batch: not a DIGEST session, not a free slot); its shape
 * is that session's, skip = (d_desc[i].off4 - d_pkt[i].off4) * 4 and rlen =
 * d_desc[i].len.  The header is read from d_arena and written into d_out,
 * where the decrypt put the plaintext; d_out == d_arena is the in-place form,
 * otherwise d_arena is not written.  d_dstatus[i] is the rule's status and
 * d_ipkt[i] = {d_pkt[i].off4 + out_off / 4, out_len}: absolute, so the array
 * can be given to espgpu_esp_classify_batch for nested ESP.  A record with
 * d_status[i] != 0 gets d_dstatus[i] = 0 and d_ipkt[i] = {d_pkt[i].off4, 0};
 * one with status 0 that cannot take part gets EINVAL and the same empty
 * d_ipkt[i].  When the work completes every d_in[sa] holds the sums of its
 * accepted records (order-free: summed per wave, and per workgroup where one
 * SA has all of it, before the 64-bit adds; never one add per record).  Both
 * buffers are 4-byte aligned (EINVAL otherwise).  Asynchronous on the
 * caller's stream, no workspace, no host round trip; n == 0 is a no-op that
 * returns 0. */
int  espgpu_esp_decap_batch(espgpu_ctx *ctx, const uint8_t *d_arena, uint8_t *d_out,
                            const struct espgpu_pkt *d_pkt, const struct espgpu_desc *d_desc,
                            const uint32_t *d_trailer, const uint8_t *d_status, uint32_t n,
                            struct espgpu_insa *d_in, uint32_t nin,
                            struct espgpu_pkt *d_ipkt, uint8_t *d_dstatus, void *stream);

/* ---- outbound encapsulation (ipsec4_perform_request / ipsec6_perform_request,
 *      ipsec_encap, esp_output's m_makespace / m_pad and protocol field, and
 *      ipsec_process_done: freebsd/netipsec/ipsec_output.c:221-242, :531-590,
 *      :720-770, :882-992, xform_esp.c:747, :772-780, :810-818, :839-843,
 *      netinet/ip_ecn.c:97-122, ip_id.c:252, key.c:8429-8445) ----
 * The steps around the framing block's sequence: from cleartext IP packets in
 * the arena (what decapsulation produces, mirrored) to the ESP-shaped records
 * espgpu_esp_frame_batch takes, and the SA's lifetime counters once a packet
 * is on its way.  The outbound sequence on a device-resident batch, all on one
 * stream:
 *   1. espgpu_esp_encap_batch   transport or tunnel, outer header, header move,
 *                               lengths, protocol field, checksum, size check;
 *                               builds d_desc, d_frame and d_opkt
 *   2. espgpu_esp_frame_batch   (the framing block above)
 *   3. espgpu_encrypt_batch
 *   4. espgpu_replay_merge      with 2's result (d_status, d_fstatus, n)
 *   5. espgpu_replay_merge      with 1's (d_status, d_estatus, n)
 *   6. espgpu_esp_sent_batch    key_sa_recordxfer for what went through
 * d_opkt is then the list of wire packets, in the form
 * espgpu_esp_classify_batch takes.  One SA's outbound policy and lifetime
 * counters; the entry at index `sa` belongs to the session with that id.  Left
 * to the caller or the host stack: the SPD lookup that picks the SA (d_sa),
 * the hhooks / enc(4), random ip_id (ip_do_randomid needs a CSPRNG: the ids
 * here are a counter's), link-local SA addresses (the scope embedding of
 * ipsec_output.c:975-981), fragmentation of the result and ip_output of it.
 * udp_ipsec_output's header (ESPGPU_ENC_NATT) is built here, in its final wire
 * form: it depends on lengths only, so nothing moves after the encrypt. */
#define ESPGPU_ENC_TUNNEL      0x01  /* sp->req[idx]->saidx.mode == IPSEC_MODE_TUNNEL          */
#define ESPGPU_ENC_AF6         0x02  /* saidx.dst is AF_INET6; clear: AF_INET                  */
#define ESPGPU_ENC_DF_SET      0x04  /* V_ip4_ipsec_dfbit 1: DF set in an outer IPv4 header    */
#define ESPGPU_ENC_DF_COPY     0x08  /* V_ip4_ipsec_dfbit 2: copied from the inner header;
                                        neither bit: clear; both: unusable                     */
#define ESPGPU_ENC_ECN_ALLOWED 0x10  /* V_ip4_ipsec_ecn / V_ip6_ipsec_ecn 1 (ECN_ALLOWED)      */
#define ESPGPU_ENC_ECN_NOCARE  0x20  /* -1 (ECN_NOCARE); neither bit: ECN_FORBIDDEN, the
                                        default; both: unusable                                */
#define ESPGPU_ENC_RFC6864     0x40  /* V_ip_rfc6864: ip_id 0 when DF is set (ip_id.c:252)     */
#define ESPGPU_ENC_NATT        0x200 /* sav->natt != NULL: udp_ipsec_output's header (the NAT-T
                                        block below); natt->sport in dst[4..5], natt->dport in
                                        dst[6..7], network order; AF_INET only                 */
#define ESPGPU_ENC_AH          0x80  /* an AH SA: espgpu_ah_encap / espgpu_ah_sent take it (the
                                        outbound AH block below); EINVAL for espgpu_esp_encap   */
#define ESPGPU_ENC_AH_KEEPTOS  0x100 /* V_ah_cleartos == 0: ip_tos is hashed as it stands; clear
                                        (the default): as zero (xform_ah.c:293)                 */
#define ESPGPU_EMSGSIZE    90    /* the result would exceed IP_MAXPACKET (xform_esp.c:747)  */
#define ESPGPU_EAFNOSUPPORT 97    /* the packet is neither IPv4 nor IPv6 (ipsec_output.c:933) */
struct espgpu_encsa {             /* 56 B, indexed by session id, lives in device memory     */
	uint64_t bytes;               /* lft_c_bytes                                             */
	uint64_t packets;             /* lft_c_allocations                                       */
	uint32_t flags;               /* ESPGPU_ENC_*                                            */
	uint8_t  ttl;                 /* V_ip_defttl / V_ip6_defhlim: the outer header's value   */
	uint8_t  pad_[3];
	uint8_t  src[16];             /* saidx.src: 4 bytes + 12 zeros for AF_INET               */
	uint8_t  dst[16];             /* saidx.dst                                               */
};
/* Host: encapsulate one cleartext packet of `len` bytes at `pkt` for SA `e`.
 * `shape` is the session's (hlen = 8 + ivlen), `headroom` and `tailroom` the
 * bytes before pkt and after pkt + len that the sequence may write, `ip_id`
 * the value an outer IPv4 header gets.  Packets are in wire form (no embedded
 * scope: ipsec_encap's in6_clearscope, ipsec_output.c:928-929, has nothing to
 * do).  The checks in order; the first that fires decides, and a refused
 * packet has nothing written and zeros in the four results:
 *   1. flags with unknown bits, both DF bits or both ECN bits          EINVAL
 *      ESPGPU_ENC_NATT with ESPGPU_ENC_AF6 (udpencap.c:222-223)        EAFNOSUPPORT
 *      ESPGPU_ENC_NATT and src[4..15] or dst[8..15] not zero           EINVAL
 *      an AF6 SA whose src or dst is unspecified (:961-964)            EINVAL
 *      an AF6 SA whose src or dst is in fe80::/10 (the host's)         ENOTSUP
 *   2. len < 20 (nothing is read)                                      EINVAL
 *      version 4: ip_hl < 5 or ip_hl * 4 > len                         EINVAL
 *        skip = ip_hl * 4, the protocol field is ip_p
 *      version 6: len < 40                                             EINVAL
 *        skip = 40 and the protocol field is ip6_nxt, extension headers or
 *        not: ipsec6_perform_request passes sizeof(struct ip6_hdr) (:580)
 *      any other version (:932-933)                                    EAFNOSUPPORT
 *      len > 65535                                                     EMSGSIZE
 *        (a deliberate difference: the reference answers ENXIO for an IPv6
 *        inner packet here, :548-552, and has no such check for IPv4)
 *   3. the packet is encapsulated (tunnel) if ESPGPU_ENC_TUNNEL is set, if
 *      the SA's family differs from the packet's, or if the SA's dst is not
 *      the unspecified address and differs from the packet's destination
 *      (the proxy case; :224-228, :543-547); else transport.
 *      tunnel, and an AF_INET SA's src or dst is zero (:938-941)       EINVAL
 *   4. oh = 0 (transport), 20 or 40 (the outer header, by the SA's family);
 *      rlen = len - skip (transport) or len (tunnel); padding as for
 *      espgpu_esp_frame; total = (transport ? skip : oh) + hlen + rlen +
 *      padding + alen.
 *      total > 65535 (xform_esp.c:747)                                 EMSGSIZE
 *      hlen + oh > headroom, or padding + alen > tailroom (where
 *      m_makespace and m_pad would fail, :772-780, :810-818)           ENOBUFS
 *      ESPGPU_ENC_NATT: total + 8 > 65535 is EMSGSIZE (a deliberate
 *      difference: the reference lets ip_len wrap, udpencap.c:240), checked
 *      behind the first; the headroom needed is hlen + oh + 8 (:227-231).
 *   5. tunnel: first the inner header is fixed: IPv4 ip_len = len, ip_sum
 *      zeroed and recomputed over ip_hl * 4 bytes (ipsec_output.c:230-232);
 *      IPv6 ip6_plen = len - 40 (:533).  Then the outer header goes to pkt -
 *      hlen - oh.  IPv4 (:946-956): version 4, ip_hl 5, TOS from
 *      ip_ecn_ingress(mode, &tos, &itos) with itos the inner TOS or traffic
 *      class, ip_len = total, ip_id = 0 with RFC6864 and DF set, else ip_id,
 *      ip_off = DF by the policy (DF_COPY: the inner IPv4 DF bit; for an IPv6
 *      inner packet DF is set iff either policy bit is, :926), ip_ttl = e->ttl,
 *      ip_p = 50 (xform_esp.c:842-843), ip_src / ip_dst from the SA, ip_sum
 *      over the finished 20 bytes (ip_output.c:780-782).  IPv6 (:969-984):
 *      flow 0, version 6, the class from ip_ecn_ingress, ip6_plen = total - 40
 *      (:742), ip6_nxt = 50, ip6_hlim = e->ttl, the SA's addresses.  The next
 *      header of the frame word is 4 or 41 (xform_esp.c:839).
 *   6. transport: the skip header bytes move from pkt to pkt - hlen, every
 *      dword loaded before the first is stored (the ranges overlap whenever
 *      hlen < skip).  IPv4: ip_len = total (ipsec_output.c:727), ip_p = 50
 *      with the old value as the next header, ip_sum recomputed over skip
 *      bytes.  IPv6: ip6_plen = total - 40, ip6_nxt = 50 likewise.  Options
 *      and everything else in the header stay.
 *   7. *out_front = hlen + oh: the wire packet is {pkt - *out_front,
 *      *out_total}.  The ESP record is its last *out_reclen = hlen + rlen +
 *      padding + alen bytes, the length espgpu_esp_frame takes: it starts
 *      behind the outer header (at pkt - hlen) or behind the moved header (at
 *      pkt - hlen + skip), 4-byte aligned with pkt.  *out_frame = rlen | next
 *      header << 16.
 *   8. ESPGPU_ENC_NATT (udp_ipsec_output, udpencap.c:212-243): the IP header
 *      of 5 or 6 (the outer one, or the moved one) lies 8 bytes further down,
 *      and between it and the ESP header stand uh_sport = dst[4..5], uh_dport
 *      = dst[6..7], uh_ulen = total + 8 - the IP header's length, uh_sum = 0.
 *      The IP header has ip_p = 17, ip_len = total + 8 and ip_sum over the
 *      finished header.  The frame word's next header (4 / 41 / the old
 *      ip_p), the record's position and *out_reclen are as without the flag;
 *      *out_front = hlen + oh + 8 and *out_total = total + 8.
 * Only the header bytes named above are written: not the payload, the ESP
 * header, the IV, the padding, the trailer or the ICV field, which are
 * framing's and encryption's.  The counters are espgpu_esp_sent's.  Null
 * pointers and an unusable shape are EINVAL. */
int  espgpu_esp_encap(const struct espgpu_encsa *e, const struct espgpu_eshape *shape, uint8_t *pkt,
                      uint32_t len, uint32_t headroom, uint32_t tailroom, uint16_t ip_id,
                      uint32_t *out_front, uint32_t *out_total, uint32_t *out_reclen,
                      uint32_t *out_frame);
/* Host: key_sa_recordxfer of ipsec_process_done (ipsec_output.c:770) for one
 * packet that went through with status `status`: 0 books `len` bytes (the wire
 * packet's total; len - 8 for an ESPGPU_ENC_NATT SA: the reference books
 * before the UDP header exists, ipsec_output.c:770, :808) and one packet into
 * *e, anything else nothing.  Returns 0, or EINVAL for a null e. */
int  espgpu_esp_sent(struct espgpu_encsa *e, uint8_t status, uint32_t len);
/* The same rule for n packets of a device-resident arena.  d_pkt[i] is the
 * cleartext packet, d_sa[i] the SA the caller's SPD lookup chose for it,
 * d_enc[nenc] and d_out[nenc] are indexed by the session id (of d_out only
 * flags is read, for ESPGPU_OUT_CTRCOMPAT).  Packet i takes part if d_sa[i] <
 * nenc and the ctx holds an ESP session with that id (as
 * espgpu_esp_frame_batch: not a DIGEST session, not a free slot); its shape
 * is that session's and its ip_id (uint16_t)(id0 + i): the caller adds n to
 * its counter.  (ip_fillid draws from a per-CPU counter only for the packets
 * that need one, ip_id.c:257; here ids stay distinct within a batch.)
 * headroom and tailroom hold for every packet, and the caller guarantees that
 * the spans [pkt - headroom, pkt + len + tailroom) of one batch lie in the
 * arena and do not overlap.  An accepted packet gets d_desc[i] = {record off4,
 * *out_reclen, sa, 0, 0}, d_frame[i] = *out_frame, d_opkt[i] = {wire off4,
 * *out_total} and d_estatus[i] = 0.  A refused packet gets its status, one
 * that takes no part EINVAL, and both d_desc[i] = {d_pkt[i].off4, 0, 0xffff,
 * 0, 0} (classification's empty descriptor: framing refuses it, encryption
 * passes over it) and d_opkt[i] = {d_pkt[i].off4, 0}.  d_arena is 4-byte
 * aligned (EINVAL otherwise).  One lane per packet, asynchronous on the
 * caller's stream, no workspace, no host round trip; n == 0 is a no-op that
 * returns 0. */
int  espgpu_esp_encap_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_pkt *d_pkt,
                            const uint16_t *d_sa, uint32_t n, const struct espgpu_encsa *d_enc,
                            const struct espgpu_outsa *d_out, uint32_t nenc, uint32_t headroom,
                            uint32_t tailroom, uint32_t id0, struct espgpu_desc *d_desc,
                            uint32_t *d_frame, struct espgpu_pkt *d_opkt, uint8_t *d_estatus,
                            void *stream);
/* espgpu_esp_sent for a batch, after the merges: a record with d_status[i] ==
 * 0 and d_desc[i].sa < nenc books d_opkt[i].len bytes (8 fewer for an
 * ESPGPU_ENC_NATT SA) and one packet into d_enc[sa].  A step of its own because a record that framing refuses
 * (WRAPCHECK) never reaches ipsec_process_done in the reference either.  The
 * sums are order-free: summed per wave, and per workgroup where one SA has all
 * of it, before the 64-bit adds, as espgpu_esp_decap_batch's.  Asynchronous on
 * the caller's stream, no workspace; n == 0 is a no-op that returns 0. */
int  espgpu_esp_sent_batch(espgpu_ctx *ctx, const struct espgpu_pkt *d_opkt,
                           const struct espgpu_desc *d_desc, const uint8_t *d_status, uint32_t n,
                           struct espgpu_encsa *d_enc, uint32_t nenc, void *stream);

/* ---- NAT-T: ESP in UDP (RFC 3948; freebsd/netipsec/udpencap.c:115-293, called
 *      from netinet/udp_usrreq.c:335-339, netipsec/ipsec_output.c:804-813 and
 *      ipsec_input.c:318-326; struct secnatt, keydb.h:94-103) ----
 * The rule parts live in the blocks above: ESPGPU_SAD_NATT and
 * ESPGPU_CLS_NATT_PORT (classification, 2a), ESPGPU_IN_NATT (decapsulation)
 * and ESPGPU_ENC_NATT (encapsulation, 8; espgpu_esp_sent).  NAT-T is IPv4-outer
 * only, as the reference's (udpencap.c:155-163, :222-223).  Still the host
 * stack's: inbound datagrams with a nonzero UDP checksum, keepalives, IKE on
 * the same port, and IPv6 NAT-T, which the reference lacks.
 *
 * Step 5b of the inbound sequence, after espgpu_esp_decap_batch:
 * udp_ipsec_adjust_cksum (udpencap.c:245-293) on the decapsulated packet, the
 * transport-mode TCP / UDP checksum fix for addresses a NAT rewrote.
 * `policy` is net.inet.ipsec.natt_cksum_policy: 0 auto, nonzero recompute.
 * A packet of `len` bytes at `pkt` with next header nxt = trailer & 0xff takes
 * part if the SA has ESPGPU_IN_NATT and nxt is 6 or 17 (`prot` at
 * ipsec_input.c:318; never a tunnel result).  The transport header starts at
 * ip_hl * 4 and the checksum field is at +16 (TCP) or +6 (UDP).  Left alone:
 * a packet that is not IPv4 with 20 <= ip_hl * 4 <= len <= 65535, or too
 * short to hold the field.
 *   auto (:261-281), delta = the low 16 bits of in->natt_cksum:
 *     delta != 0: a zero UDP checksum stays (:267-268); otherwise field =
 *       in_addword(field, delta), both as 16-bit values in memory order.
 *     delta == 0: the UDP field becomes 0 (:279).  TCP is untouched and
 *       *out_cflags = ESPGPU_NATT_CSUM_VALID: what the reference says with
 *       CSUM_DATA_VALID | CSUM_PSEUDO_HDR and csum_data 0xffff (:272-278).
 *   recompute (:282-292 with in_delayed_cksum, ip_output.c:1059-1091): field =
 *     ~(in_pseudo(ip_src, ip_dst, htons(len - ip_hl * 4 + nxt)) + the segment
 *     with the field as zero), the segment being ip_len - ip_hl * 4 bytes for
 *     TCP and uh_ulen bytes for UDP, an odd last byte as the low byte of a
 *     word (in_masks), and for UDP a result of 0 stored as 0xffff.  The sums
 *     fold as the reference's REDUCE16 / ADDCARRY do: 0 only for a sum of 0.
 *     Left alone (deliberately: the reference would sum past the mbuf, or a
 *     span the pseudo-header does not describe): a UDP packet with uh_ulen < 8
 *     or uh_ulen > len - ip_hl * 4, a TCP packet with ip_len != len.
 * Nothing but the field's two bytes is written, and nothing outside [pkt, pkt
 * + len) is read.  *out_cflags (optional) is 0 in every other case.  Returns
 * 0, or EINVAL for a null in or pkt. */
#define ESPGPU_NATT_CSUM_VALID 0x1
int  espgpu_esp_natt_cksum(const struct espgpu_insa *in, uint8_t *pkt, uint32_t len,
                           uint32_t trailer, uint32_t policy, uint8_t *out_cflags);
/* The same rule for a device-resident batch.  Packet i takes part if
 * d_status[i] == 0, d_dstatus[i] == 0, d_desc[i].sa < nin, that SA has
 * ESPGPU_IN_NATT and d_trailer[i] & 0xff is 6 or 17; it is the d_ipkt[i].len
 * bytes at d_out + d_ipkt[i].off4 * 4, as espgpu_esp_decap_batch left them.
 * d_cflags may be null; otherwise d_cflags[i] is written for every i < n.
 * Policy auto runs one lane per packet.  Recompute reads every byte of every
 * taking-part segment with a group of lanes per packet (16 unless set_tuning
 * "natt_lanes" says 8 or 32), aligned dword loads that each hold at least one
 * byte of the segment, and one dword store per packet: the field's, which on
 * the device may rewrite up to two bytes behind a TCP packet of 18 or 19
 * segment bytes with their own values (they are the record's padding).  d_out
 * is 4-byte aligned (EINVAL otherwise).  Asynchronous on the caller's stream,
 * no workspace, no host round trip; n == 0 is a no-op that returns 0. */
int  espgpu_esp_natt_cksum_batch(espgpu_ctx *ctx, uint8_t *d_out, const struct espgpu_pkt *d_ipkt,
                                 const struct espgpu_desc *d_desc, const uint32_t *d_trailer,
                                 const uint8_t *d_status, const uint8_t *d_dstatus, uint32_t n,
                                 const struct espgpu_insa *d_in, uint32_t nin, uint32_t policy,
                                 uint8_t *d_cflags, void *stream);

/* ---- inbound AH (ah_input, ah_massage_headers with out = 0 and ah_input_cb
 *      after the compare: freebsd/netipsec/xform_ah.c:144-169, :261-525,
 *      :576-600, :628-650, :758-814; then ipsec4/6_common_input_cb and
 *      key_sa_recordxfer as the decapsulation block states them) ----
 * IPv4 with options and IPv6 without extension headers (those packets stay
 * the host stack's: classification answers ENOTSUP for them).  The inbound AH
 * sequence on a device-resident batch, all on one stream:
 *   0. espgpu_esp_classify_batch with ESPGPU_CLS_AH
 *   1. espgpu_ah_input_batch         header-length checks, save, massage
 *   2. espgpu_replay_check_batch     windows with ESPGPU_REPLAY_AH
 *   3. espgpu_decrypt_batch_trailer  the digest kernel: ICV field read as zeros, compared
 *   4. espgpu_replay_update_batch
 *   5. espgpu_replay_merge four times, in this order: 1's result, 2's, 4's,
 *      0's.  A later merge overrides an earlier one: replay goes over 1's
 *      result, as ah_input checks replay first.  (A record that 1 refused has
 *      len 0 and takes no part in 2, so a replayed packet with bad options
 *      ends with 1's EINVAL where the reference answers EACCES: dropped
 *      either way, and without a window lookup.)
 *   6. espgpu_ah_decap_batch         restore, strip, mode, SA lifetime counters
 *   7. espgpu_replay_merge           with 6's result.
 * An ESP record in the same batch passes through 1 and 6 untouched with status
 * 0; an AH record passes through espgpu_esp_decap_batch with EINVAL.  The
 * per-SA state is struct espgpu_insa with ESPGPU_IN_AH (and the mode bits,
 * ESPGPU_IN_AF6, ESPGPU_IN_AH_KEEPTOS).
 *
 * Host: ah_input's checks and ah_massage_headers for one packet of `len` bytes
 * at `pkt` (the record a DIGEST descriptor names: len = desc.len, salt =
 * desc.salt), mlen the session's ICV length (a multiple of 4, 4..64; else
 * EINVAL).  With skip = salt - 12 the checks in order; the first that fires
 * decides, and a refused packet has nothing written, neither to pkt nor to
 * hsave (the reference zeroes a malformed option before it frees the packet):
 *   1. flags without ESPGPU_IN_AH, with ESPGPU_IN_PAD_RAND or ESPGPU_IN_NATT,
 *      with unknown bits, or with both mode bits                     EINVAL
 *      salt < 32, or skip & 3                                        EINVAL
 *      AF_INET: version nibble not 4 or ip_hl * 4 != skip            EINVAL
 *      AF6: version nibble not 6 or skip != 40                       EINVAL
 *      len < skip + 12                                               EINVAL
 *   2. ahsize = roundup(12 + mlen, AF6 ? 8 : 4) (ah_hdrsiz, :144-169)
 *      8 + ah_len * 4 != ahsize (:581)                               EACCES
 *      skip + ahsize > len (:591)                                    EACCES
 *   3. IPv4 (:291-393): ip_tos (unless ESPGPU_IN_AH_KEEPTOS), ip_ttl, ip_sum
 *      and ip_off are zeroed, then the option loop from byte 20 to skip:
 *      an option other than EOL or NOP at off + 1 >= skip (:303-312) EINVAL
 *      EOL ends the loop, NOP is one byte
 *      an option length < 2 (:329, :344, :370)                       EINVAL
 *      options 0x82, 0x85, 0x86, 0x94 and 0x95 are kept, every other option
 *        is zeroed, type and length bytes too (:378-381)
 *      an option running past skip (:386)                            EINVAL
 *      IPv6 (:401-422): ip6_plen == 0                                EMSGSIZE
 *      ip6_flow = 0 with the version kept, ip6_hlim = 0; s6_addr16[1] of a
 *      link-local (fe80::/10) source or destination zeroed
 *   4. hsave[0, skip) receives the first skip bytes as they arrived (the
 *      front of xform_data, :632); hsave[skip, 64) is not written.  The
 *      massaged header goes over the packet's.  Every header byte is loaded
 *      before any is stored.  The ICV stays where it is: the digest kernel
 *      reads the field as zeros and compares (:635, :745-749).
 * The AH header itself and everything behind it is never written.  Null
 * pointers are EINVAL. */
int  espgpu_ah_input(const struct espgpu_insa *in, uint32_t mlen, uint8_t *pkt, uint32_t len,
                     uint32_t salt, uint8_t *hsave);
/* The same rule for a device-resident batch, between the classification and
 * the replay check.  Record i takes part if d_desc[i].len != 0, d_desc[i].sa <
 * nin and the ctx holds a DIGEST session with that id; mlen is that session's,
 * the packet the d_desc[i].len bytes at d_arena + d_desc[i].off4 * 4 and its
 * save slot d_hsave + i * 64.  d_astatus[i] is the rule's status.  A refused
 * record also gets d_desc[i].len = 0, so the later stages pass over it.  Any
 * other record (an ESP session's, a refused one of an earlier stage) gets
 * d_astatus[i] = 0 and nothing else written.  d_arena and d_hsave are 4-byte
 * aligned (EINVAL otherwise); d_hsave holds n * 64 bytes.  One lane per
 * packet; a wave none of whose packets has IPv4 options does not run the
 * option loop.  Asynchronous on the caller's stream, no workspace, no host
 * round trip; n == 0 is a no-op that returns 0. */
int  espgpu_ah_input_batch(espgpu_ctx *ctx, uint8_t *d_arena, struct espgpu_desc *d_desc, uint32_t n,
                           const struct espgpu_insa *d_in, uint32_t nin, uint8_t *d_hsave,
                           uint8_t *d_astatus, void *stream);
/* Host: ah_input_cb after the compare and the window update, for one packet
 * that espgpu_ah_input accepted and whose ICV verified: pkt, len, salt and
 * mlen as there, hsave the slot it filled.  nxt = pkt[skip] (ah_nxt; the AH
 * header was never massaged), q = len - skip - ahsize.  The checks in order;
 * a refused packet has nothing written, books nothing and gets *out_off =
 * *out_len = 0:
 *   1. the flag, skip and length rows of espgpu_ah_input's check 1 (the
 *      version row is 3's), and len < skip + ahsize                  EINVAL
 *   2. tunnel, transport or EPFNOSUPPORT, q < 20 / q < 40: steps 2 and 3 of
 *      espgpu_esp_decap, with this nxt and q.
 *   3. transport: the saved header, with its protocol field (byte 9; IPv6:
 *      byte 6) set to nxt (:759), goes to pkt + ahsize (:762, m_striphdr :791);
 *      ip_len = skip + q with ip_sum recomputed, or ip6_plen = q, exactly as
 *      step 5 of espgpu_esp_decap; a saved header whose version / ip_hl do not
 *      agree with skip is EINVAL.  The result is {ahsize, skip + q} and the SA
 *      books as many bytes.
 *      tunnel: the packet is not touched.  The result is {skip + ahsize, q}
 *      and the SA books q bytes.
 *   4. accepted: in->bytes += booked, in->packets += 1.
 * A packet that does not come through both functions and the compare with
 * status 0 is a dropped packet: its first skip bytes in the arena stay
 * massaged, and the original header remains in hsave. */
int  espgpu_ah_decap(struct espgpu_insa *in, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t salt,
                     const uint8_t *hsave, uint32_t *out_off, uint32_t *out_len);
/* The same rule for a device-resident batch, in place (the digest writes no
 * d_out), after the merges of step 5.  Record i takes part if d_status[i] ==
 * 0, d_desc[i].sa < nin, the ctx holds a DIGEST session with that id and the
 * SA has ESPGPU_IN_AH.  d_dstatus[i] is the rule's status and d_ipkt[i] =
 * {d_desc[i].off4 + out_off / 4, out_len}: absolute, in the form
 * espgpu_esp_classify_batch takes, so AH transport around ESP goes straight
 * back into classification.  A record with d_status[i] != 0 gets d_dstatus[i]
 * = 0 and d_ipkt[i] = {d_desc[i].off4, 0}.  A record with status 0 of an ESP
 * session the ctx holds gets d_dstatus[i] = 0 and its d_ipkt[i] is not
 * written (espgpu_esp_decap_batch's result may stand there); any other record
 * with status 0 gets EINVAL and the empty d_ipkt[i].  The counters are summed
 * as espgpu_esp_decap_batch's.  d_arena and d_hsave are 4-byte aligned (EINVAL
 * otherwise).  Asynchronous on the caller's stream, no workspace, no host
 * round trip; n == 0 is a no-op that returns 0. */
int  espgpu_ah_decap_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_desc *d_desc,
                           const uint8_t *d_status, uint32_t n, struct espgpu_insa *d_in, uint32_t nin,
                           const uint8_t *d_hsave, struct espgpu_pkt *d_ipkt, uint8_t *d_dstatus,
                           void *stream);

/* ---- outbound AH (ah_output and ah_output_cb, freebsd/netipsec/xform_ah.c:
 *      833-1065, :1070-1123, with ah_massage_headers, out = 1, :291-422; around
 *      them ipsec4/6_perform_request's mode decision, ipsec_encap,
 *      ipsec_process_done's length fields and key_sa_recordxfer as the
 *      encapsulation block states them) ----
 * From cleartext IP packets in the arena to authenticated wire packets.  The
 * outbound AH sequence on a device-resident batch, all on one stream, no host
 * round trip:
 *   1. espgpu_ah_encap_batch   mode, outer header, header move, AH header,
 *                              save, massage (out = 1); builds d_desc and d_opkt
 *   2. espgpu_ah_frame_batch   SPI and ah_seq in arrival order per SA, esn_hi;
 *                              the wrap check
 *   3. espgpu_encrypt_batch    the digest kernel writes the ICV (unchanged)
 *   4. espgpu_replay_merge     with 2's result, then with 1's
 *   5. espgpu_ah_sent_batch    ah_output_cb's m_copyback of the saved header;
 *                              key_sa_recordxfer
 * d_opkt is then the list of wire packets, in the form
 * espgpu_esp_classify_batch takes.  espgpu_esp_encap_batch's d_opkt (after its
 * own sequence) can be step 1's d_pkt: an ESP-then-AH bundle.  The per-SA state
 * is struct espgpu_encsa with ESPGPU_ENC_AH (policy, addresses, ttl, lifetime
 * counters) and, of struct espgpu_outsa, count, spi and flags; both are indexed
 * by the session id.  IPv4 with options and IPv6 without extension headers, as
 * inbound.
 *
 * Deliberate differences from the reference:
 *   - An LSRR / SSRR option of length 2 or 3 is EINVAL.  The reference would
 *     assemble the "last address" (:362-365) from bytes in front of the option,
 *     as its loop has left them; no receiver can verify such a packet, and
 *     refusing it keeps the walk free of reads of bytes it has changed.
 *   - The lengths in the hashed header come from `len`: ip_len = total,
 *     ip6_plen = total - 40.  The reference adds ahsize to the field as it
 *     stands (:1001, :1012); the two agree whenever the packet's own length
 *     field is right.
 *   - The saved header is in its final wire form, ip_len and ip_sum included;
 *     the reference leaves these to ipsec_process_done and ip_output, as the
 *     encapsulation block notes.
 *   - len > 65535 is EMSGSIZE and fe80::/10 SA addresses are ENOTSUP, as for
 *     espgpu_esp_encap.
 *   - SAs without a replay structure are not modelled (the reference leaves
 *     ah_seq unwritten for them, :939).
 *   - A packet the option loop refuses consumes no sequence number: the
 *     massage is step 1 and the numbers are step 2.  (The reference has
 *     counted by then, :956, :1027; a gap is nothing a receiver can see.)
 *
 * Host, step 1: encapsulate one cleartext packet of `len` bytes at `pkt` for
 * the AH SA `e`; mlen is the session's ICV length, `headroom` the bytes before
 * pkt that may be written, `ip_id` the value an outer IPv4 header gets, hsave
 * a 64-byte save slot.  The checks in order; the first that fires decides, and
 * a refused packet has nothing written, neither to the packet nor to the slot,
 * and zeros in the three results:
 *   1. flags with unknown bits, both DF bits or both ECN bits          EINVAL
 *      ESPGPU_ENC_AH missing                                           EINVAL
 *      ESPGPU_ENC_NATT set (the reference ignores NAT-T for SAs that
 *      are not ESP's, key.c:5702)                                      EINVAL
 *      mlen not a multiple of 4 in 4..64                               EINVAL
 *      an AF6 SA whose src or dst is unspecified                       EINVAL
 *      an AF6 SA whose src or dst is in fe80::/10                      ENOTSUP
 *   2. the packet rows of espgpu_esp_encap's check 2; skip = ip_hl * 4, or 40
 *      for IPv6, extension headers or not (ipsec_output.c:574-581).
 *   3. tunnel or transport exactly as espgpu_esp_encap's check 3.
 *   4. ahsize = roundup(12 + mlen, AF6 SA ? 8 : 4) (ah_hdrsiz); oh = 0, 20 or
 *      40; total = len + ahsize + oh.
 *      total > 65535 (xform_ah.c:882)                                  EMSGSIZE
 *      ahsize + oh > headroom (m_makespace, :907)                      ENOBUFS
 *   5. tunnel: the inner header is fixed as espgpu_esp_encap's step 5 and the
 *      outer header built as there, with protocol 51, at pkt - ahsize - oh;
 *      ah_nxt is 4 or 41.
 *   6. transport: the skip header bytes move to pkt - ahsize, every dword
 *      loaded before any is stored; ip_len = total, ip_p = 51 and ip_sum
 *      recomputed, or ip6_plen = total - 40 and ip6_nxt = 51; ah_nxt is the
 *      old protocol.
 *   7. the AH header stands behind that IP header of hs bytes (oh in tunnel
 *      mode, skip in transport mode): dword 0 is ah_nxt, ah_len = (ahsize - 8)
 *      / 4, reserve 0 (:925-927).  The SPI and the sequence number are step
 *      2's.  The zero padding behind the ICV field is written (:934; it is
 *      hashed); the ICV field itself is not: the digest kernel reads it as
 *      zeros and then writes it.
 *   8. hsave[0, hs) receives the IP header in its final wire form, as 5 or 6
 *      built it: what ah_output_cb copies back.  The packet receives that
 *      header massaged as ah_massage_headers(out = 1) does: ip_tos (unless
 *      ESPGPU_ENC_AH_KEEPTOS), ip_ttl, ip_sum and ip_off zeroed, then the
 *      option loop with the kept and zeroed options and the refusals of
 *      espgpu_ah_input's check 3.  For LSRR / SSRR (0x83, 0x89) the hashed
 *      ip_dst becomes the option's last four bytes (:362-365), then the option
 *      is zeroed; of several such options the last one wins.  IPv6: ip6_flow
 *      = 0 with the version kept, ip6_hlim = 0, s6_addr16[1] of a link-local
 *      address zeroed.  A refusal of the option loop is EINVAL and precedes
 *      every write of 5-8.
 *   9. *out_front = ahsize + oh: the wire packet is {pkt - *out_front,
 *      *out_total = total}; *out_salt = hs + 12, the ICV's offset in it.
 * Null pointers are EINVAL. */
int  espgpu_ah_encap(const struct espgpu_encsa *e, uint32_t mlen, uint8_t *pkt, uint32_t len,
                     uint32_t headroom, uint16_t ip_id, uint8_t *hsave, uint32_t *out_front,
                     uint32_t *out_total, uint32_t *out_salt);
/* The same rule for n packets of a device-resident arena.  d_pkt[i] is the
 * cleartext packet and d_sa[i] the SA the caller's SPD lookup chose for it;
 * d_enc[nenc] is indexed by the session id.  Packet i takes part if d_sa[i] <
 * nenc and the ctx holds a DIGEST session with that id; mlen is that session's,
 * the ip_id (uint16_t)(id0 + i) and the save slot d_hsave + i * 64.  headroom
 * holds for every packet; the caller guarantees that the spans [pkt - headroom,
 * pkt + len) of one batch lie in the arena and do not overlap.  An accepted
 * packet gets d_desc[i] = {wire off4, total, sa, 0, hs + 12}, the DIGEST record
 * of the batch path, d_opkt[i] = {wire off4, total} and d_estatus[i] = 0.  A
 * refused packet gets its status, one that takes no part (an ESP session's
 * d_sa, a free slot's) EINVAL, and both d_desc[i] = {d_pkt[i].off4, 0, 0xffff,
 * 0, 0} and d_opkt[i] = {d_pkt[i].off4, 0}.  d_arena and d_hsave are 4-byte
 * aligned (EINVAL otherwise); d_hsave holds n * 64 bytes.  One lane per
 * packet; a wave none of whose packets has IPv4 options does not run the
 * option loop.  Asynchronous on the caller's stream, no workspace, no host
 * round trip; n == 0 is a no-op that returns 0. */
int  espgpu_ah_encap_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_pkt *d_pkt,
                           const uint16_t *d_sa, uint32_t n, const struct espgpu_encsa *d_enc,
                           uint32_t nenc, uint32_t headroom, uint32_t id0, uint8_t *d_hsave,
                           struct espgpu_desc *d_desc, struct espgpu_pkt *d_opkt, uint8_t *d_estatus,
                           void *stream);
/* Host, step 2: ah_output's SPI and sequence number (:928, :937-958, :1045-
 * 1048) for the wire packet of `len` bytes at `pkt` whose ICV field is at
 * `salt`.  len == 0, salt < 12, salt > len or salt % 4 != 0 is EINVAL.  With
 * room = what the SA may still give out from o->count (ah_output always
 * checks, whatever ESPGPU_OUT_WRAPCHECK says, unless ESPGPU_OUT_CYCSEQ is
 * set): room == 0 is EACCES (:949) with nothing touched.  Otherwise o->count++,
 * the SPI goes big-endian to salt - 8 and (uint32_t)count to salt - 4, and
 * *esn_hi = count >> 32 for ESPGPU_OUT_ESN, else 0.  o->cntr, o->salt, the pad
 * bits and ESPGPU_OUT_CTRCOMPAT mean nothing here and are neither read nor
 * written.  Null pointers are EINVAL. */
int  espgpu_ah_frame(struct espgpu_outsa *o, uint8_t *pkt, uint32_t len, uint32_t salt,
                     uint32_t *esn_hi);
/* The same rule for a batch, as espgpu_esp_frame_batch: record i takes part if
 * d_desc[i].len != 0, d_desc[i].sa < nout, the ctx holds a DIGEST session with
 * that id, 12 <= d_desc[i].salt <= d_desc[i].len and salt % 4 == 0.  The result
 * is the host rule applied to each SA's taking-part records in index order,
 * starting from d_out[sa] as it stands; d_desc[i].esn_hi is written and
 * d_desc[i].salt keeps the ICV offset.  A record refused by the wrap gets
 * EACCES and d_desc[i].len = 0, and so does the rest of its SA's batch; a
 * record that takes no part gets EINVAL and d_desc[i].len = 0.  Entries of
 * SAs with no accepted record are untouched.  The ctx's stage workspace is
 * shared with espgpu_esp_frame_batch and espgpu_replay_update_batch: ENOMEM
 * with nothing launched if it cannot grow.  d_arena is 4-byte aligned (EINVAL
 * otherwise).  n == 0 is a no-op that returns 0. */
int  espgpu_ah_frame_batch(espgpu_ctx *ctx, uint8_t *d_arena, struct espgpu_desc *d_desc, uint32_t n,
                           struct espgpu_outsa *d_out, uint32_t nout, uint8_t *d_fstatus,
                           void *stream);
/* Host, step 5: ah_output_cb's m_copyback (:1120) and key_sa_recordxfer
 * (ipsec_output.c:770) for one wire packet that went through with status
 * `status`: pkt, len and salt as espgpu_ah_encap left them, hsave the slot it
 * filled.  A nonzero status, or an SA without ESPGPU_ENC_AH, writes nothing,
 * books nothing and returns 0.  Otherwise hsave[0, salt - 12) goes back over
 * the packet's first bytes and *e books len bytes and one packet.  salt - 12
 * not a multiple of 4 in 20..60 (not 40 for an AF6 SA), salt > len, or a slot
 * whose version nibble does not agree with the SA's family is EINVAL, written
 * nowhere and booked nowhere.  A dropped packet (one that does not come
 * through the sequence with status 0) keeps its massaged header in the arena,
 * and its wire header stays in the slot. */
int  espgpu_ah_sent(struct espgpu_encsa *e, uint8_t status, uint8_t *pkt, uint32_t len, uint32_t salt,
                    const uint8_t *hsave);
/* The same rule for a batch, after the merges.  Record i qualifies if
 * d_status[i] == 0, d_desc[i].sa < nenc, the ctx holds a DIGEST session with
 * that id and the SA has ESPGPU_ENC_AH; its packet is the d_opkt[i].len bytes
 * at d_arena + d_opkt[i].off4 * 4, its salt d_desc[i].salt and its slot
 * d_hsave + i * 64.  d_sstatus[i] is the rule's status, 0 for every record that
 * does not qualify (those write nothing and book nothing).  The counters are
 * summed per wave, and per workgroup where one SA has all of it, before the
 * 64-bit adds, as espgpu_esp_sent_batch's.  d_arena and d_hsave are 4-byte
 * aligned (EINVAL otherwise).  Asynchronous on the caller's stream, no
 * workspace; n == 0 is a no-op that returns 0. */
int  espgpu_ah_sent_batch(espgpu_ctx *ctx, uint8_t *d_arena, const struct espgpu_pkt *d_opkt,
                          const struct espgpu_desc *d_desc, const uint8_t *d_status, uint32_t n,
                          struct espgpu_encsa *d_enc, uint32_t nenc, const uint8_t *d_hsave,
                          uint8_t *d_sstatus, void *stream);

/* Device time of the last timed batch's crypto kernels (ms, from HIP events
 * on the batch stream).  Process-path batches of <= 128 KiB (a burst on its
 * slot's own stream) are not timed: the two event markers cost a 32-record
 * burst 8 us of its 65. */
float espgpu_last_kernel_ms(espgpu_ctx *ctx);

/* Tuning knobs (engine-internal, for A/B measurement):
 *   "grid"      workgroups per launch (0 = 256, one per CU);
 *   "gcm_lanes" GCM lanes per record: 0 (default) 8 below 32768 records,
 *               else 4; 4 or 8 forces one kernel; others EINVAL;
 *   "overflow_mb" host overflow for process() while every staging slot is
 *               in flight, in MiB (0, the default: ERESTART; 0..4095; only
 *               requests not yet moved into a slot count against it);
 *   "xfer"      small batches' staging region moved by the xfer kernel (1,
 *               default) or by hipMemcpyAsync (0);
 *   "natt_lanes" lanes per packet of espgpu_esp_natt_cksum_batch's recompute
 *               kernel: 0 (default: 16), 8, 16 or 32; others EINVAL;
 *   "gcm_burst" GCM batches of up to this many records (default 4096) that
 *               run the small-batch design, out of place or encrypt, use the
 *               burst kernel (a 32-lane CTR pass and an 8-lane GHASH in one
 *               launch, for latency); 0 = the fused small-batch kernel;
 *   "door"      doorbell path (0, the default: off): N > 0 keeps a
 *               persistent kernel of N workgroups (one per CU) resident that
 *               serves the process path's single-session GCM batches of up
 *               to gcm_burst records -- flush() publishes a 16-byte job in
 *               pinned host memory instead of launching, the kernel stages
 *               the records in and the results out through the mapping, and
 *               poll() reads its done word -- so a burst pays no launch or
 *               completion signal; other kernels of the ctx then use the
 *               remaining CUs; 1..256, others EINVAL; changing it drains;
 *   "door_idle_us" the doorbell kernel exits after this long without a
 *               job (default 20000; 100..10^7): flush / poll relaunch it;
 *   "stage_fused" a process-path burst of one GCM session stages its own
 *               records inside the crypto kernel (1, default: one launch per
 *               burst) instead of xfer kernels around it (0);
 *   "deadline_ms" a batch outstanding this long (launch to completion) is a
 *               GPU failure (espgpu_health); 1..600000, default 2000;
 *   "fault"     fault injection for the GPU-failure path's tests: a mask of
 *               ESPGPU_FAULT_LAUNCH (the next launch fails), _QUERY (the next
 *               completion query of an in-flight batch returns an error) and
 *               _STUCK (the next batch launched is never seen to complete, so
 *               it meets the deadline); each bit is consumed once;
 *   "ah_offer"  whether espgpu_probesession bids for AH (CSP_MODE_DIGEST)
 *               sessions: 1 / 0, or -1 (the default) to let FF_GPUCRYPTO_AH in
 *               the environment decide; process-wide, `ctx` may be NULL;
 *   "gcm_opts" / "eta_opts" measurement knobs that skip work on purpose
 *               (results wrong): only in libespgpu_knobs.so, ENOTSUP in the
 *               product library unless 0.
 * (The keys of designs measured slower and removed -- "gcm_split", "gcm_bs",
 * "eta_fused", "eta_ws", "eta_lag" -- are unknown: ENOENT.)
 * Returns 0, EINVAL, ENOTSUP or ENOENT (unknown key). */
#define ESPGPU_FAULT_LAUNCH 0x1
#define ESPGPU_FAULT_QUERY  0x2
#define ESPGPU_FAULT_STUCK  0x4
int  espgpu_set_tuning(espgpu_ctx *ctx, const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif /* ESPGPU_H */
