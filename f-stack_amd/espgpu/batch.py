"""Device-resident batch path (espgpu_decrypt_batch / espgpu_encrypt_batch).

Records live in a torch.uint8 CUDA tensor (the arena, HBM), one 16-byte
espgpu_desc per record in a second tensor.  torch is plumbing here: device
memory and streams.  All crypto runs in libespgpu.so's HIP kernels.
"""
import numpy as np

from . import _lib as L

DESC_DTYPE = np.dtype([("off4", "<u4"), ("len", "<u2"), ("sa", "<u2"),
                       ("esn_hi", "<u4"), ("salt", "<u4")])
assert DESC_DTYPE.itemsize == 16


def descs_to_tensor(descs, device):
    """numpy structured DESC_DTYPE array -> uint8 CUDA tensor (n*16 bytes)."""
    import torch
    raw = np.ascontiguousarray(descs).view(np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


def _stream_ptr(stream):
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def decrypt_batch(driver, arena, desc, n, status, out=None, grouped=False, stream=None,
                  trailer=None):
    """Verify+decrypt n records.  out=None -> in place (verify-first two-pass).
    trailer: optional int32/uint32 CUDA tensor of n words receiving the fused
    esp_input_cb trailer checks (espgpu_decrypt_batch_trailer; see
    esp.trailer_word for the bit layout)."""
    for t in (arena, desc, status) + tuple(x for x in (out, trailer) if x is not None):
        assert t.is_cuda and t.is_contiguous()
    outp = out.data_ptr() if out is not None else None
    flags = L.BATCH_GROUPED if grouped else 0
    if trailer is not None:
        assert trailer.numel() >= n and trailer.element_size() == 4
        rc = driver.lib.espgpu_decrypt_batch_trailer(
            driver.ctx, arena.data_ptr(), desc.data_ptr(), n, status.data_ptr(), outp,
            trailer.data_ptr(), flags, _stream_ptr(stream))
    else:
        rc = driver.lib.espgpu_decrypt_batch(
            driver.ctx, arena.data_ptr(), desc.data_ptr(), n, status.data_ptr(), outp, flags,
            _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_decrypt_batch: %s" % driver.last_error())


def decrypt_batch_packed(driver, arena, desc, n, status, out, stride, grouped=False, stream=None):
    """Verify+decrypt n GCM records, record i's plaintext to out[i*stride:]
    (espgpu_decrypt_batch_packed: stride a multiple of 128, out of place)."""
    for t in (arena, desc, status, out):
        assert t.is_cuda and t.is_contiguous()
    assert out.numel() >= n * stride
    rc = driver.lib.espgpu_decrypt_batch_packed(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, status.data_ptr(), out.data_ptr(), stride,
        L.BATCH_GROUPED if grouped else 0, _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_decrypt_batch_packed: %s (%d)" % (driver.last_error(), rc))


def encrypt_batch(driver, arena, desc, n, status, grouped=False, stream=None):
    for t in (arena, desc, status):
        assert t.is_cuda and t.is_contiguous()
    rc = driver.lib.espgpu_encrypt_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, status.data_ptr(),
        L.BATCH_GROUPED if grouped else 0, _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_encrypt_batch: %s" % driver.last_error())


def decrypt_host(driver, arena, desc, n, status, out, chunk=0, flags=0):
    """Host-to-host pipelined decrypt (espgpu_decrypt_host): arena/desc/status/out
    are pinned CPU tensors (torch .pin_memory()); the engine streams chunks
    through HBM with H2D, kernels and D2H overlapped on three HIP streams."""
    for t in (arena, desc, status, out):
        assert not t.is_cuda and t.is_contiguous() and t.is_pinned()
    rc = driver.lib.espgpu_decrypt_host(
        driver.ctx, arena.data_ptr(), arena.numel(), desc.data_ptr(), n, status.data_ptr(),
        out.data_ptr(), chunk, flags)
    if rc:
        raise RuntimeError("espgpu_decrypt_host: %s" % driver.last_error())


REPLAY_DTYPE = np.dtype([("last", "<u8"), ("wsize", "<u4"), ("bitmap_size", "<u4"),
                         ("bitmap_off", "<u4"), ("flags", "<u4")])
assert REPLAY_DTYPE.itemsize == 24


def replay_check(driver, arena, desc, n, replay, bitmap, rstatus, stream=None):
    """Replay pre-filter (espgpu_replay_check_batch): replay is a uint8 CUDA
    tensor of REPLAY_DTYPE records indexed by session id, bitmap an int32 CUDA
    tensor of window words; rstatus receives 0 / EACCES per record, and desc
    is updated in place (len 0 for replayed records, esn_hi for ESN SAs)."""
    for t in (arena, desc, replay, bitmap, rstatus):
        assert t.is_cuda and t.is_contiguous()
    nrep = replay.numel() // REPLAY_DTYPE.itemsize
    rc = driver.lib.espgpu_replay_check_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, replay.data_ptr(), nrep,
        bitmap.data_ptr(), rstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_replay_check_batch: %s" % driver.last_error())


def replay_update(driver, arena, desc, n, status, replay, bitmap, ustatus, stream=None):
    """Window update after decrypt (espgpu_replay_update_batch): the records
    with status 0 update their SA's window in replay / bitmap (both stay on the
    device for the next batch) as espgpu_replay_update64 would one by one in
    index order; ustatus receives 0 / EACCES (EINVAL for an unusable window)
    per record, for replay_merge."""
    for t in (arena, desc, status, replay, bitmap, ustatus):
        assert t.is_cuda and t.is_contiguous()
    nrep = replay.numel() // REPLAY_DTYPE.itemsize
    rc = driver.lib.espgpu_replay_update_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, status.data_ptr(), replay.data_ptr(), nrep,
        bitmap.data_ptr(), ustatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_replay_update_batch: %s (%d)" % (driver.last_error(), rc))


OUTSA_DTYPE = np.dtype([("count", "<u8"), ("cntr", "<u8"), ("spi", "<u4"), ("salt", "<u4"),
                        ("flags", "<u4"), ("pad_", "<u4")])
assert OUTSA_DTYPE.itemsize == 32


def esp_frame(driver, arena, desc, frame, n, outsa, fstatus, stream=None):
    """Outbound framing before encrypt_batch (espgpu_esp_frame_batch): outsa
    is a uint8 CUDA tensor of OUTSA_DTYPE records indexed by session id (it
    stays on the device for the next batch), frame an int32 CUDA tensor of n
    words, rlen | next header << 16.  Each SA's records get their sequence
    numbers and counter IVs in index order, the padding and the trailer; desc
    is updated in place (esn_hi, salt; len 0 for refused records) and fstatus
    receives 0 / EINVAL per record, for replay_merge after the encrypt."""
    for t in (arena, desc, frame, outsa, fstatus):
        assert t.is_cuda and t.is_contiguous()
    assert frame.element_size() == 4 and frame.numel() >= n
    nout = outsa.numel() // OUTSA_DTYPE.itemsize
    rc = driver.lib.espgpu_esp_frame_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), frame.data_ptr(), n, outsa.data_ptr(), nout,
        fstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_frame_batch: %s (%d)" % (driver.last_error(), rc))


PKT_DTYPE = np.dtype([("off4", "<u4"), ("len", "<u4")])
SAD_DTYPE = np.dtype([("spi", "<u4"), ("sa", "<u2"), ("proto", "u1"), ("af", "u1"), ("salt", "<u4"),
                      ("flags", "<u4"), ("dst", "u1", (16,))])
assert PKT_DTYPE.itemsize == 8 and SAD_DTYPE.itemsize == 32


def sad_build(sas, nslots):
    """The SPI table of espgpu_sad_build for a SAD_DTYPE array of SAs: a
    SAD_DTYPE array of nslots slots, to be uploaded for esp_classify.
    ValueError where the C function answers EINVAL."""
    sas = np.ascontiguousarray(sas, dtype=SAD_DTYPE)
    table = np.zeros(max(int(nslots), 1), dtype=SAD_DTYPE)
    rc = L.lib().espgpu_sad_build(sas.ctypes.data, len(sas), table.ctypes.data, nslots)
    if rc:
        raise ValueError("espgpu_sad_build: %d" % rc)
    return table[:nslots]


def esp_classify(driver, arena, pkt, n, table, desc, cstatus, flags=0, stream=None):
    """Inbound classification before replay_check (espgpu_esp_classify_batch):
    pkt is a uint8 CUDA tensor of PKT_DTYPE records (where each received
    packet's IP header starts and how many bytes it has), table the uploaded
    result of sad_build.  desc receives one descriptor per packet, for the
    rest of the inbound sequence, and cstatus 0 / EINVAL / ENOTSUP / ENOENT,
    for replay_merge at its end; a refused packet's descriptor has len 0 and
    sa 0xffff.  flags: L.CLS_IPCSUM, L.CLS_NATT_PORT(port) to take ESP in UDP
    to that port, L.CLS_AH to take AH packets (their descriptor is the whole
    packet, with the ICV field's offset as its salt)."""
    for t in (arena, pkt, table, desc, cstatus):
        assert t.is_cuda and t.is_contiguous()
    assert pkt.numel() >= n * PKT_DTYPE.itemsize and desc.numel() * desc.element_size() >= n * 16
    nslots = table.numel() * table.element_size() // SAD_DTYPE.itemsize
    rc = driver.lib.espgpu_esp_classify_batch(
        driver.ctx, arena.data_ptr(), pkt.data_ptr(), n, table.data_ptr(), nslots, flags,
        desc.data_ptr(), cstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_classify_batch: %s (%d)" % (driver.last_error(), rc))


INSA_DTYPE = L.INSA_DTYPE
assert INSA_DTYPE.itemsize == 24


def esp_decap(driver, arena, out, pkt, desc, trailer, status, n, insa, ipkt, dstatus, stream=None):
    """Inbound decapsulation, the last step before the final replay_merge
    (espgpu_esp_decap_batch): pkt and desc as esp_classify took and gave them,
    trailer and status as decrypt_batch and the merges left them, insa a uint8
    CUDA tensor of INSA_DTYPE records indexed by session id (it stays on the
    device for the next batch).  A transport record's outer header is read
    from arena and written, fixed, into out just before the plaintext (out
    may be arena); a tunnel record's packet is not touched.  ipkt receives one
    PKT_DTYPE record per packet, where the resulting packet starts and its
    length (length 0 for a record that is refused or took no part), dstatus 0
    / EINVAL / ENODATA / EPFNOSUPPORT for replay_merge, and every SA's bytes
    and packets grow by what was accepted."""
    for t in (arena, out, pkt, desc, trailer, status, insa, ipkt, dstatus):
        assert t.is_cuda and t.is_contiguous()
    assert trailer.element_size() == 4 and trailer.numel() >= n
    assert pkt.numel() >= n * PKT_DTYPE.itemsize and ipkt.numel() * ipkt.element_size() >= n * PKT_DTYPE.itemsize
    nin = insa.numel() * insa.element_size() // INSA_DTYPE.itemsize
    rc = driver.lib.espgpu_esp_decap_batch(
        driver.ctx, arena.data_ptr(), out.data_ptr(), pkt.data_ptr(), desc.data_ptr(), trailer.data_ptr(),
        status.data_ptr(), n, insa.data_ptr(), nin, ipkt.data_ptr(), dstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_decap_batch: %s (%d)" % (driver.last_error(), rc))


def ah_input(driver, arena, desc, n, insa, hsave, astatus, stream=None):
    """ah_input's header-length checks and ah_massage_headers between
    esp_classify (with L.CLS_AH) and replay_check (espgpu_ah_input_batch):
    desc as esp_classify gave it, insa the INSA_DTYPE tensor whose AH SAs carry
    L.IN_AH, hsave a uint8 CUDA tensor of n * L.AH_SAVE_SLOT bytes.  Every
    record of a DIGEST session has its IP header saved into its slot and
    massaged in the arena, or is refused: astatus receives 0 / EINVAL / EACCES
    / EMSGSIZE per record for replay_merge, and a refused record's descriptor
    gets len 0.  Records of other sessions are passed over with status 0."""
    for t in (arena, desc, insa, hsave, astatus):
        assert t.is_cuda and t.is_contiguous()
    assert desc.numel() * desc.element_size() >= n * 16 and astatus.numel() >= n
    assert hsave.element_size() == 1 and hsave.numel() >= n * L.AH_SAVE_SLOT
    nin = insa.numel() * insa.element_size() // INSA_DTYPE.itemsize
    rc = driver.lib.espgpu_ah_input_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, insa.data_ptr(), nin, hsave.data_ptr(),
        astatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_ah_input_batch: %s (%d)" % (driver.last_error(), rc))


def ah_decap(driver, arena, desc, status, n, insa, hsave, ipkt, dstatus, stream=None):
    """ah_input_cb's restore and strip with ipsec4/6_common_input_cb, the last
    step of the inbound AH sequence before the final replay_merge
    (espgpu_ah_decap_batch), in place: desc and hsave as ah_input left them,
    status as decrypt_batch and the merges left it.  A transport record's
    saved header is written, fixed, just before the payload; a tunnel record's
    packet is not touched.  ipkt receives one PKT_DTYPE record per AH packet,
    absolute as esp_classify takes it (length 0 for a refused or failed
    record; an ESP record's entry is not written), dstatus 0 / EINVAL /
    EPFNOSUPPORT for replay_merge, and every SA's bytes and packets grow by
    what was accepted."""
    for t in (arena, desc, status, insa, hsave, ipkt, dstatus):
        assert t.is_cuda and t.is_contiguous()
    assert desc.numel() * desc.element_size() >= n * 16 and status.numel() >= n and dstatus.numel() >= n
    assert hsave.element_size() == 1 and hsave.numel() >= n * L.AH_SAVE_SLOT
    assert ipkt.numel() * ipkt.element_size() >= n * PKT_DTYPE.itemsize
    nin = insa.numel() * insa.element_size() // INSA_DTYPE.itemsize
    rc = driver.lib.espgpu_ah_decap_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), status.data_ptr(), n, insa.data_ptr(), nin,
        hsave.data_ptr(), ipkt.data_ptr(), dstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_ah_decap_batch: %s (%d)" % (driver.last_error(), rc))


def esp_natt_cksum(driver, out, ipkt, desc, trailer, status, dstatus, n, insa, policy=0, cflags=None, stream=None):
    """The NAT-T checksum fix after esp_decap (espgpu_esp_natt_cksum_batch):
    out, ipkt, desc, trailer, status and dstatus as esp_decap took and left
    them (before the final replay_merge, or after it with status given for
    both), insa its INSA_DTYPE tensor, whose pad_ field holds natt->cksum for
    the SAs with L.IN_NATT.  policy 0 adjusts the TCP / UDP checksum of every
    decapsulated transport packet of such an SA by that value, nonzero
    recomputes it over the segment.  cflags, if given, receives one byte per
    packet: L.NATT_CSUM_VALID where the stack is to take the TCP checksum as
    verified, else 0."""
    for t in (out, ipkt, desc, trailer, status, dstatus, insa) + ((cflags,) if cflags is not None else ()):
        assert t.is_cuda and t.is_contiguous()
    assert trailer.element_size() == 4 and trailer.numel() >= n
    assert ipkt.numel() * ipkt.element_size() >= n * PKT_DTYPE.itemsize
    assert desc.numel() * desc.element_size() >= n * 16 and status.numel() >= n and dstatus.numel() >= n
    assert cflags is None or (cflags.element_size() == 1 and cflags.numel() >= n)
    nin = insa.numel() * insa.element_size() // INSA_DTYPE.itemsize
    rc = driver.lib.espgpu_esp_natt_cksum_batch(
        driver.ctx, out.data_ptr(), ipkt.data_ptr(), desc.data_ptr(), trailer.data_ptr(), status.data_ptr(),
        dstatus.data_ptr(), n, insa.data_ptr(), nin, policy, cflags.data_ptr() if cflags is not None else None,
        _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_natt_cksum_batch: %s (%d)" % (driver.last_error(), rc))


ENCSA_DTYPE = L.ENCSA_DTYPE
assert ENCSA_DTYPE.itemsize == 56


def esp_encap(driver, arena, pkt, sa, n, encsa, outsa, headroom, tailroom, id0, desc, frame, opkt, estatus,
              stream=None):
    """Outbound encapsulation, the step before esp_frame
    (espgpu_esp_encap_batch): pkt is a uint8 CUDA tensor of PKT_DTYPE records
    (cleartext IP packets in arena), sa an int16 CUDA tensor with the session
    id the caller's SPD lookup chose for each, encsa a uint8 CUDA tensor of
    ENCSA_DTYPE records and outsa esp_frame's OUTSA_DTYPE tensor, both indexed
    by session id and equally long.  Every packet has headroom writable bytes
    in front and tailroom behind, and the spans of one batch do not overlap.
    Transport or tunnel is decided per packet; the header moves or the outer
    header is built, with ip_id (id0 + i) & 0xffff.  desc, frame and opkt
    receive what esp_frame takes and where the wire packet lies (PKT_DTYPE),
    estatus 0 / EINVAL / ENOTSUP / EAFNOSUPPORT / EMSGSIZE / ENOBUFS for
    replay_merge; a refused packet's descriptor has len 0 and sa 0xffff."""
    for t in (arena, pkt, sa, encsa, outsa, desc, frame, opkt, estatus):
        assert t.is_cuda and t.is_contiguous()
    assert sa.element_size() == 2 and sa.numel() >= n and frame.element_size() == 4 and frame.numel() >= n
    assert pkt.numel() * pkt.element_size() >= n * PKT_DTYPE.itemsize
    assert opkt.numel() * opkt.element_size() >= n * PKT_DTYPE.itemsize
    assert desc.numel() * desc.element_size() >= n * 16 and estatus.numel() >= n
    nenc = encsa.numel() * encsa.element_size() // ENCSA_DTYPE.itemsize
    assert outsa.numel() * outsa.element_size() // OUTSA_DTYPE.itemsize >= nenc
    rc = driver.lib.espgpu_esp_encap_batch(
        driver.ctx, arena.data_ptr(), pkt.data_ptr(), sa.data_ptr(), n, encsa.data_ptr(), outsa.data_ptr(), nenc,
        headroom, tailroom, id0 & 0xffffffff, desc.data_ptr(), frame.data_ptr(), opkt.data_ptr(),
        estatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_encap_batch: %s (%d)" % (driver.last_error(), rc))


def esp_sent(driver, opkt, desc, status, n, encsa, stream=None):
    """The SAs' lifetime counters after the outbound merges
    (espgpu_esp_sent_batch): every record with status 0 books its wire
    packet's length and one packet into encsa[desc.sa]."""
    for t in (opkt, desc, status, encsa):
        assert t.is_cuda and t.is_contiguous()
    assert opkt.numel() * opkt.element_size() >= n * PKT_DTYPE.itemsize
    assert desc.numel() * desc.element_size() >= n * 16 and status.numel() >= n
    nenc = encsa.numel() * encsa.element_size() // ENCSA_DTYPE.itemsize
    rc = driver.lib.espgpu_esp_sent_batch(
        driver.ctx, opkt.data_ptr(), desc.data_ptr(), status.data_ptr(), n, encsa.data_ptr(), nenc,
        _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_esp_sent_batch: %s (%d)" % (driver.last_error(), rc))


def ah_encap(driver, arena, pkt, sa, n, encsa, headroom, id0, hsave, desc, opkt, estatus, stream=None):
    """Outbound AH encapsulation, the step before ah_frame
    (espgpu_ah_encap_batch): pkt, sa and encsa as esp_encap takes them, the AH
    SAs' entries carrying L.ENC_AH; hsave a uint8 CUDA tensor of n *
    L.AH_SAVE_SLOT bytes.  Every packet has headroom writable bytes in front.
    Transport or tunnel is decided per packet; the header moves or the outer
    header is built, the AH header's first dword and padding are written, the
    wire header goes into the packet's slot and its massaged form over the
    packet.  desc receives the DIGEST record (the whole wire packet, salt = the
    ICV field's offset) and opkt where the wire packet lies, estatus 0 / EINVAL
    / ENOTSUP / EAFNOSUPPORT / EMSGSIZE / ENOBUFS for replay_merge; a refused
    packet's descriptor has len 0 and sa 0xffff."""
    for t in (arena, pkt, sa, encsa, hsave, desc, opkt, estatus):
        assert t.is_cuda and t.is_contiguous()
    assert sa.element_size() == 2 and sa.numel() >= n
    assert pkt.numel() * pkt.element_size() >= n * PKT_DTYPE.itemsize
    assert opkt.numel() * opkt.element_size() >= n * PKT_DTYPE.itemsize
    assert desc.numel() * desc.element_size() >= n * 16 and estatus.numel() >= n
    assert hsave.element_size() == 1 and hsave.numel() >= n * L.AH_SAVE_SLOT
    nenc = encsa.numel() * encsa.element_size() // ENCSA_DTYPE.itemsize
    rc = driver.lib.espgpu_ah_encap_batch(
        driver.ctx, arena.data_ptr(), pkt.data_ptr(), sa.data_ptr(), n, encsa.data_ptr(), nenc, headroom,
        id0 & 0xffffffff, hsave.data_ptr(), desc.data_ptr(), opkt.data_ptr(), estatus.data_ptr(),
        _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_ah_encap_batch: %s (%d)" % (driver.last_error(), rc))


def ah_frame(driver, arena, desc, n, outsa, fstatus, stream=None):
    """ah_output's SPI and sequence numbers before encrypt_batch
    (espgpu_ah_frame_batch): outsa as esp_frame's (count, spi and flags are
    read).  Each SA's records get their numbers in index order; desc is
    updated in place (esn_hi; len 0 for refused records) and fstatus receives
    0 / EINVAL / EACCES (the number space ended) per record, for replay_merge
    after the encrypt."""
    for t in (arena, desc, outsa, fstatus):
        assert t.is_cuda and t.is_contiguous()
    assert desc.numel() * desc.element_size() >= n * 16 and fstatus.numel() >= n
    nout = outsa.numel() * outsa.element_size() // OUTSA_DTYPE.itemsize
    rc = driver.lib.espgpu_ah_frame_batch(
        driver.ctx, arena.data_ptr(), desc.data_ptr(), n, outsa.data_ptr(), nout, fstatus.data_ptr(),
        _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_ah_frame_batch: %s (%d)" % (driver.last_error(), rc))


def ah_sent(driver, arena, opkt, desc, status, n, encsa, hsave, sstatus, stream=None):
    """ah_output_cb's restore and the SAs' lifetime counters after the
    outbound merges (espgpu_ah_sent_batch): every record with status 0 of an
    AH SA gets its wire header back from its slot and books its wire packet's
    length and one packet into encsa[desc.sa]; sstatus receives 0 / EINVAL."""
    for t in (arena, opkt, desc, status, encsa, hsave, sstatus):
        assert t.is_cuda and t.is_contiguous()
    assert opkt.numel() * opkt.element_size() >= n * PKT_DTYPE.itemsize
    assert desc.numel() * desc.element_size() >= n * 16 and status.numel() >= n and sstatus.numel() >= n
    assert hsave.element_size() == 1 and hsave.numel() >= n * L.AH_SAVE_SLOT
    nenc = encsa.numel() * encsa.element_size() // ENCSA_DTYPE.itemsize
    rc = driver.lib.espgpu_ah_sent_batch(
        driver.ctx, arena.data_ptr(), opkt.data_ptr(), desc.data_ptr(), status.data_ptr(), n, encsa.data_ptr(), nenc,
        hsave.data_ptr(), sstatus.data_ptr(), _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_ah_sent_batch: %s (%d)" % (driver.last_error(), rc))


def replay_merge(driver, status, rstatus, n, stream=None):
    rc = driver.lib.espgpu_replay_merge(driver.ctx, status.data_ptr(), rstatus.data_ptr(), n,
                                        _stream_ptr(stream))
    if rc:
        raise RuntimeError("espgpu_replay_merge: %s" % driver.last_error())
