"""One pass's results on the host: the compact result blob (include/urhgpu.h "compact result blob") as numpy views, widened to the
reference's shapes and types when somebody looks.  Needs neither torch nor a device: the blob lies in host memory."""
import ctypes as C

import numpy as np

from . import _lib


class LazyDigitized:
    """(ppseq, bits, msg_off, pauses, pos, pos_off) of one digitisation as a sequence whose members are widened to the reference's
    types when somebody looks: what crossed PCIe is the compact blob (a HostBits over pinned memory), and a caller that only wants
    the bits never pays for the int64 pulse table.  materialize() widens everything and lets go of the pinned buffer."""

    def __init__(self, host: "HostBits", want_pos: bool = True):
        self._h = host.check()
        self._want_pos = want_pos
        self._v = [None] * 6

    def _get(self, i):
        if self._v[i] is None:
            h = self._h
            if i == 0:
                self._v[0] = h.ppseq()
            elif i == 1:
                self._v[1] = h.bits()
            elif i == 2:
                self._v[2] = h.msg_off.copy()
            elif i == 3:
                self._v[3] = h.pauses.copy()
            elif i == 4:
                self._v[4] = h.bit_sample_pos() if self._want_pos else np.zeros(0, np.int64)
            else:
                self._v[5] = h.pos_offsets() if self._want_pos else h.pos_off.copy()
        return self._v[i]

    def materialize(self):
        if self._h is not None:
            for i in range(6):
                self._get(i)
            self._h = None
        return self

    def __len__(self):
        return 6

    def __getitem__(self, k):
        if isinstance(k, slice):
            return tuple(self._get(i) for i in range(*k.indices(6)))
        return self._get(range(6)[k])

    def __iter__(self):
        return (self._get(i) for i in range(6))


class HostBits:
    """One pass's results ON THE HOST, from the compact blob (include/urhgpu.h "compact result blob"): numpy views of pinned memory
    owned by the stream -- valid until three pushes later; copy what has to live longer.  The accessors widen to the reference's own
    shapes and types: ppseq() is grab_pulse_lens' int64 (P, 2), bits() one byte per bit, bit_sample_pos() int64."""

    def __init__(self, r: "_lib.HostResult", params):
        self.seq, self.n_samples = int(r.seq), int(r.n_samples)
        self.n_rows, self.n_msg, self.n_bits, self.n_pos = int(r.n_rows), int(r.n_msg), int(r.n_bits), int(r.n_pos)
        self.rows_needed, self.truncated, self.blob_bytes = int(r.rows_needed), int(r.truncated), int(r.blob_bytes)
        self.params = params
        self.d_qad_ptr = r.d_qad
        # the views are made when somebody looks (a push per 0.3 ms must not allocate a dozen objects each)
        self._len16 = (r.row_len16, r.esc, int(r.n_esc)) if r.row_len16 else None      # 16-bit lengths + escape list (URHGPU_BLOB_LEN16)
        self._row16 = (r.row16, r.esc, int(r.n_esc)) if getattr(r, "row16", None) else None      # state | length words + escape list (URHGPU_BLOB_ROW16)
        self._ptr = dict(row_len=(r.row_len, self.n_rows, np.int32), row_state=(r.row_state, self.n_rows, np.int8),
                         bits_packed=(r.bits_packed, (self.n_bits + 7) // 8, np.uint8), msg_off=(r.msg_off, self.n_msg + 1, np.int64),
                         pauses=(r.pauses, self.n_msg, np.int64), pos_off=(r.pos_off, self.n_msg + 1, np.int64),
                         pos32=(r.pos32, self.n_pos, np.uint32) if r.pos32 else None)

    def __getattr__(self, name):
        spec = self.__dict__.get("_ptr", {}).get(name, False)
        if spec is False:
            raise AttributeError(name)
        if name in ("row_len", "row_state") and self.__dict__.get("_row16") is not None:
            # one uint16 per row: (state + 1) << 13 | length; a length field of 0x1FFF = look the row up in the escape list
            w, value = self._escaped(self._row16, 0x1FFF, "packed rows")
            self.__dict__["row_len"], self.__dict__["row_state"] = value, ((w >> 13).astype(np.int16) - 1).astype(np.int8)
            return self.__dict__[name]
        if name == "row_len" and self.__dict__.get("_len16") is not None:
            # widen the shipped uint16 lengths; 0xFFFF = look the row up in the escape list (a true length of 65535 is an entry too)
            value = self.__dict__[name] = self._escaped(self._len16, 0xFFFF, "16-bit row lengths")[1]
            return value
        if spec is None:
            value = None
        else:
            ptr, count, dtype = spec
            if not ptr or count <= 0:
                value = np.zeros(0, dtype)
            else:
                nbytes = count * np.dtype(dtype).itemsize
                value = np.frombuffer((C.c_ubyte * nbytes).from_address(ptr), dtype=dtype, count=count)
        self.__dict__[name] = value
        return value

    def _escaped(self, shipped, mark, what):
        """(the shipped uint16 words, their low bits -- those of `mark` -- as int32 lengths): a length equal to `mark` is looked up in the
        escape list ({uint32 row, int32 length} pairs); every mark has its entry and every entry its mark, or the blob is refused"""
        p16, pesc, n_esc = shipped
        if self.n_rows <= 0:
            return np.zeros(0, np.uint16), np.zeros(0, np.int32)
        w = np.frombuffer((C.c_ubyte * (2 * self.n_rows)).from_address(p16), dtype=np.uint16, count=self.n_rows)
        value = (w & mark).astype(np.int32)
        marked = value == mark
        rows = np.zeros(0, np.int64)
        if n_esc > 0:
            e = np.frombuffer((C.c_ubyte * (8 * n_esc)).from_address(pesc), dtype=np.uint32, count=2 * n_esc).reshape(-1, 2)
            rows = e[:, 0].astype(np.int64)
        if int(marked.sum()) != n_esc or (n_esc and (rows.max() >= self.n_rows or not marked[rows].all() or len(np.unique(rows)) != n_esc)):
            raise _lib.UrhGpuError(_lib.ERR_UNSUPPORTED, f"compact blob: the {what} and their escape list do not match")
        if n_esc > 0:
            value[rows] = e[:, 1].copy().view(np.int32)
        return w, value

    @classmethod
    def from_blob(cls, host_ptr: int, params, seq: int = 0, n_samples: int = 0, d_qad: int = 0):
        """the same object from a compact blob that lies in host memory at host_ptr (header first; include/urhgpu.h): what
        urhgpu_stream_* hands out for a single-GPU stream, made here for blobs copied by other means (sharded passes)"""
        hdr = np.frombuffer((C.c_ubyte * 128).from_address(host_ptr), dtype=np.int64, count=16)
        if int(hdr[0]) != _lib.BLOB_MAGIC:
            raise ValueError("not a result blob")
        r = _lib.HostResult()
        r.seq, r.n_samples = seq, n_samples
        r.n_rows, r.n_msg, r.n_bits, r.n_pos, r.rows_needed = (int(hdr[k]) for k in (1, 2, 3, 4, 5))
        r.blob_bytes = abs(int(hdr[6]))
        r.truncated = int(hdr[15])
        r.pauses, r.msg_off, r.pos_off = host_ptr + int(hdr[8]), host_ptr + int(hdr[9]), host_ptr + int(hdr[10])
        r.row_state, r.bits_packed, r.row_len = host_ptr + int(hdr[11]), host_ptr + int(hdr[12]), host_ptr + int(hdr[13])
        if int(hdr[7]) & _lib.BLOB_ROW16:
            n_esc = int(np.frombuffer((C.c_ubyte * 8).from_address(host_ptr + int(hdr[11])), dtype=np.int64, count=1)[0])
            r.row16, r.row_len, r.row_state, r.esc, r.n_esc = r.row_len, None, None, host_ptr + int(hdr[11]) + 8, abs(n_esc)
        elif int(hdr[7]) & _lib.BLOB_LEN16:
            off_esc = (int(hdr[12]) + (int(hdr[3]) + 7) // 8 + 15) & ~15
            n_esc = int(np.frombuffer((C.c_ubyte * 8).from_address(host_ptr + off_esc), dtype=np.int64, count=1)[0])
            r.row_len16, r.row_len, r.esc, r.n_esc = r.row_len, None, host_ptr + off_esc + 8, abs(n_esc)
        r.pos32 = host_ptr + int(hdr[14]) if int(hdr[7]) & 1 else None
        r.blob = host_ptr
        r.d_qad = d_qad or None
        return cls(r, params)

    def check(self):
        if self.truncated & 4:
            raise _lib.UrhGpuError(_lib.ERR_UNSUPPORTED, "a row length, position or state does not fit the compact blob's narrow types "
                                                         "(take the wide device outputs)")
        if self.truncated:
            raise _lib.UrhGpuError(_lib.ERR_CAPACITY, f"output capacity too small: the pulse table needs {self.rows_needed} rows")
        return self

    def ppseq(self) -> np.ndarray:
        out = np.empty((self.n_rows, 2), np.int64)
        out[:, 0] = self.row_state
        out[:, 1] = self.row_len
        if self.n_rows and self.row_state[0] == -128:        # a sharded ASK piece whose first row was merged into the previous rank's last
            return out[1:]                                   # row (URHGPU_ROW_ABSORBED): not a row of this piece, as ShardResult.piece() has it
        return out

    def bits(self) -> np.ndarray:
        return np.unpackbits(self.bits_packed, count=self.n_bits) if self.n_bits else np.zeros(0, np.uint8)

    def bit_sample_pos(self) -> np.ndarray:
        """All messages' bit_sample_pos back to back (int64; message m: [pos_offsets()[m], pos_offsets()[m + 1])).  With positions shipped
        (want_pos) they are the device's; without, they are derived HERE from the pulse table that was shipped -- they are a function
        of it (ProtocolAnalyzer.py:346-401 computes them from ppseq too), so not shipping them costs no information, only host time
        when somebody asks."""
        if self.pos32 is not None:
            return self.pos32.astype(np.int64)
        return self._derived_positions()[0]

    def pos_offsets(self) -> np.ndarray:
        return self.pos_off.copy() if self.pos32 is not None else self._derived_positions()[1]

    def _derived_positions(self):
        if self.__dict__.get("sharded_piece"):
            raise ValueError("a rank's piece of a sharded capture does not start at sample 0 of the capture: its positions are not derivable "
                             "from its rows alone -- run the pass with write_bit_sample_pos=True to have them shipped")
        if getattr(self, "_derived", None) is None:
            self._derived = positions_from_rows(self.row_state, self.row_len, self.params)
        return self._derived

    def flat(self):
        """(bits u8, msg_off i64, pauses i64, pos i64, pos_off i64): what BitsResult.flat() gives"""
        return self.bits(), self.msg_off.copy(), self.pauses.copy(), self.bit_sample_pos(), self.pos_offsets()

    def message_data(self, sample_rate=1e6, timestamp=0.0):
        """results of a stream with msg_records, or of DevicePipeline.iq_to_bits_batch_records: the list of protocol.MessageData
        ProtocolAnalyzer.get_protocol_from_signal builds its Message objects from -- bits, pause and positions padded where the pass's record says so, RSSI and timestamp from the record.  Without
        shipped positions (want_pos=False) bit_sample_pos is derived here from the pulse table."""
        from .protocol import messages_from_records
        rec = self.__dict__.get("records")
        if rec is None:
            raise ValueError("this result carries no message records (CaptureStream(msg_records=True), or iq_to_bits_batch_records for a batch)")
        self.check()
        if len(rec) != self.n_msg or not (rec["flag"] == 1).all():
            raise _lib.UrhGpuError(_lib.ERR_CAPACITY, "output capacity too small: a message's record is missing")
        return messages_from_records(self.flat(), rec, self.params, sample_rate, timestamp)


def positions_from_rows(row_state, row_len, p):
    """bit_sample_pos of every message from the pulse table, as ProtocolAnalyzer._ppseq_to_bits builds them (:346-411), on whole arrays:
    (positions int64, back to back; offsets int64[n_msg + 1]).  A message's entries: one position per bit (total_samples + k *
    samples_per_bit), then [start, end] of the long pause that closed it -- or the capture's total_samples for the trailing message."""
    st = np.asarray(row_state, dtype=np.int64)
    ln = np.asarray(row_len, dtype=np.int64)
    n = len(st)
    sps, bps, pt = int(p.samples_per_symbol), int(p.bits_per_symbol), int(p.pause_threshold)
    spb = int(sps / bps)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int64)
    ts = np.concatenate([[0], np.cumsum(ln)[:-1]])              # total_samples before each row
    q = ln // sps
    nsym = q + (2 * (ln - q * sps) > sps)                         # int(x) + (fraction > 0.5): exact for these integers
    pause = st == -1
    long_pause = pause & (nsym > pt) & (pt != 0)
    nbits = np.where(long_pause, 0, nsym * bps)
    data = ~pause & (nsym > 0)
    if pause[0]:                                                  # "Starts with Pause": only seeds total_samples
        nbits[0] = 0
        long_pause[0] = False
    grp = np.cumsum(long_pause) - long_pause                      # group of each row (a long pause closes its own group)
    n_grp = int(grp[-1]) + 1
    has_data = np.bincount(grp[data], minlength=n_grp) > 0
    # "elif not there_was_data": a long pause after a group without data drops what was gathered; such a group is no message
    closed = np.zeros(n_grp, dtype=bool)
    closed[grp[long_pause]] = True
    close_row = np.full(n_grp, -1, dtype=np.int64)
    close_row[grp[long_pause]] = np.nonzero(long_pause)[0]
    kept = has_data
    row_kept = kept[grp] & (nbits > 0)
    cnt = nbits[row_kept]
    per_bit_base = np.repeat(ts[row_kept], cnt)
    first = np.cumsum(cnt) - cnt
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt)
    bit_pos = per_bit_base + k * spb
    bits_per_group = np.bincount(grp[row_kept], weights=cnt, minlength=n_grp).astype(np.int64)
    msgs = np.nonzero(kept)[0]
    total_end = int(ts[-1] + ln[-1])
    out, off = [], [0]
    bit_cursor = np.concatenate([[0], np.cumsum(bits_per_group[msgs])])
    for j, g in enumerate(msgs.tolist()):
        out.append(bit_pos[bit_cursor[j]:bit_cursor[j + 1]])
        if closed[g]:
            r = int(close_row[g])
            out.append(np.array([ts[r], ts[r] + ln[r]], dtype=np.int64))
        else:
            out.append(np.array([total_end], dtype=np.int64))
        off.append(off[-1] + int(bits_per_group[g]) + (2 if closed[g] else 1))
    pos = np.concatenate(out) if out else np.zeros(0, np.int64)
    return pos.astype(np.int64), np.asarray(off, dtype=np.int64)
